// asan_frames_verify.cpp — lz4mi_host_frames_verify_blocks (csrc/lz4mi_host.cpp) run once under AddressSanitizer, in
// a program of its own: no Python, no device, no HIP runtime. The two symbols lz4mi_host.cpp takes from
// lz4mi_capi.cpp are defined here, lz4mi_xxh32 as a second, byte-at-a-time implementation of the specification, so
// the run also checks the twin against a hash that shares no code with the library.
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all \
//       tools/asan_frames_verify.cpp divortio-lz4_amd/csrc/lz4mi_host.cpp -o asan_frames_verify && ./asan_frames_verify
//
// The arena is a heap block that ends exactly with the last frame, and in the last round exactly in front of the
// last record's checksum: a read outside a frame's own range there is a heap-buffer-overflow.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../include/lz4mi.h"

static uint32_t rotl(uint32_t x, int r) { return (x << r) | (x >> (32 - r)); }
static uint32_t rd32(const uint8_t* p) { return p[0] | p[1] << 8 | p[2] << 16 | (uint32_t)p[3] << 24; }

extern "C" uint32_t lz4mi_xxh32(const uint8_t* p, size_t n, uint32_t seed, uint32_t flags) {
    const uint32_t P1 = 2654435761u, P2 = 2246822519u, P3 = 3266489917u, P4 = 668265263u, P5 = 374761393u;
    if (!(flags & LZ4MI_XXH_STANDARD)) abort();   // (the twin asks for the specification's hash only)
    size_t k = 0;
    uint32_t h;
    if (n >= 16) {
        uint32_t v[4] = {seed + P1 + P2, seed + P2, seed, seed - P1};
        for (; k + 16 <= n; k += 16)
            for (int j = 0; j < 4; ++j) v[j] = rotl(v[j] + rd32(p + k + 4 * j) * P2, 13) * P1;
        h = rotl(v[0], 1) + rotl(v[1], 7) + rotl(v[2], 12) + rotl(v[3], 18);
    } else {
        h = seed + P5;
    }
    h += (uint32_t)n;
    for (; k + 4 <= n; k += 4) h = rotl(h + rd32(p + k) * P3, 17) * P4;
    for (; k < n; ++k) h = rotl(h + p[k] * P5, 11) * P1;
    h ^= h >> 15; h *= P2; h ^= h >> 13; h *= P3; h ^= h >> 16;
    return h;
}
extern "C" void lz4mi_advise_output(void*, uint64_t) {}

static void put32(std::vector<uint8_t>& v, uint32_t x) { for (int k = 0; k < 4; ++k) v.push_back((uint8_t)(x >> (8 * k))); }

// A frame with FLG 0x10 (and 0x20, version 1), 64 KiB blocks, no content size: stored blocks of the given lengths.
static std::vector<uint8_t> frame_of(const std::vector<uint32_t>& lens, uint32_t& rng) {
    std::vector<uint8_t> f;
    put32(f, 0x184D2204u);
    f.push_back(0x70);
    f.push_back(0x40);
    f.push_back(0);   // (the header checksum byte is not looked at by the walk)
    for (uint32_t n : lens) {
        put32(f, n | 0x80000000u);
        const size_t at = f.size();
        for (uint32_t k = 0; k < n; ++k) { rng ^= rng << 13; rng ^= rng >> 17; rng ^= rng << 5; f.push_back((uint8_t)rng); }
        put32(f, lz4mi_xxh32(f.data() + at, n, 0, LZ4MI_XXH_STANDARD));
    }
    put32(f, 0);
    return f;
}

#define CHECK(c) do { if (!(c)) { std::fprintf(stderr, "line %d: %s\n", __LINE__, #c); return 1; } } while (0)

int main() {
    const std::vector<std::vector<uint32_t>> shapes = {
        {1}, {3}, {4}, {15}, {16}, {17}, {31}, {32}, {127}, {128}, {129}, {4095}, {4096}, {4097}, {6143}, {6144}, {6145},
        {65536}, {65536, 65536, 100}, {7, 65536, 33, 4097, 65535}, {5000}};
    uint32_t rng = 2463534242u;
    std::vector<std::vector<uint8_t>> frames;
    std::vector<uint64_t> off, len;
    uint64_t at = 0;
    uint32_t nblocks = 0;
    for (size_t k = 0; k < shapes.size(); ++k) {
        frames.push_back(frame_of(shapes[k], rng));
        at += 5 + (k % 4);
        off.push_back(at);
        len.push_back(frames.back().size());
        at += frames.back().size();
        nblocks += (uint32_t)shapes[k].size();
    }
    const uint32_t nf = (uint32_t)frames.size();
    uint8_t* arena = (uint8_t*)std::malloc(at);   // ends with the last frame
    std::memset(arena, 0xA5, at);
    for (uint32_t f = 0; f < nf; ++f) std::memcpy(arena + off[f], frames[f].data(), frames[f].size());

    std::vector<uint64_t> bo(nblocks);
    std::vector<uint32_t> bw(nblocks), bf(nblocks), bs(nblocks);
    std::vector<int64_t> fi(8 * nf), fi0;
    int64_t totals[4];
    std::vector<int32_t> st(nblocks, 77);
    CHECK(lz4mi_host_frames_index(arena, off.data(), len.data(), nf, bo.data(), bw.data(), bf.data(), bs.data(), nblocks,
                                  fi.data(), totals, 0) == LZ4MI_OK);
    CHECK(totals[0] == nblocks && totals[1] == nblocks);
    fi0 = fi;
    auto verify = [&](uint8_t* a) {
        return lz4mi_host_frames_verify_blocks(a, off.data(), len.data(), nf, bo.data(), bw.data(), bf.data(), nblocks,
                                               fi.data(), st.data(), 0);
    };
    // intact: every record 0, finfo untouched
    CHECK(verify(arena) == LZ4MI_OK);
    for (uint32_t b = 0; b < nblocks; ++b) CHECK(st[b] == 0);
    CHECK(fi == fi0);
    // one flipped bit in the last payload byte of the last record: that record, that frame, nothing else
    const uint64_t last_pay = bo[nblocks - 1], last_n = bw[nblocks - 1] & 0x7FFFFFFFu;
    arena[last_pay + last_n - 1] ^= 0x20;
    CHECK(verify(arena) == LZ4MI_OK);
    for (uint32_t b = 0; b < nblocks; ++b) CHECK(st[b] == (b == nblocks - 1 ? LZ4MI_ERR_BLOCK_CHECKSUM : 0));
    for (uint32_t f = 0; f < nf; ++f) CHECK(fi[8 * f] == (f == nf - 1 ? LZ4MI_ERR_BLOCK_CHECKSUM : 0));
    arena[last_pay + last_n - 1] ^= 0x20;
    fi = fi0;
    // the last frame ends in front of its record's checksum, and so does a second arena: the record is cut, fails,
    // and no byte behind the frame is read
    const uint64_t cut = last_pay + last_n;
    uint8_t* small = (uint8_t*)std::malloc(cut);
    std::memcpy(small, arena, cut);
    len[nf - 1] = cut - off[nf - 1];
    CHECK(verify(small) == LZ4MI_OK);
    for (uint32_t b = 0; b < nblocks; ++b) CHECK(st[b] == (b == nblocks - 1 ? LZ4MI_ERR_BLOCK_CHECKSUM : 0));
    CHECK(fi[8 * (nf - 1)] == LZ4MI_ERR_BLOCK_CHECKSUM);
    std::free(small);
    std::free(arena);
    std::printf("asan_frames_verify ok: %u frames, %u records\n", nf, nblocks);
    return 0;
}
