// Host model of lz4mi_size_kernel (divortio-lz4_amd/csrc/lz4mi_size.hip): the same chunk loop with
// the 64 lanes as arrays, for checking the algorithm against lz4mi_host_decoded_size without a
// device and for counting certification passes per chunk at different warm-up distances
// (DESIGN.md 4.6). Built and driven by tools/size_model.py; not part of the library.
#include <cstdint>
#include <cstring>
#include <algorithm>
constexpr int kWave = 64;
constexpr int kChunk = 1024, kPad = 64, kLim = kChunk + kPad, kStageBytes = kLim, kSeg = 16;
constexpr uint32_t kSpecial = 0xFFF0u, kMalf = 0xFFFCu, kOff0 = 0xFFFDu, kEnd = 0xFFFEu, kStop = 0xFFFFu;
static int g_warm = 512;
struct Seq { uint32_t next, ll, ml; };
template <bool kLens> static Seq parse_seq(const uint8_t* s, uint32_t p, uint32_t rem) {
    Seq r{kStop, 0, 0};
    const uint32_t t = s[p];
    uint32_t q = p + 1, ll = t >> 4;
    if (ll == 15) { uint32_t b; do { if (q >= (uint32_t)kLim) return r; b = s[q++]; ll += b; } while (b == 255); }
    r.ll = ll; q += ll;
    if (q >= rem) { r.next = q > rem ? kMalf : kEnd; return r; }
    if (q + 2 > (uint32_t)kLim) return r;
    if (kLens && (s[q] | s[q + 1]) == 0) { r.next = kOff0; return r; }
    q += 2;
    uint32_t ml = t & 15;
    if (ml == 15) { uint32_t b; do { if (q >= (uint32_t)kLim) return r; b = s[q++]; ml += b; } while (b == 255); }
    r.ml = ml + 4; r.next = q >= rem ? kEnd : q;
    return r;
}
static void load16(const uint8_t* base, uint64_t r0, uint64_t len, uint8_t* dst) {
    for (int j = 0; j < 16; ++j) dst[j] = r0 + j < len ? base[r0 + j] : 0;
}
static uint32_t walk_segment(const uint16_t* nxt, uint32_t p, uint32_t lo, uint32_t& mask) {
    mask = 0;
    while (p < lo + kSeg) { mask |= 1u << (p - lo); p = nxt[p]; }
    return p;
}
static void scan255(const uint8_t* blk, uint64_t in_len, uint64_t& pos, uint64_t& len) {
    for (;;) {
        uint32_t idx[64]; uint8_t v[64][16]; uint64_t hit = 0;
        for (int l = 0; l < 64; ++l) {
            load16(blk, pos + 16u * l, in_len, v[l]);
            idx[l] = 16;
            for (int j = 15; j >= 0; --j) if (v[l][j] != 255) idx[l] = j;
            if (idx[l] < 16) hit |= 1ull << l;
        }
        if (!hit) { len += 255ull * 1024; pos += 1024; continue; }
        uint32_t f = __builtin_ctzll(hit), fi = idx[f], n = 16 * f + fi;
        len += 255ull * n + v[f][fi];
        pos += n + 1;
        return;
    }
}
static uint32_t byte_at(const uint8_t* blk, uint64_t in_len, uint64_t pos) { return pos < in_len ? blk[pos] : 0u; }

extern "C" void emu_set_warm(int w) { g_warm = w; }
extern "C" { uint64_t g_passes = 0, g_chunks = 0; }
extern "C" uint32_t emu_size(const uint8_t* blk, uint32_t in_len_, int32_t* status_out) {
    uint8_t s[kStageBytes]; uint16_t nxt[kChunk];
    const uint64_t in_len = in_len_;
    uint64_t total = 0, ip = 0; int32_t status = 0;
    while (ip < in_len) {
        const uint32_t rem = (uint32_t)(in_len - ip);
        for (int l = 0; l < 64; ++l) load16(blk, ip + 16u * l, in_len, s + 16 * l);
        for (int l = 0; l < (kStageBytes - kChunk) / 16; ++l) load16(blk, ip + kChunk + 16u * l, in_len, s + kChunk + 16 * l);
        for (int p = 0; p < kChunk; ++p) nxt[p] = (uint16_t)parse_seq<false>(s, p, rem).next;
        uint16_t jmp[992];
        for (int p = 0; p < 992; ++p) jmp[p] = nxt[p];
        for (int rnd = 0; rnd < 2; ++rnd) { uint16_t t[992]; for (int p = 0; p < 992; ++p) t[p] = jmp[p] < 992 ? jmp[jmp[p]] : jmp[p]; memcpy(jmp, t, sizeof t); }
        uint32_t e[64], x[64], mask[64];
        for (int l = 0; l < 64; ++l) {
            uint32_t lo = kSeg * l;
            e[l] = lo > (uint32_t)g_warm ? lo - g_warm : 0u;
            for (;;) { uint32_t j = e[l] < 992 ? jmp[e[l]] : kStop; if (j >= lo) break; e[l] = j; }
            while (e[l] < lo) e[l] = nxt[e[l]];
            x[l] = walk_segment(nxt, e[l], lo, mask[l]);
        }
        ++g_chunks;
        for (;;) {
            ++g_passes;
            uint64_t bad = 0, spec = 0; uint32_t xprev[64];
            for (int l = 0; l < 64; ++l) {
                xprev[l] = l ? x[l - 1] : 0;
                if (e[l] != xprev[l]) bad |= 1ull << l;
                if (x[l] >= kSpecial) spec |= 1ull << l;
            }
            uint32_t f = bad ? __builtin_ctzll(bad) : 64u, z = spec ? __builtin_ctzll(spec) : 64u;
            if (z < f) { for (uint32_t l = z + 1; l < 64; ++l) mask[l] = 0; break; }
            if (f == 64u) break;
            e[f] = xprev[f];
            x[f] = walk_segment(nxt, e[f], kSeg * f, mask[f]);
        }
        uint32_t sum[64], key[64], fin[64];
        for (int l = 0; l < 64; ++l) {
            sum[l] = 0; key[l] = fin[l] = 0xFFFFFFFFu;
            uint32_t m = mask[l], lo = kSeg * l;
            while (m) {
                uint32_t j = __builtin_ctz(m); m &= m - 1;
                uint32_t p = lo + j;
                Seq q = parse_seq<true>(s, p, rem);
                if (q.next == kStop) { fin[l] = p << 1 | 1u; break; }
                if (q.next == kMalf) { key[l] = p << 3 | 1u; break; }
                sum[l] += q.ll;
                if (q.next == kOff0) { key[l] = p << 3 | 2u; break; }
                sum[l] += q.ml;
                if (q.next == kEnd) fin[l] = p << 1;
            }
        }
        uint32_t kmin = *std::min_element(key, key + 64);
        uint32_t errlane = kmin == 0xFFFFFFFFu ? 64u : (kmin >> 3) / kSeg;
        for (uint32_t l = 0; l < 64; ++l) if (l <= errlane) total += sum[l];
        if (kmin != 0xFFFFFFFFu) { status = (kmin & 7u) == 1u ? -2 : -3; break; }
        uint32_t fmin = *std::min_element(fin, fin + 64);
        if (fmin == 0xFFFFFFFFu) { ip += x[63]; continue; }
        if (!(fmin & 1u)) break;
        uint64_t pos = ip + (fmin >> 1);
        const uint32_t t = byte_at(blk, in_len, pos++);
        uint64_t ll = t >> 4;
        if (ll == 15) scan255(blk, in_len, pos, ll);
        if (pos + ll > in_len) { status = -2; break; }
        total += ll; pos += ll;
        if (pos >= in_len) break;
        const uint32_t off = byte_at(blk, in_len, pos) | byte_at(blk, in_len, pos + 1);
        pos += 2;
        if (off == 0) { status = -3; break; }
        uint64_t ml = t & 15;
        if (ml == 15) scan255(blk, in_len, pos, ml);
        total += ml + 4;
        ip = pos;
    }
    if (total > 0x7FFFFFFFull) { *status_out = -1; return 0x7FFFFFFFu; }
    *status_out = status;
    return (uint32_t)total;
}
