// lz4mi_xxh32.hip — batched XXH32 of independent buffers (gfx950).
//
// Replaces xxHash32 (reference src/xxhash32/xxhash32.js:21-98) for many
// buffers at once (per-block digests, dictionary ids, parity checks). One
// buffer = one quad of lanes: lane j of the quad owns accumulator v(j+1) and
// reads dword j of every 16-byte stripe, so the quad reads each stripe as one
// coalesced 16-byte segment. The four chains are serial by definition, so the
// kernel is latency-bound per buffer and throughput comes from running
// 16 buffers per wave, many waves per CU.
//
// By default the lane convergence follows the reference (xxhash32.js:59-65:
// rotl(rotl(rotl(rotl(v1,1)+v2,7)+v3,12)+v4,18)); `standard` selects the
// XXH32 specification's rotl(v1,1)+rotl(v2,7)+rotl(v3,12)+rotl(v4,18).
#include "lz4mi_common.h"
#include "lz4mi_frames.h"
#include "lz4mi_launch.h"

namespace lz4mi {

constexpr uint32_t P1 = 2654435761u, P2 = 2246822519u, P3 = 3266489917u, P4 = 668265263u, P5 = 374761393u;
constexpr int32_t kErrBlockChecksum = -10;   // LZ4MI_ERR_BLOCK_CHECKSUM (include/lz4mi.h)

__device__ __forceinline__ uint32_t rotl(uint32_t x, int r) { return __builtin_amdgcn_alignbit(x, x, 32 - r); }

__device__ __forceinline__ uint32_t load_le32(const uint8_t* p, bool aligned) {
    if (aligned) return *(const uint32_t*)p;
    return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
}

// The stripe chain of one quad lane, shared by every kernel below so that they cannot drift:
// v folded over this lane's dword (at q + 16 k) of stripes [0, stripes); `load` reads one LE32.
// Software pipeline: the next kDepth stripes' words are in flight while the current kDepth are
// folded into the accumulator (one load round trip per 2 x kDepth stripes would otherwise stall
// the serial chain every kDepth steps). Nothing outside the stripes' own bytes is read.
template <class Load>
__device__ __forceinline__ uint32_t stripe_chain(uint32_t v, const uint8_t* q, uint64_t stripes, Load load) {
    uint64_t k = 0;
    constexpr int kDepth = 128;
    if (stripes >= 2 * kDepth) {
        uint32_t w[kDepth];
#pragma unroll
        for (int u = 0; u < kDepth; ++u) w[u] = load(q + 16 * u);
        for (; k + 2 * kDepth <= stripes; k += kDepth) {
            uint32_t nw[kDepth];
#pragma unroll
            for (int u = 0; u < kDepth; ++u) nw[u] = load(q + 16 * (k + kDepth + u));
#pragma unroll
            for (int u = 0; u < kDepth; ++u) v = rotl(v + w[u] * P2, 13) * P1;
#pragma unroll
            for (int u = 0; u < kDepth; ++u) w[u] = nw[u];
        }
#pragma unroll
        for (int u = 0; u < kDepth; ++u) v = rotl(v + w[u] * P2, 13) * P1;
        k += kDepth;
    }
    for (; k + 8 <= stripes; k += 8) {   // short buffers and the pipeline's remainder
        uint32_t w[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) w[u] = load(q + 16 * (k + u));
#pragma unroll
        for (int u = 0; u < 8; ++u) v = rotl(v + w[u] * P2, 13) * P1;
    }
    for (; k < stripes; ++k) v = rotl(v + load(q + 16 * k) * P2, 13) * P1;
    return v;
}

// What lane 0 of a quad does with the quad's four accumulators: the convergence (`standard`: the
// specification's), the length, the up to 15 bytes behind the last stripe and the avalanche.
__device__ __forceinline__ uint32_t finish(uint32_t v1, uint32_t v2, uint32_t v3, uint32_t v4, const uint8_t* p,
                                           uint64_t L, uint32_t seed, int standard) {
    uint32_t h;
    if (L >= 16) {
        if (standard) {
            h = rotl(v1, 1) + rotl(v2, 7) + rotl(v3, 12) + rotl(v4, 18);
        } else {
            h = rotl(v1, 1);
            h = rotl(h + v2, 7);
            h = rotl(h + v3, 12);
            h = rotl(h + v4, 18);
        }
    } else {
        h = seed + P5;
    }
    h += (uint32_t)L;
    uint64_t pos = L >= 16 ? L / 16 * 16 : 0;
    for (; pos + 4 <= L; pos += 4) h = rotl(h + load_le32(p + pos, false) * P3, 17) * P4;
    for (; pos < L; ++pos) h = rotl(h + p[pos] * P5, 11) * P1;
    h ^= h >> 15; h *= P2; h ^= h >> 13; h *= P3; h ^= h >> 16;
    return h;
}

// hashes[buf] = digest; or (TO_FRAME) the digest stored little-endian at dst + dst_off[buf]
// (frame block checksums written after their payloads; dst_off[buf] == ~0: nothing is stored,
// lz4mi_frames_enc.hip). Two instantiations, so the plain
// batch kernel keeps its register allocation.
template <bool TO_FRAME>
__global__ __launch_bounds__(256) void lz4mi_xxh32_kernel(const uint8_t* in, const uint64_t* off, const uint32_t* len,
                                                          uint32_t seed, uint32_t* hashes, uint32_t n, int standard,
                                                          uint8_t* dst, const uint64_t* dst_off) {
    const uint32_t gid = blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t buf = gid >> 2;
    const int j = threadIdx.x & 3;
    const bool live = buf < n;
    const uint8_t* p = live ? in + off[buf] : in;
    const uint64_t L = live ? len[buf] : 0;
    const bool aligned = (((uintptr_t)p) & 3) == 0;
    const uint64_t stripes = L >= 16 ? L / 16 : 0;

    uint32_t init[4] = { seed + P1 + P2, seed + P2, seed, seed - P1 };
    const uint32_t v = stripe_chain(init[j], p + 4 * j, stripes,
                                    [aligned](const uint8_t* a) { return load_le32(a, aligned); });

    // gather the quad's accumulators into every lane of the quad
    const int lane = threadIdx.x & 63, qb = lane & ~3;
    uint32_t v1 = __shfl(v, qb + 0, 64), v2 = __shfl(v, qb + 1, 64), v3 = __shfl(v, qb + 2, 64),
             v4 = __shfl(v, qb + 3, 64);
    if (!live || j != 0) return;
    if (TO_FRAME && dst_off[buf] == ~0ull) return;   // (no place: a block or frame of a batch that is not written)
    const uint32_t h = finish(v1, v2, v3, v4, p, L, seed, standard);
    if (TO_FRAME) {
        uint8_t* q8 = dst + dst_off[buf];
        for (int k = 0; k < 4; ++k) q8[k] = (uint8_t)(h >> (8 * k));
    } else {
        hashes[buf] = h;
    }
}

// Block checksums of a frame checked in place (lz4mi_verify_blocks): the same machine -- one quad
// per block, 16 blocks per wave, the stripe chain above, spec convergence, seed 0 -- over block b's
// payload in[in_off[b] .. +n), n = in_len[b] (frame_words: in_len[b] & 0x7FFFFFFF, a stored block's
// raw bytes are a payload like any other); lane 0 of the quad compares the digest with the LE32
// stored behind the payload and writes status[b] = 0 or LZ4MI_ERR_BLOCK_CHECKSUM. No digest is
// written. Nothing outside in[0 .. in_total) is read: a record the end cuts (in_off[b] + n + 4 >
// in_total) runs with length 0, reads nothing and gets LZ4MI_ERR_BLOCK_CHECKSUM.
// Frame payloads start at any residue mod 4; a 4-byte memcpy compiles to one global_load_dword at
// any alignment, so the lanes take no aligned / unaligned split.
__global__ __launch_bounds__(256) void lz4mi_verify_kernel(const uint8_t* in, uint64_t in_total, const uint64_t* in_off,
                                                           const uint32_t* in_len, int32_t* status, uint32_t n,
                                                           int frame_words) {
    const uint32_t gid = blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t buf = gid >> 2;
    const int j = threadIdx.x & 3;
    const bool live = buf < n;
    const uint64_t at = live ? in_off[buf] : 0;
    const uint32_t want = live ? (frame_words ? in_len[buf] & 0x7FFFFFFFu : in_len[buf]) : 0;
    const bool whole = live && at <= in_total && (uint64_t)want + 4 <= in_total - at;
    const uint8_t* p = whole ? in + at : nullptr;   // (nullptr: a cut record, or no block; with L = 0 never read)
    const uint64_t L = whole ? want : 0;   // (64 bits as in the kernel above: the chain loop then gets its schedule)
    const uint64_t stripes = L >= 16 ? L / 16 : 0;

    constexpr uint32_t seed = 0;
    uint32_t init[4] = { seed + P1 + P2, seed + P2, seed, seed - P1 };
    const uint32_t v = stripe_chain(init[j], p + 4 * j, stripes, [](const uint8_t* a) {
        uint32_t w;
        __builtin_memcpy(&w, a, 4);
        return w;
    });

    const int lane = threadIdx.x & 63, qb = lane & ~3;
    uint32_t v1 = __shfl(v, qb + 0, 64), v2 = __shfl(v, qb + 1, 64), v3 = __shfl(v, qb + 2, 64),
             v4 = __shfl(v, qb + 3, 64);
    if (!live || j != 0) return;
    int32_t st = kErrBlockChecksum;
    if (p) {
        const uint32_t h = finish(v1, v2, v3, v4, p, L, seed, 1);
        if (h == load_le32(p + L, false)) st = 0;
    }
    status[buf] = st;
}

// Block checksums of a batch of frames checked in place (lz4mi_frames_verify_blocks): lz4mi_verify_kernel's
// machine with per-frame bounds. The quad of block b looks up its frame f = blk_frame[b] and that frame's finfo
// row: the record is checked when f < nframes, the frame is one the call checks (frames::verify_checked) and b lies
// in the frame's own range of the lists -- entries behind totals[1] hold anything -- and it is whole when payload
// and LE32 lie inside in[frame_off[f] .. +frame_len[f]). A cut record runs with length 0, reads nothing and is
// LZ4MI_ERR_BLOCK_CHECKSUM; a record that is not checked runs with length 0 too and gets 0 (before the chain).
// finfo is only read here: which records are checked cannot depend on another quad's verdict. The fold below
// writes it.
__global__ __launch_bounds__(256) void lz4mi_frames_verify_kernel(const uint8_t* in, const uint64_t* frame_off,
                                                                  const uint64_t* frame_len, uint32_t nframes,
                                                                  const uint64_t* blk_in_off, const uint32_t* blk_word,
                                                                  const uint32_t* blk_frame, uint32_t nblocks,
                                                                  const int64_t* finfo, int32_t* blk_status) {
    const uint32_t buf = blockIdx.x * (blockDim.x >> 2) + (threadIdx.x >> 2);   // (no thread index: 4 nblocks may pass 2^32)
    const int j = threadIdx.x & 3;
    const bool live = buf < nblocks;   // (uniform per quad, like everything up to the chain)
    const uint32_t f = live ? blk_frame[buf] : ~0u;
    bool checked = false, whole = false;
    uint64_t at = 0;
    uint32_t want = 0;
    if (live && f < nframes) {
        const int64_t* fi = finfo + 8ull * f;
        checked = frames::verify_checked(fi, nblocks) && buf >= (uint64_t)fi[frames::kFirst] &&
                  buf - (uint64_t)fi[frames::kFirst] < (uint64_t)fi[frames::kCount];
        if (checked) {
            at = blk_in_off[buf];
            want = blk_word[buf] & 0x7FFFFFFFu;
            whole = frames::record_whole(at, want, frame_off[f], frame_len[f]);
        }
    }
    // A record that is not checked gets its 0 here and is no block from now on: `checked` as one more value that
    // lives through the chain would cost the third wave per SIMD (170 VGPRs against lz4mi_verify_kernel's 168).
    if (live && !checked && j == 0) blk_status[buf] = 0;
    const bool rec = live && checked;
    const uint8_t* p = whole ? in + at : nullptr;   // (nullptr: a cut record, or no record; with L = 0 never read)
    const uint64_t L = whole ? want : 0;   // (64 bits: the chain loop's schedule, as in lz4mi_verify_kernel)
    const uint64_t stripes = L >= 16 ? L / 16 : 0;

    constexpr uint32_t seed = 0;
    uint32_t init[4] = { seed + P1 + P2, seed + P2, seed, seed - P1 };
    const uint32_t v = stripe_chain(init[j], p + 4 * j, stripes, [](const uint8_t* a) {
        uint32_t w;
        __builtin_memcpy(&w, a, 4);
        return w;
    });

    const int lane = threadIdx.x & 63, qb = lane & ~3;
    uint32_t v1 = __shfl(v, qb + 0, 64), v2 = __shfl(v, qb + 1, 64), v3 = __shfl(v, qb + 2, 64),
             v4 = __shfl(v, qb + 3, 64);
    if (!rec || j != 0) return;
    int32_t st = kErrBlockChecksum;
    if (p) {
        const uint32_t h = finish(v1, v2, v3, v4, p, L, seed, 1);
        if (h == load_le32(p + L, false)) st = 0;
    }
    blk_status[buf] = st;
}

// The fold of lz4mi_frames_verify_blocks: one wave per frame over the statuses of its blocks, like the finish
// pass of the decode. A checked frame with a failing record gets finfo[f][0] = LZ4MI_ERR_BLOCK_CHECKSUM, by one
// plain store of lane 0; no other word of finfo is written, and a frame that is not checked (its [0] was set
// before the call, for one) is not touched. The result is a function of blk_status alone.
__global__ __launch_bounds__(64) void lz4mi_frames_verify_fold_kernel(int64_t* finfo, uint32_t nframes,
                                                                      uint32_t nblocks, const int32_t* blk_status) {
    const uint32_t f = blockIdx.x;
    const int lane = threadIdx.x;
    if (f >= nframes) return;
    int64_t* fi = finfo + 8ull * f;
    if (!frames::verify_checked(fi, nblocks)) return;
    const uint64_t first = (uint64_t)fi[frames::kFirst], n = (uint64_t)fi[frames::kCount];
    bool bad = false;
    for (uint64_t k = lane; k < n; k += 64) bad |= blk_status[first + k] != 0;
    if (__ballot(bad) && lane == 0) fi[frames::kErr] = kErrBlockChecksum;
}

// ---------------------------------------------------------------------------
// Synthetic block generator (identical to oracle/lz4_oracle.c
// orc_generate for kinds 0..2). One wave per block; the serial xorshift32
// stream runs on lane 0 into LDS, the wave writes it out coalesced.
__device__ __forceinline__ uint32_t xs32(uint32_t& x) {
    x ^= x << 13; x ^= x >> 17; x ^= x << 5;
    return x;
}

__global__ __launch_bounds__(64) void lz4mi_generate_kernel(uint8_t* out, uint32_t kind, uint32_t seed0,
                                                            uint32_t bsize) {
    __shared__ uint32_t tiles[216 * 16];     // 216 tiles x 64 bytes
    __shared__ uint32_t buf[1024];           // 4 KiB staging
    __shared__ uint32_t idx[64];
    const int lane = threadIdx.x;
    const uint32_t b = blockIdx.x;
    uint8_t* dst = out + (uint64_t)b * bsize;
    uint32_t x = seed0 + b;
    if (x == 0) x = 1;
    if (kind == 1) {                          // repetitive: b[i] = i % 251
        for (uint32_t i = lane; i < bsize; i += 64) dst[i] = (uint8_t)(i % 251);
        return;
    }
    if (kind == 0) {                          // random: one word per 4 bytes, little-endian
        for (uint32_t base = 0; base < bsize; base += 4096) {
            if (lane == 0) for (int k = 0; k < 1024; ++k) buf[k] = xs32(x);
            __syncthreads();
            uint32_t lim = bsize - base < 4096 ? bsize - base : 4096;
            for (uint32_t i = lane; i < lim; i += 64) dst[base + i] = ((const uint8_t*)buf)[i];
            __syncthreads();
        }
        return;
    }
    // tiles216: 216 random 64-byte tiles (one xorshift per byte), then tiles by r() % 216
    if (lane == 0) {
        uint8_t* t = (uint8_t*)tiles;
        for (int k = 0; k < 216 * 64; ++k) t[k] = (uint8_t)(xs32(x) & 255);
    }
    __syncthreads();
    for (uint32_t base = 0; base < bsize; base += 64 * 64) {
        if (lane == 0) for (int k = 0; k < 64; ++k) idx[k] = xs32(x) % 216;
        __syncthreads();
        // 64 tiles x 64 bytes: lane writes dword `lane % 16` of 4 tiles per step
        for (int s = 0; s < 64; s += 4) {
            int t = s + lane / 16, w = lane & 15;
            uint32_t pos = base + 64 * t + 4 * w;
            uint32_t v = tiles[idx[t] * 16 + w];
            if (pos + 4 <= bsize) {
                *(uint32_t*)(dst + pos) = v;            // bsize is a multiple of 4 in every config
            } else {
                for (uint32_t j = 0; j < 4 && pos + j < bsize; ++j) dst[pos + j] = (uint8_t)(v >> (8 * j));
            }
        }
        __syncthreads();
    }
}

}  // namespace lz4mi

extern "C" hipError_t lz4mi_launch_xxh32(const uint8_t* in, const uint64_t* off, const uint32_t* len, uint32_t seed,
                                         uint32_t* hashes, uint32_t n, int standard, uint8_t* dst,
                                         const uint64_t* dst_off, hipStream_t stream) {
    if (n == 0) return hipSuccess;
    // one wave (16 buffers) per workgroup: the waves spread over every CU's load path
    uint32_t threads = n * 4;
    if (dst)
        hipLaunchKernelGGL(lz4mi::lz4mi_xxh32_kernel<true>, dim3((threads + 63) / 64), dim3(64), 0, stream, in, off,
                           len, seed, hashes, n, standard, dst, dst_off);
    else
        hipLaunchKernelGGL(lz4mi::lz4mi_xxh32_kernel<false>, dim3((threads + 63) / 64), dim3(64), 0, stream, in, off,
                           len, seed, hashes, n, standard, dst, dst_off);
    return hipGetLastError();
}

extern "C" hipError_t lz4mi_launch_verify(const uint8_t* in, uint64_t in_total, const uint64_t* in_off,
                                          const uint32_t* in_len, int32_t* status, uint32_t n, int frame_words,
                                          hipStream_t stream) {
    if (n == 0) return hipSuccess;
    // as lz4mi_launch_xxh32: one wave (16 blocks) per workgroup
    hipLaunchKernelGGL(lz4mi::lz4mi_verify_kernel, dim3((n * 4 + 63) / 64), dim3(64), 0, stream, in, in_total, in_off,
                       in_len, status, n, frame_words);
    return hipGetLastError();
}

extern "C" hipError_t lz4mi_launch_frames_verify(const uint8_t* in, const uint64_t* frame_off,
                                                 const uint64_t* frame_len, uint32_t nframes,
                                                 const uint64_t* blk_in_off, const uint32_t* blk_word,
                                                 const uint32_t* blk_frame, uint32_t nblocks, int64_t* finfo,
                                                 int32_t* blk_status, hipStream_t stream) {
    if (nblocks == 0 || nframes == 0) return hipSuccess;
    // as lz4mi_launch_verify: one wave (16 blocks) per workgroup; 64-bit: nblocks * 4 may pass 2^32
    const uint32_t groups = (uint32_t)(((uint64_t)nblocks * 4 + 63) / 64);
    hipLaunchKernelGGL(lz4mi::lz4mi_frames_verify_kernel, dim3(groups), dim3(64), 0, stream, in, frame_off, frame_len,
                       nframes, blk_in_off, blk_word, blk_frame, nblocks, finfo, blk_status);
    hipLaunchKernelGGL(lz4mi::lz4mi_frames_verify_fold_kernel, dim3(nframes), dim3(64), 0, stream, finfo, nframes,
                       nblocks, blk_status);
    return hipGetLastError();
}

extern "C" hipError_t lz4mi_launch_generate(uint8_t* out, uint32_t kind, uint32_t seed0, uint32_t bsize,
                                            uint32_t nblocks, hipStream_t stream) {
    if (nblocks == 0) return hipSuccess;
    hipLaunchKernelGGL(lz4mi::lz4mi_generate_kernel, dim3(nblocks), dim3(64), 0, stream, out, kind, seed0, bsize);
    return hipGetLastError();
}
