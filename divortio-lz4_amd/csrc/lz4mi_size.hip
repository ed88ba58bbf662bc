// lz4mi_size.hip — decoded sizes of LZ4 raw blocks for MI355X (gfx950), without decoding.
//
// The sequence walk of decompressBlock (reference src/block/blockDecompress.js:55-139) with
// every copy left out: out_len[b] = the sum of the literal and match lengths along block b's
// token chain (outPos - outputOffset where the reference's loop ends or throws), status[b] =
// the first of the two errors that do not depend on output positions (Malformed Input, :75;
// Invalid Offset 0, :128). Bytes past the block's end read as 0, like the reference's
// `undefined | 0`; nothing outside the block's compressed bytes is read.
//
// One wave64 per block. Per 1 KiB chunk of the compressed stream:
//  1. Stage it (+64 B lookahead) in LDS, zero past the block's end.
//  2. next(p) of every position into an LDS table (exact for any field lengths; a
//     sequence whose fields leave the staged window is marked kStop).
//  3. Speculative walks: lane l walks from 512 bytes before its 16-byte segment (LZ4 token
//     chains resynchronise slowly on tiles216-like data: shorter warm-ups leave many lanes
//     off the chain), four tokens per step on a jump table (the next table squared twice),
//     and records the tokens it visits in the segment. Certification left to right by
//     ballot: lane l's walk is the true chain when its entry into the segment equals its
//     left neighbour's exit and the neighbour is certified; the first lane that fails
//     re-walks from its neighbour's exit. The result is the exact serial parse.
//  4. Every lane parses its certified tokens again for their lengths; the first error
//     is the wave minimum of (position << 3 | check), the lengths before it are summed.
//  5. A sequence that leaves the staged window (long literal runs, length varints longer
//     than the window) is walked by the whole wave over global memory with 255-run scans.
// Every loop is bounded by the block's length: chunk starts and scan positions strictly
// increase, the certification settles one more lane per pass.
#include "../../include/lz4mi.h"
#include "lz4mi_common.h"
#include "lz4mi_launch.h"

namespace lz4mi {
namespace size_pass {

constexpr int kChunk = 1024;                 // compressed bytes parsed per step
constexpr int kPad = 64;                     // lookahead for sequences straddling the chunk end
constexpr int kLim = kChunk + kPad;          // chunk-relative bytes a staged sequence may touch
constexpr int kStageBytes = kLim;            // whole 16-byte pieces
constexpr int kJump = kChunk - 32;           // positions with a jump-table entry (LDS: 5120 bytes in all)
constexpr int kSeg = kChunk / kWave;         // bytes of the chunk per lane
constexpr uint32_t kWarm = 512;              // speculative walks start this far before their segment
constexpr uint32_t kSpecial = 0xFFF0u;       // table values from here on end a walk
constexpr uint32_t kMalf = 0xFFFCu;          // literals run past the block's end (chain ends)
constexpr uint32_t kOff0 = 0xFFFDu;          // offset 0 (parse only; the table keeps the chain)
constexpr uint32_t kEnd = 0xFFFEu;           // last sequence of the block
constexpr uint32_t kStop = 0xFFFFu;          // sequence cannot be parsed inside the window
static_assert(kSeg == 16, "one 16-bit token mask per lane");

struct SizeShared {
    uint32_t stage[kStageBytes / 4];
    uint16_t nxt[kChunk];   // next token
    uint16_t jmp[kJump];    // token 4 steps on (or the walk's end)
};
static_assert(kStageBytes % 16 == 0 && kLim % 16 == 0, "whole 16-byte pieces");
static_assert(offsetof(SizeShared, nxt) % 16 == 0 && offsetof(SizeShared, jmp) % 16 == 0, "16-byte aligned rows");
static_assert(sizeof(SizeShared) * 32 <= 160 * 1024, "8 waves per SIMD");

// 16 bytes of base[0, len) at r0, zero past len.
__device__ __forceinline__ uint4 load16_masked(const uint8_t* base, uint64_t r0, uint64_t len) {
    uint4 v = make_uint4(0, 0, 0, 0);
    if (r0 + 16 <= len) {
        __builtin_memcpy(&v, base + r0, 16);
    } else if (r0 < len) {
        unsigned __int128 x = 0;
        if (len >= 16) {   // the last 16 bytes, shifted down
            __builtin_memcpy(&x, base + len - 16, 16);
            x >>= 8 * (uint32_t)(r0 - (len - 16));
        } else {
#pragma unroll 1
            for (uint32_t j = 0; r0 + j < len; ++j) x |= (unsigned __int128)base[r0 + j] << (8 * j);
        }
        __builtin_memcpy(&v, &x, 16);
    }
    return v;
}

struct Seq {
    uint32_t next;   // chunk-relative position of the next token, or kMalf / kOff0 / kEnd / kStop
    uint32_t ll;     // literal length (valid unless kStop / kMalf)
    uint32_t ml;     // match length incl. MIN_MATCH (0: no match parsed)
};

// The sequence whose token is at s[p] (p < kChunk); rem = bytes of the block from s[0] on.
// kLens: also the lengths and the offset test (the table build needs next only).
template <bool kLens>
__device__ __forceinline__ Seq parse_seq(const uint8_t* s, uint32_t p, uint32_t rem) {
    Seq r{kStop, 0, 0};
    const uint32_t t = s[p];
    uint32_t q = p + 1;
    uint32_t ll = t >> 4;
    if (ll == 15) {
        uint32_t b;
        do {
            if (q >= (uint32_t)kLim) return r;
            b = s[q++];
            ll += b;
        } while (b == 255);
    }
    r.ll = ll;
    q += ll;   // ll < 255 * kLim + 15: no overflow
    if (q >= rem) {   // :75, :123
        r.next = q > rem ? kMalf : kEnd;
        return r;
    }
    if (q + 2 > (uint32_t)kLim) return r;
    if (kLens && (s[q] | s[q + 1]) == 0) {   // :128
        r.next = kOff0;
        return r;
    }
    q += 2;
    uint32_t ml = t & 15;
    if (ml == 15) {
        uint32_t b;
        do {
            if (q >= (uint32_t)kLim) return r;
            b = s[q++];
            ml += b;
        } while (b == 255);
    }
    r.ml = ml + 4;
    r.next = q >= rem ? kEnd : q;
    return r;
}

// jmp[p] = jmp[jmp[p]] for every p (values past the table stay): all of a lane's gathers
// before its stores, the wave's LDS accesses execute in order.
__device__ __forceinline__ void square_jumps(uint16_t* jmp, int lane) {
    uint32_t v[kSeg];
#pragma unroll
    for (int r = 0; r < kSeg; ++r) {
        const uint32_t p = lane + kWave * r;
        v[r] = p < (uint32_t)kJump ? jmp[p] : 0u;
    }
#pragma unroll
    for (int r = 0; r < kSeg; ++r) v[r] = v[r] < (uint32_t)kJump ? jmp[v[r]] : v[r];
    __syncthreads();
#pragma unroll
    for (int r = 0; r < kSeg; ++r) {
        const uint32_t p = lane + kWave * r;
        if (p < (uint32_t)kJump) jmp[p] = (uint16_t)v[r];
    }
    __syncthreads();
}

// Lane l's walk from p: tokens visited in [lo, lo + kSeg) as a bit mask; returns the exit
// (first position at or past the segment's end, or a special value).
__device__ __forceinline__ uint32_t walk_segment(const uint16_t* nxt, uint32_t p, uint32_t lo, uint32_t& mask) {
    mask = 0;
    while (p < lo + kSeg) {   // at most kSeg steps: next(p) > p
        mask |= 1u << (p - lo);
        p = nxt[p];
    }
    return p;
}

// The run of 255s at block position pos and the byte ending it (a length field's tail):
// adds their sum to len, leaves pos after the ending byte. Bytes past the block read 0.
__device__ __forceinline__ void scan255(const uint8_t* blk, uint64_t in_len, uint64_t& pos, uint64_t& len, int lane) {
    for (;;) {   // pos grows by at least 1 per pass; a byte at or past in_len ends the run
        const uint4 v = load16_masked(blk, pos + 16u * lane, in_len);
        const uint32_t w[4] = {~v.x, ~v.y, ~v.z, ~v.w};
        uint32_t idx = 16;   // first byte of the 16 that is not 255
#pragma unroll
        for (int j = 3; j >= 0; --j)
            if (w[j]) idx = 4 * j + ((uint32_t)__builtin_ctz(w[j]) >> 3);
        const uint64_t hit = __ballot(idx < 16);
        if (hit == 0) {
            len += 255ull * (16 * kWave);
            pos += 16 * kWave;
            continue;
        }
        const uint32_t f = (uint32_t)__builtin_ctzll(hit);
        const uint32_t fi = lane_val(idx, f);
        const uint32_t word = fi < 4 ? lane_val(v.x, f) : fi < 8 ? lane_val(v.y, f) : fi < 12 ? lane_val(v.z, f) : lane_val(v.w, f);
        const uint32_t n = 16 * f + fi;
        len += 255ull * n + ((word >> (8 * (fi & 3))) & 255u);
        pos += n + 1;
        return;
    }
}

__device__ __forceinline__ uint32_t byte_at(const uint8_t* blk, uint64_t in_len, uint64_t pos) {
    return pos < in_len ? blk[pos] : 0u;
}

struct SizeArgs {
    const uint8_t* in;
    const uint64_t* in_off;
    const uint32_t* in_len;
    uint32_t* out_len;
    int32_t* status;
    uint32_t nblocks;
    int frame_words;
};

__global__ __launch_bounds__(64, 8) void lz4mi_size_kernel(SizeArgs a) {
    __shared__ SizeShared S;
    const uint32_t b = blockIdx.x;
    const int lane = threadIdx.x;
    if (b >= a.nblocks) return;
    uint32_t word = uniform(a.in_len[b]);
    if (a.frame_words && (word & 0x80000000u)) {   // stored block (bufferDecompress.js:146-148)
        if (lane == 0) {
            a.out_len[b] = word & 0x7FFFFFFFu;
            a.status[b] = LZ4MI_OK;
        }
        return;
    }
    const uint64_t in_len = word;
    const uint8_t* blk = a.in + uniform64(a.in_off[b]);
    const uint8_t* s = (const uint8_t*)S.stage;
    uint64_t total = 0;   // wave-uniform
    int32_t status = LZ4MI_OK;
    uint64_t ip = 0;      // block-relative position of the next token (wave-uniform)

    while (ip < in_len) {
        const uint32_t rem = (uint32_t)(in_len - ip);
        // 1. stage [ip, ip + kStageBytes)
        *(uint4*)(S.stage + 4 * lane) = load16_masked(blk, ip + 16u * lane, in_len);
        if (lane < (kStageBytes - kChunk) / 16)   // the lookahead
            *(uint4*)(S.stage + kChunk / 4 + 4 * lane) = load16_masked(blk, ip + kChunk + 16u * lane, in_len);
        __syncthreads();
        // 2. next-token table, positions lane + 64 r (byte reads of a row share dwords)
#pragma unroll 4
        for (int r = 0; r < kSeg; ++r) {
            const uint32_t p = lane + kWave * r;
            uint32_t n = parse_seq<false>(s, p, rem).next;
            S.nxt[p] = (uint16_t)n;
            if (p < (uint32_t)kJump) S.jmp[p] = (uint16_t)n;
        }
        __syncthreads();
        square_jumps(S.jmp, lane);
        square_jumps(S.jmp, lane);
        // 3. speculative walks, certified left to right
        const uint32_t lo = kSeg * lane;
        uint32_t e = lo > kWarm ? lo - kWarm : 0u;
        for (;;) {   // jumps while they stay before the segment
            const uint32_t j = e < (uint32_t)kJump ? S.jmp[e] : kStop;
            if (j >= lo) break;
            e = j;
        }
        while (e < lo) e = S.nxt[e];
        uint32_t mask;
        uint32_t x = walk_segment(S.nxt, e, lo, mask);
        for (;;) {   // each pass certifies at least one more lane
            uint32_t xprev = dpp<kWaveShr1>(0u, x);
            if (lane == 0) xprev = 0;
            const uint64_t bad = __ballot(e != xprev);
            const uint64_t spec = __ballot(x >= kSpecial);
            const uint32_t f = bad ? (uint32_t)__builtin_ctzll(bad) : 64u;
            const uint32_t z = spec ? (uint32_t)__builtin_ctzll(spec) : 64u;
            if (z < f) {   // the chain ends in a certified lane: nothing after it
                if ((uint32_t)lane > z) mask = 0;
                break;
            }
            if (f == 64u) break;
            if ((uint32_t)lane == f) {
                e = xprev;
                x = walk_segment(S.nxt, e, lo, mask);
            }
        }
        // 4. lengths and errors of the certified tokens
        uint32_t sum = 0, key = 0xFFFFFFFFu, fin = 0xFFFFFFFFu;   // fin: position << 1 | (1: kStop, 0: kEnd / kMalf)
        while (mask) {
            const uint32_t j = (uint32_t)__builtin_ctz(mask);
            mask &= mask - 1;
            const uint32_t p = lo + j;
            const Seq q = parse_seq<true>(s, p, rem);
            if (q.next == kStop) {
                fin = p << 1 | 1u;
                break;
            }
            if (q.next == kMalf) {
                key = p << 3 | 1u;
                break;
            }
            sum += q.ll;
            if (q.next == kOff0) {
                key = p << 3 | 2u;
                break;
            }
            sum += q.ml;
            if (q.next == kEnd) fin = p << 1;
        }
        const uint32_t kmin = wave_min(key);
        const uint32_t errlane = kmin == 0xFFFFFFFFu ? 64u : (kmin >> 3) / kSeg;
        if ((uint32_t)lane > errlane) sum = 0;
        // (sums of one chunk stay below 2^32: kChunk / 3 sequences of < 2^20 bytes)
        total += lane63(wave_incl_scan(sum, lane));
        if (kmin != 0xFFFFFFFFu) {
            status = (kmin & 7u) == 1u ? LZ4MI_ERR_MALFORMED : LZ4MI_ERR_OFFSET0;
            break;
        }
        const uint32_t fmin = wave_min(fin);
        const uint32_t x63 = lane63(x);
        __syncthreads();   // the stage and the table are rewritten next
        if (fmin == 0xFFFFFFFFu) {
            ip += x63;   // >= kChunk
            continue;
        }
        if (!(fmin & 1u)) break;   // the block's last sequence
        // 5. the sequence at ip + (fmin >> 1) leaves the window: the whole wave walks it
        uint64_t pos = ip + (fmin >> 1);
        const uint32_t t = byte_at(blk, in_len, pos++);
        uint64_t ll = t >> 4;
        if (ll == 15) scan255(blk, in_len, pos, ll, lane);
        if (pos + ll > in_len) {   // :75
            status = LZ4MI_ERR_MALFORMED;
            break;
        }
        total += ll;
        pos += ll;
        if (pos >= in_len) break;   // :123
        const uint32_t off = byte_at(blk, in_len, pos) | byte_at(blk, in_len, pos + 1);
        pos += 2;
        if (off == 0) {   // :128
            status = LZ4MI_ERR_OFFSET0;
            break;
        }
        uint64_t ml = t & 15;
        if (ml == 15) scan255(blk, in_len, pos, ml, lane);
        total += ml + 4;
        ip = pos;
    }
    if (lane == 0) {
        if (total > LZ4MI_MAX_BLOCK) {   // no decode call could be given such a capacity
            a.out_len[b] = 0x7FFFFFFFu;
            a.status[b] = LZ4MI_ERR_OUTPUT_TOO_SMALL;
        } else {
            a.out_len[b] = (uint32_t)total;
            a.status[b] = status;
        }
    }
}

}  // namespace size_pass
}  // namespace lz4mi

extern "C" hipError_t lz4mi_launch_sizes(const uint8_t* in, const uint64_t* in_off, const uint32_t* in_len,
                                         uint32_t* out_len, int32_t* status, uint32_t nblocks, int frame_words,
                                         hipStream_t stream) {
    if (nblocks == 0) return hipSuccess;
    lz4mi::size_pass::SizeArgs a{in, in_off, in_len, out_len, status, nblocks, frame_words};
    hipLaunchKernelGGL(lz4mi::size_pass::lz4mi_size_kernel, dim3(nblocks), dim3(lz4mi::kWave), 0, stream, a);
    return hipGetLastError();
}
