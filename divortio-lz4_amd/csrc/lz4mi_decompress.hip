// lz4mi_decompress.hip — LZ4 raw-block decoder for MI355X (gfx950).
//
// Replaces decompressBlock (reference src/block/blockDecompress.js:30-275) for
// batches of independent blocks. Semantics follow the reference exactly for
// spec-valid input (positions absolute in `out`, dictionary below out[0],
// clipped match writes, the four error strings). The reference's double-copy-
// tail rewrite is reproduced in reference mode, LZ4MI_JS_EXACT, by
// this kernel (the in-chunk replay, step 7; the batch kernel has one instantiation
// per mode, lz4mi_decompress_kernel / lz4mi_decompress_ref_kernel) -- batches here,
// small batches through the export path (lz4mi_expand.hip), whose blocks with a
// rewrite come back here (DecArgs::redo). Only LZ4MI_JS_COMPAT still decodes the
// blocks in order on one lane (lz4mi_decompress_serial.hip).
//
// One wave64 per block, all 4096 blocks of a batch resident at once
// (< 10 KiB LDS, <= 128 VGPRs -> 16 waves per CU). decompress_block calls the
// steps below in this order, per 1 KiB chunk of the compressed stream:
//  1. Stage it (+64 B lookahead) in LDS.
//  2. next(p) of every position, branch-free (length fields of one extension
//     byte; longer ones through a ballot-gated exact loop) into an LDS table.
//  3. Speculative walks: lane l walks next() from kWarm = 512 bytes before its 16-byte
//     segment and records the tokens it visits in the segment; LZ4 token
//     chains resynchronise within a few steps, so walks are almost always on
//     the true chain. Certification left to right by ballot: the first lane
//     whose left neighbour's exit is not on its walk re-walks from it (its
//     neighbour is settled). The result is the exact serial parse. Walks
//     start that far back: inside long literal runs a walk can take a while
//     to fall onto the true chain, and every unsettled lane costs a pass.
//  4. Sequence table in LDS, built sequence-major: the lanes list their tokens'
//     positions compactly (lane l's at base(l) + j), then lane l of row i takes
//     sequence 64i+l, reads its fields (literal source, lengths, offset), gets
//     its output start from a row prefix sum plus the carry of the rows before
//     and writes its entry once. Errors in the reference's order: a 32-bit test
//     per row pair, the exact checks only from the first flagged pair on.
//     A true token whose match length field runs past one extension byte sends
//     the chunk back to step 2 for the exact table (once).
//  5. A sequence whose parse leaves the staged window (long literal runs or
//     length varints: incompressible or highly repetitive data) is parsed from
//     global memory with wave-wide 255-run scans. It is written after step 6 by
//     the whole wave, literal run first, then (after it is stored, and after
//     step 7) the match run. In the batch kernel a chunk's last sequence that
//     overruns the window but would fit one it starts is not cut: the chunk ends
//     at its token and the next chunk begins there (parse_chunk, `defer`).
//     (Export, XP: the sequences of steps 4 and 5 go to the segment's list
//     instead, and the chunk ends here.)
//  6. Output, sequence-parallel (lane l takes sequence 64i+l), every run
//     written with exact-width unaligned 16/8/4/2/1-byte pieces (the last
//     16-byte piece of a run overlaps its predecessor instead of spilling),
//     so lanes never touch each other's bytes:
//       round 1: all literal runs (from LDS, in a pass of their own before the
//                row loop; those of >= 16 bytes, of any length, cut into
//                16-byte pieces that are dealt to the lanes, 64 per store:
//                LitDeal) and every match whose source lies entirely in
//                output finished by earlier chunks;
//       round r: after the previous round's stores are complete, every
//                pending match whose source range meets no pending match.
//     The earliest pending match is always ready, so the rounds terminate;
//     on typical data two or three suffice. Matches are read straight from
//     the output (L2, bypassing L1); an overlapping match (offset < length)
//     is read through its period: a 16-byte window that wraps is merged from
//     two loads, periods under 16 bytes are expanded in registers. Matches
//     (and matches remapped into literal runs) longer than kLaneBytes = 256
//     bytes are written by the whole wave.
//  7. Reference mode: the chunk's matches replayed with the reference's tail
//     rewrite where it would change a byte (f1_table, f1_fixup).
#include "../../include/lz4mi.h"
#include "lz4mi_common.h"
#include "lz4mi_decompress.h"
#include "lz4mi_launch.h"

#ifndef LZ4MI_LL_ADAPT
#define LZ4MI_LL_ADAPT 127   // long literal runs: s_sleep argument after every 4 KiB step while blocks with a
                             // compression ratio above 2 run on the same XCD (0: no pacing; A/B switch)
#endif
#ifndef LZ4MI_ORDER
#define LZ4MI_ORDER 1   // batches dispatched latency-bound blocks first, most compressed bytes first; 2: the
                        // latency-bound blocks first in index order; 0: index order (A/B switch)
#endif
#ifndef LZ4MI_ABLATE
#define LZ4MI_ABLATE 0   // timing-only variants (tools/): 1 = no output, 2 = parse only, 3 = next table only,
                         // 4 = output loads without stores, 5 = output stores without loads, 6 = round 1 only
#endif

#ifndef LZ4MI_TIMELINE
#define LZ4MI_TIMELINE 0   // diagnostic build (tools/timeline.py): every block's start / end time, CU, XCD
#endif

#ifndef LZ4MI_PROFILE
#define LZ4MI_PROFILE 0  // timing-only variant (tools/): per-phase wall-clock accumulation
#endif

namespace lz4mi {

// One 16-byte output piece (any alignment: gfx950 runs in unaligned mode), default cache
// policy: the written lines stay in L2 for the history reads that follow (nontemporal
// stores, which skip L2, made tiles216 2x slower: 40.6 vs 20.5 ms).
__device__ __forceinline__ void out16(uint8_t* p, const uint4& v) { __builtin_memcpy(p, &v, 16); }
// 16 bytes read / written once (streamed: nontemporal, so they do not evict the history lines
// the matches read back from L2)
typedef uint32_t u32x4_nt __attribute__((ext_vector_type(4), aligned(1)));
__device__ __forceinline__ uint4 ld16_nt(const uint8_t* p) {
    const u32x4_nt t = __builtin_nontemporal_load((const u32x4_nt*)p);
    return make_uint4(t.x, t.y, t.z, t.w);
}
__device__ __forceinline__ void st16_nt(uint8_t* p, const uint4& v) {
    const u32x4_nt t = {v.x, v.y, v.z, v.w};
    __builtin_nontemporal_store(t, (u32x4_nt*)p);
}

#if LZ4MI_LL_ADAPT
__device__ unsigned int g_lat_active[8 * 32];   // per XCD (one 128-byte line each): latency-bound blocks running
__device__ __forceinline__ uint32_t xcc_id() {
    uint32_t x;
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(x));
    return x & 7u;
}
#endif

#if LZ4MI_TIMELINE
constexpr uint32_t kTlMax = 16384;
__device__ unsigned long long g_tl[2 * kTlMax];   // per block: start, end (s_memrealtime, 100 MHz)
__device__ unsigned int g_tl_id[2 * kTlMax];      // per block: HW_ID (wave, SIMD, CU, SH, SE), XCC_ID
#endif

#if LZ4MI_PROFILE
__device__ unsigned long long g_prof[24];
// A wave's accumulator: decompress_block owns it and hands it to the phases (`prof`).
struct Prof {
    uint64_t acc[24];
    uint64_t t;
};
#define PROF(i)                              \
    do {                                     \
        const uint64_t t_ = wall_clock64();  \
        prof.acc[i] += t_ - prof.t;          \
        prof.t = t_;                         \
    } while (0)
#define PROF_COUNT(i, n) (prof.acc[i] += (n))
#else
struct Prof {};
#define PROF(i) ((void)0)
#define PROF_COUNT(i, n) ((void)0)
#endif

constexpr int kChunk = 1024;                  // compressed bytes parsed per step
constexpr int kPad = 64;                      // lookahead for sequences straddling the chunk end
constexpr int kLim = kChunk + kPad;           // chunk-relative bytes a regular sequence may touch
constexpr int kStageWords = (kLim + 28) / 4;  // + slack for 16-byte literal loads at the window end
constexpr int kMaxSeq = kChunk / 3 + 3;       // tokens starting in the chunk: every non-final sequence is >= 3 bytes
constexpr uint32_t kWarm = 512;               // speculative walks start this far before their segment
constexpr int kMaxVarint = 250;               // longer length varints go to the cut path (ml < 65536)
constexpr int32_t LZ4MI_ERR_RANGE_STATUS = LZ4MI_ERR_RANGE;   // (include/lz4mi.h)
constexpr uint32_t kEnd = 0x40000000u;        // chain ends (last sequence of the block)
constexpr uint32_t kStop = 0x40000001u;       // sequence cannot be parsed inside the window
constexpr int kWaveB = 2;                     // ... (whole-wave runs: streaming copies)
constexpr int kWaveB2 = 1;                    // ... (whole-wave periodic runs: two windows per piece)
constexpr int kLaneBytes = 256;               // longer match runs are written by the whole wave (128: tiles216 +1.8 %)
constexpr int kPeriodBulk = 1024;             // longer periodic runs are generated from an LDS copy of the pattern
constexpr int32_t kLongLit = 4096;            // literal runs at least this long: long_literals()
constexpr uint64_t kXRatioMax = 32;           // XP: blocks of higher ratio are decoded by one wave
constexpr int kSegRestarts = 16;              // XP: a guess's walk starts over at most this often
constexpr uint32_t kSegWarm = 3072;           // XP: a segment's warm-up parse (tiles216: 99 % of wrong
                                              // starts join the token chain within 860 bytes)

struct DecShared {
    union {
        uint4 t_seq[kMaxSeq];     // per sequence: {output start (block-relative), literal source (chunk-
                                  //  relative) | literal length << 16, match offset | match length << 16
                                  //  (0: final literal-only sequence), source remapped by remap_src}
        struct {
            uint16_t nxt2[kChunk];   // parse: token 2 steps after p
            uint16_t nxt4[kChunk];   // parse: token 4 steps after p (warm-up walks)
        };
    };
    union {
        uint16_t nxt[kLim];       // parse: next-token table
        uint32_t pme[kLim / 2];   // output: ends of the pending matches
    };
    uint32_t pms[kMaxSeq];        // output: starts of the pending matches
    uint32_t stage[kStageWords];
};
static_assert(kLim / 2 >= kMaxSeq, "pending list must fit in the next-token table");
static_assert(kStageWords * 4 > kLim, "the table build reads s[q + 2] for offsets ending at kLim");
static_assert(offsetof(DecShared, stage) % 16 == 0 && offsetof(DecShared, pme) % 16 == 0, "16-byte aligned rows");

// LDS a whole-wave periodic run may copy its pattern into, by phase of the
// chunk: round 1 (the pending list is not built yet), rounds 2+ (the staged
// literals are all written), the cut sequence (all of it; with the F1 check on,
// all but the sequence tables the check reads afterwards).
struct PatBuf {
    uint32_t* w;
    int32_t bytes;
};
__device__ __forceinline__ PatBuf no_pat() { return PatBuf{nullptr, 0}; }   // literal runs
__device__ __forceinline__ PatBuf pat_round1(DecShared& S) { return PatBuf{S.pms, (int32_t)sizeof(S.pms)}; }
__device__ __forceinline__ PatBuf pat_rounds(DecShared& S) { return PatBuf{S.stage, (int32_t)sizeof(S.stage)}; }
__device__ __forceinline__ PatBuf pat_all(DecShared& S) { return PatBuf{(uint32_t*)&S, (int32_t)sizeof(DecShared)}; }
__device__ __forceinline__ PatBuf pat_cut(DecShared& S) {
    return PatBuf{S.pme, (int32_t)(sizeof(DecShared) - offsetof(DecShared, pme))};
}
static_assert(offsetof(DecShared, pms) == offsetof(DecShared, pme) + sizeof(uint32_t) * (kLim / 2) &&
              offsetof(DecShared, stage) == offsetof(DecShared, pms) + sizeof(uint32_t) * kMaxSeq,
              "the cut pattern buffer spans pme, pms and the stage");

struct Ctx {
    const uint8_t* blk;   // compressed block
    uint8_t* dst;         // output start of the block (out + out_off)
    int64_t out_off;      // absolute position of dst in `out`
    int32_t in_len;
    int32_t cap;          // writable bytes from dst
    const uint8_t* dict;
    int32_t dict_len;
    int isolate;
    int32_t ip;           // chunk start (block-relative compressed position)
    int64_t O;            // output start of the current table (block-relative)
};

// 16 bytes of base[0, len) at r0, zero past len (r0 < len).
__device__ __forceinline__ uint4 load16_tail(const uint8_t* base, int64_t r0, int64_t len) {
    uint4 v = make_uint4(0, 0, 0, 0);
    unsigned __int128 x = 0;
    if (len >= 16) {   // the last 16 bytes, shifted down
        __builtin_memcpy(&x, base + len - 16, 16);
        x >>= 8 * (uint32_t)(r0 - (len - 16));
    } else {
#pragma unroll 1
        for (int j = 0; r0 + j < len; ++j) x |= (unsigned __int128)base[r0 + j] << (8 * j);
    }
    __builtin_memcpy(&v, &x, 16);
    return v;
}

// Bytes [idx, idx + 16) of the staged chunk from five naturally aligned dword
// reads: a misaligned b64/b128 LDS access replays at ~64 LDS cycles, CU-wide
// (tools/probe/lds_unaligned.hip), aligned dwords do not.
__device__ __forceinline__ uint4 stage16(const uint32_t* stage, int32_t idx) {
    const uint32_t* w = stage + (idx >> 2);
    const uint32_t sh = (uint32_t)idx & 3u;
    const uint32_t d0 = w[0], d1 = w[1], d2 = w[2], d3 = w[3], d4 = w[4];
    return make_uint4(funnel(d0, d1, sh), funnel(d1, d2, sh), funnel(d2, d3, sh), funnel(d3, d4, sh));
}

// 16 compressed bytes at block-relative r0 (zero past the block end).
__device__ __forceinline__ uint4 stage_piece(const Ctx& c, int64_t r0) {
    uint4 v = make_uint4(0, 0, 0, 0);
    if (r0 + 16 <= c.in_len) __builtin_memcpy(&v, c.blk + r0, 16);
    else if (r0 < c.in_len) v = load16_tail(c.blk, r0, c.in_len);
    return v;
}

// ---------------------------------------------------------------- parsing
// Position of the token after the one at p (chunk-relative), or kEnd / kStop.
// Exact for any field lengths.
__device__ __forceinline__ uint32_t next_token(const uint8_t* s, uint32_t p, uint32_t rem) {
    if (p >= (uint32_t)kLim) return kStop;
    uint32_t tok = s[p];
    uint32_t q = p + 1;
    uint32_t ll = tok >> 4;
    if (ll == 15) {
        uint32_t b;
        do {
            if (q >= (uint32_t)kLim) return kStop;
            b = s[q++];
            ll += b;
        } while (b == 255);
    }
    q += ll;
    if (q >= rem) return q <= (uint32_t)kLim ? kEnd : kStop;   // literal-only final sequence
    if (q + 2 > (uint32_t)kLim) return kStop;
    q += 2;
    if ((tok & 15) == 15) {
        uint32_t b, n = 0;
        do {
            if (q >= (uint32_t)kLim || ++n > (uint32_t)kMaxVarint) return kStop;
            b = s[q++];
        } while (b == 255);
    }
    return q >= rem ? kEnd : q;
}

// Same, branch-free, for length fields of at most one extension byte each;
// `slow` is set when a field is longer (the caller then uses next_token).
__device__ __forceinline__ uint32_t next_fast(const uint8_t* s, uint32_t p, uint32_t rem, bool& slow) {
    const uint32_t t = s[p], b1 = s[p + 1];
    const uint32_t x1 = (t >> 4) == 15 ? 1u : 0u;
    const uint32_t ll = x1 ? 15u + b1 : t >> 4;
    const uint32_t q = p + 1 + x1 + ll;                        // offset position
    const uint32_t mb = s[q + 2 < (uint32_t)kLim ? q + 2 : 0u];
    const uint32_t x2 = (t & 15) == 15 ? 1u : 0u;
    const uint32_t n = q + 2 + x2;
    uint32_t v = n > (uint32_t)kLim ? kStop : (n >= rem ? kEnd : n);
    if (q >= rem) v = q <= (uint32_t)kLim ? kEnd : kStop;       // literal-only final sequence
    if (x1 && p + 1 >= (uint32_t)kLim) v = kStop;
    slow = (x1 && b1 == 255) || (x2 && mb == 255 && q < rem);
    return v;
}

// The fast next-token table: positions 4w .. 4w+3 (w = lane + 64 r) from the stage
// dwords w and w+1, next = p + 1 + [literal ext] + literals + 2 + [match ext], i.e. every
// length field taken to be at most one extension byte. Valid while no field or next()
// can reach the block's end (rem > kFastRem). A literal field of 2+ bytes (ext byte 255)
// stops the chain there (0xFFFF); a match field of 2+ bytes is caught on the true tokens
// (table build) and the chunk re-parsed with the exact table. Values past the window stay
// raw (<= 1297): every walk ends at them, and a tail past kLim is a cut.
constexpr uint32_t kFastRem = kLim + 300;
__device__ __forceinline__ uint32_t next4_half(uint32_t t, uint32_t b1, uint32_t p) {
    const uint32_t hi = t >> 4;
    const uint32_t x1 = hi == 15 ? 1u : 0u;
    const uint32_t ll = x1 ? 15u + b1 : hi;
    const uint32_t x2 = (t & 15) == 15 ? 1u : 0u;
    const uint32_t n = p + 3 + x1 + x2 + ll;
    return (x1 && b1 == 255) ? 0xFFFFu : n;
}
// The lane index as a value the compiler cannot hoist out of the chunk loop: per-lane
// constants derived from it (p + 1, p + 2, ... of every row) would otherwise be computed
// once and kept in (spilled) registers, their reloads scratch loads that wait, in order,
// for every store still in flight.
__device__ __forceinline__ int opaque(int v) {
    asm volatile("" : "+v"(v));
    return v;
}

__device__ __forceinline__ void next_table_fast(const uint32_t* stage, uint16_t* nxt, int lane) {
    static_assert(kChunk % (4 * kWave) == 0, "whole dword rows per lane");
    lane = opaque(lane);
    uint32_t d0[kChunk / (4 * kWave)], d1[kChunk / (4 * kWave)];
#pragma unroll
    for (int r = 0; r < kChunk / (4 * kWave); ++r) {
        const uint32_t w = lane + kWave * r;
        d0[r] = stage[w];
        d1[r] = stage[w + 1];
    }
#pragma unroll
    for (int r = 0; r < kChunk / (4 * kWave); ++r) {
        const uint32_t w = lane + kWave * r, p = 4 * w;
        const uint32_t a = d0[r], b = d1[r];
        const uint32_t n0 = next4_half(a & 255, (a >> 8) & 255, p);
        const uint32_t n1 = next4_half((a >> 8) & 255, (a >> 16) & 255, p + 1);
        const uint32_t n2 = next4_half((a >> 16) & 255, a >> 24, p + 2);
        const uint32_t n3 = next4_half(a >> 24, b & 255, p + 3);
        *(uint2*)(nxt + p) = make_uint2(n0 | (n1 << 16), n2 | (n3 << 16));
    }
}

// out[p] = in[in[p]] (or in[p] when that is past the chunk): 4 positions per lane, the
// 16 gathers of a lane issued together.
__device__ __forceinline__ void jump_table(const uint16_t* in, uint16_t* out, int lane) {
    constexpr int R = kChunk / (4 * kWave);
    lane = opaque(lane);
    uint2 v[R];
#pragma unroll
    for (int r = 0; r < R; ++r) v[r] = *(const uint2*)(in + 4 * (lane + kWave * r));
    uint32_t y[R][4];
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const uint32_t a[4] = {v[r].x & 0xFFFFu, v[r].x >> 16, v[r].y & 0xFFFFu, v[r].y >> 16};
#pragma unroll
        for (int j = 0; j < 4; ++j) y[r][j] = a[j] < (uint32_t)kChunk ? in[a[j]] : a[j];
    }
#pragma unroll
    for (int r = 0; r < R; ++r)
        *(uint2*)(out + 4 * (lane + kWave * r)) = make_uint2(y[r][0] | (y[r][1] << 16), y[r][2] | (y[r][3] << 16));
}

// Registers loaded by global loads that an explicit wait_vmem() has already
// covered: redefine them opaquely so the compiler's wait insertion no longer
// tracks them (it would otherwise wait for every later store before their use).
__device__ __forceinline__ void settle(uint4& v) {
    asm volatile("" : "+v"(v.x), "+v"(v.y), "+v"(v.z), "+v"(v.w));
}

__device__ __forceinline__ uint16_t enc_next(uint32_t v) {
    return (uint16_t)(v == kEnd ? 0xFFFEu : v == kStop ? 0xFFFFu : v);
}

__device__ __forceinline__ uint32_t next_of(const uint16_t* nxt, uint32_t p) {
    uint32_t v = nxt[p];
    return v >= 0xFFFEu ? (v == 0xFFFEu ? kEnd : kStop) : v;
}

struct SeqInfo {
    int32_t out, lit, ll, off, ml, rsrc;
};
__device__ __forceinline__ SeqInfo seq_of(uint4 v) {
    return SeqInfo{(int32_t)v.x, (int32_t)(v.y & 0xFFFF), (int32_t)(v.y >> 16), (int32_t)(v.z & 0xFFFF),
                   (int32_t)(v.z >> 16), (int32_t)v.w};
}
// one ds_read_b128: everything of sequence k
__device__ __forceinline__ SeqInfo seq_info(const DecShared& S, uint32_t k) { return seq_of(S.t_seq[k]); }

// History (earlier output of this wave) is read with plain loads: the CU's L1 sees
// the wave's own completed stores (every read of output follows an s_waitcnt on
// the stores that wrote it), and L2 keeps the lines. Nontemporal loads (used
// until round 2) cost tiles216 17 % (19.15 vs 15.87 ms, one process, same box).
__device__ __forceinline__ uint32_t hist_u8(const uint8_t* p) { return *p; }

// Byte of earlier output at block-relative position pos (dictionary below out[0]).
__device__ __forceinline__ uint32_t hist_byte(const Ctx& c, int64_t pos) {
    int64_t abs = c.out_off + pos;
    if (abs >= 0) return hist_u8(c.dst + pos);
    return c.dict ? c.dict[c.dict_len + abs] : 0u;
}

// ------------------------------------------------------------------ runs
// A run: n output bytes at y and where they come from.
enum : uint32_t {
    R_NONE = 0,
    R_LDS = 1,    // literal bytes in the staged chunk (src = stage byte index)
    R_COMP = 2,   // literal bytes in the compressed block in global memory (src = block position)
    R_HIST = 3,   // match: earlier output (src = its block-relative position), read through `period`
    R_BYTES = 4,  // match read byte by byte (dictionary, or within 16 bytes of a buffer edge)
};

struct Run {
    int32_t y, n, src, period;   // period = match offset when the match overlaps itself, else 0
    uint32_t kind;
};

__device__ __forceinline__ Run no_run() { return Run{0, 0, 0, 0, R_NONE}; }

// lane l's value (l wave-uniform): v_readlane, not an LDS permute
__device__ __forceinline__ int32_t lane_of(int32_t v, int l) { return (int32_t)__builtin_amdgcn_readlane(v, l); }
__device__ __forceinline__ uint32_t lane_of(uint32_t v, int l) { return (uint32_t)__builtin_amdgcn_readlane((int32_t)v, l); }

__device__ __forceinline__ Run shfl_run(const Run& R, int l) {
    return Run{lane_of(R.y, l), lane_of(R.n, l), lane_of(R.src, l), lane_of(R.period, l), lane_of(R.kind, l)};
}

// The match run of a sequence whose match starts at ms; n = 0 when nothing is
// written (no match, or entirely past the capacity: the reference clips).
__device__ __forceinline__ Run match_run(const Ctx& c, int32_t ms, int32_t off, int32_t ml) {
    Run M{ms, 0, ms - off, off < ml ? off : 0, R_HIST};
    if (ml == 0 || ms >= c.cap) return M;
    // (ms < cap <= 2^31 - 1: the room cap - ms is compared, never the sum ms + ml, which leaves int32 near the top)
    M.n = ml > c.cap - ms ? c.cap - ms : ml;
    // byte-wise: a dictionary source, a periodic source within 16 bytes of the
    // buffer start (its two-window pieces would read below it), or an output end
    // within 16 bytes (a plain source's 16-byte pieces stay inside [src, src + n))
    if (c.out_off + M.src < 0 || (M.period && c.out_off + M.src < 16) || c.cap - ms < 16) M.kind = R_BYTES;
    return M;
}
// One past the last output byte a match run reads.
__device__ __forceinline__ int32_t match_src_end(const Run& M) { return M.period ? M.y : M.src + M.n; }

__device__ __forceinline__ int run_pieces(int32_t n) {
    return n >= 16 ? (n + 15) >> 4 : (n <= 0 ? 0 : ((n & (n - 1)) == 0 ? 1 : 2));
}

// One store of a run: w bytes at y. mode 1 = window a, 2 = bytes [0, k) from
// window a and the rest from window b (a period that wraps), 3 = period
// `period` < w expanded from the 16 bytes at a starting at phase k,
// 4 = byte-wise (a = run offset, b = source start).
struct Piece {
    int32_t y, a, b, k, period;
    uint32_t w, mode, kind;
};

__device__ __forceinline__ Piece plan_piece(const Run& R, int p) {
    Piece P{0, 0, 0, 16, 0, 16u, 0u, R.kind};
    if (R.kind == R_NONE || p >= run_pieces(R.n)) return P;
    int32_t d;
    if (R.n >= 16) {
        P.w = 16;
        d = 16 * p < R.n - 16 ? 16 * p : R.n - 16;
    } else {
        P.w = R.n >= 8 ? 8u : R.n >= 4 ? 4u : R.n >= 2 ? 2u : 1u;
        d = p ? R.n - (int32_t)P.w : 0;
    }
    P.y = R.y + d;
    P.period = R.period;
    if (R.kind == R_BYTES) {
        P.mode = 4;
        P.a = d;
        P.b = R.src;
    } else if (R.period == 0) {
        P.mode = 1;
        P.a = R.src + d;
    } else {
        const int32_t per = R.period, r = d % per;
        if (per < (int32_t)P.w) {
            P.mode = 3;
            P.a = R.src;
            P.k = r;
        } else if (r + (int32_t)P.w <= per) {
            P.mode = 1;
            P.a = R.src + r;
        } else {
            P.mode = 2;
            P.a = R.src + r;
            P.b = R.src + r - per;    // >= src - 15: match_run keeps 16 bytes of margin
            P.k = per - r;
        }
    }
    return P;
}

typedef uint32_t u32x2_t __attribute__((ext_vector_type(2)));
typedef uint32_t u32x4_t __attribute__((ext_vector_type(4)));

__device__ __forceinline__ void store_w(uint8_t* p, uint4 v, uint32_t w) {
    if (w == 16) {
        __builtin_memcpy(p, &v, 16);
    } else if (w == 8) {
        __builtin_memcpy(p, &v, 8);
    } else if (w == 4) {
        __builtin_memcpy(p, &v.x, 4);
    } else if (w == 2) {
        uint16_t t = (uint16_t)v.x;
        __builtin_memcpy(p, &t, 2);
    } else {
        *p = (uint8_t)v.x;
    }
}

// bytes [0, k) from a, the rest from b
__device__ __forceinline__ uint32_t pick(uint32_t a, uint32_t b, int32_t k) {
    if (k >= 4) return a;
    if (k <= 0) return b;
    uint32_t m = (1u << (8 * k)) - 1u;
    return (a & m) | (b & ~m);
}
__device__ __forceinline__ uint4 pick4(uint4 a, uint4 b, int32_t k) {
    return make_uint4(pick(a.x, b.x, k), pick(a.y, b.y, k - 4), pick(a.z, b.z, k - 8), pick(a.w, b.w, k - 12));
}

// 16 bytes of a period per < 16 held in A[0, per), starting at phase r.
__device__ __forceinline__ uint4 expand_period(uint4 A, int32_t r, int32_t per) {
    uint32_t o[4] = {0, 0, 0, 0};
    int32_t idx = r;
#pragma unroll
    for (int j = 0; j < 16; ++j) {
        const uint32_t dw = idx < 4 ? A.x : idx < 8 ? A.y : idx < 12 ? A.z : A.w;
        o[j >> 2] |= ((dw >> ((idx & 3) * 8)) & 255u) << ((j & 3) * 8);
        idx = idx + 1 == per ? 0 : idx + 1;
    }
    return make_uint4(o[0], o[1], o[2], o[3]);
}

__device__ __forceinline__ void bytes_piece(const Ctx& c, int32_t y, int32_t a, int32_t src, uint32_t w, int32_t per) {
    uint32_t o[4] = {0, 0, 0, 0};
    for (uint32_t j = 0; j < w; ++j) {
        const int32_t d = a + (int32_t)j;
        const uint32_t v = hist_byte(c, (int64_t)src + (per ? d % per : d));
        o[j >> 2] |= v << ((j & 3) * 8);
    }
    store_w(c.dst + y, make_uint4(o[0], o[1], o[2], o[3]), w);
}

// A pipeline slot: one store of w bytes at y; mode 1 = window at a, 2 = bytes
// [0, k) from the window at a, the rest from the window at a - per (a period
// that wraps), 3 = period per < 16 expanded from the window at a from phase k.
// Windows are always 16 bytes (match_run / the staging slack keep them in bounds).
struct Slot {
    int32_t y, a, k, per;
    uint32_t wm;     // width | mode << 8
};

__device__ __forceinline__ Slot no_slot() { return Slot{0, 0, 0, 0, 0u}; }

// Slot of piece p of run R (R is not R_BYTES; wrapping periods only when TWO).
__device__ __forceinline__ Slot slot_of(const Run& R, int p) {
    const Piece P = plan_piece(R, p);
    return Slot{P.y, P.a, P.k, P.period, P.mode ? (P.w | (P.mode << 8)) : 0u};
}
template <uint32_t KIND>
__device__ __forceinline__ uint4 load16(const Ctx& c, const DecShared& S, int32_t a) {
    uint4 v;
    if (KIND == R_LDS) {
        v = stage16(S.stage, a);
    } else if (KIND == R_COMP) {
        __builtin_memcpy(&v, c.blk + a, 16);
    } else {
        const u32x4_t t = *(const u32x4_t*)(c.dst + a);
        v = make_uint4(t.x, t.y, t.z, t.w);
    }
    return v;
}

template <uint32_t KIND, bool TWO, int NB>
__device__ __forceinline__ void load_slots(const Ctx& c, const DecShared& S, const Slot (&s)[NB], uint4 (&A)[NB],
                                           uint4 (&B)[NB]) {
#pragma unroll
    for (int j = 0; j < NB; ++j) {
        if (LZ4MI_ABLATE == 5) { A[j] = make_uint4(0, 0, 0, 0); B[j] = A[j]; continue; }
        if (s[j].wm >> 8) A[j] = load16<KIND>(c, S, s[j].a);
        if (TWO && (s[j].wm >> 8) == 2) B[j] = load16<KIND>(c, S, s[j].a - s[j].per);
    }
}

template <bool TWO, int NB>
__device__ __forceinline__ void store_slots(const Ctx& c, DecShared& S, const Slot (&s)[NB], const uint4 (&A0)[NB],
                                            const uint4 (&B0)[NB]) {
    uint4 A[NB], B[NB];
#pragma unroll
    for (int j = 0; j < NB; ++j) {
        A[j] = A0[j];          // (consumed on every path: see lane_store)
        settle(A[j]);
        if (TWO) {
            B[j] = B0[j];
            settle(B[j]);
        }
        const uint32_t mode = s[j].wm >> 8;
        if (!mode) continue;
        uint4 v = A[j];
        if (TWO && mode == 2) v = pick4(A[j], B[j], s[j].k);
        else if (mode == 3) v = expand_period(A[j], s[j].k, s[j].per);
        if (LZ4MI_ABLATE == 4) {      // timing only: loads kept alive, no stores
            if ((v.x ^ v.y ^ v.z ^ v.w) == 0x9E3779B9u) S.pms[0] = 1;
            continue;
        }
        const uint32_t w = s[j].wm & 255u;
        if (w == 16) out16(c.dst + s[j].y, v);
        else store_w(c.dst + s[j].y, v, w);
    }
}

template <int NB>
__device__ __forceinline__ bool any_slot(const Slot (&s)[NB]) {
    uint32_t m = 0;
#pragma unroll
    for (int j = 0; j < NB; ++j) m |= s[j].wm;
    return m != 0;
}

// Software-pipelined copy: the loads of stage n+1 are issued before the stores
// of stage n, so no load waits behind a store it does not depend on (gfx9
// counts loads and stores in one in-order vmcnt). Gen::fill(Slot (&)[NB])
// hands out this lane's next pieces (sources already complete).
template <uint32_t KIND, bool TWO, int NB, class Gen>
__device__ __forceinline__ void pipe(const Ctx& c, DecShared& S, Gen& g) {
    // (every issued load is consumed by a store before the function returns: a load left
    // in flight at the exit would make the next write of its registers wait for vmcnt(0),
    // i.e. for every store in flight)
    Slot s0[NB], s1[NB];
    uint4 a0[NB], b0[NB], a1[NB], b1[NB];
    g.fill(s0);
    if (!__ballot(any_slot<NB>(s0))) return;
    load_slots<KIND, TWO, NB>(c, S, s0, a0, b0);
    for (;;) {
        g.fill(s1);
        if (!__ballot(any_slot<NB>(s1))) {
            store_slots<TWO, NB>(c, S, s0, a0, b0);
            return;
        }
        load_slots<KIND, TWO, NB>(c, S, s1, a1, b1);
        store_slots<TWO, NB>(c, S, s0, a0, b0);
        g.fill(s0);
        if (!__ballot(any_slot<NB>(s0))) {
            store_slots<TWO, NB>(c, S, s1, a1, b1);
            return;
        }
        load_slots<KIND, TWO, NB>(c, S, s0, a0, b0);
        store_slots<TWO, NB>(c, S, s1, a1, b1);
    }
}

// Pieces of the whole wave over one run: piece p0 + lane + 64 j.
template <int NB>
struct WaveGen {
    Run R;
    int np, p0, lane;
    __device__ __forceinline__ void fill(Slot (&s)[NB]) {
#pragma unroll
        for (int j = 0; j < NB; ++j) {
            const int p = p0 + lane + kWave * j;
            s[j] = p < np ? slot_of(R, p) : no_slot();
        }
        p0 += kWave * NB;
    }
};

// SeqInfo::rsrc (t_seq .w) of a sequence whose match source was mapped to finished output:
// the source + kMemoBase when the whole match was mapped (remap_src follows it in one step for
// later rows), + kSplitBase when only its part after a literal prefix was (0: not mapped).
// The sums are taken modulo 2^32; a mapped source rs lies in [-65536, 2^31). remap_src takes a
// value for a whole-match memo only inside [kMemoLo, kMemoHi), i.e. for rs in [-65536, 2^27): a
// whole-match value of a higher source lies above the window (from 2^30 on it wraps past 2^31),
// and a split value lies in [kSplitBase - 65536, 2^32), above it for every rs -- both are
// followed hop by hop, which is exact. (kSplitBase was 0x20000000: the split values of sources in
// [2^29 - 65536, 2^29 + 2^27) lay inside the window and were followed as whole-match memos, to a
// position 2^29 too low; tests/test_gpu_big_blocks.py.) piece_pipe subtracts the base its own
// round chose (rbits, nlit_pack), never by the value's range.
constexpr uint32_t kMemoBase = 0x40000000u, kSplitBase = 0x80000000u;
constexpr uint32_t kMemoLo = kMemoBase - 65536u, kMemoHi = kMemoBase + (1u << 27);
static_assert(kSplitBase - 65536u >= kMemoHi, "no split value inside the memo window");

// A match source [rs, re) inside this table's output, mapped back through the
// sequences that wrote it (out[y] = out[y - off] inside a match): 1 = it now
// lies in output finished by earlier chunks, 2 = in sequence j's literal run
// (*lds = its stage index), 0 = it straddles sequences / the table start.
// 3 (with `split`): it starts in sequence j's literal run and goes on into j's match:
// its first *nlit bytes are literal bytes at stage index *lds, the rest maps on to
// [rs, re) (finished output) — tiles216's usual reason for a later round (72 % of them).
// S.nxt doubles as an output -> sequence map during round 1: entry b is the
// sequence holding output O + (b << sh) (built by the kernel before round 1).
__device__ __forceinline__ int remap_src(const Ctx& c, const DecShared& S, uint32_t nseq, uint32_t sh, int32_t& rs,
                                         int32_t& re, int32_t& lds, int32_t& nlit, bool split) {
    nlit = 0;
    for (int d = 0; d < 8; ++d) {
        if (re <= (int32_t)c.O) return nlit ? 3 : 1;
        if (rs < (int32_t)c.O) return 0;
        uint32_t lo = S.nxt[(uint32_t)(rs - (int32_t)c.O) >> sh];   // last sequence starting at or before rs
        SeqInfo q = seq_info(S, lo);
        int32_t nx = lo + 1 < nseq ? (int32_t)S.t_seq[lo + 1].x : INT32_MAX;   // (read together with q)
        while (nx <= rs) {
            ++lo;
            q = seq_info(S, lo);
            nx = lo + 1 < nseq ? (int32_t)S.t_seq[lo + 1].x : INT32_MAX;
        }
        const int32_t t0 = q.out;
        const int32_t ms = t0 + q.ll;
        if (re <= ms) {
            if (nlit) return 0;   // (one split at most)
            lds = q.lit + (rs - t0);
            return 2;
        }
        if (rs < ms) {
            if (!split || nlit || ms - rs > 255 || re > ms + q.ml) return 0;
            lds = q.lit + (rs - t0);
            nlit = ms - rs;
            rs = ms;
        }
        if (re > ms + q.ml) return 0;
        if ((uint32_t)q.rsrc - kMemoLo < kMemoHi - kMemoLo) {
            // sequence lo's match was itself mapped (by an earlier row) to finished output:
            // follow that mapping in one step instead of hop by hop
            const int32_t base = (int32_t)((uint32_t)q.rsrc - kMemoBase) - ms;
            rs += base;
            re += base;
            continue;
        }
        rs -= q.off;
        re -= q.off;
    }
    return 0;
}

// One 16-byte piece of a match copy: y, source, width.
struct LSlot {
    int32_t y, a;
    uint32_t w;   // 0 = none
};

template <int NB>
__device__ __forceinline__ void lane_store(const Ctx& c, DecShared& S, const LSlot (&s)[NB], const uint4 (&A0)[NB]) {
    uint4 A[NB];
#pragma unroll
    for (int j = 0; j < NB; ++j) {
        // consumed on every path (a counted wait here): a load whose register is left
        // pending on the paths that skip its store would make the next chunk's first write
        // of that register wait for vmcnt(0) — for every store in flight
        A[j] = A0[j];
        settle(A[j]);
        if (!s[j].w) continue;
        if (LZ4MI_ABLATE == 4) {
            if ((A[j].x ^ A[j].y) == 0x9E3779B9u) S.pms[0] = 1;
            continue;
        }
        out16(c.dst + s[j].y, A[j]);
    }
}

// Piece-parallel copy of a set of ready matches (sources complete, non-periodic,
// 16 <= n <= kLaneBytes): every match is cut into 16-byte pieces (the last one
// overlaps its predecessor) and the pieces of all matches are dealt to the lanes
// in order, 64 per row, so one store instruction writes ~64 pieces of ~15
// consecutive matches (4-5 adjacent lanes per match) instead of one piece of
// each of 64 matches 64+ bytes apart, and no lane idles behind a longer match of
// another lane. A match list (rank -> {y, src, n, first piece}) and a bitmap of
// first pieces live in the pending-list LDS (free while a round writes); a lane
// finds its piece's match as the number of first pieces at or below it.
struct PEnt {
    int32_t y, src, n, p0;
};
constexpr int kPieceRows = 32;                 // bitmap rows: 2 sequence rows x 64 matches x <= 16 pieces
constexpr int kPieceBatch = 8;                 // piece rows whose loads are in flight together
static_assert(2 * kWave * (kLaneBytes / 16) <= kPieceRows * kWave, "bitmap holds two sequence rows");
static_assert(2 * kWave * sizeof(PEnt) + kPieceRows * 8 <= sizeof(uint32_t) * (kLim / 2 + kMaxSeq),
              "match list and bitmap fit the pending list");

struct PieceGen {
    const PEnt* L;
    const uint64_t* bm;
    uint32_t P;        // pieces
    uint32_t t;        // next row
    int32_t rb;        // ranks before row t, minus one
    int lane;
    template <int NB>
    __device__ __forceinline__ void fill(LSlot (&s)[NB]) {
#pragma unroll
        for (int j = 0; j < NB; ++j) {
            const uint32_t row = t + j;
            const uint32_t p = 64u * row + (uint32_t)lane;
            s[j] = LSlot{0, 0, 0u};
            if (64u * row < P) {
                const uint64_t w = bm[row];
                const int32_t below = (int32_t)__builtin_amdgcn_mbcnt_hi((uint32_t)(w >> 32),
                                                                        __builtin_amdgcn_mbcnt_lo((uint32_t)w, 0u));
                const int32_t r = rb + below + (int32_t)((w >> lane) & 1u);
                rb += __popcll(w);
                if (p < P) {
                    const PEnt e = L[r];
                    const int32_t d0 = 16 * ((int32_t)p - e.p0);
                    const int32_t d = d0 < e.n - 16 ? d0 : e.n - 16;
                    s[j] = LSlot{e.y + d, e.src + d, 16u};
                }
            }
        }
        t += NB;
    }
};

// The matches of sequences 64 i + lane for every bit i of `ready` (sources: SeqInfo::rsrc
// where `rbits` says so), two sequence rows per batch.
__device__ __forceinline__ void piece_pipe(const Ctx& c, DecShared& S, uint32_t ready, uint32_t rbits, int lane,
                                           uint32_t nseq, uint32_t nlit_pack) {
    PEnt* L = reinterpret_cast<PEnt*>(S.pme);
    uint64_t* bm = reinterpret_cast<uint64_t*>(reinterpret_cast<uint8_t*>(S.pme) + 2 * kWave * sizeof(PEnt));
    for (uint32_t i0 = 0; 64u * i0 < nseq; i0 += 2) {
        if (__ballot(((ready >> i0) & 3u) != 0) == 0) continue;
        if (lane < kPieceRows) bm[lane] = 0;
        __syncthreads();
        uint32_t P = 0, R = 0;
#pragma unroll
        for (uint32_t h = 0; h < 2; ++h) {
            const uint32_t i = i0 + h;
            const bool rd = (ready >> i) & 1u;
            int32_t y = 0, src = 0, n = 0;
            if (rd) {
                const uint32_t k = 64u * i + (uint32_t)lane;
                const SeqInfo q = seq_info(S, k);
                const int32_t ms = q.out + q.ll;
                const int32_t nl = i < 4 ? (int32_t)((nlit_pack >> (8 * i)) & 255u) : 0;   // split prefix
                y = ms + nl;
                n = (q.ml > c.cap - ms ? c.cap : ms + q.ml) - y;   // (ms < cap: match_run)
                src = (rbits >> i) & 1u ? (int32_t)((uint32_t)q.rsrc - (nl ? kSplitBase : kMemoBase)) : ms - q.off;
            }
            const uint32_t np = rd ? (uint32_t)(n + 15) >> 4 : 0u;
            const uint32_t incl = wave_incl_scan(np, lane);
            const uint64_t bal = __ballot(rd);
            const uint32_t r = R + __builtin_amdgcn_mbcnt_hi((uint32_t)(bal >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)bal, 0u));
            const uint32_t p0 = P + incl - np;
            if (rd) {
                L[r] = PEnt{y, src, n, (int32_t)p0};
                atomicOr((unsigned long long*)&bm[p0 >> 6], 1ull << (p0 & 63u));
            }
            P += lane_of(incl, kWave - 1);
            R += (uint32_t)__popcll(bal);
        }
        __syncthreads();
        PieceGen g{L, bm, P, 0u, -1, lane};
        // kPieceBatch rows at a time, all loads before all stores: every slot loads (an empty
        // one the block's first 16 bytes), so the loads are straight-line code and each store
        // waits only for its own load (counted vmcnt), not for every store in flight
        while (64u * g.t < P) {
            LSlot sl[kPieceBatch];
            uint4 v[kPieceBatch];
            g.template fill<kPieceBatch>(sl);
#pragma unroll
            for (int j = 0; j < kPieceBatch; ++j) {
                const u32x4_t t = *(const u32x4_t*)(c.dst + (sl[j].w ? sl[j].a : 0));
                v[j] = make_uint4(t.x, t.y, t.z, t.w);
            }
            lane_store<kPieceBatch>(c, S, sl, v);
        }
        __syncthreads();   // the next batch rewrites the list
    }
}

// A lane's match run the pipeline does not take (periodic, or byte-wise near a
// buffer edge / in the dictionary): piece by piece.
__device__ __forceinline__ void lane_slow_run(const Ctx& c, const DecShared& S, const Run& R) {
    const int np = run_pieces(R.n);
    for (int p = 0; p < np; ++p) {
        const Piece P = plan_piece(R, p);
        if (P.mode == 4) {
            bytes_piece(c, P.y, P.a, P.b, P.w, P.period);
            continue;
        }
        const uint4 A = load16<R_HIST>(c, S, P.a);
        uint4 v = A;
        if (P.mode == 2) v = pick4(A, load16<R_HIST>(c, S, P.b), P.k);
        else if (P.mode == 3) v = expand_period(A, P.k, P.period);
        store_w(c.dst + P.y, v, P.w);
    }
}

// Long periodic run (match offset < length): the pattern plus 20 bytes of its
// repetition are copied into LDS, then every 16-byte piece at output distance d
// is five aligned dword reads at phase d mod period (no history re-reads through
// the fabric, one output stream per lane). A period longer than the buffer is
// done in slices of phases, one LDS fill and one pass over the run per slice,
// each pass writing the pieces whose phase falls in its slice.
__device__ __forceinline__ void periodic_run(const Ctx& c, const DecShared& S, int lane, const Run& R, PatBuf B) {
    const int32_t per = R.period;
    const uint8_t* src = c.dst + R.src;
    const int32_t W = B.bytes - 48;   // phases per slice (the fill covers W + 20 bytes, rounded to 16)
    const int32_t dl = R.n - 16;      // the last piece (overlaps its predecessor when n % 16)
    for (int32_t s0 = 0; s0 < per; s0 += W) {
        const int32_t e0 = per - s0 <= W ? per : s0 + W;   // this slice's phases [s0, e0)
        __syncthreads();
        for (int k = lane; 16 * k < e0 - s0 + 20; k += kWave) {
            const int32_t q = s0 + 16 * k;
            uint4 v;
            if (q + 16 <= per) {
                v = load16<R_HIST>(c, S, R.src + q);
            } else {
                unsigned __int128 x = 0;
#pragma unroll 1
                for (int j = 0; j < 16; ++j) x |= (unsigned __int128)src[(q + j) % per] << (8 * j);
                __builtin_memcpy(&v, &x, 16);
            }
            B.w[4 * k] = v.x;
            B.w[4 * k + 1] = v.y;
            B.w[4 * k + 2] = v.z;
            B.w[4 * k + 3] = v.w;
        }
        __syncthreads();
        // every piece whose phase falls in this slice; the phase is carried from piece to piece
        // pieces on the absolute 16-byte grid (whole-line stores), the unaligned head piece
        // written once more by lane 0 (same bytes), the last piece overlapping its predecessor
        const int32_t a0 = (int32_t)((0u - (uint32_t)(uintptr_t)(c.dst + R.y)) & 15u);
        if (lane == 0 && a0) {
            const int32_t ph = 0 - s0;
            if ((uint32_t)ph < (uint32_t)(e0 - s0)) out16(c.dst + R.y, stage16(B.w, ph));
        }
        const int32_t np = (R.n - a0 + 15) >> 4;
        const int32_t step = (16 * kWave) % per;
        int32_t r = (a0 + 16 * lane) % per;
#pragma unroll 2
        for (int32_t p = lane; p < np; p += kWave) {
            const int32_t d0 = a0 + 16 * p;
            const bool last = d0 > dl;
            const int32_t d = last ? dl : d0;
            const int32_t ph = (last ? d % per : r) - s0;
            if ((uint32_t)ph < (uint32_t)(e0 - s0) && LZ4MI_ABLATE != 4) {
                out16(c.dst + R.y + d, stage16(B.w, ph));
            }
            r += step;
            if (r >= per) r -= per;
        }
    }
    __syncthreads();
}


// A long literal run (incompressible data: one run per block) copied global ->
// global with 4 16-byte pieces per lane in flight (4 KiB per wave), enough to
// keep HBM busy with one wave per block; the last piece overlaps its predecessor.
// Paced (LZ4MI_LL_ADAPT) while latency-bound blocks run on the same XCD: at full rate
// these copies fill the CU's vector-memory queues, and the blocks of short matches beside
// them, whose every chunk waits on a few dependent history reads, slow down by ~25 % for
// as long as the copies run (the per-block timeline, DESIGN §4.1 "Round 5"); spread out,
// the copies finish later but inside those blocks' own lifetime.
__device__ __forceinline__ void long_literals(uint8_t* dst, const uint8_t* src, int32_t n, int lane) {
    const int32_t np = (n + 15) >> 4;
    auto at = [&](int32_t p) { return 16 * p < n - 16 ? 16 * p : n - 16; };   // past the end: the last piece again
#if LZ4MI_LL_ADAPT
    const unsigned int* lat = &g_lat_active[32 * xcc_id()];
#endif
    for (int32_t p0 = lane; p0 < np; p0 += kWave * 4) {
#if LZ4MI_LL_ADAPT
        // (issued before the step's loads: its wait is not behind theirs)
        const uint32_t busy = __hip_atomic_load(lat, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#endif
        const int32_t d0 = at(p0), d1 = at(p0 + kWave), d2 = at(p0 + 2 * kWave), d3 = at(p0 + 3 * kWave);
        uint4 v0, v1, v2, v3;
        // streamed once, never re-read soon: nontemporal, so they do not evict the history lines
        // other blocks' matches read back from L2
        v0 = ld16_nt(src + d0);
        v1 = ld16_nt(src + d1);
        v2 = ld16_nt(src + d2);
        v3 = ld16_nt(src + d3);
        st16_nt(dst + d0, v0);
        st16_nt(dst + d1, v1);
        st16_nt(dst + d2, v2);
        st16_nt(dst + d3, v3);
#if LZ4MI_LL_ADAPT
        if (busy) __builtin_amdgcn_s_sleep(LZ4MI_LL_ADAPT);
#endif
    }
}

// The whole wave writes one run (uniform R).
__device__ __forceinline__ void wave_run(const Ctx& c, DecShared& S, int lane, const Run& R, PatBuf B) {
    if (R.kind == R_NONE || R.n <= 0) return;
    // (a byte-wise periodic run whose source is inside the buffer qualifies too:
    // periodic_run reads only [src, src + period))
    const bool in_buf = R.kind == R_HIST || (R.kind == R_BYTES && c.out_off + R.src >= 0);
    if (in_buf && R.period && R.n > kPeriodBulk &&
        B.bytes > 0 && (R.period + 48 <= B.bytes || (R.n >= 4 * R.period && B.bytes >= 1024))) {
        periodic_run(c, S, lane, R, B);
        return;
    }
    const int np = run_pieces(R.n);
    if (R.kind == R_BYTES) {
        for (int p = lane; p < np; p += kWave) {
            const Piece P = plan_piece(R, p);
            bytes_piece(c, P.y, P.a, P.b, P.w, P.period);
        }
        return;
    }
    if (R.period) {
        WaveGen<kWaveB2> g{R, np, 0, lane};
        pipe<R_HIST, true, kWaveB2>(c, S, g);
        return;
    }
    WaveGen<kWaveB> g{R, np, 0, lane};
    if (R.kind == R_LDS) pipe<R_LDS, false, kWaveB>(c, S, g);
    else if (R.kind == R_COMP && R.n >= kLongLit) long_literals(c.dst + R.y, c.blk + R.src, R.n, lane);
    else if (R.kind == R_COMP) pipe<R_COMP, false, kWaveB>(c, S, g);
    else pipe<R_HIST, false, kWaveB>(c, S, g);
}

// A literal run of 1..15 bytes (v: its stage bytes) in 8/4/2/1-byte pieces by the bits of n
// (no per-width branches).
__device__ __forceinline__ void short_literals(const Ctx& c, int32_t y, int32_t n, const uint4& v) {
    if (LZ4MI_ABLATE == 4) return;
    uint8_t* d = c.dst + y;
    uint64_t lo = v.x | ((uint64_t)v.y << 32);
    const uint64_t hi = v.z | ((uint64_t)v.w << 32);
    int32_t o = 0;
    if (n & 8) { __builtin_memcpy(d, &lo, 8); lo = hi; o = 8; }
    if (n & 4) { const uint32_t t = (uint32_t)lo; __builtin_memcpy(d + o, &t, 4); lo >>= 32; o += 4; }
    if (n & 2) { const uint16_t t = (uint16_t)lo; __builtin_memcpy(d + o, &t, 2); lo >>= 16; o += 2; }
    if (n & 1) d[o] = (uint8_t)lo;
}

// Literal runs from the staged chunk (R_LDS), piece-parallel like the matches of piece_pipe:
// every run of >= 16 bytes is cut into 16-byte pieces (the last one overlaps its predecessor, so
// no byte outside [y, y + n) is written) and the pieces of all listed runs are dealt to the
// lanes in order, 64 per row; a lane does one stage16 and one out16 per row instead of every
// lane going round as often as the row's longest run needs. The run list (rank -> {y, stage
// index, n, first piece}) and the first-piece bitmap live in S.pms: the token list there is
// dead after seq_table, and round 1 needs it only for a whole-wave periodic match
// (pat_round1), before which the list is flushed.
// Two users: the chunk's own literal runs, once before round 1's loop (dealt_literals), and
// round 1's remapped sources (a match mapped into a literal run, the literal prefix of a
// split match), listed row by row and flushed when the list is full and after the loop.
// A remapped source of under 16 bytes is listed too, as one piece of its exact width
// (short_literals): round 1's row loop then holds no literal store at all.
// Bounds: the literals of a table's sequences lie inside the window (else the sequence is
// cut), so a chunk's own runs hold <= kLim bytes together, and each run of >= 16 bytes takes
// >= 17 compressed bytes of a token starting in the chunk: all of them fit one list. A
// remapped run is at most kLaneBytes long, i.e. kLaneBytes / 16 pieces, and one of under 16
// bytes is one piece: kLitRuns entries hold at most kLitRows * 64 pieces.
constexpr int kLitRuns = 64;                                   // list entries
constexpr int kLitRows = kLitRuns * (kLaneBytes / 16) / 64;    // bitmap rows
static_assert((kChunk + 16) / 17 <= kLitRuns, "every run of >= 16 literal bytes of a chunk has a list entry");
static_assert(kLim / 16 + kLitRuns <= 3 * 64, "a chunk's own runs: at most three piece rows");
static_assert(kLim / 16 + kLitRuns <= kLitRows * 64, "... which the bitmap holds");
static_assert(kLitRuns * sizeof(PEnt) + kLitRows * 8 <= sizeof(uint32_t) * kMaxSeq, "run list and bitmap fit S.pms");
static_assert(kLitRows <= kWave, "one lane clears each bitmap word");
static_assert(offsetof(DecShared, pms) % 16 == 0, "16-byte aligned list entries");

struct LitDeal {
    uint32_t P = 0, R = 0;   // pieces and runs listed (wave-uniform)
    static __device__ __forceinline__ PEnt* list(DecShared& S) { return reinterpret_cast<PEnt*>(S.pms); }
    static __device__ __forceinline__ uint64_t* bitmap(DecShared& S) {
        return reinterpret_cast<uint64_t*>(reinterpret_cast<uint8_t*>(S.pms) + kLitRuns * sizeof(PEnt));
    }
    // Lists the run {y, src, n >= 1} of every lane with `has` (bal = its ballot, not 0; at most
    // kLitRuns - R lanes).
    __device__ __forceinline__ void add(DecShared& S, int lane, bool has, uint64_t bal, int32_t y, int32_t src, int32_t n) {
        if (R == 0) {
            if (lane < kLitRows) bitmap(S)[lane] = 0;
            __syncthreads();
        }
        const uint32_t np = has ? (uint32_t)(n + 15) >> 4 : 0u;
        const uint32_t incl = wave_incl_scan(np, lane);
        const uint32_t r = R + __builtin_amdgcn_mbcnt_hi((uint32_t)(bal >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)bal, 0u));
        const uint32_t p0 = P + incl - np;
        if (has) {
            list(S)[r] = PEnt{y, src, n, (int32_t)p0};
            atomicOr((unsigned long long*)&bitmap(S)[p0 >> 6], 1ull << (p0 & 63u));
        }
        P += lane_of(incl, kWave - 1);
        R += (uint32_t)__popcll(bal);
    }
    // Writes the listed runs and empties the list.
    __device__ __forceinline__ void flush(const Ctx& c, DecShared& S, int lane) {
        if (R == 0) return;
        __syncthreads();
        const PEnt* L = list(S);
        const uint64_t* bm = bitmap(S);
        int32_t rb = -1;   // ranks before this row, minus one
        for (uint32_t t = 0; 64u * t < P; ++t) {
            const uint64_t w = bm[t];
            const int32_t below = (int32_t)__builtin_amdgcn_mbcnt_hi((uint32_t)(w >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)w, 0u));
            const int32_t r = rb + below + (int32_t)((w >> lane) & 1u);
            rb += __popcll(w);
            const uint32_t p = 64u * t + (uint32_t)lane;
            if (p < P) {
                const PEnt e = L[r];
                if (e.n < 16) {   // (a remapped source of round 1: its exact width)
                    short_literals(c, e.y, e.n, stage16(S.stage, e.src));
                } else {
                    const int32_t d0 = 16 * ((int32_t)p - e.p0);
                    const int32_t d = d0 < e.n - 16 ? d0 : e.n - 16;
                    const uint4 v = stage16(S.stage, e.src + d);
                    if (LZ4MI_ABLATE != 4) out16(c.dst + e.y + d, v);
                }
            }
        }
        __syncthreads();   // the list may be rewritten, or S.pms reused (pat_round1)
        P = R = 0;
    }
};

// The chunk's own literal runs, all of them, before round 1's loop: those of >= 16 bytes listed
// and dealt, the shorter ones written by their own lanes in 8/4/2/1-byte pieces behind one
// ballot per row (a row of text, where all 64 lanes hold one, costs what it cost inside round
// 1's loop). A row with neither pays the two ballots.
__device__ __forceinline__ void dealt_literals(const Ctx& c, DecShared& S, int lane, uint32_t nseq) {
    LitDeal D;
    for (uint32_t i = 0; 64 * i < nseq; ++i) {
        const uint32_t k = 64 * i + lane;
        const uint4& e = S.t_seq[k < nseq ? k : 0u];
        const uint32_t y = e.x, lw = e.y;
        const uint32_t n = k < nseq ? lw >> 16 : 0u;
        const bool has = n >= 16, shortL = n > 0 && n < 16;
        const uint64_t bal = __ballot(has);
        if (bal) D.add(S, lane, has, bal, (int32_t)y, (int32_t)(lw & 0xFFFFu), (int32_t)n);
        if (__ballot(shortL)) {
            if (shortL) short_literals(c, (int32_t)y, (int32_t)n, stage16(S.stage, (int32_t)(lw & 0xFFFFu)));
        }
    }
    D.flush(c, S, lane);
}

// Wave-wide 255-run varint starting at block-relative q: returns the sum and
// advances q past the terminating byte. Bytes past the block end read as 0.
__device__ __forceinline__ int64_t wave_varint(const Ctx& c, int lane, int64_t& q) {
    int64_t sum = 0;
    for (;;) {
        int64_t p = q + 16 * lane;
        int first = 16;
        uint32_t lastb = 0;
        for (int j = 0; j < 16; ++j) {
            int64_t r = p + j;
            uint32_t b = (r < c.in_len) ? c.blk[r] : 0u;
            if (b != 255u && first == 16) { first = j; lastb = b; }
        }
        uint64_t mask = __ballot(first < 16);
        if (mask) {
            int fl = __builtin_ctzll(mask);
            int fi = lane_of(first, fl);
            uint32_t fb = lane_of(lastb, fl);
            int64_t cnt = (int64_t)fl * 16 + fi;
            sum += 255 * cnt + fb;
            q += cnt + 1;
            return sum;
        }
        sum += 255 * 16 * kWave;
        q += 16 * kWave;
    }
}

// Error of a sequence per the reference's check order (0 = none):
// 1 Output Buffer Too Small, 2 Malformed Input, 3 Invalid Offset 0,
// 4 Dictionary Offset Out of Bounds, 5 reaches into another block's output.
__device__ __forceinline__ uint32_t seq_error(const Ctx& c, int64_t out_start, int64_t lit, int64_t ll, uint32_t off,
                                              int64_t ml) {
    if (out_start + ll > c.cap) return 1;
    if (lit + ll > c.in_len) return 2;
    if (ml == 0) return 0;                                // final literal-only sequence
    if (off == 0) return 3;
    int64_t ms_abs = c.out_off + out_start + ll;
    if ((int64_t)off > ms_abs + c.dict_len) return 4;
    if (c.isolate && (int64_t)off > out_start + ll) return 5;
    return 0;
}

__device__ __forceinline__ int32_t err_status(uint32_t e) { return e == 5 ? -9 : -(int32_t)e; }
// An exported segment (XP, rel) knows only its relative output positions: checks 2 and 3 here,
// 1, 4 and 5 after the parse (lz4mi_xcheck_kernel), in the same order per sequence.
template <bool XP>
__device__ __forceinline__ uint32_t seq_err(const Ctx& c, bool rel, int64_t out_start, int64_t lit, int64_t ll,
                                            uint32_t off, int64_t ml) {
    if (XP && rel) {
        if (lit + ll > c.in_len) return 2;
        if (ml == 0) return 0;
        return off == 0 ? 3u : 0u;
    }
    return seq_error(c, out_start, lit, ll, off, ml);
}

// Would the reference's double-copy-tail rewrite (src/block/blockDecompress.js:219-250,
// offset >= 8, length < 8, source in the output) change a byte of
// this match's finished output? out[p] = out[p - off] for p in [ms + ml - 8, ms).
// Reads bytes of this wave's completed output (after wait_vmem).
// 0 = no change, 1 = changes (re-decode serially), 2 = the rewrite reads bytes
// before the block's start: another block's output in a batch (reported as
// LZ4MI_ERR_CROSS_BLOCK there, like any back-reference out of the block).
__device__ __forceinline__ uint32_t f1_changes(const Ctx& c, int32_t ms, int32_t off, int32_t ml) {
    if (ml == 0 || ml >= 8 || off < 8 || c.out_off + ms - off < 0) return 0;
    const int32_t p0 = ms + ml - 8;
    if (p0 - off < 0) return c.isolate ? 2u : 1u;
    for (int32_t p = p0; p < ms && p < c.cap; ++p)
        if (hist_u8(c.dst + p) != hist_u8(c.dst + p - off)) return 1;
    return 0;
}

// Reference-exact fix-up of one chunk (LZ4MI_JS_EXACT) whose matches include a
// double-copy-tail rewrite that changes bytes (f1_changes == 1): the chunk was written
// with spec semantics; replay its matches in order with the reference's semantics.
// Literal bytes never change. Everything before the first rewritten position `lo` is
// already final, so a match is copied again only if its source reaches past `lo`
// (periodic copy: its source bytes before its start are final when it runs), and every
// rewrite is applied (blockDecompress.js:219-250: out[p] = out[p - off] for
// p in [ms + ml - 8, ms), after the copy). Later chunks then read the fixed output.
// (a call, never inlined: it is rare, and its registers are not the chunk loop's)
__device__ __noinline__ void f1_fixup(const Ctx c, const DecShared& S, int lane, uint32_t nseq, bool cut, int64_t cut_ms,
                         int32_t coff, int32_t cml) {
    int64_t lo = INT64_MAX;
    const uint32_t n = nseq + (cut ? 1u : 0u);
    for (uint32_t k = 0; k < n; ++k) {
        int64_t ms;
        int32_t off, ml;
        if (k < nseq) {
            const SeqInfo q = seq_info(S, k);
            ms = (int64_t)q.out + q.ll;
            off = q.off;
            ml = q.ml;
        } else {
            ms = cut_ms;
            off = coff;
            ml = cml;
        }
        if (ml == 0) continue;
        const bool internal = c.out_off + ms - off >= 0;   // the reference's non-dictionary branch
        if (ms - off + ml > lo) {
            if (internal) {
                for (int32_t t = lane; t < ml; t += kWave) {
                    const int64_t d = ms + t;
                    const int64_t s = ms - off + (off < ml ? t % off : t);
                    const uint32_t v = hist_u8(c.dst + s);
                    if (d < c.cap) c.dst[d] = (uint8_t)v;
                }
            } else if (lane == 0) {   // spills from the dictionary into the output: in order, byte by byte
                for (int32_t t = 0; t < ml; ++t) {
                    const uint32_t v = hist_byte(c, ms - off + t);
                    if (ms + t < c.cap) c.dst[ms + t] = (uint8_t)v;
                }
            }
            wait_vmem();
        }
        if (internal && off >= 8 && ml < 8) {
            const int64_t p = ms + ml - 8 + lane;
            const bool mine = lane < 8 - ml && c.out_off + p >= 0 && p < c.cap;
            const uint32_t v = mine ? (c.out_off + p - off >= 0 ? hist_u8(c.dst + p - off) : 0u) : 0u;
            if (mine) c.dst[p] = (uint8_t)v;
            const int64_t p0 = ms + ml - 8;
            if (p0 < lo) lo = p0;
            wait_vmem();
        }
    }
}

// ---------------------------------------------------------------- the block
// A frame's stored block (bufferDecompress.js:173-180): its bytes, in this launch, paced
// like any long literal run; larger than the slot: the reference's RangeError.
__device__ __forceinline__ int32_t stored_block(const DecArgs& a, const Ctx& c, uint32_t b, uint32_t out_cap, int lane) {
    int32_t status = 0;
    const int32_t n = c.in_len;
    if ((uint32_t)n > out_cap) {
        status = LZ4MI_ERR_RANGE_STATUS;
    } else if (n >= 16) {
        long_literals(c.dst, c.blk, n, lane);
    } else if (lane < n) {
        c.dst[lane] = c.blk[lane];
    }
    if (lane == 0) {
        a.status[b] = status;
        a.out_len[b] = status ? 0u : (uint32_t)n;
    }
    return status;
}

// ---------------------------------------------------------------- export (XP)
// Small-batch export (lz4mi_expand.hip): a wave per segment of the block, which parses its
// segment and exports the sequences instead of writing them. All of it uniform.
struct XState {
    bool on = false;                    // this block is exported (else: one wave decodes it as usual)
    uint4* xs = nullptr;                // the segment's exported sequences
    SegRec* xr = nullptr;               // its record
    uint32_t seg_lo = 0, seg_hi = 0;    // the segment: tokens in [seg_lo, seg_hi)
    // the entry found, done, the speculation failed, entry / exit tokens, sequences exported,
    // their output bytes, the first parse error; OG: output position of the entry in this
    // wave's running count; pass 1 / 2: the re-parse from `entry` of phase 1 (exact) / 2
    bool started = false, done = false, fail = false;
    uint32_t G = 0, X = 0, nx = 0, olen = 0, err = 0xFFFFFFFFu, entry = 0;
    int64_t OG = 0;
    int pass = 0, restart = 0;
};

// Does this wave (segment sg of block wblk, phase a.xphase) parse at all? Sets x.on, the
// segment, the pass and c.ip, where its parse starts.
// LK: a linked window (LZ4MI_LINKED, lz4mi_expand.hip): every block left exported by
// lz4mi_linked_prep_kernel is within the export limits and is parsed for export whatever its ratio --
// a one-wave decode would write `out` and read predecessors the gather has not written yet.
template <bool LK>
__device__ __forceinline__ bool x_enter(const DecArgs& a, Ctx& c, XState& x, int lane, uint32_t wblk, uint32_t sg,
                                        uint32_t nseg, uint32_t out_cap) {
    // (a block of long runs -- output over 32x its compressed size: repetitive data, one periodic
    // match -- decodes faster in one wave, as in the batch kernel: 1.1 ms for 4 MiB at any batch
    // size, against 0.77 ms alone / 1.57 ms for 16 through the pointers, profiles/r06c)
    x.on = LK || ((uint32_t)c.in_len <= a.x_in_max && out_cap <= a.x_out_max &&
                  (uint64_t)out_cap < (uint64_t)c.in_len * kXRatioMax &&
                  !(a.x_flat1 && (uint64_t)c.in_len * 16 >= (uint64_t)out_cap * 15));
    // past the export limits (or ratio >= 32): one wave decodes the block as usual -- segment
    // b mod 256, i.e. workgroup 257 b (mod 256 CUs: a CU of its own for every block, where
    // segment 0 would put the blocks of a batch on one CU)
    if (!x.on) return a.xphase == 0 && sg == wblk % nseg;
    const SegGeom G = seg_geom((uint32_t)c.in_len);   // S segments of ~kSegTarget bytes
    if (sg >= G.S) return false;
    x.seg_lo = sg * G.L;
    x.seg_hi = sg + 1 == G.S ? (uint32_t)c.in_len : min((uint32_t)c.in_len, x.seg_lo + G.L);
    x.xs = a.xseq + (size_t)wblk * a.xseq_stride + (size_t)sg * G.stride;
    x.xr = a.xrec + (size_t)wblk * nseg + sg;
    SegRec* const xr = x.xr;
    if (a.xphase == 2) {
        // phase 2: every segment whose guess disagrees with the previous one's exit, re-parsed
        // from that exit at once (lz4mi_xverify_kernel's `from`), a guess again -- the check then
        // runs again: a wrong guess does not make the later guesses wrong, and the segments
        // before a wrong one are mostly right (text, ~10 % of ~190 segments: chained one after
        // another in phase 1, 2.1 ms for a block)
        const uint32_t from = uniform(xr->from);
        if (from == kNoBase) return false;
        x.pass = 2;
        x.entry = from;
    }
    if (a.xphase == 1) {
        // phase 1: segments from the first wrong entry on, in order: re-parse from the previous
        // segment's final exit unless the speculative entry equals it
        const uint32_t sstar = a.xfirst[wblk];
        if (sg < sstar) return false;
        uint32_t fp = 0;
        if (sg == sstar) {
            fp = xr[-1].exit;                    // final: accepted by lz4mi_xverify_kernel
        } else {
            if (lane == 0) {
                const uint32_t* f = &xr[-1].fin;
                while ((fp = __hip_atomic_load(f, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT)) == 0u)
                    __builtin_amdgcn_s_sleep(8);
            }
            fp = lane_of(fp, 0) - 1u;
        }
        uint32_t fin = 0;
        bool reparse = false;
        if (fp == kFinErr) {                     // after the block's first error: nothing here
            fin = kFinErr;
            if (lane == 0) { xr->cnt = 0; xr->olen = 0; xr->err = 0xFFFFFFFFu; }
        } else if (fp >= x.seg_hi) {             // the chain passes over the segment
            fin = fp;
            if (lane == 0) { xr->entry = xr->exit = fp; xr->cnt = 0; xr->olen = 0; xr->err = 0xFFFFFFFFu; }
        } else if (sg != sstar && !xr->fail && xr->entry == fp) {
            fin = xr->err != 0xFFFFFFFFu ? kFinErr : xr->exit;
        } else {
            reparse = true;
        }
        if (!reparse) {
            if (lane == 0) __hip_atomic_store(&xr->fin, fin + 1u, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
            return false;
        }
        x.pass = 1;
        x.entry = fp;
    }
    // a guess: from kSegWarm before the segment, on whatever chain the walk falls onto
    c.ip = x.pass ? (int32_t)x.entry
                  : (x.seg_lo >= (uint32_t)c.in_len ? c.in_len : (int32_t)(x.seg_lo - min(x.seg_lo, kSegWarm)));
    return true;
}

// ---------------------------------------------------------------- 1. staging
// The 16-byte pieces of [at, at + kLim), two per lane (unaligned loads).
__device__ __forceinline__ void stage_loads(const Ctx& c, int64_t at, int lane, uint4& p0, uint4& p1) {
    p0 = stage_piece(c, at + 16 * opaque(lane));
    if (lane < kStageWords / 4 - kWave) p1 = stage_piece(c, at + 16 * (kWave + opaque(lane)));
}
__device__ __forceinline__ void stage_write(DecShared& S, int lane, const uint4& p0, const uint4& p1) {
    __builtin_memcpy((uint8_t*)S.stage + 16 * lane, &p0, 16);
    if (lane < kStageWords / 4 - kWave) __builtin_memcpy((uint8_t*)S.stage + 16 * (kWave + lane), &p1, 16);
}

// The next chunk's staged bytes, loaded early: during this chunk's table build or, after a
// cut sequence, ahead of this chunk's stores.
struct Prefetch {
    uint4 pf0 = make_uint4(0, 0, 0, 0), pf1 = make_uint4(0, 0, 0, 0);
    int64_t pf_at = -1;     // compressed position pf0/pf1 were loaded from
    bool have_pf = false;
};
__device__ __forceinline__ void prefetch(const Ctx& c, Prefetch& pf, int64_t at, int lane) {
    stage_loads(c, at, lane, pf.pf0, pf.pf1);
    pf.pf_at = at;
    pf.have_pf = true;
}
// Explicitly waited for (wait_vmem): the next chunk's stage does not wait for this chunk's stores.
__device__ __forceinline__ void settle(Prefetch& pf) {
    settle(pf.pf0);
    settle(pf.pf1);
}

// Stage [ip, ip + kLim), from the prefetch when it was loaded from ip.
// (each branch writes the stage itself: a write after the join would wait for the
// fresh loads of the first branch on both, i.e. for every store still in flight)
__device__ __forceinline__ void stage_chunk(const Ctx& c, DecShared& S, Prefetch& pf, int lane) {
    if (!pf.have_pf || pf.pf_at != c.ip) {
        uint4 p0, p1 = make_uint4(0, 0, 0, 0);
        stage_loads(c, (int64_t)c.ip, lane, p0, p1);
        stage_write(S, lane, p0, p1);
    } else {
        stage_write(S, lane, pf.pf0, pf.pf1);
    }
    pf.have_pf = false;
    __syncthreads();
}

// ---------------------------------------------------------------- 2, 3. chunk parse
// The exact serial parse of the staged chunk: lane l's tokens in [16 l, 16 l + 16) as the bits
// of `vis`; where the chain leaves the chunk (`tail`: chunk-relative, kEnd or kStop); the last
// token starting in the chunk and its lane; `cut`: that token's sequence leaves the staged
// window (tail == kStop) and is parsed from memory (cut_seq).
struct Parse {
    uint32_t vis, tail, last_tok;
    int last_lane;
    bool cut;
};
// `defer`: a last token whose sequence overruns the window but would fit one it starts (by the
// fast table's raw next value: under kLim bytes) is left to the next chunk, which begins at it,
// instead of being cut: its literals then come from LDS and its match joins the piece list
// (tiles216: 151 cuts in a block's 484 chunks are such sequences of 65-261 literal bytes).
// The chunk's first token is never deferred, so every chunk advances.
__device__ __forceinline__ Parse parse_chunk(DecShared& S, int lane, uint32_t rem, bool fast_tab, bool defer, Prof& prof) {
    const uint8_t* s = (const uint8_t*)S.stage;
    const uint32_t seg0 = 16u * lane, seg1 = seg0 + 16;
    uint32_t vis, tail;
    PROF(0);
    // Wave priorities by phase (the 4 waves of a SIMD are in different phases):
    // output rounds 3 > walks 1 > next-token table 0. The copies' loads and
    // stores go out first and the LDS-bound parse fills the gaps: tiles216 -0.9 %,
    // mix -2.5 %, copy -1.5 % (A/B in one process, profiles/r02j/prio_ab.json).
    __builtin_amdgcn_s_setprio(0);
    // ---- 2. next-token table -----------------------------------------
    // Away from the block's end (fast_tab) four positions per lane from two stage
    // dwords, assuming length fields of at most one extension byte: a token whose
    // literal field runs on (b1 == 255) stops the chain (the cut path parses it), and
    // a match field that runs on (checked on the true tokens in the table build) sends
    // the chunk back here for the exact table. Near the end: the exact table.
    uint16_t* nxt = S.nxt;
    if (fast_tab) {
        next_table_fast(S.stage, nxt, lane);
    } else {   // all positions' fields read at once; the rare longer length fields afterwards
        static_assert(kChunk % kWave == 0, "whole rows per lane");
        uint32_t slm = 0;
#pragma unroll
        for (int i = 0; i < kChunk / kWave; ++i) {
            bool slow;
            const uint32_t v = next_fast(s, lane + kWave * i, rem, slow);
            slm |= (slow ? 1u : 0u) << i;
            nxt[lane + kWave * i] = enc_next(v);
        }
        if (__ballot(slm != 0)) {
            for (uint32_t m = slm; m; m &= m - 1) {
                const uint32_t p = lane + kWave * __builtin_ctz(m);
                nxt[p] = enc_next(next_token(s, p, rem));
            }
        }
    }
    __syncthreads();
    // 2- and 4-step jumps (the warm-up walks only need where the chain lands)
    jump_table(nxt, S.nxt2, lane);
    __syncthreads();
    jump_table(S.nxt2, S.nxt4, lane);
    __syncthreads();
#if LZ4MI_ABLATE == 3
    return Parse{0u, (uint32_t)kChunk, 0u, 0, false};   // (the chunk loop steps by kChunk)
#endif

    PROF(1);
    __builtin_amdgcn_s_setprio(1);
    // ---- 3. speculative walks + certification -------------------------
    uint32_t x;
    vis = 0;
    {   // warm-up walk; lanes whose warm-up would start before the chunk start at it, a true token
        uint32_t p = seg0 < kWarm ? 0u : seg0 - kWarm;
        for (uint32_t q; (q = S.nxt4[p]) < seg0;) p = q;    // jumps stay short of the segment
        for (uint32_t q; (q = S.nxt2[p]) < seg0;) p = q;
        while (p < seg1) {
            if (p >= seg0) vis |= 1u << (p - seg0);
            p = next_of(nxt, p);
            PROF_COUNT(15, 1);
        }
        x = p;
    }
    uint32_t es = vis ? seg0 + __builtin_ctz(vis) : x;
    uint32_t nE = 0;
    for (int it = 0; it <= kWave; ++it) {
        // lane l - 1's values by DPP wave_shr:1 (a VALU operand, not an LDS permute)
        const uint32_t pes = dpp<kWaveShr1>(0u, es), px = dpp<kWaveShr1>(0u, x);
        nE = lane == 0 ? 0u : (pes >= seg0 ? pes : px);
        bool valid = nE >= seg1 ? (vis == 0 && x == nE) : ((vis >> (nE - seg0)) & 1u) != 0;
        uint64_t bad = __ballot(!valid);
        PROF_COUNT(13, 1);
        if (it == 0) PROF_COUNT(14, __popcll(bad));
        if (bad == 0) break;
        if (lane == __builtin_ctzll(bad)) {   // first inconsistent lane: re-walk from its true entry
            vis = 0;
            uint32_t p = nE;
            while (p < seg1) {
                vis |= 1u << (p - seg0);
                p = next_of(nxt, p);
            }
            x = p;
            es = vis ? seg0 + __builtin_ctz(vis) : x;
        }
    }
    if (nE >= seg1) vis = 0;
    else vis &= ~((1u << (nE - seg0)) - 1u);
    const uint32_t raw = lane_of(x, kWave - 1);   // where the chain leaves the chunk
    tail = raw;
    if (tail > (uint32_t)kLim && tail < kEnd) tail = kStop;   // (fast table: raw positions past the window)
    const uint64_t has = __ballot(vis != 0);
    const int last_lane = 63 - __builtin_clzll(has);
    const uint32_t last_tok = lane_val(seg0 + 31 - __builtin_clz(vis | 1u), (uint32_t)last_lane);
    if (defer && fast_tab && tail == kStop && raw < kEnd && last_tok != 0 && raw - last_tok <= (uint32_t)kLim) {
        if (lane == last_lane) vis &= ~(1u << (last_tok - seg0));
        return Parse{vis, last_tok, last_tok, last_lane, false};
    }
    return Parse{vis, tail, last_tok, last_lane, tail == kStop};
}

// ---------------------------------------------------------------- 4. sequence table
// Sequence-major from a compact token list: every lane writes the positions of its
// segment's tokens at base + j, then lane l of row i takes sequence k = 64 i + l, reads
// its fields, gets its output start from a row scan plus the carry of the rows before,
// and writes its entry once. Two rows per step, their byte reads issued together (three
// LDS round trips per step). Errors in the reference's order: a 32-bit test per row pair,
// and the exact 64-bit checks only from the first flagged pair on.
// `rel`: an exported segment (relative output positions). `redo`: the table is not built --
// a true token's match length field runs past one extension byte, which the fast next-token
// table (fast_tab) took to be one: the chunk is parsed again with the exact table.
struct SeqTable {
    uint32_t nseq;        // sequences in S.t_seq (without the cut one)
    int64_t total;        // their output bytes
    uint32_t first_err;   // sequence << 3 | seq_error of the first failing one (0xFFFFFFFF: none)
    bool redo;
};
template <bool XP>
__device__ __forceinline__ SeqTable seq_table(const Ctx& c, DecShared& S, int lane, uint32_t rem, bool rel,
                                              bool fast_tab, const Parse& P, Prof& prof) {
    PROF(2);
    const uint8_t* s = (const uint8_t*)S.stage;
    const uint32_t seg0 = 16u * lane;
    const uint32_t cnt = __popc(P.vis) - ((P.cut && lane == P.last_lane) ? 1u : 0u);
    const uint32_t incl = wave_incl_scan(cnt, lane);
    const uint32_t base = incl - cnt;
    const uint32_t nseq = lane_of(incl, kWave - 1);
    uint16_t* const tl = (uint16_t*)S.pms;   // (idle until the output phase; kMaxSeq * 2 bytes)
    static_assert(sizeof(uint16_t) * (kMaxSeq + 2 * kWave) <= sizeof(S.pms), "token list fits in the pending starts");
    {
        uint32_t m = P.vis;
        for (uint32_t j = 0; j < cnt; ++j) {
            tl[base + j] = (uint16_t)(seg0 + __builtin_ctz(m));
            m &= m - 1;
        }
    }
    __syncthreads();
    // The 32-bit form of the five checks. With c.O <= c.cap (else every row is checked exactly),
    // c.cap < 2^31, a table's output under 2^26 bytes (at most kMaxSeq sequences of under 2^17
    // bytes each: both lengths are 16-bit fields of the entry) and offsets under 2^16, every sum
    // below stays under 2^32, so the test is exact:
    //   1  out + ll > cap                  <=>  X > capr, X = (out - c.O) + ll, capr = cap - c.O
    //   2  ip + lit + ll > in_len          <=>  lit + ll > rem
    //   3  off == 0, 4 off > out_off + out + ll + dict_len, 5 isolate and off > out + ll
    //                                      <=>  off - 1 >= L45 + X (wrapping for off = 0), with
    //      L45 = c.O + (isolate ? 0 : min(out_off + dict_len, 2^16)): past 2^16 check 4 cannot fail
    // An exported segment (relative positions) has checks 2 and 3 only.
    const bool exact_all = !rel && c.O > (int64_t)c.cap;
    const uint32_t capr = rel || exact_all ? 0xFFFFFFFFu : (uint32_t)(c.cap - (int32_t)c.O);
    const int64_t d4 = c.out_off + c.dict_len;
    const uint32_t L45 = rel || exact_all ? 0x80000000u
                                          : (uint32_t)c.O + (c.isolate ? 0u : (uint32_t)(d4 < 65536 ? d4 : 65536));
    uint32_t carry = 0;   // output bytes of the rows before
    uint32_t first_err = 0xFFFFFFFFu;
    uint32_t flagged = 0xFFFFFFFFu;   // first rows the 32-bit test flags
    constexpr int kRows = 2;
    for (uint32_t i0 = 0; i0 < nseq; i0 += kRows * kWave) {
        uint32_t p[kRows], tok[kRows], b1[kRows];
#pragma unroll
        for (int r = 0; r < kRows; ++r) {
            const uint32_t k = i0 + kWave * r + lane;
            p[r] = k < nseq ? tl[k] : 0u;
        }
#pragma unroll
        for (int r = 0; r < kRows; ++r) {
            tok[r] = s[p[r]];
            b1[r] = s[p[r] + 1];
        }
        uint32_t q[kRows], lit[kRows], ll[kRows], o0[kRows], o1[kRows], mb[kRows];
#pragma unroll
        for (int r = 0; r < kRows; ++r) {
            const uint32_t x1 = (tok[r] >> 4) == 15 ? 1u : 0u;
            ll[r] = x1 ? 15u + b1[r] : tok[r] >> 4;
            lit[r] = p[r] + 1 + x1;
            q[r] = lit[r] + ll[r];
            // offset bytes inside the window (q + 2 <= kLim: a sequence may end on its last byte,
            // as next_token accepts; s[q + 2] is still staged) -- past it only a long literal run
            // (slow below)
            const uint32_t qa = q[r] + 2 <= (uint32_t)kLim ? q[r] : 0u;
            o0[r] = s[qa];
            o1[r] = s[qa + 1];
            mb[r] = s[qa + 2];
        }
        uint32_t off[kRows], ml[kRows];
        bool rerun = false;   // a true token's match length runs on past one byte (fast table)
#pragma unroll
        for (int r = 0; r < kRows; ++r) {
            const bool live = i0 + kWave * r + lane < nseq;
            off[r] = 0;
            ml[r] = 0;
            if (!live) {
                ll[r] = 0;
                continue;
            }
            uint32_t qj = q[r];
            if ((tok[r] >> 4) == 15 && b1[r] == 255) {   // literal length field of 2+ bytes
                uint32_t t = p[r] + 1, bb, llj = 15;
                do { bb = s[t++]; llj += bb; } while (bb == 255);
                ll[r] = llj;
                lit[r] = t;
                qj = t + llj;
                if (qj < rem) { o0[r] = s[qj]; o1[r] = s[qj + 1]; mb[r] = s[qj + 2]; }
            }
            if (qj < rem) {
                off[r] = o0[r] | (o1[r] << 8);
                uint32_t m = tok[r] & 15;
                if (m == 15) {
                    if (mb[r] != 255) {
                        m += mb[r];
                    } else {
                        rerun |= fast_tab;
                        uint32_t t = qj + 2, bb;
                        do { bb = s[t++]; m += bb; } while (bb == 255 && t < (uint32_t)kLim);
                    }
                }
                ml[r] = m + 4;
            }
        }
        if (__ballot(rerun)) return SeqTable{0u, 0, 0xFFFFFFFFu, true};
        bool flag = false;
#pragma unroll
        for (int r = 0; r < kRows; ++r) {
            if (r > 0 && i0 + kWave * r >= nseq) break;
            const uint32_t k = i0 + kWave * r + lane;
            const uint32_t len = ll[r] + ml[r];
            const uint32_t sc = wave_incl_scan(len, lane);
            const uint32_t ro = carry + sc - len;   // output start, relative to c.O
            carry += lane63(sc);
            if (k < nseq) {
                S.t_seq[k] = make_uint4((uint32_t)c.O + ro, lit[r] | (ll[r] << 16), off[r] | (ml[r] << 16), 0u);
                const uint32_t X = ro + ll[r];
                flag |= X > capr || lit[r] + ll[r] > rem || (ml[r] != 0 && off[r] - 1u >= L45 + X);
            }
        }
        if (__ballot(flag) != 0 && flagged > i0) flagged = i0;
    }
    __syncthreads();
    // the exact checks, from the first flagged rows on (absent on valid input); the first
    // failing sequence ends them
    for (uint32_t i0 = exact_all ? 0u : flagged; i0 < nseq && first_err == 0xFFFFFFFFu; i0 += kWave) {
        const uint32_t k = i0 + lane;
        uint32_t e = 0;
        if (k < nseq) {
            const SeqInfo q = seq_info(S, k);
            e = seq_err<XP>(c, rel, c.O + (uint32_t)(q.out - (int32_t)c.O), (int64_t)c.ip + q.lit, q.ll, q.off, q.ml);
        }
        first_err = wave_min(e ? (k << 3) | e : 0xFFFFFFFFu);
    }
    return SeqTable{nseq, (int64_t)carry, first_err, false};
}

// ---------------------------------------------------------------- 5. cut sequence
// The sequence the window could not hold (P.cut), parsed from memory: literals [clit, clit + cll),
// match offset coff and length cml (0: none), the next token at cq (block-relative).
// (Its parse is written out in decompress_block: as a function of its own it moved the export
// kernel's register allocation and cost small text batches 1-6 %, profiles/refactor_phases.)
struct CutSeq {
    int64_t cq = 0, cll = 0, cml = 0, clit = 0;
    uint32_t coff = 0;
};

// ---------------------------------------------------------------- advance
// On to the next chunk: after the table (output up to tab_hi) and the cut sequence, if any.
__device__ __forceinline__ void advance(Ctx& c, int64_t tab_hi, const Parse& P, const CutSeq& cs) {
    c.O = tab_hi;
    if (P.cut) {
        c.O += cs.cll + cs.cml;
        c.ip = (int32_t)(cs.cq < c.in_len ? cs.cq : c.in_len);
    } else if (P.tail >= kEnd) {
        c.ip = c.in_len;
    } else {
        c.ip += (int32_t)P.tail;
    }
}

// ---------------------------------------------------------------- export (XP): a chunk
// Export the chunk's sequences whose tokens lie in [seg_lo, seg_hi); the first one found is
// the segment's entry, the first at or past seg_hi its exit. Then on to the next chunk (or,
// a guess that met an impossible token before its segment, over again one byte past it).
__device__ __forceinline__ void x_export_chunk(Ctx& c, const DecShared& S, XState& x, int lane, const Parse& P,
                                               const SeqTable& T, const CutSeq& cs) {
    const bool cut = P.cut;
    const uint32_t nseq = T.nseq, seg_lo = x.seg_lo, seg_hi = x.seg_hi;
    const int64_t tab_hi = c.O + T.total;
    const uint32_t ipc = (uint32_t)c.ip;
    const uint32_t ntot = nseq + (cut ? 1u : 0u);   // the cut sequence is number nseq
    const uint32_t ecut = cut ? seq_err<true>(c, true, tab_hi, cs.clit, cs.cll, cs.coff, cs.cml) : 0u;
    const uint32_t ferr = T.first_err != 0xFFFFFFFFu ? T.first_err : (ecut ? ((nseq << 3) | ecut) : 0xFFFFFFFFu);
    const uint32_t fk = ferr == 0xFFFFFFFFu ? ntot : (ferr >> 3);
    auto x_tok = [&](uint32_t k) -> uint32_t {   // token position (block-relative)
        if (k >= nseq) return ipc + P.last_tok;
        const SeqInfo q = seq_info(S, k);
        return ipc + (uint32_t)q.lit - 1u - (q.ll >= 15 ? (uint32_t)(q.ll - 15) / 255u + 1u : 0u);
    };
    auto x_out = [&](uint32_t k) -> int64_t { return k >= nseq ? tab_hi : (int64_t)S.t_seq[k].x; };
    uint32_t k0 = ntot, k1 = ntot;
    for (uint32_t r = 0; 64u * r < ntot; ++r) {
        const uint32_t k = 64u * r + lane;
        const uint32_t t = k < ntot ? x_tok(k) : 0xFFFFFFFFu;
        const uint64_t m0 = __ballot(k < ntot && t >= seg_lo), m1 = __ballot(k < ntot && t >= seg_hi);
        if (k0 == ntot && m0) k0 = 64u * r + (uint32_t)__builtin_ctzll(m0);
        if (k1 == ntot && m1) k1 = 64u * r + (uint32_t)__builtin_ctzll(m1);
    }
    bool restart = false;
    if (!x.started && fk < k0) {
        // an error before the segment: a wrong walk, or an earlier segment's error (which
        // that segment's parse reports) -- never this segment's. A guess starts over one
        // byte past the impossible token (text: an offset of 0 read from the wrong bytes
        // failed 22 of a 4 MiB block's 255 guesses, which then waited for re-parses)
        if (x.pass == 0 && x.restart < kSegRestarts) {
            restart = true;
            ++x.restart;
        } else {
            x.fail = x.done = true;
        }
    } else {
        if (!x.started && k0 < ntot) {
            x.started = true;
            x.G = x_tok(k0);
            x.OG = x_out(k0);
        }
        if (x.started) {
            const uint32_t ke = fk < k1 ? fk + 1 : k1;   // with the failing one (checks 1, 4, 5)
            for (uint32_t k = k0 + lane; k < ke; k += kWave) {
                uint4 e;
                if (k < nseq) {
                    const SeqInfo q = seq_info(S, k);
                    e = make_uint4((uint32_t)(x_out(k) - x.OG), ipc + (uint32_t)q.lit, (uint32_t)q.ll,
                                   q.ml ? (uint32_t)q.off : 0u);
                } else {
                    e = make_uint4((uint32_t)(tab_hi - x.OG), (uint32_t)cs.clit, (uint32_t)cs.cll,
                                   cs.cml ? cs.coff : 0u);
                }
                x.xs[x.nx + (k - k0)] = e;
            }
            if (fk < k1) {
                x.err = ((x.nx + (fk - k0)) << 3) | (ferr & 7u);
                x.done = true;
            } else if (k1 < ntot) {
                x.done = true;
                x.X = x_tok(k1);
                x.olen = (uint32_t)(x_out(k1) - x.OG);
            }
            x.nx += ke - k0;
        }
    }
    if (restart) {
        c.ip = (int32_t)(x_tok(fk) + 1u);
        c.O = 0;
    } else if (!x.done) {
        advance(c, tab_hi, P, cs);
        if ((uint32_t)c.ip >= seg_hi && c.ip < c.in_len) {   // the chain leaps the segment's end
            if (!x.started) {
                x.started = true;
                x.G = (uint32_t)c.ip;
                x.OG = c.O;
            }
            x.done = true;
            x.X = (uint32_t)c.ip;
            x.olen = (uint32_t)(c.O - x.OG);
        }
    }
    __syncthreads();
}

// The segment's record, once its exit is found or the block ends.
__device__ __forceinline__ void x_finish(const DecArgs& a, const Ctx& c, XState& x, int lane, uint32_t sg) {
    if (!x.done) {   // the block's end
        if (!x.started) {
            x.G = (uint32_t)c.in_len;
            x.OG = c.O;
        }
        x.X = (uint32_t)c.in_len;
        x.olen = (uint32_t)(c.O - x.OG);
    }
    if (lane == 0) {
        SegRec* const xr = x.xr;
        xr->entry = x.G;
        xr->exit = x.X;
        xr->cnt = x.nx;
        xr->olen = x.olen;
        xr->err = x.err;
        xr->fail = (x.fail || (a.xforce && sg > 0 && (a.xforce == 2 ? x.pass != 1 : x.pass == 0))) ? 1u : 0u;
        if (x.pass == 1)   // the exact re-parse of phase 1: final
            __hip_atomic_store(&xr->fin, (x.err != 0xFFFFFFFFu ? kFinErr : x.X) + 1u, __ATOMIC_RELEASE,
                               __HIP_MEMORY_SCOPE_AGENT);
    }
}

// ---------------------------------------------------------------- 6. output rounds
// Output -> sequence map for remap_src, in the (now idle) next-token table; returns its shift.
__device__ __forceinline__ uint32_t source_map(const Ctx& c, DecShared& S, int lane, uint32_t nseq, int64_t total) {
    // output -> sequence map granule: 32 bytes for long sequences (tiles216: 16 B costs 1.8 %),
    // 16 for short ones (text: 32 B costs 6 %, more sequences per granule to step over)
    uint32_t msh = total >= 32u * nseq ? 5u : 4u;
    while ((total >> msh) >= kLim) ++msh;
    for (uint32_t k = lane; k < nseq; k += kWave) {
        const uint32_t t0 = S.t_seq[k].x - (uint32_t)c.O;
        const uint32_t t1 = (k + 1 < nseq ? S.t_seq[k + 1].x : (uint32_t)(c.O + total)) - (uint32_t)c.O;
        for (uint32_t b = (t0 + (1u << msh) - 1) >> msh; (b << msh) < t1; ++b) S.nxt[b] = (uint16_t)k;
    }
    __syncthreads();
    return msh;
}

// Round 1: all literal runs (from LDS: the chunk's own before the row loop, dealt_literals) and
// every match whose source lies, or maps back to, output finished by earlier chunks. The row
// loop holds match planning, the remap and the listing of remapped literal sources only.
// Returns the pending matches: bit i = that of sequence 64 i + lane.
__device__ __forceinline__ uint32_t round1(const Ctx& c, DecShared& S, int lane, uint32_t nseq, uint32_t msh, Prof& prof) {
    uint32_t pend = 0;    // bit i: the match of sequence 64i+lane is still to be written
    uint32_t ready = 0;   // bit i: ... is written by this lane in this round
    uint32_t rbits = 0;   // bit i: ... reads a remapped source (SeqInfo::rsrc)
    uint32_t nlit_pack = 0;   // byte i (rows < 4): literal prefix of a split match (remap_src 3)
    dealt_literals(c, S, lane, nseq);
    LitDeal D;   // the remapped sources' literal runs
    for (uint32_t i = 0; 64 * i < nseq; ++i) {            // round 1
        const uint32_t k = 64 * i + lane;
        Run M = no_run(), ML = no_run();
        const SeqInfo q = seq_info(S, k < nseq ? k : 0u);   // (its literal run: dealt_literals, above)
        PROF(23);
        if (k < nseq) {
            const int32_t t0 = q.out;
            M = match_run(c, t0 + q.ll, q.off, q.ml);
            if (M.n == 0) {
                M.kind = R_NONE;
            } else if (match_src_end(M) > (int32_t)c.O) {
                // the source is output of this table: map it back through the
                // sequences that wrote it, else wait for a later round
                int32_t rs = M.src, re = match_src_end(M), li = 0, nl = 0;
                const int r = (M.kind == R_HIST && M.period == 0)
                                  ? remap_src(c, S, nseq, msh, rs, re, li, nl, i < 4)
                                  : 0;
                if (r == 3) {   // literal prefix from the stage, the rest from finished output
                    ML = Run{M.y, nl, li, 0, R_LDS};
                    M.y += nl;
                    M.n -= nl;
                    nlit_pack |= (uint32_t)nl << (8 * i);
                }
                if (r == 1 || r == 3) {
                    M.src = rs;
                    if (c.out_off + rs < 16) M.kind = R_BYTES;
                    S.t_seq[k].w = (uint32_t)rs + (r == 3 ? kSplitBase : kMemoBase);
                    rbits |= 1u << i;
                } else if (r == 2) {
                    ML = Run{M.y, M.n, li, 0, R_LDS};
                    M.kind = R_NONE;
                } else {
                    pend |= 1u << i;
                    M.kind = R_NONE;
                }
            }
        }
        const bool longM = M.kind != R_NONE && M.n > kLaneBytes;
        const bool longML = ML.n > kLaneBytes;
        const bool fastM = M.kind == R_HIST && M.period == 0 && M.n >= 16;
        if (M.kind != R_NONE && !longM && fastM) ready |= 1u << i;
        PROF(16);
        {
            const bool dealML = ML.n > 0 && !longML;   // (under 16 bytes too: one piece of its exact width)
            if (const uint64_t bal = __ballot(dealML)) {
                if (D.R + (uint32_t)__popcll(bal) > (uint32_t)kLitRuns) D.flush(c, S, lane);
                D.add(S, lane, dealML, bal, ML.y, ML.src, ML.n);
            }
        }
        PROF(17);
        for (uint64_t lm = __ballot(longML); lm; lm &= lm - 1) wave_run(c, S, lane, shfl_run(ML, __builtin_ctzll(lm)), no_pat());
        if (M.kind != R_NONE && !longM && !fastM) lane_slow_run(c, S, M);
        if (const uint64_t mm0 = __ballot(longM)) {
            D.flush(c, S, lane);   // (pat_round1 is the list's LDS)
            for (uint64_t mm = mm0; mm; mm &= mm - 1) wave_run(c, S, lane, shfl_run(M, __builtin_ctzll(mm)), pat_round1(S));
        }
        PROF(18);
    }
    D.flush(c, S, lane);
    piece_pipe(c, S, ready, rbits, lane, nseq, nlit_pack);
    return pend;
}

// Rounds 2, 3, ...: after the previous round's stores are complete, every pending match
// whose source range meets no pending match.
__device__ __forceinline__ void later_rounds(const Ctx& c, DecShared& S, int lane, uint32_t nseq, uint32_t pend,
                                             Prof& prof) {
    for (; LZ4MI_ABLATE != 6;) {
        uint32_t np = 0;
        for (uint32_t i = 0; 64 * i < nseq; ++i) {
            const bool pk = (pend >> i) & 1u;
            const uint64_t bal = __ballot(pk);
            if (pk) {
                const uint32_t k = 64 * i + lane;
                const uint32_t idx = np + __builtin_amdgcn_mbcnt_hi((uint32_t)(bal >> 32),
                                                                    __builtin_amdgcn_mbcnt_lo((uint32_t)bal, 0u));
                const SeqInfo q = seq_info(S, k);
                const int32_t ms = q.out + q.ll;
                S.pms[idx] = (uint32_t)ms;
                S.pme[idx] = (uint32_t)(q.ml > c.cap - ms ? c.cap : ms + q.ml);   // (ms < cap: match_run)
            }
            np += (uint32_t)__popcll(bal);
        }
        if (np == 0) break;
        PROF_COUNT(11, 1);
        __syncthreads();
        wait_vmem();      // the previous round's stores are complete
        PROF(20);
        uint32_t ready = 0;   // bit i: the match of sequence 64i+lane is written by this lane in this round
        for (uint32_t i = 0; 64 * i < nseq; ++i) {
            if (__ballot((pend >> i) & 1u) == 0) continue;
            Run M = no_run();
            if ((pend >> i) & 1u) {
                const uint32_t k = 64 * i + lane;
                const SeqInfo q = seq_info(S, k);
                M = match_run(c, q.out + q.ll, q.off, q.ml);
                // first pending match ending past the source start: ready if it starts at or past the source end
                const int32_t rs = M.src, re = match_src_end(M);
                uint32_t lo = 0, hi = np;
                while (lo < hi) {
                    const uint32_t mid = (lo + hi) >> 1;
                    if ((int32_t)S.pme[mid] > rs) hi = mid;
                    else lo = mid + 1;
                }
                if (lo >= np || (int32_t)S.pms[lo] >= re) pend &= ~(1u << i);
                else M.kind = R_NONE;
            }
            const bool longM = M.kind != R_NONE && M.n > kLaneBytes;
            const bool fastM = M.kind == R_HIST && M.period == 0 && M.n >= 16;
            if (M.kind != R_NONE && !longM && fastM) ready |= 1u << i;
            if (M.kind != R_NONE && !longM && !fastM) lane_slow_run(c, S, M);
            for (uint64_t mm = __ballot(longM); mm; mm &= mm - 1) wave_run(c, S, lane, shfl_run(M, __builtin_ctzll(mm)), pat_rounds(S));
        }
        piece_pipe(c, S, ready, 0u, lane, nseq, 0u);
        __syncthreads();
    }
}

// The table's sequences, written (T.total bytes from c.O).
__device__ __forceinline__ void output_rounds(const Ctx& c, DecShared& S, int lane, const SeqTable& T, Prof& prof) {
    const uint32_t msh = source_map(c, S, lane, T.nseq, T.total);
    PROF(22);
    const uint32_t pend = round1(c, S, lane, T.nseq, msh, prof);
    PROF(19);
    later_rounds(c, S, lane, T.nseq, pend, prof);
}

// ---------------------------------------------------------------- 7. F1 replay (reference mode)
// Both return the block's status: 0, or -9 where a rewrite reads below the block's start.
// The table's sequences, after their output.
__device__ __forceinline__ int32_t f1_table(const Ctx& c, const DecShared& S, int lane, uint32_t nseq) {
    // candidates first, from the sequence table alone (offset >= 8, length < 8): a chunk
    // without one -- every tiles216 chunk -- neither drains its stores here nor reads
    // them back, so they keep draining beside the next chunk's parse as in spec mode
    bool cand = false;
    for (uint32_t k = lane; k < nseq; k += kWave) {
        const SeqInfo q = seq_info(S, k);
        cand |= q.ml != 0 && q.ml < 8 && q.off >= 8;
    }
    if (__ballot(cand)) {
        wait_vmem();    // this chunk's stores are complete before they are read back
        uint32_t dv = 0;
        for (uint32_t k = lane; k < nseq; k += kWave) {
            const SeqInfo q = seq_info(S, k);
            dv |= f1_changes(c, q.out + q.ll, q.off, q.ml);
        }
        if (__ballot(dv & 2u)) return -9;
        if (__ballot(dv)) f1_fixup(c, S, lane, nseq, false, 0, 0, 0);
    }
    return 0;
}

// The cut sequence's match (starting at ms), after the table's F1 replay (it reads the replayed
// bytes, as the reference's copy does); the tables are idle now: all of LDS can hold a
// periodic pattern. Then (f1check) its own tail rewrite, after its copy as in the reference.
__device__ __forceinline__ int32_t cut_match(const Ctx& c, DecShared& S, int lane, int32_t ms, const CutSeq& cs,
                                             bool f1check) {
    const Run M = match_run(c, ms, (int32_t)cs.coff, (int32_t)cs.cml);
    if (M.n > 0) {
        wait_vmem();    // everything below the match is read back as history
        wave_run(c, S, lane, M, pat_all(S));
    }
    if (f1check && cs.cml != 0 && cs.cml < 8 && cs.coff >= 8) {
        wait_vmem();
        const uint32_t dv = lane == 0 ? f1_changes(c, ms, (int32_t)cs.coff, (int32_t)cs.cml) : 0u;
        if (__ballot(dv & 2u)) return -9;
        if (__ballot(dv)) f1_fixup(c, S, lane, 0, true, (int64_t)ms, (int32_t)cs.coff, (int32_t)cs.cml);
    }
    return 0;
}

// ---------------------------------------------------------------- the block's loop
constexpr bool kOutput = LZ4MI_ABLATE == 0 || LZ4MI_ABLATE >= 4;      // (else timing only: nothing is written)
constexpr bool kParseOnly = LZ4MI_ABLATE == 2 || LZ4MI_ABLATE == 3;   // (timing only: steps 1-3)

// XP: the small-batch export, a wave per segment of the block (x_enter); LK: a linked window.
// CH: the caller names the block (cblk, instead of blockIdx.x and the order / redo lists) and the array it is a
// block of, which begins at out + cbase: Ctx::out_off is the slot's position in that array (the chains of a frame
// batch, lz4mi_decompress_frames_chain_kernel). Returns the status written to status[b] (0 where none is). The
// three batch kernels take none of this: with CH = false the function compiles to what it was without it -- a
// split into a wrapper and a per-block function did not (other register allocation, bench.py 0.7 % slower).
// F1: step 7 known at compile time (the batch kernel: one instantiation per decode mode, so the spec one holds
// neither f1_table nor cut_match's rewrite branch), or DecArgs::f1check (the export and frame-chain kernels).
constexpr int kF1Arg = -1, kF1Off = 0, kF1On = 1;
template <bool XP, bool LK = false, bool CH = false, int F1 = kF1Arg>
__device__ __forceinline__ int32_t decompress_block(const DecArgs& a, uint32_t cblk = 0, uint64_t cbase = 0) {
    __shared__ DecShared S;
    const bool f1check = F1 == kF1Arg ? a.f1check != 0 : F1 == kF1On;
    const int lane = threadIdx.x;
    const uint32_t nseg = XP ? a.xsegs : 1u;   // XP: waves per block (one per segment)
    if (!CH && blockIdx.x >= a.nblocks * nseg) return 0;
    const uint32_t wblk = CH ? cblk : XP ? blockIdx.x / nseg : blockIdx.x;   // (XP: block-major, segments of a block on
    const uint32_t sg = XP ? blockIdx.x - wblk * nseg : 0u;       //  consecutive CUs, every XCD)
    if (LK && uniform(a.xcnt[wblk]) == kNotExported) return 0;     // stored, refused or after a failure: not parsed
    const uint32_t b = CH ? cblk : a.order ? uniform(a.order[wblk]) : wblk;
    if (!CH && !XP && a.redo && !uniform(a.redo[b])) return 0;   // (small batches, reference mode: the blocks to redo)
#if LZ4MI_TIMELINE
    const uint64_t tl_t0 = wall_clock64();
#endif
    // the block's scalars in SGPRs (readfirstlane): as VGPRs the compiler would keep
    // per-lane copies of values derived from them and spill those to scratch
    const uint64_t in_off = uniform64(a.in_off[b]), out_off = uniform64(a.out_off[b]);
    const uint32_t out_cap = uniform(a.out_cap[b]);
    Ctx c;
    c.blk = a.in + in_off;
    const uint32_t word = uniform(a.in_len[b]);
    c.in_len = (int32_t)(a.frame_words ? word & 0x7FFFFFFFu : word);
    c.out_off = CH ? (int64_t)(out_off - cbase) : (int64_t)out_off;
    c.dst = a.out + out_off;
    c.cap = out_cap > 0x7FFFFFFFu ? 0x7FFFFFFF : (int32_t)out_cap;
    c.dict = a.dict;
    c.dict_len = a.dict ? (int32_t)a.dict_len : 0;
    c.isolate = a.isolate;
    c.ip = 0;
    c.O = 0;
    if (a.frame_words && (word & 0x80000000u)) {
        return stored_block(a, c, b, out_cap, lane);
    }
    XState x;   // (XP)
    if constexpr (XP) {
        if (!x_enter<LK>(a, c, x, lane, wblk, sg, nseg, out_cap)) return 0;
    }
    const bool xp = XP && x.on;   // parsed for export; else decoded here
#if LZ4MI_LL_ADAPT
    const bool lat_bound = (uint64_t)c.in_len * 2 < (uint64_t)out_cap;   // ratio > 2: a chain of short copies
    unsigned int* lat = &g_lat_active[32 * xcc_id()];
    if (lat_bound && lane == 0) atomicAdd(lat, 1u);
#endif
    Prefetch pf;
    Prof prof;
#if LZ4MI_PROFILE
    prof = Prof{{0}, (uint64_t)wall_clock64()};
#endif
    int32_t status = 0;
    while (c.ip < c.in_len) {
        if (XP && x.done) break;   // (XP: the segment's exit found)
        PROF_COUNT(10, 1);
        stage_chunk(c, S, pf, lane);                                        // 1
        const uint32_t rem = (uint32_t)(c.in_len - c.ip);
        // away from the block's end the fast next-token table; where it does not hold
        // (T.redo) the chunk once more, with the exact one
        Parse P;
        SeqTable T;
        for (bool fast_tab = rem > kFastRem;; fast_tab = false) {
            P = parse_chunk(S, lane, rem, fast_tab, !XP, prof);             // 2, 3
            // the next chunk's bytes: loaded while this chunk's table is built
            if (LZ4MI_ABLATE != 3 && !P.cut && P.tail < kEnd && (int64_t)c.ip + P.tail < c.in_len)
                prefetch(c, pf, (int64_t)c.ip + P.tail, lane);
            if (kParseOnly) break;
            T = seq_table<XP>(c, S, lane, rem, xp, fast_tab, P, prof);      // 4
            if (!T.redo) break;
            wait_vmem();          // (no load in flight into the parse: its registers are free)
            settle(pf);
            __syncthreads();
        }
        if (kParseOnly) {
            c.ip = P.tail == kEnd ? c.in_len : c.ip + (P.cut ? kChunk : (int32_t)P.tail);
            __syncthreads();
            continue;
        }
        if (T.first_err != 0xFFFFFFFFu && !xp) { status = err_status(T.first_err & 7); break; }
        PROF(3);
        CutSeq cs;                                                          // 5
        {
            const uint8_t* s = (const uint8_t*)S.stage;
            int64_t cq = 0, cll = 0, cml = 0, clit = 0;
            uint32_t coff = 0;
            if (P.cut) {
                // token and literal length from the staged bytes while they last
                constexpr uint32_t kStaged = 16 * (kStageWords / 4);
                uint32_t r = P.last_tok;
                const uint32_t tok = s[r++];
                cll = tok >> 4;
                bool more = cll == 15;
                while (more && r < kStaged) {
                    const uint32_t b = s[r++];
                    cll += b;
                    more = b == 255;
                }
                int64_t q = (int64_t)c.ip + r;
                if (more) cll += wave_varint(c, lane, q);
                clit = q;
                q += cll;
                if (q < c.in_len) {
                    // offset and match length: one 16-byte load covers them unless the length runs on
                    uint32_t w[4];
                    if (q + 16 <= c.in_len) {
                        __builtin_memcpy(w, c.blk + q, 16);
                    } else {
                        const uint4 t = load16_tail(c.blk, q, c.in_len);
                        w[0] = t.x;
                        w[1] = t.y;
                        w[2] = t.z;
                        w[3] = t.w;
                    }
                    coff = w[0] & 0xFFFFu;
                    q += 2;
                    cml = tok & 15;
                    if (cml == 15) {
                        bool run = true;
                        for (int t = 2; t < 16 && run; ++t) {
                            const uint32_t wd = t < 4 ? w[0] : t < 8 ? w[1] : t < 12 ? w[2] : w[3];
                            const uint32_t b = (wd >> (8 * (t & 3))) & 255u;
                            cml += b;
                            ++q;
                            run = b == 255;
                        }
                        if (run) cml += wave_varint(c, lane, q);
                    }
                    cml += 4;
                }
                cq = q;
            }
            cs = CutSeq{cq, cll, cml, clit, coff};
        }
        if constexpr (XP) {
            if (xp) {
                x_export_chunk(c, S, x, lane, P, T, cs);
                continue;
            }
        }
        const int64_t tab_hi = c.O + T.total;
        // after a cut sequence, the next chunk's bytes: their loads go out before this chunk's stores
        if (P.cut && cs.cq < c.in_len) prefetch(c, pf, cs.cq, lane);
        if (kOutput) {                                                      // 6
            PROF(4);
            __builtin_amdgcn_s_setprio(3);
            // The previous chunk's stores (read back as history below) and the next
            // chunk's loads are complete: the stores had the whole parse to drain.
            wait_vmem();
            settle(pf);
            PROF(21);
            output_rounds(c, S, lane, T, prof);
            PROF(6);
        }
        if (P.cut) {   // its checks, then its literal run; its match after the table's F1 replay
            if (kOutput) PROF_COUNT(12, 1);
            const uint32_t e = seq_error(c, tab_hi, cs.clit, cs.cll, cs.coff, cs.cml);
            if (e) { status = err_status(e); break; }
            if (kOutput)
                wave_run(c, S, lane, Run{(int32_t)tab_hi, (int32_t)cs.cll, (int32_t)cs.clit, 0, cs.cll ? (uint32_t)R_COMP : (uint32_t)R_NONE}, no_pat());
        }
        PROF(7);
        if (f1check) {                                                      // 7
            status = f1_table(c, S, lane, T.nseq);
            if (status) break;
        }
        if (kOutput && P.cut) {
            status = cut_match(c, S, lane, (int32_t)(tab_hi + cs.cll), cs, f1check);
            if (status) break;
        }
        advance(c, tab_hi, P, cs);
        __syncthreads();
        PROF(8);
    }
    if constexpr (XP) {
        if (xp) {
            x_finish(a, c, x, lane, sg);
#if LZ4MI_LL_ADAPT
            if (lat_bound && lane == 0) atomicSub(lat, 1u);
#endif
            return 0;   // status and length: lz4mi_xcheck_kernel
        }
    }
#if LZ4MI_PROFILE
    if (lane == 0)
        for (int i = 0; i < 24; ++i) atomicAdd(&g_prof[i], (unsigned long long)prof.acc[i]);
#endif
    if (lane == 0) {
        a.status[b] = status;
        a.out_len[b] = status ? 0u : (uint32_t)c.O;
        if (XP) a.xcnt[b] = kNotExported;   // (XP: a block past the export limits)
    }
#if LZ4MI_LL_ADAPT
    if (lat_bound && lane == 0) atomicSub(lat, 1u);
#endif
#if LZ4MI_TIMELINE
    wait_vmem();
    const uint64_t tl_t1 = wall_clock64();
    uint32_t hw, xcc;
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hw));
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
    if (lane == 0 && b < kTlMax) {
        g_tl[2 * b] = tl_t0;
        g_tl[2 * b + 1] = tl_t1;
        g_tl_id[2 * b] = hw;
        g_tl_id[2 * b + 1] = xcc;
    }
#endif
    return status;
}

// the batch kernel, once per decode mode (DecArgs::f1check is not read): LZ4 spec ...
__global__ __launch_bounds__(64, 4) void lz4mi_decompress_kernel(DecArgs a) {
    (void)decompress_block<false, false, false, kF1Off>(a);
}
// ... and reference mode (LZ4MI_JS_EXACT; the redo launch of a small batch)
__global__ __launch_bounds__(64, 4) void lz4mi_decompress_ref_kernel(DecArgs a) {
    (void)decompress_block<false, false, false, kF1On>(a);
}
// small batches: a wave per segment of each block, sequences exported (lz4mi_expand.hip)
__global__ __launch_bounds__(64, 4) void lz4mi_decompress_x_kernel(DecArgs a) { (void)decompress_block<true>(a); }
// a linked window: every parsed block exported (no one-wave shortcuts)
__global__ __launch_bounds__(64, 4) void lz4mi_decompress_xl_kernel(DecArgs a) { (void)decompress_block<true, true>(a); }

// After phase 0 and after phase 2 of an exported small batch, per block: the segments in order
// from segment 0 (whose entry is the block's first token): each whose speculative entry equals
// the previous one's exit is final (fin), and one the chain passes over is empty; xfirst[b] = the
// first segment that is neither (xsegs: none), where phase 1 starts; and every later segment's
// re-parse entry for phase 2 (`from`).
__global__ __launch_bounds__(64) void lz4mi_xverify_kernel(DecArgs a) {
    static_assert(kSegMax == 4 * 64, "four records per lane");
    const uint32_t b = blockIdx.x, lane = threadIdx.x;
    if (a.xcnt[b] == kNotExported) return;
    const uint32_t nseg = a.xsegs, in_len = a.in_len[b];
    const SegGeom G = seg_geom(in_len);
    SegRec* R = a.xrec + (size_t)b * nseg;
    // the records, four per lane (segment 64 q + lane), in one round trip; then the walk in registers
    uint32_t entry[4], exit[4], err[4], fail[4], hi_l[4], my_fin[4], kind[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const uint32_t sg = 64u * q + lane;
        const bool in = sg < G.S;
        entry[q] = in ? R[sg].entry : 0u;
        exit[q] = in ? R[sg].exit : 0u;
        err[q] = in ? R[sg].err : 0xFFFFFFFFu;
        fail[q] = in ? R[sg].fail : 0u;
        hi_l[q] = sg + 1 >= G.S ? in_len : min(in_len, sg * G.L + G.L);
        my_fin[q] = 0;
        kind[q] = 0;                   // 0 as parsed, 1 empty (after an error / passed over)
    }
    // the previous segment's exit and error, per lane
    uint32_t pex[4], per[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        pex[q] = __shfl_up(exit[q], 1);
        per[q] = __shfl_up(err[q], 1);
        if (lane == 0) {
            pex[q] = q ? __builtin_amdgcn_readlane(exit[q > 0 ? q - 1 : 0], 63) : 0u;
            per[q] = q ? __builtin_amdgcn_readlane(err[q > 0 ? q - 1 : 0], 63) : 0xFFFFFFFFu;
        }
    }
    // the usual case at once: segment 0, and every one after it whose guess the previous one's
    // exit confirms (no error before it, no segment passed over) -- final up to s0, the first
    // that is not (the walk below, one segment at a time, goes on from there)
    uint32_t s0 = G.S;
#pragma unroll
    for (int q = 3; q >= 0; --q) {
        const uint32_t sg = 64u * q + lane;
        const bool ok = sg < G.S && (sg == 0 || (!fail[q] && entry[q] == pex[q] && per[q] == 0xFFFFFFFFu &&
                                                 pex[q] < hi_l[q]));
        const uint64_t bad = __ballot(sg < G.S && !ok);
        if (bad) s0 = 64u * q + (uint32_t)__builtin_ctzll(bad);
    }
#pragma unroll
    for (int q = 0; q < 4; ++q)
        if (64u * q + lane < s0) my_fin[q] = err[q] != 0xFFFFFFFFu ? kFinErr : exit[q];
    uint32_t first = G.S, prev = 0;    // prev: the previous segment's final exit (kFinErr: an error)
    if (s0 > 0 && s0 < G.S) {
        const uint32_t t = s0 - 1;
        uint32_t v = 0;
#pragma unroll
        for (int q = 0; q < 4; ++q)
            if ((t >> 6) == (uint32_t)q) v = __builtin_amdgcn_readlane(my_fin[q], t & 63);
        prev = v;
    }
    bool stop = s0 >= G.S;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        if (stop || 64u * q + 63 < s0) continue;
        for (uint32_t l = 64u * q < s0 ? s0 - 64u * q : 0u; l < 64 && !stop; ++l) {
            const uint32_t sg = 64u * q + l;
            if (sg >= G.S) {
                stop = true;
                break;
            }
            const uint32_t hi = __builtin_amdgcn_readlane(hi_l[q], l);
            const uint32_t en = __builtin_amdgcn_readlane(entry[q], l), ex = __builtin_amdgcn_readlane(exit[q], l);
            const uint32_t er = __builtin_amdgcn_readlane(err[q], l), fl = __builtin_amdgcn_readlane(fail[q], l);
            uint32_t fin, k = 0;
            if (sg > 0 && prev == kFinErr) {
                fin = kFinErr;
                k = 1;
            } else if (sg > 0 && prev >= hi) {
                fin = prev;
                k = 1;
            } else if (sg == 0 || (!fl && en == prev)) {
                fin = er != 0xFFFFFFFFu ? kFinErr : ex;
            } else {
                first = sg;
                stop = true;
                break;
            }
            if (lane == l) {
                my_fin[q] = fin;
                kind[q] = k;
            }
            prev = fin;
        }
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const uint32_t sg = 64u * q + lane;
        if (sg < first) {
            if (kind[q]) {   // nothing here: after the block's first error, or the chain passes over it
                if (my_fin[q] != kFinErr) R[sg].entry = R[sg].exit = my_fin[q];
                R[sg].cnt = 0;
                R[sg].olen = 0;
                R[sg].err = 0xFFFFFFFFu;
            }
            R[sg].fin = my_fin[q] + 1u;
        }
    }
    if (lane == 0) a.xfirst_w[b] = first;
    // the re-parse of phase 2: from the previous segment's exit where a segment at or past the
    // first unchecked one disagrees with it (and that one met no error, its guess did not fail,
    // and it does not pass over this one)
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const uint32_t sg = 64u * q + lane;
        const bool redo = sg < G.S && sg >= first && sg > 0 && (fail[q] || entry[q] != pex[q]) &&
                          per[q] == 0xFFFFFFFFu && pex[q] >= sg * G.L && pex[q] < hi_l[q];   // (a failed guess: exit 0)
        if (sg < G.S) R[sg].from = redo ? pex[q] : kNoBase;
    }
}

// Dispatch order of a batch (LZ4MI_ORDER). Every block is one wave and a batch of up to
// 16 blocks per CU is resident at once, so a block's decode time is its chain latency under
// the contention of the waves beside it; and workgroups land on CUs by index (round-robin
// over the XCDs and their CUs: w, w + 256, ... share a CU, observed, used for speed only), in
// age order within a SIMD, whose oldest wave wins VALU arbitration. Measured per block
// (tools/timeline.py): tiles216 blocks in the youngest wave slot take 7 % longer than in the
// oldest, and blocks with more compressed bytes longer still, so the launch ends with the
// young heavy blocks; in the 50/50 random/tiles216 mix, CUs that drew more tiles216 blocks
// finish last. The order: blocks with a compression ratio above 2 (latency-bound chains of
// short matches) first, most compressed bytes first, then the rest in index order -- the
// heavy blocks get the oldest slots and every CU the same share of chains. A stable key
// sort (LDS bitonic) in one workgroup; batches of more than kOrderMax blocks keep their order.
constexpr uint32_t kOrderMax = 8192;
__global__ __launch_bounds__(1024) void lz4mi_block_order_kernel(const uint32_t* in_len, const uint32_t* out_cap,
                                                                 uint32_t n, uint32_t* order) {
    __shared__ uint64_t key[kOrderMax];
    const uint32_t t = threadIdx.x;
    uint32_t m = 2;
    while (m < n) m <<= 1;
    for (uint32_t i = t; i < m; i += 1024) {
        uint64_t k = ~0ull;
        if (i < n) {
            const uint32_t il = in_len[i], oc = out_cap[i];   // (a stored frame block: bit 31, not latency-bound)
            const bool lat = (uint64_t)il * 2 < (uint64_t)oc;
            const uint32_t work = LZ4MI_ORDER == 2 ? 0u : (il > 0x7FFFFFFFu ? 0x7FFFFFFFu : il);   // 2: classes only
            const uint32_t hi = lat ? 0x7FFFFFFFu - work : 0x80000000u;
            k = ((uint64_t)hi << 32) | i;
        }
        key[i] = k;
    }
    __syncthreads();
    for (uint32_t size = 2; size <= m; size <<= 1) {
        for (uint32_t stride = size >> 1; stride > 0; stride >>= 1) {
            for (uint32_t i = t; i < (m >> 1); i += 1024) {
                const uint32_t lo = 2 * i - (i & (stride - 1)), hi = lo + stride;
                const bool asc = (lo & size) == 0;
                const uint64_t x = key[lo], y = key[hi];
                if ((x > y) == asc) {
                    key[lo] = y;
                    key[hi] = x;
                }
            }
            __syncthreads();
        }
    }
    for (uint32_t i = t; i < n; i += 1024) order[i] = (uint32_t)key[i];
}

// (Defined behind every other kernel of the file: theirs stay where they were in the code object.)
// The decode twin of lz4mi_compress_chains_kernel (LZ4MI_FRAMES_CHAINS, lz4mi_frames.hip): one wave per frame of a
// frame batch, behind the place pass and the isolated batch launch. A chain frame (FLG without 0x20, more than
// one block: the place pass gave the isolated launch word 0 for its blocks) is decoded from block 0; any other
// frame from its first block whose isolated status is LZ4MI_ERR_CROSS_BLOCK, if it has one. From there on, in
// block order, every block is decoded as a lone block (isolate 0) of an array that begins at the frame's slot:
// Ctx::out_off is the slot-relative position, so nothing below the frame's first byte is read or written. The
// block before is history once its stores are complete (wait_vmem), as a chunk's predecessor is. After the
// first failing block the later ones get LZ4MI_ERR_CROSS_BLOCK and out_len 0 and are not written
// (LZ4MI_LINKED's rule, per frame). `a`: the lists with the real size words, isolate 0, no dictionary.
__global__ __launch_bounds__(64, 4) void lz4mi_decompress_frames_chain_kernel(DecArgs a, const int64_t* finfo,
                                                                              const uint64_t* frame_out_off,
                                                                              uint32_t nframes) {
    const int lane = threadIdx.x;
    const uint32_t f = blockIdx.x;
    if (f >= nframes) return;
    const int64_t* fi = finfo + 8ull * f;
    if (uniform64((uint64_t)fi[0]) || uniform64((uint64_t)fi[7])) return;   // in error or declined
    const uint64_t first = uniform64((uint64_t)fi[4]), n = uniform64((uint64_t)fi[6]);
    if (first > a.nblocks || n > a.nblocks - first) return;                 // its blocks are outside the lists
    const uint64_t base = uniform64(frame_out_off[f]);
    uint64_t k = 0;
    if ((uniform64((uint64_t)fi[1]) & 0x20) || n < 2) {   // not a chain frame: was a block left to the chain?
        uint64_t hit = 0;
        for (; k < n && !hit; k += kWave) {
            const uint64_t q = k + lane;
            hit = __ballot(q < n && a.status[first + q] == LZ4MI_ERR_CROSS_BLOCK);
        }
        if (!hit) return;
        k = k - kWave + (uint64_t)__builtin_ctzll(hit);
    }
    bool failed = false;
    for (; k < n; ++k) {
        const uint32_t b = (uint32_t)(first + k);
        if (failed) {
            if (lane == 0) {
                a.status[b] = LZ4MI_ERR_CROSS_BLOCK;
                a.out_len[b] = 0;
            }
            continue;
        }
        failed = uniform((uint32_t)decompress_block<false, false, true>(a, b, base)) != 0;
        // the block's bytes are the next one's history, and DecShared is free again
        wait_vmem();
        __syncthreads();
    }
}

}  // namespace lz4mi

#if LZ4MI_PROFILE
// Per-phase wall-clock ticks (100 MHz) summed over all waves since the last call; resets.
extern "C" int lz4mi_debug_prof(unsigned long long* out) {
    if (hipMemcpyFromSymbol(out, HIP_SYMBOL(lz4mi::g_prof), sizeof(unsigned long long) * 24) != hipSuccess) return -1;
    unsigned long long z[24] = {0};
    return hipMemcpyToSymbol(HIP_SYMBOL(lz4mi::g_prof), z, sizeof z) == hipSuccess ? 0 : -1;
}
#endif

#if LZ4MI_TIMELINE
// The last launch's per-block timeline (n <= kTlMax blocks): t[2b] start, t[2b+1] end, id[2b] HW_ID, id[2b+1] XCC_ID.
extern "C" int lz4mi_debug_timeline(unsigned long long* t, unsigned int* id, unsigned int n) {
    if (n > lz4mi::kTlMax) n = lz4mi::kTlMax;
    if (hipMemcpyFromSymbol(t, HIP_SYMBOL(lz4mi::g_tl), sizeof(unsigned long long) * 2 * n) != hipSuccess) return -1;
    return hipMemcpyFromSymbol(id, HIP_SYMBOL(lz4mi::g_tl_id), sizeof(unsigned int) * 2 * n) == hipSuccess ? 0 : -1;
}
#endif

using lz4mi::Batch;
using lz4mi::DecArgs;
using lz4mi::XLayout;

// The kernels' arguments for the blocks of `b` (the export fields: parse_exported)
static DecArgs dec_args(const Batch& b, int isolate, int f1check) {
    return DecArgs{b.in, b.in_off, b.in_len, b.out, b.out_off, b.out_cap, b.dict, b.dict_len, b.out_len, b.status,
                   b.nblocks, isolate, f1check};
}

extern "C" hipError_t lz4mi_launch_decompress(const Batch& b, int mode, int isolate, uint32_t* order,
                                              hipStream_t stream) {
    // mode 0: LZ4 spec; 1: reference-exact serial kernel; 2: spec kernel with the in-chunk
    // reference-exact fix-up of every chunk a double-copy-tail rewrite changes (f1_fixup).
    // order: nblocks words of scratch for the dispatch order (nullptr: index order)
    // mode bit 2 (4): in_len holds frame size words (LZ4MI_FRAME_WORDS)
    // isolate: the blocks may not read below their own start (a batch; a lone block of a frame batch)
    const int fw = (mode & 4) ? 1 : 0;
    mode &= 3;
    const uint32_t nblocks = b.nblocks;
    DecArgs a = dec_args(b, isolate, mode == 2 ? 1 : 0);
    a.frame_words = fw;
    if (nblocks == 0) return hipSuccess;
    if (mode == 1) return lz4mi_launch_decompress_serial(a, stream);
    if (LZ4MI_ORDER && order && nblocks > 1 && nblocks <= lz4mi::kOrderMax) {
        hipLaunchKernelGGL(lz4mi::lz4mi_block_order_kernel, dim3(1), dim3(1024), 0, stream, b.in_len, b.out_cap,
                           nblocks, order);
        a.order = order;
    }
    hipLaunchKernelGGL(mode == 2 ? lz4mi::lz4mi_decompress_ref_kernel : lz4mi::lz4mi_decompress_kernel, dim3(nblocks),
                       dim3(64), 0, stream, a);
    return hipGetLastError();
}

// The chains of a frame batch (lz4mi_decompress_frames_chain_kernel): b.in_len holds the frames' real size
// words, b.status / b.out_len what the isolated launch left. mode: 0 or 2, as above.
extern "C" hipError_t lz4mi_launch_decompress_frames_chain(const Batch& b, int mode, const int64_t* finfo,
                                                           const uint64_t* frame_out_off, uint32_t nframes,
                                                           hipStream_t stream) {
    if (nframes == 0 || b.nblocks == 0) return hipSuccess;
    DecArgs a = dec_args(b, 0, mode == 2 ? 1 : 0);
    a.dict = nullptr;
    a.dict_len = 0;
    a.frame_words = 1;
    hipLaunchKernelGGL(lz4mi::lz4mi_decompress_frames_chain_kernel, dim3(nframes), dim3(64), 0, stream, a, finfo,
                       frame_out_off, nframes);
    return hipGetLastError();
}

// A small batch in LZ4 spec or reference mode (lz4mi_expand.hip): each block within the export
// limits (x_in_max compressed, x_out_max output bytes, ratio < 32) is parsed by up to kSegMax
// waves, one per ~kSegTarget bytes of its compressed block (seg_geom), which export its
// sequences instead of writing them; the whole GPU then computes the output by pointer jumping.
// Other blocks are decoded by the same launch as usual. `xs`: scratch of
// lz4mi_small_scratch_bytes, laid out by x_layout (lz4mi_launch.h).
using lz4mi::kSegMax;
extern "C" size_t lz4mi_small_scratch_bytes(uint32_t nblocks, uint32_t x_in_max, uint32_t x_out_max) {
    return lz4mi::x_layout(nblocks, x_in_max, x_out_max, false).total;
}
extern "C" size_t lz4mi_linked_scratch_bytes(uint32_t nblocks, uint32_t x_in_max, uint32_t x_out_max) {
    return lz4mi::x_layout(nblocks, x_in_max, x_out_max, true).total;
}

// The parse of an exported pass with `kernel` (lz4mi_decompress_x_kernel, or ..._xl_kernel for a
// linked window); `a`: the blocks, the export fields are set here from the layout. The caller has
// zeroed xcnt, xfirst and xrec (zero_parse_meta).
// phase 0: every segment speculatively; the check; phase 1: the segments from the first
// wrong entry on (an empty launch when there is none). A phase-1 wave waits only for its
// predecessor, whose workgroup index is lower (dispatched first): the wait always ends.
static hipError_t zero_parse_meta(const XLayout& L, void* xs, hipStream_t stream) {   // exported; records not final
    return hipMemsetAsync(L.xcnt.in<uint8_t>(xs), 0, L.ptr.off - L.xcnt.off, stream);
}
static hipError_t parse_exported(DecArgs a, const XLayout& L, void* xs, int force_reparse, void (*kernel)(DecArgs),
                                 hipStream_t stream) {
    a.xseq = L.xseq.in<uint4>(xs);
    a.xcnt = L.xcnt.in<uint32_t>(xs);
    a.xrec = L.xrec.in<lz4mi::SegRec>(xs);
    a.xseq_stride = L.stride;
    a.xsegs = kSegMax;
    a.x_in_max = L.x_in_max;
    a.x_out_max = L.x_out_max;
    a.xfirst = L.xfirst.in<uint32_t>(xs);
    a.xfirst_w = L.xfirst.in<uint32_t>(xs);
    a.xforce = force_reparse;
    const dim3 grid(a.nblocks * kSegMax);
    hipLaunchKernelGGL(kernel, grid, dim3(64), 0, stream, a);
    hipLaunchKernelGGL(lz4mi::lz4mi_xverify_kernel, dim3(a.nblocks), dim3(64), 0, stream, a);
    // phase 2: the segments whose guesses disagree, re-parsed at once, then the check again;
    // phase 1 chains what is left (a second phase-2 pass: ~11 us of empty launches per call
    // once the guesses restart past impossible tokens)
    a.xphase = 2;
    hipLaunchKernelGGL(kernel, grid, dim3(64), 0, stream, a);
    hipLaunchKernelGGL(lz4mi::lz4mi_xverify_kernel, dim3(a.nblocks), dim3(64), 0, stream, a);
    a.xphase = 1;
    hipLaunchKernelGGL(kernel, grid, dim3(64), 0, stream, a);
    return hipGetLastError();
}

extern "C" hipError_t lz4mi_launch_decompress_small(const Batch& b, uint32_t x_in_max, uint32_t x_out_max, void* xs,
                                                    int force_reparse, int f1, hipStream_t stream) {
    const uint32_t nblocks = b.nblocks;
    if (nblocks == 0) return hipSuccess;
    const XLayout L = lz4mi::x_layout(nblocks, x_in_max, x_out_max, false);
    hipError_t e = zero_parse_meta(L, xs, stream);
    if (e != hipSuccess) return e;
    // (f1check: a block past the export limits is decoded by its segment-0 wave in the caller's mode)
    DecArgs a = dec_args(b, nblocks > 1 ? 1 : 0, f1);
    // from 64 blocks on, nearly incompressible blocks (compressed >= 15/16 of the output: random data) go to one
    // wave each too: 4 MiB of literal pointers cost more than a wave's copy once there are many such blocks
    // (random 64 / 192 blocks 1.76 / 4.79 -> 0.92 / 1.19 ms, the 50/50 mix 192 blocks 6.16 -> 4.83; below 64 a
    // mix loses: the paced one-wave copies become the critical path -- 32 blocks 1.43 -> 1.62; round 6, profiles/r06fl)
    a.x_flat1 = nblocks >= 64 ? 1 : 0;
    e = parse_exported(a, L, xs, force_reparse, lz4mi::lz4mi_decompress_x_kernel, stream);
    if (e != hipSuccess) return e;
    e = lz4mi_launch_expand(b, L, xs, false, f1, 0, stream);
    if (e != hipSuccess || !f1) return e;
    // reference mode (LZ4MI_JS_EXACT): the double-copy-tail rewrites were applied to the pointers
    // (lz4mi_xf1ptr_kernel); a block with a rewrite reading before the block is decoded again by the
    // batch kernel (LZ4MI_ERR_CROSS_BLOCK when batched); the launch is empty when there is none
    DecArgs r = dec_args(b, nblocks > 1 ? 1 : 0, 1);
    r.redo = L.redo.in<uint32_t>(xs);
    hipLaunchKernelGGL(lz4mi::lz4mi_decompress_ref_kernel, dim3(nblocks), dim3(64), 0, stream, r);
    return hipGetLastError();
}

// A linked window (LZ4MI_LINKED): the small path with every block exported and the pointers
// resolved across the window's blocks (lz4mi_expand.hip, "linked mode"). `xs`: scratch of
// lz4mi_linked_scratch_bytes; its first 256 bytes hold the call's state (zeroed by the caller
// before the first window: a failure in one window fails the blocks of the later ones).
// has_prev: the arrays hold an earlier block of the same call before this window's first.
// f1: the reference decoder's bytes (LZ4MI_LINKED_EXACT: the rewrites in pointer form, across blocks).
extern "C" hipError_t lz4mi_launch_decompress_linked(const Batch& b, uint32_t x_in_max, uint32_t x_out_max, void* xs,
                                                     int force_reparse, int frame_words, int has_prev, int f1,
                                                     hipStream_t stream) {
    if (b.nblocks == 0) return hipSuccess;
    const XLayout L = lz4mi::x_layout(b.nblocks, x_in_max, x_out_max, true);
    hipError_t e = zero_parse_meta(L, xs, stream);
    if (e == hipSuccess) e = lz4mi_launch_linked_prep(b, L, xs, frame_words, has_prev, stream);
    if (e != hipSuccess) return e;
    // the parse reads the lengths the prep wrote (no stored bit; a block that is not parsed is skipped)
    DecArgs a = dec_args(b, 0, 0);
    a.in_len = L.head.in<uint32_t>(xs) + 8;
    e = parse_exported(a, L, xs, force_reparse, lz4mi::lz4mi_decompress_xl_kernel, stream);
    if (e != hipSuccess) return e;
    return lz4mi_launch_expand(b, L, xs, true, f1, frame_words, stream);
}
