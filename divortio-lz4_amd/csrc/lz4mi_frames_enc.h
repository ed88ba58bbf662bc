// lz4mi_frames_enc.h — the per-frame steps of the frame batch encoder (lz4mi_frames_plan,
// lz4mi_frames_compress; include/lz4mi.h), written once for the device passes (lz4mi_frames_enc.hip, one lane
// per frame) and for the host twins (lz4mi_host.cpp, the calling thread): the block count and the bound, the
// listing of a frame's blocks, the checks before the encode, the record walk that gives a frame's length, and
// the header, record positions and EndMark of bufferCompress.js:144-252. finfo[f] is the eight values the
// header documents.
#pragma once
#include <stdint.h>

#include "../../include/lz4mi.h"
#include "lz4mi_frames.h"   // LZ4MI_HD, frames::block_bytes

namespace lz4mi {
namespace frames_enc {

enum { kZero = 0, kHead = 1, kSize = 2, kLen = 3, kFirst = 4, kPos = 5, kCount = 6, kDecline = 7 };

constexpr uint64_t kNone = ~0ull;   // a record or checksum position of a block / frame that is not written
constexpr uint64_t kDump = 16;      // work[0 .. kDump): where the encoder's waves of blocks that are not encoded write
constexpr uint32_t kSlice = 4096;   // blocks per encoder launch: 64 KiB of table scratch each
// the flags of both calls besides LZ4MI_DEVICE_PTRS
constexpr uint32_t kFlags = LZ4MI_FRAMES_CONTENT_CHECKSUM | LZ4MI_FRAMES_NO_CONTENT_SIZE | LZ4MI_BLOCK_CHECKSUM |
                            LZ4MI_FRAMES_DEPENDENT | LZ4MI_FRAMES_PACKED | LZ4MI_FRAMES_CHAINS;
// a flag neither call knows, or chains under an independent FLG (a broken frame): LZ4MI_ERR_ARG
inline bool bad_flags(uint32_t flags) {
    return (flags & ~kFlags) || ((flags & LZ4MI_FRAMES_CHAINS) && !(flags & LZ4MI_FRAMES_DEPENDENT));
}

// what lz4mi_frames_compress and its host twin refuse as LZ4MI_ERR_ARG before anything is looked at
inline bool bad_compress_args(const void* in, const void* blk_in_off, const void* blk_len, const void* blk_frame,
                              const void* blk_work_off, uint32_t nblocks, const void* finfo, uint32_t nframes,
                              const void* work, uint64_t work_bytes, const void* out, const void* frame_out_off,
                              const void* frame_out_cap, uint32_t flags) {
    if (nframes && (!finfo || !out)) return true;
    if (nframes && !(flags & LZ4MI_FRAMES_PACKED) && (!frame_out_off || !frame_out_cap)) return true;
    return nblocks && (!in || !blk_in_off || !blk_len || !blk_frame || !blk_work_off || !work || work_bytes < kDump);
}

// getBlockId (bufferCompress.js:77-82); its inverse is frames::block_bytes
LZ4MI_HD uint32_t block_id(uint32_t bytes) {
    return (!bytes || bytes <= 65536u) ? 4 : bytes <= 262144u ? 5 : bytes <= 1048576u ? 6 : 7;
}
using frames::block_bytes;
LZ4MI_HD uint32_t block_max(const int64_t* fi) { return block_bytes((uint32_t)(fi[kHead] >> 12) & 7); }
// (bmax is one of the four block sizes, a power of two: no 64-bit division in the lane-per-frame passes)
LZ4MI_HD uint64_t block_count(uint64_t n, uint32_t bmax) {
    return (n >> (31 - __builtin_clz(bmax))) + ((n & (bmax - 1)) ? 1 : 0);
}
LZ4MI_HD uint64_t frame_bound(uint64_t n, uint32_t bmax) { return 23u + n + 8u * block_count(n, bmax); }
// FLG (:150-155) of a call's flags
LZ4MI_HD uint32_t flg_of(uint32_t flags) {
    return 0x40u | ((flags & LZ4MI_FRAMES_DEPENDENT) ? 0u : 0x20u) | ((flags & LZ4MI_BLOCK_CHECKSUM) ? 0x10u : 0u) |
           ((flags & LZ4MI_FRAMES_NO_CONTENT_SIZE) ? 0u : 0x08u) | ((flags & LZ4MI_FRAMES_CONTENT_CHECKSUM) ? 0x04u : 0u);
}
LZ4MI_HD uint32_t header_bytes(uint32_t flg) { return 7u + ((flg & 0x08) ? 8u : 0u); }
// a block's slot in `work`, and the slots of all blocks of an n-byte source
LZ4MI_HD uint64_t slot_bytes(uint32_t n) { return ((uint64_t)n + n / 255u + 16u + 15u) & ~15ull; }
LZ4MI_HD uint64_t slots_of(uint64_t n, uint32_t bmax) {
    const uint64_t c = block_count(n, bmax);
    return c ? (c - 1) * slot_bytes(bmax) + slot_bytes((uint32_t)(n - (c - 1) * bmax)) : 0;
}
// a record (:221-231): the payload is the compressed bytes when 0 < comp < raw, else the raw ones
LZ4MI_HD bool stored(uint32_t comp, uint32_t raw) { return !(comp > 0 && comp < raw); }
LZ4MI_HD uint64_t record_bytes(uint32_t comp, uint32_t raw, uint32_t flg) {
    return 4u + (uint64_t)(stored(comp, raw) ? raw : comp) + ((flg & 0x10) ? 4u : 0u);
}

// The header checksum byte (:177-178): xxHash32 of the bytes from FLG on -- FLG, BD and, with a content size, its
// eight bytes --, >> 8. Fewer than 16 bytes: no stripe, so the reference's variant and the specification agree;
// computed from the values, whole words first, then single bytes.
LZ4MI_HD uint8_t header_checksum(uint32_t flg, uint32_t bd, uint64_t size) {
    constexpr uint32_t P1 = 2654435761u, P2 = 2246822519u, P3 = 3266489917u, P4 = 668265263u, P5 = 374761393u;
    const bool sized = (flg & 0x08) != 0;
    auto word = [&](uint32_t h, uint32_t w) { h += w * P3; return ((h << 17) | (h >> 15)) * P4; };
    auto byte = [&](uint32_t h, uint32_t b) { h += (b & 255u) * P5; return ((h << 11) | (h >> 21)) * P1; };
    uint32_t h = P5 + (sized ? 10u : 2u);
    if (sized) {
        h = word(h, (flg & 255u) | ((bd & 255u) << 8) | ((uint32_t)(size & 0xFFFFu) << 16));
        h = word(h, (uint32_t)(size >> 16));
        h = byte(h, (uint32_t)(size >> 48));
        h = byte(h, (uint32_t)(size >> 56));
    } else {
        h = byte(h, flg);
        h = byte(h, bd);
    }
    h ^= h >> 15; h *= P2; h ^= h >> 13; h *= P3; h ^= h >> 16;
    return (uint8_t)(h >> 8);
}

// The header (:147-178) at dst: magic, FLG, BD, [content size], HC. Returns its length.
LZ4MI_HD uint32_t write_header(uint8_t* dst, uint32_t flg, uint32_t bd, uint64_t size) {
    dst[0] = 0x04; dst[1] = 0x22; dst[2] = 0x4D; dst[3] = 0x18;
    dst[4] = (uint8_t)flg;
    dst[5] = (uint8_t)bd;
    uint32_t n = 6;
    if (flg & 0x08)
        for (int k = 0; k < 8; ++k) dst[n++] = (uint8_t)(size >> (8 * k));
    dst[n] = header_checksum(flg, bd, size);
    return n + 1;
}

// ------------------------------------------------------------------------------------------------ plan
// a dependent frame of more than one block is a chain: one table carried across its blocks, positions int32 from
// the frame's first byte (table values position + 1)
LZ4MI_HD bool chain_of(uint64_t count, uint32_t flags) { return (flags & LZ4MI_FRAMES_DEPENDENT) && count > 1; }
// block k of a chain over `size` bytes: src[k * bmax, +chain_len)
LZ4MI_HD uint32_t chain_len(uint64_t size, uint32_t bmax, uint64_t k) {
    const uint64_t rest = size - k * bmax;
    return (uint32_t)(rest < bmax ? rest : bmax);
}
// the declines that the lengths and the flags alone decide
LZ4MI_HD int64_t decline_of(uint64_t n, uint64_t count, uint32_t flags) {
    if (chain_of(count, flags) && (!(flags & LZ4MI_FRAMES_CHAINS) || n >= 0x7FFFFFFFull))
        return LZ4MI_FRAMES_DECLINE_DEPENDENT;
    if ((flags & LZ4MI_FRAMES_CONTENT_CHECKSUM) && n > 0xFFFFFFFFull) return LZ4MI_FRAMES_DECLINE_HASH_4G;
    return 0;
}
LZ4MI_HD void plan_count(uint64_t n, uint32_t bmax, uint32_t flags, int64_t* fi) {
    const uint64_t count = block_count(n, bmax);
    fi[kZero] = 0;
    fi[kHead] = (int64_t)(flg_of(flags) | ((block_id(bmax) & 7u) << 12));
    fi[kSize] = (int64_t)n;
    fi[kLen] = (int64_t)frame_bound(n, bmax);
    fi[kFirst] = 0;
    fi[kPos] = 0;
    fi[kCount] = (int64_t)count;
    fi[kDecline] = decline_of(n, count, flags);
}
// the blocks the frame has in the lists, and the bytes of `work` they take
LZ4MI_HD uint64_t listed(const int64_t* fi) { return fi[kDecline] ? 0 : (uint64_t)fi[kCount]; }
LZ4MI_HD uint64_t listed_work(const int64_t* fi) { return fi[kDecline] ? 0 : slots_of((uint64_t)fi[kSize], block_max(fi)); }
// Fill pass of one frame whose first block fi[kFirst] and first slot fi[kPos] (the scan's, cleared here) are
// known: its blocks into the lists, or none of them when they do not fit.
LZ4MI_HD void plan_fill(uint64_t src_off, uint32_t fidx, int64_t* fi, uint64_t* blk_in_off, uint32_t* blk_len,
                        uint32_t* blk_frame, uint64_t* blk_work_off, uint32_t cap_blocks) {
    uint64_t slot = (uint64_t)fi[kPos];
    fi[kPos] = 0;
    const uint64_t n = listed(fi), first = (uint64_t)fi[kFirst];
    if (n == 0) return;
    if (first + n > cap_blocks) {
        fi[kDecline] = LZ4MI_FRAMES_DECLINE_CAP_BLOCKS;
        return;
    }
    const uint64_t size = (uint64_t)fi[kSize], bmax = block_max(fi);
    for (uint64_t k = 0; k < n; ++k) {
        const uint64_t rest = size - k * bmax;
        const uint32_t len = (uint32_t)(rest < bmax ? rest : bmax);
        blk_in_off[first + k] = src_off + k * bmax;
        blk_len[first + k] = len;
        blk_frame[first + k] = fidx;
        blk_work_off[first + k] = slot;
        slot += slot_bytes(len);
    }
}

// -------------------------------------------------------------------------------------------- compress
// Before the encode: FLG from the call's flags, the declines only this call can see, and the frame's blocks into
// the encoder's lists (the caller has zeroed enc_off / enc_len: a block of a frame that is not written stays a
// block of length 0 at work[0], the dump slot). The blocks of a chain (LZ4MI_FRAMES_CHAINS) stay such blocks too:
// the chain pass encodes them, from blk_len / blk_work_off, and sets their enc_off and comp_len.
LZ4MI_HD void prep_frame(int64_t* fi, uint32_t nblocks, const uint32_t* blk_len, const uint64_t* blk_work_off,
                         uint64_t work_bytes, uint64_t* enc_off, uint32_t* enc_len, uint32_t flags) {
    if (fi[kDecline]) return;
    fi[kHead] = (int64_t)(flg_of(flags) | ((uint64_t)fi[kHead] & 0xFF00u));
    const uint64_t first = (uint64_t)fi[kFirst], n = (uint64_t)fi[kCount];
    if (!(first <= nblocks && n <= nblocks - first)) {
        fi[kDecline] = LZ4MI_FRAMES_DECLINE_CAP_BLOCKS;
        return;
    }
    if (const int64_t d = decline_of((uint64_t)fi[kSize], n, flags)) {
        fi[kDecline] = d;
        return;
    }
    for (uint64_t b = first; b < first + n; ++b) {
        const uint64_t off = blk_work_off[b];
        if (off < kDump || off > work_bytes || slot_bytes(blk_len[b]) > work_bytes - off) {
            fi[kDecline] = LZ4MI_FRAMES_DECLINE_CAP_BLOCKS;
            return;
        }
    }
    if (chain_of(n, flags)) {
        // the chain pass takes its blocks' lengths from the frame's: the lists must say the same (the slots
        // checked above are the ones it writes)
        const uint64_t size = (uint64_t)fi[kSize], bmax = block_max(fi);
        bool same = n == block_count(size, (uint32_t)bmax);
        for (uint64_t k = 0; same && k < n; ++k) same = blk_len[first + k] == chain_len(size, (uint32_t)bmax, k);
        if (!same) fi[kDecline] = LZ4MI_FRAMES_DECLINE_CAP_BLOCKS;
        return;
    }
    for (uint64_t b = first; b < first + n; ++b) {
        enc_off[b] = blk_work_off[b];
        enc_len[b] = blk_len[b];
    }
}
// after prep_frame: the chain pass walks this frame (FLG is the compress call's)
LZ4MI_HD bool is_chain(const int64_t* fi) { return !fi[kDecline] && fi[kCount] > 1 && !((uint64_t)fi[kHead] & 0x20u); }

// The frame's length from its blocks' compressed sizes.
LZ4MI_HD void size_frame(int64_t* fi, const uint32_t* blk_len, const uint32_t* comp_len) {
    if (fi[kDecline]) return;
    const uint32_t flg = (uint32_t)fi[kHead] & 0xFF;
    const uint64_t first = (uint64_t)fi[kFirst], n = (uint64_t)fi[kCount];
    uint64_t len = header_bytes(flg) + 4u + ((flg & 0x04) ? 4u : 0u);
    for (uint64_t b = first; b < first + n; ++b) len += record_bytes(comp_len[b], blk_len[b], flg);
    fi[kLen] = (int64_t)len;
}
// Slot mode: the frame at the caller's position, if it fits its slot and `out`.
LZ4MI_HD void place_frame(int64_t* fi, uint64_t off, uint64_t cap, uint64_t out_total) {
    if (fi[kDecline]) return;
    const uint64_t len = (uint64_t)fi[kLen];
    if (len > cap || off > out_total || len > out_total - off) fi[kDecline] = LZ4MI_FRAMES_DECLINE_OUT_CAP;
    else fi[kPos] = (int64_t)off;
}
// Packed mode, one frame after the other: the frame at `at` if it ends inside `out`. Returns the next position.
LZ4MI_HD uint64_t pack_frame(int64_t* fi, uint64_t at, uint64_t out_total) {
    if (fi[kDecline]) return at;
    const uint64_t len = (uint64_t)fi[kLen];
    if (at > out_total || len > out_total - at) {
        fi[kDecline] = LZ4MI_FRAMES_DECLINE_OUT_CAP;
        return at;
    }
    fi[kPos] = (int64_t)at;
    return at + len;
}

// Header, record positions, EndMark and the content checksum's place of a frame that is written (the caller has
// set rec_off / hash_dst to kNone and hash_len to 0 for every block and frame). hash_*[f]: the source range and
// the position in `out` of the content checksum.
LZ4MI_HD void write_frame(const int64_t* fi, uint8_t* out, const uint64_t* blk_in_off, const uint32_t* blk_len,
                          const uint32_t* comp_len, uint64_t* rec_off, uint64_t* hash_off, uint32_t* hash_len,
                          uint64_t* hash_dst) {
    if (fi[kDecline]) return;
    const uint32_t flg = (uint32_t)fi[kHead] & 0xFF, bd = ((uint32_t)fi[kHead] >> 8) & 0xFF;
    const uint64_t first = (uint64_t)fi[kFirst], n = (uint64_t)fi[kCount];
    uint64_t at = (uint64_t)fi[kPos];
    at += write_header(out + at, flg, bd, (uint64_t)fi[kSize]);
    for (uint64_t b = first; b < first + n; ++b) {
        rec_off[b] = at;
        at += record_bytes(comp_len[b], blk_len[b], flg);
    }
    for (int k = 0; k < 4; ++k) out[at + k] = 0;
    if (flg & 0x04) {
        *hash_off = n ? blk_in_off[first] : 0;
        *hash_len = (uint32_t)fi[kSize];
        *hash_dst = at + 4;
    }
}

}  // namespace frames_enc
}  // namespace lz4mi
