// lz4mi_frames.h — the per-frame steps of the frame batch (lz4mi_frames_index, include/lz4mi.h), written
// once for the device passes (lz4mi_frames.hip, one lane per frame) and for lz4mi_host_frames_index
// (lz4mi_host.cpp, the calling thread): the walk of a frame's header and size words, the listing of its
// blocks and the decoded size each block is given. finfo[f] is the eight values the header documents.
#pragma once
#include <stdint.h>

#include "../../include/lz4mi.h"

#if defined(__HIPCC__)
#define LZ4MI_HD __host__ __device__ inline
#else
#define LZ4MI_HD inline
#endif

namespace lz4mi {
namespace frames {

enum { kErr = 0, kHead = 1, kSize = 2, kTotal = 3, kFirst = 4, kEnd = 5, kCount = 6, kDecline = 7 };

// The walk of lz4mi_frame_index_kernel (bufferDecompress.js:56-92 header, :133-192 block loop) over
// f[0 .. len): bytes past the end read as 0, nothing outside is read. Checks in the reference's order:
// magic, version, then the size field, DictID and HC byte skipped.
struct Walk {
    const uint8_t* f;
    uint64_t len;
    uint64_t pos = 0, size = 0;
    uint32_t flg = 0, bd = 0, bmax = 4194304;
    int32_t err = 0;

    LZ4MI_HD Walk(const uint8_t* f_, uint64_t len_) : f(f_), len(len_) {}
    LZ4MI_HD uint32_t rd(uint64_t p) const {
        uint32_t v = 0;
        for (int k = 0; k < 4; ++k) v |= (p + k < len ? (uint32_t)f[p + k] : 0u) << (8 * k);
        return v;
    }
    LZ4MI_HD void head() {
        if (len < 4 || rd(0) != 0x184D2204u) {
            err = LZ4MI_ERR_MAGIC;
            return;
        }
        flg = len > 4 ? f[4] : 0;
        if (((flg & 0xC0) >> 6) != 1) {
            err = LZ4MI_ERR_VERSION;
            return;
        }
        bd = len > 5 ? f[5] : 0;
        const uint32_t id = len > 5 ? (bd >> 4) & 7 : 7;
        bmax = id == 4 ? 65536 : id == 5 ? 262144 : id == 6 ? 1048576 : 4194304;
        pos = 6;
        if (flg & 0x08) {
            size = (uint64_t)rd(pos) | ((uint64_t)rd(pos + 4) << 32);
            pos += 8;
        }
        if (flg & 0x01) pos += 4;
        pos += 1;
    }
    // The next block's payload position (relative to the frame) and raw size word; false at the EndMark
    // (pos then lies behind it) or at pos >= len. Every call advances pos by at least 4.
    LZ4MI_HD bool next(uint64_t& pay, uint32_t& word) {
        if (pos >= len) return false;
        word = rd(pos);
        pos += 4;
        if (word == 0) return false;
        pay = pos;
        pos += (uint64_t)(word & 0x7FFFFFFFu) + ((flg & 0x10) ? 4 : 0);
        return true;
    }
};

// finfo[kHead]: FLG | BD << 8, bit 16 = the frame's block sizes are measured (set by the fill), bits 32-63 =
// the LE32 behind the EndMark of a frame with a content checksum (FLG 0x04)
constexpr int64_t kMeasured = 1 << 16;
LZ4MI_HD bool sized(const int64_t* fi) { return (fi[kHead] & 0x08) && fi[kSize] != 0; }
LZ4MI_HD uint32_t block_max(const int64_t* fi) {
    const uint32_t id = (uint32_t)(fi[kHead] >> 12) & 7;
    return id == 4 ? 65536 : id == 5 ? 262144 : id == 6 ? 1048576 : 4194304;
}
// the blocks the frame has in the lists: none for a frame with a header error or one of the declines
// that are known before the blocks are listed
LZ4MI_HD uint64_t listed(const int64_t* fi) {
    const int64_t d = fi[kDecline];
    const bool none = fi[kErr] || d == LZ4MI_FRAMES_DECLINE_PAST_END || d == LZ4MI_FRAMES_DECLINE_EMPTY ||
                      d == LZ4MI_FRAMES_DECLINE_CAP_BLOCKS;
    return none ? 0 : (uint64_t)fi[kCount];
}

// Count pass of one frame.
LZ4MI_HD void count_frame(const uint8_t* f, uint64_t len, int64_t* fi) {
    Walk w(f, len);
    w.head();
    int64_t n = 0;
    uint64_t pay;
    uint32_t word;
    if (!w.err)
        while (w.next(pay, word)) ++n;
    const bool past = !w.err && w.pos > len;
    const int64_t sum = (!w.err && !past && (w.flg & 0x04)) ? (int64_t)((uint64_t)w.rd(w.pos) << 32) : 0;
    fi[kErr] = w.err;
    fi[kHead] = (int64_t)(w.flg | (w.bd << 8)) | sum;
    fi[kSize] = (int64_t)w.size;
    fi[kTotal] = 0;
    fi[kFirst] = 0;
    fi[kEnd] = (int64_t)w.pos;
    fi[kCount] = n;
    fi[kDecline] = w.err ? 0
                   : past ? LZ4MI_FRAMES_DECLINE_PAST_END
                   : (n == 0 || ((w.flg & 0x08) && w.size == 0)) ? LZ4MI_FRAMES_DECLINE_EMPTY
                                                                   : 0;
}

// Fill pass of one frame whose first block index finfo[kFirst] is known: its blocks into the lists, or
// none of them when they do not fit. meas_word[b]: the size word of a block to be measured, else 0.
LZ4MI_HD void fill_frame(const uint8_t* f, uint64_t len, uint64_t frame_off, uint32_t fidx, int64_t* fi,
                         uint64_t* blk_in_off, uint32_t* blk_word, uint32_t* blk_frame, uint32_t* meas_word,
                         uint32_t cap_blocks, uint32_t flags) {
    const uint64_t n = listed(fi);
    if (n == 0) return;
    const uint64_t first = (uint64_t)fi[kFirst];
    if (first + n > cap_blocks) {
        fi[kDecline] = LZ4MI_FRAMES_DECLINE_CAP_BLOCKS;
        return;
    }
    const bool unsized = !sized(fi);
    const bool exact_unsized = unsized && (flags & LZ4MI_JS_EXACT);
    const bool measure = (unsized || (flags & LZ4MI_FRAMES_MEASURE)) && !exact_unsized;
    if (exact_unsized) fi[kDecline] = LZ4MI_FRAMES_DECLINE_UNSIZED_EXACT;
    if (measure) fi[kHead] |= kMeasured;
    Walk w(f, len);
    w.head();
    uint64_t pay;
    uint32_t word;
    for (uint64_t b = first; b < first + n && w.next(pay, word); ++b) {
        blk_in_off[b] = frame_off + pay;
        blk_word[b] = word;
        blk_frame[b] = fidx;
        meas_word[b] = measure ? word : 0u;
    }
}

// Sizes of one frame's listed blocks and its decoded total. A frame with a content size takes the
// reference encoder's layout (lz4mi_frame_scan_kernel); a measured one the size walk's results
// msize / mstatus (lz4mi_decoded_sizes over meas_word).
LZ4MI_HD void size_frame(int64_t* fi, const uint32_t* blk_word, const uint32_t* msize, const int32_t* mstatus,
                         uint32_t* blk_size) {
    const uint64_t n = listed(fi), first = (uint64_t)fi[kFirst];
    if (n == 0) return;
    const uint64_t size = (uint64_t)fi[kSize];
    const uint64_t bmax = block_max(fi);
    if (fi[kDecline]) {   // (an unsized frame under LZ4MI_JS_EXACT: listed, not sized)
        for (uint64_t b = first; b < first + n; ++b) blk_size[b] = 0;
        return;
    }
    if (!(fi[kHead] & kMeasured)) {
        uint64_t op = 0;
        for (uint64_t b = first; b < first + n; ++b) {
            const uint32_t word = blk_word[b], dn = word & 0x7FFFFFFFu;
            if (word & 0x80000000u) {
                blk_size[b] = dn;
                op += dn;              // the reference advances by the declared size
            } else {
                const uint64_t left = size > op ? size - op : 0;
                blk_size[b] = (uint32_t)(left < bmax ? left : bmax);
                op += bmax;
            }
        }
        fi[kTotal] = (int64_t)size;
        return;
    }
    uint64_t total = 0, comp_max = 0;
    bool bad = false;
    for (uint64_t b = first; b < first + n; ++b) {
        const uint32_t sz = msize[b];
        blk_size[b] = sz;
        total += sz;
        if (mstatus[b]) bad = true;
        if (!(blk_word[b] & 0x80000000u) && sz > comp_max) comp_max = sz;
    }
    fi[kTotal] = (int64_t)total;
    if (bad || (!sized(fi) && comp_max > bmax)) fi[kDecline] = LZ4MI_FRAMES_DECLINE_MEASURE;
    else if (sized(fi) && total != size) fi[kDecline] = LZ4MI_FRAMES_DECLINE_SIZE_MISMATCH;
}

}  // namespace frames
}  // namespace lz4mi
