// lz4mi_frames.h — the per-frame steps of the frame batch (lz4mi_frames_index, include/lz4mi.h), written
// once for the device passes (lz4mi_frames.hip, one lane per frame) and for lz4mi_host_frames_index
// (lz4mi_host.cpp, the calling thread): the walk of a frame's header and size words, the listing of its
// blocks and the decoded size each block is given. finfo[f] is the eight values the header documents.
// The single-frame calls (lz4mi_frame_index, lz4mi_frame_decompress; lz4mi_frame.hip, one lane) use the same
// walk: index_frame and scan_frame, with lz4mi_host_frame_index / lz4mi_debug_frame_scan as their host twins.
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

// BLOCK_MAX_SIZES: the bytes of a BD byte's 3-bit block size id
LZ4MI_HD uint32_t block_bytes(uint32_t id) { return id == 4 ? 65536u : id == 5 ? 262144u : id == 6 ? 1048576u : 4194304u; }

// The reference's walk of a frame (bufferDecompress.js:56-92 header, :133-192 block loop) over
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
        // the whole word lies inside: one load, not four that wait for each other (little-endian host and
        // device: x86-64, gfx950)
        if (len >= 4 && p <= len - 4) {
            __builtin_memcpy(&v, f + p, 4);
            return v;
        }
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
        bmax = block_bytes((bd >> 4) & 7);
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
LZ4MI_HD uint32_t block_max(const int64_t* fi) { return block_bytes((uint32_t)(fi[kHead] >> 12) & 7); }
// the blocks the frame has in the lists: none for a frame with a header error or one of the declines
// that are known before the blocks are listed
LZ4MI_HD uint64_t listed(const int64_t* fi) {
    const int64_t d = fi[kDecline];
    const bool none = fi[kErr] || d == LZ4MI_FRAMES_DECLINE_PAST_END || d == LZ4MI_FRAMES_DECLINE_EMPTY ||
                      d == LZ4MI_FRAMES_DECLINE_CAP_BLOCKS;
    return none ? 0 : (uint64_t)fi[kCount];
}

// lz4mi_frames_verify_blocks: is frame fi one whose block checksums the call checks -- no error yet, FLG 0x10,
// blocks in the lists and all of them inside [0, nblocks)? Every decline that leaves the blocks listed
// (MEASURE, SIZE_MISMATCH, UNSIZED_EXACT) is irrelevant here.
LZ4MI_HD bool verify_checked(const int64_t* fi, uint32_t nblocks) {
    if (fi[kErr] || !(fi[kHead] & 0x10)) return false;
    const uint64_t n = listed(fi), first = (uint64_t)fi[kFirst];
    return n != 0 && first <= nblocks && n <= nblocks - first;
}
// Is the record at `at` (absolute in `in`) -- a payload of n bytes, n < 2^31, and the LE32 behind it -- whole
// inside the frame in[off .. off + len)? Differences only, so nothing wraps.
LZ4MI_HD bool record_whole(uint64_t at, uint64_t n, uint64_t off, uint64_t len) {
    return at >= off && at - off <= len && n + 4 <= len - (at - off);
}

// The argument rules of lz4mi_frames_verify_blocks and its host twin, behind the flags: the pointers a count needs,
// and neither array the call writes may be an array it reads or the other one (the pointers themselves).
inline bool verify_bad_args(const uint8_t* in, const uint64_t* frame_off, const uint64_t* frame_len, uint32_t nframes,
                            const uint64_t* blk_in_off, const uint32_t* blk_word, const uint32_t* blk_frame,
                            uint32_t nblocks, const int64_t* finfo, const int32_t* blk_status) {
    if (nframes && (!finfo || !frame_off || !frame_len)) return true;
    if (nblocks && (!in || !blk_in_off || !blk_word || !blk_frame || !blk_status)) return true;
    const void* wr[2] = {finfo, blk_status};
    const void* rd[6] = {in, frame_off, frame_len, blk_in_off, blk_word, blk_frame};
    if (wr[0] && wr[0] == wr[1]) return true;
    for (const void* w : wr)
        for (const void* r : rd)
            if (w && w == r) return true;
    return false;
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

// The reference encoder's layout of a result of `size` bytes: the slot of each block in frame order. A
// compressed block takes what is left of the result, block_max at most, and the position advances by
// block_max; a stored block takes its declared size, and the reference advances by the declared size.
// `size` is unsigned: a content size of 2^63 or more, which no caller has room for (lz4mi_frame_decompress
// declines size > out_cap before it scans), leaves block_max, not 0 as a signed difference would.
struct Layout {
    uint64_t size, bmax, op = 0;   // op: the next block's position in the result

    LZ4MI_HD Layout(uint64_t size_, uint64_t bmax_) : size(size_), bmax(bmax_) {}
    LZ4MI_HD uint32_t slot(uint32_t word) {
        if (word & 0x80000000u) {
            op += word & 0x7FFFFFFFu;
            return word & 0x7FFFFFFFu;
        }
        const uint64_t left = size > op ? size - op : 0;
        op += bmax;
        return (uint32_t)(left < bmax ? left : bmax);
    }
};

// Sizes of one frame's listed blocks and its decoded total. A frame with a content size takes the
// reference encoder's layout; a measured one the size walk's results msize / mstatus
// (lz4mi_decoded_sizes over meas_word).
LZ4MI_HD void size_frame(int64_t* fi, const uint32_t* blk_word, const uint32_t* msize, const int32_t* mstatus,
                         uint32_t* blk_size) {
    const uint64_t n = listed(fi), first = (uint64_t)fi[kFirst];
    if (n == 0) return;
    const uint64_t size = (uint64_t)fi[kSize], bmax = block_max(fi);
    if (fi[kDecline]) {   // (an unsized frame under LZ4MI_JS_EXACT: listed, not sized)
        for (uint64_t b = first; b < first + n; ++b) blk_size[b] = 0;
        return;
    }
    if (!(fi[kHead] & kMeasured)) {
        Layout lay(size, bmax);
        for (uint64_t b = first; b < first + n; ++b) blk_size[b] = lay.slot(blk_word[b]);
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

// ------------------------------------------------------------------------ the single-frame calls
// The eight info words of lz4mi_frame_index / lz4mi_frame_decompress after a walk: status, FLG, content size,
// the two counts, the position the walk stopped at, block_max, and 1 when it ended behind the frame or the
// lists were full. A header error leaves everything behind FLG at its initial value.
LZ4MI_HD void walk_info(const Walk& w, uint32_t n3, uint32_t n4, bool full, int64_t* info) {
    info[0] = w.err;
    info[1] = w.flg;
    info[2] = (int64_t)w.size;
    info[3] = n3;
    info[4] = n4;
    info[5] = (int64_t)w.pos;
    info[6] = w.bmax;
    info[7] = full || w.pos > w.len;
}

// lz4mi_frame_index of one frame: every block in frame order, payload position and raw size word. When the
// lists are full nothing more is written and the walk stops behind the size word of the first block that
// did not fit.
LZ4MI_HD void index_frame(const uint8_t* f, uint64_t len, uint32_t cap_blocks, uint64_t* pay_off, uint32_t* size_word,
                          int64_t* info) {
    Walk w(f, len);
    w.head();
    uint32_t n = 0;
    bool full = false;
    uint64_t pay;
    uint32_t word;
    while (!w.err && w.next(pay, word)) {
        if (n == cap_blocks) {
            full = true;
            w.pos = pay;
            break;
        }
        pay_off[n] = pay;
        size_word[n] = word;
        ++n;
    }
    walk_info(w, n, 0, full, info);
}

// The block lists of lz4mi_frame_decompress: compressed and stored blocks apart (c_idx / s_idx: the block's
// index in frame order), each with its slot of the reference encoder's layout. The caller checks the decoded
// lengths against the slots. Full lists: as in index_frame.
LZ4MI_HD void scan_frame(const uint8_t* f, uint64_t len, uint32_t cap_blocks, uint64_t* c_in_off, uint32_t* c_in_len,
                         uint64_t* c_out_off, uint32_t* c_out_cap, uint64_t* s_in_off, uint32_t* s_len,
                         uint64_t* s_out_off, uint32_t* c_idx, uint32_t* s_idx, int64_t* info) {
    Walk w(f, len);
    w.head();
    Layout lay(w.size, w.bmax);
    uint32_t nc = 0, ns = 0;
    bool full = false;
    uint64_t pay;
    uint32_t word;
    while (!w.err && w.next(pay, word)) {
        if (nc + ns == cap_blocks) {
            full = true;
            w.pos = pay;
            break;
        }
        const uint64_t at = lay.op;
        const uint32_t slot = lay.slot(word);
        if (word & 0x80000000u) {
            s_in_off[ns] = pay;
            s_len[ns] = slot;
            s_out_off[ns] = at;
            s_idx[ns] = nc + ns;
            ++ns;
        } else {
            c_in_off[nc] = pay;
            c_in_len[nc] = word;
            c_out_off[nc] = at;
            c_out_cap[nc] = slot;
            c_idx[nc] = nc + ns;
            ++nc;
        }
    }
    walk_info(w, nc, ns, full, info);
}

}  // namespace frames
}  // namespace lz4mi
