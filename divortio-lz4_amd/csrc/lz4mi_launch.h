// lz4mi_launch.h — the host side's launch interface: every lz4mi_launch_* function, declared
// once (each .hip that defines or calls one includes this header, and so does lz4mi_capi.cpp: a
// definition that disagrees with its declaration does not compile), the block list they take
// (Batch) and the layout of the small path's scratch (XLayout).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "lz4mi_decompress.h"

namespace lz4mi {

// The block list of a decode call: block b's compressed bytes at in + in_off[b] (in_len[b] of
// them), its output slot at out + out_off[b] (out_cap[b] bytes), the results in out_len[b] and
// status[b]. Device pointers.
struct Batch {
    const uint8_t* in;
    const uint64_t* in_off;
    const uint32_t* in_len;
    uint8_t* out;
    const uint64_t* out_off;
    const uint32_t* out_cap;
    const uint8_t* dict;
    uint32_t dict_len;
    uint32_t* out_len;
    int32_t* status;
    uint32_t nblocks;
    // blocks [first, first + n) of this list
    Batch slice(uint32_t first, uint32_t n) const {
        return Batch{in, in_off + first, in_len + first, out, out_off + first, out_cap + first, dict, dict_len,
                     out_len + first, status + first, n};
    }
};

// The scratch of one small-path pass (lz4mi_launch_decompress_small) or linked window
// (lz4mi_launch_decompress_linked): every region's place in it, the only size formula there is.
// Linked windows have a head in front (the call's state in its first 256 bytes, then the
// window's lengths and bases: lz4mi_linked_prep_kernel); the parse writes xseq (stride sequence
// entries per block), xcnt, xfirst and xrec (zeroed per pass up to ptr, padding included); the
// output kernels use ptr (x_out_max pointers per block), the round flags, the check results
// (best) and reference-mode marks (redo), both padded to 64 blocks, and a done byte per 16
// output bytes.
struct XRegion {
    size_t off, bytes;
    template <class T> T* in(void* xs) const { return reinterpret_cast<T*>(static_cast<uint8_t*>(xs) + off); }
};
struct XLayout {
    XRegion head, xseq, xcnt, xfirst, xrec, ptr, flags, best, redo, done;
    size_t total;
    uint32_t x_in_max, x_out_max, stride;
};
inline XLayout x_layout(uint32_t nblocks, uint32_t x_in_max, uint32_t x_out_max, bool linked) {
    const auto up256 = [](size_t n) { return (n + 255) / 256 * 256; };
    const size_t n = nblocks, pad64 = ((n + 63) & ~(size_t)63) * 4;
    XLayout L{};
    L.x_in_max = x_in_max;
    L.x_out_max = x_out_max;
    L.stride = seg_block_capacity(x_in_max);
    L.head = {0, linked ? 256 + n * 8 : 0};
    L.xseq = {up256(L.head.bytes), n * L.stride * 16};
    L.xcnt = {L.xseq.off + up256(L.xseq.bytes), n * 4};
    L.xfirst = {L.xcnt.off + L.xcnt.bytes, n * 4};
    L.xrec = {L.xfirst.off + L.xfirst.bytes, n * kSegMax * sizeof(SegRec)};
    L.ptr = {L.xcnt.off + up256(n * 8 + L.xrec.bytes), n * x_out_max * 4};
    L.flags = {L.ptr.off + L.ptr.bytes, 32 * 4};
    L.best = {L.flags.off + L.flags.bytes, pad64};
    L.redo = {L.best.off + L.best.bytes, pad64};
    L.done = {L.redo.off + L.redo.bytes, n * (x_out_max / 16)};
    L.total = L.done.off + L.done.bytes + 256;
    return L;
}

}  // namespace lz4mi

extern "C" {

// ---- decoder (lz4mi_decompress.hip, lz4mi_decompress_serial.hip, lz4mi_expand.hip, lz4mi_size.hip)
// isolate: a back-reference below a block's own start is LZ4MI_ERR_CROSS_BLOCK, not followed
hipError_t lz4mi_launch_decompress(const lz4mi::Batch& b, int mode, int isolate, uint32_t* order, hipStream_t stream);
// the chains of a frame batch (LZ4MI_FRAMES_CHAINS), behind lz4mi_launch_frames_place and the isolated batch launch:
// one wave per frame decodes, in block order and with lone-block semantics in an array that begins at the frame's
// slot, the blocks of a multi-block dependent frame, or of any other frame from its first block with status
// LZ4MI_ERR_CROSS_BLOCK on; every other frame's wave returns at once. b.in_len: the real size words (blk_word)
hipError_t lz4mi_launch_decompress_frames_chain(const lz4mi::Batch& b, int mode, const int64_t* finfo,
                                                const uint64_t* frame_out_off, uint32_t nframes, hipStream_t stream);
hipError_t lz4mi_launch_decompress_serial(const lz4mi::DecArgs& a, hipStream_t stream);
size_t lz4mi_small_scratch_bytes(uint32_t nblocks, uint32_t x_in_max, uint32_t x_out_max);
hipError_t lz4mi_launch_decompress_small(const lz4mi::Batch& b, uint32_t x_in_max, uint32_t x_out_max, void* xs,
                                         int force_reparse, int f1, hipStream_t stream);
size_t lz4mi_linked_scratch_bytes(uint32_t nblocks, uint32_t x_in_max, uint32_t x_out_max);
hipError_t lz4mi_launch_decompress_linked(const lz4mi::Batch& b, uint32_t x_in_max, uint32_t x_out_max, void* xs,
                                          int force_reparse, int frame_words, int has_prev, int f1,
                                          hipStream_t stream);
hipError_t lz4mi_launch_linked_prep(const lz4mi::Batch& b, const lz4mi::XLayout& L, void* xs, int frame_words,
                                    int has_prev, hipStream_t stream);
hipError_t lz4mi_launch_expand(const lz4mi::Batch& b, const lz4mi::XLayout& L, void* xs, bool linked, int f1,
                               int frame_words, hipStream_t stream);
hipError_t lz4mi_launch_linked_fail(uint32_t* out_len, int32_t* status, uint32_t nblocks, uint32_t* xl,
                                    hipStream_t stream);
hipError_t lz4mi_launch_sizes(const uint8_t* in, const uint64_t* in_off, const uint32_t* in_len, uint32_t* out_len,
                              int32_t* status, uint32_t nblocks, int frame_words, hipStream_t stream);

// ---- encoder, checksums, generators (lz4mi_compress.hip, lz4mi_xxh32.hip)
hipError_t lz4mi_launch_compress(const uint8_t* in, const uint64_t* in_off, const uint32_t* in_len, uint8_t* out,
                                 const uint64_t* out_off, uint32_t* out_len, uint32_t nblocks, int32_t* tables,
                                 hipStream_t stream);
hipError_t lz4mi_launch_compress_chain(const uint8_t* src, uint64_t src_total, int32_t start, int32_t len,
                                       int32_t bsize, int32_t* table, uint8_t* out, const uint64_t* out_off,
                                       uint32_t* comp_len, uint32_t nblocks, hipStream_t stream);
// the chains of a frame batch (LZ4MI_FRAMES_CHAINS), behind lz4mi_launch_frames_enc_prep and the batch encoder: one
// workgroup per frame walks the blocks of a multi-block dependent frame that is written into their slots of `work`
// and sets their enc_off and comp_len; every other frame's workgroup returns at once
hipError_t lz4mi_launch_compress_chains(const uint8_t* in, const uint64_t* blk_in_off, const uint64_t* blk_work_off,
                                        const int64_t* finfo, uint32_t nframes, uint8_t* work, uint64_t* enc_off,
                                        uint32_t* comp_len, hipStream_t stream);
hipError_t lz4mi_launch_xxh32(const uint8_t* in, const uint64_t* off, const uint32_t* len, uint32_t seed,
                              uint32_t* hashes, uint32_t n, int standard, uint8_t* dst, const uint64_t* dst_off,
                              hipStream_t stream);
hipError_t lz4mi_launch_verify(const uint8_t* in, uint64_t in_total, const uint64_t* in_off, const uint32_t* in_len,
                               int32_t* status, uint32_t n, int frame_words, hipStream_t stream);
// lz4mi_frames_verify_blocks: the block checksums of the checked frames into blk_status (one quad per listed block,
// bounds per frame), then one wave per frame folds them into finfo[f][0]
hipError_t lz4mi_launch_frames_verify(const uint8_t* in, const uint64_t* frame_off, const uint64_t* frame_len,
                                      uint32_t nframes, const uint64_t* blk_in_off, const uint32_t* blk_word,
                                      const uint32_t* blk_frame, uint32_t nblocks, int64_t* finfo, int32_t* blk_status,
                                      hipStream_t stream);
hipError_t lz4mi_launch_generate(uint8_t* out, uint32_t kind, uint32_t seed0, uint32_t bsize, uint32_t nblocks,
                                 hipStream_t stream);

// ---- frames (lz4mi_frame.hip)
hipError_t lz4mi_launch_frame_scan(const uint8_t* f, uint64_t len, uint32_t cap_blocks, uint64_t* c_in_off,
                                   uint32_t* c_in_len, uint64_t* c_out_off, uint32_t* c_out_cap, uint64_t* s_in_off,
                                   uint32_t* s_len, uint64_t* s_out_off, uint32_t* c_idx, uint32_t* s_idx,
                                   int64_t* info, hipStream_t stream);
hipError_t lz4mi_launch_frame_stored(const uint8_t* f, uint64_t len, const uint64_t* s_in_off, const uint32_t* s_len,
                                     const uint64_t* s_out_off, uint8_t* out, uint64_t cap, uint32_t ns,
                                     hipStream_t stream);
hipError_t lz4mi_launch_frame_pack(const uint8_t* raw, const uint64_t* raw_off, const uint32_t* raw_len,
                                   const uint8_t* comp, const uint64_t* comp_off, const uint32_t* comp_len,
                                   uint8_t* frame, const uint64_t* rec_off, uint32_t nblocks, uint64_t* pay_off,
                                   uint64_t* sum_off, uint32_t* pay_len, hipStream_t stream);
hipError_t lz4mi_launch_frame_index(const uint8_t* f, uint64_t len, uint32_t cap_blocks, uint64_t* pay_off,
                                    uint32_t* size_word, int64_t* info, hipStream_t stream);

// ---- frame batches (lz4mi_frames.hip)
hipError_t lz4mi_launch_frames_index(const uint8_t* in, const uint64_t* frame_off, const uint64_t* frame_len,
                                     uint32_t nframes, uint64_t* blk_in_off, uint32_t* blk_word, uint32_t* blk_frame,
                                     uint32_t* blk_size, uint32_t cap_blocks, int64_t* finfo, int64_t* totals,
                                     uint32_t* meas_word, uint32_t* msize, int32_t* mstatus, uint32_t flags,
                                     hipStream_t stream);
hipError_t lz4mi_launch_frames_place(int64_t* finfo, uint32_t nframes, const uint32_t* blk_word,
                                     const uint32_t* blk_size, uint32_t nblocks, const uint64_t* frame_out_off,
                                     const uint64_t* frame_out_cap, uint32_t* word, uint64_t* out_off, uint32_t* out_cap,
                                     uint32_t flags, hipStream_t stream);
hipError_t lz4mi_launch_frames_finish(int64_t* finfo, uint32_t nframes, uint32_t nblocks, const uint32_t* word,
                                      const uint64_t* out_off, const uint32_t* out_cap, const uint32_t* out_len,
                                      const int32_t* status, uint8_t* out, const uint64_t* frame_out_off,
                                      uint64_t* hash_off, uint32_t* hash_len, uint32_t* hashed, uint32_t* digest,
                                      uint32_t flags, hipStream_t stream);

// ---- frame batches, encode side (lz4mi_frames_enc.hip): the plan; the pass before the batch encoder (enc_off /
// enc_len: the encoder's lists, zeroed by the caller); everything behind it (rec_off, sum_off, hash_dst set to
// ~0 and pay_len, hash_len to 0 by the caller; lz4mi_launch_xxh32 stores no digest at ~0)
hipError_t lz4mi_launch_frames_plan(const uint64_t* src_off, const uint64_t* src_len, uint32_t nframes, uint32_t bmax,
                                    uint64_t* blk_in_off, uint32_t* blk_len, uint32_t* blk_frame, uint64_t* blk_work_off,
                                    uint32_t cap_blocks, int64_t* finfo, int64_t* totals, uint32_t flags,
                                    hipStream_t stream);
hipError_t lz4mi_launch_frames_enc_prep(int64_t* finfo, uint32_t nframes, uint32_t nblocks, const uint32_t* blk_len,
                                        const uint64_t* blk_work_off, uint64_t work_bytes, uint64_t* enc_off,
                                        uint32_t* enc_len, uint32_t flags, hipStream_t stream);
hipError_t lz4mi_launch_frames_enc_finish(const uint8_t* in, const uint64_t* blk_in_off, const uint32_t* blk_len,
                                          uint32_t nblocks, int64_t* finfo, uint32_t nframes, const uint8_t* work,
                                          const uint64_t* enc_off, const uint32_t* comp_len, uint8_t* out,
                                          uint64_t out_total, const uint64_t* frame_out_off,
                                          const uint64_t* frame_out_cap, uint64_t* rec_off, uint64_t* pay_off,
                                          uint64_t* sum_off, uint32_t* pay_len, uint64_t* hash_off, uint32_t* hash_len,
                                          uint64_t* hash_dst, uint32_t flags, hipStream_t stream);

}  // extern "C"
