// lz4mi_frame.hip — device-side frame block records.
//
// The frame writer's block loop (reference src/buffer/bufferCompress.js:209-239)
// emits, per block, a LE32 size word and the payload: the compressed bytes when
// 0 < compSize < blockSize, else blockSize | 0x80000000 and the raw bytes. With
// independent blocks compressed in one batch on the device, this kernel writes
// those records straight into the frame buffer at caller-computed offsets
// (exclusive prefix sum of 4 + payload), so the frame never visits the host.
// One wave per block; 16-byte unaligned pieces, the last one overlapping.
// With block checksums (FLG bit 0x10) a record is size word + payload + LE32
// XXH32(payload): the kernel then also writes each payload's frame position and
// length (pay_off/pay_len) and its checksum position (sum_off) for the batched
// XXH32 kernel that fills them in.
#include "lz4mi_common.h"
#include "lz4mi_frames_enc.h"
#include "lz4mi_launch.h"

namespace lz4mi {

__global__ __launch_bounds__(64) void lz4mi_frame_pack_kernel(const uint8_t* raw, const uint64_t* raw_off,
                                                              const uint32_t* raw_len, const uint8_t* comp,
                                                              const uint64_t* comp_off, const uint32_t* comp_len,
                                                              uint8_t* frame, const uint64_t* rec_off,
                                                              uint32_t nblocks, uint64_t* pay_off, uint64_t* sum_off,
                                                              uint32_t* pay_len) {
    const uint32_t b = blockIdx.x;
    const int lane = threadIdx.x;
    if (b >= nblocks) return;
    const uint32_t n = raw_len[b], cl = comp_len[b];
    const bool st = frames_enc::stored(cl, n);
    wave_record(frame, rec_off[b], st ? (n | 0x80000000u) : cl, st ? raw + raw_off[b] : comp + comp_off[b], st ? n : cl,
                b, pay_off, sum_off, pay_len, lane);
}

// ---------------------------------------------------------------------------
// Decode side: the frame's header and block walk on the device (the reference's
// decompressBuffer, src/buffer/bufferDecompress.js:56-92 header, :133-192 block loop).
// One lane walks the size words (each record's position depends on the previous
// size): frames::scan_frame lists compressed and stored blocks apart, with output
// positions of the reference encoder's layout; frames::index_frame lists every block
// in frame order for sharded decoding (lz4mi_frame_index). Both are lz4mi_frames.h,
// where the frame batch's walk lives.
// info[0] status (0, LZ4MI_ERR_MAGIC -5, LZ4MI_ERR_VERSION -6), [1] FLG, [2] content size,
// [3] compressed blocks (the index: blocks listed), [4] stored blocks (the index: 0),
// [5] position after the EndMark (content checksum), [6] block_max (BD), [7] 1 if the walk
// ran past the frame or the lists' capacity.
__global__ __launch_bounds__(64) void lz4mi_frame_scan_kernel(const uint8_t* f, uint64_t len, uint32_t cap_blocks,
                                                              uint64_t* c_in_off, uint32_t* c_in_len,
                                                              uint64_t* c_out_off, uint32_t* c_out_cap,
                                                              uint64_t* s_in_off, uint32_t* s_len, uint64_t* s_out_off,
                                                              uint32_t* c_idx, uint32_t* s_idx, int64_t* info) {
    if (threadIdx.x != 0) return;
    frames::scan_frame(f, len, cap_blocks, c_in_off, c_in_len, c_out_off, c_out_cap, s_in_off, s_len, s_out_off, c_idx,
                       s_idx, info);
}

__global__ __launch_bounds__(64) void lz4mi_frame_index_kernel(const uint8_t* f, uint64_t len, uint32_t cap_blocks,
                                                               uint64_t* pay_off, uint32_t* size_word, int64_t* info) {
    if (threadIdx.x != 0) return;
    frames::index_frame(f, len, cap_blocks, pay_off, size_word, info);
}

// Stored blocks' bytes into the output (one wave per stored block; clipped at `cap`
// like the reference's result.set would throw past it: the caller checks first).
__global__ __launch_bounds__(64) void lz4mi_frame_stored_kernel(const uint8_t* f, uint64_t len, const uint64_t* s_in_off,
                                                                const uint32_t* s_len, const uint64_t* s_out_off,
                                                                uint8_t* out, uint64_t cap, uint32_t ns) {
    const uint32_t b = blockIdx.x;
    const int lane = threadIdx.x;
    if (b >= ns) return;
    const uint64_t src = s_in_off[b], dst = s_out_off[b];
    uint64_t n = s_len[b];
    if (src + n > len) n = src < len ? len - src : 0;      // subarray() clips at the frame end
    if (dst + n > cap) n = dst < cap ? cap - dst : 0;
    wave_copy(out + dst, f + src, n, lane);
}

}  // namespace lz4mi

extern "C" hipError_t lz4mi_launch_frame_scan(const uint8_t* f, uint64_t len, uint32_t cap_blocks, uint64_t* c_in_off,
                                              uint32_t* c_in_len, uint64_t* c_out_off, uint32_t* c_out_cap,
                                              uint64_t* s_in_off, uint32_t* s_len, uint64_t* s_out_off, uint32_t* c_idx,
                                              uint32_t* s_idx, int64_t* info, hipStream_t stream) {
    hipLaunchKernelGGL(lz4mi::lz4mi_frame_scan_kernel, dim3(1), dim3(64), 0, stream, f, len, cap_blocks, c_in_off,
                       c_in_len, c_out_off, c_out_cap, s_in_off, s_len, s_out_off, c_idx, s_idx, info);
    return hipGetLastError();
}

extern "C" hipError_t lz4mi_launch_frame_stored(const uint8_t* f, uint64_t len, const uint64_t* s_in_off,
                                                const uint32_t* s_len, const uint64_t* s_out_off, uint8_t* out,
                                                uint64_t cap, uint32_t ns, hipStream_t stream) {
    if (ns == 0) return hipSuccess;
    hipLaunchKernelGGL(lz4mi::lz4mi_frame_stored_kernel, dim3(ns), dim3(64), 0, stream, f, len, s_in_off, s_len,
                       s_out_off, out, cap, ns);
    return hipGetLastError();
}

extern "C" hipError_t lz4mi_launch_frame_pack(const uint8_t* raw, const uint64_t* raw_off, const uint32_t* raw_len,
                                              const uint8_t* comp, const uint64_t* comp_off, const uint32_t* comp_len,
                                              uint8_t* frame, const uint64_t* rec_off, uint32_t nblocks,
                                              uint64_t* pay_off, uint64_t* sum_off, uint32_t* pay_len,
                                              hipStream_t stream) {
    if (nblocks == 0) return hipSuccess;
    hipLaunchKernelGGL(lz4mi::lz4mi_frame_pack_kernel, dim3(nblocks), dim3(64), 0, stream, raw, raw_off, raw_len,
                       comp, comp_off, comp_len, frame, rec_off, nblocks, pay_off, sum_off, pay_len);
    return hipGetLastError();
}

extern "C" hipError_t lz4mi_launch_frame_index(const uint8_t* f, uint64_t len, uint32_t cap_blocks, uint64_t* pay_off,
                                               uint32_t* size_word, int64_t* info, hipStream_t stream) {
    hipLaunchKernelGGL(lz4mi::lz4mi_frame_index_kernel, dim3(1), dim3(64), 0, stream, f, len, cap_blocks, pay_off,
                       size_word, info);
    return hipGetLastError();
}
