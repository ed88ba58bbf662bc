// lz4mi_frames_enc.hip — a batch of buffers compressed into one LZ4 frame each in one call (lz4mi_frames_plan,
// lz4mi_frames_compress; include/lz4mi.h).
//
// Only the record walk inside one frame is serial (each record's position depends on the sizes before it):
// different frames walk in parallel, one lane each, and the blocks of all of them go into the batch encoder and
// are moved by one wave each. Nothing is read back between the passes:
//   plan:     count (lane per frame) -> scan of the block counts and slot bytes (one workgroup, carried) -> fill
//             (lane per frame: the block lists, totals[])
//   compress: prep (lane per frame: FLG, declines, the encoder's lists) -> the batch encoder, in slices, then with
//             LZ4MI_FRAMES_CHAINS the chains of the multi-block dependent frames, one workgroup per frame
//             (lz4mi_compress.hip; the caller of both: lz4mi_capi.cpp) -> size (lane per frame: the frame's
//             length; its slot in slot mode) -> position (packed mode: one workgroup, a carried scan of the lengths) -> write (lane per frame:
//             header, record positions, EndMark, hash list) -> pack (wave per block: size word and payload) ->
//             lz4mi_launch_xxh32 over the payloads (block checksums) and over the sources (content checksums)
// The per-frame steps are lz4mi_frames_enc.h, shared with lz4mi_host_frames_plan / lz4mi_host_frames_compress.
#include "lz4mi_common.h"
#include "lz4mi_frames_enc.h"
#include "lz4mi_launch.h"

namespace lz4mi {
namespace frames_enc {

// the carried scans' workgroup: every step waits for its loads, so the largest workgroup takes the fewest steps
constexpr int kScanThreads = 1024;

__device__ __forceinline__ uint64_t wave_sum(uint64_t v) {
    for (int o = 32; o; o >>= 1) v += (uint64_t)__shfl_xor((unsigned long long)v, o, 64);
    return v;
}

// Inclusive scan of one value per thread over the workgroup: a shuffle scan inside each wave, the waves' sums
// through LDS (wsum: one entry per wave). `total` gets the workgroup's sum. Every thread calls it.
__device__ __forceinline__ uint64_t group_scan(uint64_t* wsum, uint64_t c, int t, uint64_t& total) {
    const int lane = t & 63, w = t >> 6;
    uint64_t v = c;
    for (int d = 1; d < 64; d <<= 1) {
        const uint64_t u = (uint64_t)__shfl_up((unsigned long long)v, d, 64);
        if (lane >= d) v += u;
    }
    __syncthreads();   // (the call before this one has read wsum)
    if (lane == 63) wsum[w] = v;
    __syncthreads();
    uint64_t below = 0;
    total = 0;
    for (int k = 0; k < kScanThreads / 64; ++k) {
        const uint64_t s = wsum[k];
        if (k < w) below += s;
        total += s;
    }
    return v + below;
}

// ------------------------------------------------------------------------------------------------ plan
__global__ __launch_bounds__(64) void lz4mi_frames_plan_count_kernel(const uint64_t* src_len, uint32_t nframes,
                                                                     uint32_t bmax, uint32_t flags, int64_t* finfo) {
    const uint32_t f = blockIdx.x * 64 + threadIdx.x;
    if (f >= nframes) return;
    plan_count(src_len[f], bmax, flags, finfo + 8ull * f);
}

// Exclusive scans of the frames' listed block counts (finfo[f][kFirst]) and slot bytes (finfo[f][kPos], from
// kDump on; the fill clears it), the totals in totals[0] and totals[3]; totals[1 .. 2] are zeroed for the fill,
// which adds to them. One workgroup walks the frames kScanThreads at a time and carries the running sums.
__global__ __launch_bounds__(kScanThreads) void lz4mi_frames_plan_scan_kernel(int64_t* finfo, uint32_t nframes,
                                                                              int64_t* totals) {
    __shared__ uint64_t wsum[kScanThreads / 64];
    const int t = threadIdx.x;
    uint64_t blocks = 0, work = kDump;
    for (uint32_t f0 = 0; f0 < nframes; f0 += kScanThreads) {
        const uint32_t f = f0 + t;
        const uint64_t c = f < nframes ? listed(finfo + 8ull * f) : 0;
        const uint64_t w = f < nframes ? listed_work(finfo + 8ull * f) : 0;
        uint64_t csum, wtot;
        const uint64_t ci = group_scan(wsum, c, t, csum);
        const uint64_t wi = group_scan(wsum, w, t, wtot);
        if (f < nframes) {
            finfo[8ull * f + kFirst] = (int64_t)(blocks + ci - c);
            finfo[8ull * f + kPos] = (int64_t)(work + wi - w);
        }
        blocks += csum;
        work += wtot;
    }
    if (t == 0) {
        totals[0] = (int64_t)blocks;
        totals[1] = totals[2] = 0;
        totals[3] = (int64_t)work;
    }
}

__global__ __launch_bounds__(64) void lz4mi_frames_plan_fill_kernel(const uint64_t* src_off, uint32_t nframes,
                                                                    int64_t* finfo, uint64_t* blk_in_off,
                                                                    uint32_t* blk_len, uint32_t* blk_frame,
                                                                    uint64_t* blk_work_off, uint32_t cap_blocks,
                                                                    int64_t* totals) {
    const uint32_t f = blockIdx.x * 64 + threadIdx.x;
    uint64_t nlisted = 0, bytes = 0;
    if (f < nframes) {
        int64_t* fi = finfo + 8ull * f;
        plan_fill(src_off[f], f, fi, blk_in_off, blk_len, blk_frame, blk_work_off, cap_blocks);
        nlisted = listed(fi);
        bytes = fi[kDecline] ? 0 : (uint64_t)fi[kLen];
    }
    nlisted = wave_sum(nlisted);
    bytes = wave_sum(bytes);
    if (threadIdx.x == 0) {
        unsigned long long* t = (unsigned long long*)totals;
        if (nlisted) atomicAdd(t + 1, (unsigned long long)nlisted);
        if (bytes) atomicAdd(t + 2, (unsigned long long)bytes);
    }
}

// -------------------------------------------------------------------------------------------- compress
__global__ __launch_bounds__(64) void lz4mi_frames_enc_prep_kernel(int64_t* finfo, uint32_t nframes, uint32_t nblocks,
                                                                   const uint32_t* blk_len,
                                                                   const uint64_t* blk_work_off, uint64_t work_bytes,
                                                                   uint64_t* enc_off, uint32_t* enc_len,
                                                                   uint32_t flags) {
    const uint32_t f = blockIdx.x * 64 + threadIdx.x;
    if (f >= nframes) return;
    prep_frame(finfo + 8ull * f, nblocks, blk_len, blk_work_off, work_bytes, enc_off, enc_len, flags);
}

// slots: slot mode (frame_out_off / frame_out_cap are read), else the position pass follows
__global__ __launch_bounds__(64) void lz4mi_frames_enc_size_kernel(int64_t* finfo, uint32_t nframes,
                                                                   const uint32_t* blk_len, const uint32_t* comp_len,
                                                                   const uint64_t* frame_out_off,
                                                                   const uint64_t* frame_out_cap, uint64_t out_total,
                                                                   int slots) {
    const uint32_t f = blockIdx.x * 64 + threadIdx.x;
    if (f >= nframes) return;
    int64_t* fi = finfo + 8ull * f;
    size_frame(fi, blk_len, comp_len);
    if (slots) place_frame(fi, frame_out_off[f], frame_out_cap[f], out_total);
}

// Packed mode: finfo[f][kPos] = the exclusive scan of the lengths of the frames that are written. One workgroup
// walks the frames kScanThreads at a time and carries the position. A frame that would end behind out_total is
// declined and takes no room, so whether a frame fits depends on the frames before it: a group of frames that
// fits as a whole (every batch whose `out` was sized from the plan's totals[2]) is placed by the parallel scan,
// a group that does not is walked by one lane, frame after frame.
__global__ __launch_bounds__(kScanThreads) void lz4mi_frames_enc_position_kernel(int64_t* finfo, uint32_t nframes,
                                                                                 uint64_t out_total) {
    __shared__ uint64_t wsum[kScanThreads / 64];
    __shared__ uint64_t next;
    const int t = threadIdx.x;
    uint64_t at = 0;
    for (uint32_t f0 = 0; f0 < nframes; f0 += kScanThreads) {
        const uint32_t f = f0 + t;
        int64_t* fi = finfo + 8ull * (f < nframes ? f : 0);
        const bool live = f < nframes && !fi[kDecline];
        const uint64_t c = live ? (uint64_t)fi[kLen] : 0;
        uint64_t sum;
        const uint64_t ci = group_scan(wsum, c, t, sum);
        if (at <= out_total && sum <= out_total - at) {   // (uniform)
            if (live) fi[kPos] = (int64_t)(at + ci - c);
            at += sum;
        } else {
            if (t == 0) {
                uint64_t p = at;
                for (uint32_t g = f0; g < nframes && g < f0 + kScanThreads; ++g) p = pack_frame(finfo + 8ull * g, p, out_total);
                next = p;
            }
            __syncthreads();
            at = next;   // (rewritten only behind the next group_scan's barriers)
        }
    }
}

__global__ __launch_bounds__(64) void lz4mi_frames_enc_write_kernel(const int64_t* finfo, uint32_t nframes, uint8_t* out,
                                                                    const uint64_t* blk_in_off, const uint32_t* blk_len,
                                                                    const uint32_t* comp_len, uint64_t* rec_off,
                                                                    uint64_t* hash_off, uint32_t* hash_len,
                                                                    uint64_t* hash_dst) {
    const uint32_t f = blockIdx.x * 64 + threadIdx.x;
    if (f >= nframes) return;
    write_frame(finfo + 8ull * f, out, blk_in_off, blk_len, comp_len, rec_off, hash_off + f, hash_len + f, hash_dst + f);
}

// Pack pass: one wave per listed block whose frame is written (rec_off[b] != kNone): the record's size word and
// payload (wave_record; with block checksums the caller has set sum_off to kNone and pay_len to 0 for every
// block).
__global__ __launch_bounds__(64) void lz4mi_frames_enc_pack_kernel(const uint8_t* in, const uint64_t* blk_in_off,
                                                                   const uint32_t* blk_len, const uint8_t* work,
                                                                   const uint64_t* enc_off, const uint32_t* comp_len,
                                                                   const uint64_t* rec_off, uint32_t nblocks,
                                                                   uint8_t* out, uint64_t* pay_off, uint64_t* sum_off,
                                                                   uint32_t* pay_len) {
    const uint32_t b = blockIdx.x;
    const int lane = threadIdx.x;
    if (b >= nblocks) return;
    const uint64_t rec = rec_off[b];
    if (rec == kNone) return;
    const uint32_t n = blk_len[b], cl = comp_len[b];
    const bool st = stored(cl, n);
    wave_record(out, rec, st ? (n | 0x80000000u) : cl, st ? in + blk_in_off[b] : work + enc_off[b], st ? n : cl, b,
                pay_off, sum_off, pay_len, lane);
}

}  // namespace frames_enc
}  // namespace lz4mi

using namespace lz4mi::frames_enc;

extern "C" hipError_t lz4mi_launch_frames_plan(const uint64_t* src_off, const uint64_t* src_len, uint32_t nframes,
                                               uint32_t bmax, uint64_t* blk_in_off, uint32_t* blk_len,
                                               uint32_t* blk_frame, uint64_t* blk_work_off, uint32_t cap_blocks,
                                               int64_t* finfo, int64_t* totals, uint32_t flags, hipStream_t stream) {
    const dim3 grid((nframes + 63) / 64), wave(64);
    if (nframes)
        hipLaunchKernelGGL(lz4mi_frames_plan_count_kernel, grid, wave, 0, stream, src_len, nframes, bmax, flags, finfo);
    hipLaunchKernelGGL(lz4mi_frames_plan_scan_kernel, dim3(1), dim3(kScanThreads), 0, stream, finfo, nframes, totals);
    if (nframes)
        hipLaunchKernelGGL(lz4mi_frames_plan_fill_kernel, grid, wave, 0, stream, src_off, nframes, finfo, blk_in_off,
                           blk_len, blk_frame, blk_work_off, cap_blocks, totals);
    return hipGetLastError();
}

extern "C" hipError_t lz4mi_launch_frames_enc_prep(int64_t* finfo, uint32_t nframes, uint32_t nblocks,
                                                   const uint32_t* blk_len, const uint64_t* blk_work_off,
                                                   uint64_t work_bytes, uint64_t* enc_off, uint32_t* enc_len,
                                                   uint32_t flags, hipStream_t stream) {
    if (!nframes) return hipSuccess;
    hipLaunchKernelGGL(lz4mi_frames_enc_prep_kernel, dim3((nframes + 63) / 64), dim3(64), 0, stream, finfo, nframes,
                       nblocks, blk_len, blk_work_off, work_bytes, enc_off, enc_len, flags);
    return hipGetLastError();
}

extern "C" hipError_t lz4mi_launch_frames_enc_finish(const uint8_t* in, const uint64_t* blk_in_off,
                                                     const uint32_t* blk_len, uint32_t nblocks, int64_t* finfo,
                                                     uint32_t nframes, const uint8_t* work, const uint64_t* enc_off,
                                                     const uint32_t* comp_len, uint8_t* out, uint64_t out_total,
                                                     const uint64_t* frame_out_off, const uint64_t* frame_out_cap,
                                                     uint64_t* rec_off, uint64_t* pay_off, uint64_t* sum_off,
                                                     uint32_t* pay_len, uint64_t* hash_off, uint32_t* hash_len,
                                                     uint64_t* hash_dst, uint32_t flags, hipStream_t stream) {
    if (!nframes) return hipSuccess;
    const dim3 grid((nframes + 63) / 64), wave(64);
    const int slots = (flags & LZ4MI_FRAMES_PACKED) ? 0 : 1;
    hipLaunchKernelGGL(lz4mi_frames_enc_size_kernel, grid, wave, 0, stream, finfo, nframes, blk_len, comp_len,
                       frame_out_off, frame_out_cap, out_total, slots);
    if (!slots)
        hipLaunchKernelGGL(lz4mi_frames_enc_position_kernel, dim3(1), dim3(kScanThreads), 0, stream, finfo, nframes,
                           out_total);
    hipLaunchKernelGGL(lz4mi_frames_enc_write_kernel, grid, wave, 0, stream, finfo, nframes, out, blk_in_off, blk_len,
                       comp_len, rec_off, hash_off, hash_len, hash_dst);
    const bool sums = (flags & LZ4MI_BLOCK_CHECKSUM) != 0;
    if (nblocks)
        hipLaunchKernelGGL(lz4mi_frames_enc_pack_kernel, dim3(nblocks), wave, 0, stream, in, blk_in_off, blk_len, work,
                           enc_off, comp_len, rec_off, nblocks, out, sums ? pay_off : nullptr, sum_off, pay_len);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    // block checksums: the spec XXH32 of every payload behind it; a block that is not written has length 0 and no
    // place (kNone: lz4mi_launch_xxh32 stores nothing for it)
    if (sums) {
        e = lz4mi_launch_xxh32(out, pay_off, pay_len, 0, nullptr, nblocks, 1, out, sum_off, stream);
        if (e != hipSuccess) return e;
    }
    // content checksums: the reference's variant of every source behind its frame's EndMark, one chain per frame
    if (flags & LZ4MI_FRAMES_CONTENT_CHECKSUM)
        e = lz4mi_launch_xxh32(in, hash_off, hash_len, 0, nullptr, nframes, 0, out, hash_dst, stream);
    return e;
}
