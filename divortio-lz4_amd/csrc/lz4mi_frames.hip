// lz4mi_frames.hip — a batch of LZ4 frames decoded in one call (lz4mi_frames_index,
// lz4mi_frames_decompress; include/lz4mi.h).
//
// Only the walk inside one frame is serial (each record's position depends on the size word before
// it): different frames walk in parallel, one lane each, and the blocks of all of them go into one
// LZ4MI_FRAME_WORDS decode launch. Nothing is read back between the passes:
//   index:      count (lane per frame) -> scan of the counts (one workgroup, carried) -> fill (lane per
//               frame: the block lists) -> lz4mi_launch_sizes over the blocks to be measured -> sizes
//               (lane per frame: blk_size, the frame's total, totals[])
//   decompress: place (lane per frame: out_off / out_cap / the words the decoder sees) -> the batch
//               decode kernel -> finish (wave per frame: the frame's status, zero tail, hash list) ->
//               lz4mi_launch_xxh32 -> compare (lane per frame)
//               with LZ4MI_FRAMES_CHAINS the chain kernel (lz4mi_decompress.hip, wave per frame) runs between
//               the batch kernel and the finish: the place pass hides the blocks of the multi-block dependent
//               frames from the batch kernel (word 0), the chain decodes them in order, and with them every
//               other frame from its first block that reached below its own start
// The per-frame steps of the index are lz4mi_frames.h, shared with lz4mi_host_frames_index.
#include "lz4mi_common.h"
#include "lz4mi_frames.h"
#include "lz4mi_launch.h"

namespace lz4mi {
namespace frames {

constexpr int kScanThreads = 256;

__global__ __launch_bounds__(64) void lz4mi_frames_count_kernel(const uint8_t* in, const uint64_t* frame_off,
                                                                const uint64_t* frame_len, uint32_t nframes,
                                                                int64_t* finfo) {
    const uint32_t f = blockIdx.x * 64 + threadIdx.x;
    if (f >= nframes) return;
    count_frame(in + frame_off[f], frame_len[f], finfo + 8ull * f);
}

// Exclusive scan of the frames' listed block counts: finfo[f][kFirst], and the total in totals[0]
// (totals[1 .. 3] are zeroed for the sizes pass, which adds to them). One workgroup walks the frames
// kScanThreads at a time and carries the running sum.
__global__ __launch_bounds__(kScanThreads) void lz4mi_frames_scan_kernel(int64_t* finfo, uint32_t nframes,
                                                                         int64_t* totals) {
    __shared__ uint64_t part[kScanThreads];
    const int t = threadIdx.x;
    uint64_t carry = 0;
    for (uint32_t f0 = 0; f0 < nframes; f0 += kScanThreads) {
        const uint32_t f = f0 + t;
        const uint64_t c = f < nframes ? listed(finfo + 8ull * f) : 0;
        part[t] = c;
        __syncthreads();
        for (int d = 1; d < kScanThreads; d <<= 1) {   // inclusive, Hillis-Steele
            const uint64_t v = t >= d ? part[t - d] : 0;
            __syncthreads();
            part[t] += v;
            __syncthreads();
        }
        if (f < nframes) finfo[8ull * f + kFirst] = (int64_t)(carry + part[t] - c);
        carry += part[kScanThreads - 1];
        __syncthreads();
    }
    if (t == 0) {
        totals[0] = (int64_t)carry;
        totals[1] = totals[2] = totals[3] = 0;
    }
}

__global__ __launch_bounds__(64) void lz4mi_frames_fill_kernel(const uint8_t* in, const uint64_t* frame_off,
                                                               const uint64_t* frame_len, uint32_t nframes,
                                                               int64_t* finfo, uint64_t* blk_in_off, uint32_t* blk_word,
                                                               uint32_t* blk_frame, uint32_t* meas_word,
                                                               uint32_t cap_blocks, uint32_t flags) {
    const uint32_t f = blockIdx.x * 64 + threadIdx.x;
    if (f >= nframes) return;
    fill_frame(in + frame_off[f], frame_len[f], frame_off[f], f, finfo + 8ull * f, blk_in_off, blk_word, blk_frame,
               meas_word, cap_blocks, flags);
}

__device__ __forceinline__ uint64_t wave_sum(uint64_t v) {
    for (int o = 32; o; o >>= 1) v += (uint64_t)__shfl_xor((unsigned long long)v, o, 64);
    return v;
}

__global__ __launch_bounds__(64) void lz4mi_frames_sizes_kernel(int64_t* finfo, uint32_t nframes,
                                                                const uint32_t* blk_word, const uint32_t* msize,
                                                                const int32_t* mstatus, uint32_t* blk_size,
                                                                int64_t* totals) {
    const uint32_t f = blockIdx.x * 64 + threadIdx.x;
    uint64_t nlisted = 0, bytes = 0, declined = 0;
    if (f < nframes) {
        int64_t* fi = finfo + 8ull * f;
        size_frame(fi, blk_word, msize, mstatus, blk_size);
        nlisted = listed(fi);
        declined = fi[kDecline] ? 1 : 0;
        bytes = (!fi[kErr] && !fi[kDecline]) ? (uint64_t)fi[kTotal] : 0;
    }
    nlisted = wave_sum(nlisted);
    bytes = wave_sum(bytes);
    declined = wave_sum(declined);
    if (threadIdx.x == 0) {
        unsigned long long* t = (unsigned long long*)totals;
        if (nlisted) atomicAdd(t + 1, (unsigned long long)nlisted);
        if (bytes) atomicAdd(t + 2, (unsigned long long)bytes);
        if (declined) atomicAdd(t + 3, (unsigned long long)declined);
    }
}

// ---------------------------------------------------------------------------------------- decompress
// Is frame fi one the call decodes, with its blocks inside the lists?
__device__ __forceinline__ bool active(const int64_t* fi, uint32_t nblocks) {
    if (fi[kErr] || fi[kDecline]) return false;
    const uint64_t first = (uint64_t)fi[kFirst], n = (uint64_t)fi[kCount];
    return first <= nblocks && n <= nblocks - first;
}

// Is frame fi one whose blocks the chain kernel decodes from block 0 (LZ4MI_FRAMES_CHAINS)? The test of
// lz4mi_decompress_frames_chain_kernel.
__device__ __forceinline__ bool chain_frame(const int64_t* fi) { return !(fi[kHead] & 0x20) && fi[kCount] > 1; }

// Place pass. The caller has zeroed word / out_off / out_cap for all nblocks: a block of a frame that is
// not decoded stays a no-op (word 0, capacity 0: nothing is read or written for it). With LZ4MI_FRAMES_CHAINS
// the blocks of a chain frame keep word 0 (the batch kernel passes them over; the chain kernel and the finish
// pass read blk_word) and get their slots.
__global__ __launch_bounds__(64) void lz4mi_frames_place_kernel(int64_t* finfo, uint32_t nframes,
                                                                const uint32_t* blk_word, const uint32_t* blk_size,
                                                                uint32_t nblocks, const uint64_t* frame_out_off,
                                                                const uint64_t* frame_out_cap, uint32_t* word,
                                                                uint64_t* out_off, uint32_t* out_cap,
                                                                uint32_t flags) {
    const uint32_t f = blockIdx.x * 64 + threadIdx.x;
    if (f >= nframes) return;
    int64_t* fi = finfo + 8ull * f;
    if (fi[kErr] || fi[kDecline]) return;
    if (!active(fi, nblocks)) {
        fi[kDecline] = LZ4MI_FRAMES_DECLINE_CAP_BLOCKS;
        return;
    }
    // an unsized frame that was indexed without LZ4MI_JS_EXACT: a contiguous reference-mode decode would not give
    // the reference's window bytes (the index call declines it when it has the flag)
    if ((flags & LZ4MI_JS_EXACT) && !sized(fi)) {
        fi[kDecline] = LZ4MI_FRAMES_DECLINE_UNSIZED_EXACT;
        return;
    }
    const uint64_t total = (uint64_t)fi[kTotal];
    if (total > frame_out_cap[f]) {
        fi[kDecline] = LZ4MI_FRAMES_DECLINE_OUT_CAP;
        return;
    }
    if ((flags & LZ4MI_VERIFY_CONTENT) && (fi[kHead] & 0x04) && total > 0xFFFFFFFFull) {
        fi[kDecline] = LZ4MI_FRAMES_DECLINE_HASH_4G;
        return;
    }
    const uint64_t first = (uint64_t)fi[kFirst], n = (uint64_t)fi[kCount], base = frame_out_off[f];
    const bool chained = (flags & LZ4MI_FRAMES_CHAINS) && chain_frame(fi);
    uint64_t run = 0;
    for (uint64_t b = first; b < first + n; ++b) {
        const uint64_t sz = blk_size[b], left = total - run;
        word[b] = chained ? 0u : blk_word[b];
        out_off[b] = base + run;
        out_cap[b] = (uint32_t)(sz < left ? sz : left);   // never past the frame's total: a stored block that
        run += sz < left ? sz : left;                     // does not fit is the decoder's LZ4MI_ERR_RANGE
    }
}

// Finish pass: one wave per frame over its blocks' statuses and lengths, in block order. With
// LZ4MI_FRAMES_CHAINS (`word` is then blk_word) only the blocks up to and including the first failing one decide
// whether the frame is declined: behind it the chain left LZ4MI_ERR_CROSS_BLOCK and length 0 (the after-failure
// rule), which are no findings about the frame.
__global__ __launch_bounds__(64) void lz4mi_frames_finish_kernel(int64_t* finfo, uint32_t nframes, uint32_t nblocks,
                                                                 const uint32_t* word, const uint64_t* out_off,
                                                                 const uint32_t* out_cap, const uint32_t* out_len,
                                                                 const int32_t* status, uint8_t* out,
                                                                 const uint64_t* frame_out_off, uint64_t* hash_off,
                                                                 uint32_t* hash_len, uint32_t* hashed, uint32_t flags) {
    const uint32_t f = blockIdx.x;
    const int lane = threadIdx.x;
    if (f >= nframes) return;
    int64_t* fi = finfo + 8ull * f;
    if (lane == 0) {
        hash_off[f] = 0;
        hash_len[f] = 0;
        hashed[f] = 0;
    }
    if (!active(fi, nblocks)) return;
    const uint64_t first = (uint64_t)fi[kFirst], n = (uint64_t)fi[kCount], base = frame_out_off[f];
    const uint64_t size = (uint64_t)fi[kSize], total = (uint64_t)fi[kTotal];
    const bool measured = (fi[kHead] & kMeasured) != 0, has_size = sized(fi);
    const bool exact = (flags & LZ4MI_JS_EXACT) != 0, chains = (flags & LZ4MI_FRAMES_CHAINS) != 0;
    int32_t first_st = 0;
    bool dependent = false, layout = false;
    uint64_t written = 0;
    for (uint64_t k0 = 0; k0 < n; k0 += kWave) {
        const uint64_t k = k0 + lane;
        const bool valid = k < n;
        const uint64_t b = first + (valid ? k : 0);
        int32_t st = valid ? status[b] : 0;
        bool decides = valid;   // does the block count for the declines?
        if (chains) {
            const uint64_t bad = __ballot(valid && st != 0);
            decides = valid && !first_st && (!bad || lane <= __builtin_ctzll(bad));
        }
        const uint32_t ol = out_len[b], cap = out_cap[b], w = word[b];
        const uint64_t rel = out_off[b] - base;
        const bool stored = (w & 0x80000000u) != 0;
        // a back-reference below the block: into an earlier block of the frame (dependent blocks), or on the
        // frame's block 0 below the frame's start -- no dictionary, the result starts at position 0: the
        // reference's check 4. In a reference mode block 0 may also report its tail rewrite reading below the
        // frame (f1_changes): that frame is decoded alone.
        bool dep = decides && st == LZ4MI_ERR_CROSS_BLOCK && (k > 0 || exact);
        if (decides && st == LZ4MI_ERR_CROSS_BLOCK && !dep) st = LZ4MI_ERR_DICT_OOB;
        bool lay;
        if (measured) lay = decides && !dep && (st != 0 || ol != cap);   // the single-frame route's host cases
        else lay = decides && !stored && ((st == 0 && ol != cap && k != n - 1) ||
                                          (st == LZ4MI_ERR_OUTPUT_TOO_SMALL && rel + cap < size));
        dependent |= __ballot(dep) != 0;
        layout |= __ballot(lay) != 0;
        const uint64_t fail = __ballot(valid && st != 0);
        if (fail && !first_st) first_st = __shfl(st, __builtin_ctzll(fail), 64);
        uint64_t end = (valid && st == 0) ? rel + (stored ? (w & 0x7FFFFFFFu) : ol) : 0;
        for (int o = 32; o; o >>= 1) {
            const uint64_t v = (uint64_t)__shfl_xor((unsigned long long)end, o, 64);
            end = v > end ? v : end;
        }
        written = end > written ? end : written;
    }
    if (dependent || layout) {
        if (lane == 0) fi[kDecline] = dependent ? LZ4MI_FRAMES_DECLINE_DEPENDENT : LZ4MI_FRAMES_DECLINE_LAYOUT;
        return;
    }
    if (written > total) written = total;
    if (lane == 0) {
        fi[kErr] = first_st;
        fi[kTotal] = (int64_t)written;
    }
    if (first_st) return;
    // the reference's result is its zero-initialised content-size array
    if (has_size && written < size) wave_zero(out + base + written, size - written, lane);
    if ((flags & LZ4MI_VERIFY_CONTENT) && (fi[kHead] & 0x04) && lane == 0) {
        hash_off[f] = base;
        hash_len[f] = (uint32_t)total;
        hashed[f] = 1;
    }
}

__global__ __launch_bounds__(64) void lz4mi_frames_compare_kernel(int64_t* finfo, uint32_t nframes,
                                                                  const uint32_t* hashed, const uint32_t* digest) {
    const uint32_t f = blockIdx.x * 64 + threadIdx.x;
    if (f >= nframes || !hashed[f]) return;
    int64_t* fi = finfo + 8ull * f;
    if (digest[f] != (uint32_t)((uint64_t)fi[kHead] >> 32)) fi[kErr] = LZ4MI_ERR_CHECKSUM;
}

}  // namespace frames
}  // namespace lz4mi

using namespace lz4mi::frames;

extern "C" hipError_t lz4mi_launch_frames_index(const uint8_t* in, const uint64_t* frame_off, const uint64_t* frame_len,
                                                uint32_t nframes, uint64_t* blk_in_off, uint32_t* blk_word,
                                                uint32_t* blk_frame, uint32_t* blk_size, uint32_t cap_blocks,
                                                int64_t* finfo, int64_t* totals, uint32_t* meas_word, uint32_t* msize,
                                                int32_t* mstatus, uint32_t flags, hipStream_t stream) {
    const dim3 grid((nframes + 63) / 64), wave(64);
    if (nframes)
        hipLaunchKernelGGL(lz4mi_frames_count_kernel, grid, wave, 0, stream, in, frame_off, frame_len, nframes, finfo);
    hipLaunchKernelGGL(lz4mi_frames_scan_kernel, dim3(1), dim3(kScanThreads), 0, stream, finfo, nframes, totals);
    if (!nframes) return hipGetLastError();
    if (cap_blocks) {
        hipError_t e = hipMemsetAsync(meas_word, 0, 4ull * cap_blocks, stream);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(lz4mi_frames_fill_kernel, grid, wave, 0, stream, in, frame_off, frame_len, nframes, finfo,
                       blk_in_off, blk_word, blk_frame, meas_word, cap_blocks, flags);
    // always issued (no flag is read back to decide): word 0 gives size 0, status 0 and an immediate exit
    hipError_t e = lz4mi_launch_sizes(in, blk_in_off, meas_word, msize, mstatus, cap_blocks, 1, stream);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(lz4mi_frames_sizes_kernel, grid, wave, 0, stream, finfo, nframes, blk_word, msize, mstatus,
                       blk_size, totals);
    return hipGetLastError();
}

extern "C" hipError_t lz4mi_launch_frames_place(int64_t* finfo, uint32_t nframes, const uint32_t* blk_word,
                                                const uint32_t* blk_size, uint32_t nblocks,
                                                const uint64_t* frame_out_off, const uint64_t* frame_out_cap,
                                                uint32_t* word, uint64_t* out_off, uint32_t* out_cap, uint32_t flags,
                                                hipStream_t stream) {
    if (!nframes) return hipSuccess;
    hipLaunchKernelGGL(lz4mi_frames_place_kernel, dim3((nframes + 63) / 64), dim3(64), 0, stream, finfo, nframes,
                       blk_word, blk_size, nblocks, frame_out_off, frame_out_cap, word, out_off, out_cap, flags);
    return hipGetLastError();
}

extern "C" hipError_t lz4mi_launch_frames_finish(int64_t* finfo, uint32_t nframes, uint32_t nblocks,
                                                 const uint32_t* word, const uint64_t* out_off, const uint32_t* out_cap,
                                                 const uint32_t* out_len, const int32_t* status, uint8_t* out,
                                                 const uint64_t* frame_out_off, uint64_t* hash_off, uint32_t* hash_len,
                                                 uint32_t* hashed, uint32_t* digest, uint32_t flags,
                                                 hipStream_t stream) {
    if (!nframes) return hipSuccess;
    hipLaunchKernelGGL(lz4mi_frames_finish_kernel, dim3(nframes), dim3(64), 0, stream, finfo, nframes, nblocks, word,
                       out_off, out_cap, out_len, status, out, frame_out_off, hash_off, hash_len, hashed, flags);
    if (!(flags & LZ4MI_VERIFY_CONTENT)) return hipGetLastError();
    // the content checksum is the reference's XXH32 variant (standard = 0) of the frame's result: independent
    // chains, one quad of lanes per frame; a frame that is not hashed has length 0
    hipError_t e = lz4mi_launch_xxh32(out, hash_off, hash_len, 0, digest, nframes, 0, nullptr, nullptr, stream);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(lz4mi_frames_compare_kernel, dim3((nframes + 63) / 64), dim3(64), 0, stream, finfo, nframes,
                       hashed, digest);
    return hipGetLastError();
}
