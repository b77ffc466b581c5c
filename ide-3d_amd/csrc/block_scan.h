// block_scan.h — the parts shared by the kernels whose output size depends on the data: the marching-cubes mesh
// (mesh.hip), the PNG zlib streams (png.hip) and the JPEG scans (jpeg.hip).  Many workgroups each produce a piece of unknown size into a slot
// of the workspace, one workgroup turns the sizes into positions, a compaction pass packs the pieces, the host reads the totals.
//
//   wave_inclusive_scan / block_exclusive_scan   the integer prefix sums (integers: any summation order gives the same bits)
//   segment_positions_kernel                     sizes of T segments in N frames -> pos[T], offsets[N + 1]
//   copy_slot_bytes                              16-byte-aligned slot -> any destination, 16 bytes per store
//   check_stream_buffers                         the buffer arguments of the two stream encoders' entry points
#pragma once

#include "common.h"

namespace ide3d {

constexpr int kScanThreads = 1024;          // the one workgroup of a scan over per-workgroup sizes

// v of the lane d below.  A scanned type of more than one word overloads it (mesh.hip).
template <class T>
__device__ __forceinline__ T lane_up(T v, int d) { return __shfl_up(v, d); }

// Inclusive prefix of v over the lanes of a wave, in lane order.
template <class T>
__device__ __forceinline__ T wave_inclusive_scan(T v) {
    const int lane = threadIdx.x & (kWave - 1);
#pragma unroll
    for (int d = 1; d < kWave; d <<= 1) {
        const T up = lane_up(v, d);
        if (lane >= d) v += up;
    }
    return v;
}

// Exclusive prefix of `value` over the THREADS threads of the workgroup in thread order, and the sum over all of them.  s_w: THREADS / kWave
// values of LDS.  Every thread calls it; it begins with the barrier that lets a caller use s_w again right after an earlier call.
// FRESH: the caller states that a barrier already lies between the last read of s_w (if any) and this call, and that barrier is left out
// (measured: with it the PNG launches were 0.3 - 0.9 % slower than before the scans were shared, profiles/png/refactor_ab.json).
template <int THREADS, bool FRESH = false, class T>
__device__ __forceinline__ T block_exclusive_scan(T value, T* s_w, T& total) {
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    const T inc = wave_inclusive_scan(value);
    if (!FRESH) __syncthreads();        // the previous call's readers are done with s_w
    if (lane == kWave - 1) s_w[wave] = inc;
    __syncthreads();
    T before{};
    total = T{};
#pragma unroll
    for (int i = 0; i < THREADS / kWave; ++i) {
        const T w = s_w[i];
        if (i < wave) before += w;
        total += w;
    }
    return before + inc - value;
}

// One workgroup of kScanThreads.  Segment i of T belongs to frame f = i / per_frame and holds sizes[i * size_stride_words] bytes.  A
// stream spends per_frame_bytes on every frame and per_segment_bytes between two segments of one frame, `lead` of the frame's bytes in
// front of its first segment.  With run(i) = the sizes of the segments before i:
//   pos[i]     = run(i) + per_frame_bytes f + per_segment_bytes (i - f) + lead          where segment i starts in `out`
//   offsets[f] = pos[f per_frame] - lead                                                where frame f starts
//   offsets[N] = run(T) + per_frame_bytes N + per_segment_bytes (T - N)                 the bytes used
// Thread t owns the contiguous range [t per, (t + 1) per) of the segments, clamped to T, per = ceil(T / kScanThreads).
static __global__ void __launch_bounds__(kScanThreads)
segment_positions_kernel(const unsigned* __restrict__ sizes, int size_stride_words, int64_t T, int64_t per_frame, int64_t N, int per_frame_bytes,
                         int per_segment_bytes, int lead, long long* __restrict__ pos, long long* __restrict__ offsets) {
    __shared__ long long s_w[kScanThreads / kWave];
    const int64_t per = cdiv64(T, kScanThreads);
    const int64_t lo = min((int64_t)threadIdx.x * per, T), hi = min(lo + per, T);
    long long sum = 0;
    for (int64_t i = lo; i < hi; ++i) sum += sizes[i * size_stride_words];
    long long total;
    long long run = block_exclusive_scan<kScanThreads, true>(sum, s_w, total);
    for (int64_t i = lo; i < hi; ++i) {
        const int64_t f = i / per_frame;
        const long long at = run + per_frame_bytes * f + per_segment_bytes * (i - f) + lead;
        pos[i] = at;
        if (i == f * per_frame) offsets[f] = at - lead;
        run += sizes[i * size_stride_words];
    }
    if (threadIdx.x == 0) offsets[N] = total + per_frame_bytes * N + per_segment_bytes * (T - N);
}

// 16 bytes starting `r` (0..15) bytes into the 32 bytes (a, b)
__device__ __forceinline__ uint4 shift_bytes(const uint4 a, const uint4 b, int r) {
    const unsigned w[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
    const unsigned sh = (unsigned)(r & 3);
    unsigned o[4];
    switch (r >> 2) {                                  // uniform over the workgroup
    case 0:
#pragma unroll
        for (int j = 0; j < 4; ++j) o[j] = __builtin_amdgcn_alignbyte(w[j + 1], w[j], sh);
        break;
    case 1:
#pragma unroll
        for (int j = 0; j < 4; ++j) o[j] = __builtin_amdgcn_alignbyte(w[j + 2], w[j + 1], sh);
        break;
    case 2:
#pragma unroll
        for (int j = 0; j < 4; ++j) o[j] = __builtin_amdgcn_alignbyte(w[j + 3], w[j + 2], sh);
        break;
    default:
#pragma unroll
        for (int j = 0; j < 4; ++j) o[j] = __builtin_amdgcn_alignbyte(w[j + 4], w[j + 3], sh);
        break;
    }
    return make_uint4(o[0], o[1], o[2], o[3]);
}

// slot[0, size) -> dst[0, size) by the nthreads (> 15) threads of a workgroup: the head up to the first 16-byte boundary of the destination,
// 16-byte groups, the tail.  `slot` is 16-byte aligned, `dst` is not bound to any alignment.  The groups are read as whole 16-byte words of
// the slot, one word ahead: the caller guarantees that slot[0, 16 ceil(size / 16) + 16) is readable.
__device__ __forceinline__ void copy_slot_bytes(uint8_t* __restrict__ dst, const uint8_t* __restrict__ slot, int size, int tid, int nthreads) {
    const int head = min(size, (int)((16 - (reinterpret_cast<uintptr_t>(dst) & 15)) & 15));
    const int groups = (size - head) >> 4;
    const int r = head & 15;                           // group k reads slot bytes [head + 16 k, +16): 16-byte aligned address + r
    if (tid < head) dst[tid] = slot[tid];
    for (int k = tid; k < groups; k += nthreads) {
        const uint8_t* const p = slot + (head - r) + 16 * k;
        const uint4 a = *reinterpret_cast<const uint4*>(p), b = *reinterpret_cast<const uint4*>(p + 16);   // p + 32 <= slot + size + 16
        *reinterpret_cast<uint4*>(dst + head + 16 * k) = shift_bytes(a, b, r);
    }
    const int tail0 = head + 16 * groups;
    if (tid < size - tail0) dst[tail0 + tid] = slot[tail0 + tid];
}

// The buffer arguments of a stream encoder's entry point `entry` ("png_encode", "jpeg_encode"): IDE3D_OK, or IDE3D_EINVAL with the error text set.
inline int check_stream_buffers(const char* entry, const void* frames, const void* workspace, int64_t workspace_bytes, int64_t workspace_need,
                                const void* out, int64_t out_capacity, int64_t worst_case, const void* offsets) {
    IDE3D_CHECK_ARG(frames && workspace && out && offsets, "%s: null pointer", entry);
    IDE3D_CHECK_ARG(workspace_bytes >= workspace_need && ptr_aligned(workspace, 16), "%s: workspace smaller than %lld bytes or not 16-byte aligned",
                    entry, (long long)workspace_need);
    IDE3D_CHECK_ARG(out_capacity >= worst_case && out_capacity < (1ll << 31), "%s: out holds %lld bytes, the worst case is %lld (and below 2 GiB)",
                    entry, (long long)out_capacity, (long long)worst_case);
    IDE3D_CHECK_ARG(ptr_aligned(offsets, 8), "%s: offsets must be 8-byte aligned", entry);
    return IDE3D_OK;
}

}  // namespace ide3d
