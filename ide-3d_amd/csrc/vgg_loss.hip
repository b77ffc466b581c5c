// vgg_loss.hip — everything of the VGG19 feature loss and its image gradient that lpips.hip does not already hold.
//
// The 13 convolutions (+ bias + ReLU) of the feature net and the 13 of its input gradient are launches of ide3d_modconv2d, the interior ReLU
// gradients are ide3d_modconv_act_backward, the (x + 1) / 2 in front, its adjoint and the four pools are ide3d_lpips_prep, _prep_backward and
// ide3d_maxpool2 (lpips.hip), and the pass in front of a pool (max-pool backward + ReLU backward, never at a tap in VGG19) is
// ide3d_maxpool2_relu_backward, the tap-less form of ide3d_lpips_stage_backward's kernel (lpips.hip).  This file holds the two passes the L1
// distance adds, both over dense NCHW fp32:
//   ide3d_feat_l1                  sum_k weight_k mean |a_k - t_k|: one launch per tap (per-workgroup partial sums -> workspace) and ONE
//                                  finishing launch for all taps;
//   ide3d_feat_l1_tap_backward     at a tap: L1 backward (a sign times a per-tap constant) + add of the next convolution's input gradient +
//                                  ReLU backward in one pass, so that no tap gradient is ever written out and read back.
// The L1 sum and the tap backward are flat streams: 16 bytes per lane where the element count is a multiple of 4 (any width that is one)
// and the pointers are 16-byte aligned, one float per lane otherwise.  At most 256 CUs x 8 workgroups, grid-stride beyond.
// Deterministic: fixed-order sums inside a thread, across a wave (butterfly), across the 4 waves of a workgroup (LDS, wave order) and across
// workgroups and taps (the finishing launch); no atomics; bit-reproducible.  |a - t| and the sums are carried in float64 (an fp32 difference
// is exact there), so the loss agrees with a float64 evaluation of the same fp32 taps to the final rounding.
// Plain fp32 / fp64 loads, stores and adds on the vector pipe (no packed fp32: the library is built without it); no matrix loop in this
// file, so section 4.2's exclusive residency does not apply.
#include "common.h"

namespace ide3d {

constexpr int kVlThreads = 256;
constexpr int kVlWaves = kVlThreads / 64;
constexpr int kVlPerBlock = kVlThreads * 4;      // elements of one workgroup pass in either form of the flat kernels

// ---- L1 head ----------------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ double vl_abs_diff(float a, float t) { return fabs((double)a - (double)t); }

// partial[workgroup] = sum of |a - t| over the workgroup's elements.  V4: `items` float4s, else `items` floats.
template <bool V4>
__global__ void __launch_bounds__(kVlThreads)
vl_l1_kernel(const float* __restrict__ a, const float* __restrict__ t, double* __restrict__ partial, int64_t items) {
    __shared__ double s_wave[kVlWaves];
    double acc = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * kVlThreads + threadIdx.x; i < items; i += (int64_t)gridDim.x * kVlThreads) {
        if (V4) {
            const float4 av = reinterpret_cast<const float4*>(a)[i], tv = reinterpret_cast<const float4*>(t)[i];
            acc += vl_abs_diff(av.x, tv.x);
            acc += vl_abs_diff(av.y, tv.y);
            acc += vl_abs_diff(av.z, tv.z);
            acc += vl_abs_diff(av.w, tv.w);
        } else {
            acc += vl_abs_diff(a[i], t[i]);
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) acc += __shfl_xor(acc, off);
    if ((threadIdx.x & 63) == 0) s_wave[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        double s = s_wave[0];
#pragma unroll
        for (int i = 1; i < kVlWaves; ++i) s += s_wave[i];
        partial[blockIdx.x] = s;
    }
}

struct VlFinish { int k; int count[IDE3D_LPIPS_MAX_TAPS]; int offset[IDE3D_LPIPS_MAX_TAPS]; double scale[IDE3D_LPIPS_MAX_TAPS]; };

// loss = sum over taps (in order) of scale_k * sum of the tap's partials: thread i takes partials i, i + 256, ... of every tap, thread 0 adds
// the 256 thread sums in index order.
__global__ void __launch_bounds__(kVlThreads)
vl_finish_kernel(const double* __restrict__ partial, VlFinish f, float* __restrict__ loss) {
    __shared__ double s_acc[kVlThreads];
    double acc = 0.0;
    for (int k = 0; k < f.k; ++k) {
        double t = 0.0;
        for (int i = threadIdx.x; i < f.count[k]; i += kVlThreads) t += partial[f.offset[k] + i];
        acc = fma(t, f.scale[k], acc);
    }
    s_acc[threadIdx.x] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        double t = 0.0;
        for (int i = 0; i < kVlThreads; ++i) t += s_acc[i];
        loss[0] = (float)t;
    }
}

// ---- tap backward ---------------------------------------------------------------------------------------------------------------------------
// dz = (g + s sign(a - t)) where a > 0, else 0; sign(0) = 0.  s sign(.) is exact, so the sum rounds once, as ATen's add of the two does.
__device__ __forceinline__ float vl_tap(float a, float t, float g, float s) {
    const float l1 = a > t ? s : (a < t ? -s : 0.f);
    return a > 0.f ? g + l1 : 0.f;
}

template <bool V4, bool HAS_G>
__global__ void __launch_bounds__(kVlThreads)
vl_tap_bwd_kernel(const float* __restrict__ a, const float* __restrict__ t, const float* __restrict__ g, float* __restrict__ dz,
                  const float* __restrict__ dloss, double weight, double count, int64_t items) {
    const float s = (float)((double)dloss[0] * weight / count);          // ((dloss * weight) / count in float64, rounded once)
    for (int64_t i = (int64_t)blockIdx.x * kVlThreads + threadIdx.x; i < items; i += (int64_t)gridDim.x * kVlThreads) {
        if (V4) {
            const float4 av = reinterpret_cast<const float4*>(a)[i], tv = reinterpret_cast<const float4*>(t)[i];
            const float4 gv = HAS_G ? reinterpret_cast<const float4*>(g)[i] : make_float4(0.f, 0.f, 0.f, 0.f);
            reinterpret_cast<float4*>(dz)[i] = make_float4(vl_tap(av.x, tv.x, gv.x, s), vl_tap(av.y, tv.y, gv.y, s), vl_tap(av.z, tv.z, gv.z, s),
                                                           vl_tap(av.w, tv.w, gv.w, s));
        } else {
            dz[i] = vl_tap(a[i], t[i], HAS_G ? g[i] : 0.f, s);
        }
    }
}

// Workgroups of a flat pass over `elements` floats: one per kVlPerBlock elements up to the cap of stream_grid, the same in both forms (so
// that the workspace size does not depend on the pointers' alignment).
static int vl_flat_grid(int64_t elements) { return stream_grid(elements, kVlPerBlock); }

static bool vl_taps_ok(const ide3d_feat_l1_tap* taps, int32_t k, int32_t n, int64_t* blocks_total) {
    if (!taps || k < 1 || k > IDE3D_LPIPS_MAX_TAPS || n < 1) return false;
    int64_t total = 0;
    for (int i = 0; i < k; ++i) {
        const ide3d_feat_l1_tap& t = taps[i];
        if (t.c < 1 || t.h < 1 || t.w < 1) return false;
        const int64_t hw = (int64_t)t.h * t.w;
        if (hw > 0x7fffffffLL || (int64_t)n * t.c * hw > (1LL << 40)) return false;
        total += vl_flat_grid((int64_t)n * t.c * hw);
    }
    if (blocks_total) *blocks_total = total;
    return true;
}

}  // namespace ide3d

using namespace ide3d;

extern "C" int64_t ide3d_feat_l1_workspace_bytes(const ide3d_feat_l1_tap* taps, int32_t k, int32_t n) {
    int64_t blocks = 0;
    if (!vl_taps_ok(taps, k, n, &blocks)) return -1;
    return blocks * (int64_t)sizeof(double);
}

extern "C" int ide3d_feat_l1(const ide3d_feat_l1_tap* taps, int32_t k, int32_t n, float* workspace, int64_t workspace_bytes, float* loss,
                             void* stream) {
    int64_t blocks = 0;
    IDE3D_CHECK_ARG(vl_taps_ok(taps, k, n, &blocks), "feat_l1: 1..%d taps [n, c, h, w] with positive sizes", IDE3D_LPIPS_MAX_TAPS);
    IDE3D_CHECK_ARG(loss != nullptr, "feat_l1: null loss");
    for (int i = 0; i < k; ++i) IDE3D_CHECK_ARG(taps[i].a && taps[i].t, "feat_l1: a and t of every tap");
    IDE3D_CHECK_ARG(workspace && ptr_aligned(workspace, 8) && workspace_bytes >= blocks * (int64_t)sizeof(double), "feat_l1: workspace too small");
    hipStream_t st = (hipStream_t)stream;
    double* partial = reinterpret_cast<double*>(workspace);
    VlFinish f;
    f.k = k;
    int64_t off = 0;
    for (int i = 0; i < k; ++i) {
        const ide3d_feat_l1_tap& t = taps[i];
        const int64_t elements = (int64_t)n * t.c * t.h * t.w;
        const int nb = vl_flat_grid(elements);
        f.count[i] = nb; f.offset[i] = (int)off; f.scale[i] = (double)t.weight / (double)elements;
        if (elements % 4 == 0 && ptr_aligned(t.a, 16) && ptr_aligned(t.t, 16))
            hipLaunchKernelGGL(vl_l1_kernel<true>, dim3(nb), dim3(kVlThreads), 0, st, t.a, t.t, partial + off, elements / 4);
        else
            hipLaunchKernelGGL(vl_l1_kernel<false>, dim3(nb), dim3(kVlThreads), 0, st, t.a, t.t, partial + off, elements);
        off += nb;
    }
    hipLaunchKernelGGL(vl_finish_kernel, dim3(1), dim3(kVlThreads), 0, st, (const double*)partial, f, loss);
    IDE3D_CHECK_LAUNCH("feat_l1");
    return IDE3D_OK;
}

extern "C" int ide3d_feat_l1_tap_backward(const float* a, const float* t, const float* g, float* dz, const float* dloss, float weight,
                                          int64_t planes, int32_t h, int32_t w, int64_t count, void* stream) {
    IDE3D_CHECK_ARG(a && t && dz && dloss, "feat_l1_tap_backward: null pointer");
    IDE3D_CHECK_ARG(planes >= 1 && h >= 1 && w >= 1 && planes * h * w < (1LL << 40) && count >= 1, "feat_l1_tap_backward: [planes, h, w], count >= 1");
    hipStream_t st = (hipStream_t)stream;
    const int64_t elements = planes * h * w;
    const dim3 grid(vl_flat_grid(elements)), threads(kVlThreads);
    const double wt = (double)weight, cnt = (double)count;
    const bool v4 = elements % 4 == 0 && ptr_aligned(a, 16) && ptr_aligned(t, 16) && ptr_aligned(g, 16) && ptr_aligned(dz, 16);
    if (v4 && g)       hipLaunchKernelGGL((vl_tap_bwd_kernel<true, true>), grid, threads, 0, st, a, t, g, dz, dloss, wt, cnt, elements / 4);
    else if (v4)       hipLaunchKernelGGL((vl_tap_bwd_kernel<true, false>), grid, threads, 0, st, a, t, g, dz, dloss, wt, cnt, elements / 4);
    else if (g)        hipLaunchKernelGGL((vl_tap_bwd_kernel<false, true>), grid, threads, 0, st, a, t, g, dz, dloss, wt, cnt, elements);
    else               hipLaunchKernelGGL((vl_tap_bwd_kernel<false, false>), grid, threads, 0, st, a, t, g, dz, dloss, wt, cnt, elements);
    IDE3D_CHECK_LAUNCH("feat_l1_tap_backward");
    return IDE3D_OK;
}
