// lpips.hip — everything of the VGG16 LPIPS distance and its image gradient that is not a convolution.
//
// The 13 convolutions (+ bias + ReLU) of the feature net and the 13 convolutions of its input gradient are launches of ide3d_modconv2d, the
// interior ReLU gradients are ide3d_modconv_act_backward; this file holds the streaming passes around them, all over dense NCHW fp32:
//   ide3d_lpips_prep / _backward     f x f area mean + affine (0..255 -> -1..1) + z-score in one pass; the adjoint broadcast;
//   ide3d_maxpool2                   2x2 stride-2 max, floor on odd sides, bit-equal to ATen's;
//   ide3d_lpips_stage_backward       max-pool backward + add of the tap's gradient + ReLU backward in one pass over the tap;
//   ide3d_maxpool2_relu_backward     the same pass without a tap (in front of a VGG19 pool);
//   ide3d_lpips_head                 channel norm, difference to the cached normalised target, lin-weighted sum, pixel mean: one launch per
//                                    tap (per-workgroup partial sums -> workspace) and ONE finishing launch for all taps; or normalise only;
//   ide3d_lpips_head_backward        the closed-form gradient of the same, one launch per tap.
// Lanes run along pixels (consecutive addresses), loops run over channels.  Pool and stage backward move 16 bytes per lane and row where
// the width is a multiple of 4 and the pointers are 16-byte aligned; the head kernels read one float per lane and channel (a wave reads 256
// contiguous bytes per channel) because their parallelism is pixels x 4 channel slices and the deep taps have few pixels; prep touches
// 3-channel images only.
// Deterministic: fixed-order sums inside a thread, across the 4 channel slices of a workgroup (LDS, slice order), across the 64 pixels of a
// workgroup (butterfly) and across workgroups and taps (the finishing launch); no atomics; bit-reproducible.  The sums are carried in
// float64 (an fp32 product is exact there), so the head agrees with a float64 evaluation of the same fp32 inputs to fp32 rounding.
// Plain fp32 / fp64 loads, stores and FMAs on the vector pipe (no packed fp32: the library is built without it); no matrix loop in this
// file, so section 4.2's exclusive residency does not apply.
#include "common.h"

namespace ide3d {

constexpr int kLpThreads = 256;
constexpr int kLpSlices = kLpThreads / 64;      // channel slices of a head workgroup, one wave each
constexpr int kLpPixels = 64;                    // pixels of a head workgroup
constexpr double kLpEps = 1e-10;                 // reference inversion/criteria/lpips/utils.py:6

// ---- prep ---------------------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kLpThreads)
lp_prep_kernel(const float* __restrict__ x, float* __restrict__ y, const float* __restrict__ mean, const float* __restrict__ stdv,
               int H, int W, int f, float in_scale, float in_shift, int64_t total) {
    const int oh = H / f, ow = W / f;
    const float inv_area = 1.f / (float)(f * f);
    for (int64_t i = (int64_t)blockIdx.x * kLpThreads + threadIdx.x; i < total; i += (int64_t)gridDim.x * kLpThreads) {
        const int ox = (int)(i % ow);
        const int64_t r = i / ow;
        const int oy = (int)(r % oh);
        const int64_t plane = r / oh;
        const int c = (int)(plane % 3);
        const float* __restrict__ src = x + (plane * H + (int64_t)oy * f) * W + (int64_t)ox * f;
        float acc = 0.f;
        for (int dy = 0; dy < f; ++dy)
            for (int dx = 0; dx < f; ++dx) acc += src[(int64_t)dy * W + dx];
        const float v = fmaf(acc * inv_area, in_scale, in_shift);
        y[i] = (v - mean[c]) / stdv[c];
    }
}

__global__ void __launch_bounds__(kLpThreads)
lp_prep_bwd_kernel(const float* __restrict__ dy, float* __restrict__ dx, const float* __restrict__ stdv, int H, int W, int f, float in_scale,
                   int64_t total) {
    const int oh = H / f, ow = W / f;
    const float k = in_scale / (float)(f * f);
    for (int64_t i = (int64_t)blockIdx.x * kLpThreads + threadIdx.x; i < total; i += (int64_t)gridDim.x * kLpThreads) {
        const int X = (int)(i % W);
        const int64_t r = i / W;
        const int Y = (int)(r % H);
        const int64_t plane = r / H;
        const int c = (int)(plane % 3);
        dx[i] = dy[(plane * oh + Y / f) * ow + X / f] * (k / stdv[c]);
    }
}

// ---- 2x2 max pool -----------------------------------------------------------------------------------------------------------------------------
// V4: w % 4 == 0 and 16-byte aligned x, 8-byte aligned y: one thread = two neighbouring windows (a float4 of each of the two rows).
template <bool V4>
__global__ void __launch_bounds__(kLpThreads)
lp_pool_kernel(const float* __restrict__ x, float* __restrict__ y, int h, int w, int64_t total) {
    const int ph = h / 2, pw = w / 2;
    const int cols = V4 ? pw / 2 : pw;
    for (int64_t i = (int64_t)blockIdx.x * kLpThreads + threadIdx.x; i < total; i += (int64_t)gridDim.x * kLpThreads) {
        const int cx = (int)(i % cols);
        const int64_t r = i / cols;
        const int py = (int)(r % ph);
        const int64_t plane = r / ph;
        const float* __restrict__ r0 = x + (plane * h + 2 * py) * (int64_t)w;
        float* __restrict__ o = y + (plane * ph + py) * (int64_t)pw;
        if (V4) {
            const float4 a = *reinterpret_cast<const float4*>(r0 + 4 * cx);
            const float4 b = *reinterpret_cast<const float4*>(r0 + w + 4 * cx);
            float m0 = a.x, m1 = a.z;
            if (pool_gt(a.y, m0)) m0 = a.y;
            if (pool_gt(b.x, m0)) m0 = b.x;
            if (pool_gt(b.y, m0)) m0 = b.y;
            if (pool_gt(a.w, m1)) m1 = a.w;
            if (pool_gt(b.z, m1)) m1 = b.z;
            if (pool_gt(b.w, m1)) m1 = b.w;
            *reinterpret_cast<float2*>(o + 2 * cx) = make_float2(m0, m1);
        } else {
            float m = r0[2 * cx];
            if (pool_gt(r0[2 * cx + 1], m)) m = r0[2 * cx + 1];
            if (pool_gt(r0[w + 2 * cx], m)) m = r0[w + 2 * cx];
            if (pool_gt(r0[w + 2 * cx + 1], m)) m = r0[w + 2 * cx + 1];
            o[cx] = m;
        }
    }
}

// ---- stage backward -------------------------------------------------------------------------------------------------------------------------
// One 2x2 cell of the tap: dz = (route(gp) + dtap) where y > 0, else 0.  `pooled`: the cell is a window of the pool (all four pixels exist and
// the stage has a pool behind it); the pooled gradient goes to the window's first maximum in row-major order.  Which of several equal maxima
// receives it cannot matter: y >= 0 after the ReLU, so a tie at the maximum with a positive value is a measure-zero coincidence of two
// different convolution outputs, and a tie at 0 is masked.  Without HAS_TAP the t's are not read and the routed value is stored as it is (no
// `+ 0.f`, so a -0.f stays -0.f); a cell that is no window is written as 0.
template <bool HAS_TAP>
__device__ __forceinline__ void lp_cell(float v00, float v01, float v10, float v11, float t00, float t01, float t10, float t11, bool pooled,
                                        float gp, float& d00, float& d01, float& d10, float& d11) {
    int idx = 0;
    float m = v00;
    if (pool_gt(v01, m)) { m = v01; idx = 1; }
    if (pool_gt(v10, m)) { m = v10; idx = 2; }
    if (pool_gt(v11, m)) { m = v11; idx = 3; }
    if (!pooled) idx = -1;
    if (HAS_TAP) {
        d00 = v00 > 0.f ? t00 + (idx == 0 ? gp : 0.f) : 0.f;
        d01 = v01 > 0.f ? t01 + (idx == 1 ? gp : 0.f) : 0.f;
        d10 = v10 > 0.f ? t10 + (idx == 2 ? gp : 0.f) : 0.f;
        d11 = v11 > 0.f ? t11 + (idx == 3 ? gp : 0.f) : 0.f;
    } else {
        d00 = (idx == 0 && v00 > 0.f) ? gp : 0.f;
        d01 = (idx == 1 && v01 > 0.f) ? gp : 0.f;
        d10 = (idx == 2 && v10 > 0.f) ? gp : 0.f;
        d11 = (idx == 3 && v11 > 0.f) ? gp : 0.f;
    }
}

// Cells cover ceil(h / 2) x ceil(w / 2): the last row / column of an odd side is a cell without a window and receives dtap only.
// V4 (w % 4 == 0, 16-byte aligned y, dtap and dz, 8-byte aligned dpool): one thread = two neighbouring cells.
// HAS_TAP false (ide3d_maxpool2_relu_backward): dtap is NULL and never read.
template <bool V4, bool HAS_TAP>
__global__ void __launch_bounds__(kLpThreads)
lp_stage_bwd_kernel(const float* __restrict__ y, const float* __restrict__ dpool, const float* __restrict__ dtap, float* __restrict__ dz,
                    int h, int w, int64_t total) {
    const int ph = h / 2, pw = w / 2, ch = (h + 1) / 2, cw = (w + 1) / 2;
    const int cols = V4 ? cw / 2 : cw;
    for (int64_t i = (int64_t)blockIdx.x * kLpThreads + threadIdx.x; i < total; i += (int64_t)gridDim.x * kLpThreads) {
        const int cx = (int)(i % cols);
        const int64_t r = i / cols;
        const int cy = (int)(r % ch);
        const int64_t plane = r / ch;
        const bool row1 = 2 * cy + 1 < h;
        const int64_t e0 = (plane * h + 2 * cy) * (int64_t)w;
        const float* __restrict__ gp = dpool ? dpool + (plane * ph + cy) * (int64_t)pw : nullptr;      // (read only where cy < ph)
        if (V4) {
            const int64_t e = e0 + 4 * cx;
            const float4 z4 = make_float4(0.f, 0.f, 0.f, 0.f);
            const float4 a = *reinterpret_cast<const float4*>(y + e), ta = HAS_TAP ? *reinterpret_cast<const float4*>(dtap + e) : z4;
            const float4 b = row1 ? *reinterpret_cast<const float4*>(y + e + w) : z4;
            const float4 tb = (HAS_TAP && row1) ? *reinterpret_cast<const float4*>(dtap + e + w) : z4;
            const bool pooled = gp != nullptr && row1;
            const float2 g = pooled ? *reinterpret_cast<const float2*>(gp + 2 * cx) : make_float2(0.f, 0.f);
            float4 da, db;
            lp_cell<HAS_TAP>(a.x, a.y, b.x, b.y, ta.x, ta.y, tb.x, tb.y, pooled, g.x, da.x, da.y, db.x, db.y);
            lp_cell<HAS_TAP>(a.z, a.w, b.z, b.w, ta.z, ta.w, tb.z, tb.w, pooled, g.y, da.z, da.w, db.z, db.w);
            *reinterpret_cast<float4*>(dz + e) = da;
            if (row1) *reinterpret_cast<float4*>(dz + e + w) = db;
        } else {
            const int64_t e = e0 + 2 * cx;
            const bool col1 = 2 * cx + 1 < w;
            const float v00 = y[e], t00 = HAS_TAP ? dtap[e] : 0.f;
            const float v01 = col1 ? y[e + 1] : 0.f, t01 = (HAS_TAP && col1) ? dtap[e + 1] : 0.f;
            const float v10 = row1 ? y[e + w] : 0.f, t10 = (HAS_TAP && row1) ? dtap[e + w] : 0.f;
            const float v11 = (row1 && col1) ? y[e + w + 1] : 0.f, t11 = (HAS_TAP && row1 && col1) ? dtap[e + w + 1] : 0.f;
            const bool pooled = gp != nullptr && row1 && col1;
            const float g = pooled ? gp[cx] : 0.f;
            float d00, d01, d10, d11;
            lp_cell<HAS_TAP>(v00, v01, v10, v11, t00, t01, t10, t11, pooled, g, d00, d01, d10, d11);
            dz[e] = d00;
            if (col1) dz[e + 1] = d01;
            if (row1) dz[e + w] = d10;
            if (row1 && col1) dz[e + w + 1] = d11;
        }
    }
}

// ---- head ---------------------------------------------------------------------------------------------------------------------------------------
// A head workgroup: 64 consecutive pixels of the flat [n, h * w] pixel index x 4 channel slices (wave s takes channels s, s + 4, ...).
struct LpPixel { bool valid; int64_t base; };          // base: element index of channel 0 of the pixel

__device__ __forceinline__ LpPixel lp_pixel(int C, int hw, int64_t pixels) {
    LpPixel p;
    const int64_t i = (int64_t)blockIdx.x * kLpPixels + (threadIdx.x & 63);
    p.valid = i < pixels;
    const int64_t img = p.valid ? i / hw : 0;
    p.base = p.valid ? img * C * (int64_t)hw + (i - img * hw) : 0;
    return p;
}

// Sum of v over the 4 channel slices of a pixel, in slice order; every thread of the pixel receives it.  Ends with a barrier.
__device__ __forceinline__ double lp_slice_sum(double v, double (*s_red)[kLpPixels]) {
    s_red[threadIdx.x >> 6][threadIdx.x & 63] = v;
    __syncthreads();
    double t = s_red[0][threadIdx.x & 63];
#pragma unroll
    for (int s = 1; s < kLpSlices; ++s) t += s_red[s][threadIdx.x & 63];
    __syncthreads();
    return t;
}

// sum_c a_c^2 of the thread's pixel
__device__ __forceinline__ double lp_norm2(const float* __restrict__ a, const LpPixel& p, int C, int hw, double (*s_red)[kLpPixels]) {
    double acc = 0.0;
    if (p.valid)
        for (int c = threadIdx.x >> 6; c < C; c += kLpSlices) { const double v = (double)a[p.base + (int64_t)c * hw]; acc = fma(v, v, acc); }
    return lp_slice_sum(acc, s_red);
}

// NORM_ONLY: out = a / (|a| + eps).  Else: partial[workgroup] = sum over its pixels of sum_c lin_c (a_c / (|a| + eps) - t_c)^2.
template <bool NORM_ONLY>
__global__ void __launch_bounds__(kLpThreads)
lp_head_kernel(const float* __restrict__ a, const float* __restrict__ t, const float* __restrict__ lin, float* __restrict__ out,
               double* __restrict__ partial, int C, int hw, int64_t pixels) {
    __shared__ double s_red[kLpSlices][kLpPixels];
    const LpPixel p = lp_pixel(C, hw, pixels);
    const double n2 = lp_norm2(a, p, C, hw, s_red);
    const float inv = (float)(1.0 / (sqrt(n2) + kLpEps));
    if (NORM_ONLY) {
        if (p.valid)
            for (int c = threadIdx.x >> 6; c < C; c += kLpSlices) out[p.base + (int64_t)c * hw] = a[p.base + (int64_t)c * hw] * inv;
        return;
    }
    double acc = 0.0;
    if (p.valid)
        for (int c = threadIdx.x >> 6; c < C; c += kLpSlices) {
            const int64_t e = p.base + (int64_t)c * hw;
            const double d = (double)(a[e] * inv - t[e]);
            acc = fma((double)lin[c] * d, d, acc);
        }
    double s = lp_slice_sum(acc, s_red);
    if (threadIdx.x < 64) {
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off);
        if (threadIdx.x == 0) partial[blockIdx.x] = s;
    }
}

struct LpFinish { int k; int count[IDE3D_LPIPS_MAX_TAPS]; int offset[IDE3D_LPIPS_MAX_TAPS]; double scale[IDE3D_LPIPS_MAX_TAPS]; };

// loss = sum over taps (in order) of scale_k * sum of the tap's partials: thread i takes partials i, i + 256, ... of every tap, thread 0 adds
// the 256 thread sums in index order.
__global__ void __launch_bounds__(kLpThreads)
lp_finish_kernel(const double* __restrict__ partial, LpFinish f, float* __restrict__ loss) {
    __shared__ double s_acc[kLpThreads];
    double acc = 0.0;
    for (int k = 0; k < f.k; ++k) {
        double t = 0.0;
        for (int i = threadIdx.x; i < f.count[k]; i += kLpThreads) t += partial[f.offset[k] + i];
        acc = fma(t, f.scale[k], acc);
    }
    s_acc[threadIdx.x] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        double t = 0.0;
        for (int i = 0; i < kLpThreads; ++i) t += s_acc[i];
        loss[0] = (float)t;
    }
}

// da_c = g_c / (n + eps) - a_c (sum_k g_k a_k) / (n (n + eps)^2), g_c = s lin_c (u_c - t_c), s = 2 dloss / (N h w); the second term is 0
// where n = 0 (the reference's autograd gives NaN there: sqrt at 0).
__global__ void __launch_bounds__(kLpThreads)
lp_head_bwd_kernel(const float* __restrict__ a, const float* __restrict__ t, const float* __restrict__ lin, const float* __restrict__ dloss,
                   float* __restrict__ da, int C, int hw, int64_t pixels, double inv_count) {
    __shared__ double s_red[kLpSlices][kLpPixels];
    const LpPixel p = lp_pixel(C, hw, pixels);
    const double n2 = lp_norm2(a, p, C, hw, s_red);
    const double n = sqrt(n2);
    const float inv = (float)(1.0 / (n + kLpEps));
    const float s = (float)(2.0 * (double)dloss[0] * inv_count);
    double acc = 0.0;
    if (p.valid)
        for (int c = threadIdx.x >> 6; c < C; c += kLpSlices) {
            const int64_t e = p.base + (int64_t)c * hw;
            const float av = a[e];
            const float g = s * lin[c] * (av * inv - t[e]);
            acc = fma((double)g, (double)av, acc);
        }
    const double dot = lp_slice_sum(acc, s_red);
    const float coef = n > 0.0 ? (float)(dot / (n * (n + kLpEps) * (n + kLpEps))) : 0.f;
    if (p.valid)
        for (int c = threadIdx.x >> 6; c < C; c += kLpSlices) {
            const int64_t e = p.base + (int64_t)c * hw;
            const float av = a[e];
            const float g = s * lin[c] * (av * inv - t[e]);
            da[e] = g * inv - av * coef;
        }
}

static bool lp_taps_ok(const ide3d_lpips_tap* taps, int32_t k, int32_t n, int64_t* blocks_total) {
    if (!taps || k < 1 || k > IDE3D_LPIPS_MAX_TAPS || n < 1) return false;
    int64_t total = 0;
    for (int i = 0; i < k; ++i) {
        const ide3d_lpips_tap& t = taps[i];
        if (t.c < 1 || t.h < 1 || t.w < 1) return false;
        const int64_t hw = (int64_t)t.h * t.w;
        if (hw > 0x7fffffffLL || (int64_t)n * t.c * hw > (1LL << 40)) return false;
        total += cdiv64((int64_t)n * hw, kLpPixels);
    }
    if (total > 0x7fffffffLL) return false;
    if (blocks_total) *blocks_total = total;
    return true;
}

// The 16-byte form where the width is a multiple of 4 and every pointer it moves vectors through is aligned (a NULL dpool or dtap counts as
// aligned); the scalar form otherwise.
template <bool HAS_TAP>
static void lp_stage_launch(const float* y, const float* dpool, const float* dtap, float* dz, int64_t planes, int h, int w, hipStream_t st) {
    const int ch = (h + 1) / 2, cw = (w + 1) / 2;
    if (w % 4 == 0 && ptr_aligned(y, 16) && ptr_aligned(dtap, 16) && ptr_aligned(dz, 16) && ptr_aligned(dpool, 8)) {
        const int64_t total = planes * ch * (cw / 2);
        hipLaunchKernelGGL((lp_stage_bwd_kernel<true, HAS_TAP>), dim3(stream_grid(total, kLpThreads)), dim3(kLpThreads), 0, st, y, dpool, dtap, dz, h,
                           w, total);
    } else {
        const int64_t total = planes * ch * cw;
        hipLaunchKernelGGL((lp_stage_bwd_kernel<false, HAS_TAP>), dim3(stream_grid(total, kLpThreads)), dim3(kLpThreads), 0, st, y, dpool, dtap, dz, h,
                           w, total);
    }
}

}  // namespace ide3d

using namespace ide3d;

extern "C" int ide3d_lpips_prep(const float* x, float* y, const float* mean, const float* std_, int32_t n, int32_t H, int32_t W, int32_t f,
                                float in_scale, float in_shift, void* stream) {
    IDE3D_CHECK_ARG(x && y && mean && std_, "lpips_prep: null pointer");
    IDE3D_CHECK_ARG(n >= 1 && H >= 1 && W >= 1 && f >= 1 && f <= 64 && H % f == 0 && W % f == 0,
                    "lpips_prep: [n, 3, H, W] with an integer area factor f in 1..64 that divides H and W");
    const int64_t total = (int64_t)n * 3 * (H / f) * (W / f);
    IDE3D_CHECK_ARG((int64_t)n * 3 * H * W < (1LL << 40), "lpips_prep: image too large");
    hipLaunchKernelGGL(lp_prep_kernel, dim3(stream_grid(total, kLpThreads)), dim3(kLpThreads), 0, (hipStream_t)stream, x, y, mean, std_, H, W, f,
                       in_scale, in_shift, total);
    IDE3D_CHECK_LAUNCH("lpips_prep");
    return IDE3D_OK;
}

extern "C" int ide3d_lpips_prep_backward(const float* dy, float* dx, const float* std_, int32_t n, int32_t H, int32_t W, int32_t f,
                                         float in_scale, void* stream) {
    IDE3D_CHECK_ARG(dy && dx && std_, "lpips_prep_backward: null pointer");
    IDE3D_CHECK_ARG(n >= 1 && H >= 1 && W >= 1 && f >= 1 && f <= 64 && H % f == 0 && W % f == 0,
                    "lpips_prep_backward: [n, 3, H, W] with an integer area factor f in 1..64 that divides H and W");
    const int64_t total = (int64_t)n * 3 * H * W;
    IDE3D_CHECK_ARG(total < (1LL << 40), "lpips_prep_backward: image too large");
    hipLaunchKernelGGL(lp_prep_bwd_kernel, dim3(stream_grid(total, kLpThreads)), dim3(kLpThreads), 0, (hipStream_t)stream, dy, dx, std_, H, W, f,
                       in_scale, total);
    IDE3D_CHECK_LAUNCH("lpips_prep_backward");
    return IDE3D_OK;
}

extern "C" int ide3d_maxpool2(const float* x, float* y, int64_t planes, int32_t h, int32_t w, void* stream) {
    IDE3D_CHECK_ARG(x && y, "maxpool2: null pointer");
    IDE3D_CHECK_ARG(planes >= 1 && h >= 2 && w >= 2 && planes * h * w < (1LL << 40), "maxpool2: [planes, h, w] with h, w >= 2");
    hipStream_t st = (hipStream_t)stream;
    if (w % 4 == 0 && ptr_aligned(x, 16) && ptr_aligned(y, 8)) {
        const int64_t total = planes * (h / 2) * (w / 4);
        hipLaunchKernelGGL(lp_pool_kernel<true>, dim3(stream_grid(total, kLpThreads)), dim3(kLpThreads), 0, st, x, y, h, w, total);
    } else {
        const int64_t total = planes * (h / 2) * (w / 2);
        hipLaunchKernelGGL(lp_pool_kernel<false>, dim3(stream_grid(total, kLpThreads)), dim3(kLpThreads), 0, st, x, y, h, w, total);
    }
    IDE3D_CHECK_LAUNCH("maxpool2");
    return IDE3D_OK;
}

extern "C" int ide3d_lpips_stage_backward(const float* y, const float* dpool, const float* dtap, float* dz, int64_t planes, int32_t h, int32_t w,
                                          void* stream) {
    IDE3D_CHECK_ARG(y && dtap && dz, "lpips_stage_backward: null pointer");
    IDE3D_CHECK_ARG(planes >= 1 && h >= 1 && w >= 1 && planes * h * w < (1LL << 40), "lpips_stage_backward: [planes, h, w]");
    IDE3D_CHECK_ARG(dpool == nullptr || (h >= 2 && w >= 2), "lpips_stage_backward: a pooled gradient needs h, w >= 2");
    lp_stage_launch<true>(y, dpool, dtap, dz, planes, h, w, (hipStream_t)stream);
    IDE3D_CHECK_LAUNCH("lpips_stage_backward");
    return IDE3D_OK;
}

extern "C" int ide3d_maxpool2_relu_backward(const float* y, const float* dpool, float* dz, int64_t planes, int32_t h, int32_t w, void* stream) {
    IDE3D_CHECK_ARG(y && dpool && dz, "maxpool2_relu_backward: null pointer");
    IDE3D_CHECK_ARG(planes >= 1 && h >= 2 && w >= 2 && planes * h * w < (1LL << 40), "maxpool2_relu_backward: [planes, h, w] with h, w >= 2");
    lp_stage_launch<false>(y, dpool, nullptr, dz, planes, h, w, (hipStream_t)stream);
    IDE3D_CHECK_LAUNCH("maxpool2_relu_backward");
    return IDE3D_OK;
}

extern "C" int64_t ide3d_lpips_head_workspace_bytes(const ide3d_lpips_tap* taps, int32_t k, int32_t n) {
    int64_t blocks = 0;
    if (!lp_taps_ok(taps, k, n, &blocks)) return -1;
    return blocks * (int64_t)sizeof(double);
}

extern "C" int ide3d_lpips_head(const ide3d_lpips_tap* taps, int32_t k, int32_t n, float* workspace, int64_t workspace_bytes, float* loss,
                                void* stream) {
    int64_t blocks = 0;
    IDE3D_CHECK_ARG(lp_taps_ok(taps, k, n, &blocks), "lpips_head: 1..%d taps [n, c, h, w] with positive sizes", IDE3D_LPIPS_MAX_TAPS);
    hipStream_t st = (hipStream_t)stream;
    if (loss == nullptr) {                                  // normalise only
        for (int i = 0; i < k; ++i) IDE3D_CHECK_ARG(taps[i].a && taps[i].out, "lpips_head: the normalise-only form needs a and out of every tap");
        for (int i = 0; i < k; ++i) {
            const ide3d_lpips_tap& t = taps[i];
            const int64_t pixels = (int64_t)n * t.h * t.w;
            hipLaunchKernelGGL(lp_head_kernel<true>, dim3((unsigned)cdiv64(pixels, kLpPixels)), dim3(kLpThreads), 0, st, t.a, (const float*)nullptr,
                               (const float*)nullptr, t.out, (double*)nullptr, t.c, t.h * t.w, pixels);
        }
        IDE3D_CHECK_LAUNCH("lpips_head");
        return IDE3D_OK;
    }
    for (int i = 0; i < k; ++i) IDE3D_CHECK_ARG(taps[i].a && taps[i].t && taps[i].lin, "lpips_head: a, t and lin of every tap");
    IDE3D_CHECK_ARG(workspace && ptr_aligned(workspace, 8) && workspace_bytes >= blocks * (int64_t)sizeof(double), "lpips_head: workspace too small");
    double* partial = reinterpret_cast<double*>(workspace);
    LpFinish f;
    f.k = k;
    int64_t off = 0;
    for (int i = 0; i < k; ++i) {
        const ide3d_lpips_tap& t = taps[i];
        const int64_t pixels = (int64_t)n * t.h * t.w;
        const int64_t nb = cdiv64(pixels, kLpPixels);
        f.count[i] = (int)nb; f.offset[i] = (int)off; f.scale[i] = 1.0 / ((double)t.h * (double)t.w * (double)n);
        hipLaunchKernelGGL(lp_head_kernel<false>, dim3((unsigned)nb), dim3(kLpThreads), 0, st, t.a, t.t, t.lin, (float*)nullptr, partial + off, t.c,
                           t.h * t.w, pixels);
        off += nb;
    }
    hipLaunchKernelGGL(lp_finish_kernel, dim3(1), dim3(kLpThreads), 0, st, (const double*)partial, f, loss);
    IDE3D_CHECK_LAUNCH("lpips_head");
    return IDE3D_OK;
}

extern "C" int ide3d_lpips_head_backward(const ide3d_lpips_tap* taps, int32_t k, int32_t n, const float* dloss, void* stream) {
    IDE3D_CHECK_ARG(lp_taps_ok(taps, k, n, nullptr), "lpips_head_backward: 1..%d taps [n, c, h, w] with positive sizes", IDE3D_LPIPS_MAX_TAPS);
    IDE3D_CHECK_ARG(dloss != nullptr, "lpips_head_backward: null dloss");
    for (int i = 0; i < k; ++i) IDE3D_CHECK_ARG(taps[i].a && taps[i].t && taps[i].lin && taps[i].out, "lpips_head_backward: a, t, lin and out of every tap");
    hipStream_t st = (hipStream_t)stream;
    for (int i = 0; i < k; ++i) {
        const ide3d_lpips_tap& t = taps[i];
        const int64_t pixels = (int64_t)n * t.h * t.w;
        hipLaunchKernelGGL(lp_head_bwd_kernel, dim3((unsigned)cdiv64(pixels, kLpPixels)), dim3(kLpThreads), 0, st, t.a, t.t, t.lin, dloss, t.out, t.c,
                           t.h * t.w, pixels, 1.0 / ((double)t.h * (double)t.w * (double)n));
    }
    IDE3D_CHECK_LAUNCH("lpips_head_backward");
    return IDE3D_OK;
}
