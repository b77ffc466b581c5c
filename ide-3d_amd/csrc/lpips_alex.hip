// lpips_alex.hip — what the AlexNet LPIPS distance and its image gradient need beside csrc/lpips.hip and the convolution kernel
// (DESIGN.md section 5.20).
//
// AlexNet's 11x11 stride-4 stem and its 5x5 convolution are launches of ide3d_modconv2d at k = 1 over unfolded patches; the input gradient
// of each is a 1x1 launch on the transposed weight followed by the adjoint of the unfolding.  This file holds the streaming passes around
// those launches, all over dense NCHW fp32:
//   ide3d_unfold2d             x [n, c, h, w] -> col [n, c k k, ho, wo], channel (ci k + ky) k + kx (F.unfold's order), zero outside the image;
//   ide3d_fold2d               its adjoint in gather form: every input pixel sums the <= ceil(k / stride)^2 patch entries that read it;
//   ide3d_maxpool3s2p0         MaxPool2d(3, 2) without padding (floor), ATen's tie rule, a byte winner index;
//   ide3d_lpips_tap_backward   at a tap: pool backward (or pass-through) + the tap's gradient + ReLU backward in one pass.
// One thread per output element, lanes along pixels of a row (consecutive addresses on the written side), grid-stride loops over a flat
// 64-bit index that is checked against its count, so any number of planes is one launch.
// Deterministic: every sum is taken inside one thread in a fixed order (fold: ky then kx ascending, carried in float64 and rounded once;
// tap backward: window rows then columns ascending, in fp32 as ATen does); no atomics; bit-reproducible.
// Plain fp32 / fp64 loads, stores and adds on the vector pipe (no packed fp32: the library is built without it); no matrix loop in this
// file, so section 4.2's exclusive residency does not apply.
#include "common.h"

namespace ide3d {

constexpr int kLaThreads = 256;
constexpr int kLaMaxK = 16;
constexpr int kLaMaxSide = 16384;          // index products (side x side) stay inside int32

struct LaGeom { int c, h, w, k, stride, pad, ho, wo; };

// ---- unfold -----------------------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kLaThreads)
la_unfold_kernel(const float* __restrict__ x, float* __restrict__ col, LaGeom g, int64_t total) {
    const int kk = g.k * g.k;
    for (int64_t i = (int64_t)blockIdx.x * kLaThreads + threadIdx.x; i < total; i += (int64_t)gridDim.x * kLaThreads) {
        const int ox = (int)(i % g.wo);
        int64_t r = i / g.wo;
        const int oy = (int)(r % g.ho);
        r /= g.ho;
        const int q = (int)(r % kk);            // ky k + kx
        r /= kk;                                // img c + ci
        const int ky = q / g.k, kx = q - ky * g.k;
        const int iy = oy * g.stride + ky - g.pad, ix = ox * g.stride + kx - g.pad;
        float v = 0.f;
        if (iy >= 0 && iy < g.h && ix >= 0 && ix < g.w) v = x[(r * g.h + iy) * (int64_t)g.w + ix];
        col[i] = v;
    }
}

// ---- fold -------------------------------------------------------------------------------------------------------------------------------------
// dx[ci, y, x] = sum over ky, kx (ascending) of dcol[(ci k + ky) k + kx, (y + pad - ky) / stride, (x + pad - kx) / stride] where both
// divisions are exact and the position lies inside ho x wo: ky runs over (y + pad) % stride, + stride, ...
__global__ void __launch_bounds__(kLaThreads)
la_fold_kernel(const float* __restrict__ dcol, float* __restrict__ dx, LaGeom g, int64_t total) {
    const int64_t howo = (int64_t)g.ho * g.wo;
    for (int64_t i = (int64_t)blockIdx.x * kLaThreads + threadIdx.x; i < total; i += (int64_t)gridDim.x * kLaThreads) {
        const int xx = (int)(i % g.w);
        const int64_t r = i / g.w;
        const int yy = (int)(r % g.h);
        const int64_t plane = r / g.h;          // img c + ci
        const float* __restrict__ p = dcol + plane * g.k * g.k * howo;
        double acc = 0.0;
        for (int ky = (yy + g.pad) % g.stride; ky < g.k; ky += g.stride) {
            const int ty = yy + g.pad - ky;
            if (ty < 0) break;                  // (ty falls as ky grows)
            const int oy = ty / g.stride;
            if (oy >= g.ho) continue;
            for (int kx = (xx + g.pad) % g.stride; kx < g.k; kx += g.stride) {
                const int tx = xx + g.pad - kx;
                if (tx < 0) break;
                const int ox = tx / g.stride;
                if (ox >= g.wo) continue;
                acc += (double)p[(int64_t)(ky * g.k + kx) * howo + (int64_t)oy * g.wo + ox];
            }
        }
        dx[i] = (float)acc;
    }
}

// ---- 3x3 stride-2 max pool without padding ---------------------------------------------------------------------------------------------------
// ATen's rule (as ide3d_maxpool3s2, csrc/parse_loss.hip): the running maximum starts at -inf with the window's first element as its index;
// v > max or v != v takes over, so the first maximum in row-major order wins and NaN wins.  Every window lies inside the plane (floor).
__global__ void __launch_bounds__(kLaThreads)
la_pool_kernel(const float* __restrict__ x, float* __restrict__ y, unsigned char* __restrict__ idx, int h, int w, int oh, int ow, int64_t total) {
    for (int64_t i = (int64_t)blockIdx.x * kLaThreads + threadIdx.x; i < total; i += (int64_t)gridDim.x * kLaThreads) {
        const int ox = (int)(i % ow);
        const int64_t r = i / ow;
        const int oy = (int)(r % oh);
        const int64_t plane = r / oh;
        const float* __restrict__ p = x + (plane * h + 2 * oy) * (int64_t)w + 2 * ox;
        float m = -INFINITY;
        int win = 0;
#pragma unroll
        for (int ky = 0; ky < 3; ++ky)
#pragma unroll
            for (int kx = 0; kx < 3; ++kx) {
                const float v = p[(int64_t)ky * w + kx];
                if (pool_gt(v, m)) { m = v; win = ky * 3 + kx; }
            }
        y[i] = m;
        if (idx) idx[i] = (unsigned char)win;
    }
}

// ---- tap backward -----------------------------------------------------------------------------------------------------------------------------
// dz = (route(g) + dtap) where y > 0, else 0.  POOLED: g [planes, oh, ow] is routed through the winner bytes: pixel (yy, xx) lies in the
// windows oy in [max(yy - 1, 0) / 2, min(yy / 2, oh - 1)] (columns likewise) and takes g where the window's winner is (yy - 2 oy) 3 + (xx - 2 ox);
// a row or column past the last window has an empty range.  Not POOLED: g [planes, h, w] is added as it is, or is NULL.
template <bool POOLED>
__global__ void __launch_bounds__(kLaThreads)
la_tap_bwd_kernel(const float* __restrict__ y, const float* __restrict__ g, const unsigned char* __restrict__ idx, const float* __restrict__ dtap,
                  float* __restrict__ dz, int h, int w, int oh, int ow, int64_t total) {
    for (int64_t i = (int64_t)blockIdx.x * kLaThreads + threadIdx.x; i < total; i += (int64_t)gridDim.x * kLaThreads) {
        float acc = 0.f;
        if (POOLED) {
            const int xx = (int)(i % w);
            const int64_t r = i / w;
            const int yy = (int)(r % h);
            const int64_t base = (r / h) * oh * (int64_t)ow;
            const int oy0 = max(yy - 1, 0) / 2, oy1 = min(yy / 2, oh - 1), ox0 = max(xx - 1, 0) / 2, ox1 = min(xx / 2, ow - 1);
            for (int oy = oy0; oy <= oy1; ++oy)
                for (int ox = ox0; ox <= ox1; ++ox) {
                    const int64_t o = base + (int64_t)oy * ow + ox;
                    if ((int)idx[o] == (yy - 2 * oy) * 3 + (xx - 2 * ox)) acc += g[o];
                }
        } else if (g != nullptr) {
            acc = g[i];
        }
        dz[i] = y[i] > 0.f ? acc + dtap[i] : 0.f;
    }
}

static bool la_geom(LaGeom& g, int32_t n, int32_t c, int32_t h, int32_t w, int32_t k, int32_t stride, int32_t pad) {
    if (n < 1 || c < 1 || h < 1 || w < 1 || h > kLaMaxSide || w > kLaMaxSide || k < 1 || k > kLaMaxK || stride < 1 || stride > k || pad < 0 || pad >= k)
        return false;
    if (h + 2 * pad < k || w + 2 * pad < k) return false;
    g.c = c; g.h = h; g.w = w; g.k = k; g.stride = stride; g.pad = pad;
    g.ho = (h + 2 * pad - k) / stride + 1;
    g.wo = (w + 2 * pad - k) / stride + 1;
    const int64_t lim = 0x7fffffffLL;
    return (int64_t)n * c * h * w <= lim && (int64_t)n * c * k * k * g.ho * g.wo <= lim;
}

#define LA_GEOM_TEXT "[n, c, h, w] with 1 <= k <= 16, 1 <= stride <= k, 0 <= pad < k, at least one window per side and fewer than 2^31 elements in x and in col"

}  // namespace ide3d

using namespace ide3d;

extern "C" int ide3d_unfold2d(const float* x, float* col, int32_t n, int32_t c, int32_t h, int32_t w, int32_t k, int32_t stride, int32_t pad,
                              void* stream) {
    IDE3D_CHECK_ARG(x && col, "unfold2d: null pointer");
    LaGeom g;
    IDE3D_CHECK_ARG(la_geom(g, n, c, h, w, k, stride, pad), "unfold2d: x " LA_GEOM_TEXT);
    const int64_t total = (int64_t)n * c * k * k * g.ho * g.wo;
    hipLaunchKernelGGL(la_unfold_kernel, dim3(stream_grid(total, kLaThreads)), dim3(kLaThreads), 0, (hipStream_t)stream, x, col, g, total);
    IDE3D_CHECK_LAUNCH("unfold2d");
    return IDE3D_OK;
}

extern "C" int ide3d_fold2d(const float* dcol, float* dx, int32_t n, int32_t c, int32_t h, int32_t w, int32_t k, int32_t stride, int32_t pad,
                            void* stream) {
    IDE3D_CHECK_ARG(dcol && dx, "fold2d: null pointer");
    LaGeom g;
    IDE3D_CHECK_ARG(la_geom(g, n, c, h, w, k, stride, pad), "fold2d: dx " LA_GEOM_TEXT);
    const int64_t total = (int64_t)n * c * h * w;
    hipLaunchKernelGGL(la_fold_kernel, dim3(stream_grid(total, kLaThreads)), dim3(kLaThreads), 0, (hipStream_t)stream, dcol, dx, g, total);
    IDE3D_CHECK_LAUNCH("fold2d");
    return IDE3D_OK;
}

extern "C" int ide3d_maxpool3s2p0(const float* x, float* y, uint8_t* idx, int64_t planes, int32_t h, int32_t w, void* stream) {
    IDE3D_CHECK_ARG(x && y, "maxpool3s2p0: null pointer");
    IDE3D_CHECK_ARG(planes >= 1 && h >= 3 && w >= 3 && h <= kLaMaxSide && w <= kLaMaxSide && planes * h * w < (1LL << 40),
                    "maxpool3s2p0: [planes, h, w] with sides in 3..%d", kLaMaxSide);
    const int oh = (h - 3) / 2 + 1, ow = (w - 3) / 2 + 1;
    const int64_t total = planes * oh * ow;
    hipLaunchKernelGGL(la_pool_kernel, dim3(stream_grid(total, kLaThreads)), dim3(kLaThreads), 0, (hipStream_t)stream, x, y, idx, h, w, oh, ow, total);
    IDE3D_CHECK_LAUNCH("maxpool3s2p0");
    return IDE3D_OK;
}

extern "C" int ide3d_lpips_tap_backward(const float* y, const float* g, const uint8_t* idx, const float* dtap, float* dz, int64_t planes,
                                        int32_t h, int32_t w, int32_t pooled, void* stream) {
    IDE3D_CHECK_ARG(y && dtap && dz, "lpips_tap_backward: null pointer");
    IDE3D_CHECK_ARG(pooled == 0 || pooled == 1, "lpips_tap_backward: pooled must be 0 or 1");
    IDE3D_CHECK_ARG(planes >= 1 && h >= 1 && w >= 1 && h <= kLaMaxSide && w <= kLaMaxSide && planes * h * w < (1LL << 40),
                    "lpips_tap_backward: [planes, h, w] with sides <= %d", kLaMaxSide);
    IDE3D_CHECK_ARG(!pooled || (g && idx), "lpips_tap_backward: a pooled gradient needs g and the winner bytes idx");
    IDE3D_CHECK_ARG(!pooled || (h >= 3 && w >= 3), "lpips_tap_backward: a pooled gradient needs h, w >= 3");
    hipStream_t st = (hipStream_t)stream;
    const int64_t total = planes * h * w;
    const dim3 grid(stream_grid(total, kLaThreads));
    if (pooled) {
        const int oh = (h - 3) / 2 + 1, ow = (w - 3) / 2 + 1;
        hipLaunchKernelGGL(la_tap_bwd_kernel<true>, grid, dim3(kLaThreads), 0, st, y, g, idx, dtap, dz, h, w, oh, ow, total);
    } else {
        hipLaunchKernelGGL(la_tap_bwd_kernel<false>, grid, dim3(kLaThreads), 0, st, y, g, (const unsigned char*)nullptr, dtap, dz, h, w, 0, 0, total);
    }
    IDE3D_CHECK_LAUNCH("lpips_tap_backward");
    return IDE3D_OK;
}
