// parse_loss.hip — everything of the face parser's cross-entropy loss and its image gradient that is not a stride-1 / 3x3 stride-2 convolution
// (DESIGN.md section 5.16).
//
// The 32 convolutions of BiSeNet (training/face_parsing.py) and 31 of the 32 convolutions of its input gradient are launches of
// ide3d_modconv2d, the plain ReLU gradients are ide3d_modconv_act_backward; this file holds the passes between them, all over NCHW fp32:
//   ide3d_parse_ce / _backward          the loss head: the align_corners=True resize of the 1/8 logits to the image size evaluated per image
//                                       pixel, a max-subtracted log-sum-exp, the mean; backward: the adjoint of that resize applied to
//                                       (softmax - onehot) dloss / (N H W), in gather form (the full-size logits never exist);
//   ide3d_resize_bilinear / _backward   the align_corners=True resize between the context scales and its adjoint in gather form;
//   ide3d_maxpool3s2 / _backward        the stem's 3x3 stride-2 pad-1 max pool (ATen's tie rule, a byte winner index) and its gradient in
//                                       gather form, the stem's ReLU mask applied in the same pass;
//   ide3d_parse_join                    out = post(t0 * scale[n, c] + t1 + t2 + bias[n, c]): the residual join relu(a + b), the gates
//                                       feat * g (+ broadcast), feat * g + feat, and backward the sum of the gradients that meet at a tensor
//                                       (a cropped transposed-convolution result, a half-resolution shortcut gradient scattered to the even
//                                       positions, a channel slice), the gate's scale, a mean's broadcast gradient and the ReLU mask;
//   ide3d_plane_sums                    out[n, c] = gain * sum_p a (* b): the spatial means and the gates' dot products;
//   ide3d_parse_stem_backward           the input gradient of the 7x7 stride-2 pad-3 stem, direct (<= 16 taps x cout channels per pixel).
// Lanes run along pixels; the grid's y runs over planes (n * c), so a thread splits a 32-bit in-plane index with one division and the
// plane's n and c are uniform over the workgroup.  The join moves 16 bytes per lane where every operand is dense and aligned and the width is a multiple of 4.
// Deterministic: no atomics; a plane's sum is one workgroup's fixed-order sum, the loss is per-workgroup partial sums (workspace) + one
// finishing launch; bit-reproducible.  The loss head and the resizes interpolate, exponentiate and sum in float64 (fp32 products are exact
// there), so they agree with a float64 evaluation of the same fp32 inputs to fp32 rounding.  Plain fp32 / fp64 arithmetic on the vector
// pipe (no packed fp32: the library is built without it); no matrix loop in this file, so section 4.2's exclusive residency does not apply.
#include "common.h"

namespace ide3d {

constexpr int kPlThreads = 256;
constexpr int kPlMaxSide = 16384;          // index products (side x side) stay inside int32

// ---- align_corners=True geometry --------------------------------------------------------------------------------------------------------------
// Output index d of an axis of `out` >= 2 points reads input position d (in - 1) / (out - 1): exact in integers.
struct PlAxis { int i0, i1; double l1; };

__device__ __forceinline__ PlAxis pl_axis(int d, int in, int out) {
    const int den = out - 1, num = d * (in - 1);
    PlAxis a;
    a.i0 = num / den;
    a.i1 = a.i0 + (a.i0 < in - 1 ? 1 : 0);
    a.l1 = (double)(num - a.i0 * den) / (double)den;
    return a;
}

// The output indices whose footprint holds input index i: those at a distance < 1 in input units.
__device__ __forceinline__ void pl_range(int i, int in, int out, int& lo, int& hi) {
    if (in == 1) { lo = 0; hi = out - 1; return; }
    const int den = out - 1, s = in - 1;
    lo = i == 0 ? 0 : ((i - 1) * den) / s + 1;
    hi = ((i + 1) * den + s - 1) / s - 1;
    if (hi > out - 1) hi = out - 1;
}

// The weight output index d (inside pl_range) puts on input index i: 1 - |d (in - 1) / (out - 1) - i|.
__device__ __forceinline__ double pl_weight(int d, int i, int in, int out) {
    if (in == 1) return 1.0;
    const int den = out - 1, num = d * (in - 1) - i * den;
    return (double)(den - (num < 0 ? -num : num)) / (double)den;
}

struct PlTaps { int o00, o01, o10, o11; double w00, w01, w10, w11; };

__device__ __forceinline__ PlTaps pl_taps(int Y, int X, int h, int w, int H, int W) {
    const PlAxis ay = pl_axis(Y, h, H), ax = pl_axis(X, w, W);
    PlTaps t;
    t.o00 = ay.i0 * w + ax.i0; t.o01 = ay.i0 * w + ax.i1; t.o10 = ay.i1 * w + ax.i0; t.o11 = ay.i1 * w + ax.i1;
    t.w00 = (1.0 - ay.l1) * (1.0 - ax.l1); t.w01 = (1.0 - ay.l1) * ax.l1; t.w10 = ay.l1 * (1.0 - ax.l1); t.w11 = ay.l1 * ax.l1;
    return t;
}

__device__ __forceinline__ double pl_interp(const float* __restrict__ p, const PlTaps& t) {
    return t.w00 * (double)p[t.o00] + t.w01 * (double)p[t.o01] + t.w10 * (double)p[t.o10] + t.w11 * (double)p[t.o11];
}

// Sum of v over the workgroup in a fixed order (a binary tree over thread indices); thread 0 holds it.
__device__ __forceinline__ double pl_block_sum(double v, double* s_red) {
    s_red[threadIdx.x] = v;
    __syncthreads();
#pragma unroll
    for (int off = kPlThreads / 2; off > 0; off >>= 1) {
        if ((int)threadIdx.x < off) s_red[threadIdx.x] += s_red[threadIdx.x + off];
        __syncthreads();
    }
    return s_red[0];
}

// The streaming kernels' grid: x over the elements of a plane (grid-stride), y over planes (grid-stride).
#define PL_PLANE_LOOP(plane, planes) for (int64_t plane = blockIdx.y; plane < (planes); plane += gridDim.y)
#define PL_ELEM_LOOP(i, count) for (int i = blockIdx.x * kPlThreads + threadIdx.x; i < (count); i += gridDim.x * kPlThreads)

static dim3 pl_grid(int64_t planes, int64_t per_plane) {
    return dim3((unsigned)stream_grid(per_plane, kPlThreads), (unsigned)(planes < 65535 ? planes : 65535));
}

// ---- resize -----------------------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kPlThreads)
pl_resize_kernel(const float* __restrict__ x, float* __restrict__ y, int h, int w, int H, int W, int64_t planes) {
    PL_PLANE_LOOP(plane, planes)
        PL_ELEM_LOOP(i, H * W) {
            const int Y = i / W, X = i - Y * W;
            const PlTaps t = pl_taps(Y, X, h, w, H, W);
            y[plane * H * (int64_t)W + i] = (float)pl_interp(x + plane * h * (int64_t)w, t);
        }
}

// dx[plane, iy, ix] = sum over the output pixels whose footprint holds (iy, ix) of their weight times dy, rows then columns ascending.
__global__ void __launch_bounds__(kPlThreads)
pl_resize_bwd_kernel(const float* __restrict__ dy, float* __restrict__ dx, int h, int w, int H, int W, int64_t planes) {
    PL_PLANE_LOOP(plane, planes)
    PL_ELEM_LOOP(i, h * w) {
        const int iy = i / w, ix = i - iy * w;
        int ylo, yhi, xlo, xhi;
        pl_range(iy, h, H, ylo, yhi);
        pl_range(ix, w, W, xlo, xhi);
        const float* __restrict__ g = dy + plane * H * (int64_t)W;
        double acc = 0.0;
        for (int Y = ylo; Y <= yhi; ++Y) {
            const double wy = pl_weight(Y, iy, h, H);
            double row = 0.0;
            for (int X = xlo; X <= xhi; ++X) row = fma(pl_weight(X, ix, w, W), (double)g[(int64_t)Y * W + X], row);
            acc = fma(wy, row, acc);
        }
        dx[plane * h * (int64_t)w + i] = (float)acc;
    }
}

// ---- loss head --------------------------------------------------------------------------------------------------------------------------------
// One thread = one image pixel: the C interpolated logits, an online max-subtracted log-sum-exp, lse - logit[label].
__global__ void __launch_bounds__(kPlThreads)
pl_ce_kernel(const float* __restrict__ lg, const int64_t* __restrict__ lab, double* __restrict__ lse, double* __restrict__ partial, int C, int h,
             int w, int H, int W, int64_t pixels) {
    __shared__ double s_red[kPlThreads];
    const int64_t i = (int64_t)blockIdx.x * kPlThreads + threadIdx.x;
    double loss = 0.0;
    if (i < pixels) {
        const int X = (int)(i % W);
        const int64_t r = i / W;
        const int Y = (int)(r % H);
        const int64_t n = r / H;
        const PlTaps t = pl_taps(Y, X, h, w, H, W);
        const int64_t hw = (int64_t)h * w;
        const float* __restrict__ p = lg + n * C * hw;
        const int64_t label = lab[i];
        double m = -INFINITY, s = 0.0, vt = 0.0;
        for (int c = 0; c < C; ++c) {
            const double v = pl_interp(p + c * hw, t);
            if (v > m) { s = s * exp(m - v) + 1.0; m = v; }
            else s += exp(v - m);
            if (c == label) vt = v;
        }
        const double l = m + log(s);
        lse[i] = l;
        loss = l - vt;
    }
    const double total = pl_block_sum(loss, s_red);
    if (threadIdx.x == 0) partial[blockIdx.x] = total;
}

// loss = (sum of the partials) * scale: thread i takes partials i, i + 256, ..., then the tree over the 256 thread sums.
__global__ void __launch_bounds__(kPlThreads)
pl_ce_finish_kernel(const double* __restrict__ partial, int64_t count, double scale, float* __restrict__ loss) {
    __shared__ double s_red[kPlThreads];
    double acc = 0.0;
    for (int64_t i = threadIdx.x; i < count; i += kPlThreads) acc += partial[i];
    const double total = pl_block_sum(acc, s_red);
    if (threadIdx.x == 0) loss[0] = (float)(total * scale);
}

// One thread = one low-resolution logit: over the image pixels whose footprint holds it, weight * (softmax - onehot), softmax recomputed
// from the interpolated logit of this channel and the pixel's saved log-sum-exp.
__global__ void __launch_bounds__(kPlThreads)
pl_ce_bwd_kernel(const float* __restrict__ lg, const int64_t* __restrict__ lab, const double* __restrict__ lse, const float* __restrict__ dloss,
                 float* __restrict__ dlg, int C, int h, int w, int H, int W, double inv_pixels, int64_t planes) {
    PL_PLANE_LOOP(plane, planes)
    PL_ELEM_LOOP(i, h * w) {
        const int iy = i / w, ix = i - iy * w;
        const int64_t n = plane / C;
        const int c = (int)(plane - n * C);
        int ylo, yhi, xlo, xhi;
        pl_range(iy, h, H, ylo, yhi);
        pl_range(ix, w, W, xlo, xhi);
        const float* __restrict__ p = lg + (n * C + c) * (int64_t)h * w;
        double acc = 0.0;
        for (int Y = ylo; Y <= yhi; ++Y) {
            const double wy = pl_weight(Y, iy, h, H);
            double row = 0.0;
            for (int X = xlo; X <= xhi; ++X) {
                const int64_t pix = (n * H + Y) * (int64_t)W + X;
                const double sm = exp(pl_interp(p, pl_taps(Y, X, h, w, H, W)) - lse[pix]) - (lab[pix] == c ? 1.0 : 0.0);
                row = fma(pl_weight(X, ix, w, W), sm, row);
            }
            acc = fma(wy, row, acc);
        }
        dlg[plane * h * (int64_t)w + i] = (float)(acc * (double)dloss[0] * inv_pixels);
    }
}

// ---- 3x3 stride-2 pad-1 max pool ---------------------------------------------------------------------------------------------------------------
// ATen's rule: the running maximum starts at -inf with the window's first valid element as its index; v > max or v != v takes over, so the
// first maximum in row-major order wins.  idx (may be NULL): the winner as ky * 3 + kx of the window anchored at (2 oy - 1, 2 ox - 1).
__global__ void __launch_bounds__(kPlThreads)
pl_pool3_kernel(const float* __restrict__ x, float* __restrict__ y, unsigned char* __restrict__ idx, int h, int w, int oh, int ow, int64_t planes) {
    PL_PLANE_LOOP(plane, planes)
    PL_ELEM_LOOP(i, oh * ow) {
        const int oy = i / ow, ox = i - oy * ow;
        const float* __restrict__ p = x + plane * h * (int64_t)w;
        const int y0 = 2 * oy - 1, x0 = 2 * ox - 1;
        const int ky0 = y0 < 0 ? 1 : 0, kx0 = x0 < 0 ? 1 : 0;
        float m = -INFINITY;
        int win = ky0 * 3 + kx0;
        for (int ky = ky0; ky < 3 && y0 + ky < h; ++ky)
            for (int kx = kx0; kx < 3 && x0 + kx < w; ++kx) {
                const float v = p[(int64_t)(y0 + ky) * w + x0 + kx];
                if (pool_gt(v, m)) { m = v; win = ky * 3 + kx; }
            }
        const int64_t o = plane * oh * (int64_t)ow + i;
        y[o] = m;
        if (idx) idx[o] = (unsigned char)win;
    }
}

// dx[y, x] = sum over the <= 4 windows that hold (y, x) and whose winner it is of dy, window rows then columns ascending (ATen's order);
// mask != NULL: 0 where mask <= 0 (the ReLU in front of the pool; mask is the pool's input).
__global__ void __launch_bounds__(kPlThreads)
pl_pool3_bwd_kernel(const float* __restrict__ dy, const unsigned char* __restrict__ idx, const float* __restrict__ mask, float* __restrict__ dx,
                    int h, int w, int oh, int ow, int64_t planes) {
    PL_PLANE_LOOP(plane, planes)
    PL_ELEM_LOOP(i, h * w) {
        const int yy = i / w, xx = i - yy * w;
        const int oy0 = yy / 2, oy1 = min((yy + 1) / 2, oh - 1), ox0 = xx / 2, ox1 = min((xx + 1) / 2, ow - 1);
        const int64_t base = plane * oh * (int64_t)ow;
        float g = 0.f;
        for (int oy = oy0; oy <= oy1; ++oy)
            for (int ox = ox0; ox <= ox1; ++ox) {
                const int64_t o = base + (int64_t)oy * ow + ox;
                if ((int)idx[o] == (yy - 2 * oy + 1) * 3 + (xx - 2 * ox + 1)) g += dy[o];
            }
        const int64_t e = plane * h * (int64_t)w + i;
        if (mask && !(mask[e] > 0.f)) g = 0.f;
        dx[e] = g;
    }
}

// ---- join -------------------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float pl_term(const ide3d_parse_term& t, int64_t n, int c, int y, int x) {
    if (t.p == nullptr) return 0.f;
    if (t.half) {
        if ((y | x) & 1) return 0.f;
        y >>= 1; x >>= 1;
    }
    return t.p[n * t.batch_stride + c * t.plane_stride + (int64_t)y * t.row_pitch + x];
}

__device__ __forceinline__ float pl_post(float v, int post, float yv) {
    if (post == 1) return v < 0.f ? 0.f : v;
    if (post == 2) return yv > 0.f ? v : 0.f;
    return v;
}

__device__ __forceinline__ float4 pl_term4(const ide3d_parse_term& t, int64_t n, int c, int y, int x) {
    if (t.p == nullptr) return make_float4(0.f, 0.f, 0.f, 0.f);
    return *reinterpret_cast<const float4*>(t.p + n * t.batch_stride + c * t.plane_stride + (int64_t)y * t.row_pitch + x);
}

// V4: w % 4 == 0, no half term, every pointer 16-byte aligned and every pitch / stride a multiple of 4: one thread = 4 pixels of a row.
template <bool V4>
__global__ void __launch_bounds__(kPlThreads)
pl_join_kernel(ide3d_parse_join_params p, int64_t planes) {
    const int cols = V4 ? p.w / 4 : p.w;
    PL_PLANE_LOOP(nc, planes)
    PL_ELEM_LOOP(i, p.h * cols) {
        const int y = i / cols, x = (i - y * cols) * (V4 ? 4 : 1);
        const int64_t n = nc / p.c;
        const int c = (int)(nc - n * p.c);
        const int64_t o = (nc * p.h + y) * (int64_t)p.w + x;
        const float sc = p.scale ? p.scale[nc] : 1.f;
        const float b = p.bias ? p.bias[nc] * p.bias_gain : 0.f;
        if (V4) {
            const float4 a = pl_term4(p.term[0], n, c, y, x), t1 = pl_term4(p.term[1], n, c, y, x), t2 = pl_term4(p.term[2], n, c, y, x);
            const float4 yv = p.post == 2 ? *reinterpret_cast<const float4*>(p.y + o) : make_float4(0.f, 0.f, 0.f, 0.f);
            float4 v;
            v.x = pl_post(a.x * sc + t1.x + t2.x + b, p.post, yv.x);
            v.y = pl_post(a.y * sc + t1.y + t2.y + b, p.post, yv.y);
            v.z = pl_post(a.z * sc + t1.z + t2.z + b, p.post, yv.z);
            v.w = pl_post(a.w * sc + t1.w + t2.w + b, p.post, yv.w);
            *reinterpret_cast<float4*>(p.out + o) = v;
        } else {
            const float v = pl_term(p.term[0], n, c, y, x) * sc + pl_term(p.term[1], n, c, y, x) + pl_term(p.term[2], n, c, y, x) + b;
            p.out[o] = pl_post(v, p.post, p.post == 2 ? p.y[o] : 0.f);
        }
    }
}

// ---- plane sums -------------------------------------------------------------------------------------------------------------------------------
// One workgroup = one plane: thread t adds elements t, t + 256, ... in float64, then the tree.
__global__ void __launch_bounds__(kPlThreads)
pl_plane_sums_kernel(const float* __restrict__ a, const float* __restrict__ b, float* __restrict__ out, int64_t hw, double gain) {
    __shared__ double s_red[kPlThreads];
    const float* __restrict__ pa = a + (int64_t)blockIdx.x * hw;
    const float* __restrict__ pb = b ? b + (int64_t)blockIdx.x * hw : nullptr;
    double acc = 0.0;
    for (int64_t i = threadIdx.x; i < hw; i += kPlThreads) acc = pb ? fma((double)pa[i], (double)pb[i], acc) : acc + (double)pa[i];
    const double total = pl_block_sum(acc, s_red);
    if (threadIdx.x == 0) out[blockIdx.x] = (float)(total * gain);
}

// ---- stem gradient ----------------------------------------------------------------------------------------------------------------------------
// y = conv2d(x, wt [cout, 3, 7, 7], stride 2, padding 3); dx[n, ci, Y, X] = sum_co sum_{ky, kx with Y + 3 - ky and X + 3 - kx even}
// dz[n, co, (Y + 3 - ky) / 2, (X + 3 - kx) / 2] wt[co, ci, ky, kx].  One thread = one pixel, all 3 channels; the weights sit in LDS; the
// <= 16 taps of a channel are summed in fp32, the channels in float64.
constexpr int kStemCin = 3, kStemK = 7, kStemMaxCout = 64, kStemTileW = 64, kStemTileH = kPlThreads / kStemTileW;

__global__ void __launch_bounds__(kPlThreads)
pl_stem_bwd_kernel(const float* __restrict__ dz, const float* __restrict__ wt, float* __restrict__ dx, int cout, int H, int W, int ho, int wo) {
    __shared__ float s_w[kStemMaxCout * kStemCin * kStemK * kStemK];
    constexpr int kk = kStemK * kStemK;
    for (int i = threadIdx.x; i < cout * kStemCin * kk; i += kPlThreads) s_w[i] = wt[i];
    __syncthreads();
    const int X = blockIdx.x * kStemTileW + (threadIdx.x % kStemTileW), Y = blockIdx.y * kStemTileH + (threadIdx.x / kStemTileW);
    const int64_t n = blockIdx.z;
    if (X >= W || Y >= H) return;
    const int py = (Y + 1) & 1, px = (X + 1) & 1;
    double acc0 = 0.0, acc1 = 0.0, acc2 = 0.0;
    for (int co = 0; co < cout; ++co) {
        const float* __restrict__ d = dz + (n * cout + co) * (int64_t)ho * wo;
        const float* __restrict__ sw = s_w + co * kStemCin * kk;
        float a0 = 0.f, a1 = 0.f, a2 = 0.f;
        for (int ky = py; ky < kStemK; ky += 2) {
            const int oy = (Y + 3 - ky) >> 1;
            if (oy < 0 || oy >= ho) continue;
            for (int kx = px; kx < kStemK; kx += 2) {
                const int ox = (X + 3 - kx) >> 1;
                if (ox < 0 || ox >= wo) continue;
                const float v = d[(int64_t)oy * wo + ox];
                const int wi = ky * kStemK + kx;
                a0 = fmaf(v, sw[wi], a0);
                a1 = fmaf(v, sw[wi + kk], a1);
                a2 = fmaf(v, sw[wi + 2 * kk], a2);
            }
        }
        acc0 += (double)a0; acc1 += (double)a1; acc2 += (double)a2;
    }
    const int64_t plane = (int64_t)H * W, o = n * kStemCin * plane + (int64_t)Y * W + X;
    dx[o] = (float)acc0;
    dx[o + plane] = (float)acc1;
    dx[o + 2 * plane] = (float)acc2;
}

static bool pl_sides_ok(int64_t planes, int32_t h, int32_t w, int32_t H, int32_t W) {
    return planes >= 1 && h >= 1 && w >= 1 && H >= 2 && W >= 2 && h <= kPlMaxSide && w <= kPlMaxSide && H <= kPlMaxSide && W <= kPlMaxSide
           && planes * h * w < (1LL << 40) && planes * H * W < (1LL << 40);
}

static bool pl_ce_ok(int32_t n, int32_t C, int32_t h, int32_t w, int32_t H, int32_t W) {
    return n >= 1 && C >= 1 && C <= 4096 && pl_sides_ok((int64_t)n * C, h, w, H, W) && cdiv64((int64_t)n * H * W, kPlThreads) <= 0x7fffffffLL;
}

}  // namespace ide3d

using namespace ide3d;

extern "C" int ide3d_resize_bilinear(const float* x, float* y, int64_t planes, int32_t h, int32_t w, int32_t H, int32_t W, void* stream) {
    IDE3D_CHECK_ARG(x && y, "resize_bilinear: null pointer");
    IDE3D_CHECK_ARG(pl_sides_ok(planes, h, w, H, W), "resize_bilinear: [planes, h, w] -> [planes, H, W] with H, W >= 2 and sides <= %d", kPlMaxSide);
    hipLaunchKernelGGL(pl_resize_kernel, pl_grid(planes, (int64_t)H * W), dim3(kPlThreads), 0, (hipStream_t)stream, x, y, h, w, H, W, planes);
    IDE3D_CHECK_LAUNCH("resize_bilinear");
    return IDE3D_OK;
}

extern "C" int ide3d_resize_bilinear_backward(const float* dy, float* dx, int64_t planes, int32_t h, int32_t w, int32_t H, int32_t W, void* stream) {
    IDE3D_CHECK_ARG(dy && dx, "resize_bilinear_backward: null pointer");
    IDE3D_CHECK_ARG(pl_sides_ok(planes, h, w, H, W), "resize_bilinear_backward: [planes, H, W] -> [planes, h, w] with H, W >= 2 and sides <= %d", kPlMaxSide);
    hipLaunchKernelGGL(pl_resize_bwd_kernel, pl_grid(planes, (int64_t)h * w), dim3(kPlThreads), 0, (hipStream_t)stream, dy, dx, h, w, H, W, planes);
    IDE3D_CHECK_LAUNCH("resize_bilinear_backward");
    return IDE3D_OK;
}

extern "C" int64_t ide3d_parse_ce_workspace_bytes(int32_t n, int32_t C, int32_t h, int32_t w, int32_t H, int32_t W) {
    if (!pl_ce_ok(n, C, h, w, H, W)) return -1;
    return cdiv64((int64_t)n * H * W, kPlThreads) * (int64_t)sizeof(double);
}

extern "C" int ide3d_parse_ce(const float* logits, const int64_t* labels, int32_t n, int32_t C, int32_t h, int32_t w, int32_t H, int32_t W,
                              double* lse, float* workspace, int64_t workspace_bytes, float* loss, void* stream) {
    IDE3D_CHECK_ARG(logits && labels && lse && loss, "parse_ce: null pointer");
    IDE3D_CHECK_ARG(pl_ce_ok(n, C, h, w, H, W), "parse_ce: logits [n, C, h, w], labels [n, H, W] with H, W >= 2 and sides <= %d", kPlMaxSide);
    const int64_t pixels = (int64_t)n * H * W, blocks = cdiv64(pixels, kPlThreads);
    IDE3D_CHECK_ARG(workspace && ptr_aligned(workspace, 8) && ptr_aligned(lse, 8) && workspace_bytes >= blocks * (int64_t)sizeof(double),
                    "parse_ce: workspace too small or misaligned");
    double* partial = reinterpret_cast<double*>(workspace);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(pl_ce_kernel, dim3((unsigned)blocks), dim3(kPlThreads), 0, st, logits, labels, lse, partial, C, h, w, H, W, pixels);
    hipLaunchKernelGGL(pl_ce_finish_kernel, dim3(1), dim3(kPlThreads), 0, st, (const double*)partial, blocks, 1.0 / (double)pixels, loss);
    IDE3D_CHECK_LAUNCH("parse_ce");
    return IDE3D_OK;
}

extern "C" int ide3d_parse_ce_backward(const float* logits, const int64_t* labels, const double* lse, const float* dloss, float* dlogits,
                                       int32_t n, int32_t C, int32_t h, int32_t w, int32_t H, int32_t W, void* stream) {
    IDE3D_CHECK_ARG(logits && labels && lse && dloss && dlogits, "parse_ce_backward: null pointer");
    IDE3D_CHECK_ARG(pl_ce_ok(n, C, h, w, H, W), "parse_ce_backward: logits [n, C, h, w], labels [n, H, W] with H, W >= 2 and sides <= %d", kPlMaxSide);
    const int64_t planes = (int64_t)n * C;
    hipLaunchKernelGGL(pl_ce_bwd_kernel, pl_grid(planes, (int64_t)h * w), dim3(kPlThreads), 0, (hipStream_t)stream, logits, labels, lse, dloss,
                       dlogits, C, h, w, H, W, 1.0 / ((double)n * H * W), planes);
    IDE3D_CHECK_LAUNCH("parse_ce_backward");
    return IDE3D_OK;
}

extern "C" int ide3d_maxpool3s2(const float* x, float* y, uint8_t* idx, int64_t planes, int32_t h, int32_t w, void* stream) {
    IDE3D_CHECK_ARG(x && y, "maxpool3s2: null pointer");
    IDE3D_CHECK_ARG(planes >= 1 && h >= 1 && w >= 1 && h <= kPlMaxSide && w <= kPlMaxSide && planes * h * w < (1LL << 40),
                    "maxpool3s2: [planes, h, w] with sides <= %d", kPlMaxSide);
    const int oh = (h - 1) / 2 + 1, ow = (w - 1) / 2 + 1;
    hipLaunchKernelGGL(pl_pool3_kernel, pl_grid(planes, (int64_t)oh * ow), dim3(kPlThreads), 0, (hipStream_t)stream, x, y, idx, h, w, oh, ow, planes);
    IDE3D_CHECK_LAUNCH("maxpool3s2");
    return IDE3D_OK;
}

extern "C" int ide3d_maxpool3s2_backward(const float* dy, const uint8_t* idx, const float* mask, float* dx, int64_t planes, int32_t h, int32_t w,
                                         void* stream) {
    IDE3D_CHECK_ARG(dy && idx && dx, "maxpool3s2_backward: null pointer");
    IDE3D_CHECK_ARG(planes >= 1 && h >= 1 && w >= 1 && h <= kPlMaxSide && w <= kPlMaxSide && planes * h * w < (1LL << 40),
                    "maxpool3s2_backward: [planes, h, w] with sides <= %d", kPlMaxSide);
    const int oh = (h - 1) / 2 + 1, ow = (w - 1) / 2 + 1;
    hipLaunchKernelGGL(pl_pool3_bwd_kernel, pl_grid(planes, (int64_t)h * w), dim3(kPlThreads), 0, (hipStream_t)stream, dy, idx, mask, dx, h, w,
                       oh, ow, planes);
    IDE3D_CHECK_LAUNCH("maxpool3s2_backward");
    return IDE3D_OK;
}

extern "C" int ide3d_parse_join(const ide3d_parse_join_params* p, void* stream) {
    IDE3D_CHECK_ARG(p != nullptr && p->out != nullptr && p->term[0].p != nullptr, "parse_join: null pointer");
    IDE3D_CHECK_ARG(p->n >= 1 && p->c >= 1 && p->h >= 1 && p->w >= 1 && p->h <= kPlMaxSide && p->w <= kPlMaxSide
                    && (int64_t)p->n * p->c * p->h * p->w < (1LL << 40), "parse_join: out [n, c, h, w] with sides <= %d", kPlMaxSide);
    IDE3D_CHECK_ARG(p->post >= 0 && p->post <= 2 && (p->post != 2 || p->y != nullptr), "parse_join: post 0 (none), 1 (relu) or 2 (mask by y > 0, y given)");
    bool v4 = p->w % 4 == 0 && ptr_aligned(p->out, 16) && (p->post != 2 || ptr_aligned(p->y, 16));
    for (int i = 0; i < IDE3D_PARSE_JOIN_TERMS; ++i) {
        const ide3d_parse_term& t = p->term[i];
        if (t.p == nullptr) continue;
        const int th = t.half ? (p->h + 1) / 2 : p->h, tw = t.half ? (p->w + 1) / 2 : p->w;
        IDE3D_CHECK_ARG(t.row_pitch >= tw && t.plane_stride >= (int64_t)(th - 1) * t.row_pitch + tw && t.batch_stride >= (p->c - 1) * t.plane_stride + 1,
                        "parse_join: term %d: row pitch, plane stride and batch stride must cover its [n, c, h, w]", i);
        v4 = v4 && !t.half && ptr_aligned(t.p, 16) && t.row_pitch % 4 == 0 && t.plane_stride % 4 == 0 && t.batch_stride % 4 == 0;
    }
    const int64_t planes = (int64_t)p->n * p->c, per_plane = (int64_t)p->h * (v4 ? p->w / 4 : p->w);
    hipStream_t st = (hipStream_t)stream;
    if (v4) hipLaunchKernelGGL(pl_join_kernel<true>, pl_grid(planes, per_plane), dim3(kPlThreads), 0, st, *p, planes);
    else hipLaunchKernelGGL(pl_join_kernel<false>, pl_grid(planes, per_plane), dim3(kPlThreads), 0, st, *p, planes);
    IDE3D_CHECK_LAUNCH("parse_join");
    return IDE3D_OK;
}

extern "C" int ide3d_plane_sums(const float* a, const float* b, float* out, int64_t planes, int64_t hw, float gain, void* stream) {
    IDE3D_CHECK_ARG(a && out, "plane_sums: null pointer");
    IDE3D_CHECK_ARG(planes >= 1 && planes <= 0x7fffffffLL && hw >= 1 && planes * hw < (1LL << 40), "plane_sums: [planes, hw]");
    hipLaunchKernelGGL(pl_plane_sums_kernel, dim3((unsigned)planes), dim3(kPlThreads), 0, (hipStream_t)stream, a, b, out, hw, (double)gain);
    IDE3D_CHECK_LAUNCH("plane_sums");
    return IDE3D_OK;
}

extern "C" int ide3d_parse_stem_backward(const float* dz, const float* weight, float* dx, int32_t n, int32_t cout, int32_t H, int32_t W, void* stream) {
    IDE3D_CHECK_ARG(dz && weight && dx, "parse_stem_backward: null pointer");
    IDE3D_CHECK_ARG(n >= 1 && n <= 65535 && cout >= 1 && cout <= kStemMaxCout && H >= 1 && W >= 1 && H <= kPlMaxSide && W <= kPlMaxSide,
                    "parse_stem_backward: dx [n, 3, H, W], weight [cout <= %d, 3, 7, 7], n <= 65535", kStemMaxCout);
    const int ho = (H - 1) / 2 + 1, wo = (W - 1) / 2 + 1;
    hipLaunchKernelGGL(pl_stem_bwd_kernel, dim3(cdiv(W, kStemTileW), cdiv(H, kStemTileH), n), dim3(kPlThreads), 0, (hipStream_t)stream, dz, weight, dx,
                       cout, H, W, ho, wo);
    IDE3D_CHECK_LAUNCH("parse_stem_backward");
    return IDE3D_OK;
}
