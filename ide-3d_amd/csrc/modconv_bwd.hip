// modconv_bwd.hip — the streaming and reduction passes of the frozen-generator convolution backward.
//
// The matrix work of the backward of a modulated convolution with respect to its input is itself a modulated convolution and runs on
// ide3d_modconv2d (modconv.hip).  What is left are three small kernels:
//   K1 ide3d_modconv_act_backward: dz = dy * act'(y) (the grad = 1 form of ide3d_bias_act, bit-equal to it) and, in the same pass,
//      dot[n, o] = sum_p dz * (u - noise - bias) with the pre-activation u recovered from y, then d dcoefs = dot / dcoefs;
//      its dot-only form: dot[n, o] = sum_p g * y (y already demodulated), d dcoefs = dot / dcoefs;
//   K2 ide3d_modconv_scale_dot: dx = styles[n, i] * t and d styles[n, i] = sum_p x * t;
//   K3 ide3d_head_weight_grad: dW[n, o, i] = sum_p dy[n, o, p] * x[n, i, p] (per-image 1x1 weights: the folded dual heads).
// The parameter gradients of trainable layers (section 5.11, PTI pivotal tuning) add two more:
//   K4 ide3d_modconv_weight_grad: the direct weight gradient of a modulated 3x3 convolution, on the matrix cores (below);
//   K5 ide3d_bias_noise_grad: db[c] = sum_{n,p} dz and dnoise[p] = sum_{n,c} dz.
// Every reduction is deterministic: workgroups write fixed-order partial sums over fixed pixel ranges, a second launch adds them in
// a fixed order.  No atomics.  Exact fp32 on the vector pipe (plain FMAs, no packed fp32: the library is built without it).
#include "common.h"

namespace ide3d {

constexpr int kBwdThreads = 256;
constexpr int kBwdChunk = 4096;            // elements of one (image, channel) plane per workgroup in K1 / K2

// Sum of v over the workgroup in a fixed order (butterfly inside each wave, then the 4 waves in index order); valid in thread 0.
__device__ __forceinline__ float block_sum(float v, float* s_red) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    if ((threadIdx.x & 63) == 0) s_red[threadIdx.x >> 6] = v;
    __syncthreads();
    float t = 0.f;
    if (threadIdx.x == 0)
        for (int i = 0; i < kBwdThreads / 64; ++i) t += s_red[i];
    return t;
}

// One element of K1.  ACT 0: dot-only (g * y); 1 linear, 3 lrelu: the grad = 1 form of bias_act_one (bias_act.hip) with dy = 1 and the
// same operation order, so that dz is bit-equal to ide3d_bias_act(dy, b, -, y, -, grad = 1, ...).
template <int ACT>
__device__ __forceinline__ float act_bwd_one(float g, float yv, float nz, float b, float alpha, float gain, float clamp, float& dz) {
    if (ACT == 0) { dz = g; return g * yv; }
    const float yy = (gain != 0.f) ? yv / gain : 0.f;
    float r = (ACT == 3) ? ((yy > 0.f) ? g : g * alpha) : g;
    r *= gain * 1.f;
    if (clamp >= 0.f) r = (yv > -clamp && yv < clamp) ? r : 0.f;
    dz = r;
    const float u = (ACT == 3) ? ((yy > 0.f) ? yy : yy / alpha) : yy;   // the pre-activation; only read where r != 0 (not clamped)
    return r * (u - nz - b);
}

// 1-D grid of n * c * chunks workgroups: workgroup b = chunk b % chunks of plane b / chunks (partial[b]).  V4: dense rows (y_pitch == w)
// and h * w % 4 == 0.
template <int ACT, bool DOT, bool V4>
__global__ void __launch_bounds__(kBwdThreads)
act_bwd_kernel(ide3d_act_bwd_params p, int pitch, int chunks, float* __restrict__ partial) {
    __shared__ float s_red[kBwdThreads / 64];
    const int plane = blockIdx.x / chunks, ch = plane % p.c;
    const int hw = p.h * p.w;
    const int e0 = (blockIdx.x % chunks) * kBwdChunk, e1 = min(e0 + kBwdChunk, hw);
    const float* __restrict__ dy = p.dy + (int64_t)plane * hw;
    const float* __restrict__ y = p.y + (int64_t)plane * p.h * pitch;
    float* __restrict__ dz = (ACT != 0) ? p.dz + (int64_t)plane * hw : nullptr;
    const float b = (p.bias && ACT != 0) ? p.bias[ch] : 0.f;
    const float ns = p.noise_strength;
    float acc = 0.f;
    if (V4) {
        for (int e = e0 + threadIdx.x * 4; e < e1; e += kBwdThreads * 4) {
            const float4 g = *reinterpret_cast<const float4*>(dy + e);
            const float4 yv = *reinterpret_cast<const float4*>(y + e);
            float4 nz = make_float4(0.f, 0.f, 0.f, 0.f);
            if (ACT != 0 && p.noise) { nz = *reinterpret_cast<const float4*>(p.noise + e); nz.x *= ns; nz.y *= ns; nz.z *= ns; nz.w *= ns; }
            float4 r;
            const float a0 = act_bwd_one<ACT>(g.x, yv.x, nz.x, b, p.alpha, p.gain, p.clamp, r.x);
            const float a1 = act_bwd_one<ACT>(g.y, yv.y, nz.y, b, p.alpha, p.gain, p.clamp, r.y);
            const float a2 = act_bwd_one<ACT>(g.z, yv.z, nz.z, b, p.alpha, p.gain, p.clamp, r.z);
            const float a3 = act_bwd_one<ACT>(g.w, yv.w, nz.w, b, p.alpha, p.gain, p.clamp, r.w);
            if (DOT) acc += (a0 + a1) + (a2 + a3);
            if (ACT != 0) *reinterpret_cast<float4*>(dz + e) = r;
        }
    } else {
        for (int e = e0 + threadIdx.x; e < e1; e += kBwdThreads) {
            const int row = e / p.w, col = e - row * p.w;
            const float nz = (ACT != 0 && p.noise) ? ns * p.noise[e] : 0.f;
            float r;
            const float a = act_bwd_one<ACT>(dy[e], y[(int64_t)row * pitch + col], nz, b, p.alpha, p.gain, p.clamp, r);
            if (DOT) acc += a;
            if (ACT != 0) dz[e] = r;
        }
    }
    if (DOT) {
        const float t = block_sum(acc, s_red);
        if (threadIdx.x == 0) partial[blockIdx.x] = t;
    }
}

// 1-D grid as act_bwd_kernel: dx = s * t, partial = sum x * t
template <bool V4>
__global__ void __launch_bounds__(kBwdThreads)
scale_dot_kernel(const float* __restrict__ x, const float* __restrict__ t, const float* __restrict__ styles, float* __restrict__ dx,
                 int hw, int chunks, float* __restrict__ partial) {
    __shared__ float s_red[kBwdThreads / 64];
    const int plane = blockIdx.x / chunks;
    const int e0 = (blockIdx.x % chunks) * kBwdChunk, e1 = min(e0 + kBwdChunk, hw);
    const int64_t base = (int64_t)plane * hw;
    const float s = styles[plane];
    float acc = 0.f;
    if (V4) {
        for (int e = e0 + threadIdx.x * 4; e < e1; e += kBwdThreads * 4) {
            const float4 tv = *reinterpret_cast<const float4*>(t + base + e);
            const float4 xv = *reinterpret_cast<const float4*>(x + base + e);
            acc += (xv.x * tv.x + xv.y * tv.y) + (xv.z * tv.z + xv.w * tv.w);
            *reinterpret_cast<float4*>(dx + base + e) = make_float4(s * tv.x, s * tv.y, s * tv.z, s * tv.w);
        }
    } else {
        for (int e = e0 + threadIdx.x; e < e1; e += kBwdThreads) {
            const float tv = t[base + e];
            acc += x[base + e] * tv;
            dx[base + e] = s * tv;
        }
    }
    const float r = block_sum(acc, s_red);
    if (threadIdx.x == 0) partial[blockIdx.x] = r;
}

// out[i] = (sum_{k < parts} partial[i * parts + k]) / (div ? div[i] : 1), in k order
__global__ void __launch_bounds__(kBwdThreads)
plane_sum_kernel(const float* __restrict__ partial, int parts, int64_t count, const float* __restrict__ div, float* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * kBwdThreads + threadIdx.x;
    if (i >= count) return;
    float s = 0.f;
    for (int k = 0; k < parts; ++k) s += partial[i * parts + k];
    out[i] = div ? s / div[i] : s;
}

// ---- K3: dW[n, o, i] = sum_p dy[n, o, p] * x[n, i, p] ------------------------------------------------------------------------------
// One workgroup: a 64 (o) x 64 (i) block of one image over one pixel range; 16 x 16 threads of 4 x 4 outputs each; 32 pixels per LDS stage
// (pixel-major, rows padded by 4 floats: 16-byte reads, stores of consecutive pixels spread over the banks).
constexpr int kWgT = 64, kWgK = 32, kWgLd = kWgT + 4;

struct WgradGeom { int tiles_o, tiles_i, splits, pix_per_split; };

static WgradGeom wgrad_geom(int n, int rows, int cin, int hw) {
    WgradGeom g;
    g.tiles_o = cdiv(rows, kWgT); g.tiles_i = cdiv(cin, kWgT);
    const int64_t base = (int64_t)n * g.tiles_o * g.tiles_i;
    int64_t s = cdiv64(1024, base);                              // ~1024 workgroups (4 per CU)
    const int64_t smax = cdiv64(hw, 256);                        // at least 256 pixels per workgroup
    if (s > smax) s = smax;
    if (s > 256) s = 256;                                        // bounds the second pass: `splits` values per output
    if (s < 1) s = 1;
    g.pix_per_split = (int)(cdiv64(cdiv64(hw, s), kWgK) * kWgK);
    g.splits = (int)cdiv64(hw, g.pix_per_split);
    return g;
}

__global__ void __launch_bounds__(kBwdThreads)
head_wgrad_kernel(const float* __restrict__ dy, const float* __restrict__ x, int rows, int cin, int hw, WgradGeom g, float* __restrict__ partial) {
    __shared__ __attribute__((aligned(16))) float s_a[kWgK][kWgLd];
    __shared__ __attribute__((aligned(16))) float s_b[kWgK][kWgLd];
    // 1-D grid: workgroup b = (image, split, tile) in that order of significance
    const int tiles = g.tiles_o * g.tiles_i, tile = blockIdx.x % tiles;
    const int split = (blockIdx.x / tiles) % g.splits, n = blockIdx.x / (tiles * g.splits);
    const int to = tile / g.tiles_i, ti = tile % g.tiles_i;
    const int o0 = to * kWgT, i0 = ti * kWgT;
    const int p0 = split * g.pix_per_split, p1 = min(p0 + g.pix_per_split, hw);
    const float* __restrict__ A = dy + (int64_t)n * rows * hw;
    const float* __restrict__ B = x + (int64_t)n * cin * hw;
    const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
    float acc[4][4];
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) acc[a][b] = 0.f;
    for (int pk = p0; pk < p1; pk += kWgK) {
        // stage 64 rows x 32 pixels of each operand: element e -> (row e / 32, pixel e % 32), zero outside the ranges
#pragma unroll
        for (int j = 0; j < kWgT * kWgK / kBwdThreads; ++j) {
            const int e = threadIdx.x + j * kBwdThreads;
            const int r = e / kWgK, k = e % kWgK, pix = pk + k;
            const bool inp = pix < p1;
            s_a[k][r] = (inp && o0 + r < rows) ? A[(int64_t)(o0 + r) * hw + pix] : 0.f;
            s_b[k][r] = (inp && i0 + r < cin) ? B[(int64_t)(i0 + r) * hw + pix] : 0.f;
        }
        __syncthreads();
#pragma unroll 8
        for (int k = 0; k < kWgK; ++k) {
            const float4 av = *reinterpret_cast<const float4*>(&s_a[k][ty * 4]);
            const float4 bv = *reinterpret_cast<const float4*>(&s_b[k][tx * 4]);
            const float aa[4] = {av.x, av.y, av.z, av.w}, bb[4] = {bv.x, bv.y, bv.z, bv.w};
#pragma unroll
            for (int a = 0; a < 4; ++a)
#pragma unroll
                for (int b = 0; b < 4; ++b) acc[a][b] = fmaf(aa[a], bb[b], acc[a][b]);
        }
        __syncthreads();
    }
    // partial [n][split][rows][cin]
    float* __restrict__ out = partial + ((int64_t)n * g.splits + split) * rows * cin;
#pragma unroll
    for (int a = 0; a < 4; ++a) {
        const int o = o0 + ty * 4 + a;
        if (o >= rows) continue;
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            const int i = i0 + tx * 4 + b;
            if (i < cin) out[(int64_t)o * cin + i] = acc[a][b];
        }
    }
}

// dw[n][o][i] = sum over splits, in split order; the loads are issued 8 at a time (independent), the adds stay in order
__global__ void __launch_bounds__(kBwdThreads)
head_wgrad_sum_kernel(const float* __restrict__ partial, int splits, int64_t per_image, int n, float* __restrict__ dw) {
    const int64_t e = (int64_t)blockIdx.x * kBwdThreads + threadIdx.x;
    if (e >= per_image * n) return;
    const int64_t img = e / per_image, r = e % per_image;
    const float* src = partial + img * splits * per_image + r;
    float s = 0.f;
    int k = 0;
    for (; k + 8 <= splits; k += 8) {
        float v[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = src[(int64_t)(k + j) * per_image];
#pragma unroll
        for (int j = 0; j < 8; ++j) s += v[j];
    }
    for (; k < splits; ++k) s += src[(int64_t)k * per_image];
    dw[e] = s;
}


// ---- K4: the direct weight gradient of a modulated 3x3 convolution -----------------------------------------
// dW[o, i, k] = sum_n d[n, o] s[n, i] sum_q A_k[n, o, q] B_k[n, i, q]: a GEMM with M = cout, N = cin x 9 taps, K = n x pixels,
//   mode 0 (stride-1 layer, g = dz [n, co, h, w]): q = output pixel, A = g[q], B = x[q + (ky - 1, kx - 1)] (zero outside the map);
//   mode 2 (up-sampling layer, g = g_t [n, co, 2h + 1, 2w + 1]): q = input pixel, A = g_t[2 q + (ky, kx)], B = x[q];
//   mode 1 (stride-2 unpadded layer, x [n, ci, h, w], g = dz [n, co, (h - 3) / 2 + 1, (w - 3) / 2 + 1]): q = output pixel, A = g[q],
//     B = x[2 q + (ky, kx)]: mode 2 with the operands' roles exchanged, the strided read on the B side of the same staging code.
// One workgroup: one image, one tap, one 64 (o) x 64 (i) tile, one range of pixels; 4 waves of one 32 x 32 accumulator tile each.  The
// operands are scaled (d on A, s on B) and split while they are staged, 32 pixels per stage: the next stage's global loads are in flight
// while the current one feeds the matrix cores.  bf16x6 (three bf16 pieces per operand, the six products above 2^-24 on
// v_mfma_f32_32x32x16_bf16) or exact fp32 (v_mfma_f32_32x32x2_f32).  Each workgroup writes its own partial slice (image, split), a second
// launch adds the slices in a fixed order: no atomics, bit-reproducible.  Exclusive residency (section 4.2): every wave claims all 512
// registers of its SIMD, so no foreign wave shares a SIMD with the LDS-fed bf16 loop.
constexpr int kWtM = 64, kWtN = 64, kWtK = 32;

struct WtGeom { int tiles_o, tiles_i, splits, pix_per_split, kpix; };

// (h, w): the grid of K pixels q (modes 0 and 2: the size of x; mode 1: the size of g)
static WtGeom wt_geom(int n, int cout, int cin, int h, int w) {
    WtGeom g;
    g.tiles_o = cdiv(cout, kWtM); g.tiles_i = cdiv(cin, kWtN); g.kpix = h * w;
    const int64_t base = (int64_t)n * 9 * g.tiles_o * g.tiles_i;
    int64_t s = cdiv64(2048, base);                              // ~2048 workgroups (8 rounds of one per CU)
    const int64_t smax = cdiv64(g.kpix, 512);                    // at least 512 pixels per workgroup
    if (s > smax) s = smax;
    if (s > 256) s = 256;
    if (s < 1) s = 1;
    g.pix_per_split = (int)(cdiv64(cdiv64(g.kpix, s), kWtK) * kWtK);
    g.splits = (int)cdiv64(g.kpix, g.pix_per_split);
    return g;
}

typedef unsigned wt_u32x4 __attribute__((ext_vector_type(4)));
typedef __bf16 wt_bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 wt_bf16x2 __attribute__((ext_vector_type(2)));
typedef float wt_f32x2 __attribute__((ext_vector_type(2)));
typedef float wt_f32x16 __attribute__((ext_vector_type(16)));

// a, b -> 3 packed bf16 pairs (round to nearest even) whose sums reproduce a and b; the residuals are exact in fp32
__device__ __forceinline__ void wt_split3(float a, float b, unsigned (&out)[3]) {
#pragma unroll
    for (int q = 0; q < 3; ++q) {
        const wt_f32x2 v = {a, b};
        const unsigned pk = __builtin_bit_cast(unsigned, __builtin_convertvector(v, wt_bf16x2));
        out[q] = pk;
        a -= __uint_as_float(pk << 16); b -= __uint_as_float(pk & 0xffff0000u);
    }
}

// the 8 consecutive K pixels q0 .. q0 + 7 (< q1) of row `r` of each operand, scaled; zero outside the ranges
template <int MODE>
__device__ __forceinline__ void wt_load(const ide3d_wgrad_params& p, const float* __restrict__ A, const float* __restrict__ B, int o, int i,
                                        float da, float sb, int ky, int kx, int q0, int q1, float (&av)[8], float (&bv)[8]) {
    const int h = p.h, w = (MODE == 1) ? (p.w - 3) / 2 + 1 : p.w;        // w: the row length of the K-pixel grid
    int y = q0 / w, xx = q0 - y * w;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const bool in = q0 + e < q1;
        if (MODE == 0) {
            av[e] = (in && o < p.cout) ? A[q0 + e] * da : 0.f;
            const int sy = y + ky - 1, sx = xx + kx - 1;
            bv[e] = (in && i < p.cin && sy >= 0 && sy < h && sx >= 0 && sx < w) ? B[sy * w + sx] * sb : 0.f;
        } else if (MODE == 1) {
            av[e] = (in && o < p.cout) ? A[q0 + e] * da : 0.f;
            bv[e] = (in && i < p.cin) ? B[(2 * y + ky) * p.w + 2 * xx + kx] * sb : 0.f;      // 2 y + ky <= h - 1, 2 xx + kx <= p.w - 1 for q < q1
        } else {
            av[e] = (in && o < p.cout) ? A[(2 * y + ky) * (2 * w + 1) + 2 * xx + kx] * da : 0.f;
            bv[e] = (in && i < p.cin) ? B[q0 + e] * sb : 0.f;
        }
        if (++xx == w) { xx = 0; ++y; }
    }
}

template <int MODE, bool SPLIT>
__global__ void __launch_bounds__(kBwdThreads, 1)
modconv_wgrad_kernel(ide3d_wgrad_params p, WtGeom g, float* __restrict__ partial) {
    asm volatile("" ::: "v255", "a255");                         // exclusive residency: one wave per SIMD, all 512 registers
    // bf16x6: [part][k step][k half][row] 16-byte units of 8 pixels, per operand; fp32: [pixel][row]
    constexpr int kUnits = 3 * 2 * 2 * 64;
    __shared__ __attribute__((aligned(16))) unsigned char s_mem[SPLIT ? 2 * kUnits * 16 : 2 * kWtK * 64 * 4];
    const int tiles = g.tiles_o * g.tiles_i;
    int b = blockIdx.x;
    const int tile = b % tiles; b /= tiles;
    const int tap = b % 9; b /= 9;
    const int split = b % g.splits, n = b / g.splits;
    const int ky = tap / 3, kx = tap % 3;
    const int o0 = (tile / g.tiles_i) * kWtM, i0 = (tile % g.tiles_i) * kWtN;
    const int q0 = split * g.pix_per_split, q1 = min(q0 + g.pix_per_split, g.kpix);
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6, half = lane >> 5, l32 = lane & 31;
    const int wm = wid >> 1, wn = wid & 1;
    // staging role: row r of both operands, pixels 8 sq .. 8 sq + 7 of the stage
    const int r = tid >> 2, sq = tid & 3;
    const int o = o0 + r, i = i0 + r;
    const int64_t gplane = (MODE == 0) ? (int64_t)p.h * p.w : (MODE == 1) ? (int64_t)g.kpix : (int64_t)(2 * p.h + 1) * (2 * p.w + 1);
    const float* __restrict__ A = p.g + ((int64_t)n * p.cout + min(o, p.cout - 1)) * gplane;
    const float* __restrict__ B = p.x + ((int64_t)n * p.cin + min(i, p.cin - 1)) * p.h * p.w;
    const float da = (o < p.cout && p.dcoefs) ? p.dcoefs[(int64_t)n * p.cout + o] : 1.f;
    const float sb = (i < p.cin && p.styles) ? p.styles[(int64_t)n * p.cin + i] : 1.f;
    wt_f32x16 acc;
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[e] = 0.f;
    float av[8], bv[8];
    wt_load<MODE>(p, A, B, o, i, da, sb, ky, kx, q0 + 8 * sq, q1, av, bv);
    for (int qk = q0; qk < q1; qk += kWtK) {
        if constexpr (SPLIT) {
            wt_u32x4* sa = reinterpret_cast<wt_u32x4*>(s_mem);
            wt_u32x4* sbm = sa + kUnits;
            unsigned pa[4][3], pb[4][3];
#pragma unroll
            for (int e = 0; e < 4; ++e) { wt_split3(av[2 * e], av[2 * e + 1], pa[e]); wt_split3(bv[2 * e], bv[2 * e + 1], pb[e]); }
#pragma unroll
            for (int part = 0; part < 3; ++part) {
                const int u = ((part * 2 + (sq >> 1)) * 2 + (sq & 1)) * 64 + r;
                sa[u] = wt_u32x4{pa[0][part], pa[1][part], pa[2][part], pa[3][part]};
                sbm[u] = wt_u32x4{pb[0][part], pb[1][part], pb[2][part], pb[3][part]};
            }
        } else {
            float* sa = reinterpret_cast<float*>(s_mem);
            float* sbm = sa + kWtK * 64;
#pragma unroll
            for (int e = 0; e < 8; ++e) { sa[(8 * sq + e) * 64 + r] = av[e]; sbm[(8 * sq + e) * 64 + r] = bv[e]; }
        }
        __syncthreads();
        if (qk + kWtK < q1) wt_load<MODE>(p, A, B, o, i, da, sb, ky, kx, qk + kWtK + 8 * sq, q1, av, bv);
        if constexpr (SPLIT) {
            const wt_u32x4* sa = reinterpret_cast<const wt_u32x4*>(s_mem);
            const wt_u32x4* sbm = sa + kUnits;
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) {
                wt_u32x4 fa[3], fb[3];
#pragma unroll
                for (int part = 0; part < 3; ++part) {
                    fa[part] = sa[((part * 2 + ks) * 2 + half) * 64 + wm * 32 + l32];
                    fb[part] = sbm[((part * 2 + ks) * 2 + half) * 64 + wn * 32 + l32];
                }
                // the six products above 2^-24, smallest first
#define IDE3D_WT_MFMA(PA, PB) acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(wt_bf16x8, fa[PA]), __builtin_bit_cast(wt_bf16x8, fb[PB]), acc, 0, 0, 0)
                IDE3D_WT_MFMA(2, 0); IDE3D_WT_MFMA(1, 1); IDE3D_WT_MFMA(0, 2);
                IDE3D_WT_MFMA(1, 0); IDE3D_WT_MFMA(0, 1); IDE3D_WT_MFMA(0, 0);
#undef IDE3D_WT_MFMA
            }
        } else {
            const float* sa = reinterpret_cast<const float*>(s_mem);
            const float* sbm = sa + kWtK * 64;
#pragma unroll
            for (int ks = 0; ks < kWtK / 2; ++ks)
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(sa[(2 * ks + half) * 64 + wm * 32 + l32], sbm[(2 * ks + half) * 64 + wn * 32 + l32], acc, 0, 0, 0);
        }
        __syncthreads();
    }
    // partial [n * splits + split][co][ci][9]
    float* __restrict__ out = partial + ((int64_t)n * g.splits + split) * p.cout * p.cin * 9;
    const int ic = i0 + wn * 32 + l32;
    if (ic < p.cin) {
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const int oc = o0 + wm * 32 + 8 * (e >> 2) + 4 * half + (e & 3);
            if (oc < p.cout) out[((int64_t)oc * p.cin + ic) * 9 + tap] = acc[e];
        }
    }
}

// ---- K5: bias and noise gradients, db[c] = sum_{n,p} dz, dnoise[p] = sum_{n,c} dz ---------------------------------------------------
// 1-D grid of pixel blocks x plane groups: each workgroup reads kBnPlanes planes over kBnPix pixels once; per plane each wave writes its
// sum over its pixels (pdb), per pixel the workgroup writes the sum over its planes (pnoise).  bn_sum_kernel adds both in fixed order.
constexpr int kBnPix = 4 * kBwdThreads, kBnPlanes = 32;

__global__ void __launch_bounds__(kBwdThreads)
bias_noise_partial_kernel(const float* __restrict__ dz, int planes, int hw, int pblocks, float* __restrict__ pdb, float* __restrict__ pnoise) {
    const int pb = blockIdx.x % pblocks, grp = blockIdx.x / pblocks;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int pl0 = grp * kBnPlanes, pl1 = min(pl0 + kBnPlanes, planes);
    const int px0 = pb * kBnPix + threadIdx.x;
    float col[4] = {0.f, 0.f, 0.f, 0.f};
    for (int pl = pl0; pl < pl1; ++pl) {
        const float* __restrict__ src = dz + (int64_t)pl * hw;
        float v[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) { const int px = px0 + j * kBwdThreads; v[j] = px < hw ? src[px] : 0.f; col[j] += v[j]; }
        float s = (v[0] + v[1]) + (v[2] + v[3]);
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off);
        if (lane == 0) pdb[((int64_t)pl * pblocks + pb) * 4 + wave] = s;
    }
    if (pnoise) {
#pragma unroll
        for (int j = 0; j < 4; ++j) { const int px = px0 + j * kBwdThreads; if (px < hw) pnoise[(int64_t)grp * hw + px] = col[j]; }
    }
}

// e < c: db[e] = sum over images, then pixel blocks and waves, in order; else dnoise[e - c] = sum over plane groups in order
__global__ void __launch_bounds__(kBwdThreads)
bias_noise_sum_kernel(const float* __restrict__ pdb, const float* __restrict__ pnoise, int n, int c, int hw, int pblocks, int groups,
                      float* __restrict__ db, float* __restrict__ dnoise) {
    const int64_t e = (int64_t)blockIdx.x * kBwdThreads + threadIdx.x;
    const int per = pblocks * 4;
    if (e < c) {
        float s = 0.f;
        for (int img = 0; img < n; ++img) {
            const float* src = pdb + ((int64_t)img * c + e) * per;
            int k = 0;
            for (; k + 8 <= per; k += 8) {
                float v[8];
#pragma unroll
                for (int j = 0; j < 8; ++j) v[j] = src[k + j];
#pragma unroll
                for (int j = 0; j < 8; ++j) s += v[j];
            }
            for (; k < per; ++k) s += src[k];
        }
        db[e] = s;
    } else if (dnoise && e < c + (int64_t)hw) {
        const int64_t px = e - c;
        float s = 0.f;
        for (int gi = 0; gi < groups; ++gi) s += pnoise[(int64_t)gi * hw + px];
        dnoise[px] = s;
    }
}

}  // namespace ide3d

using namespace ide3d;

extern "C" int64_t ide3d_act_bwd_workspace_bytes(int32_t n, int32_t c, int32_t h, int32_t w) {
    if (n <= 0 || c <= 0 || h <= 0 || w <= 0) return -1;
    return (int64_t)n * c * cdiv64((int64_t)h * w, kBwdChunk) * (int64_t)sizeof(float);
}

extern "C" int ide3d_modconv_act_backward(const ide3d_act_bwd_params* pp, void* stream) {
    IDE3D_CHECK_ARG(pp != nullptr, "modconv_act_backward: null params");
    const ide3d_act_bwd_params& p = *pp;
    IDE3D_CHECK_ARG(p.n > 0 && p.c > 0 && p.h > 0 && p.w > 0, "modconv_act_backward: bad shape");
    IDE3D_CHECK_ARG((int64_t)p.n * p.c * p.h * p.w < 0x7fffffffLL, "modconv_act_backward: input too large for 32-bit indexing");
    IDE3D_CHECK_ARG((int64_t)p.h * (p.y_pitch > 0 ? p.y_pitch : p.w) < 0x7fffffffLL, "modconv_act_backward: plane too large");
    IDE3D_CHECK_ARG(p.act == 0 || p.act == 1 || p.act == 3, "modconv_act_backward: act must be 0 (dot only), 1 (linear) or 3 (lrelu)");
    IDE3D_CHECK_ARG(p.dy && p.y && (p.act == 0 || p.dz), "modconv_act_backward: null dy / y / dz");
    IDE3D_CHECK_ARG(p.y_pitch == 0 || p.y_pitch >= p.w, "modconv_act_backward: y_pitch must be 0 or >= w");
    const bool dot = p.ddcoefs != nullptr;
    IDE3D_CHECK_ARG(!dot || p.dcoefs, "modconv_act_backward: ddcoefs needs dcoefs");
    IDE3D_CHECK_ARG(dot || p.act != 0, "modconv_act_backward: the dot-only form needs ddcoefs");
    const int hw = p.h * p.w, chunks = cdiv(hw, kBwdChunk);
    const int64_t planes = (int64_t)p.n * p.c;
    IDE3D_CHECK_ARG(planes * chunks < 0x7fffffffLL, "modconv_act_backward: too many workgroups");
    if (dot) IDE3D_CHECK_ARG(p.workspace && p.workspace_bytes >= planes * chunks * (int64_t)sizeof(float), "modconv_act_backward: workspace too small");
    const int pitch = p.y_pitch > 0 ? p.y_pitch : p.w;
    const bool v4 = pitch == p.w && hw % 4 == 0 && ((uintptr_t)p.dy & 15) == 0 && ((uintptr_t)p.y & 15) == 0 &&
                    (p.act == 0 || ((uintptr_t)p.dz & 15) == 0) && (!p.noise || ((uintptr_t)p.noise & 15) == 0);
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)(planes * chunks));
#define IDE3D_ACT_BWD(A, D) do { if (v4) hipLaunchKernelGGL((act_bwd_kernel<A, D, true>), grid, dim3(kBwdThreads), 0, st, p, pitch, chunks, p.workspace); \
                                 else    hipLaunchKernelGGL((act_bwd_kernel<A, D, false>), grid, dim3(kBwdThreads), 0, st, p, pitch, chunks, p.workspace); } while (0)
    if (p.act == 0)      IDE3D_ACT_BWD(0, true);
    else if (p.act == 1) { if (dot) IDE3D_ACT_BWD(1, true); else IDE3D_ACT_BWD(1, false); }
    else                 { if (dot) IDE3D_ACT_BWD(3, true); else IDE3D_ACT_BWD(3, false); }
#undef IDE3D_ACT_BWD
    if (dot)
        hipLaunchKernelGGL(plane_sum_kernel, dim3((unsigned)cdiv64(planes, kBwdThreads)), dim3(kBwdThreads), 0, st, p.workspace, chunks, planes, p.dcoefs, p.ddcoefs);
    IDE3D_CHECK_LAUNCH("modconv_act_backward");
    return IDE3D_OK;
}

extern "C" int ide3d_modconv_scale_dot(const float* x, const float* t, const float* styles, float* dx, float* dstyles,
                                       int32_t n, int32_t c, int32_t h, int32_t w, float* workspace, int64_t workspace_bytes, void* stream) {
    IDE3D_CHECK_ARG(x && t && styles && dx && dstyles && workspace, "modconv_scale_dot: null pointer");
    IDE3D_CHECK_ARG(n > 0 && c > 0 && h > 0 && w > 0, "modconv_scale_dot: bad shape");
    IDE3D_CHECK_ARG((int64_t)n * c * h * w < 0x7fffffffLL, "modconv_scale_dot: input too large for 32-bit indexing");
    const int hw = h * w, chunks = cdiv(hw, kBwdChunk);
    const int64_t planes = (int64_t)n * c;
    IDE3D_CHECK_ARG(workspace_bytes >= planes * chunks * (int64_t)sizeof(float), "modconv_scale_dot: workspace too small");
    const bool v4 = hw % 4 == 0 && (((uintptr_t)x | (uintptr_t)t | (uintptr_t)dx) & 15) == 0;
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)(planes * chunks));
    if (v4) hipLaunchKernelGGL(scale_dot_kernel<true>, grid, dim3(kBwdThreads), 0, st, x, t, styles, dx, hw, chunks, workspace);
    else    hipLaunchKernelGGL(scale_dot_kernel<false>, grid, dim3(kBwdThreads), 0, st, x, t, styles, dx, hw, chunks, workspace);
    hipLaunchKernelGGL(plane_sum_kernel, dim3((unsigned)cdiv64(planes, kBwdThreads)), dim3(kBwdThreads), 0, st, workspace, chunks, planes,
                       (const float*)nullptr, dstyles);
    IDE3D_CHECK_LAUNCH("modconv_scale_dot");
    return IDE3D_OK;
}

extern "C" int64_t ide3d_head_wgrad_workspace_bytes(int32_t n, int32_t rows, int32_t cin, int32_t h, int32_t w) {
    if (n <= 0 || rows <= 0 || cin <= 0 || h <= 0 || w <= 0) return -1;
    const WgradGeom g = wgrad_geom(n, rows, cin, h * w);
    return (int64_t)n * g.splits * rows * cin * (int64_t)sizeof(float);
}

extern "C" int ide3d_head_weight_grad(const float* dy, const float* x, float* dw, int32_t n, int32_t rows, int32_t cin, int32_t h, int32_t w,
                                      float* workspace, int64_t workspace_bytes, void* stream) {
    IDE3D_CHECK_ARG(dy && x && dw && workspace, "head_weight_grad: null pointer");
    IDE3D_CHECK_ARG(n > 0 && rows > 0 && cin > 0 && h > 0 && w > 0, "head_weight_grad: bad shape");
    IDE3D_CHECK_ARG((int64_t)(rows > cin ? rows : cin) * h * w < 0x7fffffffLL, "head_weight_grad: input too large for 32-bit pixel indexing");
    const int hw = h * w;
    const WgradGeom g = wgrad_geom(n, rows, cin, hw);
    IDE3D_CHECK_ARG(workspace_bytes >= (int64_t)n * g.splits * rows * cin * (int64_t)sizeof(float), "head_weight_grad: workspace too small");
    hipStream_t st = (hipStream_t)stream;
    const int64_t wgs = (int64_t)n * g.splits * g.tiles_o * g.tiles_i;
    IDE3D_CHECK_ARG(wgs < 0x7fffffffLL, "head_weight_grad: too many workgroups");
    hipLaunchKernelGGL(head_wgrad_kernel, dim3((unsigned)wgs), dim3(kBwdThreads), 0, st, dy, x, rows, cin, hw, g, workspace);
    const int64_t per = (int64_t)rows * cin;
    hipLaunchKernelGGL(head_wgrad_sum_kernel, dim3((unsigned)cdiv64(per * n, kBwdThreads)), dim3(kBwdThreads), 0, st, workspace, g.splits, per, n, dw);
    IDE3D_CHECK_LAUNCH("head_weight_grad");
    return IDE3D_OK;
}

extern "C" int64_t ide3d_wgrad_workspace_bytes(int32_t n, int32_t cin, int32_t cout, int32_t h, int32_t w) {
    if (n <= 0 || cin <= 0 || cout <= 0 || h <= 0 || w <= 0 || (int64_t)h * w >= 0x7fffffffLL) return -1;
    const WtGeom g = wt_geom(n, cout, cin, h, w);
    return (int64_t)n * g.splits * cout * cin * 9 * (int64_t)sizeof(float);
}

extern "C" int ide3d_modconv_weight_grad(const ide3d_wgrad_params* pp, void* stream) {
    IDE3D_CHECK_ARG(pp != nullptr, "modconv_weight_grad: null params");
    const ide3d_wgrad_params& p = *pp;
    IDE3D_CHECK_ARG(p.g && p.x && p.dw && p.workspace, "modconv_weight_grad: null g / x / dw / workspace");
    IDE3D_CHECK_ARG(p.n > 0 && p.cin > 0 && p.cout > 0 && p.h > 0 && p.w > 0, "modconv_weight_grad: bad shape");
    IDE3D_CHECK_ARG(p.mode == 0 || p.mode == 1 || p.mode == 2,
                    "modconv_weight_grad: mode must be 0 (3x3, stride 1), 1 (3x3, stride 2, no padding) or 2 (transposed 3x3, stride 2)");
    IDE3D_CHECK_ARG(p.mode != 1 || (p.h >= 3 && p.w >= 3), "modconv_weight_grad: mode 1 needs an input of at least 3 x 3");
    // the grid of K pixels: the size of x in modes 0 and 2, of g in mode 1
    const int qh = p.mode == 1 ? (p.h - 3) / 2 + 1 : p.h, qw = p.mode == 1 ? (p.w - 3) / 2 + 1 : p.w;
    const int64_t gplane = p.mode == 2 ? (int64_t)(2 * p.h + 1) * (2 * p.w + 1) : (int64_t)qh * qw;
    // (factor by factor: the products below must not leave 64 bits either)
    IDE3D_CHECK_ARG((int64_t)p.h * p.w < 0x7fffffffLL && gplane < 0x7fffffffLL && (int64_t)p.n * p.cin < 0x7fffffffLL && (int64_t)p.n * p.cout < 0x7fffffffLL,
                    "modconv_weight_grad: operands too large for 32-bit indexing");
    IDE3D_CHECK_ARG((int64_t)p.n * p.cin * ((int64_t)p.h * p.w) < 0x7fffffffLL && (int64_t)p.n * p.cout * gplane < 0x7fffffffLL,
                    "modconv_weight_grad: operands too large for 32-bit indexing");
    const WtGeom g = wt_geom(p.n, p.cout, p.cin, qh, qw);
    const int64_t per = (int64_t)p.cout * p.cin * 9, slices = (int64_t)p.n * g.splits;
    IDE3D_CHECK_ARG(p.workspace_bytes >= slices * per * (int64_t)sizeof(float), "modconv_weight_grad: workspace too small");
    const int64_t wgs = slices * 9 * g.tiles_o * g.tiles_i;
    IDE3D_CHECK_ARG(wgs < 0x7fffffffLL, "modconv_weight_grad: too many workgroups");
    const int arith = p.arith ? p.arith : ide3d_get_conv_arithmetic();
    IDE3D_CHECK_ARG(arith == 1 || arith == 3 || arith == 6 || arith == 16, "modconv_weight_grad: arith must be 0, 1, 3, 6 or 16");
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)wgs);
    if (arith == 1) {
        if (p.mode == 0)      IDE3D_EXCL_LAUNCH((modconv_wgrad_kernel<0, false>), grid, kBwdThreads, 0, st, p, g, p.workspace);
        else if (p.mode == 1) IDE3D_EXCL_LAUNCH((modconv_wgrad_kernel<1, false>), grid, kBwdThreads, 0, st, p, g, p.workspace);
        else                  IDE3D_EXCL_LAUNCH((modconv_wgrad_kernel<2, false>), grid, kBwdThreads, 0, st, p, g, p.workspace);
    } else {
        if (p.mode == 0)      IDE3D_EXCL_LAUNCH((modconv_wgrad_kernel<0, true>), grid, kBwdThreads, 0, st, p, g, p.workspace);
        else if (p.mode == 1) IDE3D_EXCL_LAUNCH((modconv_wgrad_kernel<1, true>), grid, kBwdThreads, 0, st, p, g, p.workspace);
        else                  IDE3D_EXCL_LAUNCH((modconv_wgrad_kernel<2, true>), grid, kBwdThreads, 0, st, p, g, p.workspace);
    }
    IDE3D_CHECK_LAUNCH("modconv_weight_grad");
    hipLaunchKernelGGL(head_wgrad_sum_kernel, dim3((unsigned)cdiv64(per, kBwdThreads)), dim3(kBwdThreads), 0, st, p.workspace, (int)slices, per, 1, p.dw);
    IDE3D_CHECK_LAUNCH("modconv_weight_grad");
    return IDE3D_OK;
}

extern "C" int64_t ide3d_bias_noise_workspace_bytes(int32_t n, int32_t c, int32_t h, int32_t w) {
    if (n <= 0 || c <= 0 || h <= 0 || w <= 0) return -1;
    const int64_t hw = (int64_t)h * w, pblocks = cdiv64(hw, kBnPix), groups = cdiv64((int64_t)n * c, kBnPlanes);
    return ((int64_t)n * c * pblocks * 4 + groups * hw) * (int64_t)sizeof(float);
}

extern "C" int ide3d_bias_noise_grad(const float* dz, float* db, float* dnoise, int32_t n, int32_t c, int32_t h, int32_t w,
                                     float* workspace, int64_t workspace_bytes, void* stream) {
    IDE3D_CHECK_ARG(dz && db && workspace, "bias_noise_grad: null dz / db / workspace");
    IDE3D_CHECK_ARG(n > 0 && c > 0 && h > 0 && w > 0, "bias_noise_grad: bad shape");
    IDE3D_CHECK_ARG((int64_t)n * c * h * w < 0x7fffffffLL, "bias_noise_grad: input too large for 32-bit indexing");
    const int hw = h * w, pblocks = cdiv(hw, kBnPix), planes = n * c, groups = cdiv(planes, kBnPlanes);
    IDE3D_CHECK_ARG(workspace_bytes >= ide3d_bias_noise_workspace_bytes(n, c, h, w), "bias_noise_grad: workspace too small");
    IDE3D_CHECK_ARG((int64_t)pblocks * groups < 0x7fffffffLL, "bias_noise_grad: too many workgroups");
    float* pdb = workspace;
    float* pnoise = dnoise ? workspace + (int64_t)planes * pblocks * 4 : nullptr;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(bias_noise_partial_kernel, dim3((unsigned)(pblocks * groups)), dim3(kBwdThreads), 0, st, dz, planes, hw, pblocks, pdb, pnoise);
    const int64_t outs = c + (dnoise ? (int64_t)hw : 0);
    hipLaunchKernelGGL(bias_noise_sum_kernel, dim3((unsigned)cdiv64(outs, kBwdThreads)), dim3(kBwdThreads), 0, st, pdb, pnoise, n, c, hw, pblocks,
                       groups, db, dnoise);
    IDE3D_CHECK_LAUNCH("bias_noise_grad");
    return IDE3D_OK;
}
