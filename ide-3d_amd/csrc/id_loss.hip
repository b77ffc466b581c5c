// id_loss.hip — everything of the ArcFace identity loss and its image gradient that is not a convolution.
//
// The 53 convolutions of the IR-SE50 face net (training/id_loss.py) and their input gradients are launches of ide3d_modconv2d; the
// per-channel affine passes, the gated residual joins and the spatial means are ide3d_parse_join / ide3d_plane_sums (parse_loss.hip).
// This file holds the rest, all over dense NCHW fp32:
//   ide3d_id_prep / _backward               average pooling by f, the fixed crop [35:223, 32:220] of the 256 x 256 frame and the adaptive
//                                           average pooling 188 -> 112 in one launch; the adjoint in gather form;
//   ide3d_prelu / _backward                 per-channel PReLU, bit-equal to ATen; the backward reads the pre-activation;
//   ide3d_se_gate / _backward               the squeeze-excite gate sigmoid(W2 relu(W1 s)) of all n in one launch, one workgroup per image;
//   ide3d_linear / _backward_input          y = x W^T + b and dx = dy W for a weight matrix that is streamed once for all n <= 8 rows:
//                                           partial sums per slice of K (of M) in a workspace + one finishing launch;
//   ide3d_id_head / _backward               e = f / |f|, loss = mean_i (1 - e_i . t_i) and its closed-form gradient.
// Lanes run along the contiguous axis; 16-byte accesses where shapes and alignment allow.  Deterministic: no atomics, every sum has a
// fixed order (a thread's own ascending loop, then a tree over thread indices, then an ascending loop over the partials).  Sums that end
// in one number (means, norms, dot products, the gate's two small matrix products) are carried in float64; the long dot products of the
// linear layer are fp32 per lane (8 terms), then a 64-lane tree, then float64 over the slices.  Plain fp32 / fp64 arithmetic on the vector
// pipe (no packed fp32: the library is built without it); no matrix loop in this file, so section 4.2's exclusive residency does not apply.
#include "common.h"

namespace ide3d {

constexpr int kIdThreads = 256;
constexpr int kIdFrame = 256, kIdTop = 35, kIdLeft = 32, kIdCrop = 188, kIdOut = 112;          // id_loss.py: x[:, :, 35:223, 32:220] -> 112
constexpr int kIdMaxFactor = 64;
constexpr int kSeMaxC = 512, kSeMaxR = 32, kSeLanes = kIdThreads / kSeMaxR;
constexpr int kLinMaxN = 8, kLinChunk = 2048, kLinRows = 8, kLinBwdThreads = 64, kLinBwdRows = 64;
constexpr int kHeadMaxM = 8192;

// AdaptiveAvgPool2d(112) over 188 points: output i averages [lo(i), hi(i)) (2 or 3 points); point r lies in windows first(r) .. last(r).
__device__ __forceinline__ int id_lo(int i) { return (i * kIdCrop) / kIdOut; }
__device__ __forceinline__ int id_hi(int i) { return ((i + 1) * kIdCrop + kIdOut - 1) / kIdOut; }
__device__ __forceinline__ int id_first(int r) { return (r * kIdOut) / kIdCrop; }
__device__ __forceinline__ int id_last(int r) { return ((r + 1) * kIdOut + kIdCrop - 1) / kIdCrop - 1; }

// Sum of v over the workgroup in a fixed order (a binary tree over thread indices); every thread receives it.
__device__ __forceinline__ double id_block_sum(double v, double* s_red) {
    __syncthreads();
    s_red[threadIdx.x] = v;
    __syncthreads();
#pragma unroll
    for (int off = kIdThreads / 2; off > 0; off >>= 1) {
        if ((int)threadIdx.x < off) s_red[threadIdx.x] += s_red[threadIdx.x + off];
        __syncthreads();
    }
    return s_red[0];
}

#define ID_PLANE_LOOP(plane, planes) for (int64_t plane = blockIdx.y; plane < (planes); plane += gridDim.y)
#define ID_ELEM_LOOP(i, count) for (int i = blockIdx.x * kIdThreads + threadIdx.x; i < (count); i += gridDim.x * kIdThreads)

static dim3 id_grid(int64_t planes, int64_t per_plane) {
    return dim3((unsigned)stream_grid(per_plane, kIdThreads), (unsigned)(planes < 65535 ? planes : 65535));
}

// ---- pooling, crop, pooling ---------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kIdThreads)
id_prep_kernel(const float* __restrict__ x, float* __restrict__ y, int f, int64_t planes) {
    const int side = kIdFrame * f;
    ID_PLANE_LOOP(plane, planes)
    ID_ELEM_LOOP(o, kIdOut * kIdOut) {
        const int i = o / kIdOut, j = o - i * kIdOut;
        const int r0 = id_lo(i), r1 = id_hi(i), c0 = id_lo(j), c1 = id_hi(j);
        const float* __restrict__ p = x + plane * side * (int64_t)side;
        double acc = 0.0;
        for (int Y = (r0 + kIdTop) * f; Y < (r1 + kIdTop) * f; ++Y) {
            double row = 0.0;
            for (int X = (c0 + kIdLeft) * f; X < (c1 + kIdLeft) * f; ++X) row += (double)p[(int64_t)Y * side + X];
            acc += row;
        }
        y[plane * (kIdOut * kIdOut) + o] = (float)(acc / (double)(f * f * (r1 - r0) * (c1 - c0)));
    }
}

// dx[Y, X] = sum over the <= 2 x 2 output windows that hold crop point (Y / f - 35, X / f - 32), rows then columns ascending, of
// dy / (f^2 * window area); an exact 0 outside the crop.
__global__ void __launch_bounds__(kIdThreads)
id_prep_bwd_kernel(const float* __restrict__ dy, float* __restrict__ dx, int f, int64_t planes) {
    const int side = kIdFrame * f;
    ID_PLANE_LOOP(plane, planes)
    ID_ELEM_LOOP(e, side * side) {
        const int Y = e / side, X = e - Y * side;
        const int r = Y / f - kIdTop, c = X / f - kIdLeft;
        float g = 0.f;
        if (r >= 0 && r < kIdCrop && c >= 0 && c < kIdCrop) {
            const float* __restrict__ q = dy + plane * (kIdOut * kIdOut);
            const int j0 = id_first(c), j1 = id_last(c);
            double acc = 0.0;
            for (int i = id_first(r); i <= id_last(r); ++i) {
                double row = 0.0;
                for (int j = j0; j <= j1; ++j) row += (double)q[i * kIdOut + j] / (double)(id_hi(j) - id_lo(j));
                acc += row / (double)(id_hi(i) - id_lo(i));
            }
            g = (float)(acc / (double)(f * f));
        }
        dx[plane * side * (int64_t)side + e] = g;
    }
}

// ---- PReLU --------------------------------------------------------------------------------------------------------------------------------------
// ATen's rule, forward and backward: the branch is taken on x > 0, so x = 0 (and NaN) multiply by the slope.
__device__ __forceinline__ float id_prelu(float x, float v, float a) { return x > 0.f ? v : a * v; }

// V4: hw % 4 == 0 and every pointer 16-byte aligned: one thread = 4 elements of a plane.
template <bool V4>
__global__ void __launch_bounds__(kIdThreads)
id_prelu_kernel(const float* __restrict__ x, const float* __restrict__ slope, float* __restrict__ y, int c, int hw, int64_t planes) {
    const int count = V4 ? hw / 4 : hw;
    ID_PLANE_LOOP(plane, planes) {
        const float a = slope[plane % c];
        ID_ELEM_LOOP(i, count) {
            const int64_t o = plane * hw + (int64_t)i * (V4 ? 4 : 1);
            if (V4) {
                const float4 v = *reinterpret_cast<const float4*>(x + o);
                *reinterpret_cast<float4*>(y + o) = make_float4(id_prelu(v.x, v.x, a), id_prelu(v.y, v.y, a), id_prelu(v.z, v.z, a), id_prelu(v.w, v.w, a));
            } else {
                y[o] = id_prelu(x[o], x[o], a);
            }
        }
    }
}

// dy may be a view: [n, c, h, w] with contiguous rows (the cropped result of a transposed convolution); x and dx are dense.
template <bool V4>
__global__ void __launch_bounds__(kIdThreads)
id_prelu_bwd_kernel(const float* __restrict__ dy, int64_t batch_stride, int64_t plane_stride, int row_pitch, const float* __restrict__ x,
                    const float* __restrict__ slope, float* __restrict__ dx, int c, int h, int w, int64_t planes) {
    const int hw = h * w, count = V4 ? hw / 4 : hw;
    ID_PLANE_LOOP(plane, planes) {
        const int64_t n = plane / c;
        const int ch = (int)(plane - n * c);
        const float a = slope[ch];
        const float* __restrict__ g = dy + n * batch_stride + ch * plane_stride;
        ID_ELEM_LOOP(i, count) {
            const int64_t o = plane * hw + (int64_t)i * (V4 ? 4 : 1);
            if (V4) {                                                       // (dense dy: plane_stride == hw, row_pitch == w)
                const float4 v = *reinterpret_cast<const float4*>(x + o), d = *reinterpret_cast<const float4*>(g + (int64_t)i * 4);
                *reinterpret_cast<float4*>(dx + o) = make_float4(id_prelu(v.x, d.x, a), id_prelu(v.y, d.y, a), id_prelu(v.z, d.z, a), id_prelu(v.w, d.w, a));
            } else {
                const int yy = i / w, xx = i - yy * w;
                dx[o] = id_prelu(x[o], g[(int64_t)yy * row_pitch + xx], a);
            }
        }
    }
}

// ---- squeeze-excite gate ------------------------------------------------------------------------------------------------------------------------
// One workgroup = one image.  hidden[j] = relu(sum_k W1[j, k] s[k]): 8 threads per hidden unit (k = l, l + 8, ...), their 8 sums added in
// order by the unit's first thread.  s_s holds s; -> s_h[0..r).
__device__ __forceinline__ void se_hidden(const float* __restrict__ w1, const float* s_s, int c, int r, double* s_part, double* s_h) {
    const int j = threadIdx.x / kSeLanes, l = threadIdx.x % kSeLanes;
    double acc = 0.0;
    if (j < r)
        for (int k = l; k < c; k += kSeLanes) acc = fma((double)w1[j * c + k], (double)s_s[k], acc);
    s_part[threadIdx.x] = acc;
    __syncthreads();
    if ((int)threadIdx.x < r) {
        double t = 0.0;
        for (int q = 0; q < kSeLanes; ++q) t += s_part[threadIdx.x * kSeLanes + q];
        s_h[threadIdx.x] = t > 0.0 ? t : 0.0;
    }
    __syncthreads();
}

__global__ void __launch_bounds__(kIdThreads)
id_se_gate_kernel(const float* __restrict__ s, const float* __restrict__ w1, const float* __restrict__ w2, float* __restrict__ g, int c, int r) {
    __shared__ float s_s[kSeMaxC];
    __shared__ double s_part[kIdThreads], s_h[kSeMaxR];
    const int64_t n = blockIdx.x;
    for (int k = threadIdx.x; k < c; k += kIdThreads) s_s[k] = s[n * c + k];
    __syncthreads();
    se_hidden(w1, s_s, c, r, s_part, s_h);
    for (int k = threadIdx.x; k < c; k += kIdThreads) {
        double z = 0.0;
        for (int j = 0; j < r; ++j) z = fma((double)w2[k * r + j], s_h[j], z);
        g[n * c + k] = (float)(1.0 / (1.0 + exp(-z)));
    }
}

// ds = W1^T ((W2^T (dg g (1 - g))) masked by hidden > 0); the hidden units are recomputed from s.
__global__ void __launch_bounds__(kIdThreads)
id_se_gate_bwd_kernel(const float* __restrict__ s, const float* __restrict__ w1, const float* __restrict__ w2, const float* __restrict__ g,
                      const float* __restrict__ dg, float* __restrict__ ds, int c, int r) {
    __shared__ float s_s[kSeMaxC];
    __shared__ double s_dz[kSeMaxC], s_part[kIdThreads], s_h[kSeMaxR], s_dh[kSeMaxR];
    const int64_t n = blockIdx.x;
    for (int k = threadIdx.x; k < c; k += kIdThreads) {
        s_s[k] = s[n * c + k];
        const double gv = (double)g[n * c + k];
        s_dz[k] = (double)dg[n * c + k] * gv * (1.0 - gv);
    }
    __syncthreads();
    se_hidden(w1, s_s, c, r, s_part, s_h);
    const int j = threadIdx.x / kSeLanes, l = threadIdx.x % kSeLanes;
    double acc = 0.0;
    if (j < r)
        for (int k = l; k < c; k += kSeLanes) acc = fma((double)w2[k * r + j], s_dz[k], acc);
    s_part[threadIdx.x] = acc;
    __syncthreads();
    if ((int)threadIdx.x < r) {
        double t = 0.0;
        for (int q = 0; q < kSeLanes; ++q) t += s_part[threadIdx.x * kSeLanes + q];
        s_dh[threadIdx.x] = s_h[threadIdx.x] > 0.0 ? t : 0.0;
    }
    __syncthreads();
    for (int k = threadIdx.x; k < c; k += kIdThreads) {
        double t = 0.0;
        for (int q = 0; q < r; ++q) t = fma((double)w1[q * c + k], s_dh[q], t);
        ds[n * c + k] = (float)t;
    }
}

// ---- linear layer -------------------------------------------------------------------------------------------------------------------------------
// Forward.  Workgroup (bx, by) takes rows 8 bx .. 8 bx + 7 of W over the slice [2048 by, 2048 by + 2048) of K: a wave owns two rows, a lane
// reads 16 bytes of each row per step (a wave reads 1 KiB of a row at once) and keeps one sum per row and image; x (n K floats) comes out
// of the cache.  partial[by, i, m] = the slice's sum for image i and row m.
__global__ void __launch_bounds__(kIdThreads)
id_linear_partial_kernel(const float* __restrict__ x, const float* __restrict__ wt, float* __restrict__ partial, int n, int K, int M) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int m0 = blockIdx.x * kLinRows + wave * 2;
    const int k0 = blockIdx.y * kLinChunk;
    if (m0 >= M) return;                                                     // (no barrier below)
    const bool two = m0 + 1 < M;
    const float* __restrict__ wa = wt + (int64_t)m0 * K;
    const float* __restrict__ wb = wt + (int64_t)(two ? m0 + 1 : m0) * K;
    float acc_a[kLinMaxN], acc_b[kLinMaxN];
#pragma unroll
    for (int i = 0; i < kLinMaxN; ++i) acc_a[i] = acc_b[i] = 0.f;
#pragma unroll
    for (int it = 0; it < kLinChunk / 256; ++it) {
        const int k = k0 + it * 256 + lane * 4;
        if (k < K) {                                                         // K % 4 == 0: a 16-byte group is inside or outside as a whole
            const float4 a = *reinterpret_cast<const float4*>(wa + k), b = *reinterpret_cast<const float4*>(wb + k);
#pragma unroll
            for (int i = 0; i < kLinMaxN; ++i)
                if (i < n) {
                    const float4 v = *reinterpret_cast<const float4*>(x + (int64_t)i * K + k);
                    acc_a[i] = fmaf(a.w, v.w, fmaf(a.z, v.z, fmaf(a.y, v.y, fmaf(a.x, v.x, acc_a[i]))));
                    acc_b[i] = fmaf(b.w, v.w, fmaf(b.z, v.z, fmaf(b.y, v.y, fmaf(b.x, v.x, acc_b[i]))));
                }
        }
    }
#pragma unroll
    for (int i = 0; i < kLinMaxN; ++i)
        if (i < n) {
            float va = acc_a[i], vb = acc_b[i];
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) {
                va += __shfl_xor(va, off);
                vb += __shfl_xor(vb, off);
            }
            if (lane == 0) {
                float* __restrict__ q = partial + ((int64_t)blockIdx.y * n + i) * M + m0;
                q[0] = va;
                if (two) q[1] = vb;
            }
        }
}

// out[e] = bias? + the sum over the slices of partial[s, e], ascending, in float64; `period`: the bias index is e % period.
__global__ void __launch_bounds__(kIdThreads)
id_linear_finish_kernel(const float* __restrict__ partial, const float* __restrict__ bias, float* __restrict__ out, int slices, int64_t count,
                        int period) {
    for (int64_t e = (int64_t)blockIdx.x * kIdThreads + threadIdx.x; e < count; e += (int64_t)gridDim.x * kIdThreads) {
        double acc = bias ? (double)bias[e % period] : 0.0;
        for (int s = 0; s < slices; ++s) acc += (double)partial[s * count + e];
        out[e] = (float)acc;
    }
}

// Input gradient.  A thread owns 4 consecutive k and walks 64 rows of W (a wave reads 1 KiB of a row at once); dy[i, m] is uniform over
// the wave.  partial[by, i, k] = the sum over rows [64 by, 64 by + 64).
__global__ void __launch_bounds__(kLinBwdThreads)
id_linear_bwd_partial_kernel(const float* __restrict__ dy, const float* __restrict__ wt, float* __restrict__ partial, int n, int K, int M) {
    const int k = (blockIdx.x * kLinBwdThreads + threadIdx.x) * 4;
    if (k >= K) return;
    const int m0 = blockIdx.y * kLinBwdRows, m1 = min(M, m0 + kLinBwdRows);
    float4 acc[kLinMaxN];
#pragma unroll
    for (int i = 0; i < kLinMaxN; ++i) acc[i] = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll 4
    for (int m = m0; m < m1; ++m) {
        const float4 v = *reinterpret_cast<const float4*>(wt + (int64_t)m * K + k);
#pragma unroll
        for (int i = 0; i < kLinMaxN; ++i)
            if (i < n) {
                const float d = dy[i * M + m];
                acc[i].x = fmaf(d, v.x, acc[i].x); acc[i].y = fmaf(d, v.y, acc[i].y);
                acc[i].z = fmaf(d, v.z, acc[i].z); acc[i].w = fmaf(d, v.w, acc[i].w);
            }
    }
#pragma unroll
    for (int i = 0; i < kLinMaxN; ++i)
        if (i < n) *reinterpret_cast<float4*>(partial + ((int64_t)blockIdx.y * n + i) * K + k) = acc[i];
}

// ---- normalised-embedding head -----------------------------------------------------------------------------------------------------------------
// One workgroup walks the images in order: |f_i| (float64), e_i = f_i / |f_i|, and with targets 1 - e_i . t_i added to the loss.
__global__ void __launch_bounds__(kIdThreads)
id_head_kernel(const float* __restrict__ f, const float* __restrict__ t, float* __restrict__ e, float* __restrict__ norm, float* __restrict__ loss,
               int n, int M) {
    __shared__ double s_red[kIdThreads];
    double total = 0.0;
    for (int i = 0; i < n; ++i) {
        const float* __restrict__ fi = f + (int64_t)i * M;
        double ss = 0.0;
        for (int k = threadIdx.x; k < M; k += kIdThreads) ss = fma((double)fi[k], (double)fi[k], ss);
        const double nrm = sqrt(id_block_sum(ss, s_red));
        double dot = 0.0;
        for (int k = threadIdx.x; k < M; k += kIdThreads) {
            const float ev = (float)((double)fi[k] / nrm);
            e[(int64_t)i * M + k] = ev;
            if (t) dot = fma((double)ev, (double)t[(int64_t)i * M + k], dot);
        }
        if (threadIdx.x == 0) norm[i] = (float)nrm;
        if (t) total += 1.0 - id_block_sum(dot, s_red);
    }
    if (t && threadIdx.x == 0) loss[0] = (float)(total / (double)n);
}

// df_i = (g - e_i (e_i . g)) / |f_i| with g = -dloss t_i / n; one workgroup per image.
__global__ void __launch_bounds__(kIdThreads)
id_head_bwd_kernel(const float* __restrict__ e, const float* __restrict__ t, const float* __restrict__ norm, const float* __restrict__ dloss,
                   float* __restrict__ df, int n, int M) {
    __shared__ double s_red[kIdThreads];
    const int64_t base = (int64_t)blockIdx.x * M;
    const double scale = -(double)dloss[0] / (double)n;
    double dot = 0.0;
    for (int k = threadIdx.x; k < M; k += kIdThreads) dot = fma((double)e[base + k], scale * (double)t[base + k], dot);
    const double eg = id_block_sum(dot, s_red), nrm = (double)norm[blockIdx.x];
    for (int k = threadIdx.x; k < M; k += kIdThreads) df[base + k] = (float)((scale * (double)t[base + k] - (double)e[base + k] * eg) / nrm);
}

static bool id_prep_ok(int32_t n, int32_t f) { return n >= 1 && n <= (1 << 20) && f >= 1 && f <= kIdMaxFactor; }

static bool id_linear_ok(int32_t n, int32_t K, int32_t M) {
    return n >= 1 && n <= kLinMaxN && K >= 4 && K % 4 == 0 && K <= (1 << 24) && M >= 1 && M <= 65535 * kLinRows && (int64_t)K * M < (1LL << 40)
           && cdiv(K, kLinChunk) <= 65535 && cdiv(M, kLinBwdRows) <= 65535;
}

}  // namespace ide3d

using namespace ide3d;

extern "C" int ide3d_id_prep(const float* x, float* y, int32_t n, int32_t f, void* stream) {
    IDE3D_CHECK_ARG(x && y, "id_prep: null pointer");
    IDE3D_CHECK_ARG(id_prep_ok(n, f), "id_prep: x [n, 3, 256 f, 256 f] with 1 <= f <= %d", kIdMaxFactor);
    const int64_t planes = (int64_t)n * 3;
    hipLaunchKernelGGL(id_prep_kernel, id_grid(planes, kIdOut * kIdOut), dim3(kIdThreads), 0, (hipStream_t)stream, x, y, f, planes);
    IDE3D_CHECK_LAUNCH("id_prep");
    return IDE3D_OK;
}

extern "C" int ide3d_id_prep_backward(const float* dy, float* dx, int32_t n, int32_t f, void* stream) {
    IDE3D_CHECK_ARG(dy && dx, "id_prep_backward: null pointer");
    IDE3D_CHECK_ARG(id_prep_ok(n, f), "id_prep_backward: dx [n, 3, 256 f, 256 f] with 1 <= f <= %d", kIdMaxFactor);
    const int64_t planes = (int64_t)n * 3, side = (int64_t)kIdFrame * f;
    hipLaunchKernelGGL(id_prep_bwd_kernel, id_grid(planes, side * side), dim3(kIdThreads), 0, (hipStream_t)stream, dy, dx, f, planes);
    IDE3D_CHECK_LAUNCH("id_prep_backward");
    return IDE3D_OK;
}

extern "C" int ide3d_prelu(const float* x, const float* slope, float* y, int32_t n, int32_t c, int32_t h, int32_t w, void* stream) {
    IDE3D_CHECK_ARG(x && slope && y, "prelu: null pointer");
    IDE3D_CHECK_ARG(n >= 1 && c >= 1 && h >= 1 && w >= 1 && (int64_t)h * w < (1LL << 30) && (int64_t)n * c * h * w < (1LL << 40),
                    "prelu: x [n, c, h, w], slope [c]");
    const int64_t planes = (int64_t)n * c;
    const int hw = h * w;
    hipStream_t st = (hipStream_t)stream;
    if (hw % 4 == 0 && ptr_aligned(x, 16) && ptr_aligned(y, 16))
        hipLaunchKernelGGL(id_prelu_kernel<true>, id_grid(planes, hw / 4), dim3(kIdThreads), 0, st, x, slope, y, c, hw, planes);
    else
        hipLaunchKernelGGL(id_prelu_kernel<false>, id_grid(planes, hw), dim3(kIdThreads), 0, st, x, slope, y, c, hw, planes);
    IDE3D_CHECK_LAUNCH("prelu");
    return IDE3D_OK;
}

extern "C" int ide3d_prelu_backward(const float* dy, int64_t dy_batch_stride, int64_t dy_plane_stride, int32_t dy_row_pitch, const float* x,
                                    const float* slope, float* dx, int32_t n, int32_t c, int32_t h, int32_t w, void* stream) {
    IDE3D_CHECK_ARG(dy && x && slope && dx, "prelu_backward: null pointer");
    IDE3D_CHECK_ARG(n >= 1 && c >= 1 && h >= 1 && w >= 1 && (int64_t)h * w < (1LL << 30) && (int64_t)n * c * h * w < (1LL << 40),
                    "prelu_backward: x [n, c, h, w], slope [c]");
    IDE3D_CHECK_ARG(dy_row_pitch >= w && dy_plane_stride >= (int64_t)(h - 1) * dy_row_pitch + w && dy_batch_stride >= (c - 1) * dy_plane_stride + 1,
                    "prelu_backward: dy's row pitch, plane stride and batch stride must cover its [n, c, h, w]");
    const int64_t planes = (int64_t)n * c;
    const int hw = h * w;
    const bool dense = dy_row_pitch == w && dy_plane_stride == hw && dy_batch_stride == (int64_t)c * hw;
    hipStream_t st = (hipStream_t)stream;
    if (dense && hw % 4 == 0 && ptr_aligned(dy, 16) && ptr_aligned(x, 16) && ptr_aligned(dx, 16))
        hipLaunchKernelGGL(id_prelu_bwd_kernel<true>, id_grid(planes, hw / 4), dim3(kIdThreads), 0, st, dy, dy_batch_stride, dy_plane_stride,
                           dy_row_pitch, x, slope, dx, c, h, w, planes);
    else
        hipLaunchKernelGGL(id_prelu_bwd_kernel<false>, id_grid(planes, hw), dim3(kIdThreads), 0, st, dy, dy_batch_stride, dy_plane_stride,
                           dy_row_pitch, x, slope, dx, c, h, w, planes);
    IDE3D_CHECK_LAUNCH("prelu_backward");
    return IDE3D_OK;
}

extern "C" int ide3d_se_gate(const float* s, const float* w1, const float* w2, float* g, int32_t n, int32_t c, int32_t r, void* stream) {
    IDE3D_CHECK_ARG(s && w1 && w2 && g, "se_gate: null pointer");
    IDE3D_CHECK_ARG(n >= 1 && c >= 1 && c <= kSeMaxC && r >= 1 && r <= kSeMaxR, "se_gate: s [n, c <= %d], w1 [r <= %d, c], w2 [c, r]", kSeMaxC, kSeMaxR);
    hipLaunchKernelGGL(id_se_gate_kernel, dim3((unsigned)n), dim3(kIdThreads), 0, (hipStream_t)stream, s, w1, w2, g, c, r);
    IDE3D_CHECK_LAUNCH("se_gate");
    return IDE3D_OK;
}

extern "C" int ide3d_se_gate_backward(const float* s, const float* w1, const float* w2, const float* g, const float* dg, float* ds, int32_t n,
                                      int32_t c, int32_t r, void* stream) {
    IDE3D_CHECK_ARG(s && w1 && w2 && g && dg && ds, "se_gate_backward: null pointer");
    IDE3D_CHECK_ARG(n >= 1 && c >= 1 && c <= kSeMaxC && r >= 1 && r <= kSeMaxR, "se_gate_backward: s [n, c <= %d], w1 [r <= %d, c], w2 [c, r]", kSeMaxC,
                    kSeMaxR);
    hipLaunchKernelGGL(id_se_gate_bwd_kernel, dim3((unsigned)n), dim3(kIdThreads), 0, (hipStream_t)stream, s, w1, w2, g, dg, ds, c, r);
    IDE3D_CHECK_LAUNCH("se_gate_backward");
    return IDE3D_OK;
}

extern "C" int64_t ide3d_linear_workspace_bytes(int32_t n, int32_t K, int32_t M) {
    if (!id_linear_ok(n, K, M)) return -1;
    return (int64_t)cdiv(K, kLinChunk) * n * M * (int64_t)sizeof(float);
}

extern "C" int64_t ide3d_linear_backward_input_workspace_bytes(int32_t n, int32_t K, int32_t M) {
    if (!id_linear_ok(n, K, M)) return -1;
    return (int64_t)cdiv(M, kLinBwdRows) * n * K * (int64_t)sizeof(float);
}

extern "C" int ide3d_linear(const float* x, const float* weight, const float* bias, float* y, int32_t n, int32_t K, int32_t M, float* workspace,
                            int64_t workspace_bytes, void* stream) {
    IDE3D_CHECK_ARG(x && weight && y, "linear: null pointer");
    IDE3D_CHECK_ARG(id_linear_ok(n, K, M), "linear: x [n <= %d, K], weight [M, K] with K a multiple of 4", kLinMaxN);
    IDE3D_CHECK_ARG(ptr_aligned(x, 16) && ptr_aligned(weight, 16), "linear: x and weight must be 16-byte aligned");
    const int slices = cdiv(K, kLinChunk);
    IDE3D_CHECK_ARG(workspace && workspace_bytes >= (int64_t)slices * n * M * (int64_t)sizeof(float), "linear: workspace too small");
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(id_linear_partial_kernel, dim3(cdiv(M, kLinRows), slices), dim3(kIdThreads), 0, st, x, weight, workspace, n, K, M);
    const int64_t count = (int64_t)n * M;
    hipLaunchKernelGGL(id_linear_finish_kernel, dim3(stream_grid(count, kIdThreads)), dim3(kIdThreads), 0, st, (const float*)workspace, bias, y,
                       slices, count, M);
    IDE3D_CHECK_LAUNCH("linear");
    return IDE3D_OK;
}

extern "C" int ide3d_linear_backward_input(const float* dy, const float* weight, float* dx, int32_t n, int32_t K, int32_t M, float* workspace,
                                           int64_t workspace_bytes, void* stream) {
    IDE3D_CHECK_ARG(dy && weight && dx, "linear_backward_input: null pointer");
    IDE3D_CHECK_ARG(id_linear_ok(n, K, M), "linear_backward_input: dy [n <= %d, M], weight [M, K] with K a multiple of 4", kLinMaxN);
    IDE3D_CHECK_ARG(ptr_aligned(weight, 16), "linear_backward_input: weight must be 16-byte aligned");
    const int slices = cdiv(M, kLinBwdRows);
    IDE3D_CHECK_ARG(workspace && ptr_aligned(workspace, 16) && workspace_bytes >= (int64_t)slices * n * K * (int64_t)sizeof(float),
                    "linear_backward_input: workspace too small or misaligned");
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(id_linear_bwd_partial_kernel, dim3(cdiv(K / 4, kLinBwdThreads), slices), dim3(kLinBwdThreads), 0, st, dy, weight, workspace,
                       n, K, M);
    const int64_t count = (int64_t)n * K;
    hipLaunchKernelGGL(id_linear_finish_kernel, dim3(stream_grid(count, kIdThreads)), dim3(kIdThreads), 0, st, (const float*)workspace,
                       (const float*)nullptr, dx, slices, count, 1);
    IDE3D_CHECK_LAUNCH("linear_backward_input");
    return IDE3D_OK;
}

extern "C" int ide3d_id_head(const float* f, const float* target, float* e, float* norm, float* loss, int32_t n, int32_t M, void* stream) {
    IDE3D_CHECK_ARG(f && e && norm && (target == nullptr || loss != nullptr), "id_head: null pointer");
    IDE3D_CHECK_ARG(n >= 1 && n <= 65535 && M >= 1 && M <= kHeadMaxM, "id_head: f [n, M <= %d]", kHeadMaxM);
    hipLaunchKernelGGL(id_head_kernel, dim3(1), dim3(kIdThreads), 0, (hipStream_t)stream, f, target, e, norm, loss, n, M);
    IDE3D_CHECK_LAUNCH("id_head");
    return IDE3D_OK;
}

extern "C" int ide3d_id_head_backward(const float* e, const float* target, const float* norm, const float* dloss, float* df, int32_t n, int32_t M,
                                      void* stream) {
    IDE3D_CHECK_ARG(e && target && norm && dloss && df, "id_head_backward: null pointer");
    IDE3D_CHECK_ARG(n >= 1 && n <= 65535 && M >= 1 && M <= kHeadMaxM, "id_head_backward: e [n, M <= %d]", kHeadMaxM);
    hipLaunchKernelGGL(id_head_bwd_kernel, dim3((unsigned)n), dim3(kIdThreads), 0, (hipStream_t)stream, e, target, norm, dloss, df, n, M);
    IDE3D_CHECK_LAUNCH("id_head_backward");
    return IDE3D_OK;
}
