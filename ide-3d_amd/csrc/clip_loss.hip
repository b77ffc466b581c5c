// clip_loss.hip — everything of the CLIP image-text loss and its image gradient that is not a dense product.
//
// The dense products of the ViT image encoder (training/clip_loss.py) - the patch embedding, in_proj, out_proj, c_fc, c_proj and their
// input gradients - are shared-weight 1x1 launches of ide3d_modconv2d over channel-major token maps [n, C, T]; the residual adds are
// ide3d_residual_join, the final projection ide3d_linear / ide3d_linear_backward_input.  This file holds the rest, all over dense fp32:
//   ide3d_clip_prep / _backward             7x nearest up-sampling, S/32 average pooling, the optional per-channel affine and the patch
//                                           unfolding in one pass (integer window counts); the adjoint in gather form;
//   ide3d_vit_embed / _backward             patch tokens + class / positional table -> ln_pre; LayerNorm backward to the patch tokens;
//   ide3d_layernorm / _backward             LayerNorm over C per token of [n, C, T] (a row pitch lets T = 1 read the class column in
//                                           place); the backward goes to the input and adds the residual stream's gradient;
//   ide3d_vit_attention / _backward         one workgroup per (image, head): q, k, v and the T x T probabilities in LDS;
//   ide3d_quickgelu / _backward             v * sigmoid(1.702 v), the backward from the pre-activation;
//   ide3d_clip_head / _backward             e = (f - base) / |f - base|, out = 1 - e . t / |t| and its closed-form gradient.
// Lanes run along the contiguous (token) axis.  Deterministic: no atomics, every sum has a fixed order (a thread's own ascending loop,
// then an ascending loop or a tree over thread indices).  Sums that end in one number (means, variances, norms, softmax denominators, the
// row dots of the softmax gradient) are carried in float64; the products of the attention (<= 64 terms each) are fp32 FMAs.  Plain fp32 /
// fp64 arithmetic on the vector pipe (no packed fp32: the library is built without it); no matrix loop in this file, so section 4.2's
// exclusive residency does not apply.
#include "common.h"

namespace ide3d {

constexpr int kClipThreads = 256;
constexpr int kClipSide = 224, kClipUp = 7, kClipMaxK = 256;          // Upsample(7) then AvgPool2d(k = S / 32): S = 32 k -> 224
constexpr int kLnTokens = 64, kLnGroups = kClipThreads / kLnTokens;
constexpr int kAttMaxT = 64, kAttMaxD = 64;
constexpr int kAttMaxLds = (4 * kAttMaxT * (kAttMaxD + 1) + 2 * kAttMaxT * (kAttMaxT + 1)) * 4;          // the backward at T = d = 64: 99,840 bytes
constexpr int kClipHeadMaxD = 8192;
constexpr double kQuickGelu = 1.702;

// Sum of v over the workgroup in a fixed order (a binary tree over thread indices); every thread receives it.
__device__ __forceinline__ double clip_block_sum(double v, double* s_red) {
    __syncthreads();
    s_red[threadIdx.x] = v;
    __syncthreads();
#pragma unroll
    for (int off = kClipThreads / 2; off > 0; off >>= 1) {
        if ((int)threadIdx.x < off) s_red[threadIdx.x] += s_red[threadIdx.x + off];
        __syncthreads();
    }
    return s_red[0];
}

// ---- up-sampling, pooling, affine, unfolding ---------------------------------------------------------------------------------------------------
// Pooled row Y of the 224 averages up-sampled rows [Y k, Y k + k); up-sampled row r is source row r / 7.  Source row s therefore enters
// with the integer count |[Y k, Y k + k) n [7 s, 7 s + 7)| over k.
__device__ __forceinline__ int clip_count(int Y, int s, int k) { return min(Y * k + k, kClipUp * s + kClipUp) - max(Y * k, kClipUp * s); }

// col[n, (ci p + ky) p + kx, gy, gx] = affine(pooled[n, ci, gy p + ky, gx p + kx]); one thread per element of col.
__global__ void __launch_bounds__(kClipThreads)
clip_prep_kernel(const float* __restrict__ x, const float* __restrict__ mean, const float* __restrict__ std, float* __restrict__ col, int k, int p,
                 int64_t total) {
    const int S = 32 * k, g = kClipSide / p, gg = g * g;
    for (int64_t o = (int64_t)blockIdx.x * kClipThreads + threadIdx.x; o < total; o += (int64_t)gridDim.x * kClipThreads) {
        const int gx = (int)(o % g), gy = (int)((o / g) % g);
        const int64_t row = o / gg;                                            // n * 3 p p + (ci p + ky) p + kx
        const int kx = (int)(row % p), ky = (int)((row / p) % p);
        const int64_t plane = row / (p * p);                                   // n * 3 + ci
        const int Y = gy * p + ky, X = gx * p + kx;
        const int s0 = (Y * k) / kClipUp, s1 = (Y * k + k - 1) / kClipUp, t0 = (X * k) / kClipUp, t1 = (X * k + k - 1) / kClipUp;
        const float* __restrict__ src = x + plane * S * (int64_t)S;
        double acc = 0.0;
        for (int s = s0; s <= s1; ++s) {
            double line = 0.0;
            for (int t = t0; t <= t1; ++t) line += (double)clip_count(X, t, k) * (double)src[(int64_t)s * S + t];
            acc += (double)clip_count(Y, s, k) * line;
        }
        double v = acc / (double)(k * k);
        if (mean) {
            const int ci = (int)(plane % 3);
            v = ((v + 1.0) * 0.5 - (double)mean[ci]) / (double)std[ci];
        }
        col[o] = (float)v;
    }
}

// dx[n, ci, s, t] = (0.5 / std_ci)? / k^2 * sum over the pooled rows Y and columns X whose windows hold (s, t), ascending, of
// count(Y, s) count(X, t) dcol[...]; one thread per input pixel.
__global__ void __launch_bounds__(kClipThreads)
clip_prep_bwd_kernel(const float* __restrict__ dcol, const float* __restrict__ std, float* __restrict__ dx, int k, int p, int64_t total) {
    const int S = 32 * k, g = kClipSide / p, gg = g * g;
    for (int64_t e = (int64_t)blockIdx.x * kClipThreads + threadIdx.x; e < total; e += (int64_t)gridDim.x * kClipThreads) {
        const int t = (int)(e % S), s = (int)((e / S) % S);
        const int64_t plane = e / ((int64_t)S * S);
        const int Y0 = (kClipUp * s) / k, Y1 = (kClipUp * s + kClipUp - 1) / k, X0 = (kClipUp * t) / k, X1 = (kClipUp * t + kClipUp - 1) / k;
        const float* __restrict__ q = dcol + plane * p * p * (int64_t)gg;
        double acc = 0.0;
        for (int Y = Y0; Y <= Y1; ++Y) {
            const int gy = Y / p, ky = Y - gy * p;
            double line = 0.0;
            for (int X = X0; X <= X1; ++X) {
                const int gx = X / p, kx = X - gx * p;
                line += (double)clip_count(X, t, k) * (double)q[(int64_t)(ky * p + kx) * gg + gy * g + gx];
            }
            acc += (double)clip_count(Y, s, k) * line;
        }
        double v = acc / (double)(k * k);
        if (std) v = v * 0.5 / (double)std[plane % 3];
        dx[e] = (float)v;
    }
}

// ---- LayerNorm over the channels of a token map ------------------------------------------------------------------------------------------------
// Workgroup (bx, by) = tokens [64 bx, 64 bx + 64) of image by.  Thread (lane, grp): token 64 bx + lane, channels grp, grp + 4, ... in
// ascending order; the four partial sums of a token are added in ascending order in float64.
// kEmbed: the value at (c, t) is table[c, t] + (t > 0 ? x[n, c, t - 1] : 0) with x [n, C, T - 1] (the patch tokens behind the class token;
// table = positional embedding transposed, class embedding added to column 0); else x[n, c, t] with rows of `pitch` floats.
template <bool kEmbed>
__device__ __forceinline__ float ln_value(const float* __restrict__ x, const float* __restrict__ table, int64_t n, int c, int t, int C, int T, int pitch) {
    if (kEmbed) {
        const float tv = table[(int64_t)c * T + t];
        return t > 0 ? x[(n * C + c) * (int64_t)(T - 1) + t - 1] + tv : tv;
    }
    return x[(n * C + c) * (int64_t)pitch + t];
}

// The ascending sum of the kLnGroups partials of this thread's token; every thread of the token receives it.
__device__ __forceinline__ double ln_token_sum(double v, double (*s_part)[kLnTokens]) {
    const int lane = threadIdx.x & (kLnTokens - 1), grp = threadIdx.x / kLnTokens;
    __syncthreads();
    s_part[grp][lane] = v;
    __syncthreads();
    double t = 0.0;
#pragma unroll
    for (int q = 0; q < kLnGroups; ++q) t += s_part[q][lane];
    return t;
}

template <bool kEmbed>
__global__ void __launch_bounds__(kClipThreads)
ln_kernel(const float* __restrict__ x, const float* __restrict__ table, const float* __restrict__ gamma, const float* __restrict__ beta,
          float* __restrict__ y, float* __restrict__ mean, float* __restrict__ rstd, int C, int T, int pitch, float eps) {
    __shared__ double s_part[kLnGroups][kLnTokens];
    const int lane = threadIdx.x & (kLnTokens - 1), grp = threadIdx.x / kLnTokens;
    const int t = blockIdx.x * kLnTokens + lane;
    const int64_t n = blockIdx.y;
    const bool live = t < T;                                                  // (dead lanes still meet the barriers)
    double acc = 0.0;
    if (live)
        for (int c = grp; c < C; c += kLnGroups) acc += (double)ln_value<kEmbed>(x, table, n, c, t, C, T, pitch);
    const double mu = ln_token_sum(acc, s_part) / (double)C;
    acc = 0.0;
    if (live)
        for (int c = grp; c < C; c += kLnGroups) {
            const double d = (double)ln_value<kEmbed>(x, table, n, c, t, C, T, pitch) - mu;
            acc = fma(d, d, acc);
        }
    const double rs = 1.0 / sqrt(ln_token_sum(acc, s_part) / (double)C + (double)eps);
    if (!live) return;
    if (grp == 0) {
        mean[n * T + t] = (float)mu;
        rstd[n * T + t] = (float)rs;
    }
    for (int c = grp; c < C; c += kLnGroups) {
        const double v = ((double)ln_value<kEmbed>(x, table, n, c, t, C, T, pitch) - mu) * rs;
        y[(n * C + c) * (int64_t)T + t] = (float)(v * (double)gamma[c] + (double)beta[c]);
    }
}

// dx = rstd (g - mean_c g - xhat mean_c (g xhat)) (+ add), g = dy gamma, xhat = (x - mean) rstd with the SAVED fp32 mean and rstd.
// Plain: dx [n, C, pitch], columns T .. pitch - 1 receive an exact 0.  kEmbed: dx [n, C, T - 1], the class column is dropped.
template <bool kEmbed>
__global__ void __launch_bounds__(kClipThreads)
ln_bwd_kernel(const float* __restrict__ dy, const float* __restrict__ x, const float* __restrict__ table, const float* __restrict__ gamma,
              const float* __restrict__ mean, const float* __restrict__ rstd, const float* __restrict__ add, float* __restrict__ dx, int C, int T,
              int pitch) {
    __shared__ double s_part[kLnGroups][kLnTokens];
    const int lane = threadIdx.x & (kLnTokens - 1), grp = threadIdx.x / kLnTokens;
    const int t = blockIdx.x * kLnTokens + lane;
    const int64_t n = blockIdx.y;
    const bool live = t < T;
    const double mu = live ? (double)mean[n * T + t] : 0.0, rs = live ? (double)rstd[n * T + t] : 0.0;
    double a = 0.0, b = 0.0;
    if (live)
        for (int c = grp; c < C; c += kLnGroups) {
            const double g = (double)dy[(n * C + c) * (int64_t)T + t] * (double)gamma[c];
            const double xh = ((double)ln_value<kEmbed>(x, table, n, c, t, C, T, pitch) - mu) * rs;
            a += g;
            b = fma(g, xh, b);
        }
    a = ln_token_sum(a, s_part) / (double)C;
    b = ln_token_sum(b, s_part) / (double)C;
    if (live && !(kEmbed && t == 0))
        for (int c = grp; c < C; c += kLnGroups) {
            const double g = (double)dy[(n * C + c) * (int64_t)T + t] * (double)gamma[c];
            const double xh = ((double)ln_value<kEmbed>(x, table, n, c, t, C, T, pitch) - mu) * rs;
            const int64_t o = kEmbed ? (n * C + c) * (int64_t)(T - 1) + t - 1 : (n * C + c) * (int64_t)pitch + t;
            double v = rs * (g - a - xh * b);
            if (add) v += (double)add[o];
            dx[o] = (float)v;
        }
    if (!kEmbed) {                                                            // the columns past T of this image's rows (first token block only)
        if (blockIdx.x == 0)
            for (int64_t i = threadIdx.x; i < (int64_t)C * (pitch - T); i += kClipThreads) {
                const int64_t c = i / (pitch - T), tt = T + i - c * (pitch - T);
                dx[(n * C + c) * (int64_t)pitch + tt] = 0.f;
            }
    }
}

// ---- multi-head attention ---------------------------------------------------------------------------------------------------------------------
// Workgroup = (head, image).  LDS rows are padded by one float (d and the pitch below are then odd or even as it comes; d + 1 is odd since
// d % 4 == 0, so a wave that walks tokens at a fixed channel hits 32 different banks).  q, k, v: [T][d + 1]; scores: [T][T + 1].
__device__ __forceinline__ void att_load(const float* __restrict__ src, float* s_dst, int T, int d) {          // src [d, T] rows of T floats
    for (int i = threadIdx.x; i < d * T; i += kClipThreads) {
        const int c = i / T, t = i - c * T;
        s_dst[t * (d + 1) + c] = src[i];
    }
}

// s_p[i][j] = softmax_j(scale q_i . k_j): the dots by all threads, then one thread per row: maximum, exponentials and their float64 sum in
// ascending order, division.
__device__ __forceinline__ void att_probs(const float* s_q, const float* s_k, float* s_p, int T, int d, float scale) {
    for (int e = threadIdx.x; e < T * T; e += kClipThreads) {
        const int i = e / T, j = e - i * T;
        float acc = 0.f;
        for (int c = 0; c < d; ++c) acc = fmaf(s_q[i * (d + 1) + c], s_k[j * (d + 1) + c], acc);
        s_p[i * (T + 1) + j] = acc * scale;
    }
    __syncthreads();
    if ((int)threadIdx.x < T) {
        float* row = s_p + threadIdx.x * (T + 1);
        float m = row[0];
        for (int j = 1; j < T; ++j) m = fmaxf(m, row[j]);
        double sum = 0.0;
        for (int j = 0; j < T; ++j) {
            const float ev = expf(row[j] - m);
            row[j] = ev;
            sum += (double)ev;
        }
        for (int j = 0; j < T; ++j) row[j] = (float)((double)row[j] / sum);
    }
    __syncthreads();
}

__global__ void __launch_bounds__(kClipThreads)
vit_attention_kernel(const float* __restrict__ qkv, float* __restrict__ out, int C, int T, int d, float scale) {
    extern __shared__ float s_att[];
    float *s_q = s_att, *s_k = s_q + T * (d + 1), *s_v = s_k + T * (d + 1), *s_p = s_v + T * (d + 1);
    const int head = blockIdx.x;
    const int64_t n = blockIdx.y;
    const float* __restrict__ base = qkv + (n * 3 * C + (int64_t)head * d) * T;
    att_load(base, s_q, T, d);
    att_load(base + (int64_t)C * T, s_k, T, d);
    att_load(base + (int64_t)2 * C * T, s_v, T, d);
    __syncthreads();
    att_probs(s_q, s_k, s_p, T, d, scale);
    float* __restrict__ dst = out + (n * C + (int64_t)head * d) * T;
    for (int e = threadIdx.x; e < d * T; e += kClipThreads) {
        const int c = e / T, i = e - c * T;
        float acc = 0.f;
        for (int j = 0; j < T; ++j) acc = fmaf(s_p[i * (T + 1) + j], s_v[j * (d + 1) + c], acc);
        dst[e] = acc;
    }
}

// dV = P^T dO, dP = dO V^T, dS = P (dP - rowsum(dP P)), dQ = scale dS K, dK = scale dS^T Q; P is recomputed from q and k.
__global__ void __launch_bounds__(kClipThreads)
vit_attention_bwd_kernel(const float* __restrict__ qkv, const float* __restrict__ dout, float* __restrict__ dqkv, int C, int T, int d, float scale) {
    extern __shared__ float s_att[];
    float *s_q = s_att, *s_k = s_q + T * (d + 1), *s_v = s_k + T * (d + 1), *s_o = s_v + T * (d + 1), *s_p = s_o + T * (d + 1),
          *s_d = s_p + T * (T + 1);
    const int head = blockIdx.x;
    const int64_t n = blockIdx.y;
    const int64_t off = (n * 3 * C + (int64_t)head * d) * T;
    att_load(qkv + off, s_q, T, d);
    att_load(qkv + off + (int64_t)C * T, s_k, T, d);
    att_load(qkv + off + (int64_t)2 * C * T, s_v, T, d);
    att_load(dout + (n * C + (int64_t)head * d) * T, s_o, T, d);
    __syncthreads();
    att_probs(s_q, s_k, s_p, T, d, scale);
    for (int e = threadIdx.x; e < T * T; e += kClipThreads) {
        const int i = e / T, j = e - i * T;
        float acc = 0.f;
        for (int c = 0; c < d; ++c) acc = fmaf(s_o[i * (d + 1) + c], s_v[j * (d + 1) + c], acc);
        s_d[i * (T + 1) + j] = acc;
    }
    __syncthreads();
    float* __restrict__ dq = dqkv + off;
    float* __restrict__ dk = dq + (int64_t)C * T;
    float* __restrict__ dv = dk + (int64_t)C * T;
    for (int e = threadIdx.x; e < d * T; e += kClipThreads) {                 // dV reads P before it is turned into dS below
        const int c = e / T, j = e - c * T;
        float acc = 0.f;
        for (int i = 0; i < T; ++i) acc = fmaf(s_p[i * (T + 1) + j], s_o[i * (d + 1) + c], acc);
        dv[e] = acc;
    }
    __syncthreads();
    if ((int)threadIdx.x < T) {
        float* prow = s_p + threadIdx.x * (T + 1);
        const float* drow = s_d + threadIdx.x * (T + 1);
        double dot = 0.0;
        for (int j = 0; j < T; ++j) dot = fma((double)drow[j], (double)prow[j], dot);
        for (int j = 0; j < T; ++j) prow[j] = (float)((double)prow[j] * ((double)drow[j] - dot));
    }
    __syncthreads();
    for (int e = threadIdx.x; e < d * T; e += kClipThreads) {
        const int c = e / T, i = e - c * T;
        float aq = 0.f, ak = 0.f;
        for (int j = 0; j < T; ++j) {
            aq = fmaf(s_p[i * (T + 1) + j], s_k[j * (d + 1) + c], aq);
            ak = fmaf(s_p[j * (T + 1) + i], s_q[j * (d + 1) + c], ak);
        }
        dq[e] = aq * scale;
        dk[e] = ak * scale;
    }
}

// ---- QuickGELU ----------------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float quickgelu_fwd(float v) { return (float)((double)v / (1.0 + exp(-kQuickGelu * (double)v))); }
__device__ __forceinline__ float quickgelu_bwd(float g, float v) {
    const double s = 1.0 / (1.0 + exp(-kQuickGelu * (double)v));
    return (float)((double)g * (s + kQuickGelu * (double)v * s * (1.0 - s)));
}

// A thread owns 4 consecutive floats; kVec: every pointer is 16-byte aligned (whole groups are one 16-byte access); the last group of a
// count that is no multiple of 4, and every group without kVec, goes float by float.  dy: NULL = forward.
template <bool kVec, bool kBwd>
__global__ void __launch_bounds__(kClipThreads)
quickgelu_kernel(const float* __restrict__ x, const float* __restrict__ dy, float* __restrict__ out, int64_t count) {
    const int64_t i = ((int64_t)blockIdx.x * kClipThreads + threadIdx.x) * 4;
    if (i >= count) return;
    if (kVec && i + 4 <= count) {
        const float4 v = *reinterpret_cast<const float4*>(x + i);
        float4 r;
        if (kBwd) {
            const float4 g = *reinterpret_cast<const float4*>(dy + i);
            r = make_float4(quickgelu_bwd(g.x, v.x), quickgelu_bwd(g.y, v.y), quickgelu_bwd(g.z, v.z), quickgelu_bwd(g.w, v.w));
        } else {
            r = make_float4(quickgelu_fwd(v.x), quickgelu_fwd(v.y), quickgelu_fwd(v.z), quickgelu_fwd(v.w));
        }
        *reinterpret_cast<float4*>(out + i) = r;
        return;
    }
    const int64_t end = (i + 4 < count) ? i + 4 : count;
    for (int64_t j = i; j < end; ++j) out[j] = kBwd ? quickgelu_bwd(dy[j], x[j]) : quickgelu_fwd(x[j]);
}

// ---- cosine head --------------------------------------------------------------------------------------------------------------------------------
// One workgroup per image: |f - base| (float64), e, then per text row 1 - e . t / |t|; image 0 also writes |t|.  rowsum[i] = the float64 sum
// of the image's row before its values are rounded to fp32 (what the mean is made of).
__global__ void __launch_bounds__(kClipThreads)
clip_head_kernel(const float* __restrict__ f, const float* __restrict__ base, const float* __restrict__ t, float* __restrict__ e,
                 float* __restrict__ norm, float* __restrict__ tnorm, float* __restrict__ out, double* __restrict__ rowsum, int D, int T) {
    __shared__ double s_red[kClipThreads];
    const int64_t i = blockIdx.x;
    const float* __restrict__ fi = f + i * D;
    const float* __restrict__ bi = base ? base + i * D : nullptr;
    double ss = 0.0;
    for (int k = threadIdx.x; k < D; k += kClipThreads) {
        const double v = bi ? (double)fi[k] - (double)bi[k] : (double)fi[k];
        ss = fma(v, v, ss);
    }
    const double nrm = sqrt(clip_block_sum(ss, s_red));
    for (int k = threadIdx.x; k < D; k += kClipThreads) {
        const double v = bi ? (double)fi[k] - (double)bi[k] : (double)fi[k];
        e[i * D + k] = (float)(v / nrm);
    }
    if (threadIdx.x == 0) norm[i] = (float)nrm;
    double total = 0.0;
    for (int r = 0; r < T; ++r) {                                             // (a thread reads back the e[k] it wrote itself)
        const float* __restrict__ tr = t + (int64_t)r * D;
        double tt = 0.0, dot = 0.0;
        for (int k = threadIdx.x; k < D; k += kClipThreads) {
            const double tv = (double)tr[k];
            tt = fma(tv, tv, tt);
            dot = fma((double)e[i * D + k], tv, dot);
        }
        const double tn = sqrt(clip_block_sum(tt, s_red));
        const double dt = clip_block_sum(dot, s_red);
        if (threadIdx.x == 0) {
            const double v = 1.0 - dt / tn;
            total += v;
            out[i * T + r] = (float)v;
            if (i == 0) tnorm[r] = (float)tn;
        }
    }
    if (threadIdx.x == 0) rowsum[i] = total;
}

// mean[0] = the sum of the n row sums in ascending order, in float64, over n T: rounded to fp32 once.
__global__ void clip_head_mean_kernel(const double* __restrict__ rowsum, float* __restrict__ mean, int n, int T) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    double total = 0.0;
    for (int i = 0; i < n; ++i) total += rowsum[i];
    mean[0] = (float)(total / ((double)n * (double)T));
}

// df_i = (g - e_i (e_i . g)) / |f_i - base_i| with g = -sum_r dout[i, r] t_r / |t_r| (r ascending); one workgroup per image.
__device__ __forceinline__ double clip_head_g(const float* __restrict__ t, const float* __restrict__ tnorm, const float* __restrict__ dout_i, int k, int D,
                                              int T) {
    double g = 0.0;
    for (int r = 0; r < T; ++r) g -= (double)dout_i[r] * (double)t[(int64_t)r * D + k] / (double)tnorm[r];
    return g;
}

__global__ void __launch_bounds__(kClipThreads)
clip_head_bwd_kernel(const float* __restrict__ e, const float* __restrict__ t, const float* __restrict__ norm, const float* __restrict__ tnorm,
                     const float* __restrict__ dout, float* __restrict__ df, int D, int T) {
    __shared__ double s_red[kClipThreads];
    const int64_t i = blockIdx.x;
    const float* __restrict__ di = dout + i * T;
    double dot = 0.0;
    for (int k = threadIdx.x; k < D; k += kClipThreads) dot = fma((double)e[i * D + k], clip_head_g(t, tnorm, di, k, D, T), dot);
    const double eg = clip_block_sum(dot, s_red), nrm = (double)norm[i];
    for (int k = threadIdx.x; k < D; k += kClipThreads)
        df[i * D + k] = (float)((clip_head_g(t, tnorm, di, k, D, T) - (double)e[i * D + k] * eg) / nrm);
}

static bool clip_prep_ok(int32_t n, int32_t k, int32_t p) {
    return n >= 1 && n <= 65535 && k >= 1 && k <= kClipMaxK && p >= 1 && p <= kClipSide && kClipSide % p == 0;
}

static bool ln_ok(int32_t n, int32_t C, int32_t T, int32_t pitch) {
    return n >= 1 && n <= 65535 && C >= 1 && C <= (1 << 20) && T >= 1 && T <= (1 << 20) && pitch >= T && pitch <= (1 << 20)
           && (int64_t)n * C * pitch < (1LL << 40);
}

static bool att_ok(int32_t n, int32_t heads, int32_t d, int32_t T) {
    return n >= 1 && n <= 65535 && heads >= 1 && heads <= 65535 && d >= 4 && d <= kAttMaxD && d % 4 == 0 && T >= 1 && T <= kAttMaxT;
}

static size_t att_lds_bytes(int T, int d, bool backward) {
    return (size_t)((backward ? 4 : 3) * T * (d + 1) + (backward ? 2 : 1) * T * (T + 1)) * sizeof(float);
}

// A launch may use 64 KB of dynamic LDS as it is; more has to be allowed per kernel (and device) first: asked only then, result checked.
static bool att_allow_lds(const void* kernel, size_t lds) {
    if (lds <= 64 * 1024) return true;
    return hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kAttMaxLds) == hipSuccess;
}

static dim3 ln_grid(int32_t n, int32_t T) { return dim3((unsigned)cdiv(T, kLnTokens), (unsigned)n); }

}  // namespace ide3d

using namespace ide3d;

extern "C" int ide3d_clip_prep(const float* x, const float* mean, const float* std, float* col, int32_t n, int32_t k, int32_t p, void* stream) {
    IDE3D_CHECK_ARG(x && col && (mean == nullptr) == (std == nullptr), "clip_prep: null pointer (mean and std come together)");
    IDE3D_CHECK_ARG(clip_prep_ok(n, k, p), "clip_prep: x [n, 3, 32 k, 32 k] with 1 <= k <= %d, patch size p dividing 224", kClipMaxK);
    const int64_t total = (int64_t)n * 3 * kClipSide * kClipSide;
    hipLaunchKernelGGL(clip_prep_kernel, dim3(stream_grid(total, kClipThreads)), dim3(kClipThreads), 0, (hipStream_t)stream, x, mean, std, col, k, p,
                       total);
    IDE3D_CHECK_LAUNCH("clip_prep");
    return IDE3D_OK;
}

extern "C" int ide3d_clip_prep_backward(const float* dcol, const float* std, float* dx, int32_t n, int32_t k, int32_t p, void* stream) {
    IDE3D_CHECK_ARG(dcol && dx, "clip_prep_backward: null pointer");
    IDE3D_CHECK_ARG(clip_prep_ok(n, k, p), "clip_prep_backward: dx [n, 3, 32 k, 32 k] with 1 <= k <= %d, patch size p dividing 224", kClipMaxK);
    const int64_t total = (int64_t)n * 3 * (32 * k) * (32 * k);
    hipLaunchKernelGGL(clip_prep_bwd_kernel, dim3(stream_grid(total, kClipThreads)), dim3(kClipThreads), 0, (hipStream_t)stream, dcol, std, dx, k, p,
                       total);
    IDE3D_CHECK_LAUNCH("clip_prep_backward");
    return IDE3D_OK;
}

extern "C" int ide3d_vit_embed(const float* patches, const float* table, const float* gamma, const float* beta, float* y, float* mean, float* rstd,
                               int32_t n, int32_t C, int32_t T, float eps, void* stream) {
    IDE3D_CHECK_ARG(patches && table && gamma && beta && y && mean && rstd, "vit_embed: null pointer");
    IDE3D_CHECK_ARG(ln_ok(n, C, T, T) && T >= 2 && eps >= 0.f, "vit_embed: patches [n, C, T - 1], table [C, T] with T >= 2");
    hipLaunchKernelGGL(ln_kernel<true>, ln_grid(n, T), dim3(kClipThreads), 0, (hipStream_t)stream, patches, table, gamma, beta, y, mean, rstd, C, T, T,
                       eps);
    IDE3D_CHECK_LAUNCH("vit_embed");
    return IDE3D_OK;
}

extern "C" int ide3d_vit_embed_backward(const float* dy, const float* patches, const float* table, const float* gamma, const float* mean,
                                        const float* rstd, float* dpatches, int32_t n, int32_t C, int32_t T, void* stream) {
    IDE3D_CHECK_ARG(dy && patches && table && gamma && mean && rstd && dpatches, "vit_embed_backward: null pointer");
    IDE3D_CHECK_ARG(ln_ok(n, C, T, T) && T >= 2, "vit_embed_backward: dy [n, C, T], patches [n, C, T - 1], table [C, T] with T >= 2");
    hipLaunchKernelGGL(ln_bwd_kernel<true>, ln_grid(n, T), dim3(kClipThreads), 0, (hipStream_t)stream, dy, patches, table, gamma, mean, rstd,
                       (const float*)nullptr, dpatches, C, T, T);
    IDE3D_CHECK_LAUNCH("vit_embed_backward");
    return IDE3D_OK;
}

extern "C" int ide3d_layernorm(const float* x, const float* gamma, const float* beta, float* y, float* mean, float* rstd, int32_t n, int32_t C,
                               int32_t T, int32_t pitch, float eps, void* stream) {
    IDE3D_CHECK_ARG(x && gamma && beta && y && mean && rstd, "layernorm: null pointer");
    IDE3D_CHECK_ARG(ln_ok(n, C, T, pitch) && eps >= 0.f, "layernorm: x [n, C, pitch >= T], y [n, C, T]");
    hipLaunchKernelGGL(ln_kernel<false>, ln_grid(n, T), dim3(kClipThreads), 0, (hipStream_t)stream, x, (const float*)nullptr, gamma, beta, y, mean, rstd,
                       C, T, pitch, eps);
    IDE3D_CHECK_LAUNCH("layernorm");
    return IDE3D_OK;
}

extern "C" int ide3d_layernorm_backward(const float* dy, const float* x, const float* gamma, const float* mean, const float* rstd, const float* add,
                                        float* dx, int32_t n, int32_t C, int32_t T, int32_t pitch, void* stream) {
    IDE3D_CHECK_ARG(dy && x && gamma && mean && rstd && dx, "layernorm_backward: null pointer");
    IDE3D_CHECK_ARG(ln_ok(n, C, T, pitch), "layernorm_backward: dy [n, C, T], x, add and dx [n, C, pitch >= T]");
    hipLaunchKernelGGL(ln_bwd_kernel<false>, ln_grid(n, T), dim3(kClipThreads), 0, (hipStream_t)stream, dy, x, (const float*)nullptr, gamma, mean, rstd,
                       add, dx, C, T, pitch);
    IDE3D_CHECK_LAUNCH("layernorm_backward");
    return IDE3D_OK;
}

extern "C" int ide3d_vit_attention(const float* qkv, float* out, int32_t n, int32_t heads, int32_t d, int32_t T, float scale, void* stream) {
    IDE3D_CHECK_ARG(qkv && out, "vit_attention: null pointer");
    IDE3D_CHECK_ARG(att_ok(n, heads, d, T), "vit_attention: qkv [n, 3 heads d, T] with d a multiple of 4, d <= %d, T <= %d", kAttMaxD, kAttMaxT);
    const size_t lds = att_lds_bytes(T, d, false);
    IDE3D_CHECK_ARG(att_allow_lds(reinterpret_cast<const void*>(vit_attention_kernel), lds), "vit_attention: %zu bytes of LDS were refused", lds);
    hipLaunchKernelGGL(vit_attention_kernel, dim3((unsigned)heads, (unsigned)n), dim3(kClipThreads), lds, (hipStream_t)stream, qkv, out, heads * d, T, d,
                       scale);
    IDE3D_CHECK_LAUNCH("vit_attention");
    return IDE3D_OK;
}

extern "C" int ide3d_vit_attention_backward(const float* qkv, const float* dout, float* dqkv, int32_t n, int32_t heads, int32_t d, int32_t T,
                                            float scale, void* stream) {
    IDE3D_CHECK_ARG(qkv && dout && dqkv, "vit_attention_backward: null pointer");
    IDE3D_CHECK_ARG(att_ok(n, heads, d, T), "vit_attention_backward: qkv [n, 3 heads d, T] with d a multiple of 4, d <= %d, T <= %d", kAttMaxD,
                    kAttMaxT);
    const size_t lds = att_lds_bytes(T, d, true);
    IDE3D_CHECK_ARG(att_allow_lds(reinterpret_cast<const void*>(vit_attention_bwd_kernel), lds), "vit_attention_backward: %zu bytes of LDS were refused", lds);
    hipLaunchKernelGGL(vit_attention_bwd_kernel, dim3((unsigned)heads, (unsigned)n), dim3(kClipThreads), lds, (hipStream_t)stream, qkv, dout, dqkv,
                       heads * d, T, d, scale);
    IDE3D_CHECK_LAUNCH("vit_attention_backward");
    return IDE3D_OK;
}

static int quickgelu_launch(const float* x, const float* dy, float* out, int64_t count, void* stream, const char* what) {
    IDE3D_CHECK_ARG(x && out, "%s: null pointer", what);
    IDE3D_CHECK_ARG(count >= 1 && count < (1LL << 40), "%s: count must be in [1, 2^40)", what);
    uintptr_t bits = reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(out) | reinterpret_cast<uintptr_t>(dy);
    IDE3D_CHECK_ARG((bits & 3) == 0, "%s: operands must be 4-byte aligned", what);
    const bool vec = (bits & 15) == 0;
    const dim3 grid((unsigned)cdiv64(cdiv64(count, 4), kClipThreads)), block(kClipThreads);
    hipStream_t s = (hipStream_t)stream;
    if (dy) {
        if (vec) hipLaunchKernelGGL((quickgelu_kernel<true, true>), grid, block, 0, s, x, dy, out, count);
        else     hipLaunchKernelGGL((quickgelu_kernel<false, true>), grid, block, 0, s, x, dy, out, count);
    } else {
        if (vec) hipLaunchKernelGGL((quickgelu_kernel<true, false>), grid, block, 0, s, x, dy, out, count);
        else     hipLaunchKernelGGL((quickgelu_kernel<false, false>), grid, block, 0, s, x, dy, out, count);
    }
    IDE3D_CHECK_LAUNCH(what);
    return IDE3D_OK;
}

extern "C" int ide3d_quickgelu(const float* x, float* y, int64_t count, void* stream) {
    return quickgelu_launch(x, nullptr, y, count, stream, "quickgelu");
}

extern "C" int ide3d_quickgelu_backward(const float* dy, const float* x, float* dx, int64_t count, void* stream) {
    IDE3D_CHECK_ARG(dy, "quickgelu_backward: null pointer");
    return quickgelu_launch(x, dy, dx, count, stream, "quickgelu_backward");
}

extern "C" int ide3d_clip_head(const float* f, const float* base, const float* text, float* e, float* norm, float* tnorm, float* out, double* rowsum,
                               float* mean, int32_t n, int32_t D, int32_t T, void* stream) {
    IDE3D_CHECK_ARG(f && text && e && norm && tnorm && out && rowsum && mean, "clip_head: null pointer");
    IDE3D_CHECK_ARG(ptr_aligned(rowsum, 8), "clip_head: rowsum must be 8-byte aligned");
    IDE3D_CHECK_ARG(n >= 1 && n <= 65535 && D >= 1 && D <= kClipHeadMaxD && T >= 1 && T <= (1 << 20), "clip_head: f [n, D <= %d], text [T, D]",
                    kClipHeadMaxD);
    hipLaunchKernelGGL(clip_head_kernel, dim3((unsigned)n), dim3(kClipThreads), 0, (hipStream_t)stream, f, base, text, e, norm, tnorm, out, rowsum, D, T);
    hipLaunchKernelGGL(clip_head_mean_kernel, dim3(1), dim3(kWave), 0, (hipStream_t)stream, (const double*)rowsum, mean, n, T);
    IDE3D_CHECK_LAUNCH("clip_head");
    return IDE3D_OK;
}

extern "C" int ide3d_clip_head_backward(const float* e, const float* text, const float* norm, const float* tnorm, const float* dout, float* df,
                                        int32_t n, int32_t D, int32_t T, void* stream) {
    IDE3D_CHECK_ARG(e && text && norm && tnorm && dout && df, "clip_head_backward: null pointer");
    IDE3D_CHECK_ARG(n >= 1 && n <= 65535 && D >= 1 && D <= kClipHeadMaxD && T >= 1 && T <= (1 << 20),
                    "clip_head_backward: e [n, D <= %d], text [T, D], dout [n, T]", kClipHeadMaxD);
    hipLaunchKernelGGL(clip_head_bwd_kernel, dim3((unsigned)n), dim3(kClipThreads), 0, (hipStream_t)stream, e, text, norm, tnorm, dout, df, D, T);
    IDE3D_CHECK_LAUNCH("clip_head_backward");
    return IDE3D_OK;
}
