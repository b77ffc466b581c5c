// adv_loss.hip — what the StyleGAN2 discriminator's adversarial loss and its image gradient need beside convolutions, FIR passes, joins and
// linear layers (training/discriminator.py, training/adv_loss.py).
//
// The blocks of a frozen `resnet` discriminator are launches of ide3d_upfirdn2d, ide3d_modconv2d, ide3d_modconv_act_backward and
// ide3d_residual_join, its two dense layers are ide3d_linear / ide3d_linear_backward_input.  This file holds the rest, over dense fp32:
//   ide3d_minibatch_std / _backward      `MinibatchStdLayer.forward` with its concatenation, and the adjoint.  Sample g * (n / G) + j is
//                                        member g of group j (what `reshape(G, -1, ...)` makes of the batch).  One workgroup = one (group j,
//                                        feature f): it owns the c / F channels of f in the G samples of j, a contiguous run of c / F * h * w
//                                        floats per sample, and the statistic's plane c + f of those samples.
//                                        Backward: with s = sqrt(var_G + 1e-8) per (channel, pixel) and D[j, f] the sum of dy[:, c + f] over the
//                                        group and the pixels, d stat / d x_g = (x_g - mean_G) / (G s) / (c / F * h * w): the term that the
//                                        derivative of the subtracted mean would add is -(1 / G) sum_g' (x_g' - mean_G) / (G s), and the
//                                        deviations of a group sum to zero, so it drops out.  Each s is recomputed from x, not saved.
//   ide3d_adv_head / _backward           the conditional projection logit_i = o_i . cmap_i / sqrt(M) (cmap NULL: M = 1, logit = o) and the
//                                        logistic loss mean_i softplus(sign logit_i) in the form max(z, 0) + log1p(exp(-|z|)), which neither
//                                        overflows at large z nor loses the value at very negative z; the closed-form gradient.
// Deterministic: no atomics; every sum is a thread's own ascending loop, then a tree over thread indices, in float64, and rounded once.
// No host synchronisation.  Plain fp32 / fp64 arithmetic on the vector pipe (no packed fp32: the library is built without it); no matrix
// loop in this file, so section 4.2's exclusive residency does not apply.
#include "common.h"

namespace ide3d {

constexpr int kAdvThreads = 256;
constexpr int kAdvMaxM = 8192;
constexpr double kMbstdEps = 1e-8;

// Sum of v over the workgroup in a fixed order (a binary tree over thread indices); every thread receives it.
__device__ __forceinline__ double adv_block_sum(double v, double* s_red) {
    __syncthreads();
    s_red[threadIdx.x] = v;
    __syncthreads();
#pragma unroll
    for (int off = kAdvThreads / 2; off > 0; off >>= 1) {
        if ((int)threadIdx.x < off) s_red[threadIdx.x] += s_red[threadIdx.x + off];
        __syncthreads();
    }
    return s_red[0];
}

// mean and sqrt(var + eps) over the G members of a group at one (channel, pixel): p points at member 0, members are `step` floats apart.
__device__ __forceinline__ void mbstd_moments(const float* __restrict__ p, int64_t step, int G, double& mean, double& sd) {
    double s = 0.0;
    for (int g = 0; g < G; ++g) s += (double)p[g * step];
    mean = s / (double)G;
    double v = 0.0;
    for (int g = 0; g < G; ++g) {
        const double d = (double)p[g * step] - mean;
        v = fma(d, d, v);
    }
    sd = sqrt(v / (double)G + kMbstdEps);
}

// grid (n / G, F).  `run` = c / F * h * w: the floats of feature f in one sample; xs / ys: floats per sample of x / y.
__global__ void __launch_bounds__(kAdvThreads)
mbstd_kernel(const float* __restrict__ x, float* __restrict__ y, int c, int hw, int G, int groups, int F, int run) {
    __shared__ double s_red[kAdvThreads];
    const int j = blockIdx.x, f = blockIdx.y;
    const int64_t xs = (int64_t)c * hw, ys = (int64_t)(c + F) * hw;
    const float* __restrict__ xp = x + j * xs + (int64_t)f * run;
    float* __restrict__ yp = y + j * ys + (int64_t)f * run;
    double acc = 0.0;
    for (int e = threadIdx.x; e < run; e += kAdvThreads) {
        double mean, sd;
        mbstd_moments(xp + e, groups * xs, G, mean, sd);
        acc += sd;
        for (int g = 0; g < G; ++g) yp[g * groups * ys + e] = xp[g * groups * xs + e];
    }
    const float stat = (float)(adv_block_sum(acc, s_red) / (double)run);
    for (int q = threadIdx.x; q < G * hw; q += kAdvThreads) {
        const int g = q / hw, p = q - g * hw;
        y[((int64_t)g * groups + j) * ys + (int64_t)(c + f) * hw + p] = stat;
    }
}

__global__ void __launch_bounds__(kAdvThreads)
mbstd_bwd_kernel(const float* __restrict__ x, const float* __restrict__ dy, float* __restrict__ dx, int c, int hw, int G, int groups, int F,
                 int run) {
    __shared__ double s_red[kAdvThreads];
    const int j = blockIdx.x, f = blockIdx.y;
    const int64_t xs = (int64_t)c * hw, ys = (int64_t)(c + F) * hw;
    double acc = 0.0;
    for (int q = threadIdx.x; q < G * hw; q += kAdvThreads) {
        const int g = q / hw, p = q - g * hw;
        acc += (double)dy[((int64_t)g * groups + j) * ys + (int64_t)(c + f) * hw + p];
    }
    const double coef = adv_block_sum(acc, s_red) / (double)run / (double)G;
    const float* __restrict__ xp = x + j * xs + (int64_t)f * run;
    const float* __restrict__ gp = dy + j * ys + (int64_t)f * run;
    float* __restrict__ op = dx + j * xs + (int64_t)f * run;
    for (int e = threadIdx.x; e < run; e += kAdvThreads) {
        double mean, sd;
        mbstd_moments(xp + e, groups * xs, G, mean, sd);
        const double k = coef / sd;
        for (int g = 0; g < G; ++g)
            op[g * groups * xs + e] = (float)((double)gp[g * groups * ys + e] + k * ((double)xp[g * groups * xs + e] - mean));
    }
}

// One workgroup walks the images in order.
__global__ void __launch_bounds__(kAdvThreads)
adv_head_kernel(const float* __restrict__ o, const float* __restrict__ cmap, float* __restrict__ logit, float* __restrict__ loss, int n, int M,
                int sign) {
    __shared__ double s_red[kAdvThreads];
    const double scale = 1.0 / sqrt((double)M);
    double total = 0.0;
    for (int i = 0; i < n; ++i) {
        double z;
        if (cmap) {
            double dot = 0.0;
            for (int m = threadIdx.x; m < M; m += kAdvThreads) dot = fma((double)o[(int64_t)i * M + m], (double)cmap[(int64_t)i * M + m], dot);
            z = adv_block_sum(dot, s_red) * scale;
        } else {
            z = (double)o[i];
        }
        if (threadIdx.x == 0) logit[i] = (float)z;
        const double t = (double)sign * z;
        total += fmax(t, 0.0) + log1p(exp(-fabs(t)));
    }
    if (threadIdx.x == 0) loss[0] = (float)(total / (double)n);
}

// grid (n): do[i, m] = dloss sign sigmoid(sign logit_i) / n * cmap[i, m] / sqrt(M).
__global__ void __launch_bounds__(kAdvThreads)
adv_head_bwd_kernel(const float* __restrict__ cmap, const float* __restrict__ logit, const float* __restrict__ dloss, float* __restrict__ dout,
                    int n, int M, int sign) {
    const int i = blockIdx.x;
    const double t = (double)sign * (double)logit[i];
    const double k = (double)dloss[0] * (double)sign / (1.0 + exp(-t)) / (double)n / sqrt((double)M);
    for (int m = threadIdx.x; m < M; m += kAdvThreads) dout[(int64_t)i * M + m] = (float)(cmap ? k * (double)cmap[(int64_t)i * M + m] : k);
}

// -> the group size G, or 0 with the error text set
static int mbstd_group(const char* what, int32_t n, int32_t c, int32_t h, int32_t w, int32_t group, int32_t features) {
    if (!(n >= 1 && c >= 1 && h >= 1 && w >= 1 && features >= 1 && group >= 0 && features <= 65535)) {
        set_error("%s: x [n, c, h, w] with n, c, h, w >= 1, group >= 0 (0: the whole batch) and 1 <= features <= 65535", what);
        return 0;
    }
    const int G = group > 0 ? group : n;
    if (n % G != 0) {
        set_error("%s: the batch n = %d is not a multiple of the group size %d", what, n, G);
        return 0;
    }
    if (c % features != 0) {
        set_error("%s: the channels c = %d are not a multiple of features = %d", what, c, features);
        return 0;
    }
    if (!((int64_t)(c / features) * h * w < (1LL << 30) && (int64_t)G * h * w < (1LL << 30) && (int64_t)n * (c + features) * h * w < (1LL << 40))) {
        set_error("%s: tensor too large", what);
        return 0;
    }
    return G;
}

static bool adv_head_ok(int32_t n, int32_t M, int32_t sign, bool has_cmap) {
    return n >= 1 && n <= 65535 && M >= 1 && M <= kAdvMaxM && (sign == 1 || sign == -1) && (has_cmap || M == 1);
}

}  // namespace ide3d

using namespace ide3d;

extern "C" int ide3d_minibatch_std(const float* x, float* y, int32_t n, int32_t c, int32_t h, int32_t w, int32_t group, int32_t features,
                                   void* stream) {
    IDE3D_CHECK_ARG(x && y, "minibatch_std: null pointer");
    const int G = mbstd_group("minibatch_std", n, c, h, w, group, features);
    if (G == 0) return IDE3D_EINVAL;
    hipLaunchKernelGGL(mbstd_kernel, dim3((unsigned)(n / G), (unsigned)features), dim3(kAdvThreads), 0, (hipStream_t)stream, x, y, c, h * w, G,
                       n / G, features, c / features * h * w);
    IDE3D_CHECK_LAUNCH("minibatch_std");
    return IDE3D_OK;
}

extern "C" int ide3d_minibatch_std_backward(const float* x, const float* dy, float* dx, int32_t n, int32_t c, int32_t h, int32_t w,
                                            int32_t group, int32_t features, void* stream) {
    IDE3D_CHECK_ARG(x && dy && dx, "minibatch_std_backward: null pointer");
    const int G = mbstd_group("minibatch_std_backward", n, c, h, w, group, features);
    if (G == 0) return IDE3D_EINVAL;
    hipLaunchKernelGGL(mbstd_bwd_kernel, dim3((unsigned)(n / G), (unsigned)features), dim3(kAdvThreads), 0, (hipStream_t)stream, x, dy, dx, c,
                       h * w, G, n / G, features, c / features * h * w);
    IDE3D_CHECK_LAUNCH("minibatch_std_backward");
    return IDE3D_OK;
}

extern "C" int ide3d_adv_head(const float* o, const float* cmap, float* logit, float* loss, int32_t n, int32_t M, int32_t sign, void* stream) {
    IDE3D_CHECK_ARG(o && logit && loss, "adv_head: null pointer");
    IDE3D_CHECK_ARG(sign == 1 || sign == -1, "adv_head: sign must be -1 or +1");
    IDE3D_CHECK_ARG(adv_head_ok(n, M, sign, cmap != nullptr), "adv_head: o [n <= 65535, M <= %d]; without cmap M must be 1", kAdvMaxM);
    hipLaunchKernelGGL(adv_head_kernel, dim3(1), dim3(kAdvThreads), 0, (hipStream_t)stream, o, cmap, logit, loss, n, M, sign);
    IDE3D_CHECK_LAUNCH("adv_head");
    return IDE3D_OK;
}

extern "C" int ide3d_adv_head_backward(const float* o, const float* cmap, const float* logit, const float* dloss, float* dout, int32_t n,
                                       int32_t M, int32_t sign, void* stream) {
    IDE3D_CHECK_ARG(o && logit && dloss && dout, "adv_head_backward: null pointer");
    IDE3D_CHECK_ARG(sign == 1 || sign == -1, "adv_head_backward: sign must be -1 or +1");
    IDE3D_CHECK_ARG(adv_head_ok(n, M, sign, cmap != nullptr), "adv_head_backward: o [n <= 65535, M <= %d]; without cmap M must be 1", kAdvMaxM);
    hipLaunchKernelGGL(adv_head_bwd_kernel, dim3((unsigned)n), dim3(kAdvThreads), 0, (hipStream_t)stream, cmap, logit, dloss, dout, n, M, sign);
    IDE3D_CHECK_LAUNCH("adv_head_backward");
    return IDE3D_OK;
}
