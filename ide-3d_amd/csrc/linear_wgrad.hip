// linear_wgrad.hip — the weight gradient of a linear layer over few rows: the trainable projectors of the encoders.
//
// ide3d_linear (id_loss.hip) serves a 4 x 4 convolution over a 4 x 4 map as the linear layer it is, ide3d_linear_backward_input its input
// gradient; this file adds dW = dy^T x under the same limits (n <= 8 rows, K a multiple of 4, 16-byte aligned operands).  It is a pure
// streaming write of M K floats (168 MB for the image projector of the 512^2 hybrid encoder): one launch, 16-byte stores, x in registers,
// no workspace.  Deterministic: every output is one thread's own sum over the images in ascending order.  Plain fp32 on the vector pipe
// (no packed fp32: the library is built without it); no matrix loop, so section 4.2's exclusive residency does not apply.
#include "common.h"

namespace ide3d {

constexpr int kLwThreads = 256;
constexpr int kLwMaxN = 8;             // as ide3d_linear
constexpr int kLwRows = 16;            // rows of dw per workgroup

// A thread owns 4 consecutive k: it keeps the 16 bytes of x of every image in registers and writes 16 bytes of each of its workgroup's
// kLwRows rows of dw (a wave writes 1 KiB of a row at once); dy[i, m] is uniform over the workgroup.
__global__ void __launch_bounds__(kLwThreads)
linear_wgrad_kernel(const float* __restrict__ dy, const float* __restrict__ x, float* __restrict__ dw, int n, int K, int M) {
    const int k = (blockIdx.x * kLwThreads + threadIdx.x) * 4;
    if (k >= K) return;                                                      // (no barrier below; K % 4 == 0: a 16-byte group is inside as a whole)
    const int m0 = blockIdx.y * kLwRows, m1 = min(M, m0 + kLwRows);
    float4 xv[kLwMaxN];
#pragma unroll
    for (int i = 0; i < kLwMaxN; ++i)
        xv[i] = (i < n) ? *reinterpret_cast<const float4*>(x + (int64_t)i * K + k) : make_float4(0.f, 0.f, 0.f, 0.f);
    for (int m = m0; m < m1; ++m) {
        float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
        for (int i = 0; i < kLwMaxN; ++i)
            if (i < n) {
                const float d = dy[(int64_t)i * M + m];
                acc.x = fmaf(d, xv[i].x, acc.x); acc.y = fmaf(d, xv[i].y, acc.y);
                acc.z = fmaf(d, xv[i].z, acc.z); acc.w = fmaf(d, xv[i].w, acc.w);
            }
        *reinterpret_cast<float4*>(dw + (int64_t)m * K + k) = acc;
    }
}

// the limits of ide3d_linear (id_loss.hip, id_linear_ok)
static bool linear_wgrad_ok(int32_t n, int32_t K, int32_t M) {
    return n >= 1 && n <= kLwMaxN && K >= 4 && K % 4 == 0 && K <= (1 << 24) && M >= 1 && M <= 65535 * 8 && (int64_t)K * M < (1LL << 40);
}

}  // namespace ide3d

using namespace ide3d;

extern "C" int ide3d_linear_weight_grad(const float* dy, const float* x, float* dw, int32_t n, int32_t K, int32_t M, void* stream) {
    IDE3D_CHECK_ARG(dy && x && dw, "linear_weight_grad: null pointer");
    IDE3D_CHECK_ARG(linear_wgrad_ok(n, K, M), "linear_weight_grad: dy [n <= %d, M], x [n, K], dw [M, K] with K a multiple of 4", kLwMaxN);
    IDE3D_CHECK_ARG(((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(dw)) & 15) == 0, "linear_weight_grad: x and dw must be 16-byte aligned");
    hipLaunchKernelGGL(linear_wgrad_kernel, dim3(cdiv(K / 4, kLwThreads), cdiv(M, kLwRows)), dim3(kLwThreads), 0, (hipStream_t)stream, dy, x, dw,
                       n, K, M);
    IDE3D_CHECK_LAUNCH("linear_weight_grad");
    return IDE3D_OK;
}
