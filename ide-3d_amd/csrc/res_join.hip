// res_join.hip — the residual join of the encoders' blocks with its gain: out = (a + b) * gain.
//
// `EncoderResBlock` ends in (conv2(conv1(x)) + skip(x)) / sqrt(2).  ide3d_parse_join (parse_loss.hip) adds up to three terms but has no gain
// on the sum, so this is a launch of its own: one pass instead of ATen's two, forward; backward, b = NULL gives dy * gain, the gradient of
// BOTH branches (one tensor, read by both).  Each output is one fp32 addition and one fp32 multiplication in that order, which is what ATen
// computes for `(a + b) * gain`: bit-equal to the definition.  A streaming pass: 16-byte accesses when every operand allows it, plain fp32
// on the vector pipe, no matrix loop (section 4.2's exclusive residency does not apply).
#include "common.h"

namespace ide3d {

constexpr int kRjThreads = 256;

// A thread owns 4 consecutive floats.  kVec: every pointer is 16-byte aligned, so a whole group is one 16-byte access; the last group of a
// count that is no multiple of 4, and every group without kVec, goes float by float, each index checked against count.
template <bool kVec, bool kTwo>
__global__ void __launch_bounds__(kRjThreads)
res_join_kernel(const float* __restrict__ a, const float* __restrict__ b, float* __restrict__ out, int64_t count, float gain) {
    const int64_t i = ((int64_t)blockIdx.x * kRjThreads + threadIdx.x) * 4;
    if (i >= count) return;
    if (kVec && i + 4 <= count) {
        float4 v = *reinterpret_cast<const float4*>(a + i);
        if (kTwo) {
            const float4 u = *reinterpret_cast<const float4*>(b + i);
            v.x += u.x; v.y += u.y; v.z += u.z; v.w += u.w;
        }
        v.x *= gain; v.y *= gain; v.z *= gain; v.w *= gain;
        *reinterpret_cast<float4*>(out + i) = v;
        return;
    }
    const int64_t end = (i + 4 < count) ? i + 4 : count;
    for (int64_t j = i; j < end; ++j) {
        float v = a[j];
        if (kTwo) v += b[j];
        out[j] = v * gain;
    }
}

}  // namespace ide3d

using namespace ide3d;

extern "C" int ide3d_residual_join(const float* a, const float* b, float* out, int64_t count, float gain, void* stream) {
    IDE3D_CHECK_ARG(a && out, "residual_join: null pointer");
    IDE3D_CHECK_ARG(count >= 1 && count < (1LL << 40), "residual_join: count must be in [1, 2^40)");
    uintptr_t bits = reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(out);
    if (b) bits |= reinterpret_cast<uintptr_t>(b);
    IDE3D_CHECK_ARG((bits & 3) == 0, "residual_join: operands must be 4-byte aligned");
    const bool vec = (bits & 15) == 0;
    const dim3 grid((unsigned)cdiv64(cdiv64(count, 4), kRjThreads)), block(kRjThreads);
    hipStream_t s = (hipStream_t)stream;
    if (b) {
        if (vec) hipLaunchKernelGGL((res_join_kernel<true, true>), grid, block, 0, s, a, b, out, count, gain);
        else     hipLaunchKernelGGL((res_join_kernel<false, true>), grid, block, 0, s, a, b, out, count, gain);
    } else {
        if (vec) hipLaunchKernelGGL((res_join_kernel<true, false>), grid, block, 0, s, a, b, out, count, gain);
        else     hipLaunchKernelGGL((res_join_kernel<false, false>), grid, block, 0, s, a, b, out, count, gain);
    }
    IDE3D_CHECK_LAUNCH("residual_join");
    return IDE3D_OK;
}
