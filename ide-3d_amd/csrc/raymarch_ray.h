// raymarch_ray.h — the per-sample ray math of the fused renderer, shared by its forward (raymarch.hip) and its backward
// (raymarch_bwd.hip), so that the backward rebuilds exactly the samples the forward composited: the jittered depth of a sample, its
// world point (camera space -> jitter -> cam2world), the density activation, and the host-side rules both launches check.
#pragma once
#include "common.h"
#include "triplane_tap.h"

namespace ide3d {

__device__ __forceinline__ float softplus_fast(float x) {
    // softplus(x) = max(x, 0) + log(1 + exp(-|x|)); abs error ~1e-7, saturates like threshold=20.  Raw v_exp_f32 / v_log_f32: the
    // exponent is <= 0 (a result below the normal range is 0 beside the 1 it is added to) and the logarithm's argument is in [1, 2], so
    // the denormal guards of __expf / __logf (a compare, a select and an ldexp each) have nothing to do here.
    const float e = __builtin_amdgcn_exp2f(-1.44269504088896340736f * fabsf(x));
    return fmaf(0.69314718055994530942f, __builtin_amdgcn_logf(1.0f + e), fmaxf(x, 0.f));
}

// Depth of sample s of ray `ray` (global ray index): z_lin[s], moved by (jitter - 0.5) * zstep when the call jitters (perturb_points).
__device__ __forceinline__ float ray_sample_depth(const ide3d_render_params& p, int64_t ray, int s, float zstep) {
    const float z = p.z_lin[s];
    return p.jitter ? __fadd_rn(z, __fmul_rn(__fsub_rn(p.jitter[ray * p.steps + s], 0.5f), zstep)) : z;
}

// Camera-space point of the sample at linear depth zl with jitter draw jl on ray r: direction times depth, then the jitter offset,
// rounded like the reference's fp32 tensor ops (get_initial_rays_trig, perturb_points).  What ray_world_point sends through cam2world;
// the backward's camera gradient needs it on its own.
__device__ __forceinline__ void ray_camera_point(const ide3d_render_params& p, int r, float zl, float jl, float zstep,
                                                 float& px, float& py, float& pz) {
    const float dx = p.rays_d_cam[r * 3 + 0], dy = p.rays_d_cam[r * 3 + 1], dz = p.rays_d_cam[r * 3 + 2];
    px = __fmul_rn(dx, zl); py = __fmul_rn(dy, zl); pz = __fmul_rn(dz, zl);
    if (p.jitter) {
        const float off = __fmul_rn(__fsub_rn(jl, 0.5f), zstep);
        px = __fadd_rn(px, __fmul_rn(off, dx));
        py = __fadd_rn(py, __fmul_rn(off, dy));
        pz = __fadd_rn(pz, __fmul_rn(off, dz));
    }
}

// World point of the sample at linear depth zl with jitter draw jl on ray r of image n: camera space -> jitter -> world, rounded
// like the reference's fp32 tensor ops (get_initial_rays_trig, perturb_points, transform_sampled_points).  The camera-space part is
// ray_camera_point's, written out (the forward's and the backward's instruction streams are pinned).
__device__ __forceinline__ void ray_world_point(const ide3d_render_params& p, int n, int r, float zl, float jl, float zstep,
                                                float& wx, float& wy, float& wz) {
    const float dx = p.rays_d_cam[r * 3 + 0], dy = p.rays_d_cam[r * 3 + 1], dz = p.rays_d_cam[r * 3 + 2];
    const float* M = p.cam2world + n * 16;
    float px = __fmul_rn(dx, zl), py = __fmul_rn(dy, zl), pz = __fmul_rn(dz, zl);
    if (p.jitter) {
        const float off = __fmul_rn(__fsub_rn(jl, 0.5f), zstep);
        px = __fadd_rn(px, __fmul_rn(off, dx));
        py = __fadd_rn(py, __fmul_rn(off, dy));
        pz = __fadd_rn(pz, __fmul_rn(off, dz));
    }
    wx = fmaf(M[0], px, fmaf(M[1], py, fmaf(M[2], pz, M[3])));
    wy = fmaf(M[4], px, fmaf(M[5], py, fmaf(M[6], pz, M[7])));
    wz = fmaf(M[8], px, fmaf(M[9], py, fmaf(M[10], pz, M[11])));
}

// The three plane projections of a world point (sample_from_triplane: xy, yz, xz).
__device__ __forceinline__ void triplane_taps(float wx, float wy, float wz, int W, int H, Tap2 (&t)[3]) {
    t[0] = make_tap(wx, wy, W, H);
    t[1] = make_tap(wy, wz, W, H);
    t[2] = make_tap(wx, wz, W, H);
}
// The same with the taps' element offsets in a plane of row stride sH, texel stride sW: what the forward's scalar-base loads take.
__device__ __forceinline__ void triplane_tap_addrs(float wx, float wy, float wz, int W, int H, int sH, int sW, TapAddr (&t)[3]) {
    t[0] = make_tap_addr(wx, wy, W, H, sH, sW);
    t[1] = make_tap_addr(wy, wz, W, H, sH, sW);
    t[2] = make_tap_addr(wx, wz, W, H, sH, sW);
}

// ---- host-side rules shared by the forward and the backward launch ----------------------------------------------------------------

// What a call must bring of its rays: nothing (sample_voxel), the rays (hierarchical pass, backward), or the feature image as well.
enum RayCheck { kNoRays, kRays, kRaysAndOutput };

static inline int check_render_params(const ide3d_render_params& p, const char* who, RayCheck rays) {
    IDE3D_CHECK_ARG(p.tex_planes && p.geo_planes, "%s: null tri-plane pointer", who);
    IDE3D_CHECK_ARG(p.geo_w0 && p.geo_b0 && p.geo_w1 && p.geo_b1 && p.tex_w0 && p.tex_b0 && p.tex_w1 && p.tex_b1,
                    "%s: null MLP weight pointer", who);
    IDE3D_CHECK_ARG(p.n > 0 && p.C > 0 && p.H > 0 && p.W > 0, "%s: bad tri-plane shape", who);
    IDE3D_CHECK_ARG(p.feat_ch >= 1 && p.feat_ch <= 32 && p.seg_ch >= 0 && p.seg_ch <= 31,
                    "%s: feat_ch <= 32 and seg_ch <= 31 required", who);
    if (rays != kNoRays) {
        IDE3D_CHECK_ARG(p.rays_d_cam && p.z_lin && p.cam2world && (p.out_feat || rays == kRays),
                        rays == kRays ? "%s: null ray pointer" : "%s: null ray / output pointer", who);
        IDE3D_CHECK_ARG(p.rays_per_img > 0 && p.steps > 0, "%s: bad ray shape", who);
        IDE3D_CHECK_ARG(p.clamp_mode == 0 || p.clamp_mode == 1, "%s: Need to choose clamp mode", who);
    }
    return IDE3D_OK;
}

// Steps per ray of the hierarchical pass: an inner pdf needs 3 samples, and ide3d_merge_depths orders at most 2048 merged samples per ray
// (kMergeMaxT = 2 * kMergedMaxSteps, raymarch.hip).  The merged march's backward declines what its forward declines.
constexpr int kMergedMinSteps = 3, kMergedMaxSteps = 1024;
constexpr bool hierarchical_steps_ok(int steps) { return steps >= kMergedMinSteps && steps <= kMergedMaxSteps; }
static inline int check_hierarchical_steps(const ide3d_render_params& p, const char* who) {
    if (hierarchical_steps_ok(p.steps)) return IDE3D_OK;
    set_error("%s: the hierarchical pass takes %d .. %d steps, got %d", who, kMergedMinSteps, kMergedMaxSteps, p.steps);
    return IDE3D_ENOKERNEL;
}

// The compiled forms of the renderer.  with_form calls f(RmForm<C, HID, SPLIT>{}) for the form that p (and, where the kernel has one, the
// split arithmetic) selects; without one the error is set under `who` (who = NULL: a size query, which answers 0).
template <int C_, int HID_, bool SPLIT_> struct RmForm { static constexpr int C = C_, HID = HID_; static constexpr bool SPLIT = SPLIT_; };
template <class F>
static inline auto with_form(const ide3d_render_params& p, bool split, const char* who, F&& f) -> decltype(f(RmForm<16, 32, false>{})) {
    if (p.C == 32 && p.hidden == 64) return split ? f(RmForm<32, 64, true>{}) : f(RmForm<32, 64, false>{});
    if (p.C == 16 && p.hidden == 32) return f(RmForm<16, 32, false>{});
    if (!who) return 0;
    set_error("%s: no fused kernel for C=%d hidden=%d", who, p.C, p.hidden);
    return IDE3D_ENOKERNEL;
}

static inline bool planes_fast(const ide3d_render_params& p) {
    auto ok = [&](const float* base, const int64_t* s) {
        return s[1] == 1 && (s[0] % 4 == 0) && (s[2] % 4 == 0) && (s[3] % 4 == 0) &&
               ((reinterpret_cast<uintptr_t>(base) & 15) == 0);
    };
    return ok(p.tex_planes, p.tex_stride) && ok(p.geo_planes, p.geo_stride) &&
           p.tex_stride[2] == p.geo_stride[2] && p.tex_stride[3] == p.geo_stride[3] &&
           (p.tex_stride[2] * p.H + p.tex_stride[3] * p.W + 3 * p.C) * 4 < 0x7fffffffLL;       // byte offsets inside an image: 31 bits (launch_voxel bounds the image strides a straddling tile adds)
}

// What no fused march takes, forward or backward (IDE3D_ENOKERNEL: the step-wise ops do).
static inline int check_march_declines(const ide3d_render_params& p, const char* who) {
    if (p.last_back) { set_error("%s: last_back is not fused; use the step-wise ops", who); return IDE3D_ENOKERNEL; }
    if (!planes_fast(p)) { set_error("%s: tri-planes must be channels_last, 16-byte aligned", who); return IDE3D_ENOKERNEL; }
    return IDE3D_OK;
}

}  // namespace ide3d
