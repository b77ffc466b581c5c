// raymarch_bwd.hip — backward of the fused ray-marcher (render_rays_kernel, raymarch.hip) with respect to the two tri-planes.
//
// Given dL/dfeat [n, feat+seg, rays], dL/ddepth [n, rays] and dL/dwsum [n, rays] (each may be NULL = zero), accumulates dL/dtex_planes
// and dL/dgeo_planes into caller-zeroed fp32 buffers.  Nothing per sample is saved by the forward: the samples are rebuilt here exactly as
// the forward builds them (raymarch_ray.h: depth, jitter, cam2world, tap indices of triplane_tap.h, density noise).
//
// Per ray (one wavefront; lane = sample, the ray walked in chunks of 64 samples):
//   sweep 1    both gathers and MLPs; per sample keep alpha_i, the transmittance T_i and
//              h_i = dL/dw_i = sum_c gfeat_c out_ic + gd z_i + gw',   gw' = gw - [white_back] sum_c gfeat_c - gd max_depth.
//              The output layer is never formed: sum_c gfeat_c out_ic = sum_k u_k hid_k + sum_c gfeat_c b1_c with the per-ray vector
//              u = W1^T gfeat (one per branch, kept in LDS), which is also the whole output-layer backward in sweep 2.
//   reverse    R_i = alpha_i h_i + (1 - alpha_i + 1e-10) R_{i+1}, R_S = 0 (a 64-lane scan of affine maps, chunks from the last);
//              dL/dalpha_i = T_i (h_i - R_{i+1}) — no division, so the last sample (delta 1e10, alpha may round to 1) is safe.
//   sweep 2    gathers and hidden layers again; dsigma_i = dL/dalpha_i delta_i exp(-delta_i a) a'(sigma_i + noise_i), back through the
//              hidden softplus and layer 0 of each MLP, and the feature gradient is scattered to the bilinear taps of all three planes.
// Arithmetic: exact fp32 on the VALU (weights are wave-uniform: scalar loads, v_fma with an SGPR operand), whatever arithmetic the
// forward's MLPs ran in; there is no matrix loop here, so DESIGN.md section 4.2's exclusive residency does not apply.
//
// Gradient output: no-return float atomics on channels_last buffers.  The per-sample feature gradients and tap weights are staged in
// LDS, then every atomic wave-instruction covers C consecutive channels of 64 / C taps (C = 32: one 128-byte segment per tap).  Taps outside
// the plane get nothing (zeros padding).  The sums depend on the order in which atomics arrive: results are NOT bit-reproducible from run
// to run (they agree to fp32 rounding).
//
// Decoder parameters (ide3d_render_rays_backward_params, a second instantiation of the same body; the tri-plane-only kernel is compiled
// from the body with every statement below removed):
//   hidden layers   dW0[k, c] = sum_samples dpre_k f_c, db0[k] = sum_samples dpre_k with the dpre sweep 2 forms anyway.  Eight hidden units
//                   at a time, dpre and hid of the chunk's 64 samples go through the staging area the scatter is not using, f is staged
//                   once per branch; lane (k, c-group) then sums its C / 8 products over the chunk's live samples.
//   output layers   per ray A^tex_k = sum_i w_i hid^tex_ik, A^geo_k = sum_i w_i hid^geo_ik, B_k = sum_i dsigma_i hid^geo_ik (summed by the
//                   same lanes into LDS); at the end of the ray dW1[c, k] += gfeat_c A_k, db1[c] += gfeat_c sum_i w_i, and the sigma row
//                   gets B_k and sum_i dsigma_i.
//   Every sum is added to the wave's own slice of a global workspace with plain vector loads and stores (an address of a slice is only
//   ever touched by one lane of one wave), and a second launch adds the slices in a fixed order: no atomics, so the decoder gradients ARE
//   bit-reproducible from run to run.
//
// Camera pose (ide3d_render_rays_backward_camera, the body's third compile-time switch CAM; the instantiations above are compiled from the
// body with every statement below removed):
//   The outputs depend on cam2world only through the sample points p = M[:3,:3] q + M[:3,3].  Once sweep 2 holds a branch's feature
//   gradient g of its sample, the lane reads that sample's 12 taps a second time (L2-resident: the gather has just touched them) and forms
//   the 12 dot products g . v_tap; with the per-axis tap factors of make_tap_frac the derivative of a plane's blend with respect to its tap
//   position is (1 - fy)(D01 - D00) + fy (D11 - D10) along x and (1 - fx)(D10 - D00) + fx (D11 - D01) along y (a tap outside the plane
//   counts as 0, a plane with no tap inside - non-finite coordinates among them - contributes nothing), times size / 2 per normalised
//   coordinate.  Summed over 3 planes x 2 branches this is gp = dL/dp (3 floats per sample), and dL/dM[r][c] = sum gp_r q_c, dL/dM[r][3] =
//   sum gp_r.  Everything is local to the lane: no LDS, no staging.
//   Per chunk the 12 products are summed over the wave (xor butterflies: a fixed order) and lanes 0 .. 11 add them to the 12 numbers of the
//   ray's image in the wave's own slice [n][12] of a second workspace, plain vector loads and stores again; a second launch adds the slices in
//   a fixed order and writes [n, 4, 4] with a zero last row.  No atomics: the camera gradient IS bit-reproducible, and equal whether the
//   call also scatters to the planes or sums the decoder gradients.
//
// Merged march of the hierarchical pass (ide3d_render_rays_merged_backward, the body's fourth compile-time switch MERGED; the instantiations
// above are compiled from the body with every statement below removed):
//   The ray has T = 2 * steps samples; the per-ray arrays, the chunk loops and the launch plan are sized by T.  Sample s is entry
//   src[ray, s] (clamped into [0, T) like render_rays_merged_kernel does) of [fine | coarse]: a coarse entry is placed by ray_world_point
//   from z_lin and the jitter draw, a fine entry at origin + dir_world * z_fine with the forward's fmul / fadd sequence, so both sweeps
//   gather the taps the forward gathered.  Depth and delta come from z_all; there is no density noise.  z_all, src and z_fine are constants
//   (the step-wise definition draws the fine depths and forms the fine points without gradient), so sweep 1, the reverse scan, sweep 2 and
//   the scatter are the plain kernel's over T samples.  Composes with PARAMS, not with CAM.
#include <algorithm>

#include "common.h"
#include "triplane_tap.h"
#include "raymarch_ray.h"

namespace ide3d {

// LDS.  Per workgroup: both layer-0 weight matrices and biases, row 0 (sigma) of the geometry output layer and its bias, read as
// broadcasts by every lane.  Per wave, in floats: feature-gradient staging [64][C + 1], tap offsets [64][12] (int) and weights [64][12],
// the two u vectors [2][64], then four per-sample arrays of the ray [Sp] (Sp = steps rounded up to 64).
template <int C, int HID>
struct BwdLds {
    static constexpr int W0 = HID * C;
    static constexpr int SHARED = 2 * W0 + 2 * HID + HID + 4;        // geo w0, tex w0, geo b0, tex b0, geo w1 row 0, geo b1[0] (+ pad)
    static constexpr int DF = 64 * (C + 1);
    static constexpr int TAPS = 64 * 12;
    static constexpr int U = 2 * 64;
    static constexpr int FIXED = DF + 2 * TAPS + U;
    static constexpr int ARRAYS = 4;
    // decoder-parameter variant: the staging area (DF + 2 * TAPS floats) holds f [64][C + 4], dpre [64][9] and hid [64][9] between two
    // scatters; three more per-ray vectors A^geo, A^tex, B [3][64] follow the u vectors
    static constexpr int FROW = C + 4, KB = 8, KROW = KB + 1;
    static constexpr int PSTAGE = 64 * FROW + 2 * 64 * KROW;
    static constexpr int PSUMS = 3 * 64;
    static_assert(PSTAGE <= DF + 2 * TAPS, "parameter-gradient staging must fit in the scatter's staging area");
    static_assert(C % 8 == 0 && HID % KB == 0 && HID <= 64, "lane (k, c-group) mapping");
};

// One wave's slice of the parameter-gradient workspace, in floats: geo dW0 [HID, C], tex dW0, geo db0 [HID], tex db0, geo dW1 [1 + seg, HID],
// tex dW1 [feat, HID], geo db1 [1 + seg], tex db1 [feat] — the order of the eight outputs of ide3d_render_param_grads.
template <int C, int HID>
struct ParamSlice {
    static constexpr int GW0 = 0, TW0 = HID * C, GB0 = 2 * HID * C, TB0 = GB0 + HID, GW1 = TB0 + HID;
    __host__ __device__ static int tw1(int seg) { return GW1 + (1 + seg) * HID; }
    __host__ __device__ static int gb1(int seg, int feat) { return tw1(seg) + feat * HID; }
    __host__ __device__ static int tb1(int seg, int feat) { return gb1(seg, feat) + 1 + seg; }
    __host__ __device__ static int total(int seg, int feat) { return tb1(seg, feat) + feat; }
    __host__ __device__ static int stride(int seg, int feat) { return (total(seg, feat) + 3) & ~3; }      // slices stay 16-byte aligned
};

// One sample's C features from one tri-plane (channels_last), summed over the three planes like the forward's blend: (xy + yz) + xz.
template <int C>
__device__ __forceinline__ void gather_sample_cl(const float* __restrict__ base, const TapAddr (&a)[3], float (&f)[C]) {
#pragma unroll
    for (int ci = 0; ci < C / 4; ++ci) {
        // one channel slice (12 tap loads) in flight at a time: left alone the scheduler issues all 96 loads of the sample first and the
        // kernel spills
        if (ci > 0) __builtin_amdgcn_sched_barrier(0);
        const float4 v0 = gather_plane_cl(base + 0 * C + 4 * ci, a[0]);
        const float4 v1 = gather_plane_cl(base + 1 * C + 4 * ci, a[1]);
        const float4 v2 = gather_plane_cl(base + 2 * C + 4 * ci, a[2]);
        f[4 * ci + 0] = (v0.x + v1.x) + v2.x;
        f[4 * ci + 1] = (v0.y + v1.y) + v2.y;
        f[4 * ci + 2] = (v0.z + v1.z) + v2.z;
        f[4 * ci + 3] = (v0.w + v1.w) + v2.w;
    }
}

// g . v for the 12 tap vectors v of one sample in one tri-plane: the loads of gather_sample_cl (clamped offsets, so unconditional), each
// dotted with the sample's feature gradient instead of blended.  D[pl][k]: k = 0 nw, 1 ne, 2 sw, 3 se like Tap2's mask bits.
template <int C>
__device__ __forceinline__ void tap_dots_cl(const float* __restrict__ base, const TapAddr (&a)[3], const float (&g)[C], float (&D)[3][4]) {
#pragma unroll
    for (int pl = 0; pl < 3; ++pl)
#pragma unroll
        for (int k = 0; k < 4; ++k) D[pl][k] = 0.f;
#pragma unroll
    for (int ci = 0; ci < C / 4; ++ci) {
        if (ci > 0) __builtin_amdgcn_sched_barrier(0);          // as in gather_sample_cl: one channel slice in flight at a time
#pragma unroll
        for (int pl = 0; pl < 3; ++pl) {
            const float* b = base + pl * C + 4 * ci;
            const float4 v[4] = {ld4(b + a[pl].o00), ld4(b + a[pl].o01), ld4(b + a[pl].o10), ld4(b + a[pl].o11)};
#pragma unroll
            for (int k = 0; k < 4; ++k)
                D[pl][k] = fmaf(v[k].w, g[4 * ci + 3], fmaf(v[k].z, g[4 * ci + 2], fmaf(v[k].y, g[4 * ci + 1], fmaf(v[k].x, g[4 * ci], D[pl][k]))));
        }
        // the slice's products are formed here: nothing reads D before the last slice, and left free they all move below the last load
        // (12 * C loaded values live at once)
        asm volatile("" : "+v"(D[0][0]), "+v"(D[0][1]), "+v"(D[0][2]), "+v"(D[0][3]), "+v"(D[1][0]), "+v"(D[1][1]), "+v"(D[1][2]), "+v"(D[1][3]),
                          "+v"(D[2][0]), "+v"(D[2][1]), "+v"(D[2][2]), "+v"(D[2][3]));
    }
}

// dL/dp of one sample from one branch, added to gp: the derivative of the three planes' blends with respect to their tap positions
// (du/dc = size / 2), dotted with the branch's feature gradient g.  Plane 0 reads (x, y), plane 1 (y, z), plane 2 (x, z).
template <int C>
__device__ __forceinline__ void add_point_grad(const float* __restrict__ img, const Tap2 (&t)[3], const TapAddr (&a)[3], const TapFrac (&fr)[3],
                                               const float (&g)[C], float half_w, float half_h, float (&gp)[3]) {
    float D[3][4];
    tap_dots_cl<C>(img, a, g, D);
    float dx[3], dy[3];
#pragma unroll
    for (int pl = 0; pl < 3; ++pl) {
        // a tap outside the plane counts as 0: by a factor, as the forward's zero weight does (selecting between the dot product and 0
        // instead lets the compiler sink each dot product into a branch of its own, below all 12 * C / 4 loads: it spills)
        const unsigned m = t[pl].mask;
        const float d00 = D[pl][0] * ((m & 1u) ? 1.0f : 0.f), d01 = D[pl][1] * ((m & 2u) ? 1.0f : 0.f);
        const float d10 = D[pl][2] * ((m & 4u) ? 1.0f : 0.f), d11 = D[pl][3] * ((m & 8u) ? 1.0f : 0.f);
        // a plane without a tap inside has fractions that may not be finite: nothing, not 0 * inf
        const float ax = m ? fr[pl].ax : 0.f, bx = m ? fr[pl].bx : 0.f, ay = m ? fr[pl].ay : 0.f, by = m ? fr[pl].by : 0.f;
        dx[pl] = fmaf(ay, d01 - d00, by * (d11 - d10)) * half_w;
        dy[pl] = fmaf(ax, d10 - d00, bx * (d11 - d01)) * half_h;
    }
    gp[0] += dx[0] + dx[2];
    gp[1] += dy[0] + dx[1];
    gp[2] += dy[1] + dy[2];
}

// Hidden pre-activation k of one MLP: b0[k] + sum_c w0[k][c] f[c] (weights in LDS, the same address in every lane)
template <int C>
__device__ __forceinline__ float hidden_pre(const float* w0, const float* b0, int k, const float (&f)[C]) {
    const float4* row = reinterpret_cast<const float4*>(w0 + k * C);
    float acc = b0[k];
#pragma unroll
    for (int c4 = 0; c4 < C / 4; ++c4) {
        const float4 w = row[c4];
        acc = fmaf(w.x, f[4 * c4 + 0], acc); acc = fmaf(w.y, f[4 * c4 + 1], acc);
        acc = fmaf(w.z, f[4 * c4 + 2], acc); acc = fmaf(w.w, f[4 * c4 + 3], acc);
    }
    return acc;
}

// df[c] += w0[k][c] dpre
template <int C>
__device__ __forceinline__ void hidden_back(const float* w0, int k, float dpre, float (&df)[C]) {
    const float4* row = reinterpret_cast<const float4*>(w0 + k * C);
#pragma unroll
    for (int c4 = 0; c4 < C / 4; ++c4) {
        const float4 w = row[c4];
        df[4 * c4 + 0] = fmaf(w.x, dpre, df[4 * c4 + 0]); df[4 * c4 + 1] = fmaf(w.y, dpre, df[4 * c4 + 1]);
        df[4 * c4 + 2] = fmaf(w.z, dpre, df[4 * c4 + 2]); df[4 * c4 + 3] = fmaf(w.w, dpre, df[4 * c4 + 3]);
    }
}

__device__ __forceinline__ float sigmoid_fast(float x) { return __builtin_amdgcn_rcpf(1.0f + __expf(-x)); }

__device__ __forceinline__ void wave_lds_sync() {
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// Stage the feature gradient df of this lane's sample and its 12 taps (offsets in the gradient buffer, -1 = no tap), then scatter
// w_tap * df[c] to the taps of the `live` samples s0 .. s0 + live - 1 of the chunk with one atomic per (tap, channel).
template <int C>
__device__ __forceinline__ void scatter_sample_grads(float* __restrict__ gimg, const int64_t* gs, const Tap2 (&t)[3], bool valid,
                                                     const float (&df)[C], int live, float* s_df, int* s_off, float* s_tw) {
    const int lane = lane_id();
    const int gH = (int)gs[2], gW = (int)gs[3];
#pragma unroll
    for (int c = 0; c < C; ++c) s_df[lane * (C + 1) + c] = df[c];
#pragma unroll
    for (int pl = 0; pl < 3; ++pl) {
        const float wk[4] = {t[pl].w00, t[pl].w01, t[pl].w10, t[pl].w11};
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int x = t[pl].ix0 + (k & 1), y = t[pl].iy0 + (k >> 1);
            const bool on = valid && ((t[pl].mask >> k) & 1u);
            s_off[lane * 12 + pl * 4 + k] = on ? y * gH + x * gW + pl * C : -1;
            s_tw[lane * 12 + pl * 4 + k] = wk[k];
        }
    }
    wave_lds_sync();
    constexpr int PER = 64 / C;                 // taps per wave-instruction
    const int c = lane % C, q_lane = lane / C;
    const int pairs = live * 12;
    for (int q0 = 0; q0 < pairs; q0 += PER) {
        const int q = q0 + q_lane;
        if (q < pairs) {
            const int off = s_off[q];
            if (off >= 0) {
                const int j = q / 12;
                atomicAdd(gimg + off + c, s_tw[q] * s_df[j * (C + 1) + c]);
            }
        }
    }
    wave_lds_sync();
}

// Parameter sums of one block of 8 hidden units over the chunk's live samples.  Lane = (k = lane / 8, c-group = lane % 8): C / 8 products
// dpre_k f_c each, added to the wave's dW0 rows (one contiguous run of 8 * C floats per wave-instruction); beside them c-group 0 sums dpre_k
// (db0, to the slice), c-group 1 w hid_k and c-group 2 dsigma hid_k (to the per-ray vectors a_w / a_ds in LDS; a_ds NULL = not this branch).
template <int C>
__device__ __forceinline__ void param_block_sums(const float* s_f, const float* s_dp, const float* s_hd, const float* s_w, const float* s_ds,
                                                 int live, float* g_w0, float* g_b0, float* a_w, float* a_ds) {
    constexpr int NC = C / 8, FROW = C + 4, KROW = 9;
    const int lane = lane_id(), cg = lane & 7, kl = lane >> 3;
    const float* msrc = (cg == 0 ? s_dp : s_hd) + kl;
    const float* ssrc = cg == 2 ? s_ds : s_w;
    const float* frow = s_f + cg * NC;
    float acc[NC], e = 0.f;
#pragma unroll
    for (int i = 0; i < NC; ++i) acc[i] = 0.f;
#pragma unroll 4
    for (int j = 0; j < live; ++j) {
        const float d = s_dp[j * KROW + kl];
        const float m = msrc[j * KROW];
        const float sc = cg == 0 ? 1.0f : ssrc[j];
        if constexpr (NC == 4) {
            const float4 v = *reinterpret_cast<const float4*>(frow + j * FROW);
            acc[0] = fmaf(d, v.x, acc[0]); acc[1] = fmaf(d, v.y, acc[1]); acc[2] = fmaf(d, v.z, acc[2]); acc[3] = fmaf(d, v.w, acc[3]);
        } else {
            const float2 v = *reinterpret_cast<const float2*>(frow + j * FROW);
            acc[0] = fmaf(d, v.x, acc[0]); acc[1] = fmaf(d, v.y, acc[1]);
        }
        e = fmaf(m, sc, e);
    }
    float* g = g_w0 + kl * C + cg * NC;
    if constexpr (NC == 4) {
        float4 v = *reinterpret_cast<float4*>(g);
        v.x += acc[0]; v.y += acc[1]; v.z += acc[2]; v.w += acc[3];
        *reinterpret_cast<float4*>(g) = v;
    } else {
        float2 v = *reinterpret_cast<float2*>(g);
        v.x += acc[0]; v.y += acc[1];
        *reinterpret_cast<float2*>(g) = v;
    }
    if (cg == 0) g_b0[kl] += e;
    else if (cg == 1) a_w[kl] += e;
    else if (cg == 2 && a_ds) a_ds[kl] += e;
}

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off);
    return v;
}

// What places the samples of the merged march: sample s of a ray is entry src[ray, s] of the concatenation [fine | coarse], at depth
// z_all[ray, s].  All three arrays are constants of the backward.
struct MergedSamples {
    const float* z_all;      // [n * rays, T] ascending depths
    const int* src;          // [n * rays, T] index into [fine | coarse]
    const float* z_fine;     // [n * rays, steps]
};

// The body of all kernels.  PARAMS = false: gradients of the tri-planes only (sl unused).  PARAMS = true: also the decoder-parameter sums,
// into the wave's slice of `slices`; a NULL grad_tex_planes / grad_geo_planes then skips that plane's scatter.  CAM = true: also the 12
// camera sums per image, into the wave's slice of `cam_slices`; a NULL plane gradient skips that plane's scatter without PARAMS too.
// MERGED = true: the T = 2 * steps samples of the hierarchical pass's merged march, placed by `ms`; sp is T rounded up to 64.
template <int C, int HID, bool PARAMS, bool CAM = false, bool MERGED = false>
__device__ __forceinline__ void render_rays_backward_body(const ide3d_render_params& p, const ide3d_render_grads& gr, int sp, float* slices,
                                                          float* cam_slices = nullptr, const MergedSamples& ms = MergedSamples{}) {
    static_assert(!(MERGED && CAM), "the merged march has no camera gradient");
    using L = BwdLds<C, HID>;
    using PS = ParamSlice<C, HID>;
    extern __shared__ __attribute__((aligned(16))) float lds[];
    float* const s_gw0 = lds;
    float* const s_tw0 = s_gw0 + L::W0;
    float* const s_gb0 = s_tw0 + L::W0;
    float* const s_tb0 = s_gb0 + HID;
    float* const s_gw1 = s_tb0 + HID;              // row 0 of geo_w1, then geo_b1[0]
    for (int i = threadIdx.x; i < L::W0; i += blockDim.x) { s_gw0[i] = p.geo_w0[i]; s_tw0[i] = p.tex_w0[i]; }
    for (int i = threadIdx.x; i < HID; i += blockDim.x) { s_gb0[i] = p.geo_b0[i]; s_tb0[i] = p.tex_b0[i]; s_gw1[i] = p.geo_w1[i]; }
    if (threadIdx.x == 0) s_gw1[HID] = p.geo_b1[0];
    __syncthreads();

    const int lane = lane_id(), wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int nw = blockDim.x >> 6;
    float* const s_df = lds + L::SHARED + wid * (L::FIXED + (PARAMS ? L::PSUMS : 0) + L::ARRAYS * sp);
    int* const s_off = reinterpret_cast<int*>(s_df + L::DF);
    float* const s_tw = s_df + L::DF + L::TAPS;
    float* const s_u = s_tw + L::TAPS;             // [0, 64): geometry branch, [64, 128): texture branch
    float* const s_a = s_u + L::U + (PARAMS ? L::PSUMS : 0);        // alpha_i, then dL/dalpha_i
    float* const s_h = s_a + sp;                   // h_i, then w_i = alpha_i T_i
    float* const s_t = s_h + sp;                   // T_i
    float* const s_x = s_t + sp;                   // sigma_i + noise_i, then (PARAMS) dsigma_i
    // PARAMS only: the staging area between two scatters, the per-ray sums A^geo, A^tex, B, and this wave's slice
    float* const s_f = s_df;
    float* const s_dp = s_f + 64 * L::FROW;
    float* const s_hd = s_dp + 64 * L::KROW;
    float* const s_sum = s_u + L::U;
    float* const sl = PARAMS ? slices + ((int64_t)blockIdx.x * nw + wid) * PS::stride(p.seg_ch, p.feat_ch) : nullptr;
    float* const csl = CAM ? cam_slices + ((int64_t)blockIdx.x * nw + wid) * ((int64_t)p.n * 12) : nullptr;

    // S: samples per ray (MERGED: T = 2 * steps, of which SC = steps are the coarse ones)
    const int SC = p.steps, S = MERGED ? 2 * SC : SC, R = p.rays_per_img, nch = p.feat_ch + p.seg_ch;
    const int64_t total_rays = (int64_t)p.n * R;
    const int sH = (int)p.tex_stride[2], sW = (int)p.tex_stride[3];
    const float zstep = (SC > 1) ? (p.z_lin[1] - p.z_lin[0]) : 0.f;

    for (int64_t ray = (int64_t)blockIdx.x * nw + wid; ray < total_rays; ray += (int64_t)gridDim.x * nw) {
        const int n = __builtin_amdgcn_readfirstlane((int)(ray / R));
        const int r = __builtin_amdgcn_readfirstlane((int)(ray - (int64_t)n * R));
        const float* gfeat = gr.grad_feat ? gr.grad_feat + (int64_t)n * nch * R + r : nullptr;
        const float gd = gr.grad_depth ? gr.grad_depth[ray] : 0.f;
        const float gw = gr.grad_wsum ? gr.grad_wsum[ray] : 0.f;
        // per-ray constants: u = W1^T gfeat of each branch (lane k = hidden unit k), the bias part of h and the background terms
        float hconst = gw - ((p.max_depth != 0.f) ? gd * p.max_depth : 0.f);
        {
            float ug = 0.f, ut = 0.f;
            if (gfeat) {
                float gsum = 0.f, bsum = 0.f;
                for (int o = 0; o < p.feat_ch; ++o) {
                    const float g = gfeat[(int64_t)o * R];
                    gsum += g; bsum = fmaf(g, p.tex_b1[o], bsum);
                    if (lane < HID) ut = fmaf(g, p.tex_w1[o * HID + lane], ut);
                }
                for (int o = 1; o <= p.seg_ch; ++o) {
                    const float g = gfeat[(int64_t)(p.feat_ch + o - 1) * R];
                    gsum += g; bsum = fmaf(g, p.geo_b1[o], bsum);
                    if (lane < HID) ug = fmaf(g, p.geo_w1[o * HID + lane], ug);
                }
                hconst += bsum - (p.white_back ? gsum : 0.f);
            }
            s_u[lane] = ug;
            s_u[64 + lane] = ut;
            if constexpr (PARAMS) { s_sum[lane] = 0.f; s_sum[64 + lane] = 0.f; s_sum[128 + lane] = 0.f; }
        }
        wave_lds_sync();
        float dnorm;
        {
            const float dx = p.rays_d_cam[r * 3 + 0], dy = p.rays_d_cam[r * 3 + 1], dz = p.rays_d_cam[r * 3 + 2];
            dnorm = sqrtf(dx * dx + dy * dy + dz * dz);
        }
        const float* geo_img = p.geo_planes + n * p.geo_stride[0];
        const float* tex_img = p.tex_planes + n * p.tex_stride[0];

        // what both sweeps rebuild of sample s: its taps, its depth and its delta
        auto sample_setup = [&](int s, Tap2 (&t)[3], TapAddr (&a)[3], float& z, float& delta) {
            const int sc = s < S ? s : S - 1;
            float wx, wy, wz;
            if constexpr (MERGED) {
                // the entry is clamped into [0, T) before it indexes anything, as the forward does
                const int sv = min(max(ms.src[ray * S + sc], 0), S - 1);
                if (sv < SC) {
                    // origin + dir_world * z_fine, the multiply and the add rounded separately: render_rays_merged_kernel's sequence,
                    // operation for operation (the taps must be the ones the forward gathered)
                    const float zf = ms.z_fine[ray * SC + sv];
                    const float dx = p.rays_d_cam[r * 3 + 0], dy = p.rays_d_cam[r * 3 + 1], dz = p.rays_d_cam[r * 3 + 2];
                    const float* M = p.cam2world + n * 16;
                    const float ux = fmaf(M[0], dx, fmaf(M[1], dy, __fmul_rn(M[2], dz)));
                    const float uy = fmaf(M[4], dx, fmaf(M[5], dy, __fmul_rn(M[6], dz)));
                    const float uz = fmaf(M[8], dx, fmaf(M[9], dy, __fmul_rn(M[10], dz)));
                    wx = __fadd_rn(M[3], __fmul_rn(ux, zf));
                    wy = __fadd_rn(M[7], __fmul_rn(uy, zf));
                    wz = __fadd_rn(M[11], __fmul_rn(uz, zf));
                } else {
                    const int i = sv - SC;
                    ray_world_point(p, n, r, p.z_lin[i], p.jitter ? p.jitter[ray * SC + i] : 0.5f, zstep, wx, wy, wz);
                }
            } else {
                const float zl = p.z_lin[sc];
                const float jl = p.jitter ? p.jitter[ray * S + sc] : 0.5f;
                ray_world_point(p, n, r, zl, jl, zstep, wx, wy, wz);
            }
            triplane_taps(wx, wy, wz, p.W, p.H, t);
#pragma unroll
            for (int pl = 0; pl < 3; ++pl) a[pl] = tap_addr(t[pl], p.W, p.H, sH, sW);
            if constexpr (MERGED) {
                z = ms.z_all[ray * S + sc];
                const float znext = (sc + 1 < S) ? ms.z_all[ray * S + sc + 1] : 0.f;
                delta = (sc + 1 < S) ? (znext - z) * dnorm : 1e10f;
            } else {
                z = ray_sample_depth(p, ray, sc, zstep);
                const float znext = (sc + 1 < S) ? ray_sample_depth(p, ray, sc + 1, zstep) : 0.f;
                delta = (sc + 1 < S) ? (znext - z) * dnorm : 1e10f;
            }
        };

        // ---- sweep 1: alpha_i, T_i, h_i, sigma_i + noise_i ----
        float carry = 1.0f;
        for (int c0 = 0; c0 < S; c0 += 64) {
            const int s = c0 + lane;
            const bool live = s < S;
            Tap2 t[3]; TapAddr a[3];
            float z, delta;
            sample_setup(s, t, a, z, delta);
            float f[C];
            gather_sample_cl<C>(geo_img, a, f);
            float sigma = s_gw1[HID], hg = 0.f;
#pragma unroll 2
            for (int k = 0; k < HID; ++k) {
                const float hid = softplus_fast(hidden_pre<C>(s_gw0, s_gb0, k, f));
                sigma = fmaf(s_gw1[k], hid, sigma);
                hg = fmaf(s_u[k], hid, hg);
            }
            gather_sample_cl<C>(tex_img, a, f);
            float ht = 0.f;
#pragma unroll 2
            for (int k = 0; k < HID; ++k) ht = fmaf(s_u[64 + k], softplus_fast(hidden_pre<C>(s_tw0, s_tb0, k, f)), ht);
            const float x = sigma + ((!MERGED && p.sigma_noise) ? p.sigma_noise[ray * S + (live ? s : S - 1)] : 0.f);
            const float dens = p.clamp_mode == 0 ? softplus_fast(x) : fmaxf(x, 0.f);
            const float alpha = live ? 1.0f - __expf(-delta * dens) : 0.f;
            const float fac = live ? (1.0f - alpha + 1e-10f) : 1.0f;
            // exclusive prefix product of fac over the 64 lanes, carried across chunks
            float incl = fac;
#pragma unroll
            for (int off = 1; off < 64; off <<= 1) {
                const float o = __shfl_up(incl, off);
                if (lane >= off) incl *= o;
            }
            const float prev = __shfl_up(incl, 1);
            const float T = carry * (lane == 0 ? 1.0f : prev);
            carry *= __shfl(incl, 63);
            if (live) {
                s_a[s] = alpha;
                s_h[s] = hconst + hg + ht + gd * z;
                s_t[s] = T;
                s_x[s] = x;
            }
        }
        wave_lds_sync();

        // ---- reverse scan: dL/dalpha_i and w_i ----
        float rcarry = 0.f;
        for (int c0 = ((S - 1) / 64) * 64; c0 >= 0; c0 -= 64) {
            const int s = c0 + lane;
            const bool live = s < S;
            const float alpha = live ? s_a[s] : 0.f, h = live ? s_h[s] : 0.f, T = live ? s_t[s] : 0.f;
            // R_i = A + B R_end over lanes i .. 63 of the chunk (composition of the affine maps R -> alpha h + (1 - alpha + 1e-10) R)
            float A = alpha * h, B = live ? (1.0f - alpha + 1e-10f) : 1.0f;
#pragma unroll
            for (int off = 1; off < 64; off <<= 1) {
                const float An = __shfl_down(A, off), Bn = __shfl_down(B, off);
                if (lane + off < 64) { A = fmaf(B, An, A); B *= Bn; }
            }
            const float incl = fmaf(B, rcarry, A);
            const float down = __shfl_down(incl, 1);
            const float rnext = lane == 63 ? rcarry : down;
            rcarry = __shfl(incl, 0);
            if (live) {
                s_a[s] = T * (h - rnext);
                s_h[s] = alpha * T;
            }
        }
        wave_lds_sync();

        // ---- sweep 2: back through both MLPs to the taps ----
        for (int c0 = 0; c0 < S; c0 += 64) {
            const int s = c0 + lane;
            const bool live = s < S;
            const int nlive = min(64, S - c0);
            Tap2 t[3]; TapAddr a[3];
            float z, delta;
            sample_setup(s, t, a, z, delta);
            const float dalpha = live ? s_a[s] : 0.f, w = live ? s_h[s] : 0.f, x = live ? s_x[s] : 0.f;
            float dens, dact;
            if (p.clamp_mode == 0) { dens = softplus_fast(x); dact = sigmoid_fast(x); }
            else { dens = fmaxf(x, 0.f); dact = x > 0.f ? 1.0f : 0.f; }
            // exp(-delta a) directly, not 1 - alpha: at the last sample (delta 1e10) alpha rounds to 1 while delta exp(-delta a) is finite
            const float dsigma = live ? dalpha * delta * __expf(-delta * dens) * dact : 0.f;
            float f[C], df[C];
            // CAM only: dL/d(world point) of the lane's sample, summed over both branches.  The taps are rebuilt from the sample index where
            // they are used, behind an opaque copy of it: merged with sample_setup's, their 60 values would stay live across the MLP loops
            float gp[3] = {0.f, 0.f, 0.f};
            auto sample_index = [&]() {
                int sc = live ? s : S - 1;
                asm volatile("" : "+v"(sc));
                return sc;
            };
            auto point_grad = [&](const float* img, const float (&g)[C]) {
                const int sc = sample_index();
                float wx, wy, wz;
                ray_world_point(p, n, r, p.z_lin[sc], p.jitter ? p.jitter[ray * S + sc] : 0.5f, zstep, wx, wy, wz);
                Tap2 t2[3]; TapAddr a2[3];
                triplane_taps(wx, wy, wz, p.W, p.H, t2);
#pragma unroll
                for (int pl = 0; pl < 3; ++pl) a2[pl] = tap_addr(t2[pl], p.W, p.H, sH, sW);
                const TapFrac fr[3] = {make_tap_frac(wx, wy, p.W, p.H), make_tap_frac(wy, wz, p.W, p.H), make_tap_frac(wx, wz, p.W, p.H)};
                add_point_grad<C>(img, t2, a2, fr, g, 0.5f * (float)p.W, 0.5f * (float)p.H, gp);
                // gp is read only after both branches: left free, the dot products sink below the scatter while their loads cannot, and
                // 12 * C loaded values stay live across it
                asm volatile("" : "+v"(gp[0]), "+v"(gp[1]), "+v"(gp[2]));
            };
            if constexpr (!PARAMS) {
                gather_sample_cl<C>(geo_img, a, f);
#pragma unroll
                for (int c = 0; c < C; ++c) df[c] = 0.f;
#pragma unroll 2
                for (int k = 0; k < HID; ++k) {
                    const float dpre = fmaf(w, s_u[k], dsigma * s_gw1[k]) * sigmoid_fast(hidden_pre<C>(s_gw0, s_gb0, k, f));
                    hidden_back<C>(s_gw0, k, dpre, df);
                }
                if constexpr (CAM) point_grad(geo_img, df);
                if constexpr (CAM) {
                    if (gr.grad_geo_planes)
                        scatter_sample_grads<C>(gr.grad_geo_planes + n * gr.grad_geo_stride[0], gr.grad_geo_stride, t, live, df, nlive, s_df, s_off, s_tw);
                } else
                    scatter_sample_grads<C>(gr.grad_geo_planes + n * gr.grad_geo_stride[0], gr.grad_geo_stride, t, live, df, nlive, s_df, s_off, s_tw);

                gather_sample_cl<C>(tex_img, a, f);
#pragma unroll
                for (int c = 0; c < C; ++c) df[c] = 0.f;
#pragma unroll 2
                for (int k = 0; k < HID; ++k) {
                    const float dpre = w * s_u[64 + k] * sigmoid_fast(hidden_pre<C>(s_tw0, s_tb0, k, f));
                    hidden_back<C>(s_tw0, k, dpre, df);
                }
                if constexpr (CAM) point_grad(tex_img, df);
                if constexpr (CAM) {
                    if (gr.grad_tex_planes)
                        scatter_sample_grads<C>(gr.grad_tex_planes + n * gr.grad_tex_stride[0], gr.grad_tex_stride, t, live, df, nlive, s_df, s_off, s_tw);
                } else
                    scatter_sample_grads<C>(gr.grad_tex_planes + n * gr.grad_tex_stride[0], gr.grad_tex_stride, t, live, df, nlive, s_df, s_off, s_tw);
            } else {
                if (live) s_x[s] = dsigma;          // x is in a register of its lane by now; param_block_sums reads dsigma of the chunk
#pragma unroll 1
                for (int br = 0; br < 2; ++br) {    // 0: geometry, 1: texture
                    const bool geo = br == 0;
                    const float* w0 = geo ? s_gw0 : s_tw0;
                    const float* b0 = geo ? s_gb0 : s_tb0;
                    float* gplanes = geo ? gr.grad_geo_planes : gr.grad_tex_planes;
                    gather_sample_cl<C>(geo ? geo_img : tex_img, a, f);
#pragma unroll
                    for (int c4 = 0; c4 < C / 4; ++c4)
                        *reinterpret_cast<float4*>(s_f + lane * L::FROW + 4 * c4) = make_float4(f[4 * c4], f[4 * c4 + 1], f[4 * c4 + 2], f[4 * c4 + 3]);
#pragma unroll
                    for (int c = 0; c < C; ++c) df[c] = 0.f;
#pragma unroll 1
                    for (int kb = 0; kb < HID; kb += L::KB) {
#pragma unroll 2
                        for (int kk = 0; kk < L::KB; ++kk) {
                            const int k = kb + kk;
                            const float pre = hidden_pre<C>(w0, b0, k, f);
                            const float dhid = geo ? fmaf(w, s_u[k], dsigma * s_gw1[k]) : w * s_u[64 + k];
                            const float dpre = dhid * sigmoid_fast(pre);
                            if (CAM || gplanes) hidden_back<C>(w0, k, dpre, df);
                            s_dp[lane * L::KROW + kk] = dpre;
                            s_hd[lane * L::KROW + kk] = softplus_fast(pre);
                        }
                        wave_lds_sync();
                        param_block_sums<C>(s_f, s_dp, s_hd, s_h + c0, s_x + c0, nlive, sl + (geo ? PS::GW0 : PS::TW0) + kb * C,
                                            sl + (geo ? PS::GB0 : PS::TB0) + kb, s_sum + br * 64 + kb, geo ? s_sum + 128 + kb : nullptr);
                        wave_lds_sync();
                    }
                    if constexpr (CAM) point_grad(geo ? geo_img : tex_img, df);
                    if (gplanes) {
                        const int64_t* gs = geo ? gr.grad_geo_stride : gr.grad_tex_stride;
                        scatter_sample_grads<C>(gplanes + n * gs[0], gs, t, live, df, nlive, s_df, s_off, s_tw);
                    }
                }
            }
            if constexpr (CAM) {
                // ---- camera: dL/dM[r][c] += gp_r q_c (c < 3), dL/dM[r][3] += gp_r, summed over the chunk, into the image's 12 numbers ----
                const int sc = sample_index();
                float cq[3], mine = 0.f;
                ray_camera_point(p, r, p.z_lin[sc], p.jitter ? p.jitter[ray * S + sc] : 0.5f, zstep, cq[0], cq[1], cq[2]);
#pragma unroll
                for (int i = 0; i < 12; ++i) {
                    const float g_r = live ? gp[i >> 2] : 0.f;
                    const float v = wave_sum((i & 3) < 3 ? g_r * cq[i & 3] : g_r);
                    if (lane == i) mine = v;
                }
                if (lane < 12) csl[(int64_t)n * 12 + lane] += mine;
            }
        }
        wave_lds_sync();
        if constexpr (PARAMS) {
            // ---- output layers: dW1 += gfeat (x) A, db1 += gfeat sum_i w_i; the sigma row gets B and sum_i dsigma_i ----
            float sw = 0.f, sds = 0.f;
            for (int c0 = 0; c0 < S; c0 += 64) {
                const int s = c0 + lane;
                if (s < S) { sw += s_h[s]; sds += s_x[s]; }
            }
            sw = wave_sum(sw); sds = wave_sum(sds);
            float* const gw1 = sl + PS::GW1;
            float* const tw1 = sl + PS::tw1(p.seg_ch);
            float* const gb1 = sl + PS::gb1(p.seg_ch, p.feat_ch);
            float* const tb1 = sl + PS::tb1(p.seg_ch, p.feat_ch);
            if (lane < HID) {
                gw1[lane] += s_sum[128 + lane];
                if (gfeat) {
                    const float ag = s_sum[lane], at = s_sum[64 + lane];
                    for (int o = 0; o < p.feat_ch; ++o) tw1[o * HID + lane] = fmaf(gfeat[(int64_t)o * R], at, tw1[o * HID + lane]);
                    for (int o = 1; o <= p.seg_ch; ++o)
                        gw1[o * HID + lane] = fmaf(gfeat[(int64_t)(p.feat_ch + o - 1) * R], ag, gw1[o * HID + lane]);
                }
            }
            if (lane == 0) gb1[0] += sds;
            if (gfeat) {
                if (lane < p.feat_ch) tb1[lane] = fmaf(gfeat[(int64_t)lane * R], sw, tb1[lane]);
                if (lane >= 1 && lane <= p.seg_ch) gb1[lane] = fmaf(gfeat[(int64_t)(p.feat_ch + lane - 1) * R], sw, gb1[lane]);
            }
            wave_lds_sync();
        }
    }
}

// The kernel of every plain form: the pointers a form does not use are passed as null.
template <int C, int HID, bool PARAMS, bool CAM>
__global__ void __launch_bounds__(512)
render_rays_backward_kernel(ide3d_render_params p, ide3d_render_grads gr, int sp, float* slices, float* cam_slices) {
    render_rays_backward_body<C, HID, PARAMS, CAM>(p, gr, sp, slices, cam_slices);
}

// The kernel of the merged forms (MERGED on, CAM off): the same body with the three arrays that place its samples.  A kernel of its own,
// so that the plain forms keep their arguments and with them their instruction streams.
template <int C, int HID, bool PARAMS>
__global__ void __launch_bounds__(512)
render_rays_merged_backward_kernel(ide3d_render_params p, ide3d_render_grads gr, int sp, float* slices, MergedSamples ms) {
    render_rays_backward_body<C, HID, PARAMS, false, true>(p, gr, sp, slices, nullptr, ms);
}

// Adds the slices in a fixed order: thread (element e, group g) sums slices g, g + 8, ..., then group 0 adds the 8 partial sums.
struct ParamOut {
    float* dst[8];
    int end[8];          // element range of dst[i] in a slice: [end[i - 1], end[i])
};

__global__ void __launch_bounds__(512)
reduce_param_slices_kernel(const float* __restrict__ slices, int nslices, int stride, ParamOut out) {
    __shared__ float part[8][64];
    const int lane = threadIdx.x & 63, g = threadIdx.x >> 6;
    const int e = blockIdx.x * 64 + lane, total = out.end[7];
    float sum = 0.f;
    if (e < total)
        for (int i = g; i < nslices; i += 8) sum += slices[(int64_t)i * stride + e];
    part[g][lane] = sum;
    __syncthreads();
    if (g == 0 && e < total) {
        float t = part[0][lane];
#pragma unroll
        for (int q = 1; q < 8; ++q) t += part[q][lane];
        float* d = out.dst[0];
        int first = 0;
#pragma unroll
        for (int q = 1; q < 8; ++q)
            if (e >= out.end[q - 1]) { d = out.dst[q]; first = out.end[q - 1]; }
        d[e - first] = t;
    }
}

// The camera sums: slices [nslices][n * 12] -> grad_cam2world [n, 4, 4], the same fixed order (group g sums slices g, g + 8, ..., group 0
// adds the 8 partial sums); the last row is written as zero.
__global__ void __launch_bounds__(512)
reduce_camera_slices_kernel(const float* __restrict__ slices, int nslices, int total, float* __restrict__ out) {
    __shared__ float part[8][64];
    const int lane = threadIdx.x & 63, g = threadIdx.x >> 6;
    const int e = blockIdx.x * 64 + lane;               // (image, row, column) = (e / 12, e % 12 / 4, e % 4)
    float sum = 0.f;
    if (e < total)
        for (int i = g; i < nslices; i += 8) sum += slices[(int64_t)i * total + e];
    part[g][lane] = sum;
    __syncthreads();
    if (g == 0 && e < total) {
        float t = part[0][lane];
#pragma unroll
        for (int q = 1; q < 8; ++q) t += part[q][lane];
        const int img = e / 12, k = e - img * 12;
        out[img * 16 + k] = t;
        if (k < 4) out[img * 16 + 12 + k] = 0.f;
    }
}

// Launch shape: 8 waves per workgroup, one workgroup per CU (the layer-0 weights are staged once per workgroup); fewer waves when the
// per-ray arrays of many steps do not fit.  nw = 0: the steps do not fit at all (lds_bytes = what one wave would need).
struct BwdPlan {
    int sp, nw;
    size_t lds_bytes;
    int64_t nblk;
};

template <int C, int HID, bool PARAMS, bool MERGED = false>
static BwdPlan plan_render_backward(const ide3d_render_params& p) {
    using L = BwdLds<C, HID>;
    BwdPlan pl;
    pl.sp = (int)cdiv64((MERGED ? 2 : 1) * (int64_t)p.steps, 64) * 64;
    const size_t wave_bytes = (L::FIXED + (PARAMS ? L::PSUMS : 0) + (size_t)L::ARRAYS * pl.sp) * sizeof(float), shared_bytes = L::SHARED * sizeof(float);
    pl.nw = 8;
    while (pl.nw > 1 && shared_bytes + pl.nw * wave_bytes > 160 * 1024) pl.nw /= 2;
    pl.lds_bytes = shared_bytes + pl.nw * wave_bytes;
    if (pl.lds_bytes > 160 * 1024) pl.nw = 0;
    const int64_t total_rays = (int64_t)p.n * p.rays_per_img;
    pl.nblk = cdiv64(total_rays, pl.nw ? pl.nw : 1);
    const int64_t cap = (int64_t)kNumCU * 8 / (pl.nw ? pl.nw : 1);
    if (pl.nblk > cap) pl.nblk = cap;
    return pl;
}

template <int C, int HID, bool MERGED = false>
static int64_t param_workspace_bytes(const ide3d_render_params& p) {
    const BwdPlan pl = plan_render_backward<C, HID, true, MERGED>(p);
    return pl.nw ? pl.nblk * pl.nw * (int64_t)ParamSlice<C, HID>::stride(p.seg_ch, p.feat_ch) * (int64_t)sizeof(float) : 0;
}

// One slice [n][12] per wave of whichever form launches (with and without the decoder sums the plans may differ in waves per workgroup).
template <int C, int HID>
static int64_t camera_workspace_bytes(const ide3d_render_params& p) {
    const BwdPlan a = plan_render_backward<C, HID, false>(p), b = plan_render_backward<C, HID, true>(p);
    if (!a.nw) return 0;
    const int64_t waves = std::max(a.nblk * a.nw, b.nblk * b.nw);
    return waves * p.n * 12 * (int64_t)sizeof(float);
}

// "<entry point> (<stage>)" for the error text of a follow-up launch (only formed when that launch fails).
static const char* stage_name(const char* what, const char* stage) {
    thread_local char buf[96];
    snprintf(buf, sizeof buf, "%s (%s)", what, stage);
    return buf;
}

// The launch of every form (q is read when PARAMS, c when CAM): the kernel, then one launch per kind of slices that adds them up.
// `what` is the entry point that was called, for the error texts.  MERGED: the merged march's kernel, its samples placed by `ms`.
template <int C, int HID, bool PARAMS, bool CAM, bool MERGED = false>
static int launch_render_backward(const ide3d_render_params& p, const ide3d_render_grads& g, const ide3d_render_param_grads* q,
                                  const ide3d_render_camera_grads* c, hipStream_t st, const char* what, const MergedSamples& ms = MergedSamples{}) {
    using PS = ParamSlice<C, HID>;
    const BwdPlan pl = plan_render_backward<C, HID, PARAMS, MERGED>(p);
    if (!pl.nw) {
        set_error("%s: %d steps per ray need %zu bytes of LDS per workgroup (at most 160 KiB)", what, (MERGED ? 2 : 1) * p.steps, pl.lds_bytes);
        return IDE3D_ENOKERNEL;
    }
    const int64_t nslices = pl.nblk * pl.nw, cam_floats = (int64_t)p.n * 12;
    float *slices = nullptr, *cam_slices = nullptr;
    if constexpr (PARAMS) {
        const int64_t need = param_workspace_bytes<C, HID, MERGED>(p);
        IDE3D_CHECK_ARG(q->workspace != nullptr && q->workspace_bytes >= need && (reinterpret_cast<uintptr_t>(q->workspace) & 15) == 0,
                        "%s: workspace of %lld bytes (16-byte aligned) required, got %lld", what, (long long)need, (long long)q->workspace_bytes);
        slices = static_cast<float*>(q->workspace);
        if (hipMemsetAsync(slices, 0, (size_t)need, st) != hipSuccess) { set_error("%s: hipMemsetAsync failed", what); return IDE3D_ELAUNCH; }
    }
    if constexpr (CAM) {
        const int64_t need = camera_workspace_bytes<C, HID>(p);
        IDE3D_CHECK_ARG(cam_floats < 0x7fffffffLL, "%s: too many images", what);
        IDE3D_CHECK_ARG(c->workspace != nullptr && c->workspace_bytes >= need && (reinterpret_cast<uintptr_t>(c->workspace) & 15) == 0,
                        "%s: camera workspace of %lld bytes (16-byte aligned) required, got %lld", what, (long long)need,
                        (long long)c->workspace_bytes);
        cam_slices = static_cast<float*>(c->workspace);
        if (hipMemsetAsync(cam_slices, 0, (size_t)(nslices * cam_floats) * sizeof(float), st) != hipSuccess) {
            set_error("%s: hipMemsetAsync failed", what);
            return IDE3D_ELAUNCH;
        }
    }
    if constexpr (MERGED) {
        auto kern = render_rays_merged_backward_kernel<C, HID, PARAMS>;
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)pl.lds_bytes);
        hipLaunchKernelGGL(kern, dim3((unsigned)pl.nblk), dim3(64 * pl.nw), pl.lds_bytes, st, p, g, pl.sp, slices, ms);
    } else {
        auto kern = render_rays_backward_kernel<C, HID, PARAMS, CAM>;
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)pl.lds_bytes);
        hipLaunchKernelGGL(kern, dim3((unsigned)pl.nblk), dim3(64 * pl.nw), pl.lds_bytes, st, p, g, pl.sp, slices, cam_slices);
    }
    IDE3D_CHECK_LAUNCH(what);
    if constexpr (PARAMS) {
        const ParamOut out = {{q->grad_geo_w0, q->grad_tex_w0, q->grad_geo_b0, q->grad_tex_b0, q->grad_geo_w1, q->grad_tex_w1, q->grad_geo_b1, q->grad_tex_b1},
                              {PS::TW0, PS::GB0, PS::TB0, PS::GW1, PS::tw1(p.seg_ch), PS::gb1(p.seg_ch, p.feat_ch), PS::tb1(p.seg_ch, p.feat_ch),
                               PS::total(p.seg_ch, p.feat_ch)}};
        hipLaunchKernelGGL(reduce_param_slices_kernel, dim3((unsigned)cdiv64(out.end[7], 64)), dim3(512), 0, st, slices, (int)nslices,
                           PS::stride(p.seg_ch, p.feat_ch), out);
        IDE3D_CHECK_LAUNCH(stage_name(what, "slice sums"));
    }
    if constexpr (CAM) {
        hipLaunchKernelGGL(reduce_camera_slices_kernel, dim3((unsigned)cdiv64(cam_floats, 64)), dim3(512), 0, st, cam_slices, (int)nslices,
                           (int)cam_floats, c->grad_cam2world);
        IDE3D_CHECK_LAUNCH(stage_name(what, "camera sums"));
    }
    return IDE3D_OK;
}

// The instantiation for what was asked for.  ms: the merged march (never with c).
template <int C, int HID>
static int launch_render_backward_form(const ide3d_render_params& p, const ide3d_render_grads& g, const ide3d_render_param_grads* q,
                                       const ide3d_render_camera_grads* c, hipStream_t st, const char* what, const MergedSamples* ms) {
    if (ms) return q ? launch_render_backward<C, HID, true, false, true>(p, g, q, nullptr, st, what, *ms)
                     : launch_render_backward<C, HID, false, false, true>(p, g, q, nullptr, st, what, *ms);
    if (q) return c ? launch_render_backward<C, HID, true, true>(p, g, q, c, st, what) : launch_render_backward<C, HID, true, false>(p, g, q, c, st, what);
    return c ? launch_render_backward<C, HID, false, true>(p, g, q, c, st, what) : launch_render_backward<C, HID, false, false>(p, g, q, c, st, what);
}

static bool grads_fit(const ide3d_render_params& p, const ide3d_render_grads& g) {
    auto ok = [&](const int64_t* s) {
        return s[1] == 1 && s[2] >= 0 && s[3] >= 0 && (s[2] * (p.H - 1) + s[3] * (p.W - 1) + 3 * p.C) < 0x7fffffffLL;
    };
    return (!g.grad_tex_planes || ok(g.grad_tex_stride)) && (!g.grad_geo_planes || ok(g.grad_geo_stride));
}

// The checks and the (C, hidden) dispatch of all four entry points.  q = NULL: no decoder gradients; c = NULL: no camera gradient;
// ms = NULL: the plain march, else the merged one (its pointers and total_steps checked by the caller) under the hierarchical pass's step
// limits (ide3d_render_rays_merged: an inner pdf needs 3 samples, ide3d_merge_depths orders at most 2048 per ray).
static int render_backward(const ide3d_render_params& p, const ide3d_render_grads& g, const ide3d_render_param_grads* q,
                           const ide3d_render_camera_grads* c, void* stream, const char* what, const MergedSamples* ms = nullptr) {
    int rc = check_render_params(p, what, kRays);
    if (!rc && ms) rc = check_hierarchical_steps(p, what);
    if (rc) return rc;
    // the tri-plane-only kernel scatters to both planes unconditionally
    IDE3D_CHECK_ARG(q || c || (g.grad_tex_planes && g.grad_geo_planes), "%s: null gradient output", what);
    IDE3D_CHECK_ARG(!c || c->grad_cam2world != nullptr, "%s: null camera-gradient output", what);
    IDE3D_CHECK_ARG(!q || (q->grad_geo_w0 && q->grad_geo_b0 && q->grad_geo_w1 && q->grad_geo_b1 && q->grad_tex_w0 && q->grad_tex_b0 &&
                           q->grad_tex_w1 && q->grad_tex_b1), "%s: null parameter-gradient output", what);
    rc = check_march_declines(p, what);
    if (rc) return rc;
    if (!grads_fit(p, g)) { set_error("%s: gradient buffers must be channels_last (channel stride 1)", what); return IDE3D_ENOKERNEL; }
    return with_form(p, false, what, [&](auto f) { return launch_render_backward_form<f.C, f.HID>(p, g, q, c, (hipStream_t)stream, what, ms); });
}

}  // namespace ide3d

extern "C" int ide3d_render_rays_backward(const ide3d_render_params* pp, const ide3d_render_grads* gg, void* stream) {
    IDE3D_CHECK_ARG(pp != nullptr && gg != nullptr, "render_rays_backward: null params");
    return ide3d::render_backward(*pp, *gg, nullptr, nullptr, stream, "render_rays_backward");
}

extern "C" int64_t ide3d_render_param_grad_workspace_bytes(const ide3d_render_params* pp) {
    using namespace ide3d;
    if (pp == nullptr || pp->n <= 0 || pp->rays_per_img <= 0 || pp->steps <= 0 || pp->feat_ch < 0 || pp->seg_ch < 0) return 0;
    return with_form(*pp, false, nullptr, [&](auto f) { return param_workspace_bytes<f.C, f.HID>(*pp); });
}

extern "C" int ide3d_render_rays_backward_params(const ide3d_render_params* pp, const ide3d_render_grads* gg, const ide3d_render_param_grads* qq,
                                                 void* stream) {
    IDE3D_CHECK_ARG(pp != nullptr && gg != nullptr && qq != nullptr, "render_rays_backward_params: null params");
    return ide3d::render_backward(*pp, *gg, qq, nullptr, stream, "render_rays_backward_params");
}

extern "C" int64_t ide3d_render_camera_grad_workspace_bytes(const ide3d_render_params* pp) {
    using namespace ide3d;
    if (pp == nullptr || pp->n <= 0 || pp->rays_per_img <= 0 || pp->steps <= 0) return 0;
    return with_form(*pp, false, nullptr, [&](auto f) { return camera_workspace_bytes<f.C, f.HID>(*pp); });
}

extern "C" int ide3d_render_rays_backward_camera(const ide3d_render_params* pp, const ide3d_render_grads* gg, const ide3d_render_param_grads* qq,
                                                 const ide3d_render_camera_grads* cc, void* stream) {
    IDE3D_CHECK_ARG(pp != nullptr && gg != nullptr, "render_rays_backward_camera: null params");
    IDE3D_CHECK_ARG(qq != nullptr || cc != nullptr || gg->grad_tex_planes || gg->grad_geo_planes, "render_rays_backward_camera: no gradient requested");
    return ide3d::render_backward(*pp, *gg, qq, cc, stream, "render_rays_backward_camera");
}

extern "C" int64_t ide3d_render_merged_param_grad_workspace_bytes(const ide3d_render_params* pp) {
    using namespace ide3d;
    if (pp == nullptr || pp->n <= 0 || pp->rays_per_img <= 0 || !hierarchical_steps_ok(pp->steps) || pp->feat_ch < 0 || pp->seg_ch < 0) return 0;
    return with_form(*pp, false, nullptr, [&](auto f) { return param_workspace_bytes<f.C, f.HID, true>(*pp); });
}

extern "C" int ide3d_render_rays_merged_backward(const ide3d_render_params* pp, const float* z_all, const int32_t* src, const float* z_fine,
                                                 int32_t total_steps, const ide3d_render_grads* gg, const ide3d_render_param_grads* qq,
                                                 void* stream) {
    IDE3D_CHECK_ARG(pp != nullptr && gg != nullptr && z_all != nullptr && src != nullptr && z_fine != nullptr,
                    "render_rays_merged_backward: null pointer");
    IDE3D_CHECK_ARG((int64_t)total_steps == 2 * (int64_t)pp->steps, "render_rays_merged_backward: total_steps must be 2 * steps = %d, got %d",
                    2 * pp->steps, total_steps);
    const ide3d::MergedSamples ms = {z_all, src, z_fine};
    return ide3d::render_backward(*pp, *gg, qq, nullptr, stream, "render_rays_merged_backward", &ms);
}
