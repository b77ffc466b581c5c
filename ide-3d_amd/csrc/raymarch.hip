// raymarch.hip — fused volumetric renderer for gfx950: ray set-up -> cam2world -> two tri-plane
// gathers -> decoder MLPs (MFMA) -> depth-ordered alpha compositing, in ONE launch.
//
// Replaces steps 3-7 of G.synthesis:
//   get_initial_rays_trig      training/volumetric_rendering.py:77-97   (points = d_cam * z)
//   perturb_points             :99-105   (offset = (U - 0.5) * (z[1] - z[0]); z += offset; p += offset * d)
//   transform_sampled_points   :108-136  (p_world = cam2world @ [p, 1])
//   sample_from_triplane x2    dnnlib/util.py:580-617
//   renderer.sample_voxel MLPs (source absent upstream; spec = DESIGN.md "decoder")
//   fancy_integration          training/volumetric_rendering.py:34-74
//
// CDNA4 mapping (round 3: DESIGN.md section 5.2c)
//   * One wavefront owns one ray and walks it in tiles of 16 depth samples, software-pipelined over the tiles of all its rays: a
//     tile's texture taps are in flight during its geometry MLP, the next tile's geometry taps during its texture MLP.
//   * Two lane layouts.  The gathers run with lane 4 j + g (sample j, 16-byte channel block g): the four lanes of a quad read 64
//     contiguous bytes of one bilinear tap — one L1 access; every tap load is the scalar-base form (plane pointer in SGPRs, 32-bit
//     byte offset, plane / slice in the immediate), all 24 of a tri-plane issued before the first is used.  The blended features
//     change lanes once (ds_bpermute) into the matrix layout lane 16 g + j (g = K block, j = column / sample).
//   * The two MLPs run in the *transposed* form out^T[features x samples] = W[features x K] * act^T[K x samples]: the features sit in
//     the B-operand layout and the D layout of layer 1 (row = 4*(l>>4)+r, col = l&15) is again a valid B operand for layer 2 once K
//     is enumerated accordingly — activations never leave registers between gather, layer 1, layer 2 and compositing.  Weights are
//     re-ordered once per workgroup into LDS in A-operand order.  (sample_voxel_kernel runs both layers per sample; render_rays_kernel
//     only the hidden layers — see the next point.)  Arithmetic: exact fp32 products on v_mfma_f32_16x16x4_f32
//     (library default), or bf16x6 (fp32-grade: 3 bf16 pieces per operand, 6 products) on v_mfma_f32_16x16x32_bf16 when a split
//     arithmetic is selected (ide3d_set_conv_arithmetic).
//   * Compositing, and the output layers once per ray: nothing non-linear sits between a branch's output layer and the sum over the
//     samples, so sum_i w_i (W1 h_i + b1) = W1 (sum_i w_i h_i) + b1 sum_i w_i.  Per sample the kernel runs the hidden layers only; sigma —
//     the one output the weights are made from — is the row-0 dot product over the lane's 16 hidden units plus two xor-shuffles across g
//     (as in density_kernel), which leaves it in every lane of the sample.  alpha / transmittance are evaluated by a 16-lane segmented
//     shuffle scan with the running transmittance carried across tiles, and each lane accumulates w * h for the 16 hidden units it holds
//     of either branch (the geometry ones right after their hidden layer: it dies before the texture MLP).  Closing a ray: a DPP
//     row reduction over the 16 samples (34 values, no LDS crossbar), then both 32-row output layers as exact fp32 FMAs in every
//     arithmetic — lane (g, j) takes rows j and j + 16 over its 16 units from a plain fp32 LDS image (conflict-free 16-byte reads), two
//     xor-shuffles add the four g slices — plus b1 * sum_i w_i; white_back / max_depth follow.  Per 16-sample tile this removed 48 of the
//     96 bf16 (64 of the 128 fp32) matrix instructions, the second bf16 split (28 v_cvt_pk + v_dot2c per 8 values) and 24 of 60 LDS
//     reads: 381 -> 320 us for the benchmark's batch (fp32 MLPs 454 -> 354; profiles/per_ray_heads/).  Nothing but the final
//     [n, feat+seg, rays] image, depth and weight sum is written.
//   * Persistent workgroups (2 per CU) take contiguous ray ranges; the range order is XCD-remapped so neighbouring rays
//     (neighbouring plane lines) share one XCD L2.
//   * The hierarchical (importance) pass is the same walk split in two around ide3d_sample_pdf and a per-ray depth merge:
//     render_ray_weights_kernel, merge_depths_kernel, render_rays_merged_kernel at the end of this file.
// Compulsory HBM traffic per image: 2 tri-planes + jitter/noise in + (feat+seg+2)*rays*4 out.  The planes are cache resident
// (L2 4 MiB/XCD + 256 MiB MALL); the kernel is bound by its vector instructions (~70 % of the VALU pipe at 2 waves per SIMD), not by HBM
// or the matrix pipe — see DESIGN.md.
#include "common.h"
#include "triplane_tap.h"
#include "raymarch_ray.h"

namespace ide3d {

typedef float f32x4 __attribute__((ext_vector_type(4)));

template <int C, int HID>
struct RmCfg {
    static constexpr int CPL = C / 16;          // float4 chunks per lane per tap
    static constexpr int NF = C / 4;            // features (K elements) per lane
    static constexpr int MT1 = HID / 16;        // layer-1 M tiles
    static constexpr int MT2 = 2;               // layer-2 M tiles (<= 32 outputs)
    // LDS carve per MLP, in floats
    static constexpr int A1 = MT1 * CPL * 64 * 4;
    static constexpr int A2 = MT2 * MT1 * 64 * 4;
    static constexpr int B0 = MT1 * 16;         // [mt][g][4]
    static constexpr int B1 = MT2 * 16;
    static constexpr int MLP = A1 + A2 + B0 + B1;
};

// The output layer w1 [nout, HID] (nout <= 32) as plain fp32, [m2][mt][lane][4]: lane 16 g + j holds w1[16 m2 + j][16 mt + 4 g + 0..3], rows
// past nout are zero.  This is the A-operand order of the fp32 matrix path, and also the order in which a lane (g, j) that holds the hidden
// units 16 mt + 4 g + r meets rows j and j + 16 (render_rays_kernel's per-ray output layer): consecutive lanes read consecutive 16 bytes.
template <int HID>
__device__ __forceinline__ void stage_out_fp32(float* __restrict__ a2, const float* __restrict__ w1, int nout) {
    constexpr int MT1 = HID / 16;
    for (int i = threadIdx.x; i < 2 * MT1 * 64 * 4; i += blockDim.x) {
        const int e = i & 3, lane = (i >> 2) & 63, rest = i >> 8;
        const int tq = rest % MT1, mt = rest / MT1;
        const int row = 16 * mt + (lane & 15), col = 16 * tq + 4 * (lane >> 4) + e;
        a2[i] = (row < nout) ? w1[row * HID + col] : 0.f;
    }
}

// Re-order one MLP's weights into LDS (A-operand order).  w0 [HID, C], w1 [nout, HID] (nout <= 32).
template <int C, int HID>
__device__ void stage_mlp(float* __restrict__ s, const float* __restrict__ w0, const float* __restrict__ b0,
                          const float* __restrict__ w1, const float* __restrict__ b1, int nout) {
    using K = RmCfg<C, HID>;
    float* a1 = s; float* a2 = a1 + K::A1; float* sb0 = a2 + K::A2; float* sb1 = sb0 + K::B0;
    for (int i = threadIdx.x; i < K::A1; i += blockDim.x) {
        const int e = i & 3, lane = (i >> 2) & 63, rest = i >> 8;
        const int ci = rest % K::CPL, mt = rest / K::CPL;
        const int row = 16 * mt + (lane & 15), col = 4 * ((lane >> 4) + 4 * ci) + e;
        a1[i] = w0[row * C + col];
    }
    stage_out_fp32<HID>(a2, w1, nout);
    for (int i = threadIdx.x; i < K::B0; i += blockDim.x) sb0[i] = b0[i];          // index = 16 mt + 4 g + r
    for (int i = threadIdx.x; i < K::B1; i += blockDim.x) sb1[i] = (i < nout) ? b1[i] : 0.f;
}

// ---- decoder MLPs on the bf16 matrix path (round 3) -----------------------------------------------------------------------------------
// v_mfma_f32_16x16x4_f32 runs at the fp32 VECTOR rate (1/16 of bf16): the two MLPs of a 16-sample tile are 128 of them = 4096 cycles
// of matrix pipe per wave and tile.  With the split arithmetic of the convolutions selected (ide3d_set_conv_arithmetic != fp32) the MLPs
// run as bf16x6 instead: every fp32 operand = 3 bf16 pieces, the 6 products above 2^-24 on v_mfma_f32_16x16x32_bf16 (K = 32 per
// instruction: layer 1 is ONE K step, layer 2 two), fp32 accumulation — 48 instead of 128 matrix instructions per tile at ~17 instead of
// 32 cycles each, fp32-grade products (no range to manage: bf16 has fp32's exponent).  The register layouts carry over: a lane (g, j)
// holds channels {4 g + e} and {16 + 4 g + e} of sample j = the 8 K values of K block g under the enumeration k(g, i) = 16 (i / 4) + 4 g
// + i % 4, and the layer-1 D registers (units 16 mt + 4 g + r) are the 8 K values of block g of K half kh = mt / 2 under
// u(kh, g, i) = 16 (2 kh + i / 4) + 4 g + i % 4; the weights are split and stored in exactly these orders once per workgroup.
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef float f32x2 __attribute__((ext_vector_type(2)));

template <int C, int HID>
struct RmSplit {
    static_assert(C == 32 && HID % 32 == 0, "split MLPs: 32 input channels (one K = 32 step), hidden width a multiple of 32");
    static constexpr int MT1 = HID / 16, KH = HID / 32;
    static constexpr int A1 = MT1 * 3 * 64;              // 16-byte units: [mt][piece][lane]
    static constexpr int A2 = 2 * KH * 3 * 64;           // [m2][k half][piece][lane]
    static constexpr int BIAS = (MT1 + 2) * 16;          // floats
    static constexpr int BYTES = (A1 + A2) * 16 + BIAS * 4;
};

// a, b -> three packed bf16 pairs (round to nearest even; the residuals are exact in fp32): low half a, high half b
// The residuals come from v_dot2c_f32_bf16: x - hi = dot((hi_a, hi_b), (-1, 0)) + x, one instruction per value instead of an unpack and
// a subtraction (exact: scripts/micro/split_dot2_check.hip compares the pieces of 2^24 values bit for bit with the mask / subtract form).
__device__ __forceinline__ void split_pair3(float a, float b, unsigned (&out)[3]) {
#pragma unroll
    for (int q = 0; q < 3; ++q) {
        const f32x2 v = {a, b};
        const bf16x2 pk = __builtin_convertvector(v, bf16x2);
        out[q] = __builtin_bit_cast(unsigned, pk);
#if defined(IDE3D_SPLIT_NO_DOT2)
        if (q < 2) { a -= __uint_as_float(out[q] << 16); b -= __uint_as_float(out[q] & 0xffff0000u); }
#else
        // (the multipliers go through scalar registers: as immediates hipcc emits the inline constant -1.0 for (-1, 0), which the instruction
        // does not read as bf16 (-1, 0))
        unsigned clo = 0x0000bf80u, chi = 0xbf800000u;
        asm volatile("" : "+s"(clo), "+s"(chi));
        const bf16x2 mlo = __builtin_bit_cast(bf16x2, clo), mhi = __builtin_bit_cast(bf16x2, chi);
        if (q < 2) { a = __builtin_amdgcn_fdot2_f32_bf16(pk, mlo, a, false); b = __builtin_amdgcn_fdot2_f32_bf16(pk, mhi, b, false); }
#endif
    }
}
__device__ __forceinline__ void split8(const float (&v)[8], u32x4 (&out)[3]) {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        unsigned pk[3];
        split_pair3(v[2 * e], v[2 * e + 1], pk);
        out[0][e] = pk[0]; out[1][e] = pk[1]; out[2][e] = pk[2];
    }
}
__device__ __forceinline__ f32x4 mfma6(const u32x4 (&a)[3], const u32x4 (&b)[3], f32x4 acc) {
    // smallest products first
#pragma unroll
    for (int sum = 2; sum >= 0; --sum)
#pragma unroll
        for (int qa = 0; qa <= sum; ++qa)
            acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a[qa]), __builtin_bit_cast(bf16x8, b[sum - qa]), acc, 0, 0, 0);
    return acc;
}

// first layer, pre-split: [mt][piece][lane]
template <int C, int HID>
__device__ __forceinline__ void stage_split_layer1(u32x4* __restrict__ a1, const float* __restrict__ w0) {
    using K = RmSplit<C, HID>;
    for (int i = threadIdx.x; i < K::MT1 * 64; i += blockDim.x) {
        const int lane = i & 63, mt = i >> 6, g = lane >> 4, row = 16 * mt + (lane & 15);
        float v[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) v[k] = w0[row * C + 16 * (k / 4) + 4 * g + k % 4];
        u32x4 pc[3];
        split8(v, pc);
#pragma unroll
        for (int q = 0; q < 3; ++q) a1[(mt * 3 + q) * 64 + lane] = pc[q];
    }
}
// biases: b0 at index 16 mt + 4 g + r, then the 32 output rows' (zero past nout)
template <int HID>
__device__ __forceinline__ void stage_split_biases(float* __restrict__ sb, const float* __restrict__ b0, const float* __restrict__ b1, int nout) {
    for (int i = threadIdx.x; i < HID; i += blockDim.x) sb[i] = b0[i];
    for (int i = threadIdx.x; i < 32; i += blockDim.x) sb[HID + i] = (i < nout) ? b1[i] : 0.f;
}

template <int C, int HID>
__device__ void stage_mlp_split(unsigned char* __restrict__ sm, const float* __restrict__ w0, const float* __restrict__ b0,
                                const float* __restrict__ w1, const float* __restrict__ b1, int nout) {
    using K = RmSplit<C, HID>;
    u32x4* a1 = reinterpret_cast<u32x4*>(sm);
    u32x4* a2 = a1 + K::A1;
    stage_split_layer1<C, HID>(a1, w0);
    for (int i = threadIdx.x; i < 2 * K::KH * 64; i += blockDim.x) {
        const int lane = i & 63, kh = (i >> 6) % K::KH, m2 = i / (64 * K::KH), g = lane >> 4, row = 16 * m2 + (lane & 15);
        float v[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) v[k] = (row < nout) ? w1[row * HID + 16 * (2 * kh + k / 4) + 4 * g + k % 4] : 0.f;
        u32x4 pc[3];
        split8(v, pc);
#pragma unroll
        for (int q = 0; q < 3; ++q) a2[((m2 * K::KH + kh) * 3 + q) * 64 + lane] = pc[q];
    }
    stage_split_biases<HID>(reinterpret_cast<float*>(a2 + K::A2), b0, b1, nout);
}

// A2U: the 16-byte units of the output layer's image that lie between the first layer and the biases (render_rays_kernel keeps a smaller one)
template <int C, int HID, int A2U = RmSplit<C, HID>::A2>
__device__ __forceinline__ void mlp_hidden_split(const unsigned char* __restrict__ sm, const float (&f)[C / 4], f32x4 (&h)[HID / 16]) {
    using K = RmSplit<C, HID>;
    const int lane = lane_id(), g = lane >> 4;
    const u32x4* a1 = reinterpret_cast<const u32x4*>(sm);
    const f32x4* sb0 = reinterpret_cast<const f32x4*>(sm + (K::A1 + A2U) * 16);
    u32x4 fb[3];
    split8(f, fb);
#pragma unroll
    for (int mt = 0; mt < K::MT1; ++mt) {
        const u32x4 a[3] = {a1[(mt * 3 + 0) * 64 + lane], a1[(mt * 3 + 1) * 64 + lane], a1[(mt * 3 + 2) * 64 + lane]};
        h[mt] = mfma6(a, fb, sb0[mt * 4 + g]);
    }
#pragma unroll
    for (int mt = 0; mt < K::MT1; ++mt)
#pragma unroll
        for (int r = 0; r < 4; ++r) h[mt][r] = softplus_fast(h[mt][r]);
}

template <int C, int HID>
__device__ __forceinline__ void mlp_tile_split(const unsigned char* __restrict__ sm, const float (&f)[C / 4], f32x4 (&out)[2]) {
    using K = RmSplit<C, HID>;
    const int lane = lane_id(), g = lane >> 4;
    const u32x4* a2 = reinterpret_cast<const u32x4*>(sm) + K::A1;
    const f32x4* sb1 = reinterpret_cast<const f32x4*>(sm + (K::A1 + K::A2) * 16) + K::MT1 * 4;
    f32x4 h[K::MT1];
    mlp_hidden_split<C, HID>(sm, f, h);
    u32x4 hb[K::KH][3];
#pragma unroll
    for (int kh = 0; kh < K::KH; ++kh) {
        const float v[8] = {h[2 * kh][0], h[2 * kh][1], h[2 * kh][2], h[2 * kh][3], h[2 * kh + 1][0], h[2 * kh + 1][1], h[2 * kh + 1][2], h[2 * kh + 1][3]};
        split8(v, hb[kh]);
    }
#pragma unroll
    for (int m2 = 0; m2 < 2; ++m2) {
        f32x4 acc = sb1[m2 * 4 + g];
#pragma unroll
        for (int kh = 0; kh < K::KH; ++kh) {
            const int o = ((m2 * K::KH + kh) * 3) * 64 + lane;
            const u32x4 a[3] = {a2[o], a2[o + 64], a2[o + 128]};
            acc = mfma6(a, hb[kh], acc);
        }
        out[m2] = acc;
    }
}

// Row 0 of the geometry output layer (sigma) from the hidden vector of a sample, which is spread over its four lanes (lane (g, j) holds
// units 16 mt + 4 g + r): a 16-term partial sum on the VALU and two xor-shuffles across g; every lane of sample j returns the value.
// s_row: w1[0][0..HID) followed by b1[0].
template <int HID>
__device__ __forceinline__ float sigma_row0(const float* __restrict__ s_row, const f32x4 (&h)[HID / 16]) {
    const int g = lane_id() >> 4;
    float acc = 0.f;
#pragma unroll
    for (int mt = 0; mt < HID / 16; ++mt) {
        const f32x4 w = *reinterpret_cast<const f32x4*>(s_row + 16 * mt + 4 * g);
#pragma unroll
        for (int r = 0; r < 4; ++r) acc += w[r] * h[mt][r];
    }
    acc += __shfl_xor(acc, 16);
    acc += __shfl_xor(acc, 32);
    return acc + s_row[HID];
}

// (density only, split form) hidden layer on the bf16 matrix path, row 0 of the second layer as a VALU dot product like mlp_sigma
template <int C, int HID>
__device__ __forceinline__ float mlp_sigma_split(const unsigned char* __restrict__ sm, const float* __restrict__ s_row, const float (&f)[C / 4]) {
    f32x4 h[HID / 16];
    mlp_hidden_split<C, HID>(sm, f, h);
    return sigma_row0<HID>(s_row, h);
}

// Gather this lane's NF features of one sample from one tri-plane (channels_last, channel stride 1).
// Lane layouts.  The matrix instructions want lane 16 g + j to hold K block g of sample (column) j: neighbouring lanes are
// DIFFERENT samples.  Gathering in that layout makes every lane of a 16-byte load its own cache-line access (16 useful bytes per L1
// access; 64 accesses per instruction; the kernel then runs at exactly the L1 access rate: 2 tri-planes x 12 taps x 8 accesses per
// sample = 0.49 ms for the 1.57 M samples of the benchmark pass, measured 0.50 — round 3).  So the gathers run in a second layout,
// lane 4 j + g (`gather layout`: four neighbouring lanes read 64 contiguous bytes of one tap of one sample — one access), each lane
// blends its 16-byte slices with the tap weights of sample lane / 4, and the blended features — 8 values per lane and tri-plane —
// change lanes once (ds_bpermute, no memory) into the matrix layout.
__device__ __forceinline__ int gather_sample(int lane) { return lane >> 2; }
__device__ __forceinline__ int gather_block(int lane) { return lane & 3; }

template <int NF>
__device__ __forceinline__ void to_matrix_lanes(float (&f)[NF]) {
    const int lane = lane_id();
    const int src = (((lane & 15) << 2) | (lane >> 4)) << 2;        // lane 16 g + j reads lane 4 j + g (byte address of its dword)
#pragma unroll
    for (int i = 0; i < NF; ++i) f[i] = __int_as_float(__builtin_amdgcn_ds_bpermute(src, __float_as_int(f[i])));
}

template <int C> struct TapBuf { float4 v[C / 16][3][4]; };

// a global-memory address known to be the same in every lane -> scalar registers (what the scalar-base load form needs)
typedef const __attribute__((address_space(1))) char* GlobalBytes;
template <class T>
__device__ __forceinline__ GlobalBytes uniform_ptr(const T* p) {
    const unsigned long long v = reinterpret_cast<unsigned long long>(p);
    const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)v), hi = __builtin_amdgcn_readfirstlane((unsigned)(v >> 32));
    return reinterpret_cast<GlobalBytes>(((unsigned long long)hi << 32) | lo);
}

__device__ __forceinline__ float4 ld4_at(GlobalBytes base, unsigned byte_off, unsigned imm) {
    typedef float v4f __attribute__((ext_vector_type(4)));
    typedef const __attribute__((address_space(1))) v4f* GlobalF4;
    const v4f v = *reinterpret_cast<GlobalF4>(base + (size_t)byte_off + imm);
    return make_float4(v[0], v[1], v[2], v[3]);
}

template <int C>
__device__ __forceinline__ void issue_taps(GlobalBytes pbc, const TapAddr (&t)[3], int g, TapBuf<C>& b, unsigned lane_extra = 0) {
    constexpr int CPL = C / 16;
    // Every 16-byte tap load of the sample — 12 per channel slice, all CPL slices — is issued before the first one is consumed; left
    // to itself the compiler loads a plane's four taps, waits, blends.
    // `pb` is wave-uniform and the tap offsets are unsigned 32-bit byte counts (planes_fast bounds them), so every load is the
    // scalar-base form — global_load_dwordx4 v, v_off, s[base:base+1] offset:imm — with the plane / slice part in the immediate: no
    // 64-bit address arithmetic per tap.
    const unsigned lane_b = 16u * (unsigned)g + lane_extra;          // lane_extra: a per-lane byte offset on top (an image further on)
#pragma unroll
    for (int ci = 0; ci < CPL; ++ci) {
#pragma unroll
        for (int pl = 0; pl < 3; ++pl) {
            const unsigned imm = (unsigned)(pl * C + 16 * ci) * 4u;
            b.v[ci][pl][0] = ld4_at(pbc, (unsigned)t[pl].o00 * 4u + lane_b, imm); b.v[ci][pl][1] = ld4_at(pbc, (unsigned)t[pl].o01 * 4u + lane_b, imm);
            b.v[ci][pl][2] = ld4_at(pbc, (unsigned)t[pl].o10 * 4u + lane_b, imm); b.v[ci][pl][3] = ld4_at(pbc, (unsigned)t[pl].o11 * 4u + lane_b, imm);
        }
    }
}

template <int C>
__device__ __forceinline__ void blend_taps(TapBuf<C>& b, const TapAddr (&t)[3], float (&f)[C / 4]) {
    constexpr int CPL = C / 16;
#pragma unroll
    for (int ci = 0; ci < CPL; ++ci)
#pragma unroll
        for (int pl = 0; pl < 3; ++pl)
#pragma unroll
            for (int k = 0; k < 4; ++k) asm volatile("" : "+v"(b.v[ci][pl][k].x), "+v"(b.v[ci][pl][k].y), "+v"(b.v[ci][pl][k].z), "+v"(b.v[ci][pl][k].w));
#pragma unroll
    for (int ci = 0; ci < CPL; ++ci) {
        float4 a[3];
#pragma unroll
        for (int pl = 0; pl < 3; ++pl) {
            float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
            acc = f4_fma(b.v[ci][pl][0], t[pl].w00, acc);
            acc = f4_fma(b.v[ci][pl][1], t[pl].w01, acc);
            acc = f4_fma(b.v[ci][pl][2], t[pl].w10, acc);
            acc = f4_fma(b.v[ci][pl][3], t[pl].w11, acc);
            a[pl] = acc;
        }
        f[4 * ci + 0] = (a[0].x + a[1].x) + a[2].x;
        f[4 * ci + 1] = (a[0].y + a[1].y) + a[2].y;
        f[4 * ci + 2] = (a[0].z + a[1].z) + a[2].z;
        f[4 * ci + 3] = (a[0].w + a[1].w) + a[2].w;
    }
}

// `t`: taps of sample gather_sample(lane); `g` = gather_block(lane).  Result in the gather layout (f[4 ci + e] = channel
// 16 ci + 4 g + e of that sample): follow with to_matrix_lanes.
template <int C>
__device__ __forceinline__ void gather_features(const float* __restrict__ pb, const TapAddr (&t)[3], int g, float (&f)[C / 4]) {
    TapBuf<C> b;
    issue_taps<C>(uniform_ptr(pb), t, g, b);
    blend_taps<C>(b, t, f);
}

// Two-layer MLP on a 16-sample tile, transposed MFMA form.  out[mt][r] = feature 16 mt + 4 g + r of sample j.
template <int C, int HID>
__device__ __forceinline__ void mlp_hidden(const float* __restrict__ s, const float (&f)[C / 4], f32x4 (&h)[HID / 16]) {
    using K = RmCfg<C, HID>;
    const int lane = lane_id();
    const f32x4* a1 = reinterpret_cast<const f32x4*>(s);
    const f32x4* sb0 = reinterpret_cast<const f32x4*>(s + K::A1 + K::A2);
    const int g = lane >> 4;
#pragma unroll
    for (int mt = 0; mt < K::MT1; ++mt) h[mt] = sb0[mt * 4 + g];
#pragma unroll
    for (int ci = 0; ci < K::CPL; ++ci) {
        f32x4 w[K::MT1];
#pragma unroll
        for (int mt = 0; mt < K::MT1; ++mt) w[mt] = a1[(mt * K::CPL + ci) * 64 + lane];
#pragma unroll
        for (int e = 0; e < 4; ++e)
#pragma unroll
            for (int mt = 0; mt < K::MT1; ++mt)
                h[mt] = __builtin_amdgcn_mfma_f32_16x16x4f32(w[mt][e], f[4 * ci + e], h[mt], 0, 0, 0);
    }
#pragma unroll
    for (int mt = 0; mt < K::MT1; ++mt)
#pragma unroll
        for (int r = 0; r < 4; ++r) h[mt][r] = softplus_fast(h[mt][r]);
}

template <int C, int HID>
__device__ __forceinline__ void mlp_tile(const float* __restrict__ s, const float (&f)[C / 4], f32x4 (&out)[2]) {
    using K = RmCfg<C, HID>;
    const int lane = lane_id();
    const f32x4* a2 = reinterpret_cast<const f32x4*>(s + K::A1);
    const f32x4* sb1 = reinterpret_cast<const f32x4*>(s + K::A1 + K::A2 + K::B0);
    const int g = lane >> 4;
    f32x4 h[K::MT1];
    mlp_hidden<C, HID>(s, f, h);
#pragma unroll
    for (int mt = 0; mt < 2; ++mt) out[mt] = sb1[mt * 4 + g];
#pragma unroll
    for (int tq = 0; tq < K::MT1; ++tq) {
        const f32x4 w0 = a2[(0 * K::MT1 + tq) * 64 + lane];
        const f32x4 w1 = a2[(1 * K::MT1 + tq) * 64 + lane];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            out[0] = __builtin_amdgcn_mfma_f32_16x16x4f32(w0[e], h[tq][e], out[0], 0, 0, 0);
            out[1] = __builtin_amdgcn_mfma_f32_16x16x4f32(w1[e], h[tq][e], out[1], 0, 0, 0);
        }
    }
}

// Density only: of the second layer just row 0 (sigma) is needed — a 64-term dot product per sample (sigma_row0): ~20 vector
// instructions instead of the 32 MFMAs (1024 cycles) of the 32-row layer.
template <int C, int HID>
__device__ __forceinline__ float mlp_sigma(const float* __restrict__ s, const float* __restrict__ s_row, const float (&f)[C / 4]) {
    f32x4 h[HID / 16];
    mlp_hidden<C, HID>(s, f, h);
    return sigma_row0<HID>(s_row, h);
}

__device__ __forceinline__ float seg16_excl_prod(float v, float& total) {
    // exclusive prefix product inside each aligned group of 16 lanes
    const int j = lane_id() & 15;
    float incl = v;
#pragma unroll
    for (int off = 1; off < 16; off <<= 1) {
        const float o = __shfl_up(incl, off, 16);
        if (j >= off) incl *= o;
    }
    total = __shfl(incl, 15, 16);
    const float prev = __shfl_up(incl, 1, 16);
    return j == 0 ? 1.0f : prev;
}

// MLP storage of one decoder branch in LDS, by arithmetic (SPLIT: bf16x6 on v_mfma_f32_16x16x32_bf16; else fp32 MFMA)
template <int C, int HID, bool SPLIT> struct MlpBytes { static constexpr int value = RmCfg<C, HID>::MLP * 4; };
template <int C, int HID> struct MlpBytes<C, HID, true> { static constexpr int value = RmSplit<C, HID>::BYTES; };

template <int C, int HID, bool SPLIT>
__device__ __forceinline__ void stage_branch(unsigned char* sm, const float* w0, const float* b0, const float* w1, const float* b1, int nout) {
    if constexpr (SPLIT) stage_mlp_split<C, HID>(sm, w0, b0, w1, b1, nout);
    else stage_mlp<C, HID>(reinterpret_cast<float*>(sm), w0, b0, w1, b1, nout);
}
template <int C, int HID, bool SPLIT>
__device__ __forceinline__ void mlp_branch(const unsigned char* sm, const float (&f)[C / 4], f32x4 (&out)[2]) {
    if constexpr (SPLIT) mlp_tile_split<C, HID>(sm, f, out);
    else mlp_tile<C, HID>(reinterpret_cast<const float*>(sm), f, out);
}

// ---- render_rays_kernel: the output layers once per ray -------------------------------------------------------------------------------
// Between the output layer of a decoder branch and the sum over a ray's samples nothing is non-linear (white_back and max_depth are added
// after the sum), so   sum_i w_i (W1 h_i + b1)  =  W1 (sum_i w_i h_i) + b1 sum_i w_i :   the sample loop runs the hidden layers only, takes
// sigma — the one output the weights w_i are made from — as the row-0 dot product (sigma_row0, as density_kernel does) and composites the
// hidden vectors; the 32-row output layers run once per ray on the composited vector, as exact fp32 FMAs in every arithmetic.
//
// LDS image of one branch: the first layer and the biases as the arithmetic's hidden layer reads them; in between the output layer as plain
// fp32 in stage_out_fp32's order, which the fp32 form's image holds anyway — the split form keeps it in place of its pre-split A2 pieces.
// Row 0 of the geometry layer and its bias follow the two branches (`s_row`, RmRender::ROW floats).
template <int C, int HID, bool SPLIT> struct RmRender {
    using K = RmCfg<C, HID>;
    static constexpr int W2_OFF = K::A1 * 4, B1_OFF = (K::A1 + K::A2 + K::B0) * 4, BYTES = K::MLP * 4;          // bytes
    static constexpr int ROW = HID + 4;
};
template <int C, int HID> struct RmRender<C, HID, true> {
    using K = RmSplit<C, HID>;
    static constexpr int W2 = 2 * K::MT1 * 64;                                                                   // 16-byte units
    static constexpr int W2_OFF = K::A1 * 16, B1_OFF = (K::A1 + W2) * 16 + HID * 4, BYTES = (K::A1 + W2) * 16 + K::BIAS * 4;
    static constexpr int ROW = HID + 4;
};

template <int C, int HID, bool SPLIT>
__device__ __forceinline__ void stage_render_branch(unsigned char* sm, const float* w0, const float* b0, const float* w1, const float* b1, int nout) {
    if constexpr (SPLIT) {
        using R = RmRender<C, HID, true>;
        stage_split_layer1<C, HID>(reinterpret_cast<u32x4*>(sm), w0);
        stage_out_fp32<HID>(reinterpret_cast<float*>(sm + R::W2_OFF), w1, nout);
        stage_split_biases<HID>(reinterpret_cast<float*>(sm + R::W2_OFF + R::W2 * 16), b0, b1, nout);
    } else {
        stage_mlp<C, HID>(reinterpret_cast<float*>(sm), w0, b0, w1, b1, nout);
    }
}
template <int C, int HID, bool SPLIT>
__device__ __forceinline__ void hidden_branch(const unsigned char* sm, const float (&f)[C / 4], f32x4 (&h)[HID / 16]) {
    if constexpr (SPLIT) mlp_hidden_split<C, HID, RmRender<C, HID, true>::W2>(sm, f, h);
    else mlp_hidden<C, HID>(reinterpret_cast<const float*>(sm), f, h);
}

// v + (v of the lane that `CTRL` names), a DPP operand of the addition: no LDS crossbar round trip
template <int CTRL>
__device__ __forceinline__ float dpp_add(float v) {
    return v + __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xf, 0xf, false));
}
// sum over each aligned row of 16 lanes, in every lane of the row: neighbours in a quad (quad_perm [1,0,3,2], [2,3,0,1]), then the other quad
// of the half row and the other half row (row_half_mirror, row_mirror: the quads / half rows are uniform by then)
__device__ __forceinline__ float row16_sum(float v) {
    v = dpp_add<0xB1>(v); v = dpp_add<0x4E>(v); v = dpp_add<0x141>(v); v = dpp_add<0x140>(v);
    return v;
}

// One branch's output layer on the composited hidden vector of a ray: acc[4 mt + r] = sum_i w_i h_i[16 mt + 4 g + r], already summed over the
// ray's samples in every lane.  Lane (g, j) forms the partial sums of rows j and j + 16 over its 16 units, two xor-shuffles add the four g
// slices: out[m2] = b1[16 m2 + j] * wsum + sum_u W1[16 m2 + j][u] H[u] in every lane (zero for rows past the decoder's).
template <int C, int HID, bool SPLIT>
__device__ __forceinline__ void heads_per_ray(const unsigned char* sm, const float (&acc)[HID / 4], float wsum, float (&out)[2]) {
    using R = RmRender<C, HID, SPLIT>;
    constexpr int MT1 = HID / 16;
    const int lane = lane_id();
    const f32x4* w2 = reinterpret_cast<const f32x4*>(sm + R::W2_OFF);
    const float* sb1 = reinterpret_cast<const float*>(sm + R::B1_OFF);
#pragma unroll
    for (int m2 = 0; m2 < 2; ++m2) {
        float a = 0.f;
#pragma unroll
        for (int mt = 0; mt < MT1; ++mt) {
            const f32x4 w = w2[(m2 * MT1 + mt) * 64 + lane];
#pragma unroll
            for (int r = 0; r < 4; ++r) a = fmaf(w[r], acc[4 * mt + r], a);
        }
        a += __shfl_xor(a, 16);
        a += __shfl_xor(a, 32);
        out[m2] = fmaf(sb1[16 * m2 + (lane & 15)], wsum, a);
    }
}

// Exclusive residency (modconv.hip `kSpExclusive`): the SPLIT forms of the three kernels below run LDS-fed bf16
// MFMA loops, beside which a foreign wave's packed-fp32 instructions return wrong values on MI355X.  They are therefore launched as 8-wave
// workgroups, one per CU: two of the workgroup's own waves, 256 registers each (`rm_claim_half_simd`), fill every SIMD, and no wave leaves
// before all have finished (`__syncthreads()` at the end), so no foreign wave ever shares a SIMD with a running MLP.  The fp32 forms
// (v_mfma_f32_16x16x4_f32 was never observed as a neighbour that matters) keep 4-wave workgroups, two per CU.
template <bool SPLIT> struct RmWaves { static constexpr int value = SPLIT ? 8 : 4; };
template <bool SPLIT> __device__ __forceinline__ void rm_claim_half_simd() { if constexpr (SPLIT) asm volatile("" ::: "v255"); }

// ---- the parts the three ray marchers (render_rays_kernel and the two of the hierarchical pass) are built from ----------------------------

// the tile after (ray, n, r, s0) of a wave that takes every NW-th ray and walks `steps` samples per ray in tiles of 16
template <int NW>
__device__ __forceinline__ void next_tile(int steps, int rays_per_img, int64_t& ray, int& n, int& r, int& s0) {
    s0 += 16;
    if (s0 >= steps) {
        s0 = 0; ray += NW; r += NW;
        while (r >= rays_per_img) { r -= rays_per_img; ++n; }
    }
}

// Dynamic LDS of a marcher: the geometry branch's image, the texture branch's when it runs one (TEX), then `s_row`.
template <int C, int HID, bool SPLIT, bool TEX>
constexpr int kMarchLdsBytes = (TEX ? 2 : 1) * RmRender<C, HID, SPLIT>::BYTES + RmRender<C, HID, SPLIT>::ROW * (int)sizeof(float);

// What a marcher's wave knows once its workgroup has staged the decoder: the LDS images, its lane in both layouts (matrix: lane 16 g + j;
// gather: 16-byte channel block gl), the end of the workgroup's contiguous ray range (XCD-remapped, see the head of the file) and the wave's
// first ray with its image n and index r in the image (wave-uniform, scalar registers).
struct MarchWave {
    unsigned char *s_geo, *s_tex;
    float* s_row;                                          // row 0 of geo_w1 + its bias
    int lane, wid, g, j, gl;
    int64_t ray_end, ray;
    int n, r;
};
template <int C, int HID, bool SPLIT, bool TEX>
__device__ __forceinline__ MarchWave march_prologue(const ide3d_render_params& p, int64_t rays_per_block) {
    using R = RmRender<C, HID, SPLIT>;
    extern __shared__ __attribute__((aligned(16))) float lds[];
    MarchWave m;
    m.s_geo = reinterpret_cast<unsigned char*>(lds);
    m.s_tex = m.s_geo + R::BYTES;
    m.s_row = reinterpret_cast<float*>(m.s_geo + (TEX ? 2 : 1) * R::BYTES);
    stage_render_branch<C, HID, SPLIT>(m.s_geo, p.geo_w0, p.geo_b0, p.geo_w1, p.geo_b1, 1 + p.seg_ch);
    if constexpr (TEX) stage_render_branch<C, HID, SPLIT>(m.s_tex, p.tex_w0, p.tex_b0, p.tex_w1, p.tex_b1, p.feat_ch);
    for (int i = threadIdx.x; i <= HID; i += blockDim.x) m.s_row[i] = (i < HID) ? p.geo_w1[i] : p.geo_b1[0];
    __syncthreads();

    m.lane = lane_id(); m.wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    m.g = m.lane >> 4; m.j = m.lane & 15; m.gl = gather_block(m.lane);
    const int64_t total_rays = (int64_t)p.n * p.rays_per_img;
    const int blk = xcd_remap(blockIdx.x, gridDim.x);
    const int64_t ray_begin = (int64_t)blk * rays_per_block;
    m.ray_end = ray_begin + rays_per_block;
    if (m.ray_end > total_rays) m.ray_end = total_rays;
    // (the image index advances by comparison from here on, not by a 64-bit division per tile)
    m.ray = ray_begin + m.wid;
    m.n = __builtin_amdgcn_readfirstlane((int)(m.ray / p.rays_per_img));
    m.r = __builtin_amdgcn_readfirstlane((int)(m.ray - (int64_t)m.n * p.rays_per_img));
    return m;
}

// Compositing weight of sample j of a tile of ray r, in every lane of the sample, from its geometry hidden vector: sigma (+ noise) -> density
// -> alpha over the distance to the next sample (`inner`; 1e10 behind the ray's last) -> the transmittance in front of it = `carry` (the
// ray's before this tile) times the 16-lane exclusive scan.  `tot`: the transmittance of the whole tile, for the caller's carry.  Lanes past
// the ray's end (`!live`) weigh nothing and leave the scan alone.
template <int HID, bool NOISE>
__device__ __forceinline__ float composite_step(const ide3d_render_params& p, const float* s_row, const f32x4 (&hg)[HID / 16], int r, float noise,
                                                float z, float znext, bool live, bool inner, float carry, float& tot) {
    float sigma = sigma_row0<HID>(s_row, hg);
    if constexpr (NOISE) sigma += noise;
    const float dens = p.clamp_mode == 0 ? softplus_fast(sigma) : fmaxf(sigma, 0.f);
    const float dx = p.rays_d_cam[r * 3 + 0], dy = p.rays_d_cam[r * 3 + 1], dz = p.rays_d_cam[r * 3 + 2];
    const float dnorm = sqrtf(dx * dx + dy * dy + dz * dz);
    const float delta = inner ? (znext - z) * dnorm : 1e10f;
    const float alpha = live ? 1.0f - __expf(-delta * dens) : 0.f;
    const float fac = live ? (1.0f - alpha + 1e-10f) : 1.0f;
    const float excl = seg16_excl_prod(fac, tot);
    return alpha * (carry * excl);
}

// acc[4 mt + r] += w * h[mt][r]: sum_i w_i h_i of the units 16 mt + 4 g + r, over this lane's samples
template <int MT1>
__device__ __forceinline__ void accumulate_hidden(float (&acc)[4 * MT1], float w, const f32x4 (&h)[MT1]) {
#pragma unroll
    for (int mt = 0; mt < MT1; ++mt)
#pragma unroll
        for (int rr = 0; rr < 4; ++rr) acc[mt * 4 + rr] += w * h[mt][rr];
}

// Closing ray `ray` (r of image n): reduce over the 16 samples held by lanes with equal g, then the output layers on the sums; the feature
// image, depth and weight sum are written with white_back / max_depth applied, and the ray's running sums start over.
template <int C, int HID, bool SPLIT>
__device__ __forceinline__ void close_ray(const ide3d_render_params& p, const MarchWave& m, int64_t ray, int n, int r, float (&acc_t)[HID / 4],
                                          float (&acc_g)[HID / 4], float& carry, float& wsum, float& dsum) {
    constexpr int NA = HID / 4;
    const int g = m.g, j = m.j, nch = p.feat_ch + p.seg_ch;
    wsum = row16_sum(wsum); dsum = row16_sum(dsum);
#pragma unroll
    for (int i = 0; i < NA; ++i) { acc_g[i] = row16_sum(acc_g[i]); acc_t[i] = row16_sum(acc_t[i]); }
    float o_t[2], o_g[2];
    heads_per_ray<C, HID, SPLIT>(m.s_tex, acc_t, wsum, o_t);
    heads_per_ray<C, HID, SPLIT>(m.s_geo, acc_g, wsum, o_g);
    // every lane holds rows j and j + 16 of both branches: the g = 0 .. 3 lanes write texture row j, j + 16, geometry row j, j + 16.
    // last_back needs the un-weighted features of the final sample; not supported in the fused kernel (host guards), white_back / max_depth are.
    const float bg = p.white_back ? (1.0f - wsum) : 0.f;
    float* of = p.out_feat + (int64_t)n * nch * p.rays_per_img + r;
    const int idx = j + 16 * (g & 1);
    const float v = (g & 2) ? ((g & 1) ? o_g[1] : o_g[0]) : ((g & 1) ? o_t[1] : o_t[0]);
    if (g < 2) {
        if (idx < p.feat_ch) of[(int64_t)idx * p.rays_per_img] = v + bg;
    } else {
        if (idx >= 1 && idx <= p.seg_ch) of[(int64_t)(p.feat_ch + idx - 1) * p.rays_per_img] = v + bg;      // row 0 is sigma
    }
    if (m.lane == 0) {
        if (p.out_depth) p.out_depth[ray] = dsum + ((p.max_depth != 0.f) ? (1.0f - wsum) * p.max_depth : 0.f);
        if (p.out_wsum) p.out_wsum[ray] = wsum;
    }
#pragma unroll
    for (int i = 0; i < NA; ++i) { acc_t[i] = 0.f; acc_g[i] = 0.f; }
    carry = 1.0f; wsum = 0.f; dsum = 0.f;
}


template <int C, int HID, bool SPLIT>
__global__ void __launch_bounds__(64 * RmWaves<SPLIT>::value, 2)
render_rays_kernel(ide3d_render_params p, int64_t rays_per_block) {
    using K = RmCfg<C, HID>;
    constexpr int NW = RmWaves<SPLIT>::value;
    rm_claim_half_simd<SPLIT>();
    // march_prologue<C, HID, SPLIT, true>, written out: this kernel's instruction stream is pinned
    extern __shared__ __attribute__((aligned(16))) float lds[];
    using R = RmRender<C, HID, SPLIT>;
    constexpr int NA = HID / 4;                            // hidden units per lane and branch
    unsigned char* s_geo = reinterpret_cast<unsigned char*>(lds);
    unsigned char* s_tex = s_geo + R::BYTES;
    float* const s_row = reinterpret_cast<float*>(s_tex + R::BYTES);           // row 0 of geo_w1 + its bias
    stage_render_branch<C, HID, SPLIT>(s_geo, p.geo_w0, p.geo_b0, p.geo_w1, p.geo_b1, 1 + p.seg_ch);
    stage_render_branch<C, HID, SPLIT>(s_tex, p.tex_w0, p.tex_b0, p.tex_w1, p.tex_b1, p.feat_ch);
    for (int i = threadIdx.x; i <= HID; i += blockDim.x) s_row[i] = (i < HID) ? p.geo_w1[i] : p.geo_b1[0];
    __syncthreads();

    const int lane = lane_id(), wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int g = lane >> 4, j = lane & 15, gl = gather_block(lane);
    const int64_t total_rays = (int64_t)p.n * p.rays_per_img;
    const int blk = xcd_remap(blockIdx.x, gridDim.x);
    const int64_t ray_begin = (int64_t)blk * rays_per_block;
    int64_t ray_end = ray_begin + rays_per_block;
    if (ray_end > total_rays) ray_end = total_rays;
    const int S = p.steps;
    const int nch = p.feat_ch + p.seg_ch;
    const int sH = (int)p.tex_stride[2], sW = (int)p.tex_stride[3];   // host guarantees tex / geo share the layout
    const float zstep = (S > 1) ? (p.z_lin[1] - p.z_lin[0]) : 0.f;

    // Depth of sample s0 + lane / 4 of `ray` (gather layout): the two small loads the tap addresses hang on, issued one tile ahead.
    auto tile_depth = [&](int64_t ray, int s0, float& zl, float& jl) {
        const int sl = min(s0 + gather_sample(lane), S - 1);
        zl = p.z_lin[sl];
        jl = p.jitter ? p.jitter[ray * S + sl] : 0.5f;
    };
    // Taps of that sample: camera space -> jitter -> world.  Everything per ray is wave-uniform (scalar loads), so a tile of the NEXT
    // ray costs the same as one of this ray.
    auto tile_taps = [&](int n, int r, float zl, float jl, TapAddr (&t)[3]) {
        float wx, wy, wz;
        ray_world_point(p, n, r, zl, jl, zstep, wx, wy, wz);
        triplane_tap_addrs(wx, wy, wz, p.W, p.H, sH, sW, t);
    };

    // Software pipeline over the tiles (ray, s0) of this wave, flattened across rays.  The loads of a tile's texture taps fly during
    // its geometry MLP and the geometry taps of the NEXT tile during its texture MLP: with the L1 access rate out of the way (gather
    // layout) the kernel is otherwise the sum of its exposed gather round trips and its arithmetic (2 waves per SIMD hide little).
    // vmcnt retires in order, so nothing that is needed during an MLP may be loaded after the taps that fly across it: the small
    // loads of a tile (its depths, the next tile's depths) are issued first, and the kernel must not spill (a scratch reload inside
    // an MLP would wait for the taps).
    // (ray, image n, ray-in-image r, s0) of the current tile: wave-uniform, kept in scalar registers (the image index advances by
    // comparison, not by a 64-bit division per tile; plane bases are scalar pointers for the scalar-base loads)
    int64_t ray = ray_begin + wid;
    int n = __builtin_amdgcn_readfirstlane((int)(ray / p.rays_per_img));
    int r = __builtin_amdgcn_readfirstlane((int)(ray - (int64_t)n * p.rays_per_img));
    int s0 = 0;
    bool have = ray < ray_end;
    TapAddr t[3];
    TapBuf<C> buf;
    if (have) {
        float zl, jl;
        tile_depth(ray, 0, zl, jl);
        tile_taps(n, r, zl, jl, t);
        issue_taps<C>(uniform_ptr(p.geo_planes + n * p.geo_stride[0]), t, gl, buf);
    }
    float acc_t[NA], acc_g[NA];                           // sum_i w_i h_i of the units 16 mt + 4 g + r, over this lane's samples
#pragma unroll
    for (int i = 0; i < NA; ++i) { acc_t[i] = 0.f; acc_g[i] = 0.f; }
    float carry = 1.0f, wsum = 0.f, dsum = 0.f;

    while (have) {
        // successor tile (next_tile, written out: pinned)
        int s0n = s0 + 16, nn = n, rn = r;
        int64_t rayn = ray;
        if (s0n >= S) {
            s0n = 0; rayn = ray + NW; rn = r + NW;
            while (rn >= p.rays_per_img) { rn -= (int)p.rays_per_img; ++nn; }
        }
        const bool haven = rayn < ray_end;
        // the prefetches below are unconditional (a conditional definition of the loop-carried tap buffer costs a register copy per
        // value and iteration): past the last tile they re-read this one
        const int64_t rayp = haven ? rayn : ray;
        const int np = haven ? nn : n, rp = haven ? rn : r, s0p = haven ? s0n : s0;
        // --- matrix layout: depth of sample s0 + lane % 16 for the compositing; gather layout: depths of the next tile ---
        const int s = s0 + j;
        const bool live = s < S;
        const int sc = live ? s : S - 1;
        float z = p.z_lin[sc];
        float znext = (sc + 1 < S) ? p.z_lin[sc + 1] : 0.f;
        if (p.jitter) {
            const float* jit = p.jitter + ray * S;
            z = __fadd_rn(z, __fmul_rn(__fsub_rn(jit[sc], 0.5f), zstep));
            if (sc + 1 < S) znext = __fadd_rn(znext, __fmul_rn(__fsub_rn(jit[sc + 1], 0.5f), zstep));
        }
        const float noise = p.sigma_noise ? p.sigma_noise[ray * S + sc] : 0.f;
        float zln, jln;
        tile_depth(rayp, s0p, zln, jln);

        float fg[K::NF], ft[K::NF];
        f32x4 hg[K::MT1], ht[K::MT1];
        blend_taps<C>(buf, t, fg);
        to_matrix_lanes(fg);
        issue_taps<C>(uniform_ptr(p.tex_planes + n * p.tex_stride[0]), t, gl, buf);          // in flight during the geometry MLP
        hidden_branch<C, HID, SPLIT>(s_geo, fg, hg);

        // --- compositing weights (before the texture MLP: the geometry hidden vector dies here) ---
        float tot;
        const float w = composite_step<HID, true>(p, s_row, hg, r, noise, z, znext, live, sc + 1 < S, carry, tot);
        carry *= tot;
        wsum += w; dsum += w * z;
#pragma unroll        // accumulate_hidden, written out here and below: pinned
        for (int mt = 0; mt < K::MT1; ++mt)
#pragma unroll
            for (int rr = 0; rr < 4; ++rr) acc_g[mt * 4 + rr] += w * hg[mt][rr];

        blend_taps<C>(buf, t, ft);
        to_matrix_lanes(ft);
        tile_taps(np, rp, zln, jln, t);                                         // next tile's geometry taps: during the texture MLP
        issue_taps<C>(uniform_ptr(p.geo_planes + np * p.geo_stride[0]), t, gl, buf);
        hidden_branch<C, HID, SPLIT>(s_tex, ft, ht);
#pragma unroll
        for (int mt = 0; mt < K::MT1; ++mt)
#pragma unroll
            for (int rr = 0; rr < 4; ++rr) acc_t[mt * 4 + rr] += w * ht[mt][rr];

        if (s0n == 0) {
            // --- close the ray (close_ray, written out: pinned) ---
            wsum = row16_sum(wsum); dsum = row16_sum(dsum);
#pragma unroll
            for (int i = 0; i < NA; ++i) { acc_g[i] = row16_sum(acc_g[i]); acc_t[i] = row16_sum(acc_t[i]); }
            float o_t[2], o_g[2];
            heads_per_ray<C, HID, SPLIT>(s_tex, acc_t, wsum, o_t);
            heads_per_ray<C, HID, SPLIT>(s_geo, acc_g, wsum, o_g);
            {
                const float bg = p.white_back ? (1.0f - wsum) : 0.f;
                float* of = p.out_feat + (int64_t)n * nch * p.rays_per_img + r;
                const int idx = j + 16 * (g & 1);
                const float v = (g & 2) ? ((g & 1) ? o_g[1] : o_g[0]) : ((g & 1) ? o_t[1] : o_t[0]);
                if (g < 2) {
                    if (idx < p.feat_ch) of[(int64_t)idx * p.rays_per_img] = v + bg;
                } else {
                    if (idx >= 1 && idx <= p.seg_ch) of[(int64_t)(p.feat_ch + idx - 1) * p.rays_per_img] = v + bg;      // row 0 is sigma
                }
                if (lane == 0) {
                    if (p.out_depth) p.out_depth[ray] = dsum + ((p.max_depth != 0.f) ? (1.0f - wsum) * p.max_depth : 0.f);
                    if (p.out_wsum) p.out_wsum[ray] = wsum;
                }
            }
#pragma unroll
            for (int i = 0; i < NA; ++i) { acc_t[i] = 0.f; acc_g[i] = 0.f; }
            carry = 1.0f; wsum = 0.f; dsum = 0.f;
        }
        ray = rayn; n = nn; r = rn; s0 = s0n; have = haven;
    }
    if constexpr (SPLIT) __syncthreads();          // exclusive residency: nobody leaves while another wave of the workgroup still multiplies
}

// Where sample_voxel takes its points from: an [n, m, 3] array, or the extract_shapes.py lattice generated in registers.
struct PointsFromMemory {
    const float* pts;
    // `row`: global row (image * m + idx); `idx`: the row inside its image
    __device__ __forceinline__ void get(int64_t row, int64_t /*idx*/, float& x, float& y, float& z) const {
        x = pts[row * 3 + 0]; y = pts[row * 3 + 1]; z = pts[row * 3 + 2];
    }
};

// extract_shapes.py:74-96 + the 0.9 scale of :103, evaluated like the reference's fp32 tensor ops, one rounding each:
// i -> float, column 2 = i % N, column 1 = (i / N) % N, column 0 = ((i / N) / N) % N with *float* division (the
// reference does not floor: its y / x "indices" carry a fractional part), then (v * voxel_size + corner) * scale.
struct PointsFromLattice {
    ide3d_lattice lat;
    int64_t first;
    __device__ __forceinline__ void get(int64_t /*row*/, int64_t idx, float& x, float& y, float& z) const {
        const int64_t i = first + idx;
        const float fn = (float)lat.n, fi = (float)i;                       // int64 -> fp32, round to nearest even
        const float q = __fdiv_rn(fi, fn);
        const int64_t r2 = (i >> 32) == 0 ? (int64_t)((unsigned)i % (unsigned)lat.n) : i % lat.n;    // 32-bit remainder when it fits
        const float s2 = (float)r2, s1 = fmodf(q, fn), s0 = fmodf(__fdiv_rn(q, fn), fn);
        x = __fmul_rn(__fadd_rn(__fmul_rn(s0, lat.voxel_size), lat.corner[2]), lat.scale);
        y = __fmul_rn(__fadd_rn(__fmul_rn(s1, lat.voxel_size), lat.corner[1]), lat.scale);
        z = __fmul_rn(__fadd_rn(__fmul_rn(s2, lat.voxel_size), lat.corner[0]), lat.scale);
    }
};

template <class Src>
__global__ void lattice_points_kernel(Src src, int64_t count, float* __restrict__ out) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < count; i += (int64_t)gridDim.x * blockDim.x) {
        float x, y, z;
        src.get(i, i, x, y, z);
        out[i * 3 + 0] = x; out[i * 3 + 1] = y; out[i * 3 + 2] = z;
    }
}

// sample_voxel: gathers + MLPs for arbitrary points, rows of [feat | seg | sigma] (or sigma only).
template <int C, int HID, class Src, bool SPLIT>
__global__ void __launch_bounds__(64 * RmWaves<SPLIT>::value, 2)
sample_voxel_kernel(ide3d_render_params p, const Src src, int64_t m, float* __restrict__ out, int64_t tiles_per_block) {
    using K = RmCfg<C, HID>;
    constexpr int NW = RmWaves<SPLIT>::value;
    rm_claim_half_simd<SPLIT>();
    extern __shared__ __attribute__((aligned(16))) float lds[];
    constexpr int MB = MlpBytes<C, HID, SPLIT>::value;
    unsigned char* s_geo = reinterpret_cast<unsigned char*>(lds);
    unsigned char* s_tex = s_geo + MB;
    float* s_stage = reinterpret_cast<float*>(s_geo + 2 * MB);                 // [NW waves][16 samples][width] row staging
    stage_branch<C, HID, SPLIT>(s_geo, p.geo_w0, p.geo_b0, p.geo_w1, p.geo_b1, 1 + p.seg_ch);
    stage_branch<C, HID, SPLIT>(s_tex, p.tex_w0, p.tex_b0, p.tex_w1, p.tex_b1, p.feat_ch);
    __syncthreads();
    const int lane = lane_id(), wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int g = lane >> 4, j = lane & 15, gl = gather_block(lane);
    const int width = p.feat_ch + p.seg_ch + 1;
    const int sH = (int)p.tex_stride[2], sW = (int)p.tex_stride[3];
    float* stage = s_stage + wid * 16 * width;
    const int64_t rows = (int64_t)p.n * m;
    const int64_t ntiles = cdiv64(rows, 16);
    const int blk = xcd_remap(blockIdx.x, gridDim.x);
    const int64_t tile_begin = (int64_t)blk * tiles_per_block;
    int64_t tile_end = tile_begin + tiles_per_block;
    if (tile_end > ntiles) tile_end = ntiles;

    // Software pipeline over this wave's tiles (same scheme as render_rays_kernel): the texture taps of a tile fly during its geometry
    // MLP, the geometry taps of the next tile during its texture MLP.  Wave-uniform per tile: the
    // image n0 of its first row (scalar plane bases); a lane whose row lies `dn` images further on (a tile straddling images: m not a
    // multiple of 16) adds dn image strides to its byte offsets.
    int64_t tile = tile_begin + wid;
    int n0 = 0;
    int64_t img_end = m;                                   // first row of image n0 + 1
    auto advance_image = [&](int64_t row0) { while (row0 >= img_end && n0 + 1 < p.n) { ++n0; img_end += m; } };
    // the point of row row0 + lane / 4 (gather layout) and how many images past n0 it lies
    auto tile_point = [&](int64_t row0, float& wx, float& wy, float& wz, int& dn) {
        const int64_t rl = row0 + gather_sample(lane);
        const int64_t rc = rl < rows ? rl : rows - 1;
        dn = 0;
        int64_t e = img_end;
        while (rc >= e) { ++dn; e += m; }
        src.get(rc, rc - (e - m), wx, wy, wz);
    };
    auto tile_taps = [&](float wx, float wy, float wz, TapAddr (&t)[3]) { triplane_tap_addrs(wx, wy, wz, p.W, p.H, sH, sW, t); };
    const unsigned geo_img_b = (unsigned)p.geo_stride[0] * 4u, tex_img_b = (unsigned)p.tex_stride[0] * 4u;

    bool have = tile < tile_end;
    TapAddr t[3];
    TapBuf<C> buf;
    int dn = 0;
    if (have) {
        float wx, wy, wz;
        advance_image(tile * 16);
        tile_point(tile * 16, wx, wy, wz, dn);
        tile_taps(wx, wy, wz, t);
        issue_taps<C>(uniform_ptr(p.geo_planes + n0 * p.geo_stride[0]), t, gl, buf, (unsigned)dn * geo_img_b);
    }
    while (have) {
        const int64_t row0 = tile * 16;
        const int64_t tilen = tile + NW;
        const bool haven = tilen < tile_end;
        const int n0c = n0, dnc = dn;
        // next tile's points first (PointsFromMemory: three small loads, ahead of the taps that fly across the MLPs).  The prefetch is
        // unconditional (a conditional definition of the loop-carried tap buffer costs a register copy per value and iteration): past
        // the last tile it re-reads this one.
        const int64_t tilep = haven ? tilen : tile;
        float wxn, wyn, wzn;
        advance_image(tilep * 16);
        tile_point(tilep * 16, wxn, wyn, wzn, dn);
        float fg[K::NF];
        blend_taps<C>(buf, t, fg);
        to_matrix_lanes(fg);
        issue_taps<C>(uniform_ptr(p.tex_planes + n0c * p.tex_stride[0]), t, gl, buf, (unsigned)dnc * tex_img_b);
        f32x4 og[2];
        mlp_branch<C, HID, SPLIT>(s_geo, fg, og);
        float ft[K::NF];
        blend_taps<C>(buf, t, ft);
        to_matrix_lanes(ft);
        tile_taps(wxn, wyn, wzn, t);
        issue_taps<C>(uniform_ptr(p.geo_planes + n0 * p.geo_stride[0]), t, gl, buf, (unsigned)dn * geo_img_b);
        f32x4 ot[2];
        mlp_branch<C, HID, SPLIT>(s_tex, ft, ot);
        // stage the 16 x width row block, then write it out contiguously
#pragma unroll
        for (int mt = 0; mt < 2; ++mt)
#pragma unroll
            for (int rr = 0; rr < 4; ++rr) {
                const int idx = 16 * mt + 4 * g + rr;
                if (idx < p.feat_ch) stage[j * width + idx] = ot[mt][rr];
                if (idx >= 1 && idx <= p.seg_ch) stage[j * width + p.feat_ch + idx - 1] = og[mt][rr];
                if (idx == 0) stage[j * width + width - 1] = og[mt][rr];
            }
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        const int64_t live_rows = (rows - row0 < 16) ? rows - row0 : 16;
        const int64_t nel = live_rows * width;
        float* dst = out + row0 * width;
        for (int i = lane; i < nel; i += kWave) dst[i] = stage[i];
        __builtin_amdgcn_wave_barrier();
        tile = tilen; have = haven;
    }
    if constexpr (SPLIT) __syncthreads();          // exclusive residency (see render_rays_kernel)
}

// Densities only (extract_shapes.py's cube, sample_voxel(sigma_only)): one gather, the hidden layer, row 0 of the second layer.  The
// kernel is bound by its vector instructions (90 % VALU-busy before this form), a third of them the point and the tap addresses of
// the tile — which every lane of a quad computes alike.  So the points and taps are computed for 64 rows at once, lane = row (the
// `super tile`), and each of its four 16-row tiles fetches its own from the lanes that hold them (ds_bpermute: 25 values per tile
// instead of ~300 vector instructions).  Same software pipeline as above: the taps of the next tile fly during the MLP of this one.
template <int C, int HID, class Src, bool SPLIT>
__global__ void __launch_bounds__(64 * RmWaves<SPLIT>::value, 2)
density_kernel(ide3d_render_params p, const Src src, int64_t m, float* __restrict__ out_sigma, int64_t supers_per_block) {
    using K = RmCfg<C, HID>;
    constexpr int NW = RmWaves<SPLIT>::value;
    rm_claim_half_simd<SPLIT>();
    extern __shared__ __attribute__((aligned(16))) float lds[];
    unsigned char* s_geo = reinterpret_cast<unsigned char*>(lds);
    float* const s_row = reinterpret_cast<float*>(s_geo + MlpBytes<C, HID, SPLIT>::value);     // row 0 of geo_w1 + its bias
    stage_branch<C, HID, SPLIT>(s_geo, p.geo_w0, p.geo_b0, p.geo_w1, p.geo_b1, 1 + p.seg_ch);
    for (int i = threadIdx.x; i <= HID; i += blockDim.x) s_row[i] = (i < HID) ? p.geo_w1[i] : p.geo_b1[0];
    __syncthreads();
    const int lane = lane_id(), wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int g = lane >> 4, j = lane & 15, gl = gather_block(lane);
    const int sH = (int)p.geo_stride[2], sW = (int)p.geo_stride[3];
    const int64_t rows = (int64_t)p.n * m;
    const int64_t nsuper = cdiv64(rows, 64);
    const int blk = xcd_remap(blockIdx.x, gridDim.x);
    const int64_t super_begin = (int64_t)blk * supers_per_block;
    int64_t super_end = super_begin + supers_per_block;
    if (super_end > nsuper) super_end = nsuper;
    const unsigned geo_img_b = (unsigned)p.geo_stride[0] * 4u;

    int n0 = 0;                                            // image of the first row of the super tile whose taps `tl` holds
    int64_t img_end = m;
    // taps of row 64 st + lane, and how many images past n0 that row lies (a super tile that straddles images)
    auto super_taps = [&](int64_t st, TapAddr (&tl)[3], int& dnl) {
        const int64_t row0 = st * 64;
        while (row0 >= img_end && n0 + 1 < p.n) { ++n0; img_end += m; }
        const int64_t rl = row0 + lane;
        const int64_t rc = rl < rows ? rl : rows - 1;
        dnl = 0;
        int64_t e = img_end;
        while (rc >= e) { ++dnl; e += m; }
        float wx, wy, wz;
        src.get(rc, rc - (e - m), wx, wy, wz);
        triplane_tap_addrs(wx, wy, wz, p.W, p.H, sH, sW, tl);
    };
    // tile k of the super tile, gather layout: lane 4 j + g takes the taps of row 16 k + j from lane 16 k + j
    auto tile_taps = [&](const TapAddr (&tl)[3], int dnl, int k, TapAddr (&t)[3], int& dn) {
        const int src_b = (16 * k + gather_sample(lane)) << 2;
#pragma unroll
        for (int pl = 0; pl < 3; ++pl) {
            t[pl].o00 = __builtin_amdgcn_ds_bpermute(src_b, tl[pl].o00); t[pl].o01 = __builtin_amdgcn_ds_bpermute(src_b, tl[pl].o01);
            t[pl].o10 = __builtin_amdgcn_ds_bpermute(src_b, tl[pl].o10); t[pl].o11 = __builtin_amdgcn_ds_bpermute(src_b, tl[pl].o11);
            t[pl].w00 = __int_as_float(__builtin_amdgcn_ds_bpermute(src_b, __float_as_int(tl[pl].w00)));
            t[pl].w01 = __int_as_float(__builtin_amdgcn_ds_bpermute(src_b, __float_as_int(tl[pl].w01)));
            t[pl].w10 = __int_as_float(__builtin_amdgcn_ds_bpermute(src_b, __float_as_int(tl[pl].w10)));
            t[pl].w11 = __int_as_float(__builtin_amdgcn_ds_bpermute(src_b, __float_as_int(tl[pl].w11)));
        }
        dn = __builtin_amdgcn_ds_bpermute(src_b, dnl);
    };

    int64_t st = super_begin + wid;
    if (st < super_end) {
    TapAddr tl[3], t[3];
    TapBuf<C> buf;
    int dnl, dn;
    super_taps(st, tl, dnl);
    tile_taps(tl, dnl, 0, t, dn);
    issue_taps<C>(uniform_ptr(p.geo_planes + n0 * p.geo_stride[0]), t, gl, buf, (unsigned)dn * geo_img_b);
    while (st < super_end) {
        const int64_t stn = st + NW;
        const int64_t stp = stn < super_end ? stn : st;              // the prefetch past the last super tile re-reads this one
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int64_t row = st * 64 + 16 * k + j;
            float fg[K::NF];
            blend_taps<C>(buf, t, fg);
            to_matrix_lanes(fg);
            if (k == 3) super_taps(stp, tl, dnl);
            tile_taps(tl, dnl, (k + 1) & 3, t, dn);
            issue_taps<C>(uniform_ptr(p.geo_planes + n0 * p.geo_stride[0]), t, gl, buf, (unsigned)dn * geo_img_b);
            float sig;
            if constexpr (SPLIT) sig = mlp_sigma_split<C, HID>(s_geo, s_row, fg);
            else sig = mlp_sigma<C, HID>(reinterpret_cast<const float*>(s_geo), s_row, fg);
            if (g == 0 && row < rows) out_sigma[row] = sig;
        }
        st = stn;
    }
    }
    if constexpr (SPLIT) __syncthreads();          // exclusive residency (see render_rays_kernel)
}

// The launch of every persistent kernel of this file: 8 waves per CU either way (RmWaves), each workgroup a contiguous range of `units` (rays,
// 16-row tiles, 64-row super tiles) whose length goes to the kernel as its last argument, after `args`; exclusive residency for the SPLIT forms.
template <bool SPLIT, class Kern, class... Args>
static int launch_persistent(Kern kern, const char* what, int64_t units, size_t lds_bytes, hipStream_t st, const Args&... args) {
    constexpr int NW = RmWaves<SPLIT>::value;
    int64_t nblk = kNumCU * 8 / NW;
    int64_t per_block = cdiv64(cdiv64(units, nblk), NW) * NW;
    if (per_block < NW) per_block = NW;
    nblk = cdiv64(units, per_block);
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes);
    if constexpr (SPLIT) IDE3D_EXCL_LAUNCH(kern, dim3((unsigned)nblk), 64 * NW, lds_bytes, st, args..., per_block);
    else hipLaunchKernelGGL(kern, dim3((unsigned)nblk), dim3(64 * NW), lds_bytes, st, args..., per_block);
    IDE3D_CHECK_LAUNCH(what);
    return IDE3D_OK;
}

template <int C, int HID, bool SPLIT, class Src>
static int launch_voxel(const ide3d_render_params& p, const Src& src, int64_t m, float* out, float* out_sigma,
                        int sigma_only, hipStream_t st) {
    // a lane whose row lies in a later image than the first row of its (super) tile adds whole image strides to its 32-bit byte
    // offsets: at most rows_per_tile - 1 images when m = 1
    const int64_t rows = (int64_t)p.n * m, rows_per_tile = sigma_only ? 64 : 16;
    {
        const int64_t max_dn = (p.n > 1) ? ((rows_per_tile - 1) / (m > 0 ? m : 1) + 1 < p.n - 1 ? (rows_per_tile - 1) / (m > 0 ? m : 1) + 1 : p.n - 1) : 0;
        const int64_t img = p.geo_stride[0] > p.tex_stride[0] ? p.geo_stride[0] : p.tex_stride[0];
        if ((max_dn * img + img) * 4 >= 0xffffffffLL) { set_error("sample_voxel: too few points per image for planes this large"); return IDE3D_ENOKERNEL; }
    }
    if (sigma_only)
        return launch_persistent<SPLIT>(density_kernel<C, HID, Src, SPLIT>, "sample_voxel (densities)", cdiv64(rows, 64),
                                        (size_t)MlpBytes<C, HID, SPLIT>::value + (size_t)(HID + 4) * sizeof(float), st, p, src, m, out_sigma);
    const size_t stage_bytes = (size_t)RmWaves<SPLIT>::value * 16 * (p.feat_ch + p.seg_ch + 1) * sizeof(float);
    return launch_persistent<SPLIT>(sample_voxel_kernel<C, HID, Src, SPLIT>, "sample_voxel", cdiv64(rows, 16),
                                    (size_t)2 * MlpBytes<C, HID, SPLIT>::value + stage_bytes, st, p, src, m, out);
}

// ---- the hierarchical (importance) pass: first-pass weights, depth merge, merged march ---------------------------
// TriplaneRenderer.forward(hierarchical=True) as four launches: render_ray_weights_kernel -> ide3d_sample_pdf (sample_pdf.hip) ->
// merge_depths_kernel -> render_rays_merged_kernel.  Per sample nothing but depths and weights is ever written: the first pass keeps the
// geometry branch only (gather, hidden layer, sigma row, transmittance scan), the merged march is render_rays_kernel's walk over the 2 S
// depth-ordered samples of a ray, each rebuilt from where it came from (`src`): a coarse sample from z_lin / jitter exactly as the first pass
// placed it, a fine one as origin + direction * depth.
// Both marchers prefetch two tiles deep: a tile's taps hang on its depths (first pass) or on what its `src` entries select (merged march:
// a load that depends on a load), so those small loads are issued one tile before the taps they feed, and a tile's `src` one tile before that.


// First pass: the compositing weights of the S linear (jittered) samples of every ray, their depths, and the pdf that ide3d_sample_pdf draws
// the fine depths from (bins = depth mid-points, weights = inner samples' weights + 1e-5), any of them optional.
template <int C, int HID, bool SPLIT>
__global__ void __launch_bounds__(64 * RmWaves<SPLIT>::value, 2)
render_ray_weights_kernel(ide3d_render_params p, float* __restrict__ out_w, float* __restrict__ out_z, float* __restrict__ out_bins,
                          float* __restrict__ out_pw, int64_t rays_per_block) {
    using K = RmCfg<C, HID>;
    constexpr int NW = RmWaves<SPLIT>::value;
    rm_claim_half_simd<SPLIT>();
    const MarchWave m = march_prologue<C, HID, SPLIT, false>(p, rays_per_block);
    const int lane = m.lane, g = m.g, j = m.j, gl = m.gl;
    const int64_t ray_end = m.ray_end;
    const int S = p.steps;
    const int sH = (int)p.geo_stride[2], sW = (int)p.geo_stride[3];
    const float zstep = p.z_lin[1] - p.z_lin[0];              // S >= 3 (host)

    auto tile_depth = [&](int64_t ray, int s0, float& zl, float& jl) {
        const int sl = min(s0 + gather_sample(lane), S - 1);
        zl = p.z_lin[sl];
        jl = p.jitter ? p.jitter[ray * S + sl] : 0.5f;
    };
    auto tile_taps = [&](int n, int r, float zl, float jl, TapAddr (&t)[3]) {
        float wx, wy, wz;
        ray_world_point(p, n, r, zl, jl, zstep, wx, wy, wz);
        triplane_tap_addrs(wx, wy, wz, p.W, p.H, sH, sW, t);
    };

    int64_t ray = m.ray;
    int n = m.n, r = m.r, s0 = 0;
    bool have = ray < ray_end;
    TapAddr t[3];
    TapBuf<C> buf;
    float zl1 = 0.f, jl1 = 0.5f;                            // depths of the tile after this one (gather layout), loaded one tile ahead
    if (have) {
        float zl, jl;
        tile_depth(ray, 0, zl, jl);
        tile_taps(n, r, zl, jl, t);
        issue_taps<C>(uniform_ptr(p.geo_planes + n * p.geo_stride[0]), t, gl, buf);
        int64_t ray1 = ray; int n1 = n, r1 = r, s1 = s0;
        next_tile<NW>(S, p.rays_per_img, ray1, n1, r1, s1);
        if (ray1 < ray_end) tile_depth(ray1, s1, zl1, jl1); else tile_depth(ray, s0, zl1, jl1);
    }
    float carry = 1.0f;

    while (have) {
        // the next tile and the one after it; past the last tile the prefetches re-read the last one (see render_rays_kernel)
        int64_t rayn = ray; int nn = n, rn = r, s0n = s0;
        next_tile<NW>(S, p.rays_per_img, rayn, nn, rn, s0n);
        const bool haven = rayn < ray_end;
        const int64_t rayp = haven ? rayn : ray;
        const int np = haven ? nn : n, rp = haven ? rn : r, s0p = haven ? s0n : s0;
        int64_t ray2 = rayn; int n2 = nn, r2 = rn, s2 = s0n;
        next_tile<NW>(S, p.rays_per_img, ray2, n2, r2, s2);
        const bool have2 = haven && ray2 < ray_end;
        const int64_t rayq = have2 ? ray2 : rayp;
        const int s0q = have2 ? s2 : s0p;

        // matrix layout: depth of sample s0 + lane % 16, the one after it, its density noise
        const int s = s0 + j;
        const bool live = s < S;
        const int sc = live ? s : S - 1;
        const float z = ray_sample_depth(p, ray, sc, zstep);
        const float znext = (sc + 1 < S) ? ray_sample_depth(p, ray, sc + 1, zstep) : 0.f;
        const float noise = p.sigma_noise ? p.sigma_noise[ray * S + sc] : 0.f;

        float fg[K::NF];
        f32x4 hg[K::MT1];
        blend_taps<C>(buf, t, fg);
        to_matrix_lanes(fg);
        tile_taps(np, rp, zl1, jl1, t);                                          // next tile's taps: in flight during this tile's MLP
        issue_taps<C>(uniform_ptr(p.geo_planes + np * p.geo_stride[0]), t, gl, buf);
        tile_depth(rayq, s0q, zl1, jl1);
        hidden_branch<C, HID, SPLIT>(m.s_geo, fg, hg);

        float tot;
        const float w = composite_step<HID, true>(p, m.s_row, hg, r, noise, z, znext, live, sc + 1 < S, carry, tot);
        carry = (s0n == 0) ? 1.0f : carry * tot;

        // the four lanes of a sample hold the same values: one output each
        if (live) {
            if (g == 0 && out_w) out_w[ray * S + s] = w;
            if (g == 1 && out_z) out_z[ray * S + s] = z;
            if (g == 2 && out_bins && s + 1 < S) out_bins[ray * (S - 1) + s] = __fmul_rn(0.5f, __fadd_rn(z, znext));
            if (g == 3 && out_pw && s >= 1 && s + 1 < S) out_pw[ray * (S - 2) + s - 1] = __fadd_rn(w, 1e-5f);
        }
        ray = rayn; n = nn; r = rn; s0 = s0n; have = haven;
    }
    if constexpr (SPLIT) __syncthreads();          // exclusive residency (see render_rays_kernel)
}

// Monotone integer image of a depth: a < b as floats <=> key(a) < key(b) as unsigned, -0 == +0, every NaN above +inf.  With the index as
// the second key the order is total for any input bits.
__device__ __forceinline__ unsigned depth_key(float v) {
    unsigned b = __float_as_uint(v);
    if ((b & 0x7fffffffu) > 0x7f800000u) return 0xffffffffu;
    if (b == 0x80000000u) b = 0u;
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}

constexpr int kMergeWaves = 4;             // rays per workgroup and step
constexpr int kMergeMaxT = 2 * kMergedMaxSteps;           // merged samples per ray: 4 * 2048 keys = 32 KB of LDS

// Stable ascending order of [z_fine | z_coarse] per ray (torch.sort(torch.cat([z_fine, z_coarse]), stable=True)): one wave per ray, the T
// keys in LDS, the rank of an element = how many precede it in (key, index) order, counted by every lane for its elements from broadcast
// reads.  T^2 comparisons: T <= 192 at the workload's size, ~25 us for 16384 rays.  The ranks of a row are a permutation of 0 .. T-1
// whatever the data, so every element of z_all / src is written exactly once and nothing outside the row is.
__global__ void __launch_bounds__(kMergeWaves * kWave)
merge_depths_kernel(const float* __restrict__ z_fine, const float* __restrict__ z_coarse, int64_t rays, int sf, int sc,
                    float* __restrict__ z_all, int* __restrict__ src) {
    extern __shared__ unsigned s_keys[];                   // [kMergeWaves][T]
    const int lane = lane_id(), wid = threadIdx.x / kWave;
    const int T = sf + sc;
    unsigned* keys = s_keys + (size_t)wid * T;
    for (int64_t base = (int64_t)blockIdx.x * kMergeWaves; base < rays; base += (int64_t)gridDim.x * kMergeWaves) {
        const int64_t ray = base + wid;
        const bool live = ray < rays;
        if (live)
            for (int i = lane; i < T; i += kWave) keys[i] = depth_key(i < sf ? z_fine[ray * sf + i] : z_coarse[ray * sc + (i - sf)]);
        __syncthreads();
        if (live) {
            for (int i = lane; i < T; i += kWave) {
                const unsigned ki = keys[i];
                int rank = 0;
                for (int k = 0; k < T; ++k) {
                    const unsigned kk = keys[k];
                    rank += (kk < ki || (kk == ki && k < i)) ? 1 : 0;
                }
                const float v = i < sf ? z_fine[ray * sf + i] : z_coarse[ray * sc + (i - sf)];
                z_all[ray * T + rank] = v;
                src[ray * T + rank] = i;
            }
        }
        __syncthreads();                                   // the keys are rewritten by the next ray of this wave
    }
}

// Merged march: render_rays_kernel's walk over the T = 2 S samples of a ray in z_all order.  Sample s of a ray is entry src[ray, s] of the
// concatenation [fine | coarse]: a coarse one is rebuilt by ray_world_point from z_lin / jitter (the point the first pass weighed), a fine one
// is origin + dir_world * z_fine.  No density noise; delta from neighbouring z_all.
template <int C, int HID, bool SPLIT>
__global__ void __launch_bounds__(64 * RmWaves<SPLIT>::value, 2)
render_rays_merged_kernel(ide3d_render_params p, const float* __restrict__ z_all, const int* __restrict__ src,
                          const float* __restrict__ z_fine, int64_t rays_per_block) {
    using K = RmCfg<C, HID>;
    constexpr int NW = RmWaves<SPLIT>::value;
    constexpr int NA = HID / 4;                            // hidden units per lane and branch
    rm_claim_half_simd<SPLIT>();
    const MarchWave m = march_prologue<C, HID, SPLIT, true>(p, rays_per_block);
    const int lane = m.lane, j = m.j, gl = m.gl;
    const int64_t ray_end = m.ray_end;
    const int S = p.steps, T = 2 * S;
    const int sH = (int)p.tex_stride[2], sW = (int)p.tex_stride[3];   // host guarantees tex / geo share the layout
    const float zstep = p.z_lin[1] - p.z_lin[0];             // S >= 3 (host)

    // src of merged sample s0 + lane / 4 of `ray` (gather layout)
    auto tile_src = [&](int64_t ray, int s0) { return src[ray * T + min(s0 + gather_sample(lane), T - 1)]; };
    // what that entry selects: a coarse sample's linear depth and jitter draw, or a fine sample's depth (in `a`).  The entry is clamped
    // into [0, T) first, so no value of it reads outside z_lin / jitter / z_fine.
    auto tile_sample = [&](int64_t ray, int sv, float& zl, float& a) {
        sv = min(max(sv, 0), T - 1);
        const bool fine = sv < S;
        const int idx = fine ? sv : sv - S;
        zl = p.z_lin[idx];
        const float* ap = fine ? z_fine : p.jitter;
        a = ap ? ap[ray * S + idx] : 0.5f;
    };
    auto tile_taps = [&](int n, int r, int sv, float zl, float a, TapAddr (&t)[3]) {
        float wx, wy, wz;
        ray_world_point(p, n, r, zl, a, zstep, wx, wy, wz);
        if (min(max(sv, 0), T - 1) < S) {
            // origin + dir_world * z, the multiply and the add rounded separately like the tensor expression
            const float dx = p.rays_d_cam[r * 3 + 0], dy = p.rays_d_cam[r * 3 + 1], dz = p.rays_d_cam[r * 3 + 2];
            const float* M = p.cam2world + n * 16;
            const float ux = fmaf(M[0], dx, fmaf(M[1], dy, __fmul_rn(M[2], dz)));
            const float uy = fmaf(M[4], dx, fmaf(M[5], dy, __fmul_rn(M[6], dz)));
            const float uz = fmaf(M[8], dx, fmaf(M[9], dy, __fmul_rn(M[10], dz)));
            wx = __fadd_rn(M[3], __fmul_rn(ux, a));
            wy = __fadd_rn(M[7], __fmul_rn(uy, a));
            wz = __fadd_rn(M[11], __fmul_rn(uz, a));
        }
        triplane_tap_addrs(wx, wy, wz, p.W, p.H, sH, sW, t);
    };

    int64_t ray = m.ray;
    int n = m.n, r = m.r, s0 = 0;
    bool have = ray < ray_end;
    TapAddr t[3];
    TapBuf<C> buf;
    int src1 = 0;                                          // src of the tile after this one (gather layout), loaded one tile ahead
    if (have) {
        const int sv = tile_src(ray, 0);
        float zl, a;
        tile_sample(ray, sv, zl, a);
        tile_taps(n, r, sv, zl, a, t);
        issue_taps<C>(uniform_ptr(p.geo_planes + n * p.geo_stride[0]), t, gl, buf);
        int64_t ray1 = ray; int n1 = n, r1 = r, s1 = s0;
        next_tile<NW>(T, p.rays_per_img, ray1, n1, r1, s1);
        src1 = (ray1 < ray_end) ? tile_src(ray1, s1) : sv;
    }
    float acc_t[NA], acc_g[NA];                           // sum_i w_i h_i of the units 16 mt + 4 g + r, over this lane's samples
#pragma unroll
    for (int i = 0; i < NA; ++i) { acc_t[i] = 0.f; acc_g[i] = 0.f; }
    float carry = 1.0f, wsum = 0.f, dsum = 0.f;

    while (have) {
        // the next tile and the one after it; past the last tile the prefetches re-read the last one (see render_rays_kernel)
        int64_t rayn = ray; int nn = n, rn = r, s0n = s0;
        next_tile<NW>(T, p.rays_per_img, rayn, nn, rn, s0n);
        const bool haven = rayn < ray_end;
        const int64_t rayp = haven ? rayn : ray;
        const int np = haven ? nn : n, rp = haven ? rn : r;
        int64_t ray2 = rayn; int n2 = nn, r2 = rn, s2 = s0n;
        next_tile<NW>(T, p.rays_per_img, ray2, n2, r2, s2);
        const bool have2 = haven && ray2 < ray_end;
        // --- matrix layout: depth of sample s0 + lane % 16 and of the one after it; gather layout: the next tile's samples, the src of the one after ---
        const int s = s0 + j;
        const bool live = s < T;
        const int sc = live ? s : T - 1;
        const float z = z_all[ray * T + sc];
        const float znext = (sc + 1 < T) ? z_all[ray * T + sc + 1] : 0.f;
        float zln, an;
        tile_sample(rayp, src1, zln, an);
        const int svn = src1;
        if (have2) src1 = tile_src(ray2, s2);

        float fg[K::NF], ft[K::NF];
        f32x4 hg[K::MT1], ht[K::MT1];
        blend_taps<C>(buf, t, fg);
        to_matrix_lanes(fg);
        issue_taps<C>(uniform_ptr(p.tex_planes + n * p.tex_stride[0]), t, gl, buf);          // in flight during the geometry MLP
        hidden_branch<C, HID, SPLIT>(m.s_geo, fg, hg);

        // --- compositing weights (before the texture MLP: the geometry hidden vector dies here) ---
        float tot;
        const float w = composite_step<HID, false>(p, m.s_row, hg, r, 0.f, z, znext, live, sc + 1 < T, carry, tot);
        carry *= tot;
        wsum += w; dsum += w * z;
        accumulate_hidden(acc_g, w, hg);

        blend_taps<C>(buf, t, ft);
        to_matrix_lanes(ft);
        tile_taps(np, rp, svn, zln, an, t);                                     // next tile's geometry taps: during the texture MLP
        issue_taps<C>(uniform_ptr(p.geo_planes + np * p.geo_stride[0]), t, gl, buf);
        hidden_branch<C, HID, SPLIT>(m.s_tex, ft, ht);
        accumulate_hidden(acc_t, w, ht);

        if (s0n == 0) close_ray<C, HID, SPLIT>(p, m, ray, n, r, acc_t, acc_g, carry, wsum, dsum);
        ray = rayn; n = nn; r = rn; s0 = s0n; have = haven;
    }
    if constexpr (SPLIT) __syncthreads();          // exclusive residency (see render_rays_kernel)
}

}  // namespace ide3d

// The decoder MLPs follow the arithmetic selected for the convolutions (ide3d_set_conv_arithmetic, modconv.hip): exact fp32 products on
// the fp32 matrix path by default, bf16x6 (fp32-grade) with any of the split arithmetics.
static bool mlp_split_selected() { return ide3d_get_conv_arithmetic() != 1; }

extern "C" int ide3d_render_rays(const ide3d_render_params* pp, void* stream) {
    using namespace ide3d;
    IDE3D_CHECK_ARG(pp != nullptr, "render_rays: null params");
    const ide3d_render_params& p = *pp;
    int rc = check_render_params(p, "render_rays", kRaysAndOutput);
    if (!rc) rc = check_march_declines(p, "render_rays");
    if (rc) return rc;
    return with_form(p, mlp_split_selected(), "render_rays", [&](auto f) {
        return launch_persistent<f.SPLIT>(render_rays_kernel<f.C, f.HID, f.SPLIT>, "render_rays", (int64_t)p.n * p.rays_per_img,
                                          kMarchLdsBytes<f.C, f.HID, f.SPLIT, true>, (hipStream_t)stream, p);
    });
}

extern "C" int ide3d_sample_voxel(const ide3d_render_params* pp, const float* pts, int64_t m,
                                  float* out, float* out_sigma, int sigma_only, void* stream) {
    using namespace ide3d;
    IDE3D_CHECK_ARG(pp != nullptr && pts != nullptr, "sample_voxel: null params");
    const ide3d_render_params& p = *pp;
    int rc = check_render_params(p, "sample_voxel", kNoRays);
    if (rc) return rc;
    IDE3D_CHECK_ARG(m >= 0, "sample_voxel: bad point count");
    IDE3D_CHECK_ARG(sigma_only ? out_sigma != nullptr : out != nullptr, "sample_voxel: null output");
    if (m == 0) return IDE3D_OK;
    if (!planes_fast(p)) { set_error("sample_voxel: tri-planes must be channels_last, 16-byte aligned"); return IDE3D_ENOKERNEL; }
    const PointsFromMemory src{pts};
    return with_form(p, mlp_split_selected(), "sample_voxel", [&](auto f) {
        return launch_voxel<f.C, f.HID, f.SPLIT>(p, src, m, out, out_sigma, sigma_only, (hipStream_t)stream);
    });
}

static int check_lattice(const ide3d_lattice* lat, int64_t first, int64_t count, const char* what) {
    using namespace ide3d;
    IDE3D_CHECK_ARG(lat != nullptr && lat->n >= 2 && lat->n <= 2048, "%s: lattice resolution must be in [2, 2048]", what);
    const int64_t total = (int64_t)lat->n * lat->n * lat->n;
    IDE3D_CHECK_ARG(first >= 0 && count >= 0 && first + count <= total, "%s: point range outside the lattice", what);
    return IDE3D_OK;
}

extern "C" int ide3d_lattice_points(const ide3d_lattice* lat, int64_t first, int64_t count, float* pts, void* stream) {
    using namespace ide3d;
    int rc = check_lattice(lat, first, count, "lattice_points");
    if (rc) return rc;
    IDE3D_CHECK_ARG(pts != nullptr || count == 0, "lattice_points: null output");
    if (count == 0) return IDE3D_OK;
    const PointsFromLattice src{*lat, first};
    hipLaunchKernelGGL(lattice_points_kernel<PointsFromLattice>, dim3(stream_grid(count, 256)), dim3(256), 0, (hipStream_t)stream,
                       src, count, pts);
    IDE3D_CHECK_LAUNCH("lattice_points");
    return IDE3D_OK;
}

extern "C" int ide3d_density_lattice(const ide3d_render_params* pp, const ide3d_lattice* lat, int64_t first, int64_t count,
                                     float* out_sigma, void* stream) {
    using namespace ide3d;
    IDE3D_CHECK_ARG(pp != nullptr, "density_lattice: null params");
    const ide3d_render_params& p = *pp;
    int rc = check_render_params(p, "density_lattice", kNoRays);
    if (rc) return rc;
    rc = check_lattice(lat, first, count, "density_lattice");
    if (rc) return rc;
    IDE3D_CHECK_ARG(out_sigma != nullptr || count == 0, "density_lattice: null output");
    if (count == 0) return IDE3D_OK;
    if (!planes_fast(p)) { set_error("density_lattice: tri-planes must be channels_last, 16-byte aligned"); return IDE3D_ENOKERNEL; }
    const PointsFromLattice src{*lat, first};
    return with_form(p, mlp_split_selected(), "density_lattice", [&](auto f) {
        return launch_voxel<f.C, f.HID, f.SPLIT>(p, src, count, nullptr, out_sigma, 1, (hipStream_t)stream);
    });
}

// What the two marchers of the hierarchical pass check alike: ide3d_render_rays' rules without its outputs, then its declines plus the step
// counts the pass cannot take (an inner pdf needs 3 samples; ide3d_merge_depths holds 2 * steps keys per ray in LDS).
static int check_hierarchical(const ide3d_render_params& p, const char* who) {
    using namespace ide3d;
    int rc = check_render_params(p, who, kRays);
    if (!rc) rc = check_hierarchical_steps(p, who);
    return rc ? rc : check_march_declines(p, who);
}

extern "C" int ide3d_render_ray_weights(const ide3d_render_params* pp, float* weights, float* z_vals, float* pdf_bins, float* pdf_weights,
                                        void* stream) {
    using namespace ide3d;
    IDE3D_CHECK_ARG(pp != nullptr, "render_ray_weights: null params");
    const ide3d_render_params& p = *pp;
    int rc = check_hierarchical(p, "render_ray_weights");
    if (rc) return rc;
    return with_form(p, mlp_split_selected(), "render_ray_weights", [&](auto f) {
        return launch_persistent<f.SPLIT>(render_ray_weights_kernel<f.C, f.HID, f.SPLIT>, "render_ray_weights", (int64_t)p.n * p.rays_per_img,
                                          kMarchLdsBytes<f.C, f.HID, f.SPLIT, false>, (hipStream_t)stream, p, weights, z_vals, pdf_bins, pdf_weights);
    });
}

extern "C" int ide3d_merge_depths(const float* z_fine, const float* z_coarse, int64_t rays, int32_t steps_fine, int32_t steps_coarse,
                                  float* z_all, int32_t* src, void* stream) {
    using namespace ide3d;
    IDE3D_CHECK_ARG(rays >= 0 && steps_fine >= 0 && steps_coarse >= 0 && (int64_t)steps_fine + steps_coarse >= 1 &&
                    (int64_t)steps_fine + steps_coarse <= kMergeMaxT, "merge_depths: bad shape (1 <= steps_fine + steps_coarse <= %d)", kMergeMaxT);
    IDE3D_CHECK_ARG(z_all && src && (z_fine || steps_fine == 0) && (z_coarse || steps_coarse == 0), "merge_depths: null pointer");
    if (rays == 0) return IDE3D_OK;
    const int T = steps_fine + steps_coarse;
    hipLaunchKernelGGL(merge_depths_kernel, dim3(stream_grid(rays, kMergeWaves)), dim3(kMergeWaves * kWave), (size_t)kMergeWaves * T * sizeof(unsigned),
                       (hipStream_t)stream, z_fine, z_coarse, rays, (int)steps_fine, (int)steps_coarse, z_all, src);
    IDE3D_CHECK_LAUNCH("merge_depths");
    return IDE3D_OK;
}

extern "C" int ide3d_render_rays_merged(const ide3d_render_params* pp, const float* z_all, const int32_t* src, const float* z_fine,
                                        int32_t total_steps, void* stream) {
    using namespace ide3d;
    IDE3D_CHECK_ARG(pp != nullptr && z_all != nullptr && src != nullptr && z_fine != nullptr, "render_rays_merged: null pointer");
    const ide3d_render_params& p = *pp;
    int rc = check_hierarchical(p, "render_rays_merged");
    if (rc) return rc;
    IDE3D_CHECK_ARG(p.out_feat != nullptr, "render_rays_merged: null output pointer");
    IDE3D_CHECK_ARG((int64_t)total_steps == 2 * (int64_t)p.steps, "render_rays_merged: total_steps must be 2 * steps = %d, got %d", 2 * p.steps, total_steps);
    return with_form(p, mlp_split_selected(), "render_rays_merged", [&](auto f) {
        return launch_persistent<f.SPLIT>(render_rays_merged_kernel<f.C, f.HID, f.SPLIT>, "render_rays_merged", (int64_t)p.n * p.rays_per_img,
                                          kMarchLdsBytes<f.C, f.HID, f.SPLIT, true>, (hipStream_t)stream, p, z_all, src, z_fine);
    });
}

namespace ide3d {
const char* raymarch_build_flags() {
    return ""
#ifdef IDE3D_SPLIT_NO_DOT2
        "IDE3D_SPLIT_NO_DOT2 "
#endif
        ;
}
}  // namespace ide3d
