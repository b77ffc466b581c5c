// upfirdn2d.hip — pad -> zero-upsample -> 2-D FIR -> decimate, for gfx950.
//
// Semantics follow the reference op (torch_utils/ops/upfirdn2d.py:118, upfirdn2d.cpp:16):
//   out[oy, ox] = gain * sum_{ky,kx} U[oy*dy + ky - pad_y0, ox*dx + kx - pad_x0] * g[ky, kx]
// where U is the zero-upsampled input (U[iy*uy, ix*ux] = x[iy, ix], 0 elsewhere / outside) and
// g = f flipped in both axes (true convolution) unless `flip` is set.
//
// Five kernels in thirteen launchable forms; which one runs is decided by one host function, upfirdn2d_plan (below the kernels), which
// the launch and the host-only query ide3d_upfirdn2d_plan both go through:
//  * upfirdn2d_tile<...>: LDS-tiled polyphase kernel for the shapes on the IDE-3D render path
//    (4x4 [1,3,3,1] filter, up in {1,2}, down in {1,2}: four instances) and for one pass of a separable
//    12-tap filter (fp32; up 2 / down 2 / unit rate along x or y: six instances), w-contiguous (NCHW) tensors.  A
//    256-thread workgroup stages the input window of its output tile in LDS (zero-filled
//    outside the image), every lane then owns a register micro-tile and walks only the taps
//    that hit non-zero samples of its polyphase component.  Filter taps are read once through
//    uniform (scalar) loads.  HBM traffic = input + output, each touched once.
//  * upfirdn2d_generic: one output element per lane, any (up, down, filter, strides, dtype);
//    lanes run along the unit-stride axis (w for NCHW, c for channels_last) so global
//    accesses stay coalesced.
//  * upfirdn2d_cell<U = 2 | 4>: up U x U through a large filter held in LDS, one thread per output row of a cell.
//  * fir44_kernel / fir_up2_kernel: lean fp32 forms of the unit-rate and up-2 4x4 tile instances (bit-equal to them).
#include "common.h"
#include "knobs.h"
#include <type_traits>

namespace ide3d {

// Optional fused epilogue (ide3d_upfirdn2d_ex): FIR -> + add -> + noise -> bias_act.  All-null = plain upfirdn2d.
template <class T>
__device__ __forceinline__ typename Elem<T>::math_t
apply_epilogue(typename Elem<T>::math_t v, const ide3d_upfirdn2d_epilogue& ep, int n, int c, int oy, int ox, int out_w) {
    using M = typename Elem<T>::math_t;
    if (ep.add) v += Elem<T>::ld((const T*)ep.add + n * ep.add_stride[0] + c * ep.add_stride[1] + oy * ep.add_stride[2] + ox * ep.add_stride[3]);
    if (ep.noise) v += (M)(ep.noise[oy * out_w + ox] * ep.noise_strength);
    if (ep.fused_act) {
        if (ep.bias) v += Elem<T>::ld((const T*)ep.bias + c);
        if (ep.act == 3) v = (v > 0) ? v : v * (M)ep.alpha;
        v *= (M)ep.act_gain;
        if (ep.clamp >= 0.f) v = (v > (M)ep.clamp) ? (M)ep.clamp : ((v < -(M)ep.clamp) ? -(M)ep.clamp : v);
    }
    return v;
}

// Epilogue of NO consecutive outputs of one row (tile kernel): the per-row pointers are formed once, the skip / noise
// operands come in as one 16-byte load when the four outputs are in bounds and aligned, the bias is a scalar.
template <class T, int NO>
__device__ __forceinline__ void epilogue_row(typename Elem<T>::math_t (&row)[NO], const ide3d_upfirdn2d_epilogue& ep,
                                             const T* add_plane, typename Elem<T>::math_t bias, int oy, int ox0, int out_w, bool full) {
    using M = typename Elem<T>::math_t;
    if (ep.add) {
        const T* ap = add_plane + (int64_t)oy * ep.add_stride[2];
        if constexpr (sizeof(T) == 4 && NO == 4) {
            if (full && ep.add_stride[3] == 1 && ((reinterpret_cast<uintptr_t>(ap + ox0) & 15) == 0)) {
                const float4 a = *reinterpret_cast<const float4*>(ap + ox0);
                row[0] += a.x; row[1] += a.y; row[2] += a.z; row[3] += a.w;
                goto add_done;
            }
        }
#pragma unroll
        for (int j = 0; j < NO; ++j) {
            const int ox = ox0 + j;
            if (ox >= 0 && ox < out_w) row[j] += Elem<T>::ld(ap + (int64_t)ox * ep.add_stride[3]);
        }
    }
add_done:
    if (ep.noise) {
        const float* np_ = ep.noise + (int64_t)oy * out_w;
        if (NO == 4 && full && ((reinterpret_cast<uintptr_t>(np_ + ox0) & 15) == 0)) {
            const float4 a = *reinterpret_cast<const float4*>(np_ + ox0);
            row[0] += (M)(a.x * ep.noise_strength); row[1] += (M)(a.y * ep.noise_strength);
            row[2] += (M)(a.z * ep.noise_strength); row[3] += (M)(a.w * ep.noise_strength);
        } else {
#pragma unroll
            for (int j = 0; j < NO; ++j) {
                const int ox = ox0 + j;
                if (ox >= 0 && ox < out_w) row[j] += (M)(np_[ox] * ep.noise_strength);
            }
        }
    }
    if (ep.fused_act) {
#pragma unroll
        for (int j = 0; j < NO; ++j) {
            M v = row[j] + bias;
            if (ep.act == 3) v = (v > 0) ? v : v * (M)ep.alpha;
            v *= (M)ep.act_gain;
            if (ep.clamp >= 0.f) v = (v > (M)ep.clamp) ? (M)ep.clamp : ((v < -(M)ep.clamp) ? -(M)ep.clamp : v);
            row[j] = v;
        }
    }
}

// ------------------------------------------------------------------------------------------------
// Generic kernel
// ------------------------------------------------------------------------------------------------

template <class T>
__global__ void __launch_bounds__(256)
upfirdn2d_generic_kernel(ide3d_upfirdn2d_params p, ide3d_upfirdn2d_epilogue ep, int c_fastest) {
    using M = typename Elem<T>::math_t;
    const T* __restrict__ x = (const T*)p.x;
    T* __restrict__ y = (T*)p.y;
    const int64_t total = (int64_t)p.n * p.c * p.out_h * p.out_w;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    int am_n = -1; float am = 0.f;
    __shared__ unsigned s_am[64];
    const bool am_lds = ep.y_amax && p.n <= 64;
    if (ep.y_amax) { if (threadIdx.x < 64) s_am[threadIdx.x] = 0u; __syncthreads(); }
    for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += stride) {
        int ox, oy, c, n;
        int64_t r = idx;
        if (c_fastest) {
            c = (int)(r % p.c); r /= p.c;
            ox = (int)(r % p.out_w); r /= p.out_w;
            oy = (int)(r % p.out_h); r /= p.out_h;
            n = (int)r;
        } else {
            ox = (int)(r % p.out_w); r /= p.out_w;
            oy = (int)(r % p.out_h); r /= p.out_h;
            c = (int)(r % p.c); r /= p.c;
            n = (int)r;
        }
        // First tap whose upsampled coordinate lands on a real sample, per axis, and the input sample it lands on: one integer
        // division per axis and output — from there tap k + up reads input i + 1 (a division per tap made this kernel ~5x slower).
        const int X0 = ox * p.down_x - p.pad_x0;           // upsampled x of tap kx = 0
        const int Y0 = oy * p.down_y - p.pad_y0;
        int kx0, ky0, ix0, iy0;
        if (p.up_x == 1) { kx0 = 0; ix0 = X0; } else { ix0 = floordiv(X0 + p.up_x - 1, p.up_x); kx0 = ix0 * p.up_x - X0; }   // ceil(X0 / up)
        if (p.up_y == 1) { ky0 = 0; iy0 = Y0; } else { iy0 = floordiv(Y0 + p.up_y - 1, p.up_y); ky0 = iy0 * p.up_y - Y0; }
        // clip the tap ranges to the image instead of testing every tap
        int ty_begin = 0, tx_begin = 0;
        if (iy0 < 0) ty_begin = -iy0;
        if (ix0 < 0) tx_begin = -ix0;
        const int ty_end = min((p.f_h - ky0 + p.up_y - 1) / p.up_y, p.in_h - iy0);      // taps ky0 + t * up < f_h and iy0 + t < in_h
        const int tx_end = min((p.f_w - kx0 + p.up_x - 1) / p.up_x, p.in_w - ix0);
        const T* xp = x + n * p.x_stride[0] + c * p.x_stride[1];
        M acc = 0;
        for (int ty = ty_begin; ty < ty_end; ++ty) {
            const int ky = ky0 + ty * p.up_y;
            const int fy = p.flip ? ky : p.f_h - 1 - ky;
            const T* xr = xp + (int64_t)(iy0 + ty) * p.x_stride[2];
            const float* fr = p.f + (int64_t)fy * p.f_stride[0];
            int kx = kx0 + tx_begin * p.up_x;
            for (int tx = tx_begin; tx < tx_end; ++tx, kx += p.up_x) {
                const int fx = p.flip ? kx : p.f_w - 1 - kx;
                acc += Elem<T>::ld(xr + (int64_t)(ix0 + tx) * p.x_stride[3]) * (M)fr[fx * p.f_stride[1]];
            }
        }
        const M out = apply_epilogue<T>(acc * (M)p.gain, ep, n, c, oy, ox, p.out_w);
        Elem<T>::st(y + n * p.y_stride[0] + c * p.y_stride[1] + oy * p.y_stride[2] + ox * p.y_stride[3], out);
        if (ep.y_amax) {                                          // running maximum per image, flushed when the image changes
            if (n != am_n) { if (am_n >= 0) { if (am_lds) amax_lds_flush(s_am, am_n, am); else if (am > 0.f) amax_raise(ep.y_amax, am_n, am); } am_n = n; am = 0.f; }
            am = fmaxf(am, fabsf((float)out));
        }
    }
    if (ep.y_amax) {
        if (am_n >= 0) { if (am_lds) amax_lds_flush(s_am, am_n, am); else if (am > 0.f) amax_raise(ep.y_amax, am_n, am); }
        if (am_lds) amax_lds_commit(ep.y_amax, s_am, p.n);
    }
}

// ------------------------------------------------------------------------------------------------
// Cell kernel: up = U x U, no decimation, any (large) filter — one thread per output row of a cell of U x U outputs
// ------------------------------------------------------------------------------------------------
// The generic kernel walks the f_h f_w / U^2 taps of an output with two global loads per multiply-add; for the large filters the reference
// sends through `upfirdn2d_kernel_large` (upfirdn2d.cu:25-108; viz/renderer.py:360 up-samples the viewer's image by 4 with 47 x 47 taps) that
// is ~10 instructions per tap.  The U x U outputs of a cell (shifted outputs q U + j, j = 0 .. U - 1 per axis) read the SAME inputs
// q .. q + ceil(f / U): input q + d meets phase j through tap k = d U - j, i.e. one input sample feeds U x U multiply-adds whose taps are
// a contiguous U x U block of the filter.  The (flipped) filter sits in LDS, zero-padded to whole blocks, and is read as one 16-byte
// broadcast per block row: 1 global load + U LDS reads per U^2 multiply-adds.  Every output adds its taps in the generic kernel's order
// (ascending input row, then column); the padding taps add x * 0, so results are bit-equal to the generic kernel's for finite inputs
// (tests/test_gpu_ops.py::test_upfirdn2d_cell_kernel_equals_generic).
__host__ __device__ inline int cell_row_floats(int ntx, int U) { return ((ntx + 1 + 7) / 8) * 8 * U; }

template <class T, int U>
__global__ void __launch_bounds__(256)
upfirdn2d_cell_kernel(ide3d_upfirdn2d_params p, ide3d_upfirdn2d_epilogue ep, int cells_x, int cells_y, int qx_min, int qy_min, int ntx, int nty) {
    using M = typename Elem<T>::math_t;
    extern __shared__ __attribute__((aligned(16))) float s_fpad[];          // [(nty + 1) U][FPW]: entry (a, b) = tap (a - (U - 1), b - (U - 1)), zero where no tap is
    const int FPW = cell_row_floats(ntx, U), FPH = (nty + 1) * U;            // rows padded to whole batches of 8 blocks: the loop below never tests a tap
    for (int e = threadIdx.x; e < FPW * FPH; e += 256) {
        const int ky = e / FPW - (U - 1), kx = e % FPW - (U - 1);
        float v = 0.f;
        if (ky >= 0 && ky < p.f_h && kx >= 0 && kx < p.f_w) {
            const int fy = p.flip ? ky : p.f_h - 1 - ky, fx = p.flip ? kx : p.f_w - 1 - kx;
            v = p.f[(int64_t)fy * p.f_stride[0] + (int64_t)fx * p.f_stride[1]];
        }
        s_fpad[e] = v;
    }
    __syncthreads();
    const T* __restrict__ x = (const T*)p.x;
    T* __restrict__ y = (T*)p.y;
    // one thread = one output ROW of a cell (U outputs): a small image (the viewer's 3 x 128 x 128 -> 512 x 512) has 49 152 cells, less than
    // one wave per SIMD; per row it is three, and a thread's chain is a quarter as long
    const int64_t total = (int64_t)p.n * p.c * cells_y * U * cells_x;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += stride) {
        int64_t r = idx;
        const int cxi = (int)(r % cells_x); r /= cells_x;
        const int jy = (int)(r % U); r /= U;
        const int cyi = (int)(r % cells_y); r /= cells_y;
        const int c = (int)(r % p.c), n = (int)(r / p.c);
        const int qx = qx_min + cxi, qy = qy_min + cyi;
        const int oy = qy * U + jy + p.pad_y0;
        if (oy < 0 || oy >= p.out_h) continue;
        M acc[U];
#pragma unroll
        for (int jx = 0; jx < U; ++jx) acc[jx] = 0;
        const T* xp = x + n * p.x_stride[0] + c * p.x_stride[1];
        for (int dy = 0; dy <= nty; ++dy) {
            const int iy = qy + dy;
            if (iy < 0 || iy >= p.in_h) continue;
            const T* xr = xp + (int64_t)iy * p.x_stride[2];
            const float* frow = s_fpad + (dy * U + U - 1 - jy) * FPW;
            // the row's samples in batches of 8 loads in flight; a sample outside the image (or behind the last tap block: zero taps) enters as
            // 0 instead of being skipped — the same sum, without a branch per sample (the loop is instruction-issue bound: few waves, 4 multiply-adds
            // per sample)
            const int s3 = (int)p.x_stride[3];
            for (int dx0 = 0; dx0 <= ntx; dx0 += 8) {
                M xv[8];
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    const int ix = qx + dx0 + e;
                    const bool ok = (unsigned)ix < (unsigned)p.in_w;
                    const M v = Elem<T>::ld(xr + (ok ? ix : 0) * s3);
                    xv[e] = ok ? v : (M)0;
                }
                const float* fb = frow + dx0 * U;
#pragma unroll
                for (int e = 0; e < 8; ++e) {
#pragma unroll
                    for (int jx = 0; jx < U; ++jx) acc[jx] += xv[e] * (M)fb[e * U + U - 1 - jx];
                }
            }
        }
#pragma unroll
        for (int jx = 0; jx < U; ++jx) {
            const int ox = qx * U + jx + p.pad_x0;
            if (ox < 0 || ox >= p.out_w) continue;
            const M out = apply_epilogue<T>(acc[jx] * (M)p.gain, ep, n, c, oy, ox, p.out_w);
            Elem<T>::st(y + n * p.y_stride[0] + c * p.y_stride[1] + oy * p.y_stride[2] + ox * p.y_stride[3], out);
        }
    }
}

// ------------------------------------------------------------------------------------------------
// Tile kernel (NCHW, compile-time up/down/filter)
// ------------------------------------------------------------------------------------------------

// Polyphase bookkeeping for one axis.  U = up factor, D = down factor (U == 1 || D == 1), F = taps.
template <int U, int D, int F>
struct Axis {
    static constexpr int NT = (F + U - 1) / U;                  // max taps per phase
    // With U > 1 (D == 1) outputs are grouped in cells of U consecutive "shifted" outputs
    // o' = o - pad0 = q*U + r.  Phase r uses filter taps k = first(r) + t*U and inputs q + off(r) + t.
    static constexpr int first(int r) { return (U - r) % U; }
    static constexpr int ntaps(int r) { return first(r) < F ? (F - first(r) + U - 1) / U : 0; }
    static constexpr int off(int r) { return r == 0 ? 0 : 1; }
    // Input window (elements) needed by C consecutive cells.
    static constexpr int window(int C) { return U > 1 ? C + NT : (C - 1) * D + F; }
    // Input step between consecutive cells.
    static constexpr int step = (U > 1) ? 1 : D;
};

// LDS geometry of one tile instance: the kernel and the host plan (upfirdn2d_plan) read it from here.
template <int UX, int UY, int DX, int DY, int FW, int FH, int CX, int CY>
struct TileGeom {
    using AX = Axis<UX, DX, FW>;
    using AY = Axis<UY, DY, FH>;
    static constexpr int TX = 32, TY = 8;                              // thread grid inside the workgroup
    static constexpr int TCX = TX * CX, TCY = TY * CY;                 // cells per tile
    static constexpr int LW = ((AX::window(TCX) + 3) & ~3) + 4;        // LDS tile width (padded, see bank note)
    static constexpr int LH = AY::window(TCY);
    static constexpr int NLD4 = (LH * (LW / 4) + 255) / 256;           // 16-byte staging loads per thread
};

// The tile kernel's staging choice, in one place for the kernel and the host plan.  The instance half is a compile-time fact (element
// size, loads per thread), the plane half a run-time one: 16-byte staging reads whole aligned quads of a row, i.e. up to
// round_up(in_w, 4) - 1 — only when the rows start on the 16-byte grid (pitch a multiple of 4 floats, plane pointer aligned) and the
// caller promised that much of every row is readable (x_row_floats: padded rows) or in_w is a multiple of 4 — the last row of the last
// plane may end the storage.
__host__ __device__ constexpr bool tile_stage16_instance(int elem_bytes, int nld4) { return elem_bytes == 4 && nld4 <= 16; }
__host__ __device__ inline bool tile_stage16_plane(int64_t pitch, int in_w, int x_row_floats, uintptr_t plane_addr) {
    const int w4 = (in_w + 3) & ~3;
    return (pitch & 3) == 0 && pitch >= w4 && w4 <= (in_w > x_row_floats ? in_w : x_row_floats) && (plane_addr & 15) == 0;
}

template <class T, int UX, int UY, int DX, int DY, int FW, int FH, int CX, int CY>
__global__ void __launch_bounds__(256)
upfirdn2d_tile_kernel(ide3d_upfirdn2d_params p, ide3d_upfirdn2d_epilogue ep, int tiles_x, int tiles_y) {
    using M = typename Elem<T>::math_t;
    using G = TileGeom<UX, UY, DX, DY, FW, FH, CX, CY>;
    using AX = typename G::AX;
    using AY = typename G::AY;
    constexpr int TX = G::TX;
    constexpr int TCX = G::TCX, TCY = G::TCY;
    constexpr int LW = G::LW, LH = G::LH;
    constexpr int WX = AX::window(CX), WY = AY::window(CY);     // per-thread register window

    __shared__ __attribute__((aligned(16))) M s_in[LH * LW];

    // Flipped + gained taps through uniform loads (stay in SGPRs / constant VGPRs).
    M g[FH][FW];
#pragma unroll
    for (int ky = 0; ky < FH; ++ky)
#pragma unroll
        for (int kx = 0; kx < FW; ++kx) {
            const int fy = p.flip ? ky : FH - 1 - ky;
            const int fx = p.flip ? kx : FW - 1 - kx;
            g[ky][kx] = (M)p.f[fy * p.f_stride[0] + fx * p.f_stride[1]] * (M)p.gain;
        }

    // Tile decomposition: blockIdx.x -> (plane, tile_y, tile_x) with XCD-aware remap so that
    // vertically adjacent tiles of one plane (which share halo rows) sit in the same XCD's L2.
    const int nblocks = gridDim.x;
    int bid = xcd_remap(blockIdx.x, nblocks);
    const int tx_i = bid % tiles_x; bid /= tiles_x;
    const int ty_i = bid % tiles_y; bid /= tiles_y;
    const int plane = bid;                                      // n * C + c
    const int n = plane / p.c, c = plane % p.c;

    // Cell-space origin.  For U > 1: q_min = floor(-pad0 / U) is the cell holding output 0.
    const int qx_min = (UX > 1) ? floordiv(-p.pad_x0, UX) : 0;
    const int qy_min = (UY > 1) ? floordiv(-p.pad_y0, UY) : 0;
    const int qx0 = qx_min + tx_i * TCX;
    const int qy0 = qy_min + ty_i * TCY;
    // Input coordinate of LDS element (0, 0).
    const int in_x0 = (UX > 1) ? qx0 : qx0 * DX - p.pad_x0;
    const int in_y0 = (UY > 1) ? qy0 : qy0 * DY - p.pad_y0;

    const T* __restrict__ xp = (const T*)p.x + n * p.x_stride[0] + c * p.x_stride[1];
    // Fast staging (round 3) for fp32 planes whose rows start 16-byte aligned (row pitch a multiple of 4 floats: dense tensors of such
    // widths, and the (2h + 1)-wide transposed-convolution output, which ide3d_modconv2d writes with padded rows for this purpose,
    // `y_pitch`): the window is fetched with 16-byte loads from the 16-byte grid — LDS column 0 is the aligned column at or left of the
    // window's first one (xoff = 0..3 further) — 5 loads per thread instead of 19 four-byte ones.  Elements outside the image (and the
    // pad columns of a padded row, which hold no data) are zeroed by per-element selects on their true coordinates.
    int xoff = 0;
    bool staged = false;
    if constexpr (tile_stage16_instance((int)sizeof(T), G::NLD4)) {
        const int64_t pitch = p.x_stride[2];
        const int w4 = (p.in_w + 3) & ~3;
        if (tile_stage16_plane(pitch, p.in_w, p.x_row_floats, reinterpret_cast<uintptr_t>(xp))) {
            const int x_al = in_x0 & ~3;                          // floor to the 16-byte grid (two's complement: also for negative origins)
            xoff = in_x0 - x_al;
            constexpr int NV = LW / 4, NLD4 = (LH * NV + 255) / 256;
            static_assert(LW % 4 == 0 && LW >= AX::window(TCX) + 4, "LDS rows hold the window shifted by up to 3 columns");
            float4 v4[NLD4];
            unsigned long long okb = 0;                             // 4 validity bits per load
#pragma unroll
            for (int k = 0; k < NLD4; ++k) {
                const int idx = (int)threadIdx.x + k * 256;
                const int ly = idx / NV, lv = idx - ly * NV;
                const int gy = in_y0 + ly, gx = x_al + 4 * lv;
                const int cy_ = min(max(gy, 0), p.in_h - 1), cxv = min(max(gx, 0), w4 - 4);
                v4[k] = *reinterpret_cast<const float4*>(reinterpret_cast<const float*>(xp) + (int64_t)cy_ * pitch + cxv);
                const bool rowok = (gy == cy_) && idx < LH * NV;
#pragma unroll
                for (int e = 0; e < 4; ++e) okb |= (rowok && gx + e >= 0 && gx + e < p.in_w) ? (1ull << (4 * k + e)) : 0ull;
            }
#pragma unroll
            for (int k = 0; k < NLD4; ++k) {
                const int idx = (int)threadIdx.x + k * 256;
                if (idx < LH * NV) {
                    float4 w = v4[k];
                    w.x = ((okb >> (4 * k + 0)) & 1ull) ? w.x : 0.f; w.y = ((okb >> (4 * k + 1)) & 1ull) ? w.y : 0.f;
                    w.z = ((okb >> (4 * k + 2)) & 1ull) ? w.z : 0.f; w.w = ((okb >> (4 * k + 3)) & 1ull) ? w.w : 0.f;
                    *reinterpret_cast<float4*>(reinterpret_cast<float*>(s_in) + 4 * idx) = w;      // = row ly, columns 4 lv .. 4 lv + 3 (LW = 4 NV)
                }
            }
            staged = true;
        }
    }
    // Stage the input window: every load is unconditional (coordinates clamped into the image, out-of-image and
    // padding elements zeroed by a select afterwards) and all of a thread's loads are issued before the first LDS
    // write — conditional loads would each sit behind their own exec-mask branch and `s_waitcnt`.
    if (!staged) {
        constexpr int NLD = (LH * LW + 255) / 256;
        constexpr int DROW = 256 / LW, DCOL = 256 % LW;          // element i + 256 is DROW rows and DCOL columns further
        M v[NLD];
        int ly = (int)threadIdx.x / LW, lx = (int)threadIdx.x % LW;
        static_assert(NLD <= 64, "staging loads per thread must fit the validity mask");
        unsigned long long okbits = 0;
#pragma unroll
        for (int k = 0; k < NLD; ++k) {
            const int iy = in_y0 + ly, ix = in_x0 + lx;
            const int cy_ = min(max(iy, 0), p.in_h - 1), cx_ = min(max(ix, 0), p.in_w - 1);
            v[k] = Elem<T>::ld(xp + cy_ * p.x_stride[2] + cx_);
            okbits |= (lx < AX::window(TCX) && iy == cy_ && ix == cx_ && ly < LH) ? (1ull << k) : 0ull;
            lx += DCOL; ly += DROW;
            if (lx >= LW) { lx -= LW; ++ly; }
        }
#pragma unroll
        for (int k = 0; k < NLD; ++k) {
            const int i = (int)threadIdx.x + k * 256;
            if (i < LH * LW) s_in[i] = ((okbits >> k) & 1ull) ? v[k] : (M)0;
        }
    }
    __syncthreads();

    const int tx = threadIdx.x % TX, ty = threadIdx.x / TX;
    // Register window.
    M win[WY][WX];
    const int lx0 = tx * CX * AX::step, ly0 = ty * CY * AY::step;
    // (Round 4, VERDICT r3 item 2: this window is read with 4-byte LDS loads at a lane stride of 4 dwords - `lds_bank_conflict_frac` 0.68.  Reading
    // it as whole 16-byte quads (hand-issued ds_read_b128, one variant per `xoff`; hipcc narrows a float4 load with unused lanes back to
    // dwords) is conflict-free but moves 336 instead of 196 bytes per thread and needs 114 instead of 88 registers: 128.6 vs 110.4 us at
    // 64ch 513 -> 512, 139 vs 136 with the epilogue.  The conflicts are not what bounds this kernel; the dword reads stay.)
#pragma unroll
    for (int wy = 0; wy < WY; ++wy)
#pragma unroll
        for (int wx = 0; wx < WX; ++wx)
            win[wy][wx] = s_in[(ly0 + wy) * LW + lx0 + xoff + wx];

    float amax_t = 0.f;
    T* __restrict__ yp = (T*)p.y + n * p.y_stride[0] + c * p.y_stride[1];
    const T* add_plane = ep.add ? (const T*)ep.add + (int64_t)n * ep.add_stride[0] + (int64_t)c * ep.add_stride[1] : nullptr;
    const M bias = (ep.fused_act && ep.bias) ? (M)Elem<T>::ld((const T*)ep.bias + c) : (M)0;
#pragma unroll
    for (int cy = 0; cy < CY; ++cy)
#pragma unroll
        for (int ry = 0; ry < UY; ++ry) {
            const int qy = qy0 + ty * CY + cy;
            const int oy = (UY > 1) ? qy * UY + ry + p.pad_y0 : qy;
            if (oy < 0 || oy >= p.out_h) continue;
            M row[CX * UX];
#pragma unroll
            for (int cx = 0; cx < CX; ++cx)
#pragma unroll
                for (int rx = 0; rx < UX; ++rx) {
                    M acc = 0;
#pragma unroll
                    for (int ty_ = 0; ty_ < AY::ntaps(ry); ++ty_)
#pragma unroll
                        for (int tx_ = 0; tx_ < AX::ntaps(rx); ++tx_) {
                            const int wy = (UY > 1) ? cy + AY::off(ry) + ty_ : cy * DY + ty_;
                            const int wx = (UX > 1) ? cx + AX::off(rx) + tx_ : cx * DX + tx_;
                            acc += win[wy][wx] * g[AY::first(ry) + ty_ * UY][AX::first(rx) + tx_ * UX];
                        }
                    row[cx * UX + rx] = acc;
                }
            // Store CX*UX consecutive outputs.
            const int qx = qx0 + tx * CX;
            const int ox0 = (UX > 1) ? qx * UX + p.pad_x0 : qx;
            T* yr = yp + oy * p.y_stride[2];
            constexpr int NO = CX * UX;
            const bool full = ox0 >= 0 && ox0 + NO <= p.out_w;
            epilogue_row<T, NO>(row, ep, add_plane, bias, oy, ox0, p.out_w, full);
#pragma unroll
            for (int j = 0; j < NO; ++j)
                if (full || (ox0 + j >= 0 && ox0 + j < p.out_w)) amax_t = fmaxf(amax_t, fabsf((float)row[j]));      // one v_max per value; NaN ignored, inf kept
            if constexpr (sizeof(T) == 4 && NO == 4) {
                if (full && ((reinterpret_cast<uintptr_t>(yr + ox0) & 15) == 0)) {
                    float4 v4 = make_float4(row[0], row[1], row[2], row[3]);
                    *reinterpret_cast<float4*>(yr + ox0) = v4;
                    continue;
                }
            }
#pragma unroll
            for (int j = 0; j < NO; ++j) {
                const int ox = ox0 + j;
                if (ox >= 0 && ox < p.out_w) Elem<T>::st(yr + ox, row[j]);
            }
        }
    // max |finished output| of this tile's image for the consumer's f16x3 scale (a tile belongs to one (image, channel) plane)
    if (ep.y_amax) amax_raise_block(ep.y_amax, n, amax_t, reinterpret_cast<float*>(s_in));      // one read / atomic per tile
}

// ------------------------------------------------------------------------------------------------
// fp32 4x4 FIR at unit rate (the filter behind every transposed convolution of the generator), lean form (round 5)
// ------------------------------------------------------------------------------------------------
// The tile kernel above is VALU-issue bound on this shape, not HBM bound (round-5 reading of profiles/round5/fir_pmc.json: 832 vector
// instructions per wave for 16 outputs per lane, of which 288 are the filter; SQ_INSTS_VALU x 4 cycles / SIMD = 73 % of the kernel's
// cycles; more waves per SIMD, 7 instead of 5, changed nothing).  This kernel computes the same values in the same order (bit-equal) with the
// bookkeeping taken out of the vector pipe:
//   * every global access is `uniform base + 32-bit lane offset` (one v_mad + the instruction's own scalar base) instead of 64-bit pointer
//     arithmetic per row (98 v_lshl_add_u64 + 56 v_mad_u64_u32 in the tile kernel);
//   * out-of-image elements of the staged window are zeroed with ONE unsigned compare each on their true coordinates when the data arrives -
//     no validity words carried across the loads (64-bit shifts / ors / selects, ~140 instructions);
//   * the row loop has no per-row alignment tests: whether a lane's four outputs are a whole, aligned quad is decided once per lane (it is
//     the same for its four rows), whether the epilogue has noise / bias / lrelu / clamp once per workgroup;
//   * lrelu with 0 <= alpha <= 1 is max(v, v * alpha) (same value as the select for every input incl. -0 and NaN).
// Conditions (else the tile kernel runs): fp32, w-contiguous, rows of x start 16-byte aligned and may be read up to round_up(in_w, 4)
// (`x_row_floats`, see the tile kernel's fast staging), rows of y 16-byte aligned, out_w % 4 == 0, planes below 2^31 bytes, no skip operand.
// Tile = 128 x 32 outputs per 256-thread workgroup (lane: 4 x 4), window 35 x 136 floats of LDS (the window starts on the 16-byte grid).
__global__ void __launch_bounds__(256)
fir44_kernel(ide3d_upfirdn2d_params p, ide3d_upfirdn2d_epilogue ep, int tiles_x, int tiles_y) {
    constexpr int TCX = 128, TCY = 32, LW = 136, LH = TCY + 3, NV = LW / 4, NLD = (LH * NV + 255) / 256;
    __shared__ __attribute__((aligned(16))) float s_in[LH * LW];
    float g[4][4];
#pragma unroll
    for (int ky = 0; ky < 4; ++ky)
#pragma unroll
        for (int kx = 0; kx < 4; ++kx) {
            const int fy = p.flip ? ky : 3 - ky, fx = p.flip ? kx : 3 - kx;
            g[ky][kx] = p.f[fy * p.f_stride[0] + fx * p.f_stride[1]] * p.gain;
        }
    int bid = xcd_remap(blockIdx.x, gridDim.x);
    const int tx_i = bid % tiles_x; bid /= tiles_x;
    const int ty_i = bid % tiles_y; bid /= tiles_y;
    const int n = bid / p.c, c = bid % p.c;
    const int in_x0 = tx_i * TCX - p.pad_x0, in_y0 = ty_i * TCY - p.pad_y0;
    const int x_al = in_x0 & ~3, xoff = in_x0 - x_al;                 // LDS column 0 = the aligned column at or left of the window's first
    const float* __restrict__ xp = (const float*)p.x + n * p.x_stride[0] + c * p.x_stride[1];       // (uniform: scalar base of every load)
    const unsigned pitch = (unsigned)p.x_stride[2];
    const int w4 = (p.in_w + 3) & ~3;
    {
        float4 v4[NLD];
        int gy[NLD], gx[NLD];
#pragma unroll
        for (int k = 0; k < NLD; ++k) {
            const int idx = (int)threadIdx.x + k * 256;
            const int ly = idx / NV, lv = idx - ly * NV;
            gy[k] = in_y0 + ly; gx[k] = x_al + 4 * lv;
            const unsigned cy_ = (unsigned)min(max(gy[k], 0), p.in_h - 1), cx_ = (unsigned)min(max(gx[k], 0), w4 - 4);
            v4[k] = *reinterpret_cast<const float4*>(xp + (cy_ * pitch + cx_));
        }
#pragma unroll
        for (int k = 0; k < NLD; ++k) {
            const int idx = (int)threadIdx.x + k * 256;
            if (idx < LH * NV) {
                const bool rowok = (unsigned)gy[k] < (unsigned)p.in_h;
                float4 w = v4[k];
                w.x = (rowok && (unsigned)(gx[k] + 0) < (unsigned)p.in_w) ? w.x : 0.f;
                w.y = (rowok && (unsigned)(gx[k] + 1) < (unsigned)p.in_w) ? w.y : 0.f;
                w.z = (rowok && (unsigned)(gx[k] + 2) < (unsigned)p.in_w) ? w.z : 0.f;
                w.w = (rowok && (unsigned)(gx[k] + 3) < (unsigned)p.in_w) ? w.w : 0.f;
                *reinterpret_cast<float4*>(s_in + 4 * idx) = w;
            }
        }
    }
    __syncthreads();
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    float win[7][7];
    {
        const float* wsrc = s_in + (ty * 4) * LW + tx * 4 + xoff;
#pragma unroll
        for (int wy = 0; wy < 7; ++wy)
#pragma unroll
            for (int wx = 0; wx < 7; ++wx) win[wy][wx] = wsrc[wy * LW + wx];
    }
    // epilogue switches, once per workgroup (scalar)
    const bool has_noise = ep.noise != nullptr, act_on = ep.fused_act != 0;
    const float nstr = ep.noise_strength;
    const float bias = (act_on && ep.bias) ? ((const float*)ep.bias)[c] : 0.f;
    const bool lrelu = act_on && ep.act == 3, lrelu_max = lrelu && ep.alpha >= 0.f && ep.alpha <= 1.f;
    const float alpha = ep.alpha, again = act_on ? ep.act_gain : 1.f;
    const bool clamp_on = act_on && ep.clamp >= 0.f;
    const float cl = ep.clamp;
    float* __restrict__ yp = (float*)p.y + n * p.y_stride[0] + c * p.y_stride[1];
    const unsigned ypitch = (unsigned)p.y_stride[2];
    const int ox0 = tx_i * TCX + tx * 4, oy0 = ty_i * TCY + ty * 4;
    const bool full = ox0 + 4 <= p.out_w;                            // (out_w % 4 == 0: a lane's quad is whole or absent)
    float amax_t = 0.f;
    if (full) {
#pragma unroll
        for (int cy = 0; cy < 4; ++cy) {
            const int oy = oy0 + cy;
            if (oy >= p.out_h) break;
            float row[4];
#pragma unroll
            for (int cx = 0; cx < 4; ++cx) {
                float acc = 0.f;
#pragma unroll
                for (int ky = 0; ky < 4; ++ky)
#pragma unroll
                    for (int kx = 0; kx < 4; ++kx) acc += win[cy + ky][cx + kx] * g[ky][kx];
                row[cx] = acc;
            }
            if (has_noise) {
                const float4 a = *reinterpret_cast<const float4*>(ep.noise + ((unsigned)oy * (unsigned)p.out_w + (unsigned)ox0));
                row[0] += a.x * nstr; row[1] += a.y * nstr; row[2] += a.z * nstr; row[3] += a.w * nstr;
            }
            if (act_on) {
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    float v = row[j] + bias;
                    if (lrelu_max) v = fmaxf(v, v * alpha);
                    else if (lrelu) v = (v > 0.f) ? v : v * alpha;
                    v *= again;
                    if (clamp_on) v = (v > cl) ? cl : ((v < -cl) ? -cl : v);
                    row[j] = v;
                }
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) amax_t = fmaxf(amax_t, fabsf(row[j]));
            *reinterpret_cast<float4*>(yp + ((unsigned)oy * ypitch + (unsigned)ox0)) = make_float4(row[0], row[1], row[2], row[3]);
        }
    }
    if (ep.y_amax) amax_raise_block(ep.y_amax, n, amax_t, s_in);
}

// fp32 4x4 FIR with 2x zero-upsampling (the skip-image upsampler, upfirdn2d.upsample2d with the [1, 3, 3, 1] filter, optionally + the skip
// operand), lean form: same polyphase arithmetic in the same order as upfirdn2d_tile_kernel<float, 2, 2, 1, 1, 4, 4, 2, 2> (bit-equal; that
// kernel spends 386 vector instructions per wave on 64 multiply-adds per lane), bookkeeping as in fir44_kernel.  Tile = 64 x 16 cells
// (128 x 32 outputs) per 256-thread workgroup, lane = 2 x 2 cells = 4 x 4 outputs from a 4 x 4 window.
__global__ void __launch_bounds__(256)
fir_up2_kernel(ide3d_upfirdn2d_params p, ide3d_upfirdn2d_epilogue ep, int tiles_x, int tiles_y) {
    using AX = Axis<2, 1, 4>;
    constexpr int TCX = 64, TCY = 16, LW = 72, LH = TCY + 2, NV = LW / 4, NLD = (LH * NV + 255) / 256;
    static_assert(AX::window(TCX) + 3 <= LW && AX::NT == 2 && AX::window(2) == 4, "window of the 4-tap polyphase filter");
    __shared__ __attribute__((aligned(16))) float s_in[LH * LW];
    float g[4][4];
#pragma unroll
    for (int ky = 0; ky < 4; ++ky)
#pragma unroll
        for (int kx = 0; kx < 4; ++kx) {
            const int fy = p.flip ? ky : 3 - ky, fx = p.flip ? kx : 3 - kx;
            g[ky][kx] = p.f[fy * p.f_stride[0] + fx * p.f_stride[1]] * p.gain;
        }
    int bid = xcd_remap(blockIdx.x, gridDim.x);
    const int tx_i = bid % tiles_x; bid /= tiles_x;
    const int ty_i = bid % tiles_y; bid /= tiles_y;
    const int n = bid / p.c, c = bid % p.c;
    const int qx0 = floordiv(-p.pad_x0, 2) + tx_i * TCX, qy0 = floordiv(-p.pad_y0, 2) + ty_i * TCY;      // cell = input coordinate of LDS element (0, 0)
    const int x_al = qx0 & ~3, xoff = qx0 - x_al;
    const float* __restrict__ xp = (const float*)p.x + n * p.x_stride[0] + c * p.x_stride[1];
    const unsigned pitch = (unsigned)p.x_stride[2];
    const int w4 = (p.in_w + 3) & ~3;
    {
        float4 v4[NLD];
        int gy[NLD], gx[NLD];
#pragma unroll
        for (int k = 0; k < NLD; ++k) {
            const int idx = (int)threadIdx.x + k * 256;
            const int ly = idx / NV, lv = idx - ly * NV;
            gy[k] = qy0 + ly; gx[k] = x_al + 4 * lv;
            const unsigned cy_ = (unsigned)min(max(gy[k], 0), p.in_h - 1), cx_ = (unsigned)min(max(gx[k], 0), w4 - 4);
            v4[k] = *reinterpret_cast<const float4*>(xp + (cy_ * pitch + cx_));
        }
#pragma unroll
        for (int k = 0; k < NLD; ++k) {
            const int idx = (int)threadIdx.x + k * 256;
            if (idx < LH * NV) {
                const bool rowok = (unsigned)gy[k] < (unsigned)p.in_h;
                float4 w = v4[k];
                w.x = (rowok && (unsigned)(gx[k] + 0) < (unsigned)p.in_w) ? w.x : 0.f;
                w.y = (rowok && (unsigned)(gx[k] + 1) < (unsigned)p.in_w) ? w.y : 0.f;
                w.z = (rowok && (unsigned)(gx[k] + 2) < (unsigned)p.in_w) ? w.z : 0.f;
                w.w = (rowok && (unsigned)(gx[k] + 3) < (unsigned)p.in_w) ? w.w : 0.f;
                *reinterpret_cast<float4*>(s_in + 4 * idx) = w;
            }
        }
    }
    __syncthreads();
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    float win[4][4];
    {
        const float* wsrc = s_in + (ty * 2) * LW + tx * 2 + xoff;
#pragma unroll
        for (int wy = 0; wy < 4; ++wy)
#pragma unroll
            for (int wx = 0; wx < 4; ++wx) win[wy][wx] = wsrc[wy * LW + wx];
    }
    const bool has_add = ep.add != nullptr, has_noise = ep.noise != nullptr, act_on = ep.fused_act != 0;
    const float nstr = ep.noise_strength;
    const float bias = (act_on && ep.bias) ? ((const float*)ep.bias)[c] : 0.f;
    const bool lrelu = act_on && ep.act == 3, lrelu_max = lrelu && ep.alpha >= 0.f && ep.alpha <= 1.f;
    const float alpha = ep.alpha, again = act_on ? ep.act_gain : 1.f;
    const bool clamp_on = act_on && ep.clamp >= 0.f;
    const float cl = ep.clamp;
    float* __restrict__ yp = (float*)p.y + n * p.y_stride[0] + c * p.y_stride[1];
    const float* __restrict__ ap = has_add ? (const float*)ep.add + n * ep.add_stride[0] + c * ep.add_stride[1] : nullptr;
    const unsigned ypitch = (unsigned)p.y_stride[2], apitch = (unsigned)ep.add_stride[2];
    const int ox0 = (qx0 + tx * 2) * 2 + p.pad_x0;                  // first of this lane's four outputs (a multiple of 4: checked on the host)
    const bool full = ox0 >= 0 && ox0 + 4 <= p.out_w;
    float amax_t = 0.f;
    if (full) {
#pragma unroll
        for (int cy = 0; cy < 2; ++cy)
#pragma unroll
            for (int ry = 0; ry < 2; ++ry) {
                const int oy = (qy0 + ty * 2 + cy) * 2 + ry + p.pad_y0;
                if (oy < 0 || oy >= p.out_h) continue;
                float row[4];
#pragma unroll
                for (int cx = 0; cx < 2; ++cx)
#pragma unroll
                    for (int rx = 0; rx < 2; ++rx) {
                        float acc = 0.f;
#pragma unroll
                        for (int ty_ = 0; ty_ < 2; ++ty_)
#pragma unroll
                            for (int tx_ = 0; tx_ < 2; ++tx_)
                                acc += win[cy + AX::off(ry) + ty_][cx + AX::off(rx) + tx_] * g[AX::first(ry) + ty_ * 2][AX::first(rx) + tx_ * 2];
                        row[cx * 2 + rx] = acc;
                    }
                if (has_add) {
                    const float4 a = *reinterpret_cast<const float4*>(ap + ((unsigned)oy * apitch + (unsigned)ox0));
                    row[0] += a.x; row[1] += a.y; row[2] += a.z; row[3] += a.w;
                }
                if (has_noise) {
                    const float4 a = *reinterpret_cast<const float4*>(ep.noise + ((unsigned)oy * (unsigned)p.out_w + (unsigned)ox0));
                    row[0] += a.x * nstr; row[1] += a.y * nstr; row[2] += a.z * nstr; row[3] += a.w * nstr;
                }
                if (act_on) {
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        float v = row[j] + bias;
                        if (lrelu_max) v = fmaxf(v, v * alpha);
                        else if (lrelu) v = (v > 0.f) ? v : v * alpha;
                        v *= again;
                        if (clamp_on) v = (v > cl) ? cl : ((v < -cl) ? -cl : v);
                        row[j] = v;
                    }
                }
#pragma unroll
                for (int j = 0; j < 4; ++j) amax_t = fmaxf(amax_t, fabsf(row[j]));
                *reinterpret_cast<float4*>(yp + ((unsigned)oy * ypitch + (unsigned)ox0)) = make_float4(row[0], row[1], row[2], row[3]);
            }
    }
    if (ep.y_amax) amax_raise_block(ep.y_amax, n, amax_t, s_in);
}

// ------------------------------------------------------------------------------------------------
// Host: one function decides the form and its geometry (upfirdn2d_plan); the launch and the ide3d_upfirdn2d_plan query go through it
// ------------------------------------------------------------------------------------------------

// the conditions of fir44_kernel (see there)
static bool fir44_applies(const ide3d_upfirdn2d_params& p, const ide3d_upfirdn2d_epilogue& ep) {
    const bool off = knob_live("IDE3D_FIR_NO_LEAN");      // read per call: tests/test_gpu_ops.py flips it inside one process
    if (off || p.dtype != IDE3D_F32 || p.f_w != 4 || p.f_h != 4 || p.up_x != 1 || p.up_y != 1 || p.down_x != 1 || p.down_y != 1) return false;
    if (p.x_stride[3] != 1 || p.y_stride[3] != 1 || ep.add || p.out_w <= 64 || (p.out_w & 3)) return false;
    const int64_t pitch = p.x_stride[2], w4 = (p.in_w + 3) & ~3;
    if ((pitch & 3) || pitch < w4 || w4 > (p.in_w > p.x_row_floats ? p.in_w : p.x_row_floats)) return false;
    if ((reinterpret_cast<uintptr_t>(p.x) & 15) || (p.x_stride[0] & 3) || (p.x_stride[1] & 3)) return false;
    if ((reinterpret_cast<uintptr_t>(p.y) & 15) || (p.y_stride[0] & 3) || (p.y_stride[1] & 3) || (p.y_stride[2] & 3)) return false;
    if (ep.noise && (reinterpret_cast<uintptr_t>(ep.noise) & 15)) return false;
    if (pitch * p.in_h >= (1ll << 29) || p.y_stride[2] * (int64_t)p.out_h >= (1ll << 29) || (int64_t)p.out_w * p.out_h >= (1ll << 29)) return false;
    if (p.x_stride[2] <= 0 || p.y_stride[2] <= 0) return false;
    return true;
}

// the conditions of fir_up2_kernel (see there)
static bool fir_up2_applies(const ide3d_upfirdn2d_params& p, const ide3d_upfirdn2d_epilogue& ep) {
    const bool off = knob_live("IDE3D_FIR_NO_LEAN");      // read per call: tests/test_gpu_ops.py flips it inside one process
    if (off || p.dtype != IDE3D_F32 || p.f_w != 4 || p.f_h != 4 || p.up_x != 2 || p.up_y != 2 || p.down_x != 1 || p.down_y != 1) return false;
    if (p.x_stride[3] != 1 || p.y_stride[3] != 1 || (p.out_w & 3) || (p.in_w & 3)) return false;
    // a lane's four outputs start at ((floor(-pad_x0 / 2) + 2 k) * 2 + pad_x0: a multiple of 4 for even pads (upsample2d: 2), never for odd ones
    if (p.pad_x0 & 1) return false;
    const int64_t pitch = p.x_stride[2];
    if ((pitch & 3) || pitch < p.in_w || pitch <= 0 || p.y_stride[2] <= 0) return false;
    if ((reinterpret_cast<uintptr_t>(p.x) & 15) || (p.x_stride[0] & 3) || (p.x_stride[1] & 3)) return false;
    if ((reinterpret_cast<uintptr_t>(p.y) & 15) || (p.y_stride[0] & 3) || (p.y_stride[1] & 3) || (p.y_stride[2] & 3)) return false;
    if (ep.add && (ep.add_stride[3] != 1 || (reinterpret_cast<uintptr_t>(ep.add) & 15) || (ep.add_stride[0] & 3) || (ep.add_stride[1] & 3) || (ep.add_stride[2] & 3) ||
                   ep.add_stride[2] <= 0 || ep.add_stride[2] * (int64_t)p.out_h >= (1ll << 29))) return false;
    if (ep.noise && (reinterpret_cast<uintptr_t>(ep.noise) & 15)) return false;
    if (pitch * p.in_h >= (1ll << 29) || p.y_stride[2] * (int64_t)p.out_h >= (1ll << 29) || (int64_t)p.out_w * p.out_h >= (1ll << 29)) return false;
    return true;
}

// up-sampling by 2 x 2 / 4 x 4 without decimation through a filter of >= 36 taps that no tile instance covers (and whose padded copy fits 48 KB of LDS)
static bool cell_applies(const ide3d_upfirdn2d_params& p, const ide3d_upfirdn2d_epilogue& ep) {
    if (knob_live("IDE3D_FIR_NO_CELL")) return false;
    if (p.up_x != p.up_y || (p.up_x != 2 && p.up_x != 4) || p.down_x != 1 || p.down_y != 1 || ep.y_amax) return false;
    if ((int64_t)p.f_w * p.f_h < 36) return false;
    const int U = p.up_x;
    return (int64_t)cell_row_floats(cdiv(p.f_w, U), U) * (cdiv(p.f_h, U) + 1) * U * 4 <= 48 * 1024 && p.x_stride[3] * (int64_t)p.in_w < (1ll << 31);
}

// cells of U shifted outputs that cover `out` outputs of one axis: floor(-pad0 / U) is the cell holding output 0
static inline int cells_of(int out, int pad0, int U) {
    if (U == 1) return out;
    return floordiv(out - 1 - pad0, U) - floordiv(-pad0, U) + 1;
}

// how the planes of x stage in a tile instance that may stage by 16 bytes: plane (n, c) starts at x + n stride[0] + c stride[1]; the
// alignment of the planes repeats with period 4 in n and in c
static int tile_staging(const ide3d_upfirdn2d_params& p) {
    int staged = 0, planes = 0;
    for (int n = 0; n < (p.n < 4 ? p.n : 4); ++n)
        for (int c = 0; c < (p.c < 4 ? p.c : 4); ++c, ++planes)
            staged += tile_stage16_plane(p.x_stride[2], p.in_w, p.x_row_floats,
                                         reinterpret_cast<uintptr_t>(p.x) + (uintptr_t)((n * p.x_stride[0] + c * p.x_stride[1]) * 4)) ? 1 : 0;
    return staged == planes ? 1 : staged == 0 ? 0 : 2;
}

template <int UX, int UY, int DX, int DY, int FW, int FH, int CX, int CY>
static int plan_tile(const ide3d_upfirdn2d_params& p, ide3d_upfirdn2d_plan_info* o) {
    using G = TileGeom<UX, UY, DX, DY, FW, FH, CX, CY>;
    o->form = IDE3D_UPFIRDN_TILE;
    o->ux = UX; o->uy = UY; o->dx = DX; o->dy = DY; o->fw = FW; o->fh = FH; o->cx = CX; o->cy = CY;
    o->tiles_x = cdiv(cells_of(p.out_w, p.pad_x0, UX), G::TCX);
    o->tiles_y = cdiv(cells_of(p.out_h, p.pad_y0, UY), G::TCY);
    o->grid = (int64_t)o->tiles_x * o->tiles_y * p.n * p.c;
    o->staging = (p.dtype == IDE3D_F32 && tile_stage16_instance(4, G::NLD4)) ? tile_staging(p) : 0;
    if (o->grid > 0x7fffffff) { set_error("upfirdn2d: grid too large"); return IDE3D_EINVAL; }
    return IDE3D_OK;
}

// Which kernel form runs, with its launch geometry.  Host arithmetic only: pointers count for their alignment and are never dereferenced.
static int upfirdn2d_plan(const ide3d_upfirdn2d_params& p, const ide3d_upfirdn2d_epilogue& ep, ide3d_upfirdn2d_plan_info* o) {
    *o = ide3d_upfirdn2d_plan_info{};
    o->staging = -1;
    const bool w_contig = (p.x_stride[3] == 1 && p.y_stride[3] == 1);
    const bool f32 = p.dtype == IDE3D_F32;
    if (p.dtype != IDE3D_F64) {
        if (w_contig && p.f_w == 4 && p.f_h == 4) {
            if (p.up_x == 1 && p.up_y == 1 && p.down_x == 1 && p.down_y == 1) {
                // 4 output rows per thread: 7 window rows serve 4 rows (halo 9 % instead of 19 %); narrow images get a
                // 64-wide tile so that lanes are not wasted on columns that do not exist
                if (p.out_w <= 64) return plan_tile<1, 1, 1, 1, 4, 4, 2, 4>(p, o);
                if (f32 && fir44_applies(p, ep)) {
                    o->form = IDE3D_UPFIRDN_FIR44;
                    o->ux = 1; o->uy = 1; o->dx = 1; o->dy = 1; o->fw = 4; o->fh = 4; o->cx = 4; o->cy = 4;
                    o->staging = 1;
                    o->tiles_x = cdiv(p.out_w, 128); o->tiles_y = cdiv(p.out_h, 32);
                    o->grid = (int64_t)o->tiles_x * o->tiles_y * p.n * p.c;
                    if (o->grid > 0x7fffffff) { set_error("upfirdn2d: grid too large"); return IDE3D_EINVAL; }
                    return IDE3D_OK;
                }
                return plan_tile<1, 1, 1, 1, 4, 4, 4, 4>(p, o);
            }
            if (p.up_x == 2 && p.up_y == 2 && p.down_x == 1 && p.down_y == 1) {
                if (f32 && fir_up2_applies(p, ep)) {
                    o->form = IDE3D_UPFIRDN_FIR_UP2;
                    o->ux = 2; o->uy = 2; o->dx = 1; o->dy = 1; o->fw = 4; o->fh = 4; o->cx = 2; o->cy = 2;
                    o->staging = 1;
                    o->tiles_x = cdiv(cells_of(p.out_w, p.pad_x0, 2), 64); o->tiles_y = cdiv(cells_of(p.out_h, p.pad_y0, 2), 16);
                    o->grid = (int64_t)o->tiles_x * o->tiles_y * p.n * p.c;
                    if (o->grid > 0x7fffffff) { set_error("upfirdn2d: grid too large"); return IDE3D_EINVAL; }
                    return IDE3D_OK;
                }
                return plan_tile<2, 2, 1, 1, 4, 4, 2, 2>(p, o);
            }
            if (p.up_x == 1 && p.up_y == 1 && p.down_x == 2 && p.down_y == 2) return plan_tile<1, 1, 2, 2, 4, 4, 4, 2>(p, o);
        }
        // one pass of a separable 12-tap filter (upfirdn2d.py:192-199 runs [1, 12] then [12, 1]; training/augment.py:295,306 sym6
        // wavelets, StyleGAN3-style up / down by 2): the same LDS-tiled polyphase kernel with a 1-D tap set
        if (f32) {
            if (w_contig && p.f_w == 12 && p.f_h == 1 && p.up_y == 1 && p.down_y == 1) {
                if (p.up_x == 2 && p.down_x == 1) return plan_tile<2, 1, 1, 1, 12, 1, 2, 4>(p, o);
                if (p.up_x == 1 && p.down_x == 2) return plan_tile<1, 1, 2, 1, 12, 1, 4, 4>(p, o);
                if (p.up_x == 1 && p.down_x == 1) return plan_tile<1, 1, 1, 1, 12, 1, 4, 4>(p, o);
            }
            if (w_contig && p.f_w == 1 && p.f_h == 12 && p.up_x == 1 && p.down_x == 1) {
                if (p.up_y == 2 && p.down_y == 1) return plan_tile<1, 2, 1, 1, 1, 12, 4, 2>(p, o);
                if (p.up_y == 1 && p.down_y == 2) return plan_tile<1, 1, 1, 2, 1, 12, 4, 2>(p, o);
                if (p.up_y == 1 && p.down_y == 1) return plan_tile<1, 1, 1, 1, 1, 12, 4, 4>(p, o);
            }
        }
        if (cell_applies(p, ep)) {
            const int U = p.up_x;
            o->form = IDE3D_UPFIRDN_CELL;
            o->cell_u = U;
            o->tiles_x = cells_of(p.out_w, p.pad_x0, U); o->tiles_y = cells_of(p.out_h, p.pad_y0, U);
            o->lds_bytes = (int64_t)cell_row_floats(cdiv(p.f_w, U), U) * (cdiv(p.f_h, U) + 1) * U * (int64_t)sizeof(float);
            o->grid = stream_grid((int64_t)p.n * p.c * o->tiles_y * U * o->tiles_x, 256);
            return IDE3D_OK;
        }
    }
    o->form = IDE3D_UPFIRDN_GENERIC;
    o->c_fastest = (p.y_stride[1] == 1 && p.c > 1) ? 1 : 0;
    o->grid = stream_grid((int64_t)p.n * p.c * p.out_h * p.out_w, 256);
    return IDE3D_OK;
}

template <class T, int UX, int UY, int DX, int DY, int FW, int FH, int CX, int CY>
static int launch_tile(const ide3d_upfirdn2d_params& p, const ide3d_upfirdn2d_epilogue& ep, const ide3d_upfirdn2d_plan_info& pl, hipStream_t st) {
    hipLaunchKernelGGL((upfirdn2d_tile_kernel<T, UX, UY, DX, DY, FW, FH, CX, CY>), dim3((unsigned)pl.grid),
                       dim3(256), 0, st, p, ep, pl.tiles_x, pl.tiles_y);
    IDE3D_CHECK_LAUNCH("upfirdn2d_tile");
    return IDE3D_OK;
}

template <class T, int U>
static int launch_cell(const ide3d_upfirdn2d_params& p, const ide3d_upfirdn2d_epilogue& ep, const ide3d_upfirdn2d_plan_info& pl, hipStream_t st) {
    hipLaunchKernelGGL((upfirdn2d_cell_kernel<T, U>), dim3((unsigned)pl.grid), dim3(256), (size_t)pl.lds_bytes, st, p, ep, pl.tiles_x, pl.tiles_y,
                       floordiv(-p.pad_x0, U), floordiv(-p.pad_y0, U), cdiv(p.f_w, U), cdiv(p.f_h, U));
    IDE3D_CHECK_LAUNCH("upfirdn2d_cell");
    return IDE3D_OK;
}

// launch what the plan says; a plan that names a form the storage type has no kernel for cannot come out of upfirdn2d_plan
template <class T>
static int launch_planned(const ide3d_upfirdn2d_params& p, const ide3d_upfirdn2d_epilogue& ep, const ide3d_upfirdn2d_plan_info& pl, hipStream_t st) {
#define IDE3D_TILE_CASE(UX, UY, DX, DY, FW, FH, CX, CY)                                                                              \
    if (pl.ux == UX && pl.uy == UY && pl.dx == DX && pl.dy == DY && pl.fw == FW && pl.fh == FH && pl.cx == CX && pl.cy == CY)         \
        return launch_tile<T, UX, UY, DX, DY, FW, FH, CX, CY>(p, ep, pl, st)
    switch (pl.form) {
    case IDE3D_UPFIRDN_FIR44:
        if constexpr (std::is_same<T, float>::value) {
            hipLaunchKernelGGL(fir44_kernel, dim3((unsigned)pl.grid), dim3(256), 0, st, p, ep, pl.tiles_x, pl.tiles_y);
            IDE3D_CHECK_LAUNCH("upfirdn2d (fir44)");
            return IDE3D_OK;
        }
        break;
    case IDE3D_UPFIRDN_FIR_UP2:
        if constexpr (std::is_same<T, float>::value) {
            hipLaunchKernelGGL(fir_up2_kernel, dim3((unsigned)pl.grid), dim3(256), 0, st, p, ep, pl.tiles_x, pl.tiles_y);
            IDE3D_CHECK_LAUNCH("upfirdn2d (fir_up2)");
            return IDE3D_OK;
        }
        break;
    case IDE3D_UPFIRDN_TILE:
        if constexpr (!std::is_same<T, double>::value) {
            IDE3D_TILE_CASE(1, 1, 1, 1, 4, 4, 2, 4);
            IDE3D_TILE_CASE(1, 1, 1, 1, 4, 4, 4, 4);
            IDE3D_TILE_CASE(2, 2, 1, 1, 4, 4, 2, 2);
            IDE3D_TILE_CASE(1, 1, 2, 2, 4, 4, 4, 2);
        }
        if constexpr (std::is_same<T, float>::value) {
            IDE3D_TILE_CASE(2, 1, 1, 1, 12, 1, 2, 4);
            IDE3D_TILE_CASE(1, 1, 2, 1, 12, 1, 4, 4);
            IDE3D_TILE_CASE(1, 1, 1, 1, 12, 1, 4, 4);
            IDE3D_TILE_CASE(1, 2, 1, 1, 1, 12, 4, 2);
            IDE3D_TILE_CASE(1, 1, 1, 2, 1, 12, 4, 2);
            IDE3D_TILE_CASE(1, 1, 1, 1, 1, 12, 4, 4);
        }
        break;
    case IDE3D_UPFIRDN_CELL:
        if constexpr (!std::is_same<T, double>::value) return pl.cell_u == 2 ? launch_cell<T, 2>(p, ep, pl, st) : launch_cell<T, 4>(p, ep, pl, st);
        break;
    case IDE3D_UPFIRDN_GENERIC:
        hipLaunchKernelGGL((upfirdn2d_generic_kernel<T>), dim3((unsigned)pl.grid), dim3(256), 0, st, p, ep, pl.c_fastest);
        IDE3D_CHECK_LAUNCH("upfirdn2d_generic");
        return IDE3D_OK;
    }
#undef IDE3D_TILE_CASE
    set_error("upfirdn2d: no kernel for the planned form %d", pl.form);
    return IDE3D_ENOKERNEL;
}

}  // namespace ide3d

// what ide3d_upfirdn2d, ide3d_upfirdn2d_ex and ide3d_upfirdn2d_plan refuse, and the plan of the rest
static int upfirdn2d_checked_plan(const ide3d_upfirdn2d_params* pp, const ide3d_upfirdn2d_epilogue* epp, ide3d_upfirdn2d_epilogue* ep_out,
                                  ide3d_upfirdn2d_plan_info* plan) {
    using namespace ide3d;
    IDE3D_CHECK_ARG(pp != nullptr, "upfirdn2d: null params");
    const ide3d_upfirdn2d_params& p = *pp;
    ide3d_upfirdn2d_epilogue ep{};
    if (epp) ep = *epp;
    IDE3D_CHECK_ARG(p.x && p.f && p.y, "upfirdn2d: null tensor pointer");
    IDE3D_CHECK_ARG(p.n > 0 && p.c > 0 && p.in_h > 0 && p.in_w > 0, "upfirdn2d: x is empty");
    IDE3D_CHECK_ARG(p.f_h >= 1 && p.f_w >= 1, "upfirdn2d: f is empty");
    IDE3D_CHECK_ARG(p.up_x >= 1 && p.up_y >= 1, "upfirdn2d: upsampling factor must be at least 1");
    IDE3D_CHECK_ARG(p.down_x >= 1 && p.down_y >= 1, "upfirdn2d: downsampling factor must be at least 1");
    IDE3D_CHECK_ARG(p.out_h >= 1 && p.out_w >= 1, "upfirdn2d: output must be at least 1x1");
    IDE3D_CHECK_ARG(!ep.fused_act || ep.act == 1 || ep.act == 3, "upfirdn2d_ex: fused activation must be linear (1) or lrelu (3)");
    if (p.dtype != IDE3D_F32 && p.dtype != IDE3D_F16 && p.dtype != IDE3D_BF16 && p.dtype != IDE3D_F64) {
        set_error("upfirdn2d: unsupported dtype code %d", p.dtype);
        return IDE3D_EINVAL;
    }
    *ep_out = ep;
    return upfirdn2d_plan(p, ep, plan);
}

static int upfirdn2d_entry(const ide3d_upfirdn2d_params* pp, const ide3d_upfirdn2d_epilogue* epp, void* stream) {
    using namespace ide3d;
    ide3d_upfirdn2d_epilogue ep;
    ide3d_upfirdn2d_plan_info plan;
    const int rc = upfirdn2d_checked_plan(pp, epp, &ep, &plan);
    if (rc != IDE3D_OK) return rc;
    const ide3d_upfirdn2d_params& p = *pp;
    hipStream_t st = (hipStream_t)stream;
    switch (p.dtype) {
    case IDE3D_F32:  return launch_planned<float>(p, ep, plan, st);
    case IDE3D_F16:  return launch_planned<__half>(p, ep, plan, st);
    case IDE3D_BF16: return launch_planned<__hip_bfloat16>(p, ep, plan, st);
    default:         return launch_planned<double>(p, ep, plan, st);
    }
}

extern "C" int ide3d_upfirdn2d_plan(const ide3d_upfirdn2d_params* pp, const ide3d_upfirdn2d_epilogue* epp, ide3d_upfirdn2d_plan_info* out) {
    using namespace ide3d;
    IDE3D_CHECK_ARG(out, "upfirdn2d_plan: null pointer");
    ide3d_upfirdn2d_epilogue ep;
    return upfirdn2d_checked_plan(pp, epp, &ep, out);
}

extern "C" int ide3d_upfirdn2d(const ide3d_upfirdn2d_params* pp, void* stream) {
    return upfirdn2d_entry(pp, nullptr, stream);
}

extern "C" int ide3d_upfirdn2d_ex(const ide3d_upfirdn2d_params* pp, const ide3d_upfirdn2d_epilogue* ep, void* stream) {
    return upfirdn2d_entry(pp, ep, stream);
}
