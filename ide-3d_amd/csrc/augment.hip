// augment.hip — the geometric and colour stages of the ADA pipeline (training/augment.py:277-306, 361-371) as one tiled launch.
//
// For fixed parameters the geometric stage is a linear map of the image:
//   P[i, j] = x[r(i - my0), r(j - mx0)]                     reflect padding by the batch-wide margins (augment.py:278-291), zero outside
//   U       = P zero-inserted by 2, filtered with 2 * f      upsample2d (augment.py:295, upfirdn2d.py:313-349): pads 6 / 5, true convolution
//             U[j] = 2 * sum_k f[k] * P[(j + 5 - k) / 2]      over the k with j + 5 - k even (6 of the 12 taps)
//   S[i, j] = bilinear, zeros, sample of U at A . (j, i, 1)   affine_grid + grid_sample (augment.py:300-303) in PIXEL units: the caller folds
//                                                             lines 292-301 and the two unnormalisations into the 2 x 3 matrix A per image
//   y[o]    = sum_k f[k] * S[2 o + 1 + k]                     downsample2d, pads -1 / -1, flipped filter (augment.py:306): correlation
// A workgroup owns a 16 x 16 output tile of up to 4 channels of one image.  Its S tile is (2 * 16 + 10)^2; the window of U under it is the
// bounding box of the affine image of the tile, known only on the device (the margins are device values), so the S tile is cut into chunks
// (row bands first, halved until the windows of x, the half-filtered rows and U fit AUG_CAP floats of LDS) and the workgroup loops over them.
// Nothing but x and y is in device memory.  The colour stage (3 x 4 matrix per image) is the epilogue when the workgroup holds all channels.
// The forward kernel's window of P is not clipped to P's extent (zeros are stored outside), so its two polyphase passes read their 6 taps
// without a bound check.  The backward kernel is the transpose, step by step, with float atomic adds into a zero-filled grad_images.
#include "common.h"

namespace ide3d {
namespace {

constexpr int AUG_TS = 16;                    // output tile side
constexpr int AUG_SS = 2 * AUG_TS + 10;       // S tile side: rows 2 o + 1 .. 2 (o + 15) + 12
constexpr int AUG_NT = 12;                    // taps of the geometric low-pass filter (sym6)
constexpr int AUG_CG = 4;                     // channels per workgroup
constexpr int AUG_CAP = 13824;                // floats of LDS for the three windows of a chunk (54 KiB; 63.6 KiB per workgroup in all)
constexpr int AUG_THREADS = 256;
constexpr int AUG_MAX_SIDE = 16384;

struct AugArgs {
    const float* x;          // forward: images; backward: grad of the output
    float* y;                // forward: output; backward: grad of the images (zero-filled by the caller)
    const float* coords;     // [n, 6]: S pixel (j, i) -> U pixel (ix, iy) = (a0 j + a1 i + a2, a3 j + a4 i + a5)
    const int* margins;      // [4] on the device: mx0, my0, mx1, my1
    const float* taps;       // [12] on the device
    const float* color;      // [n, 12] rows of the 3 x 4 colour matrix, or null
    int* bands;              // counter of workgroups that looped over more than one chunk, or null
    int n, c, h, w, tiles_x, tiles_y, cgroups;
};

struct Frame {               // what a workgroup knows before its channel loop
    int n, c0, nc, oy0, ox0, th, tw, sh, sw;      // output tile and its S tile (rows 2 oy0 + 1 .. + sh)
    int mx0, my0, wp, hp, wu, hu;                 // padded and up-sampled extents
    int bh, bw;                                   // chunk of the S tile
    float a[6];
};

struct Win { int ux0, uy0, uw, uh, px0, py0, pw, ph; };

__device__ __forceinline__ int reflect(int t, int side) {
    t = t < 0 ? -t : t;
    t = t >= side ? 2 * (side - 1) - t : t;
    return min(max(t, 0), side - 1);              // one reflection suffices for margins below the side; the clamp only guards the address
}

__device__ __forceinline__ float coord(const float* a, int j, int i) { return fmaf(a[0], (float)j, fmaf(a[1], (float)i, a[2])); }

// Upper bound of a chunk's window along one axis: the box of an affine image of bw x bh samples spans |a0| (bw - 1) + |a1| (bh - 1).
__device__ __forceinline__ int span_bound(float a0, float a1, int bw, int bh, int extent) {
    const float s = fminf(fabsf(a0) * (float)(bw - 1) + fabsf(a1) * (float)(bh - 1), 1.0e6f);       // (a NaN matrix: 1e6, clipped below)
    return min((int)s + 4, extent);
}
__device__ __forceinline__ int need_floats(int uw, int uh) {
    const int pw = uw / 2 + 7, ph = uh / 2 + 7;          // (the forward kernel's window of P is not clipped to P's extent)
    return ph * pw + ph * uw + uh * uw;
}

// Row and column of flat element e = tid, tid + 256, ... of a rows x cols array without a division per element.
struct Walk { int row, col, dq, dr; };
__device__ __forceinline__ Walk walk_begin(int cols) {
    cols = max(cols, 1);
    Walk k; k.row = (int)threadIdx.x / cols; k.col = (int)threadIdx.x % cols; k.dq = AUG_THREADS / cols; k.dr = AUG_THREADS % cols;
    return k;
}
__device__ __forceinline__ void walk_next(Walk& k, int cols) {
    k.col += k.dr; k.row += k.dq;
    if (k.col >= cols) { k.col -= cols; ++k.row; }
}

// One axis of a chunk's window: U indices [lo, lo + cnt) clipped to [0, extent), P indices [plo, plo + pcnt): every P index a tap of the
// window reads, clipped to [0, pext) when clip_p (the backward kernel: nothing outside P receives a gradient), else left as it is (the
// forward kernel fills the outside with zeros and filters without bound checks).
__device__ __forceinline__ void axis_window(float c00, float c01, float c10, float c11, int extent, int pext, bool clip_p, int& lo, int& cnt, int& plo, int& pcnt) {
    float mn = fminf(fminf(c00, c01), fminf(c10, c11)), mx = fmaxf(fmaxf(c00, c01), fmaxf(c10, c11));
    mn = fminf(fmaxf(mn, -2.f), (float)extent + 1.f);
    mx = fminf(fmaxf(mx, -2.f), (float)extent + 1.f);
    const int a = max((int)floorf(mn), 0), b = min((int)floorf(mx) + 1, extent - 1);
    lo = a; cnt = max(b - a + 1, 0);
    const int pa = clip_p ? max((a - 6) >> 1, 0) : (a - 6) >> 1, pb = clip_p ? min((b + 5) >> 1, pext - 1) : (b + 5) >> 1;
    plo = pa; pcnt = cnt > 0 ? max(pb - pa + 1, 0) : 0;
}

__device__ __forceinline__ Win chunk_window(const Frame& f, int sy, int sx, int bh, int bw, bool clip_p) {
    // the coordinate is monotone in j and in i in float32 too (two fused multiply-adds), so the four corners bound every sample exactly
    const int gy0 = 2 * f.oy0 + 1 + sy, gx0 = 2 * f.ox0 + 1 + sx, gy1 = gy0 + bh - 1, gx1 = gx0 + bw - 1;
    Win w;
    axis_window(coord(f.a, gx0, gy0), coord(f.a, gx1, gy0), coord(f.a, gx0, gy1), coord(f.a, gx1, gy1), f.wu, f.wp, clip_p, w.ux0, w.uw, w.px0, w.pw);
    axis_window(coord(f.a + 3, gx0, gy0), coord(f.a + 3, gx1, gy0), coord(f.a + 3, gx0, gy1), coord(f.a + 3, gx1, gy1), f.hu, f.hp, clip_p, w.uy0, w.uh, w.py0, w.ph);
    if (w.uw == 0 || w.uh == 0 || w.pw == 0 || w.ph == 0 || w.ph * w.pw + w.ph * w.uw + w.uh * w.uw > AUG_CAP) w.uw = w.uh = w.pw = w.ph = 0;
    return w;          // (the size test cannot fail after setup()'s choice of the chunk; it keeps every LDS index in range whatever the matrix holds)
}

__device__ __forceinline__ void setup(const AugArgs& p, Frame& f, float* s_f2, float* s_f1) {
    int b = blockIdx.x;
    const int cg = b % p.cgroups; b /= p.cgroups;
    const int tx = b % p.tiles_x; b /= p.tiles_x;
    const int ty = b % p.tiles_y; b /= p.tiles_y;
    f.n = b; f.c0 = cg * AUG_CG; f.nc = min(AUG_CG, p.c - f.c0);
    f.oy0 = ty * AUG_TS; f.ox0 = tx * AUG_TS;
    f.th = min(AUG_TS, p.h - f.oy0); f.tw = min(AUG_TS, p.w - f.ox0);
    f.sh = 2 * f.th + 10; f.sw = 2 * f.tw + 10;
    f.mx0 = min(max(p.margins[0], 0), p.w - 1); f.my0 = min(max(p.margins[1], 0), p.h - 1);
    const int mx1 = min(max(p.margins[2], 0), p.w - 1), my1 = min(max(p.margins[3], 0), p.h - 1);
    f.wp = p.w + f.mx0 + mx1; f.hp = p.h + f.my0 + my1; f.wu = 2 * f.wp; f.hu = 2 * f.hp;
#pragma unroll
    for (int i = 0; i < 6; ++i) f.a[i] = p.coords[(int64_t)f.n * 6 + i];
    if (threadIdx.x < AUG_NT) { const float t = p.taps[threadIdx.x]; s_f1[threadIdx.x] = t; s_f2[threadIdx.x] = 2.f * t; }
    // chunk of the S tile: row bands first, then column pieces, halved until the bound of the three windows fits
    int bh = f.sh, bw = f.sw;
    while (need_floats(span_bound(f.a[0], f.a[1], bw, bh, f.wu), span_bound(f.a[3], f.a[4], bw, bh, f.hu)) > AUG_CAP && (bh > 1 || bw > 1)) {
        if (bh > 1) bh = (bh + 1) >> 1; else bw = (bw + 1) >> 1;
    }
    f.bh = bh; f.bw = bw;
    if ((bh < f.sh || bw < f.sw) && p.bands && threadIdx.x == 0) atomicAdd(p.bands, 1);
}

// LDS of both kernels: s_win holds x / half-filtered / U windows of one chunk, s_s the S tile, s_d the half-decimated rows.
#define AUG_LDS                                                      \
    __shared__ float s_win[AUG_CAP];                                 \
    __shared__ float s_s[AUG_SS * AUG_SS];                           \
    __shared__ float s_d[AUG_TS * AUG_SS];                           \
    __shared__ float s_f2[AUG_NT];                                   \
    __shared__ float s_f1[AUG_NT]

__global__ void __launch_bounds__(AUG_THREADS)
augment_geometric_kernel(const AugArgs p) {
    AUG_LDS;
    Frame f;
    setup(p, f, s_f2, s_f1);
    const int tid = threadIdx.x;
    const int64_t plane = (int64_t)p.h * p.w;
    const int oyl = tid / AUG_TS, oxl = tid % AUG_TS;
    const bool live = oyl < f.th && oxl < f.tw;
    float acc[AUG_CG];
#pragma unroll
    for (int c = 0; c < AUG_CG; ++c) acc[c] = 0.f;
    __syncthreads();
    float fe[6], fo[6], f1[AUG_NT];               // the taps in registers: doubled, by phase, for the up-sampling passes; plain for the decimation
#pragma unroll
    for (int k = 0; k < 6; ++k) { fe[k] = s_f2[2 * k]; fo[k] = s_f2[2 * k + 1]; }
#pragma unroll
    for (int k = 0; k < AUG_NT; ++k) f1[k] = s_f1[k];
#pragma unroll 1
    for (int c = 0; c < f.nc; ++c) {
        const float* xc = p.x + ((int64_t)f.n * p.c + f.c0 + c) * plane;
#pragma unroll 1
        for (int sy = 0; sy < f.sh; sy += f.bh) {
#pragma unroll 1
            for (int sx = 0; sx < f.sw; sx += f.bw) {
                const int bh = min(f.bh, f.sh - sy), bw = min(f.bw, f.sw - sx);
                const Win w = chunk_window(f, sy, sx, bh, bw, false);
                float* const s_x = s_win;
                float* const s_m = s_x + w.ph * w.pw;
                float* const s_u = s_m + w.ph * w.uw;
                // the window of x behind the window of P, reflect indices; zero outside P
                {
                    Walk k = walk_begin(w.pw);
                    for (int e = tid; e < w.ph * w.pw; e += AUG_THREADS, walk_next(k, w.pw)) {
                        const int i = w.py0 + k.row, j = w.px0 + k.col;
                        const float v = xc[(int64_t)reflect(i - f.my0, p.h) * p.w + reflect(j - f.mx0, p.w)];
                        s_x[e] = (i >= 0 && i < f.hp && j >= 0 && j < f.wp) ? v : 0.f;
                    }
                }
                __syncthreads();
                // rows of P up-sampled along x: the 6 taps of the phase of j, all inside the window
                {
                    Walk k = walk_begin(w.uw);
                    for (int e = tid; e < w.ph * w.uw; e += AUG_THREADS, walk_next(k, w.uw)) {
                        const int j = w.ux0 + k.col;
                        const int k0 = (j + 5) & 1;
                        const float* src = s_x + k.row * w.pw + (((j + 5 - k0) >> 1) - w.px0);
                        float v = 0.f;
#pragma unroll
                        for (int t = 0; t < 6; ++t) v = fmaf(k0 ? fo[t] : fe[t], src[-t], v);
                        s_m[e] = v;
                    }
                }
                __syncthreads();
                // ... and along y: the window of U
                {
                    Walk k = walk_begin(w.uw);
                    for (int e = tid; e < w.uh * w.uw; e += AUG_THREADS, walk_next(k, w.uw)) {
                        const int r = w.uy0 + k.row;
                        const int k0 = (r + 5) & 1;
                        const float* src = s_m + (((r + 5 - k0) >> 1) - w.py0) * w.uw + k.col;
                        float v = 0.f;
#pragma unroll
                        for (int t = 0; t < 6; ++t) v = fmaf(k0 ? fo[t] : fe[t], src[-t * w.uw], v);
                        s_u[e] = v;
                    }
                }
                __syncthreads();
                // bilinear samples of the chunk, zero outside U
                {
                    Walk k = walk_begin(bw);
                    for (int e = tid; e < bh * bw; e += AUG_THREADS, walk_next(k, bw)) {
                        const int ly = sy + k.row, lx = sx + k.col;
                        const int gy = 2 * f.oy0 + 1 + ly, gx = 2 * f.ox0 + 1 + lx;
                        const float ix = coord(f.a, gx, gy), iy = coord(f.a + 3, gx, gy);
                        float v = 0.f;
                        if (ix > -1.f && ix < (float)f.wu && iy > -1.f && iy < (float)f.hu) {           // (false for NaN)
                            const float fx0 = floorf(ix), fy0 = floorf(iy);
                            const float fx = ix - fx0, fy = iy - fy0;
                            const int x0 = (int)fx0 - w.ux0, y0 = (int)fy0 - w.uy0;
                            const bool xa = x0 >= 0 && x0 < w.uw, xb = x0 + 1 >= 0 && x0 + 1 < w.uw;
                            const bool ya = y0 >= 0 && y0 < w.uh, yb = y0 + 1 >= 0 && y0 + 1 < w.uh;
                            const float u00 = (ya && xa) ? s_u[y0 * w.uw + x0] : 0.f, u01 = (ya && xb) ? s_u[y0 * w.uw + x0 + 1] : 0.f;
                            const float u10 = (yb && xa) ? s_u[(y0 + 1) * w.uw + x0] : 0.f, u11 = (yb && xb) ? s_u[(y0 + 1) * w.uw + x0 + 1] : 0.f;
                            const float gx1 = 1.f - fx, gy1 = 1.f - fy;
                            v = gy1 * (gx1 * u00 + fx * u01) + fy * (gx1 * u10 + fx * u11);
                        }
                        s_s[ly * AUG_SS + lx] = v;
                    }
                }
                __syncthreads();
            }
        }
        // decimating filter: along y into s_d, then along x
        {
            Walk k = walk_begin(f.sw);
            for (int e = tid; e < f.th * f.sw; e += AUG_THREADS, walk_next(k, f.sw)) {
                const float* src = s_s + 2 * k.row * AUG_SS + k.col;
                float v = 0.f;
#pragma unroll
                for (int t = 0; t < AUG_NT; ++t) v = fmaf(f1[t], src[t * AUG_SS], v);
                s_d[k.row * AUG_SS + k.col] = v;
            }
        }
        __syncthreads();
        if (live) {
            float v = 0.f;
#pragma unroll
            for (int k = 0; k < AUG_NT; ++k) v = fmaf(f1[k], s_d[oyl * AUG_SS + 2 * oxl + k], v);
#pragma unroll
            for (int cc = 0; cc < AUG_CG; ++cc) if (cc == c) acc[cc] = v;
        }
        __syncthreads();
    }
    if (!live) return;
    float* yo = p.y + ((int64_t)f.n * p.c + f.c0) * plane + (int64_t)(f.oy0 + oyl) * p.w + f.ox0 + oxl;
    if (p.color) {           // the host only passes it with all (3 or 1) channels in this workgroup
        const float* m = p.color + (int64_t)f.n * 12;
        if (p.c == 3) {
#pragma unroll
            for (int r = 0; r < 3; ++r) yo[r * plane] = fmaf(m[4 * r], acc[0], fmaf(m[4 * r + 1], acc[1], fmaf(m[4 * r + 2], acc[2], m[4 * r + 3])));
        } else {
            yo[0] = fmaf(m[0], acc[0], m[3]);
        }
    } else {
#pragma unroll
        for (int cc = 0; cc < AUG_CG; ++cc) if (cc < f.nc) yo[cc * plane] = acc[cc];
    }
}

__global__ void __launch_bounds__(AUG_THREADS)
augment_geometric_backward_kernel(const AugArgs p) {
    AUG_LDS;
    Frame f;
    setup(p, f, s_f2, s_f1);
    const int tid = threadIdx.x;
    const int64_t plane = (int64_t)p.h * p.w;
    const int oyl = tid / AUG_TS, oxl = tid % AUG_TS;
    const bool live = oyl < f.th && oxl < f.tw;
    float* const s_g = s_win;                      // the 16 x 16 tile of output gradients (free until the first chunk)
    __syncthreads();
    float f2[AUG_NT], fe[6], fo[6];               // the taps in registers: doubled for the up-sampling transposes, plain by phase for the decimation's
#pragma unroll
    for (int k = 0; k < AUG_NT; ++k) f2[k] = s_f2[k];
#pragma unroll
    for (int k = 0; k < 6; ++k) { fe[k] = s_f1[2 * k]; fo[k] = s_f1[2 * k + 1]; }
#pragma unroll 1
    for (int c = 0; c < f.nc; ++c) {
        // gradient of the geometric stage's output: the colour transpose (no offset) when the colour stage ran here
        float g = 0.f;
        if (live) {
            const float* gy = p.x + ((int64_t)f.n * p.c + f.c0) * plane + (int64_t)(f.oy0 + oyl) * p.w + f.ox0 + oxl;
            if (p.color) {
                const float* m = p.color + (int64_t)f.n * 12;
                if (p.c == 3) g = fmaf(m[c], gy[0], fmaf(m[4 + c], gy[plane], m[8 + c] * gy[2 * plane]));
                else g = m[0] * gy[0];
            } else {
                g = gy[c * plane];
            }
        }
        s_g[tid] = g;
        __syncthreads();
        // transposed decimation: along x into s_d, then along y into the S tile
        {
            Walk wk = walk_begin(f.sw);
            for (int e = tid; e < f.th * f.sw; e += AUG_THREADS, walk_next(wk, f.sw)) {
                const int o = wk.row, lx = wk.col;
                float v = 0.f;
#pragma unroll
                for (int t = 0; t < 6; ++t) {
                    const int k = (lx & 1) + 2 * t, q = (lx - k) >> 1;
                    if (lx - k >= 0 && q < f.tw) v = fmaf((lx & 1) ? fo[t] : fe[t], s_g[o * AUG_TS + q], v);
                }
                s_d[o * AUG_SS + lx] = v;
            }
        }
        __syncthreads();
        {
            Walk wk = walk_begin(f.sw);
            for (int e = tid; e < f.sh * f.sw; e += AUG_THREADS, walk_next(wk, f.sw)) {
                const int ly = wk.row, lx = wk.col;
                float v = 0.f;
#pragma unroll
                for (int t = 0; t < 6; ++t) {
                    const int k = (ly & 1) + 2 * t, q = (ly - k) >> 1;
                    if (ly - k >= 0 && q < f.th) v = fmaf((ly & 1) ? fo[t] : fe[t], s_d[q * AUG_SS + lx], v);
                }
                s_s[ly * AUG_SS + lx] = v;
            }
        }
        __syncthreads();
        float* gxc = p.y + ((int64_t)f.n * p.c + f.c0 + c) * plane;
#pragma unroll 1
        for (int sy = 0; sy < f.sh; sy += f.bh) {
#pragma unroll 1
            for (int sx = 0; sx < f.sw; sx += f.bw) {
                const int bh = min(f.bh, f.sh - sy), bw = min(f.bw, f.sw - sx);
                const Win w = chunk_window(f, sy, sx, bh, bw, true);
                float* const s_m = s_win + w.ph * w.pw;          // same layout as the forward kernel; the x window's slot stays unused
                float* const s_u = s_m + w.ph * w.uw;
                for (int e = tid; e < w.uh * w.uw; e += AUG_THREADS) s_u[e] = 0.f;
                __syncthreads();
                // transposed bilinear sample: scatter into the window of U
                Walk wk = walk_begin(bw);
                for (int e = tid; e < bh * bw; e += AUG_THREADS, walk_next(wk, bw)) {
                    const int ly = sy + wk.row, lx = sx + wk.col;
                    const int gy = 2 * f.oy0 + 1 + ly, gx = 2 * f.ox0 + 1 + lx;
                    const float ix = coord(f.a, gx, gy), iy = coord(f.a + 3, gx, gy);
                    if (ix > -1.f && ix < (float)f.wu && iy > -1.f && iy < (float)f.hu) {
                        const float v = s_s[ly * AUG_SS + lx];
                        const float fx0 = floorf(ix), fy0 = floorf(iy);
                        const float fx = ix - fx0, fy = iy - fy0;
                        const int x0 = (int)fx0 - w.ux0, y0 = (int)fy0 - w.uy0;
                        const bool xa = x0 >= 0 && x0 < w.uw, xb = x0 + 1 >= 0 && x0 + 1 < w.uw;
                        const bool ya = y0 >= 0 && y0 < w.uh, yb = y0 + 1 >= 0 && y0 + 1 < w.uh;
                        const float gx1 = 1.f - fx, gy1 = 1.f - fy;
                        if (ya && xa) atomicAdd(&s_u[y0 * w.uw + x0], gy1 * gx1 * v);
                        if (ya && xb) atomicAdd(&s_u[y0 * w.uw + x0 + 1], gy1 * fx * v);
                        if (yb && xa) atomicAdd(&s_u[(y0 + 1) * w.uw + x0], fy * gx1 * v);
                        if (yb && xb) atomicAdd(&s_u[(y0 + 1) * w.uw + x0 + 1], fy * fx * v);
                    }
                }
                __syncthreads();
                // transposed up-sampling along y: P row i collects U rows 2 i + k - 5
                wk = walk_begin(w.uw);
                for (int e = tid; e < w.ph * w.uw; e += AUG_THREADS, walk_next(wk, w.uw)) {
                    const int i = w.py0 + wk.row, jj = wk.col;
                    float v = 0.f;
#pragma unroll
                    for (int k = 0; k < AUG_NT; ++k) {
                        const int r = 2 * i + k - 5 - w.uy0;
                        if (r >= 0 && r < w.uh) v = fmaf(f2[k], s_u[r * w.uw + jj], v);
                    }
                    s_m[e] = v;
                }
                __syncthreads();
                // ... along x, and the fold of the reflect padding onto the image
                wk = walk_begin(w.pw);
                for (int e = tid; e < w.ph * w.pw; e += AUG_THREADS, walk_next(wk, w.pw)) {
                    const int il = wk.row, j = w.px0 + wk.col;
                    float v = 0.f;
#pragma unroll
                    for (int k = 0; k < AUG_NT; ++k) {
                        const int q = 2 * j + k - 5 - w.ux0;
                        if (q >= 0 && q < w.uw) v = fmaf(f2[k], s_m[il * w.uw + q], v);
                    }
                    if (v != 0.f) atomicAdd(gxc + (int64_t)reflect(w.py0 + il - f.my0, p.h) * p.w + reflect(j - f.mx0, p.w), v);
                }
                __syncthreads();
            }
        }
    }
}

// out = M[:, :3] . rgb + M[:, 3] per pixel (augment.py:363-368); transpose: grad_in = M[:, :3]^T . grad_out.  One channel: row 0 only.
__global__ void __launch_bounds__(256)
augment_color_kernel(const float* x, float* y, const float* color, int c, int64_t plane, int64_t total, int transpose) {
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
        const int64_t n = e / plane, i = e % plane;
        const float* m = color + n * 12;
        const float* xp = x + n * c * plane + i;
        float* yp = y + n * c * plane + i;
        if (c == 3) {
            const float r = xp[0], g = xp[plane], b = xp[2 * plane];
#pragma unroll
            for (int k = 0; k < 3; ++k)
                yp[k * plane] = transpose ? fmaf(m[k], r, fmaf(m[4 + k], g, m[8 + k] * b)) : fmaf(m[4 * k], r, fmaf(m[4 * k + 1], g, fmaf(m[4 * k + 2], b, m[4 * k + 3])));
        } else {
            yp[0] = transpose ? m[0] * xp[0] : fmaf(m[0], xp[0], m[3]);
        }
    }
}

int check_geometric(const char* what, const void* x, const void* y, int32_t n, int32_t c, int32_t h, int32_t w, int64_t x_numel, int64_t y_numel,
                    const void* coords, const void* margins, const void* taps, const void* color) {
    IDE3D_CHECK_ARG(n >= 1 && c >= 1 && h >= 1 && w >= 1, "%s: empty axis in [%d, %d, %d, %d]", what, n, c, h, w);
    IDE3D_CHECK_ARG(h >= 2 && w >= 2, "%s: reflect padding needs a height and a width of at least 2 (got %d x %d)", what, h, w);
    IDE3D_CHECK_ARG(h <= AUG_MAX_SIDE && w <= AUG_MAX_SIDE, "%s: a side above %d (got %d x %d)", what, AUG_MAX_SIDE, h, w);
    const int64_t numel = (int64_t)n * c * h * w;
    IDE3D_CHECK_ARG(n <= 65535 && c <= 65535, "%s: n and c must be at most 65535", what);
    IDE3D_CHECK_ARG(x_numel >= numel && y_numel >= numel, "%s: buffers of %lld and %lld floats are too short for %lld", what, (long long)x_numel, (long long)y_numel,
                    (long long)numel);
    IDE3D_CHECK_ARG(x && y && coords && margins && taps, "%s: null pointer", what);
    IDE3D_CHECK_ARG(ptr_aligned(x, 4) && ptr_aligned(y, 4) && ptr_aligned(coords, 4) && ptr_aligned(margins, 4) && ptr_aligned(taps, 4) && ptr_aligned(color, 4),
                    "%s: pointers must be 4-byte aligned", what);
    IDE3D_CHECK_ARG(!color || c == 3 || c == 1, "%s: the colour stage takes 3 channels or 1 (got %d)", what, c);
    const int64_t blocks = (int64_t)n * cdiv(h, AUG_TS) * cdiv(w, AUG_TS) * cdiv(c, AUG_CG);
    IDE3D_CHECK_ARG(blocks <= 0x7fffffffll, "%s: %lld workgroups exceed one launch", what, (long long)blocks);
    return IDE3D_OK;
}

AugArgs make_args(const float* x, float* y, int32_t n, int32_t c, int32_t h, int32_t w, const float* coords, const int32_t* margins, const float* taps,
                  const float* color, int32_t* bands) {
    AugArgs a;
    a.x = x; a.y = y; a.coords = coords; a.margins = margins; a.taps = taps; a.color = color; a.bands = bands;
    a.n = n; a.c = c; a.h = h; a.w = w; a.tiles_x = cdiv(w, AUG_TS); a.tiles_y = cdiv(h, AUG_TS); a.cgroups = cdiv(c, AUG_CG);
    return a;
}

}  // namespace
}  // namespace ide3d

extern "C" int ide3d_augment_geometric(const float* x, float* y, int32_t n, int32_t c, int32_t h, int32_t w, int64_t x_numel, int64_t y_numel,
                                       const float* coords, const int32_t* margins, const float* taps, const float* color, int32_t* band_loops,
                                       void* stream) {
    using namespace ide3d;
    const int rc = check_geometric("augment_geometric", x, y, n, c, h, w, x_numel, y_numel, coords, margins, taps, color);
    if (rc != IDE3D_OK) return rc;
    const AugArgs a = make_args(x, y, n, c, h, w, coords, margins, taps, color, band_loops);
    hipLaunchKernelGGL(augment_geometric_kernel, dim3((unsigned)((int64_t)n * a.tiles_y * a.tiles_x * a.cgroups)), dim3(AUG_THREADS), 0, (hipStream_t)stream, a);
    IDE3D_CHECK_LAUNCH("augment_geometric");
    return IDE3D_OK;
}

extern "C" int ide3d_augment_geometric_backward(const float* grad_out, float* grad_images, int32_t n, int32_t c, int32_t h, int32_t w, int64_t grad_out_numel,
                                                int64_t grad_images_numel, const float* coords, const int32_t* margins, const float* taps,
                                                const float* color, void* stream) {
    using namespace ide3d;
    const int rc = check_geometric("augment_geometric_backward", grad_out, grad_images, n, c, h, w, grad_out_numel, grad_images_numel, coords, margins, taps, color);
    if (rc != IDE3D_OK) return rc;
    const AugArgs a = make_args(grad_out, grad_images, n, c, h, w, coords, margins, taps, color, nullptr);
    hipLaunchKernelGGL(augment_geometric_backward_kernel, dim3((unsigned)((int64_t)n * a.tiles_y * a.tiles_x * a.cgroups)), dim3(AUG_THREADS), 0, (hipStream_t)stream, a);
    IDE3D_CHECK_LAUNCH("augment_geometric_backward");
    return IDE3D_OK;
}

extern "C" int ide3d_augment_color(const float* x, float* y, int32_t n, int32_t c, int64_t plane, int64_t x_numel, int64_t y_numel, const float* color,
                                   int32_t transpose, void* stream) {
    using namespace ide3d;
    IDE3D_CHECK_ARG(n >= 1 && plane >= 1, "augment_color: empty axis (n = %d, pixels = %lld)", n, (long long)plane);
    IDE3D_CHECK_ARG(c == 3 || c == 1, "augment_color: images must have 3 channels or 1 (got %d)", c);
    IDE3D_CHECK_ARG(plane <= (int64_t)AUG_MAX_SIDE * AUG_MAX_SIDE && n <= 65535, "augment_color: more than %d^2 pixels or 65535 images", AUG_MAX_SIDE);
    IDE3D_CHECK_ARG(x_numel >= (int64_t)n * c * plane && y_numel >= (int64_t)n * c * plane, "augment_color: buffers too short for %lld floats", (long long)n * c * plane);
    IDE3D_CHECK_ARG(x && y && color && ptr_aligned(x, 4) && ptr_aligned(y, 4) && ptr_aligned(color, 4), "augment_color: null or misaligned pointer");
    hipLaunchKernelGGL(augment_color_kernel, dim3((unsigned)stream_grid((int64_t)n * plane, 256)), dim3(256), 0, (hipStream_t)stream, x, y, color, (int)c, plane,
                       (int64_t)n * plane, (int)transpose);
    IDE3D_CHECK_LAUNCH("augment_color");
    return IDE3D_OK;
}
