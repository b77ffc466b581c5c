// noise_reg.hip — the projector's noise regulariser and noise normaliser as batched launches.
//
// A projector step regularises every trainable noise map of the synthesis network: for each map it walks an average-pool pyramid R, R/2,
// ..., 8 and adds mean(n * roll(n, 1, x))^2 + mean(n * roll(n, 1, y))^2 at every level; after the optimiser step every map is brought back
// to mean 0 and mean square 1.  As eager tensor ops that is ~10 launches per level and direction over ~50 levels.  Here every map of a call
// is one entry {pointer, side} of a table in device memory, ONE grid runs over the tiles of all maps, and the number of launches does not
// depend on the number of maps or on their sizes:
//   ide3d_noise_reg           3 launches: pool (the pyramid into the workspace), correlate (per tile and level the two partial sums, read
//                             through the workspace, so the roll neighbour across a tile seam or the map's wrap is a plain wrapped global
//                             index and no tile carries a halo), finalise (tile partials added in tile order in float64 -> the per-level
//                             means and the loss);
//   ide3d_noise_reg_backward  1 launch: per tile, from the coarsest level down, g_L = (2 m_x (left + right) + 2 m_y (up + down)) / N_L plus a
//                             quarter of the parent pixel's accumulated gradient; the upstream scalar is read on the device and multiplies
//                             the finished level-0 value once;
//   ide3d_noise_normalize     3 launches: tile sums; mean (tile partials in tile order) subtracted in place + tile sums of squares; scale.
// Tile = 64 x 64 level-0 pixels (the whole map below 64): the 8 x 8 level of a 512 map is one pixel per tile, so every level of a tile pools
// from the tile alone.  A workgroup finds its (map, tile) by walking the table (a handful of entries, uniform loads).
// Deterministic: fixed-order sums inside a workgroup, fixed-order sums across workgroups in a later launch, no atomics; bit-reproducible.
// Plain fp32 loads, stores and FMAs on the vector pipe (no packed fp32: the library is built without it).  There is no matrix loop in this
// file, so section 4.2's exclusive residency does not apply: these kernels share their CUs like every other streaming kernel here.
#include "common.h"

namespace ide3d {

constexpr int kNrThreads = 256;
constexpr int kNrTile = 64;               // level-0 pixels per tile side
constexpr int kNrMinSide = 4, kNrMaxSide = 512;
constexpr int kNrMaxMaps = 1024;
constexpr int kNrLdsFloats = 1024 + 256 + 64 + 16 + 4 + 1;          // levels 1.. of one tile

struct NrGeom { int side, tside, tiles_x, tiles, levels; };

__host__ __device__ __forceinline__ NrGeom nr_geom(int side) {
    NrGeom g;
    g.side = side;
    g.tside = side < kNrTile ? side : kNrTile;
    g.tiles_x = side / g.tside;
    g.tiles = g.tiles_x * g.tiles_x;
    g.levels = 1;
    for (int s = side; s > 8; s >>= 1) ++g.levels;                   // R, R / 2, ..., 8; one level for R <= 8
    return g;
}

// floats of levels 1 .. levels - 1 of a map (level 0 is the map itself)
__host__ __device__ __forceinline__ int nr_pyramid_floats(const NrGeom& g) {
    int f = 0;
    for (int l = 1; l < g.levels; ++l) f += (g.side >> l) * (g.side >> l);
    return f;
}

// Where workgroup `block` of the all-maps grid works, and where its map's slices start in the shared buffers.
struct NrWhere {
    NrGeom g;
    float* data;
    int tile, tile0;           // tile inside the map; index of the map's first tile in the grid
    int level0;                // index of the map's level 0 among all (map, level) pairs
    int pyr;                   // float offset of the map's level 1 in the pyramid region
    int part;                  // float offset of the map's [levels][tiles][2 sums][hi, lo] partial sums
    int elem0;                 // float offset of the map in the flat gradient
};

__device__ __forceinline__ void nr_advance(NrWhere& w) {
    w.tile0 += w.g.tiles; w.level0 += w.g.levels; w.pyr += nr_pyramid_floats(w.g); w.part += 4 * w.g.levels * w.g.tiles; w.elem0 += w.g.side * w.g.side;
}

__device__ __forceinline__ NrWhere nr_locate(const ide3d_noise_map* __restrict__ table, int k, int block) {
    NrWhere w;
    w.tile0 = w.level0 = w.pyr = w.part = w.elem0 = 0;
    for (int m = 0; m < k; ++m) {
        w.g = nr_geom(table[m].side);
        w.data = table[m].data;
        if (block < w.tile0 + w.g.tiles || m == k - 1) break;         // (the host launches exactly sum(tiles) workgroups)
        nr_advance(w);
    }
    w.tile = block - w.tile0;
    return w;
}

// level l >= 1 of a map inside the pyramid region
__device__ __forceinline__ int nr_level_offset(const NrWhere& w, int l) {
    int f = w.pyr;
    for (int j = 1; j < l; ++j) f += (w.g.side >> j) * (w.g.side >> j);
    return f;
}
// level l >= 1 of a tile inside the LDS pyramid
__device__ __forceinline__ int nr_lds_offset(const NrWhere& w, int l) {
    int f = 0;
    for (int j = 1; j < l; ++j) f += (w.g.tside >> j) * (w.g.tside >> j);
    return f;
}

// Sums of a and b over the workgroup in a fixed order (butterfly inside each wave, then the 4 waves in index order); valid in thread 0.
// Ends with a barrier, so s_red may be used again at once.  The sums are carried in float64 (a product of two fp32 values is exact there):
// a white-noise map's mean cancels to ~1/R of its terms, and the loss is only as good as what is left.
__device__ __forceinline__ void nr_block_sum2(double& a, double& b, double* s_red) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) { a += __shfl_xor(a, off); b += __shfl_xor(b, off); }
    if ((threadIdx.x & 63) == 0) { s_red[(threadIdx.x >> 6) * 2] = a; s_red[(threadIdx.x >> 6) * 2 + 1] = b; }
    __syncthreads();
    if (threadIdx.x == 0) {
        a = 0.0; b = 0.0;
        for (int i = 0; i < kNrThreads / 64; ++i) { a += s_red[i * 2]; b += s_red[i * 2 + 1]; }
    }
    __syncthreads();
}

// A float64 partial sum crosses launches as two plain fp32 words (value = hi + lo, 48 bits).
__device__ __forceinline__ void nr_store_split(float* p, double v) { const float hi = (float)v; p[0] = hi; p[1] = (float)(v - (double)hi); }
__device__ __forceinline__ double nr_load_split(const float* p) { return (double)p[0] + (double)p[1]; }

// ---- regulariser, launch 1: the average-pool pyramid of every tile -> workspace -----------------------------------------------------
__global__ void __launch_bounds__(kNrThreads)
nr_pool_kernel(const ide3d_noise_map* __restrict__ table, int k, float* __restrict__ pyramid) {
    __shared__ float s_lv[kNrLdsFloats];
    const NrWhere w = nr_locate(table, k, blockIdx.x);
    if (w.tile >= w.g.tiles || w.g.levels < 2) return;               // (uniform over the workgroup)
    const int S = w.g.side, T = w.g.tside;
    const int ty = w.tile / w.g.tiles_x, tx = w.tile % w.g.tiles_x;
    for (int l = 1; l < w.g.levels; ++l) {
        const int Tl = T >> l, Sl = S >> l;
        float* __restrict__ out = pyramid + nr_level_offset(w, l);
        float* s_out = s_lv + nr_lds_offset(w, l);
        const float* s_in = s_lv + nr_lds_offset(w, l - 1);          // (unused for l == 1)
        for (int i = threadIdx.x; i < Tl * Tl; i += kNrThreads) {
            const int y = i / Tl, x = i % Tl;
            float a, b, c, d;
            if (l == 1) {
                const float* r = w.data + (size_t)(ty * T + 2 * y) * S + tx * T + 2 * x;
                a = r[0]; b = r[1]; c = r[S]; d = r[S + 1];
            } else {
                const float* r = s_in + (2 * y) * (2 * Tl) + 2 * x;
                a = r[0]; b = r[1]; c = r[2 * Tl]; d = r[2 * Tl + 1];
            }
            const float v = ((a + b) + (c + d)) * 0.25f;
            s_out[i] = v;
            out[(size_t)(ty * Tl + y) * Sl + tx * Tl + x] = v;
        }
        __syncthreads();
    }
}

// ---- regulariser, launch 2: per (tile, level) sum n * left and sum n * up, neighbours through global memory with wrap ------------------
__global__ void __launch_bounds__(kNrThreads)
nr_corr_kernel(const ide3d_noise_map* __restrict__ table, int k, const float* __restrict__ pyramid, float* __restrict__ partial) {
    __shared__ double s_red[2 * kNrThreads / 64];
    const NrWhere w = nr_locate(table, k, blockIdx.x);
    if (w.tile >= w.g.tiles) return;                                 // (a grid larger than the table's tiles; uniform over the workgroup)
    const int S = w.g.side, T = w.g.tside;
    const int ty = w.tile / w.g.tiles_x, tx = w.tile % w.g.tiles_x;
    for (int l = 0; l < w.g.levels; ++l) {
        const int Tl = T >> l, Sl = S >> l, mask = Sl - 1;
        const float* __restrict__ A = l == 0 ? w.data : pyramid + nr_level_offset(w, l);
        double sx = 0.0, sy = 0.0;
        for (int i = threadIdx.x; i < Tl * Tl; i += kNrThreads) {
            const int y = ty * Tl + i / Tl, x = tx * Tl + i % Tl;
            const double c = (double)A[y * Sl + x];
            sx = fma(c, (double)A[y * Sl + ((x - 1) & mask)], sx);
            sy = fma(c, (double)A[((y - 1) & mask) * Sl + x], sy);
        }
        nr_block_sum2(sx, sy, s_red);
        if (threadIdx.x == 0) {
            float* o = partial + w.part + (l * w.g.tiles + w.tile) * 4;
            nr_store_split(o, sx); nr_store_split(o + 2, sy);
        }
    }
}

// ---- regulariser, launch 3: tile partials in tile order -> means[level][2], loss ---------------------------------------------------------
__global__ void __launch_bounds__(kNrThreads)
nr_final_kernel(const ide3d_noise_map* __restrict__ table, int k, const float* __restrict__ partial, float* __restrict__ means,
                float* __restrict__ loss) {
    __shared__ double s_acc[kNrThreads];
    NrWhere w;
    w.tile0 = w.level0 = w.pyr = w.part = w.elem0 = 0;
    double acc = 0.0;
    for (int m = 0; m < k; ++m) {
        w.g = nr_geom(table[m].side);
        if (m % kNrThreads == (int)threadIdx.x) {
            for (int l = 0; l < w.g.levels; ++l) {
                const float* p = partial + w.part + l * w.g.tiles * 4;
                double sx = 0.0, sy = 0.0;
                for (int t = 0; t < w.g.tiles; ++t) { sx += nr_load_split(p + t * 4); sy += nr_load_split(p + t * 4 + 2); }
                const double inv = 1.0 / ((double)(w.g.side >> l) * (double)(w.g.side >> l));
                const double mx = sx * inv, my = sy * inv;
                means[(w.level0 + l) * 2] = (float)mx;
                means[(w.level0 + l) * 2 + 1] = (float)my;
                acc += mx * mx + my * my;
            }
        }
        nr_advance(w);
    }
    s_acc[threadIdx.x] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        double t = 0.0;
        for (int i = 0; i < kNrThreads; ++i) t += s_acc[i];
        loss[0] = (float)t;
    }
}

// ---- regulariser backward: one launch, coarsest level first -----------------------------------------------------------------------------
__global__ void __launch_bounds__(kNrThreads)
nr_bwd_kernel(const ide3d_noise_map* __restrict__ table, int k, const float* __restrict__ pyramid, const float* __restrict__ means,
              const float* __restrict__ dloss, float* __restrict__ grad) {
    __shared__ float s_lv[kNrLdsFloats];
    const NrWhere w = nr_locate(table, k, blockIdx.x);
    if (w.tile >= w.g.tiles) return;                                 // (a grid larger than the table's tiles; uniform over the workgroup)
    const int S = w.g.side, T = w.g.tside;
    const int ty = w.tile / w.g.tiles_x, tx = w.tile % w.g.tiles_x;
    const float up = dloss[0];
    for (int l = w.g.levels - 1; l >= 0; --l) {
        const int Tl = T >> l, Sl = S >> l, mask = Sl - 1;
        const float* __restrict__ A = l == 0 ? w.data : pyramid + nr_level_offset(w, l);
        const float inv = 1.f / ((float)Sl * (float)Sl);                 // exact: a power of two
        const float cx = 2.f * means[(w.level0 + l) * 2] * inv, cy = 2.f * means[(w.level0 + l) * 2 + 1] * inv;
        const bool parent = l + 1 < w.g.levels;
        const float* s_par = s_lv + nr_lds_offset(w, l + 1);             // (read only with `parent`)
        float* s_out = s_lv + nr_lds_offset(w, l);                        // (written only for l >= 1)
        for (int i = threadIdx.x; i < Tl * Tl; i += kNrThreads) {
            const int ly = i / Tl, lx = i % Tl;
            const int y = ty * Tl + ly, x = tx * Tl + lx;
            float g = cx * (A[y * Sl + ((x - 1) & mask)] + A[y * Sl + ((x + 1) & mask)])
                    + cy * (A[((y - 1) & mask) * Sl + x] + A[((y + 1) & mask) * Sl + x]);
            if (parent) g = fmaf(0.25f, s_par[(ly >> 1) * (Tl >> 1) + (lx >> 1)], g);
            if (l == 0) grad[w.elem0 + y * S + x] = g * up;
            else        s_out[i] = g;
        }
        __syncthreads();
    }
}

// ---- normaliser ----------------------------------------------------------------------------------------------------------------------------
// PASS 0: partial[tile] = sum n.  PASS 1: n -= mean (the map's tile sums of pass 0 in tile order), partial2[tile] = sum n^2 of the result.
// PASS 2: n *= rsqrt(mean of squares) (tile sums of pass 1 in tile order).
template <int PASS>
__global__ void __launch_bounds__(kNrThreads)
nr_norm_kernel(const ide3d_noise_map* __restrict__ table, int k, const float* __restrict__ part_in, float* __restrict__ part_out) {
    __shared__ double s_red[2 * kNrThreads / 64];
    __shared__ float s_coef;
    const NrWhere w = nr_locate(table, k, blockIdx.x);
    if (w.tile >= w.g.tiles) return;                                 // (a grid larger than the table's tiles; uniform over the workgroup)
    const int S = w.g.side, T = w.g.tside;
    const int ty = w.tile / w.g.tiles_x, tx = w.tile % w.g.tiles_x;
    float coef = 0.f;
    if (PASS > 0) {
        if (threadIdx.x == 0) {
            double s = 0.0;
            for (int t = 0; t < w.g.tiles; ++t) s += nr_load_split(part_in + 2 * (w.tile0 + t));
            s /= (double)S * (double)S;
            s_coef = PASS == 1 ? (float)s : (float)(1.0 / sqrt(s));
        }
        __syncthreads();
        coef = s_coef;
    }
    double acc = 0.0, unused = 0.0;
    for (int i = threadIdx.x; i < T * T; i += kNrThreads) {
        float* p = w.data + (size_t)(ty * T + i / T) * S + tx * T + i % T;
        float v = *p;
        if (PASS == 0) acc += (double)v;
        if (PASS == 1) { v -= coef; *p = v; acc = fma((double)v, (double)v, acc); }
        if (PASS == 2) *p = v * coef;
    }
    if (PASS < 2) {
        nr_block_sum2(acc, unused, s_red);
        if (threadIdx.x == 0) nr_store_split(part_out + 2 * blockIdx.x, acc);
    }
}

// ---- host ------------------------------------------------------------------------------------------------------------------------------------
struct NrTotals { int64_t tiles, levels, pyramid, partial, elems; };

static bool nr_totals(const int32_t* sides, int32_t k, NrTotals& t) {
    t = NrTotals{0, 0, 0, 0, 0};
    if (!sides || k <= 0 || k > kNrMaxMaps) return false;
    for (int m = 0; m < k; ++m) {
        const int s = sides[m];
        if (s < kNrMinSide || s > kNrMaxSide || (s & (s - 1)) != 0) return false;
        const NrGeom g = nr_geom(s);
        t.tiles += g.tiles; t.levels += g.levels; t.pyramid += nr_pyramid_floats(g); t.partial += 4 * g.levels * g.tiles; t.elems += (int64_t)s * s;
    }
    return t.elems < 0x7fffffffLL;                                    // (1024 maps of 512^2 = 2^28 floats at the most)
}

}  // namespace ide3d

using namespace ide3d;

extern "C" int64_t ide3d_noise_reg_workspace_bytes(const int32_t* sides, int32_t k) {
    NrTotals t;
    if (!nr_totals(sides, k, t)) return -1;
    return (t.pyramid + t.partial) * (int64_t)sizeof(float);
}

extern "C" int ide3d_noise_reg_levels(const int32_t* sides, int32_t k) {
    NrTotals t;
    if (!nr_totals(sides, k, t)) return -1;
    return (int)t.levels;
}

extern "C" int ide3d_noise_reg(const ide3d_noise_map* table, const int32_t* sides, int32_t k, float* workspace, int64_t workspace_bytes,
                               float* means, float* loss, void* stream) {
    IDE3D_CHECK_ARG(table && sides && workspace && means && loss, "noise_reg: null pointer");
    NrTotals t;
    IDE3D_CHECK_ARG(nr_totals(sides, k, t), "noise_reg: 1..%d square maps with a power-of-two side of %d..%d", kNrMaxMaps, kNrMinSide, kNrMaxSide);
    IDE3D_CHECK_ARG(workspace_bytes >= (t.pyramid + t.partial) * (int64_t)sizeof(float), "noise_reg: workspace too small");
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)t.tiles);
    hipLaunchKernelGGL(nr_pool_kernel, grid, dim3(kNrThreads), 0, st, table, k, workspace);
    hipLaunchKernelGGL(nr_corr_kernel, grid, dim3(kNrThreads), 0, st, table, k, (const float*)workspace, workspace + t.pyramid);
    hipLaunchKernelGGL(nr_final_kernel, dim3(1), dim3(kNrThreads), 0, st, table, k, (const float*)(workspace + t.pyramid), means, loss);
    IDE3D_CHECK_LAUNCH("noise_reg");
    return IDE3D_OK;
}

extern "C" int ide3d_noise_reg_backward(const ide3d_noise_map* table, const int32_t* sides, int32_t k, const float* workspace,
                                        int64_t workspace_bytes, const float* means, const float* dloss, float* grad, void* stream) {
    IDE3D_CHECK_ARG(table && sides && workspace && means && dloss && grad, "noise_reg_backward: null pointer");
    NrTotals t;
    IDE3D_CHECK_ARG(nr_totals(sides, k, t), "noise_reg_backward: 1..%d square maps with a power-of-two side of %d..%d", kNrMaxMaps, kNrMinSide, kNrMaxSide);
    IDE3D_CHECK_ARG(workspace_bytes >= (t.pyramid + t.partial) * (int64_t)sizeof(float), "noise_reg_backward: workspace too small");
    hipLaunchKernelGGL(nr_bwd_kernel, dim3((unsigned)t.tiles), dim3(kNrThreads), 0, (hipStream_t)stream, table, k, workspace, means, dloss, grad);
    IDE3D_CHECK_LAUNCH("noise_reg_backward");
    return IDE3D_OK;
}

extern "C" int64_t ide3d_noise_normalize_workspace_bytes(const int32_t* sides, int32_t k) {
    NrTotals t;
    if (!nr_totals(sides, k, t)) return -1;
    return 4 * t.tiles * (int64_t)sizeof(float);
}

extern "C" int ide3d_noise_normalize(const ide3d_noise_map* table, const int32_t* sides, int32_t k, float* workspace, int64_t workspace_bytes,
                                     void* stream) {
    IDE3D_CHECK_ARG(table && sides && workspace, "noise_normalize: null pointer");
    NrTotals t;
    IDE3D_CHECK_ARG(nr_totals(sides, k, t), "noise_normalize: 1..%d square maps with a power-of-two side of %d..%d", kNrMaxMaps, kNrMinSide, kNrMaxSide);
    IDE3D_CHECK_ARG(workspace_bytes >= 4 * t.tiles * (int64_t)sizeof(float), "noise_normalize: workspace too small");
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)t.tiles);
    float* p1 = workspace;
    float* p2 = workspace + 2 * t.tiles;
    hipLaunchKernelGGL(nr_norm_kernel<0>, grid, dim3(kNrThreads), 0, st, table, k, (const float*)nullptr, p1);
    hipLaunchKernelGGL(nr_norm_kernel<1>, grid, dim3(kNrThreads), 0, st, table, k, (const float*)p1, p2);
    hipLaunchKernelGGL(nr_norm_kernel<2>, grid, dim3(kNrThreads), 0, st, table, k, (const float*)p2, (float*)nullptr);
    IDE3D_CHECK_LAUNCH("noise_normalize");
    return IDE3D_OK;
}
