// metrics.hip — what calc_metrics.py does with a detector's features: float64 moments for FID, and one fp32
// matrix-core "all pairs" engine with three epilogues (polynomial-kernel sums for KID, k-th-nearest-neighbour radii and manifold membership
// for precision / recall).  No epilogue writes the pair matrix out.  No float atomics: every output has one owner or is reduced from
// per-workgroup partials by a second launch in a fixed order, so two runs are bit-equal.
#include "common.h"

#include <math.h>

namespace ide3d {

// ---- float64 moments (metrics/metric_utils.py:107-122) ----------------------------------------------------------------------------
// raw_cov is cut into 64 x 64 tiles; one workgroup per tile ON OR ABOVE the diagonal, each thread a 4 x 4 block of float64 sums that starts
// from the caller's running value and takes one FMA per row in row order (the product of two fp32 values is exact in float64, only the
// additions round).  Each sum is stored to [j, k] and [k, j]: the matrix is bit-symmetric when the running buffer was.  The diagonal tiles
// also own raw_mean.
constexpr int kMomTile = 64, kMomRows = 16, kMomThreads = 256;

__global__ void __launch_bounds__(kMomThreads)
feature_moments_kernel(const float* __restrict__ x, int n, int d, int64_t stride, int tiles, double* __restrict__ mean, double* __restrict__ cov) {
    __shared__ float s_j[kMomRows][kMomTile], s_k[kMomRows][kMomTile];
    int b = blockIdx.x, tj = 0;
    while (b >= tiles - tj) { b -= tiles - tj; ++tj; }
    const int tk = tj + b;
    const bool diag = tj == tk;
    const int j0 = tj * kMomTile, k0 = tk * kMomTile;
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    double acc[4][4], ms[4];
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const int j = j0 + 4 * ty + a, k = k0 + 4 * tx + c;
            acc[a][c] = (j <= k && k < d) ? cov[(int64_t)j * d + k] : 0.0;
        }
    const bool owns_mean = diag && ty == 0;
#pragma unroll
    for (int c = 0; c < 4; ++c) ms[c] = (owns_mean && k0 + 4 * tx + c < d) ? mean[k0 + 4 * tx + c] : 0.0;
    for (int i0 = 0; i0 < n; i0 += kMomRows) {
#pragma unroll
        for (int q = 0; q < kMomRows * kMomTile / kMomThreads; ++q) {
            const int e = tid + q * kMomThreads, r = e >> 6, c = e & 63;
            const bool row_ok = i0 + r < n;
            const float* __restrict__ src = x + (int64_t)min(i0 + r, n - 1) * stride;
            s_j[r][c] = (row_ok && j0 + c < d) ? src[j0 + c] : 0.f;
            s_k[r][c] = (row_ok && k0 + c < d) ? src[k0 + c] : 0.f;
        }
        __syncthreads();
#pragma unroll 4
        for (int r = 0; r < kMomRows; ++r) {
            double av[4], bv[4];
#pragma unroll
            for (int a = 0; a < 4; ++a) { av[a] = (double)s_j[r][4 * ty + a]; bv[a] = (double)s_k[r][4 * tx + a]; }
#pragma unroll
            for (int a = 0; a < 4; ++a)
#pragma unroll
                for (int c = 0; c < 4; ++c) acc[a][c] = fma(av[a], bv[c], acc[a][c]);
            if (owns_mean) {
#pragma unroll
                for (int c = 0; c < 4; ++c) ms[c] += bv[c];
            }
        }
        __syncthreads();
    }
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const int j = j0 + 4 * ty + a, k = k0 + 4 * tx + c;
            if (j <= k && k < d) { cov[(int64_t)j * d + k] = acc[a][c]; cov[(int64_t)k * d + j] = acc[a][c]; }
        }
    if (owns_mean) {
#pragma unroll
        for (int c = 0; c < 4; ++c) if (k0 + 4 * tx + c < d) mean[k0 + 4 * tx + c] = ms[c];
    }
}

// ---- the pair engine --------------------------------------------------------------------------------------------------------------
// A[rows, d] . B[cols, d]^T, both K-contiguous, in 128 x 128 tiles by 256 threads: 32-wide K slices go through registers into LDS as
// [k][row] (row pitch 132 floats), each of the four waves owns a 64 x 64 quadrant as 2 x 2 v_mfma_f32_32x32x2f32 blocks.  The next slice is
// loaded while the current one is multiplied.  Every dot product is one chain over k = 0 .. d - 1 in order with fp32 rounding, the same for
// (a, b) and (b, a).  Rows past the end are clamped for the loads and dropped by the epilogues; k past d reads as 0.
constexpr int kPairTile = 128, kPairK = 32, kPairLd = 132, kPairThreads = 256, kPairLds = 2 * kPairK * kPairLd;
constexpr int kKnnKeep = 8;          // k + 1 <= 8 candidates per row
typedef float pair_f32x16 __attribute__((ext_vector_type(16)));

struct PairOperand {
    const float* p;
    const int32_t* idx;          // nullptr, or row indices into p (clamped into [0, limit))
    int rows, limit;             // rows of the pair matrix on this side; rows of p
    int64_t stride;
};

__device__ __forceinline__ const float* pair_row(const PairOperand& o, int row) {
    int g = min(row, o.rows - 1);
    if (o.idx) g = min(max(o.idx[g], 0), o.limit - 1);
    return o.p + (int64_t)g * o.stride;
}

__device__ __forceinline__ void pair_load(const float* const (&rp)[4], int k, int d, bool vec, float (&v)[16]) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        if (vec) {
            float4 t = make_float4(0.f, 0.f, 0.f, 0.f);
            if (k < d) t = *reinterpret_cast<const float4*>(rp[q] + k);
            v[4 * q] = t.x; v[4 * q + 1] = t.y; v[4 * q + 2] = t.z; v[4 * q + 3] = t.w;
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e) v[4 * q + e] = (k + e < d) ? rp[q][k + e] : 0.f;
        }
    }
}

// acc[i][j][e]: row = 64 wm + 32 i + 8 (e >> 2) + 4 half + (e & 3), column = 64 wn + 32 j + l32 of the tile
__device__ __forceinline__ int pair_acc_row(int wm, int i, int e, int half) { return 64 * wm + 32 * i + 8 * (e >> 2) + 4 * half + (e & 3); }

__device__ __forceinline__ void pair_tile(const PairOperand& A, int row0, const PairOperand& B, int col0, int d, bool vec, float* s_mem,
                                          pair_f32x16 (&acc)[2][2]) {
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6, half = lane >> 5, l32 = lane & 31, wm = wid >> 1, wn = wid & 1;
    const int kq = tid & 7, rb = tid >> 3;
    float* const sa = s_mem;
    float* const sb = s_mem + kPairK * kPairLd;
    const float* ra[4];
    const float* rbp[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) { ra[q] = pair_row(A, row0 + rb + 32 * q); rbp[q] = pair_row(B, col0 + rb + 32 * q); }
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;
    float av[16], bv[16];
    pair_load(ra, 4 * kq, d, vec, av);
    pair_load(rbp, 4 * kq, d, vec, bv);
    for (int kc = 0; kc < d; kc += kPairK) {
#pragma unroll
        for (int q = 0; q < 4; ++q)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                sa[(4 * kq + e) * kPairLd + rb + 32 * q] = av[4 * q + e];
                sb[(4 * kq + e) * kPairLd + rb + 32 * q] = bv[4 * q + e];
            }
        __syncthreads();
        if (kc + kPairK < d) {
            pair_load(ra, kc + kPairK + 4 * kq, d, vec, av);
            pair_load(rbp, kc + kPairK + 4 * kq, d, vec, bv);
        }
#pragma unroll
        for (int ks = 0; ks < kPairK / 2; ++ks) {
            const float* const pa = sa + (2 * ks + half) * kPairLd + 64 * wm + l32;
            const float* const pb = sb + (2 * ks + half) * kPairLd + 64 * wn + l32;
            const float a0 = pa[0], a1 = pa[32], b0 = pb[0], b1 = pb[32];
            acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b0, acc[0][0], 0, 0, 0);
            acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b1, acc[0][1], 0, 0, 0);
            acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b0, acc[1][0], 0, 0, 0);
            acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b1, acc[1][1], 0, 0, 0);
        }
        __syncthreads();
    }
}

// squared norms: float64 sums over k in a fixed order (lane stride, then a butterfly), rounded once to fp32.  One wave per row.
__global__ void __launch_bounds__(256)
row_norms_kernel(const float* __restrict__ f, int n, int d, int64_t stride, float* __restrict__ norms) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= n) return;
    const float* __restrict__ src = f + (int64_t)row * stride;
    double s = 0.0;
    for (int k = lane; k < d; k += 64) { const double v = (double)src[k]; s = fma(v, v, s); }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off);
    if (lane == 0) norms[row] = (float)s;
}

__device__ __forceinline__ float pair_d2(float na, float nb, float dot) { return fmaxf(0.f, (na + nb) - 2.f * dot); }

// ---- epilogue 1: polynomial-kernel sums (metrics/kernel_inception_distance.py:34-43) ------------------------------------------------
// grid = subsets x 3 x tiles^2.  which = 0: x.x, 1: y.y (both without the diagonal of the subset), 2: x.y.  Each workgroup writes the float64
// sum of its tile; poly_reduce_kernel adds the tiles of one sum in order.
__global__ void __launch_bounds__(kPairThreads)
poly_pair_kernel(const float* __restrict__ x, int nx, int64_t sx, const float* __restrict__ y, int ny, int64_t sy, int d,
                 const int32_t* __restrict__ xi, const int32_t* __restrict__ yi, int m, int tiles, int vec, double* __restrict__ partial) {
    __shared__ __attribute__((aligned(16))) float s_mem[kPairLds];
    __shared__ double s_red[kPairThreads / kWave];
    int b = blockIdx.x;
    const int tc = b % tiles; b /= tiles;
    const int tr = b % tiles; b /= tiles;
    const int which = b % 3, s = b / 3;
    const PairOperand X{x, xi + (int64_t)s * m, m, nx, sx}, Y{y, yi + (int64_t)s * m, m, ny, sy};
    const PairOperand& A = which == 1 ? Y : X;
    const PairOperand& B = which == 0 ? X : Y;
    pair_f32x16 acc[2][2];
    pair_tile(A, tr * kPairTile, B, tc * kPairTile, d, vec != 0, s_mem, acc);
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6, half = lane >> 5, l32 = lane & 31, wm = wid >> 1, wn = wid & 1;
    const double dd = (double)d;
    double sum = 0.0;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int r = tr * kPairTile + pair_acc_row(wm, i, e, half), c = tc * kPairTile + 64 * wn + 32 * j + l32;
                const double t = (double)acc[i][j][e] / dd + 1.0;
                if (r < m && c < m && (which == 2 || r != c)) sum += t * t * t;
            }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) sum += __shfl_xor(sum, off);
    if (lane == 0) s_red[wid] = sum;
    __syncthreads();
    if (tid == 0) partial[(int64_t)blockIdx.x] = ((s_red[0] + s_red[1]) + s_red[2]) + s_red[3];
}

__global__ void __launch_bounds__(64)
poly_reduce_kernel(const double* __restrict__ partial, int count, int per, double* __restrict__ sums) {
    const int e = blockIdx.x * 64 + threadIdx.x;
    if (e >= count) return;
    double s = 0.0;
    for (int t = 0; t < per; ++t) s += partial[(int64_t)e * per + t];
    sums[e] = s;
}

// ---- epilogue 2: k-th-nearest-neighbour radii (metrics/precision_recall.py:50-54) ---------------------------------------------------
// grid = row tiles x column splits.  A workgroup walks its range of column tiles; after each it passes the 128 x 128 squared distances
// through LDS in two halves of 64 columns, and thread t keeps the 8 smallest of row (t & 127) over the columns of half-half (t >> 7) in
// registers (sorted insertion, static indices).  The two lists of a row are merged at the end and written to the workspace;
// knn_merge_kernel merges the column splits of a row in order and takes the (k + 1)-th.
__device__ __forceinline__ void knn_insert(float (&b)[kKnnKeep], float v) {
    if (v < b[kKnnKeep - 1]) {
#pragma unroll
        for (int q = kKnnKeep - 1; q > 0; --q) b[q] = (v < b[q - 1]) ? b[q - 1] : ((v < b[q]) ? v : b[q]);
        b[0] = (v < b[0]) ? v : b[0];
    }
}

__host__ __device__ __forceinline__ int pair_splits(int row_tiles, int col_tiles) {
    int s = 1024 / row_tiles;
    if (s < 1) s = 1;
    return s < col_tiles ? s : col_tiles;
}

__global__ void __launch_bounds__(kPairThreads)
knn_pair_kernel(const float* __restrict__ f, int n, int d, int64_t stride, const float* __restrict__ norms, int row_tiles, int col_tiles, int splits,
                int vec, float* __restrict__ cand) {
    __shared__ __attribute__((aligned(16))) float s_mem[kPairLds];          // operands; then 128 x 65 distances; then 256 x 8 candidates
    const int rt = blockIdx.x % row_tiles, sp = blockIdx.x / row_tiles;
    const int ct0 = (int)((int64_t)sp * col_tiles / splits), ct1 = (int)((int64_t)(sp + 1) * col_tiles / splits);
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6, half = lane >> 5, l32 = lane & 31, wm = wid >> 1, wn = wid & 1;
    const PairOperand F{f, nullptr, n, n, stride};
    float na[2][16];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int e = 0; e < 16; ++e) na[i][e] = norms[min(rt * kPairTile + pair_acc_row(wm, i, e, half), n - 1)];
    float best[kKnnKeep];
#pragma unroll
    for (int q = 0; q < kKnnKeep; ++q) best[q] = INFINITY;
    const int my_row = tid & 127, my_half = tid >> 7;
    pair_f32x16 acc[2][2];
    for (int ct = ct0; ct < ct1; ++ct) {
        pair_tile(F, rt * kPairTile, F, ct * kPairTile, d, vec != 0, s_mem, acc);
#pragma unroll
        for (int pass = 0; pass < 2; ++pass) {
            if (wn == pass) {
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    const int gc = ct * kPairTile + 64 * wn + 32 * j + l32;
                    const float nb = norms[min(gc, n - 1)];
#pragma unroll
                    for (int i = 0; i < 2; ++i)
#pragma unroll
                        for (int e = 0; e < 16; ++e) {
                            const int r = pair_acc_row(wm, i, e, half);
                            float v = pair_d2(na[i][e], nb, acc[i][j][e]);
                            if (rt * kPairTile + r == gc) v = 0.f;
                            if (gc >= n) v = INFINITY;
                            s_mem[r * 65 + 32 * j + l32] = v;
                        }
                }
            }
            __syncthreads();
#pragma unroll 8
            for (int c = 0; c < 32; ++c) knn_insert(best, s_mem[my_row * 65 + 32 * my_half + c]);
            __syncthreads();
        }
    }
#pragma unroll
    for (int q = 0; q < kKnnKeep; ++q) s_mem[tid * kKnnKeep + q] = best[q];
    __syncthreads();
    if (tid < 128) {
#pragma unroll
        for (int q = 0; q < kKnnKeep; ++q) knn_insert(best, s_mem[(tid + 128) * kKnnKeep + q]);
        float* __restrict__ out = cand + (((int64_t)sp * row_tiles + rt) * kPairTile + tid) * kKnnKeep;
#pragma unroll
        for (int q = 0; q < kKnnKeep; ++q) out[q] = best[q];
    }
}

__global__ void __launch_bounds__(256)
knn_merge_kernel(const float* __restrict__ cand, int n, int k, int row_tiles, int splits, float* __restrict__ radii_sq) {
    const int row = blockIdx.x * 256 + threadIdx.x;
    if (row >= n) return;
    float best[kKnnKeep];
#pragma unroll
    for (int q = 0; q < kKnnKeep; ++q) best[q] = INFINITY;
    for (int sp = 0; sp < splits; ++sp) {
        const float* __restrict__ src = cand + ((int64_t)sp * row_tiles * kPairTile + row) * kKnnKeep;
#pragma unroll
        for (int q = 0; q < kKnnKeep; ++q) knn_insert(best, src[q]);
    }
    float out = best[0];
#pragma unroll
    for (int q = 1; q < kKnnKeep; ++q) if (q == k) out = best[q];
    radii_sq[row] = out;
}

// ---- epilogue 3: manifold membership (metrics/precision_recall.py:55-59) ------------------------------------------------------------
// grid = probe tiles x column splits.  Every lane ORs "d2 <= radius of the column" per row it holds; a ballot per row joins the 32 columns
// of a lane group, LDS joins the two waves that share rows, and inside_merge_kernel ORs the column splits.
__global__ void __launch_bounds__(kPairThreads)
inside_pair_kernel(const float* __restrict__ probes, int np, int64_t sp_stride, const float* __restrict__ manifold, int nm, int64_t sm_stride, int d,
                   const float* __restrict__ pnorms, const float* __restrict__ mnorms, const float* __restrict__ radii_sq, int row_tiles, int col_tiles,
                   int splits, int vec, uint8_t* __restrict__ flags) {
    __shared__ __attribute__((aligned(16))) float s_mem[kPairLds];
    __shared__ int s_flag[2][kPairTile];
    const int rt = blockIdx.x % row_tiles, sp = blockIdx.x / row_tiles;
    const int ct0 = (int)((int64_t)sp * col_tiles / splits), ct1 = (int)((int64_t)(sp + 1) * col_tiles / splits);
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6, half = lane >> 5, l32 = lane & 31, wm = wid >> 1, wn = wid & 1;
    const PairOperand P{probes, nullptr, np, np, sp_stride}, M{manifold, nullptr, nm, nm, sm_stride};
    float na[2][16];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int e = 0; e < 16; ++e) na[i][e] = pnorms[min(rt * kPairTile + pair_acc_row(wm, i, e, half), np - 1)];
    unsigned hit[2] = {0u, 0u};
    pair_f32x16 acc[2][2];
    for (int ct = ct0; ct < ct1; ++ct) {
        pair_tile(P, rt * kPairTile, M, ct * kPairTile, d, vec != 0, s_mem, acc);
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int gc = ct * kPairTile + 64 * wn + 32 * j + l32;
            const float nb = mnorms[min(gc, nm - 1)];
            const float rad = gc < nm ? radii_sq[gc] : -1.f;          // d2 >= 0: a column past the end is never a hit
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int e = 0; e < 16; ++e) hit[i] |= (pair_d2(na[i][e], nb, acc[i][j][e]) <= rad ? 1u : 0u) << e;
        }
    }
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const unsigned long long bal = __builtin_amdgcn_ballot_w64(((hit[i] >> e) & 1u) != 0u);
            if (l32 == 0) s_flag[wn][pair_acc_row(wm, i, e, half)] = (half ? (bal >> 32) : (bal & 0xffffffffull)) != 0ull;
        }
    __syncthreads();
    if (tid < kPairTile) flags[((int64_t)sp * row_tiles + rt) * kPairTile + tid] = (uint8_t)((s_flag[0][tid] | s_flag[1][tid]) != 0);
}

__global__ void __launch_bounds__(256)
inside_merge_kernel(const uint8_t* __restrict__ flags, int np, int row_tiles, int splits, uint8_t* __restrict__ inside) {
    const int row = blockIdx.x * 256 + threadIdx.x;
    if (row >= np) return;
    uint8_t any = 0;
    for (int sp = 0; sp < splits; ++sp) any |= flags[(int64_t)sp * row_tiles * kPairTile + row];
    inside[row] = any;
}

// ---- host side --------------------------------------------------------------------------------------------------------------------
constexpr int kMaxD = 8192, kMaxN = 1 << 22, kMaxK = 7, kMaxM = 4096, kMaxSubsets = 4096;
inline int64_t align16(int64_t v) { return (v + 15) / 16 * 16; }
inline bool pair_vec(const float* p, int64_t stride, int d) { return d % 4 == 0 && stride % 4 == 0 && ptr_aligned(p, 16); }

struct MetricsWs { int row_tiles, col_tiles, splits; int64_t norms_a, norms_b, body, total; };          // byte offsets of the sections

inline bool metrics_ws(int op, int64_t rows, int64_t cols, int64_t d, int64_t k_or_subsets, MetricsWs& w) {
    if (d < 1 || d > kMaxD) return false;
    if (op == IDE3D_METRICS_POLY) {
        if (rows != cols || rows < 2 || rows > kMaxM || k_or_subsets < 1 || k_or_subsets > kMaxSubsets) return false;
        w.row_tiles = w.col_tiles = cdiv((int)rows, kPairTile); w.splits = 1;
        w.norms_a = w.norms_b = w.body = 0;
        w.total = k_or_subsets * 3 * w.row_tiles * w.col_tiles * 8;
        return true;
    }
    if (rows < 1 || rows > kMaxN || cols < 1 || cols > kMaxN) return false;
    w.row_tiles = cdiv((int)rows, kPairTile); w.col_tiles = cdiv((int)cols, kPairTile); w.splits = pair_splits(w.row_tiles, w.col_tiles);
    if (op == IDE3D_METRICS_RADII) {
        if (rows != cols || k_or_subsets < 1 || k_or_subsets > kMaxK || rows <= k_or_subsets) return false;
        w.norms_a = w.norms_b = 0; w.body = align16(rows * 4);
        w.total = w.body + (int64_t)w.splits * w.row_tiles * kPairTile * kKnnKeep * 4;
        return true;
    }
    if (op == IDE3D_METRICS_INSIDE) {
        w.norms_a = 0; w.norms_b = align16(rows * 4); w.body = w.norms_b + align16(cols * 4);
        w.total = w.body + align16((int64_t)w.splits * w.row_tiles * kPairTile);
        return true;
    }
    return false;
}

}  // namespace ide3d

extern "C" int64_t ide3d_metrics_workspace_bytes(int32_t op, int64_t rows, int64_t cols, int32_t d, int32_t k_or_subsets) {
    ide3d::MetricsWs w;
    return ide3d::metrics_ws(op, rows, cols, d, k_or_subsets, w) ? w.total : -1;
}

extern "C" int ide3d_feature_moments(const float* x, int64_t n, int32_t d, int64_t row_stride, double* raw_mean, double* raw_cov, void* stream) {
    using namespace ide3d;
    IDE3D_CHECK_ARG(d >= 1 && d <= kMaxD, "feature_moments: d must be 1..%d (got %d)", kMaxD, d);
    IDE3D_CHECK_ARG(n >= 1 && n <= kMaxN, "feature_moments: n must be 1..%d (got %lld)", kMaxN, (long long)n);
    IDE3D_CHECK_ARG(row_stride >= d, "feature_moments: row_stride %lld is below d = %d", (long long)row_stride, d);
    IDE3D_CHECK_ARG(x && raw_mean && raw_cov, "feature_moments: null pointer");
    IDE3D_CHECK_ARG(ptr_aligned(x, 4) && ptr_aligned(raw_mean, 8) && ptr_aligned(raw_cov, 8), "feature_moments: x must be 4-byte, raw_mean and raw_cov 8-byte aligned");
    const int tiles = cdiv(d, kMomTile);
    hipLaunchKernelGGL(feature_moments_kernel, dim3((unsigned)(tiles * (tiles + 1) / 2)), dim3(kMomThreads), 0, (hipStream_t)stream, x, (int)n, (int)d, row_stride,
                       tiles, raw_mean, raw_cov);
    IDE3D_CHECK_LAUNCH("feature_moments");
    return IDE3D_OK;
}

extern "C" int ide3d_poly_kernel_sums(const float* x, int64_t nx, int64_t x_stride, const float* y, int64_t ny, int64_t y_stride, int32_t d,
                                      const int32_t* xi, const int32_t* yi, int32_t subsets, int32_t m, void* workspace, int64_t workspace_bytes,
                                      double* sums, void* stream) {
    using namespace ide3d;
    MetricsWs w;
    IDE3D_CHECK_ARG(d >= 1 && d <= kMaxD, "poly_kernel_sums: d must be 1..%d (got %d)", kMaxD, d);
    IDE3D_CHECK_ARG(nx >= 1 && nx <= kMaxN && ny >= 1 && ny <= kMaxN, "poly_kernel_sums: nx and ny must be 1..%d (got %lld, %lld)", kMaxN, (long long)nx, (long long)ny);
    IDE3D_CHECK_ARG(m >= 2 && m <= kMaxM, "poly_kernel_sums: m must be 2..%d (got %d)", kMaxM, m);
    IDE3D_CHECK_ARG(subsets >= 1 && subsets <= kMaxSubsets, "poly_kernel_sums: subsets must be 1..%d (got %d)", kMaxSubsets, subsets);
    IDE3D_CHECK_ARG(x_stride >= d && y_stride >= d, "poly_kernel_sums: a row stride is below d = %d", d);
    IDE3D_CHECK_ARG(x && y && xi && yi && workspace && sums, "poly_kernel_sums: null pointer");
    IDE3D_CHECK_ARG(metrics_ws(IDE3D_METRICS_POLY, m, m, d, subsets, w) && workspace_bytes >= w.total && ptr_aligned(workspace, 16) && ptr_aligned(sums, 8),
                    "poly_kernel_sums: workspace smaller than ide3d_metrics_workspace_bytes() or not 16-byte aligned, or sums not 8-byte aligned");
    const hipStream_t st = (hipStream_t)stream;
    const int tiles = w.row_tiles, per = tiles * tiles, count = subsets * 3;
    double* const partial = static_cast<double*>(workspace);
    hipLaunchKernelGGL(poly_pair_kernel, dim3((unsigned)((int64_t)count * per)), dim3(kPairThreads), 0, st, x, (int)nx, x_stride, y, (int)ny, y_stride, (int)d, xi, yi,
                       (int)m, tiles, (int)(pair_vec(x, x_stride, d) && pair_vec(y, y_stride, d)), partial);
    IDE3D_CHECK_LAUNCH("poly_kernel_sums");
    hipLaunchKernelGGL(poly_reduce_kernel, dim3((unsigned)cdiv(count, 64)), dim3(64), 0, st, partial, count, per, sums);
    IDE3D_CHECK_LAUNCH("poly_kernel_sums (reduce)");
    return IDE3D_OK;
}

extern "C" int ide3d_knn_radii(const float* f, int64_t n, int32_t d, int64_t row_stride, int32_t k, void* workspace, int64_t workspace_bytes, float* radii_sq,
                               void* stream) {
    using namespace ide3d;
    MetricsWs w;
    IDE3D_CHECK_ARG(d >= 1 && d <= kMaxD, "knn_radii: d must be 1..%d (got %d)", kMaxD, d);
    IDE3D_CHECK_ARG(n >= 1 && n <= kMaxN, "knn_radii: n must be 1..%d (got %lld)", kMaxN, (long long)n);
    IDE3D_CHECK_ARG(k >= 1 && k <= kMaxK, "knn_radii: k must be 1..%d (got %d)", kMaxK, k);
    IDE3D_CHECK_ARG(n > k, "knn_radii: %lld points have no %d-th neighbour", (long long)n, k);
    IDE3D_CHECK_ARG(row_stride >= d, "knn_radii: row_stride %lld is below d = %d", (long long)row_stride, d);
    IDE3D_CHECK_ARG(f && workspace && radii_sq, "knn_radii: null pointer");
    IDE3D_CHECK_ARG(metrics_ws(IDE3D_METRICS_RADII, n, n, d, k, w) && workspace_bytes >= w.total && ptr_aligned(workspace, 16) && ptr_aligned(radii_sq, 4),
                    "knn_radii: workspace smaller than ide3d_metrics_workspace_bytes() or not 16-byte aligned");
    const hipStream_t st = (hipStream_t)stream;
    uint8_t* const ws = static_cast<uint8_t*>(workspace);
    float* const norms = reinterpret_cast<float*>(ws);
    float* const cand = reinterpret_cast<float*>(ws + w.body);
    hipLaunchKernelGGL(row_norms_kernel, dim3((unsigned)cdiv64(n, 4)), dim3(256), 0, st, f, (int)n, (int)d, row_stride, norms);
    IDE3D_CHECK_LAUNCH("knn_radii (norms)");
    hipLaunchKernelGGL(knn_pair_kernel, dim3((unsigned)(w.row_tiles * w.splits)), dim3(kPairThreads), 0, st, f, (int)n, (int)d, row_stride, norms, w.row_tiles,
                       w.col_tiles, w.splits, (int)pair_vec(f, row_stride, d), cand);
    IDE3D_CHECK_LAUNCH("knn_radii");
    hipLaunchKernelGGL(knn_merge_kernel, dim3((unsigned)cdiv64(n, 256)), dim3(256), 0, st, cand, (int)n, (int)k, w.row_tiles, w.splits, radii_sq);
    IDE3D_CHECK_LAUNCH("knn_radii (merge)");
    return IDE3D_OK;
}

extern "C" int ide3d_manifold_inside(const float* probes, int64_t np, int64_t probe_stride, const float* manifold, int64_t nm, int64_t manifold_stride,
                                     int32_t d, const float* radii_sq, void* workspace, int64_t workspace_bytes, uint8_t* inside, void* stream) {
    using namespace ide3d;
    MetricsWs w;
    IDE3D_CHECK_ARG(d >= 1 && d <= kMaxD, "manifold_inside: d must be 1..%d (got %d)", kMaxD, d);
    IDE3D_CHECK_ARG(np >= 1 && np <= kMaxN && nm >= 1 && nm <= kMaxN, "manifold_inside: np and nm must be 1..%d (got %lld, %lld)", kMaxN, (long long)np, (long long)nm);
    IDE3D_CHECK_ARG(probe_stride >= d && manifold_stride >= d, "manifold_inside: a row stride is below d = %d", d);
    IDE3D_CHECK_ARG(probes && manifold && radii_sq && workspace && inside, "manifold_inside: null pointer");
    IDE3D_CHECK_ARG(metrics_ws(IDE3D_METRICS_INSIDE, np, nm, d, 0, w) && workspace_bytes >= w.total && ptr_aligned(workspace, 16) && ptr_aligned(radii_sq, 4),
                    "manifold_inside: workspace smaller than ide3d_metrics_workspace_bytes() or not 16-byte aligned");
    const hipStream_t st = (hipStream_t)stream;
    uint8_t* const ws = static_cast<uint8_t*>(workspace);
    float* const pnorms = reinterpret_cast<float*>(ws + w.norms_a);
    float* const mnorms = reinterpret_cast<float*>(ws + w.norms_b);
    uint8_t* const flags = ws + w.body;
    hipLaunchKernelGGL(row_norms_kernel, dim3((unsigned)cdiv64(np, 4)), dim3(256), 0, st, probes, (int)np, (int)d, probe_stride, pnorms);
    IDE3D_CHECK_LAUNCH("manifold_inside (probe norms)");
    hipLaunchKernelGGL(row_norms_kernel, dim3((unsigned)cdiv64(nm, 4)), dim3(256), 0, st, manifold, (int)nm, (int)d, manifold_stride, mnorms);
    IDE3D_CHECK_LAUNCH("manifold_inside (manifold norms)");
    hipLaunchKernelGGL(inside_pair_kernel, dim3((unsigned)(w.row_tiles * w.splits)), dim3(kPairThreads), 0, st, probes, (int)np, probe_stride, manifold, (int)nm,
                       manifold_stride, (int)d, pnorms, mnorms, radii_sq, w.row_tiles, w.col_tiles, w.splits,
                       (int)(pair_vec(probes, probe_stride, d) && pair_vec(manifold, manifold_stride, d)), flags);
    IDE3D_CHECK_LAUNCH("manifold_inside");
    hipLaunchKernelGGL(inside_merge_kernel, dim3((unsigned)cdiv64(np, 256)), dim3(256), 0, st, flags, (int)np, w.row_tiles, w.splits, inside);
    IDE3D_CHECK_LAUNCH("manifold_inside (merge)");
    return IDE3D_OK;
}
