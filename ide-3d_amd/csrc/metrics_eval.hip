// metrics_eval.hip — the arithmetic between the networks of the remaining metrics: perceptual path length
// (metrics/perceptual_path_length.py), Inception Score (metrics/inception_score.py) and the mIoU of parser labels
// (apps/calc_losses_on_images.py).  Five entry points, all streaming reductions:
//   ide3d_ppl_prep               window + f x f area mean + affine + z-score in one pass (ide3d_lpips_prep with a window, same bits);
//   ide3d_lpips_pair_distances   per-pair LPIPS distance of images i and i + n from raw taps: per-workgroup float64 partials, one finish;
//   ide3d_trimmed_mean           two order statistics by radix select (8-bit LDS histograms) and the mean between them, one workgroup;
//   ide3d_inception_score        split-wise column means, then the KL row sums, float64 throughout;
//   ide3d_label_iou              per-class intersection and union counts of two label maps (wave ballots, integer adds) and their IoU.
// No float atomics: every floating-point sum is float64, taken in an order fixed by the launch geometry (inside a thread, across the lanes
// of a wave by butterfly, across waves and workgroups in index order), so two runs are bit-equal.  Integer counts use LDS and global
// integer adds, which commute exactly.  Lanes run along consecutive addresses; plain loads and stores; wave64.
#include "common.h"

#include <math.h>

namespace ide3d {

constexpr int kEvThreads = 256;

__device__ __forceinline__ double ev_wave_sum(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    return v;
}

// ---- ppl prep (metrics/perceptual_path_length.py:71-83) ---------------------------------------------------------------------------
// lp_prep_kernel (lpips.hip) with a window: the same sum over the block in (dy, dx) order, the same fused affine, the same z-score.
__global__ void __launch_bounds__(kEvThreads)
ppl_prep_kernel(const float* __restrict__ x, float* __restrict__ y, const float* __restrict__ mean, const float* __restrict__ stdv,
                int H, int W, int y0, int x0, int oh, int ow, int f, float in_scale, float in_shift, int64_t total) {
    const float inv_area = 1.f / (float)(f * f);
    for (int64_t i = (int64_t)blockIdx.x * kEvThreads + threadIdx.x; i < total; i += (int64_t)gridDim.x * kEvThreads) {
        const int ox = (int)(i % ow);
        const int64_t r = i / ow;
        const int oy = (int)(r % oh);
        const int64_t plane = r / oh;
        const int c = (int)(plane % 3);
        const float* __restrict__ src = x + (plane * H + y0 + (int64_t)oy * f) * W + x0 + (int64_t)ox * f;
        float acc = 0.f;
        for (int dy = 0; dy < f; ++dy)
            for (int dx = 0; dx < f; ++dx) acc += src[(int64_t)dy * W + dx];
        const float v = fmaf(acc * inv_area, in_scale, in_shift);
        y[i] = (v - mean[c]) / stdv[c];
    }
}

// ---- pair distances (perceptual_path_length.py:89) --------------------------------------------------------------------------------
// A workgroup: 64 consecutive pixels of ONE pair x 4 channel slices (wave s takes channels s, s + 4, ...), as the head of lpips.hip.
// partial[(pair * blocks + b)] = sum over its pixels of sum_c lin_c (u_i - u_{i+n})^2, u = a * (float)(1 / (sqrt(sum_c a^2) + eps)).
constexpr int kPdPixels = 64, kPdSlices = kEvThreads / 64;
constexpr double kPdEps = 1e-10;

__device__ __forceinline__ double pd_slice_sum(double v, double (*s_red)[kPdPixels]) {
    s_red[threadIdx.x >> 6][threadIdx.x & 63] = v;
    __syncthreads();
    double t = s_red[0][threadIdx.x & 63];
#pragma unroll
    for (int s = 1; s < kPdSlices; ++s) t += s_red[s][threadIdx.x & 63];
    __syncthreads();
    return t;
}

__global__ void __launch_bounds__(kEvThreads)
pair_dist_kernel(const float* __restrict__ a, const float* __restrict__ lin, double* __restrict__ partial, int C, int hw, int n, int blocks) {
    __shared__ double s_red[kPdSlices][kPdPixels];
    const int pair = blockIdx.x / blocks, b = blockIdx.x - pair * blocks;
    const int px = b * kPdPixels + (threadIdx.x & 63), slice = threadIdx.x >> 6;
    const bool valid = px < hw;
    const float* __restrict__ p0 = a + (int64_t)pair * C * hw + (valid ? px : 0);
    const float* __restrict__ p1 = p0 + (int64_t)n * C * hw;
    double q0 = 0.0, q1 = 0.0;
    if (valid)
        for (int c = slice; c < C; c += kPdSlices) {
            const double v0 = (double)p0[(int64_t)c * hw], v1 = (double)p1[(int64_t)c * hw];
            q0 = fma(v0, v0, q0); q1 = fma(v1, v1, q1);
        }
    const double n0 = pd_slice_sum(q0, s_red), n1 = pd_slice_sum(q1, s_red);
    const float inv0 = (float)(1.0 / (sqrt(n0) + kPdEps)), inv1 = (float)(1.0 / (sqrt(n1) + kPdEps));
    double acc = 0.0;
    if (valid)
        for (int c = slice; c < C; c += kPdSlices) {
            // each product rounded on its own (never contracted into the subtraction: equal images must give exactly 0)
            const double d = (double)(__fmul_rn(p0[(int64_t)c * hw], inv0) - __fmul_rn(p1[(int64_t)c * hw], inv1));
            acc = fma((double)lin[c] * d, d, acc);
        }
    double s = pd_slice_sum(acc, s_red);
    if (threadIdx.x < 64) {
        s = ev_wave_sum(s);
        if (threadIdx.x == 0) partial[blockIdx.x] = s;
    }
}

struct PdFinish { int k; int blocks[IDE3D_LPIPS_MAX_TAPS]; int64_t offset[IDE3D_LPIPS_MAX_TAPS]; double scale[IDE3D_LPIPS_MAX_TAPS]; };

// dist[i] = scale * sum over taps (in order) of (1 / (h w)) * sum of the pair's partials (lane stride, then a butterfly).  One wave per pair.
__global__ void __launch_bounds__(64)
pair_finish_kernel(const double* __restrict__ partial, PdFinish f, double scale, float* __restrict__ dist) {
    const int pair = blockIdx.x, lane = threadIdx.x;
    double acc = 0.0;
    for (int k = 0; k < f.k; ++k) {
        const double* __restrict__ src = partial + f.offset[k] + (int64_t)pair * f.blocks[k];
        double t = 0.0;
        for (int i = lane; i < f.blocks[k]; i += 64) t += src[i];
        acc = fma(ev_wave_sum(t), f.scale[k], acc);
    }
    if (lane == 0) dist[pair] = (float)(acc * scale);
}

static bool pd_taps_ok(const ide3d_lpips_tap* taps, int32_t k, int32_t n, PdFinish* f, int64_t* blocks_total) {
    if (!taps || k < 1 || k > IDE3D_LPIPS_MAX_TAPS || n < 1 || n > (1 << 20)) return false;
    int64_t total = 0;
    for (int i = 0; i < k; ++i) {
        const ide3d_lpips_tap& t = taps[i];
        if (t.c < 1 || t.h < 1 || t.w < 1) return false;
        const int64_t hw = (int64_t)t.h * t.w;
        if (hw > 0x7fffffffLL || 2 * (int64_t)n * t.c * hw > (1LL << 40)) return false;
        const int64_t blocks = cdiv64(hw, kPdPixels);
        if (blocks * n > 0x7fffffffLL) return false;
        if (f) { f->blocks[i] = (int)blocks; f->offset[i] = total; f->scale[i] = 1.0 / ((double)t.h * (double)t.w); }
        total += blocks * n;
    }
    if (f) f->k = k;
    if (blocks_total) *blocks_total = total;
    return true;
}

// ---- trimmed mean (perceptual_path_length.py:119-122) -----------------------------------------------------------------------------
// One workgroup.  key(x): the order-preserving unsigned image of the float (negative: all bits flipped; else the sign bit set).  Four passes
// over the array, most significant byte first: every element whose key agrees with the prefix found so far for the lo (hi) rank adds one
// to a 256-bin LDS histogram; wave 0 (1) scans its histogram and picks the bin that holds the rank.  A fifth pass sums, in float64, what lies
// between the two values as floats.
constexpr int kTmThreads = 1024, kTmWaves = kTmThreads / 64;

__device__ __forceinline__ unsigned tm_key(float v) {
    const unsigned u = __float_as_uint(v);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float tm_value(unsigned k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k); }

__global__ void __launch_bounds__(kTmThreads)
trimmed_mean_kernel(const float* __restrict__ x, int n, unsigned lo_rank, unsigned hi_rank, double* __restrict__ out) {
    __shared__ unsigned s_hist[2][256];
    __shared__ unsigned s_prefix[2], s_rank[2];
    __shared__ int s_nan;
    __shared__ double s_sum[kTmWaves];
    __shared__ unsigned s_cnt[kTmWaves];
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    if (tid == 0) { s_prefix[0] = s_prefix[1] = 0u; s_rank[0] = lo_rank; s_rank[1] = hi_rank; s_nan = 0; }
    for (int pass = 0; pass < 4; ++pass) {
        const int shift = 24 - 8 * pass;
        if (tid < 512) s_hist[tid >> 8][tid & 255] = 0u;
        __syncthreads();
        const unsigned pre0 = s_prefix[0], pre1 = s_prefix[1];
        const unsigned mask = pass == 0 ? 0u : (0xffffffffu << (shift + 8));
        bool nan = false;
        for (int i = tid; i < n; i += kTmThreads) {
            const float v = x[i];
            nan |= v != v;
            const unsigned k = tm_key(v), bin = (k >> shift) & 255u;
            if ((k & mask) == pre0) atomicAdd(&s_hist[0][bin], 1u);
            if ((k & mask) == pre1) atomicAdd(&s_hist[1][bin], 1u);
        }
        if (pass == 0 && nan) s_nan = 1;          // (every writer stores the same value)
        __syncthreads();
        if (wid < 2) {
            const unsigned* __restrict__ h = s_hist[wid];
            const unsigned c0 = h[4 * lane], c1 = h[4 * lane + 1], c2 = h[4 * lane + 2], c3 = h[4 * lane + 3];
            const unsigned s = c0 + c1 + c2 + c3;
            unsigned incl = s;
#pragma unroll
            for (int off = 1; off < 64; off <<= 1) { const unsigned t = __shfl_up(incl, off); if (lane >= off) incl += t; }
            const unsigned excl = incl - s, r = s_rank[wid];
            if (excl <= r && r < incl) {          // exactly one lane: the counts of the prefix sum to more than the rank
                unsigned run = excl, bin = 4 * lane;
                if (r >= run + c0) { run += c0; ++bin; if (r >= run + c1) { run += c1; ++bin; if (r >= run + c2) { run += c2; ++bin; } } }
                s_prefix[wid] |= bin << shift;
                s_rank[wid] = r - run;
            }
        }
        __syncthreads();
    }
    const float lo = tm_value(s_prefix[0]), hi = tm_value(s_prefix[1]);
    double sum = 0.0;
    unsigned cnt = 0u;
    for (int i = tid; i < n; i += kTmThreads) {
        const float v = x[i];
        if (v >= lo && v <= hi) { sum += (double)v; ++cnt; }
    }
    sum = ev_wave_sum(sum);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) cnt += __shfl_xor(cnt, off);
    if (lane == 0) { s_sum[wid] = sum; s_cnt[wid] = cnt; }
    __syncthreads();
    if (tid == 0) {
        double t = 0.0;
        unsigned c = 0u;
        for (int w = 0; w < kTmWaves; ++w) { t += s_sum[w]; c += s_cnt[w]; }
        if (s_nan) {          // numpy: percentiles of an array with a NaN are NaN, nothing compares inside them, the mean of nothing is NaN
            const double q = __longlong_as_double(0x7ff8000000000000LL);
            out[0] = q; out[1] = q; out[2] = q; out[3] = 0.0;
        } else {
            out[0] = t / (double)c; out[1] = (double)lo; out[2] = (double)hi; out[3] = (double)c;
        }
    }
}

// ---- inception score (metrics/inception_score.py:31-34) ---------------------------------------------------------------------------
// Split s holds rows [s n / S, (s + 1) n / S); chunk c of C of a split its rows [c r / C, (c + 1) r / C) (possibly none).
// 1. colsum[s, c, j] = sum of column j over the chunk's rows: a workgroup is 64 columns x 4 row slices, joined in slice order.
// 2. logm[s, j] = log(sum over chunks in order / r).
// 3. rowpart[s, c] = sum over the chunk's rows of sum_j p (log p - logm_j): one wave per row (lane stride, butterfly), rows of a wave in
//    order, the four waves in order.
// 4. kl[s] = sum over chunks in order / r.
constexpr int kIsCols = 64, kIsSlices = kEvThreads / 64, kIsMaxChunks = 256, kIsChunkRows = 32;

struct IsGeom { int n, d, S, C; int64_t stride; };

__device__ __forceinline__ void is_rows(const IsGeom& g, int s, int c, int& r0, int& r1, int& rows) {
    const int lo = (int)((int64_t)s * g.n / g.S), hi = (int)((int64_t)(s + 1) * g.n / g.S);
    rows = hi - lo;
    r0 = lo + (int)((int64_t)c * rows / g.C);
    r1 = lo + (int)((int64_t)(c + 1) * rows / g.C);
}

__global__ void __launch_bounds__(kEvThreads)
is_colsum_kernel(const float* __restrict__ p, IsGeom g, int col_tiles, double* __restrict__ colsum) {
    __shared__ double s_red[kIsSlices][kIsCols];
    int b = blockIdx.x;
    const int ct = b % col_tiles; b /= col_tiles;
    const int c = b % g.C, s = b / g.C;
    int r0, r1, rows;
    is_rows(g, s, c, r0, r1, rows);
    const int j = ct * kIsCols + (threadIdx.x & 63), slice = threadIdx.x >> 6;
    double acc = 0.0;
    if (j < g.d)
        for (int r = r0 + slice; r < r1; r += kIsSlices) acc += (double)p[(int64_t)r * g.stride + j];
    s_red[slice][threadIdx.x & 63] = acc;
    __syncthreads();
    if (threadIdx.x < 64 && j < g.d)
        colsum[((int64_t)s * g.C + c) * g.d + j] = ((s_red[0][threadIdx.x] + s_red[1][threadIdx.x]) + s_red[2][threadIdx.x]) + s_red[3][threadIdx.x];
}

__global__ void __launch_bounds__(kEvThreads)
is_logmean_kernel(const double* __restrict__ colsum, IsGeom g, double* __restrict__ logm) {
    const int64_t e = (int64_t)blockIdx.x * kEvThreads + threadIdx.x;
    if (e >= (int64_t)g.S * g.d) return;
    const int s = (int)(e / g.d), j = (int)(e - (int64_t)s * g.d);
    int r0, r1, rows;
    is_rows(g, s, 0, r0, r1, rows);
    double t = 0.0;
    for (int c = 0; c < g.C; ++c) t += colsum[((int64_t)s * g.C + c) * g.d + j];
    logm[e] = log(t / (double)rows);
}

__global__ void __launch_bounds__(kEvThreads)
is_rowsum_kernel(const float* __restrict__ p, const double* __restrict__ logm, IsGeom g, double* __restrict__ rowpart) {
    __shared__ double s_w[kIsSlices];
    const int c = blockIdx.x % g.C, s = blockIdx.x / g.C, lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    int r0, r1, rows;
    is_rows(g, s, c, r0, r1, rows);
    const double* __restrict__ lm = logm + (int64_t)s * g.d;
    double mine = 0.0;
    for (int r = r0 + wid; r < r1; r += kIsSlices) {
        const float* __restrict__ src = p + (int64_t)r * g.stride;
        double t = 0.0;
        for (int j = lane; j < g.d; j += 64) { const double v = (double)src[j]; t += v * (log(v) - lm[j]); }
        mine += ev_wave_sum(t);
    }
    if (lane == 0) s_w[wid] = mine;
    __syncthreads();
    if (threadIdx.x == 0) rowpart[blockIdx.x] = ((s_w[0] + s_w[1]) + s_w[2]) + s_w[3];
}

__global__ void __launch_bounds__(64)
is_finish_kernel(const double* __restrict__ rowpart, IsGeom g, double* __restrict__ kl) {
    const int s = blockIdx.x * 64 + threadIdx.x;
    if (s >= g.S) return;
    int r0, r1, rows;
    is_rows(g, s, 0, r0, r1, rows);
    double t = 0.0;
    for (int c = 0; c < g.C; ++c) t += rowpart[(int64_t)s * g.C + c];
    kl[s] = t / (double)rows;
}

constexpr int kIsMaxD = 8192, kIsMaxN = 1 << 22, kIsMaxSplits = 4096;

struct IsWs { int C; int64_t logm, colsum, rowpart, total; };          // byte offsets of the sections

inline bool is_ws(int64_t n, int64_t d, int64_t S, IsWs& w) {
    if (d < 1 || d > kIsMaxD || n < 1 || n > kIsMaxN || S < 1 || S > kIsMaxSplits || n < S) return false;
    const int64_t max_rows = cdiv64(n, S);
    int64_t C = cdiv64(max_rows, kIsChunkRows);
    if (C > kIsMaxChunks) C = kIsMaxChunks;
    w.C = (int)C;
    w.logm = 0;
    w.colsum = S * d * 8;
    w.rowpart = w.colsum + S * C * d * 8;
    w.total = w.rowpart + S * C * 8;
    return true;
}

// ---- label IoU (apps/calc_losses_on_images.py:28-30) ------------------------------------------------------------------------------
// grid = images x blocks.  A wave reads 64 labels of each map per step; per class two ballots count the lanes where both maps carry it and
// where either does, lane c keeps the running counts of class c.  Waves join in LDS, workgroups in device memory, with integer adds.
constexpr int kIouMaxClasses = 32, kIouMaxBlocks = 64, kIouPerBlock = kEvThreads * 16;

template <typename T>
__device__ __forceinline__ int iou_label(const T* __restrict__ src, int64_t i, const int32_t* __restrict__ remap, int n_in) {
    const long long v = (long long)src[i];
    if (remap == nullptr) return (v >= 0 && v < kIouMaxClasses) ? (int)v : -1;
    return (v >= 0 && v < n_in) ? remap[v] : -1;
}

template <typename T>
__global__ void __launch_bounds__(kEvThreads)
label_iou_kernel(const T* __restrict__ a, const T* __restrict__ b, const int32_t* __restrict__ remap, int n_in, int64_t hw, int classes,
                 int blocks, int32_t* __restrict__ counts) {
    __shared__ int s_cnt[kIouMaxClasses][2];
    const int img = blockIdx.x / blocks, blk = blockIdx.x - img * blocks, lane = threadIdx.x & 63;
    if (threadIdx.x < 2 * kIouMaxClasses) (&s_cnt[0][0])[threadIdx.x] = 0;
    __syncthreads();
    const int64_t p0 = (int64_t)blk * hw / blocks, p1 = (int64_t)(blk + 1) * hw / blocks;
    const T* __restrict__ sa = a + (int64_t)img * hw;
    const T* __restrict__ sb = b + (int64_t)img * hw;
    int inter = 0, uni = 0;
    for (int64_t base = p0 + (threadIdx.x & ~63); base < p1; base += kEvThreads) {          // wave-uniform trip count
        const int64_t i = base + lane;
        int la = -1, lb = -1;
        if (i < p1) { la = iou_label(sa, i, remap, n_in); lb = iou_label(sb, i, remap, n_in); }
        for (int c = 0; c < classes; ++c) {
            const bool ia = la == c, ib = lb == c;
            const int both = __popcll(__builtin_amdgcn_ballot_w64(ia && ib)), any = __popcll(__builtin_amdgcn_ballot_w64(ia || ib));
            if (lane == c) { inter += both; uni += any; }
        }
    }
    if (lane < classes) { atomicAdd(&s_cnt[lane][0], inter); atomicAdd(&s_cnt[lane][1], uni); }
    __syncthreads();
    if ((int)threadIdx.x < 2 * classes) {
        const int v = (&s_cnt[0][0])[threadIdx.x];
        if (v != 0) atomicAdd(&counts[(int64_t)img * classes * 2 + threadIdx.x], v);
    }
}

__global__ void __launch_bounds__(64)
label_iou_finish_kernel(const int32_t* __restrict__ counts, int n, int classes, float* __restrict__ iou) {
    const int img = blockIdx.x * 64 + threadIdx.x;
    if (img >= n) return;
    const int32_t* __restrict__ c = counts + (int64_t)img * classes * 2;
    float t = 0.f;
    for (int k = 0; k < classes; ++k) t += (float)c[2 * k] / ((float)c[2 * k + 1] + 1e-6f);
    iou[img] = t / (float)classes;
}

}  // namespace ide3d

using namespace ide3d;

extern "C" int ide3d_ppl_prep(const float* x, float* y, const float* mean, const float* std_, int32_t n, int32_t H, int32_t W, int32_t y0,
                              int32_t x0, int32_t h, int32_t w, int32_t f, float in_scale, float in_shift, void* stream) {
    IDE3D_CHECK_ARG(x && y && mean && std_, "ppl_prep: null pointer");
    IDE3D_CHECK_ARG(ptr_aligned(x, 4) && ptr_aligned(y, 4) && ptr_aligned(mean, 4) && ptr_aligned(std_, 4), "ppl_prep: pointers must be 4-byte aligned");
    IDE3D_CHECK_ARG(n >= 1 && H >= 1 && W >= 1 && (int64_t)n * 3 * H * W < (1LL << 40), "ppl_prep: x must be [n, 3, H, W] below 2^40 elements");
    IDE3D_CHECK_ARG(h >= 1 && w >= 1 && y0 >= 0 && x0 >= 0 && (int64_t)y0 + h <= H && (int64_t)x0 + w <= W,
                    "ppl_prep: the window [%d:%d+%d, %d:%d+%d] must lie inside the %d x %d image", y0, y0, h, x0, x0, w, H, W);
    IDE3D_CHECK_ARG(f >= 1 && f <= 64 && h % f == 0 && w % f == 0, "ppl_prep: an integer area factor f in 1..64 that divides the window (got %d for %d x %d)", f, h, w);
    const int64_t total = (int64_t)n * 3 * (h / f) * (w / f);
    hipLaunchKernelGGL(ppl_prep_kernel, dim3(stream_grid(total, kEvThreads)), dim3(kEvThreads), 0, (hipStream_t)stream, x, y, mean, std_, H, W, y0, x0,
                       h / f, w / f, f, in_scale, in_shift, total);
    IDE3D_CHECK_LAUNCH("ppl_prep");
    return IDE3D_OK;
}

extern "C" int64_t ide3d_lpips_pair_workspace_bytes(const ide3d_lpips_tap* taps, int32_t k, int32_t n) {
    int64_t blocks = 0;
    if (!pd_taps_ok(taps, k, n, nullptr, &blocks)) return -1;
    return blocks * (int64_t)sizeof(double);
}

extern "C" int ide3d_lpips_pair_distances(const ide3d_lpips_tap* taps, int32_t k, int32_t n, float scale, void* workspace, int64_t workspace_bytes,
                                          float* dist, void* stream) {
    PdFinish f;
    int64_t blocks = 0;
    IDE3D_CHECK_ARG(pd_taps_ok(taps, k, n, &f, &blocks), "lpips_pair_distances: 1..%d taps [2 n, c, h, w] with positive sizes, 1 <= n <= 2^20", IDE3D_LPIPS_MAX_TAPS);
    for (int i = 0; i < k; ++i)
        IDE3D_CHECK_ARG(taps[i].a && taps[i].lin && ptr_aligned(taps[i].a, 4) && ptr_aligned(taps[i].lin, 4), "lpips_pair_distances: a and lin of every tap, 4-byte aligned");
    IDE3D_CHECK_ARG(workspace && dist && ptr_aligned(dist, 4), "lpips_pair_distances: null or misaligned pointer");
    IDE3D_CHECK_ARG(ptr_aligned(workspace, 8) && workspace_bytes >= blocks * (int64_t)sizeof(double),
                    "lpips_pair_distances: workspace smaller than ide3d_lpips_pair_workspace_bytes() or not 8-byte aligned");
    const hipStream_t st = (hipStream_t)stream;
    double* const partial = static_cast<double*>(workspace);
    for (int i = 0; i < k; ++i) {
        const ide3d_lpips_tap& t = taps[i];
        hipLaunchKernelGGL(pair_dist_kernel, dim3((unsigned)((int64_t)f.blocks[i] * n)), dim3(kEvThreads), 0, st, t.a, t.lin, partial + f.offset[i], t.c, t.h * t.w,
                           (int)n, f.blocks[i]);
    }
    hipLaunchKernelGGL(pair_finish_kernel, dim3((unsigned)n), dim3(64), 0, st, (const double*)partial, f, (double)scale, dist);
    IDE3D_CHECK_LAUNCH("lpips_pair_distances");
    return IDE3D_OK;
}

extern "C" int ide3d_trimmed_mean(const float* x, int64_t n, int64_t lo_rank, int64_t hi_rank, double* out, void* stream) {
    IDE3D_CHECK_ARG(x && out && ptr_aligned(x, 4) && ptr_aligned(out, 8), "trimmed_mean: null pointer, or x not 4-byte / out not 8-byte aligned");
    IDE3D_CHECK_ARG(n >= 1 && n <= (1 << 24), "trimmed_mean: n must be 1..2^24 (got %lld)", (long long)n);
    IDE3D_CHECK_ARG(lo_rank >= 0 && lo_rank <= hi_rank && hi_rank < n, "trimmed_mean: ranks must satisfy 0 <= lo <= hi < n (got %lld, %lld, n = %lld)",
                    (long long)lo_rank, (long long)hi_rank, (long long)n);
    hipLaunchKernelGGL(trimmed_mean_kernel, dim3(1), dim3(kTmThreads), 0, (hipStream_t)stream, x, (int)n, (unsigned)lo_rank, (unsigned)hi_rank, out);
    IDE3D_CHECK_LAUNCH("trimmed_mean");
    return IDE3D_OK;
}

extern "C" int64_t ide3d_inception_score_workspace_bytes(int64_t n, int32_t d, int32_t splits) {
    IsWs w;
    return is_ws(n, d, splits, w) ? w.total : -1;
}

extern "C" int ide3d_inception_score(const float* p, int64_t n, int32_t d, int64_t row_stride, int32_t splits, void* workspace, int64_t workspace_bytes,
                                     double* kl, void* stream) {
    IsWs w;
    IDE3D_CHECK_ARG(d >= 1 && d <= kIsMaxD, "inception_score: d must be 1..%d (got %d)", kIsMaxD, d);
    IDE3D_CHECK_ARG(n >= 1 && n <= kIsMaxN, "inception_score: n must be 1..%d (got %lld)", kIsMaxN, (long long)n);
    IDE3D_CHECK_ARG(splits >= 1 && splits <= kIsMaxSplits && n >= splits, "inception_score: 1 <= splits <= min(n, %d) (got %d for n = %lld)", kIsMaxSplits, splits, (long long)n);
    IDE3D_CHECK_ARG(row_stride >= d, "inception_score: row_stride %lld is below d = %d", (long long)row_stride, d);
    IDE3D_CHECK_ARG(p && workspace && kl && ptr_aligned(p, 4) && ptr_aligned(kl, 8), "inception_score: null pointer, or p not 4-byte / kl not 8-byte aligned");
    IDE3D_CHECK_ARG(is_ws(n, d, splits, w) && workspace_bytes >= w.total && ptr_aligned(workspace, 16),
                    "inception_score: workspace smaller than ide3d_inception_score_workspace_bytes() or not 16-byte aligned");
    const hipStream_t st = (hipStream_t)stream;
    uint8_t* const ws = static_cast<uint8_t*>(workspace);
    double* const logm = reinterpret_cast<double*>(ws + w.logm);
    double* const colsum = reinterpret_cast<double*>(ws + w.colsum);
    double* const rowpart = reinterpret_cast<double*>(ws + w.rowpart);
    const IsGeom g{(int)n, (int)d, (int)splits, w.C, row_stride};
    const int col_tiles = cdiv(d, kIsCols);
    hipLaunchKernelGGL(is_colsum_kernel, dim3((unsigned)((int64_t)splits * w.C * col_tiles)), dim3(kEvThreads), 0, st, p, g, col_tiles, colsum);
    IDE3D_CHECK_LAUNCH("inception_score (column sums)");
    hipLaunchKernelGGL(is_logmean_kernel, dim3((unsigned)cdiv64((int64_t)splits * d, kEvThreads)), dim3(kEvThreads), 0, st, (const double*)colsum, g, logm);
    hipLaunchKernelGGL(is_rowsum_kernel, dim3((unsigned)(splits * w.C)), dim3(kEvThreads), 0, st, p, (const double*)logm, g, rowpart);
    hipLaunchKernelGGL(is_finish_kernel, dim3((unsigned)cdiv(splits, 64)), dim3(64), 0, st, (const double*)rowpart, g, kl);
    IDE3D_CHECK_LAUNCH("inception_score");
    return IDE3D_OK;
}

extern "C" int ide3d_label_iou(const void* a, const void* b, int32_t dtype, int32_t n, int64_t hw, const int32_t* remap, int32_t n_in, int32_t classes,
                               int32_t* counts, float* iou, void* stream) {
    IDE3D_CHECK_ARG(dtype == IDE3D_LABEL_INT64 || dtype == IDE3D_LABEL_UINT8, "label_iou: dtype must be IDE3D_LABEL_INT64 or IDE3D_LABEL_UINT8 (got %d)", dtype);
    IDE3D_CHECK_ARG(classes >= 1 && classes <= kIouMaxClasses, "label_iou: classes must be 1..%d (got %d)", kIouMaxClasses, classes);
    IDE3D_CHECK_ARG(n >= 1 && n <= (1 << 20) && hw >= 1 && hw <= 0x7fffffffLL, "label_iou: maps must be [n, hw] with 1 <= n <= 2^20, 1 <= hw < 2^31 (the counts are int32)");
    IDE3D_CHECK_ARG(a && b && counts && iou, "label_iou: null pointer");
    const uintptr_t el = dtype == IDE3D_LABEL_INT64 ? 8 : 1;
    IDE3D_CHECK_ARG(ptr_aligned(a, el) && ptr_aligned(b, el) && ptr_aligned(counts, 4) && ptr_aligned(iou, 4) && ptr_aligned(remap, 4), "label_iou: misaligned pointer");
    IDE3D_CHECK_ARG((remap == nullptr) == (n_in == 0) && n_in >= 0 && n_in <= 65536, "label_iou: a remap table needs 1 <= n_in <= 65536 entries, none needs n_in = 0");
    const hipStream_t st = (hipStream_t)stream;
    int64_t blocks = cdiv64(hw, kIouPerBlock);
    if (blocks > kIouMaxBlocks) blocks = kIouMaxBlocks;
    const hipError_t e = hipMemsetAsync(counts, 0, (size_t)n * classes * 2 * sizeof(int32_t), st);
    if (e != hipSuccess) { set_error("label_iou: %s", hipGetErrorString(e)); return IDE3D_ELAUNCH; }
    if (dtype == IDE3D_LABEL_INT64)
        hipLaunchKernelGGL(label_iou_kernel<long long>, dim3((unsigned)(blocks * n)), dim3(kEvThreads), 0, st, static_cast<const long long*>(a),
                           static_cast<const long long*>(b), remap, (int)n_in, hw, (int)classes, (int)blocks, counts);
    else
        hipLaunchKernelGGL(label_iou_kernel<uint8_t>, dim3((unsigned)(blocks * n)), dim3(kEvThreads), 0, st, static_cast<const uint8_t*>(a),
                           static_cast<const uint8_t*>(b), remap, (int)n_in, hw, (int)classes, (int)blocks, counts);
    hipLaunchKernelGGL(label_iou_finish_kernel, dim3((unsigned)cdiv(n, 64)), dim3(64), 0, st, (const int32_t*)counts, (int)n, (int)classes, iou);
    IDE3D_CHECK_LAUNCH("label_iou");
    return IDE3D_OK;
}
