// raster.hip — triangle rasterizer for the extracted mesh: the pyrender / OpenGL step of render_mesh.py:36-61 (camera of
// render_mesh.py:48-56, one directional light at the camera pose :57, white background :47) without leaving the device (DESIGN.md
// section 5.26).  One call renders N cameras of one mesh in three launches.
//
//   project   one thread per (camera, vertex).  p_cam = R p + t with world2cam [N, 3, 4] = (R | t); d = -z_cam (view depth);
//             ndc = (f * (x, y)) / d (f_x already divided by the aspect ratio); px = ndc_x * sx + ox, py = oy - ndc_y * sy;
//             X = rint(256 px), Y = rint(256 py) as int32 (24.8 fixed point; the sample of pixel (r, c) is (256 c + 128, 256 r + 128)).
//             Every product and sum is ONE float32 operation in the order written in raster_project_kernel (no contraction), the
//             divisions are IEEE: training/mesh_render.py::project_host reproduces the integers bit for bit.
//             flags: 1 = not in front of `near` (d >= near fails, NaN included), 2 = outside the guard band |px|, |py| <= 16384
//             (with it, and H, W <= 16384, every coordinate difference is below 2^23 and every edge function below 2^47).
//             A flagged vertex has X = Y = 0.  Record: (X, Y, d, flags), 16 bytes.
//   depth     one lane per (camera, triangle) against a z-buffer [N, H, W] of uint64, cleared to all ones by the same entry point.
//             A triangle is skipped when an index is outside [0, V), when a vertex is flagged (NO clipping: a triangle that straddles
//             the near plane or leaves the guard band is dropped whole), when its doubled area A2 = (X1-X0)(Y2-Y0) - (Y1-Y0)(X2-X0) is 0,
//             or by the culling mode: the geometric normal (v1-v0) x (v2-v0) points toward the camera <=> A2 < 0 (pixel y points down).
//             Edge functions in int64, w_i = s * ((Xb-Xa)(Py-Ya) - (Yb-Ya)(Px-Xa)) over the edge a -> b opposite corner i, s = sign(A2),
//             so w0 + w1 + w2 = |A2|.  Covered <=> every w_i > 0, or w_i == 0 on a top or left edge: with (dx, dy) = s (b - a),
//             left <=> dy < 0, top <=> dy == 0 and dx > 0.  A sample on an edge shared by two triangles belongs to exactly one.
//             View depth at the sample, perspective-correct, float32: q_i = float(w_i) / d_i, depth = float(|A2|) / ((q0 + q1) + q2).
//             key = float_bits(depth) << 32 | triangle index; one no-return 64-bit unsigned atomic minimum at agent scope per covered
//             sample.  An integer minimum does not depend on the order of its operands, so the z-buffer is a function of the inputs
//             alone: two runs are bit-equal whatever the scheduling, and equal depths resolve to the lower triangle index.  (The first
//             kernel of this library that reaches its fixed-result rule through an atomic rather than by avoiding them.)
//             A lane walks its own triangle's clipped box when it holds fewer than `large_min` samples; the others are taken by the whole
//             wave, one after the other: ballot, broadcast the three records with shuffles, 64 lanes stride over the box.  Both paths
//             call the same setup / coverage / depth functions.
//   shade     one thread per pixel: unpack the winner, recompute w_i, p_i = q_i / ((q0 + q1) + q2) (perspective-correct barycentrics),
//             n = normalised sum p_i n_i (or the flat world-space face normal), turned over on a back-facing triangle when `two_sided`;
//             image = clamp(base * (ambient + diffuse * max(0, n . l)), 0, 1), base = sum p_i colour_i / 255 or base_color;
//             label = label of the corner with the largest p_i (ties: the lowest corner).  Background: depth +inf, triangle -1,
//             image bg, label -1.
//
// status word (first int32 of the workspace, cleared by `depth`): bit 0 = a triangle index was out of range, bit 1 = a triangle with a
// flagged vertex whose unflagged vertices' box meets the screen (what `validate=True` of training/mesh_render.py raises on).
#include <limits.h>
#include "common.h"
#include "knobs.h"

namespace ide3d {

constexpr int kRasterThreads = 256;
constexpr int kRasterMaxSide = 16384;
constexpr float kRasterGuard = 16384.f;
constexpr int64_t kRasterHeadBytes = 16;

struct RasterTri {
    int X0, Y0, X1, Y1, X2, Y2;
    float d0, d1, d2;
    int s;                        // sign of the doubled area
    int c0, c1, r0, r1;           // box clipped to the screen, inclusive
};

__device__ __forceinline__ int imin3(int a, int b, int c) { return min(a, min(b, c)); }
__device__ __forceinline__ int imax3(int a, int b, int c) { return max(a, max(b, c)); }

// Records (X, Y, d as bits, flags) of three unflagged vertices -> is there anything to draw?
__device__ __forceinline__ bool raster_setup(const int4 a, const int4 b, const int4 c, int cull, int H, int W, RasterTri& t) {
    t.X0 = a.x; t.Y0 = a.y; t.X1 = b.x; t.Y1 = b.y; t.X2 = c.x; t.Y2 = c.y;
    t.d0 = __int_as_float(a.z); t.d1 = __int_as_float(b.z); t.d2 = __int_as_float(c.z);
    const int64_t area2 = (int64_t)(t.X1 - t.X0) * (t.Y2 - t.Y0) - (int64_t)(t.Y1 - t.Y0) * (t.X2 - t.X0);
    t.s = area2 > 0 ? 1 : -1;
    // samples 256 k + 128 inside [min, max]
    t.c0 = max((imin3(t.X0, t.X1, t.X2) + 127) >> 8, 0);
    t.c1 = min((imax3(t.X0, t.X1, t.X2) - 128) >> 8, W - 1);
    t.r0 = max((imin3(t.Y0, t.Y1, t.Y2) + 127) >> 8, 0);
    t.r1 = min((imax3(t.Y0, t.Y1, t.Y2) - 128) >> 8, H - 1);
    if (area2 == 0) return false;
    const bool front = area2 < 0;
    if ((cull == IDE3D_RASTER_CULL_BACK && !front) || (cull == IDE3D_RASTER_CULL_FRONT && front)) return false;
    return t.c0 <= t.c1 && t.r0 <= t.r1;
}

__device__ __forceinline__ int64_t raster_edge(int s, int Xa, int Ya, int Xb, int Yb, int64_t px, int64_t py, bool& in) {
    const int dx = s * (Xb - Xa), dy = s * (Yb - Ya);
    const int64_t w = (int64_t)dx * (py - Ya) - (int64_t)dy * (px - Xa);
    in = w > 0 || (w == 0 && (dy < 0 || (dy == 0 && dx > 0)));
    return w;
}

// Edge values of the sample of pixel (r, c); returns whether the sample is covered (top-left rule).
__device__ __forceinline__ bool raster_cover(const RasterTri& t, int r, int c, int64_t& w0, int64_t& w1, int64_t& w2) {
    const int64_t px = 256ll * c + 128, py = 256ll * r + 128;
    bool i0, i1, i2;
    w0 = raster_edge(t.s, t.X1, t.Y1, t.X2, t.Y2, px, py, i0);
    w1 = raster_edge(t.s, t.X2, t.Y2, t.X0, t.Y0, px, py, i1);
    w2 = raster_edge(t.s, t.X0, t.Y0, t.X1, t.Y1, px, py, i2);
    return i0 && i1 && i2;
}

// Perspective-correct view depth; q_i = float(w_i) / d_i and their sum are returned for the barycentrics.
__device__ __forceinline__ float raster_view_depth(const RasterTri& t, int64_t w0, int64_t w1, int64_t w2, float& q0, float& q1, float& q2, float& qs) {
    q0 = __fdiv_rn((float)w0, t.d0);
    q1 = __fdiv_rn((float)w1, t.d1);
    q2 = __fdiv_rn((float)w2, t.d2);
    qs = __fadd_rn(__fadd_rn(q0, q1), q2);
    return __fdiv_rn((float)(w0 + w1 + w2), qs);
}

__device__ __forceinline__ void raster_sample(const RasterTri& t, unsigned tri, int r, int c, int W, unsigned long long* __restrict__ zbuf) {
    int64_t w0, w1, w2;
    if (!raster_cover(t, r, c, w0, w1, w2)) return;
    float q0, q1, q2, qs;
    const float depth = raster_view_depth(t, w0, w1, w2, q0, q1, q2, qs);
    const unsigned long long key = ((unsigned long long)__float_as_uint(depth) << 32) | tri;
    __hip_atomic_fetch_min(zbuf + (int64_t)r * W + c, key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__global__ void __launch_bounds__(kRasterThreads)
raster_project_kernel(const float* __restrict__ vertices, int64_t V, const float* __restrict__ world2cam, float fx, float fy, float sx, float ox,
                      float sy, float oy, float near, int4* __restrict__ records) {
    const int64_t v = (int64_t)blockIdx.x * kRasterThreads + threadIdx.x;
    if (v >= V) return;
    const int n = blockIdx.y;
    const float* const m = world2cam + n * 12;
    const float x = vertices[v * 3], y = vertices[v * 3 + 1], z = vertices[v * 3 + 2];
    float cam[3];
#pragma unroll
    for (int k = 0; k < 3; ++k)
        cam[k] = __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(m[4 * k], x), __fmul_rn(m[4 * k + 1], y)), __fmul_rn(m[4 * k + 2], z)), m[4 * k + 3]);
    const float d = -cam[2];
    int flags = d >= near ? 0 : IDE3D_RASTER_BEHIND;
    int X = 0, Y = 0;
    if (!flags) {
        const float px = __fadd_rn(__fmul_rn(__fdiv_rn(__fmul_rn(fx, cam[0]), d), sx), ox);
        const float py = __fsub_rn(oy, __fmul_rn(__fdiv_rn(__fmul_rn(fy, cam[1]), d), sy));
        if (fabsf(px) <= kRasterGuard && fabsf(py) <= kRasterGuard) {
            X = (int)rintf(__fmul_rn(px, 256.f));
            Y = (int)rintf(__fmul_rn(py, 256.f));
        } else {
            flags = IDE3D_RASTER_OUTSIDE;
        }
    }
    records[(int64_t)n * V + v] = make_int4(X, Y, __float_as_int(d), flags);
}

__global__ void __launch_bounds__(kRasterThreads)
raster_depth_kernel(const int4* __restrict__ records, const int* __restrict__ triangles, int64_t T, int64_t V, int H, int W, int cull,
                    int large_min, unsigned long long* __restrict__ zbuf, int* __restrict__ status) {
    const int n = blockIdx.y;
    records += (int64_t)n * V;
    zbuf += (int64_t)n * H * W;
    const int64_t tri = (int64_t)blockIdx.x * kRasterThreads + threadIdx.x;
    int4 a = make_int4(0, 0, 0, 0), b = a, c = a;
    RasterTri t;
    bool draw = false;
    if (tri < T) {
        const int i0 = triangles[tri * 3], i1 = triangles[tri * 3 + 1], i2 = triangles[tri * 3 + 2];
        if (i0 < 0 || i1 < 0 || i2 < 0 || i0 >= V || i1 >= V || i2 >= V) {
            atomicOr(status, IDE3D_RASTER_BAD_INDEX);
        } else {
            a = records[i0]; b = records[i1]; c = records[i2];
            if (a.w | b.w | c.w) {
                // no clipping: dropped whole.  Reported when the vertices that DO have coordinates span a box that meets the screen.
                int x0 = INT_MAX, x1 = INT_MIN, y0 = INT_MAX, y1 = INT_MIN;
                const int4 r[3] = {a, b, c};
#pragma unroll
                for (int k = 0; k < 3; ++k)
                    if (!r[k].w) { x0 = min(x0, r[k].x); x1 = max(x1, r[k].x); y0 = min(y0, r[k].y); y1 = max(y1, r[k].y); }
                if (x0 <= x1 && x1 >= 128 && x0 <= 256 * W - 128 && y1 >= 128 && y0 <= 256 * H - 128) atomicOr(status, IDE3D_RASTER_DROPPED);
            } else {
                draw = raster_setup(a, b, c, cull, H, W, t);
            }
        }
    }
    const int bw = draw ? t.c1 - t.c0 + 1 : 0, bh = draw ? t.r1 - t.r0 + 1 : 0;
    const bool large = draw && bw * bh >= large_min;
    if (draw && !large) {
        for (int r = t.r0; r <= t.r1; ++r)
            for (int col = t.c0; col <= t.c1; ++col) raster_sample(t, (unsigned)tri, r, col, W, zbuf);
    }
    // the triangles too large for one lane: the wave takes them one after the other (the loop is wave-uniform)
    unsigned long long todo = __ballot(large);
    const int lane = lane_id();
    while (todo) {
        const int src = __ffsll((long long)todo) - 1;
        todo &= todo - 1;
        const int4 ga = make_int4(__shfl(a.x, src), __shfl(a.y, src), __shfl(a.z, src), 0);
        const int4 gb = make_int4(__shfl(b.x, src), __shfl(b.y, src), __shfl(b.z, src), 0);
        const int4 gc = make_int4(__shfl(c.x, src), __shfl(c.y, src), __shfl(c.z, src), 0);
        const unsigned gtri = (unsigned)(tri - lane + src);
        RasterTri g;
        raster_setup(ga, gb, gc, cull, H, W, g);
        const int gw = g.c1 - g.c0 + 1, count = gw * (g.r1 - g.r0 + 1);
        for (int i = lane; i < count; i += kWave) {
            const int r = i / gw;
            raster_sample(g, gtri, g.r0 + r, g.c0 + (i - r * gw), W, zbuf);
        }
    }
}

struct RasterShade {
    const float* vertices; const int* triangles; const float* normals; const uint8_t* colors; const int* labels; const float* light;
    const int4* records; const unsigned long long* zbuf;
    float* depth; int* triangle; float* image; int* label;
    int64_t V;
    int H, W, two_sided;
    float ambient, diffuse, base[3], bg;
};

__global__ void __launch_bounds__(kRasterThreads)
raster_shade_kernel(const RasterShade p) {
    const int64_t hw = (int64_t)p.H * p.W;
    const int64_t pix = (int64_t)blockIdx.x * kRasterThreads + threadIdx.x;
    if (pix >= hw) return;
    const int n = blockIdx.y;
    const int r = (int)(pix / p.W), c = (int)(pix - (int64_t)r * p.W);
    const unsigned long long key = p.zbuf[n * hw + pix];
    float* const img = p.image + n * 3 * hw + pix;
    if (key == ~0ull) {
        p.depth[n * hw + pix] = __uint_as_float(0x7f800000u);
        p.triangle[n * hw + pix] = -1;
        img[0] = p.bg; img[hw] = p.bg; img[2 * hw] = p.bg;
        if (p.label) p.label[n * hw + pix] = -1;
        return;
    }
    const int tri = (int)(key & 0xffffffffu);
    const int i0 = p.triangles[(int64_t)tri * 3], i1 = p.triangles[(int64_t)tri * 3 + 1], i2 = p.triangles[(int64_t)tri * 3 + 2];
    const int4* const rec = p.records + (int64_t)n * p.V;
    RasterTri t;
    raster_setup(rec[i0], rec[i1], rec[i2], IDE3D_RASTER_CULL_NONE, p.H, p.W, t);
    int64_t w0, w1, w2;
    raster_cover(t, r, c, w0, w1, w2);
    float q0, q1, q2, qs;
    raster_view_depth(t, w0, w1, w2, q0, q1, q2, qs);
    const float b0 = __fdiv_rn(q0, qs), b1 = __fdiv_rn(q1, qs), b2 = __fdiv_rn(q2, qs);
    p.depth[n * hw + pix] = __uint_as_float((unsigned)(key >> 32));
    p.triangle[n * hw + pix] = tri;
    if (p.label) p.label[n * hw + pix] = p.labels[b2 > b0 && b2 > b1 ? i2 : b1 > b0 ? i1 : i0];
    float nn[3];
    if (p.normals) {
        const float *n0 = p.normals + (int64_t)i0 * 3, *n1 = p.normals + (int64_t)i1 * 3, *n2 = p.normals + (int64_t)i2 * 3;
#pragma unroll
        for (int k = 0; k < 3; ++k) nn[k] = __fadd_rn(__fadd_rn(__fmul_rn(b0, n0[k]), __fmul_rn(b1, n1[k])), __fmul_rn(b2, n2[k]));
    } else {
        const float *v0 = p.vertices + (int64_t)i0 * 3, *v1 = p.vertices + (int64_t)i1 * 3, *v2 = p.vertices + (int64_t)i2 * 3;
        float e1[3], e2[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) { e1[k] = __fsub_rn(v1[k], v0[k]); e2[k] = __fsub_rn(v2[k], v0[k]); }
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const int u = (k + 1) % 3, v = (k + 2) % 3;
            nn[k] = __fsub_rn(__fmul_rn(e1[u], e2[v]), __fmul_rn(e1[v], e2[u]));
        }
    }
    // sqrtf, not __fsqrt_rn: the intrinsic is the hardware's approximate root here, sqrtf is the correctly rounded one the host definition has
    const float len = sqrtf(__fadd_rn(__fadd_rn(__fmul_rn(nn[0], nn[0]), __fmul_rn(nn[1], nn[1])), __fmul_rn(nn[2], nn[2])));
    const bool turn = p.two_sided && t.s > 0;          // back-facing
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        nn[k] = len > 0.f ? __fdiv_rn(nn[k], len) : 0.f;
        if (turn) nn[k] = -nn[k];
    }
    const float* const l = p.light + n * 3;
    const float ndl = fmaxf(__fadd_rn(__fadd_rn(__fmul_rn(nn[0], l[0]), __fmul_rn(nn[1], l[1])), __fmul_rn(nn[2], l[2])), 0.f);
    const float shade = __fadd_rn(p.ambient, __fmul_rn(p.diffuse, ndl));
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        float base = p.base[k];
        if (p.colors) {
            const float c0 = (float)p.colors[(int64_t)i0 * 3 + k], c1 = (float)p.colors[(int64_t)i1 * 3 + k], c2 = (float)p.colors[(int64_t)i2 * 3 + k];
            base = __fdiv_rn(__fadd_rn(__fadd_rn(__fmul_rn(b0, c0), __fmul_rn(b1, c1)), __fmul_rn(b2, c2)), 255.f);
        }
        img[k * hw] = fminf(fmaxf(__fmul_rn(base, shade), 0.f), 1.f);
    }
}

static bool raster_shape(int32_t N, int64_t V, int32_t H, int32_t W) {
    return N >= 1 && N <= 65535 && V >= 0 && V < (1ll << 31) && H >= 1 && W >= 1 && H <= kRasterMaxSide && W <= kRasterMaxSide;
}
static int64_t raster_record_bytes(int32_t N, int64_t V) { return (int64_t)N * V * 16; }

}  // namespace ide3d

extern "C" int64_t ide3d_raster_workspace_bytes(int32_t N, int64_t V, int32_t H, int32_t W) {
    using namespace ide3d;
    if (!raster_shape(N, V, H, W)) return -1;
    return kRasterHeadBytes + raster_record_bytes(N, V) + (int64_t)N * H * W * 8;
}

#define IDE3D_RASTER_CHECK_WS(what)                                                                                                      \
    IDE3D_CHECK_ARG(raster_shape(N, V, H, W), what ": 1..65535 cameras, fewer than 2^31 vertices, images of 1..%d pixels a side", kRasterMaxSide); \
    IDE3D_CHECK_ARG(workspace && workspace_bytes >= ide3d_raster_workspace_bytes(N, V, H, W) && (reinterpret_cast<uintptr_t>(workspace) & 15) == 0, \
                    what ": workspace missing, too small or not 16-byte aligned")

extern "C" int ide3d_raster_project(const float* vertices, int64_t V, const float* world2cam, int32_t N, int32_t H, int32_t W, float fx, float fy,
                                    float sx, float ox, float sy, float oy, float near, void* workspace, int64_t workspace_bytes, void* stream) {
    using namespace ide3d;
    IDE3D_RASTER_CHECK_WS("raster_project");
    IDE3D_CHECK_ARG(world2cam && (V == 0 || vertices), "raster_project: null pointer");
    IDE3D_CHECK_ARG(near > 0.f, "raster_project: near must be positive");
    if (V == 0) return IDE3D_OK;
    int4* const records = reinterpret_cast<int4*>(static_cast<char*>(workspace) + kRasterHeadBytes);
    hipLaunchKernelGGL(raster_project_kernel, dim3((unsigned)cdiv64(V, kRasterThreads), N), dim3(kRasterThreads), 0, (hipStream_t)stream,
                       vertices, V, world2cam, fx, fy, sx, ox, sy, oy, near, records);
    IDE3D_CHECK_LAUNCH("raster_project");
    return IDE3D_OK;
}

extern "C" int ide3d_raster_depth(const int32_t* triangles, int64_t T, int64_t V, int32_t N, int32_t H, int32_t W, int32_t cull,
                                  int32_t large_min, void* workspace, int64_t workspace_bytes, void* stream) {
    using namespace ide3d;
    IDE3D_RASTER_CHECK_WS("raster_depth");
    IDE3D_CHECK_ARG(T >= 0 && T < (1ll << 31) && (T == 0 || triangles), "raster_depth: 0 <= T < 2^31 triangles (the key carries the index in 32 bits)");
    IDE3D_CHECK_ARG(cull == IDE3D_RASTER_CULL_NONE || cull == IDE3D_RASTER_CULL_BACK || cull == IDE3D_RASTER_CULL_FRONT, "raster_depth: unknown culling mode %d", cull);
    char* const base = static_cast<char*>(workspace);
    unsigned long long* const zbuf = reinterpret_cast<unsigned long long*>(base + kRasterHeadBytes + raster_record_bytes(N, V));
    hipError_t e = hipMemsetAsync(base, 0, kRasterHeadBytes, (hipStream_t)stream);
    if (e == hipSuccess) e = hipMemsetAsync(zbuf, 0xff, (size_t)N * H * W * 8, (hipStream_t)stream);
    if (e != hipSuccess) { set_error("raster_depth: clearing the z-buffer: %s", hipGetErrorString(e)); return IDE3D_ELAUNCH; }
    if (T == 0) return IDE3D_OK;
    hipLaunchKernelGGL(raster_depth_kernel, dim3((unsigned)cdiv64(T, kRasterThreads), N), dim3(kRasterThreads), 0, (hipStream_t)stream,
                       reinterpret_cast<const int4*>(base + kRasterHeadBytes), triangles, T, V, H, W, cull,
                       large_min < 0 ? kRasterLargeMin : large_min, zbuf, reinterpret_cast<int*>(base));
    IDE3D_CHECK_LAUNCH("raster_depth");
    return IDE3D_OK;
}

extern "C" int ide3d_raster_shade(const float* vertices, const int32_t* triangles, int64_t V, int32_t N, int32_t H, int32_t W,
                                  const float* normals, const uint8_t* colors, const int32_t* labels, const float* light, int32_t two_sided,
                                  float ambient, float diffuse, const float* base_color, float bg, const void* workspace, int64_t workspace_bytes,
                                  float* depth, int32_t* triangle, float* image, int32_t* label, void* stream) {
    using namespace ide3d;
    IDE3D_RASTER_CHECK_WS("raster_shade");
    IDE3D_CHECK_ARG(light && base_color && depth && triangle && image, "raster_shade: null pointer");
    IDE3D_CHECK_ARG((labels != nullptr) == (label != nullptr), "raster_shade: labels and the label output go together");
    const char* const base = static_cast<const char*>(workspace);
    RasterShade p = {};
    p.vertices = vertices; p.triangles = triangles; p.normals = normals; p.colors = colors; p.labels = labels; p.light = light;
    p.records = reinterpret_cast<const int4*>(base + kRasterHeadBytes);
    p.zbuf = reinterpret_cast<const unsigned long long*>(base + kRasterHeadBytes + raster_record_bytes(N, V));
    p.depth = depth; p.triangle = triangle; p.image = image; p.label = label;
    p.V = V; p.H = H; p.W = W; p.two_sided = two_sided ? 1 : 0;
    p.ambient = ambient; p.diffuse = diffuse; p.bg = bg;
    for (int k = 0; k < 3; ++k) p.base[k] = base_color[k];
    hipLaunchKernelGGL(raster_shade_kernel, dim3((unsigned)cdiv64((int64_t)H * W, kRasterThreads), N), dim3(kRasterThreads), 0, (hipStream_t)stream, p);
    IDE3D_CHECK_LAUNCH("raster_shade");
    return IDE3D_OK;
}
