// camera.hip — the pose helpers of training/volumetric_rendering.py as two launches.
//
// The reference builds a camera pose out of ~45 one-element tensor operations (sample_camera_positions :147-193, create_cam2world_matrix
// :195-213, LookAtPoseSampler.sample :268-295): sin / cos / clamp / cross / norm / eye / repeat / slice assignment / a 4 x 4 matmul.  On the GPU
// each of them is a launch of its own: ~0.3 ms of host time and ~0.15 ms of GPU time per pose in the drivers' per-image loops
// (gen_images.py:104-106, gen_videos.py:120-124), where a batch-1 image costs 1.3 ms.  Here: one thread per camera,
//   ide3d_sphere_points : (theta, pitch) -> clamp, [arccos(1 - 2 v / pi)], r (sin phi cos theta, cos phi, sin phi sin theta)
//   ide3d_cam2world     : forward (or look-at point) + origin -> normalise, two cross products, the assembled 4 x 4 matrix
// Every operation rounds on its own, in the reference's order (no contraction into FMAs): the results differ from the ATen chain by what
// ATen's own reduction / contraction choices differ from that, a few ulp (tests/test_gpu_ops.py: 1e-6).
#include "common.h"
#include "raymarch_ray.h"

namespace ide3d {

#pragma clang fp contract(off)

struct V3 { float x, y, z; };
__device__ __forceinline__ V3 normalized(V3 v) {                       // vectors / torch.norm(vectors, dim=-1, keepdim=True) (:21-25)
    const float n = sqrtf(v.x * v.x + v.y * v.y + v.z * v.z);
    return V3{v.x / n, v.y / n, v.z / n};
}
__device__ __forceinline__ V3 cross(V3 a, V3 b) { return V3{a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }

__global__ void __launch_bounds__(64)
sphere_points_kernel(const float* __restrict__ theta, const float* __restrict__ pitch, int n, float r, int pitch_is_v,
                     float* __restrict__ pos, float* __restrict__ phi_out) {
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= n) return;
    const float kPi = 3.14159265358979323846f;
    // torch.clamp(x, 1e-5, math.pi - 1e-5): the bounds are doubles rounded to float once
    float p = fminf(fmaxf(pitch[i], 1e-5f), (float)(3.14159265358979323846 - 1e-5));
    if (pitch[i] != pitch[i]) p = pitch[i];                           // clamp keeps NaN
    if (pitch_is_v) p = acosf(1.f - 2.f * (p * (1.f / kPi)));          // LookAtPoseSampler :284-285 (ATen divides by a host scalar as a product with its fp32 reciprocal)
    const float t = theta[i], sp = r * sinf(p);
    pos[3 * i + 0] = sp * cosf(t);
    pos[3 * i + 2] = sp * sinf(t);
    pos[3 * i + 1] = r * cosf(p);
    if (phi_out) phi_out[i] = p;
}

__global__ void __launch_bounds__(64)
cam2world_kernel(const float* __restrict__ forward, const float* __restrict__ origin, const float* __restrict__ lookat, int lookat_stride,
                 int n, float* __restrict__ out) {
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= n) return;
    const V3 o{origin[3 * i], origin[3 * i + 1], origin[3 * i + 2]};
    V3 f;
    if (lookat) {                                                      // normalize_vecs(lookat_position - origins) (:295), then the callee's own
        const float* l = lookat + (int64_t)i * lookat_stride;
        f = normalized(V3{l[0] - o.x, l[1] - o.y, l[2] - o.z});
    } else {
        f = V3{forward[3 * i], forward[3 * i + 1], forward[3 * i + 2]};
    }
    f = normalized(f);
    const V3 left = normalized(cross(V3{0.f, 1.f, 0.f}, f));
    const V3 up = normalized(cross(f, left));
    // translation @ rotation with rotation[:3, :3] = columns (-left, up, -forward): [R | origin; 0 0 0 1] for finite vectors.  The
    // reference forms it as a matrix product, whose zero factors meet every entry of a column: a degenerate forward vector (parallel
    // to the up axis: left = 0 / 0; of length zero) makes the whole column NaN, the last row included.  z* is that sum of zero products:
    // +-0 for a finite column (adding it changes nothing but the sign of a zero), NaN otherwise.
    const float zl = 0.f * left.x + 0.f * left.y + 0.f * left.z;
    const float zu = 0.f * up.x + 0.f * up.y + 0.f * up.z;
    const float zf = 0.f * f.x + 0.f * f.y + 0.f * f.z;
    float* m = out + (int64_t)i * 16;
    m[0] = -left.x + zl; m[1] = up.x + zu; m[2]  = -f.x + zf; m[3]  = o.x;
    m[4] = -left.y + zl; m[5] = up.y + zu; m[6]  = -f.y + zf; m[7]  = o.y;
    m[8] = -left.z + zl; m[9] = up.z + zu; m[10] = -f.z + zf; m[11] = o.z;
    m[12] = zl * zl;     m[13] = zu * zu;  m[14] = zf * zf;   m[15] = 1.f;
}

// The needed-cell map of the plane gate (include/ide3d_hip.h `ide3d_plane_cells`): one thread per (image, ray, step).  The sample's world
// point and tap origins are the marcher's own code (raymarch_ray.h, triplane_tap.h) at the two ends of the jitter range; a draw in between
// lands between them (the point is affine in the draw and the tap origin monotone in the point, up to a rounding the widening covers).
// The rectangle is clamped into the plane like tap_addr clamps the marcher's loads, so the border texels that a tap outside the plane
// loads with weight zero are marked too: 0 x (whatever a skipped tile's memory held) is not 0 when that is an Inf or a NaN.
// Plain byte stores of 1; lanes that store the same value to the same byte do not need to know of each other.  A workgroup is 256
// consecutive samples of one image (under three rays at 96 steps), which meet a few dozen cells between them: it marks a copy of the image's
// map in LDS (`lds_cells` = 3 * cells_h * cells_w bytes, when that fits) and then stores the set cells to memory once, 48 k stores a launch
// instead of 9 M to the same 400 cache lines (40 -> 10 us at the benchmark's size).  lds_cells == 0: every thread stores to memory itself.
__global__ void __launch_bounds__(256)
plane_cells_kernel(ide3d_render_params p, int cells_h, int cells_w, int lds_cells, uint8_t* __restrict__ cells) {
    extern __shared__ __attribute__((aligned(16))) uint8_t s_cells[];
    const int n = blockIdx.y, per_img = p.rays_per_img * p.steps;
    const int i = (int)blockIdx.x * 256 + (int)threadIdx.x;                 // sample of image n (host: per_img < 2^31)
    uint8_t* const img_cells = cells + (int64_t)n * 3 * cells_h * cells_w;
    if (lds_cells) {
        for (int k = threadIdx.x * 4; k < lds_cells; k += 1024) *reinterpret_cast<uint32_t*>(s_cells + k) = 0u;   // (lds_cells % 4 == 0: host)
        __syncthreads();
    }
    if (i < per_img) {
        const int s = i % p.steps, r = i / p.steps;
        const float zstep = (p.steps > 1) ? (p.z_lin[1] - p.z_lin[0]) : 0.f;
        const float zl = p.z_lin[s];
        float ax, ay, az, bx, by, bz;
        ray_world_point(p, n, r, zl, 0.f, zstep, ax, ay, az);          // (p.jitter is set: the call may jitter)
        ray_world_point(p, n, r, zl, 1.f, zstep, bx, by, bz);
        Tap2 ta[3], tb[3];
        triplane_taps(ax, ay, az, p.W, p.H, ta);
        triplane_taps(bx, by, bz, p.W, p.H, tb);
        uint8_t* const dst = lds_cells ? s_cells : img_cells;
#pragma unroll
        for (int pl = 0; pl < 3; ++pl) {
            // taps ix0, ix0 + 1 of both ends, one texel more on every side; make_tap saturates ix0 into [-2, W + 1]
            const int x_lo = min(max(min(ta[pl].ix0, tb[pl].ix0) - 1, 0), p.W - 1), x_hi = min(max(max(ta[pl].ix0, tb[pl].ix0) + 2, 0), p.W - 1);
            const int y_lo = min(max(min(ta[pl].iy0, tb[pl].iy0) - 1, 0), p.H - 1), y_hi = min(max(max(ta[pl].iy0, tb[pl].iy0) + 2, 0), p.H - 1);
            uint8_t* const c = dst + pl * cells_h * cells_w;
            for (int cy = y_lo >> 2; cy <= (y_hi >> 2); ++cy)
                for (int cx = x_lo >> 2; cx <= (x_hi >> 2); ++cx) c[cy * cells_w + cx] = 1;
        }
    }
    if (lds_cells) {
        __syncthreads();
        for (int k = threadIdx.x * 4; k < lds_cells; k += 1024) {
            const uint32_t v = *reinterpret_cast<const uint32_t*>(s_cells + k);
            if (v == 0u) continue;
#pragma unroll
            for (int e = 0; e < 4; ++e) if ((v >> (8 * e)) & 0xffu) img_cells[k + e] = 1;
        }
    }
}

// ide3d_plane_tile_list: one workgroup walks the tiles 1024 at a time and appends the live ones in order (ballot + prefix of the 16 waves).
__global__ void __launch_bounds__(1024)
plane_tile_list_kernel(ide3d_plane_gate g, int n, int tiles_y, int tiles_x, int th, int tw, int32_t* __restrict__ list) {
    __shared__ int s_wave[16];
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int total = n * tiles_y * tiles_x;
    int base = 0;
    for (int t0 = 0; t0 < total; t0 += 1024) {
        const int t = t0 + tid;
        bool live = false;
        if (t < total) {
            const int tx = t % tiles_x, ty = (t / tiles_x) % tiles_y, img = t / (tiles_x * tiles_y);
            const int cy0 = (ty * th) >> 2, cy1 = min((ty * th + th - 1) >> 2, g.cells_h - 1);
            const int cx0 = (tx * tw) >> 2, cx1 = min((tx * tw + tw - 1) >> 2, g.cells_w - 1);
            for (int pl = 0; pl < 3; ++pl)
                for (int cy = cy0; cy <= cy1; ++cy)
                    for (int cx = cx0; cx <= cx1; ++cx) live |= g.cells[(((int64_t)img * 3 + pl) * g.cells_h + cy) * g.cells_w + cx] != 0;
        }
        const unsigned long long bal = __builtin_amdgcn_ballot_w64(live);
        if (lane == 0) s_wave[wid] = __popcll(bal);
        __syncthreads();
        int before = base;
        for (int w = 0; w < wid; ++w) before += s_wave[w];
        if (live) list[1 + before + __popcll(bal & ((1ull << lane) - 1ull))] = t;
        for (int w = 0; w < 16; ++w) base += s_wave[w];
        __syncthreads();
    }
    if (tid == 0) list[0] = base;
}

}  // namespace ide3d

extern "C" int ide3d_plane_cells(const float* rays_d_cam, const float* z_lin, const float* cam2world, int32_t n, int32_t rays_per_img,
                                 int32_t steps, int32_t H, int32_t W, uint8_t* cells, void* stream) {
    using namespace ide3d;
    IDE3D_CHECK_ARG(rays_d_cam && z_lin && cam2world && cells, "plane_cells: null pointer");
    IDE3D_CHECK_ARG(n > 0 && rays_per_img > 0 && steps > 0 && H > 0 && W > 0, "plane_cells: bad shape");
    const int cells_h = cdiv(H, 4), cells_w = cdiv(W, 4);
    const int64_t per_img = (int64_t)rays_per_img * steps, map_bytes = 3 * (int64_t)cells_h * cells_w;
    IDE3D_CHECK_ARG(per_img < 0x7fffff00LL && n <= 65535 && n * map_bytes < 0x7fffffffLL, "plane_cells: too many samples, images or cells");
    ide3d_render_params p{};
    p.rays_d_cam = rays_d_cam; p.z_lin = z_lin; p.cam2world = cam2world;
    p.jitter = z_lin;                                   // a flag for ray_world_point only: the draws are the kernel's own 0 and 1
    p.n = n; p.rays_per_img = rays_per_img; p.steps = steps; p.H = H; p.W = W;
    hipStream_t st = (hipStream_t)stream;
    const hipError_t e = hipMemsetAsync(cells, 0, (size_t)(n * map_bytes), st);
    if (e != hipSuccess) { set_error("plane_cells: hipMemsetAsync: %s", hipGetErrorString(e)); return IDE3D_ELAUNCH; }
    const int lds_cells = (map_bytes % 4 == 0 && map_bytes <= 48 * 1024) ? (int)map_bytes : 0;       // (a 256^2 plane: 12 KB)
    hipLaunchKernelGGL(plane_cells_kernel, dim3((unsigned)cdiv64(per_img, 256), (unsigned)n), dim3(256), (size_t)lds_cells, st, p, cells_h, cells_w, lds_cells, cells);
    IDE3D_CHECK_LAUNCH("plane_cells");
    return IDE3D_OK;
}

extern "C" int ide3d_plane_tile_list(const ide3d_plane_gate* gate, int32_t n, int32_t h, int32_t w, int32_t tile_h, int32_t tile_w, int32_t* list, void* stream) {
    using namespace ide3d;
    IDE3D_CHECK_ARG(gate && gate->cells && list, "plane_tile_list: null pointer");
    IDE3D_CHECK_ARG(n > 0 && h > 0 && w > 0 && tile_h > 0 && tile_w > 0 && tile_h % 4 == 0 && tile_w % 4 == 0, "plane_tile_list: bad shape (tiles are multiples of the 4 x 4 cell)");
    IDE3D_CHECK_ARG(4 * (int64_t)gate->cells_h >= h && 4 * (int64_t)gate->cells_w >= w, "plane_tile_list: the cell map does not cover the output");
    const int tiles_y = cdiv(h, tile_h), tiles_x = cdiv(w, tile_w);
    IDE3D_CHECK_ARG((int64_t)n * tiles_y * tiles_x < 0x7fffffffLL, "plane_tile_list: too many tiles");
    hipLaunchKernelGGL(plane_tile_list_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, *gate, n, tiles_y, tiles_x, tile_h, tile_w, list);
    IDE3D_CHECK_LAUNCH("plane_tile_list");
    return IDE3D_OK;
}

extern "C" int ide3d_sphere_points(const float* theta, const float* pitch, int32_t n, float r, int32_t pitch_is_v,
                                   float* pos, float* phi_out, void* stream) {
    using namespace ide3d;
    IDE3D_CHECK_ARG(theta && pitch && pos, "sphere_points: null pointer");
    IDE3D_CHECK_ARG(n > 0, "sphere_points: bad shape");
    hipLaunchKernelGGL(sphere_points_kernel, dim3(cdiv(n, 64)), dim3(64), 0, (hipStream_t)stream, theta, pitch, n, r, pitch_is_v, pos, phi_out);
    IDE3D_CHECK_LAUNCH("sphere_points");
    return IDE3D_OK;
}

extern "C" int ide3d_cam2world(const float* forward, const float* origin, const float* lookat, int32_t lookat_stride, int32_t n,
                               float* out, void* stream) {
    using namespace ide3d;
    IDE3D_CHECK_ARG(origin && out && (forward || lookat), "cam2world: null pointer");
    IDE3D_CHECK_ARG(n > 0 && (lookat_stride == 0 || lookat_stride == 3), "cam2world: bad shape");
    hipLaunchKernelGGL(cam2world_kernel, dim3(cdiv(n, 64)), dim3(64), 0, (hipStream_t)stream, forward, origin, lookat, lookat_stride, n, out);
    IDE3D_CHECK_LAUNCH("cam2world");
    return IDE3D_OK;
}
