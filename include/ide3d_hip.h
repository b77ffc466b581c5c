/*
 * ide3d_hip.h — C ABI of libide3d_hip.so, the MI355X (gfx950) implementation of the
 * IDE-3D rendering hot path.
 *
 * Every entry point is `extern "C"`, takes plain device pointers / sizes / strides and a
 * `void* stream` (a hipStream_t; NULL = the default stream), launches asynchronously on that
 * stream and returns 0 on success or a negative IDE3D_E* code.  After a failure
 * `ide3d_last_error()` returns a human readable, thread-local message.  No entry point
 * allocates, frees or synchronises; the caller owns every buffer.
 *
 * Each declaration cites the reference interface it replaces (paths relative to the
 * IDE-3D repository, MrTornado24/IDE-3D).
 */
#ifndef IDE3D_HIP_H_
#define IDE3D_HIP_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- common --------------------------------------------------------------------------- */

#define IDE3D_OK            0
#define IDE3D_EINVAL       (-1)   /* bad argument (the reference raises via TORCH_CHECK)      */
#define IDE3D_ENOKERNEL    (-2)   /* no specialised kernel: caller must use its generic path  */
#define IDE3D_ELAUNCH      (-3)   /* hipLaunchKernel / runtime error                          */

/* element types of activation tensors */
#define IDE3D_F32  0
#define IDE3D_F16  1
#define IDE3D_BF16 2
#define IDE3D_F64  3

const char* ide3d_last_error(void);
/* ABI version (bumped on any signature change) and the gfx arch string the library was built for. */
int         ide3d_abi_version(void);
const char* ide3d_build_arch(void);
/* ABI 6.  Space-separated list of the non-default compile-time knobs this binary was built with ("" for a release build; `make EXTRA=-D...`,
 * scripts/micro/build_variant.sh).  A knob that changes RESULTS or drops a safety property — the timing-only experiments IDE3D_SP_DBG /
 * IDE3D_HEAD_DBG / IDE3D_F16_BF16MFMA (wrong values by design) and IDE3D_SP_SHARED_SIMD (no exclusive residency) — is listed
 * with a leading '!'; the host side (`hip_plugin.load()`) refuses such a library unless IDE3D_ALLOW_EXPERIMENT_BUILD=1 is set. */
const char* ide3d_build_flags(void);
/* ABI 6.  Kernels that contain an LDS-fed bf16 / fp16 matrix loop keep other waves off their SIMDs (one workgroup per CU: DESIGN.md 4.2).  The
 * library asks the HIP runtime, once per kernel and device, whether that holds where it runs (hipOccupancyMaxActiveBlocksPerMultiprocessor == 1);
 * a kernel for which it does not is never launched (the call returns IDE3D_ELAUNCH) and counted here.  0 on every supported configuration. */
int         ide3d_exclusive_violations(void);
const char* ide3d_exclusive_violation_text(void);

/* ---- bias_act ------------------------------------------------------------------------- */
/*
 * Replaces `_plugin.bias_act(x, b, xref, yref, dy, grad, dim, act, alpha, gain, clamp)`
 * (torch_utils/ops/bias_act.cpp:32, registered :94-97; kernel bias_act.cu:23).
 *   grad = 0: y = clamp(act(x + b) * gain)
 *   grad = 1: y = d/dx of the above, applied to incoming gradient x (=dy), using xref/yref
 *   grad = 2: second-order term (needs dy = the first-order incoming gradient)
 * x/xref/yref/dy/y are dense with identical memory layout, `size_x` elements of `dtype`.
 * b (may be NULL) has `size_b` elements of `dtype`; element i uses b[(i / step_b) % size_b]
 * (step_b = x.stride(dim), bias_act.cpp:80-82).  act is the reference's cuda_idx 1..9
 * (bias_act.py:22-30).  clamp < 0 disables clamping.
 */
int ide3d_bias_act(const void* x, const void* b, const void* xref, const void* yref,
                   const void* dy, void* y, int dtype, int grad, int act,
                   float alpha, float gain, float clamp,
                   int64_t size_x, int64_t size_b, int64_t step_b, void* stream);

/* ---- upfirdn2d ------------------------------------------------------------------------ */
/*
 * Replaces `_plugin.upfirdn2d(x, f, upx, upy, downx, downy, padx0, padx1, pady0, pady1,
 * flip, gain)` (torch_utils/ops/upfirdn2d.cpp:16, registered :102-105; kernels
 * upfirdn2d.cu:29,97).  x is [n, c, in_h, in_w] with arbitrary element strides (NCHW or
 * channels_last), f is a float32 [f_h, f_w] tap array with element strides, y is
 * [n, c, out_h, out_w] with its own strides; out = (in*up + pad0 + pad1 - f + down) / down
 * (upfirdn2d.cpp:35-36) must match what the caller allocated.
 */
typedef struct ide3d_upfirdn2d_params {
    const void*  x;            /* input activations                                   */
    const float* f;            /* filter taps (float32, device)                       */
    void*        y;            /* output activations                                  */
    int32_t dtype;             /* IDE3D_F32 / F16 / BF16 / F64                         */
    int32_t n, c, in_h, in_w;  /* input shape                                         */
    int32_t out_h, out_w;      /* output spatial shape                                */
    int64_t x_stride[4];       /* element strides of x: n, c, h, w                    */
    int64_t y_stride[4];       /* element strides of y: n, c, h, w                    */
    int32_t f_h, f_w;          /* filter shape                                        */
    int64_t f_stride[2];       /* element strides of f: h, w                          */
    int32_t up_x, up_y, down_x, down_y;
    int32_t pad_x0, pad_y0;    /* leading pads (trailing pads are implied by out size) */
    int32_t flip;              /* 1 = correlation (flip_filter=True)                  */
    float   gain;
    int32_t x_row_floats;      /* ABI 5.  The caller's promise: this many elements may be READ from the start of EVERY row of x (padded row
                                  storage, e.g. the `y_pitch` output of ide3d_modconv2d mode 2).  0 = no promise beyond in_w.  The tile kernels
                                  stage rows with 16-byte loads only when round_up(in_w, 4) <= max(in_w, x_row_floats), and never touch an
                                  element at or beyond round_up(in_w, 4) of a row (values past in_w are discarded). */
} ide3d_upfirdn2d_params;

int ide3d_upfirdn2d(const ide3d_upfirdn2d_params* p, void* stream);

/*
 * upfirdn2d with a fused epilogue (MI355X extension; saves the HBM round trips of the element-wise ops that always
 * follow the FIR on the render path):
 *   y = bias_act( FIR(x) + add + noise * noise_strength )
 * `add` (same dtype as x, element strides) fuses the skip accumulation `img = upsample2d(img) + torgb(x)`
 * (inversion/networks.py:1100-1111); `noise` [out_h, out_w] float32 + `bias` [c] + act fuse the tail of an
 * up-sampling SynthesisLayer, `x.add_(noise)` and `bias_act(x, b, act='lrelu', gain, clamp)` (networks.py:507-512).
 * Any pointer may be NULL; fused_act = 0 skips the bias/activation stage.  act: 1 linear, 3 lrelu.
 */
#define IDE3D_AMAX_SLOTS  32       /* slots per image in the `amax` side outputs: workgroup b raises slot b % 32 */
#define IDE3D_AMAX_STRIDE 64       /* floats between two slots (256 bytes: every slot in its own cache line / L2 channel) */
#define IDE3D_AMAX_FLOATS (IDE3D_AMAX_SLOTS * IDE3D_AMAX_STRIDE)     /* floats per image; the value of slot k is element k * STRIDE */

typedef struct ide3d_upfirdn2d_epilogue {
    const void*  add;
    int64_t      add_stride[4];
    const float* noise;
    float        noise_strength;
    const void*  bias;
    int32_t      fused_act;
    int32_t      act;
    float        alpha, act_gain, clamp;
    float*       y_amax;      /* NULL, or [n][IDE3D_AMAX_FLOATS] float32 the caller zeroed: max over a row = max |y[n, :, :, :]| of the
                                 finished output, NaNs ignored (every workgroup raises slot `its index % IDE3D_AMAX_SLOTS` ONCE, after a read that
                                 usually makes the atomic unnecessary — 32 cache lines per image instead of one hot word;
                                 non-negative floats compare like unsigned integers).
                                 Feeds `x_amax` of the convolution that consumes y in the f16x3 arithmetic (ide3d_modconv_params). */
} ide3d_upfirdn2d_epilogue;

int ide3d_upfirdn2d_ex(const ide3d_upfirdn2d_params* p, const ide3d_upfirdn2d_epilogue* ep, void* stream);

/* Host-only planning query (no launch, no device access): which kernel form ide3d_upfirdn2d / ide3d_upfirdn2d_ex would launch for these
 * parameters, with its geometry.  The pointers of `p` and `ep` (`ep` may be NULL) count for whether they are null and for their 16-byte
 * alignment only and are never dereferenced.  The launch goes through the same decision (and the tile kernel through the same staging
 * predicate), and the query refuses exactly what the launch refuses.  The knobs IDE3D_FIR_NO_LEAN / IDE3D_FIR_NO_CELL are read per
 * query as they are per launch.  For tests and tooling; not part of the reference's interface. */
enum { IDE3D_UPFIRDN_GENERIC = 0,   /* upfirdn2d_generic_kernel: one output per lane, any factors / filter / strides / dtype */
       IDE3D_UPFIRDN_CELL = 1,      /* upfirdn2d_cell_kernel<U>: up U x U (2 or 4), no decimation, filter of >= 36 taps in LDS */
       IDE3D_UPFIRDN_TILE = 2,      /* upfirdn2d_tile_kernel<ux, uy, dx, dy, fw, fh, cx, cy>: LDS-tiled polyphase kernel */
       IDE3D_UPFIRDN_FIR44 = 3,     /* fir44_kernel: fp32 4x4 filter at unit rate, lean form */
       IDE3D_UPFIRDN_FIR_UP2 = 4 }; /* fir_up2_kernel: fp32 4x4 filter with 2x zero-upsampling, lean form */
typedef struct ide3d_upfirdn2d_plan_info {
    int32_t form;                    /* IDE3D_UPFIRDN_* */
    int32_t ux, uy, dx, dy, fw, fh, cx, cy;      /* TILE: the template instance (cx, cy = cells per thread; the workgroup is 32 x 8 threads).  The lean
                                        forms report the instance whose values they reproduce bit for bit; 0 for the other forms */
    int32_t cell_u;                  /* CELL: U; 0 otherwise */
    int32_t staging;                 /* how the input window reaches LDS.  TILE: 1 = every plane by 16-byte loads, 0 = every plane by scalar loads,
                                        2 = mixed (planes differ in their 16-byte alignment); the lean forms: 1; GENERIC / CELL: -1 (no staging) */
    int32_t c_fastest;               /* GENERIC: 1 = lanes run along the channels (channels_last output with c > 1); 0 otherwise */
    int32_t tiles_x, tiles_y;        /* tiled forms: tiles per plane; CELL: cells per plane (each U x U outputs); GENERIC: 0 */
    int64_t grid;                    /* workgroups of 256 threads */
    int64_t lds_bytes;               /* dynamic LDS per workgroup (CELL: the padded filter; 0 for the other forms, whose LDS is static) */
} ide3d_upfirdn2d_plan_info;
int ide3d_upfirdn2d_plan(const ide3d_upfirdn2d_params* p, const ide3d_upfirdn2d_epilogue* ep, ide3d_upfirdn2d_plan_info* out);

/* ---- filtered_lrelu ------------------------------------------------------------------- */
/*
 * Replaces `_plugin.filtered_lrelu(x, fu, fd, b, si, up, down, px0, px1, py0, py1, sx, sy,
 * gain, slope, clamp, flip_filters, writeSigns)` (torch_utils/ops/filtered_lrelu.cpp:16,
 * parameter block filtered_lrelu.h:14-53; kernel filtered_lrelu.cu:139).  One launch does
 * bias -> up-FIR(gain up^2) -> gain*lrelu(slope) -> clamp -> down-FIR.  Filters travel in the
 * kernel argument block / LDS (no process-global constant buffer: stream-safe, unlike
 * filtered_lrelu.cu:77-78).  fu/fd are float32; shape [h, w] with f*_h = 0 meaning a separable
 * 1-D filter of f*_w taps (filtered_lrelu.cpp:49-50).
 * Sign tensor s (uint8, 4 x 2-bit codes per byte; bit0 = negative, bit1 = clamped;
 * filtered_lrelu.cu:494-519) is [n, c, s_h, s_w_bytes] contiguous.  sign_mode: 0 none,
 * 1 write, 2 read.  Returns IDE3D_ENOKERNEL when the tile does not fit the LDS budget or the
 * filter exceeds the supported tap count (the reference's `return_code = -1`,
 * filtered_lrelu.cpp:52-56): the caller then runs the generic path with
 * ide3d_filtered_lrelu_act.
 */
typedef struct ide3d_filtered_lrelu_params {
    const void*  x;
    void*        y;
    const void*  b;            /* per-channel bias, dtype of x, never NULL            */
    uint8_t*     s;            /* sign tensor or NULL                                 */
    const float* fu;
    const float* fd;
    int32_t dtype;             /* IDE3D_F32 / F16 / BF16                               */
    int32_t n, c, in_h, in_w;
    int32_t out_h, out_w;
    int64_t x_stride[4];       /* element strides n, c, h, w                          */
    int64_t y_stride[4];
    int32_t fu_w, fu_h;        /* fu_h == 0 -> separable                              */
    int32_t fd_w, fd_h;
    int64_t fu_stride[2];      /* element strides: h, w (h unused when separable)     */
    int64_t fd_stride[2];
    int32_t up, down;
    int32_t pad_x0, pad_y0;
    int32_t s_w_bytes, s_h;    /* sign tensor shape (width in bytes)                  */
    int32_t s_ofs_x, s_ofs_y;  /* sign offset (elements), sx/sy of the reference      */
    int32_t sw_limit;          /* active sign width in bytes, filtered_lrelu.cpp:125  */
    int32_t sign_mode;         /* 0 none, 1 write, 2 read                             */
    int32_t flip;
    float   gain, slope, clamp;
} ide3d_filtered_lrelu_params;

int ide3d_filtered_lrelu(const ide3d_filtered_lrelu_params* p, void* stream);

/*
 * Replaces `_plugin.filtered_lrelu_act_(x, si, sx, sy, gain, slope, clamp, writeSigns)`
 * (torch_utils/ops/filtered_lrelu.cpp:213; kernel filtered_lrelu.cu:1105).  In-place
 * gain*lrelu*clamp on x [n, c, h, w] (element strides) with sign write / read.  s_w is the
 * sign width in *elements* (a multiple of 16 when writing), s is contiguous.
 */
int ide3d_filtered_lrelu_act(void* x, uint8_t* s, int dtype,
                             int32_t n, int32_t c, int32_t h, int32_t w,
                             const int64_t x_stride[4],
                             int32_t s_w, int32_t s_h, int32_t s_ofs_x, int32_t s_ofs_y,
                             float gain, float slope, float clamp, int sign_mode, void* stream);

/* ---- tri-plane feature gather ----------------------------------------------------------- */
/*
 * Replaces `dnnlib.util.sample_from_triplane(coordinates, grid)` (dnnlib/util.py:580-617:
 * three `grid_sample(bilinear, zeros, align_corners=False)` calls — torch_utils/ops/
 * grid_sample_gradfix.py:26-29 — on the xy, yz and xz planes, summed).
 * planes: float32 [n, 3*C, H, W] addressed through element strides (NCHW or channels_last;
 *         channels_last is the fast path: each bilinear tap is one contiguous C*4-byte read).
 * coords: float32 [n, m, 3] contiguous, world coordinates in grid_sample's [-1, 1] convention.
 * out:    float32 [n*m, C] contiguous, row = n*m_total + m.
 * Tap index math is bit-exact w.r.t. ATen grid_sampler_2d: u = ((c + 1) * size - 1) / 2
 * evaluated add -> mul -> sub -> mul(0.5) in fp32 with no FMA contraction.
 */
int ide3d_triplane_sample(const float* planes, const int64_t plane_stride[4],
                          int32_t n, int32_t C, int32_t H, int32_t W,
                          const float* coords, int64_t m, float* out, void* stream);

/*
 * Same operation and same results, for samples that come from a ray grid (what the ray-marcher
 * of volumetric_rendering.py:160-191 produces): coords is [n, rays_h, rays_w, steps, 3], i.e.
 * m == rays_h * rays_w * steps with the depth step innermost.  The shape is a grouping hint
 * only: 8x8 ray tiles x 4 depth steps stage the plane texels they share in LDS once instead of
 * fetching them per sample.  Any coordinates are legal; shapes / layouts the tiled kernel does
 * not cover run `ide3d_triplane_sample`.
 */
int ide3d_triplane_sample_rays(const float* planes, const int64_t plane_stride[4],
                               int32_t n, int32_t C, int32_t H, int32_t W,
                               const float* coords, int64_t m, float* out,
                               int32_t rays_h, int32_t rays_w, int32_t steps, void* stream);

/*
 * Debug / parity hook: writes, per sample and plane, the integer tap origin (floor(u),
 * floor(v)) and the in-bounds mask of the four taps, so tests can assert bit-exact index
 * math against the oracle.  taps: int32 [n*m, 3, 3] = (ix0, iy0, mask4).
 */
int ide3d_triplane_taps(int32_t H, int32_t W, const float* coords, int64_t n_times_m,
                        int32_t* taps, void* stream);

/*
 * Debug / parity hook of the ray-grid gather: which planes `ide3d_triplane_sample_rays` stages in LDS
 * for every chunk (8x8 rays x 4 depth steps) of coords [n, rays_h, rays_w, steps, 3], computed by the
 * gather kernel's own region-table code.  masks: int32 [n, tiles, steps / 4], tiles row-major over
 * the (rays_h / 8) x (rays_w / 8) ray tiles; bit p = plane p is staged, the others are read like the
 * flat kernel reads them.  rays_h, rays_w must be multiples of 8, steps of 4; H, W <= 32767.
 */
int ide3d_triplane_tile_masks(int32_t H, int32_t W, const float* coords, int32_t n,
                              int32_t rays_h, int32_t rays_w, int32_t steps, int32_t* masks, void* stream);

/*
 * Backward of the gather w.r.t. the planes (atomic scatter-add into grad_planes, which the
 * caller zero-fills) and optionally w.r.t. the coordinates (grad_coords may be NULL).
 * Replaces aten::grid_sampler_2d_backward as used by grid_sample_gradfix.py:55-60.
 */
int ide3d_triplane_sample_backward(const float* grad_out, const float* planes,
                                   const int64_t plane_stride[4],
                                   int32_t n, int32_t C, int32_t H, int32_t W,
                                   const float* coords, int64_t m,
                                   float* grad_planes, const int64_t grad_plane_stride[4],
                                   float* grad_coords, void* stream);

/* ---- volume compositing ----------------------------------------------------------------- */
/*
 * Replaces `training.volumetric_rendering.fancy_integration` (volumetric_rendering.py:34-74).
 * rgb_sigma: float32 [rays, steps, ch+1] contiguous (sigma last), z_vals: [rays, steps],
 * dir_norm: [rays] (= ||rays_d_cam||), noise: [rays, steps] or NULL (already scaled by
 * noise_std).  Outputs: rgb [rays, ch], depth [rays], weights [rays, steps] (NULL = skip).
 * clamp_mode: 0 softplus, 1 relu.  fill_mode: 0 none, 1 'debug', 2 'weight'.
 * One wavefront integrates one ray: lane-local alpha, wave-wide exclusive prefix product of
 * (1 - alpha + 1e-10) by shuffles, then a shuffle reduction per channel.
 */
int ide3d_composite(const float* rgb_sigma, const float* z_vals, const float* dir_norm,
                    const float* noise, int64_t rays, int32_t steps, int32_t ch,
                    int clamp_mode, int last_back, int white_back, float max_depth,
                    int fill_mode, float* rgb, float* depth, float* weights, void* stream);
/* steps == 1 is accepted: one sample, delta 1e10 (the last sample's delta).  `fancy_integration` itself never sends it: the tensor
 * definition drops the lone sample (weights [N, R, 0, 1]), and the call surface follows the definition there. */

/* Host-only planning query (no launch, no device access): which of the kernel forms ide3d_composite would launch for this shape, with its
 * grid, workgroup size and dynamic LDS bytes.  `rgb_sigma` counts for its 16-byte alignment only and is never dereferenced.  The launch
 * goes through the same decision.  Same shape checks as ide3d_composite.  For tests and tooling; not part of the reference's interface. */
enum { IDE3D_COMPOSITE_FALLBACK = 0, /* composite_kernel: 4 waves per workgroup, rows read from global memory, any shape / alignment */
       IDE3D_COMPOSITE_LDS8 = 1,     /* composite_lds_kernel<8>:  ray block staged in LDS, steps * (ch + 1) <= 2048 floats */
       IDE3D_COMPOSITE_LDS20 = 2,    /* composite_lds_kernel<20>: <= 5120 floats */
       IDE3D_COMPOSITE_LDS40 = 3 };  /* composite_lds_kernel<40>: <= 10240 floats */
typedef struct ide3d_composite_plan_info {
    int32_t form;                    /* IDE3D_COMPOSITE_* */
    int32_t workgroup;               /* threads per workgroup */
    int64_t grid;                    /* workgroups */
    int64_t lds_bytes;               /* dynamic LDS per workgroup */
} ide3d_composite_plan_info;
int ide3d_composite_plan(const void* rgb_sigma, int64_t rays, int32_t steps, int32_t ch, ide3d_composite_plan_info* out);

/* ---- importance resampling ------------------------------------------------------------- */
/*
 * Replaces `training.volumetric_rendering.sample_pdf` (volumetric_rendering.py:224-265), the
 * inverse-CDF draw of the optional hierarchical pass.  bins: float32 [rays, k+1], weights:
 * [rays, k] (both contiguous), u: the draws in [0, 1] — row `r` starts at u + r * u_ray_stride
 * (0 = one row shared by all rays, the `det=True` linspace), samples: [rays, n_importance].
 * Row sums / prefix sums are accumulated in double and rounded per element like ATen's CPU
 * kernels; everything after the cdf is the reference's float expression without contraction.
 */
int ide3d_sample_pdf(const float* bins, const float* weights, const float* u, int64_t u_ray_stride,
                     int64_t rays, int32_t k, int32_t n_importance, float eps, float* samples,
                     void* stream);

/* ---- fused ray-marcher ------------------------------------------------------------------ */
/*
 * One launch for steps 3-7 of G.synthesis: camera-space sample points
 * (get_initial_rays_trig, volumetric_rendering.py:77-97) -> optional stratified jitter
 * (perturb_points :99-105) -> cam2world transform (transform_sampled_points :108-136) ->
 * two tri-plane gathers (dnnlib/util.py:580) -> decoder MLPs (renderer.sample_voxel, source
 * absent: spec in DESIGN.md) -> fancy_integration (:34-74).
 *
 * rays_d_cam [rays_per_img, 3] and z_lin [steps] are produced on the host with torch.linspace
 * exactly as the reference does, so the kernel never re-derives them.
 * cam2world: [n, 16] row-major 4x4.  jitter: [n, rays_per_img, steps] uniform [0,1) or NULL.
 * tex_planes / geo_planes: [n, 3*C, H, W] through element strides.
 * MLP weights (float32, row-major [out, in], already multiplied by their runtime gains):
 *   geo: w0 [hidden, C], b0 [hidden], w1 [1 + seg_ch, hidden], b1 [1 + seg_ch]
 *   tex: w0 [hidden, C], b0 [hidden], w1 [feat_ch, hidden],    b1 [feat_ch]
 * out_feat: [n, feat_ch + seg_ch, rays_per_img] (channel-major image planes),
 * out_depth: [n, rays_per_img], out_wsum: [n, rays_per_img] (either may be NULL).
 */
typedef struct ide3d_render_params {
    const float* rays_d_cam;
    const float* z_lin;
    const float* cam2world;
    const float* jitter;
    const float* sigma_noise;   /* [n, rays, steps] pre-scaled density noise or NULL */
    const float* tex_planes;
    const float* geo_planes;
    int64_t tex_stride[4];
    int64_t geo_stride[4];
    const float* geo_w0; const float* geo_b0; const float* geo_w1; const float* geo_b1;
    const float* tex_w0; const float* tex_b0; const float* tex_w1; const float* tex_b1;
    int32_t n, rays_per_img, steps;
    int32_t C, H, W;
    int32_t hidden, feat_ch, seg_ch;
    int32_t clamp_mode, last_back, white_back;
    float   max_depth;
    float*  out_feat;
    float*  out_depth;
    float*  out_wsum;
} ide3d_render_params;

int ide3d_render_rays(const ide3d_render_params* p, void* stream);

/*
 * Backward of ide3d_render_rays with respect to the two tri-planes (no gradient for the decoder weights, the camera, the jitter or
 * the density noise).  p: the parameters the forward received (its out_* fields are ignored).  grad_feat [n, feat_ch + seg_ch,
 * rays_per_img], grad_depth / grad_wsum [n, rays_per_img]: dL/d of the forward's three outputs, each may be NULL (= zero).  dL/dtex_planes
 * and dL/dgeo_planes are ADDED to grad_tex_planes / grad_geo_planes, [n, 3*C, H, W] through element strides with channel stride 1
 * (channels_last), which the caller zeroes.  The samples are rebuilt from p exactly as the forward built them; exact fp32 arithmetic.
 * Accumulation uses float atomics, so the sums depend on arrival order: results agree to fp32 rounding, not bit for bit, between runs.
 * IDE3D_ENOKERNEL for what the forward also declines (last_back, planes not channels_last, (C, hidden) other than (32, 64) / (16, 32)),
 * gradient buffers that are not channels_last, and step counts whose per-ray state does not fit in LDS.
 */
typedef struct ide3d_render_grads {
    const float* grad_feat;  const float* grad_depth;  const float* grad_wsum;   /* each may be NULL */
    float* grad_tex_planes;  float* grad_geo_planes;                            /* [n, 3C, H, W], accumulated into */
    int64_t grad_tex_stride[4];  int64_t grad_geo_stride[4];
} ide3d_render_grads;

int ide3d_render_rays_backward(const ide3d_render_params* p, const ide3d_render_grads* g, void* stream);

/*
 * The same backward with the gradients of the decoder's eight tensors as well: what autograd computes for `renderer.decoder` in PTI's
 * pivotal tuning (Adam over G.parameters(), inversion/training/coaches/base_coach.py:148; the step-wise definition's four linear layers
 * and their backwards, volumetric_rendering.py:34-74 composited on top).  p and g as for ide3d_render_rays_backward, except that
 * g->grad_tex_planes / g->grad_geo_planes may each be NULL: that plane's scatter is skipped (decoder-only training on detached planes).
 * The eight outputs are WRITTEN (not added to), fp32, contiguous, with the shapes of the tensors p points to; they are gradients with
 * respect to those gain-folded tensors.  workspace: ide3d_render_param_grad_workspace_bytes(p) bytes, 16-byte aligned, owned by this
 * call until the stream has passed it: one slice of partial sums per wave, added in a fixed order by a second launch, so the eight
 * gradients are bit-reproducible from run to run (the plane gradients are not).  IDE3D_ENOKERNEL in the cases of
 * ide3d_render_rays_backward.  The workspace query reads n, rays_per_img, steps, C, hidden, feat_ch and seg_ch; 0 = no kernel.
 */
typedef struct ide3d_render_param_grads {
    float* grad_geo_w0; float* grad_geo_b0; float* grad_geo_w1; float* grad_geo_b1;
    float* grad_tex_w0; float* grad_tex_b0; float* grad_tex_w1; float* grad_tex_b1;
    void* workspace;
    int64_t workspace_bytes;
} ide3d_render_param_grads;

int64_t ide3d_render_param_grad_workspace_bytes(const ide3d_render_params* p);
int ide3d_render_rays_backward_params(const ide3d_render_params* p, const ide3d_render_grads* g, const ide3d_render_param_grads* q, void* stream);

/*
 * The same backward with the gradient of the camera pose: dL/dcam2world [n, 4, 4], what autograd computes through
 * transform_sampled_points (volumetric_rendering.py:108-136) and the two grid_sample gathers (zeros padding, align_corners=False).  The
 * outputs depend on cam2world only through the sample points p = M[:3,:3] q + M[:3,3] (q the camera-space point): with gp = dL/dp of a
 * sample (the feature gradient of both branches dotted with the derivative of the bilinear blend of the three planes, times size / 2),
 * dL/dM[r][c] = sum_samples gp_r q_c (c < 3), dL/dM[r][3] = sum_samples gp_r; the last row is written as zero.  All 12 entries are free:
 * no rotation structure is assumed.  Taps outside a plane and non-finite coordinates contribute nothing, like the forward.
 * p and g as for ide3d_render_rays_backward_params (g's plane pointers may each be NULL); q: the decoder gradients as well, or NULL;
 * c: the camera gradient, or NULL.  Without c the call does what ide3d_render_rays_backward_params (q given) or ide3d_render_rays_backward
 * (q NULL, both plane pointers required) does, with this entry point's name in its error texts; q NULL, c NULL and both plane pointers NULL is IDE3D_EINVAL.  grad_cam2world is WRITTEN, fp32, contiguous.  workspace:
 * ide3d_render_camera_grad_workspace_bytes(p) bytes, 16-byte aligned, owned by this call until the stream has passed it: 12 sums per image
 * per wave, added in a fixed order by a second launch (no atomics), so the camera gradient is bit-reproducible from run to run and equal
 * whatever else the call computes.  IDE3D_ENOKERNEL in the cases of ide3d_render_rays_backward.  The workspace query reads n,
 * rays_per_img, steps, C and hidden; 0 = no kernel.
 */
typedef struct ide3d_render_camera_grads {
    float* grad_cam2world;      /* [n, 4, 4], written, last row zero */
    void* workspace;
    int64_t workspace_bytes;
} ide3d_render_camera_grads;

int64_t ide3d_render_camera_grad_workspace_bytes(const ide3d_render_params* p);
int ide3d_render_rays_backward_camera(const ide3d_render_params* p, const ide3d_render_grads* g, const ide3d_render_param_grads* q,
                                      const ide3d_render_camera_grads* c, void* stream);

/*
 * The hierarchical (importance) pass of the renderer as four launches, nothing per sample but depths and weights in memory (DESIGN.md
 * section 5.24): ide3d_render_ray_weights -> ide3d_sample_pdf -> ide3d_merge_depths -> ide3d_render_rays_merged.  All three take what
 * ide3d_render_rays takes and return IDE3D_ENOKERNEL for what it declines (last_back, planes not channels_last, (C, hidden) other than
 * (32, 64) / (16, 32)) and for steps < 3 or steps > 1024 (ide3d_merge_depths keeps the 2 * steps keys of a ray in LDS: at most 2048).
 * No atomics: results are bit-reproducible.
 *
 * ide3d_render_ray_weights: the first pass, geometry branch only.  p as for ide3d_render_rays (sigma_noise honoured, out_* ignored).
 *   weights     [n * rays_per_img, steps]      fancy_integration's third output
 *   z_vals      [n * rays_per_img, steps]      the (jittered) sample depths
 *   pdf_bins    [n * rays_per_img, steps - 1]  0.5 * (z[s] + z[s + 1])
 *   pdf_weights [n * rays_per_img, steps - 2]  weights[1 .. steps - 2] + 1e-5
 * each contiguous, each may be NULL (not written); pdf_bins / pdf_weights are ide3d_sample_pdf's bins / weights with k = steps - 2.
 *
 * ide3d_merge_depths: per ray the stable ascending order of the concatenation [z_fine | z_coarse] (torch.sort(torch.cat(...)), equal
 * depths keep concatenation order, -0 == +0, NaN last).  z_fine [rays, steps_fine], z_coarse [rays, steps_coarse], T = steps_fine +
 * steps_coarse (1 <= T <= 2048, else IDE3D_EINVAL); z_all [rays, T]: the sorted depths, bit-equal to the inputs; src [rays, T]: index
 * into the concatenation (src < steps_fine: fine sample src, else coarse sample src - steps_fine).  The order is total for any input bits:
 * every row of src is a permutation of 0 .. T-1.
 *
 * ide3d_render_rays_merged: ide3d_render_rays over the total_steps = 2 * p->steps samples of each ray in z_all order, written to p->out_feat
 * / out_depth / out_wsum (white_back / max_depth as there).  z_all / src [n * rays_per_img, total_steps] from ide3d_merge_depths of
 * z_fine [n * rays_per_img, steps] (steps_fine = steps_coarse = steps) and ide3d_render_ray_weights' z_vals.  A coarse sample is placed
 * from z_lin / jitter exactly as the first pass placed it, a fine one at cam2world[:3, 3] + (cam2world[:3, :3] * d_cam) * z_fine; delta =
 * (z_all[s + 1] - z_all[s]) * |d_cam|, 1e10 for the last sample; p->sigma_noise is ignored (no density noise).  src entries are clamped
 * into [0, total_steps) before use: no input data makes the kernel read outside its buffers.
 */
int ide3d_render_ray_weights(const ide3d_render_params* p, float* weights, float* z_vals, float* pdf_bins, float* pdf_weights,
                             void* stream);
int ide3d_merge_depths(const float* z_fine, const float* z_coarse, int64_t rays, int32_t steps_fine, int32_t steps_coarse,
                       float* z_all, int32_t* src, void* stream);
int ide3d_render_rays_merged(const ide3d_render_params* p, const float* z_all, const int32_t* src, const float* z_fine,
                             int32_t total_steps, void* stream);

/*
 * Backward of ide3d_render_rays_merged with respect to the two tri-planes and, with q, the decoder's eight tensors (DESIGN.md section
 * 5.29).  The definition is the step-wise importance pass (TriplaneRenderer.forward, training/triplane.py:300-313), which draws the fine
 * depths and forms the fine points under torch.no_grad(): differentiated are the gathers of the 2 * steps merged samples, both decoders
 * and the compositing (white_back / max_depth included); constants are z_all, src, z_fine, the jitter and the camera, so no gradient flows
 * into the first pass, the pdf draw or the merge.  It is ide3d_render_rays_backward(_params) over total_steps samples placed and spaced as
 * ide3d_render_rays_merged places and spaces them (src clamped into [0, total_steps) before use; p->sigma_noise ignored), nothing per
 * sample saved.  p, z_all, src, z_fine, total_steps: what the forward received (out_* ignored).  g as for ide3d_render_rays_backward: plane
 * gradients are ADDED to caller-zeroed channels_last buffers (float atomics: not bit-reproducible); with q either plane pointer may be NULL
 * (scatter skipped).  q: NULL (planes only, both plane pointers required) or as for ide3d_render_rays_backward_params: the eight
 * gradients are WRITTEN, bit-reproducible, workspace of ide3d_render_merged_param_grad_workspace_bytes(p) bytes (sized by 2 * p->steps;
 * 0 = no kernel), 16-byte aligned.  IDE3D_EINVAL: null pointers, total_steps != 2 * steps.  IDE3D_ENOKERNEL with an error text: steps < 3
 * or steps > 1024, last_back, planes or gradient buffers not channels_last, (C, hidden) other than (32, 64) / (16, 32), total_steps whose
 * per-ray state does not fit in LDS.  There is no camera gradient through the merged march.
 */
int64_t ide3d_render_merged_param_grad_workspace_bytes(const ide3d_render_params* p);
int ide3d_render_rays_merged_backward(const ide3d_render_params* p, const float* z_all, const int32_t* src, const float* z_fine,
                                      int32_t total_steps, const ide3d_render_grads* g, const ide3d_render_param_grads* q, void* stream);

/*
 * `renderer.sample_voxel(img_v, seg_v, pts)` (call site extract_shapes.py:146): the same two
 * gathers + MLPs for arbitrary points, no compositing.  out: [n*m, feat_ch + seg_ch + 1]
 * (sigma last).  If sigma_only != 0 only out_sigma [n*m] is written (the 256^3 density-cube
 * query) and the texture branch is skipped.
 */
int ide3d_sample_voxel(const ide3d_render_params* p, const float* pts, int64_t m,
                       float* out, float* out_sigma, int sigma_only, void* stream);

/*
 * The point lattice of `extract_shapes.create_samples` (extract_shapes.py:74-96) with the
 * 0.9 scale of extract_shapes.py:103 folded in: point i (0 <= i < n^3) is
 *   s2 = i % n,  s1 = (float(i) / n) % n,  s0 = ((float(i) / n) / n) % n     (fp32, NOT floored: reference quirk)
 *   (x, y, z) = ((s0 * voxel_size + corner[2]) * scale, (s1 * voxel_size + corner[1]) * scale,
 *                (s2 * voxel_size + corner[0]) * scale)
 * with every operation rounded to fp32 separately, i.e. bit-equal to the reference's host code.
 * corner = voxel_origin - cube_length / 2, voxel_size = cube_length / (n - 1), both rounded to fp32.
 */
typedef struct ide3d_lattice {
    int32_t n;
    float   voxel_size;
    float   corner[3];
    float   scale;
} ide3d_lattice;

/* Writes points [first, first + count) of the lattice to pts [count, 3] (device). */
int ide3d_lattice_points(const ide3d_lattice* lat, int64_t first, int64_t count, float* pts, void* stream);

/*
 * The chunk loop body of extract_shapes.py:144-148 without materialising coordinates:
 * `renderer.sample_voxel(img_v, seg_v, samples[:, first:first+count])[..., -1]` for every image
 * of p (p->n), lattice points generated in registers.  out_sigma: [p->n * count].
 * (p's ray / compositing fields are ignored, as in ide3d_sample_voxel.)
 */
int ide3d_density_lattice(const ide3d_render_params* p, const ide3d_lattice* lat, int64_t first, int64_t count,
                          float* out_sigma, void* stream);

/* ---- iso-surface mesh of a density cube ----------------------------------------------------- */
/*
 * `vertices, triangles = mcubes.marching_cubes(volume, threshold)` (render_mesh.py:31,
 * dnnlib/geometry.py:286 `extract_geometry`) on the device, in two calls around the one read the
 * caller needs to size the outputs.
 *
 * volume [X, Y, Z] float32 contiguous (Z fastest), 1..1024 points per axis.  A corner is inside
 * when value > iso (strict).  table: device copy of the 256 x 16 byte case table of
 * training/mesh_extraction.py::case_table_bytes() (byte 0: triangles of the case, then their edge
 * ids; cell corner c = x + 2y + 4z, edges = corner pairs differing in one bit, ascending).
 * workspace: ide3d_mesh_workspace_bytes(X, Y, Z) bytes (-1: unsupported grid), 16-byte aligned,
 * owned by the pair of calls: 2 x int64 totals, one (vertices, triangles) pair per workgroup of
 * 1024 points, and one int32 per point (the id of the first vertex the point owns).
 *
 * ide3d_mesh_count: two launches (count per workgroup; scan).  When the stream has passed them
 *   the first 16 bytes of the workspace hold {number of vertices, number of triangles} as int64.
 * ide3d_mesh_emit: with those two numbers (each < 2^31, else IDE3D_EINVAL) and the same volume,
 *   iso, table and workspace: vertices [V, 3] float32 = p_a + t (p_b - p_a) on every crossing
 *   grid edge, t = (iso - v_a) / (v_b - v_a) in fp32 with IEEE division, in index units, or with
 *   lat != NULL (lat->n is ignored) axis k of the volume mapped like ide3d_lattice_points:
 *   (index * voxel_size + corner[2 - k]) * scale; triangles [T, 3] int32; normals [V, 3] or NULL:
 *   the negated central-difference gradient (one-sided at the border) of both edge ends,
 *   interpolated with t and normalised, zero where it vanishes.  Triangle normals point toward
 *   lower values; flip != 0 reverses the winding and the normals.  No atomics: vertex order
 *   (owning point in memory order, x before y before z) and triangle order (cell in memory order,
 *   then table order) depend on the grid shape and the data only.
 */
int64_t ide3d_mesh_workspace_bytes(int32_t X, int32_t Y, int32_t Z);
int ide3d_mesh_count(const float* volume, int32_t X, int32_t Y, int32_t Z, float iso, const uint8_t* table,
                     void* workspace, int64_t workspace_bytes, void* stream);
int ide3d_mesh_emit(const float* volume, int32_t X, int32_t Y, int32_t Z, float iso, const uint8_t* table,
                    const ide3d_lattice* lat, int32_t flip, void* workspace, int64_t workspace_bytes,
                    int64_t num_vertices, int64_t num_triangles, float* vertices, int32_t* triangles, float* normals, void* stream);

/* ---- triangle rasterizer for the extracted mesh --------------------------------------------- */
/*
 * The pyrender / OpenGL step of render_mesh.py:36-61 (perspective camera render_mesh.py:48-56,
 * one directional light at the camera pose render_mesh.py:57, white background
 * render_mesh.py:47): N cameras of one mesh in three calls on
 * one stream.  csrc/raster.hip states the definition; training/mesh_render.py holds the host
 * definition that reproduces every integer of it.  pyrender's metallic-roughness shading is NOT
 * reproduced (ambient + diffuse Lambert instead), and there is NO clipping: a triangle with a
 * vertex behind `near` or outside the guard band |pixel coordinate| <= 16384 is dropped whole.
 *
 * vertices [V, 3] float32 world space; triangles [T, 3] int32; V, T < 2^31; 1 <= H, W <= 16384;
 * 1 <= N <= 65535.  workspace: ide3d_raster_workspace_bytes(N, V, H, W) bytes (-1: unsupported
 * shape), 16-byte aligned, owned by the three calls: a status word (16 bytes), one 16-byte
 * record (X, Y, view depth, flags) per camera and vertex, the z-buffer [N, H, W] of uint64 keys
 * (float_bits(depth) << 32 | triangle index; all ones = background).
 *
 * ide3d_raster_project (render_mesh.py:48-56): world2cam [N, 3, 4] float32 = rows of (R | t),
 *   the inverse of the camera pose, inverted by the caller in float64.  d = -z_cam,
 *   px = ((fx * x_cam) / d) * sx + ox, py = oy - ((fy * y_cam) / d) * sy, every operation one
 *   float32 operation in this order, X = rint(256 px), Y = rint(256 py).  fy = 1 / tan(yfov / 2),
 *   fx = fy / aspect.  The sample of pixel (r, c) is (256 c + 128, 256 r + 128), so sx = W / 2,
 *   ox = W / 2 puts pixel centres at c + 0.5 as OpenGL (and therefore render_mesh.py:60) does.
 * ide3d_raster_depth (render_mesh.py:60-61, the depth test): clears the status word and the
 *   z-buffer, then one 64-bit unsigned atomic minimum per covered sample (top-left rule on the
 *   integers, perspective-correct float32 depth).  The result does not depend on the order of
 *   the triangles' arrival; equal depths resolve to the lower index.  cull: IDE3D_RASTER_CULL_*
 *   (front = the geometric normal (v1 - v0) x (v2 - v0) points toward the camera).  large_min:
 *   triangles whose clipped box holds at least this many samples are rasterized by a whole
 *   wave instead of one lane (< 0: the library's measured default); results do not depend on it.
 *   Status word afterwards: IDE3D_RASTER_BAD_INDEX | IDE3D_RASTER_DROPPED.
 * ide3d_raster_shade (render_mesh.py:36-42, :47, :57): per pixel depth [N, 1, H, W] (+inf on
 *   the background), triangle [N, H, W] (-1), image [N, 3, H, W] in [0, 1] =
 *   clamp(base * (ambient + diffuse * max(0, n . l))) (bg), and, when labels [V] int32 is given,
 *   label [N, H, W] (-1).  normals [V, 3] float32 or NULL (flat face normals), colors [V, 3]
 *   uint8 or NULL (base_color: 3 floats in HOST memory), light [N, 3] float32 device memory: the
 *   camera's +z axis in world space.  two_sided: turn n over on back-facing triangles.
 */
#define IDE3D_RASTER_CULL_NONE  0
#define IDE3D_RASTER_CULL_BACK  1
#define IDE3D_RASTER_CULL_FRONT 2
#define IDE3D_RASTER_BEHIND     1   /* vertex flag: d >= near fails                              */
#define IDE3D_RASTER_OUTSIDE    2   /* vertex flag: outside the guard band                       */
#define IDE3D_RASTER_BAD_INDEX  1   /* status: a triangle index outside [0, V)                   */
#define IDE3D_RASTER_DROPPED    2   /* status: a dropped triangle's remaining box met the screen */
int64_t ide3d_raster_workspace_bytes(int32_t N, int64_t V, int32_t H, int32_t W);
int ide3d_raster_project(const float* vertices, int64_t V, const float* world2cam, int32_t N, int32_t H, int32_t W, float fx, float fy,
                         float sx, float ox, float sy, float oy, float near, void* workspace, int64_t workspace_bytes, void* stream);
int ide3d_raster_depth(const int32_t* triangles, int64_t T, int64_t V, int32_t N, int32_t H, int32_t W, int32_t cull,
                       int32_t large_min, void* workspace, int64_t workspace_bytes, void* stream);
int ide3d_raster_shade(const float* vertices, const int32_t* triangles, int64_t V, int32_t N, int32_t H, int32_t W,
                       const float* normals, const uint8_t* colors, const int32_t* labels, const float* light, int32_t two_sided,
                       float ambient, float diffuse, const float* base_color, float bg, const void* workspace, int64_t workspace_bytes,
                       float* depth, int32_t* triangle, float* image, int32_t* label, void* stream);

/* ---- PNG: row filters and deflate -------------------------------------------------------------- */
/*
 * The compression half of `save_image(imgs, 'seed0000.png', normalize=True, range=(-1, 1))`
 * (gen_images.py:115-116; torchvision + PIL on the host there): frames uint8 [n, h, w, c]
 * contiguous, c = 1 (grey) or 3 (RGB), to the n zlib streams of their PNG files (78 01, deflate
 * blocks, Adler-32 big endian), back to back in `out`; stream k is out[offsets[k], offsets[k + 1]),
 * offsets int64 [n + 1] in device memory.  The caller adds signature, IHDR, IDAT framing and CRCs.
 * training/png.py states every integer of the stream and holds the host definition that gives the
 * same bytes: PNG filter types 0-4 per row (filter_mode 0-4 forces one; 5: per row the type with
 * the smallest sum of min(v, 256 - v) over the filtered bytes, lowest type on a tie); the filtered
 * stream cut into segments of segment_bytes (a power of two, 1024..32768); per segment one deflate
 * block with dynamic Huffman codes (lengths <= 15, code-length alphabet <= 7) whose only matches are
 * runs at distance 1, ended on a byte boundary by an empty stored block (the last one by BFINAL),
 * or one stored block where that is not smaller: a segment of m bytes takes at most m + 5.
 * Four launches (filter, deflate, scan, compact); integer arithmetic, integer LDS atomics only:
 * two runs are bit-equal.
 * workspace: ide3d_png_workspace_bytes() bytes (-1: unsupported shape), 16-byte aligned: the
 * filtered streams, one slot of segment_bytes + 32 per segment, sizes and Adler sums per segment.
 * out_capacity >= ide3d_png_out_bytes() = n * (F + 5 * segments + 6), F = h * (w * c + 1): every
 * segment stored.  Refused with IDE3D_EINVAL before any launch: c not in {1, 3}, a bad
 * segment_bytes or filter_mode, an empty axis, a workspace or out below those sizes, and any of
 * the workspace, out or row count at or above 2^31.
 */
int64_t ide3d_png_workspace_bytes(int32_t n, int32_t h, int32_t w, int32_t c, int32_t segment_bytes);
int64_t ide3d_png_out_bytes(int32_t n, int32_t h, int32_t w, int32_t c, int32_t segment_bytes);
int ide3d_png_encode(const uint8_t* frames, int32_t n, int32_t h, int32_t w, int32_t c, int32_t filter_mode, int32_t segment_bytes,
                     void* workspace, int64_t workspace_bytes, uint8_t* out, int64_t out_capacity, int64_t* offsets, void* stream);

/* ---- JPEG: colour, DCT, quantiser and Huffman coding --------------------------------------------- */
/*
 * The compression behind the Motion-JPEG video sink that stands in for
 * `imageio.get_writer(mp4, mode='I', fps=60, codec='libx264', bitrate='10M')` (gen_videos.py:108,131),
 * and `.jpg` stills: frames uint8 [n, h, w, c] contiguous, c = 1 (grey) or 3 (RGB), sides
 * 1..65535, to the n entropy-coded scans of their baseline JPEG files (everything between the SOS
 * header and EOI: the restart intervals with their RSTm markers), back to back in `out`; scan k is
 * out[offsets[k], offsets[k + 1]), offsets int64 [n + 1] in device memory.  The caller adds SOI,
 * APP0, DQT, SOF0, DHT, DRI, SOS and EOI.  training/jpeg.py states every integer of the stream and
 * holds the host definition that gives the same bytes: full-range JFIF Y'CbCr in 16-bit fixed
 * point; subsampling 444 (8 x 8 MCU) or 420 (16 x 16 MCU, chroma (a + b + c + d + 2) >> 2, RGB
 * only) after edge replication to whole MCUs; an integer matrix DCT (13-bit table, 3 fractional
 * bits after each pass, error at most 0.49 of a coefficient unit); T.81 Annex K tables scaled by
 * `quality` 1..100 with the IJG rule, division rounding half away from zero; Annex K's Huffman
 * tables; restart intervals of `restart_interval` MCUs (1..65535), each starting with DC
 * predictors 0, padded with 1-bits to a byte, FF stuffed with 00, followed by RSTm (m = index
 * mod 8) except the frame's last.  Three launches (interval, scan, compact); integer arithmetic,
 * integer LDS atomics only: two runs are bit-equal.
 * workspace: ide3d_jpeg_workspace_bytes() bytes (-1: unsupported call), 16-byte aligned: one
 * worst-case slot per interval, their sizes and positions.  out_capacity >= ide3d_jpeg_out_bytes()
 * = n * sum over the frame's intervals of 2 * ceil(1658 * blocks / 8) + 2 (a block is at most
 * 20 + 63 * 26 bits, every byte stuffed).  Refused with IDE3D_EINVAL before any launch: c not in
 * {1, 3}, quality outside 1..100, an unknown subsampling, 420 with c = 1, restart_interval
 * outside 1..65535, an empty axis, a side above 65535, a workspace or out below those sizes, and
 * any of the frames, the workspace or out at or above 2^31 bytes.
 */
int64_t ide3d_jpeg_workspace_bytes(int32_t n, int32_t h, int32_t w, int32_t c, int32_t subsampling, int32_t restart_interval);
int64_t ide3d_jpeg_out_bytes(int32_t n, int32_t h, int32_t w, int32_t c, int32_t subsampling, int32_t restart_interval);
int ide3d_jpeg_encode(const uint8_t* frames, int32_t n, int32_t h, int32_t w, int32_t c, int32_t quality, int32_t subsampling,
                      int32_t restart_interval, void* workspace, int64_t workspace_bytes, uint8_t* out, int64_t out_capacity,
                      int64_t* offsets, void* stream);

/* ---- generator metrics on detector features: FID moments, KID sums, precision / recall ---- */
/*
 * What calc_metrics.py does with a detector's features once they exist.  Features are fp32,
 * row-major, K-contiguous, with a row stride >= d in elements.  Limits, refused beyond with
 * IDE3D_EINVAL before the first launch: 1 <= d <= 8192, 1 <= n <= 2^22 rows, 1 <= k <= 7,
 * 2 <= m <= 4096, 1 <= subsets <= 4096; also null pointers, a row stride below d and a workspace
 * below ide3d_metrics_workspace_bytes() or not 16-byte aligned.  No float atomics: every output
 * has one owner or is reduced from per-workgroup partials by a second launch in a fixed order,
 * so two runs are bit-equal.
 *
 * ide3d_feature_moments replaces `FeatureStats.append` (metrics/metric_utils.py:107-122):
 *   raw_mean[j] += sum_i x[i,j], raw_cov[j,k] += sum_i x[i,j] * x[i,k], float64 sums (one FMA per
 *   row in row order, products exact) into the caller's running [d] and [d, d] buffers.  Both
 *   triangles of raw_cov are written from one computed value (read from the upper one).
 *
 * The other three run on one pair engine: A[rows, d] . B[cols, d]^T in 128 x 128 tiles on
 * v_mfma_f32_32x32x2f32, each dot product one chain over k in order with fp32 rounding, the same
 * bits for (a, b) and (b, a).  The pair matrix is never written out.
 *
 * ide3d_poly_kernel_sums replaces the subset loop of metrics/kernel_inception_distance.py:34-43:
 *   xi, yi int32 [subsets, m] row indices into x [nx, d] and y [ny, d] (clamped into range);
 *   sums float64 [subsets, 3] = (sum_{i != j} p(x_i, x_j), sum_{i != j} p(y_i, y_j),
 *   sum_{i, j} p(x_i, y_j)) over the positions i, j of the subset, p(a, b) = (dot(a, b) / d + 1)^3
 *   with the division, the cube and the sums in float64.
 *
 * ide3d_knn_radii and ide3d_manifold_inside replace metrics/precision_recall.py:19-59:
 *   d2(a, b) = max(0, (|a|^2 + |b|^2) - 2 dot(a, b)) in fp32, the squared norms summed in float64
 *   and rounded once to fp32 (a launch of their own, into the workspace).
 *   radii_sq[i] = the (k + 1)-th smallest over all j of d2(f_i, f_j), the pair j == i counting as
 *   exactly 0 (`kthvalue(nhood_size + 1)` over a row that holds the point itself); n <= k refused.
 *   inside[p] (uint8) = 1 when d2(probe_p, manifold_j) <= radii_sq[j] for some j, else 0.
 *
 * ide3d_metrics_workspace_bytes(op, rows, cols, d, k_or_subsets): rows x cols are the sides of the
 * pair matrix (m, m for POLY; n, n for RADII; np, nm for INSIDE); -1 for arguments the entry
 * points refuse.  POLY: 8 bytes per (subset, sum, tile).  RADII: n norms, then 8 candidates per
 * row and column split.  INSIDE: np + nm norms, then one byte per probe and column split.  Row
 * tiles = ceil(rows / 128), column splits = min(column tiles, max(1, 1024 / row tiles)).
 */
#define IDE3D_METRICS_POLY   0
#define IDE3D_METRICS_RADII  1
#define IDE3D_METRICS_INSIDE 2
int64_t ide3d_metrics_workspace_bytes(int32_t op, int64_t rows, int64_t cols, int32_t d, int32_t k_or_subsets);
int ide3d_feature_moments(const float* x, int64_t n, int32_t d, int64_t row_stride, double* raw_mean, double* raw_cov, void* stream);
int ide3d_poly_kernel_sums(const float* x, int64_t nx, int64_t x_stride, const float* y, int64_t ny, int64_t y_stride, int32_t d,
                           const int32_t* xi, const int32_t* yi, int32_t subsets, int32_t m, void* workspace, int64_t workspace_bytes,
                           double* sums, void* stream);
int ide3d_knn_radii(const float* f, int64_t n, int32_t d, int64_t row_stride, int32_t k, void* workspace, int64_t workspace_bytes, float* radii_sq,
                    void* stream);
int ide3d_manifold_inside(const float* probes, int64_t np, int64_t probe_stride, const float* manifold, int64_t nm, int64_t manifold_stride,
                          int32_t d, const float* radii_sq, void* workspace, int64_t workspace_bytes, uint8_t* inside, void* stream);

/* ---- adaptive discriminator augmentation: the geometric and colour stages ---- */
/*
 * ide3d_augment_geometric replaces training/augment.py:290-306 (reflect F.pad, upsample2d,
 * affine_grid + grid_sample, downsample2d) with one launch and no intermediate in device memory:
 *   P[i, j] = x[r(i - my0), r(j - mx0)], r = one reflection; zero outside the padded extent;
 *   U[j]    = 2 * sum_k taps[k] * P[(j + 5 - k) / 2] over the k with j + 5 - k even, per axis;
 *   S[i, j] = bilinear sample (zero outside U) of U at (coords[0] j + coords[1] i + coords[2],
 *             coords[3] j + coords[4] i + coords[5]), for 0 <= i < 2 (h + 6), 0 <= j < 2 (w + 6);
 *   y[o]    = sum_k taps[k] * S[2 o + 1 + k], per axis: exactly [h, w].
 * x, y [n, c, h, w] contiguous float32.  margins = (mx0, my0, mx1, my1): four int32 ON THE DEVICE
 * (augment.py:278-288, batch-wide), clamped to [0, side - 1] again by the kernel.  coords [n, 6]
 * on the device: lines 292-301 and the two unnormalisations of affine_grid / grid_sample folded
 * into one map from S pixel indices to U pixel coordinates.  taps: the 12 floats of Hz_geom on
 * the device.  color: NULL, or [n, 12] = rows of the 3 x 4 matrix of augment.py:365 applied to
 * the result (c == 3), row 0 as (scale, -, -, offset) for c == 1 (augment.py:367-368).
 * band_loops: NULL, or one int32 on the device that every workgroup raises by one when the
 * window of U under its S tile exceeded its LDS budget and it looped over pieces of the tile.
 * ide3d_augment_geometric_backward is the transpose with respect to x (colour transpose without
 * the offset first): grad_images must be zero-filled, float atomic adds, so two runs agree to
 * rounding and not bit for bit.  ide3d_augment_color is the colour stage alone (lines 363-368),
 * plane = h * w, transpose != 0 for its backward.
 * Refused with IDE3D_EINVAL before any launch: an empty axis, h < 2 or w < 2, a side above
 * 16384, n or c above 65535, a buffer shorter than n c h w floats, null or misaligned pointers,
 * a colour matrix with c other than 3 or 1.
 */
int ide3d_augment_geometric(const float* x, float* y, int32_t n, int32_t c, int32_t h, int32_t w, int64_t x_numel, int64_t y_numel,
                            const float* coords, const int32_t* margins, const float* taps, const float* color, int32_t* band_loops,
                            void* stream);
int ide3d_augment_geometric_backward(const float* grad_out, float* grad_images, int32_t n, int32_t c, int32_t h, int32_t w, int64_t grad_out_numel,
                                     int64_t grad_images_numel, const float* coords, const int32_t* margins, const float* taps,
                                     const float* color, void* stream);
int ide3d_augment_color(const float* x, float* y, int32_t n, int32_t c, int64_t plane, int64_t x_numel, int64_t y_numel, const float* color,
                        int32_t transpose, void* stream);

/* ---- modulated 3x3 / 1x1 convolution (MFMA implicit GEMM) --------------------------------- */
/*
 * Replaces the ATen conv behind `conv2d_gradfix.conv2d` for the StyleGAN2 modulated
 * convolution (inversion/networks.py:55-130 `modulated_conv2d`, stride 1, `flip_weight=True`)
 * with its epilogue (`+ noise`, `bias_act(lrelu)`, networks.py:457-512) fused:
 *   y[n,o,:,:] = act( d[n,o] * sum_{i,ky,kx} w[o,i,ky,kx] * s[n,i] * x[n,i,y+ky-p,x+kx-p]
 *                     + noise_strength * noise[:, :] + b[o] ) * act_gain, clamped.
 * x [n, cin, h, w], y [n, cout, h, w] NCHW contiguous float32; w [cout, cin, k, k];
 * styles s [n, cin]; dcoefs d [n, cout] or NULL (no demodulation); noise [h, w] or NULL;
 * bias [cout] or NULL.  act: 1 linear, 3 lrelu (bias_act cuda_idx).  k in {1, 3}.
 * fp32 in / fp32 out / fp32 accumulate.  Shared-weight 1x1, stride-2, narrow (< 64 output channels, <= 32 input channels) and small
 * (< 12 pixels) layers run on v_mfma_f32_32x32x2_f32 (exact fp32 products); the shared-weight 3x3 and transposed 3x3 layers run in the arithmetic
 * selected by `arith` / ide3d_set_conv_arithmetic() below.
 */
typedef struct ide3d_modconv_params {
    const float* x; const float* w; const float* styles; const float* dcoefs;
    const float* noise; const float* bias; float* y;
    int32_t n, cin, cout, h, w_, k;
    float noise_strength;
    int32_t act; float alpha, gain, clamp;
    int32_t mode;             /* 0: stride-1 k x k "same" correlation (y is h x w);
                                 1: 3x3 correlation, stride 2, no padding (y is ((h-3)/2+1) x ((w-3)/2+1)) — the conv that
                                    follows the low-pass filter of a down-sampling Conv2dLayer (conv2d_resample.py:100-103;
                                    styles / dcoefs may be NULL: plain convolution, inversion/networks.py:169-226);
                                 2: 3x3 transposed convolution, stride 2, pad 0 (y is (2h+1) x (2w+1)) —
                                    `conv_transpose2d(x, w.transpose(0,1), stride=2)` of conv2d_resample.py:114-125 */
    int32_t weights_packed;   /* 1: `workspace` already holds the packed form of `w` from an earlier call */
    float*  workspace;        /* scratch of ide3d_modconv_workspace_bytes(): packed weights, then split-K partials */
    int64_t workspace_bytes;
    int64_t w_batch_stride;   /* 0: one weight tensor for the batch (modulation via `styles` on the input);
                                 > 0: per-image weights w + n * w_batch_stride (styles already folded in by the caller:
                                 lets heads with different styles — toRGB + toSeg, networks.py:1109,1130 — share one launch) */
    int32_t arith;            /* arithmetic of the shared-weight 3x3 layers: 0 = process default (ide3d_set_conv_arithmetic),
                                 1 = fp32 MFMA, 3 = bf16x3, 6 = bf16x6, 16 = f16x3 (see ide3d_set_conv_arithmetic) */
    const float* x_amax;      /* NULL, or [n][IDE3D_AMAX_FLOATS]: the row maximum is an upper bound of max |x[n, :, :, :]| (what `y_amax` of the
                                 producing launch holds).  The f16x3 arithmetic needs it to place x * styles inside the fp16 range;
                                 without it a launch that asked for f16x3 runs in bf16x6. */
    float*       y_amax;      /* NULL, or [n][IDE3D_AMAX_FLOATS] float32 zeroed by the caller: row maximum = max |y[n, :, :, :]| (NaNs ignored; an inf makes
                                 the consumer compute that image without range scaling) */
    int32_t      y_pitch;     /* mode 2 only: 0 = dense y [n, cout, 2h+1, 2w+1]; else the row pitch in floats (>= 2w+1) of a y whose rows are padded —
                                 [n, cout, 2h+1, y_pitch] storage, columns >= 2w+1 never written — so that rows start 16-byte aligned for the FIR
                                 that consumes it (ide3d_upfirdn2d_ex stages aligned rows with 16-byte loads) */
} ide3d_modconv_params;

int64_t ide3d_modconv_workspace_bytes(int32_t n, int32_t cin, int32_t cout, int32_t h, int32_t w, int32_t k, int32_t mode,
                                      int32_t per_image_weights);
int ide3d_modconv2d(const ide3d_modconv_params* p, void* stream);

/* A 3x3 layer (ide3d_modconv_params, mode 0) and the dual 1x1 heads that read its output (toRGB + toSeg with per-image folded weights:
 * what ide3d_modconv2d computes for them with w_batch_stride > 0, act linear, gain 1) in ONE launch: the heads run in the epilogue of
 * the workgroup that holds all cout channels of its pixels.  Results are bit-equal to the two ide3d_modconv2d calls.  Returns
 * IDE3D_ENOKERNEL (nothing launched) unless the layer runs in bf16x6 on one 128- or 64-channel block without split-K on 16 x 16 /
 * 32 x 16 tiles that cover the map, with y_amax = NULL and y_pitch = 0, and the heads take the split-bf16 path with <= 32 or
 * 161..192 rows; and when IDE3D_MODCONV_NO_HEAD_FUSION is set.  The caller then makes the two calls. */
typedef struct ide3d_modconv_head_epilogue {
    const float* w;           /* [n, rows, cin] per-image head weights (cin = the layer's cout), styles folded in */
    const float* bias;        /* [rows] or NULL */
    float*       y;           /* [n, rows, h, w] head output */
    int32_t      rows;
    float        clamp;       /* < 0: none */
    int32_t      no_activation_output;   /* 1: the layer's own output is not written (p->y may be NULL) */
    float*       workspace;   /* packed head weights: ide3d_modconv_workspace_bytes(n, cin, rows, h, w, 1, 0, 1) bytes */
    int64_t      workspace_bytes;
} ide3d_modconv_head_epilogue;
int ide3d_modconv2d_heads(const ide3d_modconv_params* p, const ide3d_modconv_head_epilogue* heads, void* stream);

/*
 * ABI 8 (entry points added).  The plane gate: the last backbone block writes only the tri-plane texels the renderer of the same call can
 * read.
 *
 * ide3d_plane_cells fills cells [n, 3, cells_h, cells_w] bytes, cells_h = ceil(H / 4), cells_w = ceil(W / 4): a cell is a 4 x 4 block of
 * texels of one plane (0: xy, 1: yz, 2: xz, the order of sample_from_triplane) of an H x W tri-plane, and is 1 when a sample that
 * ide3d_render_rays can take for this camera (rays_d_cam [rays_per_img, 3], z_lin [steps], cam2world [n, 16]: its own arguments) addresses
 * a texel in it, whatever the jitter draw: for every ray and step, the texel rectangle spanned by the taps of the jitter draws 0 and 1,
 * widened by one texel on every side and clamped into the plane like the marcher's own addresses (csrc/triplane_tap.h `tap_addr`: the
 * zero-weight loads of a tap outside the plane land on the border texels).  The map is zeroed first, in the same stream.
 *
 * A launch that is given a gate leaves every workgroup whose output tile has no set cell under it (see each entry point) before it reads
 * or writes anything else: those output elements keep what the buffer held.  gate == NULL, gate->cells == NULL, or IDE3D_NO_PLANE_GATE
 * in the environment (read per call): the dense launch.  The texels under set cells are bit-equal to the dense launch's.
 */
typedef struct ide3d_plane_gate {
    const uint8_t* cells;     /* [n, 3, cells_h, cells_w] */
    int32_t        cells_h, cells_w;
    const int32_t* tile_list; /* NULL, or ide3d_plane_tile_list's output for tile_h x tile_w tiles: see there */
    int32_t        tile_h, tile_w;
} ide3d_plane_gate;
int ide3d_plane_cells(const float* rays_d_cam, const float* z_lin, const float* cam2world, int32_t n, int32_t rays_per_img, int32_t steps,
                      int32_t H, int32_t W, uint8_t* cells, void* stream);
/* The live tiles of a map, compacted on the device: list[0] = their number, list[1 ...] = their indices (image * tiles_y + ty) * tiles_x + tx
 * in ascending order, for the tile_h x tile_w-texel tiles (multiples of 4) of an h x w output; a tile is live iff a cell of any plane lies
 * under it.  list holds 1 + n * tiles_y * tiles_x entries.  One small launch.  A gated launch that is handed the list of ITS tile size
 * (ide3d_plane_gate.tile_list / tile_h / tile_w) gives workgroup i the i-th live tile and sends the workgroups past the count home: the
 * live tiles then spread evenly over the XCDs whatever their position (without the list a workgroup keeps its tile, and the XCD that
 * owns the most live tiles sets the launch's length).  A list of another tile size is ignored. */
int ide3d_plane_tile_list(const ide3d_plane_gate* gate, int32_t n, int32_t h, int32_t w, int32_t tile_h, int32_t tile_w, int32_t* list, void* stream);
/* ide3d_modconv2d_heads whose workgroups are live iff a cell of ANY of the three planes lies under their output tile (4 * cells_h >= h,
 * 4 * cells_w >= w required). */
int ide3d_modconv2d_heads_gated(const ide3d_modconv_params* p, const ide3d_modconv_head_epilogue* heads, const ide3d_plane_gate* gate, void* stream);

/*
 * Frozen-generator backward of the synthesis convolutions (gradients for the layer inputs and the styles; weights, biases and affines
 * frozen).  Replaces the autograd of `modulated_conv2d` + `bias_act` (inversion/networks.py:55-130, SynthesisLayer :457-512), of the
 * transposed up-sampling convolution (conv2d_resample.py:112-129) and of ToRGBLayer (:670-713).  The matrix work is ide3d_modconv2d
 * (input gradient of a stride-1 layer: mode 0 with w.transpose(0,1).flip(2,3) and styles = dcoefs; of an up-sampling layer: mode 1 with
 * w.transpose(0,1); of the dual heads: per-image transposed folded weights); these entry points are the streaming and reduction passes
 * around it.  Reductions use fixed-order partial sums and a second launch, no atomics: results are bit-reproducible from run to run.
 *
 * ide3d_modconv_act_backward (K1).  act 1 / 3: dz = the grad = 1 form of ide3d_bias_act with yref = y, dy = NULL (bit-equal to it) and,
 * when ddcoefs != NULL, ddcoefs[n, c] = sum_p dz * (u - noise_strength * noise - bias) / dcoefs[n, c], u = the pre-activation recovered
 * from y (lrelu inverted; clamped elements have dz = 0).  act 0 (dot-only form): ddcoefs[n, c] = sum_p dy * y / dcoefs[n, c], dz unused.
 * dy, dz [n, c, h, w] dense; y [n, c, h, y_pitch] (y_pitch 0 = w: dense; else padded rows, e.g. the `y_pitch` output of a mode-2
 * ide3d_modconv2d); noise [h, w] or NULL; bias [c] or NULL.  workspace: ide3d_act_bwd_workspace_bytes() bytes (needed with ddcoefs only).
 */
typedef struct ide3d_act_bwd_params {
    const float* dy;
    const float* y;
    float*       dz;
    const float* noise;
    float        noise_strength;
    const float* bias;
    const float* dcoefs;
    float*       ddcoefs;
    int32_t      n, c, h, w, y_pitch;
    int32_t      act;
    float        alpha, gain, clamp;
    float*       workspace;
    int64_t      workspace_bytes;
} ide3d_act_bwd_params;

int64_t ide3d_act_bwd_workspace_bytes(int32_t n, int32_t c, int32_t h, int32_t w);
int ide3d_modconv_act_backward(const ide3d_act_bwd_params* p, void* stream);

/* K2: dx = styles[n, c] * t and dstyles[n, c] = sum_p x * t; x, t, dx [n, c, h, w] dense, workspace of ide3d_act_bwd_workspace_bytes(). */
int ide3d_modconv_scale_dot(const float* x, const float* t, const float* styles, float* dx, float* dstyles,
                            int32_t n, int32_t c, int32_t h, int32_t w, float* workspace, int64_t workspace_bytes, void* stream);

/* K3: dw[n, o, i] = sum_p dy[n, o, p] * x[n, i, p] — the gradient of per-image 1x1 weights (ide3d_modconv2d with w_batch_stride > 0, the
 * folded dual heads); dy [n, rows, h, w], x [n, cin, h, w] dense, dw [n, rows, cin].  Exact fp32 FMAs on the vector pipe. */
int64_t ide3d_head_wgrad_workspace_bytes(int32_t n, int32_t rows, int32_t cin, int32_t h, int32_t w);
int ide3d_head_weight_grad(const float* dy, const float* x, float* dw, int32_t n, int32_t rows, int32_t cin, int32_t h, int32_t w,
                           float* workspace, int64_t workspace_bytes, void* stream);

/*
 * Parameter gradients of the synthesis convolutions (PTI pivotal tuning, the generator trainable).
 *
 * ide3d_modconv_weight_grad: the direct weight gradient of a modulated 3x3 convolution, dw [cout, cin, 3, 3] (the demodulation part of
 * the weight gradient is not included: autograd adds it through the dcoefs).  g: the gradient at the convolution output before
 * demodulation; styles [n, cin] and dcoefs [n, cout] (NULL = 1).
 *   mode 0 (stride 1, pad 1, correlation; ide3d_modconv2d mode 0): g [n, cout, h, w],
 *          dw[o, i, ky, kx] = sum_n dcoefs[n, o] styles[n, i] sum_{y,x} g[n, o, y, x] x[n, i, y + ky - 1, x + kx - 1];
 *   mode 2 (transposed, stride 2, pad 0; ide3d_modconv2d mode 2): g [n, cout, 2h + 1, 2w + 1],
 *          dw[o, i, ky, kx] = sum_n dcoefs[n, o] styles[n, i] sum_{y,x} g[n, o, 2y + ky, 2x + kx] x[n, i, y, x];
 *   mode 1 (stride 2, pad 0, correlation; ide3d_modconv2d mode 1; the encoders' down-sampling layers):
 *          g [n, cout, gh, gw] with gh = (h - 3) / 2 + 1, gw = (w - 3) / 2 + 1 (h, w >= 3, else IDE3D_EINVAL),
 *          dw[o, i, ky, kx] = sum_n dcoefs[n, o] styles[n, i] sum_{y,x} g[n, o, y, x] x[n, i, 2y + ky, 2x + kx];
 *          the last row (column) of x is never read when h (w) is even.
 * x [n, cin, h, w]; all dense.  arith: 0 = the process arithmetic (ide3d_get_conv_arithmetic), 1 = exact fp32 products
 * (v_mfma_f32_32x32x2_f32), 6 = bf16x6; 3 (bf16x3) and 16 (f16x3) run bf16x6.  Split-K partial slices per (image, pixel range) in the
 * workspace, added in a fixed order by a second launch: bit-reproducible, no atomics.  Exclusive residency (its matrix loop is LDS-fed
 * bf16).  ide3d_wgrad_workspace_bytes(n, cin, cout, h, w): (h, w) is the grid of pixels the sum runs over, which is the size of x in
 * modes 0 and 2 (the same value for both) and the size of g, (gh, gw), in mode 1; a workspace sized for another grid is refused with
 * IDE3D_EINVAL when it is too small, never indexed past its end.
 */
typedef struct ide3d_wgrad_params {
    const float* g;
    const float* x;
    const float* styles;
    const float* dcoefs;
    float*       dw;
    int32_t      n, cin, cout, h, w;
    int32_t      mode;
    int32_t      arith;
    float*       workspace;
    int64_t      workspace_bytes;
} ide3d_wgrad_params;

int64_t ide3d_wgrad_workspace_bytes(int32_t n, int32_t cin, int32_t cout, int32_t h, int32_t w);
int ide3d_modconv_weight_grad(const ide3d_wgrad_params* p, void* stream);

/* db[c] = sum_{n,p} dz[n, c, p] and, when dnoise != NULL, dnoise[p] = sum_{n,c} dz[n, c, p] (the gradients of a layer's bias and of its
 * [h, w] noise map); dz [n, c, h, w] dense; workspace of ide3d_bias_noise_workspace_bytes().  Fixed-order sums, bit-reproducible. */
int64_t ide3d_bias_noise_workspace_bytes(int32_t n, int32_t c, int32_t h, int32_t w);
int ide3d_bias_noise_grad(const float* dz, float* db, float* dnoise, int32_t n, int32_t c, int32_t h, int32_t w,
                          float* workspace, int64_t workspace_bytes, void* stream);

/* Host-only planning query (no launch, no device access): the kernel family, tile and grid that ide3d_modconv2d would use for `p` in the
 * arithmetic `p->arith` resolves to.  Pointers are not dereferenced (set `x_amax` non-null to plan the f16x3 launch; `x` counts for its
 * alignment only).  For tests of the planner and for tooling; not part of the reference's interface. */
enum { IDE3D_PLAN_FP32 = 0,          /* fp32-MFMA matrix loop (modconv_kernel) */
       IDE3D_PLAN_SPLIT = 1,         /* split-bf16 / fp16 matrix loop (modconv_split_kernel) */
       IDE3D_PLAN_SPLIT_TEAMS = 2,   /* the same, two 4-wave teams per workgroup */
       IDE3D_PLAN_HEAD_SPLIT = 3,    /* per-image 1x1 heads, one tile per workgroup (head_split_kernel) */
       IDE3D_PLAN_HEAD_RESIDENT = 4, /* per-image 1x1 heads, packed weights resident in LDS (head_resident_kernel) */
       IDE3D_PLAN_HEAD_SMALL = 5 };  /* per-image 1x1 heads on maps of <= 256 pixels, fp32 FMAs (head_small_kernel) */
typedef struct ide3d_modconv_plan_info {
    int32_t kind;                    /* IDE3D_PLAN_* */
    int32_t tile_h, tile_w;          /* pixels (transposed: grid positions) per workgroup / team */
    int32_t images_per_tile;
    int32_t rows;                    /* output channels per workgroup / team */
    int32_t waves;                   /* per workgroup */
    int32_t parts, f16;              /* pieces per operand (0: fp32 products), fp16 pieces */
    int32_t split_k;                 /* > 1: partial sums + reduction launch */
    int32_t strip;                   /* transposed: main kernel on the h x w grid + strip kernel */
    int32_t transposed_all_class;
    int32_t reserved;
    int64_t workgroups;              /* of the main launch */
} ide3d_modconv_plan_info;
int ide3d_modconv_plan(const ide3d_modconv_params* p, ide3d_modconv_plan_info* out);

/*
 * Arithmetic of the shared-weight 3x3 / transposed 3x3 layers on 16-pixel-wide tiles (everything else always runs on the
 * fp32 MFMA).  The reference computes these layers with ATen's fp32 convolution (conv2d_gradfix.py:35,40), or in fp16 for
 * the `num_fp16_res` highest resolutions of a released pickle (inversion/networks.py:1058-1060):
 *   1  fp32 MFMA: exact fp32 products, fp32 accumulation (v_mfma_f32_32x32x2_f32);
 *   6  bf16x6: each fp32 operand = 3 bf16 pieces, the 6 products above 2^-24 on v_mfma_f32_32x32x16_bf16, fp32 accumulation:
 *      fp32-grade (per-product error <= ~2^-23 relative) at 6/16 of the fp32 MFMA time;
 *   3  bf16x3: 2 pieces, 3 products, per-product error ~2^-17 relative, 3/16 of the time;
 *  16  f16x3: each operand = 2 fp16 pieces (hi = fp16(a), lo = fp16(a - hi): 22 significand bits), the 3 products hi*hi + hi*lo +
 *      lo*hi on v_mfma_f32_32x32x16_f16, fp32 accumulation: per-product error <= ~2^-21 relative to |w|max(row) * |x s|max(image),
 *      3/16 of the fp32 MFMA time.  fp16's range is handled with exact power-of-two scales: one per weight row (from max |w[o]|,
 *      applied when the weights are packed) and one per image (from `x_amax[n]` * max_i |styles[n, i]|, applied while the patch is
 *      staged), both undone together with the demodulation in the epilogue.  Operands more than 2^17 below their row / image
 *      maximum lose relative (not absolute) precision: an fp16 piece cannot be smaller than 2^-24 of the scaled range.  Needs
 *      `x_amax`; without it the launch runs in bf16x6;
 *   0  back to the process default: environment IDE3D_CONV_ARITH = fp32 | bf16x6 | bf16x3 | f16x3, else bf16x6 (round 4; fp32 before).
 *      A wave of ANOTHER kernel that executes packed fp32 VALU instructions (v_pk_fma_f32 ...) on operands fresh from global memory
 *      returns wrong results on MI355X while a wave on the same SIMD runs a loop of LDS reads + bf16 / fp16 MFMAs.
 *      Every kernel of this library that contains such a loop keeps foreign waves off its SIMDs for as long as the loop runs (8-wave
 *      workgroups whose waves hold 256 registers each, or waves that claim all 512 registers of their SIMD: "exclusive residency"), so
 *      every arithmetic may run beside kernels of other libraries on other streams.
 * The same switch selects the arithmetic of per-image 1x1 heads with <= 32 or 161..192 outputs on grids of >= 512 workgroups, and of the
 * two decoder MLPs inside ide3d_render_rays / ide3d_sample_voxel / ide3d_density_lattice at C = 32, hidden = 64: exact fp32 products
 * on v_mfma_f32_16x16x4_f32 with fp32 (1) selected, bf16x6 (fp32-grade, 3 bf16 pieces per operand on v_mfma_f32_16x16x32_bf16)
 * with any of the split arithmetics (3, 6, 16).
 * Packed weights in a modconv workspace are specific to the arithmetic they were packed for.
 */
int     ide3d_set_conv_arithmetic(int32_t arith);
int32_t ide3d_get_conv_arithmetic(void);

/* ---- per-layer style preparation ------------------------------------------------------------------ */
/*
 * One launch for what precedes a modulated convolution in inference (inversion/networks.py:432, :91-93):
 *   styles[n, :] = (w[n, :] @ affine_w^T) * affine_gain + affine_b * bias_gain          FullyConnectedLayer, :152-165
 *   dcoefs[n, o] = rsqrt( sum_i styles[n, i]^2 * wsq_t[i, o] + 1e-8 ),  wsq_t[i, o] = sum_k W[o, i, k]^2
 * w: rows of `wdim` floats, `w_stride` apart; affine_w [cin, wdim]; affine_b [cin] or NULL; wsq_t [cin, cout];
 * dcoefs may be NULL (no demodulation).
 */
int ide3d_style_demod(const float* w, int64_t w_stride, const float* affine_w, const float* affine_b, const float* wsq_t,
                      int32_t n, int32_t cin, int32_t cout, int32_t wdim, float affine_gain, float bias_gain,
                      float* styles, float* dcoefs, void* stream);

/*
 * Per-image folded weights of the two heads of a dual-path block (toRGB + toSeg share w, networks.py:1093-1130):
 *   out[n, o, i] = W_h[o, i] * (affine_h(w[n]) [i] * gain_h),  h = 0 for o < cout0 else 1;  out [n, cout0 + cout1, cin].
 * Feeds ide3d_modconv2d with w_batch_stride > 0 so that both 1x1 heads are one launch.
 */
int ide3d_fold_heads(const float* w, int64_t w_stride, int32_t n, int32_t cin, int32_t wdim, float affine_gain,
                     const float* a0, const float* b0, const float* w0, int32_t cout0, float gain0,
                     const float* a1, const float* b1, const float* w1, int32_t cout1, float gain1,
                     float* out, void* stream);

/*
 * The two entry points above for ALL layers of a synthesis pass at once: every modulated layer's affine + demodulation in two
 * launches, every block's head folding in one (round 3: as 43 separate nodes of a captured graph they delay the first convolution
 * of the pass by ~0.4 ms).  A job carries exactly the per-layer arguments of ide3d_style_demod / ide3d_fold_heads; n (images) and
 * wdim are shared by the jobs.  Same code per block as the per-layer kernels: bit-identical results.  njobs <= IDE3D_STYLE_BATCH_MAX;
 * ide3d_style_demod_batch: n <= 8.
 */
#define IDE3D_STYLE_BATCH_MAX 24
typedef struct ide3d_style_job {
    const float* w; int64_t w_stride;                 /* this layer's latent of image 0, stride to the next image */
    const float* affine_w; const float* affine_b;     /* [cin, wdim], [cin] or NULL */
    const float* wsq_t;                               /* [cin, cout] or NULL (no demodulation) */
    int32_t cin, cout;
    float affine_gain, bias_gain;
    float* styles; float* dcoefs;                     /* [n, cin]; [n, cout] or NULL */
} ide3d_style_job;
typedef struct ide3d_fold_job {
    const float* w; int64_t w_stride;
    int32_t cin; float affine_gain;
    const float *a0, *b0, *w0; int32_t cout0; float gain0;
    const float *a1, *b1, *w1; int32_t cout1; float gain1;
    float* out;                                       /* [n, cout0 + cout1, cin] */
} ide3d_fold_job;
int ide3d_style_demod_batch(const ide3d_style_job* jobs, int32_t njobs, int32_t n, int32_t wdim, void* stream);
int ide3d_fold_heads_batch(const ide3d_fold_job* jobs, int32_t njobs, int32_t n, int32_t wdim, void* stream);

/* ---- the low-resolution block group of the backbone in one call (round 6, ABI 7) ------------------- */
/*
 * The first blocks of the dual-path StyleGAN2 backbone (inversion/networks.py:966-1139: 4^2, 8^2, 16^2 ... while all images' maps of a layer
 * fit one CU's LDS beside a weight slice) — every 3x3 / up-sampling SynthesisLayer (networks.py:330-514) with its noise, bias, lrelu,
 * gain and clamp, the 4x4 FIR of the up-sampling layers (conv2d_resample.py:112-129), the toRGB + toSeg heads (networks.py:670-713) and the
 * skip accumulation `img = upsample2d(img) + y` (networks.py:1100,1121) — in ONE call, one launch per phase (a layer's GEMM, its reduction
 * + epilogue, the heads).  All layers have C input and C output channels (C % 32 == 0); fp32 in / fp32 out; products in
 * the bf16x6 (or bf16x3) arithmetic of ide3d_set_conv_arithmetic, heads in plain fp32 FMAs.  Inference only.
 *   layer l: up = 1: y = lrelu(d * conv3x3(x * s) + noise + b, 0.2) * act_gain, clamped;   up = 2: the same with
 *            conv_transpose2d(stride 2) -> upfirdn2d(f, pad 1, gain 4) in place of the convolution (output 2 x the input resolution);
 *            head >= 0: heads[head] is applied to this layer's output: skip = clamp(W[n] y + b) + upsample2d(heads[head - 1].skip, f).
 *   x0: the group's input [C, res0, res0] (x0_batch_stride == 0: the learned constant, shared by the batch) or [n, C, res0, res0].
 *   x_out: the last layer's output [n, C, res, res] NCHW.  heads[k].skip [n, O, res_k, res_k] NCHW (every head's skip image is written).
 * Returns IDE3D_ENOKERNEL when the arithmetic is fp32 / f16x3 or the layers do not fit (ask ide3d_lowres_layers_supported): callers then
 * run the layers one by one (ide3d_modconv2d ...).
 */
#define IDE3D_LOWRES_MAX_LAYERS 8
#define IDE3D_LOWRES_MAX_HEADS 4
typedef struct ide3d_lowres_layer {
    const float* weight;      /* [C, C, 3, 3] */
    const float* styles;      /* [n, C] */
    const float* dcoefs;      /* [n, C] */
    const float* noise;       /* [res, res], already multiplied by noise_strength, or NULL */
    const float* bias;        /* [C] or NULL */
    float act_gain, clamp;    /* clamp < 0: none */
    int32_t up;               /* 1 or 2 */
    int32_t head;             /* index into heads[], or -1 */
    int32_t weights_packed;   /* 1: the workspace already holds this layer's packed weights (same weight version, same arithmetic) */
    int32_t reserved;
} ide3d_lowres_layer;
typedef struct ide3d_lowres_head {
    const float* w;           /* [n, O, C] per-image folded weights (ide3d_fold_heads) */
    const float* bias;        /* [O] or NULL */
    float* skip;              /* out [n, O, res, res] */
    float clamp;
    int32_t O;
} ide3d_lowres_head;
typedef struct ide3d_lowres_params {
    const float* x0; int64_t x0_batch_stride;
    const float* fir;         /* [4, 4] resample filter (upfirdn2d.setup_filter([1, 3, 3, 1])) */
    float* x_out;
    void* workspace; int64_t workspace_bytes;
    int32_t n, C, res0, nlayers, nheads;
    int32_t arith;            /* 0 = process default; only 6 (bf16x6) and 3 (bf16x3) have this form */
    int32_t reserved0;        /* not read: it selected a launch form that no longer exists; keeps the struct layout */
    int32_t reserved;
    ide3d_lowres_layer layers[IDE3D_LOWRES_MAX_LAYERS];
    ide3d_lowres_head heads[IDE3D_LOWRES_MAX_HEADS];
} ide3d_lowres_params;
/* number of leading layers (ups[l] in {1, 2}) of a group that starts at res0 which ide3d_lowres_group accepts for this batch size */
int32_t ide3d_lowres_layers_supported(int32_t n, int32_t C, int32_t res0, const int32_t* ups, int32_t nlayers, int32_t arith);
/* host only: for each of those layers, phase R's row bands per (image, channel block) and the LDS bytes its largest band needs beside the weight
 * slice (bands / scratch_bytes: nlayers entries each, or NULL); returns the same count as ide3d_lowres_layers_supported */
int32_t ide3d_lowres_phase_r_plan(int32_t n, int32_t C, int32_t res0, const int32_t* ups, int32_t nlayers, int32_t arith,
                                  int32_t* bands, int64_t* scratch_bytes);
int64_t ide3d_lowres_workspace_bytes(const ide3d_lowres_params* p);     /* only n, C, res0, nlayers, arith and layers[].up are read */
int ide3d_lowres_group(const ide3d_lowres_params* p, void* stream);

/* ---- output post-processing -------------------------------------------- */
/* ---- mapping network ---------------------------------------------------------------------- */
/*
 * `MappingNetwork.forward` (inversion/networks.py:287-325) in one launch: normalize_2nd_moment(z), embed(c) + normalize,
 * concat, `layers` x FullyConnectedLayer(lrelu, lr_multiplier), broadcast to num_ws, truncation towards w_avg.
 * z [n, z_dim], c [n, c_dim], embed_w [embed, c_dim], fc_w[l] [fc_out[l], in_l] (in_0 = z_dim + embed, in_l = fc_out[l-1]):
 * dense float32 with the RAW parameters; the runtime gains are applied here like FullyConnectedLayer does
 * (weight_gain = lr_multiplier / sqrt(in), bias_gain = lr_multiplier; the embed layer's gains are passed explicitly).
 * ws [n, num_ws, fc_out[layers-1]] is written.  truncation_psi == 1 disables truncation; truncation_cutoff < 0 = all layers.
 * workspace: ide3d_mapping_workspace_bytes() bytes of device memory (one activation buffer per layer + barrier counter + error word).
 * n <= 8, widths <= 1024 and multiples of 4; returns IDE3D_EINVAL otherwise (callers then use their generic path).
 */
typedef struct ide3d_mapping_params {
    const float* z; const float* c;
    const float* embed_w; const float* embed_b;
    const float* fc_w[16]; const float* fc_b[16];
    int32_t fc_out[16];
    const float* w_avg;
    float* ws;
    void* workspace; int64_t workspace_bytes;
    int32_t n, z_dim, c_dim, embed, layers, num_ws;
    float embed_weight_gain, embed_bias_gain, lr_multiplier, alpha, act_gain, truncation_psi;
    int32_t truncation_cutoff;
} ide3d_mapping_params;

int ide3d_mapping_workspace_bytes(void);
/* Always 1 since round 6 (ABI 7): where the one-launch kernel's 64 workgroups are not co-resident on the current device (its grid-wide barrier needs that;
 * checked against the occupancy query with a 2x margin) `ide3d_mapping` runs the same layers as one launch each. */
int ide3d_mapping_supported(void);
int ide3d_mapping(const ide3d_mapping_params* p, void* stream);

/* ---- resampling between the big kernels of G.synthesis ---------------------------------- */
/*
 * out = upsample2d(lo, [1,3,3,1]) + add, written CHANNELS-LAST: the last skip accumulation of the tri-plane backbone
 * (`img = upfirdn2d.upsample2d(img, resample_filter) + torgb(x)`, inversion/networks.py:1100-1111; upsample2d =
 * upfirdn2d(up=2, pad (2,1,2,1), gain 4), torch_utils/ops/upfirdn2d.py:313-349) producing the layout the ray-marcher gathers
 * from (32-channel texels = 128-byte lines) instead of NCHW + two transposing copies.
 * lo [n, c, h, w] and add [n, c, 2h, 2w]: float32, element strides; out: float32 [n, 2h, 2w, c] dense (= a torch
 * channels_last [n, c, 2h, 2w]), 16-byte aligned, c % 4 == 0.
 */
int ide3d_skip_upsample_add_cl(const float* lo, const int64_t lo_stride[4], const float* add, const int64_t add_stride[4],
                               int32_t n, int32_t c, int32_t h, int32_t w, float* out, void* stream);
/* ABI 8 (entry point added).  The same launch under a plane gate (ide3d_plane_gate above; 4 * cells_h >= 2h, 4 * cells_w >= 2w): the
 * workgroup of an 8 x 32 output tile of the 32-channel group cg is live iff a cell of plane cg % 3 lies under it — c must be a multiple of
 * 96: every 96 channels are one tri-plane tensor, three planes of 32. */
int ide3d_skip_upsample_add_cl_gated(const float* lo, const int64_t lo_stride[4], const float* add, const int64_t add_stride[4],
                                     int32_t n, int32_t c, int32_t h, int32_t w, float* out, const ide3d_plane_gate* gate, void* stream);

/*
 * torch.nn.functional.interpolate(x, scale 2, mode='bilinear', align_corners=False) of x [n, c, h, w] (dense NCHW float32),
 * split into up to three dense NCHW outputs: dst[k] [n, c_count[k], 2h, 2w] takes input channels c_begin[k] ...
 * (the composited 64x64 feature image -> colour features / raw RGB / semantic logits of the super-resolution blocks,
 * SURVEY.md Appendix B; ATen source-index rule `area_pixel_compute_source_index`).  c_count[k] == 0 skips output k.
 * ABI 8: dst_batch_floats (may be NULL = all dense) — floats between consecutive images of output k, 0 = dense (c_count[k] * 2h * 2w): outputs that
 * are channel ranges of ONE tensor (raw RGB | semantic logits, which the skip up-sampler of the next block then reads in one launch).
 */
int ide3d_bilinear_up2_split(const float* x, int32_t n, int32_t c, int32_t h, int32_t w,
                             float* const dst[3], const int32_t c_begin[3], const int32_t c_count[3], const int64_t* dst_batch_floats, void* stream);

/*
 * `mask2color(seg)` (dnnlib/seg_tools.py:75-81: argmax over the class channel + palette) and
 * the uint8 conversion of `layout_grid` (dnnlib/util.py:632-646), fused: writes one
 * [n, H, 2W, 3] uint8 frame per image = RGB | coloured segmentation side by side, the
 * `image_seg` layout of gen_videos.py:133-135.
 * img [n, 3, H, W], seg [n, classes, H, W] float32 NCHW; palette uint8 [classes, 3].
 */
int ide3d_frame_u8(const float* img, const float* seg, const uint8_t* palette,
                   int32_t n, int32_t classes, int32_t H, int32_t W, uint8_t* out, void* stream);

/*
 * ABI 8.  The camera-pose helpers of training/volumetric_rendering.py as two launches (the reference spells them as ~45 one-element
 * tensor operations per pose: ~0.3 ms of host time per image in gen_images.py:104-106 / gen_videos.py:120-124).  One thread per camera;
 * every operation rounds on its own, in the reference's order.
 *
 * ide3d_sphere_points — the tail of `sample_camera_positions` (:186-193) and the middle of `LookAtPoseSampler.sample` (:281-291):
 *   theta [n], pitch [n] float32 (the caller has drawn them: the random modes keep torch's generator);
 *   pitch_is_v == 0: phi = clamp(pitch, 1e-5, pi - 1e-5);   pitch_is_v == 1: phi = arccos(1 - 2 * (clamp(pitch, ...) / pi));
 *   pos [n, 3] = r * (sin phi cos theta, cos phi, sin phi sin theta);  phi_out [n] (may be NULL) = phi.
 * ide3d_cam2world — `create_cam2world_matrix(forward_vector, origin)` (:195-213): out [n, 4, 4] = T(origin) @ R(columns -left, up, -forward)
 *   with forward normalised, left = normalise(cross((0, 1, 0), forward)), up = normalise(cross(forward, left)).
 *   lookat != NULL (LookAtPoseSampler :294-295): forward = normalise(lookat - origin) first (`forward` is ignored, may be NULL);
 *   lookat_stride = 3 (one point per camera) or 0 (one point for all).
 */
int ide3d_sphere_points(const float* theta, const float* pitch, int32_t n, float r, int32_t pitch_is_v,
                        float* pos, float* phi_out, void* stream);
int ide3d_cam2world(const float* forward, const float* origin, const float* lookat, int32_t lookat_stride, int32_t n,
                    float* out, void* stream);

/*
 * ABI 8 (entry points added).  The projector's per-step work on the trainable noise maps, batched over all maps (csrc/noise_reg.hip, DESIGN.md
 * section 5.13).  `table`: k entries in DEVICE memory, one per map: a dense fp32 [side, side] map, side a power of two in 4..512.  `sides`:
 * the same k sides in HOST memory (the launch geometry and the buffer layout follow from them alone; table[i].side must equal sides[i]).
 * The number of launches does not depend on k or on the sides; no atomics, fixed-order sums, bit-reproducible; no host synchronisation.
 *
 * ide3d_noise_reg — the noise regulariser of the reference's projectors (inversion/training/projectors/w_projector_ide3d.py:114-122):
 *   loss[0] = sum over maps and pyramid levels of mean(n * roll(n, 1, x))^2 + mean(n * roll(n, 1, y))^2, the levels of a map being side,
 *   side / 2, ..., 8 by 2x2 average pooling (one level for side <= 8), the rolls wrapping around.  means [ide3d_noise_reg_levels(), 2]
 *   receives (m_x, m_y) of every (map, level) in table order, and the workspace (ide3d_noise_reg_workspace_bytes()) keeps the pooled
 *   levels; the backward reads both.
 * ide3d_noise_reg_backward — d loss / d map of the same (:123 and autograd's walk back through :116-122), for the table, workspace and
 *   means of the forward call: at level L a pixel receives (2 m_x (n_left + n_right) + 2 m_y (n_up + n_down)) / N_L, spread to its 4^L
 *   level-0 descendants with weight 4^-L.  dloss: DEVICE pointer to the upstream scalar gradient, multiplied in once per level-0 pixel.
 *   grad: the maps' gradients back to back in table order (sum of side^2 floats).
 * ide3d_noise_normalize — the re-normalisation after the optimiser step (:140-142), in place and in the reference's order:
 *   n -= mean(n); n *= rsqrt(mean(n^2)).  Workspace of ide3d_noise_normalize_workspace_bytes().
 */
typedef struct ide3d_noise_map {
    float*  data;
    int32_t side;
    int32_t reserved;
} ide3d_noise_map;

int64_t ide3d_noise_reg_workspace_bytes(const int32_t* sides, int32_t k);
int ide3d_noise_reg_levels(const int32_t* sides, int32_t k);
int ide3d_noise_reg(const ide3d_noise_map* table, const int32_t* sides, int32_t k, float* workspace, int64_t workspace_bytes,
                    float* means, float* loss, void* stream);
int ide3d_noise_reg_backward(const ide3d_noise_map* table, const int32_t* sides, int32_t k, const float* workspace, int64_t workspace_bytes,
                             const float* means, const float* dloss, float* grad, void* stream);
int64_t ide3d_noise_normalize_workspace_bytes(const int32_t* sides, int32_t k);
int ide3d_noise_normalize(const ide3d_noise_map* table, const int32_t* sides, int32_t k, float* workspace, int64_t workspace_bytes,
                          void* stream);

/*
 * ABI 8 (entry points added).  The VGG16 LPIPS distance of the reference's projectors and coaches and its image gradient: everything that
 * is not a convolution (csrc/lpips.hip; the convolutions are ide3d_modconv2d, the interior ReLU gradients
 * ide3d_modconv_act_backward).  All tensors dense NCHW fp32 in device memory.  No atomics, fixed-order sums, bit-reproducible; no host
 * synchronisation.
 *
 * ide3d_lpips_prep — what stands in front of the feature net (inversion/training/projectors/w_projector_ide3d.py:104-107: 0..255 images
 *   area-down-sampled to 256 x 256; inversion/criteria/lpips/networks.py:49-50: the z-score): x [n, 3, H, W] -> y [n, 3, H / f, W / f],
 *   y = ((mean of the f x f block) * in_scale + in_shift - mean[c]) / std[c]; f >= 1 divides H and W; mean, std: 3 floats each (DEVICE).
 * ide3d_lpips_prep_backward — its adjoint (autograd's walk back through the same lines): dx = dy[.., Y / f, X / f] * in_scale / (f^2 std[c]).
 * ide3d_maxpool2 — torchvision's `MaxPool2d(2, 2)` between the stages (networks.py:91, layers 4, 9, 16, 23): [planes, h, w] ->
 *   [planes, h / 2, w / 2], floor on odd sides, bit-equal to ATen's.
 * ide3d_lpips_stage_backward — at the last layer of a stage (networks.py:56-59: the activation feeds the tap AND the next stage), what
 *   autograd does in three passes (max-pool backward, add, ReLU backward): dz = (route(dpool) + dtap) where y > 0, else 0.  y, dtap, dz
 *   [planes, h, w]; dpool [planes, h / 2, w / 2] or NULL (the last stage); `route` sends a pooled gradient to the first maximum of its
 *   window; a row / column that the floor dropped receives dtap only.  The result does not depend on the tie rule: y >= 0, a tie at a
 *   positive maximum needs two equal convolution outputs, and a tie at 0 is masked.
 * ide3d_lpips_head — the distance from the taps (inversion/criteria/lpips/utils.py:6-8, lpips.py:32-35): per tap u = a / (sqrt(sum_c a^2) +
 *   1e-10), d = mean_{h,w} sum_c lin[c] (u - t)^2 against the cached normalised target t; loss[0] = sum over taps and images of d / n.
 *   k launches (per-workgroup partial sums -> workspace of ide3d_lpips_head_workspace_bytes()) + 1 finishing launch.  loss == NULL: the
 *   normalise-only form, out = u of every tap (k launches; t, lin, workspace unused).
 * ide3d_lpips_head_backward — d loss / d a of the same in closed form, written to `out` of every tap (k launches): s = 2 dloss / (n h w),
 *   g_c = s lin[c] (u_c - t_c), da_c = g_c / (|a| + eps) - a_c (sum_k g_k a_k) / (|a| (|a| + eps)^2), the second term 0 where |a| = 0 (the
 *   reference's autograd yields NaN there: sqrt at 0).  dloss: DEVICE pointer to the upstream scalar gradient.
 */
#define IDE3D_LPIPS_MAX_TAPS 8
typedef struct ide3d_lpips_tap {
    const float* a;        /* [n, c, h, w] the tap's activation */
    const float* t;        /* [n, c, h, w] normalised target features */
    const float* lin;      /* [c] */
    float*       out;      /* [n, c, h, w]: u (normalise-only form) or d loss / d a (backward) */
    int32_t      c, h, w;
    int32_t      reserved;
} ide3d_lpips_tap;

int ide3d_lpips_prep(const float* x, float* y, const float* mean, const float* std_, int32_t n, int32_t H, int32_t W, int32_t f,
                     float in_scale, float in_shift, void* stream);
int ide3d_lpips_prep_backward(const float* dy, float* dx, const float* std_, int32_t n, int32_t H, int32_t W, int32_t f,
                              float in_scale, void* stream);
int ide3d_maxpool2(const float* x, float* y, int64_t planes, int32_t h, int32_t w, void* stream);
int ide3d_lpips_stage_backward(const float* y, const float* dpool, const float* dtap, float* dz, int64_t planes, int32_t h, int32_t w,
                               void* stream);
int64_t ide3d_lpips_head_workspace_bytes(const ide3d_lpips_tap* taps, int32_t k, int32_t n);
int ide3d_lpips_head(const ide3d_lpips_tap* taps, int32_t k, int32_t n, float* workspace, int64_t workspace_bytes, float* loss,
                     void* stream);
int ide3d_lpips_head_backward(const ide3d_lpips_tap* taps, int32_t k, int32_t n, const float* dloss, void* stream);

/*
 * ABI 8 (entry points added).  The AlexNet LPIPS distance — the reference's default, `LPIPS(net_type='alex')`
 * (inversion/criteria/lpips/lpips.py:16, networks.py:76-84: torchvision's alexnet().features, taps behind layers 1, 4, 7, 9, 11;
 * apps/train_hybrid_encoder.py:235, inversion/configs/hyperparameters.py `lpips_type`, base_coach.py:44) — and its image gradient: what it
 * needs beside the VGG16 block above (csrc/lpips_alex.hip).  Prep, head and their gradients are the entry points
 * above; all five convolutions and their input gradients are ide3d_modconv2d, the 11x11 stride-4 stem and the 5x5 layer at k = 1 over
 * unfolded patches.  All tensors dense NCHW fp32 in device memory.  No atomics, fixed-order sums, bit-reproducible; no host synchronisation.
 *
 * ide3d_unfold2d — `F.unfold(x, k, padding=pad, stride=stride)` as [n, c k k, ho, wo], ho = (h + 2 pad - k) / stride + 1 (floor), wo
 *   likewise: channel (ci k + ky) k + kx at (oy, ox) is x[ci, oy stride + ky - pad, ox stride + kx - pad], 0 outside the image.  That is the
 *   order of weight.reshape(cout, c k k, 1, 1), so `Conv2d(3, 64, 11, 4, 2)` and `Conv2d(64, 192, 5, 1, 2)` (torchvision alexnet features
 *   0 and 3) are 1x1 convolutions over col.  1 <= k <= 16, 1 <= stride <= k, 0 <= pad < k, ho, wo >= 1, fewer than 2^31 elements in x and
 *   in col.
 * ide3d_fold2d — its adjoint (autograd's walk back through the unfolding) in gather form: dx[ci, y, x] = the sum over ky then kx ascending
 *   of dcol[(ci k + ky) k + kx, (y + pad - ky) / stride, (x + pad - kx) / stride] where both divisions are exact and the position lies
 *   inside ho x wo (<= ceil(k / stride)^2 terms, summed in float64 and rounded once); a row or column that no window reaches gets an
 *   exact 0.  The same limits.
 * ide3d_maxpool3s2p0 — `MaxPool2d(3, 2)` (torchvision alexnet features 2 and 5): [planes, h, w] -> [planes, (h-3)/2+1, (w-3)/2+1],
 *   h, w >= 3, bit-equal to ATen's (the first maximum in row-major window order wins, NaN wins); idx (may be NULL): one byte per output,
 *   the winner as ky * 3 + kx.  (ide3d_maxpool3s2 is the padding-1 geometry.)
 * ide3d_lpips_tap_backward — at a tap (networks.py:56-59: the activation feeds the tap AND the next layer), what autograd does in three
 *   passes: dz = (route(g) + dtap) where y > 0, else 0; y, dtap, dz [planes, h, w].  pooled = 1: g [planes, (h-3)/2+1, (w-3)/2+1] and idx
 *   the forward's winner bytes; each pixel sums g over the <= 4 windows whose winner it is, window rows then columns ascending; a row or
 *   column that the floor dropped receives dtap only.  pooled = 0: g [planes, h, w] is added as it is (a tap that feeds the next
 *   convolution directly), or g == NULL: the last tap, dtap alone.
 */
int ide3d_unfold2d(const float* x, float* col, int32_t n, int32_t c, int32_t h, int32_t w, int32_t k, int32_t stride, int32_t pad,
                   void* stream);
int ide3d_fold2d(const float* dcol, float* dx, int32_t n, int32_t c, int32_t h, int32_t w, int32_t k, int32_t stride, int32_t pad,
                 void* stream);
int ide3d_maxpool3s2p0(const float* x, float* y, uint8_t* idx, int64_t planes, int32_t h, int32_t w, void* stream);
int ide3d_lpips_tap_backward(const float* y, const float* g, const uint8_t* idx, const float* dtap, float* dz, int64_t planes, int32_t h,
                             int32_t w, int32_t pooled, void* stream);

/*
 * ABI 8 (entry points added).  The cross-entropy of the BiSeNet face parser's logits against integer labels and its image gradient through
 * the frozen parser (apps/train_hybrid_encoder.py:279-283, 324-328, apps/finetune_hybrid_encoder.py:170-174): everything between the
 * convolutions (csrc/parse_loss.hip; the convolutions and all but one of their input gradients are
 * ide3d_modconv2d, the plain ReLU gradients ide3d_modconv_act_backward).  NCHW fp32 in device memory.  No atomics, fixed-order sums,
 * bit-reproducible; no host synchronisation.
 *
 * ide3d_resize_bilinear — `F.interpolate(x, (H, W), mode='bilinear', align_corners=True)` (inversion/BiSeNet.py:112-121): [planes, h, w] ->
 *   [planes, H, W], H, W >= 2; interpolated in float64, rounded once.  ide3d_resize_bilinear_backward — its adjoint in gather form: each
 *   input pixel sums, rows then columns ascending, over the output pixels whose footprint holds it.
 * ide3d_parse_ce — `CrossEntropyLoss()(interpolate(logits, (H, W), bilinear, align_corners=True), labels)`: logits [n, C, h, w], labels
 *   int64 [n, H, W] (a label outside 0..C-1 contributes its log-sum-exp only); the resize is evaluated per image pixel, the
 *   max-subtracted log-sum-exp and the mean are carried in float64: one launch of per-workgroup partial sums (workspace of
 *   ide3d_parse_ce_workspace_bytes()) + one finishing launch.  lse [n, H, W] float64 receives every pixel's log-sum-exp for the backward.
 * ide3d_parse_ce_backward — dlogits [n, C, h, w] = the adjoint of that resize applied to (softmax - onehot) dloss / (n H W), gather form,
 *   softmax recomputed from the saved lse.  dloss: DEVICE pointer to the upstream scalar gradient.
 * ide3d_maxpool3s2 — `MaxPool2d(3, 2, 1)` (inversion/resnet.py:63): [planes, h, w] -> [planes, (h-1)/2+1, (w-1)/2+1], bit-equal to ATen's
 *   (the first maximum in row-major window order wins, NaN wins); idx (may be NULL): one byte per output, the winner as ky * 3 + kx.
 * ide3d_maxpool3s2_backward — gather form: dx[y, x] = the sum of dy over the <= 4 windows whose winner is (y, x), window rows then columns
 *   ascending (bit-equal to ATen's); mask (may be NULL) [planes, h, w]: dx = 0 where mask <= 0 (the ReLU in front of the pool).
 * ide3d_parse_join — out[n, c, y, x] = post(t0 * scale[n, c] + t1 + t2 + bias[n, c] * bias_gain).  Forward: the residual join relu(a + b)
 *   (resnet.py:46), the gates feat * g + broadcast / + map (BiSeNet.py:79-81, 115-120) and feat * g + feat (:206-207).  Backward: the sum
 *   of the gradients that meet at a tensor, the gate's scale, a spatial mean's broadcast gradient and the ReLU mask in one pass.  A term is a
 *   strided view (rows contiguous): a cropped transposed-convolution result, a channel slice; `half` = 1: a [n, c, (h+1)/2, (w+1)/2] map
 *   added at the even rows and columns only (the gradient of a stride-2 1x1 shortcut).  16-byte accesses when every operand allows it.
 * ide3d_plane_sums — out[plane] = gain * sum_p a[plane, p] (* b[plane, p] when b != NULL), summed in float64 in a fixed order, one
 *   workgroup per plane: the global averages (BiSeNet.py:77, 111, 203) and the gates' gradients.
 * ide3d_parse_stem_backward — the input gradient of `conv2d(x [n, 3, H, W], weight [cout <= 64, 3, 7, 7], stride 2, padding 3)`
 *   (resnet.py:61): dz [n, cout, (H-1)/2+1, (W-1)/2+1] -> dx [n, 3, H, W], direct: <= 16 taps x cout channels per pixel.
 */
#define IDE3D_PARSE_JOIN_TERMS 3
typedef struct ide3d_parse_term {
    const float* p;             /* NULL: absent (term 0 must be present) */
    int64_t      batch_stride;  /* in floats */
    int64_t      plane_stride;
    int32_t      row_pitch;
    int32_t      half;
} ide3d_parse_term;
typedef struct ide3d_parse_join_params {
    ide3d_parse_term term[IDE3D_PARSE_JOIN_TERMS];
    const float* scale;         /* [n, c] or NULL: multiplies term 0 */
    const float* bias;          /* [n, c] or NULL */
    const float* y;             /* [n, c, h, w] dense: the mask of post 2 */
    float*       out;           /* [n, c, h, w] dense */
    int32_t      n, c, h, w;
    int32_t      post;          /* 0: none, 1: ReLU, 2: 0 where y <= 0 */
    float        bias_gain;
} ide3d_parse_join_params;

int ide3d_resize_bilinear(const float* x, float* y, int64_t planes, int32_t h, int32_t w, int32_t H, int32_t W, void* stream);
int ide3d_resize_bilinear_backward(const float* dy, float* dx, int64_t planes, int32_t h, int32_t w, int32_t H, int32_t W, void* stream);
int64_t ide3d_parse_ce_workspace_bytes(int32_t n, int32_t C, int32_t h, int32_t w, int32_t H, int32_t W);
int ide3d_parse_ce(const float* logits, const int64_t* labels, int32_t n, int32_t C, int32_t h, int32_t w, int32_t H, int32_t W,
                   double* lse, float* workspace, int64_t workspace_bytes, float* loss, void* stream);
int ide3d_parse_ce_backward(const float* logits, const int64_t* labels, const double* lse, const float* dloss, float* dlogits,
                            int32_t n, int32_t C, int32_t h, int32_t w, int32_t H, int32_t W, void* stream);
int ide3d_maxpool3s2(const float* x, float* y, uint8_t* idx, int64_t planes, int32_t h, int32_t w, void* stream);
int ide3d_maxpool3s2_backward(const float* dy, const uint8_t* idx, const float* mask, float* dx, int64_t planes, int32_t h, int32_t w,
                              void* stream);
int ide3d_parse_join(const ide3d_parse_join_params* p, void* stream);
int ide3d_plane_sums(const float* a, const float* b, float* out, int64_t planes, int64_t hw, float gain, void* stream);
int ide3d_parse_stem_backward(const float* dz, const float* weight, float* dx, int32_t n, int32_t cout, int32_t H, int32_t W, void* stream);

/*
 * ABI 8 (entry points added).  The ArcFace identity loss of the hybrid encoder's training step (inversion/criteria/id_loss.py,
 * apps/train_hybrid_encoder.py:235-237, 305-335): one minus the cosine between IR-SE50 embeddings (inversion/psp/encoders/model_irse.py,
 * helpers.py), and its image gradient through the frozen net: everything that is not a convolution, a per-channel affine pass, a gated
 * join or a spatial mean (those are ide3d_modconv2d, ide3d_parse_join, ide3d_plane_sums); csrc/id_loss.hip, DESIGN.md section 5.17.
 * Dense NCHW fp32 in device memory.  No atomics, fixed-order sums, bit-reproducible; no host synchronisation.
 *
 * ide3d_id_prep — `face_pool(pool(x)[:, :, 35:223, 32:220])` (id_loss.py:19-23) in one launch: x [n, 3, 256 f, 256 f] -> y [n, 3, 112, 112];
 *   output (i, j) is the mean over rows floor(188 i / 112) .. ceil(188 (i + 1) / 112) - 1 (+ 35) and the columns likewise (+ 32) of the
 *   f x f block means, window edges in integer arithmetic, summed in float64.  ide3d_id_prep_backward — the adjoint in gather form: each
 *   input pixel inside the crop sums over the <= 2 x 2 output windows that hold it, rows then columns ascending; an exact 0 outside.
 * ide3d_prelu — `PReLU(c)`: y = x > 0 ? x : slope[c] x, bit-equal to ATen.  ide3d_prelu_backward — dx = x > 0 ? dy : slope[c] dy (ATen's
 *   rule at x = 0; x is the PRE-activation: slopes may be 0 or negative); dy is [n, c, h, w] with contiguous rows and the given strides
 *   in floats (a cropped view), x and dx are dense.  16-byte accesses when h w is a multiple of 4 and every operand dense and aligned.
 * ide3d_se_gate — `SEModule` past its average pool (helpers.py:61-78): s [n, c <= 512] spatial means, w1 [r <= 32, c], w2 [c, r] ->
 *   g [n, c] = sigmoid(w2 relu(w1 s)), one workgroup per image, float64 sums.  ide3d_se_gate_backward — dg [n, c] -> ds [n, c]; the hidden
 *   units are recomputed from s.
 * ide3d_linear — y [n, M] = x [n, K] weight^T + bias (bias may be NULL) for n <= 8, K a multiple of 4, x and weight 16-byte aligned: the
 *   weight matrix is read once for all n; one launch writes the sums of every 2048-wide slice of K to the workspace
 *   (ide3d_linear_workspace_bytes(); -1: not covered), a finishing launch adds them in ascending order in float64.
 * ide3d_linear_backward_input — dx [n, K] = dy [n, M] weight under the same limits: partial sums per 64 rows of the weight
 *   (ide3d_linear_backward_input_workspace_bytes(), 16-byte aligned) + the same finishing launch.
 * ide3d_linear_weight_grad — dw [M, K] = dy [n, M]^T x [n, K], summed over the images in ascending order, under the same limits (x and dw
 *   16-byte aligned): one launch, no workspace (the encoders' trainable projectors; csrc/linear_wgrad.hip).
 * ide3d_residual_join — out[i] = (a[i] + b[i]) * gain over `count` dense floats, or a[i] * gain when b is NULL: the join of the encoders'
 *   residual blocks, (conv2(conv1(x)) + skip(x)) / sqrt(2) (inversion/networks.py:1507-1521), and with b NULL the gradient dy * gain that
 *   both of its branches receive.  One fp32 addition, then one fp32 multiplication: bit-equal to the element-wise definition.  count in
 *   [1, 2^40); out overlaps neither input; 16-byte accesses when every operand is 16-byte aligned (csrc/res_join.hip).
 * ide3d_id_head — `l2_norm` and the loss (helpers.py:14-17, id_loss.py:26-47): e [n, M] = f / |f|, norm [n] = |f|, and, when target (unit
 *   vectors [n, M]) is not NULL, loss[0] = sum_i (1 - e_i . target_i) / n.  |f| = 0 divides by zero as the reference does.
 * ide3d_id_head_backward — df = (g - e (e . g)) / |f| with g = -dloss target / n.  dloss: DEVICE pointer to the upstream scalar gradient.
 */
int ide3d_id_prep(const float* x, float* y, int32_t n, int32_t f, void* stream);
int ide3d_id_prep_backward(const float* dy, float* dx, int32_t n, int32_t f, void* stream);
int ide3d_prelu(const float* x, const float* slope, float* y, int32_t n, int32_t c, int32_t h, int32_t w, void* stream);
int ide3d_prelu_backward(const float* dy, int64_t dy_batch_stride, int64_t dy_plane_stride, int32_t dy_row_pitch, const float* x,
                         const float* slope, float* dx, int32_t n, int32_t c, int32_t h, int32_t w, void* stream);
int ide3d_se_gate(const float* s, const float* w1, const float* w2, float* g, int32_t n, int32_t c, int32_t r, void* stream);
int ide3d_se_gate_backward(const float* s, const float* w1, const float* w2, const float* g, const float* dg, float* ds, int32_t n,
                           int32_t c, int32_t r, void* stream);
int64_t ide3d_linear_workspace_bytes(int32_t n, int32_t K, int32_t M);
int64_t ide3d_linear_backward_input_workspace_bytes(int32_t n, int32_t K, int32_t M);
int ide3d_linear(const float* x, const float* weight, const float* bias, float* y, int32_t n, int32_t K, int32_t M, float* workspace,
                 int64_t workspace_bytes, void* stream);
int ide3d_linear_backward_input(const float* dy, const float* weight, float* dx, int32_t n, int32_t K, int32_t M, float* workspace,
                                int64_t workspace_bytes, void* stream);
int ide3d_linear_weight_grad(const float* dy, const float* x, float* dw, int32_t n, int32_t K, int32_t M, void* stream);
int ide3d_residual_join(const float* a, const float* b, float* out, int64_t count, float gain, void* stream);
int ide3d_id_head(const float* f, const float* target, float* e, float* norm, float* loss, int32_t n, int32_t M, void* stream);
int ide3d_id_head_backward(const float* e, const float* target, const float* norm, const float* dloss, float* df, int32_t n, int32_t M,
                           void* stream);

/*
 * ABI 8 (entry points added).  The VGG19 feature loss of the hybrid encoder's training step (apps/train_hybrid_encoder.py:120-152, used at
 * :305: a weighted L1 distance between the relu1_1 .. relu5_1 activations of torchvision's vgg19().features of two images mapped by
 * (x + 1) / 2) and its image gradient: what it needs beside the entry points above (csrc/vgg_loss.hip).  The 13
 * convolutions and their input gradients are ide3d_modconv2d, the interior ReLU gradients ide3d_modconv_act_backward, (x + 1) / 2 and its
 * adjoint ide3d_lpips_prep / _prep_backward at f = 1, in_scale = in_shift = 0.5, mean = 0, std = 1, the pools ide3d_maxpool2.  All tensors
 * dense NCHW fp32 in device memory.  No atomics, fixed-order sums in float64, bit-reproducible; no host synchronisation.
 *
 * ide3d_feat_l1 — the loss from the taps (train_hybrid_encoder.py:141, 146-150: `weight * L1Loss()(source, target)` summed over the
 *   slices): loss[0] = sum_k weight_k * (sum |a_k - t_k|) / (n c_k h_k w_k), 1 <= k <= IDE3D_LPIPS_MAX_TAPS taps [n, c_k, h_k, w_k].
 *   k launches (per-workgroup partial sums -> workspace of ide3d_feat_l1_workspace_bytes()) + 1 finishing launch.
 * ide3d_feat_l1_tap_backward — at a tap (train_hybrid_encoder.py:147-150: the slice's output feeds the criterion AND the next slice), what
 *   autograd does in three passes (L1 backward, add of the next convolution's input gradient, ReLU backward):
 *   dz = (g + s sign(a - t)) where a > 0, else 0, with s = fp32(double(dloss[0]) * weight / count) and sign(0) = 0 as in ATen's L1
 *   backward.  a, t, g, dz [planes, h, w]; g == NULL: the last tap, the sign term alone.  dloss: DEVICE pointer to the upstream scalar
 *   gradient; count: the elements the tap's mean runs over (n c h w).
 * ide3d_maxpool2_relu_backward — behind a pool that follows a ReLU which is no tap (vgg19 features 3-4, 8-9, 17-18, 26-27; in VGG19 no tap
 *   sits in front of a pool), what autograd does in two passes: dz = dpool routed to the first maximum of its 2x2 window where y > 0, else
 *   0.  y, dz [planes, h, w] (y a ReLU output), dpool [planes, h / 2, w / 2], h, w >= 2; a row or column that the floor dropped gets an
 *   exact 0.  The result does not depend on the tie rule, for the reason given at ide3d_lpips_stage_backward.
 */
typedef struct ide3d_feat_l1_tap {
    const float* a;        /* [n, c, h, w] the tap's activation */
    const float* t;        /* [n, c, h, w] the target's activation at the same tap */
    float        weight;
    int32_t      c, h, w;
} ide3d_feat_l1_tap;

int64_t ide3d_feat_l1_workspace_bytes(const ide3d_feat_l1_tap* taps, int32_t k, int32_t n);
int ide3d_feat_l1(const ide3d_feat_l1_tap* taps, int32_t k, int32_t n, float* workspace, int64_t workspace_bytes, float* loss,
                  void* stream);
int ide3d_feat_l1_tap_backward(const float* a, const float* t, const float* g, float* dz, const float* dloss, float weight,
                               int64_t planes, int32_t h, int32_t w, int64_t count, void* stream);
int ide3d_maxpool2_relu_backward(const float* y, const float* dpool, float* dz, int64_t planes, int32_t h, int32_t w, void* stream);

/*
 * ABI 8 (entry points added).  The CLIP image-text loss of the text-guided editing and domain adaptation paths
 * (inversion/models/StyleCLIP/criteria/clip_loss.py:6-17, used at mapper/training/coach.py:206-209 and
 * optimization/run_optimization.py:49-62): one minus the cosine between the embedding a frozen CLIP ViT image encoder gives the rendered
 * image and text embeddings, and its image gradient through the encoder: everything that is not a dense product (those are shared-weight
 * 1x1 ide3d_modconv2d launches over channel-major token maps [n, C, T], ide3d_residual_join and ide3d_linear); csrc/clip_loss.hip,
 * DESIGN.md section 5.37.  Dense fp32 in device memory.  No atomics, fixed-order sums (float64 where they end in one number),
 * bit-reproducible; no host synchronisation.
 *
 * ide3d_clip_prep — `AvgPool2d(S / 32)(Upsample(scale_factor=7)(x))` (clip_loss.py:10-11, 14), the optional CLIP normalisation
 *   ((v + 1) / 2 - mean[c]) / std[c] (mean and std: DEVICE float[3], both or neither) and the unfolding into p x p patches in one pass:
 *   x [n, 3, 32 k, 32 k] -> col [n, 3 p p, 224 / p, 224 / p] in the channel order of ide3d_unfold2d, (ci p + ky) p + kx.  A pooled pixel
 *   is sum_s sum_t count(s) count(t) x[s, t] / k^2 with the integer counts |[Y k, Y k + k) n [7 s, 7 s + 7)|, summed in float64.
 *   ide3d_clip_prep_backward — the adjoint in gather form: each input pixel sums the pooled pixels whose windows hold it, rows then
 *   columns ascending (std: the same pointer as forward, or NULL).
 * ide3d_vit_embed — `x = ln_pre(cat([class_embedding, patches]) + positional_embedding)` of CLIP's VisionTransformer.forward: patches
 *   [n, C, T - 1] (the patch convolution's output), table [C, T] = positional_embedding^T with class_embedding added to column 0 ->
 *   y [n, C, T]; mean, rstd [n, T] are saved.  ide3d_vit_embed_backward — LayerNorm backward to the patch tokens [n, C, T - 1]; the class
 *   column is dropped.
 * ide3d_layernorm — `LayerNorm(C)` (eps inside the square root) over the channels of each token: x [n, C, pitch] (tokens 0 .. T - 1 of
 *   rows of `pitch` floats are read: T = 1, pitch = the map's T is `ln_post` on the class token in place) -> y [n, C, T], mean, rstd
 *   [n, T]; two passes, float64 sums.  ide3d_layernorm_backward — to the input only (gamma and beta are frozen):
 *   dx = rstd (g - mean_c g - xhat mean_c (g xhat)) + add with g = dy gamma; add (NULL or [n, C, pitch]) is the residual stream's
 *   gradient; dx [n, C, pitch], an exact 0 in the columns past T.
 * ide3d_vit_attention — `nn.MultiheadAttention` between its two projections: qkv [n, 3 heads d, T] (q, k, v stacked along the channels,
 *   head h = channels h d .. h d + d - 1 of each) -> out [n, heads d, T] = softmax_j(scale q_i . k_j) v_j; d a multiple of 4, d, T <= 64;
 *   one workgroup per (image, head), q, k, v and the T x T scores in LDS, max subtraction, the denominator in float64 in ascending order.
 *   ide3d_vit_attention_backward — dout [n, heads d, T] -> dqkv [n, 3 heads d, T]; the probabilities are recomputed from q and k:
 *   dV = P^T dO, dS = P (dP - rowsum(dP P)) with dP = dO V^T, dQ = scale dS K, dK = scale dS^T Q.
 * ide3d_quickgelu — CLIP's `QuickGELU`: y = x sigmoid(1.702 x) over `count` dense floats; 16-byte accesses when every operand is 16-byte
 *   aligned.  ide3d_quickgelu_backward — dx = dy (s + 1.702 x s (1 - s)), s = sigmoid(1.702 x), from the saved PRE-activation x.
 * ide3d_clip_head — `1 - logits_per_image / 100` (clip_loss.py:15-16) from the embeddings: f [n, D], base [n, D] or NULL, text [T, D] ->
 *   e [n, D] = (f - base) / |f - base|, norm [n] = |f - base|, tnorm [T] = |text_r| and out [n, T] = 1 - e . text_r / |text_r| (base: the
 *   frozen generator's embeddings of the directional loss); rowsum [n] (float64, 8-byte aligned) = each image's row sum before its values
 *   are rounded, and mean[0] = their ascending float64 sum over n T, rounded once (a finishing launch): the scalar of a training step.
 *   A zero norm divides by zero, as the definition does.
 * ide3d_clip_head_backward — df = (g - e (e . g)) / norm with g = -sum_r dout[i, r] text_r / |text_r|; dout: DEVICE [n, T].
 */
int ide3d_clip_prep(const float* x, const float* mean, const float* std, float* col, int32_t n, int32_t k, int32_t p, void* stream);
int ide3d_clip_prep_backward(const float* dcol, const float* std, float* dx, int32_t n, int32_t k, int32_t p, void* stream);
int ide3d_vit_embed(const float* patches, const float* table, const float* gamma, const float* beta, float* y, float* mean, float* rstd,
                    int32_t n, int32_t C, int32_t T, float eps, void* stream);
int ide3d_vit_embed_backward(const float* dy, const float* patches, const float* table, const float* gamma, const float* mean,
                             const float* rstd, float* dpatches, int32_t n, int32_t C, int32_t T, void* stream);
int ide3d_layernorm(const float* x, const float* gamma, const float* beta, float* y, float* mean, float* rstd, int32_t n, int32_t C,
                    int32_t T, int32_t pitch, float eps, void* stream);
int ide3d_layernorm_backward(const float* dy, const float* x, const float* gamma, const float* mean, const float* rstd, const float* add,
                             float* dx, int32_t n, int32_t C, int32_t T, int32_t pitch, void* stream);
int ide3d_vit_attention(const float* qkv, float* out, int32_t n, int32_t heads, int32_t d, int32_t T, float scale, void* stream);
int ide3d_vit_attention_backward(const float* qkv, const float* dout, float* dqkv, int32_t n, int32_t heads, int32_t d, int32_t T,
                                 float scale, void* stream);
int ide3d_quickgelu(const float* x, float* y, int64_t count, void* stream);
int ide3d_quickgelu_backward(const float* dy, const float* x, float* dx, int64_t count, void* stream);
int ide3d_clip_head(const float* f, const float* base, const float* text, float* e, float* norm, float* tnorm, float* out, double* rowsum,
                    float* mean, int32_t n, int32_t D, int32_t T, void* stream);
int ide3d_clip_head_backward(const float* e, const float* text, const float* norm, const float* tnorm, const float* dout, float* df,
                             int32_t n, int32_t D, int32_t T, void* stream);

/*
 * ABI 8 (entry points added).  The StyleGAN2 discriminator's adversarial loss (inversion/networks.py:1271-1502,
 * apps/train_hybrid_encoder.py:100-117, 302-313) and its image gradient: what is not a convolution, a FIR pass, a join or a linear layer
 * (those are ide3d_upfirdn2d, ide3d_modconv2d, ide3d_modconv_act_backward, ide3d_residual_join, ide3d_linear and
 * ide3d_linear_backward_input); csrc/adv_loss.hip, DESIGN.md section 5.38.  Dense fp32 in device memory.  No atomics, float64 sums in a
 * fixed order, bit-reproducible; no host synchronisation.  Bad arguments return IDE3D_EINVAL before any launch.
 *
 * ide3d_minibatch_std — `MinibatchStdLayer.forward` and its concatenation in one launch: x [n, c, h, w] -> y [n, c + features, h, w].
 *   Channels 0 .. c - 1 of y are bit copies of x.  With G = group (0: n) and sample g (n / G) + j member g of group j (the grouping of
 *   `x.reshape(G, -1, ...)`), channel c + f of every sample of group j holds the mean over the c / features channels of feature f and the
 *   h w pixels of sqrt(var_G(x) + 1e-8), computed in float64 and rounded once.  n % G != 0 or c % features != 0: IDE3D_EINVAL.
 * ide3d_minibatch_std_backward — dy [n, c + features, h, w] -> dx [n, c, h, w] = dy[:, :c] + D[j, f] / (c / features h w) *
 *   (x - mean_G) / (G std), D[j, f] = the sum of dy[:, c + f] over the group's samples and pixels; std is recomputed from x.  The
 *   derivative of the subtracted mean contributes nothing: the deviations of a group sum to zero.  With G = 1 the second term is an exact 0.
 * ide3d_adv_head — the conditional projection and the logistic loss: o, cmap [n, M] -> logit [n] = o_i . cmap_i / sqrt(M) (cmap NULL:
 *   M must be 1 and logit = o) and loss[0] = mean_i softplus(sign logit_i), softplus(z) = max(z, 0) + log1p(exp(-|z|)) in float64.
 *   sign: -1 (generator, real images) or +1 (fake images of the discriminator's loss).
 * ide3d_adv_head_backward — do [n, M] = dloss sign sigmoid(sign logit_i) / n * cmap[i, m] / sqrt(M).  dloss: DEVICE pointer to the
 *   upstream scalar gradient.
 */
int ide3d_minibatch_std(const float* x, float* y, int32_t n, int32_t c, int32_t h, int32_t w, int32_t group, int32_t features, void* stream);
int ide3d_minibatch_std_backward(const float* x, const float* dy, float* dx, int32_t n, int32_t c, int32_t h, int32_t w, int32_t group,
                                 int32_t features, void* stream);
int ide3d_adv_head(const float* o, const float* cmap, float* logit, float* loss, int32_t n, int32_t M, int32_t sign, void* stream);
int ide3d_adv_head_backward(const float* o, const float* cmap, const float* logit, const float* dloss, float* dout, int32_t n, int32_t M,
                            int32_t sign, void* stream);

/*
 * ABI 8 (entry points added).  The arithmetic between the networks of the remaining metrics: perceptual path length, Inception Score and
 * the mIoU of parser labels; csrc/metrics_eval.hip, DESIGN.md section 5.39.  No float atomics: every floating-point sum is float64 in an
 * order fixed by the launch geometry, so two runs are bit-equal; integer counts use integer adds.  No host synchronisation.  A null,
 * misaligned or undersized buffer or an out-of-range size returns IDE3D_EINVAL before any launch.
 *
 * ide3d_ppl_prep replaces metrics/perceptual_path_length.py:71-83 and the z-score in front of the feature net: x [n, 3, H, W] ->
 *   y [n, 3, h / f, w / f], y = ((mean of the f x f block inside the window [y0 : y0 + h, x0 : x0 + w]) * in_scale + in_shift - mean[c]) /
 *   std[c].  1 <= f <= 64 divides h and w; the window lies inside the image.  With the full window it is bit-equal to ide3d_lpips_prep
 *   (the same summation order).  mean, std: 3 floats each (DEVICE).
 * ide3d_lpips_pair_distances replaces perceptual_path_length.py:89: taps as for ide3d_lpips_head, each `a` [2 n, c, h, w] (t and out
 *   unused); per tap u = a * (float)(1 / (sqrt(sum_c a^2) + 1e-10)), the head's normalisation; dist[i] = scale * sum over taps of
 *   (1 / (h w)) sum_{h,w} sum_c lin[c] (u_i - u_{i+n})^2 for i < n, the sums in float64, dist float32 [n]; scale = 1 / epsilon^2.  k
 *   launches (one float64 partial per workgroup -> workspace of ide3d_lpips_pair_workspace_bytes(), 8-byte aligned) + 1 finishing launch.
 *   Identical images give exactly 0.  1 <= n <= 2^20.
 * ide3d_trimmed_mean replaces perceptual_path_length.py:119-122: x [n] fp32, 1 <= n <= 2^24, ranks 0 <= lo_rank <= hi_rank < n.
 *   lo, hi = the lo_rank-th and hi_rank-th smallest values (radix select on the order-preserving integer image of the float, 8-bit LDS
 *   histograms; no sort); out[4] (float64) = {mean of all x with lo <= x <= hi compared as floats (ties at either end are all kept), lo,
 *   hi, their count}.  Any NaN in x: out = {NaN, NaN, NaN, 0}, as numpy's percentile and mean give.  One workgroup.  The reference's
 *   ranks are lo_rank = (n - 1) / 100 and hi_rank = ceil(99 (n - 1) / 100) in integers.
 * ide3d_inception_score replaces metrics/inception_score.py:31-34: p [n, d] fp32 with a row stride >= d, split s = rows
 *   [s n / S, (s + 1) n / S); kl[s] (float64) = mean over the split's rows of sum_j p (log p - log m_j), m_j the column mean over the split,
 *   everything in float64.  1 <= d <= 8192, 1 <= S <= 4096, S <= n <= 2^22.  A zero probability yields NaN (0 * -inf), as the reference's
 *   numpy lines do.  exp, mean and std over the S values are the caller's.  Workspace: ide3d_inception_score_workspace_bytes(), 16-byte
 *   aligned (log m, then the column sums and the row sums per chunk of at least 32 rows, at most 256 chunks per split).
 * ide3d_label_iou replaces apps/calc_losses_on_images.py:28-30 after the one-hot: a, b [n, hw] label maps (int64 or uint8 by `dtype`);
 *   remap: NULL (n_in = 0), or int32 [n_in] (DEVICE) applied to both maps first (a label outside [0, n_in) counts for no class);
 *   1 <= classes <= 32, 1 <= hw < 2^31.  counts int32 [n, classes, 2] = per class the pixels where both maps carry it and where either does;
 *   iou[i] (float32) = mean over ALL classes of float(inter) / (float(union) + 1e-6f), summed in class order.  A label outside
 *   [0, classes) after the remap counts for no class.
 */
#define IDE3D_LABEL_INT64 0
#define IDE3D_LABEL_UINT8 1
int ide3d_ppl_prep(const float* x, float* y, const float* mean, const float* std_, int32_t n, int32_t H, int32_t W, int32_t y0,
                   int32_t x0, int32_t h, int32_t w, int32_t f, float in_scale, float in_shift, void* stream);
int64_t ide3d_lpips_pair_workspace_bytes(const ide3d_lpips_tap* taps, int32_t k, int32_t n);
int ide3d_lpips_pair_distances(const ide3d_lpips_tap* taps, int32_t k, int32_t n, float scale, void* workspace, int64_t workspace_bytes,
                               float* dist, void* stream);
int ide3d_trimmed_mean(const float* x, int64_t n, int64_t lo_rank, int64_t hi_rank, double* out, void* stream);
int64_t ide3d_inception_score_workspace_bytes(int64_t n, int32_t d, int32_t splits);
int ide3d_inception_score(const float* p, int64_t n, int32_t d, int64_t row_stride, int32_t splits, void* workspace, int64_t workspace_bytes,
                          double* kl, void* stream);
int ide3d_label_iou(const void* a, const void* b, int32_t dtype, int32_t n, int64_t hw, const int32_t* remap, int32_t n_in, int32_t classes,
                    int32_t* counts, float* iou, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* IDE3D_HIP_H_ */
