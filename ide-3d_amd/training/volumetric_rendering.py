"""Volume-rendering helpers of the IDE-3D generator (`training.volumetric_rendering` surface of the
reference, training/volumetric_rendering.py).

Every public name of the reference module is kept with the same arguments: `fancy_integration` (:34),
`get_initial_rays_trig` (:77), `perturb_points` (:99), `transform_sampled_points` (:108),
`truncated_normal_` (:138), `sample_camera_positions` (:147), `create_cam2world_matrix` (:195),
`sample_pdf` (:224), `LookAtPoseSampler` (:268) and the small vector helpers.  On ROCm devices
`fancy_integration` runs the wave-per-ray HIP compositing kernel (`csrc/composite.hip`) and
`render_triplane_fused` (new) runs steps ray-setup -> transform -> gathers -> MLPs -> compositing in
one launch (`csrc/raymarch.hip`); `render_triplane_hierarchical` (new) is that renderer with the importance pass, in four
launches.  Two optional keyword arguments were added so that callers (and
parity tests) can supply the random draws instead of having them generated on the device:
`perturb_points(..., jitter=)` / `transform_sampled_points(..., jitter=)` and
`fancy_integration(..., noise=)`.
"""

import math
import os
import random

import numpy as np
import torch
import torch.nn.functional as F

from torch_utils import custom_ops, hip_plugin

_plugin = None


def _init():
    global _plugin
    if _plugin is None:
        _plugin = custom_ops.get_plugin(module_name='volume_render_plugin', sources=['composite.hip', 'raymarch.hip', 'sample_pdf.hip'])
    return True


# ---- small vector helpers ------------------------------------------------------------------------

_consts = {}


def device_const(values, dtype, device):
    """A small read-only constant on `device`, uploaded ONCE per (values, dtype, device).  `torch.tensor(list, device='cuda')` is a
    pageable host-to-device copy: the host blocks until the stream has drained, i.e. until the previous image has finished, and everything
    the driver enqueues after it (the rest of the pose math, the synthesis pass) starts on an idle GPU.  The reference's
    create_cam2world_matrix does exactly that once per pose (volumetric_rendering.py:199); here the pose helpers never synchronise.
    Callers must not write to the returned tensor."""
    device = torch.device(device)
    if device.type == 'cuda' and device.index is None:          # 'cuda' = whichever device is current NOW, not at the first call
        device = torch.device('cuda', torch.cuda.current_device())
    key = (tuple(float(v) for v in values), dtype, device.type, device.index)
    t = _consts.get(key)
    if t is None:
        t = _consts[key] = torch.tensor(list(values), dtype=dtype, device=device)
    return t


def transform_vectors(matrix: torch.Tensor, vectors4: torch.Tensor) -> torch.Tensor:
    """[M, M] applied to row vectors [N, M] -> [N, M]."""
    return vectors4 @ matrix.T


def normalize_vecs(vectors: torch.Tensor) -> torch.Tensor:
    return vectors / torch.norm(vectors, dim=-1, keepdim=True)


def torch_dot(x: torch.Tensor, y: torch.Tensor):
    return (x * y).sum(-1)


# ---- compositing ------------------------------------------------------------------------------------

def _fancy_integration_torch(rgb_sigma, rays_d_cam, z_vals, noise, last_back, white_back, max_depth, clamp_mode, fill_mode):
    rgbs, sigmas = rgb_sigma[..., :-1], rgb_sigma[..., -1:]
    deltas = (z_vals[:, :, 1:] - z_vals[:, :, :-1]) * torch.norm(rays_d_cam, p=2, dim=-1, keepdim=True).unsqueeze(2)
    deltas = torch.cat([deltas, torch.full_like(deltas[:, :, :1], 1e10)], -2)
    dens_in = sigmas if noise is None else sigmas + noise
    if clamp_mode == 'softplus':
        alphas = 1 - torch.exp(-deltas * F.softplus(dens_in))
    elif clamp_mode == 'relu':
        alphas = 1 - torch.exp(-deltas * F.relu(dens_in))
    else:
        raise ValueError('Need to choose clamp mode')
    trans = torch.cumprod(torch.cat([torch.ones_like(alphas[:, :, :1]), 1 - alphas + 1e-10], -2), -2)[:, :, :-1]
    weights = alphas * trans
    weights_sum = weights.sum(2)
    if last_back:
        weights = weights.clone()
        weights[:, :, -1] += (1 - weights_sum)
    rgb_final = torch.sum(weights * rgbs, -2)
    depth_final = torch.sum(weights * z_vals, -2)
    if white_back:
        rgb_final = rgb_final + 1 - weights_sum
    if max_depth:
        depth_final = depth_final + (1 - weights_sum) * max_depth
    if fill_mode == 'debug':
        rgb_final[weights_sum.squeeze(-1) < 0.9] = torch.tensor([1., 0, 0], device=rgb_final.device, dtype=rgb_final.dtype)
    elif fill_mode == 'weight':
        rgb_final = weights_sum.expand_as(rgb_final)
    return rgb_final, depth_final, weights


def fancy_integration(rgb_sigma, rays_d_cam, z_vals, device, noise_std=0.5, last_back=False, white_back=False,
                      max_depth=None, clamp_mode=None, fill_mode=None, noise=None):
    """NeRF quadrature along rays.  rgb_sigma [N, R, S, C+1] (sigma last), rays_d_cam [N, R, 3],
    z_vals [N, R, S, 1] -> (rgb [N, R, C], depth [N, R, 1], weights [N, R, S, 1])  (reference :34-74).

    `noise` (optional, [N, R, S, 1]): standard-normal draws to use instead of `torch.randn` on `device`;
    it is multiplied by `noise_std`.  With `noise_std == 0` no draw is made.
    """
    if clamp_mode not in ('softplus', 'relu'):
        raise ValueError('Need to choose clamp mode')
    if noise is None and noise_std != 0:
        noise = torch.randn(rgb_sigma[..., -1:].shape, device=device)
    scaled_noise = None if (noise is None or noise_std == 0) else noise * noise_std

    on_gpu = rgb_sigma.device.type == 'cuda' and rgb_sigma.dtype == torch.float32
    needs_grad = torch.is_grad_enabled() and (rgb_sigma.requires_grad or z_vals.requires_grad)
    # one sample: the definition below drops it (the only delta is an empty tensor's, so weights come out [N, R, 0, 1]); the kernel would
    # integrate it with delta 1e10.  Both devices follow the definition
    if on_gpu and not needs_grad and rgb_sigma.shape[2] >= 2 and _init():
        n, r, s, c1 = rgb_sigma.shape
        dir_norm = torch.norm(rays_d_cam, p=2, dim=-1).reshape(n * r)
        rgb, depth, weights = _plugin.composite(
            rgb_sigma.reshape(n * r, s, c1), z_vals.reshape(n * r, s), dir_norm,
            None if scaled_noise is None else scaled_noise.reshape(n * r, s),
            0 if clamp_mode == 'softplus' else 1, last_back, white_back, max_depth,
            {None: 0, 'debug': 1, 'weight': 2}[fill_mode])
        return rgb.reshape(n, r, c1 - 1), depth.reshape(n, r, 1), weights.reshape(n, r, s, 1)
    # differentiable / CPU definition
    return _fancy_integration_torch(rgb_sigma, rays_d_cam, z_vals, scaled_noise, last_back, white_back, max_depth,
                                    clamp_mode, fill_mode)


# ---- rays -----------------------------------------------------------------------------------------------

def _camera_rays(device, fov, resolution):
    """Unit ray directions [W*H, 3] of a pinhole camera, row-major with x fastest, y flipped (reference :80-88)."""
    W, H = resolution
    gx, gy = torch.meshgrid(torch.linspace(-1, 1, W, device=device), torch.linspace(1, -1, H, device=device), indexing='ij')
    x = gx.T.flatten()
    y = gy.T.flatten()
    z = -torch.ones_like(x, device=device) / np.tan((2 * math.pi * fov / 360) / 2)
    return normalize_vecs(torch.stack([x, y, z], -1))


def get_initial_rays_trig(n, num_steps, device, fov, resolution, ray_start, ray_end):
    """Camera-space sample points [n, W*H, S, 3], depths [n, W*H, S, 1], ray directions [n, W*H, 3] (reference :77-97)."""
    W, H = resolution
    rays_d_cam = _camera_rays(device, fov, resolution)
    z_vals = torch.linspace(ray_start, ray_end, num_steps, device=device).reshape(1, num_steps, 1).repeat(W * H, 1, 1)
    points = rays_d_cam.unsqueeze(1).repeat(1, num_steps, 1) * z_vals
    points = points.unsqueeze(0).repeat(n, 1, 1, 1)
    z_vals = z_vals.unsqueeze(0).repeat(n, 1, 1, 1)
    rays_d_cam = rays_d_cam.unsqueeze(0).repeat(n, 1, 1).to(device)
    return points, z_vals, rays_d_cam


def perturb_points(points, z_vals, ray_directions, device, jitter=None):
    """Stratified jitter: one uniform offset of +-half a step per sample (reference :99-105).
    `jitter` (optional, same shape as z_vals) supplies the U[0,1) draws."""
    step = z_vals[:, :, 1:2, :] - z_vals[:, :, 0:1, :]
    if jitter is None:
        jitter = torch.rand(z_vals.shape, device=device)
    offset = (jitter - 0.5) * step
    z_vals = z_vals + offset
    points = points + offset * ray_directions.unsqueeze(2)
    return points, z_vals


def transform_sampled_points(points, z_vals, ray_directions, device, h_stddev=1, v_stddev=1, h_mean=math.pi * 0.5,
                             v_mean=math.pi * 0.5, radius=1, camera=None, mode='normal', jitter=None):
    """Jitter the samples, pick a camera and map points / directions / origins to world space (reference :108-136)."""
    n, num_rays, num_steps, _ = points.shape
    points, z_vals = perturb_points(points, z_vals, ray_directions, device, jitter=jitter)

    camera_origin, pitch, yaw = sample_camera_positions(n=n, r=radius, horizontal_stddev=h_stddev, vertical_stddev=v_stddev,
                                                        horizontal_mean=h_mean, vertical_mean=v_mean, device=device, mode=mode)
    cam2world = create_cam2world_matrix(normalize_vecs(-camera_origin), camera_origin, device=device)
    if camera is not None:
        cam2world = camera

    homo = torch.ones((n, num_rays, num_steps, 4), device=device)
    homo[..., :3] = points
    world_pts = torch.bmm(cam2world, homo.reshape(n, -1, 4).permute(0, 2, 1)).permute(0, 2, 1).reshape(n, num_rays, num_steps, 4)
    world_dirs = torch.bmm(cam2world[..., :3, :3], ray_directions.reshape(n, -1, 3).permute(0, 2, 1)).permute(0, 2, 1).reshape(n, num_rays, 3)
    origins = torch.zeros((n, 4, num_rays), device=device)
    origins[:, 3, :] = 1
    world_origins = torch.bmm(cam2world, origins).permute(0, 2, 1).reshape(n, num_rays, 4)[..., :3]
    return world_pts[..., :3], z_vals, world_dirs, world_origins, pitch, yaw


def truncated_normal_(tensor, mean=0, std=1):
    """Fill `tensor` in place with N(mean, std) truncated to two sigma (reference :138-145)."""
    draws = tensor.new_empty(tuple(tensor.shape) + (4,)).normal_()
    ok = (draws < 2) & (draws > -2)
    pick = ok.max(-1, keepdim=True)[1]
    tensor.data.copy_(draws.gather(-1, pick).squeeze(-1))
    tensor.data.mul_(std).add_(mean)
    return tensor


def _camera_plugin(*tensors):
    """csrc/camera.hip for poses that are float32 device tensors outside autograd (`IDE3D_NO_CAMERA_KERNELS=1`: the tensor operations), else None."""
    from torch_utils import hip_plugin
    if not hip_plugin.CameraPlugin.applies(*tensors) or os.environ.get('IDE3D_NO_CAMERA_KERNELS'):
        return None
    return hip_plugin.CameraPlugin


def sample_camera_positions(device, n=1, r=1, horizontal_stddev=0.3, vertical_stddev=0.155, horizontal_mean=math.pi * 0.5,
                            vertical_mean=math.pi * 0.5, mode='normal'):
    """Camera positions on a sphere of radius r.  theta = yaw, phi = pitch in (0, pi) (reference :147-193)."""
    def uni(scale):
        return (torch.rand((n, 1), device=device) - 0.5) * 2 * scale

    if mode == 'uniform':
        theta = uni(horizontal_stddev) + horizontal_mean
        phi = uni(vertical_stddev) + vertical_mean
    elif mode in ('normal', 'gaussian'):
        theta = torch.randn((n, 1), device=device) * horizontal_stddev + horizontal_mean
        phi = torch.randn((n, 1), device=device) * vertical_stddev + vertical_mean
    elif mode == 'hybrid':
        if random.random() < 0.5:
            theta = uni(horizontal_stddev * 2) + horizontal_mean
            phi = uni(vertical_stddev * 2) + vertical_mean
        else:
            theta = torch.randn((n, 1), device=device) * horizontal_stddev + horizontal_mean
            phi = torch.randn((n, 1), device=device) * vertical_stddev + vertical_mean
    elif mode == 'truncated_gaussian':
        theta = truncated_normal_(torch.zeros((n, 1), device=device)) * horizontal_stddev + horizontal_mean
        phi = truncated_normal_(torch.zeros((n, 1), device=device)) * vertical_stddev + vertical_mean
    elif mode == 'spherical_uniform':
        theta = uni(horizontal_stddev) + horizontal_mean
        v = uni(vertical_stddev / math.pi) + vertical_mean / math.pi
        v = torch.clamp(v, 1e-5, 1 - 1e-5)
        phi = torch.arccos(1 - 2 * v)
    else:   # deterministic: the means
        theta = torch.full((n, 1), horizontal_mean, device=device, dtype=torch.float)
        phi = torch.full((n, 1), vertical_mean, device=device, dtype=torch.float)

    cam = _camera_plugin(theta, phi)
    if cam is not None:          # clamp + spherical -> cartesian in one launch (csrc/camera.hip) instead of 14
        pos, phi = cam.sphere_points(theta, phi, r)
        return pos, phi, theta
    phi = torch.clamp(phi, 1e-5, math.pi - 1e-5)
    pos = torch.zeros((n, 3), device=device)
    pos[:, 0:1] = r * torch.sin(phi) * torch.cos(theta)
    pos[:, 2:3] = r * torch.sin(phi) * torch.sin(theta)
    pos[:, 1:2] = r * torch.cos(phi)
    return pos, phi, theta


def create_cam2world_matrix(forward_vector, origin, device=None):
    """Look-along-`forward_vector` camera at `origin`, y-up: cam2world = T(origin) @ R([-left, up, -forward]) (reference :195-213)."""
    cam = _camera_plugin(forward_vector, origin)
    if cam is not None and forward_vector.ndim == 2 and forward_vector.shape == origin.shape and forward_vector.shape[1] == 3:
        return cam.cam2world(forward_vector, origin)          # one launch instead of ~25
    forward_vector = normalize_vecs(forward_vector)
    world_up = device_const((0, 1, 0), torch.float, forward_vector.device if device is None else device).expand_as(forward_vector)
    left = normalize_vecs(torch.cross(world_up, forward_vector, dim=-1))
    up = normalize_vecs(torch.cross(forward_vector, left, dim=-1))
    n = forward_vector.shape[0]
    rot = torch.eye(4, device=device).unsqueeze(0).repeat(n, 1, 1)
    rot[:, :3, :3] = torch.stack((-left, up, -forward_vector), axis=-1)
    trans = torch.eye(4, device=device).unsqueeze(0).repeat(n, 1, 1)
    trans[:, :3, 3] = origin
    return trans @ rot


def create_world2cam_matrix(forward_vector, origin, device=None):
    return torch.inverse(create_cam2world_matrix(forward_vector, origin, device=device))


def sample_pdf(bins, weights, N_importance, det=False, eps=1e-5, u=None):
    """Inverse-CDF sampling of `N_importance` depths per ray (reference :224-265).
    bins [rays, K+1], weights [rays, K] -> samples [rays, N_importance].  `u` (not in the reference) supplies the
    draws, [N_importance] or [rays, N_importance], instead of the linspace (`det`) / `torch.rand` the call makes.
    float32 device tensors run `ide3d_sample_pdf` (one wave per ray); everything else the definition below."""
    n_rays, k = weights.shape
    if u is None:
        u = torch.linspace(0, 1, N_importance, device=bins.device) if det else torch.rand(n_rays, N_importance, device=bins.device)
    if weights.device.type == 'cuda' and weights.dtype == torch.float32 and _init() \
            and not (torch.is_grad_enabled() and (weights.requires_grad or bins.requires_grad)):
        return _plugin.sample_pdf(bins.float(), weights, u.float(), eps)
    u = u.expand(n_rays, N_importance).contiguous()
    pdf = (weights + eps)
    pdf = pdf / pdf.sum(-1, keepdim=True)
    cdf = torch.cat([torch.zeros_like(pdf[:, :1]), torch.cumsum(pdf, -1)], -1)
    idx = torch.searchsorted(cdf, u)
    lo = torch.clamp_min(idx - 1, 0)
    hi = torch.clamp_max(idx, k)
    pair = torch.stack([lo, hi], -1).view(n_rays, 2 * N_importance)
    cdf_g = torch.gather(cdf, 1, pair).view(n_rays, N_importance, 2)
    bins_g = torch.gather(bins, 1, pair).view(n_rays, N_importance, 2)
    denom = cdf_g[..., 1] - cdf_g[..., 0]
    denom[denom < eps] = 1
    return bins_g[..., 0] + (u - cdf_g[..., 0]) / denom * (bins_g[..., 1] - bins_g[..., 0])


class LookAtPoseSampler:
    """cam2world of a camera on a sphere looking at `lookat_position` (reference :268-295).
    Pitch uses phi = arccos(1 - 2 v / pi) (unlike `sample_camera_positions`)."""

    @staticmethod
    def sample(horizontal_mean, vertical_mean, lookat_position, horizontal_stddev=0, vertical_stddev=0, radius=1,
               batch_size=1, device='cpu'):
        h = torch.randn((batch_size, 1), device=device) * horizontal_stddev + horizontal_mean
        v = torch.randn((batch_size, 1), device=device) * vertical_stddev + vertical_mean
        cam = _camera_plugin(h, v, lookat_position) if torch.is_tensor(lookat_position) and lookat_position.numel() in (3, 3 * batch_size) else None
        if cam is not None:      # the draws above keep torch's generator; everything after them is two launches (csrc/camera.hip)
            origins, _ = cam.sphere_points(h, v, radius, pitch_is_v=True)
            return cam.cam2world(None, origins, lookat=lookat_position)
        v = torch.clamp(v, 1e-5, math.pi - 1e-5)
        theta = h
        phi = torch.arccos(1 - 2 * (v / math.pi))
        origins = torch.zeros((batch_size, 3), device=device)
        origins[:, 0:1] = radius * torch.sin(phi) * torch.cos(theta)
        origins[:, 2:3] = radius * torch.sin(phi) * torch.sin(theta)
        origins[:, 1:2] = radius * torch.cos(phi)
        return create_cam2world_matrix(normalize_vecs(lookat_position - origins), origins, device=device)


# ---- fused renderer (new entry point) -------------------------------------------------------------------

_ray_setup_cache = {}


def _fused_ray_setup(device, fov, resolution, num_steps, ray_start, ray_end):
    """Camera-space ray directions [W*H, 3] and the depth ramp [S] of the fused kernel: they depend on the camera model
    only, so they are built once per configuration instead of by ~15 tiny launches per frame (read-only afterwards)."""
    key = (str(device), fov, resolution, num_steps, ray_start, ray_end)
    ent = _ray_setup_cache.get(key)
    if ent is None:
        # entries are tiny ([R, 3] + [S]) and a captured hipGraph may hold their pointers: never freed
        ent = (_camera_rays(device, fov, resolution).contiguous(), torch.linspace(ray_start, ray_end, num_steps, device=device))
        _ray_setup_cache[key] = ent
    return ent


class _NoFusedKernel(Exception):
    """The library has no fused kernel for the configuration (IDE3D_ENOKERNEL)."""


_MLP_KEYS = hip_plugin.VolumeRenderPlugin.MLP_KEYS


class _RenderRaysFused(torch.autograd.Function):
    """`ide3d_render_rays` with a gradient for the two tri-planes (`ide3d_render_rays_backward`) and for the eight decoder tensors
    (`ide3d_render_rays_backward_params`, csrc/raymarch_bwd.hip).  The forward is the inference launch unchanged; what is saved is its
    inputs (planes, decoder weights, camera, jitter, noise), nothing per sample: the backward kernel rebuilds the samples.  The backward
    is one call: the camera entry point (`ide3d_render_rays_backward_camera`) when `cam2world` needs a gradient, else the parameter entry
    point when a decoder tensor needs one (both without the tap scatter when no plane does), the tri-plane-only one otherwise.  No gradient
    for the jitter or the noise."""

    @staticmethod
    def forward(ctx, tex_planes, geo_planes, rays_d_cam, z_lin, cam2world, jitter, sigma_noise, clamp_code, white_back, max_depth, *mlp_tensors):
        mlp = dict(zip(_MLP_KEYS, mlp_tensors))
        args = (rays_d_cam, z_lin, cam2world, jitter, sigma_noise, tex_planes, geo_planes, mlp, clamp_code, False, white_back, max_depth)
        res = _plugin.render_rays(*args)
        if res is None:
            raise _NoFusedKernel()
        ctx.save_for_backward(tex_planes, geo_planes, *mlp_tensors)
        ctx.args = args[:5] + args[8:]
        ctx.cam_shape = cam2world.shape
        return res

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_feat, grad_depth, grad_wsum):
        tex_planes, geo_planes, *mlp_tensors = ctx.saved_tensors
        mlp = dict(zip(_MLP_KEYS, mlp_tensors))
        a = ctx.args
        need = ctx.needs_input_grad
        planes, ups = need[0] or need[1], (grad_feat, grad_depth, grad_wsum)
        if need[4]:
            res = _plugin.render_rays_backward_camera(*a[:5], tex_planes, geo_planes, mlp, *a[5:], *ups, plane_grads=planes, param_grads=any(need[10:]))
        elif any(need[10:]):
            res = _plugin.render_rays_backward_params(*a[:5], tex_planes, geo_planes, mlp, *a[5:], *ups, plane_grads=planes)
        else:
            res = _plugin.render_rays_backward(*a[:5], tex_planes, geo_planes, mlp, *a[5:], *ups)
        if res is None:
            raise RuntimeError('render_rays_backward: no backward kernel for this configuration: '
                               + hip_plugin.load().ide3d_last_error().decode('utf-8', 'replace'))
        dtex, dgeo, dmlp, dcam = res + (None,) * (4 - len(res))        # the entry points without a decoder / camera gradient return fewer
        return (dtex if need[0] else None, dgeo if need[1] else None, None, None, dcam if dcam is None else dcam.reshape(ctx.cam_shape)) \
            + (None,) * 5 + tuple(dmlp[k] if need[10 + i] else None for i, k in enumerate(_MLP_KEYS))


class _RenderRaysMerged(torch.autograd.Function):
    """`ide3d_render_rays_merged`, the last of the hierarchical pass's four launches, with a gradient for the two tri-planes and the eight
    decoder tensors (`ide3d_render_rays_merged_backward`, csrc/raymarch_bwd.hip).  The three launches before it ran without autograd:
    z_all, src and z_fine arrive as constants, as the step-wise definition takes them (fine depths and points under no_grad).  Saved are
    the planes, the decoder tensors and those three arrays ([rays, 2S] / [rays, S]), nothing per sample.  The backward is one call,
    without the tap scatter when no plane needs a gradient.  No gradient for the camera, the jitter or the fine depths."""

    @staticmethod
    def forward(ctx, tex_planes, geo_planes, rays_d_cam, z_lin, cam2world, jitter, z_all, src, z_fine, clamp_code, white_back, max_depth,
                *mlp_tensors):
        mlp = dict(zip(_MLP_KEYS, mlp_tensors))
        res = _plugin.render_rays_merged(rays_d_cam, z_lin, cam2world, jitter, tex_planes, geo_planes, mlp, clamp_code, white_back, max_depth,
                                         z_all, src, z_fine)
        if res is None:
            raise _NoFusedKernel()
        ctx.save_for_backward(tex_planes, geo_planes, z_all, src, z_fine, *mlp_tensors)
        ctx.args = (rays_d_cam, z_lin, cam2world, jitter, clamp_code, white_back, max_depth)
        return res

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_feat, grad_depth, grad_wsum):
        tex_planes, geo_planes, z_all, src, z_fine, *mlp_tensors = ctx.saved_tensors
        mlp = dict(zip(_MLP_KEYS, mlp_tensors))
        a = ctx.args
        need = ctx.needs_input_grad
        res = _plugin.render_rays_merged_backward(*a[:4], tex_planes, geo_planes, mlp, *a[4:], z_all, src, z_fine, grad_feat, grad_depth,
                                                  grad_wsum, plane_grads=need[0] or need[1], param_grads=any(need[12:]))
        if res is None:
            raise RuntimeError('render_rays_merged_backward: no backward kernel for this configuration: '
                               + hip_plugin.load().ide3d_last_error().decode('utf-8', 'replace'))
        dtex, dgeo, dmlp = res
        return (dtex if need[0] else None, dgeo if need[1] else None) + (None,) * 10 \
            + tuple(dmlp[k] if need[12 + i] else None for i, k in enumerate(_MLP_KEYS))


def render_triplane_fused(tex_planes, geo_planes, mlp, cam2world, fov, resolution, num_steps, ray_start, ray_end,
                          jitter=None, sigma_noise=None, clamp_mode='softplus', white_back=False, max_depth=None):
    """One HIP launch for: get_initial_rays_trig -> perturb_points -> cam2world transform -> two
    `sample_from_triplane` gathers -> decoder MLPs -> fancy_integration.

    tex_planes / geo_planes: [N, 3*C, H, W] float32 (channels_last is the zero-copy layout).
    mlp: dict of contiguous float32 tensors geo_w0/b0/w1/b1, tex_w0/b0/w1/b1 ([out, in] weights with their
         runtime gains folded in).
    cam2world: [N, 4, 4].  jitter: U[0,1) draws [N, R, S] (None = no stratified jitter).
    sigma_noise: [N, R, S] density noise already scaled by noise_std, or None.
    Returns (features [N, feat+seg, H_r, W_r], depth [N, 1, H_r, W_r], weight_sum [N, 1, H_r, W_r]), or None when the
    library has no fused kernel for the configuration (IDE3D_ENOKERNEL: plane_channels / decoder widths other than
    the compiled (32, 64) and (16, 32)) — the caller then runs the step-wise HIP ops.  Launch failures raise RuntimeError.

    Gradients: when grad mode is on and a tri-plane or a tensor of `mlp` requires grad, the outputs are differentiable with respect to
    tex_planes, geo_planes and the eight tensors of `mlp` (one backward call: `ide3d_render_rays_backward`, or
    `ide3d_render_rays_backward_params` when a tensor of `mlp` needs a gradient; first order only), and with respect to `cam2world` when
    it requires grad (`ide3d_render_rays_backward_camera`, all 12 entries of the top three rows; the last row gets zero).  No gradient is
    returned for `jitter` or `sigma_noise`, whether or not they require grad: a caller that needs those must run the step-wise
    definition (TriplaneRenderer.forward does; it only sends a trainable decoder here under `triplane.fused_render_param_grad` and a
    trainable camera under `triplane.fused_render_camera_grad`).
    The forward values are those of the no-grad call, bit for bit.
    """
    assert clamp_mode in ('softplus', 'relu')
    _init()
    device = tex_planes.device
    W, H = resolution
    rays_d_cam, z_lin = _fused_ray_setup(device, float(fov), tuple(resolution), int(num_steps), float(ray_start), float(ray_end))
    if tex_planes.stride(1) != 1:
        tex_planes = tex_planes.contiguous(memory_format=torch.channels_last)
    if geo_planes.stride(1) != 1:
        geo_planes = geo_planes.contiguous(memory_format=torch.channels_last)
    clamp_code = 0 if clamp_mode == 'softplus' else 1
    if torch.is_grad_enabled() and (tex_planes.requires_grad or geo_planes.requires_grad or cam2world.requires_grad
                                    or any(mlp[k].requires_grad for k in _MLP_KEYS)):
        try:
            res = _RenderRaysFused.apply(tex_planes, geo_planes, rays_d_cam, z_lin, cam2world, jitter, sigma_noise, clamp_code,
                                         white_back, max_depth, *(mlp[k] for k in _MLP_KEYS))
        except _NoFusedKernel:
            return None
    else:
        res = _plugin.render_rays(rays_d_cam, z_lin, cam2world, jitter, sigma_noise, tex_planes, geo_planes, mlp, clamp_code, False,
                                  white_back, max_depth)
    if res is None:
        return None
    feat, depth, wsum = res
    n = tex_planes.shape[0]
    return feat.reshape(n, -1, H, W), depth.reshape(n, 1, H, W), wsum.reshape(n, 1, H, W)


def render_triplane_hierarchical(tex_planes, geo_planes, mlp, cam2world, fov, resolution, num_steps, ray_start, ray_end,
                                 jitter=None, sigma_noise=None, importance_u=None, clamp_mode='softplus', white_back=False,
                                 max_depth=None):
    """`render_triplane_fused` with the importance pass, in four HIP launches and nothing per sample in memory but depths and
    weights:

      `ide3d_render_ray_weights`  the first pass's weights (geometry branch only; `sigma_noise` applies here) -> depths, pdf
      `ide3d_sample_pdf`          `num_steps` more depths per ray from that pdf
      `ide3d_merge_depths`        both depth sets in ascending order (stable: the order of torch.sort(torch.cat([fine, coarse])))
      `ide3d_render_rays_merged`  the fused march over the 2 * num_steps samples, no density noise

    Arguments as `render_triplane_fused`; importance_u: the draws of `sample_pdf`, [num_steps] (one row for every ray) or
    [N * R, num_steps]; None -> torch.rand.  Returns the same triple, or None when the library has no kernel for the
    configuration (what `render_triplane_fused` declines, and num_steps < 3 or > 1024).

    Gradients: when grad mode is on and a tri-plane or a tensor of `mlp` requires grad, the outputs are
    differentiable with respect to tex_planes, geo_planes and the eight tensors of `mlp` through the merged march (one backward call,
    `ide3d_render_rays_merged_backward`; first order only).  As in the step-wise definition the fine depths are constants: nothing
    flows into the first pass, the pdf draw or the merge, and no gradient is returned for `cam2world`, `jitter`, `sigma_noise` or
    `importance_u`, whether or not they require grad.  The forward values are those of the no-grad call, bit for bit.
    """
    assert clamp_mode in ('softplus', 'relu')
    _init()
    device = tex_planes.device
    W, H = resolution
    rays_d_cam, z_lin = _fused_ray_setup(device, float(fov), tuple(resolution), int(num_steps), float(ray_start), float(ray_end))
    if tex_planes.stride(1) != 1:
        tex_planes = tex_planes.contiguous(memory_format=torch.channels_last)
    if geo_planes.stride(1) != 1:
        geo_planes = geo_planes.contiguous(memory_format=torch.channels_last)
    clamp_code = 0 if clamp_mode == 'softplus' else 1
    n = tex_planes.shape[0]
    first = _plugin.render_ray_weights(rays_d_cam, z_lin, cam2world, jitter, sigma_noise, tex_planes, geo_planes, mlp, clamp_code,
                                       want=('z_vals', 'pdf_bins', 'pdf_weights'))
    if first is None:
        return None
    _w, z_vals, bins, pdf_w = first
    u = torch.rand(n * W * H, num_steps, device=device) if importance_u is None else importance_u
    z_fine = _plugin.sample_pdf(bins, pdf_w, u.float())
    z_all, src = _plugin.merge_depths(z_fine, z_vals)
    if torch.is_grad_enabled() and (tex_planes.requires_grad or geo_planes.requires_grad or any(mlp[k].requires_grad for k in _MLP_KEYS)):
        try:
            res = _RenderRaysMerged.apply(tex_planes, geo_planes, rays_d_cam, z_lin, cam2world, jitter, z_all, src, z_fine, clamp_code,
                                          white_back, max_depth, *(mlp[k] for k in _MLP_KEYS))
        except _NoFusedKernel:
            return None
    else:
        res = _plugin.render_rays_merged(rays_d_cam, z_lin, cam2world, jitter, tex_planes, geo_planes, mlp, clamp_code, white_back,
                                         max_depth, z_all, src, z_fine)
    if res is None:
        return None
    feat, depth, wsum = res
    return feat.reshape(n, -1, H, W), depth.reshape(n, 1, H, W), wsum.reshape(n, 1, H, W)
