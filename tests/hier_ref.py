"""Definitions of the three launches of the hierarchical pass (`ide3d_render_ray_weights`, `ide3d_merge_depths`,
`ide3d_render_rays_merged`), composed from the oracle's own functions (oracle/ops.py: float64
gather taps and compositing; oracle/generator.py: the decoder), plus the merge as a stable sort.  TEST INFRASTRUCTURE ONLY.

`sd` is a generator state dict (keys `synthesis.renderer.decoder.*`); tex / geo [n, 3C, H, W]; cam2world [n, 4, 4];
`size` the side of the square ray grid; everything on the CPU.
"""

import torch

from oracle import generator as ogen
from oracle import ops as oracle_ops


def _coarse(sd, tex, geo, cam2world, fov, size, steps, t0, t1, jitter, ops):
    """-> per-sample decoder rows [n, R, S, feat+seg+1], depths [n, R, S, 1], camera-space directions [n, R, 3]"""
    n = tex.shape[0]
    points, z_vals, d_cam = ops.initial_rays(n, steps, fov, (size, size), t0, t1)
    if jitter is not None:
        points, z_vals = ops.perturb(points, z_vals, d_cam, jitter.reshape(n, size * size, steps, 1))
    world = ops.to_world(points, cam2world.float())
    out = ogen.sample_voxel(sd, None, tex, geo, world.reshape(n, -1, 3), ops).reshape(n, size * size, steps, -1)
    return out, z_vals, d_cam


def ray_weights(sd, tex, geo, cam2world, fov, size, steps, t0, t1, jitter=None, sigma_noise=None, clamp_mode='softplus',
                ops=oracle_ops):
    """`ide3d_render_ray_weights`: -> (weights [n*R, S], z_vals [n*R, S], pdf_bins [n*R, S-1], pdf_weights [n*R, S-2])."""
    n, rays = tex.shape[0], size * size
    out, z_vals, d_cam = _coarse(sd, tex, geo, cam2world, fov, size, steps, t0, t1, jitter, ops)
    noise = None if sigma_noise is None else sigma_noise.reshape(n, rays, steps, 1)
    _, _, w = ops.composite(out, d_cam, z_vals, noise=noise, clamp_mode=clamp_mode)
    w = w.reshape(n * rays, steps)
    z = z_vals.reshape(n * rays, steps)
    return w, z, 0.5 * (z[:, :-1] + z[:, 1:]), w[:, 1:-1] + 1e-5


def merge(z_fine, z_coarse):
    """`ide3d_merge_depths`: -> (z_all [rays, Sf+Sc], src [rays, Sf+Sc] int32), the stable ascending order of [z_fine | z_coarse]."""
    z_all, order = torch.sort(torch.cat([z_fine, z_coarse], 1), dim=1, stable=True)
    return z_all, order.to(torch.int32)


def render_merged(sd, tex, geo, cam2world, fov, size, steps, t0, t1, jitter, z_all, src, z_fine, clamp_mode='softplus',
                  white_back=False, max_depth=None, ops=oracle_ops):
    """`ide3d_render_rays_merged`: -> (features [n, feat+seg, R], depth [n, R], weight sum [n, R])."""
    n, rays = tex.shape[0], size * size
    out, _z, d_cam = _coarse(sd, tex, geo, cam2world, fov, size, steps, t0, t1, jitter, ops)
    cam2world = cam2world.float()
    rot_only = cam2world.clone()
    rot_only[:, :3, 3] = 0
    dirs = ops.to_world(d_cam, rot_only)                                   # [n, R, 3]
    fine = cam2world[:, None, None, :3, 3] + dirs[:, :, None, :] * z_fine.reshape(n, rays, steps, 1)
    out_f = ogen.sample_voxel(sd, None, tex, geo, fine.reshape(n, -1, 3), ops).reshape(n, rays, steps, -1)
    order = src.reshape(n, rays, 2 * steps, 1).long()
    both = torch.gather(torch.cat([out_f, out], 2), 2, order.expand(-1, -1, -1, out.shape[-1]))
    feat, depth, weights = ops.composite(both, d_cam, z_all.reshape(n, rays, 2 * steps, 1), clamp_mode=clamp_mode,
                                         white_back=white_back, max_depth=max_depth)
    return feat.permute(0, 2, 1), depth[..., 0], weights.sum(2)[..., 0]


def render(sd, tex, geo, cam2world, fov, size, steps, t0, t1, jitter, importance_u, sigma_noise=None, clamp_mode='softplus',
           white_back=False, max_depth=None, ops=oracle_ops):
    """The four launches end to end -> (features [n, feat+seg, size, size], depth [n, 1, size, size], weight sum [n, 1, size, size],
    and the intermediate (z_fine, z_all, src))."""
    n = tex.shape[0]
    _w, z, bins, pw = ray_weights(sd, tex, geo, cam2world, fov, size, steps, t0, t1, jitter, sigma_noise, clamp_mode, ops)
    z_fine = ops.sample_pdf(bins, pw, importance_u)
    z_all, src = merge(z_fine, z)
    feat, depth, wsum = render_merged(sd, tex, geo, cam2world, fov, size, steps, t0, t1, jitter, z_all, src, z_fine, clamp_mode,
                                      white_back, max_depth, ops)
    return feat.reshape(n, -1, size, size), depth.reshape(n, 1, size, size), wsum.reshape(n, 1, size, size), (z_fine, z_all, src)
