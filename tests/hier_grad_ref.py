"""Float64 reference for the gradients of the merged march (`ide3d_render_rays_merged_backward`): CPU autograd
through the step-wise definition of the importance pass (TriplaneRenderer.forward, training/triplane.py) with the fine depths, the merged
depths and their order given as constants, as that definition takes them (it draws z_fine and forms the fine points under no_grad).
TEST INFRASTRUCTURE ONLY.

Point set-up in fp32 like the reference implementation (tests/test_gpu_render_grad.py::_reference): coarse points through
get_initial_rays_trig / transform_sampled_points, fine points rays_o + rays_d * z_fine.  Both are cast to float64 for the gather, the
decoder and fancy_integration; rows are concatenated [fine | coarse] and gathered by src.
"""

import torch


def renderer64(spec, sd):
    """A float64 CPU TriplaneRenderer with the weights of `sd` (a generator state dict, keys `synthesis.renderer.*`), frozen."""
    from training import triplane
    R = triplane.TriplaneRenderer(spec)
    prefix = 'synthesis.renderer.'
    R.load_state_dict({k[len(prefix):]: v.detach().cpu().float() for k, v in sd.items() if k.startswith(prefix)})
    return R.double().requires_grad_(False)


def merged_outputs(R64, tex, geo, cam, fov, size, steps, t0, t1, jitter, z_all, src, z_fine, clamp_mode='softplus', white_back=False,
                   max_depth=None, rays=None):
    """tex / geo [n, 3C, H, W] float64 (graph leaves or views of one), R64 from `renderer64` (its decoder parameters may require grad);
    cam [n, 4, 4], jitter [n, R, S] | None, z_all / src [n * R, 2S], z_fine [n * R, S]: fp32 / int32 constants.
    -> (features [n, ch, size, size], depth [n, 1, size, size], weight sum [n, 1, size, size]) as graph nodes; with `rays` (indices into
    an image's rays) only those rays are rendered: [n, ch, len(rays)], [n, 1, len(rays)], [n, 1, len(rays)]."""
    from training import volumetric_rendering as vr
    n, R, S = tex.shape[0], size * size, steps
    p0, z, d_cam = vr.get_initial_rays_trig(n, S, 'cpu', fov, (size, size), t0, t1)
    j = jitter.float().reshape(n, R, S, 1) if jitter is not None else torch.full_like(z, 0.5)
    z_all = z_all.float().reshape(n, R, 2 * S, 1)
    z_fine = z_fine.float().reshape(n, R, S, 1)
    order = src.long().reshape(n, R, 2 * S, 1)
    if rays is not None:
        p0, z, d_cam, j, z_all, z_fine, order = (x[:, rays] for x in (p0, z, d_cam, j, z_all, z_fine, order))
    nr = p0.shape[1]
    with torch.no_grad():
        pts, _z, rays_d, rays_o, _p, _y = vr.transform_sampled_points(p0, z, d_cam, 'cpu', h_stddev=0, v_stddev=0, camera=cam.float(),
                                                                      mode=None, jitter=j)
        pts_fine = rays_o.unsqueeze(2) + rays_d.unsqueeze(2) * z_fine
    out = R64.sample_voxel(tex, geo, pts.reshape(n, -1, 3).double()).reshape(n, nr, S, -1)
    out_fine = R64.sample_voxel(tex, geo, pts_fine.reshape(n, -1, 3).double()).reshape(n, nr, S, -1)
    both = torch.gather(torch.cat([out_fine, out], 2), 2, order.expand(-1, -1, -1, out.shape[-1]))
    f, d, w = vr.fancy_integration(both, d_cam.double(), z_all.double(), 'cpu', noise_std=0, clamp_mode=clamp_mode, white_back=white_back,
                                   max_depth=max_depth)
    f, d, w = f.permute(0, 2, 1), d.permute(0, 2, 1), w.sum(2).permute(0, 2, 1)
    if rays is None:
        return f.reshape(n, -1, size, size), d.reshape(n, 1, size, size), w.reshape(n, 1, size, size)
    return f, d, w


def loss(feat, depth, wsum, P, feat_only=False):
    """sum(feat * Pf) + sum(depth * Pd) + sum(wsum * Pw), or the feature term alone."""
    Pf, Pd, Pw = (x.to(feat.device, feat.dtype).reshape(s.shape) for x, s in zip(P, (feat, depth, wsum)))
    total = (feat * Pf).sum()
    return total if feat_only else total + (depth * Pd).sum() + (wsum * Pw).sum()
