"""`project(..., camera_lr=...)` (training/projection.py): pose refinement beside w.  The torch definition on the CPU: this tests the
plumbing (parameter group, switch handling, returned label), not the kernel."""
import numpy as np
import torch


def _tiny():
    from training import triplane
    torch.manual_seed(0)
    return triplane.TriPlaneGenerator(triplane.tiny_spec()).eval().requires_grad_(False)


def _rotated(c, degrees):
    """The camera label turned about the world's y axis."""
    a = np.deg2rad(degrees)
    rot = torch.tensor([[np.cos(a), 0, np.sin(a), 0], [0, 1, 0, 0], [-np.sin(a), 0, np.cos(a), 0], [0, 0, 0, 1]], dtype=torch.float32)
    out = c.clone()
    out[:, :16] = (rot @ c[:, :16].reshape(4, 4)).reshape(1, 16)
    return out


def _target(G, c):
    with torch.no_grad():
        ws = G.mapping(torch.from_numpy(np.random.RandomState(3).randn(1, G.z_dim)).float(), c)
        return ((G.synthesis(ws, c=c, noise_mode='const', force_fp32=True)[0] + 1) * (255 / 2)), ws


KW = dict(num_steps=30, w_avg_samples=64, regularize_noise_weight=1e5)


def test_camera_lr_none_is_the_present_path():
    from training import projection, triplane
    G = _tiny()
    c = triplane.camera_label(0.2)
    target, _ = _target(G, c)
    runs = []
    for kw in ({}, dict(camera_lr=None, camera_project=None)):
        torch.manual_seed(7)
        w, info = projection.project(G, target, c, **dict(KW, num_steps=5), return_info=True, **kw)
        runs.append((w, info))
    assert torch.equal(runs[0][0], runs[1][0]) and runs[0][1]['losses'] == runs[1][1]['losses']
    assert 'c' not in runs[1][1]
    p = projection.Projector(G, target, c, **dict(KW, num_steps=5))
    assert p.cam_opt is None and len(p.optimizer.param_groups) == 1 and p.camera() is p.c


def test_camera_refinement_lowers_the_loss_and_moves_towards_the_true_pose():
    from training import projection, triplane
    G = _tiny()
    c_true = triplane.camera_label(0.2)
    target, ws = _target(G, c_true)
    c_start = _rotated(c_true, 4.0)
    l2 = projection.l2_distance(target[None])
    # w fixed at the true latent's neighbourhood (initial_w, tiny learning rate, no noise maps' weight change): what moves is the camera
    common = dict(KW, initial_w=ws, initial_learning_rate=1e-4, initial_noise_factor=0.0, distance=l2)
    before = triplane.fused_render_camera_grad
    torch.manual_seed(11)
    _, fixed = projection.project(G, target, c_start, return_info=True, **common)
    seen = []
    torch.manual_seed(11)
    _, refined = projection.project(G, target, c_start, return_info=True, camera_lr=2e-3,
                                    camera_project=lambda m: (seen.append(triplane.fused_render_camera_grad), m)[1], **common)
    assert triplane.fused_render_camera_grad is before, 'the switch must be restored'
    assert len(seen) == 30 and not any(seen), 'camera_project runs after every step, outside the pass'
    assert refined['losses'][-1] < fixed['losses'][-1], (refined['losses'][-1], fixed['losses'][-1])
    c_out = refined['c']
    assert c_out.shape == (1, 25) and torch.equal(c_out[:, 16:], c_start[:, 16:]), 'the intrinsics stay fixed'
    d0 = float((c_start[:, :12] - c_true[:, :12]).norm()); d1 = float((c_out[:, :12] - c_true[:, :12]).norm())
    assert d1 < d0, (d1, d0)
    assert torch.equal(c_out[:, 12:16], c_start[:, 12:16]), 'the last row has no gradient'


def test_camera_project_is_applied():
    from training import projection, triplane
    G = _tiny()
    c = triplane.camera_label(0.2)
    target, _ = _target(G, c)
    _, info = projection.project(G, target, c, return_info=True, camera_lr=1e-3, camera_project=lambda m: torch.zeros_like(m) + 0.5,
                                 **dict(KW, num_steps=2))
    assert torch.equal(info['c'][:, :16], torch.full((1, 16), 0.5))
