"""Gradient of the fused renderer with respect to the camera pose (`ide3d_render_rays_backward_camera`, ide-3d_amd/csrc/raymarch_bwd.hip),
called through the plugin, through `TriplaneRenderer.forward` under `triplane.fused_render_camera_grad`, and through `G.synthesis` with a
camera label that requires grad.  `pytest -m gpu`.

Reference: float64 CPU autograd through the step-wise definition (camera-space points and jitter in fp32 as get_initial_rays_trig /
perturb_points make them, then in float64: the camera transform of transform_sampled_points, `sample_from_triplane`, the decoder and
`fancy_integration`), same jitter and noise tensors, loss = a fixed random linear functional of all three outputs (or of one of them).
Error of an image = max |d - d_ref| / max |d_ref| over the 12 entries of the top three rows of its 4 x 4 gradient; the last row must be
exactly zero.  No entry, sample or ray is excluded anywhere.

Two families of planes.  The derivative of a bilinear blend jumps at texel boundaries, and a coordinate within rounding of one can land in
different cells in fp32 and in float64:
  smooth    a few sinusoids of at most 1.5 rad per unit sampled on the grid: a flipped cell moves one sample's derivative by at most
            1.5 * 2 / size of itself.  Bound: GRAD_TOL = 1e-4, the renderer gradients' own (tests/test_gpu_render_grad.py).
  gauss     independent normal texels.  The bound is not fixed in advance: the test measures, on the CPU, how far fp32 autograd of the
            same step-wise definition lies from its float64 run for the very inputs of the case (a quantity of the reference alone), and
            allows 10 times that (the kernel sums in another order and its taps come from non-contracted fp32).  Measured for the
            cases below: 2.3e-7 .. 5.2e-6 per image, so bounds of 2.3e-6 .. 5.2e-5; the kernel's own distance from float64 on an
            MI355X was 1.0e-7 .. 8.5e-6, at most 5.9 times the reference's on the same image.
"""

import contextlib

import numpy as np
import pytest
import torch

from test_gpu_render_grad import GRAD_TOL, _calls, _cameras, _projections

pytestmark = pytest.mark.gpu

NEW = 'render_rays_backward_camera'
SIZE = 12                  # 144 rays per image: workgroups of 8 rays straddle images at batch 3
FORMS = {'c32': dict(), 'c16': dict(plane_channels=16, decoder_hidden=32, feature_channels=8, seg_channels=5)}

CASES = {
    'b1_s17_sq16': dict(n=1, steps=17, plane=(16, 16)),
    'b3_s64_noise': dict(n=3, steps=64, noise=True),
    'b3_s65_nojitter': dict(n=3, steps=65, jitter=False),
    'b1_s1': dict(n=1, steps=1, jitter=False, plane=(16, 16)),
    'b3_s96_white_noise': dict(n=3, steps=96, noise=True, white_back=True),
    'b3_s17_depth_only': dict(n=3, steps=17, loss='depth'),
    # relu densities centred at 0: with softplus every ray's weights sum to 1 (the last delta is 1e10) and d wsum vanishes.  Gaussian planes
    # only: a smooth field's rays are dense or empty as a whole, and d wsum vanishes again
    'b3_s17_wsum_only': dict(n=3, steps=17, loss='wsum', spec=dict(clamp_mode='relu')),
    'b3_s17_feat_only': dict(n=3, steps=17, loss='feat', noise=True),
    'b3_s17_seg0': dict(n=3, steps=17, spec=dict(seg_channels=0)),
    'b3_s17_widest': dict(n=3, steps=17, spec=dict(feature_channels=32, seg_channels=31)),
    'b3_s17_leaving': dict(n=3, steps=17, cams='leaving'),
    'b3_s17_nonortho': dict(n=3, steps=17, cams='nonortho', noise=True),
}
GAUSS_CASES = ('b1_s17_sq16', 'b3_s64_noise', 'b3_s65_nojitter', 'b3_s17_nonortho', 'b3_s17_wsum_only')
SMOOTH_CASES = tuple(k for k in CASES if k != 'b3_s17_wsum_only')


@contextlib.contextmanager
def _camera_grad(on):
    from training import triplane
    old = triplane.fused_render_camera_grad
    triplane.fused_render_camera_grad = on
    try:
        yield
    finally:
        triplane.fused_render_camera_grad = old


def _smooth_planes(n, ch, H, W, g):
    """[n, ch, H, W]: per channel three sinusoids of at most 1.5 rad per unit of the normalised coordinate, sampled at the texel centres"""
    y = ((torch.arange(H, dtype=torch.float64) + 0.5) * 2 / H - 1).reshape(1, 1, 1, H, 1)
    x = ((torch.arange(W, dtype=torch.float64) + 0.5) * 2 / W - 1).reshape(1, 1, 1, 1, W)
    k = (torch.rand(n, ch, 3, 1, 2, generator=g, dtype=torch.float64) * 2 - 1) * 1.5
    ph = torch.rand(n, ch, 3, 1, 1, generator=g, dtype=torch.float64) * 6.283
    amp = torch.randn(n, ch, 3, 1, 1, generator=g, dtype=torch.float64) * 0.5
    return (amp * torch.sin(k[..., :1] * x + k[..., 1:] * y + ph)).sum(2).float()


def _case_cameras(case, seed):
    n, kind = case['n'], case.get('cams')
    cam = _cameras(n, seed)
    if kind == 'leaving':
        # pulled back along the viewing axis and turned about y, each image differently: a good part of every ray misses the cube
        g = np.random.RandomState(seed)
        for i in range(n):
            a = float(g.uniform(0.22, 0.3)) * (1 if i % 2 else -1)
            rot = torch.tensor([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]], dtype=torch.float32)
            cam[i, :3, :3] = rot @ cam[i, :3, :3]
            cam[i, :3, 3] = cam[i, :3, 3] * float(g.uniform(1.3, 1.45))
    elif kind == 'nonortho':
        cam[:, :3, :3] += torch.randn(n, 3, 3, generator=torch.Generator().manual_seed(seed)) * 0.05
    return cam


def _setup(form, case, family, seed):
    from training import triplane
    kw = dict(FORMS[form]); kw.update(case.get('spec', {}))
    sp = triplane.GeneratorSpec(**kw, render_size=SIZE, num_steps=case['steps'])
    torch.manual_seed(seed)
    Rc = triplane.TriplaneRenderer(sp)
    with torch.no_grad():
        for p in Rc.parameters():
            if p.ndim == 1:
                p.copy_(torch.randn_like(p) * 0.2)
    Rc.requires_grad_(False)
    Rg = triplane.TriplaneRenderer(sp).cuda()
    Rg.load_state_dict(Rc.state_dict())
    Rg.requires_grad_(False)
    n, C, S = case['n'], sp.plane_channels, case['steps']
    H, W = case.get('plane', (24, 16))
    g = torch.Generator().manual_seed(seed + 1)
    both = _smooth_planes(n, 6 * C, H, W, g) if family == 'smooth' else torch.randn(n, 6 * C, H, W, generator=g) * 0.7
    if sp.clamp_mode == 'relu':
        # as tests/test_gpu_render_grad.py does: about half of all samples of the rendered volume get density 0
        with torch.no_grad():
            probe = (torch.rand(n, 4096, 3, generator=g) - 0.5) * 0.6
            sig = Rc.sample_voxel(both[:, :3 * C], both[:, 3 * C:], probe)[:, -1]
            Rc.decoder.geo1.bias[0] -= float(sig.median()) / Rc.decoder.geo1.bias_gain
            Rg.load_state_dict(Rc.state_dict())
    jit = torch.rand(n, SIZE * SIZE, S, generator=g) if case.get('jitter', True) else None
    noise = torch.randn(n, SIZE * SIZE, S, generator=g) * 0.5 if case.get('noise') else None
    P = _projections(n, sp.feature_channels + sp.seg_channels, SIZE, seed + 3)
    return sp, Rg, Rc, both, _case_cameras(case, seed + 2), jit, noise, P


def _loss(feat, depth, wsum, P, which):
    Pf, Pd, Pw = (x.to(feat.device, feat.dtype) for x in P)
    terms = dict(feat=(feat * Pf).sum(), depth=(depth * Pd).sum(), wsum=(wsum * Pw).sum())
    return terms[which] if which else terms['feat'] + terms['depth'] + terms['wsum']


def _stepwise(sp, Rc, both, cam, jit, noise, white_back, dtype):
    """The step-wise definition on the CPU in `dtype` -> (feat, depth, wsum [n, ch | 1, SIZE, SIZE], world points): graph nodes of `cam`."""
    from training import volumetric_rendering as vr
    n, S, C = both.shape[0], sp.num_steps, sp.plane_channels
    R = Rc.double() if dtype == torch.float64 else Rc.float()
    p0, z, d_cam = vr.get_initial_rays_trig(n, S, 'cpu', sp.fov, (SIZE, SIZE), sp.ray_start, sp.ray_end)
    if jit is not None:
        p0, z = vr.perturb_points(p0, z, d_cam, 'cpu', jitter=jit.unsqueeze(-1))
    q = p0.reshape(n, -1, 3).to(dtype)
    wp = torch.bmm(q, cam[:, :3, :3].transpose(1, 2)) + cam[:, :3, 3].unsqueeze(1)
    b = both.to(dtype)
    out = R.sample_voxel(b[:, :3 * C], b[:, 3 * C:], wp).reshape(n, SIZE * SIZE, S, -1)
    nz = noise.unsqueeze(-1).to(dtype) if noise is not None else None
    if S > 1:
        f, d, w = vr.fancy_integration(out, d_cam.to(dtype), z.to(dtype), 'cpu', noise_std=(1.0 if nz is not None else 0.0), noise=nz,
                                       clamp_mode=sp.clamp_mode, white_back=white_back)
    else:
        # fancy_integration's deltas are empty for a single step; the oracle's loop gives that sample delta 1e10, as the kernel does
        from oracle import ops as oracle_ops
        f, d, w = oracle_ops.composite(out, d_cam, z, noise=nz, clamp_mode=sp.clamp_mode, white_back=white_back)
    f, d, w = f.permute(0, 2, 1), d.permute(0, 2, 1), w.sum(2).permute(0, 2, 1)
    return f.reshape(n, -1, SIZE, SIZE), d.reshape(n, 1, SIZE, SIZE), w.reshape(n, 1, SIZE, SIZE), wp


def _cpu_grad(sp, Rc, both, cam, jit, noise, case, P, dtype):
    c = cam.to(dtype).requires_grad_(True)
    f, d, w, wp = _stepwise(sp, Rc, both, c, jit, noise, case.get('white_back', False), dtype)
    (g,) = torch.autograd.grad(_loss(f, d, w, P, case.get('loss')), [c])
    return g, wp.detach()


def _image_errors(got, want):
    got, want = got.detach().cpu().double(), want.detach().cpu().double()
    assert got.shape == want.shape == (want.shape[0], 4, 4)
    assert float(got[:, 3].abs().max()) == 0.0, 'the last row of the camera gradient must be exactly zero'
    return [float((got[i, :3] - want[i, :3]).abs().max()) / float(want[i, :3].abs().max()) for i in range(want.shape[0])]


def _plugin_call(sp, Rg, both, cam, jit, noise, case, P, planes, params):
    """One direct call of the new plugin method -> its result tuple."""
    from training import volumetric_rendering as vr
    vr._init()
    n, C = both.shape[0], sp.plane_channels
    dev = torch.device('cuda')
    tex = both[:, :3 * C].to(dev).contiguous(memory_format=torch.channels_last)
    geo = both[:, 3 * C:].to(dev).contiguous(memory_format=torch.channels_last)
    rays_d_cam, z_lin = vr._fused_ray_setup(dev, float(sp.fov), (SIZE, SIZE), sp.num_steps, float(sp.ray_start), float(sp.ray_end))
    with torch.no_grad():
        mlp = Rg.decoder.kernel_weights()
    which = case.get('loss')
    gf, gd, gw = (None if (which and which != name) else t.reshape(n, -1, SIZE * SIZE).to(dev) for name, t in zip(('feat', 'depth', 'wsum'), P))
    args = (rays_d_cam, z_lin, cam.to(dev), None if jit is None else jit.to(dev), None if noise is None else noise.to(dev), tex, geo, mlp,
            0 if sp.clamp_mode == 'softplus' else 1, False, case.get('white_back', False), None, gf, None if gd is None else gd.reshape(n, -1), None if gw is None else gw.reshape(n, -1))
    res = vr._plugin.render_rays_backward_camera(*args, plane_grads=planes, param_grads=params)
    torch.cuda.synchronize()
    assert res is not None
    return res, args


@pytest.mark.parametrize('case_id', SMOOTH_CASES)
@pytest.mark.parametrize('form', list(FORMS))
def test_camera_gradient_vs_float64_smooth(gpu_device, form, case_id):
    case = CASES[case_id]
    seed = 100 + sorted(CASES).index(case_id) * 10 + sorted(FORMS).index(form)
    sp, Rg, Rc, both, cam, jit, noise, P = _setup(form, case, 'smooth', seed)
    before = _calls(NEW)
    (_, _, _, got), _ = _plugin_call(sp, Rg, both, cam, jit, noise, case, P, planes=False, params=False)
    assert _calls(NEW) - before == 1
    want, wp = _cpu_grad(sp, Rc, both, cam, jit, noise, case, P, torch.float64)
    outside = float((wp.abs().amax(-1) > 1).double().mean())
    if case.get('cams') == 'leaving':
        assert outside >= 1 / 3, f'only {outside:.2f} of the samples leave the cube'
    assert all(float(want[i, :3].abs().max()) > 1e-3 for i in range(case['n'])), 'a reference gradient of rounding size tests nothing'
    errs = _image_errors(got, want)
    print(f'[render-camera-grad] smooth {form} {case_id}: per-image err ' + ', '.join(f'{e:.2e}' for e in errs) + f'; {outside:.2f} of the samples outside')
    assert max(errs) <= GRAD_TOL, f'{form} {case_id}: {errs} > {GRAD_TOL}'


@pytest.mark.parametrize('case_id', GAUSS_CASES)
@pytest.mark.parametrize('form', list(FORMS))
def test_camera_gradient_vs_float64_gauss(gpu_device, form, case_id):
    """Bound per image: 10 x the distance of fp32 CPU autograd of the step-wise definition from its float64 run on the same inputs."""
    case = CASES[case_id]
    seed = 300 + sorted(CASES).index(case_id) * 10 + sorted(FORMS).index(form)
    sp, Rg, Rc, both, cam, jit, noise, P = _setup(form, case, 'gauss', seed)
    want, _ = _cpu_grad(sp, Rc, both, cam, jit, noise, case, P, torch.float64)
    own, _ = _cpu_grad(sp, Rc, both, cam, jit, noise, case, P, torch.float32)
    ref_err = _image_errors(own, want)
    (_, _, _, got), _ = _plugin_call(sp, Rg, both, cam, jit, noise, case, P, planes=False, params=False)
    errs = _image_errors(got, want)
    print(f'[render-camera-grad] gauss {form} {case_id}: per-image err ' + ', '.join(f'{e:.2e}' for e in errs)
          + '; fp32 CPU autograd vs float64 ' + ', '.join(f'{e:.2e}' for e in ref_err))
    assert all(e > 0 for e in ref_err) and all(float(want[i, :3].abs().max()) > 1e-3 for i in range(case['n']))
    assert all(e <= 10 * r for e, r in zip(errs, ref_err)), f'{form} {case_id}: {errs} against 10 x {ref_err}'


@pytest.mark.parametrize('form', list(FORMS))
def test_camera_out_of_sight_gets_exact_zeros(gpu_device, form):
    case = dict(n=2, steps=17, noise=True)
    sp, Rg, Rc, both, cam, jit, noise, P = _setup(form, case, 'gauss', 500)
    cam[:, :3, 3] += 40.0
    (_, _, _, got), _ = _plugin_call(sp, Rg, both, cam, jit, noise, case, P, planes=False, params=False)
    want, wp = _cpu_grad(sp, Rc, both, cam, jit, noise, case, P, torch.float64)
    assert float(wp.abs().amax(-1).min()) > 2 and float(want.abs().max()) == 0.0
    assert float(got.abs().max()) == 0.0, 'every tap is dropped: the camera gradient must be exactly zero'


@pytest.mark.parametrize('form', list(FORMS))
def test_call_forms_agree(gpu_device, form):
    """Camera alone (NULL plane buffers), camera + planes, camera + planes + decoder: the camera gradient is equal bit for bit in all three
    and in a second run; the decoder gradients equal those of render_rays_backward_params bit for bit; the plane gradients those of
    render_rays_backward to fp32 rounding (their atomics arrive in any order)."""
    from training import volumetric_rendering as vr
    case = CASES['b3_s65_nojitter'] | dict(noise=True)
    sp, Rg, Rc, both, cam, jit, noise, P = _setup(form, case, 'gauss', 600)
    (t0, g0, m0, alone), args = _plugin_call(sp, Rg, both, cam, jit, noise, case, P, planes=False, params=False)
    (t1, g1, m1, with_planes), _ = _plugin_call(sp, Rg, both, cam, jit, noise, case, P, planes=True, params=False)
    (t2, g2, m2, with_all), _ = _plugin_call(sp, Rg, both, cam, jit, noise, case, P, planes=True, params=True)
    (_, _, _, again), _ = _plugin_call(sp, Rg, both, cam, jit, noise, case, P, planes=True, params=True)
    assert t0 is None and g0 is None and m0 is None and m1 is None
    assert float(alone.abs().max()) > 0
    for name, other in (('with planes', with_planes), ('with planes and decoder', with_all), ('second run', again)):
        assert torch.equal(alone, other), f'camera gradient {name} differs from the camera-only call'
    ref_t, ref_g, ref_m = vr._plugin.render_rays_backward_params(*args)
    torch.cuda.synchronize()
    assert sorted(m2) == sorted(ref_m)
    for k in ref_m:
        assert torch.equal(m2[k], ref_m[k]), f'{k}: decoder gradient differs from render_rays_backward_params'
    plain_t, plain_g = vr._plugin.render_rays_backward(*args)
    torch.cuda.synchronize()
    for name, a, b in (('tex', t1, plain_t), ('geo', g1, plain_g), ('tex (all)', t2, plain_t), ('geo (all)', g2, plain_g)):
        e = float((a - b).abs().max()) / float(b.abs().max())
        assert e <= 1e-5, f'd {name} planes: {e:.2e} from render_rays_backward'


def test_module_routing(gpu_device):
    """Switch on: a camera that requires grad takes the fused path (one forward launch, the new backward once, no step-wise gather) with
    frozen planes and with trainable ones; a jitter that requires grad still declines.  Switch off: the new entry point is not reached."""
    case = dict(n=3, steps=17, noise=True)
    sp, Rg, Rc, both, cam, jit, noise, P = _setup('c32', case, 'smooth', 700)
    C = sp.plane_channels
    want, _ = _cpu_grad(sp, Rc, both, cam, jit, noise, case, P, torch.float64)
    watch = (NEW, 'render_rays', 'render_rays_backward', 'render_rays_backward_params', 'triplane_sample', 'triplane_sample_backward', 'composite')

    def run(planes_grad, jit_grad=False):
        tex = both[:, :3 * C].cuda().contiguous(memory_format=torch.channels_last).requires_grad_(planes_grad)
        geo = both[:, 3 * C:].cuda().contiguous(memory_format=torch.channels_last).requires_grad_(planes_grad)
        c = cam.cuda().requires_grad_(True)
        j = jit.cuda().requires_grad_(jit_grad)
        before = {k: _calls(k) for k in watch}
        out = Rg(tex, geo, c, jitter=j, sigma_noise=noise.cuda())
        grads = torch.autograd.grad(_loss(*out, P, None), [c] + ([tex, geo] if planes_grad else []))
        torch.cuda.synchronize()
        return grads, {k: _calls(k) - before[k] for k in watch}

    fused = {k: 0 for k in watch} | {NEW: 1, 'render_rays': 1}
    with _camera_grad(True):
        for planes_grad in (False, True):
            grads, route = run(planes_grad)
            assert route == fused, route
            assert max(_image_errors(grads[0], want)) <= GRAD_TOL
            assert all(float(g.abs().max()) > 0 for g in grads)
        grads, route = run(False, jit_grad=True)
        assert route[NEW] == 0 and route['render_rays'] == 0, route
        assert max(_image_errors(grads[0] * torch.tensor([1., 1, 1, 0], device='cuda').reshape(1, 4, 1), want)) <= GRAD_TOL
    with _camera_grad(False):
        grads, route = run(True)
        assert route[NEW] == 0 and route['render_rays_backward'] == 0, route


def test_synthesis_camera_label_gradient(gpu_device):
    """G.synthesis(ws, c) of the tiny generator with c.requires_grad: d c[:, :16] through the fused renderer against fp32 CPU autograd of
    the same module; the intrinsics get no gradient."""
    from training import triplane
    torch.manual_seed(0)
    G = triplane.TriPlaneGenerator(triplane.tiny_spec()).eval().requires_grad_(False)
    g = torch.Generator().manual_seed(5)
    z = torch.randn(2, G.z_dim, generator=g)
    c0 = torch.cat([triplane.camera_label(0.3), triplane.camera_label(-0.2)])
    jit = torch.rand(2, G.synthesis.render_size ** 2, G.spec.num_steps, generator=g)
    with torch.no_grad():
        ws = G.mapping(z, triplane.conditioning_label().repeat(2, 1))

    def grad_of(Gx, dev):
        c = c0.to(dev).requires_grad_(True)
        img, seg = Gx.synthesis(ws.to(dev), c=c, noise_mode='const', ray_jitter=jit.to(dev), return_seg=True, force_fp32=True)
        (gc,) = torch.autograd.grad(((img - 0.1) ** 2).sum() + 0.01 * (seg ** 2).sum(), [c])
        return gc

    want = grad_of(G, 'cpu')
    import copy
    Gd = copy.deepcopy(G).to(gpu_device)
    with _camera_grad(True):
        before = _calls(NEW)
        got = grad_of(Gd, gpu_device).cpu()
        torch.cuda.synchronize()
        assert _calls(NEW) - before == 1
    assert float(got[:, 16:].abs().max()) == 0.0 and float(got[:, 12:16].abs().max()) == 0.0
    e = float((got[:, :12] - want[:, :12]).abs().max()) / float(want[:, :12].abs().max())
    print(f'[render-camera-grad] synthesis d c[:, :12] fused vs fp32 CPU autograd err {e:.2e} of max-abs')
    assert float(want[:, :12].abs().max()) > 0
    assert e <= 1e-3, f'd c: {e:.2e}'          # the bound of test_gpu_render_grad.py::test_synthesis_latent_gradient for the same module
