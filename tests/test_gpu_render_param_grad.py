"""Gradients of the fused renderer with respect to the decoder MLPs (`ide3d_render_rays_backward_params`, ide-3d_amd/csrc/raymarch_bwd.hip),
reached through `TriplaneRenderer.forward` under `triplane.fused_render_param_grad` and through `render_triplane_fused` with a trainable
decoder.  `pytest -m gpu`.

Reference, loss, cases and the bound are those of tests/test_gpu_render_grad.py (float64 CPU autograd through the step-wise definition;
GRAD_TOL = 1e-4 of each reference gradient's max-abs), applied to the gradients of the module's own `weight` and `bias` of geo0, geo1, tex0
and tex1 (so the gain chain of FullyConnectedLayer.effective is covered) beside the two plane gradients.
"""

import contextlib
import copy

import numpy as np
import pytest
import torch

from test_gpu_render_grad import CASES, FORMS, GRAD_TOL, _arithmetic, _calls, _err, _gpu_planes, _loss, _projections, _reference, _render_gpu, _setup

pytestmark = pytest.mark.gpu

NEW = 'render_rays_backward_params'
ROUTE = ('render_rays', NEW, 'render_rays_backward', 'triplane_sample_backward')


@contextlib.contextmanager
def _param_grad(on):
    from training import triplane
    old = triplane.fused_render_param_grad
    triplane.fused_render_param_grad = on
    try:
        yield
    finally:
        triplane.fused_render_param_grad = old


def _decoder_params(R):
    return dict(R.decoder.named_parameters())


def _compare(tag, got, want, tol=GRAD_TOL, need_nonzero=False):
    """got / want: {name: gradient}.  A reference gradient that is identically zero must be matched by exact zeros."""
    errs = {}
    for k, w in want.items():
        if float(w.abs().max()) == 0.0:
            assert not need_nonzero, f'{tag}: the reference gradient of {k} is identically zero'
            assert float(got[k].abs().max()) == 0.0, f'{tag}: {k} must be exactly zero'
            errs[k] = 0.0
        else:
            errs[k] = _err(got[k], w)
    print(f'[render-param-grad] {tag}: ' + ', '.join(f'{k} {v:.2e}' for k, v in errs.items()))
    bound = tol if isinstance(tol, dict) else {k: tol for k in errs}
    bad = {k: (v, bound[k]) for k, v in errs.items() if not v <= bound[k]}
    assert not bad, f'{tag}: (error, bound) of max-abs {bad}'
    return errs


def _float64_grads(sp, Rc, both, C, cam, jit, noise, case, P, feat_only, rays=None):
    both64 = both.double().requires_grad_(True)
    f64, d64, w64 = _reference(sp, Rc, both64[:, :3 * C], both64[:, 3 * C:], cam, jit, noise, case.get('white_back', False),
                               case.get('max_depth'), rays=rays)
    names = list(_decoder_params(Rc))
    grads = torch.autograd.grad(_loss(f64, d64, w64, P, feat_only), [both64] + [_decoder_params(Rc)[k] for k in names], allow_unused=True)
    want = {k: (g if g is not None else torch.zeros_like(_decoder_params(Rc)[k])) for k, g in zip(names, grads[1:])}
    want['tex_planes'], want['geo_planes'] = grads[0][:, :3 * C], grads[0][:, 3 * C:]
    return want, w64


def _gpu_grads(sp, Rg, both, C, cam, jit, noise, case, P, feat_only, planes=True):
    """One forward and backward on the GPU -> ({name: gradient}, CALLS deltas of ROUTE)."""
    leaves, tex, geo = _gpu_planes(both, C, case)
    if not planes:
        leaves, tex, geo = [], tex.detach(), geo.detach()
    names = [k for k, p in _decoder_params(Rg).items() if p.requires_grad]
    before = {k: _calls(k) for k in ROUTE}
    feat, depth, wsum = _render_gpu(sp, Rg, tex, geo, cam, jit, noise, case)
    grads = torch.autograd.grad(_loss(feat, depth, wsum, P, feat_only), leaves + [_decoder_params(Rg)[k] for k in names])
    torch.cuda.synchronize()
    got = dict(zip(names, grads[len(leaves):]))
    if planes:
        g = grads[0] if case.get('views') else torch.cat([grads[0], grads[1]], 1)
        got['tex_planes'], got['geo_planes'] = g[:, :3 * C], g[:, 3 * C:]
    return got, {k: _calls(k) - before[k] for k in ROUTE}


FUSED_ROUTE = {'render_rays': 1, NEW: 1, 'render_rays_backward': 0, 'triplane_sample_backward': 0}


@pytest.mark.parametrize('case_id', list(CASES))
@pytest.mark.parametrize('form', list(FORMS))
def test_all_gradients_vs_float64(gpu_device, form, case_id):
    case = CASES[case_id]
    seed = sorted(CASES).index(case_id) * 10 + sorted(FORMS).index(form)
    sp, Rg, Rc, both, cam, jit, noise = _setup(form, case, seed)
    Rg.decoder.requires_grad_(True); Rc.decoder.requires_grad_(True)
    n, C, size = case['n'], sp.plane_channels, sp.render_size
    P = _projections(n, sp.feature_channels + sp.seg_channels, size, seed + 3)
    feat_only = case.get('loss') == 'feat'
    with _arithmetic(FORMS[form][0]), _param_grad(True):
        got, route = _gpu_grads(sp, Rg, both, C, cam, jit, noise, case, P, feat_only)
    assert route == FUSED_ROUTE, route
    want, w64 = _float64_grads(sp, Rc, both, C, cam, jit, noise, case, P, feat_only)
    if sp.clamp_mode == 'relu':
        assert float((1 - w64).max()) > 0.05, 'relu case: every ray saturated, white_back / max_depth untested'
    assert set(got) == set(want) and len(want) == 10
    _compare(f'{form} {case_id}', got, want, need_nonzero=(sp.clamp_mode == 'relu' or feat_only))


@pytest.mark.parametrize('form', list(FORMS))
def test_decoder_only_on_detached_planes(gpu_device, form):
    """No plane requires grad: the plane gradient pointers are NULL, nothing of a plane's size is allocated."""
    from training import volumetric_rendering as vr
    case = CASES['s33_crossing_noise']
    sp, Rg, Rc, both, cam, jit, noise = _setup(form, case, 41)
    Rg.decoder.requires_grad_(True); Rc.decoder.requires_grad_(True)
    n, C, size = case['n'], sp.plane_channels, sp.render_size
    P = _projections(n, sp.feature_channels + sp.seg_channels, size, 42)
    with _arithmetic(FORMS[form][0]), _param_grad(True):
        got, route = _gpu_grads(sp, Rg, both, C, cam, jit, noise, case, P, False, planes=False)
        assert route == FUSED_ROUTE, route
        # the binding itself: (None, None, eight gradients)
        _, tex, geo = _gpu_planes(both, C, case)
        rays_d_cam, z_lin = vr._fused_ray_setup(tex.device, float(sp.fov), (size, size), sp.num_steps, float(sp.ray_start), float(sp.ray_end))
        with torch.no_grad():
            mlp = Rg.decoder.kernel_weights()
        gf = P[0].reshape(n, -1, size * size).cuda()
        res = vr._plugin.render_rays_backward_params(rays_d_cam, z_lin, cam.cuda(), jit.cuda(), noise.cuda(), tex.detach(), geo.detach(), mlp,
                                                     0, False, False, None, gf, None, None, plane_grads=False)
        torch.cuda.synchronize()
    assert res[0] is None and res[1] is None, 'a plane gradient buffer was allocated'
    assert sorted(res[2]) == sorted(mlp) and all(res[2][k].shape == mlp[k].shape for k in mlp)
    want, _ = _float64_grads(sp, Rc, both, C, cam, jit, noise, case, P, False)
    _compare(f'{form} decoder only', got, {k: want[k] for k in got})


@pytest.mark.parametrize('name', ['tex1.bias', 'geo1.weight', 'geo0.weight'])
def test_one_parameter_alone(gpu_device, name):
    case = CASES['s17_225rays']
    sp, Rg, Rc, both, cam, jit, noise = _setup('c32_fp32', case, 51)
    _decoder_params(Rg)[name].requires_grad_(True)
    Rc.decoder.requires_grad_(True)
    C, size = sp.plane_channels, sp.render_size
    P = _projections(case['n'], sp.feature_channels + sp.seg_channels, size, 52)
    with _arithmetic('fp32'), _param_grad(True):
        got, route = _gpu_grads(sp, Rg, both, C, cam, jit, noise, case, P, False, planes=False)
    assert route == FUSED_ROUTE, route
    assert list(got) == [name]
    want, _ = _float64_grads(sp, Rc, both, C, cam, jit, noise, case, P, False)
    _compare(f'{name} alone', got, {name: want[name]})


@pytest.mark.parametrize('form', list(FORMS))
def test_decoder_gradients_are_bit_reproducible(gpu_device, form):
    """Two backward passes of one graph: the per-wave partial sums are added in a fixed order, so the eight decoder gradients are equal bit
    for bit (the plane gradients, summed by atomics, are not required to be)."""
    case = CASES['s33_crossing_noise']
    sp, Rg, Rc, both, cam, jit, noise = _setup(form, case, 61)
    Rg.decoder.requires_grad_(True)
    C = sp.plane_channels
    P = _projections(case['n'], sp.feature_channels + sp.seg_channels, sp.render_size, 62)
    leaves, tex, geo = _gpu_planes(both, C, case)
    params = list(_decoder_params(Rg).values())
    with _arithmetic(FORMS[form][0]), _param_grad(True):
        before = _calls(NEW)
        feat, depth, wsum = _render_gpu(sp, Rg, tex, geo, cam, jit, noise, case)
        loss = _loss(feat, depth, wsum, P, False)
        a = torch.autograd.grad(loss, leaves + params, retain_graph=True)
        b = torch.autograd.grad(loss, leaves + params)
        torch.cuda.synchronize()
    assert _calls(NEW) - before == 2
    for (k, _), x, y in zip(_decoder_params(Rg).items(), a[len(leaves):], b[len(leaves):]):
        assert float(x.abs().max()) > 0
        assert torch.equal(x, y), f'{k}: two backward passes differ'


@pytest.mark.parametrize('form', list(FORMS))
def test_forward_with_trainable_decoder_is_bit_identical(gpu_device, form):
    case = CASES['s33_crossing_noise']
    sp, Rg, Rc, both, cam, jit, noise = _setup(form, case, 11)
    leaves, tex, geo = _gpu_planes(both, sp.plane_channels, case)
    with _arithmetic(FORMS[form][0]), _param_grad(True):
        with torch.no_grad():
            ref = _render_gpu(sp, Rg, tex, geo, cam, jit, noise, case)
        Rg.decoder.requires_grad_(True)
        before = _calls('render_rays')
        out = _render_gpu(sp, Rg, tex, geo, cam, jit, noise, case)
        assert _calls('render_rays') - before == 1
    assert all(o.grad_fn is not None for o in out)
    for a, b in zip(out, ref):
        assert torch.equal(a.detach(), b), 'forward with a trainable decoder differs from the no-grad forward'


def test_full_size_batch4(gpu_device):
    """The product's size: batch 4, 64 x 64 rays, 96 steps, 256 x 256 planes.  All ten gradients of the fused path against the step-wise GPU
    path (switch off) over all rays, and both paths against float64 CPU on the fixed subset of 256 rays per image of
    test_gpu_render_grad.py::test_full_size_batch4.  Bound GRAD_TOL; for a tensor on which the step-wise path's own error against float64
    exceeds 5e-5, twice that error (such tensors are listed in DESIGN.md section 5.12)."""
    case = dict(n=4, size=64, steps=96, noise=True, plane=(256, 256))
    sp, Rg, Rc, both, cam, jit, noise = _setup('c32_bf16x6', case, 21)
    Rg.decoder.requires_grad_(True); Rc.decoder.requires_grad_(True)
    n, C, size = 4, sp.plane_channels, 64
    P = _projections(n, sp.feature_channels + sp.seg_channels, size, 22)
    rays = torch.from_numpy(np.random.RandomState(23).choice(size * size, 256, replace=False)).sort().values
    mask = torch.zeros(size * size); mask[rays] = 1
    Pm = tuple(p * mask.reshape(1, 1, size, size) for p in P)
    full, sub = {}, {}
    for on in (True, False):
        with _param_grad(on):
            full[on], route = _gpu_grads(sp, Rg, both, C, cam, jit, noise, case, P, False)
            assert route[NEW] == (1 if on else 0) and route['render_rays_backward'] == 0, route
            sub[on], _ = _gpu_grads(sp, Rg, both, C, cam, jit, noise, case, Pm, False)
    Ps = tuple(p.reshape(n, p.shape[1], -1)[:, :, rays] for p in P)
    want, _ = _float64_grads(sp, Rc, both, C, cam, jit, noise, case, Ps, False, rays=rays)
    own = _compare('full size, 256 rays per image: step-wise GPU vs float64', sub[False], want, tol=float('inf'))
    bound = {k: (GRAD_TOL if e <= 5e-5 else 2 * e) for k, e in own.items()}
    print('[render-param-grad] full size bounds: ' + ', '.join(f'{k} {v:.2e}' for k, v in bound.items()))
    _compare('full size, 256 rays per image: fused vs float64', sub[True], want, tol=bound)
    _compare('full size: fused vs step-wise GPU', full[True], full[False], tol=bound)


def test_tuning_steps_match_the_step_wise_path(gpu_device):
    """Three plain-SGD steps of pivotal tuning on the tiny generator, every synthesis parameter trainable, `hip_param_grad` on: the switch on
    against off, step for step (outputs and every parameter's gradient within GRAD_TOL), with the new entry point run once per step.  SGD,
    not Adam: Adam turns a rounding-size difference in a near-zero gradient into a full-size update.  Each tensor's learning rate moves it
    by a fixed fraction of its max-abs in the first step: 2e-2 for the decoder's tensors (asserted >= 1e-3 at every step, so stale weights
    could not pass; the gradients shrink as the loss falls), 5e-4 for the others.  The
    switch-off path sums with atomics: a tensor whose off-against-off difference over two runs exceeds GRAD_TOL / 2 is bounded by twice
    that difference instead."""
    from training import networks, triplane
    torch.manual_seed(0)
    G0 = triplane.TriPlaneGenerator(triplane.tiny_spec()).eval().requires_grad_(False)
    with torch.no_grad():
        for p in G0.synthesis.renderer.decoder.parameters():
            if p.ndim == 1:
                p.copy_(torch.randn_like(p) * 0.2)
    g = np.random.RandomState(71)
    z = torch.from_numpy(g.randn(2, G0.z_dim)).float().to(gpu_device)
    c = torch.cat([triplane.camera_label(float(g.uniform(-0.4, 0.4))) for _ in range(2)]).float().to(gpu_device)
    jit = torch.from_numpy(g.rand(2, G0.synthesis.render_size ** 2, G0.spec.num_steps)).float().to(gpu_device)
    target = None
    old = networks.hip_param_grad
    networks.hip_param_grad = True

    def run(on, lrs=None, steps=3):
        nonlocal target
        G = copy.deepcopy(G0).to(gpu_device)
        with torch.no_grad():
            ws = G.mapping(z, c)
        params = dict(G.synthesis.named_parameters())
        for p in params.values():
            p.requires_grad_(True)
        hist = []
        with _param_grad(on):
            before = _calls(NEW)
            for _ in range(steps):
                for p in params.values():
                    p.grad = None
                img = G.synthesis(ws, c=c, noise_mode='const', force_fp32=True, ray_jitter=jit)
                if target is None:
                    target = torch.randn(img.shape, generator=torch.Generator().manual_seed(72)).to(gpu_device) * 0.5
                (img - target).square().mean().backward()
                grads = {k: p.grad.detach().clone() for k, p in params.items() if p.grad is not None}
                moved = {}
                if lrs is not None:
                    with torch.no_grad():
                        for k, p in params.items():
                            if k in grads:
                                moved[k] = float((lrs[k] * grads[k]).abs().max()) / max(float(p.abs().max()), 1e-30)
                                p.sub_(lrs[k] * grads[k])
                hist.append((img.detach().clone(), grads, moved))
            torch.cuda.synchronize()
            assert _calls(NEW) - before == (steps if on else 0)
        return hist

    try:
        probe = run(False, steps=1)[0][1]
        lrs = {}
        G_ref = dict(G0.synthesis.named_parameters())
        for k, gk in probe.items():
            gmax = float(gk.abs().max())
            lrs[k] = (2e-2 if '.decoder.' in k else 5e-4) * max(float(G_ref[k].abs().max()), 1e-2) / gmax if gmax > 0 else 0.0
        runs = {'on': run(True, lrs), 'off': run(False, lrs), 'off2': run(False, lrs)}
    finally:
        networks.hip_param_grad = old
    decoder = [k for k in probe if '.decoder.' in k]
    assert len(decoder) == 8, decoder
    for step in range(3):
        (y_on, g_on, moved), (y_off, g_off, _), (y_off2, g_off2, _) = (runs[k][step] for k in ('on', 'off', 'off2'))
        slow = {k: moved[k] for k in decoder if not moved[k] >= 1e-3}
        assert not slow, f'step {step}: decoder tensors that moved by less than 1e-3 of their max-abs: {slow}'
        noise_floor = {k: _err(g_off2[k], g_off[k]) for k in g_off}
        bound = {k: (GRAD_TOL if v <= GRAD_TOL / 2 else 2 * v) for k, v in noise_floor.items()}
        wide = {k: (noise_floor[k], bound[k]) for k in bound if bound[k] > GRAD_TOL}
        print(f'[render-param-grad] tuning step {step}: output err {_err(y_on, y_off):.2e}; tensors bounded by twice their off-against-off '
              f'difference (difference, bound): {wide}')
        assert _err(y_on, y_off) <= max(GRAD_TOL, 2 * _err(y_off2, y_off)), f'step {step}: output'
        assert set(g_on) == set(g_off)
        _compare(f'tuning step {step}', g_on, g_off, tol=bound)


def test_routing_with_the_switch_on(gpu_device):
    """A camera that requires grad, the hierarchical pass and a decoder width without a compiled form do not reach the new entry point,
    and still produce gradients for the decoder."""
    from training import triplane
    case = dict(n=2, size=8, steps=9)
    sp, Rg, Rc, both, cam, jit, noise = _setup('c32_fp32', case, 31)
    Rg.decoder.requires_grad_(True)
    C = sp.plane_channels
    P = _projections(2, sp.feature_channels + sp.seg_channels, 8, 32)

    def run(R, both_r, C_r, cam_d, **kw):
        leaves, tex, geo = _gpu_planes(both_r, C_r, case)
        params = list(R.decoder.parameters())
        before = _calls(NEW)
        feat, depth, wsum = R(tex, geo, cam_d, jitter=jit.cuda(), **kw)
        grads = torch.autograd.grad(_loss(feat, depth, wsum, P, False), leaves + params)
        torch.cuda.synchronize()
        assert all(g is not None and float(g.abs().max()) > 0 for g in grads), 'a gradient is missing'
        return _calls(NEW) - before

    with _param_grad(True):
        assert run(Rg, both, C, cam.cuda()) == 1                               # the fused path, for contrast
        assert run(Rg, both, C, cam.cuda().requires_grad_(True)) == 0, 'a camera that requires grad reached the parameter backward'
        assert run(Rg, both, C, cam.cuda(), hierarchical=True) == 0, 'the hierarchical pass reached the parameter backward'
        sp_odd = triplane.GeneratorSpec(plane_channels=24, decoder_hidden=40, render_size=8, num_steps=9)
        torch.manual_seed(33)
        R_odd = triplane.TriplaneRenderer(sp_odd).cuda()
        both_odd = torch.randn(2, 6 * 24, 32, 32, generator=torch.Generator().manual_seed(34)) * 0.7
        before = _calls('render_rays')
        assert run(R_odd, both_odd, 24, cam.cuda()) == 0, 'a (24, 40) decoder reached the parameter backward'
        assert _calls('render_rays') == before, 'a (24, 40) decoder has no fused forward'
    with _param_grad(False):
        assert run(Rg, both, C, cam.cuda()) == 0, 'fused_render_param_grad = False reached the parameter backward'
