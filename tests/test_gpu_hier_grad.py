"""Gradients of the hierarchical pass's merged march (`ide3d_render_rays_merged_backward`, ide-3d_amd/csrc/raymarch_bwd.hip, DESIGN.md
section 5.29) with respect to the tri-planes and the decoder, reached through `_RenderRaysMerged`, `render_triplane_hierarchical` and
`TriplaneRenderer.forward(hierarchical=True)` under `triplane.fused_hierarchical_grad`.  `pytest -m gpu`.

Reference: tests/hier_grad_ref.py, float64 CPU autograd through the step-wise definition with z_all / src / z_fine as constants.  Loss =
sum(feat * Pf) + sum(depth * Pd) + sum(wsum * Pw) with fixed random projections, or the feature term alone.  Bound: GRAD_TOL = 1e-4 of each
reference gradient's max-abs, the bound of tests/test_gpu_render_grad.py and test_gpu_render_param_grad.py for these quantities (the plane
gradients are summed by float atomics, so nothing here is compared bit for bit but the decoder gradients between two runs).  Every test
prints its error and, for the record, the error of the step-wise HIP path (sample_voxel + torch gather + fancy_integration with autograd)
against the same reference on the same inputs.

Scenes: those of tests/test_gpu_hier.py::_scene (3 images of 5 x 5 rays, planes [3, 3C, 32, 32], z_all / src / z_fine from the CPU
definitions, so they are fixed and well-formed: every row of src is a permutation of 0 .. T-1).
"""

import contextlib

import numpy as np
import pytest
import torch

import hier_grad_ref
import hier_ref
from oracle import ops as oracle_ops
from test_gpu_hier import FOV, SIZE, T0, T1, VARIANTS, _arithmetic, _cams, _renderer, _scene
from test_gpu_render_grad import GRAD_TOL, _err, _projections

pytestmark = pytest.mark.gpu

# kernel form -> (forward arithmetic, C): the backward is exact fp32 whatever the forward's MLPs ran in
FORMS = {'c32_bf16x6': ('bf16x6', 32), 'c32_fp32': ('fp32', 32), 'c16_default': ('default', 16)}
NEW = 'render_rays_merged_backward'
FOUR = ('render_ray_weights', 'sample_pdf', 'merge_depths', 'render_rays_merged')
BORDER = (40.0, 0.5, 5.0)               # fov, ray_start, ray_end of test_gpu_render_grad's s97_border: samples leave the planes


def _calls(name):
    from torch_utils import hip_plugin
    return hip_plugin.CALLS.get(name, 0)


@contextlib.contextmanager
def _switches(**values):
    """Set module switches of training.triplane for the block."""
    from training import triplane
    old = {k: getattr(triplane, k) for k in values}
    for k, v in values.items():
        setattr(triplane, k, v)
    try:
        yield
    finally:
        for k, v in old.items():
            setattr(triplane, k, v)


_gpu_renderers, _cpu_renderers, _refs = {}, {}, {}


def _renderers(sc, dev):
    """(frozen fp32 renderer on the GPU, float64 renderer on the CPU with a trainable decoder) with the scene's weights; own copies, so that the
    scenes' shared module is never touched."""
    from training import triplane
    spec = sc['R'].spec
    key = (spec.plane_channels, sc['clamp_mode'])
    if key not in _gpu_renderers:
        Rg = triplane.TriplaneRenderer(spec)
        Rg.load_state_dict({k[len('synthesis.renderer.'):]: v.detach().cpu() for k, v in sc['sd'].items()})
        _gpu_renderers[key] = Rg.to(dev).eval().requires_grad_(False)
        R64 = hier_grad_ref.renderer64(spec, sc['sd'])
        R64.decoder.requires_grad_(True)
        _cpu_renderers[key] = R64
    return _gpu_renderers[key], _cpu_renderers[key]


def _border_scene(C, S, variant):
    """The scene of `_scene` seen through the wide, long camera of s97_border: its own first pass, pdf draw and merge."""
    base = _scene(C, S, variant)
    fov, t0, t1 = BORDER
    w, z, bins, pw = hier_ref.ray_weights(base['sd'], base['tex'], base['geo'], base['cam'], fov, SIZE, S, t0, t1, jitter=base['jit'],
                                          sigma_noise=base['noise'], clamp_mode=base['clamp_mode'])
    z_fine = oracle_ops.sample_pdf(bins, pw, base['u'])
    z_all, src = hier_ref.merge(z_fine, z)
    return dict(base, z=z, z_fine=z_fine, z_all=z_all, src=src, merged=None)


def _planes(sc, dev, views=False, nchw=False):
    """-> (leaves that require grad, tex, geo) on the GPU"""
    both = torch.cat([sc['tex'], sc['geo']], 1)
    C3 = sc['tex'].shape[1]
    if views:
        leaf = both.to(dev).contiguous(memory_format=torch.channels_last).requires_grad_(True)
        return [leaf], leaf[:, :C3], leaf[:, C3:]
    fmt = torch.contiguous_format if nchw else torch.channels_last
    tex, geo = (x.to(dev).contiguous(memory_format=fmt).requires_grad_(True) for x in (sc['tex'], sc['geo']))
    return [tex, geo], tex, geo


def _const(sc, dev):
    d = lambda x: None if x is None else x.to(dev)
    return dict(cam=sc['cam'].to(dev), jit=d(sc['jit']), z_all=sc['z_all'].to(dev), src=sc['src'].to(dev), z_fine=sc['z_fine'].to(dev))


def _merged_outputs_gpu(Rg, sc, geom, tex, geo, dev):
    """Forward of the merged march through the autograd function -> (feat [n, ch, R], depth [n, R], wsum [n, R])."""
    from training import volumetric_rendering as vr
    vr._init()
    fov, t0, t1 = geom
    size, S = sc['size'], sc['S']
    rays_d, z_lin = vr._fused_ray_setup(dev, float(fov), (size, size), S, float(t0), float(t1))
    c = _const(sc, dev)
    mlp = Rg.decoder.kernel_weights()
    code = 0 if sc['clamp_mode'] == 'softplus' else 1
    return vr._RenderRaysMerged.apply(tex, geo, rays_d, z_lin, c['cam'], c['jit'], c['z_all'], c['src'], c['z_fine'], code, sc['white_back'],
                                      sc['max_depth'], *(mlp[k] for k in vr._MLP_KEYS))


def _stepwise_outputs_gpu(Rg, sc, geom, tex, geo, dev):
    """The step-wise HIP path on the same constants: two sample_voxel tensors, cat / gather by src, fancy_integration."""
    from training import volumetric_rendering as vr
    fov, t0, t1 = geom
    n, size, S = sc['n'], sc['size'], sc['S']
    rays = size * size
    c = _const(sc, dev)
    points, z_vals, d_cam = vr.get_initial_rays_trig(n, S, dev, fov, (size, size), t0, t1)
    pts, z_vals, rays_d, rays_o, _p, _y = vr.transform_sampled_points(
        points, z_vals, d_cam, dev, h_stddev=0, v_stddev=0, camera=c['cam'], mode=None,
        jitter=(c['jit'].unsqueeze(-1) if c['jit'] is not None else torch.full_like(z_vals, 0.5)))
    out = Rg.sample_voxel(tex, geo, pts.reshape(n, -1, 3), ray_grid=(size, size, S)).reshape(n, rays, S, -1)
    pts_fine = rays_o.unsqueeze(2) + rays_d.unsqueeze(2) * c['z_fine'].reshape(n, rays, S, 1)
    out_f = Rg.sample_voxel(tex, geo, pts_fine.reshape(n, -1, 3)).reshape(n, rays, S, -1)
    both = torch.gather(torch.cat([out_f, out], 2), 2, c['src'].reshape(n, rays, 2 * S, 1).long().expand(-1, -1, -1, out.shape[-1]))
    f, d, w = vr.fancy_integration(both, d_cam, c['z_all'].reshape(n, rays, 2 * S, 1), dev, noise_std=0, clamp_mode=sc['clamp_mode'],
                                   white_back=sc['white_back'], max_depth=sc['max_depth'])
    return f.permute(0, 2, 1), d[..., 0], w.sum(2)[..., 0]


def _decoder_params(R):
    return dict(R.decoder.named_parameters())


def _reference(key, R64, sc, geom, P, feat_only=False):
    """float64 gradients {tex_planes, geo_planes, the decoder's eight parameters} and the weight sums, computed once per key."""
    if key is not None and key in _refs:
        return _refs[key]
    fov, t0, t1 = geom
    C3 = sc['tex'].shape[1]
    both64 = torch.cat([sc['tex'], sc['geo']], 1).double().requires_grad_(True)
    out = hier_grad_ref.merged_outputs(R64, both64[:, :C3], both64[:, C3:], sc['cam'], fov, sc['size'], sc['S'], t0, t1, sc['jit'],
                                       sc['z_all'], sc['src'], sc['z_fine'], clamp_mode=sc['clamp_mode'], white_back=sc['white_back'],
                                       max_depth=sc['max_depth'])
    names = list(_decoder_params(R64))
    grads = torch.autograd.grad(hier_grad_ref.loss(*out, P, feat_only), [both64] + [_decoder_params(R64)[k] for k in names], allow_unused=True)
    want = {k: (g if g is not None else torch.zeros_like(_decoder_params(R64)[k])) for k, g in zip(names, grads[1:])}
    want['tex_planes'], want['geo_planes'] = grads[0][:, :C3], grads[0][:, C3:]
    res = (want, out[2].detach())
    if key is not None:
        _refs[key] = res
    return res


def _plane_grads(leaves, grads, C3):
    g = grads[0] if len(leaves) == 1 else torch.cat([grads[0], grads[1]], 1)
    return {'tex_planes': g[:, :C3], 'geo_planes': g[:, C3:]}


def _judge(tag, got, want, stepwise=None):
    """got / want / stepwise: {name: gradient}; every entry of `got` within GRAD_TOL of the reference's max-abs.  A reference gradient that is
    identically zero must be matched by exact zeros."""
    errs, old = {}, {}
    for k, g in got.items():
        w = want[k]
        if float(w.abs().max()) == 0.0:
            assert float(g.abs().max()) == 0.0, f'{tag}: {k} must be exactly zero'
            errs[k] = 0.0
        else:
            errs[k] = _err(g, w)
        if stepwise is not None and k in stepwise and float(w.abs().max()) > 0:
            old[k] = _err(stepwise[k], w)
    print(f'[hier-grad] {tag}: ' + ', '.join(f'{k} {v:.2e}' for k, v in errs.items())
          + (' | step-wise HIP path: ' + ', '.join(f'{k} {v:.2e}' for k, v in old.items()) if old else ''))
    bad = {k: v for k, v in errs.items() if not v <= GRAD_TOL}
    assert not bad, f'{tag}: errors of max-abs {bad} > {GRAD_TOL}'
    return errs


def _run_both_paths(Rg, sc, geom, dev, P, feat_only=False, views=False, with_decoder=False, planes=True):
    """One forward + backward through the merged march and one through the step-wise HIP path -> (fused {name: grad}, step-wise {name: grad},
    CALLS deltas of the fused run)."""
    C3 = sc['tex'].shape[1]
    names = list(_decoder_params(Rg)) if with_decoder else []
    res = []
    for outputs in (_merged_outputs_gpu, _stepwise_outputs_gpu):
        leaves, tex, geo = _planes(sc, dev, views=views)
        if not planes:
            leaves, tex, geo = [], tex.detach(), geo.detach()
        before = {k: _calls(k) for k in (NEW, 'render_rays_merged', 'triplane_sample_backward')}
        out = outputs(Rg, sc, geom, tex, geo, dev)
        grads = torch.autograd.grad(hier_grad_ref.loss(*out, P, feat_only), leaves + [_decoder_params(Rg)[k] for k in names])
        torch.cuda.synchronize()
        got = dict(zip(names, grads[len(leaves):]))
        if planes:
            got.update(_plane_grads(leaves, grads, C3))
        res += [got, {k: _calls(k) - before[k] for k in before}]
    return res[0], res[2], res[1]


def _assert_conditions(sc, S, variant):
    """What the inputs must be for the case to test what it is there for (all hold on these fixed scenes)."""
    T = 2 * S
    fine = sc['src'] < S                                                     # [rays, T]
    assert torch.equal(torch.sort(sc['src'].long(), dim=1)[0], torch.arange(T).expand(fine.shape[0], -1)), 'src rows are permutations'
    changes = (fine[:, 1:] != fine[:, :-1]).sum(1)
    assert int(changes.min()) >= 2, 'every ray changes between fine and coarse at least twice'
    if S >= 16:
        between = (~fine[:, 1:-1] & fine[:, :-2] & fine[:, 2:]).any(1)
        assert float(between.float().mean()) >= 0.95, 'a coarse sample between two fine ones on at least 95 % of the rays'
    if T > 64:
        for s in (63, 64):
            assert bool(fine[:, s].any()) and bool((~fine[:, s]).any()), f'both kinds at sample {s}'
    if VARIANTS[variant]['clamp_mode'] == 'relu':
        assert float(sc['merged'][2].min()) < 0.05, 'relu variant: a ray with weight sum < 0.05 (white_back / max_depth exercised)'


# ---- 4. plane gradients against float64 -------------------------------------------------------------------------

@pytest.mark.parametrize('variant', list(VARIANTS))
@pytest.mark.parametrize('S', (3, 16, 17, 32, 33, 48))
@pytest.mark.parametrize('form', list(FORMS))
def test_plane_gradients_vs_float64(gpu_device, form, S, variant):
    """T = 6, 32, 34, 64, 66, 96: the smallest count, under one 64-sample chunk, exactly one chunk, two samples into the second chunk, one and
    a half chunks."""
    arith, C = FORMS[form]
    sc = _scene(C, S, variant)
    _assert_conditions(sc, S, variant)
    dev = gpu_device
    Rg, R64 = _renderers(sc, dev)
    geom = (FOV, T0, T1)
    P = _projections(sc['n'], sc['merged'][0].shape[1], SIZE, 1000 + S)
    with _arithmetic(arith):
        got, old, route = _run_both_paths(Rg, sc, geom, dev, P)
    assert route == {NEW: 1, 'render_rays_merged': 1, 'triplane_sample_backward': 0}, route
    want, _ = _reference((C, S, variant), R64, sc, geom, P)
    assert float(want['tex_planes'].abs().max()) > 0 and float(want['geo_planes'].abs().max()) > 0
    _judge(f'{form} S={S} {variant}', got, want, old)


# ---- 5. special rows ---------------------------------------------------------------------------------------------

def _capture_merged(monkeypatch):
    """Record (z_all, src, z_fine) of every `render_rays_merged` call."""
    from training import volumetric_rendering as vr
    vr._init()
    seen = []
    real = vr._plugin.render_rays_merged

    def spy(*args, **kwargs):
        seen.append(tuple(x.detach().cpu() for x in args[10:13]))
        return real(*args, **kwargs)

    monkeypatch.setattr(vr._plugin, 'render_rays_merged', staticmethod(spy))
    return seen


@pytest.mark.parametrize('row', ['ties', 'linspace', 'zero_density', 'border', 'channel_views', 'nchw', 'feat_only'])
@pytest.mark.parametrize('C', (32, 16))
def test_special_rows(gpu_device, monkeypatch, C, row):
    from torch_utils import hip_plugin
    from training import volumetric_rendering as vr
    dev = gpu_device
    S = 17 if row == 'border' else 16
    variant = 'nojitter_relu' if row == 'zero_density' else 'jitter_noise_softplus'
    geom = BORDER if row == 'border' else (FOV, T0, T1)
    sc = _border_scene(C, S, variant) if row == 'border' else dict(_scene(C, S, variant))
    rays = sc['n'] * SIZE * SIZE
    if row == 'ties':
        # every third fine depth is set bit-equal to a coarse depth of its ray: delta = 0 there, and the stable order puts the fine one first
        z_fine = sc['z_fine'].clone()
        z_fine[:, ::3] = sc['z'][:, ::3]
        z_all, src = hier_ref.merge(z_fine, sc['z'])
        assert int((z_all[:, 1:] == z_all[:, :-1]).sum()) >= rays * 5
        sc.update(z_fine=z_fine, z_all=z_all, src=src)
    elif row == 'linspace':
        z_fine = oracle_ops.sample_pdf(sc['bins'], sc['pw'], torch.linspace(0, 1, S).expand(rays, S).contiguous())
        z_all, src = hier_ref.merge(z_fine, sc['z'])
        sc.update(z_fine=z_fine, z_all=z_all, src=src)
    Rg, R64 = _renderers(sc, dev)
    if row == 'zero_density':
        # the last image's geometry planes hold one feature vector whose density pre-activation is negative: every sample of its rays has
        # density 0 under relu (weights 0, the outputs are the background's)
        cand = torch.randn(256, C, generator=torch.Generator().manual_seed(9)).double()
        with torch.no_grad():
            sigma = R64.decoder(torch.zeros(256, C).double(), cand)[:, -1]
        v = cand[int(sigma.argmin())].float()
        assert float(sigma.min()) < -0.1
        geo = sc['geo'].clone()
        geo[-1] = (v / 3).repeat(3)[:, None, None]
        sc.update(geo=geo)
    nch = Rg.spec.feature_channels + Rg.spec.seg_channels
    P = _projections(sc['n'], nch, SIZE, 2000 + C)
    feat_only = row == 'feat_only'
    with _arithmetic('default'):
        if row == 'nchw':
            # through the wrapper, which converts the planes; its own first pass, pdf draw and merge are recorded for the reference
            seen = _capture_merged(monkeypatch)
            leaves, tex, geo = _planes(sc, dev, nchw=True)
            assert tex.stride(1) != 1
            c = _const(sc, dev)
            before = _calls(NEW)
            out = vr.render_triplane_hierarchical(tex, geo, Rg.decoder.kernel_weights(), c['cam'], FOV, (SIZE, SIZE), S, T0, T1, jitter=c['jit'],
                                                  sigma_noise=sc['noise'].to(dev), importance_u=sc['u'].to(dev), clamp_mode=sc['clamp_mode'])
            grads = torch.autograd.grad(hier_grad_ref.loss(*out, P), leaves)
            torch.cuda.synchronize()
            assert _calls(NEW) - before == 1 and len(seen) == 1
            got = _plane_grads(leaves, grads, 3 * C)
            sc.update(zip(('z_all', 'src', 'z_fine'), seen[0]))
            _l, tex2, geo2 = _planes(sc, dev)
            o2 = _stepwise_outputs_gpu(Rg, sc, geom, tex2, geo2, dev)
            old = _plane_grads(_l, torch.autograd.grad(hier_grad_ref.loss(*o2, P), _l), 3 * C)
        else:
            got, old, route = _run_both_paths(Rg, sc, geom, dev, P, feat_only=feat_only, views=(row == 'channel_views'))
            assert route == {NEW: 1, 'render_rays_merged': 1, 'triplane_sample_backward': 0}, route
        if feat_only:
            # dL/ddepth and dL/dwsum as NULL pointers, at the binding
            rays_d, z_lin = vr._fused_ray_setup(dev, FOV, (SIZE, SIZE), S, T0, T1)
            c = _const(sc, dev)
            _l, tex, geo = _planes(sc, dev)
            with torch.no_grad():
                res = hip_plugin.VolumeRenderPlugin.render_rays_merged_backward(
                    rays_d, z_lin, c['cam'], c['jit'], tex.detach(), geo.detach(), Rg.decoder.kernel_weights(), 0, sc['white_back'],
                    sc['max_depth'], c['z_all'], c['src'], c['z_fine'], P[0].reshape(sc['n'], nch, -1).to(dev), None, None)
            assert res is not None and res[2] is None
            got = dict(got, tex_planes_null_grads=res[0], geo_planes_null_grads=res[1])
    want, w64 = _reference(None, R64, sc, geom, P, feat_only)
    if row == 'zero_density':
        assert float(w64[-1].abs().max()) == 0.0, 'the last image\'s rays must have zero weight everywhere'
        assert float(want['geo_planes'][-1].abs().max()) == 0.0 and float(want['tex_planes'][-1].abs().max()) == 0.0
        assert float(got['geo_planes'][-1].abs().max()) == 0.0 and float(got['tex_planes'][-1].abs().max()) == 0.0
    if row == 'border':
        # samples outside the planes: the float64 gather gives them zeros padding, and rays that see nothing must exist on both sides
        assert float(want['tex_planes'].abs().max()) > 0
    if feat_only:
        want = dict(want, tex_planes_null_grads=want['tex_planes'], geo_planes_null_grads=want['geo_planes'])
    _judge(f'C={C} {row}', got, want, old)


# ---- 6. decoder gradients ----------------------------------------------------------------------------------------

@pytest.mark.parametrize('planes', [True, False], ids=['planes_and_decoder', 'decoder_only'])
@pytest.mark.parametrize('variant', list(VARIANTS))
@pytest.mark.parametrize('S', (17, 33))
@pytest.mark.parametrize('form', ['c32_fp32', 'c16_default'])
def test_decoder_gradients_vs_float64(gpu_device, form, S, variant, planes):
    """The eight decoder tensors (gradients of the module's own weight and bias: the gain chain is covered), beside the planes' or alone
    (plane pointers NULL); two backward passes give bit-equal decoder gradients."""
    from torch_utils import hip_plugin
    from training import volumetric_rendering as vr
    arith, C = FORMS[form]
    sc = _scene(C, S, variant)
    dev = gpu_device
    Rg, R64 = _renderers(sc, dev)
    geom = (FOV, T0, T1)
    P = _projections(sc['n'], sc['merged'][0].shape[1], SIZE, 1000 + S)
    Rg.decoder.requires_grad_(True)
    try:
        with _arithmetic(arith):
            got, old, route = _run_both_paths(Rg, sc, geom, dev, P, with_decoder=True, planes=planes)
            assert route == {NEW: 1, 'render_rays_merged': 1, 'triplane_sample_backward': 0}, route
            # two backward passes of one graph
            leaves, tex, geo = _planes(sc, dev)
            params = list(_decoder_params(Rg).values())
            out = _merged_outputs_gpu(Rg, sc, geom, tex if planes else tex.detach(), geo if planes else geo.detach(), dev)
            loss = hier_grad_ref.loss(*out, P)
            a = torch.autograd.grad(loss, params, retain_graph=True)
            b = torch.autograd.grad(loss, params)
            for (k, _p), x, y in zip(_decoder_params(Rg).items(), a, b):
                assert float(x.abs().max()) > 0 and torch.equal(x, y), f'{k}: two backward passes differ'
            if not planes:
                rays_d, z_lin = vr._fused_ray_setup(dev, FOV, (SIZE, SIZE), S, T0, T1)
                c = _const(sc, dev)
                with torch.no_grad():
                    mlp = Rg.decoder.kernel_weights()
                    res = hip_plugin.VolumeRenderPlugin.render_rays_merged_backward(
                        rays_d, z_lin, c['cam'], c['jit'], tex.detach(), geo.detach(), mlp, 0 if sc['clamp_mode'] == 'softplus' else 1,
                        sc['white_back'], sc['max_depth'], c['z_all'], c['src'], c['z_fine'], *(p.reshape(o.shape).to(dev) for p, o in zip(P, out)),
                        plane_grads=False, param_grads=True)
                assert res[0] is None and res[1] is None, 'a plane gradient buffer was allocated'
                assert sorted(res[2]) == sorted(mlp) and all(res[2][k].shape == mlp[k].shape for k in mlp)
    finally:
        Rg.decoder.requires_grad_(False)
    want, _ = _reference((C, S, variant), R64, sc, geom, P)
    assert len(got) == (10 if planes else 8)
    _judge(f'{form} S={S} {variant} {"planes + decoder" if planes else "decoder only"}', got, want, old)


# ---- 7. through TriplaneRenderer.forward ---------------------------------------------------------------------------

@pytest.mark.parametrize('form,with_decoder', [('c32_bf16x6', False), ('c16_default', False), ('c32_fp32', True)])
def test_through_the_renderer(gpu_device, form, with_decoder):
    """`fused_hierarchical_grad` on: one launch each of the four and of the backward, none of the step-wise ops; forward values bit-equal to
    the no-grad `fused_hierarchical` forward; gradients within GRAD_TOL of the same launches composed by hand through the binding.  The
    step-wise path (switch off) draws its own z_fine from slightly different weights: printed for the record, no gate."""
    from torch_utils import hip_plugin
    from training import volumetric_rendering as vr
    Pl = hip_plugin.VolumeRenderPlugin
    arith, C = FORMS[form]
    S, variant = 17, 'jitter_noise_softplus'
    sc = _scene(C, S, variant)
    dev = gpu_device
    Rg, _R64 = _renderers(sc, dev)
    c = _const(sc, dev)
    noise, u = sc['noise'].to(dev), sc['u'].to(dev)
    P = _projections(sc['n'], sc['merged'][0].shape[1], SIZE, 3000)
    kw = dict(num_steps=S, jitter=c['jit'], sigma_noise=noise, hierarchical=True, importance_u=u, white_back=True)
    names = list(_decoder_params(Rg)) if with_decoder else []
    Rg.decoder.requires_grad_(with_decoder)
    try:
        with _arithmetic(arith), _switches(fused_render_param_grad=with_decoder):
            def run():
                leaves, tex, geo = _planes(sc, dev)
                out = Rg(tex, geo, c['cam'], **kw)
                grads = torch.autograd.grad(hier_grad_ref.loss(*out, P), leaves + [_decoder_params(Rg)[k] for k in names])
                torch.cuda.synchronize()
                return out, dict(_plane_grads(leaves, grads, 3 * C), **dict(zip(names, grads[2:])))

            with _switches(fused_hierarchical_grad=True):
                hip_plugin.CALLS.clear()
                out, got = run()
                calls = dict(hip_plugin.CALLS)
            assert {k: calls.get(k, 0) for k in FOUR + (NEW, 'composite', 'sample_voxel', 'triplane_sample_backward')} == \
                dict({k: 1 for k in FOUR + (NEW,)}, composite=0, sample_voxel=0, triplane_sample_backward=0), calls
            assert all(o.grad_fn is not None for o in out)
            # the no-grad fused forward
            with torch.no_grad(), _switches(fused_hierarchical=True):
                _l, tex, geo = _planes(sc, dev)
                hip_plugin.CALLS.clear()
                ref = Rg(tex.detach(), geo.detach(), c['cam'], **kw)
                assert hip_plugin.CALLS.get('render_rays_merged') == 1 and not hip_plugin.CALLS.get('sample_voxel')
            for x, y in zip(out, ref):
                assert torch.equal(x.detach(), y), 'forward under grad differs from the no-grad fused forward'
            # the same launches by hand
            leaves, tex, geo = _planes(sc, dev)
            rays_d, z_lin = vr._fused_ray_setup(dev, FOV, (SIZE, SIZE), S, T0, T1)
            mlp = Rg.decoder.kernel_weights()
            with torch.no_grad():
                _w, z_vals, bins, pw = Pl.render_ray_weights(rays_d, z_lin, c['cam'], c['jit'], noise, tex, geo, mlp, 0,
                                                             want=('z_vals', 'pdf_bins', 'pdf_weights'))
                z_fine = Pl.sample_pdf(bins, pw, u)
                z_all, src = Pl.merge_depths(z_fine, z_vals)
            hand = vr._RenderRaysMerged.apply(tex, geo, rays_d, z_lin, c['cam'], c['jit'], z_all, src, z_fine, 0, True, None,
                                              *(mlp[k] for k in vr._MLP_KEYS))
            for x, y in zip(out, hand):
                assert torch.equal(x.detach().reshape(y.shape), y.detach())
            grads = torch.autograd.grad(hier_grad_ref.loss(*hand, P), leaves + [_decoder_params(Rg)[k] for k in names])
            want = dict(_plane_grads(leaves, grads, 3 * C), **dict(zip(names, grads[2:])))
            with _switches(fused_hierarchical_grad=False):
                hip_plugin.CALLS.clear()
                _o, old = run()
                assert not hip_plugin.CALLS.get(NEW) and not hip_plugin.CALLS.get('render_rays_merged')
    finally:
        Rg.decoder.requires_grad_(False)
    _judge(f'{form} through the renderer{" with the decoder" if with_decoder else ""} (reference: the launches by hand; the record column is '
           f'the step-wise path with its own z_fine)', got, want, old)


# ---- 8. real layout ---------------------------------------------------------------------------------------------

def test_real_layout_batch2(gpu_device, monkeypatch):
    """Batch 2, 64 x 64 rays, 256 x 256 planes, C = 32, S = 48 (T = 96), bf16x6 forward, through the renderer; against float64 on a fixed
    subset of 256 rays per image (the loss restricted to them on both sides, as tests/test_gpu_render_grad.py::test_full_size_batch4 does)
    with the z_all / src / z_fine the pass itself produced."""
    n, size, S, C, plane = 2, 64, 48, 32, 256
    dev = gpu_device
    tex = torch.randn(n, 3 * C, plane, plane, generator=torch.Generator().manual_seed(C)) * 0.7
    geo = torch.randn(n, 3 * C, plane, plane, generator=torch.Generator().manual_seed(C + 1)) * 0.7
    R, sd = _renderer(32, 'softplus', tex, geo)
    g = torch.Generator().manual_seed(77)
    sc = dict(R=R, sd=sd, tex=tex, geo=geo, cam=_cams(n), jit=torch.rand(n, size * size, S, generator=g), clamp_mode='softplus',
              white_back=False, max_depth=None, size=size, S=S, n=n)
    noise = torch.randn(n, size * size, S, generator=g) * 0.5
    u = torch.rand(n * size * size, S, generator=g)
    Rg, R64 = _renderers(sc, dev)
    nch = Rg.spec.feature_channels + Rg.spec.seg_channels
    P = _projections(n, nch, size, 78)
    rays = torch.from_numpy(np.random.RandomState(23).choice(size * size, 256, replace=False)).sort().values
    mask = torch.zeros(size * size); mask[rays] = 1
    Pm = tuple(p * mask.reshape(1, 1, size, size) for p in P)
    seen = _capture_merged(monkeypatch)
    leaves, tx, gx = _planes(sc, dev)
    with _arithmetic('bf16x6'), _switches(fused_hierarchical_grad=True):
        before = {k: _calls(k) for k in FOUR + (NEW, 'sample_voxel')}
        out = Rg(tx, gx, sc['cam'].to(dev), img_size=size, num_steps=S, jitter=sc['jit'].to(dev), sigma_noise=noise.to(dev), hierarchical=True,
                 importance_u=u.to(dev))
        grads = torch.autograd.grad(hier_grad_ref.loss(*out, Pm), leaves)
        torch.cuda.synchronize()
    assert {k: _calls(k) - before[k] for k in before} == dict({k: 1 for k in FOUR + (NEW,)}, sample_voxel=0)
    sc.update(zip(('z_all', 'src', 'z_fine'), seen[0]))
    both64 = torch.cat([tex, geo], 1).double().requires_grad_(True)
    o64 = hier_grad_ref.merged_outputs(R64, both64[:, :3 * C], both64[:, 3 * C:], sc['cam'], FOV, size, S, T0, T1, sc['jit'], sc['z_all'],
                                       sc['src'], sc['z_fine'], rays=rays)
    Ps = tuple(p.reshape(n, p.shape[1], -1)[:, :, rays] for p in P)
    (want,) = torch.autograd.grad(hier_grad_ref.loss(*o64, Ps), [both64])
    # the step-wise HIP path on the same constants and the same restricted loss, for the record
    _l, tx2, gx2 = _planes(sc, dev)
    o2 = _stepwise_outputs_gpu(Rg, sc, (FOV, T0, T1), tx2, gx2, dev)
    old = _plane_grads(_l, torch.autograd.grad(hier_grad_ref.loss(*o2, Pm), _l), 3 * C)
    _judge('real layout, batch 2, 256 rays per image', _plane_grads(leaves, grads, 3 * C),
           {'tex_planes': want[:, :3 * C], 'geo_planes': want[:, 3 * C:]}, old)


# ---- 9. declines ---------------------------------------------------------------------------------------------------

def test_declines(gpu_device):
    """A (C, hidden) pair without a compiled form: the library answers None and the call is the step-wise one, switch on == switch off.  A
    step count the pass does not take (its per-ray state is sized by T = 2 * steps): the binding returns None with an error text, nothing
    launched."""
    from torch_utils import hip_plugin
    from training import triplane
    from training import volumetric_rendering as vr
    dev = gpu_device
    sp = triplane.GeneratorSpec(plane_channels=8, decoder_hidden=16, feature_channels=4, seg_channels=2, render_size=SIZE, num_steps=12)
    torch.manual_seed(5)
    R = triplane.TriplaneRenderer(sp).to(dev).eval().requires_grad_(False)
    g = torch.Generator().manual_seed(6)
    planes = [(torch.randn(2, 24, 32, 32, generator=g) * 0.7).to(dev) for _ in range(2)]
    kw = dict(jitter=torch.rand(2, 25, 12, generator=g).to(dev), hierarchical=True, importance_u=torch.rand(50, 12, generator=g).to(dev))
    P = _projections(2, 6, SIZE, 7)
    res, calls, grads = [], [], []
    for on in (False, True):
        with _switches(fused_hierarchical_grad=on):
            tex, geo = (x.clone().requires_grad_(True) for x in planes)
            hip_plugin.CALLS.clear()
            out = R(tex, geo, _cams(2).to(dev), **kw)
            grads.append(torch.autograd.grad(hier_grad_ref.loss(*out, P), [tex, geo]))
            torch.cuda.synchronize()
            res.append(out); calls.append(dict(hip_plugin.CALLS))
    assert calls[0] == calls[1] and calls[1].get('sample_voxel', 0) == 0 and NEW not in calls[1] and 'render_rays_merged' not in calls[1], calls
    for x, y in zip(*res):
        assert torch.equal(x, y)
    for x, y in zip(*grads):
        assert _err(x, y) <= GRAD_TOL                 # the step-wise gather backward sums with atomics too
    # a step count outside the pass's range, at the binding, with four rays
    S = 1100
    sc = _scene(16, 16, 'jitter_noise_softplus')
    Rg, _R64 = _renderers(sc, dev)
    rays_d, z_lin = vr._fused_ray_setup(dev, FOV, (2, 2), S, T0, T1)
    tex, geo = (x[:1].to(dev).contiguous(memory_format=torch.channels_last) for x in (sc['tex'], sc['geo']))
    z_fine = torch.full((4, S), 2.5, device=dev)
    z_all, src = torch.full((4, 2 * S), 2.5, device=dev), torch.arange(2 * S, dtype=torch.int32, device=dev).repeat(4, 1)
    hip_plugin.CALLS.clear()
    with torch.no_grad():
        got = hip_plugin.VolumeRenderPlugin.render_rays_merged_backward(
            rays_d, z_lin, sc['cam'][:1].to(dev), None, tex, geo, Rg.decoder.kernel_weights(), 0, False, None, z_all, src, z_fine,
            torch.zeros(1, 13, 4, device=dev), None, None)
    assert got is None and not hip_plugin.CALLS
    text = hip_plugin.load().ide3d_last_error().decode()
    assert 'render_rays_merged_backward' in text and str(S) in text, text
