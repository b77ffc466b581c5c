"""The hierarchical pass as four HIP launches (`ide3d_render_ray_weights` -> `ide3d_sample_pdf` -> `ide3d_merge_depths` ->
`ide3d_render_rays_merged`) on the GPU: each new launch against its float64 definition (tests/hier_ref.py), and the
pass end to end under `triplane.fused_hierarchical` against the oracle and against the step-wise path it replaces.  `pytest -m gpu`.

Tolerances.  Every compared quantity is measured twice against the same float64 reference, on the same inputs, in the same test: the
step-wise HIP path (sample_voxel / composite / sample_pdf kernels + torch sort and gather) and the new launches.  The new path may exceed
the step-wise error by at most 2 x (the fused kernel sums in another order: output layers on the per-ray sums; fast softplus), and must
stay inside the bounds the project accepts for this pass (tests/test_gpu_render.py::test_hierarchical_pass_gpu), relative to the
reference's scale: features 3e-4, depth 1e-4 with the tiny network (C = 16, hidden 32); features 5e-4, depth 2e-4, weight sum 2e-4 with
the full-width one (C = 32, hidden 64).  Per-sample weights lie in [0, 1] like their sum and take the weight sum's bound.

Small scene: planes [3, 3C, 32, 32] ~ N(0, 0.7), random decoder biases, 3 images of 5 x 5 rays (75 rays: no multiple of 4 or 8 waves,
image boundaries inside a workgroup's range), S in {3, 12, 16, 17, 48}: the smallest legal count, under a tile, one tile, one over, and
T = 2 S = 96.
"""

import contextlib

import pytest
import torch

import hier_ref
from oracle import generator as ogen
from oracle import ops as oracle_ops
from oracle import spec as ospec
from util import t

pytestmark = pytest.mark.gpu

TINY = dict(plane_channels=16, decoder_hidden=32, feature_channels=8, seg_channels=5)
# kernel form -> (arithmetic, network widths): both arithmetics on both compiled (C, hidden) pairs (C = 16 has the fp32 MLP in either)
FORMS = {'c32_bf16x6': ('bf16x6', {}), 'c32_fp32': ('fp32', {}), 'c16_default': ('default', TINY), 'c16_fp32': ('fp32', TINY)}
STEPS = (3, 12, 16, 17, 48)
# (features, depth, weight sum | None) of scale, by network width
BOUNDS = {16: (3e-4, 1e-4, None), 32: (5e-4, 2e-4, 2e-4)}
FOV, T0, T1, SIZE, N = 18.0, 2.25, 3.3, 5, 3
# first-pass variants: jitter and density noise given, softplus | no jitter, relu on densities centred at 0 (weight sums < 1: white_back and
# max_depth matter in the merged march)
VARIANTS = {'jitter_noise_softplus': dict(jitter=True, noise=True, clamp_mode='softplus'),
            'nojitter_relu': dict(jitter=False, noise=False, clamp_mode='relu')}


def _calls():
    from torch_utils import hip_plugin
    return dict(hip_plugin.CALLS)


@contextlib.contextmanager
def _arithmetic(name):
    from torch_utils import hip_plugin
    try:
        hip_plugin.conv_arithmetic(name)
        yield
    finally:
        hip_plugin.conv_arithmetic('default')


@contextlib.contextmanager
def _switch(on):
    from training import triplane
    old = triplane.fused_hierarchical
    triplane.fused_hierarchical = on
    try:
        yield
    finally:
        triplane.fused_hierarchical = old


def _err(actual, expected):
    a = actual.detach().cpu().double(); e = torch.as_tensor(expected).detach().cpu().double()
    assert a.shape == e.shape, f'shape {tuple(a.shape)} != {tuple(e.shape)}'
    return float((a - e).abs().max()) / (float(e.abs().max()) + 1e-12)


def _judge(what, new, old, bound):
    """`new` / `old`: errors of the new launches / the step-wise path against the same reference, relative to its scale."""
    print(f'{what}: new {new:.3e}  step-wise {old:.3e}  bound {bound}')
    assert new <= 2 * old, f'{what}: error {new:.3e} of scale > 2 x the step-wise path\'s {old:.3e}'
    if bound is not None:
        assert new <= bound, f'{what}: error {new:.3e} of scale > {bound}'


def _cams(n):
    from training import triplane
    two = [triplane.camera_label(0.4), triplane.camera_label(-0.3, pitch=1.4)]
    return torch.cat([two[i % 2] for i in range(n)])[:, :16].reshape(n, 4, 4)


_renderers, _scenes = {}, {}


def _renderer(widths_key, clamp_mode, tex_c, geo_c):
    """One decoder per (network widths, clamp mode), on the CPU; relu: densities of the volume centred at 0."""
    from training import triplane
    key = (widths_key, clamp_mode)
    if key not in _renderers:
        widths = TINY if widths_key == 16 else {}
        sp = triplane.GeneratorSpec(**widths, render_size=SIZE, fov=FOV, ray_start=T0, ray_end=T1, clamp_mode=clamp_mode)
        torch.manual_seed(11 + widths_key)
        R = triplane.TriplaneRenderer(sp).eval()
        with torch.no_grad():
            for p in R.parameters():
                if p.ndim == 1:
                    p.copy_(torch.randn_like(p) * 0.2)
        if clamp_mode == 'relu':
            sd = {'synthesis.renderer.' + k: v.detach() for k, v in R.state_dict().items()}
            probe = torch.rand(1, 4096, 3, generator=torch.Generator().manual_seed(3)) - 0.5
            sig = ogen.sample_voxel(sd, None, tex_c[:1], geo_c[:1], probe)[:, -1]
            with torch.no_grad():
                R.decoder.geo1.bias[0] -= float(sig.median()) / R.decoder.geo1.bias_gain
        sd = {'synthesis.renderer.' + k: v.detach().clone() for k, v in R.state_dict().items()}
        _renderers[key] = (R, sd)
    return _renderers[key]


def _scene(C, S, variant, plane=32, size=SIZE, n=N):
    """Inputs and float64 references of one case, computed once and shared by the arithmetics (never modified)."""
    key = (C, S, variant, plane, size, n)
    if key in _scenes:
        return _scenes[key]
    v = VARIANTS[variant]
    g = torch.Generator().manual_seed(100 * C + S)
    tex = torch.randn(n, 3 * C, plane, plane, generator=torch.Generator().manual_seed(C)) * 0.7
    geo = torch.randn(n, 3 * C, plane, plane, generator=torch.Generator().manual_seed(C + 1)) * 0.7
    R, sd = _renderer(C, v['clamp_mode'], tex, geo)
    rays = size * size
    cam = _cams(n)
    jit = torch.rand(n, rays, S, generator=g) if v['jitter'] else None
    noise = torch.randn(n, rays, S, generator=g) * 0.5 if v['noise'] else None
    u = torch.rand(n * rays, S, generator=g)
    geom = (FOV, size, S, T0, T1)
    w, z, bins, pw = hier_ref.ray_weights(sd, tex, geo, cam, *geom, jitter=jit, sigma_noise=noise, clamp_mode=v['clamp_mode'])
    z_fine = oracle_ops.sample_pdf(bins, pw, u)
    z_all, src = hier_ref.merge(z_fine, z)
    wb, md = (True, 3.75) if v['clamp_mode'] == 'relu' else (False, None)
    merged = hier_ref.render_merged(sd, tex, geo, cam, *geom, jit, z_all, src, z_fine, clamp_mode=v['clamp_mode'], white_back=wb, max_depth=md)
    _scenes[key] = dict(R=R, sd=sd, tex=tex, geo=geo, cam=cam, jit=jit, noise=noise, u=u, w=w, z=z, bins=bins, pw=pw, z_fine=z_fine,
                        z_all=z_all, src=src, merged=merged, white_back=wb, max_depth=md, clamp_mode=v['clamp_mode'], size=size, S=S, n=n)
    return _scenes[key]


def _device_inputs(sc, dev):
    from training import volumetric_rendering as vr
    vr._init()
    R = sc['R'].to(dev)
    tex, geo = (x.to(dev).contiguous(memory_format=torch.channels_last) for x in (sc['tex'], sc['geo']))
    rays_d, z_lin = vr._fused_ray_setup(dev, FOV, (sc['size'], sc['size']), sc['S'], T0, T1)
    d = lambda x: None if x is None else x.to(dev)
    return R, tex, geo, rays_d, z_lin, sc['cam'].to(dev), d(sc['jit']), d(sc['noise'])


def _stepwise_samples(R, tex, geo, cam, jit, sc, dev):
    """The step-wise path's first half on the GPU: coarse sample rows [n, R, S, ch+1], depths, camera-space directions, world origins / directions."""
    from training import volumetric_rendering as vr
    n, size, S = sc['n'], sc['size'], sc['S']
    points, z_vals, d_cam = vr.get_initial_rays_trig(n, S, dev, FOV, (size, size), T0, T1)
    pts, z_vals, rays_d, rays_o, _p, _y = vr.transform_sampled_points(
        points, z_vals, d_cam, dev, h_stddev=0, v_stddev=0, camera=cam, mode=None,
        jitter=(jit.unsqueeze(-1) if jit is not None else torch.full_like(z_vals, 0.5)))
    out = R.sample_voxel(tex, geo, pts.reshape(n, -1, 3)).reshape(n, size * size, S, -1)
    return out, z_vals, d_cam, rays_o, rays_d


@pytest.mark.parametrize('variant', list(VARIANTS))
@pytest.mark.parametrize('S', STEPS)
@pytest.mark.parametrize('form', list(FORMS))
def test_each_launch_vs_float64(gpu_device, form, S, variant):
    """render_ray_weights, merge_depths and render_rays_merged, one at a time, each fed from the float64 definitions' own intermediates."""
    from torch_utils import hip_plugin
    from training import volumetric_rendering as vr
    P = hip_plugin.VolumeRenderPlugin
    arith, widths = FORMS[form]
    C = widths.get('plane_channels', 32)
    fb, db, wb_ = BOUNDS[C]
    sc = _scene(C, S, variant)
    dev = gpu_device
    R, tex, geo, rays_d, z_lin, cam, jit, noise = _device_inputs(sc, dev)
    n, rays = sc['n'], sc['size'] ** 2
    code = 0 if sc['clamp_mode'] == 'softplus' else 1
    with _arithmetic(arith), torch.no_grad():
        mlp = R.decoder.kernel_weights()
        # ---- first pass ----
        first = P.render_ray_weights(rays_d, z_lin, cam, jit, noise, tex, geo, mlp, code)
        assert first is not None, hip_plugin.load().ide3d_last_error()
        w, z, bins, pw = first
        zl = z_lin.cpu()
        z_expr = zl.expand(n * rays, S) if sc['jit'] is None else zl + (sc['jit'].reshape(n * rays, S) - 0.5) * (zl[1] - zl[0])
        assert torch.equal(z.cpu(), z_expr.contiguous()), 'z_vals: ray_sample_depth, bit for bit'
        assert torch.equal(bins.cpu(), 0.5 * (z_expr[:, :-1] + z_expr[:, 1:])), 'pdf_bins: one rounding per operation'
        assert torch.equal(pw, w[:, 1:-1] + 1e-5), 'pdf_weights = weights[1:-1] + 1e-5 exactly'
        only = P.render_ray_weights(rays_d, z_lin, cam, jit, noise, tex, geo, mlp, code, want=('pdf_bins',))
        assert only[0] is None and only[1] is None and only[3] is None and torch.equal(only[2], bins), 'NULL outputs are skipped'
        only = P.render_ray_weights(rays_d, z_lin, cam, jit, noise, tex, geo, mlp, code, want=('weights', 'pdf_weights'))
        assert only[1] is None and only[2] is None and torch.equal(only[0], w) and torch.equal(only[3], pw)
        out, z_sw, d_cam, rays_o, rays_dw = _stepwise_samples(R, tex, geo, cam, jit, sc, dev)
        _f, _d, w_sw = vr.fancy_integration(out, d_cam, z_sw, dev, noise_std=(1.0 if noise is not None else 0.0), clamp_mode=sc['clamp_mode'],
                                            noise=None if noise is None else noise.unsqueeze(-1))
        _judge(f'{form} S={S} weights', _err(w, sc['w']), _err(w_sw.reshape(n * rays, S), sc['w']), 2e-4)

        # ---- merge: the kernel's own fine depths, against the stable sort of the same values ----
        z_fine = P.sample_pdf(bins, pw, sc['u'].to(dev))
        z_all, src = P.merge_depths(z_fine, z)
        want_z, want_src = hier_ref.merge(z_fine.cpu(), z.cpu())
        assert torch.equal(z_all.cpu().view(torch.int32), want_z.view(torch.int32)) and torch.equal(src.cpu(), want_src), 'merge_depths == stable sort'

        # ---- merged march, given the definition's z_all / src / z_fine ----
        rz_all, rsrc, rz_fine = sc['z_all'].to(dev), sc['src'].to(dev), sc['z_fine'].to(dev)
        got = P.render_rays_merged(rays_d, z_lin, cam, jit, tex, geo, mlp, code, sc['white_back'], sc['max_depth'], rz_all, rsrc, rz_fine)
        assert got is not None, hip_plugin.load().ide3d_last_error()
        pts_fine = rays_o.unsqueeze(2) + rays_dw.unsqueeze(2) * rz_fine.reshape(n, rays, S, 1)
        out_f = R.sample_voxel(tex, geo, pts_fine.reshape(n, -1, 3)).reshape(n, rays, S, -1)
        both = torch.gather(torch.cat([out_f, out], 2), 2, rsrc.reshape(n, rays, 2 * S, 1).long().expand(-1, -1, -1, out.shape[-1]))
        f_sw, d_sw, w2_sw = vr.fancy_integration(both, d_cam, rz_all.reshape(n, rays, 2 * S, 1), dev, noise_std=0, clamp_mode=sc['clamp_mode'],
                                                 white_back=sc['white_back'], max_depth=sc['max_depth'])
    rf, rd, rw = sc['merged']
    _judge(f'{form} S={S} merged features', _err(got[0], rf), _err(f_sw.permute(0, 2, 1), rf), fb)
    _judge(f'{form} S={S} merged depth', _err(got[1], rd), _err(d_sw[..., 0], rd), db)
    _judge(f'{form} S={S} merged weight sum', _err(got[2], rw), _err(w2_sw.sum(2)[..., 0], rw), wb_)
    assert hip_plugin.exclusive_violations()[0] == 0


def test_merge_depths_special_rows(gpu_device):
    """Bit-equal to the stable sort for: the deterministic linspace draws, a zero-weight ray (degenerate pdf: all fine depths equal), forced
    exact ties between fine and coarse depths, all-equal rows; for rows with NaN and +-inf the result is a permutation in which the finite
    values ascend and NaN comes last."""
    from torch_utils import hip_plugin
    P = hip_plugin.VolumeRenderPlugin
    dev = gpu_device
    g = torch.Generator().manual_seed(7)
    for S in STEPS + (96,):
        rows = 37
        z = torch.sort(torch.rand(rows, S, generator=g) * 1.05 + 2.25, dim=1)[0]
        bins = 0.5 * (z[:, :-1] + z[:, 1:])
        wts = torch.rand(rows, S - 2, generator=g) ** 4
        wts[3] = 0                                                            # zero-weight ray
        det = P.sample_pdf(bins.to(dev), (wts + 1e-5).to(dev), torch.linspace(0, 1, S).to(dev))
        fine = {'linspace': det.cpu(), 'random': torch.rand(rows, S, generator=g) * 1.05 + 2.25}
        tie = fine['random'].clone()
        tie[:, ::2] = z[:, torch.randperm(S, generator=g)][:, ::2]             # every other fine depth IS a coarse depth
        tie[5] = z[5]                                                         # a whole row of ties
        fine['ties'] = tie
        fine['all_equal'] = torch.full((rows, S), 2.5)
        for name, zf in fine.items():
            zc = torch.full((rows, S), 2.5) if name == 'all_equal' else z
            z_all, src = P.merge_depths(zf.to(dev), zc.to(dev))
            want_z, want_src = hier_ref.merge(zf, zc)
            assert torch.equal(src.cpu(), want_src), f'S={S} {name}: src'
            assert torch.equal(z_all.cpu().view(torch.int32), want_z.view(torch.int32)), f'S={S} {name}: z_all'
        # arbitrary bits
        wild = fine['random'].clone()
        wild.view(-1)[torch.randperm(rows * S, generator=g)[:rows * S // 3]] = float('nan')
        wild[:, 0] = float('inf'); wild[::2, -1] = -float('inf')
        zc = z.clone(); zc[1] = float('nan'); zc[2, 1] = float('inf')
        z_all, src = P.merge_depths(wild.to(dev), zc.to(dev))
        z_all, src, cat = z_all.cpu(), src.cpu().long(), torch.cat([wild, zc], 1)
        assert torch.equal(torch.sort(src, dim=1)[0], torch.arange(2 * S).expand(rows, -1)), f'S={S}: src is a permutation'
        assert torch.equal(torch.gather(cat, 1, src).view(torch.int32), z_all.view(torch.int32))
        nan = torch.isnan(z_all)
        assert bool((nan[:, 1:] | ~nan[:, :-1]).all()), 'NaN sorts last'
        ok = ~nan[:, 1:]
        assert bool((z_all[:, 1:] >= z_all[:, :-1])[ok].all()), 'everything before the NaNs ascends'
        want_z, want_src = hier_ref.merge(wild, zc)
        assert torch.equal(src, want_src.long())


def _tiny(golden, dev):
    from training import triplane
    (cfg, a), = golden('generator_tiny').cases
    G = triplane.TriPlaneGenerator(triplane.tiny_spec()).eval()
    G.load_state_dict({k[len('sd_'):]: t(v) for k, v in a.items() if k.startswith('sd_')})
    return G.to(dev), a


def test_end_to_end_tiny_fixture(golden, gpu_device):
    """Switch on: the tiny fixture against the oracle's importance pass and against the step-wise path (switch off); one launch each of the
    four, none of sample_voxel / composite; two runs bit-equal; through G.synthesis too."""
    from torch_utils import hip_plugin
    dev = gpu_device
    G, a = _tiny(golden, dev)
    sp = G.synthesis.renderer.spec
    rays, steps = sp.render_size ** 2, sp.num_steps
    u = torch.rand(2 * rays, steps, generator=torch.Generator().manual_seed(5))
    cam = t(a['in_c'])[:, :16].reshape(-1, 4, 4)
    sd = {k: v.detach().cpu() for k, v in G.state_dict().items()}
    want = ogen.render(sd, ospec.tiny(), t(a['out_img_v']), t(a['out_seg_v']), cam, jitter=t(a['in_jitter']), hierarchical=True, importance_u=u)
    args = (t(a['out_img_v'], dev), t(a['out_seg_v'], dev), cam.to(dev))
    kw = dict(jitter=t(a['in_jitter'], dev), hierarchical=True, importance_u=u.to(dev))
    with torch.no_grad():
        with _switch(False):
            old = G.synthesis.renderer(*args, **kw)
        with _switch(True):
            hip_plugin.CALLS.clear()
            got = G.synthesis.renderer(*args, **kw)
            calls = _calls()
            again = G.synthesis.renderer(*args, **kw)
    assert {k: calls.get(k, 0) for k in ('render_ray_weights', 'sample_pdf', 'merge_depths', 'render_rays_merged', 'sample_voxel', 'composite',
                                         'render_rays')} == dict(render_ray_weights=1, sample_pdf=1, merge_depths=1, render_rays_merged=1,
                                                                 sample_voxel=0, composite=0, render_rays=0), calls
    for x, y in zip(got, again):
        assert torch.equal(x, y), 'two runs are bit-equal'
    _judge('tiny features', _err(got[0], want[0]), _err(old[0], want[0]), 3e-4)
    _judge('tiny depth', _err(got[1], want[1]), _err(old[1], want[1]), 1e-4)
    _judge('tiny weight sum', _err(got[2], want[2]), _err(old[2], want[2]), None)
    # against the path it replaces, at the sum of the two bounds above
    assert _err(got[0], old[0]) <= 6e-4 and _err(got[1], old[1]) <= 2e-4
    with torch.no_grad(), _switch(True):
        hip_plugin.CALLS.clear()
        out = G.synthesis(t(a['out_ws'], dev), c=t(a['in_c'], dev), ray_jitter=t(a['in_jitter'], dev),
                          render_params=dict(hierarchical=True, importance_u=u.to(dev)), return_dict=True)
        assert _calls().get('render_rays_merged', 0) == 1 and _calls().get('sample_voxel', 0) == 0
        # (its planes come from the synthesis convolutions on the GPU, not from the fixture: tests/test_gpu_render.py's bound for that depth)
        assert _err(out['image_depth'], want[1]) <= 2e-4
        # the draws: None -> torch.rand on the device; one [S] row for every ray == that row repeated
        rnd = G.synthesis.renderer(*args, jitter=kw['jitter'], hierarchical=True)
        assert all(bool(torch.isfinite(x).all()) for x in rnd) and 2.0 < float(rnd[1].min()) and float(rnd[1].max()) < 3.5
        row = G.synthesis.renderer(*args, jitter=kw['jitter'], hierarchical=True, importance_u=u[0].to(dev))
        rep = G.synthesis.renderer(*args, jitter=kw['jitter'], hierarchical=True, importance_u=u[:1].expand(2 * rays, -1).contiguous().to(dev))
        for x, y in zip(row, rep):
            assert torch.equal(x, y)
    assert hip_plugin.exclusive_violations()[0] == 0


@pytest.mark.parametrize('arith', ['bf16x6', 'fp32'])
def test_end_to_end_real_layout(gpu_device, arith):
    """Planes 256 x 256, C = 32, hidden 64, S = 96 (T = 192), one image of 8 x 8 rays, switch on, against the float64 definitions and the
    step-wise path."""
    from torch_utils import hip_plugin
    from training import triplane
    dev = gpu_device
    sc = _scene(32, 96, 'jitter_noise_softplus', plane=256, size=8, n=1)
    want = hier_ref.render(sc['sd'], sc['tex'], sc['geo'], sc['cam'], FOV, 8, 96, T0, T1, sc['jit'], sc['u'], sigma_noise=sc['noise'])
    R = sc['R'].to(dev)
    args = (sc['tex'].to(dev), sc['geo'].to(dev), sc['cam'].to(dev))
    kw = dict(img_size=8, num_steps=96, jitter=sc['jit'].to(dev), sigma_noise=sc['noise'].to(dev), hierarchical=True, importance_u=sc['u'].to(dev))
    with _arithmetic(arith), torch.no_grad():
        with _switch(False):
            old = R(*args, **kw)
        with _switch(True):
            hip_plugin.CALLS.clear()
            got = R(*args, **kw)
            calls = _calls()
            again = R(*args, **kw)
    assert calls.get('render_ray_weights') == 1 and calls.get('merge_depths') == 1 and calls.get('render_rays_merged') == 1 \
        and calls.get('sample_pdf') == 1 and not calls.get('sample_voxel') and not calls.get('composite'), calls
    for x, y in zip(got, again):
        assert torch.equal(x, y), 'two runs are bit-equal'
    for name, i, bound in (('features', 0, 5e-4), ('depth', 1, 2e-4), ('weight sum', 2, 2e-4)):
        _judge(f'real layout {arith} {name}', _err(got[i], want[i]), _err(old[i], want[i]), bound)
    assert hip_plugin.exclusive_violations()[0] == 0


def test_declines_fall_back_to_the_stepwise_path(gpu_device):
    """A (C, hidden) pair without a compiled form: switch on == switch off, bit for bit, with the step-wise path's launches.  last_back: the two
    marchers decline (None, nothing launched); the renderer's forward has no last_back, so there is no caller above the binding to compare."""
    from torch_utils import hip_plugin
    from training import triplane
    dev = gpu_device
    sp = triplane.GeneratorSpec(plane_channels=8, decoder_hidden=16, feature_channels=4, seg_channels=2, render_size=SIZE, num_steps=12)
    torch.manual_seed(5)
    R = triplane.TriplaneRenderer(sp).to(dev).eval()
    g = torch.Generator().manual_seed(6)
    tex, geo = ((torch.randn(2, 24, 32, 32, generator=g) * 0.7).to(dev) for _ in range(2))
    kw = dict(jitter=torch.rand(2, 25, 12, generator=g).to(dev), hierarchical=True, importance_u=torch.rand(50, 12, generator=g).to(dev))
    res, calls = [], []
    with torch.no_grad():
        for on in (False, True):
            with _switch(on):
                hip_plugin.CALLS.clear()
                res.append(R(tex, geo, _cams(2).to(dev), **kw))
                calls.append(_calls())
    assert calls[0] == calls[1] and calls[1].get('composite') == 2 and 'render_rays_merged' not in calls[1], calls
    for x, y in zip(*res):
        assert torch.equal(x, y)
    # last_back at the binding
    sc = _scene(16, 12, 'jitter_noise_softplus')
    Rt, tex, geo, rays_d, z_lin, cam, jit, noise = _device_inputs(sc, dev)
    P = hip_plugin.VolumeRenderPlugin
    hip_plugin.CALLS.clear()
    with torch.no_grad():
        mlp = Rt.decoder.kernel_weights()
        assert P.render_ray_weights(rays_d, z_lin, cam, jit, noise, tex, geo, mlp, 0, last_back=True) is None
        assert P.render_rays_merged(rays_d, z_lin, cam, jit, tex, geo, mlp, 0, False, None, sc['z_all'].to(dev), sc['src'].to(dev),
                                    sc['z_fine'].to(dev), last_back=True) is None
    assert not _calls()


def test_declines_and_argument_errors_keep_code_and_text(gpu_device):
    """Every decline (IDE3D_ENOKERNEL = -2) and argument error (IDE3D_EINVAL = -1) of the three marchers and the two backward entry points,
    once per entry point, straight at the library: the return code and the exact ide3d_last_error() text.  Nothing is launched: each call
    carries one fault and is turned away by the host-side checks."""
    import ctypes
    from torch_utils import hip_plugin
    dev, P, lib = gpu_device, hip_plugin.VolumeRenderPlugin, hip_plugin.load()
    C, hidden, feat, seg, S, rays = 16, 32, 8, 5, 12, 25
    z = lambda *shape: torch.zeros(*shape, device=dev)
    tex, geo = (z(1, 3 * C, 8, 8).contiguous(memory_format=torch.channels_last) for _ in range(2))
    mlp = dict(geo_w0=z(hidden, C), geo_b0=z(hidden), geo_w1=z(1 + seg, hidden), geo_b1=z(1 + seg),
               tex_w0=z(hidden, C), tex_b0=z(hidden), tex_w1=z(feat, hidden), tex_b1=z(feat))
    p0, keep = P._ray_params(z(rays, 3), z(S), z(1, 4, 4), None, None, tex, geo, mlp, 0, False, False, None)
    outs = P._ray_outputs(p0, dev)
    z_all, src, z_fine = z(rays, 2 * S), torch.zeros(rays, 2 * S, dtype=torch.int32, device=dev), z(rays, S)
    dtex, dgeo = torch.zeros_like(tex), torch.zeros_like(geo)
    g = hip_plugin._RenderGrads()
    g.grad_tex_planes, g.grad_geo_planes = dtex.data_ptr(), dgeo.data_ptr()
    g.grad_tex_stride, g.grad_geo_stride = hip_plugin._i64x4(dtex.stride()), hip_plugin._i64x4(dgeo.stride())
    ptr, stream = hip_plugin._ptr, hip_plugin._stream(tex)
    merged = (ptr(z_all), ptr(src), ptr(z_fine))
    entries = {        # name -> (hierarchical, call(p, total_steps))
        'render_rays': (False, lambda p, T: lib.ide3d_render_rays(ctypes.byref(p), stream)),
        'render_ray_weights': (True, lambda p, T: lib.ide3d_render_ray_weights(ctypes.byref(p), None, None, None, None, stream)),
        'render_rays_merged': (True, lambda p, T: lib.ide3d_render_rays_merged(ctypes.byref(p), *merged, T, stream)),
        'render_rays_backward': (False, lambda p, T: lib.ide3d_render_rays_backward(ctypes.byref(p), ctypes.byref(g), stream)),
        'render_rays_merged_backward': (True, lambda p, T: lib.ide3d_render_rays_merged_backward(ctypes.byref(p), *merged, T, ctypes.byref(g), None,
                                                                                                 stream)),
    }

    def fault(**fields):
        p = type(p0).from_buffer_copy(p0)
        for k, v in fields.items():
            setattr(p, k, v)
        return p

    nchw = hip_plugin._i64x4((3 * C * 64, 64, 8, 1))
    small = hip_plugin._i64x4((24 * 64, 1, 24 * 8, 24))
    cases = [        # (fault, code, text after "<entry>: ", hierarchical entries only)
        (fault(last_back=1), -2, 'last_back is not fused; use the step-wise ops', False),
        (fault(tex_stride=nchw, geo_stride=nchw), -2, 'tri-planes must be channels_last, 16-byte aligned', False),
        (fault(C=8, hidden=16, tex_stride=small, geo_stride=small), -2, 'no fused kernel for C=8 hidden=16', False),
        (fault(steps=2), -2, 'the hierarchical pass takes 3 .. 1024 steps, got 2', True),
        (fault(steps=1025), -2, 'the hierarchical pass takes 3 .. 1024 steps, got 1025', True),
        (fault(clamp_mode=2), -1, 'Need to choose clamp mode', False),
    ]
    hip_plugin.CALLS.clear()
    seen = 0
    for name, (hier, call) in entries.items():
        for p, code, text, hier_only in cases:
            if hier_only and not hier:
                continue
            rc = call(p, 2 * p.steps)
            got = lib.ide3d_last_error().decode()
            print(name, rc, got)
            assert rc == code and got == f'{name}: {text}', (name, rc, got)
            seen += 1
    for name in ('render_rays_merged', 'render_rays_merged_backward'):
        rc = entries[name][1](p0, 2 * S + 1)
        got = lib.ide3d_last_error().decode()
        print(name, rc, got)
        assert rc == -1 and got == f'{name}: total_steps must be 2 * steps = {2 * S}, got {2 * S + 1}', (name, rc, got)
        seen += 1
    assert seen == 5 * 4 + 3 * 2 + 2 and not _calls()
    assert all(float(o.abs().max()) == 0 for o in (dtex, dgeo)), 'nothing ran'
    del keep, outs
