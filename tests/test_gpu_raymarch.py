"""The fused ray-marcher (`render_rays_kernel`, ide-3d_amd/csrc/raymarch.hip) at its edges against the float64 oracle.  `pytest -m gpu`.

The kernel has three compiled forms, chosen at run time in `ide3d_render_rays`: C=32 with the bf16x6 MLP (any split arithmetic, 8 waves per
workgroup), C=32 with the fp32 MLP (`conv_arithmetic('fp32')`, 4 waves) and C=16 (the tiny spec, fp32 MLP, 4 waves).  Every form runs the
same case list, which together covers: step counts that are not a multiple of the 16-sample tile (1, 5, 17, 33, 97) and one that is (16);
ray counts that are not a multiple of the wave count, or smaller than it; batches whose rays per wave cross images; a different camera per
image; jitter as a tensor and off; density noise; `white_back`, `clamp_mode='relu'` and `max_depth`; rays that leave the planes (zeros
padding); non-square planes; tex / geo as channel-range views of one channels_last tensor; and the decoder widths at their limits.

Reference: `oracle.generator.render` / `sample_voxel` on `oracle.ops`: the tri-plane taps are accumulated in float64, the compositing is a
sequential float64 loop, the ray coordinates are rounded to fp32 the way the reference's fp32 ray math rounds them, and the decoder layers are
fp32 products with float64 activations rounded once.

Tolerances are those of tests/test_gpu_render.py, for every case: features 3e-4 of the feature scale, depth and weight sum 1e-4 of theirs.
"""

import contextlib

import numpy as np
import pytest
import torch

from oracle import generator as ogen
from oracle import ops as oracle_ops
from oracle import spec as ospec

pytestmark = pytest.mark.gpu

FEAT_TOL, DEPTH_TOL = 3e-4, 1e-4

# kernel form -> (arithmetic, renderer spec overrides)
TINY = dict(plane_channels=16, decoder_hidden=32, feature_channels=8, seg_channels=5)
FORMS = {'c32_bf16x6': ('bf16x6', {}), 'c32_fp32': ('fp32', {}), 'c16': ('default', TINY)}

# n images of size x size rays, `steps` samples per ray; planes [n, 3C, H, W] (default 32 x 32)
CASES = {
    # 225 rays (not a multiple of 4 or 8), one partial tile after a full one
    's17_225rays': dict(n=1, size=15, steps=17),
    # 4 rays per image (< waves per workgroup); 2400 rays: every wave walks several rays that lie 1 (4 waves) or 2 (8 waves) images apart
    's1_2x2_600img': dict(n=600, size=2, steps=1, jitter=False, plane=(16, 16)),
    # 5 x 1089 rays: blocks of 12 / 24 rays, each wave's ray sequence crosses images; density noise
    's33_crossing_noise': dict(n=5, size=33, steps=33, noise=True),
    # relu on densities centred at 0 (the last sample often has alpha 0, so the weight sum is < 1): white_back and max_depth matter
    's5_relu_white_maxdepth': dict(n=8, size=15, steps=5, jitter=False, clamp_mode='relu', white_back=True, max_depth=3.75),
    # fov 40, rays from 0.5 to 5.0: many samples outside [-1, 1] on some plane (zeros padding)
    's97_border': dict(n=1, size=16, steps=97, fov=40.0, ray_start=0.5, ray_end=5.0),
    # H != W, exactly one tile per ray
    's16_nonsquare': dict(n=3, size=9, steps=16, plane=(48, 80)),
    # tex = x[:, :3C], geo = x[:, 3C:] of one channels_last [n, 6C, H, W]: pixel stride 6C, geo base 3C floats in
    's33_channel_views': dict(n=3, size=8, steps=33, views=True, noise=True),
    # the widest decoder the kernel takes: 32 features, 31 semantic channels (all 32 output rows of both branches)
    's17_widest_decoder': dict(n=1, size=15, steps=17, clamp_mode='relu', white_back=True, spec=dict(feature_channels=32, seg_channels=31)),
    # the narrowest: RGB only, no semantic channels
    's5_narrowest_decoder': dict(n=3, size=7, steps=5, noise=True, spec=dict(feature_channels=3, seg_channels=0)),
    # the product's size (64 x 64 rays, 96 steps) on 256 x 256 planes, checked on a fixed subset of 320 rays per image
    's96_full_size_subset': dict(n=2, size=64, steps=96, noise=True, plane=(256, 256), subset=320),
}


def _calls(name):
    from torch_utils import hip_plugin
    return hip_plugin.CALLS.get(name, 0)


def _rel(actual, expected, tol, what):
    a = actual.detach().cpu().double(); e = torch.as_tensor(expected).detach().cpu().double()
    assert a.shape == e.shape, f'{what}: shape {tuple(a.shape)} != {tuple(e.shape)}'
    scale = float(e.abs().max()) + 1e-12
    err = float((a - e).abs().max())
    assert err <= tol * scale, f'{what}: max abs err {err:.3e} > {tol} * scale {scale:.3e}'


@contextlib.contextmanager
def _arithmetic(name):
    from torch_utils import hip_plugin
    try:
        hip_plugin.conv_arithmetic(name)
        yield
    finally:
        hip_plugin.conv_arithmetic('default')


def _cameras(n, seed):
    """A different camera for every image: yaw in [-0.6, 0.6], pitch pi/2 +- 0.3, radius 2.7 +- 0.2."""
    from training import triplane
    g = np.random.RandomState(seed)
    return torch.cat([triplane.camera_label(float(g.uniform(-0.6, 0.6)), pitch=float(np.pi / 2 + g.uniform(-0.3, 0.3)),
                                            radius=float(2.7 + g.uniform(-0.2, 0.2))) for _ in range(n)])[:, :16].reshape(n, 4, 4)


def _setup(form, case, seed):
    """-> (renderer on the GPU, state dict for the oracle, oracle Spec, tex / geo as the kernel reads them, their CPU copies, cameras,
    jitter | None, sigma noise | None) for one case."""
    from training import triplane
    _arith, base = FORMS[form]
    sp_kw = dict(base, **case.get('spec', {}))
    render_kw = dict(render_size=case['size'], num_steps=case['steps'], fov=case.get('fov', 18.0), ray_start=case.get('ray_start', 2.25),
                     ray_end=case.get('ray_end', 3.3), clamp_mode=case.get('clamp_mode', 'softplus'))
    sp = triplane.GeneratorSpec(**sp_kw, **render_kw)
    osp = ospec.Spec(**sp_kw, **render_kw)
    torch.manual_seed(seed)
    R = triplane.TriplaneRenderer(sp).eval()
    with torch.no_grad():
        for p in R.parameters():
            if p.ndim == 1:
                p.copy_(torch.randn_like(p) * 0.2)
    n, C = case['n'], sp.plane_channels
    H, W = case.get('plane', (32, 32))
    g = torch.Generator().manual_seed(seed + 1)
    if case.get('views'):
        both = (torch.randn(n, 6 * C, H, W, generator=g) * 0.7).contiguous(memory_format=torch.channels_last)
        tex_c, geo_c = both[:, :3 * C].contiguous(), both[:, 3 * C:].contiguous()
        both = both.cuda()
        tex, geo = both[:, :3 * C], both[:, 3 * C:]
        assert tex.stride(1) == 1 and tex.stride(3) == 6 * C and geo.data_ptr() == both.data_ptr() + 3 * C * 4
    else:
        tex_c, geo_c = torch.randn(n, 3 * C, H, W, generator=g) * 0.7, torch.randn(n, 3 * C, H, W, generator=g) * 0.7
        tex, geo = (x.cuda().contiguous(memory_format=torch.channels_last) for x in (tex_c, geo_c))
    if osp.clamp_mode == 'relu':
        # centre the densities of the rendered volume at 0, so that about half of all samples have density 0
        sd = {'synthesis.renderer.' + k: v.detach() for k, v in R.state_dict().items()}
        probe = torch.rand(1, 4096, 3, generator=g) - 0.5
        sig = ogen.sample_voxel(sd, osp, tex_c[:1], geo_c[:1], probe)[:, -1]
        with torch.no_grad():
            R.decoder.geo1.bias[0] -= float(sig.median()) / R.decoder.geo1.bias_gain
    sd = {'synthesis.renderer.' + k: v.detach().clone() for k, v in R.state_dict().items()}
    rays, S = case['size'] ** 2, case['steps']
    cam = _cameras(n, seed + 2)
    jit = torch.rand(n, rays, S, generator=g) if case.get('jitter', True) else None
    noise = torch.randn(n, rays, S, generator=g) * 0.5 if case.get('noise') else None
    return R.cuda(), sd, osp, tex, geo, tex_c, geo_c, cam, jit, noise


def _oracle(sd, osp, tex, geo, cam, jit, noise, white_back, max_depth, rays=None):
    """-> features [n, rays, ch], depth [n, rays], weight sum [n, rays] of the float64 reference; `rays` selects a subset of each image."""
    n, size, S = tex.shape[0], osp.render_size, osp.num_steps
    if rays is None:
        f, d, w = ogen.render(sd, osp, tex, geo, cam, jitter=jit, sigma_noise=noise, ops=oracle_ops, white_back=white_back, max_depth=max_depth)
        return f.reshape(n, -1, size * size).transpose(1, 2), d.reshape(n, -1), w.reshape(n, -1)
    # the same stages as ogen.render, on the selected rays only
    p, z, d_cam = oracle_ops.initial_rays(n, S, osp.fov, (size, size), osp.ray_start, osp.ray_end)
    p, z, d_cam = p[:, rays], z[:, rays], d_cam[:, rays]
    if jit is not None:
        p, z = oracle_ops.perturb(p, z, d_cam, jit[:, rays].unsqueeze(-1))
    world = oracle_ops.to_world(p, cam.float())
    out = ogen.sample_voxel(sd, osp, tex, geo, world.reshape(n, -1, 3), oracle_ops).reshape(n, len(rays), S, -1)
    f, d, w = oracle_ops.composite(out, d_cam, z, noise=None if noise is None else noise[:, rays].unsqueeze(-1), clamp_mode=osp.clamp_mode,
                                   white_back=white_back, max_depth=max_depth)
    return f, d[..., 0], w.sum(2)[..., 0]


def _render(R, osp, tex, geo, cam, jit, noise, case):
    """One fused launch through the product's entry points: `TriplaneRenderer.forward`, or `render_triplane_fused` for `max_depth`."""
    from training import volumetric_rendering as vr
    size, S = osp.render_size, osp.num_steps
    jit_d = None if jit is None else jit.cuda()
    noise_d = None if noise is None else noise.cuda()
    with torch.no_grad():
        if case.get('max_depth'):
            return vr.render_triplane_fused(tex, geo, R.decoder.kernel_weights(), cam.cuda(), osp.fov, (size, size), S, osp.ray_start,
                                            osp.ray_end, jitter=jit_d, sigma_noise=noise_d, clamp_mode=osp.clamp_mode,
                                            white_back=case.get('white_back', False), max_depth=case['max_depth'])
        return R(tex, geo, cam.cuda(), jitter=(False if jit is None else jit_d), sigma_noise=noise_d, white_back=case.get('white_back', False))


@pytest.mark.parametrize('case_id', list(CASES))
@pytest.mark.parametrize('form', list(FORMS))
def test_fused_renderer_edges_vs_float64(gpu_device, form, case_id):
    case = CASES[case_id]
    seed = sorted(CASES).index(case_id) * 10 + sorted(FORMS).index(form)
    R, sd, osp, tex, geo, tex_c, geo_c, cam, jit, noise = _setup(form, case, seed)
    n, size = case['n'], case['size']
    with _arithmetic(FORMS[form][0]):
        before = _calls('render_rays')
        feat, depth, wsum = _render(R, osp, tex, geo, cam, jit, noise, case)
        assert _calls('render_rays') - before == 1, 'the fused kernel must have run exactly once'
    nch = osp.feature_channels + osp.seg_channels
    assert feat.shape == (n, nch, size, size) and depth.shape == wsum.shape == (n, 1, size, size)
    rays = None
    if case.get('subset'):
        rays = torch.from_numpy(np.random.RandomState(seed).choice(size * size, case['subset'], replace=False)).sort().values
    want_f, want_d, want_w = _oracle(sd, osp, tex_c, geo_c, cam, jit, noise, case.get('white_back', False), case.get('max_depth'), rays)
    got_f, got_d, got_w = feat.reshape(n, nch, -1).transpose(1, 2), depth.reshape(n, -1), wsum.reshape(n, -1)
    if rays is not None:
        got_f, got_d, got_w = got_f[:, rays], got_d[:, rays], got_w[:, rays]
    if osp.clamp_mode == 'relu':
        # the case is only meaningful when the background terms are: some rays must keep a visible part of their transmittance
        assert float((1 - want_w).max()) > 0.05, 'relu case: every ray saturated, white_back / max_depth untested'
    _rel(got_f, want_f, FEAT_TOL, f'{form} {case_id} features')
    _rel(got_d, want_d, DEPTH_TOL, f'{form} {case_id} depth')
    _rel(got_w, want_w, DEPTH_TOL, f'{form} {case_id} weight sum')


def test_split_arithmetics_share_the_bf16x6_renderer(gpu_device):
    """bf16x3 and f16x3 select the same compiled form as bf16x6 (every split arithmetic runs the bf16x6 MLP): bit-equal outputs."""
    case = CASES['s33_crossing_noise']
    R, sd, osp, tex, geo, tex_c, geo_c, cam, jit, noise = _setup('c32_bf16x6', case, 7)
    out = {}
    for arith in ('bf16x6', 'bf16x3', 'f16x3'):
        with _arithmetic(arith):
            before = _calls('render_rays')
            out[arith] = _render(R, osp, tex, geo, cam, jit, noise, case)
            assert _calls('render_rays') - before == 1
    for arith in ('bf16x3', 'f16x3'):
        for a, b in zip(out[arith], out['bf16x6']):
            assert torch.equal(a, b), f'{arith} renderer output differs from bf16x6'


def test_trainable_decoder_is_differentiated(gpu_device):
    """Planes and camera without grad, only the decoder trainable: `forward`, `sample_voxel` and `density_lattice` must not take the fused
    kernels (raw pointers, no autograd) and the decoder's gradients must equal those of the same module run on the CPU in float64."""
    from training import triplane
    from training import volumetric_rendering as vr
    torch.manual_seed(3)
    sp = triplane.GeneratorSpec(render_size=8, num_steps=9)
    Rc = triplane.TriplaneRenderer(sp)
    with torch.no_grad():
        for p in Rc.parameters():
            if p.ndim == 1:
                p.copy_(torch.randn_like(p) * 0.2)
    Rg = triplane.TriplaneRenderer(sp).to(gpu_device)
    Rg.load_state_dict(Rc.state_dict())
    Rc = Rc.double()
    assert all(p.requires_grad for p in Rg.decoder.parameters())
    g = torch.Generator().manual_seed(4)
    n, rays, S = 2, 64, 9
    tex, geo = torch.randn(n, 96, 32, 32, generator=g) * 0.7, torch.randn(n, 96, 32, 32, generator=g) * 0.7
    cam = _cameras(n, 5)
    jit = torch.rand(n, rays, S, generator=g)
    pts = torch.rand(n, 50, 3, generator=g) * 2.4 - 1.2
    wf, wd = torch.randn(n, 51, 8, 8, generator=g), torch.randn(n, 1, 8, 8, generator=g)
    ws, wl = torch.randn(n * 50, 52, generator=g), torch.randn(n * 27, generator=g)
    texd, geod = tex.to(gpu_device), geo.to(gpu_device)
    names = ('render_rays', 'sample_voxel', 'density_lattice')
    before = {k: _calls(k) for k in names}
    feat, depth, wsum = Rg(texd, geod, cam.to(gpu_device), jitter=jit.to(gpu_device))
    sv = Rg.sample_voxel(texd, geod, pts.to(gpu_device))
    lat = Rg.density_lattice(texd, geod, 3, 0.5, np.array([-0.5, -0.5, -0.5]), 0.9, 0, 27)
    assert {k: _calls(k) - before[k] for k in names} == {k: 0 for k in names}, 'a fused kernel ran for a trainable decoder'
    for what, x in (('features', feat), ('depth', depth), ('weight sum', wsum), ('sample_voxel', sv), ('density_lattice', lat)):
        assert x.grad_fn is not None, f'{what} carries no grad_fn'
    params = list(Rg.decoder.parameters())
    got_r = torch.autograd.grad((feat * wf.to(gpu_device)).sum() + (depth * wd.to(gpu_device)).sum(), params)
    got_v = torch.autograd.grad((sv * ws.to(gpu_device)).sum() + (lat * wl.to(gpu_device)).sum(), params)
    # the same module on the CPU in float64: the step-wise forward (ray set-up in fp32 like the reference), planes and decoder in float64
    tex64, geo64 = tex.double(), geo.double()
    p0, z, d_cam = vr.get_initial_rays_trig(n, S, 'cpu', sp.fov, (8, 8), sp.ray_start, sp.ray_end)
    wp, z, *_ = vr.transform_sampled_points(p0, z, d_cam, 'cpu', h_stddev=0, v_stddev=0, camera=cam, mode=None, jitter=jit.unsqueeze(-1))
    out = Rc.sample_voxel(tex64, geo64, wp.reshape(n, -1, 3).double()).reshape(n, rays, S, -1)
    f64, d64, _w = vr.fancy_integration(out, d_cam.double(), z.double(), 'cpu', noise_std=0, clamp_mode='softplus')
    f64, d64 = f64.permute(0, 2, 1).reshape(n, -1, 8, 8), d64.permute(0, 2, 1).reshape(n, 1, 8, 8)
    _rel(feat, f64, FEAT_TOL, 'trainable-decoder features'); _rel(depth, d64, DEPTH_TOL, 'trainable-decoder depth')
    from training import shape_extraction
    lat_pts = shape_extraction.lattice_points(3, 0.5, np.array([-0.5, -0.5, -0.5]), 0.9, 0, 27, 'cpu')
    sv64 = Rc.sample_voxel(tex64, geo64, pts.double())
    lat64 = Rc.sample_voxel(tex64, geo64, lat_pts.double().unsqueeze(0).expand(n, -1, -1), sigma_only=True)
    cparams = list(Rc.decoder.parameters())
    want_r = torch.autograd.grad((f64 * wf.double()).sum() + (d64 * wd.double()).sum(), cparams)
    want_v = torch.autograd.grad((sv64 * ws.double()).sum() + (lat64 * wl.double()).sum(), cparams)
    for (name, _p), a, b in zip(Rg.decoder.named_parameters(), got_r, want_r):
        _rel(a, b, 1e-4, f'render gradient of decoder.{name}')
    for (name, _p), a, b in zip(Rg.decoder.named_parameters(), got_v, want_v):
        _rel(a, b, 1e-4, f'point-query gradient of decoder.{name}')
