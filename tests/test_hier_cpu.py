"""The hierarchical pass as four HIP launches, what can be checked without a GPU: the C boundary of the three new
entry points and their host-side argument rules, the float64 definitions of tests/hier_ref.py against the oracle's own importance pass,
the merge definition on hand-made rows, and the routing of `TriplaneRenderer.forward` under `triplane.fused_hierarchical`."""

import ctypes
import os
import re

import numpy as np
import pytest
import torch

import hier_ref
from oracle import generator as ogen
from oracle import spec as ospec
from util import assert_close, t

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ('ide3d_render_ray_weights', 'ide3d_merge_depths', 'ide3d_render_rays_merged')
EINVAL, ENOKERNEL = -1, -2


def _lib():
    from torch_utils import hip_plugin
    path = hip_plugin.lib_path()
    assert os.path.isfile(path), f'{path} missing: run __graft_entry__.build()'
    lib = ctypes.CDLL(path)
    vp, i32, i64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64
    P = ctypes.POINTER(hip_plugin._RenderParams)
    lib.ide3d_render_ray_weights.argtypes = [P, vp, vp, vp, vp, vp]
    lib.ide3d_merge_depths.argtypes = [vp, vp, i64, i32, i32, vp, vp, vp]
    lib.ide3d_render_rays_merged.argtypes = [P, vp, vp, vp, i32, vp]
    for name in NEW:
        getattr(lib, name).restype = ctypes.c_int
    return lib


def test_new_entry_points_declared_listed_and_exported():
    from torch_utils import hip_plugin
    src = open(os.path.join(ROOT, 'include', 'ide3d_hip.h')).read()
    src = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    lib = _lib()
    for name in NEW:
        assert re.search(r'\bint\s+%s\s*\(' % name, src), f'{name} not declared in include/ide3d_hip.h'
        assert name in hip_plugin.EXPORTED_SYMBOLS
        assert hasattr(lib, name), f'{name} not exported'
    for method in ('render_ray_weights', 'merge_depths', 'render_rays_merged'):
        assert callable(getattr(hip_plugin.VolumeRenderPlugin, method))


def _params(hip_plugin, backing, steps=12, C=8, hidden=16, last_back=0, channels_last=True):
    """An ide3d_render_params whose pointers all name `backing` (16-byte aligned host memory: nothing here may reach a launch)."""
    p = hip_plugin._RenderParams()
    addr = backing.ctypes.data
    assert addr % 16 == 0
    for f in ('rays_d_cam', 'z_lin', 'cam2world', 'tex_planes', 'geo_planes', 'out_feat', *hip_plugin.VolumeRenderPlugin.MLP_KEYS):
        setattr(p, f, addr)
    H = W = 8
    strides = (3 * C * H * W, 1, W * 3 * C, 3 * C) if channels_last else (3 * C * H * W, H * W, W, 1)
    p.tex_stride = p.geo_stride = (ctypes.c_int64 * 4)(*strides)
    p.n, p.rays_per_img, p.steps = 1, 4, steps
    p.C, p.H, p.W, p.hidden, p.feat_ch, p.seg_ch = C, H, W, hidden, 4, 2
    p.clamp_mode, p.last_back = 0, last_back
    return p


def test_host_side_argument_checks():
    """Null pointers are IDE3D_EINVAL; steps < 3, last_back, planes that are not channels_last and a (C, hidden) without a compiled form are
    IDE3D_ENOKERNEL: all decided on the host, before any device call (this test runs without a GPU)."""
    from torch_utils import hip_plugin
    lib = _lib()
    buf = np.zeros(4096 + 16, dtype=np.uint8)
    off = (-buf.ctypes.data) % 16
    backing = buf[off:off + 4096]
    a = backing.ctypes.data
    ok = _params(hip_plugin, backing)
    # null pointers
    assert lib.ide3d_render_ray_weights(None, a, a, a, a, None) == EINVAL
    assert lib.ide3d_render_rays_merged(None, a, a, a, 24, None) == EINVAL
    for args in ((None, a, a), (a, None, a), (a, a, None)):
        assert lib.ide3d_render_rays_merged(ctypes.byref(ok), *args, 24, None) == EINVAL
    bad = _params(hip_plugin, backing)
    bad.z_lin = None
    assert lib.ide3d_render_ray_weights(ctypes.byref(bad), a, a, a, a, None) == EINVAL
    bad = _params(hip_plugin, backing)
    bad.geo_w1 = None
    assert lib.ide3d_render_rays_merged(ctypes.byref(bad), a, a, a, 24, None) == EINVAL
    for args in ((None, a, a, a), (a, None, a, a), (a, a, None, a), (a, a, a, None)):
        assert lib.ide3d_merge_depths(args[0], args[1], 4, 12, 12, args[2], args[3], None) == EINVAL
    assert lib.ide3d_merge_depths(a, a, 4, 2048, 1, a, a, None) == EINVAL           # T above the LDS the kernel is given
    assert lib.ide3d_merge_depths(a, a, -1, 12, 12, a, a, None) == EINVAL
    assert lib.ide3d_merge_depths(a, a, 0, 12, 12, a, a, None) == 0                 # no rays: nothing to launch
    # declines
    for kw in (dict(steps=2), dict(steps=1), dict(steps=1025), dict(last_back=1), dict(channels_last=False), dict()):
        p = _params(hip_plugin, backing, **kw)                                       # dict(): C = 8, hidden = 16 has no compiled form
        assert lib.ide3d_render_ray_weights(ctypes.byref(p), a, a, a, a, None) == ENOKERNEL, kw
        assert lib.ide3d_render_rays_merged(ctypes.byref(p), a, a, a, 2 * p.steps, None) == ENOKERNEL, kw
    p = _params(hip_plugin, backing, steps=12)
    p.out_feat = None
    assert lib.ide3d_render_rays_merged(ctypes.byref(p), a, a, a, 24, None) == EINVAL
    p = _params(hip_plugin, backing, steps=12)
    assert lib.ide3d_render_rays_merged(ctypes.byref(p), a, a, a, 23, None) == EINVAL   # total_steps must be 2 * steps


# ---- the definitions ---------------------------------------------------------------------------------------

def _tiny(golden):
    from training import triplane
    (cfg, a), = golden('generator_tiny').cases
    G = triplane.TriPlaneGenerator(triplane.tiny_spec()).eval()
    G.load_state_dict({k[len('sd_'):]: t(v) for k, v in a.items() if k.startswith('sd_')})
    return G, a


@pytest.fixture(scope='module')
def tiny_case(golden):
    G, a = _tiny(golden)
    sp = ospec.tiny()
    rays, steps = sp.render_size ** 2, sp.num_steps
    u = torch.rand(2 * rays, steps, generator=torch.Generator().manual_seed(5))
    cam = t(a['in_c'])[:, :16].reshape(-1, 4, 4)
    sd = {k: v.detach() for k, v in G.state_dict().items()}
    tex, geo, jit = t(a['out_img_v']), t(a['out_seg_v']), t(a['in_jitter'])
    want = ogen.render(sd, sp, tex, geo, cam, jitter=jit, hierarchical=True, importance_u=u)
    plain = ogen.render(sd, sp, tex, geo, cam, jitter=jit)
    got = hier_ref.render(sd, tex, geo, cam, sp.fov, sp.render_size, steps, sp.ray_start, sp.ray_end, jit, u)
    return dict(G=G, sp=sp, sd=sd, tex=tex, geo=geo, cam=cam, jit=jit, u=u, want=want, plain=plain, got=got)


def test_hier_ref_equals_the_oracles_importance_pass(tiny_case):
    c = tiny_case
    for g_, w_, name in zip(c['got'][:3], c['want'], ('features', 'depth', 'weight sum')):
        assert_close(g_, w_, rtol=1e-4, atol=1e-5, what=f'hier_ref {name}')
    z_fine, z_all, src = c['got'][3]
    # the oracle sorts without `stable`: the comparison above stands on a fixture without ties
    assert float((z_all[:, 1:] - z_all[:, :-1]).min()) > 0


def test_fine_samples_move_the_result(tiny_case):
    """A merged march that ignored the fine samples (or placed them on the coarse ones) would reproduce the plain render: the two differ by
    6 % of the feature scale on this fixture (0.64 of 10.6), far above every tolerance used for the pass."""
    c = tiny_case
    scale = float(c['want'][0].abs().max())
    diff = float((c['want'][0] - c['plain'][0]).abs().max())
    print(f'hierarchical vs plain features: {diff:.3g} at scale {scale:.3g}')
    assert diff > 1e-2 * scale
    assert float((c['got'][0] - c['plain'][0]).abs().max()) > 1e-2 * scale


def _check_merge(z_fine, z_coarse):
    z_all, src = hier_ref.merge(z_fine, z_coarse)
    cat = torch.cat([z_fine, z_coarse], 1)
    T = cat.shape[1]
    for r in range(cat.shape[0]):
        s = src[r].long()
        assert sorted(s.tolist()) == list(range(T)), 'src is a permutation'
        assert torch.equal(cat[r][s].view(torch.int32), z_all[r].view(torch.int32)), 'z_all is the input, bit for bit, in src order'
        v = z_all[r]
        for k in range(T - 1):
            a, b = float(v[k]), float(v[k + 1])
            if np.isnan(a):
                assert np.isnan(b), 'NaN sorts last'
            elif not np.isnan(b):
                assert a <= b, 'ascending'
                if a == b:
                    assert int(s[k]) < int(s[k + 1]), 'equal depths keep concatenation order'
            if np.isnan(a) and np.isnan(b):
                assert int(s[k]) < int(s[k + 1]), 'NaNs keep concatenation order'
    return z_all, src


def test_merge_definition_on_hand_made_rows():
    inf, nan = float('inf'), float('nan')
    coarse = torch.tensor([[1.0, 2.0, 3.0, 4.0]])
    # exact ties between a fine and a coarse depth: the fine one (earlier in the concatenation) first
    z_all, src = _check_merge(torch.tensor([[3.0, 1.0, 2.5, 4.0]]), coarse)
    assert src.tolist() == [[1, 4, 5, 2, 0, 6, 3, 7]]
    assert z_all.tolist() == [[1.0, 1.0, 2.0, 2.5, 3.0, 3.0, 4.0, 4.0]]
    # all equal: the identity
    z_all, src = _check_merge(torch.full((1, 4), 2.0), torch.full((1, 4), 2.0))
    assert src.tolist() == [list(range(8))]
    # NaN and +-inf: finite values in order, -inf first, +inf after them, NaN last
    z_all, src = _check_merge(torch.tensor([[nan, 2.5, -inf, inf]]), torch.tensor([[1.0, nan, 3.0, inf]]))
    assert src.tolist() == [[2, 4, 1, 6, 3, 7, 0, 5]]
    _check_merge(torch.tensor([[nan, nan, nan]]), torch.tensor([[nan, 1.0, nan]]))


# ---- routing ------------------------------------------------------------------------------------------------

def test_switch_defaults_off_and_routes_only_what_the_launches_cover(tiny_case, monkeypatch):
    from training import triplane
    from training import volumetric_rendering as vr
    assert triplane.fused_hierarchical is False
    c = tiny_case
    R = c['G'].synthesis.renderer
    calls = []

    def spy(*args, **kwargs):
        calls.append(kwargs)
        return None                 # "no kernel": the caller must fall through to the step-wise code

    monkeypatch.setattr(vr, 'render_triplane_hierarchical', spy)
    args = (c['tex'], c['geo'], c['cam'])
    kw = dict(jitter=c['jit'], hierarchical=True, importance_u=c['u'])
    with torch.no_grad():
        base = R(*args, **kw)
    assert not calls, 'switch off: the step-wise path'
    monkeypatch.setattr(triplane, 'fused_hierarchical', True)
    with torch.no_grad():
        cpu = R(*args, **kw)                                                        # CPU tensors
    grad = R(c['tex'].clone().requires_grad_(True), c['geo'], c['cam'], **kw)       # a tensor that needs a gradient
    with torch.no_grad():
        R(*args, jitter=c['jit'], hierarchical=False)                               # the plain render never goes there
    assert not calls and grad[0].requires_grad
    for x, y in zip(cpu + tuple(g.detach() for g in grad), base + base):
        assert torch.equal(x, y)
    # with the device test out of the way: sigma_noise_fine keeps the call step-wise, its absence sends it to the new path once, and a None
    # from there falls through to the step-wise result
    monkeypatch.setattr(triplane.TriplaneRenderer, '_hip_ok', lambda self, *tensors: True)
    monkeypatch.setattr(triplane.TriplaneRenderer, 'sample_voxel', _cpu_sample_voxel)
    with torch.no_grad():
        R(*args, sigma_noise_fine=torch.zeros(2, 64, 24), **kw)
        assert not calls
        out = R(*args, **kw)
    assert len(calls) == 1 and calls[0]['importance_u'] is c['u'] and calls[0]['jitter'] is c['jit']
    for x, y in zip(out, base):
        assert torch.equal(x, y)


def _cpu_sample_voxel(self, img_v, seg_v, pts, sigma_only=False, ray_grid=None):
    from dnnlib import util
    out = self.decoder(util.sample_from_triplane(pts, img_v, ray_grid=ray_grid), util.sample_from_triplane(pts, seg_v, ray_grid=ray_grid))
    return out[:, -1] if sigma_only else out
