"""The VGG16 LPIPS distance (training/lpips.py) without a GPU: its torch definition against the float64 restatement of tests/lpips_ref.py
(value and image gradient, an all-zero tap pixel included), the reference class's state-dict names, the torchvision-key helper, the
projector closure, `project()` with it, and the C ABI of csrc/lpips.hip.

Tolerance of the fp32 path against float64 (value: relative error; gradient: relative L2): an fp32 dot product of K <= 4608 terms carries a
relative error of about sqrt(K) * 2^-24 = 4e-6 of the size of its terms, and the value passes 13 such layers, the gradient 26; added as
independent errors that is sqrt(26) * 4e-6 = 2e-5.  (A wrong mask, a dropped pool row or a mis-scaled tap is 1e-2 or more.)"""

import ctypes
import os
import re

import pytest
import torch

import lpips_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 2e-5
NARROW = (16, 32, 64, 64, 64)
CASES = [(NARROW, (2, 3, 32, 32), 0), (NARROW, (1, 3, 40, 24), 1), (lpips_ref.VGG16, (1, 3, 32, 32), 2)]          # (widths, shape, seed)


def _module(widths, sd=None):
    from training import lpips
    m = lpips.LPIPS('vgg', widths=widths)
    m.load_state_dict(sd if sd is not None else lpips_ref.synthetic_state_dict(widths))
    return m


def _value_and_grad(m, x, y):
    leaf = x.clone().requires_grad_(True)
    v = m(leaf, y)
    (g,) = torch.autograd.grad(v, [leaf])
    return v.detach(), g


@pytest.mark.parametrize('widths,shape,seed', CASES)
def test_torch_path_against_float64(widths, shape, seed):
    sd = lpips_ref.synthetic_state_dict(widths)
    x, y = lpips_ref.images(shape, seed)
    want_v, want_g = lpips_ref.lpips64_with_grad(sd, x, y)
    v, g = _value_and_grad(_module(widths, sd), x, y)
    assert v.dtype == torch.float32 and v.ndim == 0 and g.shape == x.shape
    ev = abs(float(v) - float(want_v)) / float(want_v)
    eg = float((g.double() - want_g).norm() / want_g.norm())
    print(f'value {float(v):.6f} rel err {ev:.2e}; gradient rel L2 {eg:.2e}')
    assert float(want_v) > 0 and float(want_g.norm()) > 0
    assert ev <= TOL and eg <= TOL


def test_all_zero_tap_pixel_has_a_finite_gradient():
    """A bias of -1e3 on conv3_3 makes relu3_3 zero everywhere: the norm is 0 at every pixel of that tap (and, behind zero inputs, the later
    taps are constant).  The reference's autograd gives NaN there; here the gradient is finite and equals the float64 closed form."""
    sd = lpips_ref.synthetic_state_dict(NARROW, bias_shift={14: -1e3})
    x, y = lpips_ref.images((2, 3, 32, 32), 3)
    z = (x.double() - sd['net.mean'].double()) / sd['net.std'].double()
    assert float(lpips_ref.taps64(sd, z)[2].abs().max()) == 0.0
    want_v, want_g = lpips_ref.lpips64_with_grad(sd, x, y)
    v, g = _value_and_grad(_module(NARROW, sd), x, y)
    assert bool(torch.isfinite(g).all()) and bool(torch.isfinite(v))
    assert float(want_g.norm()) > 0
    assert abs(float(v) - float(want_v)) <= TOL * float(want_v)
    assert float((g.double() - want_g).norm() / want_g.norm()) <= TOL


def test_normalisation_gradient_is_zero_at_a_zero_pixel():
    from training import lpips
    a = torch.randn(1, 4, 2, 2)
    a[0, :, 0, 1] = 0
    a.requires_grad_(True)
    g = torch.randn(1, 4, 2, 2)
    (da,) = torch.autograd.grad(lpips._Normalize.apply(a), [a], g)
    assert bool(torch.isfinite(da).all())
    assert torch.equal(da[0, :, 0, 1], g[0, :, 0, 1] / lpips.EPS)          # the direct term only
    leaf = a.detach().double().requires_grad_(True)
    (want,) = torch.autograd.grad(lpips_ref._Unit.apply(leaf), [leaf], g.double())
    assert float((da.double() - want).abs().max()) <= 1e-6 * float(want.abs().max())


def test_state_dict_keys_and_order():
    from training import lpips
    m = lpips.LPIPS('vgg')
    assert list(m.state_dict().keys()) == lpips_ref.state_dict_keys()
    sd = m.state_dict()
    assert tuple(sd['net.layers.0.weight'].shape) == (64, 3, 3, 3) and tuple(sd['net.layers.28.weight'].shape) == (512, 512, 3, 3)
    assert [tuple(sd[f'lin.{k}.1.weight'].shape) for k in range(5)] == [(1, c, 1, 1) for c in (64, 128, 256, 512, 512)]
    assert tuple(sd['net.mean'].shape) == (1, 3, 1, 1) and tuple(sd['net.std'].shape) == (1, 3, 1, 1)
    assert torch.equal(sd['net.mean'].flatten(), torch.tensor(lpips_ref.MEAN)) and torch.equal(sd['net.std'].flatten(), torch.tensor(lpips_ref.STD))
    assert not any(p.requires_grad for p in m.parameters())
    m.load_state_dict(lpips_ref.synthetic_state_dict())          # strict


def test_torchvision_key_helper_round_trips():
    from training import lpips
    sd = lpips_ref.synthetic_state_dict(NARROW)
    features = {k.replace('net.layers.', 'features.'): v for k, v in sd.items() if k.startswith('net.layers.')}
    features['classifier.0.weight'] = torch.zeros(2, 2)           # ignored
    lin = [sd[f'lin.{k}.1.weight'].flatten() for k in range(5)]
    m = lpips.LPIPS('vgg', widths=NARROW).load_torchvision_state_dict(features, lin)
    got = m.state_dict()
    assert list(got.keys()) == lpips_ref.state_dict_keys()
    for k, v in sd.items():
        assert torch.equal(got[k], v), k
    bare = {k.replace('features.', ''): v for k, v in features.items() if k.startswith('features.')}
    m2 = lpips.LPIPS('vgg', widths=NARROW).load_torchvision_state_dict(bare, [w.reshape(1, -1, 1, 1) for w in lin])
    assert all(torch.equal(m2.state_dict()[k], v) for k, v in sd.items())


@pytest.mark.parametrize('net_type', ['alex', 'squeeze'])
def test_other_nets_raise_with_the_reason(net_type):
    from training import lpips
    with pytest.raises(NotImplementedError, match='11x11, 5x5 and strided'):
        lpips.LPIPS(net_type)


def test_distance_to_cached_features_equals_forward():
    m = _module(NARROW)
    x, y = lpips_ref.images((2, 3, 32, 32), 4)
    feats = m.features(y)
    assert len(feats) == 5 and not any(t.requires_grad for t in feats)
    assert [t.shape[1] for t in feats] == list(NARROW) and [t.shape[2] for t in feats] == [32, 16, 8, 4, 2]
    assert torch.equal(m.distance_to(x, feats), m(x, y))
    assert float(m(y, y)) == 0.0


def test_lpips_distance_down_samples_and_rescales():
    """0..255 images of 64 x 64 against size = 32: the closure equals LPIPS of the 2 x 2 block means mapped to [-1, 1]; an image at or below
    `size` is only rescaled; a non-integer factor is resized by area interpolation."""
    from training import lpips
    m = _module(NARROW)
    g = torch.Generator().manual_seed(5)
    target, img = torch.rand(1, 3, 64, 64, generator=g) * 255, torch.rand(1, 3, 64, 64, generator=g) * 255

    def block_mean(t, f):
        return t.reshape(1, 3, t.shape[2] // f, f, t.shape[3] // f, f).mean(dim=(3, 5))
    d = lpips.lpips_distance(target, m, size=32)
    want = lpips_ref.lpips64(lpips_ref.synthetic_state_dict(NARROW), block_mean(img, 2) / 127.5 - 1, block_mean(target, 2) / 127.5 - 1)
    assert abs(float(d(img)) - float(want)) <= TOL * float(want)
    d64 = lpips.lpips_distance(target, m, size=64)
    assert abs(float(d64(img)) - float(m(img / 127.5 - 1, target / 127.5 - 1))) <= 1e-6 * float(d64(img))
    d48 = lpips.lpips_distance(target, m, size=48)
    small = lambda t: torch.nn.functional.interpolate(t, size=(48, 48), mode='area') / 127.5 - 1
    assert abs(float(d48(img)) - float(m(small(img), small(target)))) <= 1e-6 * float(d48(img))
    leaf = img.clone().requires_grad_(True)
    (gi,) = torch.autograd.grad(d(leaf), [leaf])
    assert gi.shape == img.shape and bool(torch.isfinite(gi).all()) and float(gi.abs().max()) > 0


def test_project_with_lpips_distance_on_cpu_tensors():
    from training import lpips, projection, triplane
    torch.manual_seed(0)
    G = triplane.TriPlaneGenerator(triplane.tiny_spec()).eval()
    c = triplane.camera_label(0.2)
    target = torch.rand(3, G.img_resolution, G.img_resolution, generator=torch.Generator().manual_seed(1)) * 255
    m = _module(NARROW)
    w, info = projection.project(G, target, c, num_steps=3, w_avg_samples=32, return_info=True, distance=lpips.lpips_distance(target[None], m))
    assert tuple(w.shape) == (1, G.num_ws, G.w_dim) and bool(torch.isfinite(w).all())
    assert len(info['losses']) == 3 and all(v == v and abs(v) != float('inf') for v in info['losses'])


def test_fused_switch_and_cpu_routing():
    from training import lpips
    assert isinstance(lpips.fused, bool)
    m = _module(NARROW)
    assert not m._on_hip(torch.zeros(1, 3, 32, 32)), 'CPU tensors take the torch definition'


# ---- the C ABI ---------------------------------------------------------------------------------------------------------------------------------
def _header():
    return re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'ide3d_hip.h')).read(), flags=re.S)


SYMBOLS = ('ide3d_lpips_prep', 'ide3d_lpips_prep_backward', 'ide3d_maxpool2', 'ide3d_lpips_stage_backward', 'ide3d_lpips_head_workspace_bytes',
           'ide3d_lpips_head', 'ide3d_lpips_head_backward')


def test_entry_points_are_declared_listed_and_exported():
    from torch_utils import hip_plugin
    h = re.sub(r'\s+', ' ', _header())
    assert re.search(r'int ide3d_lpips_prep\(const float\* x, float\* y, const float\* mean, const float\* std_, int32_t n, int32_t H, int32_t W, '
                     r'int32_t f, float in_scale, float in_shift, void\* stream\);', h)
    assert re.search(r'int ide3d_lpips_prep_backward\(const float\* dy, float\* dx, const float\* std_, int32_t n, int32_t H, int32_t W, int32_t f, '
                     r'float in_scale, void\* stream\);', h)
    assert re.search(r'int ide3d_maxpool2\(const float\* x, float\* y, int64_t planes, int32_t h, int32_t w, void\* stream\);', h)
    assert re.search(r'int ide3d_lpips_stage_backward\(const float\* y, const float\* dpool, const float\* dtap, float\* dz, int64_t planes, '
                     r'int32_t h, int32_t w, void\* stream\);', h)
    assert re.search(r'int64_t ide3d_lpips_head_workspace_bytes\(const ide3d_lpips_tap\* taps, int32_t k, int32_t n\);', h)
    assert re.search(r'int ide3d_lpips_head\(const ide3d_lpips_tap\* taps, int32_t k, int32_t n, float\* workspace, int64_t workspace_bytes, '
                     r'float\* loss, void\* stream\);', h)
    assert re.search(r'int ide3d_lpips_head_backward\(const ide3d_lpips_tap\* taps, int32_t k, int32_t n, const float\* dloss, void\* stream\);', h)
    assert hip_plugin._ABI_VERSION == 8
    path = hip_plugin.lib_path()
    assert os.path.isfile(path), f'{path} missing: run __graft_entry__.build()'
    lib = ctypes.CDLL(path)
    for name in SYMBOLS:
        assert name in hip_plugin.EXPORTED_SYMBOLS and hasattr(lib, name), name
    assert lib.ide3d_abi_version() == 8
    assert hip_plugin.PLUGINS['lpips_plugin'] is hip_plugin.LpipsPlugin


def test_tap_struct_matches_header():
    from torch_utils import hip_plugin
    body = re.search(r'typedef struct ide3d_lpips_tap \{(.*?)\} ide3d_lpips_tap;', _header(), re.S).group(1)
    names = [n for d in body.split(';') if d.strip() for n in re.findall(r'([A-Za-z_][A-Za-z0-9_]*)\s*(?:,|$)', d.strip())]
    cls = hip_plugin._LpipsTap
    assert names == [f[0] for f in cls._fields_] == ['a', 't', 'lin', 'out', 'c', 'h', 'w', 'reserved']
    assert ctypes.sizeof(cls) == 48 and cls.c.offset == 32 and cls.reserved.offset == 44
    assert int(re.search(r'#define IDE3D_LPIPS_MAX_TAPS (\d+)', _header()).group(1)) == hip_plugin.LPIPS_MAX_TAPS


def test_workspace_query_and_argument_checks():
    """8 bytes per head workgroup of 64 pixels, summed over the taps; bad arguments are refused before anything is launched."""
    from torch_utils import hip_plugin
    lib = hip_plugin.load()
    taps = (hip_plugin._LpipsTap * 2)()
    taps[0].c, taps[0].h, taps[0].w = 64, 256, 256
    taps[1].c, taps[1].h, taps[1].w = 512, 5, 3
    assert lib.ide3d_lpips_head_workspace_bytes(taps, 2, 4) == (4 * 65536 // 64 + 1) * 8
    assert lib.ide3d_lpips_head_workspace_bytes(taps, 1, 1) == 1024 * 8
    assert lib.ide3d_lpips_head_workspace_bytes(taps, 9, 1) == -1 and lib.ide3d_lpips_head_workspace_bytes(None, 1, 1) == -1
    taps[1].w = 0
    assert lib.ide3d_lpips_head_workspace_bytes(taps, 2, 1) == -1
    assert lib.ide3d_lpips_head(taps, 2, 1, None, 0, None, None) == -1          # IDE3D_EINVAL
    assert lib.ide3d_lpips_prep(None, None, None, None, 1, 8, 8, 1, 1.0, 0.0, None) == -1
    assert b'null pointer' in lib.ide3d_last_error()
    assert lib.ide3d_lpips_prep(8, 8, 8, 8, 1, 8, 12, 3, 1.0, 0.0, None) == -1 and b'area factor' in lib.ide3d_last_error()
    assert lib.ide3d_maxpool2(8, 8, 1, 1, 4, None) == -1
    assert lib.ide3d_lpips_stage_backward(8, 8, 8, 8, 1, 1, 4, None) == -1 and b'pooled gradient' in lib.ide3d_last_error()


def test_every_vgg16_launch_at_256_has_a_kernel():
    """The 13 convolutions of the feature net and the 13 of its input gradient at 256 x 256: conv1_1 (cin 3) and
    its gradient (cout 3) take the exact-fp32 family, everything else the split-bf16 family of the default arithmetic."""
    from torch_utils import hip_plugin
    cin, side, plans = 3, 256, []
    for s, (count, cout) in enumerate(zip(lpips_ref.STAGES, lpips_ref.VGG16)):
        if s > 0:
            side //= 2
        for _ in range(count):
            for n in (1, 4):
                for arith in (6, 1):
                    fwd = hip_plugin.modconv_plan(n, cin, cout, side, side, arith=arith, epilogue='relu')
                    bwd = hip_plugin.modconv_plan(n, cout, cin, side, side, arith=arith, epilogue='grad')
                    assert fwd['workgroups'] > 0 and bwd['workgroups'] > 0
                    if (n, arith) == (1, 6):
                        plans += [(cin, cout, fwd['kind']), (cout, cin, bwd['kind'])]
            cin = cout
    assert len(plans) == 26
    assert plans[0] == (3, 64, 'fp32') and plans[1] == (64, 3, 'fp32')
