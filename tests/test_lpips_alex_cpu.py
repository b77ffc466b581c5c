"""The AlexNet LPIPS distance (training/lpips_alex.py) without a GPU: its torch definition against the float64 restatement of
tests/lpips_alex_ref.py (value and image gradient, the unreached row and column, an all-zero tap), the reference class's state-dict names,
the torchvision-key helper in both spellings of the lin keys, the projector closure, `project()` with it, the C ABI of csrc/lpips_alex.hip
and the convolution kernel's plan for every launch of the full net.

Tolerance of the fp32 path against float64 (value: relative error; gradient: relative L2): that of tests/test_lpips_cpu.py, 2e-5, derived
there for 13 layers of dot products of up to 4608 terms; this net has 5 layers of at most 3456 terms, so the bound holds with room."""

import ctypes
import os
import re

import pytest
import torch

import lpips_alex_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 2e-5
NARROW = (8, 12, 16, 12, 12)
CASES = [((2, 3, 32, 32), 0), ((1, 3, 38, 46), 1)]          # (shape, seed)


def _module(widths=NARROW, sd=None):
    from training import lpips_alex
    m = lpips_alex.LPIPS(widths=widths)
    m.load_state_dict(sd if sd is not None else ref.synthetic_state_dict(widths))
    return m


def _value_and_grad(m, x, y):
    leaf = x.clone().requires_grad_(True)
    v = m(leaf, y)
    (g,) = torch.autograd.grad(v, [leaf])
    return v.detach(), g


# ---- the torch definition --------------------------------------------------------------------------------------------------------------------
def test_default_net_type_and_the_others():
    import inspect
    from training import lpips, lpips_alex
    sig = inspect.signature(lpips_alex.LPIPS.__init__)
    assert sig.parameters['net_type'].default == 'alex' and sig.parameters['version'].default == '0.1'
    m = lpips_alex.LPIPS()
    assert isinstance(m.net, lpips_alex.AlexNetFeatures) and m.net.widths == (64, 192, 384, 256, 256)
    assert isinstance(m, lpips.LPIPS)
    with pytest.raises(NotImplementedError, match=r'training\.lpips'):
        lpips_alex.LPIPS('vgg')
    with pytest.raises(NotImplementedError):
        lpips_alex.LPIPS('squeeze')


def test_state_dict_keys_and_order():
    from training import lpips_alex
    m = lpips_alex.LPIPS()
    sd = m.state_dict()
    assert list(sd.keys()) == ref.state_dict_keys()
    assert [tuple(sd[f'net.layers.{i}.weight'].shape) for i in ref.CONV_INDEX] == [(64, 3, 11, 11), (192, 64, 5, 5), (384, 192, 3, 3),
                                                                                  (256, 384, 3, 3), (256, 256, 3, 3)]
    assert [tuple(sd[f'lin.{k}.1.weight'].shape) for k in range(5)] == [(1, c, 1, 1) for c in ref.ALEX]
    assert torch.equal(sd['net.mean'].flatten(), torch.tensor(ref.MEAN)) and torch.equal(sd['net.std'].flatten(), torch.tensor(ref.STD))
    assert tuple(sd['net.mean'].shape) == (1, 3, 1, 1) and tuple(sd['net.std'].shape) == (1, 3, 1, 1)
    assert not any(p.requires_grad for p in m.parameters())
    layers = m.net.layers
    assert len(layers) == 12
    convs = {i: (layers[i].kernel_size, layers[i].stride, layers[i].padding) for i in ref.CONV_INDEX}
    assert convs == {0: ((11, 11), (4, 4), (2, 2)), 3: ((5, 5), (1, 1), (2, 2)), 6: ((3, 3), (1, 1), (1, 1)), 8: ((3, 3), (1, 1), (1, 1)),
                     10: ((3, 3), (1, 1), (1, 1))}
    for i in (2, 5):
        assert isinstance(layers[i], torch.nn.MaxPool2d) and (layers[i].kernel_size, layers[i].stride, layers[i].padding) == (3, 2, 0)
    m.load_state_dict(ref.synthetic_state_dict())          # strict


def test_torchvision_key_helper_takes_both_spellings():
    from training import lpips_alex
    sd = ref.synthetic_state_dict(NARROW)
    features = {k.replace('net.layers.', 'features.'): v for k, v in sd.items() if k.startswith('net.layers.')}
    features['classifier.1.weight'] = torch.zeros(2, 2)           # ignored
    lin = [sd[f'lin.{k}.1.weight'].flatten() for k in range(5)]
    got = lpips_alex.LPIPS(widths=NARROW).load_torchvision_state_dict(features, lin).state_dict()
    assert list(got.keys()) == ref.state_dict_keys()
    assert all(torch.equal(got[k], v) for k, v in sd.items())
    bare = {k.replace('features.', ''): v for k, v in features.items() if k.startswith('features.')}
    file_keys = {f'lin{k}.model.1.weight': sd[f'lin.{k}.1.weight'] for k in range(5)}          # the reference's alex.pth
    got2 = lpips_alex.LPIPS(widths=NARROW).load_torchvision_state_dict(bare, file_keys).state_dict()
    assert all(torch.equal(got2[k], v) for k, v in sd.items())


_reference = {}


def _float64(shape, seed):
    if (shape, seed) not in _reference:
        x, y = ref.images(shape, seed)
        _reference[(shape, seed)] = (x, y) + ref.lpips64_with_grad(ref.synthetic_state_dict(NARROW), x, y)
    return _reference[(shape, seed)]


@pytest.mark.parametrize('shape,seed', CASES)
def test_torch_path_against_float64(shape, seed):
    x, y, want_v, want_g = _float64(shape, seed)
    v, g = _value_and_grad(_module(), x, y)
    assert v.dtype == torch.float32 and v.ndim == 0 and g.shape == x.shape
    ev = abs(float(v) - float(want_v)) / float(want_v)
    eg = float((g.double() - want_g).norm() / want_g.norm())
    print(f'value {float(v):.6f} rel err {ev:.2e}; gradient rel L2 {eg:.2e}')
    assert float(want_v) > 0 and float(want_g.norm()) > 0
    assert ev <= TOL and eg <= TOL


@pytest.mark.parametrize('shape,sizes', [((2, 3, 32, 32), [(7, 7), (3, 3), (1, 1), (1, 1), (1, 1)]),
                                         ((1, 3, 38, 46), [(8, 10), (3, 4), (1, 1), (1, 1), (1, 1)])])
def test_tap_sizes(shape, sizes):
    m = _module()
    feats = m.features(ref.images(shape, 2)[0])
    assert [tuple(t.shape[2:]) for t in feats] == sizes and [t.shape[1] for t in feats] == list(NARROW)
    sd = ref.synthetic_state_dict(NARROW)
    assert [tuple(t.shape[2:]) for t in ref.unit_taps64(sd, ref.images(shape, 2)[0])] == sizes


def test_gradient_is_zero_where_no_stem_window_reaches():
    """38 x 46: 8 x 10 stem windows of 11 at stride 4 behind a padding of 2 read rows -2..36 and columns -2..44."""
    x, y, _, want_g = _float64(*CASES[1])
    _, g = _value_and_grad(_module(), x, y)
    assert float(g[:, :, 37].abs().max()) == 0.0 and float(g[:, :, :, 45].abs().max()) == 0.0
    assert float(want_g[:, :, 37].abs().max()) == 0.0 and float(want_g[:, :, :, 45].abs().max()) == 0.0
    assert float(g[:, :, 36].abs().max()) > 0 and float(g[:, :, :, 44].abs().max()) > 0


def test_all_zero_tap_has_a_finite_gradient():
    """A bias of -1e3 on the third convolution makes tap 3 zero everywhere: its norm is 0 at every pixel (and, behind zero inputs, the later
    taps are constant).  The reference's autograd gives NaN there; here the gradient is finite and equals the float64 closed form."""
    sd = ref.synthetic_state_dict(NARROW, bias_shift={6: -1e3})
    x, y = ref.images((2, 3, 32, 32), 3)
    z = (x.double() - sd['net.mean'].double()) / sd['net.std'].double()
    assert float(ref.taps64(sd, z)[2].abs().max()) == 0.0
    want_v, want_g = ref.lpips64_with_grad(sd, x, y)
    v, g = _value_and_grad(_module(sd=sd), x, y)
    assert bool(torch.isfinite(g).all()) and bool(torch.isfinite(v))
    assert float(want_g.norm()) > 0
    assert abs(float(v) - float(want_v)) <= TOL * float(want_v)
    assert float((g.double() - want_g).norm() / want_g.norm()) <= TOL


# ---- the closure and the routing -------------------------------------------------------------------------------------------------------------
def test_distance_to_cached_features_equals_forward():
    m = _module()
    x, y = ref.images((2, 3, 32, 32), 4)
    feats = m.features(y)
    assert len(feats) == 5 and not any(t.requires_grad for t in feats)
    assert torch.equal(m.distance_to(x, feats), m(x, y))
    assert float(m(y, y)) == 0.0


def test_lpips_distance_down_samples_and_rescales():
    """0..255 images of 64 x 64 against size = 32: the closure equals LPIPS of the 2 x 2 block means mapped to [-1, 1]."""
    from training import lpips
    m = _module()
    g = torch.Generator().manual_seed(5)
    target, img = torch.rand(1, 3, 64, 64, generator=g) * 255, torch.rand(1, 3, 64, 64, generator=g) * 255

    def block_mean(t, f):
        return t.reshape(1, 3, t.shape[2] // f, f, t.shape[3] // f, f).mean(dim=(3, 5))
    d = lpips.lpips_distance(target, m, size=32)
    want = ref.lpips64(ref.synthetic_state_dict(NARROW), block_mean(img, 2) / 127.5 - 1, block_mean(target, 2) / 127.5 - 1)
    assert abs(float(d(img)) - float(want)) <= TOL * float(want)
    leaf = img.clone().requires_grad_(True)
    (gi,) = torch.autograd.grad(d(leaf), [leaf])
    assert gi.shape == img.shape and bool(torch.isfinite(gi).all()) and float(gi.abs().max()) > 0


def test_project_with_lpips_distance_on_cpu_tensors():
    from training import lpips, projection, triplane
    torch.manual_seed(0)
    G = triplane.TriPlaneGenerator(triplane.tiny_spec()).eval()
    c = triplane.camera_label(0.2)
    target = torch.rand(3, G.img_resolution, G.img_resolution, generator=torch.Generator().manual_seed(1)) * 255
    w, info = projection.project(G, target, c, num_steps=3, w_avg_samples=32, return_info=True, distance=lpips.lpips_distance(target[None], _module()))
    assert tuple(w.shape) == (1, G.num_ws, G.w_dim) and bool(torch.isfinite(w).all())
    assert len(info['losses']) == 3 and all(v == v and abs(v) != float('inf') for v in info['losses'])


def test_fused_switch_and_cpu_routing():
    from training import lpips_alex
    assert isinstance(lpips_alex.fused, bool)
    m = _module()
    assert not m._on_hip(torch.zeros(1, 3, 32, 32)), 'CPU tensors take the torch definition'


def test_a_side_below_31_raises_cleanly():
    """31 is the smallest side whose stem output (7) survives two 3x3 stride-2 pools; 30 leaves the second pool a 2 x 2 map.  Every path
    refuses it with the same ValueError instead of ATen's pooling error."""
    m = _module()
    x31, y31 = ref.images((1, 3, 31, 31), 6)
    assert [tuple(t.shape[2:]) for t in m.features(y31)] == [(7, 7), (3, 3), (1, 1), (1, 1), (1, 1)]
    assert bool(torch.isfinite(m(x31, y31)))
    for shape in [(1, 3, 30, 40), (1, 3, 40, 30)]:
        x, y = ref.images(shape, 6)
        with pytest.raises(ValueError, match='at least 31'):
            m.features(y)
        with pytest.raises(ValueError, match='at least 31'):
            m(x, y)


# ---- the C ABI ---------------------------------------------------------------------------------------------------------------------------------
def _header():
    return re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'ide3d_hip.h')).read(), flags=re.S)


SYMBOLS = ('ide3d_unfold2d', 'ide3d_fold2d', 'ide3d_maxpool3s2p0', 'ide3d_lpips_tap_backward')


def test_entry_points_are_declared_listed_and_exported():
    from torch_utils import hip_plugin
    h = re.sub(r'\s+', ' ', _header())
    assert re.search(r'int ide3d_unfold2d\(const float\* x, float\* col, int32_t n, int32_t c, int32_t h, int32_t w, int32_t k, int32_t stride, '
                     r'int32_t pad, void\* stream\);', h)
    assert re.search(r'int ide3d_fold2d\(const float\* dcol, float\* dx, int32_t n, int32_t c, int32_t h, int32_t w, int32_t k, int32_t stride, '
                     r'int32_t pad, void\* stream\);', h)
    assert re.search(r'int ide3d_maxpool3s2p0\(const float\* x, float\* y, uint8_t\* idx, int64_t planes, int32_t h, int32_t w, void\* stream\);', h)
    assert re.search(r'int ide3d_lpips_tap_backward\(const float\* y, const float\* g, const uint8_t\* idx, const float\* dtap, float\* dz, '
                     r'int64_t planes, int32_t h, int32_t w, int32_t pooled, void\* stream\);', h)
    assert hip_plugin._ABI_VERSION == 8
    path = hip_plugin.lib_path()
    assert os.path.isfile(path), f'{path} missing: run __graft_entry__.build()'
    lib = ctypes.CDLL(path)
    for name in SYMBOLS:
        assert name in hip_plugin.EXPORTED_SYMBOLS and hasattr(lib, name), name
    assert lib.ide3d_abi_version() == 8
    assert hip_plugin.PLUGINS['lpips_alex_plugin'] is hip_plugin.LpipsAlexPlugin


def test_argument_checks():
    """Bad arguments are refused with IDE3D_EINVAL (-1) and a text before anything is launched (so a null stream is fine here)."""
    from torch_utils import hip_plugin
    lib = hip_plugin.load()
    err = lib.ide3d_last_error
    for fn, what in ((lib.ide3d_unfold2d, b'unfold2d'), (lib.ide3d_fold2d, b'fold2d')):
        assert fn(None, 8, 1, 3, 32, 32, 11, 4, 2, None) == -1 and b'null pointer' in err() and what in err()
        assert fn(8, None, 1, 3, 32, 32, 11, 4, 2, None) == -1 and b'null pointer' in err()
        assert fn(8, 8, 1, 3, 32, 32, 17, 4, 2, None) == -1 and b'k <= 16' in err()          # k = 17
        assert fn(8, 8, 1, 3, 32, 32, 0, 1, 0, None) == -1
        assert fn(8, 8, 1, 3, 32, 32, 3, 4, 1, None) == -1 and b'stride <= k' in err()       # stride > k
        assert fn(8, 8, 1, 3, 32, 32, 3, 0, 1, None) == -1
        assert fn(8, 8, 1, 3, 32, 32, 3, 1, 3, None) == -1 and b'pad < k' in err()           # pad >= k
        assert fn(8, 8, 1, 3, 32, 32, 3, 1, -1, None) == -1
        assert fn(8, 8, 1, 3, 4, 32, 11, 4, 2, None) == -1                                   # no window: 4 + 4 < 11
        assert fn(8, 8, 1, 3 * 2 ** 12, 2 ** 10, 2 ** 10, 1, 1, 0, None) == -1              # 2^31 * 1.5 elements
        assert fn(8, 8, 0, 3, 32, 32, 3, 1, 1, None) == -1
    assert lib.ide3d_maxpool3s2p0(None, 8, None, 1, 8, 8, None) == -1 and b'null pointer' in err()
    assert lib.ide3d_maxpool3s2p0(8, None, None, 1, 8, 8, None) == -1
    assert lib.ide3d_maxpool3s2p0(8, 8, None, 1, 2, 8, None) == -1 and b'maxpool3s2p0' in err()          # below 3 x 3
    assert lib.ide3d_maxpool3s2p0(8, 8, None, 1, 8, 2, None) == -1
    assert lib.ide3d_maxpool3s2p0(8, 8, None, 0, 8, 8, None) == -1
    tb = lib.ide3d_lpips_tap_backward
    assert tb(None, None, None, 8, 8, 1, 8, 8, 0, None) == -1 and b'null pointer' in err()
    assert tb(8, None, None, None, 8, 1, 8, 8, 0, None) == -1 and tb(8, None, None, 8, None, 1, 8, 8, 0, None) == -1
    assert tb(8, 8, None, 8, 8, 1, 8, 8, 1, None) == -1 and b'winner bytes' in err()          # pooled = 1 with idx == NULL
    assert tb(8, None, 8, 8, 8, 1, 8, 8, 1, None) == -1
    assert tb(8, 8, 8, 8, 8, 1, 2, 8, 1, None) == -1 and b'h, w >= 3' in err()
    assert tb(8, 8, 8, 8, 8, 1, 8, 8, 2, None) == -1
    assert tb(8, 8, 8, 8, 8, 0, 8, 8, 0, None) == -1


# ---- the launch plans --------------------------------------------------------------------------------------------------------------------------
def test_every_alexnet_launch_at_256_has_a_kernel():
    """The five convolutions of the feature net and the five of its input gradient at 256 x 256: the stem and the
    5x5 layer as 1x1 launches over 363 and 1600 patch channels at 63 x 63 and 31 x 31, the 3x3 layers at 15 x 15."""
    from torch_utils import hip_plugin
    launches = [(363, 64, 63, 1), (1600, 192, 31, 1), (192, 384, 15, 3), (384, 256, 15, 3), (256, 256, 15, 3)]          # cin, cout, side, k
    plans = []
    for cin, cout, side, k in launches:
        for n in (1, 4):
            for arith in (6, 1):
                fwd = hip_plugin.modconv_plan(n, cin, cout, side, side, k=k, arith=arith, epilogue='relu')
                bwd = hip_plugin.modconv_plan(n, cout, cin, side, side, k=k, arith=arith, epilogue='grad')
                assert fwd['workgroups'] > 0 and bwd['workgroups'] > 0
                if (n, arith) == (1, 6):
                    plans += [(cin, cout, fwd['kind']), (cout, cin, bwd['kind'])]
    print(plans)
    assert len(plans) == 10
