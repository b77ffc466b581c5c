"""The VGG19 feature loss (training/vgg_loss.py) without a GPU: its torch definition against the float64 restatement of
tests/vgg_loss_ref.py (value and image gradient), the reference class's state-dict names, the torchvision-key helper, `n_layers`, the
smallest side, the closure, the C ABI of csrc/vgg_loss.hip, the convolution kernel's plan for every launch of the full net, and the kink
margin of the end-to-end cases that test_gpu_vgg_loss.py runs.

Tolerance of the fp32 path against float64 (value: relative error; gradient: relative L2): that of tests/test_lpips_alex_cpu.py and
tests/test_lpips_cpu.py, 2e-5, derived there for 13 layers of dot products of up to 4608 terms, which is this net's depth and width.  It
is a bound on rounding only because the inputs keep away from the kinks of ReLU and |.| (test_kink_margin_of_the_end_to_end_cases)."""

import ctypes
import os
import re

import pytest
import torch

import vgg_loss_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 2e-5
NARROW = ref.NARROW


def _module(widths=NARROW, n_layers=5, sd=None):
    from training import vgg_loss
    m = vgg_loss.VGGLoss(None, n_layers, widths)
    m.load_state_dict(sd if sd is not None else ref.synthetic_state_dict(widths, 0, n_layers))
    return m


def _value_and_grad(m, x, y):
    leaf = x.clone().requires_grad_(True)
    v = m(leaf, y)
    (g,) = torch.autograd.grad(v, [leaf])
    return v.detach(), g


# ---- the torch definition --------------------------------------------------------------------------------------------------------------------
def test_state_dict_keys_and_layout():
    from training import vgg_loss
    want = ['layers.0.0', 'layers.1.2', 'layers.1.5', 'layers.2.7', 'layers.2.10', 'layers.3.12', 'layers.3.14', 'layers.3.16', 'layers.3.19',
            'layers.4.21', 'layers.4.23', 'layers.4.25', 'layers.4.28']
    want = [f'{k}.{n}' for k in want for n in ('weight', 'bias')]
    assert ref.state_dict_keys() == want
    for m in (vgg_loss.VGG19Features(), vgg_loss.VGGLoss()):
        sd = m.state_dict()
        assert list(sd.keys()) == want
        assert [tuple(sd[k].shape) for k in want if k.endswith('weight')] == [
            (64, 3, 3, 3), (64, 64, 3, 3), (128, 64, 3, 3), (128, 128, 3, 3), (256, 128, 3, 3), (256, 256, 3, 3), (256, 256, 3, 3), (256, 256, 3, 3),
            (512, 256, 3, 3), (512, 512, 3, 3), (512, 512, 3, 3), (512, 512, 3, 3), (512, 512, 3, 3)]
        assert not any(p.requires_grad for p in m.parameters())
        assert [len(s) for s in m.layers] == [2, 5, 5, 9, 9]
        for s, piece in enumerate(m.layers):
            for name, mod in piece.named_children():
                i = int(name)
                if i in vgg_loss.CONV_INDEX:
                    assert isinstance(mod, torch.nn.Conv2d) and (mod.kernel_size, mod.stride, mod.padding) == ((3, 3), (1, 1), (1, 1))
                elif i in (4, 9, 18, 27):
                    assert isinstance(mod, torch.nn.MaxPool2d) and (mod.kernel_size, mod.stride, mod.padding) == (2, 2, 0)
                else:
                    assert isinstance(mod, torch.nn.ReLU)
        m.load_state_dict(ref.synthetic_state_dict())          # strict
    m = vgg_loss.VGGLoss()
    assert m.weights == (1.0, 1.0, 1.0, 1.0, 1.0) and isinstance(m.layers, torch.nn.ModuleList) and m.widths == (64, 128, 256, 512, 512)


def test_torchvision_key_helper_round_trips():
    from training import vgg_loss
    sd = ref.synthetic_state_dict(NARROW)
    features = {'features.' + k.split('.', 2)[2]: v for k, v in sd.items()}
    assert 'features.28.weight' in features and 'features.0.bias' in features
    features['classifier.0.weight'] = torch.zeros(2, 2)           # ignored
    features['features.30.weight'] = torch.zeros(2, 2)            # behind the last slice: ignored
    got = vgg_loss.VGGLoss(widths=NARROW).load_torchvision_state_dict(features).state_dict()
    assert list(got.keys()) == ref.state_dict_keys() and all(torch.equal(got[k], v) for k, v in sd.items())
    bare = {k.replace('features.', ''): v for k, v in features.items() if k.startswith('features.')}
    got2 = vgg_loss.VGGLoss(widths=NARROW).load_torchvision_state_dict(bare).state_dict()
    assert all(torch.equal(got2[k], v) for k, v in sd.items())
    got3 = vgg_loss.VGGLoss(n_layers=2, widths=NARROW).load_torchvision_state_dict(features).state_dict()
    assert list(got3.keys()) == ref.state_dict_keys(2) and all(torch.equal(v, sd[k]) for k, v in got3.items())


_reference = {}


def _float64(widths, n_layers, shape, seed):
    key = (widths, n_layers, shape, seed)
    if key not in _reference:
        x, y = ref.images(shape, seed)
        _reference[key] = (x, y) + ref.vgg64_with_grad(ref.synthetic_state_dict(widths, 0, n_layers), x, y, n_layers)
    return _reference[key]


@pytest.mark.parametrize('widths,n_layers,shape,seed', ref.E2E_CASES)
def test_torch_path_against_float64(widths, n_layers, shape, seed):
    x, y, want_v, want_g = _float64(widths, n_layers, shape, seed)
    v, g = _value_and_grad(_module(widths, n_layers), x, y)
    assert v.dtype == torch.float32 and v.ndim == 0 and g.shape == x.shape
    ev = abs(float(v) - float(want_v)) / float(want_v)
    eg = float((g.double() - want_g).norm() / want_g.norm())
    print(f'value {float(v):.6f} rel err {ev:.2e}; gradient rel L2 {eg:.2e}')
    assert float(want_v) > 0 and float(want_g.norm()) > 0
    assert ev <= TOL and eg <= TOL


@pytest.mark.parametrize('widths,n_layers,shape,seed', ref.E2E_CASES)
def test_kink_margin_of_the_end_to_end_cases(widths, n_layers, shape, seed):
    """ReLU, |.| and the winner of a 2x2 maximum are not differentiable where two arguments meet: one fp32-versus-float64 sign flip or
    winner switch moves the gradient by orders of magnitude more than rounding does (a single switched winner of the third pool: 1.4e-2
    relative L2 of the image gradient at [2, 3, 32, 32]).  So for the image that is differentiated every end-to-end case keeps, in float64,
      - every pre-activation of every convolution,
      - the gap between the two largest values of every pool window with a positive maximum,
      - every non-zero tap difference a - t
    further from 0 than m_l = 8 x the largest error of the fp32 CPU ATen evaluation of that layer against float64 on the same inputs (the
    factor 8: room for another accumulation order; vgg_loss_ref.kink_margins says why the target's own kinks do not count).  The seeds
    were searched until this holds; it is a condition on the inputs that the reference alone satisfies, not a tolerance on the code under
    test.  Margins: DESIGN.md section 5.22."""
    x, y = ref.images(shape, seed)
    km = ref.kink_margins(ref.synthetic_state_dict(widths, 0, n_layers), x, y, n_layers)
    assert len(km['conv']) == len(ref.convs_of(n_layers)) and len(km['tap']) == n_layers and len(km['pool']) == min(n_layers, 5) - 1
    for kind in ('conv', 'pool', 'tap'):
        print(f'{kind:4s} m_l / closest:', ' '.join(f'{m:.1e}/{v:.1e}' for m, v in km[kind]))
        for l, (m, v) in enumerate(km[kind]):
            assert 0 < m < 1e-3 and v > m, f'{kind} {l}: the closest approach to a kink, {v:.2e}, lies within m_l = {m:.2e}'


def test_tap_sizes_and_dropped_row_and_column():
    """[1, 3, 40, 24]: sides 40 -> 20 -> 10 -> 5 -> 2 and 24 -> 12 -> 6 -> 3 -> 1: the last pools drop a row and a column."""
    m = _module()
    feats = m.features(ref.images((1, 3, 40, 24), 1)[0])
    assert [tuple(t.shape[1:]) for t in feats] == [(16, 40, 24), (32, 20, 12), (64, 10, 6), (64, 5, 3), (64, 2, 1)]
    assert not any(t.requires_grad for t in feats)


def test_n_layers_truncates():
    from training import vgg_loss
    sd5 = ref.synthetic_state_dict(NARROW)
    x, y = ref.images((1, 3, 16, 16), 2)
    for n_layers in (1, 2, 3, 4):
        m = _module(NARROW, n_layers)
        assert len(m.layers) == n_layers and list(m.state_dict().keys()) == ref.state_dict_keys(n_layers)
        assert all(torch.equal(v, sd5[k]) for k, v in m.state_dict().items())
        assert len(m.features(y)) == n_layers
        want = ref.vgg64(sd5, x, y, n_layers)
        assert abs(float(m(x, y)) - float(want)) <= TOL * float(want)
    full = float(_module()(x, y))
    assert float(_module(NARROW, 4)(x, y)) < full
    with pytest.raises(AssertionError):
        vgg_loss.VGGLoss(n_layers=6)
    with pytest.raises(AssertionError):
        vgg_loss.VGGLoss(n_layers=0)


def test_a_side_below_16_raises_cleanly():
    m = _module()
    x16, y16 = ref.images((1, 3, 16, 16), 3)
    assert [tuple(t.shape[2:]) for t in m.features(y16)] == [(16, 16), (8, 8), (4, 4), (2, 2), (1, 1)]
    assert bool(torch.isfinite(m(x16, y16)))
    for shape in [(1, 3, 15, 20), (1, 3, 20, 15)]:
        x, y = ref.images(shape, 3)
        with pytest.raises(ValueError, match='at least 16'):
            m.features(y)
        with pytest.raises(ValueError, match='at least 16'):
            m(x, y)
        with pytest.raises(ValueError, match='at least 16'):
            m.distance_to(x, m.features(y16))
    with pytest.raises(ValueError, match='at least 16'):
        _module(NARROW, 2)(*ref.images((1, 3, 15, 15), 3))          # every path, whatever n_layers


# ---- the closure and the routing -------------------------------------------------------------------------------------------------------------
def test_distance_to_cached_features_equals_forward():
    m = _module()
    x, y = ref.images((2, 3, 32, 32), 4)
    feats = m.features(y)
    assert len(feats) == 5 and not any(t.requires_grad for t in feats)
    assert torch.equal(m.distance_to(x, feats), m(x, y))
    assert float(m(y, y)) == 0.0


def test_vgg_distance_rescales_weighs_and_adds_the_base():
    from training import vgg_loss
    m = _module()
    g = torch.Generator().manual_seed(5)
    target, img = torch.rand(1, 3, 32, 32, generator=g) * 255, torch.rand(1, 3, 32, 32, generator=g) * 255
    want = ref.vgg64(ref.synthetic_state_dict(NARROW), img / 127.5 - 1, target / 127.5 - 1)
    d = vgg_loss.vgg_distance(target, m, weight=0.5, base=lambda images: images.mean() * 0 + 3.0)
    assert abs(float(d(img)) - (0.5 * float(want) + 3.0)) <= TOL * (0.5 * float(want) + 3.0)
    leaf = img.clone().requires_grad_(True)
    (gi,) = torch.autograd.grad(vgg_loss.vgg_distance(target, m)(leaf), [leaf])
    assert gi.shape == img.shape and bool(torch.isfinite(gi).all()) and float(gi.abs().max()) > 0


def test_project_with_vgg_distance_on_cpu_tensors():
    from training import projection, triplane, vgg_loss
    torch.manual_seed(0)
    G = triplane.TriPlaneGenerator(triplane.tiny_spec()).eval()
    c = triplane.camera_label(0.2)
    target = torch.rand(3, G.img_resolution, G.img_resolution, generator=torch.Generator().manual_seed(1)) * 255
    # without the w noise and the noise regulariser the step loss is the distance alone (the first step runs at learning rate 0)
    w, info = projection.project(G, target, c, num_steps=5, w_avg_samples=32, return_info=True, initial_noise_factor=0.0, regularize_noise_weight=0.0,
                                 distance=vgg_loss.vgg_distance(target[None], _module()))
    assert tuple(w.shape) == (1, G.num_ws, G.w_dim) and bool(torch.isfinite(w).all())
    losses = info['losses']
    assert len(losses) == 5 and all(v == v and abs(v) != float('inf') for v in losses) and losses[-1] < losses[0], losses


def test_fused_switch_and_cpu_routing():
    from training import vgg_loss
    assert isinstance(vgg_loss.fused, bool)
    old, vgg_loss.fused = vgg_loss.fused, True
    try:
        assert not _module()._on_hip(torch.zeros(1, 3, 32, 32)), 'CPU tensors take the torch definition'
    finally:
        vgg_loss.fused = old


# ---- the C ABI ---------------------------------------------------------------------------------------------------------------------------------
def _header():
    return re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'ide3d_hip.h')).read(), flags=re.S)


SYMBOLS = ('ide3d_feat_l1_workspace_bytes', 'ide3d_feat_l1', 'ide3d_feat_l1_tap_backward', 'ide3d_maxpool2_relu_backward')


def test_entry_points_are_declared_listed_and_exported():
    from torch_utils import hip_plugin
    h = re.sub(r'\s+', ' ', _header())
    assert re.search(r'int64_t ide3d_feat_l1_workspace_bytes\(const ide3d_feat_l1_tap\* taps, int32_t k, int32_t n\);', h)
    assert re.search(r'int ide3d_feat_l1\(const ide3d_feat_l1_tap\* taps, int32_t k, int32_t n, float\* workspace, int64_t workspace_bytes, '
                     r'float\* loss, void\* stream\);', h)
    assert re.search(r'int ide3d_feat_l1_tap_backward\(const float\* a, const float\* t, const float\* g, float\* dz, const float\* dloss, '
                     r'float weight, int64_t planes, int32_t h, int32_t w, int64_t count, void\* stream\);', h)
    assert re.search(r'int ide3d_maxpool2_relu_backward\(const float\* y, const float\* dpool, float\* dz, int64_t planes, int32_t h, int32_t w, '
                     r'void\* stream\);', h)
    assert ctypes.sizeof(hip_plugin._FeatL1Tap) == 32
    assert hip_plugin._ABI_VERSION == 8
    path = hip_plugin.lib_path()
    assert os.path.isfile(path), f'{path} missing: run __graft_entry__.build()'
    lib = ctypes.CDLL(path)
    for name in SYMBOLS:
        assert name in hip_plugin.EXPORTED_SYMBOLS and hasattr(lib, name), name
    assert lib.ide3d_abi_version() == 8
    assert hip_plugin.PLUGINS['vgg_loss_plugin'] is hip_plugin.VggLossPlugin


def test_argument_checks():
    """Bad arguments are refused with IDE3D_EINVAL (-1) and a text before anything is launched (so a null stream is fine here)."""
    from torch_utils import hip_plugin
    lib = hip_plugin.load()
    err = lib.ide3d_last_error
    tb = lib.ide3d_feat_l1_tap_backward
    assert tb(None, 8, None, 8, 8, 1.0, 1, 8, 8, 64, None) == -1 and b'null pointer' in err() and b'feat_l1_tap_backward' in err()
    assert tb(8, None, None, 8, 8, 1.0, 1, 8, 8, 64, None) == -1 and tb(8, 8, None, None, 8, 1.0, 1, 8, 8, 64, None) == -1
    assert tb(8, 8, None, 8, None, 1.0, 1, 8, 8, 64, None) == -1                       # dloss is a device pointer, never NULL
    assert tb(8, 8, None, 8, 8, 1.0, 0, 8, 8, 64, None) == -1 and tb(8, 8, None, 8, 8, 1.0, 1, 0, 8, 64, None) == -1
    assert tb(8, 8, None, 8, 8, 1.0, 1, 8, 8, 0, None) == -1 and b'count' in err()
    pb = lib.ide3d_maxpool2_relu_backward
    assert pb(None, 8, 8, 1, 8, 8, None) == -1 and b'null pointer' in err() and b'maxpool2_relu_backward' in err()
    assert pb(8, None, 8, 1, 8, 8, None) == -1 and pb(8, 8, None, 1, 8, 8, None) == -1          # no form without a pooled gradient
    assert pb(8, 8, 8, 1, 1, 8, None) == -1 and b'h, w >= 2' in err()
    assert pb(8, 8, 8, 1, 8, 1, None) == -1 and pb(8, 8, 8, 0, 8, 8, None) == -1
    taps = (hip_plugin._FeatL1Tap * 9)()
    for t in taps:
        t.a, t.t, t.weight, t.c, t.h, t.w = 8, 8, 1.0, 4, 4, 4
    assert lib.ide3d_feat_l1_workspace_bytes(taps, 2, 3) == 2 * 8                               # one workgroup per tap of 192 elements
    assert lib.ide3d_feat_l1_workspace_bytes(taps, 9, 1) == -1 and lib.ide3d_feat_l1_workspace_bytes(taps, 0, 1) == -1
    assert lib.ide3d_feat_l1_workspace_bytes(taps, 1, 0) == -1 and lib.ide3d_feat_l1_workspace_bytes(None, 1, 1) == -1
    assert lib.ide3d_feat_l1(taps, 9, 1, 8, 1 << 20, 8, None) == -1 and b'feat_l1' in err()
    assert lib.ide3d_feat_l1(taps, 2, 3, 8, 8, 8, None) == -1 and b'workspace too small' in err()
    assert lib.ide3d_feat_l1(taps, 2, 3, None, 16, 8, None) == -1
    assert lib.ide3d_feat_l1(taps, 2, 3, 8, 16, None, None) == -1 and b'null loss' in err()
    taps[1].t = None
    assert lib.ide3d_feat_l1(taps, 2, 3, 8, 16, 8, None) == -1 and b'a and t' in err()
    taps[1].t, taps[1].c = 8, 0
    assert lib.ide3d_feat_l1_workspace_bytes(taps, 2, 3) == -1


# ---- the launch plans --------------------------------------------------------------------------------------------------------------------------
def test_every_vgg19_launch_has_a_kernel():
    """The 13 convolutions of the feature net and the 13 of its input gradient at 256 x 256 and 512 x 512, batch 1 and 4, in the default
    split-bf16 arithmetic (6) and in fp32 (1): conv1_1 (cin 3) and its gradient (cout 3) take the exact-fp32
    family, as in VGG16 (tests/test_lpips_cpu.py)."""
    from torch_utils import hip_plugin
    for size in (256, 512):
        cin, side, plans = 3, size, []
        for s, (count, cout) in enumerate(zip(ref.STAGES, ref.VGG19)):
            if s > 0:
                side //= 2
            for _ in range(count):
                for n in (1, 4):
                    for arith in (6, 1):
                        fwd = hip_plugin.modconv_plan(n, cin, cout, side, side, arith=arith, epilogue='relu')
                        bwd = hip_plugin.modconv_plan(n, cout, cin, side, side, arith=arith, epilogue='grad')
                        assert fwd['workgroups'] > 0 and bwd['workgroups'] > 0
                        if (n, arith) == (1, 6):
                            plans += [(cin, cout, side, fwd['kind']), (cout, cin, side, bwd['kind'])]
                cin = cout
        print(size, plans)
        assert len(plans) == 26 and side == size // 16
        assert plans[0] == (3, 64, size, 'fp32') and plans[1] == (64, 3, size, 'fp32')
