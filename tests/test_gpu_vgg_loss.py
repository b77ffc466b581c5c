"""The VGG19 feature loss on the GPU (training/vgg_loss.py over csrc/vgg_loss.hip, csrc/lpips.hip, csrc/modconv.hip): the three new passes
against ATen bit for bit or against a float64 sum, the prep identity, the whole loss and its image gradient against float64 beside the
module's own fp32 ATen path, the routing rules with the launch count, and `project()` with the closure."""

import contextlib

import pytest
import torch
import torch.nn.functional as F

import vgg_loss_ref as ref

pytestmark = pytest.mark.gpu

NARROW = ref.NARROW
# [planes, h, w]: the smallest window; an even map; odd sides (a dropped row and a dropped column); another odd height; the 16-byte form;
# more than one workgroup with an odd height in the 16-byte form
SHAPES = [(1, 2, 2), (2, 4, 4), (3, 5, 7), (5, 9, 6), (2, 8, 8), (3, 33, 68)]


@contextlib.contextmanager
def _fused(on):
    from training import vgg_loss
    old, vgg_loss.fused = vgg_loss.fused, on
    try:
        yield
    finally:
        vgg_loss.fused = old


def _plugin(gpu_device):
    from torch_utils import hip_plugin
    hip_plugin.load()
    return hip_plugin.VggLossPlugin


def _rand(shape, seed, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


# ---- the streaming passes ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('shape', SHAPES)
def test_maxpool2_relu_backward_is_bit_equal_to_autograd(gpu_device, shape):
    """y = relu(randn): about half of the entries are exact zeros, so windows with several zeros and all-zero windows occur."""
    V = _plugin(gpu_device)
    planes, h, w = shape
    y = F.relu(_rand((1, planes, h, w), 1)).to(gpu_device)
    dpool = _rand((1, planes, h // 2, w // 2), 2).to(gpu_device)
    leaf = y.clone().requires_grad_(True)
    (routed,) = torch.autograd.grad(F.max_pool2d(leaf, 2), [leaf], dpool)
    want = routed * (y > 0)
    from torch_utils import hip_plugin
    dz = torch.full_like(y, float('nan'))                                  # through the C entry point, into a NaN-filled result
    rc = hip_plugin.load().ide3d_maxpool2_relu_backward(hip_plugin._ptr(y), hip_plugin._ptr(dpool), hip_plugin._ptr(dz), planes, h, w,
                                                        hip_plugin._stream(y))
    assert rc == 0 and bool(torch.isfinite(dz).all()), 'an element was not written'
    assert torch.equal(dz, want)
    assert torch.equal(V.maxpool2_relu_backward(y, dpool), dz)
    assert bool((dz[y == 0] == 0).all()) and int((dz != 0).sum()) > 0
    if h % 2:
        assert float(dz[:, :, h - 1].abs().max()) == 0.0 and float(y[:, :, h - 1].max()) > 0
    if w % 2:
        assert float(dz[:, :, :, w - 1].abs().max()) == 0.0 and float(y[:, :, :, w - 1].max()) > 0


@pytest.mark.parametrize('with_g', [True, False])
@pytest.mark.parametrize('shape', SHAPES)
def test_feat_l1_tap_backward_is_bit_equal(gpu_device, shape, with_g):
    """dz = where(a > 0, g + s32 sign(a - t), 0), s32 = fp32(double(dloss) * weight / count), with the planted entries a == t > 0 (sign 0),
    a = 0 < t, a = t = 0 and a = -0.0 (masked), a dloss other than 1 and a weight other than 1."""
    V = _plugin(gpu_device)
    planes, h, w = shape
    a, t = F.relu(_rand((1, planes, h, w), 3)), F.relu(_rand((1, planes, h, w), 4))
    fa, ft = a.view(-1), t.view(-1)
    fa[0], ft[0] = 0.75, 0.75            # a == t > 0
    fa[1], ft[1] = 0.0, 0.5              # a = 0 < t
    fa[2], ft[2] = 0.0, 0.0              # a = t = 0
    fa[3], ft[3] = -0.0, 0.25            # a = -0.0
    g = _rand((1, planes, h, w), 5) if with_g else None
    dloss, weight, count = torch.tensor(0.37), 1.5, 7 * a.numel()          # (count is the caller's: not tied to the shape)
    s32 = torch.tensor(float(dloss.double()) * weight / count, dtype=torch.float32).to(gpu_device)
    ad, td, gd = a.to(gpu_device), t.to(gpu_device), (g.to(gpu_device) if with_g else None)
    term = s32 * torch.sign(ad - td)
    want = torch.where(ad > 0, gd + term if with_g else term, torch.zeros_like(ad))
    from torch_utils import hip_plugin
    dz = torch.full_like(ad, float('nan'))
    dl = dloss.to(gpu_device)
    rc = hip_plugin.load().ide3d_feat_l1_tap_backward(hip_plugin._ptr(ad), hip_plugin._ptr(td), hip_plugin._ptr(gd), hip_plugin._ptr(dz),
                                                      hip_plugin._ptr(dl), weight, planes, h, w, count, hip_plugin._stream(ad))
    assert rc == 0 and bool(torch.isfinite(dz).all()), 'an element was not written'
    assert torch.equal(dz, want)
    flat = dz.view(-1).cpu()
    assert float(flat[0]) == (float(g.view(-1)[0]) if with_g else 0.0) and float(flat[1]) == 0.0 and float(flat[2]) == 0.0 and float(flat[3]) == 0.0
    # the wrapper: count = a.numel()
    s32 = torch.tensor(float(dloss.double()) * weight / a.numel(), dtype=torch.float32).to(gpu_device)
    term = s32 * torch.sign(ad - td)
    assert torch.equal(V.feat_l1_tap_backward(ad, td, gd, dl, weight), torch.where(ad > 0, gd + term if with_g else term, torch.zeros_like(ad)))


L1_CASES = [[(2, 3, 5, 7), (2, 16, 4, 4)],                                              # an odd element count beside the 16-byte form
            [(1, 70, 33, 17)],                                                          # 39270 elements: more than one workgroup, no multiple of 4
            [(1, 16, 32, 32), (1, 32, 16, 16), (1, 64, 8, 8), (1, 64, 4, 4), (1, 64, 2, 2)]]          # a 32 x 32 narrow net


@pytest.mark.parametrize('shapes', L1_CASES)
def test_feat_l1_against_float64(gpu_device, shapes):
    """Against a float64 sum of the same fp32 taps: float64 accumulation leaves only the final rounding to fp32, at most 2^-24, and the bound
    is twice that.  Unequal weights, so a swapped weight shows; bit-identical over two runs."""
    V = _plugin(gpu_device)
    acts = [F.relu(_rand(s, 10 + i)) for i, s in enumerate(shapes)]
    tgts = [F.relu(_rand(s, 20 + i)) for i, s in enumerate(shapes)]
    weights = [1.0, 0.5, 2.0, 0.25, 3.0][:len(shapes)]
    want = sum(wt * float((a.double() - t.double()).abs().sum()) / a.numel() for a, t, wt in zip(acts, tgts, weights))
    swapped = sum(wt * float((a.double() - t.double()).abs().sum()) / a.numel() for a, t, wt in zip(acts, tgts, weights[::-1]))
    ad, td = [a.to(gpu_device) for a in acts], [t.to(gpu_device) for t in tgts]
    got = V.feat_l1(ad, td, weights)
    assert got.dtype == torch.float32 and got.ndim == 0
    err = abs(float(got.double()) - want) / want
    print(f'loss {float(got):.8f}, relative error {err:.2e}')
    assert err <= 2.0 ** -23
    assert len(shapes) == 1 or abs(swapped - want) / want > 1e-3
    assert torch.equal(V.feat_l1(ad, td, weights), got)
    assert float(V.feat_l1(ad, ad, weights)) == 0.0


def test_prep_at_the_loss_constants_is_x_plus_1_over_2(gpu_device):
    """ide3d_lpips_prep at f = 1, in_scale = in_shift = 0.5, mean 0, std 1 is (x + 1) / 2 bit for bit: fma(x, 0.5, 0.5) rounds the exact
    (x + 1) / 2 once, and so does halving the rounded x + 1; and its adjoint is dy / 2."""
    from torch_utils import hip_plugin
    hip_plugin.load()
    x = (torch.rand(2, 3, 16, 20, generator=torch.Generator().manual_seed(6)) * 2 - 1).to(gpu_device)
    zero, one = torch.zeros(3, device=gpu_device), torch.ones(3, device=gpu_device)
    assert torch.equal(hip_plugin.LpipsPlugin.prep(x, zero, one, 1, 0.5, 0.5), (x + 1) / 2)
    dy = _rand((2, 3, 16, 20), 7).to(gpu_device)
    assert torch.equal(hip_plugin.LpipsPlugin.prep_backward(dy, one, 1, 0.5), dy / 2)


# ---- end to end --------------------------------------------------------------------------------------------------------------------------------
def _module(widths, device, n_layers=5):
    from training import vgg_loss
    m = vgg_loss.VGGLoss(None, n_layers, widths)
    m.load_state_dict(ref.synthetic_state_dict(widths, 0, n_layers))
    return m.to(device)


def _value_and_grad(m, x, y):
    leaf = x.clone().requires_grad_(True)
    v = m(leaf, y)
    (g,) = torch.autograd.grad(v, [leaf])
    return float(v.detach()), g.cpu().double()


_reference = {}


def _float64(widths, n_layers, shape, seed):
    key = (widths, n_layers, shape, seed)
    if key not in _reference:
        x, y = ref.images(shape, seed)
        _reference[key] = (x, y) + ref.vgg64_with_grad(ref.synthetic_state_dict(widths, 0, n_layers), x, y, n_layers)
    return _reference[key]


@pytest.mark.parametrize('arith', ['default', 'fp32'])
@pytest.mark.parametrize('widths,n_layers,shape,seed', ref.E2E_CASES)
def test_end_to_end_against_float64(gpu_device, widths, n_layers, shape, seed, arith):
    """Value (relative error) and image gradient (relative L2) against float64, with the bounds of
    tests/test_gpu_lpips_alex.py::test_end_to_end_against_float64: the gradient within 4 x the error of the module's own fp32 ATen path
    (`fused = False`) on the same inputs, the value within the larger of that and 4 x 2^-24 (rounding the scalar to fp32 alone costs up to
    2^-24).  The inputs keep away from every kink (tests/test_vgg_loss_cpu.py::test_kink_margin_of_the_end_to_end_cases), so both errors are
    rounding.  The measured errors are in DESIGN.md section 5.22."""
    from torch_utils import hip_plugin
    x, y, want_v, want_g = _float64(widths, n_layers, shape, seed)
    m = _module(widths, gpu_device, n_layers)
    xd, yd = x.to(gpu_device), y.to(gpu_device)
    with _fused(False):
        tv, tg = _value_and_grad(m, xd, yd)
    hip_plugin.conv_arithmetic(arith)
    try:
        before = hip_plugin.CALLS.get('feat_l1_tap_backward', 0)
        with _fused(True):
            hv, hg = _value_and_grad(m, xd, yd)
        assert hip_plugin.CALLS.get('feat_l1_tap_backward', 0) == before + n_layers, 'the HIP path did not run'
    finally:
        hip_plugin.conv_arithmetic('default')
    wv, wn = float(want_v), float(want_g.norm())
    ev_t, eg_t = abs(tv - wv) / wv, float((tg - want_g).norm()) / wn
    ev_h, eg_h = abs(hv - wv) / wv, float((hg - want_g).norm()) / wn
    print(f'{arith}: value rel err HIP {ev_h:.2e} ATen {ev_t:.2e}; gradient rel L2 HIP {eg_h:.2e} ATen {eg_t:.2e}')
    assert wv > 0 and wn > 0
    assert eg_h <= 4 * eg_t
    assert ev_h <= max(4 * ev_t, 4 * 2.0 ** -24)


# one pass of the HIP path, by entry point: the target's features, and what the distance with its gradient adds
FEATURES_CALLS = {'lpips_prep': 1, 'modconv2d': 13, 'maxpool2': 4}
DISTANCE_CALLS = {'lpips_prep': 1, 'modconv2d': 13 + 13, 'maxpool2': 4, 'feat_l1': 1, 'feat_l1_tap_backward': 5, 'maxpool2_relu_backward': 4,
                  'modconv_act_backward': 4, 'lpips_prep_backward': 1}


def _calls_of(fn):
    from torch_utils import hip_plugin
    before = dict(hip_plugin.CALLS)
    fn()
    return {k: v - before.get(k, 0) for k, v in hip_plugin.CALLS.items() if v != before.get(k, 0)}


def test_routing_and_launch_count(gpu_device):
    m = _module(NARROW, gpu_device)
    x, y = (t.to(gpu_device) for t in ref.images((1, 3, 32, 32), 8))
    with _fused(True):
        feats = []
        assert _calls_of(lambda: feats.extend(m.features(y))) == FEATURES_CALLS
        assert len(feats) == 5 and not any(t.requires_grad for t in feats)
        assert _calls_of(lambda: _value_and_grad(m, x, y)) == {k: v + FEATURES_CALLS.get(k, 0) for k, v in DISTANCE_CALLS.items()}
        leaf = x.clone().requires_grad_(True)
        assert _calls_of(lambda: m.distance_to(leaf, feats).backward()) == DISTANCE_CALLS
        assert leaf.grad is not None and bool(torch.isfinite(leaf.grad).all()) and float(leaf.grad.abs().max()) > 0
        # what takes the torch definition
        assert _calls_of(lambda: _value_and_grad(m.half(), x.half(), y.half())) == {}
        m.float()
        m.layers[0][0].weight.requires_grad_(True)
        assert _calls_of(lambda: _value_and_grad(m, x, y)) == {}
        m.layers[0][0].weight.requires_grad_(False)
        assert _calls_of(lambda: m(x[:, :, :, :31], y[:, :, :, :31])) == {}, 'a view that is not dense'
        with pytest.raises(ValueError, match='at least 16'):
            m(x[:, :, :15].contiguous(), y[:, :, :15].contiguous())
        with pytest.raises(ValueError, match='at least 16'):
            m.features(y[:, :, :, :15].contiguous())
    with _fused(False):
        assert _calls_of(lambda: _value_and_grad(m, x, y)) == {}


def test_project_with_vgg_distance_on_gpu(gpu_device):
    from training import projection, triplane, vgg_loss
    torch.manual_seed(0)
    G = triplane.TriPlaneGenerator(triplane.tiny_spec()).eval().to(gpu_device)
    c = triplane.camera_label(0.2)
    target = torch.rand(3, G.img_resolution, G.img_resolution, generator=torch.Generator().manual_seed(1)) * 255
    m = _module(NARROW, gpu_device)
    with _fused(True):
        d = vgg_loss.vgg_distance(target[None].to(gpu_device), m)
        # without the w noise and the noise regulariser the step loss is the distance alone (the first step runs at learning rate 0)
        p = projection.Projector(G, target, c, num_steps=5, w_avg_samples=32, distance=d, initial_noise_factor=0.0, regularize_noise_weight=0.0)
        start = p.pivot().clone()
        losses = []
        calls = _calls_of(lambda: losses.extend(float(p.step(i)) for i in range(5)))
    assert calls.get('feat_l1') == 5 and calls.get('feat_l1_tap_backward') == 25 and calls.get('lpips_prep_backward') == 5 and len(losses) == 5
    assert all(v == v and abs(v) != float('inf') for v in losses)
    assert losses[-1] < losses[0], losses
    assert bool(torch.isfinite(p.pivot()).all()) and not torch.equal(p.pivot(), start)
