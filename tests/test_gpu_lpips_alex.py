"""The AlexNet LPIPS distance on the GPU (training/lpips_alex.py over csrc/lpips_alex.hip, csrc/lpips.hip, csrc/modconv.hip): every streaming
pass against ATen bit for bit or against the float64 restatements of tests/lpips_alex_ref.py, the whole distance and its image gradient
against float64 beside the module's own fp32 ATen path, the routing rules with the launch count, and `project()` with the closure."""

import contextlib

import pytest
import torch
import torch.nn.functional as F

import lpips_alex_ref as ref

pytestmark = pytest.mark.gpu

NARROW = (8, 12, 16, 12, 12)
E2E_CASES = [(NARROW, (2, 3, 32, 32), 0), (NARROW, (1, 3, 38, 46), 1), (ref.ALEX, (1, 3, 64, 64), 2)]          # (widths, shape, seed)
# 1e-6 of the largest magnitude: the project's bound for its fp32 element-wise passes and reductions against float64
FP32 = 1e-6


@contextlib.contextmanager
def _fused(on):
    from training import lpips_alex
    old, lpips_alex.fused = lpips_alex.fused, on
    try:
        yield
    finally:
        lpips_alex.fused = old


def _plugin(gpu_device):
    from torch_utils import hip_plugin
    hip_plugin.load()
    return hip_plugin.LpipsAlexPlugin


def _rand(shape, seed, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


def _close(got, want, bound=FP32):
    err, scale = float((got.cpu().double() - want).abs().max()), float(want.abs().max())
    print(f'max err {err:.3e} of scale {scale:.3e} = {err / scale:.2e}')
    return err <= bound * scale


# (k, stride, pad, shape): the stem's geometry with a row and a column that no window reaches, the 5x5 layer's on a map smaller than the
# window, an unpadded stride-2 one with odd sides, and the stem's at the smallest side the net takes
UNFOLD_CASES = [(11, 4, 2, (2, 3, 38, 46)), (5, 1, 2, (1, 7, 3, 4)), (3, 2, 0, (1, 2, 7, 9)), (11, 4, 2, (1, 3, 31, 31))]


@pytest.mark.parametrize('k,stride,pad,shape', UNFOLD_CASES)
def test_unfold2d_is_bit_equal_to_aten(gpu_device, k, stride, pad, shape):
    A = _plugin(gpu_device)
    x = _rand(shape, 1).to(gpu_device)
    n, c, h, w = shape
    ho, wo = (h + 2 * pad - k) // stride + 1, (w + 2 * pad - k) // stride + 1
    col = A.unfold2d(x, k, stride, pad)
    assert tuple(col.shape) == (n, c * k * k, ho, wo)
    assert torch.equal(col, F.unfold(x, k, padding=pad, stride=stride).reshape(n, c * k * k, ho, wo))


@pytest.mark.parametrize('k,stride,pad,shape', UNFOLD_CASES)
def test_fold2d_is_the_adjoint(gpu_device, k, stride, pad, shape):
    """Against the float64 adjoint (at most 25 terms, summed in float64 by the kernel and rounded once: 1e-6 of the largest magnitude holds
    with 2^-24 = 6e-8); bit-equal on repeat; every element of a NaN-filled result is overwritten; exact zeros where no window reaches."""
    A = _plugin(gpu_device)
    n, c, h, w = shape
    ho, wo = (h + 2 * pad - k) // stride + 1, (w + 2 * pad - k) // stride + 1
    dcol = _rand((n, c * k * k, ho, wo), 2)
    dd = dcol.to(gpu_device)
    from torch_utils import hip_plugin
    dx = torch.full((n, c, h, w), float('nan'), device=gpu_device)          # through the C entry point, into a NaN-filled result
    rc = hip_plugin.load().ide3d_fold2d(hip_plugin._ptr(dd), hip_plugin._ptr(dx), n, c, h, w, k, stride, pad, hip_plugin._stream(dd))
    assert rc == 0 and bool(torch.isfinite(dx).all()), 'an element was not written'
    assert _close(dx, ref.fold64(dcol, (h, w), k, stride, pad))
    again = A.fold2d(dd, (h, w), k, stride, pad)
    assert tuple(again.shape) == shape and torch.equal(again, dx)
    # <x, fold(d)> = <unfold(x), d>
    x = _rand(shape, 3)
    lhs = float((x.double() * dx.cpu().double()).sum())
    rhs = float((F.unfold(x.double(), k, padding=pad, stride=stride).reshape(dcol.shape) * dcol.double()).sum())
    assert abs(lhs - rhs) <= 1e-5 * max(abs(rhs), 1.0)
    reach_h, reach_w = (ho - 1) * stride + k - pad, (wo - 1) * stride + k - pad          # first row / column that no window reads
    if reach_h < h:
        assert float(dx[:, :, reach_h:].abs().max()) == 0.0
    if reach_w < w:
        assert float(dx[:, :, :, reach_w:].abs().max()) == 0.0
    if (k, stride, shape) == (11, 4, (2, 3, 38, 46)):
        assert reach_h == 37 and reach_w == 45


POOL_SHAPES = [(2, 5, 8, 10), (1, 3, 7, 7), (1, 2, 3, 3), (3, 1, 9, 4)]


def _winner_bytes(x):
    """ATen's argmax (a flat index into the input plane) decoded to ky * 3 + kx of the window anchored at (2 oy, 2 ox)."""
    y, flat = F.max_pool2d(x, 3, 2, return_indices=True)
    w = x.shape[3]
    oy = torch.arange(y.shape[2], device=x.device)[:, None]
    ox = torch.arange(y.shape[3], device=x.device)[None, :]
    return y, ((flat // w - 2 * oy) * 3 + (flat % w - 2 * ox)).to(torch.uint8)


@pytest.mark.parametrize('shape', POOL_SHAPES)
def test_maxpool3s2p0_is_bit_equal_to_aten(gpu_device, shape):
    A = _plugin(gpu_device)
    x = _rand(shape, 3).to(gpu_device)
    for t in (x, F.relu(x)):                                # the second: many equal zeros, so the tie rule shows
        want, want_idx = _winner_bytes(t)
        y, idx = A.maxpool3s2p0(t)
        assert torch.equal(y, want) and idx.dtype == torch.uint8 and torch.equal(idx, want_idx)
        y2, none = A.maxpool3s2p0(t, want_idx=False)
        assert none is None and torch.equal(y2, want)
    xn = x.clone()
    xn[0, 0, 1, 1] = float('nan')
    y, idx = A.maxpool3s2p0(xn)
    assert bool(torch.isnan(y[0, 0, 0, 0])) and int(idx[0, 0, 0, 0]) == 4


@pytest.mark.parametrize('form', ['pooled', 'pass', 'last'])
@pytest.mark.parametrize('shape', POOL_SHAPES)
def test_tap_backward(gpu_device, shape, form):
    """ReLU'd activations (half of them zero), so windows with several zeros and all-zero windows occur; rows and columns past the last
    window ((2, 5, 8, 10): row 7 and column 9; (3, 1, 9, 4): column 3) must receive dtap alone.  At most 4 + 1 fp32 terms: 1e-6."""
    A = _plugin(gpu_device)
    n, c, h, w = shape
    y = F.relu(_rand(shape, 4))
    dtap = _rand(shape, 5)
    yd = y.to(gpu_device)
    if form == 'pooled':
        g = _rand((n, c, (h - 3) // 2 + 1, (w - 3) // 2 + 1), 6)
        idx = A.maxpool3s2p0(yd)[1]
    else:
        g, idx = (_rand(shape, 6) if form == 'pass' else None), None
    args = (yd, None if g is None else g.to(gpu_device), idx, dtap.to(gpu_device))
    dz = A.tap_backward(*args)
    assert _close(dz, ref.tap_backward64(y, g, dtap, form == 'pooled'))
    assert bool((dz.cpu()[y == 0] == 0).all())
    assert torch.equal(A.tap_backward(*args), dz)
    if form == 'pooled':
        reach_h, reach_w = 2 * ((h - 3) // 2) + 3, 2 * ((w - 3) // 2) + 3
        assert (reach_h < h) == (h % 2 == 0) and (reach_w < w) == (w % 2 == 0)
        if reach_h < h:
            assert torch.equal(dz.cpu()[:, :, reach_h:], (dtap * (y > 0))[:, :, reach_h:])
        if reach_w < w:
            assert torch.equal(dz.cpu()[:, :, :, reach_w:], (dtap * (y > 0))[:, :, :, reach_w:])


def _module(widths, device, sd=None):
    from training import lpips_alex
    m = lpips_alex.LPIPS(widths=widths)
    m.load_state_dict(sd if sd is not None else ref.synthetic_state_dict(widths))
    return m.to(device)


def _value_and_grad(m, x, y):
    leaf = x.clone().requires_grad_(True)
    v = m(leaf, y)
    (g,) = torch.autograd.grad(v, [leaf])
    return float(v.detach()), g.cpu().double()


_reference = {}


def _float64(widths, shape, seed):
    key = (widths, shape, seed)
    if key not in _reference:
        x, y = ref.images(shape, seed)
        _reference[key] = (x, y) + ref.lpips64_with_grad(ref.synthetic_state_dict(widths), x, y)
    return _reference[key]


@pytest.mark.parametrize('arith', ['default', 'fp32'])
@pytest.mark.parametrize('widths,shape,seed', E2E_CASES)
def test_end_to_end_against_float64(gpu_device, widths, shape, seed, arith):
    """Value (relative error) and image gradient (relative L2) against float64.  The gradient bound is 4 x the error of the module's own fp32
    ATen path (`fused = False`) on the same inputs, the yardstick and margin of tests/test_gpu_lpips.py: the library's convolutions are
    fp32-grade but accumulate in another order; a wrong mask, a dropped row or a mis-scaled tap is orders of
    magnitude above that.  The value bound is the larger of that and 4 x 2^-24: rounding the scalar to fp32 alone costs up to 2^-24.
    The measured errors are in DESIGN.md section 5.20."""
    from torch_utils import hip_plugin
    x, y, want_v, want_g = _float64(widths, shape, seed)
    m = _module(widths, gpu_device)
    xd, yd = x.to(gpu_device), y.to(gpu_device)
    with _fused(False):
        tv, tg = _value_and_grad(m, xd, yd)
    hip_plugin.conv_arithmetic(arith)
    try:
        before = hip_plugin.CALLS.get('lpips_tap_backward', 0)
        with _fused(True):
            hv, hg = _value_and_grad(m, xd, yd)
        assert hip_plugin.CALLS.get('lpips_tap_backward', 0) == before + 5, 'the HIP path did not run'
    finally:
        hip_plugin.conv_arithmetic('default')
    wv, wn = float(want_v), float(want_g.norm())
    ev_t, eg_t = abs(tv - wv) / wv, float((tg - want_g).norm()) / wn
    ev_h, eg_h = abs(hv - wv) / wv, float((hg - want_g).norm()) / wn
    print(f'{arith}: value rel err HIP {ev_h:.2e} ATen {ev_t:.2e}; gradient rel L2 HIP {eg_h:.2e} ATen {eg_t:.2e}')
    assert wv > 0 and wn > 0
    assert eg_h <= 4 * eg_t
    assert ev_h <= max(4 * ev_t, 4 * 2.0 ** -24)


def test_all_zero_tap_on_the_hip_path(gpu_device):
    sd = ref.synthetic_state_dict(NARROW, bias_shift={6: -1e3})
    x, y = ref.images((2, 3, 32, 32), 3)
    want_v, want_g = ref.lpips64_with_grad(sd, x, y)
    with _fused(True):
        v, g = _value_and_grad(_module(NARROW, gpu_device, sd), x.to(gpu_device), y.to(gpu_device))
    assert bool(torch.isfinite(g).all())
    assert abs(v - float(want_v)) <= 2e-5 * float(want_v) and float((g - want_g).norm() / want_g.norm()) <= 2e-5          # (tolerance of test_lpips_alex_cpu.py)


# one forward + backward of the HIP path, by entry point: the target's features, then the distance and its gradient
FEATURES_CALLS = {'lpips_prep': 1, 'unfold2d': 2, 'modconv2d': 5, 'maxpool3s2p0': 2, 'lpips_head': 1}
DISTANCE_CALLS = {'lpips_prep': 1, 'unfold2d': 2, 'modconv2d': 5 + 5, 'maxpool3s2p0': 2, 'lpips_head': 1, 'lpips_head_backward': 1,
                  'lpips_tap_backward': 5, 'fold2d': 2, 'lpips_prep_backward': 1}


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
        assert _calls_of(lambda: _value_and_grad(m, x, y)) == {k: v + FEATURES_CALLS.get(k, 0) for k, v in DISTANCE_CALLS.items()}
        leaf = x.clone().requires_grad_(True)
        calls = _calls_of(lambda: m.distance_to(leaf, feats).backward())
        assert calls == DISTANCE_CALLS and 'modconv_act_backward' not in calls
        # what takes the torch definition
        assert _calls_of(lambda: _value_and_grad(m.half(), x.half(), y.half())) == {}
        m.float()
        m.net.layers[0].weight.requires_grad_(True)
        assert _calls_of(lambda: _value_and_grad(m, x, y)) == {}
        m.net.layers[0].weight.requires_grad_(False)
        assert _calls_of(lambda: m(x[:, :, :, :31], y[:, :, :, :31])) == {}, 'a view that is not dense'
        with pytest.raises(ValueError, match='at least 31'):
            m(x[:, :, :30].contiguous(), y[:, :, :30].contiguous())
    with _fused(False):
        assert _calls_of(lambda: _value_and_grad(m, x, y)) == {}


def test_project_with_lpips_distance_on_gpu(gpu_device):
    from training import lpips, projection, triplane
    torch.manual_seed(0)
    G = triplane.TriPlaneGenerator(triplane.tiny_spec()).eval().to(gpu_device)
    c = triplane.camera_label(0.2)
    target = torch.rand(3, G.img_resolution, G.img_resolution, generator=torch.Generator().manual_seed(1)) * 255
    m = _module(NARROW, gpu_device)
    with _fused(True):
        d = lpips.lpips_distance(target[None].to(gpu_device), m, size=32)          # 64 -> 32: the area factor 2 runs in ide3d_lpips_prep
        p = projection.Projector(G, target, c, num_steps=3, w_avg_samples=32, distance=d)
        start = p.pivot().clone()
        losses = []
        calls = _calls_of(lambda: losses.extend(float(p.step(i)) for i in range(3)))
    assert calls.get('lpips_head') == 3 and calls.get('fold2d') == 6 and calls.get('lpips_prep_backward') == 3 and len(losses) == 3
    assert all(v == v and abs(v) != float('inf') for v in losses)
    assert bool(torch.isfinite(p.pivot()).all()) and not torch.equal(p.pivot(), start)
