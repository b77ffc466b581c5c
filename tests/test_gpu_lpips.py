"""The VGG16 LPIPS distance on the GPU (training/lpips.py over csrc/lpips.hip, csrc/modconv.hip, csrc/modconv_bwd.hip): every streaming
pass against the float64 restatements of tests/lpips_ref.py, the whole distance and its image gradient against float64 beside the module's
own fp32 ATen path, the routing rules with the launch count, and `project()` with the closure."""

import contextlib

import pytest
import torch
import torch.nn.functional as F

import lpips_ref

pytestmark = pytest.mark.gpu

NARROW = (16, 32, 64, 64, 64)
E2E_CASES = [(NARROW, (2, 3, 32, 32), 0), (NARROW, (1, 3, 40, 24), 1), (lpips_ref.VGG16, (1, 3, 32, 32), 2)]          # as test_lpips_cpu.py
# 1e-6 of the largest magnitude: the project's bound for its fp32 element-wise passes and reductions against float64
FP32 = 1e-6


@contextlib.contextmanager
def _fused(on):
    from training import lpips
    old, lpips.fused = lpips.fused, on
    try:
        yield
    finally:
        lpips.fused = old


def _plugin(gpu_device):
    from torch_utils import hip_plugin
    hip_plugin.load()
    return hip_plugin.LpipsPlugin


def _rand(shape, seed, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


def _close(got, want, bound=FP32):
    err, scale = float((got.cpu().double() - want).abs().max()), float(want.abs().max())
    print(f'max err {err:.3e} of scale {scale:.3e} = {err / scale:.2e}')
    return err <= bound * scale


@pytest.mark.parametrize('shape,f', [((2, 3, 8, 12), 1), ((2, 3, 8, 12), 2), ((1, 3, 16, 16), 4)])
def test_prep_forward_and_backward(gpu_device, shape, f):
    P = _plugin(gpu_device)
    x = torch.rand(*shape, generator=torch.Generator().manual_seed(1)) * 255
    mean, std = torch.tensor(lpips_ref.MEAN, device=gpu_device), torch.tensor(lpips_ref.STD, device=gpu_device)
    y = P.prep(x.to(gpu_device), mean, std, f, 2 / 255, -1.0)
    assert tuple(y.shape) == (shape[0], 3, shape[2] // f, shape[3] // f)
    assert _close(y, lpips_ref.prep64(x, f, 2 / 255, -1.0))
    dy = _rand(y.shape, 2)
    dx = P.prep_backward(dy.to(gpu_device), std, f, 2 / 255)
    assert dx.shape == x.shape
    assert _close(dx, lpips_ref.prep_backward64(dy, f, 2 / 255))


# the issue's two shapes (scalar path: w % 4 != 0, the second with an odd height and width) and two whose rows take the 16-byte path (w % 4 == 0),
# the second with an odd height
POOL_SHAPES = [(2, 5, 6, 10), (1, 3, 7, 5), (2, 3, 6, 8), (1, 2, 5, 12)]


@pytest.mark.parametrize('shape', POOL_SHAPES)
def test_maxpool2_is_bit_equal_to_aten(gpu_device, shape):
    P = _plugin(gpu_device)
    x = _rand(shape, 3).to(gpu_device)
    assert torch.equal(P.maxpool2(x), F.max_pool2d(x, 2))
    xr = F.relu(x)                                          # many equal zeros
    assert torch.equal(P.maxpool2(xr), F.max_pool2d(xr, 2))


@pytest.mark.parametrize('with_dpool', [True, False])
@pytest.mark.parametrize('shape', POOL_SHAPES)
def test_stage_backward(gpu_device, shape, with_dpool):
    """ReLU'd activations (half of them zero), so windows with several zeros and all-zero windows occur; at the odd shapes the last row and
    column have no window and must receive dtap alone."""
    P = _plugin(gpu_device)
    n, c, h, w = shape
    y = F.relu(_rand(shape, 4))
    dtap = _rand(shape, 5)
    dpool = _rand((n, c, h // 2, w // 2), 6) if with_dpool else None
    dz = P.stage_backward(y.to(gpu_device), None if dpool is None else dpool.to(gpu_device), dtap.to(gpu_device))
    want = lpips_ref.stage_backward64(y, dpool, dtap)
    assert _close(dz, want)
    assert bool((dz.cpu()[y == 0] == 0).all())
    if h % 2:
        assert torch.equal(dz.cpu()[:, :, -1], dtap[:, :, -1] * (y[:, :, -1] > 0))
    if w % 2:
        assert torch.equal(dz.cpu()[:, :, :, -1], dtap[:, :, :, -1] * (y[:, :, :, -1] > 0))


HEAD_CASES = [(2, 16, 5, 3, True), (2, 512, 2, 1, False), (3, 7, 9, 11, True)]          # n, c, h, w, one all-zero pixel; the last: > 1 workgroup, c % 4 != 0


def _head_inputs(n, c, h, w, zero_pixel, seed):
    a = F.relu(_rand((n, c, h, w), seed) + 0.3)
    if zero_pixel:
        a[0, :, h // 2, w // 2] = 0
    t = F.relu(_rand((n, c, h, w), seed + 1) + 0.3)
    t = t / (t.square().sum(1, keepdim=True).sqrt() + 1e-10)
    if zero_pixel:
        t[0, :, h // 2, w // 2] = 0          # (a target that is zero there too: the direct term g / eps vanishes, as at a tap that is zero for every input)
    lin = torch.rand(c, generator=torch.Generator().manual_seed(seed + 2))
    return a, t, lin


@pytest.mark.parametrize('n,c,h,w,zero_pixel', HEAD_CASES)
def test_head_forward_and_backward(gpu_device, n, c, h, w, zero_pixel):
    """fp32 streaming sums of at most 512 terms, carried in float64 by the kernels: 1e-6 of the value forward, 1e-6 of max |gradient| backward;
    bit-identical over two runs."""
    P = _plugin(gpu_device)
    a, t, lin = _head_inputs(n, c, h, w, zero_pixel, 7)
    leaf = a.double().requires_grad_(True)
    want = lpips_ref.head64(leaf, t, lin)
    (want_g,) = torch.autograd.grad(want * 0.7, [leaf])
    want = want.detach()
    ad, td, ld = a.to(gpu_device), t.to(gpu_device), lin.to(gpu_device)
    got = P.head([ad], [td], [ld])
    print(f'value {float(got):.7f} vs {float(want):.7f}')
    assert abs(float(got) - float(want)) <= FP32 * float(want)
    up = torch.tensor(0.7, device=gpu_device)
    (da,) = P.head_backward([ad], [td], [ld], up)
    assert bool(torch.isfinite(da).all())
    assert _close(da, want_g)
    assert torch.equal(P.head([ad], [td], [ld]), got) and torch.equal(P.head_backward([ad], [td], [ld], up)[0], da)
    (u,) = P.normalize([ad])
    assert _close(u, lpips_ref._Unit.apply(a.double()))
    if zero_pixel:
        assert float(u[0, :, h // 2, w // 2].abs().max()) == 0


def test_head_over_several_taps_adds_them_in_order(gpu_device):
    P = _plugin(gpu_device)
    cases = [_head_inputs(n, c, h, w, z, 20 + i) for i, (n, c, h, w, z) in enumerate([(2, 16, 8, 8, False), (2, 32, 4, 4, True), (2, 64, 2, 1, False)])]
    want = sum(lpips_ref.head64(a.double(), t, lin) for a, t, lin in cases)
    dev = [[v.to(gpu_device) for v in col] for col in zip(*cases)]
    got = P.head(*dev)
    assert abs(float(got) - float(want)) <= FP32 * float(want)
    assert torch.equal(P.head(*dev), got)


def _module(widths, device, sd=None):
    from training import lpips
    m = lpips.LPIPS('vgg', widths=widths)
    m.load_state_dict(sd if sd is not None else lpips_ref.synthetic_state_dict(widths))
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
        x, y = lpips_ref.images(shape, seed)
        _reference[key] = (x, y) + lpips_ref.lpips64_with_grad(lpips_ref.synthetic_state_dict(widths), x, y)
    return _reference[key]


@pytest.mark.parametrize('arith', ['default', 'fp32'])
@pytest.mark.parametrize('widths,shape,seed', E2E_CASES)
def test_end_to_end_against_float64(gpu_device, widths, shape, seed, arith):
    """Value (relative error) and image gradient (relative L2) against float64; the bound is 4 x the error of the module's own fp32 ATen path
    (`fused = False`) on the same inputs: the library's bf16x6 and exact-fp32 convolutions are fp32-grade but
    accumulate in another order over 13 layers; a wrong mask, a dropped row or a mis-scaled tap is two orders of magnitude above that.
    Measured on an MI355X (HIP / ATen): gradient 2.2e-6 / 1.9e-6, 2.2e-6 / 1.7e-6, 4.4e-6 / 3.2e-6 (2.8e-6 / 3.2e-6 with fp32 products); the
    value errors (2e-8 .. 1.2e-7) are the distance of the float64 value to the nearest or second-nearest fp32 number on both paths."""
    from torch_utils import hip_plugin
    x, y, want_v, want_g = _float64(widths, shape, seed)
    m = _module(widths, gpu_device)
    xd, yd = x.to(gpu_device), y.to(gpu_device)
    with _fused(False):
        tv, tg = _value_and_grad(m, xd, yd)
    hip_plugin.conv_arithmetic(arith)
    try:
        before = hip_plugin.CALLS.get('lpips_head', 0)
        with _fused(True):
            hv, hg = _value_and_grad(m, xd, yd)
        assert hip_plugin.CALLS.get('lpips_head', 0) > before, 'the HIP path did not run'
    finally:
        hip_plugin.conv_arithmetic('default')
    wv, wn = float(want_v), float(want_g.norm())
    ev_t, eg_t = abs(tv - wv) / wv, float((tg - want_g).norm()) / wn
    ev_h, eg_h = abs(hv - wv) / wv, float((hg - want_g).norm()) / wn
    print(f'{arith}: value rel err HIP {ev_h:.2e} ATen {ev_t:.2e}; gradient rel L2 HIP {eg_h:.2e} ATen {eg_t:.2e}')
    assert eg_h <= 4 * eg_t
    assert ev_h <= 4 * ev_t


def test_all_zero_tap_on_the_hip_path(gpu_device):
    sd = lpips_ref.synthetic_state_dict(NARROW, bias_shift={14: -1e3})
    x, y = lpips_ref.images((2, 3, 32, 32), 3)
    want_v, want_g = lpips_ref.lpips64_with_grad(sd, x, y)
    with _fused(True):
        v, g = _value_and_grad(_module(NARROW, gpu_device, sd), x.to(gpu_device), y.to(gpu_device))
    assert bool(torch.isfinite(g).all())
    assert abs(v - float(want_v)) <= 2e-5 * float(want_v) and float((g - want_g).norm() / want_g.norm()) <= 2e-5          # (tolerance of test_lpips_cpu.py)


# one forward + backward of the HIP path, by entry point: the target's features, then the distance and its gradient
FEATURES_CALLS = {'lpips_prep': 1, 'modconv2d': 13, 'maxpool2': 4, 'lpips_head': 1}
DISTANCE_CALLS = {'lpips_prep': 1, 'modconv2d': 13 + 13, 'maxpool2': 4, 'lpips_head': 1, 'lpips_head_backward': 1, 'lpips_stage_backward': 5,
                  'modconv_act_backward': 8, 'lpips_prep_backward': 1}


def _calls_of(fn):
    from torch_utils import hip_plugin
    before = dict(hip_plugin.CALLS)
    fn()
    return {k: v - before.get(k, 0) for k, v in hip_plugin.CALLS.items() if v != before.get(k, 0)}


def test_routing_and_launch_count(gpu_device):
    m = _module(NARROW, gpu_device)
    x, y = (t.to(gpu_device) for t in lpips_ref.images((1, 3, 32, 32), 8))
    with _fused(True):
        feats = []
        assert _calls_of(lambda: feats.extend(m.features(y))) == FEATURES_CALLS
        assert _calls_of(lambda: _value_and_grad(m, x, y)) == {k: v + FEATURES_CALLS.get(k, 0) for k, v in DISTANCE_CALLS.items()}
        leaf = x.clone().requires_grad_(True)
        assert _calls_of(lambda: m.distance_to(leaf, feats).backward()) == DISTANCE_CALLS
        # what takes the torch definition
        assert _calls_of(lambda: _value_and_grad(m.half(), x.half(), y.half())) == {}
        m.float()
        m.net.layers[0].weight.requires_grad_(True)
        assert _calls_of(lambda: _value_and_grad(m, x, y)) == {}
        m.net.layers[0].weight.requires_grad_(False)
        assert _calls_of(lambda: m(x[:, :, :, 1:17], y[:, :, :, 1:17])) == {}, 'a view that is not dense'
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
    assert calls.get('lpips_head') == 3 and calls.get('lpips_prep_backward') == 3 and len(losses) == 3
    assert all(v == v and abs(v) != float('inf') for v in losses)
    assert bool(torch.isfinite(p.pivot()).all()) and not torch.equal(p.pivot(), start)
