"""The face parser's cross-entropy loss on the GPU (training/parse_loss.py over csrc/parse_loss.hip, csrc/modconv.hip, csrc/modconv_bwd.hip):
every new pass alone against float64 torch on the same fp32 inputs beside the ATen fp32 operator, the whole loss and its image gradient
against float64 and the reference's fixture beside the module's own ATen path, the routing rules with the launch counts, reproducibility.

Bound of a pass: 4 x the error of the ATen fp32 operator on the same inputs, with a floor of one fp32 ulp of the largest magnitude."""

import contextlib

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import parse_loss_ref as R

pytestmark = pytest.mark.gpu


def _plugin(gpu_device):
    from torch_utils import hip_plugin
    hip_plugin.load()
    return hip_plugin.ParseLossPlugin


def _rand(shape, seed, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


def _within(got, want, aten, what=''):
    """max |got - want| <= max(4 max |aten - want|, one fp32 ulp of max |want|); want: float64."""
    want = want.cpu().double()
    err, ref = float((got.cpu().double() - want).abs().max()), float((aten.cpu().double() - want).abs().max())
    floor = float(np.spacing(np.float32(float(want.abs().max()))))
    print(f'{what}: max err {err:.3e}, ATen {ref:.3e}, one ulp of the largest magnitude {floor:.3e}')
    return err <= max(4 * ref, floor)


def _aten_vjp(fn, x, dy):
    leaf = x.clone().requires_grad_(True)
    (g,) = torch.autograd.grad(fn(leaf), [leaf], dy)
    return g


# ---- each pass alone ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('shape,size', [((2, 3, 5, 7), (40, 56)), ((1, 4, 2, 3), (4, 6))])
def test_resize_and_its_adjoint(gpu_device, shape, size):
    P = _plugin(gpu_device)
    x, dy = _rand(shape, 1), _rand(shape[:2] + size, 2)
    up = lambda t: F.interpolate(t, size, mode='bilinear', align_corners=True)
    xd, dyd = x.to(gpu_device), dy.to(gpu_device)
    y = P.resize(xd, size)
    assert tuple(y.shape) == shape[:2] + size
    assert _within(y, up(x.double()), up(xd), 'resize')
    dx = P.resize_backward(dyd, shape[2:])
    assert dx.shape == x.shape
    assert _within(dx, _aten_vjp(up, x.double(), dy.double()), _aten_vjp(up, xd, dyd), 'adjoint')
    assert torch.equal(P.resize_backward(dyd, shape[2:]), dx)


@pytest.mark.parametrize('scale', [1.0, 80.0])
def test_loss_head(gpu_device, scale):
    """[2, 20, 8, 8] logits against 64 x 64 labels; scaled so that the logits reach +-80 and beyond: exp() of an unshifted logit would
    overflow fp32.  Several workgroups, so the finishing launch adds 32 partial sums.  Bit-identical over two runs."""
    P = _plugin(gpu_device)
    lg = _rand((2, 20, 8, 8), 3)
    lg = lg * (scale / float(lg.abs().max())) if scale != 1.0 else lg
    lab = torch.randint(0, 20, (2, 64, 64), generator=torch.Generator().manual_seed(4))
    ce = lambda t, l: F.cross_entropy(F.interpolate(t, (64, 64), mode='bilinear', align_corners=True), l)
    lgd, labd = lg.to(gpu_device), lab.to(gpu_device)
    loss, lse = P.ce(lgd, labd)
    want = ce(lg.double(), lab)
    assert loss.ndim == 0 and bool(torch.isfinite(loss))
    assert _within(loss, want, ce(lgd, labd), 'loss')
    dloss = torch.tensor([0.7], device=gpu_device)
    dl = P.ce_backward(lgd, labd, lse, dloss)
    want_g = _aten_vjp(lambda t: ce(t, lab), lg.double(), torch.tensor(0.7, dtype=torch.float64))
    aten_g = _aten_vjp(lambda t: ce(t, labd), lgd, dloss[0])
    assert _within(dl, want_g, aten_g, 'dlogits')
    loss2, lse2 = P.ce(lgd, labd)
    assert torch.equal(loss2, loss) and torch.equal(lse2, lse) and torch.equal(P.ce_backward(lgd, labd, lse, dloss), dl)


@pytest.mark.parametrize('shape', [(2, 3, 7, 9), (1, 2, 6, 10)])
def test_maxpool_and_its_gradient_are_bit_equal_to_aten(gpu_device, shape):
    """Odd and even sides, so windows hang over the border on every side.  Random inputs and integer-valued inputs in 0..2 (ties in nearly
    every window: the first maximum in row-major order must take the gradient); forward and gradient bit-equal to ATen in both."""
    P = _plugin(gpu_device)
    for x in (_rand(shape, 5), torch.randint(0, 3, shape, generator=torch.Generator().manual_seed(6)).float()):
        xd = x.to(gpu_device)
        y, idx = P.maxpool(xd)
        assert torch.equal(y, F.max_pool2d(xd, 3, 2, 1))
        dy = _rand(tuple(y.shape), 7).to(gpu_device)
        want = _aten_vjp(lambda t: F.max_pool2d(t, 3, 2, 1), xd, dy)
        dx = P.maxpool_backward(dy, idx, shape[2:])
        assert torch.equal(dx, want)
        assert float((dx.cpu().double() - _aten_vjp(lambda t: F.max_pool2d(t, 3, 2, 1), x.double(), dy.cpu().double())).abs().max()) <= 1e-6
        assert torch.equal(P.maxpool_backward(dy, idx, shape[2:], mask=xd), want * (xd > 0))


@pytest.mark.parametrize('shape', [(2, 5, 6, 10), (2, 5, 6, 12)])          # the second: rows of 16-byte accesses
def test_residual_join_and_gates(gpu_device, shape):
    P = _plugin(gpu_device)
    n, c, h, w = shape
    a, b, dy = (_rand(shape, s) for s in (8, 9, 10))
    g, m = torch.rand(n, c, 1, 1, generator=torch.Generator().manual_seed(11)), _rand((n, c, 1, 1), 12)
    ad, bd, dyd, gd, md = (t.to(gpu_device) for t in (a, b, dy, g, m))
    D = lambda t: t.double()
    # forward: the residual join, the refinement gates (+ broadcast, + map), the fusion gate
    y = P.join([ad, bd], post=1)
    assert _within(y, F.relu(D(a) + D(b)), F.relu(ad + bd), 'relu(a + b)')
    assert _within(P.join([ad], scale=gd, bias=md), D(a) * D(g) + D(m), ad * gd + md, 'feat * g + broadcast')
    assert _within(P.join([ad, bd], scale=gd), D(a) * D(g) + D(b), ad * gd + bd, 'feat * g + map')
    assert _within(P.join([ad, ad], scale=gd), D(a) * D(g) + D(a), ad * gd + ad, 'feat * g + feat')
    # the means and the gates' dot products, bit-identical over two runs
    mean = P.plane_sums(ad, None, 1.0 / (h * w))
    assert tuple(mean.shape) == (n, c, 1, 1)
    assert _within(mean, D(a).mean(dim=(2, 3), keepdim=True), ad.mean(dim=(2, 3), keepdim=True), 'mean')
    dot = P.plane_sums(dyd, ad)
    assert _within(dot, (D(dy) * D(a)).sum(dim=(2, 3), keepdim=True), (dyd * ad).sum(dim=(2, 3), keepdim=True), 'dot')
    assert torch.equal(P.plane_sums(ad, None, 1.0 / (h * w)), mean) and torch.equal(P.plane_sums(dyd, ad), dot)
    # backward of the join: the masked gradient
    yc = y.cpu()
    assert _within(P.join([dyd], y=y, post=2), D(dy) * (yc > 0), dyd * (y > 0), 'dy (y > 0)')
    # backward of a gate: dfeat = (dy * gate + dmean / (h w)) (feat > 0)
    feat = F.relu(a)
    got = P.join([dyd], scale=gd, bias=md, bias_gain=1.0 / (h * w), y=feat.to(gpu_device), post=2)
    assert _within(got, (D(dy) * D(g) + D(m) / (h * w)) * (feat > 0), (dyd * gd + md / (h * w)) * (feat.to(gpu_device) > 0), 'gate backward')
    # the gradients that meet at a block's input: a cropped (h + 1) x (w + 1) map, a half-resolution map at the even positions, a channel slice
    big, half, wide = _rand((n, c, h + 1, w + 1), 13), _rand((n, c, h // 2, w // 2), 14), _rand((n, 2 * c, h, w), 15)
    bigd, halfd, wided = (t.to(gpu_device) for t in (big, half, wide))

    def total(bg, hf, wd):
        v = bg[:, :, 1:h + 1, 1:w + 1] + wd[:, :c]
        v[:, :, ::2, ::2] += hf
        return v
    got = P.join([bigd[:, :, 1:h + 1, 1:w + 1], (halfd, True), wided[:, :c]], y=y, post=2)
    assert _within(got, total(D(big), D(half), D(wide)) * (yc > 0), total(bigd, halfd, wided) * (y > 0), 'three gradients + mask')
    got = P.join([wided[:, c:], bd])
    assert _within(got, D(wide)[:, c:] + D(b), wided[:, c:] + bd, 'slice + map')


def test_stem_gradient(gpu_device):
    P = _plugin(gpu_device)
    wt, dz = _rand((64, 3, 7, 7), 16, 0.1), _rand((1, 64, 32, 48), 17)
    conv = lambda t, k: F.conv2d(t, k, stride=2, padding=3)
    wd, dzd = wt.to(gpu_device), dz.to(gpu_device)
    dx = P.stem_backward(dzd, wd, (64, 96))
    assert tuple(dx.shape) == (1, 3, 64, 96)
    want = _aten_vjp(lambda t: conv(t, wt.double()), torch.zeros(1, 3, 64, 96, dtype=torch.float64), dz.double())
    aten = _aten_vjp(lambda t: conv(t, wd), torch.zeros(1, 3, 64, 96, device=gpu_device), dzd)
    assert _within(dx, want, aten, 'stem gradient')
    assert torch.equal(P.stem_backward(dzd, wd, (64, 96)), dx)


# ---- end to end --------------------------------------------------------------------------------------------------------------------------------
@contextlib.contextmanager
def _switches(fused, arith=0):
    from training import parse_loss
    old = parse_loss.fused, parse_loss.arith
    parse_loss.fused, parse_loss.arith = fused, arith
    try:
        yield
    finally:
        parse_loss.fused, parse_loss.arith = old


@contextlib.contextmanager
def _deterministic_aten():
    old = torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark
    torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark = True, False
    try:
        yield
    finally:
        torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark = old


def _dirty(device):
    """Leave NaNs in the allocator's free blocks, so that the next torch.empty of any size up to 64 MiB starts from them."""
    blocks = [torch.full((1 << s,), float('nan'), device=device) for s in (10, 14, 16, 18, 20, 22, 24) for _ in range(4)]
    torch.cuda.synchronize()
    del blocks


# The fall-back routes run the PyTorch definition in fp32 through ATen, which is not reproducible on this GPU with its default algorithms:
# two runs of the same call differ by 1e-6 .. 6e-6 in the gradient, and about one run in ten of the [2, 3, 64, 64] case lands 5.2e-4 away
# (measured with `parse_loss.fused = False` alone, no code of this library involved; an earlier form of the routing test, which compared
# two such runs at 1e-5, failed intermittently for that reason).  So the routes are run with deterministic algorithms requested, under
# which 12 runs were bit-identical, and "agrees with the definition" is measured against its float64 CPU evaluation.  An fp32 dot product of
# K <= 4608 terms carries a relative error of about sqrt(K) 2^-24 = 4e-6 of the size of its terms; the loss passes 20 such layers in a row
# and the gradient 40: sqrt(40) x 4e-6 = 2.5e-5 as independent errors (the convention of tests/test_lpips_cpu.py).  A route that computed
# anything else - other labels, a dropped branch - is off by 1e-2 or more.
FALLBACK_TOL = 2.5e-5

_cache = {}


def _gpu_net(gpu_device):
    if 'net' not in _cache:
        _cache['net'] = R.parser(device=gpu_device)
    return _cache['net']


def _float64(case):
    """The fixture's inputs and the float64 CPU evaluation of the module's definition on them, computed once."""
    if case not in _cache:
        img, lab, fix_loss, fix_grad = R.fixture(case)
        l64, g64 = R.definition(R.parser(dtype=torch.float64), img.double(), lab)
        _cache[case] = (img, lab, float(l64), g64, float(fix_loss), fix_grad.double())
    return _cache[case]


def _loss_and_grad(net, img, lab):
    from training import parse_loss
    leaf = img.clone().requires_grad_(True)
    loss = parse_loss.cross_entropy(net, leaf, lab)
    (g,) = torch.autograd.grad(loss, [leaf])
    return float(loss.detach()), g.cpu().double()


def _calls_of(fn):
    from torch_utils import hip_plugin
    before = dict(hip_plugin.CALLS)
    fn()
    return {k: v - before.get(k, 0) for k, v in hip_plugin.CALLS.items() if v != before.get(k, 0)}


@pytest.mark.parametrize('arith', [0, 1], ids=['bf16x6', 'fp32'])
@pytest.mark.parametrize('case', [0, 1])
def test_end_to_end_against_float64_and_the_fixture(gpu_device, case, arith):
    """[2, 3, 64, 64] and [1, 3, 96, 64]: the smallest sizes at which all three feature scales exist, the second with a non-square 1/32
    map.  Loss: relative error; image gradient: relative L2.  Against float64 the bound is 4 x the error of the module's `fused = False`
    ATen path on the same GPU and inputs (another summation order over at most a few hundred terms per output); the loss bound has no
    floor, as the issue states it.  The ATen path is not reproducible on this GPU (two runs of it differ by 1e-6 .. 6e-6 in the gradient and
    by 0 .. 5 ulps in the loss), so its error - the yardstick - is measured with deterministic algorithms requested.  Against the fixture
    (the reference's float32 CPU run, itself e_fix away from float64) the bound used here is 4 x that ATen error + e_fix, by the triangle
    inequality: an interpretation of the issue, whose wording also admits 4 x ATen's distance to the fixture; with the measured figures the
    bound used is the tighter of the two.
    Measured on an MI355X (HIP / ATen): loss 4.4e-7 / 2.0e-7 and 5.8e-7 / 3.8e-7 in bf16x6, 1.2e-7 / 2.0e-7 and 1.2e-7 / 3.8e-7 with fp32
    products (one fp32 ulp of these losses is 8e-8 of the value); gradient 3.0e-6 / 3.6e-6 and 3.3e-6 / 2.8e-6 in bf16x6, 2.5e-6 / 3.6e-6 and
    1.3e-6 / 2.8e-6 with fp32 products.  No seed was changed: no case's ATen error is dominated by a flipped ReLU mask or pooling winner."""
    img, lab, l64, g64, fix_loss, fix_grad = _float64(case)
    net, imgd, labd = _gpu_net(gpu_device), img.to(gpu_device), lab.to(gpu_device)
    with _switches(False), _deterministic_aten():
        tl, tg = _loss_and_grad(net, imgd, labd)
    with _switches(True, arith):
        calls = _calls_of(lambda: _cache.__setitem__('e2e', _loss_and_grad(net, imgd, labd)))
    hl, hg = _cache.pop('e2e')
    assert calls.get('parse_ce') == 1 and calls.get('parse_stem_backward') == 1, 'the HIP path did not run'
    gn = float(g64.norm())
    el_t, eg_t = abs(tl - l64) / l64, float((tg - g64).norm()) / gn
    el_h, eg_h = abs(hl - l64) / l64, float((hg - g64).norm()) / gn
    el_f, eg_f = abs(fix_loss - l64) / l64, float((fix_grad - g64).norm()) / gn
    print(f'case {case} arith {arith}: loss rel err HIP {el_h:.2e} ATen {el_t:.2e} fixture {el_f:.2e}; gradient rel L2 HIP {eg_h:.2e} ATen {eg_t:.2e} '
          f'fixture {eg_f:.2e}; HIP vs fixture: loss {abs(hl - fix_loss) / l64:.2e} gradient {float((hg - fix_grad).norm()) / gn:.2e}')
    assert eg_h <= 4 * eg_t
    assert el_h <= 4 * el_t
    assert float((hg - fix_grad).norm()) / gn <= 4 * eg_t + eg_f
    assert abs(hl - fix_loss) / l64 <= 4 * el_t + el_f


# one cross_entropy(...).backward() on the HIP path, by entry point
FUSED_CALLS = {'modconv2d': 32 + 31, 'modconv_act_backward': 10, 'parse_join': 11 + 13, 'plane_sums': 4 + 4, 'resize_bilinear': 2,
               'resize_bilinear_backward': 2, 'maxpool3s2': 1, 'maxpool3s2_backward': 1, 'parse_ce': 1, 'parse_ce_backward': 1,
               'parse_stem_backward': 1}


def test_routing_launch_counts_and_reproducibility(gpu_device):
    from torch_utils import hip_plugin
    from training import parse_loss
    img, lab, l64, g64, _, _ = _float64(0)
    net, imgd, labd = _gpu_net(gpu_device), img.to(gpu_device), lab.to(gpu_device)
    with _switches(True):
        leaf = imgd.clone().requires_grad_(True)
        assert _calls_of(lambda: parse_loss.cross_entropy(net, leaf, labd).backward()) == FUSED_CALLS
        runs = [_loss_and_grad(net, imgd, labd) for _ in range(2)]
        assert runs[0][0] == runs[1][0] and torch.equal(runs[0][1], runs[1][1]), 'two fused runs are bit-identical'
        assert torch.equal(leaf.grad.cpu().double(), runs[0][1])
        # fresh temporaries that start from NaNs change nothing
        _dirty(gpu_device)
        again = _loss_and_grad(net, imgd, labd)
        assert again[0] == runs[0][0] and torch.equal(again[1], runs[0][1]), 'the fused pass read memory it had not written'
        # what takes the PyTorch definition, and still agrees with it (float64, FALLBACK_TOL)
        net64 = R.parser(dtype=torch.float64)

        def plain(n, x, t, want=None):
            got = []
            with _deterministic_aten():
                calls = _calls_of(lambda: got.append(_loss_and_grad(n, x, t)))
            wl, wg = want if want is not None else R.definition(net64, x.cpu().double(), t.cpu())
            el, eg = abs(got[0][0] - float(wl)) / float(wl), float((got[0][1] - wg).norm() / wg.norm())
            print(f'fall-back route: loss rel err {el:.2e}, gradient rel L2 {eg:.2e}, calls {calls}')
            assert el <= FALLBACK_TOL and eg <= FALLBACK_TOL
            return calls
        p = net.cp.resnet.conv1.weight
        p.requires_grad_(True)
        try:
            assert plain(net, imgd, labd, (l64, g64)) == {}, 'a trainable parameter'
        finally:
            p.requires_grad_(False)
        assert plain(R.parser(), img, lab, (l64, g64)) == {}, 'a CPU image'
        g = torch.Generator().manual_seed(72)          # (random, not a zero-padded image: flat borders put ReLUs and pool windows on exact ties)
        x72, t72 = torch.rand(1, 3, 72, 72, generator=g) * 2 - 1, torch.randint(0, 20, (1, 72, 72), generator=g)
        assert plain(net, x72.to(gpu_device), t72.to(gpu_device)) == {}, 'a 72 x 72 image'
    with _switches(False):
        assert _calls_of(lambda: _loss_and_grad(net, imgd, labd)) == {}
    assert hip_plugin.exclusive_violations()[0] == 0


def test_project_with_parse_distance_on_gpu(gpu_device):
    from training import parse_loss, projection, triplane
    torch.manual_seed(0)
    G = triplane.TriPlaneGenerator(triplane.tiny_spec()).eval().to(gpu_device)
    c = triplane.camera_label(0.2)
    target = torch.rand(3, G.img_resolution, G.img_resolution, generator=torch.Generator().manual_seed(1)) * 255
    tgt = target[None].to(gpu_device)
    with _switches(True):
        d = parse_loss.parse_distance(tgt, _gpu_net(gpu_device), weight=0.1, base=projection.l2_distance(tgt))
        p = projection.Projector(G, target, c, num_steps=2, w_avg_samples=32, distance=d)
        start = p.pivot().clone()
        losses = []
        calls = _calls_of(lambda: losses.extend(float(p.step(i)) for i in range(2)))
    assert calls.get('parse_ce') == 2 and calls.get('parse_stem_backward') == 2
    assert all(v == v and abs(v) != float('inf') for v in losses)
    assert bool(torch.isfinite(p.pivot()).all()) and not torch.equal(p.pivot(), start)
