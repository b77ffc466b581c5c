"""The ArcFace identity loss on the GPU (training/id_loss.py over csrc/id_loss.hip, csrc/parse_loss.hip, csrc/modconv.hip): every new pass
alone against float64 torch on the same fp32 inputs beside the ATen fp32 operator, the whole loss and its image gradient against float64
and the reference's fixture beside the module's own ATen path, the routing rules with the launch counts, reproducibility.

Bound of a pass: 4 x the error of the ATen fp32 operator on the same inputs and device, with a floor of one fp32 ulp of the largest
magnitude (the convention of tests/test_gpu_parse_loss.py)."""

import contextlib

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import id_loss_ref as R

pytestmark = pytest.mark.gpu


def _plugin(gpu_device):
    from torch_utils import hip_plugin
    hip_plugin.load()
    return hip_plugin.IdLossPlugin


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
@pytest.mark.parametrize('shape', [(2, 3, 256, 256), (1, 3, 512, 512)])
def test_prep_and_its_adjoint(gpu_device, shape):
    P = _plugin(gpu_device)
    f = shape[2] // 256
    x, dy = _rand(shape, 1), _rand((shape[0], 3, 112, 112), 2)
    xd, dyd = x.to(gpu_device), dy.to(gpu_device)
    y = P.prep(xd)
    assert tuple(y.shape) == (shape[0], 3, 112, 112)
    assert _within(y, R.prep_definition(x.double()), R.prep_definition(xd), 'prep')
    # the window edges by value: rows floor(188 i / 112) .. ceil(188 (i + 1) / 112) - 1 (+ 35), columns likewise (+ 32), of the block means
    blocks = F.avg_pool2d(x.double(), f) if f > 1 else x.double()
    yc = y.cpu().double()
    for i, (lo, hi) in {0: (0, 2), 55: (92, 94), 56: (94, 96), 111: (186, 188)}.items():
        assert (lo, hi) == (188 * i // 112, -(-188 * (i + 1) // 112))
        for j, (clo, chi) in {0: (0, 2), 56: (94, 96), 111: (186, 188)}.items():
            want = blocks[:, :, 35 + lo:35 + hi, 32 + clo:32 + chi].mean(dim=(2, 3))
            assert float((yc[:, :, i, j] - want).abs().max()) <= 1e-6 * max(float(want.abs().max()), 1.0), (i, j)
    dx = P.prep_backward(dyd, shape[2:])
    assert dx.shape == x.shape
    assert _within(dx, _aten_vjp(R.prep_definition, x.double(), dy.double()), _aten_vjp(R.prep_definition, xd, dyd), 'adjoint')
    outside = dx.clone()
    outside[:, :, 35 * f:223 * f, 32 * f:220 * f] = 0
    assert float(outside.abs().max()) == 0.0 and not bool(torch.signbit(outside).any()), 'an exact 0 outside the crop'
    assert torch.equal(P.prep_backward(dyd, shape[2:]), dx) and torch.equal(P.prep(xd), y)


@pytest.mark.parametrize('shape', [(2, 5, 7, 9), (1, 16, 28, 28)])          # the second: 16-byte accesses
def test_prelu_and_its_gradient_are_bit_equal_to_aten(gpu_device, shape):
    """Slopes include 0 and negative values, inputs include exact zeros (ATen multiplies x = 0 by the slope, forward and backward).  The
    gradient also from a cropped view, as the stride-2 blocks pass it."""
    P = _plugin(gpu_device)
    n, c, h, w = shape
    x = _rand(shape, 3)
    x[torch.rand(shape, generator=torch.Generator().manual_seed(4)) < 0.2] = 0.0
    a = _rand((c,), 5, 0.5)
    a[0], a[1] = 0.0, -0.75
    xd, ad = x.to(gpu_device), a.to(gpu_device)
    y = P.prelu(xd, ad)
    assert torch.equal(y, F.prelu(xd, ad))
    dy = _rand(shape, 6).to(gpu_device)
    want = _aten_vjp(lambda t: F.prelu(t, ad), xd, dy)
    assert torch.equal(P.prelu_backward(dy, xd, ad), want)
    big = _rand((n, c, h + 1, w + 1), 7).to(gpu_device)
    view = big[:, :, 1:h + 1, 1:w + 1]
    assert torch.equal(P.prelu_backward(view, xd, ad), _aten_vjp(lambda t: F.prelu(t, ad), xd, view.contiguous()))


@pytest.mark.parametrize('n,c', [(1, 16), (3, 48), (2, 512)])
def test_se_gate_and_its_gradient(gpu_device, n, c):
    P = _plugin(gpu_device)
    r = c // 16
    s, dg = _rand((n, c, 1, 1), 8, 0.5), _rand((n, c, 1, 1), 9)
    w1, w2 = _rand((r, c, 1, 1), 10, c ** -0.5), _rand((c, r, 1, 1), 11, 1.0)
    gate = lambda t, a, b: torch.sigmoid(F.conv2d(F.relu(F.conv2d(t, a)), b))
    sd, dgd, w1d, w2d = (t.to(gpu_device) for t in (s, dg, w1, w2))
    g = P.se_gate(sd, w1d, w2d)
    assert g.shape == s.shape
    assert _within(g, gate(s.double(), w1.double(), w2.double()), gate(sd, w1d, w2d), 'gate')
    ds = P.se_gate_backward(sd, w1d, w2d, g, dgd)
    want = _aten_vjp(lambda t: gate(t, w1.double(), w2.double()), s.double(), dg.double())
    assert _within(ds, want, _aten_vjp(lambda t: gate(t, w1d, w2d), sd, dgd), 'gate gradient')
    assert torch.equal(P.se_gate(sd, w1d, w2d), g) and torch.equal(P.se_gate_backward(sd, w1d, w2d, g, dgd), ds)


@pytest.mark.parametrize('n,K,M', [(1, 784, 8), (3, 3136, 40), (3, 25088, 512)])
def test_linear_and_its_input_gradient(gpu_device, n, K, M):
    """K = 784 is less than one slice of 2048, 3136 and 25088 are no multiples of it (the last slice is partial); M = 8 and 40 are less than
    the 64 rows of a gradient slice, M = 512 is 8 of them.  Two runs are bit-identical."""
    P = _plugin(gpu_device)
    x, w, b, dy = _rand((n, K), 12), _rand((M, K), 13, K ** -0.5), _rand((M,), 14), _rand((n, M), 15)
    xd, wd, bd, dyd = (t.to(gpu_device) for t in (x, w, b, dy))
    y = P.linear(xd, wd, bd)
    assert _within(y, F.linear(x.double(), w.double(), b.double()), F.linear(xd, wd, bd), 'linear')
    assert _within(P.linear(xd, wd), F.linear(x.double(), w.double()), F.linear(xd, wd), 'linear without bias')
    dx = P.linear_backward_input(dyd, wd)
    assert tuple(dx.shape) == (n, K)
    assert _within(dx, dy.double() @ w.double(), dyd @ wd, 'input gradient')
    assert torch.equal(P.linear(xd, wd, bd), y) and torch.equal(P.linear_backward_input(dyd, wd), dx)


def test_linear_odd_rows_and_more_images_than_one_launch(gpu_device):
    """M = 13: a wave with one row only and waves without any; n = 11: two launches of 8 and 3 images."""
    P = _plugin(gpu_device)
    x, w, dy = _rand((11, 2052), 16), _rand((13, 2052), 17, 0.02), _rand((11, 13), 18)
    xd, wd, dyd = (t.to(gpu_device) for t in (x, w, dy))
    assert _within(P.linear(xd, wd), F.linear(x.double(), w.double()), F.linear(xd, wd), 'linear')
    assert _within(P.linear_backward_input(dyd, wd), dy.double() @ w.double(), dyd @ wd, 'input gradient')


@pytest.mark.parametrize('n,M,dloss', [(1, 8, 1.0), (3, 512, 0.7), (3, 8, 1.0)])
def test_head_and_its_gradient(gpu_device, n, M, dloss):
    P = _plugin(gpu_device)
    f, t = _rand((n, M), 19, 3.0), F.normalize(_rand((n, M), 20), dim=1)
    fn = lambda a, b: (1 - (a / a.norm(dim=1, keepdim=True) * b).sum(1)).mean()
    fd, td = f.to(gpu_device), t.to(gpu_device)
    e, norm, loss = P.head(fd, td)
    assert _within(e, f.double() / f.double().norm(dim=1, keepdim=True), fd / fd.norm(dim=1, keepdim=True), 'embedding')
    assert _within(norm, f.double().norm(dim=1), fd.norm(dim=1), 'norm')
    assert loss.ndim == 0 and _within(loss, fn(f.double(), t.double()), fn(fd, td), 'loss')
    dl = torch.tensor([dloss], device=gpu_device)
    df = P.head_backward(e, td, norm, dl)
    want = _aten_vjp(lambda a: fn(a, t.double()), f.double(), torch.tensor(dloss, dtype=torch.float64))
    assert _within(df, want, _aten_vjp(lambda a: fn(a, td), fd, dl[0]), 'gradient')
    e2, norm2, none = P.head(fd)
    assert none is None and torch.equal(e2, e) and torch.equal(norm2, norm) and torch.equal(P.head_backward(e, td, norm, dl), df)


# ---- end to end --------------------------------------------------------------------------------------------------------------------------------
@contextlib.contextmanager
def _switches(fused, arith=0):
    from training import id_loss
    old = id_loss.fused, id_loss.arith
    id_loss.fused, id_loss.arith = fused, arith
    try:
        yield
    finally:
        id_loss.fused, id_loss.arith = old


@contextlib.contextmanager
def _deterministic_aten():
    old = torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark
    torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark = True, False
    try:
        yield
    finally:
        torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark = old


_cache = {}


def _crit(spec, gpu_device):
    if spec not in _cache:
        _cache[spec] = R.idloss(getattr(R, spec), device=gpu_device)
    return _cache[spec]


def _inputs(spec, shape):
    """(y_hat, y, float64 loss, gradient, e(y)) of a case, computed once: the fixture's first case for IR-SE50, seeded smooth images otherwise."""
    key = (spec, shape)
    if key not in _cache:
        if spec == 'IR_SE50':
            fx = R.fixture(0)
            y_hat, y = fx['y_hat'], fx['y']
        else:
            y_hat, y = R.to_float(R.smooth_images(shape, 31)), R.to_float(R.smooth_images(shape, 32))
        l64, g64, _, t64 = R.loss64(R.backbone(getattr(R, spec)), y_hat, y, getattr(R, spec)['units'])
        _cache[key] = (y_hat, y, l64, g64, t64)
    return _cache[key]


def _loss_and_grad(crit, img, feats):
    leaf = img.clone().requires_grad_(True)
    loss = crit.distance_to(leaf, feats)
    (g,) = torch.autograd.grad(loss, [leaf])
    return float(loss.detach()), g.cpu().double()


def _calls_of(fn):
    from torch_utils import hip_plugin
    before = dict(hip_plugin.CALLS)
    fn()
    return {k: v - before.get(k, 0) for k, v in hip_plugin.CALLS.items() if v != before.get(k, 0)}


def fused_calls(units, shortcut_convs=3):
    """One `distance_to(...).backward()` on the HIP path, by entry point: B blocks, S of them with a convolution
    on the shortcut."""
    B, S = sum(units), shortcut_convs
    return {'id_prep': 1, 'modconv2d': 2 * (1 + 2 * B + S), 'prelu': 1 + B, 'parse_join': 2 * B + 2 * B, 'plane_sums': B + B, 'se_gate': B,
            'linear': 1, 'id_head': 1, 'id_head_backward': 1, 'linear_backward_input': 1, 'se_gate_backward': B, 'prelu_backward': 1 + B,
            'id_prep_backward': 1}


def _errors(crit, y_hat, y, t64, l64, g64, arith, gpu_device):
    """(loss relative error, gradient relative L2) of the HIP path and of the module's ATen path (deterministic algorithms requested: its
    default ones are not reproducible on this GPU) against float64, with the targets taken from float64 on both."""
    imgd, feats = y_hat.to(gpu_device), t64.float().to(gpu_device)
    with _switches(False), _deterministic_aten():
        tl, tg = _loss_and_grad(crit, imgd, feats)
    with _switches(True, arith):
        calls = _calls_of(lambda: _cache.__setitem__('run', _loss_and_grad(crit, imgd, feats)))
    hl, hg = _cache.pop('run')
    assert calls.get('id_head') == 1 and calls.get('id_prep_backward') == 1, 'the HIP path did not run'
    gn = float(g64.norm())
    return (abs(hl - l64) / l64, float((hg - g64).norm()) / gn), (abs(tl - l64) / l64, float((tg - g64).norm()) / gn), hl, hg


@pytest.mark.parametrize('arith', [0, 1], ids=['default', 'fp32'])
@pytest.mark.parametrize('spec,shape', [('NARROW', (2, 3, 256, 256)), ('NARROW', (1, 3, 512, 512)), ('SHORT', (2, 3, 256, 256)), ('SHORT', (1, 3, 512, 512))])
def test_end_to_end_against_float64(gpu_device, spec, shape, arith):
    """Loss: relative error; image gradient: relative L2 (the measures of tests/test_gpu_parse_loss.py).  Bound: 4 x the error of the
    module's `fused = False` ATen path on the same GPU and inputs, with a floor of one fp32 ulp (2^-23, relative).
    Measured on an MI355X (HIP / ATen): gradient 4.4e-7 .. 5.1e-7 / 7.4e-7 .. 9.0e-7, loss 3.3e-9 .. 1.0e-7 / 7.6e-8 .. 4.6e-7 over the eight
    cases."""
    y_hat, y, l64, g64, t64 = _inputs(spec, shape)
    (el_h, eg_h), (el_t, eg_t), _, hg = _errors(_crit(spec, gpu_device), y_hat, y, t64, l64, g64, arith, gpu_device)
    floor = 2.0 ** -23
    print(f'{spec} {shape} arith {arith}: loss rel err HIP {el_h:.2e} ATen {el_t:.2e}; gradient rel L2 HIP {eg_h:.2e} ATen {eg_t:.2e}; floor {floor:.2e}')
    assert eg_h <= max(4 * eg_t, floor)
    assert el_h <= max(4 * el_t, floor)
    f = shape[2] // 256
    hg[:, :, 35 * f:223 * f, 32 * f:220 * f] = 0
    assert float(hg.abs().max()) == 0.0


def test_ir_se50_against_the_fixture(gpu_device):
    """The full IR-SE50 on the fixture's 256 x 256 case.  Against float64: 4 x the ATen error (floor 2^-23); against the fixture (the
    reference's fp32 CPU run, itself e_fix away from float64): 4 x the ATen error + e_fix, by the triangle inequality.  The gradient is
    compared on the fixture's samples (every 4th row and column inside the crop).
    Measured on an MI355X: gradient HIP 4.7e-7, ATen 8.9e-7, fixture samples 1.2e-6, HIP against the fixture 1.3e-6; loss 4.3e-8 / 1.2e-7 /
    1.2e-7 / 7.9e-8; embeddings (max error) 8.1e-8 / 2.2e-7 / 1.8e-7."""
    y_hat, y, l64, g64, t64 = _inputs('IR_SE50', R.CASES[0])
    fx = R.fixture(0)
    crit = _crit('IR_SE50', gpu_device)
    (el_h, eg_h), (el_t, eg_t), hl, hg = _errors(crit, y_hat, y, t64, l64, g64, 0, gpu_device)
    floor = 2.0 ** -23
    s64, sfix, sh = R.crop_samples(g64), fx['grad_samples'].double(), R.crop_samples(hg)
    sn = float(s64.norm())
    el_f, eg_f = abs(fx['loss'] - l64) / l64, float((sfix - s64).norm()) / sn
    el_hf, eg_hf = abs(hl - fx['loss']) / l64, float((sh - sfix).norm()) / sn
    print(f'IR-SE50: loss rel err HIP {el_h:.2e} ATen {el_t:.2e} fixture {el_f:.2e}; gradient rel L2 HIP {eg_h:.2e} ATen {eg_t:.2e} fixture (samples) '
          f'{eg_f:.2e}; HIP vs fixture: loss {el_hf:.2e} gradient samples {eg_hf:.2e}; floor {floor:.2e}')
    assert eg_h <= max(4 * eg_t, floor) and el_h <= max(4 * el_t, floor)
    assert eg_hf <= max(4 * eg_t, floor) + eg_f and el_hf <= max(4 * el_t, floor) + el_f
    # the embeddings of the target through the fused forward against the fixture's
    with _switches(True):
        e = crit.features(y.to(gpu_device)).cpu().double()
    with _switches(False), _deterministic_aten():
        e_t = crit.features(y.to(gpu_device)).cpu().double()
    err_h, err_t, err_f = (float((a - t64).abs().max()) for a in (e, e_t, fx['feats'].double()))
    ulp = float(np.spacing(np.float32(float(t64.abs().max()))))
    print(f'IR-SE50 embeddings: max err HIP {err_h:.2e} ATen {err_t:.2e} fixture {err_f:.2e}; one ulp {ulp:.2e}')
    assert err_h <= max(4 * err_t, ulp) and float((e - fx['feats'].double()).abs().max()) <= max(4 * err_t, ulp) + err_f


def _dirty(device):
    """Leave NaNs in the allocator's free blocks, so that the next torch.empty of any size up to 64 MiB starts from them."""
    blocks = [torch.full((1 << s,), float('nan'), device=device) for s in (10, 14, 16, 18, 20, 22, 24) for _ in range(4)]
    torch.cuda.synchronize()
    del blocks


# fp32 dot products of K <= 576 terms (the narrow nets) carry a relative error of about sqrt(K) 2^-24 = 1.4e-6 of the size of their terms;
# the loss passes 2 B + 2 such layers in a row and the gradient twice as many: for B = 6, sqrt(28) x 1.4e-6 = 7.6e-6 as independent errors
# (the convention of tests/test_gpu_parse_loss.py).  A route that computed anything else is off by 1e-2 or more.
FALLBACK_TOL = 7.6e-6


def test_routing_launch_counts_and_reproducibility(gpu_device):
    from torch_utils import hip_plugin
    from training import id_loss
    spec, shape = 'NARROW', (2, 3, 256, 256)
    y_hat, y, l64, g64, t64 = _inputs(spec, shape)
    crit = _crit(spec, gpu_device)
    imgd, feats = y_hat.to(gpu_device), t64.float().to(gpu_device)
    with _switches(True):
        leaf = imgd.clone().requires_grad_(True)
        assert _calls_of(lambda: crit.distance_to(leaf, feats).backward()) == fused_calls(R.NARROW['units'])
        forward_only = _calls_of(lambda: crit.features(imgd))
        assert forward_only.get('id_head') == 1 and 'id_head_backward' not in forward_only and forward_only.get('modconv2d') == 1 + 2 * 6 + 3
        runs = [_loss_and_grad(crit, imgd, feats) for _ in range(2)]
        assert runs[0][0] == runs[1][0] and torch.equal(runs[0][1], runs[1][1]), 'two fused runs are bit-identical'
        assert torch.equal(leaf.grad.cpu().double(), runs[0][1])
        _dirty(gpu_device)
        again = _loss_and_grad(crit, imgd, feats)
        assert again[0] == runs[0][0] and torch.equal(again[1], runs[0][1]), 'the fused pass read memory it had not written'
        # forward(y_hat, y, x): the reference's triple, its loss on the HIP path
        yd = y.to(gpu_device)
        out = []
        calls = _calls_of(lambda: out.append(crit(imgd, yd, yd)))
        loss, sim, logs = out[0]
        assert calls.get('id_head') == 2 and abs(float(loss) - l64) <= 1e-4 and sim == pytest.approx(-float(loss), abs=1e-5) and len(logs) == 2

        # what takes the PyTorch definition, and still agrees with it (float64, FALLBACK_TOL)
        def plain(c, x, t, want):
            got = []
            with _deterministic_aten():
                calls = _calls_of(lambda: got.append(_loss_and_grad(c, x, t)))
            el, eg = abs(got[0][0] - want[0]) / want[0], float((got[0][1] - want[1]).norm() / want[1].norm())
            print(f'fall-back route: loss rel err {el:.2e}, gradient rel L2 {eg:.2e}, calls {calls}')
            assert el <= FALLBACK_TOL and eg <= FALLBACK_TOL
            return calls
        p = crit.facenet.input_layer[0].weight
        p.requires_grad_(True)
        try:
            assert plain(crit, imgd, feats, (l64, g64)) == {}, 'a trainable parameter'
        finally:
            p.requires_grad_(False)
        assert plain(R.idloss(R.NARROW), y_hat, t64.float(), (l64, g64)) == {}, 'a CPU image'
        sd = {k: (v.double() if v.is_floating_point() else v) for k, v in R.backbone(R.NARROW).state_dict().items()}
        tb = R.embed(sd, y[:1].double(), R.NARROW['units'])
        for bad in ((384, 384), (256, 320)):                        # the reference pools to 256 x 256 only when the HEIGHT is not 256
            xb = R.to_float(R.smooth_images((1, 3, 384, 384), 33))[:, :, :bad[0], :bad[1]].contiguous()
            leaf64 = xb.double().requires_grad_(True)
            l = (1 - (R.embed(sd, leaf64, R.NARROW['units']) * tb).sum(1)).mean()
            (gb,) = torch.autograd.grad(l, [leaf64])
            assert plain(crit, xb.to(gpu_device), tb.float().to(gpu_device), (float(l.detach()), gb)) == {}, f'a {bad[0]} x {bad[1]} image'
        assert not id_loss._on_hip(crit.facenet, imgd.half()), 'an fp16 image'
        ir = R.idloss(R.NARROW, device=gpu_device, mode='ir')
        assert _calls_of(lambda: ir.features(imgd)) == {}, "mode='ir'"
    with _switches(False):
        assert _calls_of(lambda: _loss_and_grad(crit, imgd, feats)) == {}
    assert hip_plugin.exclusive_violations()[0] == 0


def test_project_with_id_distance_on_gpu(gpu_device):
    """Three projector steps with the identity term on the HIP path against the same steps with `fused = False`.  The tiny generator's
    images are repeated to 256 x 256 (an exact operation) so that the fused route takes them.  Bound per step's loss: the end-to-end bound's
    reasoning applied to a trajectory - each step's gradient differs by at most the sum of both paths' fp32 errors (FALLBACK_TOL each, relative
    L2), Adam turns a relative gradient error into the same relative error of its update, and the loss is Lipschitz in the pivot with the
    gradient as its constant: after k steps the losses differ by at most k x 2 x FALLBACK_TOL, relative."""
    from training import id_loss, projection, triplane
    crit = _crit('SHORT', gpu_device)

    def run(fused):
        torch.manual_seed(0)
        G = triplane.TriPlaneGenerator(triplane.tiny_spec()).eval().to(gpu_device)
        c = triplane.camera_label(0.2)
        target = torch.rand(3, G.img_resolution, G.img_resolution, generator=torch.Generator().manual_seed(1)) * 255
        rep = 256 // G.img_resolution
        up = lambda t: t.repeat_interleave(rep, dim=2).repeat_interleave(rep, dim=3)
        tgt = target[None].to(gpu_device)
        with _switches(fused), _deterministic_aten():
            inner = id_loss.id_distance(up(tgt), crit)
            p = projection.Projector(G, target, c, num_steps=3, w_avg_samples=32, distance=lambda images: inner(up(images)))
            start = p.pivot().clone()
            losses = []
            calls = _calls_of(lambda: losses.extend(float(p.step(i)) for i in range(3)))
        assert bool(torch.isfinite(p.pivot()).all()) and not torch.equal(p.pivot(), start)
        return losses, calls
    hip, calls = run(True)
    aten, calls_aten = run(False)
    assert calls.get('id_head') == 3 and calls.get('id_prep_backward') == 3 and 'id_head' not in calls_aten
    print(f'projector losses: HIP {hip}, ATen {aten}')
    for k, (a, b) in enumerate(zip(hip, aten)):
        assert abs(a - b) <= (k + 1) * 2 * FALLBACK_TOL * abs(b), (k, a, b)
