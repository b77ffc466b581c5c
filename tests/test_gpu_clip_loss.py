"""The CLIP image-text loss on the GPU (training/clip_loss.py over csrc/clip_loss.hip, csrc/modconv.hip, csrc/res_join.hip,
csrc/id_loss.hip): every new pass alone against float64 torch on the same fp32 inputs beside the ATen fp32 operator, the whole loss and
its image gradient against float64 beside the module's own ATen path, the routing rules, reproducibility, the projector closure.

Bound everywhere (tests/test_gpu_id_loss.py::_within): max |got - want| <= max(4 max |aten - want|, one fp32 ulp of max |want|), `want` the
float64 result on the same fp32 inputs, `aten` the module's PyTorch definition in fp32 on the same device, or the corresponding torch
operator for a single launch."""

import contextlib

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import clip_loss_ref as R

pytestmark = pytest.mark.gpu


def _plugin(gpu_device):
    from torch_utils import hip_plugin
    hip_plugin.load()
    return hip_plugin.ClipLossPlugin


def _within(got, want, aten, what=''):
    """max |got - want| <= max(4 max |aten - want|, one fp32 ulp of max |want|); want: float64."""
    want = want.detach().cpu().double()
    err, ref = float((got.detach().cpu().double() - want).abs().max()), float((aten.detach().cpu().double() - want).abs().max())
    floor = float(np.spacing(np.float32(float(want.abs().max()))))
    print(f'{what}: max err {err:.3e}, ATen {ref:.3e}, one ulp of the largest magnitude {floor:.3e}')
    return err <= max(4 * ref, floor)


def _vjp(fn, x, dy):
    leaf = x.detach().clone().requires_grad_(True)
    (g,) = torch.autograd.grad(fn(leaf), [leaf], dy)
    return g


@contextlib.contextmanager
def _switches(fused, arith=0):
    from training import clip_loss
    old = clip_loss.fused, clip_loss.arith
    clip_loss.fused, clip_loss.arith = fused, arith
    try:
        yield
    finally:
        clip_loss.fused, clip_loss.arith = old


def _calls_of(fn):
    from torch_utils import hip_plugin
    before = dict(hip_plugin.CALLS)
    fn()
    return {k: v - before.get(k, 0) for k, v in hip_plugin.CALLS.items() if v != before.get(k, 0)}


# ---- each pass alone ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('p', [32, 56])
@pytest.mark.parametrize('S', [32, 64, 96, 160, 224])
def test_prep_and_its_adjoint(gpu_device, S, p):
    """k = S / 32 = 1 (every source pixel seven times in a row), 2, 3, 5 (windows that straddle source pixels unevenly), 7 (the identity);
    p = 32 and 56 (7 x 7 and 4 x 4 patches); with and without the normalisation.  Two runs are bit-identical."""
    P = _plugin(gpu_device)
    g = 224 // p
    x, dcol = R.images((2, 3, S, S), S + p), R.rows((2, 3 * p * p, g, g), 1)
    xd, dd = x.to(gpu_device), dcol.to(gpu_device)
    for mean, std in ((None, None), (torch.tensor(R.CLIP_MEAN), torch.tensor(R.CLIP_STD))):
        md, sd = (None, None) if mean is None else (mean.to(gpu_device), std.to(gpu_device))
        m64, s64 = (None, None) if mean is None else (mean.double(), std.double())
        col = P.prep(xd, p, md, sd)
        assert tuple(col.shape) == (2, 3 * p * p, g, g)
        assert _within(col, R.prep_definition(x.double(), p, m64, s64), R.prep_definition(xd, p, md, sd), f'prep S {S} p {p} affine {mean is not None}')
        if S == 224 and mean is None:
            assert torch.equal(col, R.unfold(xd, p)), 'k = 7: the identity'
        dx = P.prep_backward(dd, (S, S), p, sd)
        assert dx.shape == x.shape
        want = _vjp(lambda t: R.prep_definition(t, p, m64, s64), x.double(), dcol.double())
        assert _within(dx, want, _vjp(lambda t: R.prep_definition(t, p, md, sd), xd, dd), 'adjoint')
        assert torch.equal(P.prep(xd, p, md, sd), col) and torch.equal(P.prep_backward(dd, (S, S), p, sd), dx)


def _ln_inputs(n, C, T, seed):
    x = R.rows((n, C, T), seed) * 1.5 + 0.3
    if T > 1:
        x[:, :, 1] = 0.37                                                         # one token is constant: variance 0
    gamma, beta = torch.rand(C, generator=torch.Generator().manual_seed(seed + 1)) + 0.5, R.rows((C,), seed + 2) * 0.1
    return x, gamma, beta, R.rows((n, C, T), seed + 3), R.rows((n, C, T), seed + 4)


@pytest.mark.parametrize('C,T', [(8, 5), (60, 17), (768, 50), (768, 1)])
def test_layernorm_and_its_gradient(gpu_device, C, T):
    """Over the channels of each token of [n, C, T]; one token constant; the gradient with and without the residual stream's addend.
    (768, 1) is `ln_post`: once on a one-token map and once on the class column of a 50-token map, read in place."""
    P = _plugin(gpu_device)
    n = 2
    x, gamma, beta, dy, add = _ln_inputs(n, C, T, 20)
    dev = lambda *ts: (t.to(gpu_device) for t in ts)
    xd, gd, bd, dyd, addd = dev(x, gamma, beta, dy, add)
    y, mean, rstd = P.layernorm(xd, gd, bd)
    assert _within(y, R.layernorm_definition(x.double(), gamma.double(), beta.double()), R.layernorm_definition(xd, gd, bd), f'layernorm {C} {T}')
    m64 = x.double().mean(dim=1)
    assert _within(mean, m64, xd.mean(dim=1), 'mean') and tuple(rstd.shape) == (n, T)
    if T > 1:
        assert float((y[:, :, 1] - bd).abs().max()) <= 1e-6, 'a constant token normalises to beta'
    for a, ad in ((None, None), (add, addd)):
        want = _vjp(lambda t: R.layernorm_definition(t, gamma.double(), beta.double()), x.double(), dy.double()) + (0 if a is None else a.double())
        aten = _vjp(lambda t: R.layernorm_definition(t, gd, bd), xd, dyd)
        aten = aten if a is None else aten + ad
        # the constant token's gradient is rstd = 316 times an fp32 cancellation in ATen too: it is compared apart, against its own scale
        keep = [t for t in range(T) if t != 1] if T > 1 else [0]
        dx = P.layernorm_backward(dyd, xd, gd, mean, rstd, ad)
        assert _within(dx[:, :, keep], want[:, :, keep], aten[:, :, keep], f'gradient, addend {a is not None}')
        assert _within(dx, want, aten, 'gradient with the constant token')
        assert torch.equal(P.layernorm_backward(dyd, xd, gd, mean, rstd, ad), dx)
    assert torch.equal(P.layernorm(xd, gd, bd)[0], y)
    if T == 1:
        wide = R.rows((n, C, 50), 30)
        wide[:, :, :1] = x
        wd = wide.to(gpu_device)
        y1, m1, r1 = P.layernorm(wd, gd, bd, 1)
        assert torch.equal(y1, y) and torch.equal(m1, mean) and torch.equal(r1, rstd)
        dw = P.layernorm_backward(dyd, wd, gd, m1, r1)
        assert tuple(dw.shape) == (n, C, 50) and torch.equal(dw[:, :, :1], P.layernorm_backward(dyd, xd, gd, mean, rstd))
        assert float(dw[:, :, 1:].abs().max()) == 0.0 and not bool(torch.signbit(dw[:, :, 1:]).any()), 'an exact 0 past the class token'


@pytest.mark.parametrize('C,T', [(8, 5), (60, 17), (768, 50)])
def test_embed_and_its_gradient(gpu_device, C, T):
    """Patch tokens + the class / positional table -> ln_pre; the gradient goes to the patch tokens, the class column is dropped.  One
    token is constant (the table's column and the patches' are set so)."""
    P = _plugin(gpu_device)
    n = 2
    tok, gamma, beta, dy, _ = _ln_inputs(n, C, T, 40)
    table = R.rows((C, T), 45) * 0.2
    patches = (tok - table)[:, :, 1:].contiguous()
    patches[:, :, 0] = 0.25
    table[:, 1] = 0.125                                                            # token 1 = 0.375 in every channel
    pd, td, gd, bd, dyd = (t.to(gpu_device) for t in (patches, table, gamma, beta, dy))
    y, mean, rstd = P.embed(pd, td, gd, bd)
    want = R.embed_definition(patches.double(), table.double(), gamma.double(), beta.double())
    assert tuple(y.shape) == (n, C, T) and _within(y, want, R.embed_definition(pd, td, gd, bd), f'embed {C} {T}')
    side = int(round((T - 1) ** 0.5))
    if side * side == T - 1:                                                       # the patch convolution's [n, C, g, g] output as it comes
        assert torch.equal(P.embed(pd.reshape(n, C, side, side), td, gd, bd)[0], y)
    dp = P.embed_backward(dyd, pd, td, gd, mean, rstd)
    want = _vjp(lambda t: R.embed_definition(t, table.double(), gamma.double(), beta.double()), patches.double(), dy.double())
    aten = _vjp(lambda t: R.embed_definition(t, td, gd, bd), pd, dyd)
    keep = [t for t in range(T - 1) if t != 0]
    assert dp.shape == patches.shape and _within(dp[:, :, keep], want[:, :, keep], aten[:, :, keep], 'gradient')
    assert _within(dp, want, aten, 'gradient with the constant token')
    assert torch.equal(P.embed(pd, td, gd, bd)[0], y) and torch.equal(P.embed_backward(dyd, pd, td, gd, mean, rstd), dp)


@pytest.mark.parametrize('heads,d,T,qscale', [(1, 4, 2, 1.0), (3, 20, 17, 1.0), (2, 32, 5, 1.0), (12, 64, 50, 1.0), (1, 64, 64, 1.0), (3, 20, 17, 30.0)])
def test_attention_and_its_gradient(gpu_device, heads, d, T, qscale):
    """The smallest shape, odd sizes, ViT-B/32's, the largest the kernel covers, and q scaled by 30: a saturated softmax."""
    P = _plugin(gpu_device)
    n, C = 2, heads * d
    qkv, dout = R.rows((n, 3 * C, T), 50), R.rows((n, C, T), 51)
    qkv[:, :C] *= qscale
    qd, dd = qkv.to(gpu_device), dout.to(gpu_device)
    out = P.attention(qd, heads)
    assert tuple(out.shape) == (n, C, T)
    assert _within(out, R.attention_definition(qkv.double(), heads), R.attention_definition(qd, heads), f'attention {heads} {d} {T} x{qscale}')
    dq = P.attention_backward(qd, dd, heads)
    want = _vjp(lambda t: R.attention_definition(t, heads), qkv.double(), dout.double())
    assert dq.shape == qkv.shape and _within(dq, want, _vjp(lambda t: R.attention_definition(t, heads), qd, dd), 'gradient')
    assert torch.equal(P.attention(qd, heads), out) and torch.equal(P.attention_backward(qd, dd, heads), dq)
    assert bool(torch.isfinite(out).all()) and bool(torch.isfinite(dq).all())


@pytest.mark.parametrize('count', [1, 7, 4099])
def test_quickgelu_and_its_gradient(gpu_device, count):
    """Values up to +-20 (sigmoid saturated on both sides) and an exact 0; 16-byte accesses and, from an address that is no multiple of
    16, the scalar form."""
    P = _plugin(gpu_device)
    x = (torch.rand(count + 1, generator=torch.Generator().manual_seed(60)) * 40 - 20)
    x[0], x[-1] = 0.0, 20.0
    dy = R.rows((count + 1,), 61)
    xd, dd = x.to(gpu_device), dy.to(gpu_device)
    for lo in (0, 1):
        xs, ds, x64, d64 = xd[lo:lo + count], dd[lo:lo + count], x[lo:lo + count].double(), dy[lo:lo + count].double()
        y = P.quickgelu(xs)
        assert _within(y, R.quickgelu_definition(x64), R.quickgelu_definition(xs), f'quickgelu {count} offset {lo}')
        dx = P.quickgelu_backward(ds, xs)
        assert _within(dx, _vjp(R.quickgelu_definition, x64, d64), _vjp(R.quickgelu_definition, xs, ds), 'gradient')
        assert torch.equal(P.quickgelu(xs), y) and torch.equal(P.quickgelu_backward(ds, xs), dx)


@pytest.mark.parametrize('T', [1, 3])
@pytest.mark.parametrize('D', [4, 512])
def test_head_and_its_gradient(gpu_device, D, T):
    P = _plugin(gpu_device)
    n = 3
    f, text, base, dout = R.rows((n, D), 70) * 2, R.rows((T, D), 71) * 3, R.rows((n, D), 72), R.rows((n, T), 73)
    fd, td, bd, dd = (t.to(gpu_device) for t in (f, text, base, dout))
    for b, bdev in ((None, None), (base, bd)):
        out, e, norm, tnorm, avg = P.head(fd, td, bdev)
        b64 = None if b is None else b.double()
        assert tuple(out.shape) == (n, T) and _within(out, R.cosine_rows(f.double(), text.double(), b64), R.cosine_rows(fd, td, bdev), f'head {D} {T} base {b is not None}')
        assert _within(avg, R.cosine_rows(f.double(), text.double(), b64).mean(), R.cosine_rows(fd, td, bdev).mean(), 'mean')
        assert _within(norm, (f.double() - (0 if b is None else b64)).norm(dim=1), (fd - (0 if b is None else bdev)).norm(dim=1), 'norm')
        df = P.head_backward(e, td, norm, tnorm, dd)
        want = _vjp(lambda t: R.cosine_rows(t, text.double(), b64), f.double(), dout.double())
        assert _within(df, want, _vjp(lambda t: R.cosine_rows(t, td, bdev), fd, dd), 'gradient')
        assert torch.equal(P.head(fd, td, bdev)[0], out) and torch.equal(P.head_backward(e, td, norm, tnorm, dd), df)


# ---- the whole loss ----------------------------------------------------------------------------------------------------------------------------
_memo = {}


def _crit(spec, S, gpu_device):
    key = (spec, S)
    if key not in _memo:
        _memo[key] = R.cliploss(getattr(R, spec), S, device=gpu_device)
    return _memo[key]


def _case(spec, S, n):
    """Inputs and the float64 results of one case, computed once: (x, text, base, direction, distance_to's (loss, grad), directional's)."""
    key = ('case', spec, S, n)
    if key not in _memo:
        net = R.visual(getattr(R, spec))
        D = net.output_dim
        x, text, base, direction = R.images((n, 3, S, S), 80 + n), R.rows((3, D), 81), R.rows((n, D), 82), R.rows((D,), 83)
        a = R.loss64(net, x, text)
        b = R.loss64(net, x, direction, base)
        _memo[key] = (x, text, base, direction, (a[0], a[1]), (b[0], b[1]))
    return _memo[key]


def _run(crit, fn):
    """(loss, gradient, path) of fn(leaf) on `crit`."""
    def go(x):
        leaf = x.clone().requires_grad_(True)
        loss = fn(leaf)
        (g,) = torch.autograd.grad(loss, [leaf])
        return loss.detach(), g, crit.last_path
    return go


CASES = [(spec, S, n) for spec in ('NARROW', 'WIDE', 'ODD') for S in (64, 96) for n in (1, 3)] + [('NARROW', 64, 9)]


@pytest.mark.parametrize('spec,S,n', CASES)
def test_end_to_end_against_float64(gpu_device, spec, S, n):
    """`distance_to` and `directional`: loss and image gradient.  narrow-deep (twelve blocks), wide-shallow (ViT-B/32's widths), odd (17
    tokens, head dimension 20, 56 x 56 patches); n = 9 on the narrow net: the final projection in two launches of 8 and 1 images.
    The scalar is the head's own float64 mean of the unrounded rows (one rounding), not an fp32 mean of the rounded rows."""
    crit = _crit(spec, S, gpu_device)
    x, text, base, direction, want_a, want_b = _case(spec, S, n)
    xd, td, bd, dd = (t.to(gpu_device) for t in (x, text, base, direction))
    for what, fn, (l64, g64) in (('distance_to', lambda t: crit.distance_to(t, td), want_a), ('directional', lambda t: crit.directional(t, bd, dd), want_b)):
        with _switches(False):
            tl, tg, path = _run(crit, fn)(xd)
            assert path == 'torch'
        with _switches(True):
            calls = _calls_of(lambda: _memo.__setitem__('run', _run(crit, fn)(xd)))
        hl, hg, path = _memo.pop('run')
        assert path == 'hip' and calls.get('clip_head') == 1 and calls.get('clip_prep_backward') == 1, 'the HIP path did not run'
        assert calls.get('linear') == -(-n // 8) and calls.get('vit_attention') == crit.visual.layers == calls.get('vit_attention_backward')
        assert _within(hl, torch.tensor(l64, dtype=torch.float64), tl, f'{spec} S {S} n {n} {what}: loss')
        assert _within(hg, g64, tg, f'{spec} S {S} n {n} {what}: image gradient')
        assert hg.shape == x.shape


def test_reproducibility_and_forward_rows(gpu_device):
    """Two runs are `torch.equal`, also after the allocator's free blocks were filled with NaNs; `forward` gives the [n, T] rows and
    `features` the embeddings, both on the HIP path."""
    spec, S, n = 'ODD', 96, 3
    crit = _crit(spec, S, gpu_device)
    x, text, base, direction, _, _ = _case(spec, S, n)
    xd, td = x.to(gpu_device), text.to(gpu_device)
    with _switches(True):
        runs = [_run(crit, lambda t: crit.distance_to(t, td))(xd) for _ in range(2)]
        assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
        blocks = [torch.full((1 << s,), float('nan'), device=gpu_device) for s in (10, 14, 16, 18, 20, 22, 24) for _ in range(4)]
        torch.cuda.synchronize()
        del blocks
        again = _run(crit, lambda t: crit.distance_to(t, td))(xd)
        assert torch.equal(again[0], runs[0][0]) and torch.equal(again[1], runs[0][1]), 'the fused pass read memory it had not written'
        rows = crit(xd, td)
        assert crit.last_path == 'hip' and tuple(rows.shape) == (n, 3) and abs(float(rows.mean()) - float(runs[0][0])) <= 2 * R.ulp(float(runs[0][0]))
        f = crit.features(xd)
        assert crit.last_path == 'hip' and not f.requires_grad
    sd = {k: v.double().cpu() for k, v in crit.visual.state_dict().items()}
    f64 = R.embed(sd, x.double(), crit.visual.heads)
    with _switches(False):
        ft = crit.features(xd)
        rt = crit(xd, td)
    assert _within(f, f64, ft, 'embeddings') and _within(rows, R.cosine_rows(f64, text.double()), rt, 'rows')
    from torch_utils import hip_plugin
    assert hip_plugin.exclusive_violations()[0] == 0


def test_what_takes_the_pytorch_definition(gpu_device):
    """65 tokens (p = 28), a trainable parameter and an fp16 image take the PyTorch definition, launch nothing of csrc/clip_loss.hip, and
    agree with float64 (`aten`: the functional restatement of tests/clip_loss_ref.py in fp32 on the same device).  One quantity departs
    from the bound of the module docstring: the gradient of an fp16 image is returned in fp16 by autograd, so half an fp16 ulp of the
    largest gradient (2^-11 max |g|) is added to 4 x the ATen error; `_within`'s fp32 floor cannot hold for a value stored in fp16."""
    S, n = 64, 2
    x, text = R.images((n, 3, S, S), 90), R.rows((2, 32), 91)
    td = text.to(gpu_device)

    def check(crit, xd, what):
        net = crit.visual
        sd32 = {k: v.detach() for k, v in net.state_dict().items()}
        sd64 = {k: v.detach().double().cpu() for k, v in net.state_dict().items()}
        x32 = xd.detach().float()
        x64 = x32.double().cpu()
        loss = lambda sd, xx, tt: R.cosine_rows(R.embed(sd, xx, net.heads), tt).mean()
        leaf64 = x64.clone().requires_grad_(True)
        l64 = loss(sd64, leaf64, text.double())
        (g64,) = torch.autograd.grad(l64, [leaf64])
        leaf32 = x32.clone().requires_grad_(True)
        l32 = loss(sd32, leaf32, td)
        (g32,) = torch.autograd.grad(l32, [leaf32])
        with _switches(True):
            calls = _calls_of(lambda: _memo.__setitem__('run', _run(crit, lambda t: crit.distance_to(t, td))(xd)))
        hl, hg, path = _memo.pop('run')
        assert path == 'torch' and not any(k.startswith(('clip_', 'vit_', 'layernorm', 'quickgelu')) for k in calls), (what, calls)
        assert hg.dtype == xd.dtype
        assert _within(hl, l64, l32, f'{what}: loss')
        if xd.dtype == torch.float32:
            assert _within(hg, g64, g32, f'{what}: image gradient')
        else:                                                                       # the gradient is rounded to fp16 on its way out: one more half ulp
            err = float((hg.double().cpu() - g64).abs().max())
            assert err <= 4 * float((g32.double().cpu() - g64).abs().max()) + 2.0 ** -11 * float(g64.abs().max()), what
    check(_crit('B16', S, gpu_device), x.to(gpu_device), '65 tokens')
    crit = _crit('NARROW', S, gpu_device)
    p = crit.visual.ln_pre.weight
    p.requires_grad_(True)
    try:
        check(crit, x.to(gpu_device), 'a trainable parameter')
    finally:
        p.requires_grad_(False)
    check(crit, x.to(gpu_device).half(), 'an fp16 image')
    with _switches(True):
        assert _run(crit, lambda t: crit.distance_to(t, td))(x.to(gpu_device))[2] == 'hip'


def test_project_with_clip_distance_on_gpu(gpu_device):
    """Three projector steps on the tiny generator (64 x 64 images) with the CLIP term on the HIP path: the loss is finite and the pivot moves."""
    from training import clip_loss, projection, triplane
    crit = _crit('NARROW', 64, gpu_device)
    torch.manual_seed(0)
    G = triplane.TriPlaneGenerator(triplane.tiny_spec()).eval().to(gpu_device)
    assert G.img_resolution == 64
    c = triplane.camera_label(0.2)
    target = torch.rand(3, 64, 64, generator=torch.Generator().manual_seed(1)) * 255
    text = R.rows((2, 32), 95).to(gpu_device)
    with _switches(True):
        d = clip_loss.clip_distance(text, crit, weight=0.5, base=projection.l2_distance(target[None].to(gpu_device)))
        p = projection.Projector(G, target, c, num_steps=3, w_avg_samples=32, distance=d)
        start = p.pivot().clone()
        losses = []
        calls = _calls_of(lambda: losses.extend(float(p.step(i)) for i in range(3)))
    assert calls.get('clip_head') == 3 and calls.get('clip_prep_backward') == 3
    assert all(np.isfinite(v) for v in losses) and bool(torch.isfinite(p.pivot()).all()) and not torch.equal(p.pivot(), start)
