"""The discriminator's adversarial loss on the GPU (training/adv_loss.py over csrc/adv_loss.hip and the convolution, FIR, join and linear
entry points): the four new entry points through the C ABI against float64 on the same fp32 inputs, the whole loss and its image gradient
against the float64 restatement of tests/adv_loss_ref.py beside the module's own `fused = False` path, the routing rules with the launch
counts, and `project()` with `adv_distance`.  DESIGN.md section 5.38."""

import contextlib
import ctypes
import math

import pytest
import torch

import adv_loss_ref as R

pytestmark = pytest.mark.gpu

ULP = 2.0 ** -23


def _lib():
    from torch_utils import hip_plugin
    return hip_plugin.load(), hip_plugin


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _nan(shape, device):
    return torch.full(shape, float('nan'), dtype=torch.float32, device=device)


# ---- the entry points alone ----------------------------------------------------------------------------------------------------------------------
MBSTD = [(1, 4, 4, 4, 4, 1), (4, 6, 4, 4, 2, 2), (4, 5, 2, 3, 4, 1), (8, 16, 4, 4, 4, 1), (6, 8, 4, 4, 0, 1), (8, 512, 4, 4, 4, 1)]


@pytest.mark.parametrize('n,c,h,w,group,features', MBSTD)
def test_minibatch_std_and_its_backward(gpu_device, n, c, h, w, group, features):
    """Through the C entry points into NaN-filled outputs: every element is written; the first C channels are bit copies; the statistic is
    within 2^-23 relative of float64 (computed in float64 and rounded once: twice that rounding); dx is within 2^-23 (|dy| + |term|)
    elementwise; with G = 1 the second term is exactly 0; two runs are bit-equal.  `group` is what the binding passes: min(group_size, n),
    0 for the whole batch.  Measured on an MI355X: statistic 3.0e-9 .. 4.1e-8 relative; dx inside its bound everywhere."""
    lib, hp = _lib()
    g = torch.Generator().manual_seed(n * 1000 + c)
    x = torch.randn(n, c, h, w, generator=g) * 1.5 + 0.3
    dy = torch.randn(n, c + features, h, w, generator=g)
    xd, dyd = x.to(gpu_device), dy.to(gpu_device)
    arg = min(group, n)
    G = arg if arg > 0 else n
    ys, dxs = [], []
    for _ in range(2):
        y, dx = _nan([n, c + features, h, w], gpu_device), _nan([n, c, h, w], gpu_device)
        assert lib.ide3d_minibatch_std(_p(xd), _p(y), n, c, h, w, arg, features, hp._stream(xd)) == 0, lib.ide3d_last_error()
        assert lib.ide3d_minibatch_std_backward(_p(xd), _p(dyd), _p(dx), n, c, h, w, arg, features, hp._stream(xd)) == 0, lib.ide3d_last_error()
        ys.append(y.cpu())
        dxs.append(dx.cpu())
    y, dx = ys[0], dxs[0]
    assert bool(torch.isfinite(y).all()) and bool(torch.isfinite(dx).all()), 'an element was not written'
    assert torch.equal(ys[0], ys[1]) and torch.equal(dxs[0], dxs[1]), 'two runs are bit-equal'
    assert torch.equal(y[:, :c], x)
    y64 = R.mbstd64(x.double(), G, features)
    rel = float(((y[:, c:].double() - y64[:, c:]).abs() / y64[:, c:].abs()).max())
    dx64, term = R.mbstd64_backward(x.double(), dy.double(), G, features)
    excess = float(((dx.double() - dx64).abs() - ULP * (dy[:, :c].double().abs() + term.abs())).max())
    print(f'[{n}, {c}, {h}, {w}] group {group} F {features}: statistic rel err {rel:.2e}; dx error over its bound {excess:.2e} (<= 0 passes)')
    assert rel <= ULP
    assert excess <= 0
    if G == 1:
        assert torch.equal(dx, dy[:, :c])
    # the binding and the layer's inference path launch the same
    P = hp.AdvLossPlugin
    assert torch.equal(P.minibatch_std(xd, group or None, features).cpu(), y) and torch.equal(P.minibatch_std_backward(xd, dyd, group or None, features).cpu(), dx)


@pytest.mark.parametrize('sign', [-1, 1])
@pytest.mark.parametrize('n,M', [(1, 1), (3, 5), (8, 16), (8, 512)])
def test_adv_head_and_its_backward(gpu_device, n, M, sign):
    """(1, 1) runs without cmap.  Rows 0 and 1 (n > 1) are planted at logits of about +30 and -30 beside ordinary ones: exp(30) is finite
    but a naive log(1 + exp(z)) in fp32 returns 0 for softplus(-30) = 9.4e-14 and rounds softplus(30).  Loss, logits and `do` within 2^-23
    relative of float64 (elementwise for `do`; its float64 takes the kernel's own fp32 logits, the entry point's input); everything finite;
    two runs bit-equal.  Measured on an MI355X: logits <= 5.7e-8, loss <= 5.1e-8, `do` <= 5.9e-8."""
    lib, hp = _lib()
    g = torch.Generator().manual_seed(n * 100 + M)
    o = torch.randn(n, M, generator=g)
    cmap = torch.randn(n, M, generator=g) if M > 1 else None
    if n > 1:
        for row, z in ((0, 30.0), (1, -30.0)):
            o[row] = z * math.sqrt(M) * cmap[row] / cmap[row].square().sum()
    od, cd = o.to(gpu_device), None if cmap is None else cmap.to(gpu_device)
    dloss = torch.tensor([0.7], device=gpu_device)
    outs = []
    for _ in range(2):
        logit, loss, do = _nan([n], gpu_device), _nan([1], gpu_device), _nan([n, M], gpu_device)
        assert lib.ide3d_adv_head(_p(od), _p(cd), _p(logit), _p(loss), n, M, sign, hp._stream(od)) == 0, lib.ide3d_last_error()
        assert lib.ide3d_adv_head_backward(_p(od), _p(cd), _p(logit), _p(dloss), _p(do), n, M, sign, hp._stream(od)) == 0, lib.ide3d_last_error()
        outs.append((logit.cpu(), loss.cpu(), do.cpu()))
    (logit, loss, do), again = outs
    assert all(torch.equal(a, b) for a, b in zip(outs[0], again)), 'two runs are bit-equal'
    assert all(bool(torch.isfinite(t).all()) for t in outs[0])
    z64, l64 = R.head64(o.double(), None if cmap is None else cmap.double(), sign)
    do64 = R.head64_backward(o.double(), None if cmap is None else cmap.double(), logit.double(), float(dloss.cpu()), sign)
    if n > 1:
        assert abs(float(z64[0]) - 30) < 1e-3 and abs(float(z64[1]) + 30) < 1e-3
    e_logit = float(((logit.double() - z64).abs() / z64.abs()).max())
    e_loss = abs(float(loss) - float(l64)) / float(l64)
    e_do = float(((do.double() - do64).abs() / do64.abs()).max())
    print(f'n {n} M {M} sign {sign}: rel err logits {e_logit:.2e} loss {e_loss:.2e} do {e_do:.2e}; loss {float(loss):.6f}')
    assert e_logit <= ULP and e_loss <= ULP and e_do <= ULP
    assert float(do.abs().min()) > 0, 'the gradient of a saturated logit keeps its value'


# ---- end to end --------------------------------------------------------------------------------------------------------------------------------
@contextlib.contextmanager
def _switches(fused, arith=0):
    from training import adv_loss
    old = adv_loss.fused, adv_loss.arith
    adv_loss.fused, adv_loss.arith = fused, arith
    try:
        yield
    finally:
        adv_loss.fused, adv_loss.arith = old


@contextlib.contextmanager
def _deterministic_aten():
    old = torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark
    torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark = True, False
    try:
        yield
    finally:
        torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark = old


_cache = {}


def _case(name, gpu_device):
    """(ADVLoss on the device, img, c, {sign: (float64 loss, gradient, logits)}, clamp share) of a case, computed once and left unchanged."""
    if name not in _cache:
        from training import adv_loss, discriminator
        D = R.build(name, discriminator.Discriminator)
        img, c = R.case_inputs(name)
        taps = []
        ref = {-1: R.loss64(D.state_dict(), R.CASES[name]['kwargs'], img, c, -1, taps), 1: R.loss64(D.state_dict(), R.CASES[name]['kwargs'], img, c, 1)}
        _cache[name] = (adv_loss.ADVLoss(D.to(gpu_device)), img, c, ref, R.clamp_share(taps))
    return _cache[name]


def _calls_of(fn):
    from torch_utils import hip_plugin
    before = dict(hip_plugin.CALLS)
    fn()
    return {k: v - before.get(k, 0) for k, v in hip_plugin.CALLS.items() if v != before.get(k, 0)}


def _generator(crit, img, c=None, cmap=None):
    leaf = img.clone().requires_grad_(True)
    loss = crit.generator_loss(leaf, c, cmap)
    (g,) = torch.autograd.grad(loss, [leaf])
    return float(loss.detach()), g.cpu().double()


def _discriminator(crit, img, cmap):
    """discriminator_loss with the case's images as the real and as the fake batch (so both halves run the pre-activations whose kink
    margins test_adv_loss_cpu.py asserts) -> (loss, gradient of the real half, gradient of the fake half)."""
    real, fake = img.clone().requires_grad_(True), img.clone().requires_grad_(True)
    loss = crit.discriminator_loss(real, fake, cmap_real=cmap, cmap_fake=cmap)
    gr, gf = torch.autograd.grad(loss, [real, fake])
    return float(loss.detach()), gr.cpu().double(), gf.cpu().double()


def fused_calls(B, evaluations=1, mapped=0):
    """One `generator_loss(...).backward()` on the HIP path, by entry point, for a discriminator of B blocks.
    `mapped`: the leaky-ReLU layers of the label's mapping when the call maps `c` itself (`cmap=` not given): the mapping network is not
    part of the walker, its layers launch ide3d_bias_act as in every inference call."""
    calls = {
        'modconv2d': 2 * (3 * B + 2),                   # fromrgb, 3 per block, the epilogue's; as many on derived weights
        'upfirdn2d': 4 * B,                             # skip and conv1 of each block, and their adjoints
        'residual_join': 2 * B,                         # a block's output; its input gradient
        'minibatch_std': 1, 'linear': 2, 'bias_act': 1, 'adv_head': 1,
        'adv_head_backward': 1, 'linear_backward_input': 2,
        'modconv_act_backward': 3 * B + 3,              # fc, the epilogue's convolution, 3 per block (skip: its gain), fromrgb
        'minibatch_std_backward': 1,
    }
    calls['bias_act'] += mapped
    return {k: v * evaluations for k, v in calls.items()}


@pytest.mark.parametrize('arith', [0, 1], ids=['default', 'fp32'])
@pytest.mark.parametrize('name', ['fixture', 'uncond', 'clamped'])
def test_end_to_end_against_float64(gpu_device, name, arith):
    """Value: relative error; image gradient: relative L2, for generator_loss and for both halves of discriminator_loss.  Bound: the HIP
    gradient's error is at most 4 x that of the module's own `fused = False` path on the same GPU and inputs; the value's at most
    max(4 x that path's, 4 * 2^-24).  Measured on an MI355X (HIP / fused = False): gradient 2.6e-7 .. 6.3e-7 / 2.1e-7 .. 6.3e-7, value
    1.3e-9 .. 1.5e-7 / 1.3e-9 .. 6.9e-8 over the cases, the same in both arithmetics."""
    crit, img, c, ref, share = _case(name, gpu_device)
    if name == 'clamped':
        assert share >= 0.01, 'the clamp mask is exercised'
    imgd, cd = img.to(gpu_device), None if c is None else c.to(gpu_device)
    B = len(crit.D.block_resolutions)
    cm = crit.cmap(cd)           # the label is mapped once (fp32, by the mapping network's own path) for both paths
    with _switches(False), _deterministic_aten():
        tg, td = _generator(crit, imgd, cmap=cm), _discriminator(crit, imgd, cm)
        assert crit.last_path == 'torch'
    run = {}
    with _switches(True, arith):
        calls_g = _calls_of(lambda: run.__setitem__('g', _generator(crit, imgd, cmap=cm)))
        assert crit.last_path == 'hip'
        calls_d = _calls_of(lambda: run.__setitem__('d', _discriminator(crit, imgd, cm)))
    assert calls_g == fused_calls(B) and calls_d == fused_calls(B, evaluations=2), 'the HIP path did not run'
    hg, hd = run['g'], run['d']
    (lg, gg, _), (lf, gf, _) = ref[-1], ref[1]
    floor = 4 * 2.0 ** -24
    rows = [('generator_loss value', abs(hg[0] - lg) / lg, abs(tg[0] - lg) / lg, floor),
            ('generator_loss gradient', R.rel_l2(hg[1], gg), R.rel_l2(tg[1], gg), 0.0),
            ('discriminator_loss value', abs(hd[0] - lg - lf) / (lg + lf), abs(td[0] - lg - lf) / (lg + lf), floor),
            ('discriminator_loss gradient, real half', R.rel_l2(hd[1], gg), R.rel_l2(td[1], gg), 0.0),
            ('discriminator_loss gradient, fake half', R.rel_l2(hd[2], gf), R.rel_l2(td[2], gf), 0.0)]
    for what, hip, aten, fl in rows:
        print(f'{name} arith {arith}: {what}: HIP {hip:.2e}, fused = False {aten:.2e}')
    for what, hip, aten, fl in rows:
        assert hip <= max(4 * aten, fl), what


def test_routing_launch_counts_and_reproducibility(gpu_device):
    """The exact launch table of one generator_loss forward + backward, bit-equal repeats, and what takes the PyTorch definition.  That
    definition is built from the package's differentiable ops, which launch ide3d_bias_act and ide3d_upfirdn2d on CUDA tensors as they
    do for every other network of the package: 'no HIP calls' is asserted as no call of any entry point of the fused walker."""
    from torch_utils import hip_plugin
    from training import adv_loss, discriminator
    crit, img, c, ref, _ = _case('fixture', gpu_device)
    imgd, cd = img.to(gpu_device), c.to(gpu_device)
    walker = set(fused_calls(1)) - {'bias_act', 'upfirdn2d'}

    def plain(calls):
        return not (set(calls) & walker)
    with _switches(True):
        leaf = imgd.clone().requires_grad_(True)
        assert _calls_of(lambda: crit.generator_loss(leaf, cd).backward()) == fused_calls(2, mapped=8)
        cm = crit.cmap(cd)
        assert _calls_of(lambda: crit(imgd, cmap=cm)) == {k: v for k, v in fused_calls(2).items() if k in
                                                          ('minibatch_std', 'linear', 'bias_act', 'adv_head')} | {'modconv2d': 8, 'upfirdn2d': 4, 'residual_join': 2}
        runs = [_generator(crit, imgd, cd) for _ in range(2)]
        assert runs[0][0] == runs[1][0] and torch.equal(runs[0][1], runs[1][1]) and torch.equal(leaf.grad.cpu().double(), runs[0][1])
        # logits: the fused forward without a gradient; the PyTorch definition for an image that requires one
        z = crit.logits(imgd, cd)
        assert crit.last_path == 'hip' and tuple(z.shape) == (4, 1)
        assert float((z[:, 0].cpu().double() - ref[-1][2]).abs().max()) <= 1e-5
        assert crit.logits(leaf, cd).requires_grad and crit.last_path == 'torch'
        # the layer's own inference path
        with torch.no_grad():
            calls = _calls_of(lambda: crit.D(imgd, cd))
        assert calls.get('minibatch_std') == 1 and 'adv_head' not in calls
        # what takes the PyTorch definition
        def torch_path(cr, x, cc=cd, **kw):
            lf = x.clone().requires_grad_(True) if not x.requires_grad else x
            calls = _calls_of(lambda: cr.generator_loss(lf, cc, **kw).backward())
            assert cr.last_path == 'torch' and plain(calls), calls
        torch_path(crit, imgd.half())
        wide = torch.zeros(4, 6, 16, 20, device=gpu_device)
        wide[..., :16] = imgd
        view = wide.requires_grad_(True)[..., :16]
        assert not view.is_contiguous() and view.requires_grad
        torch_path(crit, view)
        p = crit.D.b8.conv1.weight
        p.requires_grad_(True)
        try:
            torch_path(crit, imgd)
        finally:
            p.requires_grad_(False)
            p.grad = None
        torch_path(crit, imgd, cd.clone().requires_grad_(True))
        D9 = discriminator.Discriminator(**dict(R.CASES['fixture']['kwargs'], epilogue_kwargs=dict(mbstd_group_size=3))).eval().requires_grad_(False).to(gpu_device)
        torch_path(adv_loss.ADVLoss(D9), torch.randn(9, 6, 16, 16, device=gpu_device), torch.randn(9, 25, device=gpu_device))
        with pytest.raises(ValueError):
            crit.generator_loss(imgd[:3], cd[:3])
    with _switches(False):
        calls = _calls_of(lambda: _generator(crit, imgd, cd))
        assert crit.last_path == 'torch' and plain(calls), calls
    assert hip_plugin.exclusive_violations()[0] == 0


PROJECT_KWARGS = dict(c_dim=25, img_resolution=64, img_channels=3, channel_base=512, channel_max=16, conv_clamp=256)


def test_project_with_adv_distance_on_gpu(gpu_device):
    """Five projector steps of the tiny generator with the adversarial term on the HIP path against the same steps with `fused = False`
    (the ATen path of the same module is the yardstick): the new entry points are counted five times, the losses are finite and within
    1e-4 relative of the other path's.  The projector's loss adds its noise regulariser (about 1e4 for this generator) to the distance; the
    weight 1e4 keeps the adversarial term (about 0.7 unweighted) of that size, so that the comparison is about it."""
    from training import adv_loss, discriminator, projection, triplane
    torch.manual_seed(4)
    D = discriminator.Discriminator(**PROJECT_KWARGS).eval().requires_grad_(False).to(gpu_device)
    crit = adv_loss.ADVLoss(D)

    def run(fused):
        torch.manual_seed(0)
        G = triplane.TriPlaneGenerator(triplane.tiny_spec()).eval().to(gpu_device)
        c = triplane.camera_label(0.2)
        target = torch.rand(3, G.img_resolution, G.img_resolution, generator=torch.Generator().manual_seed(1)) * 255
        with _switches(fused), _deterministic_aten():
            p = projection.Projector(G, target, c, num_steps=5, w_avg_samples=32, distance=adv_loss.adv_distance(c.to(gpu_device), crit, weight=1e4))
            start = p.pivot().clone()
            losses = []
            calls = _calls_of(lambda: losses.extend(float(p.step(i)) for i in range(5)))
        assert bool(torch.isfinite(p.pivot()).all()) and not torch.equal(p.pivot(), start)
        return losses, calls
    hip, calls = run(True)
    aten, calls_aten = run(False)
    for k in ('adv_head', 'adv_head_backward', 'minibatch_std', 'minibatch_std_backward'):
        assert calls.get(k) == 5 and k not in calls_aten, (k, calls)
    print(f'projector losses: HIP {hip}, fused = False {aten}')
    assert all(math.isfinite(v) for v in hip + aten)
    for a, b in zip(hip, aten):
        assert abs(a - b) <= 1e-4 * abs(b), (a, b)
