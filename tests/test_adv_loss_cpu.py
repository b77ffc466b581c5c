"""The StyleGAN2 discriminator and its adversarial loss without a GPU (training/discriminator.py, training/adv_loss.py; DESIGN.md section
5.38): parity with the reference-run fixture through the float64 restatement of tests/adv_loss_ref.py, the restatement of the minibatch
standard deviation and its analytic adjoint against float64 autograd, the routing rules, and the kink margins of the end-to-end cases."""

import pytest
import torch
import torch.nn.functional as F

import adv_loss_ref as R
from training import adv_loss, discriminator, networks


def _calls_of(fn):
    from torch_utils import hip_plugin
    before = dict(hip_plugin.CALLS)
    fn()
    return {k: v - before.get(k, 0) for k, v in hip_plugin.CALLS.items() if v != before.get(k, 0)}


def _loss_and_grad(crit, img, c, sign=-1):
    leaf = img.clone().requires_grad_(True)
    loss = crit._loss(leaf, c, None, sign)
    (g,) = torch.autograd.grad(loss, [leaf])
    return float(loss.detach()), g


def test_parity_with_the_reference_run_fixture():
    """The package's class loads the reference discriminator's state dict with strict=True (same keys, same order) and reproduces its
    logits and the image gradient of softplus(-logits).mean().  Tolerance: the package's fp32 CPU error against the float64 restatement
    is at most 4 x the fixture's own fp32 error against it, floor 4 * 2^-24 relative (one fp32 rounding is 2^-24; 4: the factor the other
    loss tests give a second fp32 path).  The fixture's error below 1e-4 ties the restatement to the reference: a wrong definition errs
    by percent.  Measured: fixture and package both 5.8e-7 (logits) and 5.5e-7 (gradient, relative L2) - the two fp32 CPU runs are the
    same ATen calls."""
    d, sd = R.fixture()
    kw = R.CASES['fixture']['kwargs']
    D = discriminator.Discriminator(**kw)
    D.load_state_dict(sd, strict=True)
    assert list(D.state_dict().keys()) == [str(k) for k in d['keys']]
    assert sum(p.numel() for p in D.parameters()) == 16272 and tuple(D.b4.conv.weight.shape) == (16, 17, 3, 3)
    assert networks.Discriminator is discriminator.Discriminator and networks.MinibatchStdLayer is discriminator.MinibatchStdLayer
    assert networks.DiscriminatorBlock is discriminator.DiscriminatorBlock and networks.DiscriminatorEpilogue is discriminator.DiscriminatorEpilogue
    D.eval().requires_grad_(False)
    img, c = torch.from_numpy(d['img']), torch.from_numpy(d['c'])
    assert torch.equal(img, R.case_inputs('fixture')[0]) and torch.equal(c, R.case_inputs('fixture')[1])
    l64, g64, z64 = R.loss64(sd, kw, img, c)
    crit = adv_loss.ADVLoss(D)
    loss, grad = _loss_and_grad(crit, img, c)
    with torch.no_grad():
        logits = crit.logits(img, c)
    assert crit.last_path == 'torch' and tuple(logits.shape) == (4, 1)
    fix = dict(logits=R.rel_l2(torch.from_numpy(d['logits'])[:, 0], z64), grad=R.rel_l2(torch.from_numpy(d['grad']), g64), loss=abs(float(d['loss']) - l64) / l64)
    got = dict(logits=R.rel_l2(logits[:, 0], z64), grad=R.rel_l2(grad, g64), loss=abs(loss - l64) / l64)
    print(f'against float64: fixture {fix}, package {got}')
    floor = 4 * 2.0 ** -24
    for key in ('logits', 'grad', 'loss'):
        assert fix[key] < 1e-4, key
        assert got[key] <= max(4 * fix[key], floor), key


MBSTD_CASES = [  # n, c, h, w, group_size, F
    (4, 6, 4, 4, 2, 1),           # interleaved groups: {0, 2} and {1, 3}
    (4, 6, 3, 2, 4, 1),           # G = N
    (6, 4, 2, 2, None, 1),        # the whole batch
    (4, 6, 4, 4, 2, 2),           # F = 2 with c / F = 3
    (3, 4, 2, 2, 1, 1),           # G = 1
    (2, 4, 2, 2, 4, 2),           # a group size larger than the batch: min(group_size, n)
]


@pytest.mark.parametrize('n,c,h,w,group,features', MBSTD_CASES)
def test_mbstd_restatement_and_its_analytic_backward(n, c, h, w, group, features):
    """The float64 restatement and its analytic adjoint against float64 autograd through the layer's own PyTorch definition."""
    g = torch.Generator().manual_seed(n * 100 + c)
    x = torch.randn(n, c, h, w, generator=g, dtype=torch.float64)
    dy = torch.randn(n, c + features, h, w, generator=g, dtype=torch.float64)
    leaf = x.clone().requires_grad_(True)
    y = discriminator.MinibatchStdLayer(group, features)(leaf)
    (gx,) = torch.autograd.grad(y, [leaf], dy)
    y64 = R.mbstd64(x, group, features)
    dx64, term = R.mbstd64_backward(x, dy, group, features)
    assert tuple(y.shape) == (n, c + features, h, w) and torch.equal(y64[:, :c], x)
    assert float((y64 - y.detach()).abs().max()) <= 1e-14 * float(y.detach().abs().max())
    assert float((dx64 - gx).abs().max()) <= 1e-13 * float(gx.abs().max())
    G = n if group is None else min(group, n)
    if G == 1:
        assert float(term.abs().max()) == 0.0 and torch.equal(dx64, dy[:, :c])
    if 1 < G < n:
        wrong = R.mbstd64(x, group, features, grouping=lambda n_, G_, j: [j * G_ + g_ for g_ in range(G_)])
        assert float((wrong - y.detach()).abs().max()) > 1e-3, 'a j * G + g grouping has to fail'


def test_head_restatement_against_autograd():
    g = torch.Generator().manual_seed(7)
    o, cmap = torch.randn(5, 16, generator=g, dtype=torch.float64) * 8, torch.randn(5, 16, generator=g, dtype=torch.float64) * 4
    for sign in (-1, 1):
        for cm in (cmap, None):
            leaf = (o if cm is not None else o[:, :1]).clone().requires_grad_(True)
            z = (leaf * cm).sum(1, keepdim=True) / 4 if cm is not None else leaf
            loss = F.softplus(sign * z).mean()
            (do,) = torch.autograd.grad(loss, [leaf])
            logit, l64 = R.head64(leaf.detach(), cm, sign)
            assert abs(float(l64) - float(loss.detach())) <= 1e-14 * float(loss.detach())
            assert float((R.head64_backward(leaf.detach(), cm, logit, 1.0, sign) - do).abs().max()) <= 1e-14 * float(do.abs().max())
    big = torch.tensor([[30.0], [-30.0], [800.0], [-800.0]], dtype=torch.float64)
    assert torch.isfinite(R.softplus64(big)).all() and float(R.softplus64(big)[1]) > 0 and float(R.softplus64(big)[2]) == 800.0


def test_routing_without_a_gpu(monkeypatch):
    """CPU tensors, a trainable D and the other architectures take the PyTorch definition and launch nothing; a batch that is no multiple
    of the minibatch-std group raises ValueError."""
    monkeypatch.setattr(adv_loss, 'fused', True)
    D = R.build('fixture', discriminator.Discriminator)
    img, c = R.case_inputs('fixture')
    crit = adv_loss.ADVLoss(D)
    assert crit.last_path is None
    out = []
    assert _calls_of(lambda: out.append(_loss_and_grad(crit, img, c))) == {} and crit.last_path == 'torch'
    l64, g64, _ = R.loss64(D.state_dict(), R.CASES['fixture']['kwargs'], img, c)
    assert abs(out[0][0] - l64) <= 1e-5 * l64 and R.rel_l2(out[0][1], g64) <= 1e-5
    # forward is generator_loss; discriminator_loss is d_logistic_loss of the two logits; the helpers are the app's formulas
    with torch.no_grad():
        z = crit.logits(img, c)
        assert torch.equal(crit(img, c), crit.generator_loss(img, c)) and torch.equal(crit.generator_loss(img, cmap=crit.cmap(c)), crit(img, c))
        fake = img.flip(0)
        dl = crit.discriminator_loss(img, fake, c, c)
        assert float((dl - adv_loss.d_logistic_loss(z, crit.logits(fake, c))).abs()) <= 1e-6
        assert float((crit(img, c) - adv_loss.g_nonsaturating_loss(z)).abs()) <= 1e-6
    D.b16.conv0.weight.requires_grad_(True)
    assert _calls_of(lambda: crit.generator_loss(img, c).backward()) == {} and crit.last_path == 'torch'
    assert D.b16.conv0.weight.grad is not None and bool(torch.isfinite(D.b16.conv0.weight.grad).all())
    for arch in ('orig', 'skip'):
        Da = discriminator.Discriminator(**dict(R.CASES['fixture']['kwargs'], architecture=arch)).eval().requires_grad_(False)
        ca = adv_loss.ADVLoss(Da)
        assert _calls_of(lambda: _loss_and_grad(ca, img, c)) == {} and ca.last_path == 'torch'
        assert ('fromrgb' in dict(Da.b8.named_children())) == (arch == 'skip') and not hasattr(Da.b16, 'skip')
    with pytest.raises(ValueError):
        crit.generator_loss(img[:3], c[:3])
    with pytest.raises(ValueError):
        discriminator.MinibatchStdLayer(2)(torch.zeros(3, 4, 2, 2))
    with pytest.raises(ValueError):
        discriminator.MinibatchStdLayer(1, 3)(torch.zeros(2, 4, 2, 2))


def test_r1_freeze_layers_and_forced_fp32():
    """R1's `create_graph=True` works through `Discriminator.forward`; `freeze_layers` registers the first layers as buffers; the loss
    evaluates a discriminator with fp16 blocks in fp32."""
    kw = R.CASES['fixture']['kwargs']
    torch.manual_seed(3)
    D = discriminator.Discriminator(**kw)
    img, c = R.case_inputs('fixture')
    leaf = img.clone().requires_grad_(True)
    r1 = adv_loss.d_r1_loss(adv_loss.ADVLoss(D).logits(leaf, c), leaf)
    r1.backward()
    assert float(r1.detach()) > 0 and all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for n, p in D.named_parameters() if n.endswith('.weight') and n.startswith('b'))
    assert float(D.b16.conv0.weight.grad.abs().max()) > 0
    # the same penalty from the float64 restatement: the gradient of the logits' sum
    sd = D.state_dict()
    leaf64 = img.double().requires_grad_(True)
    z64 = R.logits64({k: v.detach() for k, v in sd.items()}, kw, leaf64, R.cmap64(sd, c))
    (g64,) = torch.autograd.grad(z64.sum(), [leaf64])
    want = float(g64.square().reshape(4, -1).sum(1).mean())
    assert abs(float(r1.detach()) - want) <= 1e-4 * want
    Df = discriminator.Discriminator(**kw, block_kwargs=dict(freeze_layers=2))
    assert [n for n, _ in Df.named_parameters() if n.startswith('b16')] == ['b16.conv1.weight', 'b16.conv1.bias', 'b16.skip.weight']
    assert list(Df.state_dict().keys()) == list(D.state_dict().keys()) or set(Df.state_dict().keys()) == set(D.state_dict().keys())
    Dh = discriminator.Discriminator(**kw, num_fp16_res=4)
    Dh.load_state_dict(sd)
    assert Dh.b16.use_fp16 and Dh.b8.use_fp16 and not D.b16.use_fp16
    with torch.no_grad():
        assert torch.equal(adv_loss.ADVLoss(Dh).logits(img, c), adv_loss.ADVLoss(D).logits(img, c))


def test_kink_margin_of_the_end_to_end_cases():
    """In float64 every leaky-ReLU pre-activation of the end-to-end cases, and every distance of an output from an active clamp, is at least
    1e-5 of the layer's RMS pre-activation: fp32 rounding (1e-7) cannot put an element on the other side of a kink, so the gradient
    comparisons of tests/test_gpu_adv_loss.py compare the same piecewise-linear function.  A condition that picks the seeds of
    adv_loss_ref.CASES, not a measurement; the 'clamped' case has at least 1 % of its clamped activations on the clamp."""
    for name, case in R.CASES.items():
        D = R.build(name, discriminator.Discriminator)
        img, c = R.case_inputs(name)
        taps = []
        R.loss64(D.state_dict(), case['kwargs'], img, c, taps=taps)
        count = sum(t['u'].numel() for t in taps if t['act'] == 'lrelu')
        margin, share = R.kink_margin(taps), R.clamp_share(taps)
        print(f'{name}: {count} leaky-ReLU activations, kink margin {margin:.2e}, on the clamp {share:.3f}')
        assert margin >= 1e-5, name
        assert (share >= 0.01) if name == 'clamped' else (share == 0.0), name
