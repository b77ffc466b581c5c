"""The shared walkers of the three tapped feature-net losses (training/feature_loss.py under training/lpips.py, training/lpips_alex.py and
training/vgg_loss.py) without a GPU: each loss's fused pass - the orchestration the HIP path runs - on a float64 torch restatement of every
launch (tests/feature_loss_ref.py `TorchOps`) against float64 autograd through the module's own torch definition, and the ordered launch
sequence of each pass against the lists in the module docstrings and the launch counts the GPU tests pin."""

import collections
import copy

import pytest
import torch

import feature_loss_ref as R

NARROW = (4, 4, 8, 8, 8)
BOUND = 1e-10          # see test_lpips_walkers_against_autograd
DLOSS = 0.75           # the upstream gradient handed to the backward pass


def _images(shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return [((torch.rand(*shape, generator=g) * 2 - 1) * scale).double() for _ in range(2)]


def _lpips(kind, seed):
    from training import lpips, lpips_alex
    torch.manual_seed(seed)
    return lpips.LPIPS('vgg', widths=NARROW) if kind == 'vgg' else lpips_alex.LPIPS(widths=NARROW)


def _rel(got, want):
    return float((got - want).norm() / want.norm())


def _check(loss, grad, want_loss, want_grad):
    err_l, err_g = abs(float(loss) - float(want_loss)) / abs(float(want_loss)), _rel(grad, DLOSS * want_grad)
    print(f'value {float(want_loss):.6e}: relative error {err_l:.2e}; gradient: relative L2 {err_g:.2e} (bound {BOUND:.0e})')
    assert float(want_grad.abs().max()) > 0
    assert err_l <= BOUND and err_g <= BOUND


def _lpips_case(m, x, y, f, in_scale, in_shift, ops):
    """-> (loss, grad) of the fused pass on `ops`, (loss, grad) of float64 autograd through the torch definition of a `.double()` copy."""
    from training import lpips
    m64 = copy.deepcopy(m).double()
    leaf = x.clone().requires_grad_(True)
    want = m64._distance(leaf, m64._features(y, f, in_scale, in_shift), f, in_scale, in_shift)
    (want_grad,) = torch.autograd.grad(want, [leaf])
    with torch.no_grad():
        feats, lins = lpips._fused_features(ops, m, y, f, in_scale, in_shift), m._lin_vectors()
        loss, saved = lpips._fused_forward(ops, m, x, feats, lins, f, in_scale, in_shift)
        grad = lpips._fused_backward(ops, m, saved, feats, lins, f, in_scale, torch.full([1], DLOSS, dtype=torch.float64))
    return (loss, grad), (want.detach(), want_grad)


# the smallest shapes at which a walker can still go wrong: the last pool leaves 1 x 1; odd sides after the second and third pool (VGG);
# the minimum side; a ragged last stem window and odd pool inputs (AlexNet)
@pytest.mark.parametrize('kind,shape', [('vgg', (1, 3, 16, 16)), ('vgg', (2, 3, 18, 22)), ('alex', (1, 3, 31, 31)), ('alex', (2, 3, 35, 43))])
def test_lpips_walkers_against_autograd(kind, shape):
    """Bound 1e-10 on the relative error of the value and the relative L2 of the gradient: both sides are float64 evaluations of the same
    fp32 parameters that differ only in summation order, and 13 layers of fan-in at most 72 stay orders below it (measured here: 2e-15 or
    less); a wrong tap index, a dropped pool route or a misplaced fold is 1e-2 or more.  Inputs are seeded rand * 2 - 1: the only ties are
    at ReLU zeros, which both sides mask."""
    m = _lpips(kind, 1)
    x, y = _images(shape, 2)
    got, want = _lpips_case(m, x, y, 1, 1.0, 0.0, R.TorchOps(torch.float64))
    _check(*got, *want)


def test_lpips_area_factor_through_features_and_distance():
    """`_features` / `_distance` with area factor 2 and the 0..255 rescaling of `lpips_distance`: the prep pass and its adjoint."""
    m = _lpips('vgg', 3)
    x, y = (127.5 * (t + 1) for t in _images((1, 3, 32, 32), 4))
    got, want = _lpips_case(m, x, y, 2, 2.0 / 255.0, -1.0, R.TorchOps(torch.float64))
    _check(*got, *want)


def _vgg_case(m, x, y, ops):
    from training import vgg_loss
    m64 = copy.deepcopy(m).double()
    leaf = x.clone().requires_grad_(True)
    want = m64.distance_to(leaf, m64.features(y))
    (want_grad,) = torch.autograd.grad(want, [leaf])
    with torch.no_grad():
        acts, tap_at = vgg_loss._fused_taps(ops, m, y)[:2]
        feats = [acts[i] for i in tap_at]
        loss, saved = vgg_loss._fused_forward(ops, m, x, feats)
        grad = vgg_loss._fused_backward(ops, m, saved, feats, torch.full([1], DLOSS, dtype=torch.float64))
    return (loss, grad), (want.detach(), want_grad)


@pytest.mark.parametrize('n_layers,shape', [(5, (1, 3, 16, 16)), (5, (2, 3, 18, 22)), (2, (2, 3, 18, 22)), (2, (1, 3, 16, 16))])
def test_vgg19_walkers_against_autograd(n_layers, shape):
    """The tap / pool / interior dispatch of the VGG19 backward, with all five slices and with the first two (the chain then ends at a tap
    whose convolution has a pool in front).  Bound: as test_lpips_walkers_against_autograd."""
    from training import vgg_loss
    torch.manual_seed(5)
    m = vgg_loss.VGGLoss(n_layers=n_layers, widths=NARROW)
    x, y = _images(shape, 6)
    got, want = _vgg_case(m, x, y, R.TorchOps(torch.float64))
    _check(*got, *want)


# ---- the launch sequences of the module docstrings ------------------------------------------------------------------------------------------
def _chain(stages, pool='maxpool2'):
    out = []
    for s, count in enumerate(stages):
        out += ([pool] if s > 0 else []) + ['conv'] * count
    return out


VGG16_FORWARD = ['prep'] + _chain((2, 2, 3, 3, 3))
# per stage, last to first: stage_backward at its end, act_backward inside; a convolution on the derived weight behind each
VGG16_BACKWARD = sum((['stage_backward', 'conv'] + ['relu_backward', 'conv'] * (count - 1) for count in (3, 3, 3, 2, 2)), []) + ['prep_backward']
ALEX_FORWARD = ['prep', 'unfold2d', 'conv', 'maxpool3s2p0', 'unfold2d', 'conv', 'maxpool3s2p0', 'conv', 'conv', 'conv']
ALEX_BACKWARD = ['tap_backward', 'conv'] * 3 + ['tap_backward', 'conv', 'fold2d'] * 2 + ['prep_backward']
VGG19_FORWARD = ['prep'] + _chain((2, 2, 4, 4, 1))
VGG19_BACKWARD = (['feat_l1_tap_backward', 'conv']                                                                    # tap 5
                  + (['maxpool2_relu_backward', 'conv'] + ['relu_backward', 'conv'] * 2 + ['feat_l1_tap_backward', 'conv']) * 2     # stages 4, 3
                  + (['maxpool2_relu_backward', 'conv', 'feat_l1_tap_backward', 'conv']) * 2 + ['prep_backward'])                    # stages 2, 1


def _counts(log):
    return dict(collections.Counter(R.ENTRY[name] for name in log))


@pytest.mark.parametrize('kind,shape,forward,backward', [('vgg', (1, 3, 16, 16), VGG16_FORWARD, VGG16_BACKWARD),
                                                         ('alex', (1, 3, 31, 31), ALEX_FORWARD, ALEX_BACKWARD)])
def test_lpips_launch_sequences(kind, shape, forward, backward):
    """The ordered launches of `features` and of `distance_to` + backward equal the lists of the module docstrings, and their counts per
    entry point equal what the GPU tests pin (`FEATURES_CALLS`, `DISTANCE_CALLS`)."""
    import test_gpu_lpips
    import test_gpu_lpips_alex
    pinned = test_gpu_lpips if kind == 'vgg' else test_gpu_lpips_alex
    from training import lpips
    m = _lpips(kind, 1)
    x, y = _images(shape, 2)
    ops = R.RecordingOps(torch.float64)
    with torch.no_grad():
        feats = lpips._fused_features(ops, m, y, 1, 1.0, 0.0)
    assert ops.log == forward + ['normalize'] and _counts(ops.log) == pinned.FEATURES_CALLS
    ops.log.clear()
    with torch.no_grad():
        loss, saved = lpips._fused_forward(ops, m, x, feats, m._lin_vectors(), 1, 1.0, 0.0)
        lpips._fused_backward(ops, m, saved, feats, m._lin_vectors(), 1, 1.0, torch.ones([1], dtype=torch.float64))
    assert ops.log == forward + ['head', 'head_backward'] + backward and _counts(ops.log) == pinned.DISTANCE_CALLS


def test_vgg19_launch_sequences():
    import test_gpu_vgg_loss as pinned
    from training import vgg_loss
    torch.manual_seed(5)
    m = vgg_loss.VGGLoss(widths=NARROW)
    x, y = _images((1, 3, 16, 16), 6)
    ops = R.RecordingOps(torch.float64)
    with torch.no_grad():
        acts, tap_at = vgg_loss._fused_taps(ops, m, y)[:2]
    assert ops.log == VGG19_FORWARD and _counts(ops.log) == pinned.FEATURES_CALLS and tap_at == [0, 2, 4, 8, 12]
    ops.log.clear()
    feats = [acts[i] for i in tap_at]
    with torch.no_grad():
        loss, saved = vgg_loss._fused_forward(ops, m, x, feats)
        vgg_loss._fused_backward(ops, m, saved, feats, torch.ones([1], dtype=torch.float64))
    assert ops.log == VGG19_FORWARD + ['feat_l1'] + VGG19_BACKWARD and _counts(ops.log) == pinned.DISTANCE_CALLS
