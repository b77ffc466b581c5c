"""The hybrid encoder as a trainable network through HIP (training/networks.py `hip_plain_conv_grad`): mode 1 of
ide3d_modconv_weight_grad (csrc/modconv_bwd.hip), ide3d_linear_weight_grad (csrc/linear_wgrad.hip), ide3d_residual_join (csrc/res_join.hip),
and the autograd Functions that put them and the existing launches on `Conv2dLayer`, `EqualConv2d` and `EncoderResBlock`.  `pytest -m gpu`.

Reference: float64 PyTorch on the CPU, of the same module where there is one (`copy.deepcopy(m).double()`: the differentiable ATen path).
Errors are max|a - e| / max|e|; the bounds are the project's own for the same arithmetic: KERNEL_TOL for a launch alone, GRAD_TOL through
a layer or the network.  Losses are sum(y * P) with a fixed random P, zero where an lrelu pre-activation lies on its kink.
"""

import copy

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

KERNEL_TOL = 1e-5
GRAD_TOL = 1e-4
DEV = torch.device('cuda', 0)
CONV_OPS = ('aten::convolution', 'aten::_convolution', 'aten::miopen_', 'aten::cudnn_', 'aten::conv')
NEW_CALLS = ('modconv_weight_grad', 'head_weight_grad', 'modconv_act_backward', 'bias_noise_grad', 'linear_weight_grad', 'linear_backward_input',
             'residual_join')


@pytest.fixture
def switch_on():
    from training import networks
    old = getattr(networks, 'hip_plain_conv_grad', False)
    networks.hip_plain_conv_grad = True
    yield
    networks.hip_plain_conv_grad = old


def _calls(names=NEW_CALLS + ('modconv2d', 'upfirdn2d', 'linear')):
    from torch_utils import hip_plugin
    return {k: hip_plugin.CALLS.get(k, 0) for k in names}


def _delta(before, after):
    return {k: after[k] - before[k] for k in before}


def _err(actual, expected):
    a = actual.detach().cpu().double(); e = expected.detach().cpu().double()
    assert a.shape == e.shape, f'shape {tuple(a.shape)} != {tuple(e.shape)}'
    assert bool(torch.isfinite(a).all()), 'non-finite result'
    return float((a - e).abs().max()) / (float(e.abs().max()) + 1e-30)


def _double(mod):
    ref = copy.deepcopy(mod).cpu().double()
    for m in ref.modules():
        if getattr(m, 'resample_filter', None) is not None:
            m.resample_filter = m.resample_filter.float()
    return ref


def _profiled(fn):
    """(fn(), the names of the ATen operators it ran): the spy of test_gpu_param_grad.py."""
    with torch.profiler.profile(activities=[torch.profiler.ProfilerActivity.CPU]) as prof:
        out = fn()
    return out, {e.name for e in prof.events()}


def _conv_names(names):
    return sorted(n for n in names if n.startswith(CONV_OPS))


# ---- 1. the mode-1 weight gradient alone -------------------------------------------------------------------------------------------------
# (n, cin, cout, H, W): odd sizes with channels off the 64-tile; several pixel splits; the 4^2 end of the tower; a narrow operand; even sizes
# whose last input row and column no window reads (NaN there in the input)
WGRAD_SHAPES = [(2, 24, 40, 9, 7), (1, 32, 64, 65, 65), (3, 512, 512, 9, 9), (1, 3, 32, 33, 33), (1, 8, 8, 10, 8)]


def _wgrad_case(n, cin, cout, H, W, modulated):
    g = torch.Generator().manual_seed(H * 1000 + cin)
    gh, gw = (H - 3) // 2 + 1, (W - 3) // 2 + 1
    x = torch.randn(n, cin, H, W, generator=g)
    dz = torch.randn(n, cout, gh, gw, generator=g)
    s = (torch.randn(n, cin, generator=g) + 1.5) if modulated else None
    d = (torch.rand(n, cout, generator=g) + 0.5) if modulated else None
    xs = x.double() * (s.double()[:, :, None, None] if modulated else 1.0)
    up = dz.double() * (d.double()[:, :, None, None] if modulated else 1.0)
    w = torch.zeros(cout, cin, 3, 3, dtype=torch.float64, requires_grad=True)
    want, = torch.autograd.grad(F.conv2d(xs, w, stride=2), w, up)
    # what no window reads is poisoned after the reference has been formed
    if H % 2 == 0:
        x[:, :, H - 1, :] = float('nan')
    if W % 2 == 0:
        x[:, :, :, W - 1] = float('nan')
    return x, dz, s, d, want


@pytest.mark.parametrize('arith', [6, 1], ids=['bf16x6', 'fp32'])
@pytest.mark.parametrize('modulated', [False, True], ids=['plain', 'styles_dcoefs'])
@pytest.mark.parametrize('shape', WGRAD_SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_mode_1_weight_gradient_against_float64(shape, modulated, arith):
    from torch_utils import hip_plugin
    P = hip_plugin.ModconvGradPlugin
    x, dz, s, d, want = _wgrad_case(*shape, modulated)
    args = (dz.to(DEV), x.to(DEV), None if s is None else s.to(DEV), None if d is None else d.to(DEV))
    before = _calls(('modconv_weight_grad',))
    got = P.weight_grad(*args, mode=1, arith=arith)
    assert _delta(before, _calls(('modconv_weight_grad',))) == {'modconv_weight_grad': 1}
    again = P.weight_grad(*args, mode=1, arith=arith)
    assert torch.equal(got, again), 'not bit-reproducible'
    err = _err(got, want)
    print(f'mode-1 weight gradient {shape} arith {arith}: err {err:.2e}')
    assert err < KERNEL_TOL


# ---- 2. the projector's weight gradient alone ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n,K,M', [(1, 8, 5), (3, 8192, 512), (8, 2052, 17)])
def test_linear_weight_gradient_against_float64(n, K, M):
    from torch_utils import hip_plugin
    P = hip_plugin.IdLossPlugin
    g = torch.Generator().manual_seed(K + M)
    dy, x = torch.randn(n, M, generator=g), torch.randn(n, K, generator=g)
    before = _calls(('linear_weight_grad',))
    got = P.linear_weight_grad(dy.to(DEV), x.to(DEV))
    assert _delta(before, _calls(('linear_weight_grad',))) == {'linear_weight_grad': 1}
    assert torch.equal(got, P.linear_weight_grad(dy.to(DEV), x.to(DEV))), 'not bit-reproducible'
    err = _err(got, dy.double().t() @ x.double())
    print(f'linear weight gradient n {n} K {K} M {M}: err {err:.2e}')
    assert err < KERNEL_TOL


@pytest.mark.parametrize('n,K', [(9, 8), (1, 6)])
def test_linear_weight_gradient_refuses_what_it_does_not_cover(n, K):
    from torch_utils import hip_plugin
    before = _calls(('linear_weight_grad',))
    with pytest.raises(RuntimeError, match='linear_weight_grad'):
        hip_plugin.IdLossPlugin.linear_weight_grad(torch.randn(n, 5, device=DEV), torch.randn(n, K, device=DEV))
    assert _delta(before, _calls(('linear_weight_grad',))) == {'linear_weight_grad': 0}


# ---- 3. every Conv2dLayer form -------------------------------------------------------------------------------------------------------------
FORMS = [(1, 1, 'lrelu', True), (3, 1, 'lrelu', True), (3, 2, 'lrelu', True), (1, 2, 'linear', False)]
LAYER_SHAPES = [(2, 3, 32, 16), (1, 19, 32, 34), (2, 40, 72, 10), (1, 512, 512, 8)]


def _conv_layer(k, down, act, bias, cin, cout):
    from training import networks
    torch.manual_seed(cin * 7 + cout + k)
    lay = networks.Conv2dLayer(cin, cout, k, bias=bias, activation=act, down=down)
    if bias:
        with torch.no_grad():
            lay.bias.normal_(0, 0.5)
    return lay


def _off_kinks(ref, y, P):
    """P with zeros where the float64 pre-activation lies within 1e-5 of its max-abs of the lrelu kink."""
    if ref.activation != 'lrelu':
        return P
    u = y / ref.act_gain
    u = torch.where(u > 0, u, u / 0.2)
    return torch.where(u.abs() < 1e-5 * float(u.abs().max()), torch.zeros_like(P), P)


@pytest.mark.parametrize('shape', LAYER_SHAPES, ids=lambda s: 'x'.join(map(str, s)))
@pytest.mark.parametrize('form', FORMS, ids=lambda f: f'k{f[0]}_down{f[1]}_{f[2]}')
def test_conv2d_layer_gradients_against_float64(form, shape, switch_on):
    k, down, act, bias = form
    n, cin, cout, res = shape
    lay = _conv_layer(k, down, act, bias, cin, cout)
    ref = _double(lay)
    g = torch.Generator().manual_seed(res + cin)
    x = torch.randn(n, cin, res, res, generator=g)
    xr = x.double().requires_grad_(True)
    yr = ref(xr)
    P = _off_kinks(ref, yr.detach(), torch.randn(yr.shape, generator=g, dtype=torch.float64))
    (yr * P).sum().backward()

    lay = lay.to(DEV)
    xd = x.to(DEV).requires_grad_(True)
    with torch.no_grad():
        y_inf = lay(xd)

    def step():
        y = lay(xd)
        (y * P.to(DEV, torch.float32)).sum().backward()
        return y
    y, names = _profiled(step)
    assert type(y.grad_fn).__name__.startswith('_PlainConvGrad'), type(y.grad_fn).__name__
    assert torch.equal(y.detach(), y_inf), 'the training forward differs from the inference forward'
    assert not _conv_names(names), _conv_names(names)
    errs = {'y': _err(y, yr), 'x': _err(xd.grad, xr.grad), 'weight': _err(lay.weight.grad, ref.weight.grad)}
    if bias:
        errs['bias'] = _err(lay.bias.grad, ref.bias.grad)
    print(f'Conv2dLayer {form} {shape}: ' + ', '.join(f'{a} {b:.2e}' for a, b in errs.items()))
    assert all(v < GRAD_TOL for v in errs.values()), errs

    # without a gradient for x: the forward's convolution (and FIR) only
    for p in lay.parameters():
        p.grad = None
    before = _calls()
    x_plain = x.to(DEV)
    (lay(x_plain) * P.to(DEV, torch.float32)).sum().backward()
    used = _delta(before, _calls())
    assert used['modconv2d'] == 1 and used['upfirdn2d'] == (1 if down == 2 else 0), used
    assert x_plain.grad is None and not x_plain.requires_grad
    # the weight gradient still ran, once: the 3x3 launch or the 1x1 one, never both
    assert (used['modconv_weight_grad'], used['head_weight_grad']) == ((1, 0) if k == 3 else (0, 1)), used
    assert used['bias_noise_grad'] == (1 if bias else 0), used
    assert _err(lay.weight.grad, ref.weight.grad) < GRAD_TOL


# ---- 4. the projector ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n', [1, 3])
def test_projector_against_float64(n, switch_on):
    from training import encoders
    torch.manual_seed(n)
    proj = encoders.EqualConv2d(512, 2 * 64, 4, padding=0, bias=False)
    ref = copy.deepcopy(proj).double()
    g = torch.Generator().manual_seed(10 + n)
    x = torch.randn(n, 512, 4, 4, generator=g)
    P = torch.randn(n, 128, 1, 1, generator=g, dtype=torch.float64)
    xr = x.double().requires_grad_(True)
    yr = ref(xr)
    (yr * P).sum().backward()
    proj = proj.to(DEV)
    xd = x.to(DEV).requires_grad_(True)

    def step():
        y = proj(xd)
        (y * P.to(DEV, torch.float32)).sum().backward()
        return y
    before = _calls()
    y, names = _profiled(step)
    used = _delta(before, _calls())
    assert not _conv_names(names), _conv_names(names)
    assert used['linear'] == 1 and used['linear_backward_input'] == 1 and used['linear_weight_grad'] == 1, used
    errs = {'y': _err(y, yr), 'x': _err(xd.grad, xr.grad), 'weight': _err(proj.weight.grad, ref.weight.grad)}
    print(f'EqualConv2d 4x4 n {n}: ' + ', '.join(f'{a} {b:.2e}' for a, b in errs.items()))
    assert all(v < GRAD_TOL for v in errs.values()), errs


def test_padded_equal_conv_keeps_aten(switch_on):
    from training import encoders
    torch.manual_seed(0)
    conv = encoders.EqualConv2d(16, 8, 3, padding=1, bias=False).to(DEV)
    x = torch.randn(2, 16, 4, 4, device=DEV, requires_grad=True)
    before = _calls()
    _, names = _profiled(lambda: conv(x).square().sum().backward())
    assert _conv_names(names)
    assert not any(_delta(before, _calls()).values())


# ---- the residual join alone, and on a block -----------------------------------------------------------------------------------------------
# counts: one float; a tail behind whole 16-byte groups; more than one workgroup (256 threads x 4 floats) with a tail; the 8^2 x 512 map.
# `offset` floats into a larger buffer: 0 = 16-byte aligned operands, 1 = the float-by-float kernel
@pytest.mark.parametrize('offset', [0, 1], ids=['aligned', 'unaligned'])
@pytest.mark.parametrize('count', [1, 7, 1027, 2 * 512 * 8 * 8])
def test_residual_join_equals_the_elementwise_definition_bit_for_bit(count, offset):
    from torch_utils import hip_plugin
    P = hip_plugin.IdLossPlugin
    g = torch.Generator().manual_seed(count)
    a = torch.randn(count + offset, generator=g).to(DEV)[offset:]
    b = torch.randn(count + offset, generator=g).to(DEV)[offset:]
    gain = 1 / 2 ** 0.5
    before = _calls(('residual_join',))
    y = P.residual_join(a, b, gain)
    d = P.residual_join(a, None, gain)
    assert _delta(before, _calls(('residual_join',))) == {'residual_join': 2}
    assert y.shape == a.shape and torch.equal(y, (a + b) * gain) and torch.equal(d, a * gain)
    assert _err(y, (a.cpu().double() + b.cpu().double()) * gain) < KERNEL_TOL


def test_residual_join_refuses_what_it_does_not_cover():
    from torch_utils import hip_plugin
    P = hip_plugin.IdLossPlugin
    a = torch.randn(8, device=DEV)
    before = _calls(('residual_join',))
    for bad in (lambda: P.residual_join(a, torch.randn(9, device=DEV), 1.0), lambda: P.residual_join(a[:0], None, 1.0),
                lambda: P.residual_join(a.double(), None, 1.0)):
        with pytest.raises(RuntimeError):
            bad()
    assert _delta(before, _calls(('residual_join',))) == {'residual_join': 0}


def test_encoder_block_joins_in_one_launch_each_way(switch_on):
    """EncoderResBlock with the switch on: one ide3d_residual_join forward and one backward, the forward bit-equal to the no_grad inference
    forward (whose join is the two ATen operators), gradients against float64."""
    from training import encoders
    torch.manual_seed(7)
    blk = encoders.EncoderResBlock(40, 72)
    with torch.no_grad():
        blk.conv1.bias.normal_(0, 0.3); blk.conv2.bias.normal_(0, 0.3)
    ref = _double(blk)
    g = torch.Generator().manual_seed(8)
    x = torch.randn(2, 40, 10, 10, generator=g); P = torch.randn(2, 72, 5, 5, generator=g)
    xr = x.double().requires_grad_(True)
    (ref(xr) * P.double()).sum().backward()
    blk = blk.to(DEV)
    xi = x.to(DEV).requires_grad_(True)
    before = _calls(('residual_join',))
    y = blk(xi)
    assert _delta(before, _calls(('residual_join',))) == {'residual_join': 1}
    (y * P.to(DEV)).sum().backward()
    assert _delta(before, _calls(('residual_join',))) == {'residual_join': 2}
    with torch.no_grad():
        assert torch.equal(y.detach(), blk(x.to(DEV)))
    assert _delta(before, _calls(('residual_join',))) == {'residual_join': 2}          # inference keeps its path
    errs = {'x': _err(xi.grad, xr.grad), **{k: _err(p.grad, dict(ref.named_parameters())[k].grad) for k, p in blk.named_parameters()}}
    print('EncoderResBlock(40, 72) against float64: ' + ', '.join(f'{a} {b:.2e}' for a, b in errs.items()))
    assert all(v < GRAD_TOL for v in errs.values()), errs


# ---- 5. / 6. the whole network ---------------------------------------------------------------------------------------------------------------
def _encoder(seed=0):
    from training import encoders
    torch.manual_seed(seed)
    E = encoders.HybridEncoder(size=16, n_latents_app=2, n_latents_geo=1, w_dim=64)
    with torch.no_grad():
        for name, p in E.named_parameters():
            if name.endswith('bias'):
                p.normal_(0, 0.3)
    return E


def _encoder_inputs(seed=1):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(2, 3, 16, 16, generator=g), torch.randn(2, 19, 16, 16, generator=g), torch.randn(2, 3, 64, generator=g)


def test_hybrid_encoder_parameter_gradients_against_float64(switch_on):
    E = _encoder()
    ref = _double(E)
    img, seg, P = _encoder_inputs()
    (ref(img.double(), seg.double()) * P.double()).sum().backward()
    want = {k: p.grad for k, p in ref.named_parameters()}
    E = E.to(DEV)

    def step():
        ws = E(img.to(DEV), seg.to(DEV))
        (ws * P.to(DEV)).sum().backward()
        return ws
    before = _calls()
    ws, names = _profiled(step)
    used = _delta(before, _calls())
    assert not _conv_names(names), _conv_names(names)
    assert used['modconv_weight_grad'] > 0 and used['head_weight_grad'] > 0 and used['linear_weight_grad'] == 2, used
    assert used['residual_join'] == 2 * 2 * 2, used             # two towers of two blocks (16 -> 8 -> 4), forward and backward
    errs = {k: _err(p.grad, want[k]) for k, p in E.named_parameters()}
    assert set(errs) == set(want)
    worst = max(errs, key=errs.get)
    print(f'HybridEncoder(16): worst parameter {worst}: {errs[worst]:.2e} over {len(errs)} parameters')
    bad = {k: v for k, v in errs.items() if not v < GRAD_TOL}
    assert not bad, bad


def test_steps_after_in_place_updates_use_the_new_weights(switch_on):
    """The launches read cached products of the parameters (the scaled weights, their transposes) and packed copies of those in the
    workspaces: after Adam's in-place update, the next forward must read the new values."""
    from training import encoders
    E = _encoder(2).to(DEV)
    img, seg, P = (t.to(DEV) for t in _encoder_inputs(3))
    opt = torch.optim.Adam(E.parameters(), lr=1e-2)
    for step in range(2):
        opt.zero_grad(set_to_none=True)
        ws = E(img, seg)
        assert type(ws.grad_fn).__name__ != 'NoneType'
        if step > 0:
            fresh = encoders.HybridEncoder(size=16, n_latents_app=2, n_latents_geo=1, w_dim=64).to(DEV)
            fresh.load_state_dict(E.state_dict())
            assert torch.equal(ws.detach(), fresh(img, seg).detach()), 'the forward after an in-place update read stale weights'
            with torch.no_grad():
                assert torch.equal(E.convs_img(img), fresh.convs_img(img))
        (ws * P).sum().backward()
        opt.step()
    # and the backward's cached transposes: the second step's gradients equal the fresh module's
    fresh = encoders.HybridEncoder(size=16, n_latents_app=2, n_latents_geo=1, w_dim=64).to(DEV)
    fresh.load_state_dict(E.state_dict())
    grads = []
    for m in (E, fresh):
        m.zero_grad(set_to_none=True)
        xi = img.clone().requires_grad_(True)
        (m(xi, seg) * P).sum().backward()
        grads.append(xi.grad)
    assert torch.equal(*grads)


# ---- 7. switch off -----------------------------------------------------------------------------------------------------------------------------
def test_switch_off_routes_nothing_through_the_new_functions():
    from training import encoders, networks
    assert networks.hip_plain_conv_grad is False
    torch.manual_seed(5)
    blk = encoders.EncoderResBlock(40, 72).to(DEV)
    x = torch.randn(2, 40, 10, 10, device=DEV)
    P = torch.randn(2, 72, 5, 5, device=DEV)

    def grads():
        blk.zero_grad(set_to_none=True)
        xi = x.clone().requires_grad_(True)
        y = blk(xi)
        (y * P).sum().backward()
        return {'x': xi.grad, **{k: p.grad.clone() for k, p in blk.named_parameters()}}
    before = _calls(NEW_CALLS)
    off, names = _profiled(grads)
    assert not any(_delta(before, _calls(NEW_CALLS)).values()), _delta(before, _calls(NEW_CALLS))
    assert _conv_names(names)
    networks.hip_plain_conv_grad = True
    try:
        on = grads()
    finally:
        networks.hip_plain_conv_grad = False
    assert _delta(before, _calls(NEW_CALLS))['modconv_weight_grad'] == 2
    errs = {k: _err(on[k], off[k]) for k in off}
    print('EncoderResBlock switch on vs off: ' + ', '.join(f'{a} {b:.2e}' for a, b in errs.items()))
    assert all(v < GRAD_TOL for v in errs.values()), errs
