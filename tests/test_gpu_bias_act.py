"""`ide3d_bias_act` (csrc/bias_act.hip) in all three orders against float64 (tests/bias_act_cases.py: the plain definition and its autograd
on the stored inputs), through the public `bias_act()` surface and directly through `BiasActPlugin.bias_act`: fp32, fp16, bf16 and float64
storage; the 16-byte vector loads of x, xref, yref and dy, the scalar tail, the per-element bias index (channels-last, [N, C], dim != 1), the
unaligned-base fallback, the plane kernel's entry threshold, the second trip of the grid-stride loop, and the branch points of the formulas.

Bound (tests/edge_bound.py): error against float64 <= max(4 x the error of the same definition evaluated by ATen in the storage type on the
same device, one ulp of the storage type at the largest magnitude).  Exact results are compared exactly: zeros where clamped or where the
derivative is an exact zero, the clamp value where clamped, dy itself on the positive side of relu and lrelu with gain 1.
Measured on an MI355X (profiles/small_ops/edge_suite_measured.json): no comparison outside its bound; the largest error / bound is 0.99 in
fp32 (db), 0.56 in fp16 and bf16, 0.50 in float64 through the public surface, 0.38 from unaligned bases (1.00 in float64: d_x of swish, at
ATen's own error), 0.25 across the plane-kernel threshold.  The gradients of the smooth activations are formed from x + b, which the op
keeps for them; formed from the stored y, as the reference kernel does, tanh, sigmoid, elu, selu and swish missed the bound by factors of
1.1 to 3 on the 30-element layout (for instance bf16 d_x 6.1e-03 against 2.0e-03, fp32 d_x 3.5e-07 against 2.1e-07)."""

import os

import pytest
import torch

import bias_act_cases as bc
from edge_bound import max_err, ulp, within

pytestmark = pytest.mark.gpu

DTYPES = {'float32': torch.float32, 'float16': torch.float16, 'bfloat16': torch.bfloat16, 'float64': torch.float64}


def _calls():
    from torch_utils import hip_plugin
    return hip_plugin.CALLS.get('bias_act', 0)


def _to_layout(t, layout, dev):
    t = t.to(dev)
    return t.contiguous(memory_format=torch.channels_last) if layout.channels_last else t


def _orders(fn, x, b, dy, ddx, second=True):
    """(y, dx, db, d_dy, d_x) of y = fn(x, b) by autograd: dx, db = dy-weighted first order; d_dy, d_x = ddx-weighted derivatives of dx."""
    xx = x.detach().requires_grad_(True)
    bb = None if b is None else b.detach().requires_grad_(True)
    dyy = dy.detach().requires_grad_(True)
    y = fn(xx, bb)
    grads = torch.autograd.grad(y, [xx] + ([bb] if bb is not None else []), dyy, create_graph=second)
    dx, db = grads[0], (grads[1] if bb is not None else None)
    d_dy = d_x = None
    if second and dx.requires_grad:
        d_dy, d_x = torch.autograd.grad(dx, [dyy, xx], ddx, allow_unused=True)
    return [None if t is None else t.detach() for t in (y, dx, db, d_dy, d_x)]


def _aten_orders(x, b, dy, ddx, layout, act, cfg, dtype):
    """The plain definition by ATen on the device in the storage type; where ATen cannot differentiate twice in that type, in fp32 and rounded."""
    from torch_utils.ops import bias_act
    fn = lambda xx, bb: bias_act._bias_act_ref(xx, bb, dim=layout.dim if layout.dim is not None else 1, act=act, alpha=cfg.alpha, gain=cfg.gain, clamp=cfg.clamp)
    try:
        return _orders(fn, x, b, dy, ddx)
    except RuntimeError:
        up = lambda t: None if t is None else t.float()
        return [None if t is None else t.to(dtype) for t in _orders(fn, up(x), up(b), up(dy), up(ddx))]


def _compare(what, kernel, name, g, a, want, free, und, skip, dtype, layout, act, cfg, dy, ddx, g_dx=None):
    """One quantity of one case against float64 (bound and exact parts).  `und`: elements whose clamp decision may fall either way, for the
    kernel and for ATen alike (either value counts); `skip`: the kinks, where ATen follows another convention and therefore says nothing
    about the error of the definition."""
    w, f = getattr(want, name), getattr(free, name)
    other = [i for i in range(want.y.ndim) if i != layout.dim]
    if name == 'db':
        # ATen's own db without what its skipped elements contribute beyond the reference; where the sum holds an undecided element, either sum
        a_db, a_dx = a
        a = a_db.cpu().double() - torch.where(skip, a_dx.cpu().double() - want.dx, torch.zeros_like(want.dx)).sum(other)
        # an undecided element counts as the kernel's own dx decided it (inside the clamp, or clamped): db is the sum of that dx
        if bool(und.any()):
            gd = g_dx.cpu().double()
            pick = torch.where((gd - free.dx).abs() < gd.abs(), free.dx, torch.zeros_like(gd))
            w = torch.where(und, pick, want.dx).sum(other)
        return within(g, w, a, dtype, kernel, name)
    a = torch.where(skip, w, torch.zeros_like(w) if a is None else a.cpu().double())
    if name == 'y':
        ok = within(g, w, a, dtype, kernel, name)
    else:
        ok = within(g, w, a, dtype, kernel, name, alt=(f, torch.zeros_like(w)), undecided=und)          # inside the clamp, or clamped: either
    gc = g.cpu().double()
    if name != 'y':
        exact0 = (w == 0) & ~und
        if act in ('tanh', 'sigmoid', 'swish') and cfg.gain != 0:
            # a zero of the reference next to saturation is its own rounding (1 - t^2 with t rounded to 1; the true value is 4 e^-2|u|,
            # which the kernel may well return): exact zeros are required where the output is clamped only
            exact0 = exact0 & (want.yu.abs() >= (cfg.clamp if cfg.clamp is not None else float('inf')))
        assert not bool(gc[exact0].any()), f'{what} {name}: {int((gc[exact0] != 0).sum())} values that must be exact zeros are not'
    elif cfg.clamp is not None:
        out = (want.yu.abs() > cfg.clamp) & ~und
        assert torch.equal(gc[out], want.y[out]), f'{what}: clamped outputs are not the clamp value'
    if name in ('dx', 'd_dy') and act in ('relu', 'lrelu') and cfg.gain == 1:
        src = (dy if name == 'dx' else ddx).double()
        through = (want.yu > 0) & (want.yu.abs() < (cfg.clamp if cfg.clamp is not None else float('inf'))) & ~und
        assert torch.equal(gc[through], src[through]), f'{what} {name}: the positive side must pass the gradient through unchanged'
    return ok


def _reference(layout, dtype, act, cfg):
    x, b, dy, ddx = bc.inputs(layout, dtype, cfg)
    if dtype == torch.float64:          # a float64 evaluation is no reference for a float64 launch: 40-digit decimal arithmetic
        want, free = bc.closed_form_exact(x, b, layout.dim, act, cfg, dy, ddx)
    else:
        want = bc.closed_form(x, b, layout.dim, act, cfg, dy, ddx)
        free = bc.closed_form(x, b, layout.dim, act, cfg._replace(clamp=None), dy, ddx)          # what an element gives if it counts as inside the clamp
    und = bc.undecided(want, act, cfg, ulp(bc.CLAMP, dtype))
    skip = bc.kinks(x, b, layout.dim, act, cfg)
    return x, b, dy, ddx, want, free, und, skip


def _check_case(dev, layout, dtype, act, cfg, what, second=True, forward_only=False):
    from torch_utils.ops import bias_act
    x, b, dy, ddx, want, free, und, skip = _reference(layout, dtype, act, cfg)
    xd, dyd, ddxd = (_to_layout(t, layout, dev) for t in (x, dy, ddx))
    bd = None if b is None else b.to(dev)
    kw = dict(dim=layout.dim if layout.dim is not None else 1, act=act, alpha=cfg.alpha, gain=cfg.gain, clamp=cfg.clamp)
    fn = lambda xx, bb: bias_act.bias_act(xx, bb, **kw)
    identity = act == 'linear' and cfg.gain == 1 and cfg.clamp is None
    before = _calls()
    if forward_only:
        got = [fn(xd, bd)] + [None] * 4
        aten = [bias_act._bias_act_ref(xd, bd, **kw)] + [None] * 4
        launches = 1
    else:
        got = _orders(fn, xd, bd, dyd, ddxd, second)
        aten = _aten_orders(xd, bd, dyd, ddxd, layout, act, cfg, dtype)
        # forward; the first-order launch; with `second`, that launch again for d(dx)/d(dy), the second-order launch of a smooth activation,
        # and, where the first-order node took y as an input, one more first-order launch: the engine runs the forward node's backward
        # with a zero gradient for y (nothing of dx depends on y)
        keeps_y = 'y' in bias_act.activation_funcs[act].ref
        launches = (0 if identity and b is None else 1) + (0 if identity else 1 + ((1 + (act in bc.SMOOTH) + keeps_y) if second else 0))
    assert _calls() - before == launches, (what, _calls() - before, launches)
    y = got[0]
    assert y.dtype == dtype and y.shape == xd.shape and y.stride() == xd.stride()
    ok = True
    for name, g, a in zip(('y', 'dx', 'db', 'd_dy', 'd_x'), got, aten):
        if g is None:
            assert forward_only or (name == 'db' and b is None) or (name in ('d_dy', 'd_x') and not second) or (name == 'd_x' and act not in bc.SMOOTH), (what, name)
            continue
        if name == 'db':
            a = (aten[2], aten[1])
        ok &= _compare(what, 'bias_act', name, g, a, want, free, und, skip, dtype, layout, act, cfg, dy, ddx, g_dx=got[1])
    assert ok, f'{what}: outside the bound (figures above)'


@pytest.mark.parametrize('act', bc.ACTS)
@pytest.mark.parametrize('dtype', ['float32', 'float16', 'bfloat16'])
@pytest.mark.parametrize('layout', bc.LAYOUTS, ids=[l.name for l in bc.LAYOUTS])
def test_all_orders_through_the_public_surface(gpu_device, layout, dtype, act):
    """Every parameter set of the case module; y, dx, db, d(dx)/d(dy) and d(dx)/dx, and the number of launches.

    lrelu with a negative slope has y > 0 on both sides of its kink: the op keeps x for it and the first-order launch reads the side from
    x + b (with the sign of y, as the reference kernel has it, dx was off by up to 1.09e+01 at alpha = -0.5).
    Measured on an MI355X: profiles/small_ops/edge_suite_measured.json, kernel bias_act."""
    for cfg in bc.configs(act):
        if act == 'linear' and cfg.clamp is not None:
            _check_case(gpu_device, layout, DTYPES[dtype], act, cfg, f'{layout.name} {dtype} {act} {cfg} forward', forward_only=True)
            cfg = cfg._replace(clamp=None)
        _check_case(gpu_device, layout, DTYPES[dtype], act, cfg, f'{layout.name} {dtype} {act} {cfg}')


@pytest.mark.parametrize('act', bc.ACTS)
def test_all_orders_in_float64(gpu_device, act):
    """One shape; the reference is the 40-digit evaluation of the case module (a float64 evaluation carries a few ulp of its own).
    Measured: profiles/small_ops/edge_suite_measured.json, kernel bias_act, float64."""
    layout = bc.LAYOUT_BY_NAME['nchw_tail']
    for cfg in bc.configs(act):
        if act == 'linear' and cfg.clamp is not None:
            cfg = cfg._replace(clamp=None)
        _check_case(gpu_device, layout, torch.float64, act, cfg, f'float64 {act} {cfg}')


@pytest.mark.parametrize('channels_last', [False, True], ids=['nchw_order1', 'channels_last_forward'])
def test_second_trip_of_the_grid_stride_loop(gpu_device, channels_last):
    """527 816 fp32 vectors on 2048 x 256 lanes: first order in NCHW (tanh reads yref, swish xref), forward in channels-last."""
    layout = bc.BIG._replace(channels_last=channels_last)
    cfg = bc.CONFIGS[1]
    for act in ('tanh', 'swish'):
        _check_case(gpu_device, layout, torch.float32, act, cfg, f'second trip {act}', second=False, forward_only=channels_last)


@pytest.mark.parametrize('dtype,planes', [('float32', (1020, 1024, 1028)), ('float16', (2040, 2048, 2056))])
def test_plane_kernel_threshold(gpu_device, dtype, planes):
    """Planes of 255, 256 and 257 vectors: the forward pass enters the plane kernel at 256.  Bit-equal to the indexed kernel
    (IDE3D_BIAS_ACT_NO_PLANES=1) on both sides of the threshold, and inside the bound against float64."""
    from torch_utils.ops import bias_act
    dt = DTYPES[dtype]
    bits = torch.int32 if dt == torch.float32 else torch.int16
    for plane in planes:
        for shape, dim in (((2, 3, 1, plane), 1), ((1, 1, 1, plane), None)):
            layout = bc.Layout('plane', shape, dim, False, '')
            for act, cfg in (('lrelu', bc.CONFIGS[0]), ('sigmoid', bc.CONFIGS[1]), ('linear', bc.CONFIGS[2])):
                x, b, dy, ddx = bc.inputs(layout, dt, cfg)
                xd, bd = x.to(gpu_device), None if b is None else b.to(gpu_device)
                kw = dict(dim=1, act=act, alpha=cfg.alpha, gain=cfg.gain, clamp=cfg.clamp)
                y = bias_act.bias_act(xd, bd, **kw)
                try:
                    os.environ['IDE3D_BIAS_ACT_NO_PLANES'] = '1'
                    indexed = bias_act.bias_act(xd, bd, **kw)
                finally:
                    os.environ.pop('IDE3D_BIAS_ACT_NO_PLANES', None)
                assert torch.equal(y.view(bits), indexed.view(bits)), (plane, shape, act)
                want = bc.closed_form(x, b, dim, act, cfg, dy, ddx)
                assert within(y, want.y, bias_act._bias_act_ref(xd, bd, **kw), dt, 'bias_act_plane', 'y'), (plane, shape, act)


@pytest.mark.parametrize('dtype,layout', [('float32', 'nchw_tail'), ('float16', 'nchw_step5'), ('bfloat16', 'fc'), ('float64', 'dim2')])
def test_unaligned_bases_take_the_scalar_kernel(gpu_device, dtype, layout):
    """Directly through BiasActPlugin.bias_act: x, xref, yref and dy are views that start one element into a larger buffer.  All three orders
    equal the aligned launches bit for bit (same operations per element), stay inside the bound, and leave the buffers' margins alone.
    Measured: profiles/small_ops/edge_suite_measured.json, kernel bias_act_scalar.  (The softplus gradients are formed from x + b, which the
    op keeps: from the stored y the float64 second order was 4.72e-16 from the reference against a bound of 4.44e-16.)"""
    from torch_utils import hip_plugin
    from torch_utils.ops import bias_act
    P = hip_plugin.BiasActPlugin.bias_act
    dt, layout = DTYPES[dtype], bc.LAYOUT_BY_NAME[layout]
    null = torch.empty([0], dtype=dt, device=gpu_device)
    for act in ('lrelu', 'tanh', 'softplus', 'swish'):
        cfg = bc.CONFIGS[1]
        idx = bias_act.activation_funcs[act].cuda_idx
        x, b, dy, ddx, want, free, und, skip = _reference(layout, dt, act, cfg)
        xd, dyd, ddxd, bd = x.to(gpu_device), dy.to(gpu_device), ddx.to(gpu_device), b.to(gpu_device)
        args = (layout.dim, idx, cfg.alpha, cfg.gain, cfg.clamp)
        y = P(xd, bd, null, null, null, 0, *args)
        aligned = [y, P(dyd, bd, xd, y, null, 1, *args), P(ddxd, bd, xd, y, dyd, 2, *args)]
        (xv, xbuf), (yv, ybuf), (dyv, dybuf), (ddxv, ddxbuf) = (bc.offset_view(t) for t in (xd, y, dyd, ddxd))
        assert all(v.data_ptr() % 16 for v in (xv, yv, dyv, ddxv))
        before = _calls()
        shifted = [P(xv, bd, null, null, null, 0, *args), P(dyv, bd, xv, yv, null, 1, *args), P(ddxv, bd, xv, yv, dyv, 2, *args)]
        assert _calls() == before + 3
        aten = _aten_orders(xd, bd, dyd, ddxd, layout, act, cfg, dt)
        ok = True
        for name, s, al, a in zip(('y', 'dx', 'd_x'), shifted, aligned, (aten[0], aten[1], aten[4])):
            assert torch.equal(s, al), f'{dtype} {act} {name}: the scalar kernel differs from the vector kernel'
            ok &= _compare(f'unaligned {dtype} {act}', 'bias_act_scalar', name, s, a, want, free, und, skip, dt, layout, act, cfg, dy, ddx)
        assert ok, f'unaligned {dtype} {act}: outside the bound (figures above)'
        for view, buf, src in ((xv, xbuf, xd), (yv, ybuf, y), (dyv, dybuf, dyd), (ddxv, ddxbuf, ddxd)):
            n = src.numel()
            assert bool((buf[:1] == 1234.5).all()) and bool((buf[1 + n:] == 1234.5).all()) and torch.equal(view, src)
