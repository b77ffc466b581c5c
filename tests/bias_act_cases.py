"""The inputs and the float64 reference of the bias_act suites: tests/test_bias_act_cases_cpu.py pins the closed forms below to float64
autograd through the plain definition (`torch_utils.ops.bias_act._bias_act_ref`), tests/test_gpu_bias_act.py runs `ide3d_bias_act`
(csrc/bias_act.hip) in all three orders against them.

Orders, for u = x + b, y = clamp(a(u) gain):
    0   y
    1   dx   = dy  gain a'(u)      where |a(u) gain| < clamp, else 0          (db = dx summed to the bias axis)
        d_dy = ddx gain a'(u)      the same launch with ddx in the place of dy: d(dx)/d(dy) applied to ddx
    2   d_x  = ddx dy gain a''(u)  where |a(u) gain| < clamp, else 0: d(dx)/dx applied to ddx

Conventions at the points where the definition is not differentiable (those of the reference kernel; autograd differs at some):
    |y| == clamp       gradient 0 (torch.clamp passes the gradient at its ends)
    u == 0             relu' = 0, lrelu' = alpha, elu' = 1, selu' = scale (autograd: scale alpha), elu'' = selu'' = 0 (autograd: e^0 and
                       scale alpha e^0)
    softplus, u > 20   a = u, a' = 1, a'' = 0: the definition's threshold
    lrelu, alpha < 0   y is positive on both sides of the kink: the op keeps x and the side comes from u, not from the sign of y
    linear             keeps neither x nor y for the backward pass, so its gradient is not zeroed where y was clamped; the gradient cases
                       of 'linear' run without clamp, as tests/test_gpu_ops.py::test_bias_act_gradients does

All parameters are exact in fp32 (the C ABI takes alpha, gain and clamp as fp32): gain 0, 0.75, 1, 2, clamp 2, alpha 0.25, 0, -0.5.
Biases are multiples of 1/4 in [-4, 4], so that x = t - b is exact in every storage type for the planted u = t that have to be exact."""

import collections
import decimal

import torch

ACTS = ('linear', 'relu', 'lrelu', 'tanh', 'sigmoid', 'elu', 'selu', 'softplus', 'swish')
SMOOTH = ('tanh', 'sigmoid', 'elu', 'selu', 'softplus', 'swish')          # a second-order launch exists
EXACT_POSITIVE_SIDE = ('linear', 'relu', 'lrelu', 'elu')                   # a(u) = u for u > 0: y = u gain is exact for gain 1 and 2
SELU_SCALE, SELU_ALPHA = 1.0507009873554804934193349852946, 1.6732632423543772848170429916717
CLAMP = 2.0

Config = collections.namedtuple('Config', 'gain clamp alpha')
# (gain, clamp, alpha); the lrelu-only ones carry another alpha
CONFIGS = (Config(1.0, CLAMP, 0.25), Config(2.0, CLAMP, 0.25), Config(0.75, None, 0.25), Config(0.0, None, 0.25))
LRELU_CONFIGS = (Config(1.0, CLAMP, 0.0), Config(2.0, None, -0.5))

Layout = collections.namedtuple('Layout', 'name shape dim channels_last why')
LAYOUTS = (
    Layout('nchw_tail', (3, 5, 17, 13), 1, False, 'numel % 4 == 3 and % 8 == 3: the scalar tail after the vectors; bias step 221: per element'),
    Layout('nchw_step5', (2, 3, 1, 5), 1, False, 'bias step 5, no multiple of the vector: a vector spans two channels'),
    Layout('channels_last', (2, 8, 9, 7), 1, True, 'bias step 1'),
    Layout('fc', (5, 33), 1, False, '2-D [N, C] as in every fully connected layer: bias step 1, 165 elements'),
    Layout('dim0', (4, 3, 6, 5), 0, False, 'bias along the batch axis: step 90'),
    Layout('dim2', (4, 3, 6, 5), 2, False, 'bias along the rows: step 5, size 6'),
    Layout('no_bias', (2, 3, 4, 4), None, False, 'b = None'),
)
LAYOUT_BY_NAME = {l.name: l for l in LAYOUTS}
BIG = Layout('second_trip', (3, 5, 401, 351), 1, False, '527 816 fp32 vectors > 2048 x 256 lanes, and a tail of one element')

# planted u = x + b: the branch points of the formulas
PLANTED = (0.0, 'clamp+', 'clamp-', 90.0, -90.0, 45.0, -45.0, 21.0, 20.5, -0.25)


def configs(act):
    return CONFIGS + (LRELU_CONFIGS if act == 'lrelu' else ())


def _bias_view(b, shape, dim):
    s = [1] * len(shape)
    s[dim] = -1
    return b.reshape(s)


def inputs(layout, dtype, cfg, seed=0):
    """(x, b | None, dy, ddx) in `dtype` on the CPU, NCHW-contiguous.  x: randn * 3 with the planted values at every 7th element (closer in a small tensor) from the
    front and in the last elements (the tail), so that u = x + b is exactly the planted value where that matters (0 and +-clamp / gain)."""
    g = torch.Generator().manual_seed(seed)
    shape = layout.shape
    x = (torch.randn(*shape, generator=g, dtype=torch.float64) * 3).to(dtype)
    dy = torch.randn(*shape, generator=g, dtype=torch.float64).to(dtype)
    ddx = torch.randn(*shape, generator=g, dtype=torch.float64).to(dtype)
    b = None
    bias = torch.zeros(shape, dtype=torch.float64)
    if layout.dim is not None:
        b = (torch.randint(-16, 17, (shape[layout.dim],), generator=g).double() / 4).to(dtype)
        bias = _bias_view(b.double(), shape, layout.dim).expand(shape)
    edge = CLAMP / cfg.gain if cfg.gain else 1.0
    targets = [edge if t == 'clamp+' else -edge if t == 'clamp-' else t for t in PLANTED]
    n = x.numel()
    flat, fb = x.reshape(-1), bias.reshape(-1)
    step = max(1, min(7, (n - 3) // len(targets)))
    where = [step * i for i in range(len(targets))] + [n - 1 - i for i in range(3)]
    assert len(set(where)) == len(where) and max(where) < n
    for k, p in enumerate(where):
        flat[p] = (targets[k % len(targets)] - fb[p]).to(dtype)
    return x, b, dy, ddx


def act_terms(act, u, alpha):
    """(a, a', a'') of float64 u, with the conventions of the module docstring."""
    one, zero = torch.ones_like(u), torch.zeros_like(u)
    if act == 'linear':
        return u, one, zero
    if act == 'relu':
        return torch.where(u > 0, u, zero), torch.where(u > 0, one, zero), zero
    if act == 'lrelu':
        return torch.where(u > 0, u, u * alpha), torch.where(u > 0, one, one * alpha), zero
    if act == 'tanh':
        t = torch.tanh(u)
        return t, 1 - t * t, -2 * t * (1 - t * t)
    if act == 'sigmoid':
        s = torch.sigmoid(u)
        return s, s * (1 - s), s * (1 - s) * (1 - 2 * s)
    if act == 'elu':
        e = torch.exp(u)
        return torch.where(u >= 0, u, torch.expm1(u)), torch.where(u >= 0, one, e), torch.where(u >= 0, zero, e)
    if act == 'selu':
        e = SELU_SCALE * SELU_ALPHA * torch.exp(u)
        return torch.where(u >= 0, SELU_SCALE * u, SELU_SCALE * SELU_ALPHA * torch.expm1(u)), torch.where(u >= 0, SELU_SCALE * one, e), torch.where(u >= 0, zero, e)
    if act == 'softplus':
        s = torch.sigmoid(u)
        return torch.where(u > 20, u, torch.log1p(torch.exp(u))), torch.where(u > 20, one, s), torch.where(u > 20, zero, s * (1 - s))
    if act == 'swish':
        s = torch.sigmoid(u)
        return u * s, s + u * s * (1 - s), s * (1 - s) * (2 + u * (1 - 2 * s))
    raise KeyError(act)


Terms = collections.namedtuple('Terms', 'y dx db d_dy d_x yu')


def closed_form(x, b, dim, act, cfg, dy, ddx):
    """The five quantities in float64 from inputs in any dtype (their stored values are the operands), and yu = a(u) gain before the clamp."""
    x, dy, ddx = x.double(), dy.double(), ddx.double()
    u = x if b is None else x + _bias_view(b.double(), x.shape, dim)
    a, a1, a2 = act_terms(act, u, cfg.alpha)
    yu = a * cfg.gain
    y, live = yu, torch.ones_like(u, dtype=torch.bool)
    if cfg.clamp is not None:
        y = yu.clamp(-cfg.clamp, cfg.clamp)
        if act != 'linear':
            live = yu.abs() < cfg.clamp
    zero = torch.zeros_like(u)
    dx = torch.where(live, dy * cfg.gain * a1, zero)
    d_dy = torch.where(live, ddx * cfg.gain * a1, zero)
    d_x = torch.where(live, ddx * dy * cfg.gain * a2, zero)
    db = None if b is None else dx.sum([i for i in range(x.ndim) if i != dim])
    return Terms(y, dx, db, d_dy, d_x, yu)


def _act_terms_exact(act, u, alpha):
    """(a, a', a'') of one decimal.Decimal u, the same expressions as `act_terms`."""
    D = decimal.Decimal
    zero, one, two = D(0), D(1), D(2)
    if act == 'linear':
        return u, one, zero
    if act == 'relu':
        return (u, one, zero) if u > 0 else (zero, zero, zero)
    if act == 'lrelu':
        return (u, one, zero) if u > 0 else (u * alpha, alpha, zero)
    if act == 'tanh':
        e2 = (two * u).exp()
        t = (e2 - one) / (e2 + one)
        return t, one - t * t, -two * t * (one - t * t)
    if act in ('elu', 'selu'):
        sc, sa = (one, one) if act == 'elu' else (D(SELU_SCALE), D(SELU_SCALE) * D(SELU_ALPHA))
        if u >= 0:
            return sc * u, sc, zero
        e = u.exp()
        return sa * (e - one), sa * e, sa * e
    if act == 'softplus' and u > 20:
        return u, one, zero
    e = u.exp()
    s = e / (one + e)
    if act == 'sigmoid':
        return s, s * (one - s), s * (one - s) * (one - two * s)
    if act == 'softplus':
        return (one + e).ln(), s, s * (one - s)
    if act == 'swish':
        return u * s, s + u * s * (one - s), s * (one - s) * (two + u * (one - two * s))
    raise KeyError(act)


def closed_form_exact(x, b, dim, act, cfg, dy, ddx):
    """`closed_form` with and without the clamp, evaluated in 40-digit decimal arithmetic and rounded once to float64: the reference of the
    float64 launches, for which a float64 evaluation (a few ulp of its own) is no reference.  Returns (Terms with clamp, Terms without)."""
    D = decimal.Decimal
    with decimal.localcontext() as ctx:
        ctx.prec = 40
        shape = x.shape
        bias = torch.zeros(shape, dtype=torch.float64) if b is None else _bias_view(b.double(), shape, dim).expand(shape)
        xs, bs, dys, ddxs = (t.double().reshape(-1).tolist() for t in (x, bias, dy, ddx))
        gain, alpha = D(cfg.gain), D(cfg.alpha)
        clamp = None if cfg.clamp is None else D(cfg.clamp)
        rows = dict(y=[], dx=[], d_dy=[], d_x=[], yu=[], fy=[], fdx=[], fd_dy=[], fd_x=[])
        for xv, bv, dyv, ddxv in zip(xs, bs, dys, ddxs):
            a, a1, a2 = _act_terms_exact(act, D(xv) + D(bv), alpha)
            yu = a * gain
            fdx, fd_dy, fd_x = D(dyv) * gain * a1, D(ddxv) * gain * a1, D(ddxv) * D(dyv) * gain * a2
            live = clamp is None or act == 'linear' or abs(yu) < clamp
            y = yu if clamp is None else max(-clamp, min(clamp, yu))
            for k, v in (('y', y), ('yu', yu), ('fy', yu), ('fdx', fdx), ('fd_dy', fd_dy), ('fd_x', fd_x),
                         ('dx', fdx if live else D(0)), ('d_dy', fd_dy if live else D(0)), ('d_x', fd_x if live else D(0))):
                rows[k].append(v)
        other = [i for i in range(len(shape)) if i != dim]

        def tensor(vals):
            return torch.tensor([float(v) for v in vals], dtype=torch.float64).reshape(shape)

        def bias_sum(vals):
            if b is None:
                return None
            n = shape[dim]
            idx = torch.arange(n).reshape([-1 if i == dim else 1 for i in range(len(shape))]).expand(shape).reshape(-1).tolist()
            sums = [D(0)] * n
            for i, v in zip(idx, vals):
                sums[i] += v
            return torch.tensor([float(v) for v in sums], dtype=torch.float64)

        want = Terms(tensor(rows['y']), tensor(rows['dx']), bias_sum(rows['dx']), tensor(rows['d_dy']), tensor(rows['d_x']), tensor(rows['yu']))
        free = Terms(tensor(rows['fy']), tensor(rows['fdx']), bias_sum(rows['fdx']), tensor(rows['fd_dy']), tensor(rows['fd_x']), tensor(rows['yu']))
    return want, free


def kinks(x, b, dim, act, cfg):
    """Elements where autograd and the conventions above may differ: u == 0, |yu| == clamp."""
    x = x.double()
    u = x if b is None else x + _bias_view(b.double(), x.shape, dim)
    k = u == 0
    if cfg.clamp is not None:
        k = k | ((act_terms(act, u, cfg.alpha)[0] * cfg.gain).abs() == cfg.clamp)
    return k


def undecided(terms, act, cfg, dtype_ulp_at_clamp):
    """Elements whose clamp decision the kernel takes from the stored y, which carries the storage rounding (one ulp) and the evaluation of
    the activation in the math type (a few): |yu| within 8 ulp of the clamp.  y exactly at the clamp on the exact side of an activation
    (y = u gain, gain 1 or 2) is decided: the stored y is the clamp itself."""
    if cfg.clamp is None or act == 'linear':
        return torch.zeros_like(terms.yu, dtype=torch.bool)
    near = (terms.yu.abs() - cfg.clamp).abs() <= 8 * dtype_ulp_at_clamp
    if act in EXACT_POSITIVE_SIDE and cfg.gain in (1.0, 2.0):
        near = near & ~(terms.yu == cfg.clamp)
    return near


def offset_view(t, margin=8, poison=1234.5):
    """(`t`'s values as a contiguous view that starts one element into a poisoned buffer, the buffer): the base address is no multiple of 16
    bytes, which sends the launch through the scalar kernel."""
    buf = torch.full((t.numel() + 2 * margin,), poison, dtype=t.dtype, device=t.device)
    view = buf[1:1 + t.numel()].view(t.shape)
    view.copy_(t)
    return view, buf
