"""The bias_act case module (tests/bias_act_cases.py) without a GPU: its closed-form first- and second-order expressions are float64 autograd
through the plain definition wherever the definition is differentiable, they keep the stated conventions where it is not, and the inputs
reach the paths and branch points the GPU suite (tests/test_gpu_bias_act.py) is there for."""

import pytest
import torch

import bias_act_cases as bc


def _autograd(x, b, dim, act, cfg, dy, ddx):
    from torch_utils.ops import bias_act
    xx = x.double().requires_grad_(True)
    bb = None if b is None else b.double().requires_grad_(True)
    dyy = dy.double().requires_grad_(True)
    y = bias_act._bias_act_ref(xx, bb, dim=dim if dim is not None else 1, act=act, alpha=cfg.alpha, gain=cfg.gain, clamp=cfg.clamp)
    grads = torch.autograd.grad(y, [xx] + ([bb] if bb is not None else []), dyy, create_graph=True)
    dx, db = grads[0], (grads[1] if bb is not None else None)
    d_dy, d_x = torch.autograd.grad(dx, [dyy, xx], ddx.double(), allow_unused=True)
    return y.detach(), dx.detach(), None if db is None else db.detach(), d_dy, d_x


@pytest.mark.parametrize('clamped', [True, False], ids=['clamp', 'noclamp'])
@pytest.mark.parametrize('act', bc.ACTS)
def test_closed_forms_are_float64_autograd_of_the_definition(act, clamped):
    for layout in (bc.LAYOUT_BY_NAME['nchw_tail'], bc.LAYOUT_BY_NAME['fc'], bc.LAYOUT_BY_NAME['no_bias']):
        for cfg in bc.configs(act):
            if (cfg.clamp is not None) != clamped:
                continue
            if act == 'linear' and clamped:          # the quirk: see the case module
                cfg = cfg._replace(clamp=None)
            x, b, dy, ddx = bc.inputs(layout, torch.float64, cfg)
            got = bc.closed_form(x, b, layout.dim, act, cfg, dy, ddx)
            y, dx, db, d_dy, d_x = _autograd(x, b, layout.dim, act, cfg, dy, ddx)
            kink = bc.kinks(x, b, layout.dim, act, cfg)
            assert bool(kink.any()) and int(kink.sum()) <= 8
            tol = dict(rtol=1e-12, atol=1e-13)
            torch.testing.assert_close(got.y, y, **tol)          # the forward value has no convention
            torch.testing.assert_close(got.dx[~kink], dx[~kink], **tol)
            torch.testing.assert_close(got.d_dy[~kink], d_dy[~kink], **tol)
            if d_x is None:          # nothing of dx depends on x: the piecewise linear activations
                assert act in ('linear', 'relu', 'lrelu') and not bool(got.d_x.any())
            else:
                torch.testing.assert_close(got.d_x[~kink], d_x[~kink], **tol)
            if db is not None and not bool(kink.any() and (got.dx[kink] != dx[kink]).any()):
                torch.testing.assert_close(got.db, db, **tol)
            # at the kinks: the stated conventions
            u = x if b is None else x + bc._bias_view(b, x.shape, layout.dim)
            at0 = u == 0
            first = {'linear': 1, 'relu': 0, 'lrelu': cfg.alpha, 'tanh': 1, 'sigmoid': 0.25, 'elu': 1, 'selu': bc.SELU_SCALE, 'softplus': 0.5, 'swish': 0.5}[act]
            if cfg.clamp is None or first * 0 == 0:          # u = 0 gives y = a(0) gain, inside the clamp for every activation here
                torch.testing.assert_close(got.dx[at0], dy[at0] * cfg.gain * first, **tol)
            if act in ('elu', 'selu'):
                assert not bool(got.d_x[at0].any())
            if cfg.clamp is not None and act != 'linear':
                edge = got.yu.abs() == cfg.clamp
                assert not bool(got.dx[edge].any()) and not bool(got.d_dy[edge].any()) and not bool(got.d_x[edge].any())
                if act in bc.EXACT_POSITIVE_SIDE:
                    assert bool(edge.any()) and bool((dx[edge & (u > 0)] != 0).all()), 'autograd passes the gradient at the ends of the clamp'


@pytest.mark.parametrize('dtype', [torch.float32, torch.float16, torch.bfloat16, torch.float64])
def test_inputs_hold_the_branch_points_in_every_storage_type(dtype):
    for layout in bc.LAYOUTS:
        for cfg in bc.CONFIGS:
            x, b, dy, ddx = bc.inputs(layout, dtype, cfg)
            assert x.dtype == dy.dtype == ddx.dtype == dtype and x.is_contiguous()
            u = x.double() if b is None else x.double() + bc._bias_view(b.double(), x.shape, layout.dim)
            if b is not None:
                assert b.dtype == dtype and bool((b.double() * 4 == (b.double() * 4).round()).all()) and float(b.abs().max()) <= 4
            assert bool((u == 0).any())
            assert bool((u > 80).any()) and bool((u < -80).any()) and bool(((u > 40) & (u < 80)).any()) and bool(((u < -40) & (u > -80)).any())
            assert bool((u == 21).any()) and bool((u == 20.5).any())
            if cfg.clamp is not None:
                assert bool((u * cfg.gain == bc.CLAMP).any()) and bool((u * cfg.gain == -bc.CLAMP).any())


def test_layouts_reach_the_paths_they_name():
    L = bc.LAYOUT_BY_NAME
    numel = lambda s: torch.Size(s).numel()
    assert numel(L['nchw_tail'].shape) % 4 == 3 and numel(L['nchw_tail'].shape) % 8 == 3 and (17 * 13) % 4 != 0
    assert L['nchw_step5'].shape[2] * L['nchw_step5'].shape[3] == 5
    assert L['fc'].shape == (5, 33) and len(L['fc'].shape) == 2
    x = torch.empty(L['channels_last'].shape).contiguous(memory_format=torch.channels_last)
    assert x.stride(1) == 1
    assert torch.empty(L['dim0'].shape).stride(0) == 90 and torch.empty(L['dim2'].shape).stride(2) == 5
    assert numel(bc.BIG.shape) // 4 > 2048 * 256 and numel(bc.BIG.shape) % 4 == 1
    v, buf = bc.offset_view(torch.arange(24.0).reshape(2, 3, 4))
    assert v.data_ptr() % 16 == 4 and v.is_contiguous() and torch.equal(v, torch.arange(24.0).reshape(2, 3, 4))
    assert float(buf[0]) == 1234.5 and bool((buf[25:] == 1234.5).all())


@pytest.mark.parametrize('act', bc.ACTS)
def test_decimal_reference_is_the_closed_form(act):
    """The 40-digit evaluation (the reference of the float64 launches) and the float64 closed forms are one set of expressions: they agree to a
    few float64 ulp of the largest magnitude, with and without the clamp, on the layout with the bias along the rows."""
    layout = bc.LAYOUT_BY_NAME['dim2']
    for cfg in bc.configs(act):
        x, b, dy, ddx = bc.inputs(layout, torch.float64, cfg)
        want, free = bc.closed_form_exact(x, b, layout.dim, act, cfg, dy, ddx)
        for exact, cf in ((want, cfg), (free, cfg._replace(clamp=None))):
            f64 = bc.closed_form(x, b, layout.dim, act, cf, dy, ddx)
            for name in ('y', 'dx', 'db', 'd_dy', 'd_x', 'yu'):
                a, e = getattr(f64, name), getattr(exact, name)
                assert float((a - e).abs().max()) <= 1e-14 * max(float(e.abs().max()), 1e-300) or not bool(e.any()), (cfg, name)
        assert torch.equal(want.yu.abs() < bc.CLAMP, bc.closed_form(x, b, layout.dim, act, cfg, dy, ddx).yu.abs() < bc.CLAMP)
