"""Every launchable form of csrc/upfirdn2d.hip at its edges against the float64 oracle, on the case table of tests/upfirdn2d_cases.py
(which tests/test_upfirdn2d_cases_cpu.py proves to reach every form, tile instance, staging path and both sides of every dispatch
condition).  Needs a real MI355X: `pytest -m gpu`.

Every case runs through the public call (`Upfirdn2dPlugin.upfirdn2d_ex`), takes the form the table states (`upfirdn2d_plan` on the
tensors actually passed), and every output element is compared with the float64 oracle under a bound derived here, not a flat tolerance.

The bound (u = 2^-24: the accumulation is float for fp32, fp16 and bf16 storage; 2^-53 for float64).
  Plain FIR.  An output is gain * sum of at most T = ceil(f_h / up_y) * ceil(f_w / up_x) products x * g.  To first order the computed value
  carries one rounding of f * gain (tile and lean kernels) or of the final * gain (generic, cell), one per product and T - 1 additions, each
  relative to a partial sum that is at most A = |gain| * upfirdn(|x|, |f|) (the same oracle on absolute values):
      |y - ref| <= (T + 3) * u * A            (T + 1 first-order terms; the other two cover the second order.  Fused multiply-adds only lower it.)
  Fused epilogue  y = act_gain * lrelu(FIR + add + noise * strength + bias), clamped.  Every further operation rounds once, relative to a
  value that is at most the sum of the absolute operands, so A grows by |add| + |noise * strength| + |bias| and the count by
      1 (+ add)   2 (noise * strength, + noise)   1 (+ bias)   1 (* alpha, lrelu only)   1 (* act_gain);
  the error before the activation passes through a slope of at most max(1, |alpha|) (a value that changes sign under the error is itself
  smaller than the error on both sides of zero, so the wrong branch costs no more) and through |act_gain|; the clamp only contracts:
      |y - ref| <= (T + 3 + roundings) * u * A * |act_gain| * max(1, |alpha|)
  The reference takes alpha, act_gain, clamp and noise_strength as the float32 numbers the ABI carries.
  fp16 / bf16 storage.  Operands are the stored values; the one rounding of the output adds 2^-11 |ref| (2^-8 |ref| for bf16) and rounds the
  error above with it (a factor 1 + 2^-11), plus half a subnormal step, 2^-25, for fp16.
  The separable call (torch_utils.ops.upfirdn2d with a 1-D filter) is two passes.  The first pass leaves an error of at most
  (T1 + 3) u A1 in the intermediate, which is stored in the accumulation type (fp32: its storage adds no rounding), the second pass maps
  it linearly through |f| and |gain| and adds (T2 + 3) u times its own absolute sum, which is at most A2 = |gain| upfirdn(|x|, |f| x |f|) (1 + (T1 + 3) u):
      |y - ref| <= (T1 + 3 + (T2 + 3) (1 + (T1 + 3) u)) * u * A2
  The backward pass is the adjoint call on dy (factors exchanged, filter mirrored): the plain bound with the adjoint's T and A.

The worst error / bound per form and storage type is in DESIGN.md (section on this suite); `test_worst_ratios` prints the table of a run."""
import os

import pytest
import torch

import upfirdn2d_cases as uc
from oracle import ops as oracle_ops

pytestmark = pytest.mark.gpu

WORST = {}          # (form, instance or U, dtype) -> worst error / bound seen in this process


def _hp():
    from torch_utils import hip_plugin
    return hip_plugin


@pytest.fixture(autouse=True)
def _native_calls():
    _hp().CALLS.clear()
    yield


class knob:
    """IDE3D_FIR_NO_LEAN / IDE3D_FIR_NO_CELL for the calls inside (the library reads them per call)."""
    def __init__(self, name):
        self.name = name

    def __enter__(self):
        os.environ[self.name] = '1'

    def __exit__(self, *a):
        os.environ.pop(self.name, None)


def _plan(case, ts):
    p = _hp().upfirdn2d_plan(ts['x'], ts['f'], *case.call_args(), **case.plan_kwargs(ts))
    return dict(form=p['form'], instance=p['instance'], staging=p['staging'], cell_u=p['cell_u'], c_fastest=p['c_fastest'], tiles=(p['tiles_x'], p['tiles_y']))


def _run(case, dev, ts=None, amax_init=None):
    """-> (y, per-image maximum read back from the y_amax rows or None, the operands)."""
    hp = _hp()
    ts = ts or case.tensors(dev)
    am = None
    if case.epi.get('amax'):
        am = torch.zeros(case.shape[0], hp.AMAX_FLOATS, device=dev)
        if amax_init is not None:
            am[:, 5 * hp.AMAX_STRIDE] = amax_init.to(dev)
    y = hp.Upfirdn2dPlugin.upfirdn2d_ex(ts['x'], ts['f'], *case.call_args(), **case.epilogue_kwargs(ts, am))
    return y, (None if am is None else am.amax(dim=1)), ts


def _key(case):
    return (case.form, case.instance or case.cell_u or '', case.dtype)


@pytest.mark.parametrize('case', uc.CASES, ids=[c.name for c in uc.CASES])
def test_case_against_float64(gpu_device, case):
    y, am, ts = _run(case, gpu_device)
    assert _plan(case, ts) == case.stated_plan(), case.why
    assert _hp().CALLS.get('upfirdn2d') == 1
    assert y.dtype == case.torch_dtype and tuple(y.shape) == case.out_shape
    assert y.is_contiguous(memory_format=torch.channels_last if case.layout == ('cl',) and case.shape[1] > 1 else torch.contiguous_format)
    ratio = uc.worst_ratio(y, case)
    WORST[_key(case)] = max(WORST.get(_key(case), 0.0), ratio)
    print(f'{case.name}: {case.form} {case.instance or case.cell_u or ""} {case.dtype} worst error / bound {ratio:.3f}')
    assert ratio <= 1.0, f'{case.name}: error / bound {ratio:.3f} ({case.why})'
    if am is not None:          # max |y| per image, exactly
        assert torch.equal(am, y.abs().amax(dim=(1, 2, 3))), case.name


def test_worst_ratios(gpu_device):
    """The table DESIGN.md quotes (run after the cases; every entry was already asserted <= 1 there)."""
    for k in sorted(WORST, key=str):
        print('worst error / bound', k, f'{WORST[k]:.3f}')
    assert all(v <= 1.0 for v in WORST.values())


@pytest.mark.parametrize('case', uc.LEAN_CASES, ids=[c.name for c in uc.LEAN_CASES])
def test_lean_kernels_equal_the_tile_kernels_bit_for_bit(gpu_device, case):
    y, am, ts = _run(case, gpu_device)
    with knob('IDE3D_FIR_NO_LEAN'):
        p = _plan(case, ts)
        assert p['form'] == 'tile' and p['instance'] == case.instance and p['tiles'] == case.tiles
        y_tile, am_tile, _ = _run(case, gpu_device, ts)
    assert _plan(case, ts)['form'] == case.form
    assert torch.equal(y, y_tile), case.name
    if am is not None:
        assert torch.equal(am, am_tile) and torch.equal(am, y.abs().amax(dim=(1, 2, 3)))


@pytest.mark.parametrize('case', uc.CELL_CASES, ids=[c.name for c in uc.CELL_CASES])
def test_cell_kernel_equals_the_generic_kernel_bit_for_bit(gpu_device, case):
    y, _, ts = _run(case, gpu_device)
    with knob('IDE3D_FIR_NO_CELL'):
        assert _plan(case, ts)['form'] == 'generic'
        y_gen, _, _ = _run(case, gpu_device, ts)
    assert bool(torch.isfinite(y).all()) and torch.equal(y, y_gen), case.name


@pytest.mark.parametrize('a,b', uc.TWINS, ids=[f'{a.name}-{b.name}' for a, b in uc.TWINS])
def test_16_byte_and_scalar_staging_agree_bit_for_bit(gpu_device, a, b):
    ya, _, tsa = _run(a, gpu_device)
    yb, _, tsb = _run(b, gpu_device)
    assert {_plan(a, tsa)['staging'], _plan(b, tsb)['staging']} == {0, 1} and torch.equal(tsa['x'], tsb['x'])
    assert torch.equal(ya, yb), (a.name, b.name)


@pytest.mark.parametrize('case', uc.AMAX_CASES, ids=[c.name for c in uc.AMAX_CASES])
def test_y_amax_keeps_a_value_above_the_true_maximum(gpu_device, case):
    y, am, _ = _run(case, gpu_device)
    true = y.abs().amax(dim=(1, 2, 3))
    assert torch.equal(am, true)
    init = torch.zeros(case.shape[0])
    init[-1] = float(true[-1]) * 2 + 1          # one image's row raised beforehand: it stays; the other rows are found as before
    y2, am2, _ = _run(case, gpu_device, amax_init=init)
    want = true.clone()
    want[-1] = init[-1]
    assert torch.equal(y2, y) and torch.equal(am2, want), case.name


NONFINITE = ('t64_w63_h33', 't128_w65_h33', 't128_w129_h32', 'tup2_inw65', 'tup2_odd_pads', 'dn2_two_tiles', 'dn2_two_tiles_padded', 'f44_w132_h33', 'f44_crop', 'up2_wide_p1', 'up2_wide_p3',
             'x_up_large', 'x_dn_large_other', 'x_1_large', 'y_up_large', 'y_dn_large', 'y_1_large_other', 'gen_up23', 'gen_5x5', 'gen_cl_c2', 'gen_3x7', 'gen_f64',
             'cell_12_u2', 'cell_8x16_u4', 'cell_9x7_u2', 'cell_cl')


@pytest.mark.parametrize('name', NONFINITE)
def test_one_nan_and_one_inf_sample_stay_inside_their_footprint(gpu_device, name):
    """No filter of these cases has a zero tap: the outputs a sample reaches are exactly those of its footprint.  Outside it the result is
    bit-equal to the run with the sample set to 0.  The cell kernel adds x * 0 for the padding taps of its whole-block filter copy, so a
    non-finite sample reaches every output of the cells that READ it (input rows q_y .. q_y + nty, columns q_x .. q_x + round_up(ntx + 1, 8) - 1):
    there bit-equality is asserted for the other cells only (the accepted difference from the generic kernel)."""
    case = uc.BY_NAME[name].replace(epi=None)
    f = case.filter()
    assert bool((f != 0).all())
    n, c, h, w = case.shape
    spots = ((n - 1, c - 1, h // 3, w // 4, float('nan')), (0, 0, h - 1 - h // 5, w - 1, float('inf')))
    x0, hit = case.values('x'), torch.zeros(case.shape, dtype=torch.float64)
    x_bad = x0.clone()
    for i, j, sy, sx, v in spots:
        x0[i, j, sy, sx], x_bad[i, j, sy, sx], hit[i, j, sy, sx] = 0, v, 1
    kw = dict(up=case.up, down=case.down, padding=list(case.pad), flip_filter=case.flip)
    foot = oracle_ops.upfirdn2d(hit, f.abs(), **kw) > 0
    assert bool(foot.any()) and not bool(foot.all())
    hp = _hp()
    ys = []
    for xv in (x0, x_bad):
        x = uc.strided(xv, case.layout, gpu_device)
        assert _plan(case, dict(x=x, f=f, add=None, noise=None, bias=None)) == case.stated_plan()
        ys.append(hp.Upfirdn2dPlugin.upfirdn2d_ex(x, f.to(gpu_device), *case.call_args()).cpu())
    y0, y1 = ys
    assert bool(torch.isfinite(y0).all())
    assert not bool(torch.isfinite(y1[foot]).any()), f'{name}: a finite output inside the footprint'
    same = ~foot
    if case.form == 'cell':
        u = case.cell_u
        ntx, nty = -(-f.shape[1] // u), -(-f.shape[0] // u)
        reach = 8 * ((ntx + 1 + 7) // 8)
        oy, ox = torch.arange(case.out_shape[2])[:, None], torch.arange(case.out_shape[3])[None, :]
        qy, qx = torch.div(oy - case.pad[2], u, rounding_mode='floor'), torch.div(ox - case.pad[0], u, rounding_mode='floor')
        for i, j, sy, sx, _ in spots:
            reads = (qy <= sy) & (sy <= qy + nty) & (qx <= sx) & (sx <= qx + reach - 1)
            assert bool((foot[i, j] <= reads).all())
            same[i, j] &= ~reads
        assert bool(same.any())
    assert torch.equal(y0[same], y1[same]), f'{name}: an output outside the footprint changed'


# ---- backward ---------------------------------------------------------------------------------------------------------------------------

BACKWARD = (
    # forward shape, forward kwargs, the form and instance of the adjoint call
    ((1, 2, 9, 72), dict(up=1, padding=[2, 1, 2, 1], gain=4), 'fir44', uc.T128),
    ((1, 2, 16, 72), dict(down=2, padding=[1, 1, 1, 1]), 'fir_up2', uc.TUP2),
    ((2, 3, 17, 130), dict(up=2, padding=[2, 1, 2, 1], gain=4), 'tile', uc.TDN2),
    ((2, 3, 9, 11), dict(up=(2, 3), padding=[2, 1, 3, 2], gain=4), 'generic', None),          # (gains are powers of two: the definition's float32 f * gain is exact)
    ((1, 2, 33, 67), dict(up=1, padding=[1, 1, 1, 1], gain=4), 'tile', uc.T128),
)


@pytest.mark.parametrize('shape,kw,form,instance', BACKWARD, ids=[f'adjoint_{b[2]}_{i}' for i, b in enumerate(BACKWARD)])
def test_backward_against_float64_autograd(gpu_device, shape, kw, form, instance):
    from torch_utils.ops import upfirdn2d as up
    hp = _hp()
    g = torch.Generator().manual_seed(91)
    x, f = torch.randn(*shape, generator=g), uc.A44
    xd = x.to(gpu_device).requires_grad_(True)
    y = up.upfirdn2d(xd, f.to(gpu_device), **kw)
    dy = torch.sin(torch.arange(y.numel(), dtype=torch.float32) * 0.37).reshape(y.shape)
    gx = torch.autograd.grad((y * dy.to(gpu_device)).sum(), xd)[0]
    assert hp.CALLS.get('upfirdn2d') == 2
    x64 = x.double().requires_grad_(True)
    want = torch.autograd.grad((up._upfirdn2d_ref(x64, f, **kw) * dy.double()).sum(), x64)[0]
    # the adjoint call, as _Upfirdn2dHip.backward forms it
    ux, uy = up._parse_scaling(kw.get('up', 1))
    dx, dy_ = up._parse_scaling(kw.get('down', 1))
    px0, px1, py0, py1 = kw['padding']
    back = dict(up=(dx, dy_), down=(ux, uy), flip_filter=True, gain=kw.get('gain', 1),
                padding=[4 - px0 - 1, shape[3] * ux - y.shape[3] * dx + px0 - ux + 1, 4 - py0 - 1, shape[2] * uy - y.shape[2] * dy_ + py0 - uy + 1])
    p = hp.upfirdn2d_plan(dy, f, dx, dy_, ux, uy, *back['padding'], True, back['gain'])
    assert (p['form'], p['instance']) == (form, instance)
    t = -(-4 // dx) * -(-4 // dy_) + 3
    bound = t * 2.0 ** -24 * oracle_ops.upfirdn2d(dy.double().abs(), f.abs(), **back)
    assert tuple(bound.shape) == shape
    ratio = float(((gx.cpu().double() - want).abs() / bound.clamp_min(1e-300)).max())
    print(f'backward planned as {form} {instance}: worst error / bound {ratio:.3f}')
    assert ratio <= 1.0


# ---- the separable call -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('kw,first,second', [
    (dict(up=2, padding=[6, 5, 6, 5], gain=4), uc.X_UP, uc.Y_UP),
    (dict(down=2, padding=[-1, -1, -1, -1], flip_filter=True), uc.X_DN, uc.Y_DN),
    (dict(padding=[6, 5, 6, 5]), uc.X_1, uc.Y_1)], ids=['up2', 'down2', 'unit'])
def test_separable_12_tap_call_end_to_end(gpu_device, kw, first, second):
    from torch_utils.ops import upfirdn2d as up
    hp = _hp()
    g = torch.Generator().manual_seed(17)
    x, f = torch.randn(2, 3, 41, 70, generator=g), uc.A12
    y = up.upfirdn2d(x.to(gpu_device), f.to(gpu_device), **kw)
    assert hp.CALLS.get('upfirdn2d') == 2
    u, d = kw.get('up', 1), kw.get('down', 1)
    px0, px1, py0, py1 = kw['padding']
    flip = kw.get('flip_filter', False)
    p1 = hp.upfirdn2d_plan(x, (1, 12), u, 1, d, 1, px0, px1, 0, 0, flip, 1.0)
    mid = (2, 3, 41, (70 * u + px0 + px1 - 12 + d) // d)
    p2 = hp.upfirdn2d_plan(dict(shape=mid, stride=(3 * 41 * mid[3], 41 * mid[3], mid[3], 1), dtype=torch.float32), (12, 1), 1, u, 1, d, 0, 0, py0, py1, flip, kw.get('gain', 1))
    assert (p1['form'], p1['instance'], p2['form'], p2['instance']) == ('tile', first, 'tile', second)
    ref = oracle_ops.upfirdn2d(x.double(), f, up=u, down=d, padding=kw['padding'], flip_filter=flip, gain=kw.get('gain', 1))
    a2 = oracle_ops.upfirdn2d(x.double().abs(), f.abs(), up=u, down=d, padding=kw['padding'], flip_filter=flip, gain=kw.get('gain', 1))
    eps = 2.0 ** -24
    t1 = t2 = -(-12 // u) + 3
    bound = (t1 + t2 * (1 + t1 * eps)) * eps * a2
    assert tuple(y.shape) == tuple(ref.shape)
    ratio = float(((y.cpu().double() - ref).abs() / bound.clamp_min(1e-300)).max())
    print(f'separable {kw}: worst error / bound {ratio:.3f}')
    assert ratio <= 1.0


def test_the_launch_refuses_what_the_plan_refuses(gpu_device):
    hp = _hp()
    x, f = torch.zeros(1, 2, 5, 6, device=gpu_device), uc.A44.to(gpu_device)
    for kw in (dict(act=2), dict(act=9)):
        with pytest.raises(RuntimeError):
            hp.Upfirdn2dPlugin.upfirdn2d_ex(x, f, 1, 1, 1, 1, 1, 1, 1, 1, False, 1.0, **kw)
        with pytest.raises(RuntimeError):
            hp.upfirdn2d_plan(x, f, 1, 1, 1, 1, 1, 1, 1, 1, False, 1.0, **kw)
    for args in ((0, 1, 1, 1, 1, 1, 1, 1), (1, 1, 1, 0, 1, 1, 1, 1), (1, 1, 1, 1, -9, 1, 1, 1)):
        with pytest.raises(RuntimeError):
            hp.Upfirdn2dPlugin.upfirdn2d_ex(x, f, *args, False, 1.0)
        with pytest.raises(RuntimeError):
            hp.upfirdn2d_plan(x, f, *args, False, 1.0)
    assert not hp.CALLS
