"""csrc/filtered_lrelu.hip across output tiles, dtypes and sign modes against the float64 definition (`oracle.ops.filtered_lrelu`), DESIGN.md
section 5.21.  Needs a real MI355X: `pytest -m gpu`.  Cases and closed forms: tests/filtered_lrelu_cases.py (held to the kernel source by
tests/test_filtered_lrelu_cases_cpu.py).

Bounds, with scale = max |want|:
  fp32          |got - want| <= 1e-5 scale                        (the suite's bound for FIR sums, tests/test_gpu_ops.py)
  fp16 / bf16   |got - want| <= u |want| + 1e-5 scale, u = 2^-11 / 2^-8: fp32 arithmetic, one rounding to nearest at the store (common.h `Elem<T>::st`)
  float64       1e-12 scale (generic path: upfirdn2d and the activation kernel in float64)
Sign bytes are byte output and compared bit for bit on data for which the classified value is exact.  Every test prints its measured maximum as
a multiple of its bound.
"""

import warnings

import numpy as np
import pytest
import torch

import filtered_lrelu_cases as C
from oracle import ops as oracle_ops

pytestmark = pytest.mark.gpu

F32, F16, BF16 = torch.float32, torch.float16, torch.bfloat16
ULP = {F32: 0.0, F16: 2.0 ** -11, BF16: 2.0 ** -8}
NAME = {F32: 'fp32', F16: 'fp16', BF16: 'bf16', torch.float64: 'fp64'}
INF = float('inf')


@pytest.fixture(autouse=True)
def _native_calls():
    from torch_utils import hip_plugin
    hip_plugin.CALLS.clear()
    yield hip_plugin.CALLS


def _calls(name):
    from torch_utils import hip_plugin
    return hip_plugin.CALLS.get(name, 0)


def _held(got, want, dtype, what, rel=1e-5):
    """Asserts the bound of the module docstring and prints the measured maximum as a multiple of it."""
    got, want = got.detach().cpu().double(), want.double()
    assert got.shape == want.shape, f'{what}: shape {tuple(got.shape)} != {tuple(want.shape)}'
    scale = float(want.abs().max())
    assert scale > 0, what
    ratio = ((got - want).abs() / (ULP.get(dtype, 0.0) * want.abs() + rel * scale))
    worst = float(ratio.max())
    print(f'[filtered_lrelu] {what} [{NAME[dtype]}]: {worst:.4f} of the bound')
    assert worst <= 1.0, f'{what} [{NAME[dtype]}]: {worst:.3f} of the bound at {np.unravel_index(int(ratio.argmax()), ratio.shape)}'
    return worst


def _filters(case, dev, dyadic=False):
    fu, fd = C.make_filter(case['fu'], dyadic), C.make_filter(case['fd'], dyadic)
    return (None if fu is None else fu.to(dev)), (None if fd is None else fd.to(dev))


def _op(case, x, b, flip, dev, dyadic=False):
    from torch_utils.ops import filtered_lrelu
    fu, fd = _filters(case, dev, dyadic)
    return filtered_lrelu.filtered_lrelu(x, fu=fu, fd=fd, b=b, up=case['up'], down=case['down'], padding=case['pad'], gain=case['gain'],
                                         slope=case['slope'], clamp=case['clamp'], flip_filter=flip)


def _raw(case, x, b, signs, sx, sy, flip, write, dev, dyadic=True):
    """hip_plugin.FilteredLReluPlugin.filtered_lrelu; an absent filter is one separable tap, as the op hands it over."""
    from torch_utils import hip_plugin
    fu, fd = _filters(case, dev, dyadic)
    one = torch.ones([1], device=dev)
    clamp = INF if case['clamp'] is None else case['clamp']
    return hip_plugin.FilteredLReluPlugin.filtered_lrelu(x, one if fu is None else fu, one if fd is None else fd, b, signs, case['up'], case['down'], *case['pad'],
                                                         sx, sy, case['gain'], case['slope'], clamp, flip, write)


# ---- 1. values at tile edges, every instance and dtype -----------------------------------------------------------------------------------

_INPUTS, _WANT = {}, {}


def _inputs(case, dtype):
    """x ~ N(0, 1), b of order 1, rounded to the storage type (computed once per case and dtype)."""
    key = (case['name'], dtype)
    if key not in _INPUTS:
        g = torch.Generator().manual_seed(1000 + [c['name'] for c in C.VALUE_CASES].index(case['name']))
        x = torch.randn(*case['shape'], generator=g).to(dtype)
        b = (torch.randn(case['shape'][1], generator=g) * 1.2).to(dtype)
        _INPUTS[key] = (x, b)
    return _INPUTS[key]


def _want(case, dtype, flip):
    key = (case['name'], dtype, flip)
    if key not in _WANT:
        x, b = _inputs(case, dtype)
        _WANT[key] = C.forward64(case, x, b, flip)[0]
    return _WANT[key]


def _rounded_once(y, y32, exact, what):
    """The narrow launch is the fp32 launch of the same kernel rounded once to nearest.  Generic kernel: bit for bit.  Specialised kernel in fp16:
    the compiler folds the last multiply-add of the vertical down pass into the conversion (v_fma_mixlo_f16: the exact a * b + c rounded ONCE to
    fp16, where the fp32 launch rounds it to fp32 first), so an element may differ from the rounded fp32 result, but only where the fp32 result e32
    lies within half an fp32 ulp of the midpoint of the two fp16 candidates: |e - e32| <= ulp32 / 2 for the exact e, and the midpoint lies between
    e and e32 when they round to different sides."""
    r = y32.to(y.dtype)
    if exact:
        assert torch.equal(y, r), f'{what}: the narrow launch is not the rounded fp32 launch'
        return
    differ = (y != r).cpu().numpy()
    mid = (y.cpu().double().numpy() + r.cpu().double().numpy()) / 2
    e32 = y32.cpu().numpy()
    ok = np.abs(e32.astype(np.float64) - mid) <= np.spacing(np.abs(e32)).astype(np.float64) / 2
    print(f'[filtered_lrelu] {what}: {int(differ.sum())} of {differ.size} elements rounded from the unrounded last multiply-add')
    assert not (differ & ~ok).any(), f'{what}: {int((differ & ~ok).sum())} elements are not the fp32 result rounded once'
    # (such an element needs the fp32 value within 2^-14 of the fp16 spacing of a midpoint, on either side: about 2^-13 of the elements; 8 x that + 4)
    assert differ.sum() <= 4 + differ.size * 2.0 ** -10, f'{what}: {int(differ.sum())} of {differ.size} elements differ'


_VALUE_PARAMS = [(c, dt) for c in C.VALUE_CASES for dt in (F32, F16) + ((BF16,) if c['bf16'] else ())]


@pytest.mark.parametrize('case,dtype', _VALUE_PARAMS, ids=[f"{c['name']}-{NAME[dt]}" for c, dt in _VALUE_PARAMS])
def test_values_against_float64(gpu_device, case, dtype):
    """Every instance of the specialised kernel on 2 x 2 tiles with partial last tiles, the generic kernel past its largest tile; both filter
    orientations; fp16 on every case, bf16 on every generic case and on three instance tuples (where it takes the generic kernel).  A narrow launch
    equals the fp32 launch of the same kernel family on the widened inputs, rounded once (`_rounded_once`)."""
    x, b = _inputs(case, dtype)
    same_family = dtype == F16 or (dtype == BF16 and C.instance_of(case) not in C.source_instances())
    assert bool((x.float().abs().max() > 2) and (b.float().abs().max() > 0.3))
    for flip in (False, True):
        y = _op(case, x.to(gpu_device), b.to(gpu_device), flip, gpu_device)
        assert y.dtype == dtype and tuple(y.shape) == (*case['shape'][:2], *C.out_hw(case)) and y.is_contiguous()
        _held(y, _want(case, dtype, flip), dtype, f"y {case['name']} flip={flip}")
        if same_family:
            y32 = _op(case, x.float().to(gpu_device), b.float().to(gpu_device), flip, gpu_device)
            _rounded_once(y, y32, exact=C.instance_of(case) not in C.source_instances(), what=f"{case['name']} flip={flip} {NAME[dtype]}")
    assert _calls('filtered_lrelu') == (4 if same_family else 2) and _calls('filtered_lrelu_act_') == 0
    # the two orientations of an asymmetric filter must differ, or the flag was not tested
    if case['fu'] is not None or case['fd'] is not None:
        a, bb = _want(case, dtype, False), _want(case, dtype, True)
        assert float((a - bb).abs().max()) > 1e-3 * float(a.abs().max())


@pytest.mark.parametrize('dtype', [F32, F16], ids=['fp32', 'fp16'])
@pytest.mark.parametrize('name', ['A0', 'G0'])
def test_layouts_equal_the_dense_call(gpu_device, name, dtype):
    """channels_last (the result is channels_last too), a W-offset view and an H-strided view, each inside a NaN-filled storage: bit-equal to the
    dense call, i.e. every read goes through the strides and none leaves the view."""
    case = next(c for c in C.VALUE_CASES if c['name'] == name)
    x, b = _inputs(case, dtype)
    x, b = x.to(gpu_device), b.to(gpu_device)
    n, c, h, w = x.shape
    nan = lambda *shape: torch.full(shape, float('nan'), dtype=dtype, device=gpu_device)
    for flip in (False, True):
        dense = _op(case, x, b, flip, gpu_device)
        assert not bool(torch.isnan(dense).any())
        with warnings.catch_warnings():
            warnings.simplefilter('ignore', RuntimeWarning)          # (the op warns about channels_last input, as the reference does)
            y = _op(case, x.contiguous(memory_format=torch.channels_last), b, flip, gpu_device)
        assert y.is_contiguous(memory_format=torch.channels_last) and not y.is_contiguous()
        assert torch.equal(y, dense), f'{name} channels_last flip={flip}'
        base = nan(n, c, h, w + 3)
        base[..., 3:] = x
        view = base[..., 3:]
        assert view.stride(2) == w + 3 and view.storage_offset() == 3
        assert torch.equal(_op(case, view, b, flip, gpu_device), dense), f'{name} W-offset view flip={flip}'
        base = nan(n, c, 2 * h, w)
        base[:, :, ::2] = x
        view = base[:, :, ::2]
        assert view.stride(2) == 2 * w
        assert torch.equal(_op(case, view, b, flip, gpu_device), dense), f'{name} H-strided view flip={flip}'


# ---- 2. the sign tensor is byte output ------------------------------------------------------------------------------------------------------

_SIGN_REF = {}
# cases whose dyadic data (by the oracle alone) contain exact zeros AND values exactly at the clamp in both filter orientations
_EDGE_VALUES = {'S-A0', 'S-A2', 'S-A3', 'S-A5', 'S-A7', 'S-G0'}


def _sign_ref(case, flip):
    """Dyadic inputs, the oracle's (y, codes) and the exactness / frequency checks, on the CPU and before any launch (once per case and flip)."""
    key = (case['name'], flip)
    if key not in _SIGN_REF:
        x, b = C.dyadic_inputs(case, 100)
        y64, codes = C.forward64(case, x, b, flip)
        z = C.intermediate64(case, x, b, flip).numpy()
        zi = z * 2.0 ** 20
        assert np.array_equal(zi, np.rint(zi)), 'the classified value must be a multiple of 2^-20'
        m = np.abs(zi).astype(np.int64)
        m = m[m > 0]
        m = m // (m & -m)
        assert int(m.max()) < 2 ** 23, 'the classified value must need fewer than 24 significant bits'          # (every partial sum of its terms too: same grid, smaller)
        act = np.where(z < 0, z * case['slope'], z)
        freq = [float((codes.numpy() == k).mean()) for k in range(3)]
        assert freq[0] >= 0.05 and freq[1] >= 0.05 and (case['clamp'] is None or freq[2] >= 0.05), f"degenerate data for {case['name']}: code frequencies {freq}"
        assert np.array_equal(codes.numpy()[z == 0], np.zeros(int((z == 0).sum()), dtype=np.uint8))          # exact zeros are code 0 ...
        if case['clamp'] is not None:
            assert not (codes.numpy()[np.abs(act) == case['clamp']] == 2).any()                                  # ... values exactly at the clamp are not clamped
        if case['name'] in _EDGE_VALUES:
            assert (z == 0).any() and (np.abs(act) == case['clamp']).any(), case['name']
        _SIGN_REF[key] = (x, b, y64, codes)
    return _SIGN_REF[key]


def _valid_bytes_equal(so, want_packed, sw_active, what):
    full = sw_active // 4
    bad = int((so[..., :full] != want_packed[..., :full]).sum())
    assert bad == 0, f'{what}: {bad} sign bytes differ'
    if sw_active % 4:          # the last, partly valid byte of a row: its valid 2-bit fields only
        mask = np.uint8((1 << (2 * (sw_active % 4))) - 1)
        bad = int(((so[..., full] & mask) != (want_packed[..., full] & mask)).sum())
        assert bad == 0, f'{what}: {bad} partly valid sign bytes differ'


@pytest.mark.parametrize('case', C.SIGN_CASES, ids=[c['name'] for c in C.SIGN_CASES])
def test_sign_bytes_exact_across_tiles_and_dtypes(gpu_device, case):
    """Sign-write launches of every instance (+ two generic configurations) over 2 x 2 tiles: every valid 2-bit field equals the oracle's code,
    the tensor has the reference's shape, and the fp16 / bf16 launches write the bytes of the fp32 launch."""
    sh, sw_active, row_bytes = C.sign_hw(case)
    assert sh > 32 * case['down'] and sw_active > 32 * case['down']          # bytes from a second tile row and column
    for flip in (False, True):
        x, b, y64, codes = _sign_ref(case, flip)
        want_packed = C.pack_codes(codes[:, :, :sh, :sw_active], row_bytes)
        first = None
        for dtype in (F32, F16, BF16):
            assert torch.equal(x.to(dtype).float(), x) and torch.equal(b.to(dtype).float(), b)
            y, so, rc = _raw(case, x.to(dtype).to(gpu_device), b.to(dtype).to(gpu_device), torch.empty([0]), 0, 0, flip, True, gpu_device)
            assert rc == 0
            assert so.dtype == torch.uint8 and tuple(so.shape) == (*case['shape'][:2], sh, row_bytes) and (row_bytes * 4) % 16 == 0
            so = so.cpu().numpy()
            what = f"{case['name']} flip={flip} {NAME[dtype]}"
            _valid_bytes_equal(so, want_packed, sw_active, what)
            written = (sw_active + 3) // 4
            if first is None:
                first = so
            else:
                assert np.array_equal(so[..., :written], first[..., :written]), f'{what}: bytes differ from the fp32 launch'
            _held(y, y64, dtype, 'y with sign write ' + what)
            if case['name'] == 'S-G0' and dtype == F32:          # 4x4 filters: the down-sampled sums are exact as well
                assert torch.equal(y.cpu(), y64.float()), what
    assert _calls('filtered_lrelu') == 6


# ---- 3. sign-read mode and autograd over several tiles ------------------------------------------------------------------------------------------

@pytest.mark.parametrize('case', C.SIGN_CASES, ids=[c['name'] for c in C.SIGN_CASES])
def test_backward_reads_the_signs_across_tiles(gpu_device, case):
    """dx, db through `filtered_lrelu.filtered_lrelu` == the float64 closed form on the oracle's codes (tests/filtered_lrelu_cases.py `backward64`,
    itself == autograd through the definition on the CPU): one launch forward (sign write), one backward (filters swapped, sign read at the
    offset px0 - (fu_w - 1), on a sign tensor narrower than the region read)."""
    for flip in (False, True):
        x, b, y64, codes = _sign_ref(case, flip)
        xd, bd = x.to(gpu_device).requires_grad_(True), b.to(gpu_device).requires_grad_(True)
        before = _calls('filtered_lrelu')
        y = _op(case, xd, bd, flip, gpu_device, dyadic=True)
        dy = C.dyadic_grad(y.shape, 200 + flip)
        dx, db = torch.autograd.grad(y, [xd, bd], dy.to(gpu_device))
        assert _calls('filtered_lrelu') == before + 2 and _calls('filtered_lrelu_act_') == 0
        want = C.backward64(case, codes, dy, flip)
        what = f"{case['name']} flip={flip}"
        _held(y, y64, F32, 'y ' + what)
        _held(dx, want, F32, 'dx ' + what)
        _held(db, want.sum([0, 2, 3]), F32, 'db ' + what)
        if case['name'] == 'S-G0':          # every intermediate exact
            assert torch.equal(dx.cpu(), want.float()), what


def test_second_order_runs_sign_read_at_the_forwards_offsets(gpu_device):
    """d/d(dy) of <dx, w> is the op applied to w with the stored codes in place of the activation (the transpose of the backward pass)."""
    case = next(c for c in C.SIGN_CASES if c['name'] == 'S-A0')
    x, b, _y64, codes = _sign_ref(case, False)
    xd = x.to(gpu_device).requires_grad_(True)
    y = _op(case, xd, b.to(gpu_device), False, gpu_device, dyadic=True)
    dy = C.dyadic_grad(y.shape, 300).to(gpu_device).requires_grad_(True)
    dx, = torch.autograd.grad(y, xd, dy, create_graph=True)
    w = torch.randint(-4, 5, tuple(x.shape), generator=torch.Generator().manual_seed(301)).float() / 4
    ddy, = torch.autograd.grad((dx * w.to(gpu_device)).sum(), dy)
    assert _calls('filtered_lrelu') == 3
    _held(ddy, C.coded_forward64(case, codes, w, False), F32, 'second order S-A0')


@pytest.mark.parametrize('name', ['S-A0', 'S-G0'])
def test_sign_read_left_of_and_above_the_sign_tensor(gpu_device, name):
    """A raw sign-read launch whose offsets put the first columns and rows of the first tile outside the sign tensor: only the gain there, the
    coded factor inside.  The sign tensor is packed on the CPU from the oracle's codes, not taken from a sign-write launch."""
    case = next(c for c in C.SIGN_CASES if c['name'] == name)
    x, b, _y64, codes = _sign_ref(case, False)
    sh, sw_active, row_bytes = C.sign_hw(case)
    codes = codes.numpy()[:, :, :sh, :sw_active]
    s = torch.from_numpy(C.pack_codes(codes, row_bytes)).to(gpu_device)
    sx, sy = -6, -5
    zh, zw = C.z_hw(case)
    shifted = np.zeros((*codes.shape[:2], zh, zw), dtype=np.uint8)          # code of z element (zy, zx) = codes[zy + sy, zx + sx], 0 (gain only) where that is outside
    hh, ww = min(zh + sy, sh), min(zw + sx, sw_active)
    shifted[:, :, -sy:-sy + hh, -sx:-sx + ww] = codes[:, :, :hh, :ww]
    assert (shifted[:, :, :-sy] == 0).all() and (shifted[:, :, :, :-sx] == 0).all() and (shifted != 0).mean() > 0.2
    y, so, rc = _raw(case, x.to(gpu_device), b.to(gpu_device), s, sx, sy, False, False, gpu_device)
    assert rc == 0 and so.numel() == 0 and _calls('filtered_lrelu') == 1
    fu, fd = C.make_filter(case['fu'], True), C.make_filter(case['fd'], True)
    z = oracle_ops.upfirdn2d(x.double() + b.double().reshape(1, -1, 1, 1), fu, up=case['up'], padding=case['pad'], gain=case['up'] ** 2)
    want = oracle_ops.upfirdn2d(z * C.code_factor(case, shifted), fd, down=case['down'])
    _held(y, want, F32, f'raw sign read {name}')
    if name == 'S-G0':
        assert torch.equal(y.cpu(), want.float())


# ---- 4. the stand-alone activation kernel with signs (the return_code = -1 route) -----------------------------------------------------------------

def test_generic_path_float64_with_gradient(gpu_device):
    """float64 has no fused kernel: upfirdn2d -> filtered_lrelu_act_ (sign write) -> upfirdn2d, and the same backward with the signs read at the
    offset (-1, -1), all in float64 (gain, slope and clamp are fp32 in the ABI: values that fp32 holds exactly)."""
    case = dict(up=2, down=2, fu=(4, 4), fd=(4, 4), shape=(1, 2, 19, 23), pad=[2, 1, 2, 1], gain=1.25, slope=0.25, clamp=0.5)
    g = torch.Generator().manual_seed(41)
    x = torch.randn(*case['shape'], generator=g, dtype=torch.float64)
    b = torch.randn(2, generator=g, dtype=torch.float64)
    y64, codes = C.forward64(case, x, b, False)
    assert min(float((codes == k).float().mean()) for k in range(3)) > 0.05
    xd, bd = x.to(gpu_device).requires_grad_(True), b.to(gpu_device).requires_grad_(True)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore', RuntimeWarning)
        y = _op(case, xd, bd, False, gpu_device)
        assert _calls('filtered_lrelu_act_') == 1 and _calls('filtered_lrelu') == 0
        dy = torch.randn(*y.shape, generator=g, dtype=torch.float64) + 0.5
        dx, db = torch.autograd.grad(y, [xd, bd], dy.to(gpu_device))
    assert _calls('filtered_lrelu_act_') == 2 and _calls('filtered_lrelu') == 0
    want = C.backward64(case, codes, dy, False)
    _held(y, y64, torch.float64, 'generic path y', rel=1e-12)
    _held(dx, want, torch.float64, 'generic path dx', rel=1e-12)
    _held(db, want.sum([0, 2, 3]), torch.float64, 'generic path db', rel=1e-12)


def test_generic_path_when_the_fused_kernel_declines(gpu_device):
    """fp32 with a 2-D 65 x 65 filter pair (more than 8192 taps): the fused entry declines, the activation kernel writes the signs.  Integer taps
    with a power-of-two sum on dyadic data: bytes (all of them: fields past the width are zero codes) and y are exact."""
    i, j = np.mgrid[0:65, 0:65]
    k = ((7 * i + 11 * j) % 13 == 0).astype(np.int64)
    k[30, 37] += 512 - int(k.sum())
    assert int(k.sum()) == 512 and k[30, 37] > 0 and not np.array_equal(k, k[::-1, ::-1])
    f = torch.from_numpy(k.astype(np.float32) / 512)
    g = torch.Generator().manual_seed(42)
    x = torch.randint(-6, 7, (1, 2, 8, 8), generator=g).float() / 4
    b = torch.tensor([1.0, -1.0]) / 8
    kw = dict(up=1, down=1, padding=64, gain=64.0, slope=0.25, clamp=0.25)          # (unit-sum taps spread over 65 x 65: the gain brings the values to the clamp)
    y64, codes = oracle_ops.filtered_lrelu(x.double(), fu=f, fd=f, b=b.double(), return_signs=True, **kw)
    assert tuple(codes.shape[2:]) == (72, 72) and min(float((codes == c).float().mean()) for c in range(3)) > 0.05
    from torch_utils.ops import filtered_lrelu
    with pytest.warns(RuntimeWarning, match='no fused HIP kernel'):
        y = filtered_lrelu.filtered_lrelu(x.to(gpu_device).requires_grad_(True), fu=f.to(gpu_device), fd=f.to(gpu_device), b=b.to(gpu_device), **kw)
    assert _calls('filtered_lrelu') == 0 and _calls('filtered_lrelu_act_') == 1
    so = y.grad_fn.saved_tensors[2]
    assert so.dtype == torch.uint8 and tuple(so.shape) == (1, 2, 72, 80 // 4)
    assert np.array_equal(so.cpu().numpy(), C.pack_codes(codes, 20))
    _held(y, y64, F32, 'declined configuration y')
    assert torch.equal(y.detach().cpu(), y64.float())


@pytest.mark.parametrize('dtype', [F32, F16, BF16, torch.float64], ids=['fp32', 'fp16', 'bf16', 'fp64'])
def test_activation_kernel_raw_on_channels_last(gpu_device, dtype):
    """`filtered_lrelu_act_` in place on a channels_last tensor 10 wide (16 sign columns): values and bytes against the element-wise definition,
    zero codes past the width; then sign read at an offset, where fields past the width and positions outside the tensor only scale."""
    from torch_utils import hip_plugin
    plug = hip_plugin.FilteredLReluPlugin
    g = torch.Generator().manual_seed(43)
    gain, slope, clamp = 2.0, 0.25, 0.75
    v = torch.randint(-6, 7, (2, 3, 5, 10), generator=g).float() / 8          # dyadic: exact in every dtype, also after gain and slope
    x = v.to(dtype).to(gpu_device).contiguous(memory_format=torch.channels_last)
    assert x.stride(1) == 1
    so = plug.filtered_lrelu_act_(x, torch.empty([0]), 0, 0, gain, slope, clamp, True)
    z = v.double().numpy() * gain
    codes = np.where(np.abs(np.where(z < 0, z * slope, z)) > clamp, 2, (z < 0).astype(np.int64)).astype(np.uint8)
    want = np.clip(np.where(z < 0, z * slope, z), -clamp, clamp)
    assert all((codes == k).mean() > 0.05 for k in range(3)) and (z == 0).any() and (np.abs(want) == clamp).any()
    assert x.is_contiguous(memory_format=torch.channels_last) and np.array_equal(x.cpu().double().numpy(), want)
    assert so.dtype == torch.uint8 and tuple(so.shape) == (2, 3, 5, 4)
    assert np.array_equal(so.cpu().numpy(), C.pack_codes(codes, 4))
    # sign read at (sx, sy) = (-3, 1) on another channels_last tensor
    v2 = torch.randint(-6, 7, (2, 3, 5, 10), generator=g).float() / 8
    x2 = v2.to(dtype).to(gpu_device).contiguous(memory_format=torch.channels_last)
    none = plug.filtered_lrelu_act_(x2, so, -3, 1, gain, slope, clamp, False)
    assert none.numel() == 0 and _calls('filtered_lrelu_act_') == 2
    padded = np.zeros((2, 3, 5, 16), dtype=np.uint8)
    padded[..., :10] = codes
    factor = np.full(v2.shape, gain)
    for yy in range(5):
        for xx in range(10):
            sx_, sy_ = xx - 3, yy + 1
            if 0 <= sx_ < 16 and 0 <= sy_ < 5:
                cd = padded[:, :, sy_, sx_]
                factor[:, :, yy, xx] = np.where(cd == 2, 0.0, np.where(cd == 1, gain * slope, gain))
    assert np.array_equal(x2.cpu().double().numpy(), v2.double().numpy() * factor)


# ---- 5. what the entry point must refuse -------------------------------------------------------------------------------------------------------

def test_refused_arguments_launch_nothing(gpu_device):
    from torch_utils import hip_plugin
    plug = hip_plugin.FilteredLReluPlugin
    f = C.taps(12).to(gpu_device)
    x = torch.randn(1, 2, 9, 9, device=gpu_device)
    b = torch.zeros(2, device=gpu_device)
    none = torch.empty([0])
    args = lambda x_, b_, up, sx, write: (x_, f, f, b_, none, up, 2, 10, 11, 10, 11, sx, 0, 1.0, 0.2, INF, False, write)
    with pytest.raises(RuntimeError, match='up and down must be at least 1'):
        plug.filtered_lrelu(*args(x, b, 0, 0, False))
    with pytest.raises(RuntimeError, match='x is empty'):
        plug.filtered_lrelu(*args(x[:, :, :0], b, 2, 0, False))
    with pytest.raises(RuntimeError, match='float16, bfloat16 or float32'):
        plug.filtered_lrelu(*args(x.double(), b.double(), 2, 0, False))
    y, so, rc = plug.filtered_lrelu(*args(x, b, 2, 2, True))          # sign write needs sx % 4 == 0: declined, no kernel
    assert rc == -1 and y.numel() == 0 and so.numel() == 0
    assert _calls('filtered_lrelu') == 0
    y, so, rc = plug.filtered_lrelu(*args(x, b, 2, 4, True))          # ... and the same call with an aligned offset runs
    assert rc == 0 and _calls('filtered_lrelu') == 1 and tuple(y.shape) == (1, 2, 9, 9)
