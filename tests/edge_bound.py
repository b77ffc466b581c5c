"""The bound of the small-kernel edge suites (tests/test_gpu_bias_act.py, test_gpu_resample.py, test_gpu_camera.py), the project's convention
(tests/test_gpu_id_loss.py `_within`) for any storage dtype:

    max |got - want| <= max(4 max |aten - want|, one ulp of the storage dtype at max |want|)

`want` is float64, `aten` the same definition evaluated by ATen in the storage dtype on the same device.  Every call prints its figures in
one line that starts with MEASURED; profiles/small_ops/edge_suite_measured.json is the per-kernel maximum of those lines."""

import math

import torch

MANTISSA_BITS = {torch.float64: 52, torch.float32: 23, torch.float16: 10, torch.bfloat16: 7}
DTYPE_NAMES = {torch.float64: 'float64', torch.float32: 'float32', torch.float16: 'float16', torch.bfloat16: 'bfloat16'}


def ulp(value, dtype):
    """The spacing of `dtype` at |value| (normal range)."""
    value = abs(float(value))
    if value == 0 or not math.isfinite(value):
        return 0.0
    return 2.0 ** (math.floor(math.log2(value)) - MANTISSA_BITS[dtype])


def max_err(got, want, alt=None, undecided=None, strict=True):
    """max |got - want| over the entries where `want` is finite; where `undecided` is set, the smallest of |got - want| and |got - alt| for
    every alternative (an element whose branch the storage rounding may decide either way).  `strict`: `got` is non-finite exactly where `want` is, with NaN in
    the same positions and infinities of the same sign; otherwise the entries where `got` is not finite are left out as well."""
    want = want.detach().cpu().double()
    got = got.detach().cpu().double()
    assert got.shape == want.shape, (got.shape, want.shape)
    err = (got - want).abs()
    if undecided is not None and bool(undecided.any()):
        for other in (alt if isinstance(alt, (tuple, list)) else (alt,)):
            err = torch.where(undecided, torch.minimum(err, (got - other.detach().cpu().double()).abs()), err)
    finite = torch.isfinite(want)
    if strict:
        assert torch.equal(torch.isfinite(got), finite), 'non-finite values in other positions than the reference'
        assert torch.equal(torch.isnan(got), torch.isnan(want)), 'NaN in other positions than the reference'
        inf = ~finite & ~torch.isnan(want)
        assert torch.equal(got[inf], want[inf]), 'infinities of another sign'
    else:
        finite = finite & torch.isfinite(got)
    return float(err[finite].max()) if bool(finite.any()) else 0.0


def within(got, want, aten, dtype, kernel, quantity, alt=None, undecided=None):
    err, ref = max_err(got, want, alt, undecided), max_err(aten, want, alt, undecided, strict=False)
    want = want.detach().cpu().double()
    finite = want[torch.isfinite(want)]
    floor = ulp(float(finite.abs().max()) if finite.numel() else 0.0, dtype)
    bound = max(4 * ref, floor)
    print(f'MEASURED kernel={kernel} quantity={quantity} dtype={DTYPE_NAMES[dtype]} err={err:.3e} aten={ref:.3e} ulp={floor:.3e} bound={bound:.3e}')
    return err <= bound
