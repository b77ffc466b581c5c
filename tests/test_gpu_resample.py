"""The two resampling kernels of csrc/resample.hip at their edges, against float64.

`ide3d_skip_upsample_add_cl` (upsample2d(lo, [1, 3, 3, 1]) + add, written channels-last) against `oracle.ops.upsample2d(...) + add` in float64:
a one-pixel image, a last column tile of two pixels, exact tiles, three channel groups with four channels in the last; `lo` NCHW,
channels-last and as a slice of a tensor that is wider in every axis; `add` as a channel slice and channels-last; the `out=` form; an
infinity and a NaN in `lo` (only the outputs whose taps reach them are non-finite) and around the slice (nothing is).
`ide3d_bilinear_up2_split` against `F.interpolate(mode='bilinear', align_corners=False)` in float64: one row, two columns, an odd channel
count, an empty range, overlapping ranges, the `adjacent=` form.

Bound (tests/edge_bound.py): error <= max(4 x the error of `upfirdn2d.upsample2d(...) + add`, or of fp32 `F.interpolate`, on the device,
one fp32 ulp of the largest magnitude).  Measured: profiles/small_ops/edge_suite_measured.json, kernels skip_upsample_add_cl and
bilinear_up2_split."""

import pytest
import torch
import torch.nn.functional as F

from edge_bound import within
from oracle import ops as oracle_ops

pytestmark = pytest.mark.gpu

SKIP_SHAPES = [(1, 4, 1, 1), (1, 4, 3, 17), (2, 32, 4, 16), (1, 68, 5, 16)]


def _plugin():
    from torch_utils import hip_plugin
    hip_plugin.load()
    return hip_plugin.ResamplePlugin


def _calls(name):
    from torch_utils import hip_plugin
    return hip_plugin.CALLS.get(name, 0)


def _wider(t, fill):
    """(`t` as a slice of a tensor that is wider in every axis and holds `fill` around it, that tensor)."""
    n, c, h, w = t.shape
    big = torch.full((n + 1, c + 4, h + 2, w + 3), fill, dtype=t.dtype, device=t.device)
    view = big[1:, 2:2 + c, 1:1 + h, 2:2 + w]
    view.copy_(t)
    return view, big


def _skip_reference(lo, add):
    from torch_utils.ops import upfirdn2d
    f = upfirdn2d.setup_filter([1, 3, 3, 1])
    return oracle_ops.upsample2d(lo.double(), f) + add.double()


def _skip_on_device(lo, add):
    from torch_utils.ops import upfirdn2d
    f = upfirdn2d.setup_filter([1, 3, 3, 1]).to(lo.device)
    return upfirdn2d.upsample2d(lo.contiguous(), f) + add


@pytest.mark.parametrize('n,c,h,w', SKIP_SHAPES)
def test_skip_upsample_add_layouts(gpu_device, n, c, h, w):
    P = _plugin()
    g = torch.Generator().manual_seed(31)
    lo = torch.randn(n, c, h, w, generator=g)
    wide = torch.randn(n, 2 * c, 2 * h, 2 * w, generator=g)
    add = wide[:, c:]
    want = _skip_reference(lo, add)
    lod, addd = lo.to(gpu_device), wide.to(gpu_device)[:, c:]
    aten = _skip_on_device(lod, addd)
    sliced, _ = _wider(lod, 7.0)
    assert not sliced.is_contiguous() and sliced.stride(3) == 1
    forms = {
        'nchw lo, sliced add': (lod, addd),
        'channels-last lo': (lod.contiguous(memory_format=torch.channels_last), addd),
        'lo a slice of a wider tensor': (sliced, addd),
        'channels-last add': (lod, addd.contiguous(memory_format=torch.channels_last)),
    }
    first = None
    for name, (l, a) in forms.items():
        before = _calls('skip_upsample_add_cl')
        got = P.skip_upsample_add_cl(l, a)
        assert _calls('skip_upsample_add_cl') == before + 1
        assert got.shape == (n, c, 2 * h, 2 * w) and got.is_contiguous(memory_format=torch.channels_last)
        assert within(got, want, aten, torch.float32, 'skip_upsample_add_cl', 'out'), name
        first = got if first is None else first
        assert torch.equal(got, first), f'{name}: the strides of the inputs change the values'
    # out=: written in place, nothing else allocated for the result, margins of a larger buffer untouched
    buf = torch.full((n * c * 4 * h * w + 8,), 55.0, device=gpu_device)
    out = buf[4:-4].view(n, 2 * h, 2 * w, c).permute(0, 3, 1, 2)
    assert out.is_contiguous(memory_format=torch.channels_last) and out.data_ptr() % 16 == 0
    ret = P.skip_upsample_add_cl(lod, addd, out=out)
    assert ret.data_ptr() == out.data_ptr() and torch.equal(out, first)
    assert bool((buf[:4] == 55.0).all()) and bool((buf[-4:] == 55.0).all())


@pytest.mark.parametrize('n,c,h,w', SKIP_SHAPES)
def test_skip_upsample_add_non_finite_neighbours(gpu_device, n, c, h, w):
    """One inf and one NaN in `lo`: the outputs whose four taps reach them, and no others, are non-finite (same positions, same sign as the
    float64 reference).  The same two values in the part of a wider tensor around the slice: nothing in the output is non-finite."""
    P = _plugin()
    g = torch.Generator().manual_seed(32)
    lo = torch.randn(n, c, h, w, generator=g)
    add = torch.randn(n, c, 2 * h, 2 * w, generator=g)
    clean_want = _skip_reference(lo, add)
    lod, addd = lo.to(gpu_device), add.to(gpu_device)
    clean_aten = _skip_on_device(lod, addd)
    for fill in (float('inf'), float('nan')):
        sliced, big = _wider(lod, fill)
        assert not bool(torch.isfinite(big).all())
        got = P.skip_upsample_add_cl(sliced, addd)
        assert bool(torch.isfinite(got).all()), f'{fill} outside the slice reached the output'
        assert within(got, clean_want, clean_aten, torch.float32, 'skip_upsample_add_cl', 'out_in_poisoned_surroundings')
    bad = lo.clone()
    bad[0, 0, 0, 0] = float('inf')                         # a corner: 2 x 2 outputs (1 x 1 image: all of them)
    bad[n - 1, c - 1, h - 1, w - 1] = float('nan')          # the opposite corner of the last channel
    if w > 8:
        bad[0, 1, h // 2, 8] = float('-inf')               # inside
    want = _skip_reference(bad, add)
    badd = bad.to(gpu_device)
    got = P.skip_upsample_add_cl(badd, addd)
    touched = ~torch.isfinite(want)
    assert 8 <= int(touched.sum()) <= 9 + 9 + 16          # a pixel reaches 4 outputs per axis, fewer at the border
    assert within(got, want, _skip_on_device(badd, addd), torch.float32, 'skip_upsample_add_cl', 'out_with_inf_nan')          # positions and signs: edge_bound.max_err
    assert torch.equal(got.cpu()[~touched], P.skip_upsample_add_cl(lod, addd).cpu()[~touched]), 'an output away from the non-finite inputs changed'


BILINEAR_CASES = [
    ('one_row', (2, 3, 1, 4), [(0, 3)], None),
    ('two_columns', (1, 4, 5, 2), [(0, 2), (2, 2)], None),
    ('odd_channels', (1, 5, 3, 4), [(1, 4)], None),
    ('empty_range', (2, 5, 3, 4), [(0, 3), (1, 0), (3, 2)], None),
    ('empty_first', (1, 5, 3, 4), [(2, 0), (0, 5)], None),
    ('overlapping', (2, 5, 3, 6), [(0, 4), (2, 3), (1, 2)], None),
    ('adjacent', (2, 7, 4, 6), [(0, 4), (0, 3), (4, 3)], (1, 2)),
    ('adjacent_overlapping', (1, 5, 1, 2), [(0, 2), (1, 3)], (0, 1)),
]


@pytest.mark.parametrize('name,shape,ranges,adjacent', BILINEAR_CASES, ids=[c[0] for c in BILINEAR_CASES])
def test_bilinear_up2_split_edges(gpu_device, name, shape, ranges, adjacent):
    P = _plugin()
    n, c, h, w = shape
    x = torch.randn(*shape, generator=torch.Generator().manual_seed(33))
    xd = x.to(gpu_device)
    before = _calls('bilinear_up2_split')
    outs = P.bilinear_up2_split(xd, ranges, adjacent=adjacent)
    assert _calls('bilinear_up2_split') == before + 1 and len(outs) == len(ranges)
    for k, (o, (b, cnt)) in enumerate(zip(outs, ranges)):
        assert o.shape == (n, cnt, 2 * h, 2 * w) and o.dtype == torch.float32
        if cnt == 0:
            continue
        want = F.interpolate(x[:, b:b + cnt].double(), size=(2 * h, 2 * w), mode='bilinear', align_corners=False)
        aten = F.interpolate(xd[:, b:b + cnt], size=(2 * h, 2 * w), mode='bilinear', align_corners=False)
        assert within(o, want, aten, torch.float32, 'bilinear_up2_split', 'out'), (name, k)
    if adjacent:
        i, j = adjacent
        assert outs[i]._base is outs[j]._base and outs[i]._base.shape == (n, ranges[i][1] + ranges[j][1], 2 * h, 2 * w)
        plain = P.bilinear_up2_split(xd, ranges)
        for o, q in zip(outs, plain):
            assert torch.equal(o, q)
