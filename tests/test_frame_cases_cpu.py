"""The frame-conversion inputs (tests/frame_cases.py) without a GPU: the values separate a conversion that rounds the product and the sum
(the definition) from one that rounds once (a contracted kernel), the oracle is the definition, and the argmax cases say what they claim."""

import numpy as np
import torch

import frame_cases as fc
from oracle import ops as oracle_ops


def test_boundary_values_separate_single_from_twice_rounded_conversion():
    """A condition on the inputs: at least 100 values on at least 100 distinct byte boundaries give another byte when 127.5 x + 128 is rounded
    once.  A kernel that contracts the conversion cannot pass tests/test_gpu_frame.py on them."""
    v = fc.boundary_values()
    assert v.dtype == np.float32 and not np.isnan(v).any()
    for special in (0.0, 1.0, -1.0, np.inf, -np.inf, fc.CLAMP_END, -fc.CLAMP_END, 1.1754942e-38):
        assert (v == np.float32(special)).any(), special
    assert (np.signbit(v) & (v == 0)).any() and (~np.signbit(v) & (v == 0)).any()
    two, one = fc.twice_rounded(v), fc.single_rounded(v)
    differ = two != one
    boundaries = np.unique(fc.boundary_of(v[differ]))
    print(f'{int(differ.sum())} of {v.size} values differ, on {boundaries.size} byte boundaries')
    assert int(differ.sum()) >= 100 and boundaries.size >= 100
    assert np.abs(two[differ].astype(int) - one[differ].astype(int)).max() == 1
    # every boundary has all its 129 neighbours in the table, on both sides of it
    k = fc.boundary_of(v[:257 * (2 * fc.ULPS + 1) - fc.ULPS])
    assert np.array_equal(np.unique(k), np.arange(257))
    # the ends saturate: everything at or beyond the clamp ends, and the infinities
    assert two[v == np.inf][0] == 255 and two[v == -np.inf][0] == 0
    assert two[v == np.float32(fc.CLAMP_END)][0] == 255 and two[v == -np.float32(fc.CLAMP_END)][0] == 0
    assert two[v == 1.0][0] == 255 and two[v == -1.0][0] == 0 and (two[v == 0] == 128).all()


def test_the_oracle_is_the_twice_rounded_definition():
    v = fc.boundary_values()
    for n, h, w in ((1, 2850, 4), (1, 1, 11396), (3, 31, 124)):
        img = fc.image(v, n, h, w)
        seg = fc.seg_logits(n, 2, h, w)
        got = oracle_ops.frame_u8(img, seg, oracle_ops.PALETTE[:2])
        assert got.shape == (n, h, 2 * w, 3) and got.dtype == np.uint8
        want = fc.twice_rounded(img.numpy().reshape(-1)).reshape(n, 3, h, w).transpose(0, 2, 3, 1)
        assert np.array_equal(got[:, :, :w], want)
        # ... and the ATen branch of frames_u8 is the same expression
        from training import distributed_render
        pal = torch.from_numpy(oracle_ops.PALETTE[:2])
        assert np.array_equal(distributed_render.frames_u8(img, seg, pal).numpy(), got)


def test_argmax_cases_hold_what_they_claim():
    for name, seg in fc.argmax_cases():
        classes = seg.shape[1]
        last = classes - 1
        idx = torch.argmax(seg, dim=1)[0, 0].tolist()
        assert idx[0] == 0 and idx[1] == 0 and idx[2] == 0 and idx[3] == 0, name
        assert idx[4] == last and idx[5] == 0 and idx[6] == last // 2 and idx[7] == last // 2, (name, idx)
        assert bool(torch.isnan(seg[0, :, 0, 4:7]).any(dim=0).all())
        if classes > 1:
            assert bool(torch.signbit(seg[0, 1, 0, 2])) and bool(torch.signbit(seg[0, 0, 0, 3])) and not bool(torch.signbit(seg[0, 1, 0, 3]))
        pal = oracle_ops.PALETTE[:classes]
        img = torch.zeros(1, 3, 1, 8)
        assert np.array_equal(oracle_ops.frame_u8(img, seg, pal)[0, 0, 8:], pal[idx])
