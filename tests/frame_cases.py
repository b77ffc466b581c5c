"""The inputs of the frame-conversion suites: tests/test_frame_cases_cpu.py checks them without a GPU, tests/test_gpu_frame.py runs
`ide3d_frame_u8` (csrc/frame.hip) and the ATen branch of `training.distributed_render.frames_u8` on them.

The definition is `(x * 127.5 + 128).clamp(0, 255).to(uint8)`: the product is rounded to fp32, then the sum, then the value is truncated.
A kernel that contracts the two into one fused multiply-add rounds once.  The two agree unless the product's rounding carries the sum
across an integer, which can only happen for x next to (k - 128) / 127.5, the pre-image of a byte boundary k.  `boundary_values()` holds
every fp32 value within 64 ulp of each of the 257 pre-images; on a random image such a value turns up about twice per million pixels.

`twice_rounded` and `single_rounded` evaluate both ways on the CPU.  The single rounding is taken in float64: x (24 bits) times 127.5
(8 bits) is exact there, and so is the sum with 128 for every |x| >= 2^-21; below that the float64 sum rounds to a value next to 128 that
is no fp32 midpoint, so the fp32 result is the singly rounded one as well."""

import numpy as np
import torch

ULPS = 64
CLAMP_END = 1.0039216          # 128 / 127.5 rounded: 127.5 x + 128 = 256 here, and 0 at the negative end


def boundary_values(seed=0, randn=1024):
    """float32 [N]: the neighbours of every byte boundary's pre-image, the special values, a block of randn.  No NaN (its uint8 cast is
    unspecified)."""
    centre = ((np.arange(257, dtype=np.float64) - 128.0) / 127.5).astype(np.float32)
    steps = np.arange(-ULPS, ULPS + 1, dtype=np.int32)
    # integer steps on the bit pattern walk through the neighbouring floats of either sign (+ away from zero).  The centre of k = 128 is
    # +0: its pattern steps up into the positive subnormals and down into NaN patterns, which are dropped; the negative subnormals
    # are added by sign below
    near = (centre.view(np.int32)[:, None] + steps[None, :]).astype(np.int32).view(np.float32).reshape(-1)
    near = near[np.isfinite(near)]
    tiny = (np.arange(1, ULPS + 1, dtype=np.int32)).view(np.float32)
    special = np.array([0.0, -0.0, 1.0, -1.0, np.inf, -np.inf, CLAMP_END, -CLAMP_END, np.float32(1.1754942e-38), -np.float32(1.1754942e-38)],
                       dtype=np.float32)          # 1.1754942e-38: the largest subnormal
    rnd = torch.randn(randn, generator=torch.Generator().manual_seed(seed)).numpy()
    out = np.concatenate([near, -tiny, special, rnd]).astype(np.float32)
    assert not np.isnan(out).any()
    return out


def boundary_of(values):
    """The byte boundary k (0 .. 256) next to each value: round(127.5 x + 128) in float64, clipped."""
    with np.errstate(invalid='ignore'):
        k = np.rint(values.astype(np.float64) * 127.5 + 128.0)
    return np.clip(np.nan_to_num(k, posinf=256, neginf=0), 0, 256).astype(np.int64)


def _to_byte(t):
    return np.clip(t, np.float32(0), np.float32(255)).astype(np.uint8)


def twice_rounded(values):
    """The definition: fp32 product, fp32 sum, clamp, truncate."""
    v = values.astype(np.float32)
    return _to_byte((v * np.float32(127.5)).astype(np.float32) + np.float32(128))


def single_rounded(values):
    """What a fused multiply-add gives: one rounding of the exact 127.5 x + 128."""
    return _to_byte((values.astype(np.float64) * 127.5 + 128.0).astype(np.float32))


def image(values, n, h, w):
    """float32 [n, 3, h, w] that holds `values` in order, repeated until the image is full (so every group of four pixels, whichever lane and
    grid-stride trip converts it, meets boundary values)."""
    assert 3 * n * h * w >= values.size, (values.size, n, h, w)
    return torch.from_numpy(np.resize(values, 3 * n * h * w).reshape(n, 3, h, w).copy())


def seg_logits(n, classes, h, w, seed=1):
    return torch.randn(n, classes, h, w, generator=torch.Generator().manual_seed(seed))


def argmax_cases():
    """[(name, seg [1, classes, 1, 8])] for classes = 1, 2, 19: exact ties (the first index wins, +0 against -0 included), NaN in one
    class (it counts as the maximum), NaN in the first class, NaN in two classes (the first one wins), all -inf, +inf against finite."""
    inf, nan = float('inf'), float('nan')
    out = []
    for classes in (1, 2, 19):
        g = torch.Generator().manual_seed(classes)
        seg = torch.randn(1, classes, 1, 8, generator=g)
        last = classes - 1
        seg[0, :, 0, 0] = 0.5                                   # all equal
        seg[0, :, 0, 1] = -inf                                  # all -inf
        seg[0, :, 0, 2] = -0.0; seg[0, 0, 0, 2] = 0.0          # +0 first, then -0
        seg[0, :, 0, 3] = 0.0; seg[0, 0, 0, 3] = -0.0          # -0 first, then +0: still the first
        seg[0, last, 0, 4] = nan                                # NaN in the last class
        seg[0, 0, 0, 5] = nan                                   # NaN in the first class
        seg[0, last // 2, 0, 6] = nan; seg[0, last, 0, 6] = nan  # two NaN: the first of them
        seg[0, :, 0, 7] = -1.0; seg[0, last, 0, 7] = inf; seg[0, last // 2, 0, 7] = inf
        out.append((f'classes{classes}', seg))
    return out
