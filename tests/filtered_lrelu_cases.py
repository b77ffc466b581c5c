"""Case tables and float64 closed forms for tests/test_gpu_filtered_lrelu.py; tests/test_filtered_lrelu_cases_cpu.py
holds the tables to csrc/filtered_lrelu.hip without a GPU.

`INSTANCE_CASES` has at least one case per compile-time instance of `filtered_lrelu_sep_kernel` (the `IDE3D_FLS` lines), each with 2 x 2
output tiles of 32 x 32 and a partial last tile in both directions; `GENERIC_CASES` are configurations no instance matches, with an output
wider and taller than the generic kernel's largest tile (64 x 32).  `SIGN_CASES` reuse the instance geometries (+ two generic ones) with
dyadic data, for which the value that is classified is exact in fp32 in any summation order.
"""

import os
import re

import numpy as np
import torch

from oracle import ops as oracle_ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNEL_SOURCE = os.path.join(ROOT, 'ide-3d_amd', 'csrc', 'filtered_lrelu.hip')


# ---- what the kernel source says -----------------------------------------------------------------------------------------------------

def source_instances(text=None):
    """The (up, down, fu taps, fd taps) tuples of the IDE3D_FLS(...) lines."""
    text = open(KERNEL_SOURCE).read() if text is None else text
    return [tuple(int(v) for v in m) for m in re.findall(r'^\s*IDE3D_FLS\((\d+), (\d+), (\d+), (\d+)\)\s*$', text, flags=re.M)]


def source_instance_tile(text=None):
    text = open(KERNEL_SOURCE).read() if text is None else text
    m = re.search(r'static constexpr int TOW = (\d+), TOH = (\d+);', text)
    return int(m.group(1)), int(m.group(2))


def source_generic_tiles(text=None):
    """(candidate tiles (w, h) in the order tried, LDS budget in bytes) of `launch_flr` / `flr_geometry`."""
    text = open(KERNEL_SOURCE).read() if text is None else text
    cand = re.search(r'static const int cand\[\]\[2\] = \{(.*?)\};', text).group(1)
    budget = re.search(r'sizeof\(float\) <= (\d+) \* 1024', text)
    return [(int(a), int(b)) for a, b in re.findall(r'\{(\d+), (\d+)\}', cand)], int(budget.group(1)) * 1024


def generic_tile(up, down, fu_shape, fd_shape, cand, budget):
    """`flr_geometry` + the candidate loop of `launch_flr` restated: the first tile whose LDS carve fits.  Filter shapes are (taps,) for a
    separable filter and (h, w) for a 2-D one."""
    r4 = lambda v: (v + 3) & ~3
    fuw, fuh = fu_shape[-1], fu_shape[0]
    fdw, fdh = fd_shape[-1], fd_shape[0]
    for tow, toh in cand:
        if (tow * down) % 4:
            continue
        zw, zh = r4((tow - 1) * down + fdw), (toh - 1) * down + fdh
        iw, ih = (zw + fuw - 1) // up + 2, (zh + fuh - 1) // up + 2
        o = r4((fuw * fuh if len(fu_shape) == 2 else 2 * fuw) + (fdw * fdh if len(fd_shape) == 2 else 2 * fdw))
        o = r4(o + iw * ih)
        o = r4(o + (0 if len(fu_shape) == 2 else ih * zw))
        o = r4(o + zh * zw)
        o += 0 if len(fd_shape) == 2 else zh * tow
        if o * 4 <= budget:
            return tow, toh
    return None


# ---- filters ---------------------------------------------------------------------------------------------------------------------------

def taps(n, skew=0.3):
    """n asymmetric low-pass taps with unit sum (fp32), so that a flipped filter gives another result."""
    i = np.arange(n, dtype=np.float64)
    k = (1 + i * (n - 1 - i)) * (1 + skew * i / n) + 0.5 * (i % 3 == 1)
    return torch.from_numpy((k / k.sum()).astype(np.float32))


def taps2d(h, w):
    """A 2-D filter that is neither symmetric nor an outer product."""
    k = np.outer(taps(h, 0.4).double().numpy(), taps(w, -0.25).double().numpy())
    i, j = np.mgrid[0:h, 0:w]
    k = k + 0.2 * ((3 * i + 5 * j) % 7) / (7.0 * h * w)
    return torch.from_numpy((k / k.sum()).astype(np.float32))


# integer taps whose sum is a power of two (dyadic after normalisation), asymmetric
DYADIC = {
    8: ([1, 2, 4, 8, 8, 4, 3, 2], 32),
    9: ([1, 2, 3, 5, 8, 6, 4, 2, 1], 32),
    12: ([1, 1, 2, 4, 8, 16, 8, 8, 8, 4, 2, 2], 64),
    24: ([1, 1, 1, 2, 2, 2, 4, 6, 8, 10, 12, 14, 14, 12, 10, 8, 6, 5, 3, 2, 2, 1, 1, 1], 128),
}
DYADIC_4X4 = ([[1, 2, 3, 2], [2, 6, 8, 4], [3, 8, 9, 4], [1, 3, 5, 3]], 64)


def dyadic_taps(n):
    k, s = DYADIC[n]
    assert sum(k) == s and s & (s - 1) == 0 and k != k[::-1]
    return torch.tensor(k, dtype=torch.float32) / s


def dyadic_4x4():
    k, s = DYADIC_4X4
    k = torch.tensor(k, dtype=torch.float32)
    assert int(k.sum()) == s and not torch.equal(k, k.flip(0, 1)) and not torch.equal(k, k.t())
    return k / s


def make_filter(spec, dyadic=False):
    """spec: None | n (separable taps) | (h, w) (2-D)."""
    if spec is None:
        return None
    if isinstance(spec, int):
        return dyadic_taps(spec) if dyadic else taps(spec)
    if dyadic:
        assert tuple(spec) == (4, 4)
        return dyadic_4x4()
    return taps2d(*spec)


def filter_shape(spec):
    """Shape as the kernel sees it: an absent filter is one separable tap."""
    return (1,) if spec is None else ((spec,) if isinstance(spec, int) else tuple(spec))


# ---- the cases -------------------------------------------------------------------------------------------------------------------------

def _case(name, up, down, fu, fd, shape, pad, gain, slope, clamp, why, bf16=False):
    return dict(name=name, up=up, down=down, fu=fu, fd=fd, shape=shape, pad=pad, gain=gain, slope=slope, clamp=clamp, why=why, bf16=bf16)


# (slope, clamp, gain) cover {0, 0.2, 1.5} x {None, 0.8} and gains other than sqrt(2) over the set
INSTANCE_CASES = [
    _case('A0', 2, 2, 12, 12, (2, 3, 37, 41), [10, 11, 10, 11], 1.3, 0.2, 0.8, 'rx0 = ry0 = 0: aligned horizontal pass', bf16=True),
    _case('A1', 2, 2, 12, 12, (2, 3, 37, 41), [9, 10, 11, 12], 0.9, 1.5, None, 'odd pad_x0 / pad_y0: unaligned horizontal pass, row_ok guards; 40 wide: 16-byte stores in the partial tile'),
    _case('A2', 4, 2, 12, 12, (1, 2, 19, 21), [12, 9, 8, 13], 2.5, 0.0, 0.8, 'pad_x0 % 4 == 0: aligned pass of up 4 (8-byte window reads)', bf16=True),
    _case('A3', 4, 2, 12, 12, (1, 2, 19, 21), [11, 10, 10, 11], 1.3, 0.2, None, 'phases 3 and 2'),
    _case('A4', 4, 2, 24, 12, (1, 2, 18, 17), [16, 17, 16, 17], 0.9, 1.5, 0.8, 'aligned pass with 6 taps per phase'),
    _case('A4u', 4, 2, 24, 12, (1, 2, 18, 17), [17, 16, 16, 17], 2.5, 0.2, 0.8, 'pad_x0 = 17: phase 1'),
    _case('A5', 2, 2, 8, 8, (1, 2, 35, 34), [6, 7, 6, 7], 1.3, 0.0, None, '8 + 8 taps', bf16=True),
    _case('A6', 2, 1, 12, None, (1, 2, 18, 17), [6, 5, 6, 5], 0.9, 0.2, 0.8, 'no down-sampling filter: the absent filter as one separable tap'),
    _case('A7', 1, 2, None, 12, (1, 2, 70, 67), [5, 6, 5, 6], 2.5, 1.5, 0.8, 'no up-sampling filter: input rows longer than a wave (IWP > 64 staging) on four tiles'),
]

GENERIC_CASES = [
    _case('G0', 2, 2, (4, 4), (4, 4), (1, 2, 40, 70), [2, 1, 2, 1], 1.3, 0.2, 0.8, '2-D 4x4 pair'),
    _case('G1', 3, 3, 9, 9, (1, 2, 40, 70), [7, 8, 7, 8], 0.9, 1.5, None, 'up = down = 3, separable'),
    _case('G2', 2, 4, 12, 12, (1, 2, 67, 131), [10, 11, 10, 11], 2.5, 0.0, 0.8, 'down 4: the 64x32 and 32x32 tiles do not fit the LDS budget'),
    _case('G3', 2, 2, 12, (5, 5), (1, 2, 40, 70), [7, 8, 7, 8], 1.3, 0.2, None, 'separable up filter, 2-D down filter'),
    _case('G4', 2, 2, (5, 5), 12, (1, 2, 40, 70), [7, 8, 7, 8], 0.9, 1.5, 0.8, '2-D up filter, separable down filter'),
    _case('G5', 4, 2, (16, 16), (4, 4), (1, 2, 20, 35), [9, 9, 9, 9], 2.5, 0.2, 0.8, '2-D 16x16 up filter at up 4'),
    _case('G6', 1, 1, None, None, (1, 2, 40, 70), [2, 1, 1, 0], 1.3, 0.0, 0.8, 'no filters at all'),
]
for _c in GENERIC_CASES:
    _c['bf16'] = True

VALUE_CASES = INSTANCE_CASES + GENERIC_CASES

# dyadic data: gain 2, slope 1/4; bias (in eighths, per channel) and clamp chosen per case so that each code occurs in >= 5 % of the oracle's elements
SIGN_SLOPE, SIGN_GAIN = 0.25, 2.0


def _sign(name, value_case, bias8, clamp):
    c = dict(next(v for v in VALUE_CASES if v['name'] == value_case))
    c.update(name=name, bias8=bias8, clamp=clamp, gain=SIGN_GAIN, slope=SIGN_SLOPE)
    return c


SIGN_CASES = [
    _sign('S-A0', 'A0', (1, -2, 0), 0.5),
    _sign('S-A1', 'A1', (-1, 2, 1), None),
    _sign('S-A2', 'A2', (1, -1), 0.5),
    _sign('S-A3', 'A3', (2, -1), 0.25),
    _sign('S-A4', 'A4', (-1, 1), 0.5),
    _sign('S-A4u', 'A4u', (1, 0), None),
    _sign('S-A5', 'A5', (-1, 1), 0.5),
    _sign('S-A6', 'A6', (1, -1), 0.25),
    _sign('S-A7', 'A7', (2, -2), 0.5),
    _sign('S-G0', 'G0', (1, -1), 0.5),
    _sign('S-G1', 'G1', (-1, 1), 0.5),
]


def instance_of(case):
    """(up, down, fu taps, fd taps) when both filters are separable (or absent), else None."""
    fu, fd = filter_shape(case['fu']), filter_shape(case['fd'])
    return (case['up'], case['down'], fu[0], fd[0]) if len(fu) == 1 and len(fd) == 1 else None


def z_hw(case):
    """Size of the up-sampled intermediate."""
    fu = filter_shape(case['fu'])
    p = case['pad']
    return (case['shape'][2] * case['up'] + p[2] + p[3] - (fu[0] - 1), case['shape'][3] * case['up'] + p[0] + p[1] - (fu[-1] - 1))


def out_hw(case):
    fd = filter_shape(case['fd'])
    zh, zw = z_hw(case)
    return ((zh - (fd[0] - 1) + case['down'] - 1) // case['down'], (zw - (fd[-1] - 1) + case['down'] - 1) // case['down'])


def sign_hw(case):
    """(rows, active columns, bytes per row) of the sign tensor a forward pass writes (filtered_lrelu.cpp:89-93)."""
    fd = filter_shape(case['fd'])
    oh, ow = out_hw(case)
    sh, sw_active = oh * case['down'] - (case['down'] - 1) + fd[0] - 1, ow * case['down'] - (case['down'] - 1) + fd[-1] - 1
    return sh, sw_active, ((sw_active + 15) & ~15) >> 2


# ---- float64 definitions -----------------------------------------------------------------------------------------------------------------

def f32(v):
    """A scalar as the C ABI carries it (gain, slope and clamp are fp32 there)."""
    return None if v is None else float(np.float32(v))


def forward64(case, x, b, flip, fu=None, fd=None):
    """oracle.ops.filtered_lrelu in float64 on the given (already rounded) x and b: (y, codes)."""
    fu = make_filter(case['fu'], 'bias8' in case) if fu is None else fu
    fd = make_filter(case['fd'], 'bias8' in case) if fd is None else fd
    return oracle_ops.filtered_lrelu(x.double(), fu=fu, fd=fd, b=b.double(), up=case['up'], down=case['down'], padding=case['pad'],
                                     gain=f32(case['gain']), slope=f32(case['slope']), clamp=f32(case['clamp']), flip_filter=flip, return_signs=True)


def intermediate64(case, x, b, flip):
    """The value that is classified: gain * up^2 * up-FIR(x + b), before slope and clamp."""
    fu = make_filter(case['fu'], 'bias8' in case)
    a = x.double() + b.double().reshape(1, -1, 1, 1)
    return oracle_ops.upfirdn2d(a, fu, up=case['up'], padding=case['pad'], gain=case['up'] ** 2, flip_filter=flip) * f32(case['gain'])


def code_factor(case, codes):
    """Per-element factor of the backward pass: gain * slope where negative, 0 where clamped, gain elsewhere."""
    codes = codes.numpy() if isinstance(codes, torch.Tensor) else codes
    g, s = f32(case['gain']), f32(case['slope'])
    return torch.from_numpy(np.where(codes == 2, 0.0, np.where(codes == 1, g * s, g)))


def _adjoint_pad(f_shape, in_len_up, out_len_down, p0, up):
    return f_shape - 1 - p0, in_len_up - out_len_down + p0 - (up - 1)


def backward64(case, codes, dy, flip):
    """dx of the op for the output gradient dy, in float64: the transposed down-FIR of dy, times the coded factor, through the transposed
    up-FIR.  The transpose of upfirdn2d(up u, down d, filter f, pads p, flip) is upfirdn2d(up d, down u, f, mirrored pads, not flip)."""
    fu, fd = make_filter(case['fu'], 'bias8' in case), make_filter(case['fd'], 'bias8' in case)
    fus, fds = filter_shape(case['fu']), filter_shape(case['fd'])
    up, down, p = case['up'], case['down'], case['pad']
    (zh, zw), (oh, ow), (xh, xw) = z_hw(case), out_hw(case), case['shape'][2:]
    px = _adjoint_pad(fds[-1], zw, ow * down, 0, 1)
    py = _adjoint_pad(fds[0], zh, oh * down, 0, 1)
    dz = oracle_ops.upfirdn2d(dy.double(), fd, up=down, padding=[*px, *py], flip_filter=not flip)
    assert tuple(dz.shape[2:]) == (zh, zw)
    dz = dz * code_factor(case, codes)
    px = _adjoint_pad(fus[-1], xw * up, zw, p[0], up)
    py = _adjoint_pad(fus[0], xh * up, zh, p[2], up)
    dx = oracle_ops.upfirdn2d(dz, fu, down=up, padding=[*px, *py], flip_filter=not flip, gain=up ** 2)
    assert tuple(dx.shape[2:]) == (xh, xw)
    return dx


def coded_forward64(case, codes, w, flip):
    """The op with its activation replaced by the coded factor (no bias): the transpose of `backward64`, i.e. the second-order term."""
    fu, fd = make_filter(case['fu'], 'bias8' in case), make_filter(case['fd'], 'bias8' in case)
    z = oracle_ops.upfirdn2d(w.double(), fu, up=case['up'], padding=case['pad'], gain=case['up'] ** 2, flip_filter=flip) * code_factor(case, codes)
    return oracle_ops.upfirdn2d(z, fd, down=case['down'], flip_filter=flip)


def pack_codes(codes, bytes_per_row):
    """[n, c, h, w] codes -> [n, c, h, bytes_per_row] bytes: element 4k + j in bits 2j .. 2j + 1 of byte k, zero codes past w."""
    codes = codes.numpy() if isinstance(codes, torch.Tensor) else codes
    n, c, h, w = codes.shape
    full = np.zeros((n, c, h, bytes_per_row * 4), dtype=np.uint8)
    full[..., :w] = codes
    return (full[..., 0::4] | (full[..., 1::4] << 2) | (full[..., 2::4] << 4) | (full[..., 3::4] << 6)).astype(np.uint8)


def unpack_codes(packed):
    packed = packed.cpu().numpy() if isinstance(packed, torch.Tensor) else packed
    return np.stack([(packed >> (2 * j)) & 3 for j in range(4)], axis=-1).reshape(*packed.shape[:3], -1)


def dyadic_inputs(case, seed):
    """x in multiples of 1/4 within [-1.5, 1.5], bias in eighths: exact in fp16, bf16 and fp32."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randint(-6, 7, case['shape'], generator=g).float() / 4
    b = torch.tensor(case['bias8'], dtype=torch.float32) / 8
    assert b.numel() == case['shape'][1]
    return x, b


def dyadic_grad(shape, seed):
    """Output gradient in multiples of 1/4 with a non-zero mean (so that its sum, the bias gradient, is not a cancellation)."""
    return torch.randint(-2, 7, tuple(shape), generator=torch.Generator().manual_seed(seed)).float() / 4
