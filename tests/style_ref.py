"""Float64 references of the style preparation (csrc/style.hip) with per-element rounding bounds, from the formulas the kernels replace
(`SynthesisLayer` / the output heads in training/networks.py, quoted at the top of style.hip):

    styles[n, i]  = (sum_k w[n, k] A[i, k]) * a_gain + b[i] * b_gain
    dcoefs[n, o]  = rsqrt(sum_i styles[n, i]^2 * wsq_t[i, o] + 1e-8)            wsq_t[i, o] = sum over the taps of W[o, i]^2
    folded[n, o, i] = W_head[o, i] * (styles_head[n, i] * gain_head)            (the heads' affine has bias gain 1)

Inputs are the float32 tensors the kernels get, widened; gains are the float32 values the ABI receives.  u = 2^-24; a "1 ulp" device
function (`rsqrtf`) counts as 2 u.

styles:   |got - ref| <= (D + 4) u |scale| (a_gain * sum_k |w_k A_ik| + b_gain |b_i|) + 1e-30
  D is the depth of the dot product on the path taken; the 4 are * a_gain, b * b_gain, +, * scale.  The path (`is_vec`, the routing
  condition of `affine_rows` restated): 16-byte loads when w_dim is a multiple of 4 and the affine weight is 16-byte aligned, else scalar.
    vector path: a lane sums groups of four columns, one group per 256-column slab: product, two levels of pair sum (3), one accumulation
                 per slab (ceil(w_dim / 256)), then the 6-level tree across the 64 lanes:   D = 9 + ceil(w_dim / 256)
    scalar path: a lane sums columns lane, lane + 64, ... in order: the product (1) and one accumulation per term (ceil(w_dim / 64)), then
                 the tree:                                                                   D = 7 + ceil(w_dim / 64)

dcoefs, from the kernel's OWN styles output (float32 bits, widened: telescoped like the mapping layers): every term of the sum is
non-negative, so the error of the sum is relative to it:
    the square (1), its product with wsq_t (1), a thread's running sum over its ceil(cin / 32) channels, the sum of the 32 threads' parts
    (31 additions), + 1e-8 (1):  34 + ceil(cin / 32) roundings on the argument, which rsqrt halves;  `rsqrtf` 2 u, and 1 u of margin for the
    second order:
    |got - ref| <= ((34 + ceil(cin / 32)) / 2 + 3) u ref

folded heads:  |got - W s64| <= |W| E_s + u |W s64|,  E_s the styles bound with scale = gain_head and b_gain = 1: the one product after the
styles rounds once.
"""

import math

import numpy as np
import torch

U = 2.0 ** -24
TINY = 1e-30
STYLE_ROWS, FOLD_CI, DEMOD_MAX_CI, DEMOD_MAX_N, BATCH_MAX = 32, 64, 512, 8, 24


def f32(v):
    return float(np.float32(v))


def cdiv(a, b):
    return -(-a // b)


def is_vec(wdim, affine_ptr):
    """`affine_rows`' routing: 16-byte loads need w_dim % 4 == 0 and a 16-byte aligned weight (row blocks start at multiples of
    32 or 64 rows of w_dim floats: they keep the alignment of the base)."""
    return wdim % 4 == 0 and affine_ptr % 16 == 0


def affine_depth(wdim, vec):
    return 9 + cdiv(wdim, 256) if vec else 7 + cdiv(wdim, 64)


def demod_chunks(cin):
    """Passes of `style_demod_body` over its channel range (DEMOD_MAX_CI channels per pass)."""
    return cdiv(cin, DEMOD_MAX_CI)


def demod_groups(n):
    """Launches of the per-layer demodulation (DEMOD_MAX_N images each)."""
    return cdiv(n, DEMOD_MAX_N)


def styles(w, A, b, a_gain, b_gain, vec, scale=1.0):
    """w [n, wdim], A [cin, wdim], b [cin] | None (float32) -> (ref, bound) float64 [n, cin]."""
    ag, bg, sc = f32(a_gain), f32(b_gain), f32(scale)
    w64, A64 = w.double(), A.double()
    ref = (w64 @ A64.t()) * ag
    mag = (w64.abs() @ A64.abs().t()) * ag
    if b is not None:
        ref = ref + b.double() * bg
        mag = mag + b.double().abs() * bg
    bound = (affine_depth(w.shape[1], vec) + 4) * U * abs(sc) * mag + TINY
    return ref * sc, bound


def dcoefs(styles32, wsq_t):
    """styles32 [n, cin]: the kernel's own output; wsq_t [cin, cout] float32 -> (ref, bound) float64 [n, cout]."""
    cin = styles32.shape[1]
    ref = (styles32.double().square() @ wsq_t.double() + 1e-8).rsqrt()
    return ref, ((34 + cdiv(cin, 32)) / 2 + 3) * U * ref


def fold_heads(w, a_gain, A0, b0, W0, g0, vec0, A1, b1, W1, g1, vec1):
    """-> (ref, bound) float64 [n, cout0 + cout1, cin]."""
    refs, bounds = [], []
    for A, b, W, g, vec in ((A0, b0, W0, g0, vec0), (A1, b1, W1, g1, vec1)):
        s, e = styles(w, A, b, a_gain, 1.0, vec, scale=g)
        W64 = W.double()
        r = W64[None] * s[:, None, :]
        refs.append(r); bounds.append(W64.abs()[None] * e[:, None, :] + U * r.abs())
    return torch.cat(refs, dim=1), torch.cat(bounds, dim=1)
