"""Float64 reference of the mapping network, one stage at a time, with a per-element rounding bound for each stage.

Written from the definition (`training/networks.py`: `normalize_2nd_moment`, `FullyConnectedLayer`, `MappingNetwork.forward` / `_truncate`),
not from csrc/mapping.hip.  Inputs are the float32 tensors the kernel gets, widened; gains are the float32 values the C ABI receives
(`float32(lr_multiplier)`, `float32(alpha)`, `float32(sqrt 2)`), widened, so the reference answers the question the kernel was asked.

u = 2^-24 is one rounding to nearest.  A result the device documents as "1 ulp" (`rsqrtf`) is counted as 2 u.

One layer:  y_i = lrelu(wg * sum_k x_k W_ik + bg * b_i) * gain,  wg = lr / sqrt(K),  bg = lr.

    |got - ref| <= LAYER_ROUNDINGS * u * gain * (wg * A_i + bg * |b_i|) + 1e-30,      A_i = sum_k |x_k W_ik|

Count for a sum formed 4 columns at a time per lane of a 64-lane wave, at most 4 such groups per lane (K <= 1024), then a 6-level tree:
  * 4 per group of 4: the product, two levels of the pair sum, the accumulation into the lane's running sum;
  * 3 further accumulations of the lane's at most 4 groups;
  * 6 for the tree across the 64 lanes;
  * 3 for wg: `rsqrtf(K)` is 1 ulp = 2 u, its product with lr 1 more (3, not 2: 1 ulp is up to 2 u);
  * 5 for the epilogue: * wg, b * bg, +, * alpha, * gain.  lrelu does not enlarge an error (slope <= 1, continuous at 0).
That is 21; 24 keeps 3 for the second-order terms (24 u * 21 u is far below 1 u) and for products contracted into sums, which only remove
roundings.  Every partial sum is at most A_i in magnitude, so each rounding is at most u * A_i * wg * gain after the scaling.

Input stage.  z half, x = z * rsqrt(mean(z^2) + 1e-8): all terms of the sum of squares are non-negative, so its error is relative:
  * at most 4 squares per thread (K <= 1024 over 256 threads): 1 for the square, 3 for the thread's running sum;
  * 6 for the tree of a wave, 4 for the sum of the 4 waves' results;
  * 1 for the division by z_dim, 1 for + 1e-8:  16 u on the argument, which rsqrt halves to 8 u;
  * 2 for `rsqrtf`, 1 for the product with z:  11 u, taken as Z_ROUNDINGS = 12 with 1 for the second order.
Embedding half, v = wgain * sum_k c_k W_ek + bgain * b_e before its normalisation: a sequential sum of c_dim products (c_dim roundings
with contraction, counted as c_dim), * wgain, b * bgain, + : (c_dim + 3) u * (wgain * sum |c W| + bgain * |b|) = Ev.  Through
y = v / r, r = sqrt(mean(v^2) + 1e-8), to first order  |dy_e| <= Ev_e / r + |v_e| * sum_k |v_k| Ev_k / (E r^3);  the normalisation's own
roundings add Z_ROUNDINGS * u * |y_e| as for z.  E0 enters layer 0's bound as gain * wg * sum_k |W_ik| E0_k (lrelu and the scaling are
Lipschitz with these constants).

Truncation (`ws[:, :cutoff] = w_avg.lerp(ws[:, :cutoff], psi)`), against the kernel's own last activation x_L:
    |got - lerp64(w_avg, x_L, psi32)| <= 4 u (|w_avg| + |x_L|) max(1, |psi|, |1 - psi|)
ATen's lerp is a + psi * d for |psi| < 0.5 and v - d * (1 - psi) otherwise, d = v - a: the difference, the product, the sum are 3 roundings
of quantities of at most (|a| + |v|) max(|psi|, |1 - psi|, 1), the second form rounds 1 - psi as well: 4.
"""

import math

import numpy as np
import torch

U = 2.0 ** -24
LAYER_ROUNDINGS = 24
Z_ROUNDINGS = 12
TRUNC_ROUNDINGS = 4
TINY = 1e-30


def f32(v):
    """The float32 value the ABI receives for a Python number, as a Python float."""
    return float(np.float32(v))


def input_stage(z, c, embed_w, embed_b, embed_wgain, embed_bgain):
    """z [n, z_dim], c [n, c_dim] | None, embed_w [embed, c_dim] | None (float32) -> (x0, E0) float64 [n, z_dim + embed]."""
    xs, es = [], []
    if z.shape[1] > 0:
        z64 = z.double()
        x = z64 * (z64.square().mean(dim=1, keepdim=True) + 1e-8).rsqrt()
        xs.append(x); es.append(Z_ROUNDINGS * U * x.abs())
    if embed_w is not None:
        c64, w64 = c.double(), embed_w.double()
        wg, bg = f32(embed_wgain), f32(embed_bgain)
        v = (c64 @ w64.t()) * wg
        mag = (c64.abs() @ w64.abs().t()) * wg
        if embed_b is not None:
            v = v + embed_b.double() * bg
            mag = mag + embed_b.double().abs() * bg
        ev = (c.shape[1] + 3) * U * mag
        E = v.shape[1]
        r = (v.square().mean(dim=1, keepdim=True) + 1e-8).sqrt()
        y = v / r
        ey = ev / r + v.abs() * (v.abs() * ev).sum(dim=1, keepdim=True) / (E * r ** 3) + Z_ROUNDINGS * U * y.abs()
        xs.append(y); es.append(ey)
    return torch.cat(xs, dim=1), torch.cat(es, dim=1)


def layer(x, w, b, lr_multiplier, alpha, act_gain, e_in=None):
    """One lrelu FullyConnectedLayer in float64.  x [n, K] float64 (the kernel's own previous activation, or x0), w [O, K], b [O] | None
    float32 -> (y, bound) float64 [n, O].  `e_in`: a bound on the error of x (the input stage's E0), carried into the bound."""
    K = w.shape[1]
    lr, al, gn = f32(lr_multiplier), f32(alpha), f32(act_gain)
    wg = lr / math.sqrt(K)
    w64 = w.double()
    pre = (x @ w64.t()) * wg
    mag = (x.abs() @ w64.abs().t()) * wg
    if b is not None:
        pre = pre + b.double() * lr
        mag = mag + b.double().abs() * lr
    y = torch.where(pre > 0, pre, pre * al) * gn
    bound = LAYER_ROUNDINGS * U * gn * mag + TINY
    if e_in is not None:
        bound = bound + gn * wg * (e_in @ w64.abs().t())
    return y, bound


def slice_cutoff(cutoff, num_ws):
    """How many leading rows `ws[:, :cutoff]` selects (a Python slice: None = all, negative counts from the end)."""
    return len(range(num_ws)[:cutoff])


def truncate(x_last, w_avg, psi, cutoff, num_ws):
    """x_last [n, w] (float32: the kernel's own activation), w_avg [w] -> (ref float64 [n, num_ws, w], bound, truncated [num_ws] bool).
    Rows that are not truncated are copies of x_last: bound 0 there."""
    n, wd = x_last.shape
    x64 = x_last.double()[:, None, :].expand(n, num_ws, wd)
    trunc = torch.zeros(num_ws, dtype=torch.bool)
    if f32(psi) != 1.0:
        trunc[:slice_cutoff(cutoff, num_ws)] = True
    p = f32(psi)
    a = w_avg.double()
    lerp = a + p * (x64 - a)
    ref = torch.where(trunc[None, :, None], lerp, x64)
    bound = TRUNC_ROUNDINGS * U * (a.abs() + x64.abs()) * max(1.0, abs(p), abs(1.0 - p))
    bound = torch.where(trunc[None, :, None], bound, torch.zeros_like(bound))
    return ref, bound, trunc


def forward(z, c, embed_w, embed_b, embed_wgain, embed_bgain, fc_ws, fc_bs, lr_multiplier, alpha, act_gain, num_ws, w_avg, psi, cutoff):
    """The whole network in float64 (no bounds): what `MappingNetwork.forward` defines."""
    x, _ = input_stage(z, c, embed_w, embed_b, embed_wgain, embed_bgain)
    for w, b in zip(fc_ws, fc_bs):
        x, _ = layer(x, w, b, lr_multiplier, alpha, act_gain)
    ws = x[:, None, :].repeat(1, num_ws, 1)
    if f32(psi) != 1.0:
        k = slice_cutoff(cutoff, num_ws)
        a = w_avg.double()
        ws[:, :k] = a + f32(psi) * (ws[:, :k] - a)
    return ws
