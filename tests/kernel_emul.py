"""Float32 numpy models of the summation order of csrc/mapping.hip and csrc/style.hip: which lane holds which column, groups of four,
256-column slabs, the xor tree across a wave's 64 lanes, the epilogue's operation order.  They run on the CPU and serve two ends
(tests/test_mapping_style_ref_cpu.py): a correct implementation with this order stays inside the bounds of mapping_ref / style_ref on every
case of the GPU suites, and the same order with one seeded defect leaves them by orders of magnitude.  numpy rounds every float32 operation
(no contraction), so the models have at least the roundings the kernels have.  `defect`: None or one of DEFECTS."""

import numpy as np

F = np.float32
DEFECTS = ('drop_tail_slab', 'bias_next_row', 'skip_lane_63', 'image_clamp')


def _rsqrt(v):
    return (F(1) / np.sqrt(v.astype(F), dtype=F)).astype(F)


def _tree(acc):
    """acc [..., 64]: v += shfl_xor(v, off) for off = 32 .. 1; lane 0's value."""
    lanes = np.arange(64)
    for off in (32, 16, 8, 4, 2, 1):
        acc = (acc + acc[..., lanes ^ off]).astype(F)
    return acc[..., 0]


def _pad(a, k):
    out = np.zeros(a.shape[:-1] + (k,), dtype=F)
    out[..., :a.shape[-1]] = a
    return out


def _dot_vec(x, w, defect=None):
    """x [n, K], w [O, K] -> [n, O]: lane l holds columns 4 l .. 4 l + 3 of every 256-column slab; per slab (p0 + p1) + (p2 + p3) is
    added to the lane's sum; then the tree."""
    K = x.shape[1]
    ns = -(-K // 256)
    if defect == 'drop_tail_slab' and K % 256:
        w = w.copy(); w[:, (K // 256) * 256:] = 0
    xp = _pad(x.astype(F), ns * 256).reshape(x.shape[0], 1, ns, 64, 4)
    wp = _pad(w.astype(F), ns * 256).reshape(1, w.shape[0], ns, 64, 4)
    acc = np.zeros((x.shape[0], w.shape[0], 64), dtype=F)
    for t in range(ns):
        p = (wp[:, :, t] * xp[:, :, t]).astype(F)
        acc = (acc + ((p[..., 0] + p[..., 1]).astype(F) + (p[..., 2] + p[..., 3]).astype(F)).astype(F)).astype(F)
    if defect == 'skip_lane_63':
        acc[..., 63] = 0
    return _tree(acc)


def _dot_scalar(x, w, defect=None):
    """Lane l holds columns l, l + 64, ...: a sequential sum per lane, then the tree."""
    K = x.shape[1]
    ns = -(-K // 64)
    if defect == 'drop_tail_slab' and K % 64:
        w = w.copy(); w[:, (K // 64) * 64:] = 0
    xp = _pad(x.astype(F), ns * 64).reshape(x.shape[0], 1, ns, 64)
    wp = _pad(w.astype(F), ns * 64).reshape(1, w.shape[0], ns, 64)
    acc = np.zeros((x.shape[0], w.shape[0], 64), dtype=F)
    for t in range(ns):
        acc = (acc + (wp[:, :, t] * xp[:, :, t]).astype(F)).astype(F)
    if defect == 'skip_lane_63':
        acc[..., 63] = 0
    return _tree(acc)


def _next_row(b):
    return np.concatenate([b[1:], b[-1:]])


def _block_sum(v):
    """v [n, K]: thread t sums elements t, t + 256, ...; a tree per wave; the 4 waves' sums in order."""
    n, K = v.shape
    per = -(-K // 256)
    vp = _pad(v.astype(F), per * 256).reshape(n, per, 256)
    s = np.zeros((n, 256), dtype=F)
    for j in range(per):
        s = (s + vp[:, j]).astype(F)
    waves = _tree(s.reshape(n, 4, 64))
    t = np.zeros(n, dtype=F)
    for i in range(4):
        t = (t + waves[:, i]).astype(F)
    return t


def _normalize(v):
    sq = (v * v).astype(F)
    s = _rsqrt(((_block_sum(sq) / F(v.shape[1])).astype(F) + F(1e-8)).astype(F))
    return (v * s[:, None]).astype(F)


def mapping_input(z, c, embed_w, embed_b, embed_wgain, embed_bgain):
    parts = []
    if z.shape[1]:
        parts.append(_normalize(z.astype(F)))
    if embed_w is not None:
        acc = np.zeros((c.shape[0], embed_w.shape[0]), dtype=F)
        for k in range(c.shape[1]):
            acc = (acc + (c[:, k:k + 1] * embed_w[None, :, k]).astype(F)).astype(F)
        v = (acc * F(embed_wgain)).astype(F)
        if embed_b is not None:
            v = (v + (embed_b * F(embed_bgain)).astype(F)).astype(F)
        parts.append(_normalize(v))
    return np.concatenate(parts, axis=1)


def mapping_layer(x, w, b, lr_multiplier, alpha, act_gain, defect=None):
    """x [n, K] float32 -> [n, O] float32 in the order of `gemv_block` / `gemv_rows` (the two differ in which wave owns a row, not in a
    row's sum)."""
    n, K = x.shape
    if defect == 'image_clamp' and n > 1:
        x = x.copy(); x[n - 1] = x[n - 2]
    v = _dot_vec(x, w, defect)
    wg = (F(lr_multiplier) * _rsqrt(np.array(K, dtype=F))).astype(F)
    v = (v * wg).astype(F)
    if b is not None:
        bb = _next_row(b) if defect == 'bias_next_row' else b
        v = (v + (bb * F(lr_multiplier)).astype(F)).astype(F)
    v = np.where(v > 0, v, (v * F(alpha)).astype(F)).astype(F)
    return (v * F(act_gain)).astype(F)


def affine(w, A, b, a_gain, b_gain, out_scale, vec, defect=None):
    """styles [n, cin] in the order of `affine_rows` / `affine_rows_half`."""
    acc = (_dot_vec if vec else _dot_scalar)(w, A, defect)
    v = (acc * F(a_gain)).astype(F)
    if b is not None:
        bb = _next_row(b) if defect == 'bias_next_row' else b
        v = (v + (bb * F(b_gain)).astype(F)).astype(F)
    return (v * F(out_scale)).astype(F)


def demod(styles, wsq_t):
    """dcoefs [n, cout]: thread (column, part) sums its channels part, part + 32, ... in order; the 32 parts in order; rsqrt(t + 1e-8)."""
    n, cin = styles.shape
    s2 = (styles * styles).astype(F)
    per = -(-cin // 32)
    s2p = _pad(s2, per * 32).reshape(n, per, 32)
    wp = np.zeros((per * 32, wsq_t.shape[1]), dtype=F); wp[:cin] = wsq_t
    wp = wp.reshape(per, 32, -1)
    acc = np.zeros((n, 32, wsq_t.shape[1]), dtype=F)
    for q in range(per):
        acc = (acc + (s2p[:, q, :, None] * wp[None, q]).astype(F)).astype(F)
    t = np.zeros((n, wsq_t.shape[1]), dtype=F)
    for p in range(32):
        t = (t + acc[:, p]).astype(F)
    return _rsqrt((t + F(1e-8)).astype(F))


def fold(w, a_gain, A0, b0, W0, g0, vec0, A1, b1, W1, g1, vec1, defect=None):
    s0 = affine(w, A0, b0, a_gain, 1.0, g0, vec0, defect)
    s1 = affine(w, A1, b1, a_gain, 1.0, g1, vec1, defect)
    return np.concatenate([(W0[None] * s0[:, None, :]).astype(F), (W1[None] * s1[:, None, :]).astype(F)], axis=1)
