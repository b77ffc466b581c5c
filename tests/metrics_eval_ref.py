"""Float64 / longdouble restatement of the arithmetic of csrc/metrics_eval.hip (PPL, Inception Score, mIoU), written from the definitions
of DESIGN.md section 5.39, the error bounds the GPU tests hold the kernels to, and the inputs the CPU and GPU tests share.  No reference
value here comes from the product; only the sampler's rig at the end builds product modules.

Every bound is first order in the unit roundoffs, times (1 + 1e-3) for the higher orders:
  U32 = 2^-24  the relative error of one fp32 rounding;
  U64 = 2^-53  the same for float64;
  the device's float64 `log` counts as 1 ulp = 2^-52 relative: the HIP math API's documented maximum error of double-precision `log`
  ("log: 1 ULP" in the ROCm HIP math reference table of double-precision functions).
"""
import numpy as np

U32 = 2.0 ** -24
U64 = 2.0 ** -53
LOG_ULP = 2.0 ** -52
SLACK = 1 + 1e-3


# ---- ppl prep ---------------------------------------------------------------------------------------------------------------------

def ppl_prep(x, mean, std, window, f, in_scale, in_shift):
    """-> (y float64 [n, 3, h / f, w / f], bound): y = ((block mean inside the window) * in_scale + in_shift - mean[c]) / std[c].
    The device adds the f^2 fp32 values of a block in order ((f^2 - 1) roundings against the sum of magnitudes), multiplies by fl(1 / f^2)
    (two more), applies one FMA, one subtraction and one division, each rounded once."""
    y0, x0, h, w = window
    x64 = x.astype(np.float64)[:, :, y0:y0 + h, x0:x0 + w]
    n, c = x64.shape[:2]
    blocks = x64.reshape(n, c, h // f, f, w // f, f)
    m, a = blocks.mean(axis=(3, 5)), np.abs(blocks).mean(axis=(3, 5))
    mean64, std64 = (np.asarray(t, np.float32).astype(np.float64).reshape(1, 3, 1, 1) for t in (mean, std))
    s, sh = float(np.float32(in_scale)), float(np.float32(in_shift))
    v = m * s + sh
    d = v - mean64
    y = d / std64
    e_v = abs(s) * (f * f + 1) * U32 * a + U32 * np.abs(v)
    e_d = e_v + U32 * np.abs(d)
    return y, (e_d / np.abs(std64) + U32 * np.abs(y)) * SLACK + 1e-45


# ---- pair distances ---------------------------------------------------------------------------------------------------------------

def pair_taps(shapes, n, seed, zero_pixel=True, identical=False):
    """Seeded raw taps [2 n, c, h, w] (ReLU-like: max(randn + 0.3, 0)) and lin vectors [c] in 0..1; the second half a small step away from
    the first, as in PPL (`identical`: equal to it).  `zero_pixel`: pixel (0, 0) of image 0 is zero in every channel (u = 0 there)."""
    rng = np.random.RandomState(seed)
    taps, lins = [], []
    for c, h, w in shapes:
        a = np.maximum(rng.randn(n, c, h, w) + 0.3, 0)
        b = a if identical else np.maximum(a + 1e-2 * rng.randn(n, c, h, w), 0)
        t = np.concatenate([a, b]).astype(np.float32)
        if zero_pixel:
            t[0, :, 0, 0] = 0
            if identical:
                t[n, :, 0, 0] = 0
        taps.append(t)
        lins.append(rng.rand(c).astype(np.float32))
    return taps, lins


def pair_distances(taps, lins, scale):
    """-> (dist float64 [n], bound [n]).  The device forms u' = fl(a * fl(1 / (|a| + 1e-10))) (|a| from a float64 sum: two fp32 roundings, so
    |u' - u| <= 2 U32 |u|), the difference d' = fl(u'_i - u'_j) (one more, of |d|), and everything after it in float64; the result is
    rounded to fp32 once."""
    s = float(np.float32(scale))
    n = taps[0].shape[0] // 2
    dist, err = np.zeros([n]), np.zeros([n])
    for a, lin in zip(taps, lins):
        a64 = a.astype(np.float64)
        u = a64 / (np.sqrt(np.square(a64).sum(axis=1, keepdims=True)) + 1e-10)
        u0, u1 = u[:n], u[n:]
        d = u0 - u1
        e_d = 2 * U32 * (np.abs(u0) + np.abs(u1)) + U32 * np.abs(d)
        l = np.abs(lin.astype(np.float64)).reshape(1, -1, 1, 1)
        hw = a.shape[2] * a.shape[3]
        terms = l * np.square(d)
        dist += (lin.astype(np.float64).reshape(1, -1, 1, 1) * np.square(d)).sum(axis=(1, 2, 3)) / hw
        err += (l * (2 * np.abs(d) * e_d + np.square(e_d))).sum(axis=(1, 2, 3)) / hw + (a.shape[1] + hw + 64) * U64 * terms.sum(axis=(1, 2, 3)) / hw
    dist, err = dist * s, err * s
    return dist, err * SLACK + U32 * np.abs(dist) + 1e-45


# ---- trimmed mean -----------------------------------------------------------------------------------------------------------------

def percentile_ranks(n):
    return (n - 1) // 100, -((-99 * (n - 1)) // 100)


def trimmed_mean(x, lo_rank, hi_rank):
    """-> (mean longdouble, lo, hi, count, sum of magnitudes of the kept values) by a full sort."""
    s = np.sort(x)
    lo, hi = s[lo_rank], s[hi_rank]
    kept = x[(x >= lo) & (x <= hi)].astype(np.longdouble)
    with np.errstate(invalid='ignore'):
        return kept.sum() / len(kept), float(lo), float(hi), len(kept), float(np.abs(kept).sum())


# ---- inception score --------------------------------------------------------------------------------------------------------------

def softmax_rows(n, d, seed):
    rng = np.random.RandomState(seed)
    z = rng.randn(n, d) * 2
    e = np.exp(z - z.max(axis=1, keepdims=True))
    return (e / e.sum(axis=1, keepdims=True)).astype(np.float32)


def inception_kl(p, splits):
    """-> (kl longdouble [splits], bound [splits]).  Per term p (log p - log m): the two logs at 1 ulp each, m itself a float64 sum of `rows`
    values and a division (an absolute (rows + 1) U64 on its log), the difference and the product rounded once each; then float64 sums of d
    terms per row and of the rows."""
    n, d = p.shape
    kl, bound = np.zeros([splits], np.longdouble), np.zeros([splits])
    for s in range(splits):
        part = p[s * n // splits:(s + 1) * n // splits].astype(np.longdouble)
        rows = len(part)
        logm = np.log(part.mean(axis=0, keepdims=True))
        logp = np.log(part)
        terms = part * (logp - logm)
        kl[s] = terms.sum() / rows
        e_term = part * (np.abs(logp) * LOG_ULP + np.abs(logm) * LOG_ULP + (rows + 1) * U64 + 2 * np.abs(logp - logm) * U64)
        bound[s] = float((e_term.sum() + (d + rows + 300) * U64 * np.abs(terms).sum()) / rows) * SLACK + U64 * abs(float(kl[s]))
    return kl, bound


# ---- label IoU --------------------------------------------------------------------------------------------------------------------

def label_counts(a, b, classes, remap=None):
    """-> (counts int64 [n, classes, 2], iou float64 [n]) from one-hot maps; labels outside the table or outside [0, classes) light no class."""
    a, b = (np.asarray(t).astype(np.int64).reshape(len(t), -1) for t in (a, b))
    if remap is not None:
        table = np.asarray(remap, np.int64)
        a, b = (np.where((m >= 0) & (m < len(table)), table[np.clip(m, 0, len(table) - 1)], -1) for m in (a, b))
    hot = lambda m: (m[:, None, :] == np.arange(classes)[None, :, None])
    ha, hb = hot(a), hot(b)
    inter, union = (ha & hb).sum(axis=2), (ha | hb).sum(axis=2)
    return np.stack([inter, union], axis=2), (inter / (union + 1e-6)).mean(axis=1)


IOU_BOUND = 19 * 2.0 ** -24          # 19 terms in [0, 1], each rounded, and their fp32 sum

REMAP = (0, 1, 6, 7, 4, 5, 2, 2, 10, 11, 12, 8, 9, 15, 3, 17, 16, 18, 13, 14)          # parser ids -> generator ids ('celebahq')


def reference_iou(counts):
    """calc_losses_on_images.py:28-30 from the sums of the one-hot maps, in torch float32."""
    import torch
    inter, union = torch.from_numpy(np.asarray(counts[:, :, 0])), torch.from_numpy(np.asarray(counts[:, :, 1]))
    return torch.mean(torch.div(inter.float(), union.float() + 1e-6), dim=1)


def label_maps(n, h, w, seed, top=20):
    rng = np.random.RandomState(seed)
    a = rng.randint(0, top, size=(n, h, w))
    b = np.where(rng.rand(n, h, w) < 0.7, a, rng.randint(0, top, size=(n, h, w)))
    return a.astype(np.int64), b.astype(np.int64)


def trimmed_cases():
    """Seeded fp32 vectors: n = 1, 2, 100, 101, 1000; ties across both percentile ranks; all equal; one inf; +-0 and negatives."""
    rng = np.random.RandomState(3)
    cases = {f'n{n}': rng.randn(n).astype(np.float32) for n in (1, 2, 100, 101, 1000)}
    ties = rng.randn(300).astype(np.float32)
    s = np.sort(ties)
    ties[ties <= s[4]] = s[2]                   # five equal values across the lo rank (2)
    ties[ties >= s[295]] = s[297]               # five equal values across the hi rank (297)
    cases['ties'] = ties
    cases['equal'] = np.full([257], 1.5, np.float32)
    inf = rng.randn(100).astype(np.float32)
    inf[17] = np.inf
    cases['inf'] = inf
    cases['zeros'] = np.array([0.0, -0.0, 1.0, -1.0, -0.0, 0.0] * 20, np.float32)
    return cases


# ---- the sampler's test rig (the only part of this file that builds product modules; it computes nothing itself) ---------------------

def feature_callable(lp):
    """An `LPIPS` module with the reference detector's call shape: 0..255 images -> the vector whose squared differences sum to LPIPS,
    sqrt(lin / (h w)) u of every tap, concatenated."""
    import torch

    class FeatureCallable(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.lp = lp

        def forward(self, img, resize_images=False, return_lpips=True):
            assert not resize_images and return_lpips
            feats = self.lp.features(img * (2 / 255) - 1)
            return torch.cat([(u * (l[1].weight / (u.shape[2] * u.shape[3])).sqrt()).flatten(1) for u, l in zip(feats, self.lp.lin)], dim=1)

    return FeatureCallable()


def tiny_sampler(vgg16, dev='cpu', **kwargs):
    import torch
    from training import metrics, triplane
    torch.manual_seed(0)
    G = triplane.TriPlaneGenerator(triplane.tiny_spec()).eval().requires_grad_(False).to(dev)
    args = dict(G=G, G_kwargs={}, epsilon=1e-2, space='w', sampling='end', crop=False, vgg16=vgg16)
    args.update(kwargs)
    return metrics.PPLSampler(**args).eval().requires_grad_(False).to(dev)


def camera_labels(n, dev='cpu'):
    import torch
    from training import triplane
    return torch.cat([triplane.camera_label(0.2 * j - 0.1, device=dev) for j in range(n)])
