"""Float64 (and longdouble) restatement of the metric sums of training/metrics.py, written from the formulas of DESIGN.md section 5.34, and
the error bounds the GPU tests hold csrc/metrics.hip to.  Nothing here calls the product."""
import numpy as np

EPS32 = 2.0 ** -24          # half an ulp of 1 in fp32: the relative error of one fp32 rounding


def features(kind, n, d, seed):
    """Seeded fp32 features: 'gauss' randn; 'relu' max(randn + 0.5, 0) (large norms against small distances); 'dup' gauss with rows 10..14
    equal to row 9."""
    rng = np.random.RandomState(seed)
    x = rng.randn(n, d)
    if kind == 'relu':
        x = np.maximum(x + 0.5, 0)
    x = x.astype(np.float32)
    if kind == 'dup':
        x[10:15] = x[9]
    return x


def probes_for(kind, manifold, count, seed):
    """Probes of the same kind; 'dup': probes 0..6 equal manifold rows 0..6, probes 7..19 = manifold rows 20..32 + 1e-3 randn."""
    p = features('gauss' if kind == 'dup' else kind, count, manifold.shape[1], seed)
    if kind == 'dup':
        p[0:7] = manifold[0:7]
        p[7:20] = manifold[20:33] + (1e-3 * np.random.RandomState(seed + 1).randn(13, manifold.shape[1])).astype(np.float32)
    return p


# ---- moments ----------------------------------------------------------------------------------------------------------------------

def moments(x):
    """-> (column sums, x^T x, sum_i |x_ij x_ik|) of fp32 rows in longdouble."""
    xl = x.astype(np.longdouble)
    return xl.sum(axis=0), xl.T @ xl, np.abs(xl).T @ np.abs(xl)


# ---- polynomial kernel sums -------------------------------------------------------------------------------------------------------

def poly_sums(x, y, xi, yi):
    """-> (sums [subsets, 3], bounds [subsets, 3]): the three sums of p = (dot / d + 1)^3 in float64 and, for a dot product that is a chain of
    d fp32 FMAs, sum 3 (|t| + 1)^2 delta (1 + 1e-3) with t = dot / d and delta = (d + 2) 2^-24 sum_k |x_ik y_jk| / d over the same pairs."""
    x64, y64 = x.astype(np.float64), y.astype(np.float64)
    d = x.shape[1]
    sums, bounds = np.zeros([len(xi), 3]), np.zeros([len(xi), 3])
    for s in range(len(xi)):
        a, b = x64[np.clip(xi[s], 0, len(x) - 1)], y64[np.clip(yi[s], 0, len(y) - 1)]
        m = len(a)
        off = 1.0 - np.eye(m)
        for w, (u, v, mask) in enumerate(((a, a, off), (b, b, off), (a, b, np.ones([m, m])))):
            t = u @ v.T / d
            delta = (d + 2) * EPS32 * (np.abs(u) @ np.abs(v).T) / d
            sums[s, w] = ((t + 1) ** 3 * mask).sum()
            bounds[s, w] = (3 * (np.abs(t) + 1) ** 2 * delta * mask).sum() * (1 + 1e-3)
    return sums, bounds


def kid_from_sums(sums, m):
    t = 0.0
    for sxx, syy, sxy in sums:
        t += (sxx + syy) / (m - 1) - sxy * 2 / m
    return t / len(sums) / m


# ---- distances, radii, membership -------------------------------------------------------------------------------------------------

def d2(a, b):
    """[na, nb] squared distances of fp32 rows in float64, as sums of squared differences (0 exactly for equal rows)."""
    a64, b64 = a.astype(np.float64), b.astype(np.float64)
    out = np.empty([len(a), len(b)])
    for i in range(len(a)):
        out[i] = np.square(a64[i][None, :] - b64).sum(axis=1)
    return out


def tau(a, b):
    """[na, nb]: (d + 8) 2^-24 (|a|^2 + |b|^2): the dot product's d 2^-24 sum |a_k b_k| <= d 2^-25 (|a|^2 + |b|^2) taken twice, the two norm
    roundings, the sum and the difference."""
    na, nb = np.square(a.astype(np.float64)).sum(axis=1), np.square(b.astype(np.float64)).sum(axis=1)
    return (a.shape[1] + 8) * EPS32 * (na[:, None] + nb[None, :])


def radii(f, k):
    """-> (r64 [n], bound [n]): the (k + 1)-th smallest of row i of d2(f, f) (the row holds the point itself at 0) and max_j tau(i, j): an
    order statistic moves no further than its inputs."""
    dist = d2(f, f)
    return np.sort(dist, axis=1)[:, k], tau(f, f).max(axis=1)


def membership(probes, manifold, r64):
    """-> (inside [np] bool, decided [np] bool).  Decided inside: some j has d2 <= r64_j - tol(p, j); decided outside: every j has
    d2 > r64_j + tol(p, j); tol(p, j) = tau(p, j) + max_i tau(j, i) covers the distance's and the radius's error."""
    dist = d2(probes, manifold)
    tol = tau(probes, manifold) + tau(manifold, manifold).max(axis=1)[None, :]
    sure_in = (dist <= r64[None, :] - tol).any(axis=1)
    sure_out = (dist > r64[None, :] + tol).all(axis=1)
    return (dist <= r64[None, :]).any(axis=1), sure_in | sure_out


def precision_recall(real, gen, k):
    out = []
    for manifold, probes in ((real, gen), (gen, real)):
        out.append(float(membership(probes, manifold, radii(manifold, k)[0])[0].mean()))
    return tuple(out)


# ---- Frechet distance -------------------------------------------------------------------------------------------------------------

def mean_cov(x):
    x64 = x.astype(np.float64)
    mean = x64.mean(axis=0)
    return mean, x64.T @ x64 / len(x) - np.outer(mean, mean)
