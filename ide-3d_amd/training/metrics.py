"""Generator metrics on detector features: what `calc_metrics.py` does once a detector has turned images into features (FID, KID and
precision / recall: metrics/frechet_inception_distance.py, kernel_inception_distance.py, precision_recall.py and the `FeatureStats` of
metrics/metric_utils.py:84-160), with the sums over features on the device (csrc/metrics.hip).

The detectors themselves are not here: every function takes a detector as a callable the user loads, like the loss networks.

Definitions (every function below has a numpy float64 form in this module; CPU tensors and numpy arrays take it, float32 CUDA tensors take
the kernels):

  moments    raw_mean[j] = sum_i x[i,j], raw_cov[j,k] = sum_i x[i,j] x[i,k] in float64; mean = raw_mean / N, cov = raw_cov / N - mean mean^T
             (the reference's, not the unbiased estimate).
  FID        |mu_a - mu_b|^2 + tr S_a + tr S_b - 2 tr (S_a S_b)^(1/2), the last term as sum_i sqrt(lambda_i(S_b^(1/2) S_a S_b^(1/2))):
             the same spectrum as S_a S_b, but of a symmetric matrix, so `eigh` does it (negative eigenvalues, which only rounding
             produces, count as 0).  Host, float64, no scipy.
  KID        per subset of m rows of each set (gen drawn before real, `choice(n, m, replace=False)`), with p(a, b) = (a.b / d + 1)^3:
             t += (sum_{i != j} p(x_i, x_j) + sum_{i != j} p(y_i, y_j)) / (m - 1) - 2 sum_{i,j} p(x_i, y_j) / m; KID = t / subsets / m.
             The device computes a.b in fp32 on the matrix cores and everything after it in float64.
  radii      radii_sq[i] = the (k + 1)-th smallest over j of d2(f_i, f_j), j == i counting as exactly 0.
  inside     inside[p] = any_j d2(probe_p, manifold_j) <= radii_sq[j].
  d2         max(0, |a|^2 + |b|^2 - 2 a.b).  On the device in fp32 with float64 norms rounded once.  NO fp16 anywhere: the reference
             casts the features to fp16 and rounds the radii to fp16 (precision_recall.py:42-53); this module does not reproduce that.
"""

import pickle

import numpy as np
import torch

from torch_utils import hip_plugin

_ROW_BATCH = 2048          # rows per block of the host definitions' distance matrices


def _on_device(x):
    return isinstance(x, torch.Tensor) and x.is_cuda and x.dtype == torch.float32


def _f64(x):
    """Any [n, d] tensor or array as a numpy float64 array."""
    if isinstance(x, torch.Tensor):
        x = x.detach().cpu().numpy()
    x = np.asarray(x, dtype=np.float64)
    if x.ndim != 2:
        raise ValueError(f'features must be [n, d], got shape {x.shape}')
    return x


def _rows(x):
    """A float32 CUDA feature tensor the kernels take: [n, d] with contiguous rows."""
    if x.ndim != 2:
        raise ValueError(f'features must be [n, d], got shape {tuple(x.shape)}')
    x = x.detach()
    return x if (x.stride(1) == 1 and x.stride(0) >= x.shape[1]) else x.contiguous()


# ---- feature statistics -----------------------------------------------------------------------------------------------------------

class FeatureStats:
    """metric_utils.FeatureStats (metrics/metric_utils.py:84-160) with the same attributes, truncation and pickles.  A float32 CUDA tensor
    given to `append_torch` stays on the device: the captured features are kept there and `raw_mean` / `raw_cov` become float64 device
    tensors that `ide3d_feature_moments` updates in place.  Everything else takes the reference's numpy float64 arithmetic."""

    def __init__(self, capture_all=False, capture_mean_cov=False, max_items=None):
        self.capture_all = capture_all
        self.capture_mean_cov = capture_mean_cov
        self.max_items = max_items
        self.num_items = 0
        self.num_features = None
        self.all_features = None
        self.raw_mean = None
        self.raw_cov = None

    def set_num_features(self, num_features):
        if self.num_features is not None:
            assert num_features == self.num_features
        else:
            self.num_features = num_features
            self.all_features = []
            self.raw_mean = np.zeros([num_features], dtype=np.float64)
            self.raw_cov = np.zeros([num_features, num_features], dtype=np.float64)

    def is_full(self):
        return (self.max_items is not None) and (self.num_items >= self.max_items)

    def _truncate(self, x):
        if (self.max_items is not None) and (self.num_items + x.shape[0] > self.max_items):
            if self.num_items >= self.max_items:
                return None
            x = x[:self.max_items - self.num_items]
        return x

    def _moments_to(self, device):
        """Move the running sums to `device` (None: the host, as numpy) without changing a bit."""
        if device is None:
            if isinstance(self.raw_mean, torch.Tensor):
                self.raw_mean, self.raw_cov = self.raw_mean.cpu().numpy(), self.raw_cov.cpu().numpy()
        elif not isinstance(self.raw_mean, torch.Tensor) or self.raw_mean.device != device:
            self.raw_mean = torch.as_tensor(self.raw_mean, dtype=torch.float64).to(device).contiguous()
            self.raw_cov = torch.as_tensor(self.raw_cov, dtype=torch.float64).to(device).contiguous()

    def append(self, x):
        x = np.asarray(x, dtype=np.float32)
        assert x.ndim == 2
        x = self._truncate(x)
        if x is None:
            return
        self.set_num_features(x.shape[1])
        self.num_items += x.shape[0]
        if self.capture_all:
            self.all_features.append(x)
        if self.capture_mean_cov:
            self._moments_to(None)
            x64 = x.astype(np.float64)
            self.raw_mean += x64.sum(axis=0)
            self.raw_cov += x64.T @ x64

    def append_torch(self, x, num_gpus=1, rank=0):
        assert isinstance(x, torch.Tensor) and x.ndim == 2
        assert 0 <= rank < num_gpus
        if num_gpus > 1:
            raise NotImplementedError('FeatureStats.append_torch: the feature exchange between GPUs (num_gpus > 1) is not implemented; '
                                      'collect per-rank statistics and add their raw sums')
        if not _on_device(x):
            self.append(x.detach().cpu().numpy())
            return
        x = self._truncate(x)
        if x is None or x.shape[0] == 0:
            return
        x = _rows(x)
        self.set_num_features(int(x.shape[1]))
        self.num_items += int(x.shape[0])
        if self.capture_all:
            self.all_features.append(x.clone())
        if self.capture_mean_cov:
            self._moments_to(x.device)
            hip_plugin.MetricsPlugin.feature_moments(x, self.raw_mean, self.raw_cov)

    def get_all(self):
        assert self.capture_all
        return np.concatenate([f.cpu().numpy() if isinstance(f, torch.Tensor) else f for f in self.all_features], axis=0)

    def get_all_torch(self):
        assert self.capture_all
        devs = [f.device for f in self.all_features if isinstance(f, torch.Tensor)]
        if not devs:
            return torch.from_numpy(self.get_all())
        return torch.cat([f if isinstance(f, torch.Tensor) else torch.from_numpy(f).to(devs[0]) for f in self.all_features], dim=0)

    def get_mean_cov(self):
        assert self.capture_mean_cov
        raw_mean, raw_cov = (t.cpu().numpy() if isinstance(t, torch.Tensor) else t for t in (self.raw_mean, self.raw_cov))
        mean = raw_mean / self.num_items
        cov = raw_cov / self.num_items
        cov = cov - np.outer(mean, mean)
        return mean, cov

    def save(self, pkl_file):
        """The reference's pickle: its attribute names, numpy arrays only, so either side loads the other's file."""
        state = dict(self.__dict__)
        if state['all_features'] is not None:
            state['all_features'] = [f.cpu().numpy() if isinstance(f, torch.Tensor) else f for f in state['all_features']]
        for name in ('raw_mean', 'raw_cov'):
            if isinstance(state[name], torch.Tensor):
                state[name] = state[name].cpu().numpy()
        with open(pkl_file, 'wb') as f:
            pickle.dump(state, f)

    @staticmethod
    def load(pkl_file):
        with open(pkl_file, 'rb') as f:
            s = dict(pickle.load(f))
        obj = FeatureStats(capture_all=s['capture_all'], max_items=s['max_items'])
        obj.__dict__.update(s)
        return obj


# ---- FID --------------------------------------------------------------------------------------------------------------------------

def _psd_sqrt(s):
    lam, v = np.linalg.eigh((s + s.T) * 0.5)
    return (v * np.sqrt(np.clip(lam, 0, None))) @ v.T


def frechet_distance(mu_a, sigma_a, mu_b, sigma_b):
    """Squared Frechet distance of two Gaussians in numpy float64 (frechet_inception_distance.py:36-39 without scipy's sqrtm)."""
    mu_a, mu_b = np.asarray(mu_a, np.float64), np.asarray(mu_b, np.float64)
    sigma_a, sigma_b = np.asarray(sigma_a, np.float64), np.asarray(sigma_b, np.float64)
    root_b = _psd_sqrt(sigma_b)
    mid = root_b @ sigma_a @ root_b
    lam = np.linalg.eigvalsh((mid + mid.T) * 0.5)
    return float(np.square(mu_a - mu_b).sum() + np.trace(sigma_a) + np.trace(sigma_b) - 2 * np.sqrt(np.clip(lam, 0, None)).sum())


def fid(stats_real, stats_gen):
    mu_real, sigma_real = stats_real.get_mean_cov()
    mu_gen, sigma_gen = stats_gen.get_mean_cov()
    return frechet_distance(mu_gen, sigma_gen, mu_real, sigma_real)


# ---- KID --------------------------------------------------------------------------------------------------------------------------

def poly_kernel_sums_host(x, y, xi, yi):
    """The numpy float64 definition: [subsets, 3] sums for x[xi[s]] and y[yi[s]] (indices clamped into range)."""
    x, y = _f64(x), _f64(y)
    xi = np.clip(np.asarray(xi, np.int64), 0, x.shape[0] - 1)
    yi = np.clip(np.asarray(yi, np.int64), 0, y.shape[0] - 1)
    d = x.shape[1]
    out = np.zeros([xi.shape[0], 3], np.float64)
    for s in range(xi.shape[0]):
        a, b = x[xi[s]], y[yi[s]]
        kxx, kyy, kxy = (a @ a.T / d + 1) ** 3, (b @ b.T / d + 1) ** 3, (a @ b.T / d + 1) ** 3
        out[s] = kxx.sum() - np.trace(kxx), kyy.sum() - np.trace(kyy), kxy.sum()
    return out


def poly_kernel_sums(x, y, xi, yi):
    """-> numpy float64 [subsets, 3]: (sum_{i != j} p(x_i, x_j), sum_{i != j} p(y_i, y_j), sum_{i, j} p(x_i, y_j)) per subset of row
    indices xi, yi [subsets, m].  float32 CUDA features take `ide3d_poly_kernel_sums`, anything else the numpy definition."""
    if not (_on_device(x) and _on_device(y)):
        return poly_kernel_sums_host(x, y, xi, yi)
    x, y = _rows(x), _rows(y)
    xi = torch.as_tensor(np.asarray(xi), dtype=torch.int32).to(x.device).contiguous()
    yi = torch.as_tensor(np.asarray(yi), dtype=torch.int32).to(x.device).contiguous()
    P = hip_plugin.MetricsPlugin
    subsets, m = (int(v) for v in xi.shape)
    ws = P.workspace(P.POLY, m, m, x.shape[1], subsets, x.device)
    sums = torch.empty([subsets, 3], dtype=torch.float64, device=x.device)
    P.poly_kernel_sums(x, y, xi, yi, ws, sums)
    return sums.cpu().numpy()


def kid_from_sums(sums, m):
    """The reference's combination (kernel_inception_distance.py:42-43) of [subsets, 3] sums, in Python float64."""
    t = 0.0
    for sxx, syy, sxy in np.asarray(sums, np.float64).tolist():
        t += (sxx + syy) / (m - 1) - sxy * 2 / m
    return float(t / len(sums) / m)


def kid_indices(num_real, num_gen, num_subsets=100, max_subset_size=1000, rng=None):
    """-> (xi into gen, yi into real), int32 [subsets, m]: the reference's draws, gen before real in every subset."""
    rng = np.random if rng is None else rng
    m = min(min(num_real, num_gen), max_subset_size)
    xi, yi = [], []
    for _ in range(num_subsets):
        xi.append(rng.choice(num_gen, m, replace=False))
        yi.append(rng.choice(num_real, m, replace=False))
    return np.asarray(xi, np.int32).reshape(num_subsets, m), np.asarray(yi, np.int32).reshape(num_subsets, m)


def kid(real, gen, num_subsets=100, max_subset_size=1000, rng=None, indices=None):
    """Kernel inception distance of two feature sets [n, d] (kernel_inception_distance.py:34-44).  `rng`: a numpy RandomState (None: numpy's
    global one, as in the reference); `indices=(xi, yi)` (into gen, into real) overrides the draw."""
    if indices is None:
        indices = kid_indices(real.shape[0], gen.shape[0], num_subsets, max_subset_size, rng)
    xi, yi = indices
    m = int(np.asarray(xi).shape[1])
    if m < 2:
        raise ValueError('kid: subsets need at least 2 rows')
    return kid_from_sums(poly_kernel_sums(gen, real, xi, yi), m)


# ---- precision / recall -----------------------------------------------------------------------------------------------------------

def _d2_host(a, b, na, nb):
    return np.maximum(0.0, (na[:, None] + nb[None, :]) - 2.0 * (a @ b.T))


def knn_radii_host(f, k):
    f = _f64(f)
    n = f.shape[0]
    if not 1 <= k < n:
        raise ValueError(f'knn_radii: k = {k} needs 1 <= k < n = {n}')
    norms = np.square(f).sum(axis=1)
    out = np.empty([n], np.float64)
    for r0 in range(0, n, _ROW_BATCH):
        r1 = min(r0 + _ROW_BATCH, n)
        d2 = _d2_host(f[r0:r1], f, norms[r0:r1], norms)
        d2[np.arange(r1 - r0), np.arange(r0, r1)] = 0.0
        out[r0:r1] = np.partition(d2, k, axis=1)[:, k]
    return out


def manifold_inside_host(probes, manifold, radii_sq):
    probes, manifold = _f64(probes), _f64(manifold)
    radii_sq = np.asarray(radii_sq.detach().cpu().numpy() if isinstance(radii_sq, torch.Tensor) else radii_sq, np.float64)
    npr, nm = np.square(probes).sum(axis=1), np.square(manifold).sum(axis=1)
    out = np.empty([probes.shape[0]], bool)
    for r0 in range(0, probes.shape[0], _ROW_BATCH):
        r1 = min(r0 + _ROW_BATCH, probes.shape[0])
        out[r0:r1] = (_d2_host(probes[r0:r1], manifold, npr[r0:r1], nm) <= radii_sq[None, :]).any(axis=1)
    return out


def knn_radii(f, k=3):
    """-> [n] squared distance of every row to its k-th nearest other row (float32 on the features' device through `ide3d_knn_radii`;
    float64 on the CPU through the numpy definition)."""
    if not _on_device(f):
        return torch.from_numpy(knn_radii_host(f, k))
    f = _rows(f)
    P = hip_plugin.MetricsPlugin
    ws = P.workspace(P.RADII, f.shape[0], f.shape[0], f.shape[1], k, f.device)
    radii_sq = torch.empty([f.shape[0]], dtype=torch.float32, device=f.device)
    P.knn_radii(f, k, ws, radii_sq)
    return radii_sq


def manifold_inside(probes, manifold, radii_sq):
    """-> bool [np]: does the probe lie within the radius of some manifold row."""
    if not (_on_device(probes) and _on_device(manifold)):
        return torch.from_numpy(manifold_inside_host(probes, manifold, radii_sq))
    probes, manifold = _rows(probes), _rows(manifold)
    radii_sq = radii_sq.to(device=probes.device, dtype=torch.float32).contiguous()
    P = hip_plugin.MetricsPlugin
    ws = P.workspace(P.INSIDE, probes.shape[0], manifold.shape[0], probes.shape[1], 0, probes.device)
    inside = torch.empty([probes.shape[0]], dtype=torch.uint8, device=probes.device)
    P.manifold_inside(probes, manifold, radii_sq, ws, inside)
    return inside != 0


def precision_recall(real, gen, nhood_size=3):
    """-> (precision, recall) of precision_recall.py:36-60: the fraction of gen rows inside the manifold of real rows, and of real rows
    inside the manifold of gen rows, a manifold being the balls round its rows out to their `nhood_size`-th neighbour.  Two radii calls and two
    membership calls on fp32 features; the reference's fp16 rounding of the features, the distances and the radii is NOT reproduced."""
    results = []
    for manifold, probes in ((real, gen), (gen, real)):
        radii_sq = knn_radii(manifold, nhood_size)
        results.append(float(manifold_inside(probes, manifold, radii_sq).to(torch.float64).mean()))
    return results[0], results[1]


# ---- the loops that fill a FeatureStats -------------------------------------------------------------------------------------------

def _three_channels(images):
    return images.repeat([1, 3, 1, 1]) if images.shape[1] == 1 else images


def feature_stats_for_generator(G, detector, c_iter, max_items, batch_size=64, batch_gen=None, G_kwargs={}, detector_kwargs={}, **stats_kwargs):
    """The loop of metric_utils.py:262-298: batches of `batch_gen` images from G(z, c) with z ~ N(0, 1) and c from `c_iter`, to uint8,
    `batch_size` at a time through `detector` (any callable on uint8 [N, 3, H, W] images), into a FeatureStats of `max_items` rows."""
    if batch_gen is None:
        batch_gen = min(batch_size, 4)
    assert batch_size % batch_gen == 0
    assert max_items is not None
    device = next(G.parameters()).device
    stats = FeatureStats(max_items=max_items, **stats_kwargs)
    with torch.no_grad():
        while not stats.is_full():
            images = []
            for _i in range(batch_size // batch_gen):
                z = torch.randn([batch_gen, G.z_dim], device=device)
                img = G(z=z, c=next(c_iter), **G_kwargs)
                images.append((img * 127.5 + 128).clamp(0, 255).to(torch.uint8))
            features = detector(_three_channels(torch.cat(images)), **detector_kwargs)
            stats.append_torch(features)
    return stats


def feature_stats_for_images(batches, detector, max_items=None, detector_kwargs={}, **stats_kwargs):
    """The same for an iterable of uint8 image batches [N, C, H, W] (the dataset side of metric_utils.py:244-250)."""
    stats = FeatureStats(max_items=max_items, **stats_kwargs)
    with torch.no_grad():
        for images in batches:
            if stats.is_full():
                break
            stats.append_torch(detector(_three_channels(images), **detector_kwargs))
    return stats
