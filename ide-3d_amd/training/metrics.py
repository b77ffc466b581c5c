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


# ====================================================================================================================================
# Perceptual path length, Inception Score and mIoU (metrics/perceptual_path_length.py, metrics/inception_score.py,
# apps/calc_losses_on_images.py; csrc/metrics_eval.hip).  As above: every function has a host definition that CPU
# tensors and numpy arrays take, and float32 (labels: int64 / uint8) CUDA tensors take the kernels.
#
#   PPL        dist = |lpips(G(w_t)) - lpips(G(w_{t+eps}))|^2 / eps^2 per sample; PPL = the mean of the distances between their 1 % and
#              99 % order statistics (`percentile(..., 'lower')` and `(..., 'higher')`, both ends and their ties kept).
#   IS         per split of the rows of p [n, d]: kl = mean_i sum_j p_ij (log p_ij - log mean_i p_ij); IS = mean and std of exp(kl).
#              A zero probability gives NaN (0 * -inf), as the reference's numpy lines do.
#   mIoU       per image, the mean over ALL classes of |a == c and b == c| / (|a == c or b == c| + 1e-6) in float32.
# ====================================================================================================================================

_MULTI_GPU = ('the feature exchange between GPUs (num_gpus > 1) is not implemented; collect per-rank statistics and add their raw sums')


def _single_gpu(what, num_gpus):
    if num_gpus > 1:
        raise NotImplementedError(f'{what}: {_MULTI_GPU}')


# ---- PPL --------------------------------------------------------------------------------------------------------------------------

def slerp(a, b, t):
    """Spherical interpolation of batches of vectors (perceptual_path_length.py:22-31): both ends normalised, the result on the unit sphere."""
    unit = lambda v: torch.nn.functional.normalize(v, dim=-1, eps=0.0)
    start, end = unit(a), unit(b)
    cosine = torch.linalg.vecdot(start, end, dim=-1).unsqueeze(-1)
    angle = torch.acos(cosine) * t                           # the arc walked from `start`, a fraction t of the angle between the ends
    tangent = unit(end - cosine * start)                     # the unit direction at `start` in the plane of the two, towards `end`
    return unit(torch.cos(angle) * start + torch.sin(angle) * tangent)


def _rgb_of(out):
    """The RGB image of what `G.synthesis` returns (a tensor, a tuple that starts with it, or the `return_dict` form)."""
    if isinstance(out, dict):
        return out['image']
    return out[0] if isinstance(out, (tuple, list)) else out


class PPLSampler(torch.nn.Module):
    """perceptual_path_length.PPLSampler: `forward(c) -> dist [n]` for camera / conditioning labels c [n, c_dim], with the reference's
    constructor arguments and its order of RNG calls (`rand` for t, one `randn([2 n, z_dim]).chunk(2)`, `randn_like` into every
    `*.noise_const` of the sampler's own deep copy of G).  `vgg16`:
      a `training.lpips.LPIPS('vgg')` module - float32 CUDA images then run ide3d_ppl_prep -> the fused feature walk over the 2 n images ->
        ide3d_lpips_pair_distances (13 activations are written, no normalised taps, no feature vector); anything else takes the torch
        definition of the same distance through the module;
      any other callable `vgg16(img_0_255, resize_images=False, return_lpips=True) -> [2 n, F]` (the reference's detector) - the reference's
        lines as torch ops.
    `last_path`: 'hip' or 'torch', the path of the last call."""

    def __init__(self, G, G_kwargs, epsilon, space, sampling, crop, vgg16):
        import copy
        assert space in ['z', 'w']
        assert sampling in ['full', 'end']
        super().__init__()
        self.G = copy.deepcopy(G)
        self.G_kwargs = G_kwargs
        self.epsilon = epsilon
        self.space = space
        self.sampling = sampling
        self.crop = crop
        self.vgg16 = copy.deepcopy(vgg16)
        self.last_path = None

    def images(self, c):
        """The 2 n images of one batch (t first, then t + epsilon), as synthesis returns them."""
        n = c.shape[0]
        t = torch.rand([n], device=c.device) * (1 if self.sampling == 'full' else 0)
        z0, z1 = torch.randn([n * 2, self.G.z_dim], device=c.device).chunk(2)
        if self.space == 'w':
            w0, w1 = self.G.mapping(z=torch.cat([z0, z1]), c=torch.cat([c, c])).chunk(2)
            wt0 = w0.lerp(w1, t.unsqueeze(1).unsqueeze(2))
            wt1 = w0.lerp(w1, t.unsqueeze(1).unsqueeze(2) + self.epsilon)
        else:
            zt0 = slerp(z0, z1, t.unsqueeze(1))
            zt1 = slerp(z0, z1, t.unsqueeze(1) + self.epsilon)
            wt0, wt1 = self.G.mapping(z=torch.cat([zt0, zt1]), c=torch.cat([c, c])).chunk(2)
        for name, buf in self.G.named_buffers():
            if name.endswith('.noise_const'):
                buf.copy_(torch.randn_like(buf))
        kwargs = dict(self.G_kwargs)
        kwargs.setdefault('c', torch.cat([c, c]))          # this synthesis network renders from the camera label
        return _rgb_of(self.G.synthesis(ws=torch.cat([wt0, wt1]), noise_mode='const', force_fp32=True, **kwargs))

    def _window(self, img):
        """(y0, x0, h, w) of the centre crop (perceptual_path_length.py:72-75), or the whole image, and the area factor down to 256."""
        H, W = (int(v) for v in img.shape[2:])
        window = (0, 0, H, W)
        if self.crop:
            assert H == W
            c = H // 8
            window = (c * 3, c * 2, c * 4, c * 4)
        factor = max(self.G.img_resolution // 256, 1)
        return window, factor

    def distances(self, img):
        """dist [n] of 2 n images in -1..1."""
        from training import feature_loss, lpips
        (y0, x0, h, w), f = self._window(img)
        eps2 = self.epsilon ** 2
        lp = self.vgg16
        if not (isinstance(lp, lpips.LPIPS) and type(lp.net) is lpips.VGG16Features):
            # the reference's lines 71-89 for its detector
            img = img[:, :, y0:y0 + h, x0:x0 + w]
            if f > 1:
                img = img.reshape([-1, img.shape[1], img.shape[2] // f, f, img.shape[3] // f, f]).mean([3, 5])
            img = (img + 1) * (255 / 2)
            if img.shape[1] == 1:
                img = img.repeat([1, 3, 1, 1])
            lpips_t0, lpips_t1 = lp(img, resize_images=False, return_lpips=True).chunk(2)
            self.last_path = 'torch'
            return (lpips_t0 - lpips_t1).square().sum(1) / eps2
        if img.shape[1] == 1:
            img = img.repeat([1, 3, 1, 1])
        if (isinstance(img, torch.Tensor) and img.is_cuda and h % f == 0 and w % f == 0 and lp._sides_ok(h // f, w // f)
                and lp._on_hip(img.contiguous())):
            P = hip_plugin.MetricsEvalPlugin
            x = img.detach().contiguous()
            with torch.no_grad():
                saved = feature_loss.forward_walk(feature_loss.HipOps.get(), feature_loss.plan_of(lp.net),
                                                  lambda: P.ppl_prep(x, lp.net.mean, lp.net.std, (y0, x0, h, w), f), False)
                dist = P.lpips_pair_distances(feature_loss.tapped(saved), lp._lin_vectors(), 1.0 / eps2)
            self.last_path = 'hip'
            return dist
        z = lpips._prep_torch(img[:, :, y0:y0 + h, x0:x0 + w], lp.net, f, 1.0, 0.0)
        dist = None
        for a, l in zip(lp.net.taps(z), lp.lin):
            u0, u1 = lpips._Normalize.apply(a).chunk(2)
            d = ((u0 - u1).square() * l[1].weight).sum(dim=1).mean(dim=(1, 2))
            dist = d if dist is None else dist + d
        self.last_path = 'torch'
        return dist / eps2

    def forward(self, c):
        return self.distances(self.images(c))


def percentile_ranks(n):
    """(lo_rank, hi_rank): the positions in sorted order that `np.percentile(x, 1, method='lower')` and `(x, 99, method='higher')` pick
    from n values, in integers."""
    if n < 1:
        raise ValueError('percentile_ranks: no values')
    return (n - 1) // 100, -((-99 * (n - 1)) // 100)


def trimmed_mean_host(x, lo_rank, hi_rank):
    """The numpy float64 definition of ide3d_trimmed_mean -> (mean, lo, hi, count); any NaN in x: (nan, nan, nan, 0)."""
    x = np.asarray(x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else x).reshape(-1)
    if not 0 <= lo_rank <= hi_rank < x.size:
        raise ValueError(f'trimmed_mean: ranks must satisfy 0 <= lo <= hi < n, got {lo_rank}, {hi_rank}, n = {x.size}')
    if np.isnan(x).any():
        return float('nan'), float('nan'), float('nan'), 0
    part = np.partition(x, (lo_rank, hi_rank))
    lo, hi = part[lo_rank], part[hi_rank]
    kept = x[(x >= lo) & (x <= hi)].astype(np.float64)
    with np.errstate(invalid='ignore'):
        return float(kept.sum() / kept.size), float(lo), float(hi), int(kept.size)


def ppl_from_distances(dist):
    """The trimmed mean of perceptual_path_length.py:119-122.  A float32 CUDA vector takes `ide3d_trimmed_mean` and ONE read of its
    mean; CPU tensors and numpy arrays the numpy float64 definition."""
    n = int(dist.numel() if isinstance(dist, torch.Tensor) else np.asarray(dist).size)
    lo_rank, hi_rank = percentile_ranks(n)
    if _on_device(dist):
        out = hip_plugin.MetricsEvalPlugin.trimmed_mean(dist.detach().reshape(-1).contiguous(), lo_rank, hi_rank)
        return float(out[0].item())
    return trimmed_mean_host(dist, lo_rank, hi_rank)[0]


def compute_ppl(G, vgg16, c_iter, num_samples, epsilon, space, sampling, crop, batch_size, G_kwargs={}, num_gpus=1, rank=0):
    """perceptual_path_length.compute_ppl: `num_samples` distances, `batch_size` at a time with labels from `c_iter`, then their trimmed mean.
    The distances stay where the sampler computes them until the one final read."""
    _single_gpu('compute_ppl', num_gpus)
    device = next(G.parameters()).device
    sampler = PPLSampler(G=G, G_kwargs=G_kwargs, epsilon=epsilon, space=space, sampling=sampling, crop=crop, vgg16=vgg16)
    sampler.eval().requires_grad_(False).to(device)
    dist = []
    with torch.no_grad():
        for _batch_start in range(0, num_samples, batch_size):
            dist.append(sampler(next(c_iter)))
    return ppl_from_distances(torch.cat(dist)[:num_samples])


def ppl2_wend(G, vgg16, c_iter, num_samples=50000, G_kwargs={}, num_gpus=1, rank=0):
    """`ppl2_wend` of metrics/metric_main.py: PPL in W at the path end points, full image."""
    return compute_ppl(G, vgg16, c_iter, num_samples=num_samples, epsilon=1e-4, space='w', sampling='end', crop=False, batch_size=2,
                       G_kwargs=G_kwargs, num_gpus=num_gpus, rank=rank)


# ---- Inception Score --------------------------------------------------------------------------------------------------------------

def _check_splits(n, num_splits):
    if num_splits < 1 or n < num_splits:
        raise ValueError(f'inception_score: {n} rows cannot fill {num_splits} splits')


def inception_kl_host(probs, num_splits):
    """The numpy float64 definition -> kl [num_splits] (inception_score.py:31-34 without the exp)."""
    p = _f64(probs)
    n = p.shape[0]
    _check_splits(n, num_splits)
    kl = np.empty([num_splits], np.float64)
    with np.errstate(divide='ignore', invalid='ignore'):
        for i in range(num_splits):
            part = p[i * n // num_splits:(i + 1) * n // num_splits]
            kl[i] = np.mean(np.sum(part * (np.log(part) - np.log(np.mean(part, axis=0, keepdims=True))), axis=1))
    return kl


def inception_kl(probs, num_splits):
    """-> numpy float64 [num_splits]; float32 CUDA probabilities take `ide3d_inception_score`."""
    if not _on_device(probs):
        return inception_kl_host(probs, num_splits)
    p = _rows(probs)
    _check_splits(int(p.shape[0]), num_splits)
    return hip_plugin.MetricsEvalPlugin.inception_score(p, num_splits).cpu().numpy()


def inception_score(probs, num_splits=10):
    """-> (mean, std) of exp(kl) over the splits of probs [n, d] (inception_score.py:30-36)."""
    scores = np.exp(inception_kl(probs, num_splits))
    return float(np.mean(scores)), float(np.std(scores))


def is50k(G, detector, c_iter, num_gen=50000, num_splits=10, batch_size=64, batch_gen=None, G_kwargs={}, num_gpus=1, rank=0):
    """`is50k` of metrics/metric_main.py: `detector` is the Inception network as a callable that returns class probabilities (it receives
    `no_output_bias=True`, as in the reference); the probabilities stay on the device they are computed on."""
    _single_gpu('is50k', num_gpus)
    stats = feature_stats_for_generator(G, detector, c_iter, max_items=num_gen, batch_size=batch_size, batch_gen=batch_gen, G_kwargs=G_kwargs,
                                        detector_kwargs=dict(no_output_bias=True), capture_all=True)
    return inception_score(stats.get_all_torch(), num_splits)


# ---- mIoU -------------------------------------------------------------------------------------------------------------------------

def _labels_np(x):
    x = np.asarray(x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else x).astype(np.int64)
    return x.reshape(x.shape[0], -1)


def label_iou_host(a, b, classes=19, remap=None):
    """The numpy definition -> (iou float32 [n], counts int32 [n, classes, 2]) as CPU tensors."""
    a, b = _labels_np(a), _labels_np(b)
    if a.shape != b.shape:
        raise ValueError(f'label_iou: the maps differ in shape ({a.shape}, {b.shape})')
    if remap is not None:
        table = np.asarray(remap.detach().cpu().numpy() if isinstance(remap, torch.Tensor) else remap).astype(np.int64).reshape(-1)
        a, b = (np.where((m >= 0) & (m < table.size), table[np.clip(m, 0, table.size - 1)], -1) for m in (a, b))
    counts = np.zeros([a.shape[0], classes, 2], np.int32)
    for c in range(classes):
        ia, ib = a == c, b == c
        counts[:, c, 0] = (ia & ib).sum(axis=1)
        counts[:, c, 1] = (ia | ib).sum(axis=1)
    terms = counts[:, :, 0].astype(np.float32) / (counts[:, :, 1].astype(np.float32) + np.float32(1e-6))
    return torch.from_numpy(terms.mean(axis=1, dtype=np.float32)), torch.from_numpy(counts)


def label_iou(a, b, classes=19, remap=None):
    """-> (iou float32 [n], counts int32 [n, classes, 2]: intersection and union per class) of two label maps [n, ...].  `remap`: a table
    applied to both maps first (a label outside the table, or outside [0, classes) after it, counts for no class).  int64 or uint8 CUDA maps
    take `ide3d_label_iou`; anything else the numpy definition."""
    if not (1 <= classes <= 32):
        raise ValueError(f'label_iou: classes must be 1..32, got {classes}')
    on_dev = all(isinstance(t, torch.Tensor) and t.is_cuda and t.dtype in (torch.int64, torch.uint8) for t in (a, b)) and a.dtype == b.dtype
    if not on_dev:
        return label_iou_host(a, b, classes, remap)
    if remap is not None:
        remap = torch.as_tensor(remap).to(device=a.device, dtype=torch.int32).reshape(-1).contiguous()
    return hip_plugin.MetricsEvalPlugin.label_iou(a.detach().contiguous(), b.detach().contiguous(), classes, remap)


class mIOU(torch.nn.Module):
    """apps/calc_losses_on_images.mIOU: `forward(source, target) -> [n]`, images in -1..1.  Both are resized to `size`^2 (bilinear,
    `align_corners=True`), parsed by `bisNet` (`training.parse_loss.labels`: the argmax class ids) and compared class by class after the
    `celebahq` remap of `face_parsing.id_remap`, which the kernel applies; no one-hot tensor exists."""

    def __init__(self, bisNet, classes=19, size=512):
        super().__init__()
        from training import face_parsing
        self.bisNet = bisNet
        self.classes, self.size = classes, size
        self.register_buffer('remap', torch.tensor(face_parsing.REMAP, dtype=torch.int32), persistent=False)

    def labels(self, img):
        from training import parse_loss
        img = torch.nn.functional.interpolate(img, size=(self.size, self.size), mode='bilinear', align_corners=True)
        return parse_loss.labels(self.bisNet, img)

    def forward(self, source, target):
        return label_iou(self.labels(source), self.labels(target), self.classes, self.remap.to(source.device))[0]
