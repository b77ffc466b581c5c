"""csrc/metrics.hip on the GPU against the float64 restatement of tests/metrics_ref.py: the float64 moments, the
k-th-neighbour radii, manifold membership, the polynomial-kernel sums, buffer guards, refusals and one end-to-end run from a generator and a
stand-in detector to FID, KID and precision / recall.  Every bound is derived in metrics_ref from the number formats."""
import ctypes

import numpy as np
import pytest
import torch

import metrics_ref
from training import metrics

pytestmark = pytest.mark.gpu

GUARD = 0xA5


def P():
    from torch_utils import hip_plugin
    return hip_plugin.MetricsPlugin


def guarded(nbytes, dev, pad=4096):
    """-> (whole buffer filled with GUARD, the 16-byte aligned view of nbytes in its middle)."""
    big = torch.full([nbytes + 2 * pad], GUARD, dtype=torch.uint8, device=dev)
    return big, big[pad:pad + nbytes]


def untouched_outside(big, nbytes, pad=4096):
    return bool((big[:pad] == GUARD).all()) and bool((big[pad + nbytes:] == GUARD).all())


# ---- moments ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('n,d,stride', [(1, 1, 1), (64, 33, 33), (257, 100, 107), (129, 256, 256)])
def test_moments(gpu_device, n, d, stride):
    n0 = 5          # rows whose numpy float64 sums are the non-zero running buffers the device adds to
    x = metrics_ref.features('relu', n0 + n, d, 20 + d)
    cut = n0 + max(1, (2 * n) // 5) if n > 1 else n0 + 1
    x0 = x[:n0].astype(np.float64)
    runs = []
    for _ in range(2):
        big_m, vm = guarded(8 * d, gpu_device)
        big_c, vc = guarded(8 * d * d, gpu_device)
        mean, cov = vm.view(torch.float64), vc.view(torch.float64).view(d, d)
        mean.copy_(torch.from_numpy(x0.sum(axis=0))); cov.copy_(torch.from_numpy(x0.T @ x0))
        for lo, hi in ((n0, cut), (cut, n0 + n)):
            if hi > lo:
                wide = torch.zeros([hi - lo, stride], dtype=torch.float32, device=gpu_device) + 7.0
                wide[:, :d] = torch.from_numpy(x[lo:hi]).to(gpu_device)
                P().feature_moments(wide[:, :d], mean, cov)
        torch.cuda.synchronize()
        assert untouched_outside(big_m, 8 * d) and untouched_outside(big_c, 8 * d * d)
        runs.append((mean.cpu().numpy().copy(), cov.cpu().numpy().copy()))
    (mean, cov), (mean2, cov2) = runs
    assert np.array_equal(mean, mean2) and np.array_equal(cov, cov2), 'two runs are bit-equal'
    assert np.array_equal(cov, cov.T), 'bit-symmetric'
    want_mean, want_cov, abs_cov = metrics_ref.moments(x)
    N = n0 + n
    err_m = np.abs(mean.astype(np.longdouble) - want_mean)
    err_c = np.abs(cov.astype(np.longdouble) - want_cov)
    bound_m = N * 2.0 ** -52 * np.abs(x.astype(np.longdouble)).sum(axis=0)
    bound_c = N * 2.0 ** -52 * abs_cov
    print(f'moments {n} x {d}: largest error / bound: mean {float((err_m / np.maximum(bound_m, 1e-300)).max()):.3f}, cov {float((err_c / np.maximum(bound_c, 1e-300)).max()):.3f}')
    assert (err_m <= bound_m).all() and (err_c <= bound_c).all()


def test_feature_stats_keeps_device_features_and_moments(gpu_device):
    from torch_utils import hip_plugin
    x = metrics_ref.features('gauss', 50, 33, 30)
    s = metrics.FeatureStats(capture_all=True, capture_mean_cov=True, max_items=45)
    before = hip_plugin.CALLS.get('feature_moments', 0)
    s.append(x[:7])                                                   # numpy first: the running sums move to the device unchanged
    for lo, hi in ((7, 20), (20, 50)):
        s.append_torch(torch.from_numpy(x[lo:hi]).to(gpu_device))
    assert hip_plugin.CALLS.get('feature_moments', 0) == before + 2
    assert s.num_items == 45 and s.is_full()
    assert s.raw_cov.is_cuda and s.raw_cov.dtype == torch.float64 and s.raw_mean.is_cuda
    got = s.get_all_torch()
    assert got.is_cuda and torch.equal(got.cpu(), torch.from_numpy(x[:45])) and np.array_equal(s.get_all(), x[:45])
    want_mean, want_cov, abs_cov = metrics_ref.moments(x[:45])
    assert (np.abs(s.raw_cov.cpu().numpy().astype(np.longdouble) - want_cov) <= 45 * 2.0 ** -52 * abs_cov).all()
    mean, cov = s.get_mean_cov()
    ref_mean, ref_cov = metrics_ref.mean_cov(x[:45])
    np.testing.assert_allclose(mean, ref_mean, rtol=0, atol=1e-13)
    np.testing.assert_allclose(cov, ref_cov, rtol=0, atol=1e-12)
    with pytest.raises(NotImplementedError):
        s.append_torch(torch.from_numpy(x).to(gpu_device), num_gpus=2)


# ---- radii and membership ---------------------------------------------------------------------------------------------------------

CASES = {          # name -> (kind, n, d, k, probes)
    'gauss_64': ('gauss', 64, 16, 3, 64), 'dup_130': ('dup', 130, 33, 3, 70), 'relu_257': ('relu', 257, 96, 3, 129), 'gauss_640': ('gauss', 640, 128, 3, 385),
    'gauss_129_k1': ('gauss', 129, 100, 1, 257), 'gauss_200_k5': ('gauss', 200, 4, 5, 200), 'gauss_4': ('gauss', 4, 8, 3, 37),
}
_case = {}


def case(name):
    """Features, probes and their float64 reference, computed once and never modified."""
    if name not in _case:
        kind, n, d, k, count = CASES[name]
        f = metrics_ref.features(kind, n, d, 40 + n)
        p = metrics_ref.probes_for(kind, f, count, 41 + n)
        r64, bound = metrics_ref.radii(f, k)
        inside, decided = metrics_ref.membership(p, f, r64)
        _case[name] = dict(kind=kind, k=k, f=f, p=p, r64=r64, bound=bound, inside=inside, decided=decided)
    return _case[name]


@pytest.mark.parametrize('name', sorted(CASES))
def test_radii(gpu_device, name):
    from torch_utils import hip_plugin
    c = case(name)
    before = hip_plugin.CALLS.get('knn_radii', 0)
    got = metrics.knn_radii(torch.from_numpy(c['f']).to(gpu_device), c['k'])
    assert hip_plugin.CALLS.get('knn_radii', 0) == before + 1
    assert got.is_cuda and got.dtype == torch.float32 and got.shape == (len(c['f']),)
    again = metrics.knn_radii(torch.from_numpy(c['f']).to(gpu_device), c['k'])
    assert torch.equal(got, again), 'two runs are bit-equal'
    r = got.cpu().numpy().astype(np.float64)
    err = np.abs(r - c['r64'])
    print(f'{name}: largest radius error / bound {float((err / c["bound"]).max()):.4f}')
    assert (err <= c['bound']).all()
    if c['kind'] == 'dup':
        print(f'{name}: radii of the identical rows {r[9:15].tolist()}')
        assert (r[9:15] == 0).all(), 'six identical rows: the self pair and three more at exactly 0'


@pytest.mark.parametrize('name', sorted(CASES))
def test_membership_and_precision_recall(gpu_device, name):
    c = case(name)
    f, p = torch.from_numpy(c['f']).to(gpu_device), torch.from_numpy(c['p']).to(gpu_device)
    radii_sq = metrics.knn_radii(f, c['k'])                         # the device's own radii
    inside = metrics.manifold_inside(p, f, radii_sq)
    assert inside.is_cuda and inside.dtype == torch.bool and torch.equal(inside, metrics.manifold_inside(p, f, radii_sq))
    got = inside.cpu().numpy()
    undecided = int((~c['decided']).sum())
    print(f'{name}: {undecided} of {len(got)} probes undecided, {int(got.sum())} inside')
    assert undecided <= 0.01 * len(got), 'a condition on the case, not a measurement of the kernel'
    assert np.array_equal(got[c['decided']], c['inside'][c['decided']])
    # precision / recall up to the undecided probes of either direction
    back_r64, _ = metrics_ref.radii(c['p'], c['k']) if len(c['p']) > c['k'] else (None, None)
    if back_r64 is not None:
        rec_inside, rec_decided = metrics_ref.membership(c['f'], c['p'], back_r64)
        precision, recall = metrics.precision_recall(f, p, c['k'])          # real = the manifold set, gen = the probes
        assert abs(precision - c['inside'].mean()) <= undecided / len(got) + 1e-12
        assert abs(recall - rec_inside.mean()) <= int((~rec_decided).sum()) / len(rec_inside) + 1e-12


# ---- KID sums ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('nx,ny,d,subsets,m', [(40, 50, 33, 3, 17), (300, 257, 100, 5, 129), (64, 64, 256, 2, 64)])
def test_poly_kernel_sums_and_kid(gpu_device, nx, ny, d, subsets, m):
    from torch_utils import hip_plugin
    rng = np.random.RandomState(d)
    x, y = metrics_ref.features('gauss', nx, d, 50), metrics_ref.features('relu', ny, d, 51)
    xi = np.stack([rng.choice(nx, m, replace=False) for _ in range(subsets)]).astype(np.int32)
    yi = np.stack([rng.choice(ny, m, replace=False) for _ in range(subsets)]).astype(np.int32)
    xi[-1] = xi[0]; yi[-1, :m // 2] = yi[0, :m // 2]          # repeated indices across subsets
    want, bound = metrics_ref.poly_sums(x, y, xi, yi)
    xd, yd = torch.from_numpy(x).to(gpu_device), torch.from_numpy(y).to(gpu_device)
    before = hip_plugin.CALLS.get('poly_kernel_sums', 0)
    got = metrics.poly_kernel_sums(xd, yd, xi, yi)
    assert hip_plugin.CALLS.get('poly_kernel_sums', 0) == before + 1
    assert got.dtype == np.float64 and got.shape == (subsets, 3)
    assert np.array_equal(got, metrics.poly_kernel_sums(xd, yd, xi, yi)), 'two runs are bit-equal'
    err = np.abs(got - want)
    print(f'poly sums {nx} x {ny} x {d}, {subsets} subsets of {m}: largest error / bound {float((err / bound).max()):.4f}')
    assert (err <= bound).all()
    assert np.array_equal(got[-1, 0], got[0, 0]), 'the same rows give the same sum'
    k = metrics.kid(yd, xd, indices=(xi, yi))          # real = y, gen = x
    assert k == metrics_ref.kid_from_sums(got, m)
    # a wider row stride takes the scalar loads and gives the same bits
    wide = torch.zeros([nx, d + 3], dtype=torch.float32, device=gpu_device); wide[:, :d] = xd
    assert np.array_equal(metrics.poly_kernel_sums(wide[:, :d], yd, xi, yi), got)


def test_poly_kernel_sums_exclude_the_diagonal(gpu_device):
    """Identical rows of squared norm d: every p is exactly 8, so the sums count pairs: m (m - 1) without the diagonal, m^2 with it."""
    m, d = 130, 16
    ones = torch.ones([5, d], dtype=torch.float32, device=gpu_device)
    xi = np.zeros([2, m], np.int32); xi[1] = np.arange(m) % 5
    yi = np.full([2, m], 99, np.int32); yi[1, 0] = -4          # clamped into range
    got = metrics.poly_kernel_sums(ones, ones, xi, yi)
    assert got.tolist() == [[8.0 * m * (m - 1), 8.0 * m * (m - 1), 8.0 * m * m]] * 2


# ---- buffers and refusals ---------------------------------------------------------------------------------------------------------

def test_outputs_and_workspaces_are_written_only_inside_their_views(gpu_device):
    c = case('relu_257')
    f, p = torch.from_numpy(c['f']).to(gpu_device), torch.from_numpy(c['p']).to(gpu_device)
    n, d, count, k = len(c['f']), c['f'].shape[1], len(c['p']), c['k']
    ws_bytes = P().workspace_bytes(P().RADII, n, n, d, k)
    big_ws, ws = guarded(ws_bytes, gpu_device)
    big_r, vr = guarded(4 * n, gpu_device)
    radii_sq = vr.view(torch.float32)
    P().knn_radii(f, k, ws, radii_sq)
    torch.cuda.synchronize()
    assert untouched_outside(big_ws, ws_bytes) and untouched_outside(big_r, 4 * n)
    assert torch.equal(radii_sq, metrics.knn_radii(f, k))
    ws_bytes = P().workspace_bytes(P().INSIDE, count, n, d, 0)
    big_ws, ws = guarded(ws_bytes, gpu_device)
    big_i, inside = guarded(count, gpu_device)
    P().manifold_inside(p, f, radii_sq, ws, inside)
    torch.cuda.synchronize()
    assert untouched_outside(big_ws, ws_bytes) and untouched_outside(big_i, count)
    assert set(inside.unique().tolist()) <= {0, 1} and torch.equal(inside != 0, metrics.manifold_inside(p, f, radii_sq))
    subsets, m = 3, 129
    xi = torch.from_numpy((np.arange(subsets * m).reshape(subsets, m) % n).astype(np.int32)).to(gpu_device)
    yi = torch.from_numpy((np.arange(subsets * m).reshape(subsets, m) * 7 % count).astype(np.int32)).to(gpu_device)
    ws_bytes = P().workspace_bytes(P().POLY, m, m, d, subsets)
    big_ws, ws = guarded(ws_bytes, gpu_device)
    big_s, vs = guarded(8 * subsets * 3, gpu_device)
    sums = vs.view(torch.float64).view(subsets, 3)
    P().poly_kernel_sums(f, p, xi, yi, ws, sums)
    torch.cuda.synchronize()
    assert untouched_outside(big_ws, ws_bytes) and untouched_outside(big_s, 8 * subsets * 3)
    assert np.array_equal(sums.cpu().numpy(), metrics.poly_kernel_sums(f, p, xi.cpu().numpy(), yi.cpu().numpy()))


def test_refusals_launch_nothing(gpu_device):
    from torch_utils import hip_plugin
    lib = hip_plugin.load()
    f = torch.ones([8, 8], dtype=torch.float32, device=gpu_device)
    idx = torch.zeros([2, 4], dtype=torch.int32, device=gpu_device)
    ws = torch.full([1 << 16], GUARD, dtype=torch.uint8, device=gpu_device)
    out = torch.full([1 << 12], GUARD, dtype=torch.uint8, device=gpu_device)
    p = lambda t, o=0: ctypes.c_void_p(t.data_ptr() + o)
    bad = dict(
        moments_d=lib.ide3d_feature_moments(p(f), 8, 0, 8, p(out), p(ws), None), moments_stride=lib.ide3d_feature_moments(p(f), 8, 8, 7, p(out), p(ws), None),
        moments_n=lib.ide3d_feature_moments(p(f), 0, 8, 8, p(out), p(ws), None), moments_null=lib.ide3d_feature_moments(p(f), 8, 8, 8, None, p(ws), None),
        poly_m=lib.ide3d_poly_kernel_sums(p(f), 8, 8, p(f), 8, 8, 8, p(idx), p(idx), 2, 1, p(ws), ws.numel(), p(out), None),
        poly_ws=lib.ide3d_poly_kernel_sums(p(f), 8, 8, p(f), 8, 8, 8, p(idx), p(idx), 2, 4, p(ws), 47, p(out), None),
        poly_aligned=lib.ide3d_poly_kernel_sums(p(f), 8, 8, p(f), 8, 8, 8, p(idx), p(idx), 2, 4, p(ws, 8), 1024, p(out), None),
        radii_k=lib.ide3d_knn_radii(p(f), 8, 8, 8, 8, p(ws), ws.numel(), p(out), None), radii_n=lib.ide3d_knn_radii(p(f), 3, 8, 8, 3, p(ws), ws.numel(), p(out), None),
        radii_ws=lib.ide3d_knn_radii(p(f), 8, 8, 8, 3, p(ws), lib.ide3d_metrics_workspace_bytes(1, 8, 8, 8, 3) - 1, p(out), None),
        inside_d=lib.ide3d_manifold_inside(p(f), 8, 8, p(f), 8, 8, 8193, p(out), p(ws), ws.numel(), p(out), None),
        inside_ws=lib.ide3d_manifold_inside(p(f), 8, 8, p(f), 8, 8, 8, p(out), p(ws), lib.ide3d_metrics_workspace_bytes(2, 8, 8, 8, 0) - 1, p(out), None),
        inside_null=lib.ide3d_manifold_inside(p(f), 8, 8, p(f), 8, 8, 8, None, p(ws), ws.numel(), p(out), None))
    assert all(rc == -1 for rc in bad.values()), bad
    torch.cuda.synchronize()
    assert bool((ws == GUARD).all()) and bool((out == GUARD).all())
    with pytest.raises(RuntimeError):
        metrics.knn_radii(f[:3], 3)
    with pytest.raises(RuntimeError):
        P().feature_moments(f, torch.zeros([8], dtype=torch.float32, device=gpu_device), torch.zeros([8, 8], dtype=torch.float64, device=gpu_device))


# ---- end to end -------------------------------------------------------------------------------------------------------------------

class StandInDetector(torch.nn.Module):
    """Two random convolutions and a spatial mean: 64 features per uint8 image."""

    def __init__(self, seed):
        super().__init__()
        g = torch.Generator().manual_seed(seed)
        self.w0 = torch.nn.Parameter(torch.randn(16, 3, 3, 3, generator=g) / 5)
        self.w1 = torch.nn.Parameter(torch.randn(64, 16, 3, 3, generator=g) / 12)

    def forward(self, images, gain=1.0):
        assert images.dtype == torch.uint8 and images.shape[1] == 3
        h = torch.relu(torch.nn.functional.conv2d(images.float() / 127.5 - 1, self.w0, stride=2))
        return torch.relu(torch.nn.functional.conv2d(h, self.w1, stride=2) + 0.5).mean(dim=(2, 3)) * gain


def test_generator_to_fid_kid_and_precision_recall(gpu_device):
    from torch_utils import hip_plugin
    from training import triplane
    detector = StandInDetector(0).to(gpu_device).requires_grad_(False)

    def labels():
        k = 0
        while True:
            yield torch.cat([triplane.camera_label(0.1 * ((k + j) % 9 - 4), device=gpu_device) for j in range(4)])
            k += 4

    stats = []
    for seed in (0, 1):
        torch.manual_seed(seed)
        G = triplane.TriPlaneGenerator(triplane.tiny_spec()).eval().requires_grad_(False).to(gpu_device)
        torch.manual_seed(10 + seed)
        stats.append(metrics.feature_stats_for_generator(G, detector, labels(), max_items=96, batch_size=32, batch_gen=4, G_kwargs=dict(noise_mode='const'),
                                                         detector_kwargs=dict(gain=2.0), capture_all=True, capture_mean_cov=True))
    real, gen = stats
    for s in stats:
        assert s.num_items == 96 and s.num_features == 64 and s.raw_cov.is_cuda and s.get_all_torch().is_cuda and s.get_all_torch().shape == (96, 64)
    fr, fg = real.get_all(), gen.get_all()
    assert np.isfinite(fr).all() and fr.std(axis=0).min() > 0 and not np.array_equal(fr, fg)
    # FID: the device's running sums within the moments bound of the captured features; the distance is the host formula on them
    for s, feats in ((real, fr), (gen, fg)):
        want_mean, want_cov, abs_cov = metrics_ref.moments(feats)
        assert (np.abs(s.raw_cov.cpu().numpy().astype(np.longdouble) - want_cov) <= 96 * 2.0 ** -52 * abs_cov).all()
        assert (np.abs(s.raw_mean.cpu().numpy().astype(np.longdouble) - want_mean) <= 96 * 2.0 ** -52 * np.abs(feats.astype(np.longdouble)).sum(axis=0)).all()
    value = metrics.fid(real, gen)
    host = metrics.frechet_distance(*metrics_ref.mean_cov(fg), *metrics_ref.mean_cov(fr))
    print(f'FID {value!r} (from float64 moments of the same features: {host!r})')
    assert np.isfinite(value) and value == metrics.frechet_distance(*gen.get_mean_cov(), *real.get_mean_cov())
    # KID
    xi, yi = metrics.kid_indices(96, 96, num_subsets=3, max_subset_size=50, rng=np.random.RandomState(0))
    sums = metrics.poly_kernel_sums(gen.get_all_torch(), real.get_all_torch(), xi, yi)
    want, bound = metrics_ref.poly_sums(fg, fr, xi, yi)
    assert (np.abs(sums - want) <= bound).all()
    assert metrics.kid(real.get_all_torch(), gen.get_all_torch(), indices=(xi, yi)) == metrics_ref.kid_from_sums(sums, 50)
    # precision / recall
    precision, recall = metrics.precision_recall(real.get_all_torch(), gen.get_all_torch(), 3)
    for got, manifold, probes in ((precision, fr, fg), (recall, fg, fr)):
        inside, decided = metrics_ref.membership(probes, manifold, metrics_ref.radii(manifold, 3)[0])
        assert abs(got - inside.mean()) <= (~decided).sum() / len(probes) + 1e-12
    print(f'KID {metrics_ref.kid_from_sums(sums, 50)!r}, precision {precision}, recall {recall}')
    assert hip_plugin.exclusive_violations()[0] == 0
