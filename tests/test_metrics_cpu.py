"""Generator metrics without a GPU: the numpy definitions of training/metrics.py against tests/metrics_ref.py,
`FeatureStats` (truncation, algebra, pickles, the reference's class when it imports), the Frechet distance against scipy's sqrtm formula,
KID's draw order, the routing of CPU tensors, the C ABI with its workspace arithmetic and every refusal, and the INTEGRATION.md note."""
import ctypes
import importlib.util
import os
import pickle
import re

import numpy as np
import pytest
import torch

import metrics_ref
from training import metrics

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the numpy definitions --------------------------------------------------------------------------------------------------------

def _subsets(rng, n, subsets, m):
    return np.stack([rng.choice(n, m, replace=False) for _ in range(subsets)]).astype(np.int32)


def test_poly_kernel_sums_and_kid_match_the_restatement():
    rng = np.random.RandomState(0)
    x, y = metrics_ref.features('gauss', 40, 33, 1), metrics_ref.features('relu', 50, 33, 2)
    xi, yi = _subsets(rng, 40, 3, 17), _subsets(rng, 50, 3, 17)
    xi[1] = xi[0]          # repeated indices across subsets
    want, _ = metrics_ref.poly_sums(x, y, xi, yi)
    got = metrics.poly_kernel_sums(torch.from_numpy(x), torch.from_numpy(y), xi, yi)
    assert got.dtype == np.float64 and got.shape == (3, 3)
    np.testing.assert_allclose(got, want, rtol=1e-12)
    np.testing.assert_allclose(metrics.poly_kernel_sums(x, y, xi, yi), want, rtol=1e-12)          # numpy arrays as well
    k = metrics.kid(torch.from_numpy(y), torch.from_numpy(x), indices=(xi, yi))          # real = y, gen = x
    assert abs(k - metrics_ref.kid_from_sums(want, 17)) <= 1e-12 * abs(k)
    # out-of-range indices are clamped; the diagonal is excluded: a subset of identical rows of norm^2 = d has p = 8 everywhere
    ones = np.ones([4, 8], np.float32)
    s = metrics.poly_kernel_sums(ones, ones, np.array([[0, 1, 2, 9]], np.int32), np.array([[-3, 1, 2, 3]], np.int32))
    assert s.tolist() == [[8.0 * 12, 8.0 * 12, 8.0 * 16]]


@pytest.mark.parametrize('kind,n,d,k,count', [('gauss', 64, 16, 3, 64), ('dup', 130, 33, 3, 70), ('relu', 257, 96, 3, 129), ('gauss', 4, 8, 3, 200)])
def test_radii_membership_and_precision_recall_match_the_restatement(kind, n, d, k, count):
    f = metrics_ref.features(kind, n, d, 3)
    p = metrics_ref.probes_for(kind, f, count, 4)
    r64, _ = metrics_ref.radii(f, k)
    got = metrics.knn_radii(torch.from_numpy(f), k)
    assert got.dtype == torch.float64 and not got.is_cuda
    scale = np.square(f.astype(np.float64)).sum(axis=1).max()
    assert np.abs(got.numpy() - r64).max() <= 1e-12 * scale          # the expanded form against the differences, both float64
    if kind == 'dup':
        assert (got.numpy()[9:15] <= 1e-12 * scale).all() and (r64[9:15] == 0).all()
    want, decided = metrics_ref.membership(p, f, r64)
    assert decided.all(), 'the float64 definition decides every probe of these cases'
    inside = metrics.manifold_inside(torch.from_numpy(p), torch.from_numpy(f), torch.from_numpy(r64))
    assert inside.dtype == torch.bool and np.array_equal(inside.numpy(), want)
    pr = metrics.precision_recall(torch.from_numpy(f), torch.from_numpy(p), k)
    assert pr == pytest.approx(metrics_ref.precision_recall(f, p, k), abs=1e-15)
    with pytest.raises(ValueError):
        metrics.knn_radii(torch.from_numpy(f[:k]), k)


def test_precision_recall_docstring_names_the_missing_fp16_rounding():
    assert 'fp16' in metrics.precision_recall.__doc__ and 'NOT reproduced' in metrics.precision_recall.__doc__


# ---- FeatureStats -----------------------------------------------------------------------------------------------------------------

def _fill(cls, batches, **kw):
    s = cls(**kw)
    for b in batches:
        s.append_torch(torch.from_numpy(b))
    return s


def test_feature_stats_truncation_algebra_and_pickle(tmp_path):
    x = metrics_ref.features('relu', 50, 12, 5)
    batches = [x[:16], x[16:37], x[37:]]
    s = _fill(metrics.FeatureStats, batches, capture_all=True, capture_mean_cov=True, max_items=40)
    assert s.num_items == 40 and s.num_features == 12 and s.is_full()
    assert np.array_equal(s.get_all(), x[:40]) and torch.equal(s.get_all_torch(), torch.from_numpy(x[:40]))
    assert [len(f) for f in s.all_features] == [16, 21, 3]
    s.append(x[:5])
    assert s.num_items == 40 and len(s.all_features) == 3, 'a full object ignores what follows'
    mean, cov = s.get_mean_cov()
    want_mean, want_cov = metrics_ref.mean_cov(x[:40])
    np.testing.assert_allclose(mean, want_mean, rtol=0, atol=1e-14)
    np.testing.assert_allclose(cov, want_cov, rtol=0, atol=1e-13)
    assert s.raw_mean.dtype == np.float64 and s.raw_cov.shape == (12, 12)
    open_ended = _fill(metrics.FeatureStats, batches, capture_mean_cov=True)
    assert open_ended.num_items == 50 and not open_ended.is_full()
    with pytest.raises(AssertionError):
        open_ended.get_all()
    with pytest.raises(NotImplementedError, match='num_gpus'):
        s.append_torch(torch.from_numpy(x), num_gpus=2, rank=1)
    # float64 and float16 CPU tensors take the reference's cast to float32
    t = metrics.FeatureStats(capture_all=True)
    t.append_torch(torch.from_numpy(x).double()); t.append_torch(torch.from_numpy(x).half())
    assert t.get_all().dtype == np.float32 and np.array_equal(t.get_all()[:50], x)
    path = str(tmp_path / 'stats.pkl')
    s.save(path)
    with open(path, 'rb') as f:
        raw = pickle.load(f)
    assert set(raw) == {'capture_all', 'capture_mean_cov', 'max_items', 'num_items', 'num_features', 'all_features', 'raw_mean', 'raw_cov'}
    assert all(isinstance(a, np.ndarray) for a in raw['all_features']) and isinstance(raw['raw_mean'], np.ndarray) and isinstance(raw['raw_cov'], np.ndarray)
    back = metrics.FeatureStats.load(path)
    assert back.num_items == 40 and back.max_items == 40 and back.capture_mean_cov and np.array_equal(back.get_all(), s.get_all())
    assert np.array_equal(back.raw_cov, s.raw_cov) and np.array_equal(back.raw_mean, s.raw_mean)


def _reference_feature_stats():
    from oracle import ref_import
    path = os.path.join(ref_import.REFERENCE_ROOT, 'metrics', 'metric_utils.py')
    if not os.path.isfile(path):
        pytest.skip('the reference tree is not present')
    try:
        spec = importlib.util.spec_from_file_location('_reference_metric_utils', path)
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
    except Exception as e:          # its imports (dnnlib of the overlay stands in) may not resolve everywhere
        pytest.skip(f'the reference\'s metric_utils does not import here: {type(e).__name__}: {e}')
    return mod.FeatureStats


def test_feature_stats_against_the_reference_class(tmp_path):
    Ref = _reference_feature_stats()
    x = metrics_ref.features('gauss', 50, 12, 6)
    batches = [x[:16], x[16:37], x[37:]]
    kw = dict(capture_all=True, capture_mean_cov=True, max_items=45)
    ours, theirs = _fill(metrics.FeatureStats, batches, **kw), _fill(Ref, batches, **kw)
    assert ours.num_items == theirs.num_items == 45 and ours.num_features == theirs.num_features
    assert np.array_equal(ours.get_all(), theirs.get_all())
    assert np.array_equal(ours.raw_mean, theirs.raw_mean) and np.array_equal(ours.raw_cov, theirs.raw_cov)          # the same numpy arithmetic
    for a, b in zip(ours.get_mean_cov(), theirs.get_mean_cov()):
        assert np.array_equal(a, b)
    assert sorted(ours.__dict__) == sorted(theirs.__dict__)
    # either side loads the other's pickle
    po, pt = str(tmp_path / 'ours.pkl'), str(tmp_path / 'theirs.pkl')
    ours.save(po); theirs.save(pt)
    for loaded in (Ref.load(po), metrics.FeatureStats.load(pt)):
        assert loaded.num_items == 45 and np.array_equal(loaded.get_all(), x[:45]) and np.array_equal(loaded.raw_cov, theirs.raw_cov)
        assert loaded.capture_mean_cov and np.array_equal(loaded.get_mean_cov()[1], theirs.get_mean_cov()[1])


# ---- Frechet distance -------------------------------------------------------------------------------------------------------------

def _sqrtm_fid(mu_a, sigma_a, mu_b, sigma_b):
    linalg = pytest.importorskip('scipy.linalg')
    s, _ = linalg.sqrtm(np.dot(sigma_a, sigma_b), disp=False)          # frechet_inception_distance.py:37-38
    return float(np.real(np.square(mu_a - mu_b).sum() + np.trace(sigma_a + sigma_b - s * 2)))


@pytest.mark.parametrize('n,d,rel', [(256, 64, 1e-9), (384, 96, 1e-9), (40, 48, 1e-6)])
def test_frechet_distance_against_sqrtm(n, d, rel):
    rng = np.random.RandomState(d)
    mix = rng.randn(d, d) / np.sqrt(d)
    a = metrics_ref.features('gauss', n, d, 7) @ mix.astype(np.float32)
    b = metrics_ref.features('relu', n, d, 8)
    (mu_a, sa), (mu_b, sb) = metrics_ref.mean_cov(a), metrics_ref.mean_cov(b)
    want = _sqrtm_fid(mu_a, sa, mu_b, sb)
    got = metrics.frechet_distance(mu_a, sa, mu_b, sb)
    print(f'n = {n}, d = {d}: {got!r} against sqrtm {want!r}, relative {abs(got - want) / abs(want):.2e}')
    assert abs(got - want) <= rel * abs(want)
    assert abs(metrics.frechet_distance(mu_b, sb, mu_a, sa) - got) <= rel * abs(want), 'symmetric in its arguments'
    # a set against itself: each of the d eigenvalues of S^(1/2) S S^(1/2) moves by at most eps |S|^2 (Weyl), its root by sqrt(eps) |S|
    assert abs(metrics.frechet_distance(mu_a, sa, mu_a, sa)) <= 2 * d * np.sqrt(np.finfo(np.float64).eps) * np.linalg.eigvalsh(sa).max()
    sr, sg = metrics.FeatureStats(capture_mean_cov=True), metrics.FeatureStats(capture_mean_cov=True)
    sr.append(b); sg.append(a)
    assert abs(metrics.fid(sr, sg) - want) <= rel * abs(want)


# ---- KID's draws ------------------------------------------------------------------------------------------------------------------

def test_kid_draw_order_under_a_seeded_random_state():
    real, gen = metrics_ref.features('gauss', 30, 8, 9), metrics_ref.features('relu', 23, 8, 10)
    rng = np.random.RandomState(123)
    want_x, want_y = [], []
    for _ in range(4):          # kernel_inception_distance.py:37-39: gen first, then real
        want_x.append(rng.choice(23, 10, replace=False)); want_y.append(rng.choice(30, 10, replace=False))
    xi, yi = metrics.kid_indices(30, 23, num_subsets=4, max_subset_size=10, rng=np.random.RandomState(123))
    assert xi.dtype == np.int32 and np.array_equal(xi, want_x) and np.array_equal(yi, want_y)
    got = metrics.kid(torch.from_numpy(real), torch.from_numpy(gen), num_subsets=4, max_subset_size=10, rng=np.random.RandomState(123))
    t = 0.0
    for s in range(4):
        x, y = gen[want_x[s]].astype(np.float64), real[want_y[s]].astype(np.float64)
        a = (x @ x.T / 8 + 1) ** 3 + (y @ y.T / 8 + 1) ** 3
        b = (x @ y.T / 8 + 1) ** 3
        t += (a.sum() - np.diag(a).sum()) / 9 - b.sum() * 2 / 10
    assert got == pytest.approx(t / 4 / 10, rel=1e-12)
    # m = min(both sizes, max_subset_size); the global generator when rng is None
    assert metrics.kid_indices(30, 23, 2, 1000, np.random.RandomState(0))[0].shape == (2, 23)
    np.random.seed(5)
    a = metrics.kid_indices(30, 23, 1, 10)
    np.random.seed(5)
    assert np.array_equal(a[0][0], np.random.choice(23, 10, replace=False))


# ---- routing ----------------------------------------------------------------------------------------------------------------------

def test_cpu_tensors_take_the_numpy_definitions_without_a_plugin_call():
    from torch_utils import hip_plugin
    before = dict(hip_plugin.CALLS)
    x, y = torch.from_numpy(metrics_ref.features('gauss', 20, 6, 11)), torch.from_numpy(metrics_ref.features('gauss', 24, 6, 12))
    s = metrics.FeatureStats(capture_all=True, capture_mean_cov=True)
    s.append_torch(x)
    assert isinstance(s.raw_cov, np.ndarray) and isinstance(s.all_features[0], np.ndarray)
    metrics.kid(x, y, num_subsets=2, max_subset_size=8, rng=np.random.RandomState(0))
    metrics.precision_recall(x, y, 3)
    metrics.fid(s, s)
    assert dict(hip_plugin.CALLS) == before

    def detector(images, scale=1.0):
        assert images.dtype == torch.uint8 and images.shape[1] == 3
        return images.float().mean(dim=(2, 3)) * scale

    grey = [torch.full([4, 1, 5, 5], v, dtype=torch.uint8) for v in (1, 2, 3)]
    st = metrics.feature_stats_for_images(grey, detector, max_items=10, detector_kwargs=dict(scale=2.0), capture_all=True)
    assert st.num_items == 10 and np.array_equal(st.get_all()[:, 0], np.repeat([2.0, 4.0, 6.0], 4)[:10].astype(np.float32))


# ---- C ABI ------------------------------------------------------------------------------------------------------------------------

NAMES = ('ide3d_metrics_workspace_bytes', 'ide3d_feature_moments', 'ide3d_poly_kernel_sums', 'ide3d_knn_radii', 'ide3d_manifold_inside')


def test_c_abi_declarations_and_workspace_arithmetic():
    from torch_utils import hip_plugin
    with open(os.path.join(ROOT, 'include', 'ide3d_hip.h')) as f:
        h = f.read()
    for cite in ('metrics/metric_utils.py:107-122', 'kernel_inception_distance.py:34-43', 'precision_recall.py:19-59'):
        assert cite in h, cite
    path = hip_plugin.lib_path()
    assert os.path.isfile(path), f'{path} missing: run __graft_entry__.build()'
    lib, loaded = ctypes.CDLL(path), hip_plugin.load()
    for name in NAMES:
        assert name in hip_plugin.EXPORTED_SYMBOLS and hasattr(lib, name), name
        m = re.search(r'(int64_t|int) %s\(([^)]*)\);' % name, h)
        assert m, name
        assert len(getattr(loaded, name).argtypes) == len(m.group(2).split(',')), name
    assert hip_plugin.PLUGINS['metrics_plugin'] is hip_plugin.MetricsPlugin
    assert loaded.ide3d_abi_version() == 8 and hip_plugin._ABI_VERSION == 8, 'entry points were only added'
    ws = loaded.ide3d_metrics_workspace_bytes
    POLY, RADII, INSIDE = 0, 1, 2
    cd = lambda a, b: -(-a // b)
    al = lambda v: cd(v, 16) * 16
    splits = lambda rt, ct: min(ct, max(1, 1024 // rt))
    for m, subsets in ((2, 1), (17, 3), (128, 1), (129, 5), (1000, 100), (4096, 4096)):
        assert ws(POLY, m, m, 2048, subsets) == subsets * 3 * cd(m, 128) ** 2 * 8
    for n, k in ((4, 3), (128, 1), (129, 7), (640, 3), (50000, 3), (1 << 22, 3)):
        rt = cd(n, 128)
        assert ws(RADII, n, n, 4096, k) == al(4 * n) + splits(rt, rt) * rt * 128 * 8 * 4, n
    for n_p, n_m in ((1, 1), (64, 70), (385, 640), (50000, 50000), (1 << 22, 5)):
        rt, ct = cd(n_p, 128), cd(n_m, 128)
        assert ws(INSIDE, n_p, n_m, 1, 0) == al(4 * n_p) + al(4 * n_m) + al(splits(rt, ct) * rt * 128), (n_p, n_m)
    for bad in ((POLY, 1, 1, 8, 1), (POLY, 4097, 4097, 8, 1), (POLY, 8, 9, 8, 1), (POLY, 8, 8, 0, 1), (POLY, 8, 8, 8193, 1), (POLY, 8, 8, 8, 0), (POLY, 8, 8, 8, 4097),
                (RADII, 3, 3, 8, 3), (RADII, 8, 8, 8, 0), (RADII, 8, 8, 8, 8), (RADII, 8, 9, 8, 3), (RADII, (1 << 22) + 1, (1 << 22) + 1, 8, 3), (RADII, 8, 8, 8193, 3),
                (INSIDE, 0, 8, 8, 0), (INSIDE, 8, 0, 8, 0), (INSIDE, (1 << 22) + 1, 8, 8, 0), (INSIDE, 8, (1 << 22) + 1, 8, 0), (INSIDE, 8, 8, 0, 0), (3, 8, 8, 8, 3), (-1, 8, 8, 8, 3)):
        assert ws(*bad) == -1, bad


def test_every_refusal_comes_before_the_first_launch():
    """No GPU here: a call that reached a launch would fail with another code (or crash on the dummy pointers)."""
    from torch_utils import hip_plugin
    lib = hip_plugin.load()
    buf = (ctypes.c_uint8 * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    off = ctypes.c_void_p(ctypes.addressof(buf) + 4)          # 4-byte aligned only
    big = 1 << 40
    N = 1 << 22

    def check(fn, name, cases):
        got = {k: fn(*args) for k, args in cases.items()}
        assert all(rc == -1 for rc in got.values()), (name, got)
        assert name.encode() in lib.ide3d_last_error()

    check(lib.ide3d_feature_moments, 'feature_moments', dict(
        d0=(p, 8, 0, 8, p, p, None), d_big=(p, 8, 8193, 8193, p, p, None), n0=(p, 0, 8, 8, p, p, None), n_big=(p, N + 1, 8, 8, p, p, None),
        stride=(p, 8, 8, 7, p, p, None), null_x=(None, 8, 8, 8, p, p, None), null_mean=(p, 8, 8, 8, None, p, None), null_cov=(p, 8, 8, 8, p, None, None),
        aligned=(p, 8, 8, 8, off, p, None)))
    ok = dict(x=p, nx=40, sx=8, y=p, ny=50, sy=8, d=8, xi=p, yi=p, subsets=2, m=4, ws=p, wsb=big, sums=p)

    def poly(**kw):
        a = dict(ok, **kw)
        return (a['x'], a['nx'], a['sx'], a['y'], a['ny'], a['sy'], a['d'], a['xi'], a['yi'], a['subsets'], a['m'], a['ws'], a['wsb'], a['sums'], None)

    need = lib.ide3d_metrics_workspace_bytes(0, 4, 4, 8, 2)
    check(lib.ide3d_poly_kernel_sums, 'poly_kernel_sums', dict(
        d0=poly(d=0), d_big=poly(d=8193, sx=8193, sy=8193), nx0=poly(nx=0), ny_big=poly(ny=N + 1), m1=poly(m=1), m_big=poly(m=4097), subsets0=poly(subsets=0),
        subsets_big=poly(subsets=4097), stride_x=poly(sx=7), stride_y=poly(sy=7), null_x=poly(x=None), null_y=poly(y=None), null_xi=poly(xi=None),
        null_yi=poly(yi=None), null_ws=poly(ws=None), null_sums=poly(sums=None), workspace=poly(wsb=need - 1), aligned=poly(ws=off)))
    need = lib.ide3d_metrics_workspace_bytes(1, 8, 8, 8, 3)
    check(lib.ide3d_knn_radii, 'knn_radii', dict(
        d0=(p, 8, 0, 8, 3, p, big, p, None), d_big=(p, 8, 8193, 8193, 3, p, big, p, None), n0=(p, 0, 8, 8, 3, p, big, p, None), n_big=(p, N + 1, 8, 8, 3, p, big, p, None),
        k0=(p, 8, 8, 8, 0, p, big, p, None), k8=(p, 80, 8, 8, 8, p, big, p, None), n_le_k=(p, 3, 8, 8, 3, p, big, p, None), stride=(p, 8, 8, 7, 3, p, big, p, None),
        null_f=(None, 8, 8, 8, 3, p, big, p, None), null_ws=(p, 8, 8, 8, 3, None, big, p, None), null_out=(p, 8, 8, 8, 3, p, big, None, None),
        workspace=(p, 8, 8, 8, 3, p, need - 1, p, None), aligned=(p, 8, 8, 8, 3, off, big, p, None)))
    need = lib.ide3d_metrics_workspace_bytes(2, 8, 9, 8, 0)
    check(lib.ide3d_manifold_inside, 'manifold_inside', dict(
        d0=(p, 8, 8, p, 9, 8, 0, p, p, big, p, None), d_big=(p, 8, 8193, p, 9, 8193, 8193, p, p, big, p, None), np0=(p, 0, 8, p, 9, 8, 8, p, p, big, p, None),
        nm0=(p, 8, 8, p, 0, 8, 8, p, p, big, p, None), np_big=(p, N + 1, 8, p, 9, 8, 8, p, p, big, p, None), nm_big=(p, 8, 8, p, N + 1, 8, 8, p, p, big, p, None),
        stride_p=(p, 8, 7, p, 9, 8, 8, p, p, big, p, None), stride_m=(p, 8, 8, p, 9, 7, 8, p, p, big, p, None), null_probes=(None, 8, 8, p, 9, 8, 8, p, p, big, p, None),
        null_manifold=(p, 8, 8, None, 9, 8, 8, p, p, big, p, None), null_radii=(p, 8, 8, p, 9, 8, 8, None, p, big, p, None), null_ws=(p, 8, 8, p, 9, 8, 8, p, None, big, p, None),
        null_inside=(p, 8, 8, p, 9, 8, 8, p, p, big, None, None), workspace=(p, 8, 8, p, 9, 8, 8, p, p, need - 1, p, None), aligned=(p, 8, 8, p, 9, 8, 8, p, off, big, p, None)))


def test_integration_note_names_the_patches():
    with open(os.path.join(ROOT, 'INTEGRATION.md')) as f:
        text = f.read()
    for needle in ('metrics/frechet_inception_distance.py', 'metrics/kernel_inception_distance.py', 'metrics/precision_recall.py', 'metric_utils.FeatureStats',
                   'from training.metrics import FeatureStats', 'from training.metrics import frechet_distance', 'from training.metrics import kid',
                   'from training.metrics import precision_recall'):
        assert needle in text, needle
