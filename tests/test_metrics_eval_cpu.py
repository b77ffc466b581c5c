"""The host side of PPL, Inception Score and mIoU (training/metrics.py) without a GPU: the rank formulas, the numpy
definitions against the reference's lines restated on float64 copies, slerp, the sampler's two torch paths, and the C ABI."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import metrics_eval_ref as ref
from metrics_eval_ref import REMAP, camera_labels, label_maps, reference_iou, tiny_sampler, trimmed_cases
from training import metrics

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- trimmed mean -----------------------------------------------------------------------------------------------------------------

def test_rank_formulas_equal_numpy_percentile_positions():
    for n in list(range(1, 5001)) + [50000]:
        a = np.arange(n)
        lo, hi = metrics.percentile_ranks(n)
        assert lo == np.percentile(a, 1, method='lower') and hi == np.percentile(a, 99, method='higher'), n
        assert (lo, hi) == ref.percentile_ranks(n)
    with pytest.raises(ValueError):
        metrics.percentile_ranks(0)


def reference_ppl(dist):
    """perceptual_path_length.py:120-122 on a float64 copy."""
    dist = np.asarray(dist, np.float64)
    lo = np.percentile(dist, 1, method='lower')
    hi = np.percentile(dist, 99, method='higher')
    return np.extract(np.logical_and(dist >= lo, dist <= hi), dist).mean()


@pytest.mark.parametrize('name', sorted(trimmed_cases()))
def test_host_trimmed_mean_equals_the_reference_lines(name):
    x = trimmed_cases()[name]
    want = reference_ppl(x)
    for given in (x, torch.from_numpy(x)):
        got = metrics.ppl_from_distances(given)
        assert got == want or (np.isinf(want) and got == want), (name, got, want)
    lo_rank, hi_rank = metrics.percentile_ranks(len(x))
    mean, lo, hi, count = metrics.trimmed_mean_host(x, lo_rank, hi_rank)
    w_mean, w_lo, w_hi, w_count, _ = ref.trimmed_mean(x, lo_rank, hi_rank)
    assert (lo, hi, count) == (w_lo, w_hi, w_count) and (mean == float(w_mean) or abs(mean - float(w_mean)) <= 1e-15 * abs(mean))


def test_host_trimmed_mean_nan_and_bad_ranks():
    x = np.random.RandomState(4).randn(100).astype(np.float32)
    x[50] = np.nan
    assert np.isnan(metrics.ppl_from_distances(x)) and np.isnan(metrics.ppl_from_distances(torch.from_numpy(x)))
    mean, lo, hi, count = metrics.trimmed_mean_host(x, 0, 99)
    assert np.isnan(mean) and np.isnan(lo) and np.isnan(hi) and count == 0
    for lo_rank, hi_rank in ((-1, 5), (6, 5), (0, 100)):
        with pytest.raises(ValueError):
            metrics.trimmed_mean_host(x, lo_rank, hi_rank)


# ---- inception score --------------------------------------------------------------------------------------------------------------

def reference_is(probs, num_splits):
    """inception_score.py:30-36 on a float64 copy."""
    gen_probs = np.asarray(probs, np.float64)
    num_gen = len(gen_probs)
    scores = []
    with np.errstate(divide='ignore', invalid='ignore'):
        for i in range(num_splits):
            part = gen_probs[i * num_gen // num_splits:(i + 1) * num_gen // num_splits]
            kl = part * (np.log(part) - np.log(np.mean(part, axis=0, keepdims=True)))
            scores.append(np.exp(np.mean(np.sum(kl, axis=1))))
    return float(np.mean(scores)), float(np.std(scores))


@pytest.mark.parametrize('n,d,splits', [(10, 1, 10), (7, 5, 3), (64, 33, 1)])
def test_host_inception_score_equals_the_reference_lines(n, d, splits):
    p = ref.softmax_rows(n, d, 10 + n)
    want = reference_is(p, splits)
    for given in (p, torch.from_numpy(p)):
        got = metrics.inception_score(given, splits)
        assert abs(got[0] - want[0]) <= 1e-12 * abs(want[0]) and abs(got[1] - want[1]) <= 1e-12 * max(abs(want[1]), abs(want[0]))
    kl, _ = ref.inception_kl(p, splits)
    assert np.allclose(metrics.inception_kl(p, splits), kl.astype(np.float64), rtol=1e-12, atol=1e-15)
    if d == 1:
        assert got[0] == 1.0, 'one class: every kl is exactly 0'


def test_host_inception_score_refuses_and_propagates_nan():
    p = ref.softmax_rows(7, 5, 1)
    with pytest.raises(ValueError):
        metrics.inception_score(p, 8)
    with pytest.raises(ValueError):
        metrics.inception_score(p, 0)
    p[3, 2] = 0
    mean, std = metrics.inception_score(p, 3)
    assert np.isnan(mean) and np.isnan(std) and np.isnan(reference_is(p, 3)[0])
    kl = metrics.inception_kl(p, 3)
    assert np.isnan(kl[1]) and np.isfinite(kl[[0, 2]]).all(), 'only the split that holds the zero'


# ---- label IoU --------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('use_remap', [False, True])
@pytest.mark.parametrize('dtype', [np.int64, np.uint8])
def test_host_label_iou_counts_and_values(dtype, use_remap):
    a, b = label_maps(3, 17, 23, 5)
    a[a == 4] = 0; b[b == 4] = 0                       # class 4 (and what maps to it) absent from both
    b[b == 9] = 1                                      # class 9 present in a only
    a[0, 0, :5] = 40; b[0, 1, :5] = 200                # labels outside the table and outside [0, classes)
    a[1, 2, 3] = 19                                    # 19: inside the 20-entry table (-> 14), outside [0, 19) without it
    remap = REMAP if use_remap else None
    a, b = a.astype(dtype), b.astype(dtype)
    want_counts, _ = ref.label_counts(a, b, 19, remap)
    for given in ((a, b), (torch.from_numpy(a), torch.from_numpy(b))):
        iou, counts = metrics.label_iou(*given, classes=19, remap=remap)
        assert counts.dtype == torch.int32 and iou.dtype == torch.float32 and tuple(counts.shape) == (3, 19, 2)
        assert np.array_equal(counts.numpy(), want_counts)
        want = reference_iou(want_counts)
        assert float((iou - want).abs().max()) <= ref.IOU_BOUND
        assert 0 <= float(iou.min()) and float(iou.max()) <= 1
    absent = [c for c in range(19) if want_counts[:, c, 1].sum() == 0]
    one_sided = [c for c in range(19) if want_counts[:, c, 0].sum() == 0 and want_counts[:, c, 1].sum() > 0]
    assert absent and one_sided, 'the case holds a class absent from both maps and one present in one map only'
    assert want_counts[:, :, 1].sum() < 2 * a.size, 'out-of-range labels light no class'


def test_host_label_iou_against_the_one_hot_lines():
    """The reference's own tensors: scatter to one-hot, then its three lines."""
    a, b = label_maps(2, 9, 11, 6, top=19)
    hot = lambda m: torch.zeros(2, 19, 9, 11).scatter_(1, torch.from_numpy(m)[:, None], 1)
    source, target = hot(a), hot(b)
    want = torch.mean(torch.div(torch.sum(source * target, dim=[2, 3]).float(), torch.sum((source + target) > 0, dim=[2, 3]).float() + 1e-6), dim=1)
    iou, _ = metrics.label_iou(a, b, 19)
    assert float((iou - want).abs().max()) <= ref.IOU_BOUND
    with pytest.raises(ValueError):
        metrics.label_iou(a, b, 33)


# ---- slerp ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('t', [0.0, 1.0, 0.5 + 1e-4])
def test_slerp(t):
    g = torch.Generator().manual_seed(7)
    a, b = torch.randn(5, 32, generator=g, dtype=torch.float64), torch.randn(5, 32, generator=g, dtype=torch.float64)
    an, bn = a / a.norm(dim=-1, keepdim=True), b / b.norm(dim=-1, keepdim=True)
    omega = torch.acos((an * bn).sum(-1, keepdim=True))
    want = (torch.sin((1 - t) * omega) * an + torch.sin(t * omega) * bn) / torch.sin(omega)          # the great-circle definition
    got = metrics.slerp(a, b, torch.full([5, 1], t, dtype=torch.float64))
    assert float((got - want).abs().max()) <= 1e-12
    got32 = metrics.slerp(a.float(), b.float(), torch.full([5, 1], t))
    assert float((got32.double() - want).abs().max()) <= 32 * 2.0 ** -23
    assert float((got.norm(dim=-1) - 1).abs().max()) <= 1e-14


# ---- the sampler ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('space,sampling,crop', [('w', 'end', False), ('z', 'full', True)])
def test_sampler_module_and_callable_paths_agree_on_cpu(space, sampling, crop):
    from training import lpips
    torch.manual_seed(1)
    lp = lpips.LPIPS('vgg', widths=(4, 4, 8, 8, 8)).eval()
    c = camera_labels(2)
    dists = []
    for vgg16 in (lp, ref.feature_callable(lp)):
        s = tiny_sampler(vgg16, space=space, sampling=sampling, crop=crop)
        torch.manual_seed(5)
        with torch.no_grad():
            dists.append(s(c))
        assert s.last_path == 'torch'
    a, b = dists
    assert a.shape == (2,) and a.dtype == torch.float32 and bool((a > 0).all()) and bool(torch.isfinite(a).all())
    # the same fp32 features, subtracted before or after the scaling by sqrt(lin / (h w)): a few roundings of each of the F terms
    assert float(((a - b).abs() / a).max()) <= 1e-3, (a, b)
    # the RNG calls: t, one randn for both latents, then every noise_const in order
    s = tiny_sampler(lp, space=space, sampling=sampling, crop=crop)
    torch.manual_seed(5)
    t = torch.rand([2]); z = torch.randn([4, s.G.z_dim])
    first_noise = next(buf for name, buf in s.G.named_buffers() if name.endswith('.noise_const'))
    want_noise = torch.randn_like(first_noise)
    torch.manual_seed(5)
    with torch.no_grad():
        s.images(c)
    assert torch.equal(first_noise, want_noise) and t.shape == (2,) and z.shape == (4, 32)


def test_compute_ppl_and_multi_gpu_refusal_on_cpu():
    from training import lpips
    torch.manual_seed(1)
    lp = lpips.LPIPS('vgg', widths=(4, 4, 8, 8, 8)).eval()
    s = tiny_sampler(lp)

    def labels():
        while True:
            yield camera_labels(2)
    torch.manual_seed(2)
    value = metrics.compute_ppl(s.G, lp, labels(), num_samples=3, epsilon=1e-2, space='w', sampling='end', crop=False, batch_size=2)
    assert np.isfinite(value) and value > 0
    for call in (lambda: metrics.compute_ppl(s.G, lp, labels(), 3, 1e-2, 'w', 'end', False, 2, num_gpus=2),
                 lambda: metrics.ppl2_wend(s.G, lp, labels(), num_samples=2, num_gpus=2),
                 lambda: metrics.is50k(s.G, None, labels(), num_gen=2, num_gpus=2)):
        with pytest.raises(NotImplementedError, match='num_gpus > 1'):
            call()


def test_miou_module_on_cpu_equals_the_reference_class():
    from training import face_parsing
    torch.manual_seed(3)
    net = face_parsing.BiSeNet(20).eval().requires_grad_(False)
    g = torch.Generator().manual_seed(4)
    a, b = torch.rand(1, 3, 64, 64, generator=g) * 2 - 1, torch.rand(1, 3, 64, 64, generator=g) * 2 - 1
    m = metrics.mIOU(net, size=64)
    got = m(a, b)
    source, target = (face_parsing.scatter(face_parsing.parsing_img(net, x, return_mask=False)[1], label_size=(64, 64)) for x in (a, b))
    want = torch.mean(torch.div(torch.sum(source * target, dim=[2, 3]).float(), torch.sum((source + target) > 0, dim=[2, 3]).float() + 1e-6), dim=1)
    assert got.shape == (1,) and float((got - want).abs().max()) <= ref.IOU_BOUND


# ---- C ABI ------------------------------------------------------------------------------------------------------------------------

NAMES = ('ide3d_ppl_prep', 'ide3d_lpips_pair_distances', 'ide3d_trimmed_mean', 'ide3d_inception_score', 'ide3d_label_iou')
QUERIES = ('ide3d_lpips_pair_workspace_bytes', 'ide3d_inception_score_workspace_bytes')


def test_c_abi_declarations_and_workspace_arithmetic():
    from torch_utils import hip_plugin
    with open(os.path.join(ROOT, 'include', 'ide3d_hip.h')) as f:
        h = f.read()
    for cite in ('perceptual_path_length.py:71-83', 'perceptual_path_length.py:89', 'perceptual_path_length.py:119-122', 'inception_score.py:31-34',
                 'calc_losses_on_images.py:28-30'):
        assert cite in h, cite
    path = hip_plugin.lib_path()
    assert os.path.isfile(path), f'{path} missing: run __graft_entry__.build()'
    lib, loaded = ctypes.CDLL(path), hip_plugin.load()
    for name in NAMES + QUERIES:
        assert name in hip_plugin.EXPORTED_SYMBOLS and hasattr(lib, name), name
        m = re.search(r'(int64_t|int) %s\(([^)]*)\);' % name, h)
        assert m, name
        assert len(getattr(loaded, name).argtypes) == len(m.group(2).split(',')), name
        if name in NAMES:
            assert m.group(2).rstrip().endswith('void* stream'), name
    assert hip_plugin.PLUGINS['metrics_eval_plugin'] is hip_plugin.MetricsEvalPlugin
    assert loaded.ide3d_abi_version() == 8 == hip_plugin._ABI_VERSION, 'entry points were only added'
    ws = loaded.ide3d_inception_score_workspace_bytes
    cd = lambda a, b: -(-a // b)
    for n, d, s in ((10, 1, 10), (7, 5, 3), (257, 1008, 10), (50000, 1008, 10), (1 << 22, 8192, 1)):
        chunks = min(256, cd(cd(n, s), 32))
        assert ws(n, d, s) == 8 * (s * d + s * chunks * d + s * chunks), (n, d, s)
    assert ws(3, 5, 4) == -1 and ws(10, 0, 1) == -1 and ws(10, 8193, 1) == -1 and ws((1 << 22) + 1, 8, 1) == -1
    taps = (hip_plugin._LpipsTap * 2)()
    taps[0].c, taps[0].h, taps[0].w = 4, 16, 16
    taps[1].c, taps[1].h, taps[1].w = 8, 3, 7
    assert loaded.ide3d_lpips_pair_workspace_bytes(taps, 2, 3) == 8 * 3 * (4 + 1)
    assert loaded.ide3d_lpips_pair_workspace_bytes(taps, 2, 0) == -1 and loaded.ide3d_lpips_pair_workspace_bytes(taps, 9, 1) == -1
    # refusals need no device: every check stands in front of the first launch
    p = ctypes.c_void_p(4096)
    assert loaded.ide3d_trimmed_mean(p, 10, 3, 2, p, None) == -1 and loaded.ide3d_trimmed_mean(p, 10, 0, 10, p, None) == -1
    assert loaded.ide3d_trimmed_mean(None, 10, 0, 9, p, None) == -1 and loaded.ide3d_trimmed_mean(p, 10, 0, 9, ctypes.c_void_p(4100), None) == -1
    assert loaded.ide3d_ppl_prep(p, p, p, p, 1, 8, 8, 0, 0, 8, 8, 3, 1.0, 0.0, None) == -1, 'f does not divide the window'
    assert loaded.ide3d_ppl_prep(p, p, p, p, 1, 8, 8, 4, 0, 8, 8, 1, 1.0, 0.0, None) == -1, 'the window leaves the image'
    assert loaded.ide3d_inception_score(p, 3, 5, 5, 4, p, 1 << 20, p, None) == -1, 'n < S'
    assert loaded.ide3d_label_iou(p, p, 0, 1, 16, None, 0, 33, p, p, None) == -1, 'classes > 32'
    assert b'classes' in loaded.ide3d_last_error()
