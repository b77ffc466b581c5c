"""csrc/metrics_eval.hip on the GPU against the float64 / longdouble restatement of tests/metrics_eval_ref.py: the
windowed prep, the pair distances, the trimmed mean, the Inception Score sums, the label IoU, refusals, and one end-to-end run of the PPL
sampler, `compute_ppl`, `is50k` and `mIOU`.  Every output and workspace sits in a guarded buffer; every bound is derived in the ref file."""
import ctypes

import numpy as np
import pytest
import torch

import metrics_eval_ref as ref
from test_gpu_metrics import GUARD, guarded, untouched_outside
from metrics_eval_ref import REMAP, camera_labels, label_maps, reference_iou, tiny_sampler, trimmed_cases
from training import metrics

pytestmark = pytest.mark.gpu

MEAN, STD = (-.030, -.088, -.188), (.458, .448, .450)


def P():
    from torch_utils import hip_plugin
    return hip_plugin.MetricsEvalPlugin


def calls(name):
    from torch_utils import hip_plugin
    return hip_plugin.CALLS.get(name, 0)


def f32_view(nbytes, dev):
    big, v = guarded(nbytes, dev)
    return big, v.view(torch.float32)


# ---- ppl prep ---------------------------------------------------------------------------------------------------------------------

def prep_input(n, H, W, seed, dev):
    x = (torch.rand(n, 3, H, W, generator=torch.Generator().manual_seed(seed)) * 2 - 1).contiguous()
    return x, x.to(dev), torch.tensor(MEAN, device=dev), torch.tensor(STD, device=dev)


def test_ppl_prep_full_window_is_bit_equal_to_lpips_prep(gpu_device):
    from torch_utils import hip_plugin
    _, xd, mean, std = prep_input(2, 32, 48, 1, gpu_device)
    for scale, shift in ((1.0, 0.0), (2.0 / 255.0, -1.0)):
        want = hip_plugin.LpipsPlugin.prep(xd * (1 if shift == 0 else 127.5), mean, std, 2, scale, shift)
        big, out = f32_view(4 * want.numel(), gpu_device)
        before = calls('ppl_prep')
        got = P().ppl_prep(xd * (1 if shift == 0 else 127.5), mean, std, None, 2, scale, shift, out=out)
        torch.cuda.synchronize()
        assert calls('ppl_prep') == before + 1 and untouched_outside(big, 4 * want.numel())
        assert torch.equal(got[:want.numel()].view_as(want), want)


@pytest.mark.parametrize('n,H,W,f,window', [(1, 8, 8, 1, (7, 7, 1, 1)), (2, 64, 64, 2, (24, 16, 32, 32)), (3, 40, 24, 4, (4, 8, 32, 12))])
def test_ppl_prep_windows(gpu_device, n, H, W, f, window):
    x, xd, mean, std = prep_input(n, H, W, 2 + H, gpu_device)
    want, bound = ref.ppl_prep(x.numpy(), MEAN, STD, window, f, 0.75, 0.125)
    runs = []
    for _ in range(2):
        big, out = f32_view(4 * want.size, gpu_device)
        got = P().ppl_prep(xd, mean, std, window, f, 0.75, 0.125, out=out)
        torch.cuda.synchronize()
        assert untouched_outside(big, 4 * want.size)
        runs.append(got[:want.size].cpu().numpy().reshape(want.shape).copy())
    assert np.array_equal(runs[0], runs[1]), 'two runs are bit-equal'
    err = np.abs(runs[0].astype(np.float64) - want)
    print(f'ppl_prep {n} x {H} x {W}, f = {f}, window {window}: largest error / bound {float((err / bound).max()):.4f}')
    assert (err <= bound).all()


# ---- pair distances ---------------------------------------------------------------------------------------------------------------

PAIR_SHAPES = {'one': [(1, 1, 1)], 'five': [(4, 16, 16), (8, 8, 8), (16, 4, 4), (16, 2, 2), (16, 1, 1)], 'odd': [(5, 3, 7)]}


def run_pairs(taps, lins, scale, dev):
    acts, lv = [torch.from_numpy(t).to(dev) for t in taps], [torch.from_numpy(l).to(dev) for l in lins]
    n = taps[0].shape[0] // 2
    nbytes = P().pair_workspace_bytes(acts, lv)
    big_ws, ws = guarded(nbytes, dev)
    big_d, dist = f32_view(4 * n, dev)
    before = calls('lpips_pair_distances')
    P().lpips_pair_distances(acts, lv, scale, workspace=ws, dist=dist)
    torch.cuda.synchronize()
    assert calls('lpips_pair_distances') == before + 1
    assert untouched_outside(big_ws, nbytes) and untouched_outside(big_d, 4 * n)
    return dist.cpu().numpy().copy()


@pytest.mark.parametrize('n', [1, 3])
@pytest.mark.parametrize('name', sorted(PAIR_SHAPES))
def test_pair_distances(gpu_device, name, n):
    taps, lins = ref.pair_taps(PAIR_SHAPES[name], n, 7 + n)
    scale = 1e4
    want, bound = ref.pair_distances(taps, lins, scale)
    got = run_pairs(taps, lins, scale, gpu_device)
    assert np.array_equal(got, run_pairs(taps, lins, scale, gpu_device)), 'two runs are bit-equal'
    err = np.abs(got.astype(np.float64) - want)
    print(f'pair distances {name}, n = {n}: {got.tolist()} largest error / bound {float((err / bound).max()):.4f}')
    assert (err <= bound).all() and np.isfinite(got).all()
    same, lins = ref.pair_taps(PAIR_SHAPES[name], n, 7 + n, identical=True)
    assert (run_pairs(same, lins, 1e8, gpu_device) == 0).all(), 'identical image pairs give exactly 0'


# ---- trimmed mean -----------------------------------------------------------------------------------------------------------------

def device_trimmed(x, lo_rank, hi_rank, dev):
    xd = torch.from_numpy(x).to(dev)
    big, v = guarded(32, dev)
    before = calls('trimmed_mean')
    P().trimmed_mean(xd, lo_rank, hi_rank, out=v.view(torch.float64))
    torch.cuda.synchronize()
    assert calls('trimmed_mean') == before + 1 and untouched_outside(big, 32)
    return v.view(torch.float64).cpu().numpy().copy()


def gpu_trimmed_cases():
    rng = np.random.RandomState(9)
    cases = trimmed_cases()          # n = 1, 2, 100, 101, 1000, ties across both ranks, all equal, one inf, +-0 and negatives
    for n in (1023, 1024, 1025, 50000):
        cases[f'n{n}'] = (rng.randn(n) * rng.choice([1e-3, 1.0, 1e3], n)).astype(np.float32)
    return cases


@pytest.mark.parametrize('name', sorted(gpu_trimmed_cases()))
def test_trimmed_mean(gpu_device, name):
    x = gpu_trimmed_cases()[name]
    lo_rank, hi_rank = metrics.percentile_ranks(len(x))
    got = device_trimmed(x, lo_rank, hi_rank, gpu_device)
    assert np.array_equal(got, device_trimmed(x, lo_rank, hi_rank, gpu_device)), 'two runs are bit-equal'
    mean, lo, hi, count, sum_abs = ref.trimmed_mean(x, lo_rank, hi_rank)
    assert (got[1], got[2], got[3]) == (lo, hi, count), (name, got, lo, hi, count)
    if np.isinf(float(mean)):
        assert got[0] == float(mean)
    else:
        err = abs(np.longdouble(got[0]) - mean)
        print(f'trimmed mean {name}: {got.tolist()}, error {float(err):.3e}, bound {count * 2.0 ** -52 * sum_abs:.3e}')
        assert err <= count * 2.0 ** -52 * sum_abs
    assert metrics.ppl_from_distances(torch.from_numpy(x).to(gpu_device)) == got[0]
    if name == 'n101':          # other ranks than the percentiles': the extremes and the median
        for lo_rank, hi_rank in ((0, 100), (50, 50), (100, 100)):
            mean, lo, hi, count, sum_abs = ref.trimmed_mean(x, lo_rank, hi_rank)
            got = device_trimmed(x, lo_rank, hi_rank, gpu_device)
            assert (got[1], got[2], got[3]) == (lo, hi, count) and abs(np.longdouble(got[0]) - mean) <= count * 2.0 ** -52 * sum_abs


def test_trimmed_mean_nan(gpu_device):
    x = np.random.RandomState(4).randn(1500).astype(np.float32)
    x[1234] = np.nan
    got = device_trimmed(x, *metrics.percentile_ranks(len(x)), gpu_device)
    assert np.isnan(got[:3]).all() and got[3] == 0
    assert np.isnan(metrics.ppl_from_distances(torch.from_numpy(x).to(gpu_device)))


# ---- inception score --------------------------------------------------------------------------------------------------------------

def device_kl(p, splits, stride, dev):
    n, d = p.shape
    wide = torch.full([n, stride], 0.5, dtype=torch.float32, device=dev)
    wide[:, :d] = torch.from_numpy(p).to(dev)
    nbytes = P().inception_workspace_bytes(n, d, splits)
    big_ws, ws = guarded(nbytes, dev)
    big_k, v = guarded(8 * splits, dev)
    before = calls('inception_score')
    P().inception_score(wide[:, :d], splits, workspace=ws, kl=v.view(torch.float64))
    torch.cuda.synchronize()
    assert calls('inception_score') == before + 1 and untouched_outside(big_ws, nbytes) and untouched_outside(big_k, 8 * splits)
    return v.view(torch.float64).cpu().numpy().copy()


@pytest.mark.parametrize('n,d,splits,stride', [(10, 1, 10, 1), (7, 5, 3, 5), (257, 1008, 10, 1008), (129, 33, 1, 40)])
def test_inception_score(gpu_device, n, d, splits, stride):
    p = ref.softmax_rows(n, d, 10 + n)
    want, bound = ref.inception_kl(p, splits)
    got = device_kl(p, splits, stride, gpu_device)
    assert np.array_equal(got, device_kl(p, splits, stride, gpu_device)), 'two runs are bit-equal'
    err = np.abs(got.astype(np.longdouble) - want).astype(np.float64)
    print(f'inception kl {n} x {d} in {splits}: largest error / bound {float((err / np.maximum(bound, 1e-300)).max()):.4f}')
    assert (err <= bound).all()
    mean, std = metrics.inception_score(torch.from_numpy(p).to(gpu_device), splits)
    assert (mean, std) == (float(np.mean(np.exp(got))), float(np.std(np.exp(got))))
    host = metrics.inception_score(p, splits)
    assert abs(mean - host[0]) <= 1e-12 * host[0]


def test_inception_score_zero_probability_gives_nan(gpu_device):
    p = ref.softmax_rows(70, 33, 3)
    p[40, 7] = 0
    got = device_kl(p, 5, 33, gpu_device)
    assert np.isnan(got[2]) and np.isfinite(got[[0, 1, 3, 4]]).all(), 'only the split that holds the zero'
    with pytest.raises(ValueError):
        metrics.inception_score(torch.from_numpy(p[:3]).to(gpu_device), 4)


# ---- label IoU --------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('use_remap', [False, True])
@pytest.mark.parametrize('dtype', [torch.int64, torch.uint8])
@pytest.mark.parametrize('n,h,w', [(1, 1, 1), (3, 17, 23), (2, 512, 512)])
def test_label_iou(gpu_device, n, h, w, dtype, use_remap):
    a, b = label_maps(n, h, w, 5 + h)
    if h > 1:
        a[0, 0, :5] = 40; b[0, 1, :5] = 200; a[-1, 2, 3] = 19          # outside the table, outside [0, classes), and 19 (inside the table only)
    remap = REMAP if use_remap else None
    want, _ = ref.label_counts(a, b, 19, remap)
    ad, bd = torch.from_numpy(a).to(gpu_device).to(dtype), torch.from_numpy(b).to(gpu_device).to(dtype)
    table = torch.tensor(REMAP, dtype=torch.int32, device=gpu_device) if use_remap else None
    big_c, vc = guarded(4 * n * 19 * 2, gpu_device)
    big_i, vi = guarded(4 * n, gpu_device)
    before = calls('label_iou')
    iou, counts = P().label_iou(ad, bd, 19, table, counts=vc.view(torch.int32), iou=vi.view(torch.float32))
    torch.cuda.synchronize()
    assert calls('label_iou') == before + 1 and untouched_outside(big_c, 4 * n * 19 * 2) and untouched_outside(big_i, 4 * n)
    counts = counts.view(n, 19, 2).cpu().numpy()
    assert np.array_equal(counts, want), 'counts are exactly the one-hot sums'
    assert float((iou.cpu() - reference_iou(want)).abs().max()) <= ref.IOU_BOUND
    iou2, counts2 = metrics.label_iou(ad, bd, 19, remap)
    assert torch.equal(iou2, iou) and np.array_equal(counts2.cpu().numpy(), want)


# ---- refusals ---------------------------------------------------------------------------------------------------------------------

def test_refusals_launch_nothing(gpu_device):
    from torch_utils import hip_plugin
    lib = hip_plugin.load()
    f = torch.rand([2, 3, 8, 8], dtype=torch.float32, device=gpu_device)
    lab = torch.zeros([2, 64], dtype=torch.int64, device=gpu_device)
    ws = torch.full([1 << 16], GUARD, dtype=torch.uint8, device=gpu_device)
    out = torch.full([1 << 12], GUARD, dtype=torch.uint8, device=gpu_device)
    p = lambda t, o=0: ctypes.c_void_p(t.data_ptr() + o)
    taps = (hip_plugin._LpipsTap * 1)()
    taps[0].a, taps[0].lin, taps[0].c, taps[0].h, taps[0].w = f.data_ptr(), f.data_ptr(), 3, 8, 8
    no_lin = (hip_plugin._LpipsTap * 1)()
    no_lin[0].a, no_lin[0].c, no_lin[0].h, no_lin[0].w = f.data_ptr(), 3, 8, 8
    need = lib.ide3d_lpips_pair_workspace_bytes(taps, 1, 1)
    is_need = lib.ide3d_inception_score_workspace_bytes(8, 8, 2)
    prep = lambda *a: lib.ide3d_ppl_prep(p(f), p(out), p(f), p(f), *a, 1.0, 0.0, None)
    before = dict(hip_plugin.CALLS)
    bad = dict(
        prep_null=lib.ide3d_ppl_prep(p(f), None, p(f), p(f), 2, 8, 8, 0, 0, 8, 8, 2, 1.0, 0.0, None),
        prep_misaligned=lib.ide3d_ppl_prep(p(f), p(out, 2), p(f), p(f), 2, 8, 8, 0, 0, 8, 8, 2, 1.0, 0.0, None),
        prep_f=prep(2, 8, 8, 0, 0, 8, 6, 4), prep_f0=prep(2, 8, 8, 0, 0, 8, 8, 0), prep_outside=prep(2, 8, 8, 2, 0, 8, 8, 1),
        prep_negative=prep(2, 8, 8, 0, -1, 4, 4, 1), prep_empty=prep(2, 8, 8, 0, 0, 0, 8, 1),
        pair_null=lib.ide3d_lpips_pair_distances(taps, 1, 1, 1.0, None, need, p(out), None),
        pair_lin=lib.ide3d_lpips_pair_distances(no_lin, 1, 1, 1.0, p(ws), need, p(out), None),
        pair_short=lib.ide3d_lpips_pair_distances(taps, 1, 1, 1.0, p(ws), need - 1, p(out), None),
        pair_misaligned=lib.ide3d_lpips_pair_distances(taps, 1, 1, 1.0, p(ws, 4), need, p(out), None),
        pair_n=lib.ide3d_lpips_pair_distances(taps, 1, 0, 1.0, p(ws), need, p(out), None),
        tm_null=lib.ide3d_trimmed_mean(p(f), 64, 0, 63, None, None), tm_misaligned=lib.ide3d_trimmed_mean(p(f), 64, 0, 63, p(out, 4), None),
        tm_hi=lib.ide3d_trimmed_mean(p(f), 64, 0, 64, p(out), None), tm_lo=lib.ide3d_trimmed_mean(p(f), 64, -1, 5, p(out), None),
        tm_order=lib.ide3d_trimmed_mean(p(f), 64, 6, 5, p(out), None), tm_n=lib.ide3d_trimmed_mean(p(f), (1 << 24) + 1, 0, 5, p(out), None),
        is_splits=lib.ide3d_inception_score(p(f), 3, 8, 8, 4, p(ws), ws.numel(), p(out), None),
        is_short=lib.ide3d_inception_score(p(f), 8, 8, 8, 2, p(ws), is_need - 1, p(out), None),
        is_misaligned=lib.ide3d_inception_score(p(f), 8, 8, 8, 2, p(ws, 8), is_need, p(out), None),
        is_stride=lib.ide3d_inception_score(p(f), 8, 8, 7, 2, p(ws), ws.numel(), p(out), None),
        is_null=lib.ide3d_inception_score(p(f), 8, 8, 8, 2, p(ws), ws.numel(), None, None),
        iou_classes=lib.ide3d_label_iou(p(lab), p(lab), 0, 2, 64, None, 0, 33, p(out), p(out, 2048), None),
        iou_dtype=lib.ide3d_label_iou(p(lab), p(lab), 2, 2, 64, None, 0, 19, p(out), p(out, 2048), None),
        iou_null=lib.ide3d_label_iou(p(lab), None, 0, 2, 64, None, 0, 19, p(out), p(out, 2048), None),
        iou_table=lib.ide3d_label_iou(p(lab), p(lab), 0, 2, 64, None, 20, 19, p(out), p(out, 2048), None),
        iou_misaligned=lib.ide3d_label_iou(p(lab, 4), p(lab), 0, 2, 60, None, 0, 19, p(out), p(out, 2048), None))
    assert all(rc == -1 for rc in bad.values()), bad
    torch.cuda.synchronize()
    assert bool((ws == GUARD).all()) and bool((out == GUARD).all())
    assert dict(hip_plugin.CALLS) == before
    with pytest.raises(RuntimeError):
        P().trimmed_mean(f.reshape(-1), 5, 4)
    with pytest.raises(RuntimeError):
        P().ppl_prep(f, f[0, :, 0, 0], f[0, :, 0, 0], (0, 0, 8, 8), 3)
    with pytest.raises(RuntimeError):
        P().label_iou(lab, lab, 33)
    assert dict(hip_plugin.CALLS) == before


# ---- end to end -------------------------------------------------------------------------------------------------------------------

def float64_distances(img, lp64, window, f, eps):
    """The sampler's distance in float64 on the CPU: crop, area mean, z-score, the taps of a float64 copy of the net, the definition."""
    from training import lpips
    y0, x0, h, w = window
    z = lpips._prep_torch(img.double().cpu()[:, :, y0:y0 + h, x0:x0 + w], lp64.net, f, 1.0, 0.0)
    dist = 0
    for a, l in zip(lp64.net.taps(z), lp64.lin):
        u0, u1 = (a / (a.square().sum(dim=1, keepdim=True).sqrt() + 1e-10)).chunk(2)
        dist = dist + ((u0 - u1).square() * l[1].weight).sum(dim=1).mean(dim=(1, 2))
    return dist / eps ** 2


@pytest.mark.parametrize('eps', [1e-4, 1e-2])
def test_sampler_takes_the_hip_path_and_matches_float64(gpu_device, eps):
    """Both paths render the same images (same RNG state, deterministic kernels: asserted), so the float64 evaluation starts from those
    images: it covers everything in which the two paths differ.  Measured on MI355X (printed below): largest
    relative error of the HIP path 1.8e-6 at eps = 1e-4 and 1.5e-6 at eps = 1e-2, of the ATen fp32 path 3.1e-6 and 3.5e-6."""
    import copy
    from training import lpips
    torch.manual_seed(1)
    lp = lpips.LPIPS('vgg', widths=(4, 4, 8, 8, 8)).eval().to(gpu_device)
    lp64 = copy.deepcopy(lp).cpu().double()
    c = camera_labels(2, gpu_device)
    hip, aten = tiny_sampler(lp, gpu_device, epsilon=eps), tiny_sampler(ref.feature_callable(lp), gpu_device, epsilon=eps)
    saved = lpips.fused
    try:
        out = {}
        for name, s in (('hip', hip), ('aten', aten)):
            lpips.fused = name == 'hip'          # the callable's own features through ATen: the fp32 torch path the HIP path is measured against
            torch.manual_seed(11)
            before = (calls('ppl_prep'), calls('lpips_pair_distances'), calls('lpips_head'))
            with torch.no_grad():
                img = s.images(c)
                dist = s.distances(img)
            delta = (calls('ppl_prep') - before[0], calls('lpips_pair_distances') - before[1], calls('lpips_head') - before[2])
            out[name] = (img, dist, delta)
            assert s.last_path == ('hip' if name == 'hip' else 'torch')
    finally:
        lpips.fused = saved
    assert out['hip'][2] == (1, 1, 0), 'one prep, one pair-distance call, no normalised taps'
    assert out['aten'][2] == (0, 0, 0)
    assert torch.equal(out['hip'][0], out['aten'][0]), 'the same RNG state gives the same images'
    img = out['hip'][0]
    assert img.shape == (4, 3, 64, 64)
    want = float64_distances(img, lp64, (0, 0, 64, 64), 1, eps)
    err = {name: float(((out[name][1].double().cpu() - want).abs() / want).max()) for name in out}
    print(f'PPL sampler at eps = {eps}: distances {want.tolist()}; largest relative error of the HIP path {err["hip"]:.3e}, of the ATen fp32 path {err["aten"]:.3e}')
    assert bool((want > 0).all())
    assert err['hip'] <= 4 * err['aten'], err
    # The two paths against each other.  Each feature carries an fp32 error of about sqrt(K) 2^-24 of its size from every one of 13
    # convolutions of K <= 72 terms: at most 13 sqrt(72) 2^-24 = 6.6e-6 |u| in all.  The pair's features differ by about eps |u| (w moves by eps
    # of the way between two latents), so a distance has a relative error of about 2 x 6.6e-6 / eps, and two paths differ by twice that.
    between = float(((out['hip'][1] - out['aten'][1]).abs().double().cpu() / want).max())
    print(f'PPL sampler at eps = {eps}: largest relative difference between the HIP and the callable path {between:.3e}, allowed {2.64e-5 / eps:.3e}')
    assert between <= 2.64e-5 / eps


def test_compute_ppl_is50k_and_miou_end_to_end(gpu_device):
    from training import face_parsing, lpips, triplane
    torch.manual_seed(1)
    lp = lpips.LPIPS('vgg', widths=(4, 4, 8, 8, 8)).eval().to(gpu_device)
    torch.manual_seed(0)
    G = triplane.TriPlaneGenerator(triplane.tiny_spec()).eval().requires_grad_(False).to(gpu_device)

    def labels(n):
        while True:
            yield camera_labels(n, gpu_device)

    before = (calls('lpips_pair_distances'), calls('trimmed_mean'))
    torch.manual_seed(3)
    value = metrics.compute_ppl(G, lp, labels(2), num_samples=8, epsilon=1e-2, space='w', sampling='end', crop=False, batch_size=2)
    assert np.isfinite(value) and value > 0
    assert (calls('lpips_pair_distances') - before[0], calls('trimmed_mean') - before[1]) == (4, 1)
    print(f'compute_ppl of 8 samples: {value!r}')

    class Softmax(torch.nn.Module):
        """A stand-in for the Inception network: one random projection of the pooled image and a softmax."""
        def __init__(self):
            super().__init__()
            self.w = torch.nn.Parameter(torch.randn(3 * 16, 40, generator=torch.Generator().manual_seed(5)))

        def forward(self, images, no_output_bias=False):
            assert no_output_bias and images.dtype == torch.uint8
            x = torch.nn.functional.adaptive_avg_pool2d(images.float() / 127.5 - 1, 4).flatten(1)
            return torch.softmax(x @ self.w, dim=1)

    detector = Softmax().to(gpu_device).requires_grad_(False)
    torch.manual_seed(4)
    before = calls('inception_score')
    mean, std = metrics.is50k(G, detector, labels(4), num_gen=64, num_splits=4, batch_size=16, batch_gen=4, G_kwargs=dict(noise_mode='const'))
    assert calls('inception_score') == before + 1
    torch.manual_seed(4)
    probs = metrics.feature_stats_for_generator(G, detector, labels(4), max_items=64, batch_size=16, batch_gen=4, G_kwargs=dict(noise_mode='const'),
                                                detector_kwargs=dict(no_output_bias=True), capture_all=True).get_all()
    host = metrics.inception_score(probs, 4)
    print(f'is50k of 64 images in 4 splits: {(mean, std)!r}, host definition {host!r}')
    assert probs.shape == (64, 40) and abs(mean - host[0]) <= 1e-12 * host[0] and abs(std - host[1]) <= 1e-12 * host[0]

    torch.manual_seed(6)
    net = face_parsing.BiSeNet(20).eval().requires_grad_(False).to(gpu_device)
    g = torch.Generator().manual_seed(7)
    a, b = (torch.rand(2, 3, 64, 64, generator=g) * 2 - 1).to(gpu_device), (torch.rand(2, 3, 64, 64, generator=g) * 2 - 1).to(gpu_device)
    m = metrics.mIOU(net).to(gpu_device)
    la, lb = m.labels(a), m.labels(b)          # computed once, fed to both
    assert la.shape == (2, 512, 512) and la.dtype == torch.int64
    before = calls('label_iou')
    iou, counts = metrics.label_iou(la, lb, 19, m.remap)
    assert calls('label_iou') == before + 1
    source, target = (face_parsing.scatter(face_parsing.id_remap(t[:, None])) for t in (la, lb))
    inter, union = torch.sum(source * target, dim=[2, 3]), torch.sum((source + target) > 0, dim=[2, 3])
    assert torch.equal(counts[:, :, 0].long(), inter.long()) and torch.equal(counts[:, :, 1].long(), union.long())
    want = torch.mean(torch.div(inter.float(), union.float() + 1e-6), dim=1)
    assert float((iou - want).abs().max()) <= ref.IOU_BOUND
    got = m(a, b)
    assert got.shape == (2,) and got.is_cuda and torch.equal(got, iou), 'the module is the same labels through the same kernel'
