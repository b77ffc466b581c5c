"""The arithmetic of PPL, Inception Score and mIoU on one GPU (csrc/metrics_eval.hip) at the sizes of the
reference's own workloads, each beside what it replaces, on the same box with the thread count left at the machine's setting:
  trimmed mean   50 000 distances: `ppl_from_distances` (one launch, one host read) against `.cpu().numpy()` + the three numpy
                 lines of perceptual_path_length.py:119-122
  IS             50 000 x 1008 probabilities in 10 splits: `inception_score` against `.cpu().numpy()` + the numpy loop of
                 inception_score.py:31-35
  mIoU           4 pairs of 512^2 parser logits [4, 20, 512, 512]: argmax + `label_iou` with the in-kernel remap against argmax + id_remap +
                 scatter to one-hot + the three ATen lines of calc_losses_on_images.py:28-30
  PPL batch      `PPLSampler.forward` of 2 pairs at the FFHQ configuration (512^2, VGG16 widths, random weights) with the `LPIPS` module
                 (the HIP path) against the same module wrapped as a feature callable (the reference's lines; its features once through
                 the module's fused walk and once through ATen)
Times are host clocks around work that ends in a device synchronise or a host read: [median, min, max] in milliseconds of the repeats after
one warm-up call.  Prints one JSON line and writes it to --out (default profiles/metrics_eval)/bench_metrics_eval.json."""
import argparse, json, os, shutil, statistics, subprocess, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'ide-3d_amd')); sys.path.insert(0, ROOT)
import numpy as np
import torch
from training import face_parsing, lpips, metrics, triplane
from torch_utils import hip_plugin

ap = argparse.ArgumentParser()
ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'metrics_eval'))
ap.add_argument('--n', type=int, default=50000)
ap.add_argument('--skip-ppl', action='store_true')
args = ap.parse_args()
dev = torch.device('cuda:0')
N = args.n


def timed(fn, reps):
    fn(); torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        torch.cuda.synchronize(); t0 = time.perf_counter(); fn(); torch.cuda.synchronize(); out.append((time.perf_counter() - t0) * 1e3)
    return [round(statistics.median(out), 4), round(min(out), 4), round(max(out), 4)]


def smi():
    """GPU 0's clocks and power as `rocm-smi --showclocks --showpower --json` reads them while work is queued (read only)."""
    exe = shutil.which('rocm-smi') or '/opt/rocm/bin/rocm-smi'
    if not os.path.exists(exe):
        return None
    try:
        for _ in range(20):
            metrics.inception_score(probs, 10)
        o = subprocess.run([exe, '--showclocks', '--showpower', '--json'], capture_output=True, text=True, timeout=20)
        torch.cuda.synchronize()
        card = next(iter(json.loads(o.stdout).values()))
        return {k: v for k, v in card.items() if any(w in k.lower() for w in ('sclk', 'mclk', 'power'))}
    except Exception as e:      # noqa: BLE001 - diagnostics only
        return {'error': f'{type(e).__name__}: {e}'[:120]}


g = torch.Generator(device=dev).manual_seed(0)
res = {'n': N, 'threads': torch.get_num_threads()}

# ---- trimmed mean ----
dist = torch.randn([N], device=dev, generator=g).square() * 300


def reference_ppl():
    d = dist.cpu().numpy()
    lo = np.percentile(d, 1, method='lower')
    hi = np.percentile(d, 99, method='higher')
    return float(np.extract(np.logical_and(d >= lo, d <= hi), d).mean())


r = {'device_ms': timed(lambda: metrics.ppl_from_distances(dist), 30), 'reference_cpu_numpy_ms': timed(reference_ppl, 30),
     'values': [metrics.ppl_from_distances(dist), reference_ppl()], 'bytes_read': 5 * 4 * N}
res['trimmed_mean_50000'] = r
print('trimmed mean', r, file=sys.stderr, flush=True)

# ---- inception score ----
D, SPLITS = 1008, 10
probs = torch.softmax(torch.randn([N, D], device=dev, generator=g) * 2, dim=1)


def reference_is():
    gen_probs = probs.cpu().numpy()
    scores = []
    for i in range(SPLITS):
        part = gen_probs[i * N // SPLITS:(i + 1) * N // SPLITS]
        kl = part * (np.log(part) - np.log(np.mean(part, axis=0, keepdims=True)))
        scores.append(np.exp(np.mean(np.sum(kl, axis=1))))
    return float(np.mean(scores)), float(np.std(scores))


r = {'device_ms': timed(lambda: metrics.inception_score(probs, SPLITS), 10), 'reference_cpu_numpy_fp32_ms': timed(reference_is, 3),
     'values': [list(metrics.inception_score(probs, SPLITS)), list(reference_is())], 'bytes_read': 2 * 4 * N * D}
r['device_read_gb_per_s_end_to_end'] = round(r['bytes_read'] / (r['device_ms'][0] * 1e-3) / 1e9, 1)
res['inception_score_50000x1008'] = r
print('inception score', r, file=sys.stderr, flush=True)

# ---- mIoU ----
logits_a = torch.randn([4, 20, 512, 512], device=dev, generator=g)
logits_b = logits_a + 0.8 * torch.randn([4, 20, 512, 512], device=dev, generator=g)
table = torch.tensor(face_parsing.REMAP, dtype=torch.int32, device=dev)


def device_miou():
    return metrics.label_iou(logits_a.argmax(1), logits_b.argmax(1), 19, table)[0]


def reference_miou():
    source, target = (face_parsing.scatter(face_parsing.id_remap(l.argmax(1, keepdim=True), 'celebahq')) for l in (logits_a, logits_b))
    return torch.mean(torch.div(torch.sum(source * target, dim=[2, 3]).float(), torch.sum((source + target) > 0, dim=[2, 3]).float() + 1e-6), dim=1)


la, lb = logits_a.argmax(1), logits_b.argmax(1)
r = {'device_argmax_and_label_iou_ms': timed(device_miou, 30), 'device_label_iou_alone_ms': timed(lambda: metrics.label_iou(la, lb, 19, table), 30),
     'reference_aten_ms': timed(reference_miou, 30), 'values': [device_miou().tolist(), reference_miou().tolist()], 'label_bytes_read': 2 * 8 * la.numel()}
res['miou_4x512x512'] = r
print('mIoU', r, file=sys.stderr, flush=True)
del logits_a, logits_b

# ---- a PPL batch ----
class FeatureCallable(torch.nn.Module):
    """An `LPIPS` module with the reference detector's call shape: sqrt(lin / (h w)) u of every tap, concatenated."""

    def __init__(self, lp):
        super().__init__()
        self.lp = lp

    def forward(self, img, resize_images=False, return_lpips=True):
        feats = self.lp.features(img * (2 / 255) - 1)
        return torch.cat([(u * (l[1].weight / (u.shape[2] * u.shape[3])).sqrt()).flatten(1) for u, l in zip(feats, self.lp.lin)], dim=1)


if not args.skip_ppl:
    torch.manual_seed(0)
    G = triplane.TriPlaneGenerator().eval().requires_grad_(False).to(dev)
    lp = lpips.LPIPS('vgg').eval().to(dev)
    c = torch.cat([triplane.camera_label(0.1, device=dev), triplane.camera_label(-0.2, device=dev)])
    kw = dict(G=G, G_kwargs={}, epsilon=1e-4, space='w', sampling='end', crop=False)
    hip = metrics.PPLSampler(vgg16=lp, **kw).eval().requires_grad_(False).to(dev)
    call = metrics.PPLSampler(vgg16=FeatureCallable(lp), **kw).eval().requires_grad_(False).to(dev)
    r = {'resolution': G.img_resolution, 'pairs': 2}
    with torch.no_grad():
        img = hip.images(c)
        r['hip_path_forward_ms'] = timed(lambda: hip(c), 10)
        r['hip_path_distances_alone_ms'] = timed(lambda: hip.distances(img), 10)
        assert hip.last_path == 'hip'
        r['callable_fused_features_forward_ms'] = timed(lambda: call(c), 10)
        r['callable_fused_features_distances_alone_ms'] = timed(lambda: call.distances(img), 10)
        lpips.fused = False
        r['callable_aten_features_forward_ms'] = timed(lambda: call(c), 10)
        r['callable_aten_features_distances_alone_ms'] = timed(lambda: call.distances(img), 10)
        lpips.fused = True
        r['values'] = [hip.distances(img).tolist(), call.distances(img).tolist()]
    res['ppl_batch_2x2_ffhq'] = r
    print('PPL batch', r, file=sys.stderr, flush=True)

res['gpu_clock_and_power'] = smi()
names = ('ppl_prep', 'lpips_pair_distances', 'trimmed_mean', 'inception_score', 'label_iou')
line = json.dumps(dict(metric='PPL, Inception Score and mIoU arithmetic', device=torch.cuda.get_device_name(0),
                       timing='milliseconds, [median, min, max] of the repeats', **res, native_launches={k: hip_plugin.CALLS.get(k, 0) for k in names}))
print(line)
os.makedirs(args.out, exist_ok=True)
with open(os.path.join(args.out, 'bench_metrics_eval.json'), 'w') as f:
    f.write(line + '\n')
