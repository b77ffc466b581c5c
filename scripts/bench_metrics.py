"""What calc_metrics.py does with a detector's features, on one GPU (csrc/metrics.hip), at the sizes of fid50k_full,
kid50k_full and pr50k3_full on random features: the float64 moments of 50 000 x 2048 (appended in batches of 64, and in one call), the KID
sums of 100 subsets of 1000 from 50 000 x 2048, and precision / recall (k = 3) of 50 000 x 4096 against 50 000 x 4096.  Beside each, on the
same box with the thread count left at the machine's setting, the reference's way of computing it:
  moments    `x.cpu().numpy()` then numpy float64 `x64.T @ x64` per batch of 64 (metric_utils.py:107-134)
  KID        the numpy loop of kernel_inception_distance.py:37-42 on the float32 features
  P/R        fp16 `torch.cdist` in column batches of 10 000, `.cpu()`, `kthvalue` / `<=` on the host (precision_recall.py:19-59)
The host baselines run on the stated fraction of their work and are scaled (`baseline_fraction`, `scaled: true`).  Times are host clocks
around work that ends in a device synchronise: [median, min, max] of the repeats after one warm-up call.  Prints one JSON line and writes it to
--out (default profiles/metrics)/bench_metrics.json."""
import argparse, json, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'ide-3d_amd')); sys.path.insert(0, ROOT)
import numpy as np
import torch
from training import metrics
from torch_utils import hip_plugin

ap = argparse.ArgumentParser()
ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'metrics'))
ap.add_argument('--n', type=int, default=50000)
args = ap.parse_args()
dev = torch.device('cuda:0')
N, D_INC, D_VGG, K = args.n, 2048, 4096, 3
SUBSETS, M = 100, min(1000, N)


def timed(fn, reps):
    fn(); torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        torch.cuda.synchronize(); t0 = time.perf_counter(); fn(); torch.cuda.synchronize(); out.append(time.perf_counter() - t0)
    return [round(statistics.median(out), 4), round(min(out), 4), round(max(out), 4)]


def once(fn):
    torch.cuda.synchronize(); t0 = time.perf_counter(); fn(); torch.cuda.synchronize()
    return time.perf_counter() - t0


g = torch.Generator(device=dev).manual_seed(0)
res = {'n': N, 'threads': torch.get_num_threads()}

# ---- moments ----
x = torch.relu(torch.randn([N, D_INC], device=dev, generator=g) + 0.5)


def moments_batched():
    s = metrics.FeatureStats(capture_mean_cov=True)
    for lo in range(0, N, 64):
        s.append_torch(x[lo:lo + 64])
    return s


def moments_one_call():
    s = metrics.FeatureStats(capture_mean_cov=True)
    s.append_torch(x)
    return s


flop = 2.0 * N * D_INC * D_INC
r = {'device_batches_of_64_s': timed(moments_batched, 3), 'device_one_call_s': timed(moments_one_call, 3), 'flop_full_matrix': flop}
r['device_one_call_fp64_tflops_of_the_triangle'] = round(flop / 2 / r['device_one_call_s'][0] / 1e12, 2)
frac = 1 / 8
rows = int(N * frac) // 64 * 64

def host_moments():
    s_mean, s_cov = np.zeros([D_INC]), np.zeros([D_INC, D_INC])
    for lo in range(0, rows, 64):
        x64 = x[lo:lo + 64].cpu().numpy().astype(np.float64)
        s_mean += x64.sum(axis=0); s_cov += x64.T @ x64

t = once(host_moments)
r['baseline_numpy_fp64_s'] = round(t * N / rows, 3); r['baseline_fraction'] = round(rows / N, 4); r['scaled'] = True
r['speedup_batches_of_64'] = round(r['baseline_numpy_fp64_s'] / r['device_batches_of_64_s'][0], 1)
res['moments_50000x2048'] = r
print('moments', r, file=sys.stderr, flush=True)

# ---- KID ----
y = torch.relu(torch.randn([N, D_INC], device=dev, generator=g) + 0.4)
xi, yi = metrics.kid_indices(N, N, SUBSETS, M, np.random.RandomState(0))
r = {'subsets': SUBSETS, 'm': M, 'device_s': timed(lambda: metrics.kid(y, x, indices=(xi, yi)), 3), 'flop': 3 * SUBSETS * 2.0 * M * M * D_INC}
r['device_fp32_tflops'] = round(r['flop'] / r['device_s'][0] / 1e12, 2)
part = 10
xh, yh = x.cpu().numpy(), y.cpu().numpy()

def host_kid():
    t = 0
    for s in range(part):
        a_, b_ = xh[xi[s]], yh[yi[s]]
        a = (a_ @ a_.T / D_INC + 1) ** 3 + (b_ @ b_.T / D_INC + 1) ** 3
        b = (a_ @ b_.T / D_INC + 1) ** 3
        t += (a.sum() - np.diag(a).sum()) / (M - 1) - b.sum() * 2 / M
    return t

t = once(host_kid)
r['baseline_numpy_s'] = round(t * SUBSETS / part, 3); r['baseline_fraction'] = part / SUBSETS; r['scaled'] = True
r['speedup'] = round(r['baseline_numpy_s'] / r['device_s'][0], 1)
del xh, yh
res['kid_100x1000x2048'] = r
print('kid', r, file=sys.stderr, flush=True)
del x, y

# ---- precision / recall ----
real = torch.relu(torch.randn([N, D_VGG], device=dev, generator=g) + 0.5)
gen = torch.relu(torch.randn([N, D_VGG], device=dev, generator=g) + 0.45)
out = {}
r = {'k': K, 'device_s': timed(lambda: out.__setitem__('pr', metrics.precision_recall(real, gen, K)), 2), 'flop': 4 * 2.0 * N * N * D_VGG}
r['device_fp32_tflops'] = round(r['flop'] / r['device_s'][0] / 1e12, 2)
r['precision_recall'] = list(out['pr'])
r['radii_s'] = timed(lambda: metrics.knn_radii(real, K), 1)
print('precision / recall', r, file=sys.stderr, flush=True)
try:
    rb = min(10000, N)
    real16, gen16 = real.to(torch.float16), gen.to(torch.float16)

    def distances(rows16, cols16):
        return torch.cat([torch.cdist(rows16.unsqueeze(0), cb.unsqueeze(0))[0].cpu() for cb in cols16.split(10000)], dim=1)

    def host_pr_one_row_batch():          # one row batch of a radii sweep and one of a membership sweep
        kth = distances(real16[:rb], real16).to(torch.float32).kthvalue(K + 1).values.to(torch.float16)
        full = torch.cat([kth, kth.new_full([N - rb], float('inf'))]) if N > rb else kth
        return (distances(gen16[:rb], real16) <= full).any(dim=1)

    t = once(host_pr_one_row_batch)
    batches = -(-N // rb)
    r['baseline_fp16_cdist_cpu_kthvalue_s'] = round(t * batches * 2, 2); r['baseline_fraction'] = round(1 / (2 * batches), 4); r['scaled'] = True
    r['speedup'] = round(r['baseline_fp16_cdist_cpu_kthvalue_s'] / r['device_s'][0], 1)
except Exception as e:      # noqa: BLE001 - the baseline is a comparison, not the product
    r['baseline_error'] = f'{type(e).__name__}: {e}'[:200]
res['precision_recall_50000x4096'] = r


def clock_now():
    """GPU 0's clocks as `rocm-smi --showclocks --json` reads them while radii calls are queued (read only; None without the tool)."""
    import shutil, subprocess
    exe = shutil.which('rocm-smi') or '/opt/rocm/bin/rocm-smi'
    if not os.path.exists(exe):
        return None
    try:
        small = real[:8192]
        for _ in range(20):
            metrics.knn_radii(small, K)
        o = subprocess.run([exe, '--showclocks', '--json'], capture_output=True, text=True, timeout=20)
        torch.cuda.synchronize()
        card = next(iter(json.loads(o.stdout).values()))
        return {k.lower().split()[0] + '_mhz': v.strip('()').replace('Mhz', '').replace('MHz', '') for k, v in card.items()
                if ('sclk' in k.lower() or 'mclk' in k.lower()) and 'speed' in k.lower()}
    except Exception as e:      # noqa: BLE001 - diagnostics only
        return {'error': f'{type(e).__name__}: {e}'[:120]}


res['gpu_clock'] = clock_now()
line = json.dumps(dict(metric='detector features -> FID moments, KID sums, precision / recall', device=torch.cuda.get_device_name(0),
                       timing='seconds, [median, min, max] of the repeats', **res,
                       native_launches={k: hip_plugin.CALLS.get(k, 0) for k in ('feature_moments', 'poly_kernel_sums', 'knn_radii', 'manifold_inside')}))
print(line)
os.makedirs(args.out, exist_ok=True)
with open(os.path.join(args.out, 'bench_metrics.json'), 'w') as f:
    f.write(line + '\n')
