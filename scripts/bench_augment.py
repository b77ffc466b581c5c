"""The geometric + colour stages of the ADA pipeline on one GPU (csrc/augment.hip): `AugmentPipe.apply` on given
parameters, forward and forward + backward, the fused path beside this module's own PyTorch definition (`augment.fused = False`: the HIP
upfirdn2d of this package plus ATen pad / affine_grid / grid_sample, which reads the margins back), at 512 x 512, batch 4 and 32, with 3
channels (bgc parameters: geometry + colour) and 19 (the mask: geometry only), parameters drawn once at p = 0.6 with a fixed seed; then the
whole `forward` including `sample_params`, and the peak memory of both paths.  Times are `torch.cuda.Event` pairs around blocks of REPS calls
after a warm-up block, ms per call: [median, min, max] of 5 blocks.  Prints one JSON line and writes it to --out (default
profiles/augment)/bench_augment.json.  Not measured: kernels one by one under a profiler, more than one GPU."""
import argparse, json, os, statistics, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'ide-3d_amd')); sys.path.insert(0, ROOT)
import torch
from training import augment
from torch_utils import hip_plugin

ap = argparse.ArgumentParser()
ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'augment'))
ap.add_argument('--res', type=int, default=512)
ap.add_argument('--batches', type=int, nargs='+', default=[4, 32])
ap.add_argument('--reps', type=int, default=10)
ap.add_argument('--baseline-cap-gb', type=float, default=40.0, help='skip the PyTorch definition where its intermediates are estimated above this')
args = ap.parse_args()
dev = torch.device('cuda:0')
BGC = dict(xflip=1, rotate90=1, xint=1, scale=1, rotate=1, aniso=1, xfrac=1, brightness=1, contrast=1, lumaflip=1, hue=1, saturation=1)
BLOCKS = 5


def blocks(fn, reps):
    """[median, min, max] of BLOCKS blocks of `reps` calls, ms per call, device events; one warm-up block first."""
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(BLOCKS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record(); b.synchronize()
        out.append(a.elapsed_time(b) / reps)
    return [round(statistics.median(out), 4), round(min(out), 4), round(max(out), 4)]


def peak(fn):
    fn(); torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats(); base = torch.cuda.memory_allocated()
    fn(); torch.cuda.synchronize()
    return int(torch.cuda.max_memory_allocated() - base)


def clock_now(fn):
    """GPU 0's clocks as `rocm-smi --showclocks --json` reads them while fused calls are queued (read only; None without the tool)."""
    import shutil, subprocess
    exe = shutil.which('rocm-smi') or '/opt/rocm/bin/rocm-smi'
    if not os.path.exists(exe):
        return None
    try:
        for _ in range(50):
            fn()
        o = subprocess.run([exe, '--showclocks', '--json'], capture_output=True, text=True, timeout=20)
        torch.cuda.synchronize()
        card = next(iter(json.loads(o.stdout).values()))
        return {k.lower().split()[0] + '_mhz': v.strip('()').replace('Mhz', '').replace('MHz', '') for k, v in card.items()
                if ('sclk' in k.lower() or 'mclk' in k.lower()) and 'speed' in k.lower()}
    except Exception as e:      # noqa: BLE001 - diagnostics only
        return {'error': f'{type(e).__name__}: {e}'[:120]}


pipe = augment.AugmentPipe(**BGC).to(dev)
pipe.p.fill_(0.6)
res = {'res': args.res, 'p': 0.6, 'reps_per_block': args.reps, 'blocks': BLOCKS}
last = None
for n in args.batches:
    for c in (3, 19):
        torch.manual_seed(1000 + n)
        prm = pipe.sample_params(n, 3, args.res, args.res, dev)
        if c != 3:
            prm = augment.AugmentParams(G_inv=prm.G_inv)          # the mask takes the image's warp and no colour
        x = torch.rand([n, c, args.res, args.res], device=dev) * 2 - 1
        w = torch.rand_like(x)
        xg = x.clone().requires_grad_(True)

        def fwd():
            return pipe.apply(x, prm)

        def fwd_bwd():
            xg.grad = None
            (pipe.apply(xg, prm) * w).sum().backward()

        m = augment.margins(prm.G_inv, args.res, args.res).cpu().tolist()
        # the PyTorch definition holds the up-sampled padded images, the resampled ones and the half-way tensor of the decimation
        est = n * c * 4 * (2 * (args.res + m[1] + m[3])) * (2 * (args.res + m[0] + m[2])) * 2.5
        r = {'margins': m, 'output_bytes': x.numel() * 4, 'pytorch_definition_intermediates_estimated_bytes': int(est)}
        loops0 = hip_plugin.AugmentPlugin.band_loops(dev)
        y_fused = pipe.apply(x, prm)
        r['band_loop_workgroups_per_forward'] = hip_plugin.AugmentPlugin.band_loops(dev) - loops0
        paths = [('fused', True)] + ([('pytorch_definition', False)] if est <= args.baseline_cap_gb * 1e9 else [])
        for name, flag in paths:
            augment.fused = flag
            r[name] = {'forward_ms': blocks(fwd, args.reps), 'forward_backward_ms': blocks(fwd_bwd, args.reps), 'forward_peak_bytes': peak(fwd),
                       'forward_backward_peak_bytes': peak(fwd_bwd)}
            if c == 3:
                r[name]['forward_with_sample_params_ms'] = blocks(lambda: pipe(x), args.reps)
            if not flag:
                r['max_abs_difference_between_paths'] = float((pipe.apply(x, prm) - y_fused).abs().max())
        augment.fused = True
        if 'pytorch_definition' in r:
            r['speedup_forward'] = round(r['pytorch_definition']['forward_ms'][0] / r['fused']['forward_ms'][0], 2)
            r['speedup_forward_backward'] = round(r['pytorch_definition']['forward_backward_ms'][0] / r['fused']['forward_backward_ms'][0], 2)
        else:
            r['pytorch_definition'] = f'not measured: intermediates estimated above {args.baseline_cap_gb} GB'
        del y_fused
        torch.cuda.empty_cache()
        res[f'batch{n}_c{c}'] = r
        last = fwd
res['gpu_clock'] = clock_now(last)
line = json.dumps(dict(metric='ADA geometric + colour stages, apply() on given parameters', device=torch.cuda.get_device_name(0),
                       timing='ms per call, [median, min, max] of 5 blocks, device events', **res,
                       native_launches={k: v for k, v in hip_plugin.CALLS.items() if k.startswith('augment') or k == 'upfirdn2d'}))
print(line)
os.makedirs(args.out, exist_ok=True)
with open(os.path.join(args.out, 'bench_augment.json'), 'w') as f:
    f.write(line + '\n')
