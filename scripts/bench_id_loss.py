"""The ArcFace identity loss (training/id_loss.py) with the full IR-SE50, the HIP path (`id_loss.fused = True`) against the ATen path of the
same module (`fused = False`: the plain PyTorch definition), alternated in one process:

    id_256_b1, id_256_b4, id_512_b1, id_512_b4    `distance_to` + the image gradient at 256 x 256 and 512 x 512 input, batch 1 and batch 4

    python scripts/bench_id_loss.py [--blocks 5] [--iters 10] [--warmup 3]

prints one JSON line: per case and path the device-event median over blocks of the time per call, the spread of the blocks (max - min), the
block times, and the peak memory of one call (torch.cuda.max_memory_allocated minus what was allocated before it).  The net has random
weights (the timing does not depend on them)."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'ide-3d_amd')); sys.path.insert(0, ROOT)

PATHS = {'hip': True, 'aten': False}


def measure(cases, blocks, iters, warmup):
    """cases: {name: callable()}; every callable is run under both paths -> {name: {path: figures}}."""
    import torch
    from training import id_loss
    from torch_utils import hip_plugin
    for name, fn in cases.items():
        for fused in PATHS.values():
            id_loss.fused = fused
            before = hip_plugin.CALLS.get('id_head', 0)
            for _ in range(warmup):
                fn()
            took_hip = hip_plugin.CALLS.get('id_head', 0) > before
            assert took_hip == fused, f'{name}: fused = {fused} but the HIP loss head ' + ('ran' if took_hip else 'did not run')
    torch.cuda.synchronize()
    times = {(c, p): [] for c in cases for p in PATHS}
    for _ in range(blocks):
        for c, fn in cases.items():
            for p, fused in PATHS.items():
                id_loss.fused = fused
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(iters):
                    fn()
                e1.record()
                torch.cuda.synchronize()
                times[(c, p)].append(e0.elapsed_time(e1) / iters)
    out = {}
    for c, fn in cases.items():
        out[c] = {}
        for p, fused in PATHS.items():
            id_loss.fused = fused
            torch.cuda.synchronize()
            base = torch.cuda.memory_allocated()
            torch.cuda.reset_peak_memory_stats()
            fn()
            torch.cuda.synchronize()
            t = times[(c, p)]
            out[c][p] = dict(ms=round(statistics.median(t), 3), spread_ms=round(max(t) - min(t), 3), blocks_ms=[round(v, 3) for v in t],
                             peak_mib=round((torch.cuda.max_memory_allocated() - base) / 2 ** 20, 1))
        out[c]['hip_over_aten'] = round(out[c]['hip']['ms'] / out[c]['aten']['ms'], 3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--blocks', type=int, default=5)
    ap.add_argument('--iters', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--only', default=None, help='run one case (for a kernel trace)')
    ap.add_argument('--path', default=None, choices=list(PATHS), help='with --only: run that path alone, untimed')
    args = ap.parse_args()

    import torch
    from training import id_loss
    dev = torch.device('cuda', 0)
    torch.manual_seed(0)
    default = id_loss.fused
    crit = id_loss.IDLoss().to(dev)
    cases = {}
    for size in (256, 512):
        for n in (1, 4):
            g = torch.Generator().manual_seed(size + n)
            x = (torch.rand(n, 3, size, size, generator=g) * 2 - 1).to(dev).requires_grad_(True)
            feats = crit.features((torch.rand(n, 3, size, size, generator=g) * 2 - 1).to(dev))

            def call(x=x, feats=feats):
                x.grad = None
                crit.distance_to(x, feats).backward()
            cases[f'id_{size}_b{n}'] = call
    if args.only:
        cases = {args.only: cases[args.only]}
    result = dict(bench='id_loss', blocks=args.blocks, iters=args.iters)
    try:
        if args.only and args.path:
            id_loss.fused = PATHS[args.path]
            for _ in range(args.warmup + args.iters):
                cases[args.only]()
            torch.cuda.synchronize()
            result.update(only=args.only, path=args.path, untimed=True)
        else:
            result.update(measure(cases, args.blocks, args.iters, args.warmup))
    finally:
        id_loss.fused = default
    print(json.dumps(result))


if __name__ == '__main__':
    main()
