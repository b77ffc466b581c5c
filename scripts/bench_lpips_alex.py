"""The AlexNet LPIPS distance (training/lpips_alex.py) at the resolution the reference's losses run at, the HIP path (`lpips_alex.fused =
True`) against the ATen path of the same module (`fused = False`), alternated in one process:

    lpips_alex_b1, lpips_alex_b4    `distance_to` against cached target features + the image gradient, 256 x 256, batch 1 and batch 4

    python scripts/bench_lpips_alex.py [--blocks 5] [--iters 10] [--warmup 3] [--out profiles/lpips_alex/bench_lpips_alex.json]

prints one JSON line and writes it to --out: per case and path the device-event median over blocks of the time per call, the spread of the
blocks (max - min), the block times, the peak memory of one call (torch.cuda.max_memory_allocated minus what was allocated before it) and
the library launches of one call by entry point.  `fused_default_by_rule`: the HIP path is not slower than the ATen path at any batch size
by more than the larger block spread of the two.  The net is AlexNet with random weights (the timing does not depend on them)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'ide-3d_amd')); sys.path.insert(0, ROOT)

import loss_bench


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--blocks', type=int, default=5)
    ap.add_argument('--iters', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--size', type=int, default=256)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'lpips_alex', 'bench_lpips_alex.json'))
    args = ap.parse_args()

    import torch
    from training import lpips_alex
    dev = torch.device('cuda', 0)
    torch.manual_seed(0)
    default = lpips_alex.fused
    net = lpips_alex.LPIPS().to(dev)
    cases = {}
    for n in (1, 4):
        g = torch.Generator().manual_seed(n)
        x = (torch.rand(n, 3, args.size, args.size, generator=g) * 2 - 1).to(dev).requires_grad_(True)
        y = (torch.rand(n, 3, args.size, args.size, generator=g) * 2 - 1).to(dev)
        lpips_alex.fused = False
        feats = net.features(y)

        def call(x=x, feats=feats):
            x.grad = None
            net.distance_to(x, feats).backward()
        cases[f'lpips_alex_b{n}'] = call
    result = dict(bench='lpips_alex', size=args.size, blocks=args.blocks, iters=args.iters, fused_shipped=default)
    try:
        result.update(loss_bench.measure(lpips_alex, cases, args.blocks, args.iters, args.warmup, launches=True))
    finally:
        lpips_alex.fused = default
    result['fused_default_by_rule'] = all(
        result[c]['hip']['ms'] <= result[c]['aten']['ms'] + max(result[c]['hip']['spread_ms'], result[c]['aten']['spread_ms']) for c in cases)
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
