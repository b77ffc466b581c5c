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
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'ide-3d_amd')); sys.path.insert(0, ROOT)

import loss_bench


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--blocks', type=int, default=5)
    ap.add_argument('--iters', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--only', default=None, help='run one case (for a kernel trace)')
    ap.add_argument('--path', default=None, choices=list(loss_bench.PATHS), help='with --only: run that path alone, untimed')
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
            id_loss.fused = loss_bench.PATHS[args.path]
            for _ in range(args.warmup + args.iters):
                cases[args.only]()
            torch.cuda.synchronize()
            result.update(only=args.only, path=args.path, untimed=True)
        else:
            result.update(loss_bench.measure(id_loss, cases, args.blocks, args.iters, args.warmup, hip_call='id_head'))
    finally:
        id_loss.fused = default
    print(json.dumps(result))


if __name__ == '__main__':
    main()
