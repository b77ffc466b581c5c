"""The VGG19 feature loss (training/vgg_loss.py) at the resolutions the hybrid encoder trains at, the HIP path (`vgg_loss.fused = True`)
against the ATen path of the same module (`fused = False`), alternated in one process:

    vgg_loss_256_b1, vgg_loss_256_b4, vgg_loss_512_b1, vgg_loss_512_b4
                                    `distance_to` against cached target features + the image gradient, 256 x 256 and 512 x 512, batch 1
                                    and batch 4

    python scripts/bench_vgg_loss.py [--blocks 5] [--iters 5] [--warmup 2] [--sizes 256 512] [--out profiles/vgg_loss/bench_vgg_loss.json]

prints one JSON line and writes it to --out: per case and path the device-event median over blocks of the time per call, the spread of the
blocks (max - min), the block times, the peak memory of one call (torch.cuda.max_memory_allocated minus what was allocated before it) and
the library launches of one call by entry point.  `fused_default_by_rule`: the HIP path is faster than the ATen path at every one of the
four points (the rule by which `vgg_loss.fused` ships True).  The net is VGG19 with random weights (the timing does not depend on them)."""
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
    ap.add_argument('--iters', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--sizes', type=int, nargs='+', default=[256, 512])
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'vgg_loss', 'bench_vgg_loss.json'))
    args = ap.parse_args()

    import torch
    from training import vgg_loss
    dev = torch.device('cuda', 0)
    torch.manual_seed(0)
    default = vgg_loss.fused
    net = vgg_loss.VGGLoss(dev)
    cases = {}
    for size in args.sizes:
        for n in (1, 4):
            g = torch.Generator().manual_seed(n)
            x = (torch.rand(n, 3, size, size, generator=g) * 2 - 1).to(dev).requires_grad_(True)
            y = (torch.rand(n, 3, size, size, generator=g) * 2 - 1).to(dev)
            vgg_loss.fused = False
            feats = net.features(y)

            def call(x=x, feats=feats):
                x.grad = None
                net.distance_to(x, feats).backward()
            cases[f'vgg_loss_{size}_b{n}'] = call
    result = dict(bench='vgg_loss', sizes=args.sizes, blocks=args.blocks, iters=args.iters, fused_shipped=default)
    try:
        result.update(loss_bench.measure(vgg_loss, cases, args.blocks, args.iters, args.warmup, launches=True))
    finally:
        vgg_loss.fused = default
    result['fused_default_by_rule'] = all(result[c]['hip']['ms'] < result[c]['aten']['ms'] for c in cases)
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
