"""The discriminator's adversarial loss (training/adv_loss.py) on the FFHQ configuration (img_resolution 512, 6 image channels, c_dim 25,
default channels, conv_clamp 256), the HIP path (`adv_loss.fused = True`) against the ATen path of the same module (`fused = False`: the
plain PyTorch definition), alternated in one process:

    adv_512_b1, adv_512_b4    `generator_loss` + the image gradient at batch 1 and batch 4, the label mapped once outside the timed call

    python scripts/bench_adv_loss.py [--blocks 5] [--iters 10] [--warmup 3]

prints one JSON line: per case and path the device-event median over blocks of the time per call, the spread of the blocks (max - min), the
block times, the peak memory of one call (torch.cuda.max_memory_allocated minus what was allocated before it) and the library launches of
one call.  The discriminator has random weights (the timing does not depend on them)."""
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
    assert args.blocks >= 5 or args.only, 'the median is taken over at least 5 blocks'

    import torch
    from training import adv_loss, discriminator
    dev = torch.device('cuda', 0)
    torch.manual_seed(0)
    default = adv_loss.fused
    D = discriminator.Discriminator(c_dim=25, img_resolution=512, img_channels=6, conv_clamp=256).eval().requires_grad_(False).to(dev)
    crit = adv_loss.ADVLoss(D)
    cases = {}
    for n in (1, 4):
        g = torch.Generator().manual_seed(n)
        x = (torch.rand(n, 6, 512, 512, generator=g) * 2 - 1).to(dev).requires_grad_(True)
        with torch.no_grad():
            cmap = crit.cmap(torch.randn(n, 25, generator=g).to(dev))

        def call(x=x, cmap=cmap):
            x.grad = None
            crit.generator_loss(x, cmap=cmap).backward()
        cases[f'adv_512_b{n}'] = call
    if args.only:
        cases = {args.only: cases[args.only]}
    result = dict(bench='adv_loss', blocks=args.blocks, iters=args.iters)
    try:
        if args.only and args.path:
            adv_loss.fused = loss_bench.PATHS[args.path]
            for _ in range(args.warmup + args.iters):
                cases[args.only]()
            torch.cuda.synchronize()
            result.update(only=args.only, path=args.path, untimed=True)
        else:
            result.update(loss_bench.measure(adv_loss, cases, args.blocks, args.iters, args.warmup, hip_call='adv_head', launches=True))
    finally:
        adv_loss.fused = default
    print(json.dumps(result))


if __name__ == '__main__':
    main()
