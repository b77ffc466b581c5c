"""The VGG16 LPIPS distance (training/lpips.py) at the projectors' resolution, the HIP path (`lpips.fused = True`) against the ATen path of
the same module (`fused = False`), alternated in one process:

    lpips_b1, lpips_b4    `distance_to` against cached target features + the image gradient, 256 x 256, batch 1 and batch 4
    projector_step        one `Projector.step` of the full spec (512 x 512 images, area factor 2 in front of the net) with `lpips_distance`

    python scripts/bench_lpips.py [--blocks 5] [--iters 10] [--warmup 3] [--no-projector]

prints one JSON line: per case and path the device-event median over blocks of the time per call, the spread of the blocks (max - min), the
block times, and the peak memory of one call (torch.cuda.max_memory_allocated minus what was allocated before it).  The net is VGG16 with
random weights (the timing does not depend on them)."""
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
    ap.add_argument('--no-projector', action='store_true')
    ap.add_argument('--w-avg-samples', type=int, default=1000)
    args = ap.parse_args()

    import torch
    from training import lpips, projection, triplane
    dev = torch.device('cuda', 0)
    torch.manual_seed(0)
    default = lpips.fused
    net = lpips.LPIPS('vgg').to(dev)
    cases = {}
    for n in (1, 4):
        g = torch.Generator().manual_seed(n)
        x = (torch.rand(n, 3, args.size, args.size, generator=g) * 2 - 1).to(dev).requires_grad_(True)
        y = (torch.rand(n, 3, args.size, args.size, generator=g) * 2 - 1).to(dev)
        lpips.fused = False
        feats = net.features(y)

        def call(x=x, feats=feats):
            x.grad = None
            net.distance_to(x, feats).backward()
        cases[f'lpips_b{n}'] = call
    result = dict(bench='lpips', size=args.size, blocks=args.blocks, iters=args.iters)
    try:
        result.update(loss_bench.measure(lpips, cases, args.blocks, args.iters, args.warmup))
        if not args.no_projector:
            sp = triplane.GeneratorSpec()
            G = triplane.TriPlaneGenerator(sp).eval().requires_grad_(False)
            with torch.no_grad():
                for name, p in G.synthesis.named_parameters():
                    if name.endswith('noise_strength'):
                        p.fill_(0.1)                      # random init has 0; a trained generator does not
            G = G.to(dev)
            c = triplane.camera_label(0.2).to(dev)
            target = torch.rand(3, sp.img_resolution, sp.img_resolution, generator=torch.Generator().manual_seed(7)).to(dev) * 255
            lpips.fused = False
            P = projection.Projector(G, target, c, num_steps=1000, w_avg_samples=args.w_avg_samples,
                                     distance=lpips.lpips_distance(target[None], net, size=args.size))
            del G
            counter = [100]                               # past the learning-rate ramp-up, inside the w-noise ramp

            def step():
                counter[0] += 1
                P.step(counter[0])
            result.update(loss_bench.measure(lpips, {'projector_step': step}, args.blocks, max(args.iters // 5, 1), max(args.warmup - 1, 1)))
            result['projector_resolution'] = sp.img_resolution
    finally:
        lpips.fused = default
    print(json.dumps(result))


if __name__ == '__main__':
    main()
