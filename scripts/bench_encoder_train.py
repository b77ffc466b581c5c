"""One training step of the hybrid encoder (training/encoders.py, `HybridEncoder(512, 10, 8, 512)`: forward, `ws.square().mean().backward()`,
Adam), with the plain convolutions' gradients through HIP (`networks.hip_plain_conv_grad = True`) against the ATen
path of the same module (the switch off), alternated in one process, at batch 1, 4 and 8:

    python scripts/bench_encoder_train.py [--blocks 5] [--iters 5] [--warmup 2] [--batches 1,4,8] [--size 512] [--paths hip,aten]

prints one JSON line and writes it to profiles/encoder_train/bench_encoder_train.json: per batch size and path the device-event median over
blocks of the time per step, the spread of the blocks (max - min), the block times, the peak memory of one step
(torch.cuda.max_memory_allocated minus what was allocated before it) and the library's launches per step (hip_plugin.CALLS; the ATen
path's own kernels are not counted there).  The encoder has random weights (the timing does not depend on them)."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'ide-3d_amd')); sys.path.insert(0, ROOT)

PATHS = {'hip': True, 'aten': False}


def measure(cases, blocks, iters, warmup, paths=PATHS):
    """cases: {name: callable()}; every callable is run under both paths -> {name: {path: figures}}."""
    import torch
    from training import networks
    from torch_utils import hip_plugin
    for name, fn in cases.items():
        for on in paths.values():
            networks.hip_plain_conv_grad = on
            before = hip_plugin.CALLS.get('linear_weight_grad', 0)
            for _ in range(warmup):
                fn()
            took_hip = hip_plugin.CALLS.get('linear_weight_grad', 0) > before
            assert took_hip == on, f'{name}: switch {on} but the HIP projector gradient ' + ('ran' if took_hip else 'did not run')
    torch.cuda.synchronize()
    times = {(c, p): [] for c in cases for p in paths}
    for _ in range(blocks):
        for c, fn in cases.items():
            for p, on in paths.items():
                networks.hip_plain_conv_grad = on
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
        for p, on in paths.items():
            networks.hip_plain_conv_grad = on
            torch.cuda.synchronize()
            base = torch.cuda.memory_allocated()
            torch.cuda.reset_peak_memory_stats()
            calls = dict(hip_plugin.CALLS)
            fn()
            torch.cuda.synchronize()
            launches = {k: v - calls.get(k, 0) for k, v in hip_plugin.CALLS.items() if v - calls.get(k, 0)}
            t = times[(c, p)]
            out[c][p] = dict(ms=round(statistics.median(t), 3), spread_ms=round(max(t) - min(t), 3), blocks_ms=[round(v, 3) for v in t],
                             peak_mib=round((torch.cuda.max_memory_allocated() - base) / 2 ** 20, 1),
                             library_calls=sum(launches.values()), library_calls_by_entry=launches)
        if len(paths) == 2:
            out[c]['hip_over_aten'] = round(out[c]['hip']['ms'] / out[c]['aten']['ms'], 3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--blocks', type=int, default=5)
    ap.add_argument('--iters', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--batches', default='1,4,8')
    ap.add_argument('--size', type=int, default=512)
    ap.add_argument('--paths', default='hip,aten', help='one path alone for a kernel trace (scripts/step_timeline.py <dir> <out> MeanOps)')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'encoder_train', 'bench_encoder_train.json'))
    args = ap.parse_args()

    import torch
    from training import encoders, networks
    dev = torch.device('cuda', 0)
    torch.manual_seed(0)
    default = networks.hip_plain_conv_grad
    E = encoders.HybridEncoder(args.size, 10, 8, 512).to(dev)
    opt = torch.optim.Adam(E.parameters(), lr=1e-4)
    cases = {}
    for n in map(int, args.batches.split(',')):
        g = torch.Generator().manual_seed(n)
        img = (torch.rand(n, 3, args.size, args.size, generator=g) * 2 - 1).to(dev)
        seg = torch.rand(n, 19, args.size, args.size, generator=g).to(dev)

        def step(img=img, seg=seg):
            opt.zero_grad(set_to_none=True)
            E(img, seg).square().mean().backward()
            opt.step()
        cases[f'encoder_{args.size}_b{n}'] = step
    result = dict(bench='encoder_train', blocks=args.blocks, iters=args.iters)
    try:
        result.update(measure(cases, args.blocks, args.iters, args.warmup, {p: PATHS[p] for p in args.paths.split(',')}))
    finally:
        networks.hip_plain_conv_grad = default
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
