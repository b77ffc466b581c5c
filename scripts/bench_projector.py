"""The latent-projection step with trainable noise maps (training/projection.py: `Projector.step`, the schedule of the reference's
w_projector_ide3d.py) on the full spec at batch 1, in three configurations alternated in one process:

    off      networks.hip_noise_grad = False, projection.fused_noise_ops = False   (noisy layers on the ATen convolution backward, the
                                                                                    regulariser and the normaliser as eager tensor ops)
    route    hip_noise_grad = True,  fused_noise_ops = False                       (the layers on the HIP gradient path)
    fused    hip_noise_grad = True,  fused_noise_ops = True                        (and the noise ops in csrc/noise_reg.hip)

    python scripts/bench_projector.py [--blocks 5] [--iters 2] [--warmup 2] [--configs off,route,fused]

prints one JSON line: per configuration the device-event median over blocks of the time per step, the spread of the blocks (max - min) and
the peak memory of one step (torch.cuda.max_memory_allocated minus what was allocated before it), and `accepted`: fused is not slower than
off by more than off's own spread.

Kernel launches per step come from a run of their own under the profiler:

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python scripts/bench_projector.py --trace-steps 3
    python scripts/bench_projector.py --parse-trace DIR

--trace-steps runs, per configuration, one warm-up step and then that many steps between two marker launches (an erfinv kernel, which
nothing else in the step uses); --parse-trace counts the dispatches between the markers in the kernel trace and prints them per step."""
import argparse
import csv
import glob
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'ide-3d_amd')); sys.path.insert(0, ROOT)

CONFIGS = {'off': (False, False), 'route': (True, False), 'fused': (True, True)}
MARKER = 'erfinv'


def parse_trace(path):
    files = sorted(glob.glob(os.path.join(path, '**', '*kernel_trace.csv'), recursive=True))
    assert files, f'no *kernel_trace.csv under {path}'
    rows = []
    for f in files:
        with open(f, newline='') as fh:
            rows += [(int(r['Start_Timestamp']), r['Kernel_Name']) for r in csv.DictReader(fh)]
    rows.sort()
    marks = [i for i, (_, name) in enumerate(rows) if MARKER in name]
    assert len(marks) % 2 == 0 and marks, f'{len(marks)} marker launches'
    out = []
    for a, b in zip(marks[0::2], marks[1::2]):
        out.append(b - a - 1)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--blocks', type=int, default=5)
    ap.add_argument('--iters', type=int, default=2)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--configs', default='off,route,fused')
    ap.add_argument('--w-avg-samples', type=int, default=1000)
    ap.add_argument('--trace-steps', type=int, default=0)
    ap.add_argument('--parse-trace', default=None)
    args = ap.parse_args()
    names = args.configs.split(',')
    if args.parse_trace:
        counts = parse_trace(args.parse_trace)
        # the traced run used the default --configs order unless told otherwise, and --trace-steps is recovered from nothing: pass it again
        steps = args.trace_steps or 3
        assert len(counts) == len(names), (counts, names)
        print(json.dumps(dict(bench='projector_launches', steps=steps, launches_per_step={n: round(c / steps, 1) for n, c in zip(names, counts)})))
        return

    import torch
    from training import networks, projection, triplane
    dev = torch.device('cuda', 0)
    torch.manual_seed(0)
    sp = triplane.GeneratorSpec()
    G = triplane.TriPlaneGenerator(sp).eval().requires_grad_(False)
    with torch.no_grad():
        for name, p in G.synthesis.named_parameters():
            if name.endswith('noise_strength'):
                p.fill_(0.1)                      # random init has 0; a trained generator does not
    G = G.to(dev)
    c = triplane.camera_label(0.2).to(dev)
    target = torch.rand(3, sp.img_resolution, sp.img_resolution, generator=torch.Generator().manual_seed(7)).to(dev) * 255
    P = projection.Projector(G, target, c, num_steps=1000, w_avg_samples=args.w_avg_samples)
    del G
    counter = [100]                               # past the learning-rate ramp-up, inside the w-noise ramp

    def step():
        counter[0] += 1
        P.step(counter[0])

    def select(name):
        networks.hip_noise_grad, projection.fused_noise_ops = CONFIGS[name]

    try:
        if args.trace_steps:
            x = torch.rand(64, device=dev)
            for name in names:
                select(name)
                step()
                torch.cuda.synchronize()
                torch.erfinv(x)
                for _ in range(args.trace_steps):
                    step()
                torch.erfinv(x)
                torch.cuda.synchronize()
            print(json.dumps(dict(bench='projector_trace', configs=names, steps=args.trace_steps)))
            return
        for name in names:
            select(name)
            for _ in range(args.warmup):
                step()
        torch.cuda.synchronize()
        times = {name: [] for name in names}
        for _ in range(args.blocks):
            for name in names:
                select(name)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(args.iters):
                    step()
                e1.record()
                torch.cuda.synchronize()
                times[name].append(e0.elapsed_time(e1) / args.iters)
        result = dict(bench='projector_step', spec='full', batch=1, noise_maps=len(P.maps), blocks=args.blocks, iters=args.iters)
        for name in names:
            select(name)
            torch.cuda.synchronize()
            base = torch.cuda.memory_allocated()
            torch.cuda.reset_peak_memory_stats()
            step()
            torch.cuda.synchronize()
            t = times[name]
            result[name] = dict(ms=round(statistics.median(t), 3), spread_ms=round(max(t) - min(t), 3), blocks_ms=[round(v, 3) for v in t],
                                peak_mib=round((torch.cuda.max_memory_allocated() - base) / 2 ** 20, 1))
        if 'off' in result and 'fused' in result:
            result['accepted'] = result['fused']['ms'] - result['off']['ms'] <= result['off']['spread_ms']
    finally:
        networks.hip_noise_grad, projection.fused_noise_ops = True, True
    print(json.dumps(result))


if __name__ == '__main__':
    main()
