"""One pivotal-tuning step of PTI inversion on the full spec: `G.synthesis(w_pivot, c, noise_mode='const', force_fp32=True)` with every
synthesis parameter trainable, an L2 loss against a fixed target, backward, `Adam.step()` (lr 3e-4), with the parameter gradients of the
synthesis convolutions on HIP (`networks.hip_param_grad = True`) against the ATen / MIOpen path (False),
alternated in one process.  Prints one JSON line.

    python scripts/bench_param_grad.py [--batches 1,4] [--blocks 5] [--iters 2] [--warmup 2] [--modes on,off] [--kernels]

--kernels: per-launch times of the new entry points at the full spec's layer shapes, batch 1 (device-event medians, each call including
its second, reducing launch): the weight gradient with its FLOP rate (2 cout cin 9 pixels), the bias / noise reduction with bytes / t.

Times are device-event medians over blocks (per step), after warm-up.  Peak memory is torch.cuda.max_memory_allocated over one step,
minus what was allocated before it."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'ide-3d_amd')); sys.path.insert(0, ROOT)
import torch  # noqa: E402
from training import networks, triplane  # noqa: E402


def _time(fn, warmup, blocks, iters, modes):
    out = {m: [] for m in modes}
    for m in modes:
        networks.hip_param_grad = m
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    for _ in range(blocks):
        for m in modes:
            networks.hip_param_grad = m
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(iters):
                fn()
            e1.record()
            torch.cuda.synchronize()
            out[m].append(e0.elapsed_time(e1) / iters)
    networks.hip_param_grad = False
    return {m: statistics.median(v) for m, v in out.items()}


def _peak(fn, mode):
    networks.hip_param_grad = mode
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    networks.hip_param_grad = False
    return (torch.cuda.max_memory_allocated() - base) / 2 ** 20


def _event_ms(fn, reps=20):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    t = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); fn(); e1.record()
        torch.cuda.synchronize()
        t.append(e0.elapsed_time(e1))
    return statistics.median(t)


def kernels():
    networks._modconv_init(); networks._modconv_grad_init()
    gp = networks._modconv_grad_plugin
    dev = torch.device('cuda', 0)
    g = torch.Generator(device=dev).manual_seed(0)
    rnd = lambda *s: torch.randn(*s, device=dev, generator=g)
    out = {}
    for name, cin, cout, res, up in (('s1_512@4', 512, 512, 4, 1), ('s1_512@16', 512, 512, 16, 1), ('s1_512@64', 512, 512, 64, 1),
                                     ('s1_256@128', 256, 256, 128, 1), ('s1_128@256', 128, 128, 256, 1), ('s1_64@512', 64, 64, 512, 1),
                                     ('up_512_512@8', 512, 512, 8, 2), ('up_512_256@128', 512, 256, 128, 2),
                                     ('up_256_128@256', 256, 128, 256, 2), ('up_128_64@512', 128, 64, 512, 2)):
        h = res // up
        x, s, d = rnd(1, cin, h, h), rnd(1, cin).abs() + 0.5, rnd(1, cout).abs() + 0.1
        gg = rnd(1, cout, res, res) if up == 1 else rnd(1, cout, res + 1, res + 1)
        mode = 0 if up == 1 else 2
        r = {}
        for arith, an in ((6, 'bf16x6'), (1, 'fp32')):
            t = _event_ms(lambda: gp.weight_grad(gg, x, s, d, mode=mode, arith=arith))
            r[f'wgrad_{an}_us'] = round(t * 1e3, 1)
            r[f'wgrad_{an}_tflops'] = round(2 * cout * cin * 9 * h * h / t / 1e9, 1)
        dz = rnd(1, cout, res, res)
        t = _event_ms(lambda: gp.bias_noise_grad(dz, noise=True))
        r.update(bias_noise_us=round(t * 1e3, 1), bias_noise_gbps=round(dz.numel() * 4 / t / 1e6, 1))
        out[name] = r
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batches', default='1,4')
    ap.add_argument('--blocks', type=int, default=5)
    ap.add_argument('--iters', type=int, default=2)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--modes', default='on,off')
    ap.add_argument('--kernels', action='store_true')
    args = ap.parse_args()
    if args.kernels:
        print(json.dumps(kernels()))
        return
    dev = torch.device('cuda', 0)
    torch.manual_seed(0)
    sp = triplane.GeneratorSpec()
    result = dict(bench='param_grad_pti_step')
    for n in [int(b) for b in args.batches.split(',')]:
        torch.manual_seed(0)
        G = triplane.TriPlaneGenerator(sp).to(dev).eval().requires_grad_(False)
        g = torch.Generator().manual_seed(7)
        z = torch.randn(n, G.z_dim, generator=g).to(dev)
        c = torch.cat([triplane.camera_label(0.2)] * n).to(dev)
        with torch.no_grad():
            w_pivot = G.mapping(z, c)
            target = torch.rand(n, 3, sp.img_resolution, sp.img_resolution, generator=g).to(dev) * 2 - 1
        G.synthesis.requires_grad_(True)
        opt = torch.optim.Adam(G.synthesis.parameters(), lr=3e-4)

        def step():
            opt.zero_grad(set_to_none=True)
            img = G.synthesis(w_pivot, c=c, noise_mode='const', force_fp32=True)
            loss = ((img - target) ** 2).mean()
            loss.backward()
            opt.step()

        modes = tuple({'on': True, 'off': False}[m] for m in args.modes.split(','))
        ms = _time(step, args.warmup, args.blocks, args.iters, modes)
        mem = {m: _peak(step, m) for m in modes}
        r = result[f'tuning_step_b{n}'] = {}
        for m, name in ((True, 'hip'), (False, 'aten')):
            if m in ms:
                r[f'{name}_ms'], r[f'{name}_peak_mib'] = round(ms[m], 3), round(mem[m], 1)
        if len(ms) == 2:
            r['speedup'] = round(ms[False] / ms[True], 2)
        del G, opt
        torch.cuda.empty_cache()
    print(json.dumps(result))


if __name__ == '__main__':
    main()
