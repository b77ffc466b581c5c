"""One projector step of PTI-style inversion (frozen full-spec generator, `G.synthesis(ws)` with ws.requires_grad, L2 loss against a
fixed target, backward; fused renderer backward on) with the frozen-generator convolution backward (`networks.hip_conv_grad = True`,
csrc/modconv_bwd.hip + ide3d_modconv2d) against the ATen convolution backward (False), alternated in one process.  Prints one JSON line.

    python scripts/bench_conv_grad.py [--batches 1,4] [--blocks 5] [--iters 2] [--warmup 2] [--modes on,off] [--kernels]

--kernels: the backward's launches of single layers of the full spec at batch 1 instead (device-event medians): K1, K2 and K3 with the
bytes they must move and (bytes)/t, and the input-gradient convolutions (ide3d_modconv2d mode 0 / mode 1 / per-image 1x1) with their
FLOP rate.

Times are device-event medians over blocks (per step), after warm-up.  Peak memory is torch.cuda.max_memory_allocated over one step,
minus what was allocated before it.  Kernel times come from a separate `rocprofv3 --kernel-trace --stats` run of this script."""
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
        networks.hip_conv_grad = m
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    for _ in range(blocks):
        for m in modes:
            networks.hip_conv_grad = m
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(iters):
                fn()
            e1.record()
            torch.cuda.synchronize()
            out[m].append(e0.elapsed_time(e1) / iters)
    networks.hip_conv_grad = True
    return {m: statistics.median(v) for m, v in out.items()}


def _peak(fn, mode):
    networks.hip_conv_grad = mode
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    networks.hip_conv_grad = True
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
    """Per-launch times of the backward of single full-spec layers at batch 1 (each call is one entry point: K1 / K2 / K3 include their
    second, reducing launch)."""
    networks._modconv_init(); networks._modconv_grad_init()
    gp, mp = networks._modconv_grad_plugin, networks._modconv_plugin
    dev = torch.device('cuda', 0)
    g = torch.Generator(device=dev).manual_seed(0)
    rnd = lambda *s: torch.randn(*s, device=dev, generator=g)
    out = {}
    for name, cin, cout, res, up in (('s1_512@16', 512, 512, 16, 1), ('s1_256@64', 256, 256, 64, 1), ('s1_128@128', 128, 128, 128, 1),
                                     ('s1_64@256', 64, 64, 256, 1), ('up_512_256@128', 512, 256, 128, 2), ('up_256_128@256', 256, 128, 256, 2),
                                     ('up_128_64@512', 128, 64, 512, 2)):
        h = res // up
        x, w = rnd(1, cin, h, h), rnd(cout, cin, 3, 3)
        s, d = rnd(1, cin).abs() + 0.5, rnd(1, cout).abs() + 0.1
        y, dy, noise, b = rnd(1, cout, res, res), rnd(1, cout, res, res), rnd(res, res), rnd(cout)
        wt = networks._grad_weight(w, up == 1)
        k1 = _event_ms(lambda: gp.act_backward(dy, y, 3, 0.2, 2 ** 0.5, -1.0, noise=noise, bias=b, dcoefs=d))
        k1_bytes = 3 * dy.numel() * 4 + noise.numel() * 4
        r = dict(k1_us=round(k1 * 1e3, 1), k1_gbps=round(k1_bytes / k1 / 1e6, 1))
        if up == 1:
            conv = _event_ms(lambda: mp.modconv2d(dy, wt, d, None, None, 0.0, None, 1, 0.0, 1.0, -1.0))
            r['conv_mode0_us'] = round(conv * 1e3, 1)
            flops = 2 * cout * cin * 9 * res * res
        else:
            gt = rnd(1, cout, res + 1, res + 1)
            k1d = _event_ms(lambda: gp.act_backward(gt, gt, 0, 0.0, 1.0, -1.0, dcoefs=d))
            r.update(k1_dot_us=round(k1d * 1e3, 1), k1_dot_gbps=round(2 * gt.numel() * 4 / k1d / 1e6, 1))
            conv = _event_ms(lambda: mp.modconv2d(gt, wt, d, None, None, 0.0, None, 1, 0.0, 1.0, -1.0, mode=1))
            r['conv_mode1_us'] = round(conv * 1e3, 1)
            flops = 2 * cout * cin * 9 * h * h
        r['conv_tflops'] = round(flops / conv / 1e9, 1)
        t = rnd(1, cin, h, h)
        k2 = _event_ms(lambda: gp.scale_dot(x, t, s))
        r.update(k2_us=round(k2 * 1e3, 1), k2_gbps=round(3 * t.numel() * 4 / k2 / 1e6, 1))
        out[name] = r
    for name, rows, cin, res in (('heads_192x128@256', 192, 128, 256), ('heads_192x512@32', 192, 512, 32), ('heads_22x64@512', 22, 64, 512),
                                 ('heads_22x128@256', 22, 128, 256)):
        dy, x = rnd(1, rows, res, res), rnd(1, cin, res, res)
        wT = rnd(1, cin, rows, 1, 1)
        k3 = _event_ms(lambda: gp.head_weight_grad(dy, x))
        conv = _event_ms(lambda: mp.modconv2d(dy, wT, None, None, None, 0.0, None, 1, 0.0, 1.0, -1.0))
        out[name] = dict(k3_us=round(k3 * 1e3, 1), k3_gbps=round((dy.numel() + x.numel()) * 4 / k3 / 1e6, 1),
                         k3_tflops=round(2 * rows * cin * res * res / k3 / 1e9, 1), conv_1x1_us=round(conv * 1e3, 1))
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
    G = triplane.TriPlaneGenerator(sp).to(dev).eval().requires_grad_(False)
    result = dict(bench='conv_grad_projector', fused_render_grad=triplane.fused_render_grad)
    for n in [int(b) for b in args.batches.split(',')]:
        g = torch.Generator().manual_seed(7)
        z = torch.randn(n, G.z_dim, generator=g).to(dev)
        c = torch.cat([triplane.camera_label(0.2)] * n).to(dev)
        with torch.no_grad():
            ws0 = G.mapping(z, c)
            target = torch.rand(n, 3, sp.img_resolution, sp.img_resolution, generator=g).to(dev) * 2 - 1
        ws = ws0.clone().requires_grad_(True)

        def step():
            img = G.synthesis(ws, c=c, noise_mode='const')
            loss = ((img - target) ** 2).mean()
            loss.backward()
            ws.grad = None

        modes = tuple({'on': True, 'off': False}[m] for m in args.modes.split(','))
        ms = _time(step, args.warmup, args.blocks, args.iters, modes)
        mem = {m: _peak(step, m) for m in modes}
        r = result[f'projector_step_b{n}'] = {}
        for m, name in ((True, 'hip'), (False, 'aten')):
            if m in ms:
                r[f'{name}_ms'], r[f'{name}_peak_mib'] = round(ms[m], 3), round(mem[m], 1)
        if len(ms) == 2:
            r['speedup'] = round(ms[False] / ms[True], 2)
        torch.cuda.empty_cache()
    print(json.dumps(result))


if __name__ == '__main__':
    main()
