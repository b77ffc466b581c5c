"""The fused renderer's backward with decoder-parameter gradients (`triplane.fused_render_param_grad = True`,
ide3d_render_rays_backward_params) against the step-wise definition (False), alternated in one process.  Full spec:
64 x 64 rays, 96 steps, 256 x 256 planes.  Prints one JSON line.

    python scripts/bench_decoder_grad.py [--batches 1,4] [--blocks 5] [--iters 5] [--warmup 2] [--rows a,b,c]

  a  renderer forward + backward alone, decoder and planes both requiring grad: switch on / off, with peak memory
  b  the full-spec tuning step of scripts/bench_param_grad.py (`networks.hip_param_grad = True` in both modes): switch on / off
  c  the tri-plane-only backward (frozen decoder, the switch at its default): the non-regression row, to compare with the same
     measurement (scripts/bench_render_grad.py --no-projector) on the parent commit's library

Times are device-event medians over blocks (per iteration), after warm-up, with the block-to-block spread (max - min); peak memory is
torch.cuda.max_memory_allocated over one step, minus what was allocated before it."""
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
    """{mode: (median ms per iteration, max - min over blocks)}, the modes alternated block by block"""
    out = {m: [] for m in modes}
    for m in modes:
        triplane.fused_render_param_grad = m
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    for _ in range(blocks):
        for m in modes:
            triplane.fused_render_param_grad = m
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(iters):
                fn()
            e1.record()
            torch.cuda.synchronize()
            out[m].append(e0.elapsed_time(e1) / iters)
    triplane.fused_render_param_grad = False
    return {m: (statistics.median(v), max(v) - min(v)) for m, v in out.items()}


def _peak(fn, mode):
    triplane.fused_render_param_grad = mode
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    triplane.fused_render_param_grad = False
    return (torch.cuda.max_memory_allocated() - base) / 2 ** 20


def _row(ms, mem=None):
    r = {}
    for m, name in ((True, 'on'), (False, 'off')):
        if m in ms:
            r[f'{name}_ms'], r[f'{name}_spread_ms'] = round(ms[m][0], 3), round(ms[m][1], 3)
            if mem is not None:
                r[f'{name}_peak_mib'] = round(mem[m], 1)
    if len(ms) == 2:
        r['speedup'] = round(ms[False][0] / ms[True][0], 2)
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batches', default='1,4')
    ap.add_argument('--blocks', type=int, default=5)
    ap.add_argument('--iters', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--rows', default='a,b,c')
    args = ap.parse_args()
    rows = args.rows.split(',')
    dev = torch.device('cuda:0')
    sp = triplane.GeneratorSpec()
    rays, S, C = sp.render_size ** 2, sp.num_steps, sp.plane_channels
    nch = sp.feature_channels + sp.seg_channels
    result = dict(bench='decoder_grad', spec=dict(rays=rays, steps=S, plane=sp.plane_resolution, C=C, hidden=sp.decoder_hidden),
                  device=torch.cuda.get_device_name(dev))
    for n in (int(b) for b in args.batches.split(',')):
        if 'a' in rows or 'c' in rows:
            torch.manual_seed(0)
            R = triplane.TriplaneRenderer(sp).to(dev).eval()
            g = torch.Generator().manual_seed(n)
            tex = (torch.randn(n, 3 * C, sp.plane_resolution, sp.plane_resolution, generator=g) * 0.7).to(dev).contiguous(
                memory_format=torch.channels_last).requires_grad_(True)
            geo = (torch.randn(n, 3 * C, sp.plane_resolution, sp.plane_resolution, generator=g) * 0.7).to(dev).contiguous(
                memory_format=torch.channels_last).requires_grad_(True)
            cam = torch.cat([triplane.camera_label(0.5 * (i % 3 - 1)) for i in range(n)])[:, :16].reshape(-1, 4, 4).to(dev)
            jit = torch.rand(n, rays, S, generator=g).to(dev)
            Pf = torch.randn(n, nch, sp.render_size, sp.render_size, generator=g).to(dev)
            Pd = torch.randn(n, 1, sp.render_size, sp.render_size, generator=g).to(dev)

            def step():
                feat, depth, wsum = R(tex, geo, cam, jitter=jit)
                leaves = [tex, geo] + [p for p in R.decoder.parameters() if p.requires_grad]
                torch.autograd.grad((feat * Pf).sum() + (depth * Pd).sum() + wsum.sum(), leaves)

            if 'a' in rows:
                R.requires_grad_(True)
                ms = _time(step, args.warmup, args.blocks, args.iters, (True, False))
                result[f'a_renderer_trainable_decoder_b{n}'] = _row(ms, {m: _peak(step, m) for m in (True, False)})
            if 'c' in rows:
                R.requires_grad_(False)
                ms = _time(step, args.warmup, args.blocks, args.iters, (False,))
                result[f'c_renderer_planes_only_b{n}'] = dict(fused_ms=round(ms[False][0], 3), spread_ms=round(ms[False][1], 3))
            del tex, geo, R
            torch.cuda.empty_cache()
        if 'b' in rows:
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

            def tune():
                opt.zero_grad(set_to_none=True)
                img = G.synthesis(w_pivot, c=c, noise_mode='const', force_fp32=True)
                ((img - target) ** 2).mean().backward()
                opt.step()

            networks.hip_param_grad = True
            try:
                ms = _time(tune, args.warmup, args.blocks, max(1, args.iters // 2), (True, False))
                result[f'b_tuning_step_b{n}'] = _row(ms, {m: _peak(tune, m) for m in (True, False)})
            finally:
                networks.hip_param_grad = False
            del G, opt
            torch.cuda.empty_cache()
    print(json.dumps(result))


if __name__ == '__main__':
    main()
