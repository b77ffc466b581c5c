"""The fused renderer's backward with the camera gradient (`triplane.fused_render_camera_grad = True`,
ide3d_render_rays_backward_camera) against the step-wise definition (False), alternated in one process.  Full spec:
64 x 64 rays, 96 steps, 256 x 256 planes.  Prints one JSON line.

    python scripts/bench_camera_grad.py [--batches 1,4] [--blocks 5] [--iters 5] [--warmup 2] [--rows a,b,c]

  a  renderer forward + backward, only the camera requiring grad (planes and decoder frozen): switch on / off, with peak memory
  b  the same with the planes requiring grad too (a projector's step: w and the pose): switch on / off, with peak memory
  c  the tri-plane-only backward (frozen camera, the switch at its default): the non-regression row, to compare with row c of
     scripts/bench_decoder_grad.py on the parent commit's library

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
from training import triplane  # noqa: E402


def _time(fn, warmup, blocks, iters, modes):
    """{mode: (median ms per iteration, max - min over blocks)}, the modes alternated block by block"""
    out = {m: [] for m in modes}
    for m in modes:
        triplane.fused_render_camera_grad = m
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    for _ in range(blocks):
        for m in modes:
            triplane.fused_render_camera_grad = m
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(iters):
                fn()
            e1.record()
            torch.cuda.synchronize()
            out[m].append(e0.elapsed_time(e1) / iters)
    triplane.fused_render_camera_grad = False
    return {m: (statistics.median(v), max(v) - min(v)) for m, v in out.items()}


def _peak(fn, mode):
    triplane.fused_render_camera_grad = mode
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    triplane.fused_render_camera_grad = False
    return (torch.cuda.max_memory_allocated() - base) / 2 ** 20


def _row(ms, mem):
    r = {}
    for m, name in ((True, 'on'), (False, 'off')):
        r[f'{name}_ms'], r[f'{name}_spread_ms'], r[f'{name}_peak_mib'] = round(ms[m][0], 3), round(ms[m][1], 3), round(mem[m], 1)
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
    result = dict(bench='camera_grad', spec=dict(rays=rays, steps=S, plane=sp.plane_resolution, C=C, hidden=sp.decoder_hidden),
                  device=torch.cuda.get_device_name(dev))
    for n in (int(b) for b in args.batches.split(',')):
        torch.manual_seed(0)
        R = triplane.TriplaneRenderer(sp).to(dev).eval().requires_grad_(False)
        g = torch.Generator().manual_seed(n)
        tex = (torch.randn(n, 3 * C, sp.plane_resolution, sp.plane_resolution, generator=g) * 0.7).to(dev).contiguous(memory_format=torch.channels_last)
        geo = (torch.randn(n, 3 * C, sp.plane_resolution, sp.plane_resolution, generator=g) * 0.7).to(dev).contiguous(memory_format=torch.channels_last)
        cam = torch.cat([triplane.camera_label(0.5 * (i % 3 - 1)) for i in range(n)])[:, :16].reshape(-1, 4, 4).to(dev)
        jit = torch.rand(n, rays, S, generator=g).to(dev)
        Pf = torch.randn(n, nch, sp.render_size, sp.render_size, generator=g).to(dev)
        Pd = torch.randn(n, 1, sp.render_size, sp.render_size, generator=g).to(dev)

        def step():
            feat, depth, wsum = R(tex, geo, cam, jitter=jit)
            torch.autograd.grad((feat * Pf).sum() + (depth * Pd).sum() + wsum.sum(), [t for t in (cam, tex, geo) if t.requires_grad])

        for row, name, planes, camera in (('a', 'a_camera_only', False, True), ('b', 'b_camera_and_planes', True, True)):
            if row in rows:
                tex.requires_grad_(planes); geo.requires_grad_(planes); cam.requires_grad_(camera)
                ms = _time(step, args.warmup, args.blocks, args.iters, (True, False))
                result[f'{name}_b{n}'] = _row(ms, {m: _peak(step, m) for m in (True, False)})
        if 'c' in rows:
            tex.requires_grad_(True); geo.requires_grad_(True); cam.requires_grad_(False)
            ms = _time(step, args.warmup, args.blocks, args.iters, (False,))
            result[f'c_renderer_planes_only_b{n}'] = dict(fused_ms=round(ms[False][0], 3), spread_ms=round(ms[False][1], 3))
        del tex, geo, R
        torch.cuda.empty_cache()
    print(json.dumps(result))


if __name__ == '__main__':
    main()
