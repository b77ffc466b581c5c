"""The hierarchical (importance) pass with gradients on one GPU: `TriplaneRenderer.forward(hierarchical=True)` forward + backward to the
tri-planes, and once to the planes and the decoder (under `triplane.fused_render_param_grad`), with `triplane.fused_hierarchical_grad` off
(the step-wise path: sample_voxel x2, cat / sort / gather, fancy_integration, autograd through all of it) and on (four launches forward,
one launch backward), alternating in one process: batch 1 and 4, 64 x 64 rays on 256 x 256 planes (C = 32,
hidden 64), S = 48 and 96.  Per shape and gradient set: milliseconds per call between device events after warm-up of both paths (median
and min / max of 7 rounds of 10 calls), peak device memory above the inputs, the two paths' plane gradients against each other (they draw
different z_fine: a scale, not a gate), and the backward launch alone.
Prints one JSON line and writes it to profiles/hier_grad/bench_hier_grad.json (or under --out).

    python scripts/bench_hier_grad.py [--batches 1,4] [--steps 48,96] [--rounds 7] [--reps 10] [--out DIR]
"""
import argparse, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'ide-3d_amd')); sys.path.insert(0, ROOT)
import torch
from training import triplane, volumetric_rendering as vr
from torch_utils import hip_plugin

ap = argparse.ArgumentParser()
ap.add_argument('--batches', default='1,4')
ap.add_argument('--steps', default='48,96')
ap.add_argument('--rounds', type=int, default=7)
ap.add_argument('--reps', type=int, default=10)
ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'hier_grad'))
args = ap.parse_args()
dev = torch.device('cuda:0')


def timed(fn, reps):
    """Milliseconds per call between two device events."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize(); a.record()
    for _ in range(reps):
        fn()
    b.record(); torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def peak_mb(fn):
    torch.cuda.synchronize(); torch.cuda.empty_cache(); torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return (torch.cuda.max_memory_allocated() - base) / 1e6


def rel(a, b):
    return float((a - b).abs().max()) / float(b.abs().max())


def stats(xs):
    xs = sorted(xs)
    return dict(median_ms=xs[len(xs) // 2], min_ms=xs[0], max_ms=xs[-1])


torch.manual_seed(0)
sp = triplane.GeneratorSpec()
R = triplane.TriplaneRenderer(sp).to(dev).eval().requires_grad_(False)
with torch.no_grad():
    for p in R.parameters():
        if p.ndim == 1:
            p.copy_(torch.randn_like(p) * 0.2)
nch = sp.feature_channels + sp.seg_channels
res = {}
for n in (int(b) for b in args.batches.split(',')):
    for S in (int(s) for s in args.steps.split(',')):
        g = torch.Generator().manual_seed(10 * n + S)
        tex, geo = ((torch.randn(n, 96, 256, 256, generator=g) * 0.7).to(dev).contiguous(memory_format=torch.channels_last).requires_grad_(True)
                    for _ in range(2))
        cam = torch.cat([triplane.camera_label(0.4 - 0.2 * i) for i in range(n)])[:, :16].reshape(n, 4, 4).to(dev)
        jit, u = torch.rand(n, 4096, S, generator=g).to(dev), torch.rand(n * 4096, S, generator=g).to(dev)
        Pf, Pd = torch.randn(n, nch, 64, 64, generator=g).to(dev), torch.randn(n, 1, 64, 64, generator=g).to(dev)
        shape = {}
        for what in ('planes', 'planes_and_decoder'):
            with_decoder = what == 'planes_and_decoder'
            R.decoder.requires_grad_(with_decoder)
            triplane.fused_render_param_grad = with_decoder
            leaves = [tex, geo] + (list(R.decoder.parameters()) if with_decoder else [])

            def call(on):
                triplane.fused_hierarchical_grad = on
                feat, depth, wsum = R(tex, geo, cam, num_steps=S, jitter=jit, hierarchical=True, importance_u=u)
                return torch.autograd.grad((feat * Pf).sum() + (depth * Pd).sum() + wsum.sum(), leaves)

            hip_plugin.CALLS.clear()
            grads = {on: call(on) for on in (False, True)}
            assert hip_plugin.CALLS.get('render_rays_merged_backward') == 1, dict(hip_plugin.CALLS)
            for _ in range(3):
                call(False); call(True)
            times = {False: [], True: []}
            for _ in range(args.rounds):                        # alternating: both paths see the same machine
                for on in (False, True):
                    times[on].append(timed(lambda: call(on), args.reps))
            r = dict(stepwise=stats(times[False]), fused=stats(times[True]))
            r['speedup_of_medians'] = r['stepwise']['median_ms'] / r['fused']['median_ms']
            r['stepwise']['peak_MB_above_inputs'] = peak_mb(lambda: call(False))
            r['fused']['peak_MB_above_inputs'] = peak_mb(lambda: call(True))
            r['memory_ratio'] = r['stepwise']['peak_MB_above_inputs'] / r['fused']['peak_MB_above_inputs']
            r['plane_grads_rel_diff'] = dict(tex=rel(grads[True][0], grads[False][0]), geo=rel(grads[True][1], grads[False][1]))
            del grads
            shape[what] = r
        R.decoder.requires_grad_(False)
        triplane.fused_render_param_grad = False
        # the backward launch alone (planes only), beside the plain march's backward over S samples for scale
        P = hip_plugin.VolumeRenderPlugin
        rays_d, z_lin = vr._fused_ray_setup(dev, float(sp.fov), (64, 64), S, float(sp.ray_start), float(sp.ray_end))
        with torch.no_grad():
            mlp = R.decoder.kernel_weights()
            td, gd = tex.detach(), geo.detach()
            _w, z, bins, pw = P.render_ray_weights(rays_d, z_lin, cam, jit, None, td, gd, mlp, 0, want=('z_vals', 'pdf_bins', 'pdf_weights'))
            z_fine = P.sample_pdf(bins, pw, u)
            z_all, src = P.merge_depths(z_fine, z)
            gf, gdp = Pf.reshape(n, nch, -1), Pd.reshape(n, -1)
            parts = dict(render_rays_merged_backward=lambda: P.render_rays_merged_backward(rays_d, z_lin, cam, jit, td, gd, mlp, 0, False, None, z_all,
                                                                                          src, z_fine, gf, gdp, None),
                         plain_render_rays_backward_for_scale=lambda: P.render_rays_backward(rays_d, z_lin, cam, jit, None, td, gd, mlp, 0, False,
                                                                                            False, None, gf, gdp, None))
            for fn in parts.values():
                fn()
            shape['launch_ms'] = {k: min(timed(fn, 10) for _ in range(3)) for k, fn in parts.items()}
        shape['atomic_bytes'] = 2 * 3 * 4 * 32 * 4 * n * 4096 * 2 * S
        res[f'batch{n}_S{S}'] = shape
        del tex, geo
        torch.cuda.empty_cache()
triplane.fused_hierarchical_grad = False
line = json.dumps(dict(metric='hierarchical pass forward + backward: step-wise path vs fused_hierarchical_grad', device=torch.cuda.get_device_name(0),
                       rounds=args.rounds, reps_per_round=args.reps, arithmetic=hip_plugin.conv_arithmetic(), **res,
                       exclusive_violations=hip_plugin.exclusive_violations()[0]))
print(line)
os.makedirs(args.out, exist_ok=True)
with open(os.path.join(args.out, 'bench_hier_grad.json'), 'w') as f:
    f.write(line + '\n')
