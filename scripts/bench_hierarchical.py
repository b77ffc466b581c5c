"""The hierarchical (importance) pass of the renderer on one GPU: `TriplaneRenderer.forward(hierarchical=True)` with
`triplane.fused_hierarchical` off (step-wise HIP ops: sample_voxel x2, composite x2, sample_pdf, torch cat / sort / gather) and on (four
launches), alternating in one process: batch 1 and 4, 64 x 64 rays on 256 x 256 planes (C = 32, hidden 64),
S = 48 and 96.  Per shape: milliseconds per call between device events after warm-up (median and min / max of the rounds), peak device
memory above the inputs, the two paths' outputs against each other, and the new path's launches one by one.
Prints one JSON line and writes it to profiles/hierarchical/bench_hierarchical.json."""
import json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'ide-3d_amd')); sys.path.insert(0, ROOT)
import torch
from training import triplane, volumetric_rendering as vr
from torch_utils import hip_plugin

dev = torch.device('cuda:0')
ROUNDS, REPS = 7, 10


def timed(fn, reps=REPS):
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
R = triplane.TriplaneRenderer(sp).to(dev).eval()
with torch.no_grad():
    for p in R.parameters():
        if p.ndim == 1:
            p.copy_(torch.randn_like(p) * 0.2)
res = {}
for n in (1, 4):
    for S in (48, 96):
        g = torch.Generator().manual_seed(10 * n + S)
        tex, geo = ((torch.randn(n, 96, 256, 256, generator=g) * 0.7).to(dev).contiguous(memory_format=torch.channels_last) for _ in range(2))
        cam = torch.cat([triplane.camera_label(0.4 - 0.2 * i) for i in range(n)])[:, :16].reshape(n, 4, 4).to(dev)
        jit, u = torch.rand(n, 4096, S, generator=g).to(dev), torch.rand(n * 4096, S, generator=g).to(dev)

        def call(on):
            triplane.fused_hierarchical = on
            with torch.no_grad():
                return R(tex, geo, cam, num_steps=S, jitter=jit, hierarchical=True, importance_u=u)

        out = {on: call(on) for on in (False, True)}
        for _ in range(3):
            call(False); call(True)
        times = {False: [], True: []}
        for _ in range(ROUNDS):                             # alternating: both paths see the same machine
            for on in (False, True):
                times[on].append(timed(lambda: call(on)))
        r = dict(stepwise=stats(times[False]), four_launches=stats(times[True]))
        r['speedup_of_medians'] = r['stepwise']['median_ms'] / r['four_launches']['median_ms']
        r['stepwise']['peak_MB_above_inputs'] = peak_mb(lambda: call(False))
        r['four_launches']['peak_MB_above_inputs'] = peak_mb(lambda: call(True))
        r['outputs_rel_diff'] = dict(zip(('features', 'depth', 'weight_sum'), (rel(a, b) for a, b in zip(out[True], out[False]))))
        # the new path's launches one by one
        P = hip_plugin.VolumeRenderPlugin
        rays_d, z_lin = vr._fused_ray_setup(dev, float(sp.fov), (64, 64), S, float(sp.ray_start), float(sp.ray_end))
        with torch.no_grad():
            mlp = R.decoder.kernel_weights()
            first = lambda: P.render_ray_weights(rays_d, z_lin, cam, jit, None, tex, geo, mlp, 0, want=('z_vals', 'pdf_bins', 'pdf_weights'))
            _w, z, bins, pw = first()
            z_fine = P.sample_pdf(bins, pw, u)
            z_all, src = P.merge_depths(z_fine, z)
            parts = dict(render_ray_weights=first, sample_pdf=lambda: P.sample_pdf(bins, pw, u), merge_depths=lambda: P.merge_depths(z_fine, z),
                         render_rays_merged=lambda: P.render_rays_merged(rays_d, z_lin, cam, jit, tex, geo, mlp, 0, False, None, z_all, src, z_fine),
                         plain_render_rays_for_scale=lambda: P.render_rays(rays_d, z_lin, cam, jit, None, tex, geo, mlp, 0, False, False, None))
            for fn in parts.values():
                fn()
            r['launch_ms'] = {k: min(timed(fn, 20) for _ in range(3)) for k, fn in parts.items()}
        res[f'batch{n}_S{S}'] = r
triplane.fused_hierarchical = False
line = json.dumps(dict(metric='hierarchical pass: step-wise ops vs four launches', device=torch.cuda.get_device_name(0), rounds=ROUNDS,
                       reps_per_round=REPS, arithmetic=hip_plugin.conv_arithmetic(), **res,
                       exclusive_violations=hip_plugin.exclusive_violations()[0]))
print(line)
out = os.path.join(ROOT, 'profiles', 'hierarchical')
os.makedirs(out, exist_ok=True)
with open(os.path.join(out, 'bench_hierarchical.json'), 'w') as f:
    f.write(line + '\n')
