"""Mesh -> image on one GPU (csrc/raster.hip): the mesh of a 256^3 cube (the analytic sphere of
scripts/bench_mesh.py) rendered at 512^2 with 1 and 8 cameras per call, with and without normals and colours: ms per frame of each of the
three launches and of `render_mesh` as a caller sees it, the numpy host definition at 128^2 on the same mesh, and the sweep of the
lane / wave threshold `large_min` on that mesh and on the mesh plus one screen-filling triangle.
Prints one JSON line and writes it to profiles/mesh_render/bench_mesh_render.json."""
import json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'ide-3d_amd')); sys.path.insert(0, ROOT)
import numpy as np
import torch
from training import mesh_extraction as me, mesh_render as mr
from torch_utils import hip_plugin
from bench import gpu_state_under_load

dev = torch.device('cuda:0')
REPS = 20
SIZE = 512


def timed(fn, reps=REPS):
    """Milliseconds per call between two device events (3 warm-up calls)."""
    for _ in range(3):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize(); a.record()
    for _ in range(reps):
        fn()
    b.record(); torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def wall(fn, reps=REPS):
    """Milliseconds per call on the host clock, device idle before and after."""
    for _ in range(3):
        fn()
    torch.cuda.synchronize(); t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps * 1e3


def launches(v, t, cams, normals=None, colors=None, large_min=None):
    """ms per FRAME of the three launches (device events around each alone) for the cameras of one call."""
    P, N = hip_plugin.RasterPlugin, cams.shape[0]
    w2c, light = mr.camera_matrices(cams)
    w2c, light = torch.from_numpy(w2c).to(dev), torch.from_numpy(light).to(dev)
    view = mr.view_constants(SIZE, SIZE)
    ws = P.project(v, w2c, SIZE, SIZE, view, 0.05)
    out = {'project_ms': timed(lambda: P.project(v, w2c, SIZE, SIZE, view, 0.05)) / N,
           'depth_ms': timed(lambda: P.depth(ws, v, t, N, SIZE, SIZE, large_min=large_min)) / N,
           'shade_ms': timed(lambda: P.shade(ws, v, t, N, SIZE, SIZE, light, normals=normals, colors=colors)) / N}
    out['three_launches_ms'] = sum(out.values())
    return out


N3 = 256
g = torch.arange(N3, device=dev, dtype=torch.float32) - ((N3 - 1) / 2)
sphere = (96.0 - torch.sqrt((g + 0.13)[:, None, None] ** 2 + (g - 0.21)[None, :, None] ** 2 + (g + 0.37)[None, None, :] ** 2)).contiguous()
v, t, n = me.marching_cubes(sphere, 0.0, normals=True)
v = (v / N3 - 0.5).contiguous()          # the frame of mesh_from_cube_file: the turntable cameras see it whole
colors = ((n * 0.5 + 0.5) * 255).to(torch.uint8).contiguous()
cams = mr.turntable_cameras(8, device=dev)
res = {'vertices': int(v.shape[0]), 'triangles': int(t.shape[0]), 'size': SIZE}

for ncam in (1, 8):
    for name, kw in (('plain', {}), ('normals_colors', dict(normals=n, colors=colors))):
        r = launches(v, t, cams[:ncam], **kw)
        r['render_mesh_wall_ms'] = wall(lambda: mr.render_mesh(v, t, cams[:ncam], size=SIZE, validate=False, **kw)) / ncam
        r['render_mesh_validate_wall_ms'] = wall(lambda: mr.render_mesh(v, t, cams[:ncam], size=SIZE, validate=True, **kw)) / ncam
        res[f'{ncam}_cameras_{name}'] = r

out = mr.render_mesh(v, t, cams[:1], size=SIZE, normals=n, colors=colors, validate=False)
res['foreground_share'] = float((out['triangle'] >= 0).float().mean())
res['turntable_240_frames_wall_s'] = wall(lambda: [f for f in mr.render_turntable(dict(vertices=v, triangles=t, normals=n), num_frames=240, size=SIZE, chunk=8)], reps=2) / 1e3

# the lane / wave threshold: the mesh alone (every triangle a few pixels) and with one screen-filling triangle in front of the far half
big = torch.tensor([[-3.0, -3.0, -0.3], [3.0, -3.0, -0.3], [0.0, 4.0, -0.3]], device=dev)
v_big, t_big = torch.cat([v, big]).contiguous(), torch.cat([t, torch.tensor([[v.shape[0], v.shape[0] + 1, v.shape[0] + 2]], dtype=torch.int32, device=dev)]).contiguous()
sweep = {}
for large_min in (0, 64, 128, 256, 512, 1024, 2048, 4096, 2 ** 31 - 1):
    sweep[str(large_min)] = {'mesh_depth_ms': launches(v, t, cams[:1], large_min=large_min)['depth_ms'],
                             'mesh_plus_screen_filling_depth_ms': launches(v_big, t_big, cams[:1], large_min=large_min)['depth_ms']}
res['large_min_sweep'] = sweep
a = mr.render_mesh(v_big, t_big, cams[:1], size=SIZE, validate=False, large_min=0)
b = mr.render_mesh(v_big, t_big, cams[:1], size=SIZE, validate=False, large_min=2 ** 31 - 1)
res['lane_and_wave_paths_bit_equal'] = all(torch.equal(a[k], b[k]) for k in a)
res['screen_filling_share'] = float((a['triangle'] == t.shape[0]).float().mean())

vh, th = v.cpu(), t.cpu()
t0 = time.perf_counter()
host = mr.render_mesh(vh, th, cams[:1].cpu(), size=128, validate=False)
res['host_definition_128_ms'] = (time.perf_counter() - t0) * 1e3
dev128 = mr.render_mesh(v, t, cams[:1], size=128, validate=False)
res['equals_host_definition_128'] = all(torch.equal(dev128[k].cpu(), host[k]) for k in host)

ws = hip_plugin.RasterPlugin.project(v, torch.from_numpy(mr.camera_matrices(cams)[0]).to(dev), SIZE, SIZE, mr.view_constants(SIZE, SIZE), 0.05)
res['gpu_state'] = gpu_state_under_load(lambda i: hip_plugin.RasterPlugin.depth(ws, v, t, 8, SIZE, SIZE), busy_steps=400)
line = json.dumps(dict(metric='mesh -> image', device=torch.cuda.get_device_name(0), reps=REPS, **res,
                       native_launches={k: c for k, c in hip_plugin.CALLS.items() if k.startswith('raster')}))
print(line)
outdir = os.path.join(ROOT, 'profiles', 'mesh_render')
os.makedirs(outdir, exist_ok=True)
with open(os.path.join(outdir, 'bench_mesh_render.json'), 'w') as f:
    f.write(line + '\n')
