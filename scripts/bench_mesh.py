"""Density cube -> iso-surface mesh on one GPU (csrc/mesh.hip): cube + mesh at 128^3 and 256^3 on a
random-init generator (threshold = the cube's median: random weights have no surface at the drivers' default of 10), and the mesh
alone on an analytic sphere of 256^3 with the per-call breakdown and the host definition as the alternative a user had.
Prints one JSON line and writes it to profiles/mesh/bench_mesh.json."""
import json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'ide-3d_amd')); sys.path.insert(0, ROOT)
import numpy as np
import torch
from training import mesh_extraction as me, shape_extraction as se, triplane
from torch_utils import hip_plugin

dev = torch.device('cuda:0')
REPS = 20


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
    """Milliseconds per call on the host clock, device idle before and after (what a caller of marching_cubes waits for)."""
    for _ in range(3):
        fn()
    torch.cuda.synchronize(); t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps * 1e3


def breakdown(vol, iso):
    table = torch.from_numpy(me.case_table_bytes().copy())
    P = hip_plugin.MeshPlugin
    ws, nv, nt = P.count(vol, iso, table)
    out = dict(vertices=nv, triangles=nt, workspace_MB=ws.numel() * 8 / 1e6)
    lib, st = hip_plugin.load(), hip_plugin._stream(vol)
    X, Y, Z = vol.shape
    tab = P._table(table, vol.device)
    out['count_and_scan_2_launches_ms'] = timed(lambda: lib.ide3d_mesh_count(hip_plugin._ptr(vol), X, Y, Z, iso, hip_plugin._ptr(tab), hip_plugin._ptr(ws), ws.numel() * 8, st))
    out['vertices_launch_ms'] = timed(lambda: P.emit(vol, iso, table, ws, nv, 0))
    both = timed(lambda: P.emit(vol, iso, table, ws, nv, nt))
    out['triangles_launch_ms'] = both - out['vertices_launch_ms']
    out['vertices_with_normals_launch_ms'] = timed(lambda: P.emit(vol, iso, table, ws, nv, 0, normals=True))
    out['marching_cubes_wall_ms'] = wall(lambda: me.marching_cubes(vol, iso))
    out['marching_cubes_with_normals_wall_ms'] = wall(lambda: me.marching_cubes(vol, iso, normals=True))
    out['volume_MB'] = vol.numel() * 4 / 1e6
    return out


res = {}
torch.manual_seed(0)
G = triplane.TriPlaneGenerator().eval().to(dev)
z = torch.from_numpy(np.random.RandomState(0).randn(1, 512)).float().to(dev)
with torch.no_grad():
    ws = G.mapping(z, triplane.conditioning_label(dev), truncation_psi=0.5)
    img_v, seg_v = se.triplanes_from_ws(G.synthesis, ws, noise_mode='const')
    R = G.synthesis.renderer
    for N in (128, 256):
        cube_fn = lambda: se.density_cube(R, img_v, seg_v, N, max_batch=None)
        cube = cube_fn()[0]
        iso = float(cube.reshape(-1).kthvalue(cube.numel() // 2).values)
        r = breakdown(cube, iso)
        r['threshold_cube_median'] = iso
        r['density_cube_ms'] = timed(cube_fn)
        r['cube_plus_mesh_wall_ms'] = wall(lambda: me.marching_cubes(cube_fn()[0], iso, lattice=(2.0 / (N - 1), np.array([-1.0, -1.0, -1.0]), 0.9)))
        res[f'generator_{N}'] = r

N = 256
g = torch.arange(N, device=dev, dtype=torch.float32) - ((N - 1) / 2)
sphere = (96.0 - torch.sqrt((g + 0.13)[:, None, None] ** 2 + (g - 0.21)[None, :, None] ** 2 + (g + 0.37)[None, None, :] ** 2)).contiguous()
res['sphere_256'] = breakdown(sphere, 0.0)
host = sphere.cpu().numpy()
t0 = time.perf_counter()
hv, ht, _ = me.marching_cubes_host(host, 0.0)
res['sphere_256']['host_definition_ms'] = (time.perf_counter() - t0) * 1e3
res['sphere_256']['device_to_host_copy_of_the_cube_ms'] = wall(lambda: sphere.cpu(), reps=5)
v, t = me.marching_cubes(sphere, 0.0)
res['sphere_256']['equals_host_definition'] = bool(np.array_equal(t.cpu().numpy(), ht) and np.abs(v.cpu().numpy() - hv).max() <= 2e-5)
line = json.dumps(dict(metric='density cube -> mesh', device=torch.cuda.get_device_name(0), reps=REPS, **res,
                       native_launches={k: v for k, v in hip_plugin.CALLS.items() if k.startswith('mesh') or k == 'density_lattice'}))
print(line)
out = os.path.join(ROOT, 'profiles', 'mesh')
os.makedirs(out, exist_ok=True)
with open(os.path.join(out, 'bench_mesh.json'), 'w') as f:
    f.write(line + '\n')
