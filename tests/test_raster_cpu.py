"""training/mesh_render.py without a GPU: the numpy host definition of the rasterizer (csrc/raster.hip) against
the plain-loop float64 / Python-int restatement of tests/raster_ref.py, the documented handling of triangles that are not drawn, the
closed forms of a sphere seen head-on, the turntable cameras, the cube-file and y4m round trips, and the C ABI."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

import raster_ref as rr
from training import mesh_render as mr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CAM = rr.head_on_camera(4.0)


def host_render(v, t, cam=CAM, size=16, fov=rr.FOV_EXACT, **kw):
    out = mr.render_mesh(torch.from_numpy(np.asarray(v, dtype=np.float32)), torch.from_numpy(np.asarray(t, dtype=np.int32)),
                         torch.from_numpy(np.asarray(cam)), size=size, fov=fov, **kw)
    return {k: a.numpy() for k, a in out.items()}


def host_records(v, cam=CAM, size=16, fov=rr.FOV_EXACT, **kw):
    return mr.project_vertices(torch.from_numpy(np.asarray(v, dtype=np.float32)), torch.from_numpy(np.asarray(cam)), size=size, fov=fov, **kw).numpy()


# ---- coverage -------------------------------------------------------------------------------------------------------------------

def test_exact_placement_of_the_test_meshes():
    """The premise of the partition tests: at fov 90 the projection puts the corners on the intended multiples of 1/8 pixel exactly."""
    for ox, oy in rr.offsets64():
        v, _, (x0, y0, x1, y1) = rr.split_quad(ox, oy)
        rec = host_records(v)[0]
        assert rec[:, :2].tolist() == [[round(256 * x), round(256 * y)] for x, y in ((x0, y0), (x1, y0), (x1, y1), (x0, y1))]
        assert (rec[:, 3] == 0).all() and rr.record_depths(rec).tolist() == [1.0, 2.0, 2.0, 1.0]


def test_split_quad_partition():
    """64 sub-pixel offsets; at (0, 0) the corners and the diagonal lie exactly on sample points.  Every sample of the half-open square
    [x0, x1) x [y0, y1) is covered by exactly one of the two triangles, no other sample by any; the host definition's map agrees."""
    for ox, oy in rr.offsets64():
        v, t, (x0, y0, x1, y1) = rr.split_quad(ox, oy)
        cover = rr.coverage_int(host_records(v)[0], t, 16, 16)
        tri = host_render(v, t)['triangle'][0]
        for r in range(16):
            for c in range(16):
                inside = x0 <= c + 0.5 < x1 and y0 <= r + 0.5 < y1
                assert len(cover.get((r, c), [])) == (1 if inside else 0), (ox, oy, r, c)
                assert tri[r, c] == (cover[(r, c)][0] if inside else -1), (ox, oy, r, c)
    v, t, _ = rr.split_quad(0.0, 0.0)
    on_diagonal = [rr.edge_values(*rr._oriented(host_records(v)[0], t[0].tolist()), k + 2, k + 2)[1][0] for k in range(8)]
    assert on_diagonal == [0] * 8, 'the diagonal was meant to pass through sample points'


def _polygon_side(ring8, x8, y8):
    """+1 strictly inside, -1 strictly outside, 0 on the boundary of a convex polygon; coordinates in 1/8 pixel as Python ints."""
    cr = [(bx - ax) * (y8 - ay) - (by - ay) * (x8 - ax) for (ax, ay), (bx, by) in zip(ring8, ring8[1:] + ring8[:1])]
    if all(v > 0 for v in cr) or all(v < 0 for v in cr):
        return 1
    if all(v >= 0 for v in cr) or all(v <= 0 for v in cr):
        return 0
    return -1


def test_closed_fan_partition():
    """A vertex shared by a closed fan (exactly on a sample point at offset (0, 0)) and the spokes belong to exactly one triangle."""
    centre_hit = 0
    for ox, oy in rr.offsets64():
        v, t, ring = rr.closed_fan(ox, oy)
        ring8 = [(round(8 * x), round(8 * y)) for x, y in ring]
        cover = rr.coverage_int(host_records(v)[0], t, 16, 16)
        tri = host_render(v, t)['triangle'][0]
        for r in range(16):
            for c in range(16):
                side, n = _polygon_side(ring8, 8 * c + 4, 8 * r + 4), len(cover.get((r, c), []))
                assert n == 1 if side > 0 else n == 0 if side < 0 else n <= 1, (ox, oy, r, c, n)
                assert tri[r, c] == (cover[(r, c)][0] if n else -1)
        centre_hit += (ox, oy) == (0.0, 0.0) and len(cover[(8, 8)]) == 1
    assert centre_hit == 1


# ---- nearest triangle -------------------------------------------------------------------------------------------------------------

def sphere_case(size=64):
    v, t, n = rr.sphere_mesh()
    return v, t, n, rr.head_on_camera(2.7), size


def test_triangle_map_is_the_float64_argmin():
    """The host definition's winner per pixel = the covering triangle of least float64 depth; near ties (within twice the float32 depth
    bound, rr.NEAR_TIE_REL) may go either way for at most 1 % of the covered pixels.  Measured share here: interpenetrating pair 0 of
    439 covered pixels, sphere 0 of 1976, duplicated quad 0 (exact ties go to the lower index)."""
    v, t = rr.interpenetrating_pair()
    tri = host_render(v, t, size=32)['triangle'][0]
    covered, used = rr.check_triangle_map(tri, host_records(v, size=32)[0], t, 32, 32)
    print(f'pair: {used} near ties of {covered} covered pixels')
    assert covered > 200 and used <= 0.01 * covered and set(np.unique(tri)) == {-1, 0, 1}
    v, t, _, cam, size = sphere_case()
    tri = host_render(v, t, cam=cam, size=size, fov=18.0, validate=False)['triangle'][0]
    covered, used = rr.check_triangle_map(tri, host_records(v, cam=cam, size=size, fov=18.0)[0], t, size, size)
    print(f'sphere: {used} near ties of {covered} covered pixels')
    assert covered > 1000 and used <= 0.01 * covered
    v, t, _ = rr.split_quad(0.25, 0.625)
    t2 = np.concatenate([t, t, t[::-1]])
    tri = host_render(v, t2)['triangle'][0]
    covered, used = rr.check_triangle_map(tri, host_records(v)[0], t2, 16, 16)
    assert covered == 64 and used == 0 and set(np.unique(tri)) == {-1, 0, 1}


def test_cull_modes_follow_the_geometric_normal():
    v, t, _ = rr.split_quad(0.375, 0.125)
    t = np.concatenate([t, t[:, ::-1] + 0])                    # the same two triangles with the opposite winding, behind in index
    normal_z = [float(np.cross(v[b] - v[a], v[c] - v[a])[2]) for a, b, c in t]          # the camera looks down -z: toward it is +z
    for cull, want in (('none', {0, 1}), ('back', {i for i in range(4) if normal_z[i] > 0}), ('front', {i for i in range(4) if normal_z[i] < 0})):
        tri = host_render(v, t, cull=cull)['triangle'][0]
        assert set(np.unique(tri)) - {-1} == want and (tri >= 0).sum() == 64, cull
    assert {i for i in range(4) if normal_z[i] > 0} in ({0, 1}, {2, 3})


# ---- what is not drawn ------------------------------------------------------------------------------------------------------------

def test_skipped_raised_or_clipped():
    H = W = 16
    w = lambda px, py, d: rr.screen_to_world(px, py, d, H, W)
    quad_v, quad_t, _ = rr.split_quad()
    base = host_render(quad_v, quad_t)['triangle']

    def with_extra(points):
        v = np.concatenate([quad_v, np.array(points, dtype=np.float32)])
        return v, np.concatenate([quad_t, [[4, 5, 6]]]).astype(np.int32)

    # degenerate (three points on one line, two equal points): skipped, nothing to report
    for pts in ([w(1, 1, 1), w(5, 5, 1), w(9, 9, 1)], [w(1, 1, 1), w(1, 1, 1), w(9, 3, 1)]):
        assert np.array_equal(host_render(*with_extra(pts))['triangle'], base)
    # off-screen but inside the guard band: skipped silently
    assert np.array_equal(host_render(*with_extra([w(-40, 3, 1), w(-20, 3, 1), w(-30, 12, 1)]))['triangle'], base)
    # partly off-screen: clipped to the screen box, drawn exactly where coverage_int says
    v, t = with_extra([w(-9, -7, 0.5), w(14, 1, 0.5), w(2, 30, 0.5)])
    tri = host_render(v, t)['triangle'][0]
    cover = rr.coverage_int(host_records(v)[0], t, H, W)
    want = {rc for rc, ts in cover.items() if 2 in ts}
    assert len(want) > 40 and {(r, c) for r, c in zip(*np.nonzero(tri == 2))} == want
    # wholly behind the camera: skipped silently (a camera that looks away gives the background)
    out = host_render(quad_v, quad_t, cam=rr.looking_away_camera(4.0))
    assert (out['triangle'] == -1).all() and np.isinf(out['depth']).all() and (out['image'] == 1).all()
    # straddling `near`: no clipping -> raised by validate, dropped whole without it
    v, t = with_extra([w(4, 4, 1), w(12, 5, 1), [0.0, 0.0, 4.0 - 0.01]])
    with pytest.raises(ValueError, match='no clipping'):
        host_render(v, t)
    assert np.array_equal(host_render(v, t, validate=False)['triangle'], base)
    assert host_records(v)[0][6, 3] == mr.BEHIND
    # outside the guard band with the rest on the screen: the same
    v, t = with_extra([w(4, 4, 1), w(12, 5, 1), w(20000, 5, 1)])
    assert host_records(v)[0][6].tolist()[:2] == [0, 0] and host_records(v)[0][6, 3] == mr.OUTSIDE
    with pytest.raises(ValueError, match='no clipping'):
        host_render(v, t)
    assert np.array_equal(host_render(v, t, validate=False)['triangle'], base)
    # outside the guard band with the rest off the screen: nothing a user would miss
    v, t = with_extra([w(-50, 4, 1), w(-30, 5, 1), w(-20000, 5, 1)])
    assert np.array_equal(host_render(v, t)['triangle'], base)


def test_out_of_range_index_is_skipped_and_raised():
    """CPU only: no GPU test feeds such an index."""
    v, t, _ = rr.split_quad()
    base = host_render(v, t)['triangle']
    for bad in (4, -1, 2 ** 31 - 1):
        t2 = np.concatenate([t, [[0, 1, bad]]]).astype(np.int32)
        with pytest.raises(ValueError, match='outside'):
            host_render(v, t2)
        assert np.array_equal(host_render(v, t2, validate=False)['triangle'], base)
        assert rr.coverage_int(host_records(v)[0], t2, 16, 16) == rr.coverage_int(host_records(v)[0], t, 16, 16)


def test_empty_mesh_and_sizes():
    out = host_render(np.zeros([0, 3]), np.zeros([0, 3]), size=(5, 9))
    assert out['depth'].shape == (1, 1, 5, 9) and out['image'].shape == (1, 3, 5, 9) and (out['triangle'] == -1).all()
    v, t, _ = rr.split_quad()
    out = host_render(v, t, cam=np.concatenate([CAM, CAM]).reshape(2, 16), labels=np.arange(4), bg=0.25)
    assert out['label'].shape == (2, 16, 16) and np.array_equal(out['triangle'][0], out['triangle'][1])
    assert (out['image'][:, :, 0, 0] == 0.25).all() and (out['label'][0][out['triangle'][0] < 0] == -1).all()


# ---- closed forms -----------------------------------------------------------------------------------------------------------------

def test_sphere_head_on_closed_forms():
    v, t, n, cam, size = sphere_case()
    dist, r, voxel = 2.7, rr.SPHERE_RADIUS, 1.0 / rr.SPHERE_N
    for normals in (n, None):
        out = host_render(v, t, cam=cam, size=size, fov=18.0, normals=normals, validate=False)
        centre = out['depth'][0, 0, size // 2 - 1:size // 2 + 1, size // 2 - 1:size // 2 + 1]
        assert np.abs(centre - (dist - r)).max() <= voxel
        # the silhouette is the tangent cone: a circle of radius r f (H / 2) / sqrt(dist^2 - r^2) pixels; pixel centres inside a circle
        # of radius R number pi R^2 up to the one-pixel rim 2 pi R, and the chords of a mesh with edges <= sqrt(3) voxel stay within the
        # sagitta 3 voxel^2 / (8 r) of the sphere
        f = 1 / math.tan(math.radians(18.0) / 2)
        R = r * f * (size / 2) / math.sqrt(dist ** 2 - r ** 2)
        sag = 3 * voxel ** 2 / (8 * r) * f * (size / 2) / dist
        count = int((out['triangle'][0] >= 0).sum())
        assert abs(count - math.pi * R ** 2) <= 2 * math.pi * R * (1 + sag), (count, math.pi * R ** 2)
        if normals is not None:          # the centre faces the light: n . l = 1 up to the tilt of a normal half a pixel off the axis
            assert np.abs(out['image'][0, :, size // 2 - 1:size // 2 + 1, size // 2 - 1:size // 2 + 1] - (mr.AMBIENT + mr.DIFFUSE)).max() <= 1e-3


def test_depth_and_shading_follow_the_float64_definition():
    """Every foreground pixel of the sphere (vertex normals, colours, labels) and of the pair (flat normals) against shade64 / depth64
    on the same snapped integers, within the per-pixel bound derived in tests/raster_ref.py."""
    v, t, n, _, size = sphere_case(32)
    cam = rr.head_on_camera(2.7, shift=(0.0137, -0.0071))
    rng = np.random.default_rng(0)
    colors, labels = rng.integers(0, 256, size=[v.shape[0], 3]).astype(np.uint8), rng.integers(0, 19, size=v.shape[0]).astype(np.int32)
    rec = host_records(v, cam=cam, size=size, fov=18.0)[0]
    for kw in (dict(normals=n, colors=colors, labels=labels), dict(normals=n), dict(colors=colors), dict(base_color=(0.9, 0.5, 0.2))):
        out = host_render(v, t, cam=cam, size=size, fov=18.0, validate=False, **kw)
        worst = rr.check_shading({k: a[0] for k, a in out.items()}, rec, v, t, mr.camera_matrices(cam)[1][0], **kw)
        print(f'{sorted(kw)}: worst error / bound {worst:.3f}')


# ---- cameras and files ------------------------------------------------------------------------------------------------------------

def test_turntable_cameras_match_the_formula():
    """render_mesh.py:45-46, 52-53 restated in float64; 1e-6 is the bound of the pose helpers' own device test (tests/test_gpu_ops.py)."""
    num = 12
    cams = mr.turntable_cameras(num).double().numpy()
    assert cams.shape == (num, 4, 4)
    for i in range(num):
        yaw = math.pi * (0.5 + 0.15 * math.cos(2 * math.pi * i / num))
        pitch = math.pi * (0.5 - 0.05 * math.sin(2 * math.pi * i / num))
        pos = 2.7 * np.array([math.sin(pitch) * math.cos(yaw), math.cos(pitch), math.sin(pitch) * math.sin(yaw)])
        fwd = -pos / np.linalg.norm(pos)
        left = np.cross([0.0, 1.0, 0.0], fwd); left /= np.linalg.norm(left)
        up = np.cross(fwd, left); up /= np.linalg.norm(up)
        want = np.eye(4)
        want[:3, 0], want[:3, 1], want[:3, 2], want[:3, 3] = -left, up, -fwd, pos
        assert np.abs(cams[i] - want).max() <= 1e-6, i
    # the origin projects to the image centre for every one of them
    rec = mr.project_vertices(torch.zeros(1, 3), torch.from_numpy(cams), size=64).numpy()
    assert (np.abs(rec[:, 0, :2] - 64 * 128) <= 1).all() and (rec[:, 0, 3] == 0).all()


def test_mesh_from_cube_file_round_trip(tmp_path):
    from training import mesh_extraction as me
    g = np.mgrid[0:16, 0:16, 0:16].astype(np.float32)
    cube = 40 - 8 * np.sqrt(((g - 7.5) ** 2).sum(0))            # negative outside: np.maximum(cube, 0) must not move the 10.0 surface
    path = os.path.join(tmp_path, 'cube.npy')
    np.save(path, cube)
    mesh = mr.mesh_from_cube_file(path, threshold=10.0, normals=True)
    hv, ht, hn = me.marching_cubes_host(np.maximum(cube, 0), 10.0, normals=True)
    assert ht.shape[0] > 0 and np.array_equal(mesh['triangles'].numpy(), ht)
    assert np.abs(mesh['vertices'].numpy() - (hv / 16 - 0.5)).max() <= 1e-6 and np.allclose(mesh['normals'].numpy(), hn, atol=1e-6)
    radius = np.linalg.norm(mesh['vertices'].numpy() - (7.5 / 16 - 0.5), axis=1)
    assert np.abs(radius - 3.75 / 16).max() <= 0.5 / 16


def test_turntable_frames_through_y4m(tmp_path):
    from training import video_render
    v, t, n = rr.sphere_mesh()
    mesh = {'vertices': torch.from_numpy(v), 'triangles': torch.from_numpy(t), 'normals': torch.from_numpy(n)}
    frames = list(mr.render_turntable(mesh, num_frames=5, size=(24, 40), chunk=2))
    assert len(frames) == 5 and all(f.shape == (24, 40, 3) and f.dtype == torch.uint8 for f in frames)
    assert all((f == 255).any() and (f < 255).any() for f in frames)
    path = os.path.join(tmp_path, 'render.y4m')
    assert video_render.write_y4m(iter(frames), path) == 5
    info, data = video_render.read_y4m(path)
    assert data.shape == (5, 3, 24, 40) and info['W'] == '40' and info['H'] == '24'
    assert np.array_equal(data[3], video_render.rgb_u8_to_yuv444(frames[3]).numpy())


# ---- C ABI ------------------------------------------------------------------------------------------------------------------------

def test_c_abi():
    from torch_utils import hip_plugin
    with open(os.path.join(ROOT, 'include', 'ide3d_hip.h')) as f:
        h = f.read()
    decl = {
        'ide3d_raster_workspace_bytes': 'int32_t N, int64_t V, int32_t H, int32_t W',
        'ide3d_raster_project': 'const float* vertices, int64_t V, const float* world2cam, int32_t N, int32_t H, int32_t W, float fx, float fy, '
                                'float sx, float ox, float sy, float oy, float near, void* workspace, int64_t workspace_bytes, void* stream',
        'ide3d_raster_depth': 'const int32_t* triangles, int64_t T, int64_t V, int32_t N, int32_t H, int32_t W, int32_t cull, '
                              'int32_t large_min, void* workspace, int64_t workspace_bytes, void* stream',
        'ide3d_raster_shade': 'const float* vertices, const int32_t* triangles, int64_t V, int32_t N, int32_t H, int32_t W, '
                              'const float* normals, const uint8_t* colors, const int32_t* labels, const float* light, int32_t two_sided, '
                              'float ambient, float diffuse, const float* base_color, float bg, const void* workspace, int64_t workspace_bytes, '
                              'float* depth, int32_t* triangle, float* image, int32_t* label, void* stream',
    }
    ctype = {'int32_t': ctypes.c_int32, 'int64_t': ctypes.c_int64, 'float': ctypes.c_float}
    assert 'render_mesh.py:36-61' in h and 'render_mesh.py:48-56' in h and 'render_mesh.py:57' in h
    path = hip_plugin.lib_path()
    assert os.path.isfile(path), f'{path} missing: run __graft_entry__.build()'
    lib, loaded = ctypes.CDLL(path), hip_plugin.load()
    for name, args in decl.items():
        m = re.search(r'(int64_t|int) %s\(([^)]*)\);' % name, h)
        assert m and re.sub(r'\s+', ' ', m.group(2)) == args, name
        assert name in hip_plugin.EXPORTED_SYMBOLS and hasattr(lib, name), name
        argtypes = getattr(loaded, name).argtypes
        assert len(argtypes) == len(args.split(','))
        for a, got in zip(args.split(','), argtypes):          # scalars by type, every pointer as a pointer
            kind = a.strip().rsplit(' ', 1)[0]
            assert (got is ctype[kind]) if kind in ctype else (got is ctypes.c_void_p or issubclass(got, ctypes._Pointer)), (name, a)
    assert hip_plugin._ABI_VERSION == 8 and lib.ide3d_abi_version() == 8
    assert hip_plugin.PLUGINS['raster_plugin'] is hip_plugin.RasterPlugin
    q = loaded.ide3d_raster_workspace_bytes          # host arithmetic: status word, 16 bytes per camera and vertex, 8 per camera and pixel
    assert q(1, 0, 1, 1) == 16 + 8 and q(8, 100000, 512, 512) == 16 + 8 * 100000 * 16 + 8 * 512 * 512 * 8
    assert q(3, 7, 24, 40) == 16 + 3 * 7 * 16 + 3 * 24 * 40 * 8
    for bad in ((0, 1, 4, 4), (1, -1, 4, 4), (1, 1, 0, 4), (1, 1, 4, 16385), (65536, 1, 4, 4), (1, 2 ** 31, 4, 4)):
        assert q(*bad) == -1
