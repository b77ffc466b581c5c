"""csrc/raster.hip on the GPU: the projection bit for bit against the host definition and within its derived error of float64, the
triangle map against the host definition and against the Python-int coverage / float64 depth of tests/raster_ref.py, the lane and
wave paths, many workgroups under contention, order independence, shading, and generator -> mesh -> image."""
import numpy as np
import pytest
import torch

import raster_ref as rr
from training import mesh_render as mr

pytestmark = pytest.mark.gpu

CAM = rr.head_on_camera(4.0)
KEYS = ('depth', 'triangle', 'image', 'label')


def _quads():
    return [dict(v=v, t=t) for v, t, _ in (rr.split_quad(ox, oy) for ox, oy in rr.offsets64())]


def _fans():
    return [dict(v=v, t=t) for v, t, _ in (rr.closed_fan(ox, oy) for ox, oy in rr.offsets64())]


def _pair():
    v, t = rr.interpenetrating_pair()
    return [dict(v=v, t=t, size=32)]


def _duplicate():
    v, t, _ = rr.split_quad(0.25, 0.625)
    return [dict(v=v, t=np.concatenate([t, t, t[::-1]]), exact_ties=True)]


def _sphere():
    v, t, n = rr.sphere_mesh()
    return [dict(v=v, t=t, normals=n, cam=rr.head_on_camera(2.7, shift=(0.0137, -0.0071)), size=64, fov=18.0)]


def _three_cameras():
    v, t = rr.interpenetrating_pair()
    cam = np.concatenate([rr.head_on_camera(4.0), rr.looking_away_camera(4.0), rr.head_on_camera(4.5, shift=(0.3, -0.2))])
    return [dict(v=v, t=t, cam=cam, size=32, all_background=1)]


def _empty():
    v, _ = rr.interpenetrating_pair()
    return [dict(v=v, t=np.zeros([0, 3], dtype=np.int32), size=32)]


def _nonsquare():
    v, t = rr.interpenetrating_pair()
    return [dict(v=v * np.float32(0.7), t=t, size=(24, 40))]


def _align_corners():
    v, t = rr.interpenetrating_pair()
    return [dict(v=v, t=t, size=32, align_corners=True)]


def _cull():
    v, t, _ = rr.split_quad(0.375, 0.125)
    return [dict(v=v, t=np.concatenate([t, t[:, ::-1] + 0]), cull=cull) for cull in ('none', 'back', 'front')]


GROUPS = {'quad64': _quads, 'fan64': _fans, 'pair': _pair, 'duplicate': _duplicate, 'sphere': _sphere, 'three_cameras': _three_cameras,
          'empty': _empty, 'nonsquare': _nonsquare, 'align_corners': _align_corners, 'cull': _cull}
_cache = {}


def group(name):
    """The cases of a group with the host definition's outputs and records: computed once, never modified."""
    if name not in _cache:
        cases = GROUPS[name]()
        for case in cases:
            case.setdefault('cam', CAM); case.setdefault('size', 16); case.setdefault('fov', rr.FOV_EXACT)
            case['labels'] = (np.arange(case['v'].shape[0]) * 7 % 19).astype(np.int32)
            case['host'] = render(case, None)
            case['host_records'] = records(case, None)
        _cache[name] = cases
    return _cache[name]


def _render_kw(case):
    return {k: case[k] for k in ('size', 'fov', 'cull', 'align_corners') if k in case}


def _t(a, dev):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev if dev is not None else 'cpu')


def render(case, dev, large_min=None, triangles=None):
    out = mr.render_mesh(_t(case['v'], dev), _t(case['t'] if triangles is None else triangles, dev), torch.from_numpy(case['cam']),
                         normals=_t(case.get('normals'), dev), labels=_t(case['labels'], dev), validate=False, large_min=large_min, **_render_kw(case))
    return {k: a.cpu().numpy() for k, a in out.items()}


def records(case, dev):
    kw = {k: v for k, v in _render_kw(case).items() if k != 'cull'}
    return mr.project_vertices(_t(case['v'], dev), torch.from_numpy(case['cam']), **kw).cpu().numpy()


def _calls(what):
    from torch_utils import hip_plugin
    return hip_plugin.CALLS.get(what, 0)


def assert_same(a, b, what=''):
    for k in KEYS:
        assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and np.array_equal(a[k], b[k]), f'{what}: {k} differs'


# ---- 1. projection ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('name', sorted(GROUPS))
def test_projection_bit_for_bit_and_within_float32_of_float64(name, gpu_device):
    """float32 against float64, u = 2^-24.  Camera space: world2cam is the float64 inverse rounded once (u per entry), each row is three
    products and three sums of float32 values: |delta| <= 7u S with S = sum |m_k| |p_k| + |t| (first order).  Pixel coordinate
    px = ((fx x) / d) sx + ox: fx, the product, the quotient, the scale and the sum round once each and ox is exact: 6u (|px - ox| + |ox|)
    at most, and the camera-space errors arrive as (sx fx / d) (delta_x + |x| / d delta_z).  The snap adds half a unit of 1/256 pixel;
    the bound is one unit plus 256 times the above."""
    u = 2.0 ** -24
    for case in group(name):
        before = _calls('raster_project')
        rec = records(case, gpu_device)
        assert _calls('raster_project') == before + 1
        assert rec.dtype == np.int32 and np.array_equal(rec, case['host_records'])
        H, W = mr._size(case['size'])
        align = case.get('align_corners', False)
        px, py, d = rr.project64(case['v'], case['cam'], H, W, case['fov'], align)
        fx, fy, sx, ox, sy, oy = (float(a) for a in mr.view_constants(H, W, case['fov'], align))
        v64 = np.abs(case['v'].astype(np.float64))
        for n in range(rec.shape[0]):
            m = np.linalg.inv(case['cam'][n])
            S = np.abs(m[:3, :3]) @ v64.T + np.abs(m[:3, 3:4])                                      # [3, V]
            ok = rec[n, :, 3] == 0
            assert (ok == (d[n] >= 0.05)).all(), 'no test vertex is near the near plane or the guard band'
            for got, want, f, s, o, row in ((rec[n, :, 0], px[n], fx, sx, ox, 0), (rec[n, :, 1], py[n], fy, sy, oy, 1)):
                cam = np.abs(want - o) / (s * f) * d[n]                                             # |x_cam| back from the pixel coordinate
                err = s * f / d[n] * (7 * u * S[row] + cam / d[n] * 7 * u * S[2]) + 6 * u * (np.abs(want - o) + o)
                assert (np.abs(got - 256 * want) <= 1 + 256 * err)[ok].all()
            assert np.abs(rr.record_depths(rec[n]) - d[n]).max() <= 7 * u * S[2].max()


# ---- 2. the triangle map ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('name', sorted(GROUPS))
def test_triangle_map(name, gpu_device):
    """Equal to the host definition exactly, and, on the GPU's own snapped coordinates, the covering triangle of least float64 depth
    (rr.check_triangle_map; near ties within twice the float32 depth bound for at most 1 % of the covered pixels)."""
    for case in group(name):
        before = [_calls(k) for k in ('raster_project', 'raster_depth', 'raster_shade')]
        got = render(case, gpu_device)
        assert [_calls(k) for k in ('raster_project', 'raster_depth', 'raster_shade')] == [b + 1 for b in before]
        assert_same(got, case['host'], name)
        rec = records(case, gpu_device)
        H, W = mr._size(case['size'])
        for n in range(rec.shape[0]):
            covered, used = rr.check_triangle_map(got['triangle'][n], rec[n], case['t'], H, W, case.get('cull', 'none'))
            assert used <= 0.01 * covered
            assert (covered == 0) == (name == 'empty' or n == case.get('all_background'))
            assert ((got['triangle'][n] >= 0).sum() == covered) and (np.isinf(got['depth'][n, 0]) == (got['triangle'][n] < 0)).all()
        if 'cull' in case:
            front = [float(np.cross(case['v'][b] - case['v'][a], case['v'][c] - case['v'][a])[2]) > 0 for a, b, c in case['t']]
            drawn = set(np.unique(got['triangle'])) - {-1}
            want = {'none': {0, 1}, 'back': {i for i in range(4) if front[i]}, 'front': {i for i in range(4) if not front[i]}}[case['cull']]
            assert drawn == want and len(want) == 2
        if case.get('exact_ties'):
            assert set(np.unique(got['triangle'])) == {-1, 0, 1}, 'equal depths go to the lower index'


# ---- 3. lane path and wave path -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('name', sorted(GROUPS))
def test_lane_and_wave_paths_agree(name, gpu_device):
    for case in group(name):
        for large_min in (0, 2 ** 31 - 1):
            assert_same(render(case, gpu_device, large_min=large_min), case['host'], f'{name} large_min={large_min}')


def test_screen_filling_triangle_over_tiny_ones(gpu_device):
    """256^2, one triangle that covers the screen (in the middle of their depth range, so it wins some pixels and loses others) over 2,000 tiny ones, at the
    library's default threshold: the large one goes to its wave, the rest stay in their lanes."""
    H = W = 256
    v, t = rr.tiny_triangles(2000, H, W, seed=3)
    big = np.array([rr.screen_to_world(px, py, d, H, W) for px, py, d in ((-40.0, -30.0, 1.5), (600.0, -20.0, 2.5), (-30.0, 590.0, 1.8))], dtype=np.float32)
    case = dict(v=np.concatenate([v, big]), t=np.concatenate([t[:1000], [[6000, 6001, 6002]], t[1000:]]).astype(np.int32), cam=CAM, size=H,
                fov=rr.FOV_EXACT, labels=np.zeros(6003, dtype=np.int32))
    host = render(case, None)
    assert (host['triangle'] >= 0).all() and (host['triangle'] == 1000).mean() > 0.5 and (host['triangle'] != 1000).sum() > 500
    for large_min in (None, 0, 2 ** 31 - 1):
        assert_same(render(case, gpu_device, large_min=large_min), host, f'large_min={large_min}')


# ---- 4. many workgroups -------------------------------------------------------------------------------------------------------------

def test_many_workgroups_under_contention(gpu_device):
    """70,000 triangles of 1-3 pixels on 32^2: 274 workgroups with a ragged last one (70,000 = 273 * 256 + 112), about 100 atomics per pixel."""
    v, t = rr.tiny_triangles(70000, 32, 32, seed=4)
    case = dict(v=v, t=t, cam=CAM, size=32, fov=rr.FOV_EXACT, labels=(np.arange(v.shape[0]) % 5).astype(np.int32))
    host = render(case, None)
    assert (host['triangle'] >= 0).mean() > 0.95 and host['triangle'].max() > 69000
    assert_same(render(case, gpu_device), host)


# ---- 5. order independence ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('name', ['pair', 'duplicate', 'sphere', 'three_cameras'])
def test_order_independence(name, gpu_device):
    for case in group(name):
        a = render(case, gpu_device)
        assert_same(render(case, gpu_device), a, 'second run on cloned inputs')
        perm = np.random.default_rng(5).permutation(case['t'].shape[0])
        b = render(case, gpu_device, triangles=case['t'][perm])
        assert np.array_equal(a['depth'], b['depth']) and np.array_equal(a['image'], b['image']) and np.array_equal(a['label'], b['label'])
        back = np.where(b['triangle'] >= 0, perm[np.maximum(b['triangle'], 0)], -1)
        if case.get('exact_ties'):          # the copies of a triangle have the same depth everywhere: whichever comes first in the list wins
            same = (case['t'][np.maximum(back, 0)] == case['t'][np.maximum(a['triangle'], 0)]).all(axis=-1)
            assert ((back >= 0) == (a['triangle'] >= 0)).all() and same[a['triangle'] >= 0].all()
        else:
            assert np.array_equal(back, a['triangle'])


# ---- 6. shading ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('smooth', [True, False])
@pytest.mark.parametrize('colored', [True, False])
def test_shading_against_float64(smooth, colored, gpu_device):
    """image and depth against shade64 / depth64 on the GPU's own snapped integers, per-pixel bound derived in tests/raster_ref.py from
    the operation count (worst error / bound measured: DESIGN.md section 5.26); labels exactly (no barycentric tie in the inputs:
    checked in float64 by check_shading)."""
    v, t, n = rr.sphere_mesh()
    rng = np.random.default_rng(6)
    cam = np.concatenate([rr.head_on_camera(2.7, shift=(0.0137, -0.0071)), rr.head_on_camera(2.2, shift=(-0.21, 0.13))])
    kw = dict(base_color=(0.9, 0.5, 0.2), ambient=0.25, diffuse=0.6)
    if smooth:
        kw['normals'] = n
    if colored:
        kw['colors'] = rng.integers(0, 256, size=[v.shape[0], 3]).astype(np.uint8)
    kw['labels'] = rng.integers(0, 19, size=v.shape[0]).astype(np.int32)
    dev_kw = {k: (_t(a, gpu_device) if isinstance(a, np.ndarray) else a) for k, a in kw.items()}
    out = mr.render_mesh(_t(v, gpu_device), _t(t, gpu_device), torch.from_numpy(cam), size=32, validate=False, **dev_kw)
    out = {k: a.cpu().numpy() for k, a in out.items()}
    rec = mr.project_vertices(_t(v, gpu_device), torch.from_numpy(cam), size=32).cpu().numpy()
    light = mr.camera_matrices(cam)[1]
    worst = max(rr.check_shading({k: a[i] for k, a in out.items()}, rec[i], v, t, light[i], **kw) for i in range(2))
    print(f'smooth={smooth} colored={colored}: worst image error / bound {worst:.3f}')
    assert (out['triangle'] >= 0).sum() > 300


# ---- 7. generator -> mesh -> image --------------------------------------------------------------------------------------------------

@pytest.fixture(scope='module')
def tiny_generator(gpu_device):
    from training import triplane
    torch.manual_seed(0)
    G = triplane.TriPlaneGenerator(triplane.tiny_spec()).eval().to(gpu_device)
    z = torch.from_numpy(np.random.RandomState(0).randn(1, G.z_dim)).float().to(gpu_device)
    return G, z, triplane.conditioning_label(gpu_device)


def test_extracted_mesh_renders(tiny_generator, gpu_device):
    from training import mesh_extraction as me, shape_extraction as se
    G, z, c = tiny_generator
    with torch.no_grad():
        ws = G.mapping(z, c, truncation_psi=0.5)
        img_v, seg_v = se.triplanes_from_ws(G.synthesis, ws, noise_mode='const')
        cube = se.density_cube(G.synthesis.renderer, img_v, seg_v, voxel_resolution=32, max_batch=None)[0]
    mesh = me.extract_mesh(G, ws, voxel_resolution=32, threshold=float(cube.median()), normals=True, vertex_attributes=True)
    cams = mr.turntable_cameras(2, device=gpu_device)
    kw = dict(size=64, validate=False)
    out = mr.render_mesh(mesh['vertices'], mesh['triangles'], cams, normals=mesh['normals'], colors=mesh['colors'], labels=mesh['labels'], **kw)
    assert all(a.is_cuda for a in out.values()) and out['image'].shape == (2, 3, 64, 64) and out['label'].dtype == torch.int32
    fg = out['triangle'] >= 0
    assert fg.any() and torch.isfinite(out['image']).all() and torch.isfinite(out['depth'][:, 0][fg]).all()
    assert int(out['label'][fg].min()) >= 0 and (out['label'][~fg] == -1).all()
    host = mr.render_mesh(mesh['vertices'].cpu(), mesh['triangles'].cpu(), cams.cpu(), normals=mesh['normals'].cpu(), colors=mesh['colors'].cpu(),
                          labels=mesh['labels'].cpu(), **kw)
    assert_same({k: a.cpu().numpy() for k, a in out.items()}, {k: a.numpy() for k, a in host.items()})
    frames = list(mr.render_turntable(mesh, num_frames=3, size=32, chunk=2))
    assert len(frames) == 3 and frames[0].shape == (32, 32, 3) and frames[0].dtype == torch.uint8 and frames[0].is_cuda
