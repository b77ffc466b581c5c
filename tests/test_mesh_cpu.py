"""Marching cubes without a GPU: the generated case table (exhaustive combinatorial properties), the host definition of
training/mesh_extraction.py against the plain-loop float64 restatement of tests/mesh_ref.py, topology and closed forms on three
volumes, edge cases, the PLY files, the `mcubes` overlay and the C ABI."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import mesh_ref as mr
from training import mesh_extraction as me

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VOLUMES = {'sphere': (mr.sphere_volume, 2), 'torus': (mr.torus_volume, 0), 'noise': (mr.noise_volume, -26)}
_cache = {}


def case(name):
    """(volume float64, reference vertices, reference triangles, public CPU result), computed once and never modified."""
    if name not in _cache:
        vol = VOLUMES[name][0]()
        vr, tr = mr.reference_mesh(vol, 0.0, me.case_table(), me.EDGES)
        v, t, n = me.marching_cubes(torch.from_numpy(vol), 0.0, normals=True)
        _cache[name] = (vol, vr, tr, v.numpy(), t.numpy(), n.numpy())
    return _cache[name]


# ---- the table -----------------------------------------------------------------------------------------------------------------

def test_table_counts():
    table = me.case_table()
    assert len(table) == 256 and table[0] == () and table[255] == ()
    assert max(len(t) for t in table) == 5 and sum(len(t) for t in table) == 820
    assert me.EDGES == ((0, 1), (0, 2), (0, 4), (1, 3), (1, 5), (2, 3), (2, 6), (3, 7), (4, 5), (4, 6), (5, 7), (6, 7))
    assert me.EDGE_AXIS == (0, 1, 2, 1, 2, 0, 2, 2, 0, 1, 1, 0)
    packed = me.case_table_bytes()
    assert packed.shape == (256, 16) and packed.dtype == np.uint8
    for c, tris in enumerate(table):
        assert packed[c, 0] == len(tris) and packed[c, 1:1 + 3 * len(tris)].tolist() == [e for t in tris for e in t]
        assert not packed[c, 1 + 3 * len(tris):].any()


def test_table_uses_exactly_the_sign_changing_edges():
    table = me.case_table()
    for c in range(256):
        crossing = {e for e, (a, b) in enumerate(me.EDGES) if ((c >> a) & 1) != ((c >> b) & 1)}
        assert {e for t in table[c] for e in t} == crossing, c
        assert {e for t in table[255 - c] for e in t} == crossing, c


def _boundary(tris):
    """Directed edges of a triangle list that no reversed edge cancels."""
    he = [(t[k], t[(k + 1) % 3]) for t in tris for k in range(3)]
    assert len(set(he)) == len(he)
    return {h for h in he if (h[1], h[0]) not in he}


def test_table_is_crack_free():
    """The triangles of a case leave exactly the face segments open, and on every face those segments are the reverse of what
    EVERY neighbour case with the same corner signs on the shared face draws there."""
    table, faces = me.case_table(), me.cell_faces()
    for c in range(256):
        segs = [set(me.face_segments(c, f)) for f in faces]
        assert _boundary(table[c]) == set().union(*segs), c
        for fi, face in enumerate(faces):
            axis, bit = fi // 2, 1 << (fi // 2)
            other = faces[fi ^ 1]                                    # the neighbour's face that coincides with this one
            assert {k ^ bit for k in face} == set(other)
            fixed = sum(((c >> k) & 1) << (k ^ bit) for k in face)
            free = [k for k in range(8) if k not in other]
            for m in range(16):
                nc = fixed | sum(((m >> i) & 1) << k for i, k in enumerate(free))
                theirs = set()
                for a, b in me.face_segments(nc, other):
                    ea, eb = (tuple(sorted(k ^ bit for k in me.EDGES[e])) for e in (a, b))
                    theirs.add((me.EDGES.index(eb), me.EDGES.index(ea)))          # mapped into this cell's edge ids and reversed
                assert theirs == segs[fi], (c, fi, nc)


# ---- host definition against the loop reference --------------------------------------------------------------------------------

@pytest.mark.parametrize('name', sorted(VOLUMES))
def test_cpu_matches_reference(name):
    vol, vr, tr, v, t, _ = case(name)
    assert v.dtype == np.float32 and t.dtype == np.int32 and v.shape == (vr.shape[0], 3) and t.shape == tr.shape
    # float64 arithmetic, rounded once to float32 at coordinates below 32: half an ulp = 2^-20 = 9.6e-7
    idx = mr.match_vertices(vr, v, 1e-6)
    assert mr.triangle_keys(vr[idx], t) == mr.triangle_keys(vr, tr)
    # the documented order: by owning point, x before y before z; triangles by cell, then table order (the reference's loop order)
    v32, t32, _ = me.marching_cubes_host(vol.astype(np.float32), 0.0)
    assert np.array_equal(t32, t) and np.abs(v32.astype(np.float64) - v).max() <= 2e-6


@pytest.mark.parametrize('name', sorted(VOLUMES))
def test_topology(name):
    vol, vr, tr, v, t, _ = case(name)
    assert mr.is_closed(tr) and mr.is_closed(t)
    chi = mr.euler(vr.shape[0], tr)
    assert chi == VOLUMES[name][1] and mr.euler(v.shape[0], t) == chi
    assert mr.signed_volume(vr, tr) > 0 and mr.signed_volume(v, t) > 0
    vf, tf = me.marching_cubes(torch.from_numpy(vol), 0.0, flip=True)
    assert torch.equal(vf, torch.from_numpy(v)) and mr.is_closed(tf.numpy()) and mr.signed_volume(vf.numpy(), tf.numpy()) < 0


def test_sphere_closed_forms():
    _, vr, tr, v, t, n = case('sphere')
    for verts, tris in ((vr, tr), (v.astype(np.float64), t)):
        r = np.linalg.norm(verts - mr.SPHERE_CENTRE, axis=1)
        print('max | |v - c| - 9 | =', np.abs(r - 9).max(), ' volume / (4/3 pi 9^3) - 1 =', mr.signed_volume(verts, tris) / (4 / 3 * np.pi * 729) - 1)
        assert np.abs(r - 9).max() <= 0.02
        assert abs(mr.signed_volume(verts, tris) / (4 / 3 * np.pi * 729) - 1) <= 0.015
    radial = (v - mr.SPHERE_CENTRE) / np.linalg.norm(v - mr.SPHERE_CENTRE, axis=1, keepdims=True)
    angle = np.degrees(np.arccos(np.clip((radial * n).sum(axis=1), -1, 1)))
    print('normals vs radial: 99th percentile', np.percentile(angle, 99), 'deg, max', angle.max(), 'deg')
    assert (angle <= 3).mean() >= 0.99
    assert np.abs(np.linalg.norm(n, axis=1) - 1).max() <= 1e-6


# ---- edges ---------------------------------------------------------------------------------------------------------------------

def test_empty_volumes():
    for fill in (-1.0, 1.0):
        out = me.marching_cubes(torch.full([6, 7, 8], fill), 0.0, normals=True)
        assert [tuple(o.shape) for o in out] == [(0, 3), (0, 3), (0, 3)]
        assert out[0].dtype == torch.float32 and out[1].dtype == torch.int32


def test_value_equal_to_threshold_is_outside():
    vol = torch.full([5, 5, 5], -1.0)
    vol[2, 2, 2] = 0.0
    v, t = me.marching_cubes(vol, 0.0)
    assert v.shape[0] == 0 and t.shape[0] == 0
    vol = torch.zeros([5, 5, 5])                    # everything at the threshold (outside) around one inside point
    vol[2, 2, 2] = 1.0
    v, t = me.marching_cubes(vol, 0.0)
    assert v.shape[0] == 6 and t.shape[0] == 8 and mr.is_closed(t.numpy()) and mr.euler(6, t.numpy()) == 2
    assert sorted(map(tuple, v.tolist())) == sorted([(1, 2, 2), (3, 2, 2), (2, 1, 2), (2, 3, 2), (2, 2, 1), (2, 2, 3)])
    # many corners exactly at the threshold: still closed, zero-area triangles allowed
    vol = np.round(mr.sphere_volume(14, 4.0, (0, 0, 0)) * 2) / 2
    assert (vol == 0).sum() > 50
    v, t = me.marching_cubes(torch.from_numpy(vol), 0.0)
    vr, tr = mr.reference_mesh(vol, 0.0, me.case_table(), me.EDGES)
    assert mr.is_closed(t.numpy()) and t.shape == tr.shape and mr.signed_volume(v.numpy(), t.numpy()) > 0
    mr.match_vertices(vr, v.numpy(), 1e-6)


def test_non_cubic_grid():
    vol = mr.noise_volume((5, 9, 17), seed=1, border=None)
    vr, tr = mr.reference_mesh(vol, 0.1, me.case_table(), me.EDGES)
    v, t = me.marching_cubes(torch.from_numpy(vol), 0.1)
    idx = mr.match_vertices(vr, v.numpy(), 1e-6)
    assert mr.triangle_keys(vr[idx], t.numpy()) == mr.triangle_keys(vr, tr)
    # an axis of one point has no cell: vertices on the crossing edges, no triangle
    v, t = me.marching_cubes(torch.tensor([[[-1.0, 1.0, 3.0, -1.0]]]), 0.0)
    assert t.shape == (0, 3) and v.tolist() == [[0, 0, 0.5], [0, 0, 2.75]]


def test_surface_crossing_the_border_is_open_only_there():
    n = 12
    vol = mr.sphere_volume(n, 5.0, (-4.2, 0.3, 3.9))
    v, t = me.marching_cubes(torch.from_numpy(vol), 0.0)
    v, t = v.numpy(), t.numpy()
    opened = mr.open_half_edges(t)
    assert opened
    for a, b in opened:
        on_border = ((v[a] == 0) & (v[b] == 0)) | ((v[a] == n - 1) & (v[b] == n - 1))
        assert on_border.any(), (v[a], v[b])


def test_lattice_and_normals_of_the_host_definition():
    vol = mr.sphere_volume().astype(np.float32)
    lattice = (2.0 / 23, np.array([-1.0, -1.1, -1.2]), 0.9)
    v, t = me.marching_cubes(torch.from_numpy(vol), 0.0)
    w, t2 = me.marching_cubes(torch.from_numpy(vol), 0.0, lattice=lattice)
    want = 0.9 * (v.double().numpy() * (2.0 / 23) + np.array([-1.2, -1.1, -1.0]))
    assert torch.equal(t, t2) and np.abs(w.numpy() - want).max() <= 1e-6 * np.abs(want).max()
    flat = torch.zeros([4, 4, 4])
    flat[1:3, 1:3, 1:3] = 1.0
    flat[0, 0, 0] = 1.0                      # an isolated corner: the gradient is one-sided there
    _, _, n = me.marching_cubes(flat, 0.5, normals=True)
    assert torch.isfinite(n).all()


# ---- files and interface -------------------------------------------------------------------------------------------------------

def test_ply_round_trip(tmp_path):
    _, _, _, v, t, n = case('sphere')
    rng = np.random.default_rng(3)
    colors = rng.integers(0, 256, size=(v.shape[0], 3), dtype=np.uint8)
    labels = rng.integers(0, 19, size=v.shape[0])
    path = me.save_mesh(str(tmp_path / 'out'), 'head', torch.from_numpy(v), torch.from_numpy(t), normals=n, colors=colors, labels=labels)
    assert path.endswith('head.ply')
    with open(path, 'rb') as f:
        assert f.read(40).startswith(b'ply\nformat binary_little_endian 1.0\n')
    back = me.read_ply(path)
    assert np.array_equal(back['vertices'], v) and np.array_equal(back['triangles'], t) and np.array_equal(back['normals'], n)
    assert np.array_equal(back['colors'], colors) and np.array_equal(back['labels'], labels)
    me.write_ply(str(tmp_path / 'bare.ply'), v, t)
    back = me.read_ply(str(tmp_path / 'bare.ply'))
    assert sorted(back) == ['triangles', 'vertices'] and np.array_equal(back['vertices'], v) and np.array_equal(back['triangles'], t)
    me.write_ply(str(tmp_path / 'empty.ply'), np.zeros([0, 3]), np.zeros([0, 3]))
    assert me.read_ply(str(tmp_path / 'empty.ply'))['triangles'].shape == (0, 3)


def test_mcubes_overlay():
    import mcubes
    assert os.path.dirname(os.path.abspath(mcubes.__file__)) == os.path.join(ROOT, 'ide-3d_amd')
    vol, vr, tr, _, t, _ = case('sphere')
    vertices, triangles = mcubes.marching_cubes(vol.astype(np.float32), 0.0)
    assert isinstance(vertices, np.ndarray) and vertices.dtype == np.float64 and vertices.shape == (vr.shape[0], 3)
    assert isinstance(triangles, np.ndarray) and triangles.dtype == np.int64 and np.array_equal(triangles, t)
    mr.match_vertices(mr.reference_mesh(vol.astype(np.float32), 0.0, me.case_table(), me.EDGES)[0], vertices, 1e-12)
    # what the reference does with the result (dnnlib/geometry.py:290, render_mesh.py:32)
    assert (vertices / (24 - 1.0) * 2.0 - 1.0).astype('float32').shape == vertices.shape


def test_c_abi():
    from torch_utils import hip_plugin
    with open(os.path.join(ROOT, 'include', 'ide3d_hip.h')) as f:
        h = f.read()
    assert re.search(r'int64_t ide3d_mesh_workspace_bytes\(int32_t X, int32_t Y, int32_t Z\);', h)
    assert re.search(r'int ide3d_mesh_count\(const float\* volume, int32_t X, int32_t Y, int32_t Z, float iso, const uint8_t\* table,\s*'
                     r'void\* workspace, int64_t workspace_bytes, void\* stream\);', h)
    assert re.search(r'int ide3d_mesh_emit\(const float\* volume, int32_t X, int32_t Y, int32_t Z, float iso, const uint8_t\* table,\s*'
                     r'const ide3d_lattice\* lat, int32_t flip, void\* workspace, int64_t workspace_bytes,\s*int64_t num_vertices, '
                     r'int64_t num_triangles, float\* vertices, int32_t\* triangles, float\* normals, void\* stream\);', h)
    assert 'render_mesh.py:31' in h and 'dnnlib/geometry.py:286' in h
    path = hip_plugin.lib_path()
    assert os.path.isfile(path), f'{path} missing: run __graft_entry__.build()'
    lib, loaded = ctypes.CDLL(path), hip_plugin.load()
    for name in ('ide3d_mesh_workspace_bytes', 'ide3d_mesh_count', 'ide3d_mesh_emit'):
        assert name in hip_plugin.EXPORTED_SYMBOLS and hasattr(lib, name), name
        m = re.search(r'(int64_t|int) %s\(([^)]*)\);' % name, h)
        assert len(getattr(loaded, name).argtypes) == len(m.group(2).split(',')), name
    assert hip_plugin._ABI_VERSION == 8 and lib.ide3d_abi_version() == 8
    assert hip_plugin.PLUGINS['mesh_plugin'] is hip_plugin.MeshPlugin
    # host arithmetic only: 16 bytes of totals, one 8-byte pair per 1024 points rounded up to 16 bytes, 4 bytes per point
    q = loaded.ide3d_mesh_workspace_bytes
    assert q(256, 256, 256) == 16 + 16384 * 8 + 4 * 256 ** 3
    assert q(5, 9, 17) == 16 + 16 + 4 * 765
    assert q(33, 18, 7) == 16 + 48 + 4 * 4158
    assert q(1024, 1024, 1024) == 16 + (1 << 20) * 8 + 4 * (1 << 30)
    assert q(1, 1, 1) == 16 + 16 + 4
    for bad in ((0, 4, 4), (4, -1, 4), (1025, 4, 4), (4, 4, 1025)):
        assert q(*bad) == -1


def test_extract_mesh_on_the_host():
    """Generator -> cube -> mesh with the host definition: world coordinates of the cube's lattice, attributes from one
    `sample_voxel` call at the vertices."""
    from training import shape_extraction as se, triplane
    torch.manual_seed(0)
    G = triplane.TriPlaneGenerator(triplane.tiny_spec()).eval()
    z, c, N = torch.from_numpy(np.random.RandomState(0).randn(1, G.z_dim)).float(), triplane.conditioning_label(), 10
    with torch.no_grad():
        ws = G.mapping(z, c, truncation_psi=0.5)
        img_v, seg_v = se.triplanes_from_ws(G.synthesis, ws, noise_mode='const')
        cube = se.density_cube(G.synthesis.renderer, img_v, seg_v, voxel_resolution=N, max_batch=None)[0]
    threshold = float(cube.median())
    out = me.extract_mesh(G, z, c, voxel_resolution=N, threshold=threshold, vertex_attributes=True)
    v, t = me.marching_cubes(cube, threshold)
    assert t.shape[0] > 0 and torch.equal(out['triangles'], t)
    want = 0.9 * (v.double() * (2.0 / (N - 1)) - 1.0)
    assert (out['vertices'].double() - want).abs().max() <= 1e-6
    spec = G.synthesis.renderer.spec
    assert out['labels'].shape == (v.shape[0],) and 0 <= int(out['labels'].min()) and int(out['labels'].max()) < spec.seg_channels
    assert out['colors'].shape == (v.shape[0], 3) and out['colors'].dtype == torch.uint8
    with torch.no_grad():
        feat = G.synthesis.renderer.sample_voxel(img_v, seg_v, out['vertices'].unsqueeze(0))
    assert torch.equal(out['labels'], feat[:, spec.feature_channels:spec.feature_channels + spec.seg_channels].argmax(dim=1))
