"""csrc/mesh.hip on the GPU: marching cubes against the plain-loop float64 restatement of tests/mesh_ref.py, determinism, the
compaction across many workgroups, `lattice=`, normals, and generator -> mesh."""
import numpy as np
import pytest
import torch

import mesh_ref as mr
from training import mesh_extraction as me

pytestmark = pytest.mark.gpu

# (volume builder, threshold); [33, 18, 7]: no axis is a multiple of anything the kernels tile by, 4158 points = 4 full workgroup
# chunks of 1024 and a ragged fifth, and the last layer of points in every axis owns crossing edges
VOLUMES = {
    'sphere': (mr.sphere_volume, 0.0),
    'torus': (mr.torus_volume, 0.0),
    'noise': (mr.noise_volume, 0.0),
    'odd_5x9x17': (lambda: mr.noise_volume((5, 9, 17), seed=1, border=None), 0.1),
    'ragged_33x18x7': (lambda: mr.noise_volume((33, 18, 7), seed=2, border=None), -0.2),
}
_cache = {}


def case(name):
    """(float32 volume as numpy, threshold, reference vertices, reference triangles): computed once, never modified."""
    if name not in _cache:
        build, iso = VOLUMES[name]
        vol = build().astype(np.float32)
        vr, tr = mr.reference_mesh(vol, np.float32(iso), me.case_table(), me.EDGES)
        _cache[name] = (vol, iso, vr, tr)
    return _cache[name]


def _calls(what):
    from torch_utils import hip_plugin
    return hip_plugin.CALLS.get(what, 0)


@pytest.mark.parametrize('name', sorted(VOLUMES))
def test_kernel_matches_reference(name, gpu_device):
    vol, iso, vr, tr = case(name)
    before = _calls('mesh_emit')
    v, t = me.marching_cubes(torch.from_numpy(vol).to(gpu_device), iso)
    assert _calls('mesh_emit') == before + 1
    assert v.device.type == 'cuda' and v.dtype == torch.float32 and t.dtype == torch.int32
    v, t = v.cpu().numpy(), t.cpu().numpy()
    assert v.shape == (vr.shape[0], 3) and t.shape == tr.shape
    # fp32 against float64 at coordinates below 32 (33 points is the longest axis): the values and the threshold are the same fp32
    # numbers on both sides; iso - v_a and v_b - v_a round once each and the IEEE division once: |dt| <= 3 * 2^-24 (t <= 1); the sum
    # index + t rounds to half an ulp of a number below 32 = 2^-20.  Together 2^-20 + 3 * 2^-24 = 1.13e-6 < 2e-6.
    idx = mr.match_vertices(vr, v, 2e-6)
    assert mr.triangle_keys(vr[idx], t) == mr.triangle_keys(vr, tr)
    closed_ref = mr.is_closed(tr)
    assert mr.is_closed(t) == closed_ref
    if closed_ref:
        assert mr.euler(v.shape[0], t) == mr.euler(vr.shape[0], tr)
    else:
        assert sorted(mr.open_half_edges(idx[t])) == sorted(mr.open_half_edges(tr))
    # the documented order is the host definition's
    hv, ht, _ = me.marching_cubes_host(vol, iso)
    assert np.array_equal(ht, t) and np.abs(hv - v).max() <= 2e-6


def test_two_runs_are_bit_equal(gpu_device):
    vol = torch.from_numpy(case('noise')[0]).to(gpu_device)
    a = me.marching_cubes(vol, 0.0, normals=True)
    b = me.marching_cubes(vol.clone(), 0.0, normals=True)
    assert a[0].shape[0] > 0
    for x, y in zip(a, b):
        assert torch.equal(x, y)


def test_compaction_across_many_workgroups(gpu_device):
    """96^3 points = 864 workgroups of 1024 points: the single scan launch gives every thread but the last ones one offset pair."""
    vol = mr.sphere_volume(96, 40.0).astype(np.float32)
    v, t = me.marching_cubes(torch.from_numpy(vol).to(gpu_device), 0.0)
    hv, ht, _ = me.marching_cubes_host(vol, 0.0)
    assert v.shape == hv.shape and t.shape == ht.shape
    assert int(t.min()) >= 0 and int(t.max()) < v.shape[0]
    assert torch.unique(t).numel() == v.shape[0]
    t = t.cpu().numpy()
    assert np.array_equal(t, ht)
    assert mr.is_closed(t) and mr.euler(v.shape[0], t) == 2
    assert np.abs(v.cpu().numpy() - hv).max() <= 8e-6          # coordinates below 128: half an ulp is 2^-18


def test_all_below_and_all_above(gpu_device):
    for fill in (-1.0, 1.0):
        out = me.marching_cubes(torch.full([9, 6, 5], fill, device=gpu_device), 0.0, normals=True)
        assert [tuple(o.shape) for o in out] == [(0, 3), (0, 3), (0, 3)] and out[1].dtype == torch.int32


def test_lattice(gpu_device):
    vol = torch.from_numpy(case('sphere')[0]).to(gpu_device)
    voxel_size, corner, scale = 2.0 / 23, np.array([-1.0, -1.1, -1.2]), 0.9
    v, t = me.marching_cubes(vol, 0.0)
    w, t2 = me.marching_cubes(vol, 0.0, lattice=(voxel_size, corner, scale))
    want = scale * (v.double().cpu().numpy() * voxel_size + corner[::-1])
    assert torch.equal(t, t2)
    assert np.abs(w.cpu().numpy() - want).max() <= 1e-6 * np.abs(want).max()


def test_normals(gpu_device):
    for name in ('sphere', 'ragged_33x18x7'):
        vol, iso, _, _ = case(name)
        for flip in (False, True):
            v, t, n = me.marching_cubes(torch.from_numpy(vol).to(gpu_device), iso, normals=True, flip=flip)
            hv, ht, hn = me.marching_cubes_host(vol, iso, normals=True, flip=flip)
            assert np.array_equal(t.cpu().numpy(), ht)
            assert np.abs(n.cpu().numpy() - hn).max() <= 1e-5
    # stripes along x: the central difference vanishes at both ends of every interior x edge -> zero normals, never NaN
    vol = (torch.arange(6) % 2).float()[:, None, None].expand(6, 4, 4).contiguous()
    v, t, n = me.marching_cubes(vol.to(gpu_device), 0.5, normals=True)
    _, _, hn = me.marching_cubes_host(vol.numpy(), 0.5, normals=True)
    n = n.cpu()
    assert torch.isfinite(n).all() and np.abs(n.numpy() - hn).max() <= 1e-5
    inner = (v[:, 0].cpu() > 1) & (v[:, 0].cpu() < 4)
    assert inner.any() and (n[inner] == 0).all() and (n[~inner] != 0).any()


@pytest.fixture(scope='module')
def tiny_generator(gpu_device):
    from training import triplane
    torch.manual_seed(0)
    G = triplane.TriPlaneGenerator(triplane.tiny_spec()).eval().to(gpu_device)
    z = torch.from_numpy(np.random.RandomState(0).randn(1, G.z_dim)).float().to(gpu_device)
    return G, z, triplane.conditioning_label(gpu_device)


def test_extract_mesh(tiny_generator, gpu_device):
    from training import shape_extraction as se
    G, z, c = tiny_generator
    N = 32
    with torch.no_grad():
        ws = G.mapping(z, c, truncation_psi=0.5)
        img_v, seg_v = se.triplanes_from_ws(G.synthesis, ws, noise_mode='const')
        cube = se.density_cube(G.synthesis.renderer, img_v, seg_v, voxel_resolution=N, max_batch=None)[0]
    threshold = float(cube.median())
    before = _calls('mesh_emit')
    out = me.extract_mesh(G, z, c, voxel_resolution=N, threshold=threshold, normals=True, vertex_attributes=True)
    assert _calls('mesh_emit') == before + 1
    assert torch.equal(me.extract_mesh(G, ws, voxel_resolution=N, threshold=threshold)['vertices'], out['vertices'])
    lattice = (2.0 / (N - 1), np.array([-1.0, -1.0, -1.0]), 0.9)
    hv, ht, hn = me.marching_cubes_host(cube.cpu().numpy(), threshold, normals=True, lattice=lattice)
    assert ht.shape[0] > 0 and np.array_equal(out['triangles'].cpu().numpy(), ht)
    assert np.abs(out['vertices'].cpu().numpy() - hv).max() <= 1e-6          # world coordinates within [-0.9, 0.9]
    assert np.abs(out['normals'].cpu().numpy() - hn).max() <= 1e-5
    spec = G.synthesis.renderer.spec
    labels, colors = out['labels'], out['colors']
    assert labels.shape == (hv.shape[0],) and int(labels.min()) >= 0 and int(labels.max()) < spec.seg_channels
    assert colors.shape == (hv.shape[0], 3) and colors.dtype == torch.uint8
    with torch.no_grad():
        feat = G.synthesis.renderer.sample_voxel(img_v, seg_v, out['vertices'].unsqueeze(0))
    assert torch.equal(labels, feat[:, spec.feature_channels:spec.feature_channels + spec.seg_channels].argmax(dim=1))
    assert torch.equal(colors, (feat[:, :3] * 127.5 + 128).clamp(0, 255).to(torch.uint8))


def test_largest_grid_indexes_past_2_to_the_31_bytes(gpu_device):
    """1024^3 points (4 GiB of volume, byte offsets past 2^32, 2^20 workgroup pairs through the one scan launch): a 12^3 block of noise
    in the far corner, last layer of points included, must give the mesh of that block alone, shifted."""
    from torch_utils import hip_plugin
    n, m = 1024, 12
    block = mr.noise_volume((m + 1, m + 1, m + 1), seed=5, border=None).astype(np.float32)
    block[0] = block[:, 0] = block[:, :, 0] = -1.0                     # the layer that faces the empty rest of the grid
    hv, ht, _ = me.marching_cubes_host(block, 0.0)
    try:
        vol = torch.full([n, n, n], -1.0, device=gpu_device)
        vol[n - m - 1:, n - m - 1:, n - m - 1:] = torch.from_numpy(block).to(gpu_device)
        v, t = me.marching_cubes(vol, 0.0)
        assert ht.shape[0] > 0 and np.array_equal(t.cpu().numpy(), ht)
        # index + t is rounded to fp32 below 1024: half an ulp is 2^-15 = 3.1e-5 (the block's own result carries 1e-6)
        assert np.abs(v.cpu().numpy().astype(np.float64) - (hv.astype(np.float64) + (n - m - 1))).max() <= 4e-5
    finally:
        hip_plugin.MeshPlugin._ws.table.clear()                         # do not keep 4 GiB of workspace for the rest of the session
