"""The float64 reference of the plane gate's needed-cell map (tests/plane_cells_ref.py) against the project's own step-wise ray code, and
the properties the device test (tests/test_gpu_plane_cells.py) leans on: the cap `hull` dilated by one cell contains `reads` and stays
short of "everything" where the camera sees part of the volume, so a map that marks every cell cannot pass."""
import math

import numpy as np
import pytest
import torch

import plane_cells_ref as ref


def test_cameras_and_rays_match_the_project():
    from training import triplane, volumetric_rendering as vr
    for yaw, pitch, radius in ((0.0, math.pi / 2, 2.7), (-0.5, math.pi / 2, 2.7), (0.3, 0.35, 2.7), (0.2, math.pi / 2, 1.2)):
        want = triplane.camera_label(yaw, pitch=pitch, radius=radius)[0, :16].reshape(4, 4).numpy()
        np.testing.assert_allclose(ref._orbit(yaw, pitch, radius), want, atol=2e-6)
    for fov in (18.0, 60.0):
        np.testing.assert_allclose(ref.camera_rays(fov, ref.SIZE), vr._camera_rays('cpu', fov, (ref.SIZE, ref.SIZE)).numpy(), atol=1e-6)


@pytest.mark.parametrize('name', sorted(ref.CASES))
def test_exact_cells_are_the_taps_of_the_stepwise_points(name):
    """`exact` at jitter 0.5 = the cells under the in-bounds taps of the points the step-wise renderer samples
    (get_initial_rays_trig + transform_sampled_points, float32), up to taps that sit within float32 rounding of a texel edge."""
    from training import volumetric_rendering as vr
    cam, fov = ref.CASES[name]
    n = cam.shape[0]
    points, z_vals, rays_d = vr.get_initial_rays_trig(n, ref.STEPS, 'cpu', fov, (ref.SIZE, ref.SIZE), ref.T0, ref.T1)
    pts, *_ = vr.transform_sampled_points(points, z_vals, rays_d, 'cpu', h_stddev=0, v_stddev=0, camera=torch.from_numpy(cam), mode=None,
                                          jitter=torch.full_like(z_vals, 0.5))
    w = pts.reshape(n, -1, 3).double().numpy()
    got = np.zeros([n, 3, ref.PLANE // 4, ref.PLANE // 4], dtype=np.uint8)
    for pl, (a, b) in enumerate(((0, 1), (1, 2), (0, 2))):
        u = ((w[..., a] + 1) * ref.PLANE - 1) / 2
        v = ((w[..., b] + 1) * ref.PLANE - 1) / 2
        for dx in (0, 1):
            for dy in (0, 1):
                x, y = np.floor(u).astype(int) + dx, np.floor(v).astype(int) + dy
                ok = (x >= 0) & (x < ref.PLANE) & (y >= 0) & (y < ref.PLANE)
                for i in range(n):
                    got[i, pl, y[i][ok[i]] // 4, x[i][ok[i]] // 4] = 1
    want = ref.exact(cam, fov, ref.SIZE, ref.STEPS, ref.T0, ref.T1, ref.PLANE, ref.PLANE, jitters=(0.5,))
    differ = int((got != want).sum())
    assert differ <= 2, f'{differ} cells differ between the float32 step-wise points and the float64 reference'
    assert not (got & ~ref.dilate(want)).any() and not (want & ~ref.dilate(got)).any()


@pytest.mark.parametrize('name', sorted(ref.CASES))
def test_cap_contains_reads_and_is_not_everything(name):
    cam, fov = ref.CASES[name]
    args = (cam, fov, ref.SIZE, ref.STEPS, ref.T0, ref.T1, ref.PLANE, ref.PLANE)
    ex, rd, hu = ref.exact(*args), ref.reads(*args), ref.hull(*args)
    assert not (ex & ~rd).any() and not (rd & ~hu).any(), 'exact <= reads <= hull'
    cap = ref.dilate(hu)
    share = cap.mean(axis=(1, 2, 3))
    print(name, 'exact', ex.mean(), 'reads', rd.mean(), 'hull', hu.mean(), 'cap', share)
    if name == 'fov60':
        # the widest camera: its rays span the plane it faces (xy) from border to border and beyond.  (16 rays are further apart than a
        # cell there, so cells between them stay clear, and the depth range covers only part of the z axis of the other two planes:
        # "every cell set" needs more rays and steps than the cases have.)
        assert rd[0, 0, 0].any() and rd[0, 0, -1].any() and rd[0, 0, :, 0].any() and rd[0, 0, :, -1].any()
        assert (rd & ~ex).any()
    else:
        assert (share < 0.8).all(), f'the cap must stay short of the whole plane: {share}'
    if name == 'plane_corner':
        assert ex[0, 0, -1, -1] == 1, 'the last row and column of the xy plane are live'
    if name == 'close_leaves_volume':
        assert (rd & ~ex).any(), 'taps outside the planes are loaded from clamped border addresses'


def test_benchmark_cameras_touch_less_than_half_of_the_tiles():
    """The figure the gate rests on: at 256^2, for the benchmark's yaws, the 16 x 16-texel tiles that hold a needed
    cell of any plane are under half of all tiles.  64 x 64 rays x 96 steps, the jitter range covered by `hull`."""
    cams = np.stack([ref._orbit(y) for y in (-0.5, 0.0, 0.5, 0.25)])
    hu = ref.hull(cams, 18.0, 64, 96, ref.T0, ref.T1, 256, 256, per_segment=5)
    tiles = hu.any(axis=1).reshape(4, 16, 4, 16, 4).any(axis=(2, 4))       # 16 x 16 tiles of 4 x 4 cells, union of the planes
    share = tiles.mean(axis=(1, 2))
    print('live 16 x 16 tiles per image:', share, 'cells per plane:', hu.mean(axis=(0, 2, 3)))
    assert (share < 0.5).all(), share
