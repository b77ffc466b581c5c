"""The needed-cell map of the plane gate on the device (ide3d_plane_cells, csrc/camera.hip) against the float64 reference of
tests/plane_cells_ref.py, 16 x 16 rays x 12 steps on 64^2 planes: the map contains every cell the marcher can address (`reads`: the taps of
the draws 0, 0.5, 1 - 2^-24 and one random draw per sample, in bounds or clamped) and is contained in the continuous hull dilated by one
cell, so neither a hole nor "mark everything" passes.  Cameras: yaw 0 and +-0.5 (two images), a steep pitch, a camera so close that rays
leave the volume, fov 60, and one aimed at a plane corner (last row and column live).

Taps outside the plane do mark cells: the border texels the marcher loads them from (tap_addr clamps the address, the weight is zero),
because a skipped tile's memory may hold an Inf or a NaN and 0 x that is not 0.  They do not wrap, and they never reach past the border
cells: `hull` is built from the same clamped addresses and caps them."""
import numpy as np
import pytest
import torch

import plane_cells_ref as ref

pytestmark = pytest.mark.gpu


def _device_map(dev, cam, fov, size=ref.SIZE, steps=ref.STEPS, plane=ref.PLANE):
    from torch_utils import hip_plugin
    from training import volumetric_rendering as vr
    vr._init()
    rays, z_lin = vr._fused_ray_setup(dev, float(fov), (size, size), int(steps), float(ref.T0), float(ref.T1))
    cells = hip_plugin.plane_cells(rays, z_lin, torch.from_numpy(cam).to(dev), plane, plane)
    torch.cuda.synchronize()
    return cells.cpu().numpy()


@pytest.mark.parametrize('name', sorted(ref.CASES))
def test_map_between_reads_and_dilated_hull(gpu_device, name):
    cam, fov = ref.CASES[name]
    got = _device_map(gpu_device, cam, fov)
    args = (cam, fov, ref.SIZE, ref.STEPS, ref.T0, ref.T1, ref.PLANE, ref.PLANE)
    assert got.shape == (cam.shape[0], 3, ref.PLANE // 4, ref.PLANE // 4) and set(np.unique(got)) <= {0, 1}
    rd, cap = ref.reads(*args), ref.dilate(ref.hull(*args))
    print(name, 'device share', got.mean(axis=(1, 2, 3)), 'reads', rd.mean(axis=(1, 2, 3)), 'cap', cap.mean(axis=(1, 2, 3)))
    missing, extra = rd & ~got, got & ~cap
    assert not missing.any(), f'{int(missing.sum())} addressed cells are not in the map, first at {np.argwhere(missing)[0]}'
    assert not extra.any(), f'{int(extra.sum())} cells of the map are outside the dilated hull, first at {np.argwhere(extra)[0]}'
    if name == 'plane_corner':
        assert got[0, 0, -1, -1] == 1
    if name == 'yaw_pm05':
        assert (got[0] != got[1]).any(), 'the two cameras see different cells'


def test_map_is_rewritten_per_call_and_odd_plane_sizes_are_covered(gpu_device):
    """The map is zeroed by the call itself (a buffer reused across replays of a graph must not keep the last camera's cells), and a
    plane whose size is no multiple of the cell (62 x 62: 16 x 16 cells, the last one partial) stays inside its map."""
    from torch_utils import hip_plugin
    from training import volumetric_rendering as vr
    vr._init()
    dev = gpu_device
    rays, z_lin = vr._fused_ray_setup(dev, 18.0, (ref.SIZE, ref.SIZE), ref.STEPS, float(ref.T0), float(ref.T1))
    lib = hip_plugin.load()
    cells = torch.full([1, 3, 16, 16], 7, dtype=torch.uint8, device=dev)
    guard = torch.full([64], 9, dtype=torch.uint8, device=dev)               # (allocated right behind: a write past the map would land here or beyond)
    cam = torch.from_numpy(ref.CASES['plane_corner'][0]).to(dev)
    rc = lib.ide3d_plane_cells(rays.data_ptr(), z_lin.data_ptr(), cam.data_ptr(), 1, rays.shape[0], z_lin.shape[0], 62, 62, cells.data_ptr(),
                               hip_plugin._stream(cells))
    assert rc == 0, lib.ide3d_last_error()
    torch.cuda.synchronize()
    got = cells.cpu().numpy()
    assert set(np.unique(got)) <= {0, 1} and got[0, 0, 15, 15] == 1 and (guard == 9).all()
    args = (ref.CASES['plane_corner'][0], 18.0, ref.SIZE, ref.STEPS, ref.T0, ref.T1, 62, 62)
    assert not (ref.reads(*args) & ~got).any() and not (got & ~ref.dilate(ref.hull(*args))).any()
