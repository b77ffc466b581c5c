"""The pose kernels of csrc/camera.hip (`ide3d_sphere_points`, `ide3d_cam2world`) at their edges: whole and ragged workgroups of 64 cameras
(n = 64, 65, 129), pitch at and outside the clamp ends, NaN pitch, `pitch_is_v` with v at both clamp ends, forward vectors parallel to the
world's up axis and of length zero, a look-at point that is the camera's own position, one look-at point for all cameras and one each.

Two comparisons.  Against the ATen chain of training/volumetric_rendering.py (IDE3D_NO_CAMERA_KERNELS=1) through the public functions, with
the tolerances of tests/test_gpu_ops.py::test_camera_pose_kernels (3e-6) and NaN in the same positions.  Against a float64 restatement of the
three reference functions (tests/camera_ref.py) with the convention of tests/edge_bound.py: error <= max(4 x the error of the restatement evaluated by
ATen in fp32 on the device, one fp32 ulp of the largest magnitude).  The arccos next to +-1 is ill-conditioned for the kernel and for ATen
alike, which is why the bound is ATen's own error and no fixed figure."""

import math

import pytest
import torch

from camera_ref import _normalize, cam2world_ref, lookat_ref, sphere_ref
from edge_bound import within
from util import assert_close

pytestmark = pytest.mark.gpu

SIZES = (64, 65, 129)
F32 = torch.float32


def _plugin():
    from torch_utils import hip_plugin
    hip_plugin.load()
    return hip_plugin.CameraPlugin


def _both(monkeypatch, fn, what):
    """fn() through the kernels and through the ATen chain under one generator state: the existing tolerance, NaN in the same positions."""
    from torch_utils import hip_plugin
    count = lambda: hip_plugin.CALLS.get('sphere_points', 0) + hip_plugin.CALLS.get('cam2world', 0)
    monkeypatch.delenv('IDE3D_NO_CAMERA_KERNELS', raising=False)
    torch.manual_seed(5)
    before = count()
    got = fn()
    assert count() > before, f'{what}: no kernel launch'
    monkeypatch.setenv('IDE3D_NO_CAMERA_KERNELS', '1')
    torch.manual_seed(5)
    before = count()
    ref = fn()
    assert count() == before
    monkeypatch.delenv('IDE3D_NO_CAMERA_KERNELS')
    got, ref = (t if isinstance(t, tuple) else (t,) for t in (got, ref))
    for g, r in zip(got, ref):
        assert g.shape == r.shape and g.dtype == r.dtype and g.device == r.device
        nan = torch.isnan(r)
        assert torch.equal(torch.isnan(g), nan), f'{what}: NaN in other positions than the ATen chain'
        assert_close(torch.where(nan, torch.zeros_like(g), g), torch.where(nan, torch.zeros_like(r), r), rtol=0, atol=3e-6, what=what)
    return got


@pytest.mark.parametrize('n', SIZES)
def test_sphere_points(gpu_device, monkeypatch, n):
    """Pitch exactly 0, pi, below 0 and above pi (clamped), NaN (kept, in the same positions), random; theta over several turns.
    Measured: profiles/small_ops/edge_suite_measured.json, kernel sphere_points."""
    from training import volumetric_rendering as vr
    dev = gpu_device
    for mean in (0.0, math.pi, -0.3, 4.0, float('nan'), 1.9):
        got = _both(monkeypatch, lambda: vr.sample_camera_positions(dev, n=n, r=1.7, horizontal_mean=1.1, vertical_mean=mean, mode=None), f'pitch {mean}')
        assert got[0].shape == (n, 3) and got[1].shape == (n, 1)
    _both(monkeypatch, lambda: vr.sample_camera_positions(dev, n=n, r=1.7, horizontal_stddev=0.4, vertical_stddev=0.9, horizontal_mean=1.1, vertical_mean=1.5, mode='normal'), 'normal')
    g = torch.Generator().manual_seed(n)
    theta = (torch.rand(n, 1, generator=g) - 0.5) * 20
    pitch = torch.rand(n, 1, generator=g) * 5 - 1          # about two in five outside (0, pi)
    pitch[0], pitch[1], pitch[2], pitch[3], pitch[n - 1], pitch[n - 2] = 0.0, math.pi, -0.5, float('nan'), float('nan'), 3.5
    for is_v in (False, True):
        pos, phi = _plugin().sphere_points(theta.to(dev), pitch.to(dev), 2.7, pitch_is_v=is_v)
        want_pos, want_phi = sphere_ref(theta.double(), pitch.double(), 2.7, is_v)
        aten_pos, aten_phi = sphere_ref(theta.to(dev), pitch.to(dev), 2.7, is_v)
        assert pos.shape == (n, 3) and phi.shape == (n, 1)
        assert torch.equal(torch.isnan(phi.cpu()), torch.isnan(pitch)) and torch.equal(torch.isnan(pos.cpu()), torch.isnan(pitch).expand(n, 3))
        assert within(pos, want_pos, aten_pos, F32, 'sphere_points', 'pos_v' if is_v else 'pos')
        assert within(phi, want_phi, aten_phi, F32, 'sphere_points', 'phi_v' if is_v else 'phi')
        if not is_v:          # the clamp ends themselves: fp32(1e-5) and fp32(pi - 1e-5)
            lo, hi = torch.tensor(1e-5, dtype=F32), torch.tensor(math.pi - 1e-5, dtype=F32)
            assert float(phi[0]) == float(lo) and float(phi[2]) == float(lo) and float(phi[1]) == float(hi) and float(phi[n - 2]) == float(hi)


@pytest.mark.parametrize('n', SIZES)
def test_pitch_is_v_at_both_clamp_ends(gpu_device, monkeypatch, n):
    """LookAtPoseSampler with v clamped at 1e-5 and at pi - 1e-5: phi = arccos(1 - 2 v / pi) next to 0 and pi; and spread draws."""
    from training import volumetric_rendering as vr
    dev = gpu_device
    lookat = torch.tensor([0.0, 0.05, 0.2], device=dev)
    for v_mean, v_std in ((-1.0, 0.0), (7.0, 0.0), (0.0, 0.0), (math.pi, 0.0), (1.4, 1.5)):
        out, = _both(monkeypatch, lambda: vr.LookAtPoseSampler.sample(1.3, v_mean, lookat, horizontal_stddev=0.3, vertical_stddev=v_std, radius=2.7, batch_size=n, device=dev),
                     f'v {v_mean} +- {v_std}')
        assert out.shape == (n, 4, 4) and not bool(torch.isnan(out).any())
    g = torch.Generator().manual_seed(n)
    h, v = torch.randn(n, 1, generator=g), torch.rand(n, 1, generator=g) * 5 - 1
    v[0], v[1], v[n - 1] = -2.0, 9.0, 1e-5
    for stride, look in ((0, torch.tensor([0.1, 0.0, -0.2])), (3, torch.randn(n, 3, generator=g) * 0.1)):
        P = _plugin()
        origins, _ = P.sphere_points(h.to(dev), v.to(dev), 2.7, pitch_is_v=True)
        got = P.cam2world(None, origins, lookat=look.to(dev))
        want = lookat_ref(h.double(), v.double(), look.double(), 2.7)
        aten = lookat_ref(h.to(dev), v.to(dev), look.to(dev), 2.7)
        assert within(got, want, aten, F32, 'cam2world', f'lookat_stride{stride}')


@pytest.mark.parametrize('n', SIZES)
def test_cam2world_degenerate_forward_vectors(gpu_device, monkeypatch, n):
    """forward parallel to (0, 1, 0) (the left vector is 0 / 0) and of length zero: NaN exactly where the ATen chain has NaN (whole columns
    of the matrix product, the last row included), the translation column untouched; everything else inside the bound.  First and last camera of every workgroup among them."""
    from training import volumetric_rendering as vr
    dev = gpu_device
    g = torch.Generator().manual_seed(100 + n)
    fwd, org = torch.randn(n, 3, generator=g), torch.randn(n, 3, generator=g)
    fwd[0] = torch.tensor([0.0, 1.0, 0.0]); fwd[1] = torch.tensor([0.0, -2.5, 0.0]); fwd[2] = 0.0
    fwd[63] = torch.tensor([0.0, 3.0, 0.0]); fwd[n - 1] = 0.0
    fwd[5] = torch.tensor([1e-10, 1.0, 0.0])          # nearly parallel (the square is a normal fp32 number): finite
    got, = _both(monkeypatch, lambda: vr.create_cam2world_matrix(fwd.to(dev), org.to(dev), device=dev), 'degenerate forward')
    want = cam2world_ref(fwd.double(), org.double())
    aten = cam2world_ref(fwd.to(dev), org.to(dev))
    bad = torch.zeros(n, dtype=torch.bool); bad[[0, 1, 2, 63, n - 1]] = True
    nan = torch.isnan(got.cpu())
    assert torch.equal(nan.any(dim=(1, 2)), bad) and torch.equal(nan, torch.isnan(want))
    assert torch.equal(got[:, :3, 3].cpu(), org) and torch.equal(got[~bad][:, 3].cpu(), torch.tensor([0.0, 0.0, 0.0, 1.0]).expand(n - int(bad.sum()), 4))
    # the reference multiplies translation @ rotation: the NaN of a column reaches its last row too
    assert bool(nan[0, :, 0].all()) and bool(nan[0, :, 1].all()) and not bool(nan[0, :, 2:].any()) and bool(nan[2, :, :3].all()) and not bool(nan[2, :, 3].any())
    assert within(got, want, aten, F32, 'cam2world', 'forward')


@pytest.mark.parametrize('n', SIZES)
def test_lookat_equal_to_the_origin_and_both_strides(gpu_device, monkeypatch, n):
    """lookat == origin gives a zero forward vector: NaN rotation for that camera only.  One look-at point for all cameras ([3] and [1, 3]:
    stride 0) and one per camera ([n, 3]: stride 3) through the public function."""
    from training import volumetric_rendering as vr
    dev = gpu_device
    g = torch.Generator().manual_seed(200 + n)
    for look in (torch.tensor([0.0, 0.05, 0.2]), torch.tensor([[0.1, 0.0, -0.2]]), torch.randn(n, 3, generator=g) * 0.1):
        _both(monkeypatch, lambda: vr.LookAtPoseSampler.sample(1.3, 1.4, look.to(dev), horizontal_stddev=0.3, vertical_stddev=0.2, radius=2.7, batch_size=n, device=dev),
              f'lookat {tuple(look.shape)}')
    P = _plugin()
    org = torch.randn(n, 3, generator=g)
    look = torch.randn(n, 3, generator=g) * 0.1
    for i in (0, 63, n - 1):
        look[i] = org[i]
    got = P.cam2world(None, org.to(dev), lookat=look.to(dev))
    want = cam2world_ref(_normalize(look.double() - org.double()), org.double())
    aten = cam2world_ref(_normalize(look.to(dev) - org.to(dev)), org.to(dev))
    bad = torch.zeros(n, dtype=torch.bool); bad[[0, 63, n - 1]] = True
    assert torch.equal(torch.isnan(got.cpu()).any(dim=(1, 2)), bad)
    assert within(got, want, aten, F32, 'cam2world', 'lookat_eq_origin')
    one = org[7].clone()          # stride 0: the shared point is camera 7's own position
    got = P.cam2world(None, org.to(dev), lookat=one.to(dev))
    want = cam2world_ref(_normalize(one.double() - org.double()), org.double())
    aten = cam2world_ref(_normalize(one.to(dev) - org.to(dev)), org.to(dev))
    bad = torch.zeros(n, dtype=torch.bool); bad[7] = True
    assert torch.equal(torch.isnan(got.cpu()).any(dim=(1, 2)), bad)
    assert within(got, want, aten, F32, 'cam2world', 'lookat_shared')
