"""What tests/test_gpu_camera.py and tests/test_gpu_resample.py rest on, without a GPU: the restated pose functions (tests/camera_ref.py) are
the product's own ATen chain bit for bit on the CPU, the bound helper (tests/edge_bound.py) computes what its docstring says, and the skip
accumulation's float64 reference spreads a non-finite input to the outputs whose taps reach it and no further."""

import math

import pytest
import torch

import camera_ref
import edge_bound


@pytest.mark.parametrize('n', [1, 65])
def test_restated_pose_functions_are_the_products_chain(n):
    from training import volumetric_rendering as vr
    g = torch.Generator().manual_seed(n)
    for mean in (0.0, math.pi, -0.3, 4.0, 1.9):
        pos, phi, theta = vr.sample_camera_positions('cpu', n=n, r=1.7, horizontal_mean=1.1, vertical_mean=mean, mode=None)
        want_pos, want_phi = camera_ref.sphere_ref(theta, torch.full((n, 1), mean), 1.7)
        assert torch.equal(pos, want_pos) and torch.equal(phi, want_phi)
    fwd, org = torch.randn(n, 3, generator=g), torch.randn(n, 3, generator=g)
    fwd[0] = torch.tensor([0.0, 1.0, 0.0])
    a, b = vr.create_cam2world_matrix(fwd, org), camera_ref.cam2world_ref(fwd, org)
    assert bool(torch.isnan(a[0, :3, :3]).any()) and torch.equal(torch.isnan(a), torch.isnan(b))
    assert torch.equal(torch.nan_to_num(a), torch.nan_to_num(b))
    for look in (torch.tensor([0.0, 0.05, 0.2]), torch.randn(n, 3, generator=g) * 0.1):
        for v_mean in (-1.0, 7.0, 1.4):
            torch.manual_seed(5)
            got = vr.LookAtPoseSampler.sample(1.3, v_mean, look, horizontal_stddev=0.3, vertical_stddev=0.2, radius=2.7, batch_size=n)
            torch.manual_seed(5)
            h = torch.randn((n, 1)) * 0.3 + 1.3
            v = torch.randn((n, 1)) * 0.2 + v_mean
            assert torch.equal(got, camera_ref.lookat_ref(h, v, look, 2.7))


def test_bound_helper():
    f32, f16, bf16, f64 = torch.float32, torch.float16, torch.bfloat16, torch.float64
    assert edge_bound.ulp(1.0, f32) == 2.0 ** -23 and edge_bound.ulp(1.999, f32) == 2.0 ** -23 and edge_bound.ulp(2.0, f32) == 2.0 ** -22
    assert edge_bound.ulp(3.0, f16) == 2.0 ** -9 and edge_bound.ulp(3.0, bf16) == 2.0 ** -6 and edge_bound.ulp(0.75, f64) == 2.0 ** -53
    assert edge_bound.ulp(0.0, f32) == 0.0
    for dt in (f32, f16, bf16):
        x = torch.tensor([1.0, 2.0, 0.75, 100.0]).to(dt)
        nxt = torch.nextafter(x.float(), torch.tensor(float('inf'))) if dt == f32 else None
        if nxt is not None:
            assert [float(v) for v in (nxt - x)] == [edge_bound.ulp(float(v), dt) for v in x]
    want = torch.tensor([1.0, -4.0, float('nan'), float('inf')], dtype=f64)
    got = torch.tensor([1.0, -4.0 + 2.0 ** -21, float('nan'), float('inf')])
    aten = torch.tensor([1.0 + 2.0 ** -23, -4.0, 0.0, float('nan')])          # the comparison operator may be non-finite elsewhere
    assert edge_bound.max_err(got, want) == 2.0 ** -21
    assert edge_bound.within(got, want, aten, f32, 'none', 'none')          # one ulp at 4 is 2^-21; 4 x ATen's 2^-23 is as much
    assert not edge_bound.within(got + torch.tensor([0.0, 2.0 ** -21, 0.0, 0.0]), want, aten, f32, 'none', 'none')
    for bad in (torch.tensor([1.0, -4.0, 0.0, float('inf')]), torch.tensor([1.0, -4.0, float('nan'), -float('inf')]), torch.tensor([float('nan'), -4.0, float('nan'), float('inf')])):
        with pytest.raises(AssertionError):
            edge_bound.max_err(bad, want)
    und = torch.tensor([False, True, False, False])
    assert edge_bound.max_err(torch.tensor([1.0, 0.0, float('nan'), float('inf')]), want, alt=torch.zeros(4, dtype=f64), undecided=und) == 0.0


def test_skip_reference_spreads_non_finite_inputs_to_their_taps_only():
    from oracle import ops as oracle_ops
    from torch_utils.ops import upfirdn2d
    f = upfirdn2d.setup_filter([1, 3, 3, 1])
    lo = torch.randn(1, 2, 3, 17, generator=torch.Generator().manual_seed(0), dtype=torch.float64)
    clean = oracle_ops.upsample2d(lo, f)
    # the polyphase form the kernel evaluates: even outputs (in[m - 1] + 3 in[m]) / 4, odd (3 in[m] + in[m + 1]) / 4, zero outside
    pad = torch.nn.functional.pad(lo, (1, 1, 1, 1))
    rows = torch.stack([(pad[:, :, :-2] + 3 * pad[:, :, 1:-1]) / 4, (3 * pad[:, :, 1:-1] + pad[:, :, 2:]) / 4], dim=3).reshape(1, 2, 6, 19)
    poly = torch.stack([(rows[..., :-2] + 3 * rows[..., 1:-1]) / 4, (3 * rows[..., 1:-1] + rows[..., 2:]) / 4], dim=4).reshape(1, 2, 6, 34)
    torch.testing.assert_close(clean, poly, rtol=1e-13, atol=1e-13)
    lo[0, 0, 0, 0], lo[0, 1, 1, 8] = float('inf'), float('nan')
    bad = ~torch.isfinite(oracle_ops.upsample2d(lo, f))
    want = torch.zeros_like(bad)
    want[0, 0, 0:3, 0:3] = True          # pixel m reaches outputs 2m - 1 .. 2m + 2
    want[0, 1, 1:5, 15:19] = True
    assert torch.equal(bad, want)
