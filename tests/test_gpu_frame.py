"""`ide3d_frame_u8` (csrc/frame.hip) byte for byte: against the oracle (the reference's `layout_grid` conversion beside `mask2color`) and
against the ATen branch of `training.distributed_render.frames_u8` on the same device tensors, on the inputs of tests/frame_cases.py, where a
conversion that rounds 127.5 x + 128 once gives other bytes (tests/test_frame_cases_cpu.py: 126 values on 126 byte boundaries).  The
two branches of `frames_u8` are chosen by W % 4, so they must not differ by a byte."""

import numpy as np
import pytest
import torch

import frame_cases as fc
from oracle import ops as oracle_ops

pytestmark = pytest.mark.gpu


def _both_branches(img, seg, pal, out=None):
    """(kernel branch, ATen branch) of frames_u8 on device tensors.  A float64 image holds the same values and takes the ATen branch, which
    converts it back to fp32 first."""
    from torch_utils import hip_plugin
    from training import distributed_render
    before = hip_plugin.CALLS.get('frame_u8', 0)
    got = distributed_render.frames_u8(img, seg, pal, out=out)
    assert hip_plugin.CALLS.get('frame_u8', 0) == before + 1
    aten = distributed_render.frames_u8(img.double(), seg, pal)
    assert hip_plugin.CALLS.get('frame_u8', 0) == before + 1
    return got, aten


@pytest.mark.parametrize('n,h,w', [(1, 2850, 4), (1, 1, 11396), (3, 31, 124)], ids=['W4', 'H1', 'n3'])
def test_boundary_values_byte_exact(gpu_device, n, h, w):
    """One vector per row, one row, three images; directly and through `out=`."""
    img = fc.image(fc.boundary_values(), n, h, w)
    seg = fc.seg_logits(n, 19, h, w)
    want = oracle_ops.frame_u8(img, seg)
    pal = torch.from_numpy(oracle_ops.PALETTE).to(gpu_device)
    imgd, segd = img.to(gpu_device), seg.to(gpu_device)
    got, aten = _both_branches(imgd, segd, pal)
    assert got.shape == (n, h, 2 * w, 3) and got.dtype == torch.uint8
    diff = got.cpu().numpy() != want
    assert not diff.any(), f'{int(diff.sum())} bytes differ from the oracle, first at {np.argwhere(diff)[0]}'
    assert torch.equal(got, aten), 'the two branches of frames_u8 differ'
    out = torch.full((n, h, 2 * w, 3), 77, dtype=torch.uint8, device=gpu_device)
    ret, _ = _both_branches(imgd, segd, pal, out=out)
    assert ret.data_ptr() == out.data_ptr() and np.array_equal(out.cpu().numpy(), want)


def test_second_grid_stride_trip(gpu_device):
    """1024 x 513 four-pixel groups: 1024 more than the 2048 x 256 lanes of the grid, so the last two rows are converted in the loop's second
    trip.  The boundary values repeat through the whole image."""
    n, h, w = 1, 1024, 2052
    assert n * h * (w // 4) > 2048 * 256
    img = fc.image(fc.boundary_values(), n, h, w)
    seg = fc.seg_logits(n, 2, h, w)
    pal = torch.from_numpy(oracle_ops.PALETTE[:2].copy()).to(gpu_device)
    got, aten = _both_branches(img.to(gpu_device), seg.to(gpu_device), pal)
    assert np.array_equal(got.cpu().numpy(), oracle_ops.frame_u8(img, seg, oracle_ops.PALETTE[:2]))
    assert torch.equal(got, aten)


@pytest.mark.parametrize('name,seg', fc.argmax_cases(), ids=[n for n, _ in fc.argmax_cases()])
def test_argmax_ties_nan_and_infinities(gpu_device, name, seg):
    """palette[torch.argmax(seg, 1)]: the first maximum wins (+0 == -0), NaN is the maximum, the first NaN wins, all -inf gives class 0."""
    classes = seg.shape[1]
    pal = torch.from_numpy(oracle_ops.PALETTE[:classes].copy())
    img = torch.zeros(1, 3, 1, 8)
    want = pal[torch.argmax(seg, dim=1)]
    got, aten = _both_branches(img.to(gpu_device), seg.to(gpu_device), pal.to(gpu_device))
    assert torch.equal(got[:, :, 8:].cpu(), want), (name, got[:, :, 8:].cpu().tolist(), want.tolist())
    assert bool((got[:, :, :8] == 128).all())
    assert torch.equal(got, aten)
