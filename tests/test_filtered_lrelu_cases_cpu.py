"""The case tables of tests/filtered_lrelu_cases.py against csrc/filtered_lrelu.hip, and their float64 closed forms against autograd through
the op's definition (no GPU): a new kernel instance without a case, a case that no longer crosses a tile border, or a wrong closed form
fails here rather than leave tests/test_gpu_filtered_lrelu.py checking less than it says."""

import numpy as np
import torch

import filtered_lrelu_cases as C


def test_case_table_tracks_the_instance_table():
    instances = C.source_instances()
    assert len(instances) == len(set(instances)) >= 6
    assert {C.instance_of(c) for c in C.INSTANCE_CASES} == set(instances), 'every IDE3D_FLS instance needs a case (and every case an instance)'
    assert {C.instance_of(c) for c in C.SIGN_CASES} >= set(instances)
    assert not any(C.instance_of(c) in instances for c in C.GENERIC_CASES)
    tow, toh = C.source_instance_tile()
    assert (tow, toh) == (32, 32)
    for c in C.INSTANCE_CASES:
        oh, ow = C.out_hw(c)
        assert oh > toh and ow > tow and oh % toh and ow % tow, f"{c['name']}: {oh} x {ow} needs more than one tile per side and a partial last tile"
    for inst in instances:          # the last tile's element stores (width % 4 != 0) for every instance
        assert any(C.out_hw(c)[1] % 4 for c in C.INSTANCE_CASES if C.instance_of(c) == inst), inst
    # generic kernel: more than one of the tile it picks per side, and one case on a smaller tile than the first candidate
    cand, budget = C.source_generic_tiles()
    picked = set()
    for c in C.GENERIC_CASES:
        tile = C.generic_tile(c['up'], c['down'], C.filter_shape(c['fu']), C.filter_shape(c['fd']), cand, budget)
        assert tile is not None, c['name']
        oh, ow = C.out_hw(c)
        assert ow > cand[0][0] >= tile[0] and oh > cand[0][1] >= tile[1], c['name']
        picked.add(tile)
    assert cand[0] in picked and len(picked) > 1
    # scalars the issue asks for, over the set
    assert {c['slope'] for c in C.VALUE_CASES} == {0.0, 0.2, 1.5} and {c['clamp'] for c in C.VALUE_CASES} == {None, 0.8}
    assert all(abs(c['gain'] - np.sqrt(2)) > 0.1 for c in C.VALUE_CASES)
    # sign-offsets of the backward pass: non-zero in the 4x4 and the 8-tap cases
    ofs = {c['name']: c['pad'][0] - (C.filter_shape(c['fu'])[-1] - 1) for c in C.SIGN_CASES}
    assert ofs['S-G0'] == -1 and ofs['S-A5'] == -1 and ofs['S-A1'] == -2


def test_closed_forms_equal_autograd_through_the_definition():
    """`backward64` and `coded_forward64` (what the GPU test holds the sign-read launches to) == float64 autograd through bias_act / upfirdn2d."""
    from torch_utils.ops import filtered_lrelu
    g = torch.Generator().manual_seed(21)
    small = [dict(up=2, down=2, fu=8, fd=12, shape=(1, 2, 7, 6), pad=[9, 10, 8, 11], gain=1.3, slope=0.2, clamp=0.8),
             dict(up=4, down=1, fu=12, fd=None, shape=(2, 1, 5, 4), pad=[5, 6, 7, 4], gain=0.9, slope=1.5, clamp=None),
             dict(up=1, down=3, fu=None, fd=(5, 5), shape=(1, 2, 13, 11), pad=[3, 1, 0, 2], gain=2.5, slope=0.0, clamp=0.8),
             dict(up=2, down=4, fu=(4, 4), fd=9, shape=(1, 1, 9, 10), pad=[2, 3, 4, 1], gain=1.3, slope=0.2, clamp=0.8)]
    for case in small:
        for flip in (False, True):
            x = torch.randn(*case['shape'], generator=g, dtype=torch.float64).requires_grad_(True)
            b = torch.randn(case['shape'][1], generator=g, dtype=torch.float64).requires_grad_(True)
            fu, fd = C.make_filter(case['fu']), C.make_filter(case['fd'])
            kw = dict(up=case['up'], down=case['down'], padding=case['pad'], gain=C.f32(case['gain']), slope=C.f32(case['slope']), clamp=C.f32(case['clamp']), flip_filter=flip)
            y = filtered_lrelu.filtered_lrelu(x, fu=fu, fd=fd, b=b, impl='ref', **kw)
            want_y, codes = C.forward64(case, x.detach(), b.detach(), flip)
            assert tuple(y.shape[2:]) == C.out_hw(case) and tuple(codes.shape[2:]) == C.z_hw(case)
            assert float((y.detach() - want_y).abs().max()) <= 1e-12 * float(want_y.abs().max())
            dy = torch.randn(*y.shape, generator=g, dtype=torch.float64)
            dx, db = torch.autograd.grad(y, [x, b], dy)
            want = C.backward64(case, codes, dy, flip)
            scale = float(want.abs().max())
            assert scale > 0 and float((dx - want).abs().max()) <= 1e-12 * scale, case
            assert float((db - want.sum([0, 2, 3])).abs().max()) <= 1e-11 * scale
            # <B dy, w> == <dy, B^T w>: the coded forward is the transpose of the backward
            w = torch.randn(*x.shape, generator=g, dtype=torch.float64)
            lhs, rhs = float((want * w).sum()), float((dy * C.coded_forward64(case, codes, w, flip)).sum())
            assert abs(lhs - rhs) <= 1e-11 * max(abs(lhs), 1.0)


def test_pack_and_unpack_are_inverse_and_little_endian_in_fields():
    codes = torch.tensor([[[[0, 1, 2, 1, 2, 0]]]], dtype=torch.uint8)
    packed = C.pack_codes(codes, 4)
    assert packed.shape == (1, 1, 1, 4) and packed[0, 0, 0].tolist() == [0 | 1 << 2 | 2 << 4 | 1 << 6, 2, 0, 0]
    assert np.array_equal(C.unpack_codes(packed)[..., :6], codes.numpy())
