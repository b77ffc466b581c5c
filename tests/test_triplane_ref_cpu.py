"""tests/triplane_ref.py is the operation: its two gradients equal float64 CPU autograd through
`dnnlib.util._sample_from_triplane_ref` (three ATen grid_sample look-ups) to 1e-12 relative with no element left out, and its error
scales A and term counts k equal a scalar loop that spells the definition out.

The helper takes the tap position in float32 (the project's tap index contract), autograd takes it in float64 from the coordinate.  For
the two to be the same function of the same numbers the inputs are made so that the float32 evaluation is exact: every coordinate is an
integer cell in [-2, size] plus a fraction in [0.05, 0.95], mapped to a coordinate and rounded to a multiple of 2^-16.  Then c + 1 (< 8, 19
bits), times the size (<= 9: 23 bits), minus 1 and the halving are all exact in float32, so both sides see one and the same u.  The rounding
moves u by at most size * 2^-17 < 1e-4, so the fraction stays inside [0.01, 0.99] (asserted) and the texel cannot differ either.  Cells -2 and
size have no tap in bounds, cells -1 and size - 1 have one or two: partial masks and fully-outside samples are part of the comparison.
"""

import math

import torch

import triplane_ref
from dnnlib import util

N, C, H, W, M = 2, 5, 6, 9, 66


def _axis(cells, frac, size):
    u = cells.double() + frac
    c = (2.0 * u + 1.0) / size - 1.0
    return (torch.round(c * 65536.0) / 65536.0).float()


def _inputs():
    g = torch.Generator().manual_seed(77)
    co = torch.empty(N, M, 3)
    perm = lambda size: torch.stack([(torch.arange(M) % (size + 3) - 2)[torch.randperm(M, generator=g)] for _ in range(N)])
    frac = lambda: torch.rand(N, M, generator=g, dtype=torch.float64) * 0.9 + 0.05
    co[..., 0] = _axis(perm(W), frac(), W)
    co[..., 2] = _axis(perm(H), frac(), H)
    # y is plane 0's v (scaled by H) and plane 1's u (scaled by W): draw it on the W scale, keep the draws whose H-scale fraction fits as well
    cells = perm(W)
    for i in range(N):
        for j in range(M):
            while True:
                y = _axis(cells[i, j], float(torch.rand((), generator=g, dtype=torch.float64)) * 0.9 + 0.05, W)
                v = ((float(y) + 1.0) * H - 1.0) / 2.0
                if 0.05 <= v - math.floor(v) <= 0.95:
                    break
            co[i, j, 1] = y
    planes = torch.randn(N, 3 * C, H, W, generator=g, dtype=torch.float64)
    go = torch.randn(N * M, C, generator=g, dtype=torch.float64)
    return co, planes, go


def test_inputs_cover_every_cell_and_stay_off_the_texel_borders():
    co, _, _ = _inputs()
    seen = [set(), set(), set()]
    for p, (a, b) in enumerate(triplane_ref.PLANE_AXES):
        for axis, size in ((a, W), (b, H)):
            u32 = triplane_ref.unnormalize32(co[..., axis], size)
            u64 = ((co[..., axis].double() + 1.0) * size - 1.0) / 2.0
            assert torch.equal(u32.double(), u64)          # the float32 evaluation is exact: one position for both sides
            fr = u64 - torch.floor(u64)
            assert float(fr.min()) >= 0.01 and float(fr.max()) <= 0.99
            if (axis, size) in ((0, W), (1, W), (2, H)):
                seen[axis] |= set(torch.floor(u64).long().flatten().tolist())
    assert seen[0] == set(range(-2, W + 1)) and seen[1] == set(range(-2, W + 1)) and seen[2] == set(range(-2, H + 1))


def test_helper_equals_float64_autograd_with_nothing_left_out():
    co, planes, go = _inputs()
    ref = triplane_ref.triplane_backward_ref(go, planes, co)
    assert bool(ref.finite.all())
    assert not bool(ref.hit.all()) and bool(ref.hit.any())          # fully-outside samples are in the set
    p = planes.clone().requires_grad_(True)
    c = co.double().requires_grad_(True)
    out = util._sample_from_triplane_ref(c, p)
    gp, gc = torch.autograd.grad((out * go).sum(), [p, c])
    worst = 0.0
    for what, got, want in (('planes', ref.grad_planes, gp), ('coords', ref.grad_coords, gc)):
        assert got.shape == want.shape and got.dtype == torch.float64
        err = (got - want).abs()
        assert bool(((want == 0) == (got == 0)).all()), what
        rel = float((err / want.abs().clamp_min(1e-300)).max())
        worst = max(worst, rel)
        print(f'{what}: {want.numel()} elements compared, {int((want != 0).sum())} non-zero, worst relative error {rel:.2e}')
        assert bool((err <= 1e-12 * want.abs()).all()), what          # every element, none excluded
    # samples with no tap in bounds: exactly zero coordinate gradient
    assert bool((ref.grad_coords[~ref.hit] == 0).all()) and bool((gc[~ref.hit] == 0).all())


def test_error_scales_and_counts_equal_the_scalar_definition():
    """A, k and both gradients, one term at a time in Python floats."""
    co, planes, go = _inputs()
    ref = triplane_ref.triplane_backward_ref(go, planes, co)
    gp = torch.zeros(N, 3 * C, H, W, dtype=torch.float64); ap = torch.zeros_like(gp); kp = torch.zeros(gp.shape, dtype=torch.int64)
    gc = torch.zeros(N, M, 3, dtype=torch.float64); ac = torch.zeros_like(gc); kc = torch.zeros(gc.shape, dtype=torch.int64)
    pos = {(axis, size): triplane_ref.unnormalize32(co[..., axis], size).double() for axis in range(3) for size in (H, W)}
    P, G = planes.tolist(), go.reshape(N, M, C).tolist()
    for i in range(N):
        for j in range(M):
            for p, (a, b) in enumerate(triplane_ref.PLANE_AXES):
                u, v = float(pos[(a, W)][i, j]), float(pos[(b, H)][i, j])
                x0, y0 = math.floor(u), math.floor(v)
                bx, by = u - x0, v - y0
                ax, ay = 1.0 - bx, 1.0 - by
                for ch in range(C):
                    g_ = G[i][j][ch]
                    val = {}
                    for dx, dy, w in ((0, 0, ax * ay), (1, 0, bx * ay), (0, 1, ax * by), (1, 1, bx * by)):
                        x, y = x0 + dx, y0 + dy
                        inside = 0 <= x < W and 0 <= y < H
                        val[dx, dy] = (P[i][p * C + ch][y][x] if inside else 0.0, inside)
                        if inside:
                            gp[i, p * C + ch, y, x] += g_ * w
                            ap[i, p * C + ch, y, x] += abs(g_ * w)
                            kp[i, p * C + ch, y, x] += 1
                    for axis, half, pairs in ((a, 0.5 * W, (((1, 0), (0, 0), ay), ((1, 1), (0, 1), by))),
                                              (b, 0.5 * H, (((0, 1), (0, 0), ax), ((1, 1), (1, 0), bx)))):
                        for hi, lo, f in pairs:
                            if val[hi][1] or val[lo][1]:
                                term = g_ * (val[hi][0] - val[lo][0]) * f * half
                                gc[i, j, axis] += term
                                ac[i, j, axis] += abs(term)
                                kc[i, j, axis] += 1
    assert torch.equal(ref.cnt_planes, kp) and torch.equal(ref.cnt_coords, kc)
    for what, got, want in (('grad_planes', ref.grad_planes, gp), ('A planes', ref.abs_planes, ap),
                            ('grad_coords', ref.grad_coords, gc), ('A coords', ref.abs_coords, ac)):
        scale = ap if 'planes' in what else ac
        assert bool(((got - want).abs() <= 1e-13 * scale).all()), what
    assert bool((ref.abs_planes >= ref.grad_planes.abs() * (1 - 1e-12)).all()) and bool((ref.abs_coords >= ref.grad_coords.abs() * (1 - 1e-12)).all())
    assert int(kp.max()) > 1 and int((kp == 0).sum()) > 0


# ---- the forward definition and the host model of the ray-grid kernel (tests/test_gpu_triplane_fwd.py) ----------------------------------

def test_forward_ref_equals_float64_grid_sample():
    """`triplane_forward_ref` = three float64 ATen grid_sample look-ups (bilinear, zeros padding, align_corners=False), summed; on the
    inputs above both sides see one and the same tap position, so every element is compared, to 1e-12 of its A."""
    co, planes, _ = _inputs()
    out, A, hit, finite = triplane_ref.triplane_forward_ref(planes, co)
    assert out.shape == A.shape == (N * M, C) and out.dtype == torch.float64 and hit.shape == finite.shape == (N, M)
    assert bool(finite.all()) and bool(hit.any()) and not bool(hit.all())
    want = util._sample_from_triplane_ref(co.double(), planes)
    assert want.shape == out.shape
    err = (out - want).abs()
    print(f'forward: {out.numel()} elements, worst error / A {float((err / A.clamp_min(1e-300)).max()):.2e}')
    assert bool((err <= 1e-12 * A).all())
    assert bool((A >= out.abs() * (1 - 1e-12)).all())
    dead = (~hit).reshape(-1)
    assert bool((out[dead] == 0).all()) and bool((want[dead] == 0).all()) and bool((A[dead] == 0).all())
    assert torch.equal(hit, triplane_ref.triplane_backward_ref(torch.ones(N * M, C, dtype=torch.float64), planes, co).hit)
    # a plane that reads a non-finite coordinate has no tap; the plane that does not read it is untouched
    bad = co.clone()
    bad[0, :len(triplane_ref.NONFINITE)] = torch.tensor(triplane_ref.NONFINITE)
    far = torch.nan_to_num(bad, nan=1e30, posinf=1e30, neginf=-1e30)
    o_bad, a_bad, hit_bad, fin_bad = triplane_ref.triplane_forward_ref(planes, bad)
    o_far, a_far, hit_far, fin_far = triplane_ref.triplane_forward_ref(planes, far)
    assert int((~fin_bad).sum()) == len(triplane_ref.NONFINITE) and bool(fin_far.all())
    assert torch.equal(o_bad, o_far) and torch.equal(a_bad, a_far) and torch.equal(hit_bad, hit_far)
    assert not bool(hit_bad[0, 6]) and bool(hit_bad[0, :3].all())          # (nan, inf, -inf): nothing left; (nan, 0, 0): plane 1 is


def test_tile_plan_is_the_launchers_rule():
    assert triplane_ref.tile_plan(2, 16, 16, 8) == (2, 1)            # the variants case: a workgroup per chunk
    assert triplane_ref.tile_plan(4, 32, 32, 64) == (4, 4)           # the hand-over case: 256 workgroups of four chunks
    assert triplane_ref.tile_plan(1, 64, 64, 96) == (4, 6)           # the benchmark's shape
    assert triplane_ref.tile_plan(3, 16, 24, 12) == (3, 1) and triplane_ref.tile_plan(8, 64, 64, 96) == (1, 24)
    assert triplane_ref.tile_plan(1, 8, 8, 28) == (7, 1)             # only divisors of the chunk count


def test_virtual_index_saturates_and_maps_nan_to_zero():
    c = torch.tensor([float('nan'), float('-inf'), -1e30, -1.5, -1.0, 0.0, 1.0, 1.5, 1e30, float('inf')])
    assert triplane_ref.virtual_index(c, 8).tolist() == [0, 0, 0, 0, 0, 4, 8, 8, 8, 8]
    assert triplane_ref.virtual_index(c, 1).tolist() == [0, 0, 0, 0, 0, 1, 1, 1, 1, 1]


def test_constructed_ray_grids_take_the_prescribed_variants():
    """What the GPU suite relies on, from the host model alone: every chunk of every constructed case gets the mask its kind prescribes."""
    import triplane_cases
    for name, case in (('variants', triplane_cases.variants_case()), ('hand-over', triplane_cases.handover_case()),
                       ('8x24', triplane_cases.mixed_case(311, 2, 20, 28, (8, 24, 8))), ('24x8', triplane_cases.mixed_case(312, 2, 20, 28, (24, 8, 8))),
                       ('channel slice', triplane_cases.mixed_case(313, 2, 20, 28, (16, 16, 8))),
                       ('edges 5x9', triplane_cases.edge_grid_case(5, 9)), ('edges 9x5', triplane_cases.edge_grid_case(9, 5))):
        got = triplane_ref.staged_masks(case['coords'], case['H'], case['W'], case['ray_grid'])
        assert got.shape == case['want'].shape, name
        assert torch.equal(got, case['want']), (name, got.flatten().tolist(), case['want'].flatten().tolist())
        print(f'{name}: masks {sorted(set(got.flatten().tolist()))} over {got.numel()} chunks')


def test_variants_case_reaches_every_mask_and_the_three_way_tie():
    import triplane_cases
    case = triplane_cases.variants_case()
    masks = triplane_ref.staged_masks(case['coords'], case['H'], case['W'], case['ray_grid']).flatten()
    assert set(masks.tolist()) == set(range(8))
    cost = triplane_ref.staged_costs(case['coords'], case['H'], case['W'], case['ray_grid']).reshape(3, -1)
    tie = case['kinds'].index('tie')
    l = cost[:, tie].tolist()
    assert l[0] == l[1] == l[2] == 184 and sum(l) > triplane_ref.TT_CAP and int(masks[tie]) == 3          # usable, over budget, all pairs equal
    # 'big' is unstaged because of its size, 'out' because it leaves the plane: both with mask 0
    assert int(masks[case['kinds'].index('big')]) == 0 and int(masks[case['kinds'].index('out')]) == 0
    _, _, hit, _ = triplane_ref.triplane_forward_ref(torch.zeros(2, 3, 48, 64), case['coords'])
    per_chunk = hit.reshape(2, 2, 8, 2, 8, 2, 4).permute(0, 1, 3, 5, 2, 4, 6).reshape(16, 256)
    assert bool(per_chunk[case['kinds'].index('big')].all()) and not bool(per_chunk[case['kinds'].index('out')].any())


def test_handover_case_changes_the_mask_inside_workgroups():
    import triplane_cases
    case = triplane_cases.handover_case()
    segs, cps = triplane_ref.tile_plan(case['n'], *case['ray_grid'])
    assert (segs, cps) == (4, 4) and cps >= 4
    masks = triplane_ref.staged_masks(case['coords'], case['H'], case['W'], case['ray_grid'])
    per_wg = masks.reshape(-1, cps)                                 # a workgroup = (image, tile, segment): cps consecutive chunks
    assert per_wg.shape[0] == 256
    steps = {(int(a), int(b)) for row in per_wg.tolist() for a, b in zip(row[:-1], row[1:])}
    assert all(a != b for a, b in steps)                            # neighbouring chunks never share a mask
    for m_ in (0, 1, 2, 4):
        assert (7, m_) in steps and (m_, 7) in steps, m_
    assert any(a in (3, 5, 6) and b in (3, 5, 6) for a, b in steps)
    # ... nor a box: the plane-0 region of neighbouring chunks differs in origin or size wherever both are staged
    co = case['coords'].reshape(case['n'], 4, 8, 4, 8, 16, 4, 3).permute(0, 1, 3, 5, 2, 4, 6, 7).reshape(-1, cps, 256, 3)
    lo = triplane_ref.virtual_index(co[..., 0], case['W']).amin(-1)
    hi = triplane_ref.virtual_index(co[..., 0], case['W']).amax(-1)
    same = (lo[:, 1:] == lo[:, :-1]) & (hi[:, 1:] == hi[:, :-1])
    assert float(same.double().mean()) < 0.05
