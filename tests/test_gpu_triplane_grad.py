"""`triplane_backward_kernel` (csrc/triplane.hip: the atomics scatter into the planes and the hand-written coordinate gradient behind
`_TriplaneSampleHip.backward` / `TriplanePlugin.sample_backward`) against the float64 definition of tests/triplane_ref.py, at the shapes,
coordinates and layouts where each line of the kernel can go wrong.  Needs a real MI355X: `pytest -m gpu`.

Every compared element has its own bound, from fp32 rounding of the sum the kernel actually forms (u = 2^-24, one rounding to nearest):

  plane gradient   |got - ref| <= (k + 4) * 2^-24 * A + 1e-30
      A = sum of |go * w| over the k terms the reference added into the texel.  A term is go * (fx * fy): both fractions come from one
      subtraction each (exact, or rounded once for -1 < u < 0), their product and the product with go round once each: four roundings.
      The k atomic adds happen in any order; each rounds a partial sum that is at most A: k - 1 more.  1e-30 is for sums that end below
      the normal range.
  coordinate gradient   |got - ref| <= (2C + 16) * 2^-23 * A
      A = sum of |go * (tap difference) * fraction| * size / 2 over the terms of the two planes that feed the coordinate.  Per term: the
      difference, the fraction, two products, the sum of the two terms of a channel, one add into the lane's partial per trip of the
      lane loop, six shuffle levels, the sum of the two planes and the size / 2 factor: far fewer than 2 * (2C + 16) roundings for every C
      used here.  Where the fraction is recomputed as 1 - (u - floor(u)) its absolute error (<= 2^-25, only for -1 < u < 0) multiplies taps
      at x = -1, which zero padding makes 0 on both sides.

A swapped axis, a wrong size / 2, a dropped tap or a mis-strided atomic is an error of the order of A: five orders above these bounds.
Each test prints its worst error / bound.  The result is not bit-reproducible (fp32 atomics are unordered) and nothing here asserts so.

Rows with NaN / inf coordinates are the only ones ever left out, and only of the coordinate-gradient comparison (ATen's own gradient
there is a mix of NaN and 0): each test asserts that the rows the reference marks non-finite are exactly the ones it inserted.
"""

import math

import pytest
import torch

import triplane_ref

pytestmark = pytest.mark.gpu


def _calls(name):
    from torch_utils import hip_plugin
    return hip_plugin.CALLS.get(name, 0)


# ---- coordinate sets ---------------------------------------------------------------------------------------------------------------

def _uniform(g, n, m):
    return (torch.rand(n, m, 3, generator=g) * 2 - 1) * 1.1


from triplane_ref import NONFINITE, axis_edges as _axis_edges, edges as _edges          # shared with tests/test_gpu_triplane_fwd.py


# ---- comparison --------------------------------------------------------------------------------------------------------------------

def _ratio(err, bound):
    """Worst err / bound; where the bound is 0 (nothing was added) the error has to be 0 as well."""
    zero = bound == 0
    assert bool((err[zero] == 0).all()), 'an element that receives nothing is not exactly 0'
    return float((err[~zero] / bound[~zero]).max()) if bool((~zero).any()) else 0.0


def _compare(name, got_planes, got_coords, ref, C, inserted_nonfinite=0):
    gp = got_planes.detach().cpu().double()
    assert gp.shape == ref.grad_planes.shape
    assert bool(torch.isfinite(gp).all()), f'{name}: non-finite plane gradient'
    assert bool((gp[ref.cnt_planes == 0] == 0).all()), f'{name}: a texel no tap touches received something'
    rp = _ratio((gp - ref.grad_planes).abs(), triplane_ref.plane_bound(ref))
    rc = None
    left_out = int((~ref.finite).sum())
    assert left_out == inserted_nonfinite, f'{name}: {left_out} rows left out, {inserted_nonfinite} non-finite rows inserted'
    if got_coords is not None:
        gc = got_coords.detach().cpu().double()
        assert gc.shape == ref.grad_coords.shape
        keep = ref.finite
        assert bool(torch.isfinite(gc[keep]).all()), f'{name}: non-finite coordinate gradient in a finite row'
        assert bool((gc[keep & ~ref.hit] == 0).all()), f'{name}: a sample with no tap in bounds has a coordinate gradient'
        rc = _ratio((gc - ref.grad_coords).abs()[keep], triplane_ref.coord_bound(ref, C)[keep])
    print(f'triplane-grad {name}: worst error / bound: planes {rp:.3f}' + ('' if rc is None else f', coords {rc:.3f}')
          + f'; rows left out of the coordinate comparison: {left_out}')
    assert rp <= 1.0, f'{name}: plane gradient {rp:.3f} x its bound'
    assert rc is None or rc <= 1.0, f'{name}: coordinate gradient {rc:.3f} x its bound'
    return rp, rc


def _backward(gpu_device, go, planes_dev, co, need_coord_grad=True):
    from torch_utils import hip_plugin
    before = _calls('triplane_sample_backward')
    gp, gc = hip_plugin.TriplanePlugin.sample_backward(go.to(gpu_device), planes_dev, co.to(gpu_device), need_coord_grad)
    assert _calls('triplane_sample_backward') == before + 1
    return gp, gc


def _channels_last(x, gpu_device):
    return x.to(gpu_device).contiguous(memory_format=torch.channels_last)


# ---- shapes: each exists because of one line of the kernel -------------------------------------------------------------------------

SHAPES = [
    (1, 1, 1, 1, 1),            # degenerate everything: m = 1, single-texel planes
    (3, 3, 5, 9, 7),            # C no multiple of 4; H != W; image index from row / m with odd m
    (2, 32, 16, 16, 50),        # the generator's channel count
    (1, 64, 4, 7, 33),          # every lane live: the shuffle reduction adds 64 real partials
    (2, 65, 6, 4, 19),          # second trip of the lane loop with a single live lane
    (1, 96, 8, 8, 40),          # second trip with 32 live lanes
    (2, 4, 8, 8, 5000),         # 10000 rows > 8192 waves: second trip of the grid-stride loop, image boundary inside it
]


def _case(seed, n, C, H, W, m, kind):
    g = torch.Generator().manual_seed(seed)
    planes = torch.randn(n, 3 * C, H, W, generator=g)
    go = torch.randn(n * m, C, generator=g)
    co = _uniform(g, n, m) if kind == 'uniform' else _edges(g, n, m, H, W)
    return planes, go, co


@pytest.mark.parametrize('kind', ['uniform', 'edges'])
@pytest.mark.parametrize('n,C,H,W,m', SHAPES, ids=lambda v: str(v))
def test_backward_shapes(gpu_device, n, C, H, W, m, kind):
    planes, go, co = _case(100 + C + m, n, C, H, W, m, kind)
    ref = triplane_ref.triplane_backward_ref(go, planes, co)
    gp, gc = _backward(gpu_device, go, _channels_last(planes, gpu_device), co)
    _compare(f'n{n} C{C} {H}x{W} m{m} {kind}', gp, gc, ref, C)


def test_backward_every_edge_combination_on_non_square_planes(gpu_device):
    """All side and corner combinations of the edge values at H != W in one launch (the parametrised shapes cycle through a prefix)."""
    n, C, H, W = 1, 3, 5, 9
    g = torch.Generator().manual_seed(31)
    m = len(_axis_edges(W)) * (len(_axis_edges(W)) + len(_axis_edges(H))) * len(_axis_edges(H))
    planes = torch.randn(n, 3 * C, H, W, generator=g)
    go = torch.randn(n * m, C, generator=g)
    co = _edges(g, n, m, H, W)
    ref = triplane_ref.triplane_backward_ref(go, planes, co)
    masks = torch.stack([torch.stack(tp['mask']).sum(0) for tp in triplane_ref.taps(co, H, W)])
    assert {0, 1, 2, 4} <= set(masks.flatten().tolist())          # fully outside, corner, side, inside
    gp, gc = _backward(gpu_device, go, _channels_last(planes, gpu_device), co)
    _compare(f'all {m} edge combinations 5x9', gp, gc, ref, C)


@pytest.mark.parametrize('n,C,H,W,m', [SHAPES[1], SHAPES[4], SHAPES[6]], ids=lambda v: str(v))
def test_backward_non_finite_rows(gpu_device, n, C, H, W, m):
    """NaN / inf rows: the planes receive nothing from them and stay finite; every other row's coordinate gradient is compared."""
    planes, go, co = _case(200 + C, n, C, H, W, m, 'uniform')
    g = torch.Generator().manual_seed(5)
    rows = torch.randperm(n * m, generator=g)[:len(NONFINITE)]
    co.reshape(-1, 3)[rows] = torch.tensor(NONFINITE)
    ref = triplane_ref.triplane_backward_ref(go, planes, co)
    assert torch.equal((~ref.finite).reshape(-1).nonzero().flatten().sort().values, rows.sort().values)
    gp, gc = _backward(gpu_device, go, _channels_last(planes, gpu_device), co)
    _compare(f'n{n} C{C} {H}x{W} m{m} non-finite rows', gp, gc, ref, C, inserted_nonfinite=len(NONFINITE))


@pytest.mark.parametrize('kind', ['one texel', 'four texels'])
def test_backward_collisions(gpu_device, kind):
    """4096 atomic adds per touched texel and channel."""
    n, C, H, W, m = 1, 4, 8, 8, 4096
    g = torch.Generator().manual_seed(41)
    planes = torch.randn(n, 3 * C, H, W, generator=g)
    go = torch.randn(n * m, C, generator=g)
    if kind == 'one texel':
        co = torch.tensor([0.3, -0.2, 0.55]).expand(n, m, 3).contiguous()
    else:                                   # u in [3, 5): two texel origins per axis
        co = ((2 * (3 + 2 * torch.rand(n, m, 3, generator=g)) + 1) / 8 - 1).float()
    ref = triplane_ref.triplane_backward_ref(go, planes, co)
    touched = ref.cnt_planes[ref.cnt_planes > 0]
    assert int(touched.max()) == m and (int(touched.min()) == m if kind == 'one texel' else touched.numel() == 3 * C * 9)
    gp, gc = _backward(gpu_device, go, _channels_last(planes, gpu_device), co)
    _compare(f'collisions, {kind}', gp, gc, ref, C)


# ---- layouts through the plugin ----------------------------------------------------------------------------------------------------

def _layout_inputs():
    n, C, H, W, m = 2, 8, 6, 10, 400
    g = torch.Generator().manual_seed(51)
    wide = torch.randn(n, 30, H, W, generator=g)
    go = torch.randn(n * m, C, generator=g)
    co = torch.cat([_uniform(g, n, m // 2), _edges(g, n, m - m // 2, H, W)], dim=1).contiguous()
    return n, C, H, W, m, wide, go, co


@pytest.mark.parametrize('layout', ['channels_last', 'nchw', 'channel slice', 'expanded'])
def test_backward_layouts(gpu_device, layout):
    n, C, H, W, m, wide, go, co = _layout_inputs()
    if layout == 'channels_last':
        planes = _channels_last(wide[:, 3:27], gpu_device)
        assert planes.stride(1) == 1
    elif layout == 'nchw':
        planes = wide[:, 3:27].to(gpu_device).contiguous()
        assert planes.stride(3) == 1
    elif layout == 'channel slice':          # non-dense strides, base 12 bytes past a 16-byte boundary
        planes = _channels_last(wide, gpu_device)[:, 3:27]
        assert planes.stride() == (30 * H * W, 1, 30 * W, 30) and planes.data_ptr() % 16 == 12
    else:
        planes = _channels_last(wide[:1, 3:27], gpu_device).expand(n, -1, -1, -1)
        assert planes.stride(0) == 0 and planes.shape[0] == n
    ref = triplane_ref.triplane_backward_ref(go, planes.cpu().contiguous(), co)          # of the materialised tensor
    gp, gc = _backward(gpu_device, go, planes, co)
    assert gp.shape == (n, 3 * C, H, W)
    _compare(f'layout {layout}, grad strides {tuple(gp.stride())}', gp, gc, ref, C)


# ---- through sample_from_triplane under autograd -----------------------------------------------------------------------------------

def _wrapper_inputs():
    n, C, H, m = 2, 8, 7, 200
    g = torch.Generator().manual_seed(61)
    planes = torch.randn(n, 3 * C, H, H, generator=g)
    go = torch.randn(n * m, C, generator=g)
    co = torch.cat([_uniform(g, n, m // 2), _edges(g, n, m - m // 2, H, H)], dim=1).contiguous()
    return n, C, H, m, planes, go, co


def test_autograd_nchw_leaf(gpu_device):
    from dnnlib import util
    n, C, H, m, planes, go, co = _wrapper_inputs()
    ref = triplane_ref.triplane_backward_ref(go, planes, co)
    leaf = planes.to(gpu_device).contiguous().requires_grad_(True)
    cc = co.to(gpu_device).requires_grad_(True)
    before = _calls('triplane_sample_backward')
    out = util.sample_from_triplane(cc, leaf, ray_grid=False)
    gp, gc = torch.autograd.grad(out, [leaf, cc], grad_outputs=go.to(gpu_device))
    assert _calls('triplane_sample_backward') == before + 1
    assert gp.shape == leaf.shape and gc.shape == cc.shape
    _compare('autograd, NCHW leaf', gp, gc, ref, C)


def test_autograd_expanded_leaf_receives_the_sum_over_images(gpu_device):
    """The kernel sees stride(0) == 0 and writes per-image gradients; autograd's expand adds them: one more fp32 add per image, which the
    bound of the summed element ((sum of k) + (n - 1) + 4) * 2^-24 * (sum of A) covers."""
    from dnnlib import util
    n, C, H, m, planes, go, co = _wrapper_inputs()
    one = planes[:1]
    ref = triplane_ref.triplane_backward_ref(go, one.expand(n, -1, -1, -1).contiguous(), co)
    leaf = _channels_last(one, gpu_device).requires_grad_(True)
    grid = leaf.expand(n, -1, -1, -1)
    assert grid.stride(0) == 0 and grid.stride(1) == 1
    cc = co.to(gpu_device).requires_grad_(True)
    before = _calls('triplane_sample_backward')
    out = util.sample_from_triplane(cc, grid, ray_grid=False)
    gp, gc = torch.autograd.grad(out, [leaf, cc], grad_outputs=go.to(gpu_device))
    assert _calls('triplane_sample_backward') == before + 1
    assert gp.shape == leaf.shape
    summed = ref._replace(grad_planes=ref.grad_planes.sum(0, keepdim=True), abs_planes=ref.abs_planes.sum(0, keepdim=True),
                          cnt_planes=ref.cnt_planes.sum(0, keepdim=True) + (n - 1) * (ref.cnt_planes.sum(0, keepdim=True) > 0))
    _compare('autograd, expanded leaf', gp, gc, summed, C)


def test_autograd_planes_only(gpu_device):
    """Coordinates that need no gradient: the kernel gets a null grad_coords and the plane gradient is the same."""
    from dnnlib import util
    from torch_utils import hip_plugin
    n, C, H, m, planes, go, co = _wrapper_inputs()
    ref = triplane_ref.triplane_backward_ref(go, planes, co)
    leaf = _channels_last(planes, gpu_device).requires_grad_(True)
    before = _calls('triplane_sample_backward')
    out = util.sample_from_triplane(co.to(gpu_device), leaf, ray_grid=False)
    gp, = torch.autograd.grad(out, [leaf], grad_outputs=go.to(gpu_device))
    assert _calls('triplane_sample_backward') == before + 1
    _compare('autograd, planes only', gp, None, ref, C)
    gp2, none = hip_plugin.TriplanePlugin.sample_backward(go.to(gpu_device), leaf.detach(), co.to(gpu_device), False)
    assert none is None
    _compare('plugin, grad_coords == nullptr', gp2, None, ref, C)
    gp3, gc3 = _backward(gpu_device, go, leaf.detach(), co)
    _compare('plugin, with grad_coords', gp3, gc3, ref, C)


# ---- adjoint identity at a production-like size ------------------------------------------------------------------------------------

def test_adjoint_identity_at_production_size(gpu_device):
    """<sample(P, c), G> = <P, grad_planes(G, c)>: both are the sum of the same N <= 12 * C * n * m terms t = P * w * G (3 planes, 4 taps),
    and need no reference.  Both inner products are accumulated in float64, so what separates them is the fp32 rounding inside the two
    kernels: a term of the forward sees at most 9 roundings (two fractions, their product, four FMAs of the tap blend, two adds of the
    plane sum), a term of the backward k + 3 (the plane-gradient bound above, K = the largest k of any texel).  Hence

        |lhs - rhs| <= sum_t (K + 12) * 2^-24 * |t| <= (12 * C * n * m)^(1/2) * 2^-23 * (K + 12) / 2 * (sum_t t^2)^(1/2)

    by Cauchy-Schwarz, and sum_t t^2 <= sum_t w * P^2 * G^2 = <sample(P^2, c), G^2> because 0 <= w <= 1; that last inner product comes from
    ATen's float64 CPU grid_sample.  A mis-strided or dropped tap changes one side by the order of (sum_t t^2)^(1/2) itself, more than three
    orders above the bound.  The plane gradient is also compared with the float64 reference on every 997th texel."""
    from dnnlib import util
    from torch_utils import hip_plugin
    n, C, H, m = 2, 32, 256, 16 * 16 * 24
    g = torch.Generator().manual_seed(71)
    planes = torch.randn(n, 3 * C, H, H, generator=g)
    go = torch.randn(n * m, C, generator=g)
    co = ((torch.rand(n, m, 3, generator=g) * 2 - 1) * 0.7)
    P = _channels_last(planes, gpu_device)
    out = hip_plugin.TriplanePlugin.sample(P, co.to(gpu_device))
    gp, gc = _backward(gpu_device, go, P, co)
    lhs = float((out.double() * go.to(gpu_device).double()).sum())
    rhs = float((P.double() * gp.double()).sum())
    ref = triplane_ref.triplane_backward_ref(go, planes, co)
    K = int(ref.cnt_planes.max())
    sq = float((util._sample_from_triplane_ref(co.double(), planes.double() ** 2) * go.double() ** 2).sum())
    bound = math.sqrt(12 * C * n * m) * 2.0 ** -23 * (K + 12) / 2 * math.sqrt(sq)
    print(f'triplane-grad adjoint: lhs {lhs:.6f} rhs {rhs:.6f} |diff| {abs(lhs - rhs):.3e} bound {bound:.3e} ratio {abs(lhs - rhs) / bound:.2e}'
          f' (K {K}, (sum t^2)^(1/2) <= {math.sqrt(sq):.1f})')
    assert abs(lhs - rhs) <= bound
    sub = slice(None, None, 997)
    pick = lambda x: x.reshape(-1)[sub]
    picked = ref._replace(grad_planes=pick(ref.grad_planes), abs_planes=pick(ref.abs_planes), cnt_planes=pick(ref.cnt_planes))
    assert int((picked.cnt_planes > 0).sum()) > 1000
    assert bool(torch.isfinite(gp).all())
    _compare('production size, every 997th texel', pick(gp.cpu().contiguous()), gc, picked, C)
