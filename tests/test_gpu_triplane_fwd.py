"""The forward tri-plane gather - every flat kernel of csrc/triplane.hip (`triplane_sample_cl2_kernel<LPS>`, `triplane_sample_cl_kernel<LPS>`,
`triplane_sample_strided_kernel`) and the ray-grid kernel of csrc/triplane_tile.hip with each of its eight blend variants - against the
float64 definition `triplane_ref.triplane_forward_ref`, at the shapes, layouts and coordinates where each line of them can go wrong.
Needs a real MI355X: `pytest -m gpu`.

The bound is derived, per element, from the sum the kernels form (u = 2^-24, one rounding to nearest):

    |got - ref| <= 12 * 2^-24 * A + 1e-30,      A = sum of |v * w| over the in-bounds taps of the three planes

  * a term v * (fx * fy): both fractions come from one subtraction each ((floor(u) + 1) - u and u - floor(u): exact, or rounded once), their
    product rounds once, the product with v once (or not at all where it is contracted into the accumulation): at most 4 roundings;
  * the four accumulations of a plane each round a partial sum that is at most A_plane: 4 more, and the A_plane add up to A;
  * two additions join the three planes, each rounding a partial sum of at most A: 2 more;
  * 4 + 4 + 2 = 10, and a margin of 2 for the second-order terms, as in `plane_bound`.  1e-30 is for sums that end below the normal range.

The reference takes the tap position from the tap index contract (float32, `triplane_ref.unnormalize32`) and does everything after it in
float64, so a swapped axis, a stale table, a dropped tap or a wrong stride is an error of the order of A: five orders above the bound.
Rows without a tap in bounds must be exactly 0.  A non-finite coordinate contributes nothing: the planes that read it add exactly nothing,
and the row comes out with the bits it has when that coordinate is +-1e30 instead (far outside: no tap either).  The plane that does not
read the coordinate still contributes, as it does in ATen - only rows in which every plane reads a non-finite coordinate are all zero.
Plane values are finite throughout: the kernels load clamped texels unconditionally and multiply by a zero weight, so an inf texel beside an
out-of-plane tap would give NaN (gather section).

Which kernel a call reaches cannot be seen from its result - all forms are bit-equal by design - so the tests restate the host's routing
conditions (`triplane_cases.flat_route`, `triplane_cases.tile_accepts`: line by line from `ide3d_triplane_sample`, `launch_cl2` and
`launch_triplane_tile`) and assert the route each shape was made for; the launch counters show that the native entry point ran.  Which blend
variant the ray-grid kernel took per chunk comes from the device itself: `TriplanePlugin.tile_masks` runs the kernel's own `axis_index`,
`wave_reduce_pk4` and `build_region_table`, and every ray-grid case asserts hook == host model (`triplane_ref.staged_masks`) == the masks
the case was constructed for.

Every test prints its worst error / bound.
"""

import collections

import pytest
import torch

import triplane_cases
import triplane_ref
from triplane_ref import NONFINITE, edges as _edges

pytestmark = pytest.mark.gpu

C_TILE = 32          # the only channel count of the ray-grid kernel


def _calls(name):
    from torch_utils import hip_plugin
    return hip_plugin.CALLS.get(name, 0)


def _uniform(g, n, m):
    return (torch.rand(n, m, 3, generator=g) * 2 - 1) * 1.1


def _channels_last(x, device):
    """A copy of x [n, c, H, W] on `device` with element strides (H * W * c, 1, W * c, c), spelled out: `contiguous(memory_format=...)`
    leaves the strides of size-1 dimensions to chance."""
    n, c, H, W = x.shape
    return torch.empty_strided((n, c, H, W), (H * W * c, 1, W * c, c), dtype=x.dtype, device=device).copy_(x)


def _insert_nonfinite(g, co):
    """Overwrites len(NONFINITE) random rows; returns how many."""
    flat = co.reshape(-1, 3)
    if flat.shape[0] < 20:
        return 0
    rows = torch.randperm(flat.shape[0], generator=g)[:len(NONFINITE)]
    flat[rows] = torch.tensor(NONFINITE)
    return len(NONFINITE)


def _sample(planes_dev, co, gpu_device, ray_grid=None):
    from torch_utils import hip_plugin
    which = 'triplane_sample' if ray_grid is None else 'triplane_sample_rays'
    before = _calls(which)
    out = hip_plugin.TriplanePlugin.sample(planes_dev, co.to(gpu_device), ray_grid=ray_grid)
    assert _calls(which) == before + 1
    return out


def _compare(name, got, planes, co, inserted_nonfinite=0, ref=None):
    """`planes`: the materialised [n, 3C, H, W] tensor the kernel was given a view of."""
    out, A, hit, finite = ref if ref is not None else triplane_ref.triplane_forward_ref(planes, co)
    g64 = got.detach().cpu().double()
    assert g64.shape == out.shape and got.dtype == torch.float32
    assert bool(torch.isfinite(g64).all()), f'{name}: non-finite output'
    left = int((~finite).sum())
    assert left == inserted_nonfinite, f'{name}: {left} non-finite rows, {inserted_nonfinite} inserted'
    dead = (~hit).reshape(-1)
    assert bool((g64[dead] == 0).all()), f'{name}: a row with no tap in bounds is not exactly 0'
    ratio = float(((g64 - out).abs() / triplane_ref.forward_bound(A)).max())
    print(f'triplane-fwd {name}: worst error / bound {ratio:.3f} over {out.numel()} elements; rows without a tap: {int(dead.sum())},'
          f' with a non-finite coordinate: {left}')
    assert ratio <= 1.0, f'{name}: {ratio:.3f} x the bound'
    return ratio


def _nonfinite_is_far_outside(sample, co, got):
    """A non-finite coordinate contributes exactly what a coordinate with no tap in bounds contributes: the same bits."""
    far = torch.nan_to_num(co, nan=1e30, posinf=1e30, neginf=-1e30)
    assert torch.equal(sample(far), got), 'a non-finite coordinate changed more than its own planes'


def _planes_coords(seed, n, C, H, W, m, kind):
    g = torch.Generator().manual_seed(seed)
    planes = torch.randn(n, 3 * C, H, W, generator=g)
    if kind == 'uniform':
        co = _uniform(g, n, m)
    elif kind == 'edges':
        co = _edges(g, n, m, H, W)
    else:
        co = torch.cat([_uniform(g, n, m // 2), _edges(g, n, m - m // 2, H, W)], dim=1).contiguous()
    return planes, co, _insert_nonfinite(g, co)


def _route(planes_dev, m):
    return triplane_cases.flat_route(tuple(planes_dev.shape), tuple(planes_dev.stride()), planes_dev.data_ptr(), m)


# ---- flat kernels: each shape exists for one line of code ------------------------------------------------------------------------------

CL2_SHAPES = [
    (1, 4, 1, 1, 1),            # cl2<1>: one row, single-texel planes
    (2, 4, 5, 9, 77),           # cl2<1>: odd m, the image boundary falls inside a wave; H != W
    (3, 8, 9, 5, 129),          # cl2<2>: two image boundaries, rows % 64 != 0
    (2, 16, 6, 11, 200),        # cl2<4>
    (1, 32, 16, 16, 333),       # cl2<8>: the generator's channel count, two workgroups
    (2, 64, 7, 4, 65),          # cl2<16>
    (1, 128, 4, 6, 70),         # cl2<32>
    (1, 256, 3, 5, 40),         # cl2<64>: one sample per round, a partial wave
]


@pytest.mark.parametrize('kind', ['uniform', 'edges'])
@pytest.mark.parametrize('n,C,H,W,m', CL2_SHAPES, ids=lambda v: str(v))
def test_flat_cl2_every_lane_count(gpu_device, n, C, H, W, m, kind):
    planes, co, bad = _planes_coords(1000 + C + m, n, C, H, W, m, kind)
    dev = _channels_last(planes, gpu_device)
    assert dev.stride() == (3 * C * H * W, 1, 3 * C * W, 3 * C) and _route(dev, m) == 'cl2'
    got = _sample(dev, co, gpu_device)
    _compare(f'cl2<{C // 4}> n{n} C{C} {H}x{W} m{m} {kind}', got, planes, co, bad)
    _nonfinite_is_far_outside(lambda c: _sample(dev, c, gpu_device), co, got)


def test_flat_cl2_second_trip_of_the_base_loop(gpu_device):
    """400 001 rows over 1536 workgroups round up to 512 rows per workgroup: every wave runs its `base` loop twice, the last workgroup ends
    inside a wave."""
    n, C, H, W, m = 1, 4, 8, 8, 400001
    cdiv = lambda a, b: -(-a // b)
    assert cdiv(cdiv(n * m, 256 * 6), 256) * 256 == 512
    planes, co, bad = _planes_coords(1101, n, C, H, W, m, 'both')
    dev = _channels_last(planes, gpu_device)
    assert _route(dev, m) == 'cl2'
    _compare('cl2<1> rows_per_block 512', _sample(dev, co, gpu_device), planes, co, bad)


@pytest.mark.parametrize('kind', ['uniform', 'edges'])
@pytest.mark.parametrize('n,C,H,W,m,layout', [
    (2, 12, 5, 7, 90, 'channels_last'),          # C / 4 = 3 does not divide 64: strided kernel despite the unit channel stride
    (1, 20, 4, 4, 50, 'channels_last'),          # C / 4 = 5
    (2, 3, 5, 9, 70, 'nchw'),                    # a partial 32-channel chunk; C no multiple of 4
    (1, 33, 6, 4, 300, 'nchw'),                  # a second chunk of one channel; two workgroups
    (2, 65, 4, 7, 50, 'nchw'),                   # a third chunk
], ids=lambda v: str(v))
def test_flat_strided_kernel(gpu_device, n, C, H, W, m, layout, kind):
    planes, co, bad = _planes_coords(1200 + C + m, n, C, H, W, m, kind)
    dev = _channels_last(planes, gpu_device) if layout == 'channels_last' else planes.to(gpu_device).contiguous()
    assert dev.stride(1) == (1 if layout == 'channels_last' else H * W) and _route(dev, m) == 'strided'
    got = _sample(dev, co, gpu_device)
    _compare(f'strided {layout} n{n} C{C} {H}x{W} m{m} {kind}', got, planes, co, bad)
    _nonfinite_is_far_outside(lambda c: _sample(dev, c, gpu_device), co, got)


def test_flat_strided_second_grid_stride_trip(gpu_device):
    """600 000 rows > 2048 workgroups x 256: the first 75 712 rows' workgroups come round again, across the image boundary at 300 000."""
    n, C, H, W, m = 2, 2, 4, 4, 300000
    assert n * m > 2048 * 256
    planes, co, bad = _planes_coords(1301, n, C, H, W, m, 'both')
    dev = planes.to(gpu_device).contiguous()
    assert _route(dev, m) == 'strided'
    _compare('strided, second grid-stride trip', _sample(dev, co, gpu_device), planes, co, bad)


def _layout_inputs():
    n, C, H, W, m = 2, 32, 9, 13, 150
    g = torch.Generator().manual_seed(1401)
    wide = torch.randn(n, 128, H, W + 5, generator=g)
    store = torch.randn(3 * C * H * W * (n + 1) // 2, generator=g)
    co = torch.cat([_uniform(g, n, m // 2), _edges(g, n, m - m // 2, H, W)], dim=1).contiguous()
    return n, C, H, W, m, wide, store, co, _insert_nonfinite(g, co)


@pytest.mark.parametrize('layout', ['expanded', 'overlapping', 'channel slice', 'w slice'])
def test_flat_layouts(gpu_device, layout):
    """`launch_cl2` declines an image stride <= 0 and images that overlap (H * s[2] * 4 > image stride in bytes: its buffer resource is
    sized by the image stride): the expanded and the overlapping planes therefore run the v1 kernel `triplane_sample_cl_kernel<8>`, which
    nothing else here reaches.  The two slices stay on cl2 with a pixel stride / row pitch that no dense tensor has."""
    n, C, H, W, m, wide, store, co, bad = _layout_inputs()
    if layout == 'expanded':
        dev = _channels_last(wide[:1, :96, :, :W], gpu_device).expand(n, -1, -1, -1)
        assert dev.stride(0) == 0 and dev.stride(1) == 1
        want_route = 'cl'
    elif layout == 'overlapping':             # image 1 starts in the middle of image 0
        half = 3 * C * H * W // 2
        dev = store.to(gpu_device).as_strided((n, 3 * C, H, W), (half, 1, 3 * C * W, 3 * C))
        assert half % 4 == 0 and H * dev.stride(2) > dev.stride(0)
        want_route = 'cl'
    elif layout == 'channel slice':
        dev = _channels_last(wide[..., :W], gpu_device)[:, :96]
        assert dev.stride() == (128 * H * W, 1, 128 * W, 128)
        want_route = 'cl2'
    else:
        dev = _channels_last(wide[:, :96], gpu_device)[..., 2:2 + W]
        assert dev.stride() == (96 * H * (W + 5), 1, 96 * (W + 5), 96) and dev.data_ptr() % 16 == 0
        want_route = 'cl2'
    assert _route(dev, m) == want_route
    planes = dev.cpu().contiguous()          # the materialised tensor
    got = _sample(dev, co, gpu_device)
    _compare(f'layout {layout} ({want_route}), strides {tuple(dev.stride())}', got, planes, co, bad)
    _nonfinite_is_far_outside(lambda c: _sample(dev, c, gpu_device), co, got)
    dense = _channels_last(planes, gpu_device)
    assert _route(dense, m) == 'cl2' and torch.equal(_sample(dense, co, gpu_device), got)          # v1 and v2, views and copies: one arithmetic


# ---- the ray-grid kernel -----------------------------------------------------------------------------------------------------------------

MASKS_RUN = collections.Counter()          # mask -> chunks, as the device reported them, over the ray-grid tests of this module


def _ray_grid(gpu_device, name, dev, case, bad=0, tile=True):
    """The four assertions of a ray-grid case; `dev` is any view, its materialised copy is the reference's input."""
    from torch_utils import hip_plugin
    co, rg, H, W = case['coords'], case['ray_grid'], case['H'], case['W']
    assert tuple(dev.shape) == (case['n'], 3 * C_TILE, H, W)
    assert triplane_cases.tile_accepts(tuple(dev.shape), tuple(dev.stride()), dev.data_ptr(), rg) == tile
    tiled = _sample(dev, co, gpu_device, ray_grid=rg)                                   # 1. the entry point ran (counter inside)
    if tile:                                                                            # 2. the device's own table code == the host model
        model = triplane_ref.staged_masks(co, H, W, rg)
        hook = hip_plugin.TriplanePlugin.tile_masks(H, W, co.to(gpu_device), rg).cpu().long()
        assert torch.equal(hook, model), f'{name}: device masks {hook.flatten().tolist()} != host model {model.flatten().tolist()}'
        assert torch.equal(model, case['want']), f'{name}: not the variants the case was made for'
        MASKS_RUN.update(hook.flatten().tolist())
        seen = dict(sorted(collections.Counter(hook.flatten().tolist()).items()))
        print(f'triplane-fwd {name}: chunks per mask {seen}, (segments, chunks per workgroup) {triplane_ref.tile_plan(case["n"], *rg)}')
    flat = _sample(dev, co, gpu_device)
    assert torch.equal(tiled, flat), f'{name}: not bit-equal to the flat kernel'         # 3.
    planes = dev.cpu().contiguous()
    _compare(name, tiled, planes, co, bad)                                              # 4.
    return tiled


def _tile_planes(seed, n, H, W, gpu_device):
    g = torch.Generator().manual_seed(seed)
    return _channels_last(torch.randn(n, 3 * C_TILE, H, W, generator=g), gpu_device)


def test_ray_grid_every_blend_variant(gpu_device):
    """Sixteen workgroups of one chunk: every mask 0..7 by construction, the three-way tie, oversized and outside boxes; H != W, so plane 1
    reading y on H or z on W lands on other texels."""
    case = triplane_cases.variants_case()
    assert triplane_ref.tile_plan(case['n'], *case['ray_grid']) == (2, 1)
    _ray_grid(gpu_device, 'variants 48x64', _tile_planes(1501, case['n'], case['H'], case['W'], gpu_device), case)
    assert set(triplane_ref.staged_masks(case['coords'], case['H'], case['W'], case['ray_grid']).flatten().tolist()) == set(range(8))


def test_ray_grid_hand_over_between_unlike_chunks(gpu_device):
    """256 workgroups of four chunks: chunks k + 2, k + 1, k share two line buffers, two tap tables and two region tables, and here they
    differ in mask, box origin and box size (tests/test_triplane_ref_cpu.py lists the transitions), so a table read from the wrong buffer
    or one iteration late gives other texels."""
    case = triplane_cases.handover_case()
    assert triplane_ref.tile_plan(case['n'], *case['ray_grid']) == (4, 4)
    _ray_grid(gpu_device, 'hand-over 40x56', _tile_planes(1502, case['n'], case['H'], case['W'], gpu_device), case)


@pytest.mark.parametrize('H,W', [(5, 9), (9, 5)])
def test_ray_grid_edge_coordinates_on_planes_smaller_than_a_footprint(gpu_device, H, W):
    case = triplane_cases.edge_grid_case(H, W)
    dev = _tile_planes(1503 + H, case['n'], H, W, gpu_device)
    tiled = _ray_grid(gpu_device, f'edges {H}x{W}', dev, case, bad=len(NONFINITE))
    _nonfinite_is_far_outside(lambda c: _sample(dev, c, gpu_device, ray_grid=case['ray_grid']), case['coords'], tiled)


@pytest.mark.parametrize('layout', ['channel slice', 'w slice', 'rays 8x24', 'rays 24x8'])
def test_ray_grid_layouts(gpu_device, layout):
    """A pixel stride of 128 floats (> 96), a row pitch that is not W pixels, and ray grids with rays_w != rays_h; all with staged and
    unstaged planes in neighbouring chunks."""
    n, H, W = 2, 20, 28
    g = torch.Generator().manual_seed(1601)
    wide = torch.randn(n, 128, H, W + 5, generator=g)
    if layout == 'channel slice':
        case = triplane_cases.mixed_case(313, n, H, W, (16, 16, 8))
        dev = _channels_last(wide[..., :W], gpu_device)[:, :96]
        assert dev.stride() == (128 * H * W, 1, 128 * W, 128)
    elif layout == 'w slice':
        case = triplane_cases.mixed_case(313, n, H, W, (16, 16, 8))
        dev = _channels_last(wide[:, :96], gpu_device)[..., 2:2 + W]
        assert dev.stride() == (96 * H * (W + 5), 1, 96 * (W + 5), 96)
    else:
        case = triplane_cases.mixed_case(311 if layout == 'rays 8x24' else 312, n, H, W, (8, 24, 8) if layout == 'rays 8x24' else (24, 8, 8))
        dev = _channels_last(wide[:, :96, :, :W], gpu_device)
    _ray_grid(gpu_device, f'layout {layout}', dev, case)


def test_ray_grid_single_texel_planes(gpu_device):
    n, rg = 2, (16, 8, 8)
    g = torch.Generator().manual_seed(1701)
    co = _uniform(g, n, rg[0] * rg[1] * rg[2]) * 2
    bad = _insert_nonfinite(g, co)
    dev = torch.randn(n, 1, 1, 3 * C_TILE, generator=g).to(gpu_device).as_strided((n, 3 * C_TILE, 1, 1), (96, 1, 96, 96))
    case = dict(n=n, H=1, W=1, coords=co, ray_grid=rg, want=torch.zeros(n, 2, 2, dtype=torch.int64))
    _ray_grid(gpu_device, 'single-texel planes', dev, case, bad=bad)


def test_ray_grid_the_kernel_refuses_returns_the_flat_kernels_bits(gpu_device):
    n, H, W, rg = 2, 20, 28, (12, 20, 6)
    g = torch.Generator().manual_seed(1801)
    co = _uniform(g, n, rg[0] * rg[1] * rg[2])
    case = dict(n=n, H=H, W=W, coords=co, ray_grid=rg)
    _ray_grid(gpu_device, 'refused grid 12x20x6', _tile_planes(1802, n, H, W, gpu_device), case, tile=False)


def test_ray_grid_every_mask_was_reported_by_the_device(gpu_device):
    """Sums up what the hook reported in this module; on its own it runs the variants case."""
    if not MASKS_RUN:
        test_ray_grid_every_blend_variant(gpu_device)
    print(f'triplane-fwd chunks per blend variant, as the device reported them: {dict(sorted(MASKS_RUN.items()))}')
    assert set(MASKS_RUN) == set(range(8))
