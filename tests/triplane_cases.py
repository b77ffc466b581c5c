"""Inputs of the forward gather suite (tests/test_gpu_triplane_fwd.py) that have to be *constructed*: ray grids whose chunks make the
ray-grid kernel (csrc/triplane_tile.hip) take a prescribed blend variant, and the host-side restatement of which kernel a call reaches.
tests/test_triplane_ref_cpu.py checks the constructions against the host model of tests/triplane_ref.py without a GPU; the GPU suite checks
the host model against the device's own table code (`TriplanePlugin.tile_masks`).

A chunk is 8 x 8 rays x 4 depth steps.  Its coordinates are drawn per world axis from an interval given in tap positions (texels): x and y
on the W scale, z on the H scale; y also feeds plane 0's H axis, where the same interval is H / W times as long.  The two ends of each
interval sit on samples picked at random among the 256, so the box is only right if the reduction sees every lane of every wave.

  kind      x      y      z       staged planes (mask)
  'all'     small  small  small   7
  'p0'      small  small  border  1     z leaves the plane: planes 1 and 2 (both read z) cannot be staged
  'p1'      border small  small   2
  'p2'      small  border small   4
  'p01'     large  small  large   3     plane 2 = (x, z) is oversized (> 320 lines); the other two fit together
  'p02'     small  large  large   5     plane 1 = (y, z) is oversized (> 256 lines)
  'p12'     large  large  small   6     plane 0 = (x, y) is oversized
  'big'     huge   huge   huge    0     every plane oversized, every tap in bounds
  'out'     beyond the plane      0     no tap in bounds
  'tie'     13     13     10      3     every plane fits alone (184 lines each), the three do not fit together (552 > 504), every pair costs
                                        368: the first pair wins.  Only where H / W = 3 / 4 (y: 13 texels on W are 10 on H)
"""

import torch

import triplane_ref

MASK_OF = {'all': 7, 'p0': 1, 'p1': 2, 'p2': 4, 'p01': 3, 'p02': 5, 'p12': 6, 'big': 0, 'out': 0, 'tie': 3}


def _interval(g, size, what):
    """[lo, hi] in tap positions on an axis of `size` texels; both ends keep 0.3 of a texel away from a texel border."""
    rnd = lambda a, b: a + int(torch.randint(0, max(b - a, 0) + 1, (), generator=g))
    if what == 'border':
        return -0.4, 1.7 + rnd(0, 1)
    if what == 'out':
        return size + 5.3, size + 7.7
    span = {'small': rnd(1, 3), 'large': rnd(22, 24), 'huge': 30, 't13': 13, 't10': 10}[what]
    lo = rnd(0, size - 2 - span)
    return lo + 0.3, lo + span + 0.7


_KINDS = {'all': ('small', 'small', 'small'), 'p0': ('small', 'small', 'border'), 'p1': ('border', 'small', 'small'),
          'p2': ('small', 'border', 'small'), 'p01': ('large', 'small', 'large'), 'p02': ('small', 'large', 'large'),
          'p12': ('large', 'large', 'small'), 'big': ('huge', 'huge', 'huge'), 'out': ('out', 'out', 'out')}


def chunk_coords(g, kind, H, W):
    """[256, 3] float32 coordinates of one chunk, sample t = (ray t >> 2 of the 8 x 8 tile, depth step t & 3)."""
    if kind == 'tie':
        assert H * 4 == W * 3
        ivs = [_interval(g, W, 't13'), (8.3, 21.7), _interval(g, H, 't10')]          # y: 13 texels on W, floor(6.1) .. floor(16.15) = 10 on H
    else:
        ivs = [_interval(g, size, what) for size, what in zip((W, W, H), _KINDS[kind])]
    co = torch.empty(256, 3, dtype=torch.float64)
    for axis, ((lo, hi), size) in enumerate(zip(ivs, (W, W, H))):
        u = lo + (hi - lo) * torch.rand(256, generator=g, dtype=torch.float64)
        ends = torch.randperm(256, generator=g)[:2]
        u[ends[0]], u[ends[1]] = lo, hi
        co[:, axis] = (2.0 * u + 1.0) / size - 1.0
    return co.float()


def ray_grid_coords(g, kinds, H, W):
    """kinds: nested lists [n][tiles_y][tiles_x][chunks] of chunk kinds -> (coords [n, rays_h * rays_w * steps, 3], ray_grid,
    expected masks int64 [n, tiles, chunks])."""
    n, ty, tx, ch = len(kinds), len(kinds[0]), len(kinds[0][0]), len(kinds[0][0][0])
    co = torch.empty(n, ty, tx, ch, 8, 8, 4, 3)
    want = torch.empty(n, ty, tx, ch, dtype=torch.int64)
    for i in range(n):
        for a in range(ty):
            for b in range(tx):
                for c in range(ch):
                    co[i, a, b, c] = chunk_coords(g, kinds[i][a][b][c], H, W).reshape(8, 8, 4, 3)
                    want[i, a, b, c] = MASK_OF[kinds[i][a][b][c]]
    rg = (ty * 8, tx * 8, ch * 4)
    co = co.permute(0, 1, 4, 2, 5, 3, 6, 7).reshape(n, rg[0] * rg[1] * rg[2], 3).contiguous()
    return co, rg, want.reshape(n, ty * tx, ch)


def _nest(flat, n, ty, tx, ch):
    it = iter(flat)
    return [[[[next(it) for _ in range(ch)] for _ in range(tx)] for _ in range(ty)] for _ in range(n)]


def variants_case():
    """Planes 48 x 64, n = 2, rays 16 x 16, steps 8: 16 chunks, one workgroup each (`tile_plan` -> 2 segments of one chunk); every mask
    0..7 and the three-way tie."""
    H, W = 48, 64
    kinds = ['all', 'big', 'p0', 'p1', 'p2', 'p01', 'p02', 'p12', 'tie', 'out', 'p12', 'p02', 'p01', 'p2', 'p1', 'p0']
    co, rg, want = ray_grid_coords(torch.Generator().manual_seed(301), _nest(kinds, 2, 2, 2, 2), H, W)
    return dict(H=H, W=W, n=2, coords=co, ray_grid=rg, want=want, kinds=kinds)


# what one workgroup (four consecutive chunks) sees in the hand-over case: neighbouring chunks differ in mask, and every chunk draws its own
# box origin and size
HANDOVER_SEQUENCES = (('all', 'big', 'all', 'p0'), ('p0', 'all', 'p1', 'all'), ('all', 'p2', 'all', 'out'), ('out', 'all', 'p01', 'p02'),
                      ('p12', 'p01', 'all', 'p1'), ('p2', 'all', 'big', 'all'), ('p02', 'p12', 'p2', 'p12'))


def handover_case():
    """Planes 40 x 56, n = 4, rays 32 x 32, steps 64: `tile_plan` -> 4 segments of 4 chunks, 256 workgroups.  Workgroup k (image, tile,
    segment) runs sequence k % 7 of HANDOVER_SEQUENCES."""
    H, W, n = 40, 56, 4
    kinds = [k for wg in range(n * 16 * 4) for k in HANDOVER_SEQUENCES[wg % len(HANDOVER_SEQUENCES)]]
    co, rg, want = ray_grid_coords(torch.Generator().manual_seed(302), _nest(kinds, n, 4, 4, 16), H, W)
    return dict(H=H, W=W, n=n, coords=co, ray_grid=rg, want=want, kinds=kinds)


def mixed_case(seed, n, H, W, ray_grid):
    """A ray grid of any tile shape on planes too small for the oversized kinds: 'all', the three single planes and 'out' in rotation,
    shifted per tile so that tiles differ."""
    rh, rw, steps = ray_grid
    ty, tx, ch = rh // 8, rw // 8, steps // 4
    rot = ('all', 'p0', 'p1', 'all', 'p2', 'out')
    kinds = [rot[(i * 5 + t * 2 + c) % len(rot)] for i in range(n) for t in range(ty * tx) for c in range(ch)]
    co, rg, want = ray_grid_coords(torch.Generator().manual_seed(seed), _nest(kinds, n, ty, tx, ch), H, W)
    assert rg == tuple(ray_grid)
    return dict(H=H, W=W, n=n, coords=co, ray_grid=rg, want=want, kinds=kinds)


def edge_grid_case(H, W):
    """All `edges` combinations (5488 at H != W) plus the NONFINITE rows laid into 2 x (16 x 24 rays x 8 steps).  The planes are smaller
    than a footprint, so no chunk can stage anything."""
    g = torch.Generator().manual_seed(303 + H)
    n, rg = 2, (16, 24, 8)
    m = rg[0] * rg[1] * rg[2]
    co = triplane_ref.edges(g, n, m, H, W)
    rows = torch.randperm(n * m, generator=g)[:len(triplane_ref.NONFINITE)]
    co.reshape(-1, 3)[rows] = torch.tensor(triplane_ref.NONFINITE)
    return dict(H=H, W=W, n=n, coords=co, ray_grid=rg, want=torch.zeros(n, 6, 2, dtype=torch.int64), nonfinite_rows=rows)


# ---- which kernel a call reaches: the host code of csrc/triplane.hip and `launch_triplane_tile`, restated ---------------------------------

def flat_route(shape, stride, data_ptr, m):
    """'cl2' | 'cl' | 'strided' for `ide3d_triplane_sample` on planes of this shape / element strides / address (the output comes from
    torch's allocator and is 16-byte aligned)."""
    n, c3, H, W = shape
    C = c3 // 3
    s = stride
    cl = (s[1] == 1 and C % 4 == 0 and s[0] % 4 == 0 and s[2] % 4 == 0 and s[3] % 4 == 0 and s[2] > 0 and s[3] > 0
          and s[2] * H < 0x7fffffff and s[3] * W < 0x7fffffff and data_ptr % 16 == 0)
    lps = C // 4
    if not (cl and 1 <= lps <= 64 and 64 % lps == 0):
        return 'strided'
    sn = s[0] * 4
    if m <= 0 or m >= 2 ** 31 or sn <= 0 or sn >= 2 ** 31 or H * s[2] * 4 > sn:
        return 'cl'                      # launch_cl2 declines: no image stride to bound a buffer resource with, or images that overlap
    return 'cl2'


def tile_accepts(shape, stride, data_ptr, ray_grid):
    """Whether `ide3d_triplane_sample_rays` runs the ray-grid kernel (else it hands the call to `ide3d_triplane_sample`)."""
    n, c3, H, W = shape
    rh, rw, steps = ray_grid
    s = stride
    if data_ptr % 16 or s[0] % 4 or s[2] % 4 or s[3] % 4:
        return False
    if c3 != 96 or rh % 8 or rw % 8 or steps % 4 or H > 0x7fff or W > 0x7fff:
        return False
    if s[1] != 1 or s[3] < 96 or s[2] <= 0:
        return False
    sn = s[0] * 4
    return 0 < sn < 2 ** 31 and H * s[2] * 4 <= sn and n * rh * rw * steps < 2 ** 31
