"""Float64 definitions of the tri-plane gather (csrc/triplane.hip, csrc/triplane_tile.hip), plain torch on the CPU: its backward
(`triplane_backward_ref`), its forward (`triplane_forward_ref`) and an integer model of the decisions the ray-grid kernel takes per chunk
(`tile_plan`, `staged_masks`), plus the edge coordinate sets both GPU suites use.

The gradient with respect to the coordinates is piecewise constant in the texel, so a reference must not disagree with the kernel about
which texel a sample is in.  The tap position therefore comes from the project's own contract (DESIGN.md "tap index contract",
`test_triplane_tap_indices_bit_exact`): u = ((c + 1) * size - 1) / 2 in float32 as separate add, mul, sub, mul(0.5) operations.
Everything after it - floor, fractions, weights, zero-padding masks, the scatter and the coordinate gradient - is float64.

Plane p reads (u from a -> W, v from b -> H): p0 = (x, y), p1 = (y, z), p2 = (x, z).
"""

import collections
import itertools

import torch

PLANE_AXES = ((0, 1), (1, 2), (0, 2))          # (coordinate that feeds u, coordinate that feeds v) per plane

TriplaneGrad = collections.namedtuple('TriplaneGrad', [
    'grad_planes',          # [n, 3C, H, W] float64
    'grad_coords',          # [n, m, 3] float64
    'abs_planes',           # A: sum of |go * w| over the terms added into each texel
    'cnt_planes',           # k: their number (int64)
    'abs_coords',           # A: sum of |go * (difference of taps) * fraction| * size / 2 over the terms added into each coordinate
    'cnt_coords',           # k: their number (int64)
    'finite',               # [n, m] bool: the sample's coordinates (and its tap positions) are finite
    'hit',                  # [n, m] bool: at least one tap of one plane is in bounds
])


def unnormalize32(c, size):
    """The tap position of the contract: float32, one rounding per operation."""
    c = c.to(torch.float32)
    return torch.mul(torch.sub(torch.mul(torch.add(c, 1.0), float(size)), 1.0), 0.5)


def taps(coords, H, W):
    """Per plane: floor(u), floor(v), the fractions bx = u - floor(u), by = v - floor(v) (float64, from the float32 position) and the
    in-bounds masks of the four taps (nw, ne, sw, se).  Samples with a non-finite position have every mask False and fractions 0."""
    res = []
    for a, b in PLANE_AXES:
        u = unnormalize32(coords[..., a], W).double()
        v = unnormalize32(coords[..., b], H).double()
        ok = torch.isfinite(u) & torch.isfinite(v)
        u = torch.where(ok, u, torch.zeros_like(u))
        v = torch.where(ok, v, torch.zeros_like(v))
        fu, fv = torch.floor(u), torch.floor(v)
        x0 = (fu >= 0) & (fu < W) & ok
        x1 = (fu + 1 >= 0) & (fu + 1 < W) & ok
        y0 = (fv >= 0) & (fv < H)
        y1 = (fv + 1 >= 0) & (fv + 1 < H)
        res.append(dict(fu=fu, fv=fv, bx=u - fu, by=v - fv, ok=ok, mask=(x0 & y0, x1 & y0, x0 & y1, x1 & y1)))
    return res


def triplane_backward_ref(grad_out, planes, coords):
    """grad_out [n * m, C], planes [n, 3C, H, W], coords [n, m, 3] (float32 values) -> TriplaneGrad."""
    n, c3, H, W = planes.shape
    C = c3 // 3
    m = coords.shape[1]
    coords = coords.detach().cpu().to(torch.float32)
    go = grad_out.detach().cpu().double().reshape(n, m, C)
    # texel-major copy [n, 3, H, W, C] of the planes: one tap of one sample is a row of C values
    pl = planes.detach().cpu().double().reshape(n, 3, C, H, W).permute(0, 1, 3, 4, 2).contiguous()
    flat = pl.reshape(n * 3 * H * W, C)
    gp, ap, kp = torch.zeros_like(flat), torch.zeros_like(flat), torch.zeros(flat.shape[0], dtype=torch.int64)
    gc = torch.zeros(n, m, 3, dtype=torch.float64)
    ac = torch.zeros(n, m, 3, dtype=torch.float64)
    kc = torch.zeros(n, m, 3, dtype=torch.int64)
    finite = torch.isfinite(coords).all(dim=-1)
    hit = torch.zeros(n, m, dtype=torch.bool)
    img = torch.arange(n).reshape(n, 1)
    chan = torch.arange(C)
    for p, tp in enumerate(taps(coords, H, W)):
        finite &= tp['ok']
        bx, by = tp['bx'], tp['by']
        ax, ay = 1.0 - bx, 1.0 - by
        weights = (ax * ay, bx * ay, ax * by, bx * by)
        vals = []
        for (dx, dy), w, mk in zip(((0, 0), (1, 0), (0, 1), (1, 1)), weights, tp['mask']):
            hit |= mk
            ix = torch.where(mk, tp['fu'] + dx, torch.zeros_like(bx)).long()
            iy = torch.where(mk, tp['fv'] + dy, torch.zeros_like(by)).long()
            idx = (((img * 3 + p) * H + iy) * W + ix).reshape(-1)
            elem = (idx.unsqueeze(-1) * C + chan).reshape(-1)
            mkf = mk.double()
            term = (go * (w * mkf).unsqueeze(-1)).reshape(-1)
            gp.view(-1).index_add_(0, elem, term)
            ap.view(-1).index_add_(0, elem, term.abs())
            kp.index_add_(0, idx, mk.reshape(-1).long())
            vals.append(flat[idx].reshape(n, m, C) * mkf.unsqueeze(-1))
        v00, v01, v10, v11 = vals
        m00, m01, m10, m11 = (mk.long() for mk in tp['mask'])
        # d/du and d/dv of the blend, as the two terms each the kernel adds per channel
        for axis, size, d0, f0, d1, f1, k0, k1 in ((PLANE_AXES[p][0], W, v01 - v00, ay, v11 - v10, by, m00 | m01, m10 | m11),
                                                   (PLANE_AXES[p][1], H, v10 - v00, ax, v11 - v01, bx, m00 | m10, m01 | m11)):
            t0 = go * d0 * f0.unsqueeze(-1) * (0.5 * size)
            t1 = go * d1 * f1.unsqueeze(-1) * (0.5 * size)
            gc[..., axis] += (t0 + t1).sum(dim=-1)
            ac[..., axis] += (t0.abs() + t1.abs()).sum(dim=-1)
            kc[..., axis] += (k0 + k1) * C

    def back(x):
        return x.reshape(n, 3, H, W, -1).permute(0, 1, 4, 2, 3).reshape(n, c3, H, W).contiguous()

    return TriplaneGrad(back(gp), gc, back(ap), back(kp.unsqueeze(-1).expand(-1, C)), ac, kc, finite, hit)


def triplane_forward_ref(planes, coords):
    """planes [n, 3C, H, W], coords [n, m, 3] (float32 values) -> (out, abs_sum, hit, finite):
      out      [n * m, C] float64: per plane the in-bounds taps v * ((1 - bx | bx) * (1 - by | by)), summed over the three planes;
      abs_sum  [n * m, C] float64: A = the sum of |v * w| over those taps (the scale of `forward_bound`);
      hit      [n, m] bool: at least one tap of one plane is in bounds (rows without one are exactly 0);
      finite   [n, m] bool: all three coordinates (and their tap positions) are finite.  A plane that reads a non-finite coordinate has
               no tap; the plane that does not read it still contributes, as it does in ATen."""
    n, c3, H, W = planes.shape
    C = c3 // 3
    m = coords.shape[1]
    coords = coords.detach().cpu().to(torch.float32)
    flat = planes.detach().cpu().double().reshape(n, 3, C, H, W).permute(0, 1, 3, 4, 2).reshape(n * 3 * H * W, C)
    out = torch.zeros(n, m, C, dtype=torch.float64)
    A = torch.zeros(n, m, C, dtype=torch.float64)
    finite = torch.isfinite(coords).all(dim=-1)
    hit = torch.zeros(n, m, dtype=torch.bool)
    img = torch.arange(n).reshape(n, 1)
    for p, tp in enumerate(taps(coords, H, W)):
        finite &= tp['ok']
        bx, by = tp['bx'], tp['by']
        ax, ay = 1.0 - bx, 1.0 - by
        for (dx, dy), w, mk in zip(((0, 0), (1, 0), (0, 1), (1, 1)), (ax * ay, bx * ay, ax * by, bx * by), tp['mask']):
            hit |= mk
            ix = torch.where(mk, tp['fu'] + dx, torch.zeros_like(bx)).long()
            iy = torch.where(mk, tp['fv'] + dy, torch.zeros_like(by)).long()
            idx = (((img * 3 + p) * H + iy) * W + ix).reshape(-1)
            term = flat[idx].reshape(n, m, C) * (w * mk.double()).unsqueeze(-1)
            out += term
            A += term.abs()
    return out.reshape(n * m, C), A.reshape(n * m, C), hit, finite


def forward_bound(abs_sum):
    """fp32 bound of one output element of the gather: 12 * 2^-24 * A + 1e-30.  A term v * (fx * fy) carries at most four roundings (two
    fractions, their product, the product with v), the four accumulations of a plane round a partial sum <= A_plane each, two additions
    join the planes: 4 + 4 + 2 = 10, and a margin of 2 as in `plane_bound`.  1e-30 is for sums that end below the normal range."""
    return 12.0 * 2.0 ** -24 * abs_sum + 1e-30


# ---- host model of the ray-grid kernel's decisions (csrc/triplane_tile.hip), integers only ---------------------------------------------

TT_EDGE, TT_DS = 8, 4                    # a chunk: 8 x 8 rays x 4 depth steps = 256 samples
TT_CAP = 504                             # LDS lines per buffer (PC_CAP)
TT_LINES = (320, 256, 320)               # largest staged region per plane (TT_SEGS_A / TT_SEGS_B * 32)
TT_NUM_CU = 256


def tile_plan(n, rays_h, rays_w, steps):
    """(segs, chunks_per_seg) of `launch_triplane_tile` for n images in one group: one workgroup per ray tile, the depth axis cut into
    more segments only until every one of the 256 CUs has a workgroup, and only into divisors of the chunk count."""
    chunks = steps // TT_DS
    tiles = (rays_h // TT_EDGE) * (rays_w // TT_EDGE)
    ps = 1
    while ps < chunks and (n * tiles * ps < TT_NUM_CU or chunks % ps):
        ps += 1
    return ps, chunks // ps


def virtual_index(c, size):
    """`axis_index`: clamp(floor(u), -1, size - 1) + 1 after saturating floor(u) to [-2, size + 1]; NaN gives 0.  int64."""
    fu = torch.floor(unnormalize32(c, size))
    fu = torch.where(torch.isnan(fu), torch.full_like(fu, -2.0), fu).clamp(-2.0, float(size) + 1.0)
    return fu.long().clamp(-1, size - 1) + 1


def staged_costs(coords, H, W, ray_grid):
    """coords [n, rays_h * rays_w * steps, 3] -> int64 [3, n, tiles, chunks]: per plane the LDS lines its region of that chunk needs
    (bw * bh rounded up to 8), or TT_CAP + 1 = 505 where the plane cannot be staged.  Tiles are row-major over the ray grid, chunks run
    along the depth axis."""
    rh, rw, steps = ray_grid
    n = coords.shape[0]
    ty, tx, ch = rh // TT_EDGE, rw // TT_EDGE, steps // TT_DS
    co = coords.detach().cpu().to(torch.float32).reshape(n, ty, TT_EDGE, tx, TT_EDGE, ch, TT_DS, 3)
    co = co.permute(0, 1, 3, 5, 2, 4, 6, 7).reshape(n, ty * tx, ch, TT_EDGE * TT_EDGE * TT_DS, 3)

    def box(axis, size):          # over the 256 samples of the chunk
        v = virtual_index(co[..., axis], size)
        return v.amin(dim=-1), v.amax(dim=-1)

    xw, yh, yw, zh = box(0, W), box(1, H), box(1, W), box(2, H)
    cost = []
    for p, ((x_lo, x_hi), (y_lo, y_hi)) in enumerate(((xw, yh), (yw, zh), (xw, zh))):
        bw, bh = x_hi - x_lo + 2, y_hi - y_lo + 2
        lines = (bw * bh + 7) // 8 * 8
        inside = (x_lo >= 1) & (x_lo + bw - 2 <= W - 1) & (y_lo >= 1) & (y_lo + bh - 2 <= H - 1)
        cost.append(torch.where(inside & (lines <= TT_LINES[p]), lines, torch.full_like(lines, TT_CAP + 1)))
    return torch.stack(cost)


def staged_masks(coords, H, W, ray_grid):
    """-> int64 [n, tiles, chunks]: bit p = plane p of that chunk is staged in LDS (`build_region_table`): all three if they fit TT_CAP
    lines together, else the cheapest pair (ties: 01, 02, 12), else the cheapest single plane (ties: 0, 1, 2), else none."""
    l0, l1, l2 = staged_costs(coords, H, W, ray_grid)
    masks = torch.zeros_like(l0)
    best = torch.full_like(l0, TT_CAP + 1)
    for s, bits in ((l0 + l1, 3), (l0 + l2, 5), (l1 + l2, 6)):          # strict "<": a tie keeps the earlier one
        take = s < best
        best = torch.where(take, s, best)
        masks = torch.where(take, torch.full_like(masks, bits), masks)
    single = masks == 0
    for s, bits in ((l0, 1), (l1, 2), (l2, 4)):
        take = single & (s < best)
        best = torch.where(take, s, best)
        masks = torch.where(take, torch.full_like(masks, bits), masks)
    return torch.where(l0 + l1 + l2 <= TT_CAP, torch.full_like(masks, 7), masks)


def plane_bound(ref):
    """fp32 bound of one texel of the plane gradient: k atomic adds in any order plus the roundings of go * w (two fractions, their
    product, the product with go): (k + 4) * 2^-24 * A, and 1e-30 for sums that end below the normal range."""
    return (ref.cnt_planes.double() + 4.0) * 2.0 ** -24 * ref.abs_planes + 1e-30


def coord_bound(ref, C):
    """fp32 bound of one coordinate gradient: two planes of C channels with a handful of roundings each plus six shuffle levels:
    (2C + 16) * 2^-23 * A (A carries the size / 2 factor)."""
    return (2.0 * C + 16.0) * 2.0 ** -23 * ref.abs_coords


# ---- coordinate sets shared by the backward and the forward suites ------------------------------------------------------------------

def axis_edges(size):
    """Coordinates of one axis, by where their tap position u = ((c + 1) * size - 1) / 2 falls."""
    s = float(size)
    centres = [(2 * i + 1) / s - 1 for i in sorted({0, size // 2, size - 1})]          # u = i: an exact texel centre where fp32 allows
    return ([-1.0, 0.0, 1.0]                                   # the plane's edges (u = -0.5, size - 0.5: half a texel outside the outermost centres) and its middle
            + centres
            + [-1 - 0.5 / s, 1 + 0.5 / s]                      # u = -0.75, size - 0.25: one tap of the axis in bounds, inside the padding
            + [-1 - 1 / s, 1 + 1 / s]                          # u = -1, size: the in-bounds tap has weight 0 / no tap in bounds
            + [-1 - 3 / s, 1 + 3 / s, -1e30, 1e30])            # more than one texel outside, and far outside


def edges(g, n, m, H, W):
    """Every combination of the per-axis edge values (sides: two taps in bounds, corners: one), shuffled, cycled over the n * m rows."""
    xs, zs = axis_edges(W), axis_edges(H)
    ys = xs if H == W else xs + zs                              # y is plane 0's v (H) and plane 1's u (W)
    combos = torch.tensor(list(itertools.product(xs, ys, zs)), dtype=torch.float32)
    combos = combos[torch.randperm(combos.shape[0], generator=g)]
    idx = torch.arange(n * m) % combos.shape[0]
    return combos[idx].reshape(n, m, 3).contiguous()


NONFINITE = [[float('nan'), 0.0, 0.0], [0.0, float('nan'), 0.0], [0.0, 0.0, float('nan')], [float('inf'), 0.1, 0.0],
             [0.0, float('-inf'), 0.2], [0.3, 0.0, float('inf')], [float('nan'), float('inf'), float('-inf')]]
