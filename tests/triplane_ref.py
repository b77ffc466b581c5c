"""Float64 definition of the tri-plane gather's backward (`triplane_backward_kernel`, csrc/triplane.hip), plain torch on the CPU.

The gradient with respect to the coordinates is piecewise constant in the texel, so a reference must not disagree with the kernel about
which texel a sample is in.  The tap position therefore comes from the project's own contract (DESIGN.md "tap index contract",
`test_triplane_tap_indices_bit_exact`): u = ((c + 1) * size - 1) / 2 in float32 as separate add, mul, sub, mul(0.5) operations.
Everything after it - floor, fractions, weights, zero-padding masks, the scatter and the coordinate gradient - is float64.

Plane p reads (u from a -> W, v from b -> H): p0 = (x, y), p1 = (y, z), p2 = (x, z).
"""

import collections

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


def plane_bound(ref):
    """fp32 bound of one texel of the plane gradient: k atomic adds in any order plus the roundings of go * w (two fractions, their
    product, the product with go): (k + 4) * 2^-24 * A, and 1e-30 for sums that end below the normal range."""
    return (ref.cnt_planes.double() + 4.0) * 2.0 ** -24 * ref.abs_planes + 1e-30


def coord_bound(ref, C):
    """fp32 bound of one coordinate gradient: two planes of C channels with a handful of roundings each plus six shuffle levels:
    (2C + 16) * 2^-23 * A (A carries the size / 2 factor)."""
    return (2.0 * C + 16.0) * 2.0 ** -23 * ref.abs_coords
