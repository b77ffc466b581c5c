"""Float64 numpy restatement of the geometric and colour stages of training/augment.py, written from the definition in
include/ide3d_hip.h; no torch op computes anything here.

For N images x [C, H, W], inverse pixel transforms G_inv [N, 3, 3] and the 12 taps f:
    margins (mx0, my0, mx1, my1): ceil of the batch-wide reach of the transformed corners plus 6, clamped to [0, side - 1]
    P[i, j] = x[r(i - my0), r(j - mx0)]                       one reflection
    U       = Uy P Ux^T,  U_[r, i] = 2 f[r + 5 - 2 i]          zero insertion, pads 6 / 5, true convolution, gain 2 per axis
    S[i, j] = bilinear, zeros, sample of U at A (j, i, 1)      A: lines 292-301 and both unnormalisations folded (`coords`)
    y       = Dy S Dx^T,  D_[o, 2 o + 1 + k] = f[k]            pads -1 / -1, flipped filter, decimation by 2
    colour  = M[:, :3] y + M[:, 3]                            3 channels; the mean row, summed, for one channel

Every function returns (value, absval, coordinate term):
  absval           the same map on |x| with |taps| (bilinear weights are non-negative already) and |M|;
  coordinate term  a bound of the change of the value when every sampling coordinate moves by up to d = n_c 2^-24 max|coordinate|:
                   |dS| <= d (Lx + Ly) with Lx, Ly the largest neighbour differences of U around the sample's cell (a bilinear
                   interpolant is Lipschitz with those constants, across cell borders too), pushed through |D| and |M|.
A tolerance is  n 2^-24 absval + coordinate term.

Counts, from the code under test:
  N_OPS = 84: the longest chain of float32 additions and multiplications from an input pixel to an output in csrc/augment.hip:
      up-sampling 2 x (6 multiplications + 5 additions) = 22 (the doubling of the taps is exact), bilinear weights and blend
      (1 - fx, 1 - fy, two products and one addition per row, two products and one addition across) = 9, decimation
      2 x (12 + 11) = 46, colour 3 + 3 = 6, and one more for the float32 rounding of each tap.  The PyTorch definition runs the same
      filters as convolutions with the same number of terms and ATen's four-product blend: not longer.
  NC_KERNEL = 6: coords (float64 fold, one rounding per entry: 3 on a coordinate's path), two fused multiply-adds, and the
      subtraction of the floor (exact) -> 5; one spare for the conversion of the indices.  max|coordinate| is
      |a0| j + |a1| i + |a2| at the far corner of the sampling grid, which bounds every intermediate.
      The same n_c holds for the PyTorch definition and the reference-run golden file, whose float32 matrix chain is longer: at the
      shapes tested their coordinates stay within the same bound (largest error / bound seen 0.05), so no second count is needed.
"""

import numpy as np

N_OPS = 84
NC_KERNEL = 6
U = 2.0 ** -24

SYM6 = [0.015404109327027373, 0.0034907120842174702, -0.11799011114819057, -0.048311742585633, 0.4910559419267466, 0.787641141030194,
        0.3379294217276218, -0.07263752278646252, -0.021060292512300564, 0.04472490177066578, 0.0017677118642428036, -0.007800708325034148]


def taps_f32():
    """The Hz_geom buffer: sym6 normalised to unit sum, as float32 values in float64."""
    f = np.asarray(SYM6, dtype=np.float32)
    return (f / f.sum(dtype=np.float32)).astype(np.float64)


def margin_values(G_inv, H, W):
    """Unclamped reach (x0, y0, x1, y1) before ceil, float64, and the int margins after clamp and ceil."""
    G = np.asarray(G_inv, dtype=np.float64)
    cx, cy = (W - 1) / 2, (H - 1) / 2
    corners = np.array([[-cx, -cy, 1], [cx, -cy, 1], [cx, cy, 1], [-cx, cy, 1]]).T
    moved = G @ corners                                               # [N, 3, 4]
    xs, ys = moved[:, 0, :].ravel(), moved[:, 1, :].ravel()
    raw = np.array([(-xs).max(), (-ys).max(), xs.max(), ys.max()]) + np.array([6 - cx, 6 - cy, 6 - cx, 6 - cy])
    clamped = np.minimum(np.maximum(raw, 0), [W - 1, H - 1, W - 1, H - 1])
    return raw, np.ceil(clamped).astype(np.int64)


def margin_distance(raw, H, W):
    """Smallest distance to an integer of the reach values that the clamp leaves alone."""
    hi = np.array([W - 1, H - 1, W - 1, H - 1])
    free = raw[(raw > 0) & (raw < hi)]
    return float(np.abs(free - np.round(free)).min()) if free.size else 1.0


def coords(G_inv, m, H, W):
    """[N, 2, 3] float64: sampling-grid pixel (j, i, 1) -> pixel coordinates in U."""
    mx0, my0, mx1, my1 = [float(v) for v in m]
    T = lambda tx, ty: np.array([[1, 0, tx], [0, 1, ty], [0, 0, 1.0]])
    Sc = lambda s: np.diag([s, s, 1.0])
    ws, hs = 2 * (W + 6), 2 * (H + 6)
    wu, hu = 2 * (W + mx0 + mx1), 2 * (H + my0 + my1)
    G = T((mx0 - mx1) / 2, (my0 - my1) / 2) @ np.asarray(G_inv, dtype=np.float64)
    G = Sc(2.0) @ G @ Sc(0.5)
    G = T(-0.5, -0.5) @ G @ T(0.5, 0.5)
    G = T((wu - 1) / 2, (hu - 1) / 2) @ G @ T(-(ws - 1) / 2, -(hs - 1) / 2)
    return G[:, :2, :]


def _reflect(t, side):
    t = np.where(t < 0, -t, t)
    return np.where(t >= side, 2 * (side - 1) - t, t)


def _axis(side, m0, m1, f):
    """(R [side_p, side] one-hot reflect padding, Up [2 side_p, side_p], D [side, 2 (side + 6)])."""
    sp = side + m0 + m1
    R = np.zeros([sp, side]); R[np.arange(sp), _reflect(np.arange(sp) - m0, side)] = 1
    Up = np.zeros([2 * sp, sp])
    for r in range(2 * sp):
        for k in range(12):
            if (r + 5 - k) % 2 == 0 and 0 <= (r + 5 - k) // 2 < sp:
                Up[r, (r + 5 - k) // 2] += 2 * f[k]
    D = np.zeros([side, 2 * (side + 6)])
    for o in range(side):
        D[o, 2 * o + 1: 2 * o + 13] = f
    return R, Up, D


class Geometry:
    """The linear map of one batch's geometric stage: per-axis matrices and per-image bilinear taps."""

    def __init__(self, G_inv, H, W, f=None, n_c=NC_KERNEL):
        self.f = taps_f32() if f is None else np.asarray(f, dtype=np.float64)
        self.H, self.W, self.N = H, W, len(G_inv)
        self.raw, self.m = margin_values(G_inv, H, W)
        mx0, my0, mx1, my1 = [int(v) for v in self.m]
        self.Ry, self.Uy, self.Dy = _axis(H, my0, my1, self.f)
        self.Rx, self.Ux, self.Dx = _axis(W, mx0, mx1, self.f)
        self.A = coords(G_inv, self.m, H, W)
        hs, ws = 2 * (H + 6), 2 * (W + 6)
        self.hu, self.wu = self.Uy.shape[0], self.Ux.shape[0]
        jj, ii = np.meshgrid(np.arange(ws, dtype=np.float64), np.arange(hs, dtype=np.float64))
        self.ix = self.A[:, 0, 0, None, None] * jj + self.A[:, 0, 1, None, None] * ii + self.A[:, 0, 2, None, None]
        self.iy = self.A[:, 1, 0, None, None] * jj + self.A[:, 1, 1, None, None] * ii + self.A[:, 1, 2, None, None]
        mag = lambda a: np.abs(a[:, 0]) * (ws - 1) + np.abs(a[:, 1]) * (hs - 1) + np.abs(a[:, 2])
        self.dx = n_c * U * mag(self.A[:, 0])                       # [N]: how far a float32 coordinate may sit from the float64 one
        self.dy = n_c * U * mag(self.A[:, 1])

    def _sample(self, n, Uimg):
        """Bilinear, zeros: Uimg [C, hu, wu] -> [C, hs, ws]."""
        x0, y0 = np.floor(self.ix[n]).astype(np.int64), np.floor(self.iy[n]).astype(np.int64)
        fx, fy = self.ix[n] - x0, self.iy[n] - y0
        Up = np.zeros([Uimg.shape[0], self.hu + 4, self.wu + 4]); Up[:, 2:-2, 2:-2] = Uimg
        out = 0
        for dy, wy in ((0, 1 - fy), (1, fy)):
            for dx, wx in ((0, 1 - fx), (1, fx)):
                yy, xx = np.clip(y0 + dy + 2, 0, self.hu + 3), np.clip(x0 + dx + 2, 0, self.wu + 3)
                out = out + Up[:, yy, xx] * (wy * wx)
        return out

    def _scatter(self, n, gS, spread=False):
        """Transpose of _sample: gS [C, hs, ws] -> [C, hu, wu].  spread: the bound of the CHANGE of the result when the coordinates move by
        (dx, dy): every tap weight is a product of tents, which move by at most dx and dy; taps one cell further out may come alive."""
        x0, y0 = np.floor(self.ix[n]).astype(np.int64), np.floor(self.iy[n]).astype(np.int64)
        acc = np.zeros([gS.shape[0], self.hu, self.wu])
        tent = lambda t: np.maximum(1 - np.abs(t), 0)
        for dy in ((-1, 0, 1, 2) if spread else (0, 1)):
            for dx in ((-1, 0, 1, 2) if spread else (0, 1)):
                yy, xx = y0 + dy, x0 + dx
                ty, tx = tent(self.iy[n] - yy), tent(self.ix[n] - xx)
                if spread:
                    near_x, near_y = np.abs(self.ix[n] - xx) <= 1 + self.dx[n], np.abs(self.iy[n] - yy) <= 1 + self.dy[n]
                    wgt = (self.dx[n] * near_x * np.minimum(ty + self.dy[n], 1) * near_y + self.dy[n] * near_y * np.minimum(tx + self.dx[n], 1) * near_x)
                else:
                    wgt = ty * tx
                ok = (yy >= 0) & (yy < self.hu) & (xx >= 0) & (xx < self.wu)
                for c in range(gS.shape[0]):
                    np.add.at(acc[c], (yy[ok], xx[ok]), (gS[c] * wgt)[ok])
        return acc

    def _slopes(self, n, Uimg):
        """d (Lx + Ly) per sample: the bound of |dS|."""
        Up = np.zeros([Uimg.shape[0], self.hu + 6, self.wu + 6]); Up[:, 3:-3, 3:-3] = Uimg
        ddx = np.abs(np.diff(Up, axis=2)); ddy = np.abs(np.diff(Up, axis=1))
        x0 = np.clip(np.floor(self.ix[n]).astype(np.int64), -2, self.wu) + 3
        y0 = np.clip(np.floor(self.iy[n]).astype(np.int64), -2, self.hu) + 3
        Lx = 0; Ly = 0
        for r in (-1, 0, 1, 2):
            for c in (-1, 0, 1):
                Lx = np.maximum(Lx, ddx[:, y0 + r, x0 + c])           # |U[r, c + 1] - U[r, c]|
                Ly = np.maximum(Ly, ddy[:, y0 + c, x0 + r])
        inside = (self.ix[n] > -1 - self.dx[n]) & (self.ix[n] < self.wu + self.dx[n]) & (self.iy[n] > -1 - self.dy[n]) & (self.iy[n] < self.hu + self.dy[n])
        return (self.dx[n] * Lx + self.dy[n] * Ly) * inside

    def forward(self, x):
        """x [N, C, H, W] -> (y, absval, coordinate term), float64."""
        x = np.asarray(x, dtype=np.float64)
        y, a, ct = np.zeros_like(x), np.zeros_like(x), np.zeros_like(x)
        aUy, aUx, aDy, aDx = np.abs(self.Uy), np.abs(self.Ux), np.abs(self.Dy), np.abs(self.Dx)
        for n in range(self.N):
            Uimg = self.Uy @ (self.Ry @ x[n] @ self.Rx.T) @ self.Ux.T
            y[n] = self.Dy @ self._sample(n, Uimg) @ self.Dx.T
            a[n] = aDy @ self._sample(n, aUy @ (self.Ry @ np.abs(x[n]) @ self.Rx.T) @ aUx.T) @ aDx.T
            ct[n] = aDy @ self._slopes(n, Uimg) @ aDx.T
        return y, a, ct

    def transpose(self, g):
        """g [N, C, H, W] -> (the transposed map applied to g, absval, coordinate term)."""
        g = np.asarray(g, dtype=np.float64)
        y, a, ct = np.zeros_like(g), np.zeros_like(g), np.zeros_like(g)
        aUy, aUx, aDy, aDx = np.abs(self.Uy), np.abs(self.Ux), np.abs(self.Dy), np.abs(self.Dx)
        for n in range(self.N):
            y[n] = self.Ry.T @ (self.Uy.T @ self._scatter(n, self.Dy.T @ g[n] @ self.Dx) @ self.Ux) @ self.Rx
            gS = aDy.T @ np.abs(g[n]) @ aDx
            a[n] = self.Ry.T @ (aUy.T @ self._scatter(n, gS) @ aUx) @ self.Rx
            ct[n] = self.Ry.T @ (aUy.T @ self._scatter(n, gS, spread=True) @ aUx) @ self.Rx
        return y, a, ct


def color_rows(C, channels):
    """[N, 4, 4] -> [N, 3 or 1, 4] float64: the rows the colour stage applies."""
    C = np.asarray(C, dtype=np.float64)
    if channels == 3:
        return C[:, :3, :]
    grey = C[:, :3, :].mean(axis=1)
    return np.stack([grey[:, :3].sum(axis=1), grey[:, 3]], axis=1)[:, None, :]       # [N, 1, (scale, offset)]


def color(y, absval, ct, C):
    """The colour stage on top of a (value, absval, coordinate term) triple."""
    ch = y.shape[1]
    M = color_rows(C, ch)
    if ch == 3:
        lin, off = M[:, :, :3], M[:, :, 3]
    else:
        lin, off = M[:, :, :1], M[:, :, 1]
    mix = lambda m, v: np.einsum('nij,njhw->nihw', m, v)
    return mix(lin, y) + off[:, :, None, None], mix(np.abs(lin), absval) + np.abs(off)[:, :, None, None], mix(np.abs(lin), ct)


def color_linear(y, absval, ct, C):
    """The colour stage without its offset (what a second differentiation leaves) on top of a (value, absval, coordinate term) triple."""
    v, a, c = color(y, absval, ct, C)
    M = color_rows(C, y.shape[1])
    off = M[:, :, 3] if y.shape[1] == 3 else M[:, :, 1]
    return v - off[:, :, None, None], a - np.abs(off)[:, :, None, None], c


def color_transpose(g, C):
    """Transpose of the colour stage without the offset: (value, absval)."""
    ch = g.shape[1]
    M = color_rows(C, ch)
    lin = M[:, :, :3] if ch == 3 else M[:, :, :1]
    mix = lambda m, v: np.einsum('nji,njhw->nihw', m, v)
    return mix(lin, g), mix(np.abs(lin), np.abs(g))


def bound(absval, ct, n=N_OPS):
    return n * U * absval + ct


def report(name, got, want, tol):
    """Print the largest error-to-bound ratio and return whether every element is within its bound."""
    err = np.abs(np.asarray(got, dtype=np.float64) - want)
    ratio = float((err / np.maximum(tol, 1e-300)).max())
    print(f'{name}: largest error / bound = {ratio:.3f} (largest error {float(err.max()):.3e})')
    return bool((err <= tol).all())


# ---- the parameters of the reference's debug_percentile mode, restated in float64 -------------------------------------------------

BGC = dict(xflip=1, rotate90=1, xint=1, scale=1, rotate=1, aniso=1, xfrac=1, brightness=1, contrast=1, lumaflip=1, hue=1, saturation=1)


def _erfinv(y):
    """Inverse error function by Newton steps on math.erf (float64)."""
    import math
    x = 0.0
    for _ in range(60):
        x -= (math.erf(x) - y) / (2 / math.sqrt(math.pi) * math.exp(-x * x))
    return x


def debug_matrices(pct, channels, H, W):
    """(G_inv [3, 3], C [4, 4]) of the bgc configuration at debug_percentile pct (augment.py:202-268, 317-355, default strengths)."""
    pct = float(np.float32(pct))
    T = lambda tx, ty: np.array([[1, 0, tx], [0, 1, ty], [0, 0, 1.0]])
    R = lambda t: np.array([[np.cos(t), np.sin(-t), 0], [np.sin(t), np.cos(t), 0], [0, 0, 1.0]])
    z = _erfinv(2 * pct - 1)
    G = np.diag([1 / (1 - 2 * np.floor(pct * 2)), 1, 1.0])
    G = G @ R(np.pi / 2 * np.floor(pct * 4))
    t = (pct * 2 - 1) * 0.125
    G = G @ T(-np.round(t * W), -np.round(t * H))
    s = 2 ** (z * 0.2)
    G = G @ np.diag([1 / s, 1 / s, 1.0])
    G = G @ R((pct * 2 - 1) * np.pi)
    G = G @ np.diag([1 / s, s, 1.0])
    G = G @ T(-z * 0.125 * W, -z * 0.125 * H)
    C = np.eye(4)
    b = z * 0.2
    Tb = np.eye(4); Tb[:3, 3] = b
    C = Tb @ C
    C = np.diag([2 ** (z * 0.5)] * 3 + [1.0]) @ C
    v = np.array([1, 1, 1, 0]) / np.sqrt(3)
    vv = np.outer(v, v)
    C = (np.eye(4) - 2 * vv * np.floor(pct * 2)) @ C
    if channels > 1:
        th = (pct * 2 - 1) * np.pi
        K = np.array([[0, -v[2], v[1], 0], [v[2], 0, -v[0], 0], [-v[1], v[0], 0, 0], [0, 0, 0, 0.0]])
        Rot = np.cos(th) * (np.eye(4) - vv) + vv + np.sin(th) * K
        Rot[3, :] = [0, 0, 0, 1]; Rot[:, 3] = [0, 0, 0, 1]
        C = Rot @ C
        C = (vv + (np.eye(4) - vv) * 2 ** z) @ C
    return G, C


# ---- the cases of the golden file (scripts/make_augment_golden.py) ------------------------------------------------------------------

SHAPES = [(2, 3, 17, 33), (2, 3, 24, 20), (2, 3, 5, 7), (2, 1, 2, 2)]
PERCENTILES = [0.1, 0.3, 0.37, 0.62, 0.9]
MARGIN_CLEARANCE = 1e-3          # every unclamped margin lies at least this far from an integer, so float32 and float64 agree on the ceil

_cache = {}


def golden():
    import os
    if 'golden' not in _cache:
        _cache['golden'] = dict(np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'augment.npz')))
    return _cache['golden']


def golden_case(si, pi, n_c):
    """(x, golden output, float64 output, tolerance, Geometry, G_inv [N, 3, 3], C [N, 4, 4]) of one bgc case; computed once per n_c."""
    key = (si, pi, n_c)
    if key not in _cache:
        n, c, h, w = SHAPES[si]
        G, C = debug_matrices(PERCENTILES[pi], c, h, w)
        Gn, Cn = np.stack([G] * n), np.stack([C] * n)
        geo = Geometry(Gn, h, w, n_c=n_c)
        x = golden()[f'x_{si}']
        y, a, ct = color(*geo.forward(x), Cn)
        _cache[key] = (x, golden()[f'bgc_{si}_{pi}'], y, bound(a, ct), geo, Gn, Cn)
    return _cache[key]
