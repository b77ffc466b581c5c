"""Float64 references and the case table of the inverse-cdf sampling suites (tests/test_gpu_sample_pdf.py; checked without a GPU at the end
of tests/test_composite_cases_cpu.py; `cdf_at` also serves tests/test_gpu_ops.py::test_sample_pdf_kernel).

`ide3d_sample_pdf` (csrc/sample_pdf.hip) gives lane l of a wave the run [l * per, l * per + per) of a ray's k weights, per = ceil(k / 64):
  k = 63, 65, 129      trailing lanes have an empty run (i0 = min(l * per, k) = k)
  k = 127, 2047        the last lane's run is one short
  k = 64, 128, 2048    every run full
A workgroup takes four rays per grid-stride trip and every wave must reach both barriers of every trip of its workgroup, so a ray count of
8192 + 3 leaves the last trip with a wave that has no ray.

The sampled function is discontinuous where a draw meets a cdf knot (the bin changes) and where a bin's mass meets eps (`denom < eps -> 1`).
The table keeps away from both: in the float64 cdf every bin mass is >= 1e-6 away from eps and every draw >= 1e-5 away from every knot, so
every correct float32 evaluation takes the same bin and branch as the float64 inverse cdf, and all elements can be compared.  The placed
draws of `placed_case` sit ON those edges instead and are held to the properties that survive them.
"""

import torch

EPS = 1e-5


def expand(u, rays):
    return u.expand(rays, u.shape[-1]) if u.ndim == 1 else u


def cdf64(wts, eps=EPS):
    """[rays, k + 1] float64 cdf of (wts + eps) / sum(wts + eps)."""
    pd = wts.double() + eps
    return torch.cat([torch.zeros(wts.shape[0], 1, dtype=torch.float64), torch.cumsum(pd / pd.sum(-1, keepdim=True), -1)], -1)


def cdf_at(bins, wts, smp, eps=EPS):
    """(the float64 piece-wise linear cdf of the ray at each sample [rays, n], the tolerance of `cdf(sample) = u` [rays, 1]).
    tolerance: the mass eps of a bin on the `denom -> 1` branch + a float32 ulp of the depth (2.4e-7 near 3) times the steepest cdf
    slope of the ray."""
    cd = cdf64(wts, eps)
    bd = bins.double()
    i = (torch.searchsorted(bd, smp.double().contiguous(), right=True) - 1).clamp(0, bd.shape[1] - 2)
    b0, b1 = torch.gather(bd, 1, i), torch.gather(bd, 1, i + 1)
    c0, c1 = torch.gather(cd, 1, i), torch.gather(cd, 1, i + 1)
    steepest = ((cd[:, 1:] - cd[:, :-1]) / (bd[:, 1:] - bd[:, :-1])).max(-1, keepdim=True)[0]
    return c0 + (smp.double() - b0) / (b1 - b0) * (c1 - c0), 2e-5 + steepest * 5e-7


def inverse_cdf64(bins, wts, u, eps=EPS):
    """The definition of sample_pdf evaluated in float64 -> [rays, n] float64."""
    cd = cdf64(wts, eps)
    k = wts.shape[1]
    ud = expand(u, wts.shape[0]).double().contiguous()
    idx = torch.searchsorted(cd, ud)
    lo, hi = (idx - 1).clamp(min=0), idx.clamp(max=k)
    c0, c1 = torch.gather(cd, 1, lo), torch.gather(cd, 1, hi)
    bd = bins.double()
    b0, b1 = torch.gather(bd, 1, lo), torch.gather(bd, 1, hi)
    den = c1 - c0
    den = torch.where(den < eps, torch.ones_like(den), den)
    return b0 + (ud - c0) / den * (b1 - b0)


def _knot_distance(cd, u):
    """Distance of every draw to the nearest cdf knot of the rays it is used with: u [rays, n] against its own ray, u [n] against all."""
    if u.ndim == 1:
        knots = torch.sort(cd.reshape(-1))[0][None]
        ud = u.double()[None].contiguous()
    else:
        knots, ud = cd, u.double().contiguous()
    i = torch.searchsorted(knots, ud).clamp(1, knots.shape[1] - 1)
    d = torch.minimum((ud - torch.gather(knots, 1, i - 1)).abs(), (torch.gather(knots, 1, i) - ud).abs())
    return d[0] if u.ndim == 1 else d


def margins(bins, wts, u, eps=EPS):
    cd = cdf64(wts, eps)
    mass = cd[:, 1:] - cd[:, :-1]
    return dict(bin_mass_to_eps=float((mass - eps).abs().min()), draw_to_knot=float(_knot_distance(cd, u).min()),
                bin_width=float((bins[:, 1:] - bins[:, :-1]).min()))


class PdfCase:
    def __init__(self, index, k, rays, n, per_ray):
        self.index, self.k, self.rays, self.n, self.per_ray = index, k, rays, n, per_ray
        self.name = f'k{k}-r{rays}-n{n}-' + ('per_ray' if per_ray else 'shared')
        self._inputs = None

    def inputs(self):
        """bins [rays, k + 1] increasing in [2.25, 3.3], weights [rays, k] (a floor of 0.05 under one random peak), draws [n] or [rays, n]
        in (0, 1) picked by rejection so that they keep 2e-5 from every knot.  float32 on the CPU; built once, not to be written to."""
        if self._inputs is None:
            g = torch.Generator().manual_seed(9000 + self.index)
            k, rays, n = self.k, self.rays, self.n
            steps = 0.3 + torch.rand(rays, k + 1, generator=g, dtype=torch.float64)
            bins = (2.25 + 1.05 * (torch.cumsum(steps, -1) - steps[:, :1]) / (steps.sum(-1, keepdim=True) - steps[:, :1])).float()
            centre = torch.rand(rays, 1, generator=g) * k
            w = 0.05 + torch.exp(-((torch.arange(k)[None] - centre) / (k / 8 + 1)) ** 2) * torch.rand(rays, k, generator=g)
            cd = cdf64(w)
            cand = torch.rand((rays, 8 * n + 64) if self.per_ray else (8 * n + 64,), generator=g) * 0.998 + 0.001
            ok = _knot_distance(cd, cand) >= 2e-5
            if self.per_ray:
                u = torch.stack([cand[r][ok[r]][:n] for r in range(rays)])
            else:
                u = cand[ok][:n]
            assert u.shape[-1] == n
            self._inputs = (bins, w, u.contiguous())
        return self._inputs


def _table():
    rows = []
    for k in (1, 2, 63, 64, 65, 127, 128, 129, 2047, 2048):
        rows.append((k, 5, 7, k % 2 == 0))                    # alternately shared and per-ray draws
    rows.append((94, 8192 + 3, 7, True))                      # second grid-stride trip, the last workgroup's fourth wave without a ray
    for n in (1, 64, 65):                                     # one draw; one per lane; a second draw for lane 0 only
        rows.append((94, 5, n, False))
        rows.append((65, 6, n, True))
    return tuple(PdfCase(i, *r) for i, r in enumerate(rows))


CASES = _table()


def placed_case():
    """k = 94, 7 rays, per-ray draws ON the edges the table avoids, sorted per ray.  Ray 0: all weights zero.  Ray 1: a run of zero-weight
    bins 40..49 with draws inside it.  Ray 2: zero-weight runs at both ends.  Rays 3..6: as in the table.
    Draws of every ray: -0.5, 0, 1e-7, float32 cdf knots 1, 40, 45, 50, k - 1 and k of the float32 definition, two float32 values inside
    bins 40..49's cdf span, 1, the float32 after 1, 1.5, and four random ones."""
    g = torch.Generator().manual_seed(9100)
    k, rays = 94, 7
    steps = 0.3 + torch.rand(rays, k + 1, generator=g, dtype=torch.float64)
    bins = (2.25 + 1.05 * (torch.cumsum(steps, -1) - steps[:, :1]) / (steps.sum(-1, keepdim=True) - steps[:, :1])).float()
    centre = torch.rand(rays, 1, generator=g) * k
    w = 0.05 + torch.exp(-((torch.arange(k)[None] - centre) / (k / 8 + 1)) ** 2) * torch.rand(rays, k, generator=g)
    w[0] = 0
    w[1, 40:50] = 0
    w[2, :10] = 0
    w[2, 84:] = 0
    pdf = (w + EPS) / (w + EPS).sum(-1, keepdim=True)
    c32 = torch.cat([torch.zeros(rays, 1), torch.cumsum(pdf, -1)], -1)          # the float32 definition's knots
    one = torch.ones(rays, 1)
    lo, hi = c32[:, 40:41], c32[:, 50:51]
    u = torch.cat([-0.5 * one, 0 * one, 1e-7 * one, c32[:, [1, 40, 45, 50, k - 1, k]], lo + (hi - lo) * 0.25, lo + (hi - lo) * 0.75,
                   one, torch.nextafter(one, 2 * one), 1.5 * one, torch.rand(rays, 4, generator=g)], -1)
    return bins, w, torch.sort(u, -1)[0].contiguous()
