"""The case table of the compositing suites: tests/test_composite_cases_cpu.py checks the table itself without a GPU (which kernel form of
csrc/composite.hip every case takes, by `hip_plugin.composite_plan`; that the options reach every form; that the float64 loop of
oracle/ops.py and the tensor definition agree), tests/test_gpu_composite.py runs `ide3d_composite` on it.

`ide3d_composite` has four forms, chosen by block = steps * (ch + 1) floats of one ray and the address of rgb_sigma:
  lds8 / lds20 / lds40   composite_lds_kernel<8 | 20 | 40>: block % 4 == 0, block <= 2048 | 5120 | 10240, 16-byte aligned rgb_sigma, and
                         4 * (block + pad4(steps)) * 4 bytes <= 160 KB
  fallback               composite_kernel: everything else; samples in chunks of 64 with the transmittance carried across chunks

Every case runs once per clamp mode, each with its own options (letters: L last_back, W white_back, D max_depth = 5, F fill_mode 'weight',
G fill_mode 'debug', N noise).  Every case that takes an LDS form runs again from a view that starts one float into a larger buffer: the
view is contiguous, so the binding keeps it, and the misaligned address sends the same numbers through the fallback kernel.

Rays of a case (5 to 9; the grid-stride case 8192 + 5): ray 0 has sigma = -30 everywhere (transparent: relu gives exact zeros), ray 1
sigma = +50 everywhere (opaque), ray 2 two equal neighbouring depths (across the 64-sample chunk edge where there is one), the rest random.
Depths are sorted in [2.25, 3.3]; ray directions have norms that float32 holds and computes exactly (0.5 .. 1.5), so that the norm taken on
the device, on the host and in the oracle are one number.
"""

import torch

MAX_DEPTH = 5.0
NOISE_STD = 0.5          # a power of two: noise * noise_std is exact, so the oracle and the kernel see the same scaled draws
CLAMP_MODES = ('softplus', 'relu')
OPTION_LETTERS = 'LWDFGN'

# (steps, ch + 1, options with softplus, options with relu, expected form from an aligned buffer, rays or None, what the shape is there for)
_TABLE = (
    (13, 4, 'GN', 'GD', 'lds8', None, 'nvec = 13: the min(i, nvec - 1) tail load; debug fill'),
    (2, 4, 'G', 'GW', 'lds8', None, 'two samples; from the offset view the smallest block % 4 == 0 in the fallback'),
    (64, 32, 'FLN', 'LWD', 'lds8', None, 'block 2048: the upper edge of NLD = 8'),
    (27, 76, 'N', 'WD', 'lds20', None, 'block 2052: first past lds8'),
    (96, 53, 'L', 'LN', 'lds20', None, 'the coarse workload; two sample chunks'),
    (32, 65, 'F', 'W', 'lds20', None, 'ch = 64: one full channel trip'),
    (30, 132, 'WD', 'LF', 'lds20', None, 'ch = 131: three channel trips'),
    (80, 64, 'LWDN', '', 'lds20', None, 'block 5120: the upper edge of NLD = 20'),
    (61, 84, 'LN', 'WD', 'lds40', None, 'block 5124: first past lds20'),
    (157, 64, 'FD', 'LWN', 'lds40', None, 'block 10048, 160 768 + 2 560 bytes: near the LDS limit; three sample chunks'),
    (13, 7, '', 'WD', 'fallback', None, 'block 91: not a multiple of 4'),
    (64, 7, 'L', 'N', 'lds8', None, 'block 448 is a multiple of 4 after all; from the offset view exactly one chunk in the fallback'),
    (65, 7, 'N', 'LD', 'fallback', None, 'one sample in the second chunk: the carry'),
    (129, 7, 'WD', 'LWN', 'fallback', None, 'one sample in the third chunk'),
    (192, 53, 'L', 'LWD', 'fallback', None, 'the hierarchical workload: block 10176 fits, the LDS bytes (165 888) do not'),
    (160, 64, 'F', 'N', 'fallback', None, 'block 10240 fits, the LDS bytes (166 400) do not'),
    (197, 52, 'N', 'F', 'fallback', None, 'block 10244 > 10240'),
    (1024, 10, 'LD', 'W', 'fallback', None, 'kMaxSteps: 16 chunks'),
    (40, 256, 'W', 'LFN', 'fallback', None, 'ch = 255: four channel trips, the last one ragged'),
    (13, 7, 'N', 'LWD', 'fallback', 8192 + 5, 'second grid-stride trip of 2048 workgroups x 4 waves, ragged last workgroup'),
)

# rays_d_cam rows whose 2-norm is exact in float32 whatever the order of the three squares: 1, 1.25, 0.5, 1.5, 0.75
_DIRS = ((0.0, 0.0, -1.0), (0.75, 1.0, 0.0), (0.0, -0.5, 0.0), (1.0, -0.5, 1.0), (0.25, 0.5, -0.5))
_DIR_NORMS = (1.0, 1.25, 0.5, 1.5, 0.75)


class Case:
    def __init__(self, index, steps, row, opts_softplus, opts_relu, form, rays, why):
        self.index, self.steps, self.ch, self.form, self.why = index, steps, row - 1, form, why
        self.rays = rays if rays is not None else 5 + index % 5
        self.opts = dict(softplus=opts_softplus, relu=opts_relu)
        self.name = f'{steps}x{row}' + (f'-r{rays}' if rays else '')
        self._inputs = None

    def kwargs(self, clamp_mode):
        """The keyword arguments of fancy_integration / _fancy_integration_torch / oracle composite that the option letters stand for
        (without the noise: see `inputs`)."""
        o = self.opts[clamp_mode]
        return dict(clamp_mode=clamp_mode, last_back='L' in o, white_back='W' in o, max_depth=MAX_DEPTH if 'D' in o else None,
                    fill_mode='weight' if 'F' in o else 'debug' if 'G' in o else None)

    def has_noise(self, clamp_mode):
        return 'N' in self.opts[clamp_mode]

    def inputs(self):
        """rgb_sigma [1, R, S, ch + 1], rays_d_cam [1, R, 3], z_vals [1, R, S, 1], noise [1, R, S, 1] (standard normal; a run with N passes
        it with noise_std = NOISE_STD), all float32 on the CPU.  Built once; callers must not write to them."""
        if self._inputs is None:
            g = torch.Generator().manual_seed(7000 + self.index)
            R, S, C = self.rays, self.steps, self.ch
            rs = torch.randn(1, R, S, C + 1, generator=g)
            rs[..., -1] *= 3
            rs[0, 0, :, -1] = -30.0
            rs[0, 1, :, -1] = 50.0
            z = torch.sort(torch.rand(1, R, S, 1, generator=g) * 1.05 + 2.25, dim=2)[0]
            j = 63 if S > 64 else (S - 1) // 2
            z[0, 2, j + 1] = z[0, 2, j]
            d = torch.tensor(_DIRS)[torch.arange(R) % len(_DIRS)][None].contiguous()
            noise = torch.randn(1, R, S, 1, generator=g)
            self._inputs = (rs, d, z, noise)
        return self._inputs

    def equal_depths_at(self):
        return 63 if self.steps > 64 else (self.steps - 1) // 2

    def dir_norms(self):
        return torch.tensor(_DIR_NORMS)[torch.arange(self.rays) % len(_DIRS)]


CASES = tuple(Case(i, *row) for i, row in enumerate(_TABLE))
LDS_CASES = tuple(c for c in CASES if c.form != 'fallback')
RUNS = tuple((c, m) for c in CASES for m in CLAMP_MODES)


def offset_view(x, pad=4):
    """The same values as a contiguous view that starts one float into a larger buffer (on x's device): the allocation is 16-byte aligned
    or better, so the view's address is 4 mod 16."""
    buf = torch.empty(x.numel() + pad, dtype=x.dtype, device=x.device)
    view = buf[1:1 + x.numel()].view(x.shape)
    view.copy_(x)
    assert view.is_contiguous() and view.data_ptr() % 16 == 4
    return view


# ---- references, computed once per (case, clamp mode) and shared -------------------------------------------------------------------------

_refs = {}


def scaled_noise(case, clamp_mode):
    return case.inputs()[3] * NOISE_STD if case.has_noise(clamp_mode) else None


def reference(case, clamp_mode):
    """(float64 (rgb, depth, weights) of oracle/ops.py's sequential loop, the float32 tensor definition's (rgb, depth, weights) on the CPU)."""
    key = (case.index, clamp_mode)
    if key not in _refs:
        from oracle import ops as oracle_ops
        from training import volumetric_rendering as vr
        rs, d, z, _ = case.inputs()
        kw = case.kwargs(clamp_mode)
        nz = scaled_noise(case, clamp_mode)
        want = oracle_ops.composite(rs, d, z, noise=nz, keep_double=True, **kw)
        with torch.no_grad():
            defn = vr._fancy_integration_torch(rs, d, z, nz, kw['last_back'], kw['white_back'], kw['max_depth'], clamp_mode, kw['fill_mode'])
        _refs[key] = (want, defn)
    return _refs[key]


QUANTITIES = ('rgb', 'depth', 'weights')
ACCEPTED = {'rgb': (2e-5, 2e-5), 'depth': (2e-5, 2e-5), 'weights': (2e-5, 1e-6)}          # (rtol, atol): the project's bounds for compositing
ULP = 2.0 ** -23


def max_err(got, want64):
    return float((got.detach().cpu().double() - want64).abs().max())


# The floor of the tight bound.  Four float32 ulps were enough up to 96 samples and no longer at 129: the transmittance is a product of one expf per
# sample, and the device's expf (the platform's math library, not the code under test) errs to one side on these arguments, by 0.03 to 0.12
# ulp in the mean (a CPU's: within 0.04 of zero; single errors up to 0.63 ulp against 0.55).  A mean error adds up linearly over the product:
# measured at 1024 samples, 1024 x 0.109 ulp x 2^-24 x T = 3.2e-6 of the last weight (T = 0.487), and the tensor definition run on the
# device in float32 carries the same 3.1e-6 where a CPU's carries 1.4e-7.  So the floor grants 1/8 ulp (of a factor below 1: 2^-24) per
# sample on top of the four, = (4 + steps / 16) ulps of max(1, max |ref|), and is capped per quantity at twice the worst error the kernel was
# measured at over this table (colour 6.873e-6, depth 2.318e-6, weights 3.059e-6; all at 1024 samples).
MEASURED_WORST = {'rgb': 6.873e-6, 'depth': 2.318e-6, 'weights': 3.059e-6}


def floor(quantity, steps, want64):
    return min(2.0 * MEASURED_WORST[quantity], (4.0 + steps / 16.0) * ULP * max(1.0, float(want64.abs().max())))


def tight_bound(quantity, steps, defn, want64):
    """max(2 x the float32 definition's max-norm error against float64 on the CPU, the floor above)."""
    return max(2.0 * max_err(defn, want64), floor(quantity, steps, want64))
