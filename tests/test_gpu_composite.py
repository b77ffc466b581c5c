"""`ide3d_composite` (csrc/composite.hip) in all four kernel forms against the float64 loop of oracle/ops.py, on the case table of
tests/composite_cases.py (the table itself, and which form each case takes: tests/test_composite_cases_cpu.py).  Needs an MI355X.

Bounds.  The project's accepted compositing bounds (weights rtol 2e-5 / atol 1e-6, colour and depth 2e-5 / 2e-5) hold for every case.  The
bound that catches a subtle error is tighter, per case and quantity in max-norm: the kernel's error against float64 is at most
max(2 x the error of the float32 tensor definition on the CPU for the same inputs, a floor).  The first term measures the reference
arithmetic, not the code under test; the factor 2 is there because the wave's shuffle tree and the 64-sample carry order the products
differently from `cumprod`.  The floor is there because the definition's error is exactly 0 in some cases: 4 float32 ulps of
max(1, max |ref|) plus 1/16 ulp per sample for the one-sided error of the device's expf, capped at twice the kernel's worst measured error
(composite_cases.floor has the reasoning and the figures).

Every run prints `form case quantity error bound ratio`; `test_worst_ratio_per_form` prints the summary that DESIGN.md records."""

import pytest
import torch

import composite_cases as cc
from oracle import ops as oracle_ops
from util import assert_close

pytestmark = pytest.mark.gpu

KEYS = [(c, m, False) for c, m in cc.RUNS] + [(c, m, True) for c, m in cc.RUNS if c.form != 'fallback']
IDS = [f'{c.name}-{m}-' + ('offset' if o else 'aligned') for c, m, o in KEYS]
LDS_RUNS = [(c, m) for c, m in cc.RUNS if c.form != 'fallback']
LDS_IDS = [f'{c.name}-{m}' for c, m in LDS_RUNS]

_results = {}


def _calls():
    from torch_utils import hip_plugin
    return hip_plugin.CALLS.get('composite', 0)


def _device_inputs(case, mode, offset, dev):
    rs, d, z, noise = case.inputs()
    x = rs.to(dev)
    if offset:
        x = cc.offset_view(x)
    return x, d.to(dev), z.to(dev), (noise.to(dev) if case.has_noise(mode) else None)


def _form(case, offset):
    return 'fallback' if offset else case.form


def run(case, mode, offset, dev):
    """fancy_integration on the device, once per (case, clamp mode, buffer): (rgb, depth, weights) on the CPU.  Asserts the kernel form
    through the plan query on the very tensor that is launched, and one `composite` launch."""
    key = (case.index, mode, offset)
    if key not in _results:
        from torch_utils import hip_plugin
        from training import volumetric_rendering as vr
        x, d, z, noise = _device_inputs(case, mode, offset, dev)
        assert hip_plugin.composite_plan(x[0])['form'] == _form(case, offset)
        before = _calls()
        with torch.no_grad():
            out = vr.fancy_integration(x, d, z, dev, noise_std=cc.NOISE_STD if noise is not None else 0, noise=noise, **case.kwargs(mode))
        assert _calls() == before + 1
        _results[key] = tuple(o.cpu() for o in out)
    return _results[key]


@pytest.mark.parametrize('case,mode,offset', KEYS, ids=IDS)
def test_kernel_against_float64(gpu_device, case, mode, offset):
    got = run(case, mode, offset, gpu_device)
    want, defn = cc.reference(case, mode)
    R, S, C = case.rays, case.steps, case.ch
    assert [tuple(g.shape) for g in got] == [(1, R, C), (1, R, 1), (1, R, S, 1)] and all(g.dtype == torch.float32 for g in got)
    form = _form(case, offset) + (' by pointer' if offset else '')
    report = []
    for name, g, w, f in zip(cc.QUANTITIES, got, want, defn):
        err, bound = cc.max_err(g, w), cc.tight_bound(name, case.steps, f, w)
        report.append((name, err, bound))
        print(f'{form:20s} {case.name}-{mode} {name:8s} err {err:.3e} bound {bound:.3e} (definition {cc.max_err(f, w):.3e}) ratio {err / bound:.3f}')
    for name, g, w in zip(cc.QUANTITIES, got, want):
        rtol, atol = cc.ACCEPTED[name]
        assert_close(g, w, rtol=rtol, atol=atol, what=f'{case.name} {mode} {form} {name}')
    for name, err, bound in report:
        assert err <= bound, f'{case.name} {mode} {form} {name}: error {err:.3e} against float64 exceeds {bound:.3e}'


def test_worst_ratio_per_form(gpu_device):
    """The summary of the tight bound: worst error / bound per form and quantity over the table (every ratio is asserted <= 1 above)."""
    worst = {}
    for case, mode, offset in KEYS:
        got, (want, defn) = run(case, mode, offset, gpu_device), cc.reference(case, mode)
        form = _form(case, offset) + (' by pointer' if offset else '')
        for name, g, w, f in zip(cc.QUANTITIES, got, want, defn):
            r = cc.max_err(g, w) / cc.tight_bound(name, case.steps, f, w)
            if r >= worst.get((form, name), (-1.0, ''))[0]:
                worst[(form, name)] = (r, f'{case.name}-{mode}')
    forms = sorted({k[0] for k in worst})
    assert forms == sorted(['fallback', 'fallback by pointer', 'lds8', 'lds20', 'lds40'])
    for form in forms:
        line = ', '.join(f"{name} {worst[(form, name)][0]:.3f} ({worst[(form, name)][1]})" for name in cc.QUANTITIES)
        print(f'worst error / bound, {form}: {line}')
        assert all(worst[(form, name)][0] <= 1.0 for name in cc.QUANTITIES)


@pytest.mark.parametrize('case,mode', LDS_RUNS, ids=LDS_IDS)
def test_lds_forms_equal_the_fallback_bit_for_bit(gpu_device, case, mode):
    """The LDS-staged kernels and the fallback are the same arithmetic in the same order: only where the rows are read from differs."""
    a, b = run(case, mode, False, gpu_device), run(case, mode, True, gpu_device)
    for name, x, y in zip(cc.QUANTITIES, a, b):
        assert torch.equal(x, y), f'{case.name} {mode} {name}: {case.form} and the fallback differ by up to {float((x - y).abs().max()):.3e}'


@pytest.mark.parametrize('case,mode,offset', KEYS, ids=IDS)
def test_without_weights_output(gpu_device, case, mode, offset):
    """want_weights=False (weights == NULL): colour and depth bit-equal to the run that writes the weights."""
    from torch_utils import hip_plugin
    x, d, z, noise = _device_inputs(case, mode, offset, gpu_device)
    kw = case.kwargs(mode)
    R, S = case.rays, case.steps
    before = _calls()
    rgb, depth, w = hip_plugin.VolumeRenderPlugin.composite(
        x[0], z.reshape(R, S), case.dir_norms().to(gpu_device), None if noise is None else (noise * cc.NOISE_STD).reshape(R, S),
        cc.CLAMP_MODES.index(mode), kw['last_back'], kw['white_back'], kw['max_depth'], {None: 0, 'debug': 1, 'weight': 2}[kw['fill_mode']],
        want_weights=False)
    assert _calls() == before + 1 and w is None
    full = run(case, mode, offset, gpu_device)
    assert torch.equal(rgb.cpu(), full[0][0]) and torch.equal(depth.cpu(), full[1][0, :, 0])


@pytest.mark.parametrize('case,mode,offset', KEYS, ids=IDS)
def test_properties(gpu_device, case, mode, offset):
    rgb, depth, w = run(case, mode, offset, gpu_device)
    want, _ = cc.reference(case, mode)
    kw = case.kwargs(mode)
    # the opaque ray: partition of unity
    assert abs(float(w[0, 1].double().sum()) - 1) <= 1e-5
    if mode == 'relu':
        # the transparent ray: every alpha is exactly 0, so nothing is left to round: zeros (ones with white_back, max_depth with max_depth,
        # (1, 0, 0) with 'debug'; with last_back the last sample alone) — bit-equal to the rounded float64 result
        for name, g, r in zip(cc.QUANTITIES, (rgb, depth, w), want):
            assert torch.equal(g[0, 0], r[0, 0].float()), f'{case.name} {name} of the transparent ray'
        if not kw['last_back']:
            assert float(w[0, 0].abs().max()) == 0
            if kw['fill_mode'] is None:
                assert bool((rgb[0, 0] == (1.0 if kw['white_back'] else 0.0)).all())
            assert float(depth[0, 0, 0]) == (cc.MAX_DEPTH if kw['max_depth'] else 0.0)
    if kw['fill_mode'] == 'debug':
        wsum = want[2][0, :, :, 0].sum(-1)          # (no debug case has last_back)
        red = (rgb[0] == torch.tensor([1.0, 0.0, 0.0])).all(-1)
        assert torch.equal(red, wsum < 0.9) and bool(red.any()) and bool((~red).any())
    if kw['fill_mode'] == 'weight':
        assert bool((rgb[0] == rgb[0, :, :1]).all())


@pytest.mark.parametrize('ch', [3, 4, 64])
def test_one_sample(gpu_device, ch):
    """steps == 1.  `fancy_integration` follows the tensor definition there (which drops the lone sample) on every device: no launch, the
    CPU's shapes and values, IndexError with last_back.  `ide3d_composite` itself accepts it as one sample with delta 1e10: the float64
    loop of the oracle defines that value."""
    from torch_utils import hip_plugin
    from training import volumetric_rendering as vr
    g = torch.Generator().manual_seed(70 + ch)
    R = 6
    rs = torch.randn(1, R, 1, ch + 1, generator=g)
    rs[0, 0, 0, -1], rs[0, 1, 0, -1] = -30.0, 50.0
    d = torch.tensor(cc._DIRS)[torch.arange(R) % 5][None].contiguous()
    z = torch.rand(1, R, 1, 1, generator=g) + 2.25
    before = _calls()
    for kw in (dict(clamp_mode='relu'), dict(clamp_mode='softplus', white_back=True, max_depth=5.0)):
        with torch.no_grad():
            got = vr.fancy_integration(rs.to(gpu_device), d.to(gpu_device), z.to(gpu_device), gpu_device, noise_std=0, **kw)
            ref = vr.fancy_integration(rs, d, z, 'cpu', noise_std=0, **kw)
        for a, b in zip(got, ref):
            assert a.device.type == 'cuda' and a.shape == b.shape and torch.equal(a.cpu(), b)
        assert got[2].shape == (1, R, 0, 1)
    with pytest.raises(IndexError):
        vr.fancy_integration(rs.to(gpu_device), d.to(gpu_device), z.to(gpu_device), gpu_device, noise_std=0, clamp_mode='relu', last_back=True)
    assert _calls() == before, 'one sample is not sent to the kernel'
    # the binding's own answer, from an aligned buffer (ch + 1 a multiple of 4: an LDS form) and from an offset view
    dn = torch.tensor(cc._DIR_NORMS)[torch.arange(R) % 5]
    for mode, last_back, white_back, max_depth in (('softplus', False, True, 5.0), ('relu', True, False, None), ('relu', False, False, 5.0)):
        want = oracle_ops.composite(rs, d, z, last_back=last_back, white_back=white_back, max_depth=max_depth, clamp_mode=mode, keep_double=True)
        for offset in (False, True):
            x = rs.to(gpu_device)
            x = cc.offset_view(x) if offset else x
            form = hip_plugin.composite_plan(x[0])['form']
            assert form == ('lds8' if (ch + 1) % 4 == 0 and not offset else 'fallback')
            rgb, depth, w = hip_plugin.VolumeRenderPlugin.composite(x[0], z.reshape(R, 1).to(gpu_device), dn.to(gpu_device), None,
                                                                    cc.CLAMP_MODES.index(mode), last_back, white_back, max_depth, 0)
            for name, a, b in zip(cc.QUANTITIES, (rgb[None], depth[None, :, None], w[None, :, :, None]), want):
                assert a.shape == b.shape
                floor = cc.floor(name, 1, b)
                assert cc.max_err(a, b) <= floor, f'one sample, {ch} channels, {mode}, {form}: {name} off by {cc.max_err(a, b):.3e} > {floor:.3e}'
    assert _calls() == before + 6


def test_refusals_launch_nothing(gpu_device):
    from torch_utils import hip_plugin
    comp = hip_plugin.VolumeRenderPlugin.composite
    dev = gpu_device
    before = _calls()
    with pytest.raises(RuntimeError, match='steps'):
        comp(torch.zeros(3, 1025, 4, device=dev), torch.zeros(3, 1025, device=dev), torch.ones(3, device=dev), None, 0, False, False, None, 0)
    with pytest.raises(RuntimeError, match='debug'):
        comp(torch.zeros(3, 13, 5, device=dev), torch.zeros(3, 13, device=dev), torch.ones(3, device=dev), None, 0, False, False, None, 1)
    with pytest.raises(RuntimeError, match='clamp mode'):
        comp(torch.zeros(3, 13, 4, device=dev), torch.zeros(3, 13, device=dev), torch.ones(3, device=dev), None, 2, False, False, None, 0)
    assert _calls() == before
    rgb, depth, w = comp(torch.zeros(0, 13, 4, device=dev), torch.zeros(0, 13, device=dev), torch.ones(0, device=dev), None, 0, False, False, None, 0)
    assert rgb.shape == (0, 3) and depth.shape == (0,) and w.shape == (0, 13)
