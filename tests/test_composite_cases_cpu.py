"""The compositing case table (tests/composite_cases.py) without a GPU: which kernel form of csrc/composite.hip every case takes, through the
host-only query `ide3d_composite_plan` (the launch goes through the same function); that the table reaches every form with every option;
and that its two references stand: the float64 loop of oracle/ops.py equals the tensor definition evaluated in float64, and the float32
definition stays inside the project's accepted compositing bounds on these inputs, so the GPU suite measures the kernel and not the table.
The pdf-sampling table (tests/pdf_ref.py) is checked the same way at the end."""
import ctypes
import os
import re

import pytest
import torch

import composite_cases as cc
import pdf_ref
from oracle import ops as oracle_ops
from util import assert_close

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _plan(*a, **kw):
    from torch_utils import hip_plugin
    return hip_plugin.composite_plan(*a, **kw)


def test_composite_plan_abi_cpu():
    """Declared in the header, listed, exported, mirrored field for field, and outside the launch counters."""
    from torch_utils import hip_plugin
    src = open(os.path.join(ROOT, 'include', 'ide3d_hip.h')).read()
    assert re.search(r'\bint ide3d_composite_plan\(const void\* rgb_sigma, int64_t rays, int32_t steps, int32_t ch, ide3d_composite_plan_info\* out\);', src)
    body = re.search(r'typedef struct ide3d_composite_plan_info \{(.*?)\} ide3d_composite_plan_info;', src, re.S).group(1)
    body = re.sub(r'/\*.*?\*/', '', body, flags=re.S)
    fields = [(m.group(1), m.group(2)) for m in re.finditer(r'(int32_t|int64_t)\s+(\w+)\s*;', body)]
    ctype = {'int32_t': ctypes.c_int32, 'int64_t': ctypes.c_int64}
    assert [(n, ctype[t]) for t, n in fields] == list(hip_plugin._CompositePlanInfo._fields_)
    enum = re.findall(r'IDE3D_COMPOSITE_([A-Z0-9]+) = (\d)', src)
    assert [(n.lower(), int(v)) for n, v in enum] == list(zip(hip_plugin.COMPOSITE_FORMS, range(4)))
    assert 'ide3d_composite_plan' in hip_plugin.EXPORTED_SYMBOLS
    assert hasattr(ctypes.CDLL(hip_plugin.lib_path()), 'ide3d_composite_plan')
    assert hip_plugin._ABI_VERSION == 8
    hip_plugin.CALLS.clear()
    _plan(0, 5, 13, 6)
    assert not hip_plugin.CALLS, 'a plan query is not a launch'


def test_plan_reports_the_launch_geometry():
    p = _plan(0, 4 * 4096, 96, 52)          # the coarse workload: one 64-thread workgroup per ray, block + pad4(steps) floats of LDS
    assert p == dict(form='lds20', grid=16384, workgroup=64, lds_bytes=(96 * 53 + 96) * 4)
    p = _plan(0, 4 * 4096, 192, 52)         # the hierarchical workload: 4-wave workgroups, capped at 8 per CU, one float per sample and wave
    assert p == dict(form='fallback', grid=2048, workgroup=256, lds_bytes=4 * 192 * 4)
    assert _plan(0, 7, 13, 6) == dict(form='fallback', grid=2, workgroup=256, lds_bytes=4 * 13 * 4)
    assert _plan(0, 8192 + 5, 13, 6)['grid'] == 2048
    assert _plan(0, 2 ** 31 + 7, 13, 3)['grid'] == 2 ** 31 - 1
    assert _plan(0, 0, 13, 3)['form'] == 'lds8'          # no rays: still a plan (the launch returns before it)
    assert _plan(0, 3, 1, 3)['form'] == 'lds8' and _plan(0, 3, 1, 4)['form'] == 'fallback'          # one sample is a shape like any other
    for align in (4, 8, 12):
        assert _plan(align, 7, 96, 52)['form'] == 'fallback'
    assert _plan(4096 + 16, 7, 96, 52)['form'] == 'lds20'


@pytest.mark.parametrize('steps,row,form', [
    (64, 32, 'lds8'), (513, 4, 'lds20'), (27, 76, 'lds20'), (80, 64, 'lds20'), (1024, 5, 'lds20'), (1, 5124, 'lds40'), (61, 84, 'lds40'),
    (157, 64, 'lds40'), (160, 64, 'fallback'), (1, 10236, 'lds40'), (1, 10240, 'fallback'), (1, 10244, 'fallback'), (1024, 10, 'fallback'), (2, 5, 'fallback'), (2, 6, 'lds8')])
def test_plan_thresholds(steps, row, form):
    """Both sides of every condition: block % 4, block <= 2048 / 5120 / 10240 floats, 16 * (block + pad4(steps)) <= 160 KB."""
    assert _plan(0, 5, steps, row - 1)['form'] == form


def test_plan_refuses_what_the_launch_refuses():
    for steps, ch in ((0, 3), (1025, 3), (13, 0)):
        with pytest.raises(RuntimeError):
            _plan(0, 5, steps, ch)
    with pytest.raises(RuntimeError):
        _plan(0, -1, 13, 3)


def test_every_case_takes_the_form_the_table_states():
    for c in cc.CASES:
        rs = c.inputs()[0][0]
        assert rs.shape == (c.rays, c.steps, c.ch + 1) and rs.data_ptr() % 16 == 0
        assert _plan(rs)['form'] == c.form, (c.name, c.why)
        assert _plan(rs.data_ptr(), c.rays, c.steps, c.ch) == _plan(rs)
        if c.form != 'fallback':
            v = cc.offset_view(rs)
            assert torch.equal(v, rs)
            assert _plan(v)['form'] == 'fallback', c.name
        assert 5 <= c.rays <= 9 or c.rays == 8192 + 5


def test_all_forms_occur_and_every_option_occurs_in_every_form():
    seen = {}
    for c, mode in cc.RUNS:
        seen.setdefault(c.form, set()).update(c.opts[mode])
        if c.form != 'fallback':
            seen.setdefault('fallback by pointer', set()).update(c.opts[mode])
    assert set(seen) == {'fallback', 'lds8', 'lds20', 'lds40', 'fallback by pointer'}
    plain = set(cc.OPTION_LETTERS) - {'G'}          # 'debug' needs three colour channels: block = 4 * steps <= 4096, always lds8 when aligned
    for form, opts in seen.items():
        assert opts >= plain, (form, sorted(plain - opts))
    assert 'G' in seen['lds8'] and 'G' in seen['fallback by pointer']
    # the two clamp modes: every case has both
    assert all(set(c.opts) == set(cc.CLAMP_MODES) for c in cc.CASES)
    # what the fallback's chunk loop and channel loop need
    fb = [c for c in cc.CASES if c.form == 'fallback']
    assert {65, 129, 192, 1024} <= {c.steps for c in fb} and any(c.steps == 64 for c in cc.LDS_CASES) and any(c.ch > 192 for c in fb) and any(c.rays > 8192 and c.rays % 4 for c in fb)
    assert any(c.ch == 64 for c in cc.LDS_CASES) and any(c.ch > 128 for c in cc.LDS_CASES) and any(c.steps > 128 for c in cc.LDS_CASES)
    assert any((c.steps * (c.ch + 1) // 4) % 64 for c in cc.LDS_CASES if c.form == 'lds20')          # the tail load beyond the 52-float case


def test_inputs_are_what_the_docstring_says():
    for c in cc.CASES:
        rs, d, z, noise = c.inputs()
        assert bool((rs[0, 0, :, -1] == -30).all()) and bool((rs[0, 1, :, -1] == 50).all())
        assert bool((z[0, :, 1:] >= z[0, :, :-1]).all()) and float(z.min()) >= 2.25 and float(z.max()) <= 3.3
        j = c.equal_depths_at()
        assert float(z[0, 2, j, 0]) == float(z[0, 2, j + 1, 0])
        assert torch.equal(torch.norm(d, p=2, dim=-1)[0], c.dir_norms())
        assert torch.equal(torch.norm(d.double(), p=2, dim=-1)[0], c.dir_norms().double())
        assert torch.equal((noise * cc.NOISE_STD).double(), noise.double() * cc.NOISE_STD)


@pytest.mark.parametrize('case,mode', cc.RUNS, ids=[f'{c.name}-{m}' for c, m in cc.RUNS])
def test_the_two_references_agree_and_the_definition_is_within_bounds(case, mode):
    from training import volumetric_rendering as vr
    rs, d, z, _ = case.inputs()
    kw = case.kwargs(mode)
    nz = cc.scaled_noise(case, mode)
    want, defn = cc.reference(case, mode)
    def64 = vr._fancy_integration_torch(rs.double(), d.double(), z.double(), None if nz is None else nz.double(), kw['last_back'], kw['white_back'],
                                        kw['max_depth'], mode, kw['fill_mode'])
    for name, a, b, f in zip(cc.QUANTITIES, def64, want, defn):
        assert a.dtype == b.dtype == torch.float64 and f.dtype == torch.float32 and a.shape == b.shape == f.shape
        # 1e-12 relative; sums of signed products can cancel, so an absolute 1e-12 of the largest value stands beside it
        assert_close(a, b, rtol=1e-12, atol=1e-12 * max(1.0, float(b.abs().max())), what=f'{case.name} {mode} {name}: definition in float64 vs oracle')
        rtol, atol = cc.ACCEPTED[name]
        assert_close(f, b, rtol=rtol, atol=atol, what=f'{case.name} {mode} {name}: float32 definition vs float64')
    # the properties the GPU suite asserts are properties of the reference too
    wsum = want[2][0, :, :, 0].sum(-1)
    if not kw['last_back']:
        assert abs(float(wsum[1]) - 1) < 1e-8
    if mode == 'relu':          # the transparent ray: exact zeros (with last_back the whole weight goes to the last sample)
        w0 = want[2][0, 0, :, 0]
        assert float(w0[:-1].abs().max()) == 0 and float(w0[-1]) == (1.0 if kw['last_back'] else 0.0)
    if kw['fill_mode'] == 'debug':
        # the threshold rows are decided well away from 0.9, on both sides of it
        assert float((wsum - 0.9).abs().min()) > 1e-3 and bool((wsum < 0.9).any()) and bool((wsum > 0.9).any())
        assert bool((want[0][0][wsum < 0.9] == torch.tensor([1.0, 0.0, 0.0], dtype=torch.float64)).all())


def test_one_sample_follows_the_definition_on_the_cpu():
    """steps == 1: the tensor definition drops the lone sample (its only delta belongs to an empty tensor) and raises with last_back; the
    call surface is the definition there on every device (the GPU suite asserts the routing)."""
    from training import volumetric_rendering as vr
    g = torch.Generator().manual_seed(5)
    rs, d, z = torch.randn(1, 5, 1, 4, generator=g), torch.tensor(cc._DIRS)[None], torch.full((1, 5, 1, 1), 2.5)
    rgb, depth, w = vr.fancy_integration(rs, d, z, 'cpu', noise_std=0, clamp_mode='relu')
    assert w.shape == (1, 5, 0, 1) and rgb.shape == (1, 5, 3) and depth.shape == (1, 5, 1)
    assert float(rgb.abs().max()) == 0 and float(depth.abs().max()) == 0
    rgb, _, _ = vr.fancy_integration(rs, d, z, 'cpu', noise_std=0, clamp_mode='softplus', white_back=True)
    assert bool((rgb == 1).all())
    with pytest.raises(IndexError):
        vr.fancy_integration(rs, d, z, 'cpu', noise_std=0, clamp_mode='relu', last_back=True)
    # the oracle's loop integrates the sample with delta 1e10: what `ide3d_composite` itself returns for steps == 1
    _, _, w1 = oracle_ops.composite(rs, d, z, clamp_mode='softplus')
    assert w1.shape == (1, 5, 1, 1) and bool((w1 == 1).all())


# ---- the pdf-sampling table ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('case', pdf_ref.CASES, ids=[c.name for c in pdf_ref.CASES])
def test_pdf_table_keeps_its_margins_and_the_float32_definition_inverts_the_float64_cdf(case):
    bins, w, u = case.inputs()
    assert bins.shape == (case.rays, case.k + 1) and w.shape == (case.rays, case.k) and u.shape[-1] == case.n
    assert u.ndim == (2 if case.per_ray else 1)
    m = pdf_ref.margins(bins, w, u)
    assert m['bin_mass_to_eps'] >= 1e-6, m
    assert m['draw_to_knot'] >= 1e-5, m
    want = pdf_ref.inverse_cdf64(bins, w, u)
    got = oracle_ops.sample_pdf(bins, w, u if case.per_ray else u[None])
    # away from the knots and from eps both evaluations take the same bin and the same branch: the float32 expression's own rounding is left
    assert got.shape == want.shape == (case.rays, case.n)
    assert float((got.double() - want).abs().max()) <= 5e-6, case.name
    f, tol = pdf_ref.cdf_at(bins, w, got)
    assert bool(((f - pdf_ref.expand(u, case.rays).double()).abs() <= tol).all())


def test_pdf_table_sits_on_the_lane_run_boundaries():
    ks = {c.k for c in pdf_ref.CASES}
    assert {1, 2, 63, 64, 65, 127, 128, 129, 2047, 2048, 94} <= ks
    assert {c.n for c in pdf_ref.CASES} >= {1, 7, 64, 65}
    assert any(c.per_ray for c in pdf_ref.CASES) and any(not c.per_ray for c in pdf_ref.CASES)
    big = [c for c in pdf_ref.CASES if c.rays > 8192]
    assert big and all(c.rays % 4 == 3 for c in big)          # second trip: the last workgroup's fourth wave has no ray
    runs = {}
    for k in (63, 64, 65, 127, 128, 129, 2047, 2048):
        per = -(-k // 64)
        lens = [min(min(lane * per, k) + per, k) - min(lane * per, k) for lane in range(64)]
        assert sum(lens) == k
        runs[k] = (lens.count(0), sum(1 for n in lens if 0 < n < per))          # (empty lanes, short runs)
    assert runs == {63: (1, 0), 64: (0, 0), 65: (31, 1), 127: (0, 1), 128: (0, 0), 129: (21, 0), 2047: (0, 1), 2048: (0, 0)}
