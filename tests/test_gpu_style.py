"""The style preparation kernels (csrc/style.hip: `style_affine_kernel`, `style_demod_kernel`, `fold_heads_kernel` and their batch forms) at
their edges against the float64 formulas.  Needs a real MI355X: `pytest -m gpu`.

References and the derivation of every bound constant are in tests/style_ref.py: styles within (D + 4) u of the magnitude of their sum, D the
rounding depth of the path taken (16-byte loads or scalar); dcoefs, computed from the kernel's OWN styles, within
((34 + ceil(cin / 32)) / 2 + 3) u relative; folded head weights within |W| E_s + u |W s|.  The cases and the routes they are built for are
in tests/style_cases.py; tests/test_mapping_style_ref_cpu.py asserts the routes and shows that a model of the kernels' summation order stays
inside the bounds while a dropped tail slab, a bias row off by one or a skipped lane leaves them by more than 100 x.

Every test prints its worst error / bound and checks `hip_plugin.CALLS` for the native call.
"""

import pytest
import torch

import style_cases
import style_ref

pytestmark = pytest.mark.gpu


def _calls(name):
    from torch_utils import hip_plugin
    return hip_plugin.CALLS.get(name, 0)


def _ratio(got, ref, bound):
    g = got.detach().cpu().double()
    assert g.shape == ref.shape and bool(torch.isfinite(g).all())
    return float(((g - ref).abs() / bound).max())


def _check_style(got_s, got_d, w, A, b, a_gain, b_gain, wsq_t, vec):
    """(styles, dcoefs) of one job against the references; w, A, b, wsq_t are the CPU originals."""
    ref, bound = style_ref.styles(w, A, b, a_gain, b_gain, vec)
    rs = _ratio(got_s, ref, bound)
    rd = 0.0
    if wsq_t is None:
        assert got_d is None
    else:
        dref, dbound = style_ref.dcoefs(got_s.detach().cpu(), wsq_t)
        rd = _ratio(got_d, dref, dbound)
    return rs, rd


@pytest.mark.parametrize('shape,mis,want', style_cases.STYLE_CASES, ids=['x'.join(map(str, c[0])) for c in style_cases.STYLE_CASES])
def test_style_demod_within_the_bounds(gpu_device, shape, mis, want):
    from torch_utils import hip_plugin
    n, cin, cout, wdim = shape
    worst = [0.0, 0.0]
    before = _calls('style_demod')
    for has_bias, bias_gain, form in style_cases.VARIANTS:
        w, A, b, wsq_t, a_gain = style_cases.style_inputs(shape, has_bias, form)
        wd = style_cases.latent_to(w, gpu_device)
        assert wd.stride() == w.stride() or form == 'column'
        Ad = style_cases._offset(A, mis, gpu_device)
        assert style_cases.route(shape, Ad.data_ptr()) == want
        s, d = hip_plugin.StylePlugin.style_demod(wd, Ad, None if b is None else b.to(gpu_device), a_gain, bias_gain,
                                                  None if wsq_t is None else wsq_t.to(gpu_device))
        rs, rd = _check_style(s, d, w, A, b, a_gain, bias_gain, wsq_t, want['vec'])
        worst = [max(worst[0], rs), max(worst[1], rd)]
    assert _calls('style_demod') == before + len(style_cases.VARIANTS)
    print(f"style_demod {shape} ({'16-byte' if want['vec'] else 'scalar'} path): worst error / bound styles {worst[0]:.3f} dcoefs {worst[1]:.3f}")
    assert max(worst) <= 1.0


@pytest.mark.parametrize('wdim', [30, 260])
def test_fold_heads_within_the_bound(gpu_device, wdim):
    """Each launch has one head's affine weight 16-byte aligned and the other's not: at w_dim 260 the two halves of a workgroup take different
    paths; at w_dim 30 both are scalar whatever the alignment."""
    from torch_utils import hip_plugin
    worst = {True: 0.0, False: 0.0}
    before = _calls('fold_heads')
    cases = [c for c in style_cases.FOLD_CASES if c[2] == wdim]
    for cin, heads, _, mis0 in cases:
        w, a_gain, A0, b0, W0, g0, A1, b1, W1, g1 = style_cases.fold_inputs(cin, heads, wdim)
        A0d, A1d = style_cases._offset(A0, mis0, gpu_device), style_cases._offset(A1, not mis0, gpu_device)
        vec0, vec1 = style_ref.is_vec(wdim, A0d.data_ptr()), style_ref.is_vec(wdim, A1d.data_ptr())
        assert (vec0, vec1) == ((not mis0, mis0) if wdim % 4 == 0 else (False, False))
        dv = lambda t: t.to(gpu_device)
        out = hip_plugin.StylePlugin.fold_heads(style_cases.latent_to(w, gpu_device), a_gain, A0d, dv(b0), dv(W0), g0, A1d, dv(b1), dv(W1), g1)
        assert out.shape == (style_cases.FOLD_N, sum(heads), cin, 1, 1)
        ref, bound = style_ref.fold_heads(w, a_gain, A0, b0, W0, g0, vec0, A1, b1, W1, g1, vec1)
        worst[mis0] = max(worst[mis0], _ratio(out.reshape(ref.shape), ref, bound))
    assert _calls('fold_heads') == before + len(cases)
    print(f'fold_heads w_dim {wdim}: worst error / bound {worst[False]:.3f} (head 0 aligned), {worst[True]:.3f} (head 0 misaligned)')
    assert max(worst.values()) <= 1.0


@pytest.mark.parametrize('name', list(style_cases.BATCH_LISTS))
def test_style_batch_is_bit_equal_to_per_layer_and_within_the_bounds(gpu_device, name):
    from torch_utils import hip_plugin
    P = hip_plugin.StylePlugin
    n, wdim, ws, jobs = style_cases.batch_inputs(name)
    wsd = ws.to(gpu_device)
    dv = lambda t: None if t is None else t.to(gpu_device)
    djobs = [(wsd[:, k], dv(A), dv(b), ag, bg, dv(wsq)) for k, (_, A, b, ag, bg, wsq) in enumerate(jobs)]
    before = _calls('style_demod_batch')
    got = P.style_demod_batch(djobs)
    assert _calls('style_demod_batch') == before + style_ref.cdiv(len(jobs), style_ref.BATCH_MAX)
    assert len(got) == len(jobs)
    worst = [0.0, 0.0]
    for (w, A, b, ag, bg, wsq), dj, (s, d) in zip(jobs, djobs, got):
        s1, d1 = P.style_demod(*dj)
        assert torch.equal(s, s1), f'{name}: batch styles differ from the per-layer call'
        assert (d is None and d1 is None and wsq is None) or torch.equal(d, d1), f'{name}: batch dcoefs differ from the per-layer call'
        rs, rd = _check_style(s, d, w, A, b, ag, bg, wsq, style_ref.is_vec(wdim, dj[1].data_ptr()))
        worst = [max(worst[0], rs), max(worst[1], rd)]
    if name == 'all_plain':
        assert all(d is None for _, d in got), 'no job asks for demodulation: the second launch has nothing to write'
    print(f'style_demod_batch {name}: worst error / bound styles {worst[0]:.3f} dcoefs {worst[1]:.3f}')
    assert max(worst) <= 1.0


def test_style_batch_declines_nine_images(gpu_device):
    from torch_utils import hip_plugin
    g = torch.Generator().manual_seed(3)
    jobs = [(torch.randn(9, 36, generator=g).to(gpu_device), torch.randn(33, 36, generator=g).to(gpu_device), None, 1 / 6, 1.0, None)]
    before = _calls('style_demod_batch')
    assert hip_plugin.StylePlugin.style_demod_batch(jobs) is None
    assert _calls('style_demod_batch') == before


def test_fold_heads_batch_is_bit_equal_to_per_layer(gpu_device):
    """Head jobs with cin 1, 63, 65 and 130 in one launch (block counts 1, 1, 2, 3) == the per-layer calls, which
    `test_fold_heads_within_the_bound` holds to the bound."""
    from torch_utils import hip_plugin
    P = hip_plugin.StylePlugin
    dv = lambda t: t.to(gpu_device)
    jobs = []
    ws = None
    for cin, heads, wdim, mis0 in [c for c in style_cases.FOLD_CASES if c[2] == 260 and c[1] == (3, 19)]:
        w, a_gain, A0, b0, W0, g0, A1, b1, W1, g1 = style_cases.fold_inputs(cin, heads, wdim)
        ws = style_cases.latent_to(w, gpu_device) if ws is None else ws
        jobs.append((ws, a_gain, style_cases._offset(A0, mis0, gpu_device), dv(b0), dv(W0), g0,
                     style_cases._offset(A1, not mis0, gpu_device), dv(b1), dv(W1), g1))
    before = _calls('fold_heads_batch')
    got = P.fold_heads_batch(jobs)
    assert _calls('fold_heads_batch') == before + 1 and len(got) == len(jobs) == 8
    for j, o in zip(jobs, got):
        assert torch.equal(o, P.fold_heads(*j))
