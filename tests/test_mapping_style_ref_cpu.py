"""The instruments of the mapping / style edge suites (tests/test_gpu_mapping.py, tests/test_gpu_style.py), checked without a GPU:

  * the float64 references (mapping_ref, style_ref) equal the module's CPU path, to fp32 rounding: they are pinned to the definition;
  * a float32 model of each kernel's summation order (kernel_emul) stays within the derived bounds on every case of the GPU suites:
    the chosen inputs keep a correct implementation inside its bound before a GPU is involved;
  * the same model with one seeded defect leaves the bound by at least 100 x: the bounds are sharp enough to catch a dropped tail slab, a
    bias row off by one, a skipped lane and a wrong image clamp;
  * the case tables reach the routes they were built for (the host / kernel conditions restated in mapping_cases.route, style_cases.route).
"""

import math

import numpy as np
import pytest
import torch

import kernel_emul
import mapping_cases
import mapping_ref
import style_cases
import style_ref
from util import assert_close


# ---- references == the module's CPU path -----------------------------------------------------------------------------------------

@pytest.mark.parametrize('z_dim,c_dim,w_dim,num_ws,layers', [(32, 25, 32, 12, 2), (64, 0, 48, 5, 3), (0, 3, 8, 4, 1), (10, 1, 16, 3, 2)])
def test_mapping_reference_is_the_modules_cpu_path(z_dim, c_dim, w_dim, num_ws, layers):
    from training import networks
    torch.manual_seed(11)
    kw = dict(embed_features=6) if z_dim == 10 else {}
    M = networks.MappingNetwork(z_dim, c_dim, w_dim, num_ws, num_layers=layers, **kw).eval()
    fcs = [getattr(M, f'fc{i}') for i in range(layers)]
    with torch.no_grad():
        M.w_avg.copy_(torch.randn(w_dim) * 0.3)
        for fc in fcs:
            fc.bias.copy_(torch.randn_like(fc.bias))
        if c_dim:
            M.embed.bias.copy_(torch.randn_like(M.embed.bias))
    z = torch.randn(3, z_dim) if z_dim else None
    c = torch.randn(3, c_dim) if c_dim else None
    emb = M.embed if c_dim else None
    for psi, cutoff in ((1, None), (0.7, None), (0.3, 3), (0.7, -2), (0.7, 0), (1.5, num_ws + 3), (0.7, -num_ws - 3)):
        with torch.no_grad():
            want = M(z, c, truncation_psi=psi, truncation_cutoff=cutoff)
        got = mapping_ref.forward(z if z is not None else torch.zeros(3, 0), c, emb.weight if emb else None, emb.bias if emb else None,
                                  emb.weight_gain if emb else 1.0, emb.bias_gain if emb else 1.0, [f.weight for f in fcs], [f.bias for f in fcs],
                                  fcs[0].bias_gain, 0.2, math.sqrt(2), num_ws, M.w_avg, psi, cutoff)
        assert_close(got, want, rtol=1e-4, atol=1e-5, what=f'mapping_ref z{z_dim} c{c_dim} psi{psi} cutoff{cutoff}')


def test_slice_cutoff_is_the_python_slice():
    for num_ws in (1, 12, 18):
        for cutoff in (None, 0, 1, num_ws - 1, num_ws, num_ws + 3, -1, -2, -num_ws + 1, -num_ws, -num_ws - 3):
            assert mapping_ref.slice_cutoff(cutoff, num_ws) == torch.zeros(2, num_ws)[:, :cutoff].shape[1]


@pytest.mark.parametrize('shape', [(3, 33, 33, 260), (2, 7, 5, 30), (2, 65, 31, 100)])
def test_style_references_are_the_modules_cpu_path(shape):
    from training import networks
    n, cin, cout, wdim = shape
    w, A, b, _, a_gain = style_cases.style_inputs(shape, True, 'column')
    g = torch.Generator().manual_seed(5)
    W = torch.randn(cout, cin, 3, 3, generator=g)
    aff = networks.FullyConnectedLayer(wdim, cin, bias_init=1)
    with torch.no_grad():
        aff.weight.copy_(A); aff.bias.copy_(b)
        s_mod = aff(w)
        d_mod = ((W.unsqueeze(0) * s_mod.reshape(n, 1, -1, 1, 1)).square().sum(dim=[2, 3, 4]) + 1e-8).rsqrt()       # modulated_conv2d, fused form
    assert math.isclose(aff.weight_gain, a_gain) and aff.bias_gain == 1
    s_ref, _ = style_ref.styles(w, A, b, a_gain, 1.0, vec=True)
    assert_close(s_ref, s_mod, rtol=1e-5, atol=1e-5, what='styles')
    wsq_t = W.double().square().sum(dim=[2, 3]).t().contiguous().float()
    d_ref, _ = style_ref.dcoefs(s_mod, wsq_t)
    assert_close(d_ref, d_mod, rtol=1e-5, atol=0, what='dcoefs')
    # the heads (ToRGBLayer.forward: styles = affine(w) * weight_gain; modulated weight = W * styles)
    rgb, seg = networks.ToRGBLayer(cin, 3, wdim), networks.ToRGBLayer(cin, 19, wdim)
    with torch.no_grad():
        for head in (rgb, seg):
            head.affine.weight.copy_(torch.randn(cin, wdim, generator=g)); head.affine.bias.copy_(torch.randn(cin, generator=g) + 1)
        want = torch.cat([h.weight.reshape(h.weight.shape[0], cin)[None] * (h.affine(w) * h.weight_gain)[:, None, :] for h in (rgb, seg)], dim=1)
    ref, _ = style_ref.fold_heads(w, rgb.affine.weight_gain, rgb.affine.weight.detach(), rgb.affine.bias.detach(), rgb.weight.detach().reshape(3, cin), rgb.weight_gain, True,
                                  seg.affine.weight.detach(), seg.affine.bias.detach(), seg.weight.detach().reshape(19, cin), seg.weight_gain, True)
    assert_close(ref, want, rtol=1e-5, atol=1e-5, what='folded heads')


# ---- routes ----------------------------------------------------------------------------------------------------------------------

def test_mapping_cases_reach_their_routes():
    seen = dict(rows=False, block=False, alternating=False, odd_per=False, idle=False, two_blocks=False, short_block=False)
    for c in mapping_cases.CASES:
        r = mapping_cases.route(c)
        for key, want in c['route'].items():
            assert r[key] == want, f"case {c['name']}: {key} is {r[key]}, built for {want}"
        ob = r['one_block']
        seen['rows'] |= not all(ob); seen['block'] |= any(ob)
        seen['alternating'] |= any(a != b for a, b in zip(ob, ob[1:]))
        seen['odd_per'] |= any(p % 2 == 1 and p > 1 for p in r['per'])
        seen['idle'] |= any(r['idle'])
        seen['two_blocks'] |= r['blocks'] == 2 and c['n'] == 8
        seen['short_block'] |= r['blocks'] == 2 and c['n'] % mapping_cases.NB in (1, 3)
        k = c['z_dim'] + c['embed']
        assert k % 4 == 0 and all(o % 4 == 0 and 0 < o <= 1024 for o in c['widths']) and 1 <= c['n'] <= 8 and len(c['widths']) <= 16
    assert all(seen.values()), seen
    assert [c['widths'] for c in mapping_cases.CASES if c['name'] == 'i'] == [[8] * 16]
    assert mapping_cases.PSI_BELOW_HALF < 0.5 and np.float32(mapping_cases.PSI_BELOW_HALF) == np.nextafter(np.float32(0.5), np.float32(0))


def test_style_cases_reach_their_routes():
    for shape, mis, want in style_cases.STYLE_CASES:
        A = style_cases._offset(torch.zeros(shape[1], shape[3]), mis)
        assert A.is_contiguous() and (A.data_ptr() % 16 != 0) == mis
        assert style_cases.route(shape, A.data_ptr()) == want, (shape, style_cases.route(shape, A.data_ptr()), want)
    routes = [w for _, _, w in style_cases.STYLE_CASES]
    assert any(not r['vec'] for r in routes) and any(r['chunks'] == 2 for r in routes) and {r['groups'] for r in routes} >= {0, 1, 2, 3}
    assert len(style_cases.BATCH_LISTS['jobs24'][2]) == style_ref.BATCH_MAX and len(style_cases.BATCH_LISTS['jobs25'][2]) == style_ref.BATCH_MAX + 1
    assert style_cases.BATCH_LISTS['first_plain'][2][0][1] == 0 and style_cases.BATCH_LISTS['last_plain'][2][-1][1] == 0
    assert all(co == 0 for _, co, _ in style_cases.BATCH_LISTS['all_plain'][2])
    assert {ci for ci, _, _ in style_cases.BATCH_LISTS['max_cin'][2]} >= {1, 33, 520}
    for w in (style_cases.latent(f, 3, 8, torch.Generator().manual_seed(0)) for f in ('contiguous', 'column', 'expanded')):
        assert w.stride(1) == 1
    assert style_cases.latent('expanded', 3, 8, torch.Generator().manual_seed(0)).stride(0) == 0


# ---- the modelled kernels stay inside the bounds; seeded defects do not --------------------------------------------------------------

def _np(t):
    return None if t is None else t.numpy()


def _emulate_mapping(c, defect=None, at_layer=None):
    """The telescoped activations of the model.  A defect is applied at one layer only (`at_layer`): the check takes the model's own
    previous activation as the next layer's input, exactly as the GPU test does."""
    t = mapping_cases.tensors(c)
    x = kernel_emul.mapping_input(_np(t['z']), _np(t['c']), _np(t['embed_w']), _np(t['embed_b']), t['embed_wgain'], t['embed_bgain'])
    acts = []
    for l, (w, b) in enumerate(zip(t['fc_w'], t['fc_b'])):
        x = kernel_emul.mapping_layer(x, _np(w), _np(b), mapping_cases.LR, mapping_cases.ALPHA, mapping_cases.GAIN,
                                      defect if l == at_layer else None)
        acts.append(x)
    return acts


@pytest.mark.parametrize('name', [c['name'] for c in mapping_cases.CASES])
def test_modelled_mapping_kernel_is_within_the_bounds(name):
    c = mapping_cases.BY_NAME[name]
    ratios = mapping_cases.check(c, _emulate_mapping(c))
    print(f'mapping model {name}: worst error / bound per layer {[round(r, 3) for r in ratios]}')
    assert max(ratios) <= 1.0


def test_modelled_truncation_is_within_the_bound():
    c = mapping_cases.BY_NAME['b']
    x = _emulate_mapping(c)[-1]
    a = mapping_cases.tensors(c)['w_avg'].numpy()
    F = np.float32
    worst = 0.0
    for num_ws in (1, 18):
        for psi in (1, 0.7, 0.5, mapping_cases.PSI_BELOW_HALF, 0.3, 0, -0.5, 1.5):
            for cutoff in (None, 0, 1, num_ws - 1, num_ws, num_ws + 3, -1, -num_ws - 1):
                p = F(psi)
                d = (x - a).astype(F)
                v = (a + (p * d).astype(F)).astype(F) if abs(p) < 0.5 else (x - (d * (F(1) - p)).astype(F)).astype(F)
                k = mapping_ref.slice_cutoff(cutoff, num_ws) if p != 1 else 0
                got = np.repeat(x[:, None, :], num_ws, axis=1)
                got[:, :k] = v[:, None, :]
                worst = max(worst, mapping_cases.check_truncation(x, torch.from_numpy(a), got, num_ws, psi, cutoff))
    print(f'truncation model: worst error / bound {worst:.3f}')
    assert worst <= 1.0


# (case, layer) at which each defect can show: a partial last slab, a bias, 64 lanes' worth of columns, two images
_MAPPING_DEFECTS = [('drop_tail_slab', 'd', 0), ('drop_tail_slab', 'd', 3),('drop_tail_slab', 'b', 1), ('drop_tail_slab', 'g2', 0),
                    ('bias_next_row', 'b', 0), ('bias_next_row', 'c', 1), ('bias_next_row', 'e8', 1), ('bias_next_row', 'h1', 2),
                    ('skip_lane_63', 'f', 0), ('skip_lane_63', 'e5', 1), ('skip_lane_63', 'd', 1),
                    ('image_clamp', 'c', 0), ('image_clamp', 'e5', 1), ('image_clamp', 'f', 1), ('image_clamp', 'g3', 0),
                    ('image_clamp', 'j', 0), ('skip_lane_63', 'j', 1)]


@pytest.mark.parametrize('defect,name,layer', _MAPPING_DEFECTS)
def test_seeded_mapping_defect_leaves_the_bound(defect, name, layer):
    c = mapping_cases.BY_NAME[name]
    ratios = mapping_cases.check(c, _emulate_mapping(c, defect, layer))
    print(f'mapping model {name} layer {layer} with {defect}: error / bound {ratios[layer]:.3g}')
    assert ratios[layer] >= 100.0
    assert all(r <= 1.0 for l, r in enumerate(ratios) if l != layer), 'the telescoped check must confine a fault to its layer'


def _style_ratios(shape, mis, has_bias, bias_gain, form, defect=None):
    n, cin, cout, wdim = shape
    w, A, b, wsq_t, a_gain = style_cases.style_inputs(shape, has_bias, form)
    vec = style_ref.is_vec(wdim, 4 if mis else 0)
    s = kernel_emul.affine(w.numpy(), A.numpy(), _np(b), a_gain, bias_gain, 1.0, vec, defect)
    ref, bound = style_ref.styles(w, A, b, a_gain, bias_gain, vec)
    rs = float(((torch.from_numpy(s).double() - ref).abs() / bound).max())
    rd = 0.0
    if cout:
        d = kernel_emul.demod(s, wsq_t.numpy())
        dref, dbound = style_ref.dcoefs(torch.from_numpy(s), wsq_t)
        rd = float(((torch.from_numpy(d).double() - dref).abs() / dbound).max())
    return rs, rd


@pytest.mark.parametrize('shape,mis', [(s, m) for s, m, _ in style_cases.STYLE_CASES], ids=['x'.join(map(str, c[0])) for c in style_cases.STYLE_CASES])
def test_modelled_style_kernels_are_within_the_bounds(shape, mis):
    worst = [0.0, 0.0]
    for has_bias, bias_gain, form in style_cases.VARIANTS:
        rs, rd = _style_ratios(shape, mis, has_bias, bias_gain, form)
        worst = [max(worst[0], rs), max(worst[1], rd)]
    print(f'style model {shape}: worst error / bound styles {worst[0]:.3f} dcoefs {worst[1]:.3f}')
    assert max(worst) <= 1.0


@pytest.mark.parametrize('defect,shape,mis', [('drop_tail_slab', (3, 33, 33, 260), False), ('drop_tail_slab', (2, 7, 5, 30), False),
                                               ('drop_tail_slab', (2, 65, 31, 100), True), ('bias_next_row', (3, 33, 33, 260), False),
                                               ('bias_next_row', (2, 65, 31, 100), True), ('skip_lane_63', (4, 96, 64, 1024), False),
                                               ('skip_lane_63', (2, 65, 31, 100), True)])
def test_seeded_style_defect_leaves_the_bound(defect, shape, mis):
    rs, _ = _style_ratios(shape, mis, True, 0.37, 'column', defect)
    print(f'style model {shape} with {defect}: error / bound {rs:.3g}')
    assert rs >= 100.0


@pytest.mark.parametrize('cin,heads,wdim,mis0', style_cases.FOLD_CASES)
def test_modelled_fold_heads_is_within_the_bound(cin, heads, wdim, mis0):
    w, a_gain, A0, b0, W0, g0, A1, b1, W1, g1 = style_cases.fold_inputs(cin, heads, wdim)
    vec0, vec1 = style_ref.is_vec(wdim, 4 if mis0 else 0), style_ref.is_vec(wdim, 0 if mis0 else 4)
    ref, bound = style_ref.fold_heads(w, a_gain, A0, b0, W0, g0, vec0, A1, b1, W1, g1, vec1)
    ratio = {}
    for defect in (None, 'bias_next_row', 'skip_lane_63'):
        got = kernel_emul.fold(w.numpy(), a_gain, A0.numpy(), b0.numpy(), W0.numpy(), g0, vec0, A1.numpy(), b1.numpy(), W1.numpy(), g1, vec1, defect)
        ratio[defect] = float(((torch.from_numpy(got).double() - ref).abs() / bound).max())
    print(f'fold model cin {cin} heads {heads} wdim {wdim} head 0 {"misaligned" if mis0 else "aligned"}: error / bound ' + ', '.join(f'{k}: {v:.3g}' for k, v in ratio.items()))
    assert ratio[None] <= 1.0
    if cin > 1:
        assert ratio['bias_next_row'] >= 100.0
    if wdim > 63:
        assert ratio['skip_lane_63'] >= 100.0
