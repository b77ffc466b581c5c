"""The fused ray-marcher applies the decoders' output layers once per ray: `sum_i w_i (W1 h_i + b1) = W1 (sum_i w_i h_i) + b1 sum_i w_i`
(`render_rays_kernel`, ide-3d_amd/csrc/raymarch.hip).  These cases aim at the terms of that identity, against the float64 oracle, through the
helpers and at the tolerances of tests/test_gpu_raymarch.py (features 3e-4 of the feature scale, depth and weight sum 1e-4).  `pytest -m gpu`.

* `bias_relu*`: output biases of several units on rays whose weight sum is well below 1 (`clamp_mode='relu'`, densities centred at 0): the
  `b1 * wsum` term, with and without `white_back` (which adds `1 - wsum` after it).
* `octave_rows`: every output row (weights and bias; not the density row, which would saturate every ray) scaled by 2^U(-8, 8), and every
  output channel held to 3e-4 of its OWN scale: a small row's error cannot hide behind a large row's.  The scaling is exact (powers of
  two), so a channel's error relative to its own scale is expected to be what it is unscaled.
* `s1_*`, `s17_*`, `s96_*`: one sample per ray, a partial last tile and six whole tiles, with no semantic channels (the geometry branch
  is the density row alone) and with the widest decoder (all 32 output rows of both branches).

Every case runs in the three compiled forms of the kernel and asserts that the fused kernel ran exactly once.
"""

import numpy as np
import pytest
import torch

from test_gpu_raymarch import DEPTH_TOL, FEAT_TOL, FORMS, _arithmetic, _calls, _oracle, _rel, _render, _setup

pytestmark = pytest.mark.gpu

WIDEST = dict(feature_channels=32, seg_channels=31)
NO_SEG = dict(feature_channels=3, seg_channels=0)

CASES = {
    'bias_relu': dict(n=4, size=12, steps=17, clamp_mode='relu', big_bias=True),
    'bias_relu_white': dict(n=4, size=12, steps=17, clamp_mode='relu', big_bias=True, white_back=True),
    'octave_rows': dict(n=2, size=12, steps=33, noise=True, octaves=True),
    's1_widest': dict(n=3, size=9, steps=1, jitter=False, spec=WIDEST),
    's1_no_seg': dict(n=3, size=9, steps=1, jitter=False, spec=NO_SEG),
    's17_no_seg': dict(n=2, size=9, steps=17, noise=True, spec=NO_SEG),
    's96_widest': dict(n=2, size=8, steps=96, spec=WIDEST),
    's96_no_seg': dict(n=2, size=8, steps=96, spec=NO_SEG),
}


def _shape_decoder(R, case, seed):
    """Rewrite the output layers of the renderer `_setup` made, in place; row 0 of the geometry layer (the density) is left alone.
    -> the state dict the oracle reads."""
    g = torch.Generator().manual_seed(seed + 5)
    dec = R.decoder
    with torch.no_grad():
        if case.get('big_bias'):
            # effective biases ~ N(0, 4^2): several times the features the weights produce
            for layer, first in ((dec.tex1, 0), (dec.geo1, 1)):
                b = torch.randn(layer.bias.shape[0] - first, generator=g) * 4.0 / layer.bias_gain
                layer.bias[first:] = b.to(layer.bias.device)
        if case.get('octaves'):
            for layer, first in ((dec.tex1, 0), (dec.geo1, 1)):
                k = torch.exp2(torch.rand(layer.bias.shape[0] - first, generator=g) * 16 - 8).to(layer.bias.device)
                layer.weight[first:] *= k[:, None]
                layer.bias[first:] *= k
    return {'synthesis.renderer.' + k: v.detach().cpu().clone() for k, v in R.state_dict().items()}


@pytest.mark.parametrize('case_id', list(CASES))
@pytest.mark.parametrize('form', list(FORMS))
def test_per_ray_output_layers_vs_float64(gpu_device, form, case_id):
    case = CASES[case_id]
    seed = 200 + sorted(CASES).index(case_id) * 10 + sorted(FORMS).index(form)
    R, sd, osp, tex, geo, tex_c, geo_c, cam, jit, noise = _setup(form, case, seed)
    sd = _shape_decoder(R, case, seed)
    n, size = case['n'], case['size']
    with _arithmetic(FORMS[form][0]):
        before = _calls('render_rays')
        feat, depth, wsum = _render(R, osp, tex, geo, cam, jit, noise, case)
        assert _calls('render_rays') - before == 1, 'the fused kernel must have run exactly once'
    nch = osp.feature_channels + osp.seg_channels
    assert feat.shape == (n, nch, size, size) and depth.shape == wsum.shape == (n, 1, size, size)
    want_f, want_d, want_w = _oracle(sd, osp, tex_c, geo_c, cam, jit, noise, case.get('white_back', False), case.get('max_depth'))
    got_f, got_d, got_w = feat.reshape(n, nch, -1).transpose(1, 2), depth.reshape(n, -1), wsum.reshape(n, -1)
    assert bool(torch.isfinite(want_f).all()) and bool(torch.isfinite(want_d).all())
    if case.get('big_bias'):
        # the b1 * wsum term is only exercised where the weight sum is visibly short of 1
        assert float((1 - want_w).max()) > 0.05, 'relu case: every ray saturated, the bias term is not separated from the bias'
    err = (got_f.cpu().double() - want_f.double()).abs()
    ch_err, ch_scale = err.amax(dim=(0, 1)), want_f.double().abs().amax(dim=(0, 1))
    print(f'\n{form} {case_id}: features err {float(err.max()):.3e} of scale {float(want_f.abs().max()):.3e} '
          f'(worst channel {float((ch_err / ch_scale).max()):.3e} of its own scale); '
          f'depth {float((got_d.cpu().double() - want_d.double()).abs().max() / want_d.abs().max()):.3e}; '
          f'weight sum {float((got_w.cpu().double() - want_w.double()).abs().max() / want_w.abs().max()):.3e}; '
          f'max(1 - wsum) {float((1 - want_w).max()):.3f}')
    if case.get('octaves'):
        assert float(ch_scale.max() / ch_scale.min()) > 2.0 ** 6, 'the rows must span many octaves'
        for ch in range(nch):
            _rel(got_f[..., ch], want_f[..., ch], FEAT_TOL, f'{form} {case_id} feature channel {ch}')
    _rel(got_f, want_f, FEAT_TOL, f'{form} {case_id} features')
    _rel(got_d, want_d, DEPTH_TOL, f'{form} {case_id} depth')
    _rel(got_w, want_w, DEPTH_TOL, f'{form} {case_id} weight sum')
