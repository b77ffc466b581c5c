"""A frozen SynthesisLayer with a trainable const noise map on the HIP gradient path (training/networks.py `hip_noise_grad`, DESIGN.md section
5.13): what the reference's projectors do to every layer of `G.synthesis`.  `pytest -m gpu`.

Reference: float64 CPU autograd through the layer's own definition, loss = sum(y * P) with P zeroed within 1e-5 of the lrelu kink (the helpers
of test_gpu_modconv_grad.py).  Errors are the max-abs difference as a fraction of the reference gradient's max-abs, bounded by GRAD_TOL = 1e-4.
The route is asserted through hip_plugin.CALLS."""

import copy

import pytest
import torch

from test_gpu_modconv_grad import GRAD_TOL, _away_from_kinks, _double, _err, _generator, _inputs, _layer, _ws_camera_jitter

pytestmark = pytest.mark.gpu

DEV = torch.device('cuda', 0)
COUNTED = ('bias_noise_grad', 'modconv_act_backward', 'modconv_scale_dot', 'modconv2d')

# (cin, cout, resolution of the output, up); batch 2; noise_strength 0.3 (random init has 0: the map's gradient would vanish)
LAYERS = {'s1_64_16': (64, 64, 16, 1), 'up_64_32_32': (64, 32, 32, 2), 'up_40_24_32_odd_channels': (40, 24, 32, 2)}


def _calls():
    from torch_utils import hip_plugin
    return {k: hip_plugin.CALLS.get(k, 0) for k in COUNTED}


def _run(lay, x, w, P, dev, alone):
    """-> (d noise_const, dx, dws, calls before, after the forward, after the backward); dx and dws None when the map trains alone."""
    lay.noise_const.requires_grad_(True)
    lay.noise_const.grad = None
    x, w = x.to(dev), w.to(dev)
    if not alone:
        x.requires_grad_(True); w.requires_grad_(True)
    c0 = _calls()
    y = lay(x, w, noise_mode='const')
    c1 = _calls()
    (y * P.to(dev, y.dtype)).sum().backward()
    c2 = _calls()
    return lay.noise_const.grad.clone(), x.grad, w.grad, c0, c1, c2


_reference = {}


def _case(case):
    """The layer, its inputs and the float64 gradients (computed once per layer, shared by the tests below, never modified)."""
    if case not in _reference:
        cin, cout, res, up = LAYERS[case]
        lay = _layer(cin, cout, res, up, seed=sum(map(ord, case)) % 1000, noise_strength=0.3)
        x, w = _inputs(2, cin, res // up, 32, seed=1)
        P = torch.randn(2, cout, res, res, generator=torch.Generator().manual_seed(2))
        ref = _double(lay)
        P = _away_from_kinks(ref, x.double(), w.double(), P, 'const')
        dn, dx, dw, *_ = _run(ref, x.double(), w.double(), P, 'cpu', alone=False)
        _reference[case] = (lay, x, w, P, dn, dx, dw)
    return _reference[case]


@pytest.mark.parametrize('alone', [False, True], ids=['with_x_and_ws', 'alone'])
@pytest.mark.parametrize('case', sorted(LAYERS))
def test_noise_map_gradient_against_float64(case, alone):
    from training import networks
    assert networks.hip_noise_grad and networks.hip_conv_grad
    lay, x, w, P, dn_ref, dx_ref, dw_ref = _case(case)
    gpu = copy.deepcopy(lay).to(DEV)
    dn, dx, dw, c0, c1, c2 = _run(gpu, x, w, P, DEV, alone)
    # the route (what fails without `hip_noise_grad`): K1 and K5 ran in the backward
    assert c2['bias_noise_grad'] == c1['bias_noise_grad'] + 1, 'the layer declined the HIP gradient path'
    assert c2['modconv_act_backward'] > c1['modconv_act_backward']
    if alone:
        assert c2['modconv2d'] == c1['modconv2d'], 'the input-gradient convolution ran for a map that trains alone'
        assert c2['modconv_scale_dot'] == c0['modconv_scale_dot']
        assert dx is None and dw is None
    else:
        assert c2['modconv2d'] == c1['modconv2d'] + 1 and c2['modconv_scale_dot'] == c1['modconv_scale_dot'] + 1
        e_dx, e_dw = _err(dx, dx_ref), _err(dw, dw_ref)
        assert e_dx < GRAD_TOL and e_dw < GRAD_TOL, f'dx {e_dx:.2e} dws {e_dw:.2e}'
    e = _err(dn, dn_ref)
    print(f'{case} alone={alone}: d noise_const {e:.2e}')
    assert e < GRAD_TOL, f'd noise_const {e:.2e}'


@pytest.mark.parametrize('case', sorted(LAYERS))
def test_switch_off_keeps_the_aten_definition(case):
    from training import networks
    lay, x, w, P, dn_ref, dx_ref, dw_ref = _case(case)
    gpu = copy.deepcopy(lay).to(DEV)
    networks.hip_noise_grad = False
    try:
        dn, dx, dw, c0, c1, c2 = _run(gpu, x, w, P, DEV, alone=False)
    finally:
        networks.hip_noise_grad = True
    for k in ('bias_noise_grad', 'modconv_act_backward', 'modconv_scale_dot'):
        assert c2[k] == c0[k], k
    assert _err(dn, dn_ref) < GRAD_TOL and _err(dx, dx_ref) < GRAD_TOL and _err(dw, dw_ref) < GRAD_TOL


@pytest.mark.parametrize('case', ['s1_64_16', 'up_64_32_32'])
def test_two_backward_passes_are_bit_identical(case):
    lay, x, w, P, *_ = _case(case)
    gpu = copy.deepcopy(lay).to(DEV)
    a = _run(gpu, x, w, P, DEV, alone=False)[0]
    b = _run(gpu, x, w, P, DEV, alone=False)[0]
    assert torch.equal(a, b)


def test_noise_mode_none_and_random_decline():
    """A trainable map the call does not add (noise_mode 'none'), or random noise, keeps the ATen definition."""
    lay, x, w, P, *_ = _case('s1_64_16')
    gpu = copy.deepcopy(lay).to(DEV)
    gpu.noise_const.requires_grad_(True)
    xg, wg = x.to(DEV).requires_grad_(True), w.to(DEV).requires_grad_(True)
    before = _calls()
    for mode in ('none', 'random'):
        gpu(xg, wg, noise_mode=mode).sum().backward()
    after = _calls()
    for k in ('bias_noise_grad', 'modconv_act_backward', 'modconv_scale_dot'):
        assert after[k] == before[k], k


def test_tiny_spec_step_matches_switch_off():
    """`G.synthesis(ws)` with ws and every noise map trainable (all noise strengths 0.3, the same ray jitter): switch on against switch off,
    every map's gradient and d ws; K5 runs once per noisy layer."""
    from training import networks, projection
    G = _generator({})
    with torch.no_grad():
        for name, p in G.synthesis.named_parameters():
            if name.endswith('noise_strength'):
                p.fill_(0.3)
    G = G.to(DEV)
    ws0, c, jit = _ws_camera_jitter(G, 2, 0)
    maps = projection.noise_maps(G)
    noisy = [m for m in G.synthesis.modules() if isinstance(m, networks.SynthesisLayer) and m.use_noise]
    assert len(maps) == len(noisy) > 0
    for m in maps:
        m.requires_grad_(True)
    with torch.no_grad():
        target = torch.randn_like(G.synthesis(ws0, c=c, noise_mode='const', ray_jitter=jit))
    grads = {}
    for switch in (True, False):
        networks.hip_noise_grad = switch
        try:
            ws = ws0.clone().requires_grad_(True)
            for m in maps:
                m.grad = None
            before = _calls()['bias_noise_grad']
            img = G.synthesis(ws, c=c, noise_mode='const', ray_jitter=jit)
            (img - target).square().mean().backward()
            ran = _calls()['bias_noise_grad'] - before
        finally:
            networks.hip_noise_grad = True
        assert ran == (len(noisy) if switch else 0), f'K5 ran {ran} times for {len(noisy)} noisy layers (switch {switch})'
        grads[switch] = (ws.grad.clone(), [m.grad.clone() for m in maps])
    e_ws = _err(grads[True][0], grads[False][0])
    e_maps = [_err(a, b) for a, b in zip(grads[True][1], grads[False][1])]
    print(f'tiny step, on vs off: d ws {e_ws:.2e}, maps max {max(e_maps):.2e}')
    assert e_ws < 1e-4
    assert max(e_maps) < 1e-4, e_maps
