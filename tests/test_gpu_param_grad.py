"""Parameter gradients of the synthesis convolutions (training/networks.py `hip_param_grad`: ide3d_modconv_weight_grad and
ide3d_bias_noise_grad in csrc/modconv_bwd.hip): the weights, biases, noise strengths and affines of the 3x3, the
up-sampling and the dual-head layers, as PTI pivotal tuning trains them.  `pytest -m gpu`.

Reference: float64 CPU autograd through the layers' own definitions (the differentiable ATen path of the same modules, parameters cast to
float64).  Loss = sum(y * P) with a fixed random projection P kept off the lrelu kinks and the clamp.  Errors are the max-abs difference as
a fraction of the reference gradient's max-abs, bounded by GRAD_TOL.
"""

import copy
import ctypes
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

GRAD_TOL = 1e-4
DEV = torch.device('cuda', 0)
NEW_CALLS = ('modconv_weight_grad', 'bias_noise_grad')
LAYER_PARAMS = ('weight', 'bias', 'noise_strength', 'affine.weight', 'affine.bias')


@pytest.fixture(autouse=True)
def _param_grad_on():
    from training import networks
    old = networks.hip_param_grad
    networks.hip_param_grad = True
    yield
    networks.hip_param_grad = old


def _calls():
    from torch_utils import hip_plugin
    return {k: hip_plugin.CALLS.get(k, 0) for k in NEW_CALLS + ('modconv_act_backward', 'head_weight_grad')}


def _err(actual, expected):
    a = actual.detach().cpu().double(); e = expected.detach().cpu().double()
    assert a.shape == e.shape, f'shape {tuple(a.shape)} != {tuple(e.shape)}'
    return float((a - e).abs().max()) / (float(e.abs().max()) + 1e-30)


def _layer(cin, cout, res, up, seed, act='lrelu', clamp=None, noise_strength=0.3, w_dim=32):
    from training import networks
    torch.manual_seed(seed)
    lay = networks.SynthesisLayer(cin, cout, w_dim=w_dim, resolution=res, up=up, activation=act, conv_clamp=clamp)
    with torch.no_grad():
        lay.bias.normal_(0, 0.5)
        lay.noise_strength.fill_(noise_strength)
        lay.affine.bias.normal_(1, 0.3)
    return lay.requires_grad_(False)


def _double(mod):
    ref = copy.deepcopy(mod).double()
    for m in ref.modules():
        if getattr(m, 'resample_filter', None) is not None:
            m.resample_filter = m.resample_filter.float()
    return ref


def _inputs(n, cin, res_in, w_dim, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(n, cin, res_in, res_in, generator=g) * scale, torch.randn(n, w_dim, generator=g)


def _away_from_kinks(ref, x, w, P, noise_mode):
    """P with zeros where the float64 pre-activation lies within 1e-5 of its max-abs of the lrelu kink or of the clamp."""
    with torch.no_grad():
        y = ref(x, w, noise_mode=noise_mode)
    u = y / ref.act_gain
    if ref.activation == 'lrelu':
        u = torch.where(u > 0, u, u / 0.2)
    near = u.abs() < 1e-5 * float(u.abs().max())
    if ref.conv_clamp is not None:
        near |= (y.abs() - ref.conv_clamp).abs() < 1e-5 * ref.conv_clamp
    return torch.where(near, torch.zeros_like(P), P.double()).float()


def _param(mod, name):
    for part in name.split('.')[:-1]:
        mod = getattr(mod, part)
    return getattr(mod, name.split('.')[-1])


def _run_layer(lay, x, w, P, noise_mode, dev, params, inputs=()):
    """{name: grad} of `lay(x, w)` with loss sum(y * P), the parameters in `params` (and 'x' / 'ws' in `inputs`) trainable."""
    lay.requires_grad_(False)
    for name in params:
        _param(lay, name).requires_grad_(True)
        _param(lay, name).grad = None
    x = x.to(dev).requires_grad_('x' in inputs)
    w = w.to(dev).requires_grad_('ws' in inputs)
    y = lay(x, w, noise_mode=noise_mode)
    (y * P.to(dev, y.dtype)).sum().backward()
    out = {name: _param(lay, name).grad for name in params}
    if 'x' in inputs:
        out['x'] = x.grad
    if 'ws' in inputs:
        out['ws'] = w.grad
    return y.detach(), out


# (cin, cout, resolution of the output, up, batch, extra) — section 5.10's layer shapes
LAYERS = {
    's1_512_4_b4': (512, 512, 4, 1, 4, {}),
    's1_512_16_b2': (512, 512, 16, 1, 2, {}),
    's1_256_64_b1': (256, 256, 64, 1, 1, {}),
    's1_128_128_b1': (128, 128, 128, 1, 1, {}),
    's1_64_256_b1': (64, 64, 256, 1, 1, {}),
    's1_96_32_b3_linear_clamp': (96, 96, 32, 1, 3, dict(act='linear', clamp=256.0)),
    's1_40_24_odd_channels_b2': (40, 40, 24, 1, 2, {}),
    's1_64_32_noise_none_b2': (64, 64, 32, 1, 2, dict(noise_mode='none')),
    's1_128_32_clamp_b1': (128, 128, 32, 1, 1, dict(clamp=256.0, scale=60.0)),
    'up_512_512_8_b4': (512, 512, 8, 2, 4, {}),
    'up_512_256_128_b1': (512, 256, 128, 2, 1, {}),
    'up_256_128_256_b1': (256, 128, 256, 2, 1, {}),
    'up_32_128_256_b1': (32, 128, 256, 2, 1, {}),
    'up_128_64_512_b1': (128, 64, 512, 2, 1, {}),
    'up_40_24_32_odd_channels_b2': (40, 24, 32, 2, 2, dict(noise_mode='none')),
}
# each parameter alone, on a few of the shapes (the others run all of them together, with x and ws)
ALONE = ('s1_512_16_b2', 's1_40_24_odd_channels_b2', 'up_512_256_128_b1', 'up_40_24_32_odd_channels_b2')


def _setup(case):
    cin, cout, res, up, n, extra = LAYERS[case]
    extra = dict(extra)
    noise_mode, scale = extra.pop('noise_mode', 'const'), extra.pop('scale', 1.0)
    lay = _layer(cin, cout, res, up, seed=sum(map(ord, case)) % 1000, **extra)
    x, w = _inputs(n, cin, res // up, 32, seed=1, scale=scale)
    P = torch.randn(n, cout, res, res, generator=torch.Generator().manual_seed(2))
    ref = _double(lay)
    P = _away_from_kinks(ref, x.double(), w.double(), P, noise_mode)
    return lay, ref, x, w, P, noise_mode


def _check_layer(case, lay, ref, x, w, P, noise_mode, params, inputs):
    _, gr = _run_layer(ref, x.double(), w.double(), P, noise_mode, 'cpu', params, inputs)
    gpu = copy.deepcopy(lay).to(DEV)
    before = _calls()
    _, gg = _run_layer(gpu, x, w, P, noise_mode, DEV, params, inputs)
    after = _calls()
    assert after['modconv_act_backward'] > before['modconv_act_backward'], 'the layer did not take the HIP gradient path'
    if 'weight' in params:
        assert after['modconv_weight_grad'] > before['modconv_weight_grad']
    if 'bias' in params or ('noise_strength' in params and noise_mode == 'const'):
        assert after['bias_noise_grad'] > before['bias_noise_grad']
    errs = {}
    for k, ref_g in gr.items():
        if ref_g is None:           # noise_strength without noise
            assert gg[k] is None or float(gg[k].abs().max()) == 0.0, k
            continue
        errs[k] = _err(gg[k], ref_g)
    print(f'{case} {sorted(params)} {sorted(inputs)}: ' + '  '.join(f'{k} {v:.2e}' for k, v in errs.items()))
    bad = {k: v for k, v in errs.items() if not v < GRAD_TOL}
    assert not bad, bad


@pytest.mark.parametrize('case', sorted(LAYERS))
def test_layer_parameter_gradients_against_float64(case):
    lay, ref, x, w, P, noise_mode = _setup(case)
    _check_layer(case, lay, ref, x, w, P, noise_mode, LAYER_PARAMS, ('x', 'ws'))
    if case in ALONE:
        for name in LAYER_PARAMS:
            if name == 'noise_strength' and noise_mode == 'none':
                continue            # the output does not depend on it: nothing to differentiate
            _check_layer(case, lay, ref, x, w, P, noise_mode, (name,), ())
        _check_layer(case, lay, ref, x, w, P, noise_mode, LAYER_PARAMS, ())


@pytest.mark.parametrize('rows,cin,res,n', [(192, 128, 64, 2), (22, 64, 128, 1), (8, 16, 16, 3)])
def test_dual_head_parameter_gradients_against_float64(rows, cin, res, n):
    from training import networks
    torch.manual_seed(rows + cin)
    co = 3 if rows == 22 else rows // 2
    tr = networks.ToRGBLayer(cin, co, w_dim=32, conv_clamp=256.0)
    ts = networks.ToRGBLayer(cin, rows - co, w_dim=32, conv_clamp=256.0)
    with torch.no_grad():
        for h in (tr, ts):
            h.bias.normal_(0, 0.5); h.affine.bias.normal_(1, 0.3)
    x, w = _inputs(n, cin, res, 32, seed=7)
    P = torch.randn(n, rows, res, res, generator=torch.Generator().manual_seed(8))

    def run(trm, tsm, dev, dtype):
        xx = x.to(dev, dtype).requires_grad_(True); ww = w.to(dev, dtype)
        if dev == 'cpu':
            y = torch.cat([trm(xx, ww), tsm(xx, ww)], dim=1)
        else:
            heads = networks._dual_head(xx, trm, tsm, ww)
            assert heads is not None, 'the heads declined the HIP gradient path'
            y = torch.cat(heads, dim=1)
        (y * P.to(dev, dtype)).sum().backward()
        out = {f'{h}.{k}': p.grad for h, m in (('rgb', trm), ('seg', tsm)) for k, p in m.named_parameters()}
        out['x'] = xx.grad
        return out

    ref = run(_double(tr), _double(ts), 'cpu', torch.float64)
    before = _calls()
    got = run(copy.deepcopy(tr).to(DEV), copy.deepcopy(ts).to(DEV), DEV, torch.float32)
    after = _calls()
    assert after['head_weight_grad'] > before['head_weight_grad'] and after['bias_noise_grad'] > before['bias_noise_grad']
    errs = {k: _err(got[k], ref[k]) for k in ref}
    print(f'heads {rows} x {cin} @{res} b{n}: ' + '  '.join(f'{k} {v:.2e}' for k, v in errs.items()))
    bad = {k: v for k, v in errs.items() if not v < GRAD_TOL}
    assert not bad, bad


# ---- the kernels alone ---------------------------------------------------------------------------------------------------------------

def _wgrad_reference(g, x, s, d, mode):
    """float64 dw of sum(g * d[n,o] * conv(w, s[n,i] x)) (mode 0: 3x3 pad 1 correlation; mode 2: transposed 3x3 stride 2)."""
    xs = x.double() * s.double()[:, :, None, None]
    gd = g.double() * d.double()[:, :, None, None]
    cout, cin = g.shape[1], x.shape[1]
    W = torch.zeros(cout, cin, 3, 3, dtype=torch.float64, requires_grad=True)
    if mode == 0:
        y = torch.nn.functional.conv2d(xs, W, padding=1)
    else:
        y = torch.nn.functional.conv_transpose2d(xs, W.transpose(0, 1), stride=2)
    (y * gd).sum().backward()
    return W.grad


@pytest.mark.parametrize('arith', [6, 1])
@pytest.mark.parametrize('mode,n,cin,cout,h,w', [
    (0, 2, 64, 64, 512, 512),      # several pixel splits per image
    (0, 3, 40, 24, 7, 5),
    (0, 1, 512, 512, 4, 4),
    (2, 1, 128, 64, 128, 128),
    (2, 2, 24, 40, 9, 6),
])
def test_weight_grad_kernel_against_float64(mode, n, cin, cout, h, w, arith):
    from torch_utils import hip_plugin
    g = torch.Generator().manual_seed(cin + cout + h)
    gh, gw = (h, w) if mode == 0 else (2 * h + 1, 2 * w + 1)
    gg = torch.randn(n, cout, gh, gw, generator=g)
    x = torch.randn(n, cin, h, w, generator=g)
    s = torch.randn(n, cin, generator=g) + 1.0
    d = torch.rand(n, cout, generator=g) + 0.5
    ref = _wgrad_reference(gg, x, s, d, mode)
    before = _calls()['modconv_weight_grad']
    got = hip_plugin.ModconvGradPlugin.weight_grad(gg.to(DEV), x.to(DEV), s.to(DEV), d.to(DEV), mode=mode, arith=arith)
    assert _calls()['modconv_weight_grad'] == before + 1
    e = _err(got, ref)
    print(f'weight_grad mode {mode} {cin}->{cout} @{h}x{w} b{n} arith {arith}: {e:.2e}')
    assert e < 1e-5
    # bit-reproducible
    again = hip_plugin.ModconvGradPlugin.weight_grad(gg.to(DEV), x.to(DEV), s.to(DEV), d.to(DEV), mode=mode, arith=arith)
    assert torch.equal(got, again)


@pytest.mark.parametrize('n,c,h,w', [(2, 64, 512, 512), (4, 512, 4, 4), (3, 24, 33, 17), (1, 22, 64, 64)])
def test_bias_noise_kernel_against_float64(n, c, h, w):
    from torch_utils import hip_plugin
    dz = torch.randn(n, c, h, w, generator=torch.Generator().manual_seed(c + h))
    db, dn = hip_plugin.ModconvGradPlugin.bias_noise_grad(dz.to(DEV), noise=True)
    assert _err(db, dz.double().sum(dim=(0, 2, 3))) < 1e-5
    assert _err(dn, dz.double().sum(dim=(0, 1))) < 1e-5
    db2, none = hip_plugin.ModconvGradPlugin.bias_noise_grad(dz.to(DEV))
    assert none is None and torch.equal(db, db2)


def test_backward_is_bit_reproducible():
    for up, res in ((1, 32), (2, 64)):
        lay = _layer(128, 64, res, up, seed=21).to(DEV)
        x, w = _inputs(2, 128, res // up, 32, seed=22)
        P = torch.randn(2, 64, res, res, generator=torch.Generator().manual_seed(23))
        grads = [_run_layer(lay, x, w, P, 'const', DEV, LAYER_PARAMS, ('x',))[1] for _ in range(2)]
        for k in grads[0]:
            assert torch.equal(grads[0][k], grads[1][k]), k


# ---- tuning steps --------------------------------------------------------------------------------------------------------------------

def test_steps_after_in_place_updates_use_the_new_weights():
    """Two Adam steps (a large learning rate, so that every weight moves): after each update the switch-on step must see the new weights
    (the packed-weight workspaces are keyed by tensor version), i.e. match the switch-off path step for step."""
    from training import networks
    torch.manual_seed(31)
    layers0 = torch.nn.ModuleList([_layer(64, 64, 16, 1, seed=32), _layer(64, 32, 32, 2, seed=33)])
    x, w = _inputs(2, 64, 16, 32, seed=34)
    x, w = x.to(DEV), w.to(DEV)
    target = torch.randn(2, 32, 32, 32, generator=torch.Generator().manual_seed(35)).to(DEV)
    runs = {}
    for switch in (True, False):
        networks.hip_param_grad = switch
        layers = copy.deepcopy(layers0).to(DEV).requires_grad_(True)
        for lay in layers:
            lay.noise_const.requires_grad_(False)
        opt = torch.optim.Adam(layers.parameters(), lr=0.05)
        hist = []
        before = _calls()['modconv_weight_grad']
        for _ in range(3):
            opt.zero_grad(set_to_none=True)
            y = layers[1](layers[0](x, w, noise_mode='const'), w, noise_mode='const')
            (y - target).square().mean().backward()
            hist.append((y.detach().clone(), {k: p.grad.clone() for k, p in layers.named_parameters()}))
            opt.step()
        assert (_calls()['modconv_weight_grad'] > before) == switch
        runs[switch] = hist
    networks.hip_param_grad = True
    for step in range(3):
        (y_on, g_on), (y_off, g_off) = runs[True][step], runs[False][step]
        assert _err(y_on, y_off) < GRAD_TOL, f'step {step}: output'
        errs = {k: _err(g_on[k], g_off[k]) for k in g_off}
        bad = {k: v for k, v in errs.items() if not v < GRAD_TOL}
        assert not bad, f'step {step}: {bad}'


def _generator(spec_kwargs, seed=0):
    from training import triplane
    torch.manual_seed(seed)
    spec = triplane.tiny_spec(**spec_kwargs) if spec_kwargs is not None else triplane.GeneratorSpec()
    return triplane.TriPlaneGenerator(spec).eval().requires_grad_(False)


def _pivot(G, n, seed):
    from training import triplane
    g = np.random.RandomState(seed)
    dev = G.mapping.fc0.weight.device
    z = torch.from_numpy(g.randn(n, G.z_dim)).float().to(dev)
    c = torch.cat([triplane.camera_label(float(g.uniform(-0.4, 0.4))) for _ in range(n)]).float().to(dev)
    jit = torch.from_numpy(g.rand(n, G.synthesis.render_size ** 2, G.spec.num_steps)).float().to(dev)
    with torch.no_grad():
        ws = G.mapping(z, c)
    return ws, c, jit


def _trainable(G):
    """The synthesis parameters a PTI coach tunes (all of them), minus the const noise maps (buffers anyway)."""
    for p in G.synthesis.parameters():
        p.requires_grad_(True)
    return {k: p for k, p in G.synthesis.named_parameters()}


def _tuning_step(G, ws, c, jit, target, switch):
    from training import networks
    old = networks.hip_param_grad
    networks.hip_param_grad = switch
    try:
        params = _trainable(G)
        for p in params.values():
            p.grad = None
        with torch.profiler.profile(activities=[torch.profiler.ProfilerActivity.CPU]) as prof:
            img = G.synthesis(ws, c=c, noise_mode='const', force_fp32=True, ray_jitter=jit)
            (img - target).square().mean().backward()
    finally:
        networks.hip_param_grad = old
    names = {e.name for e in prof.events()}
    return {k: p.grad.detach().clone() for k, p in params.items() if p.grad is not None}, names


CONV_OPS = ('aten::convolution', 'aten::_convolution', 'aten::miopen_', 'aten::cudnn_', 'aten::conv')


def _compare_steps(g_on, g_off):
    """Parameters outside the loss's graph on the ATen path (the super-resolution blocks' seg heads, whose output the image loss does not
    read) have no gradient there; the fused dual-head launch gives them an all-zero one."""
    assert set(g_off) <= set(g_on), sorted(set(g_off) - set(g_on))
    for k in set(g_on) - set(g_off):
        assert float(g_on[k].abs().max()) == 0.0, k
    errs = {k: _err(g_on[k], g_off[k]) for k in g_off if float(g_off[k].abs().max()) > 0}
    worst = max(errs, key=errs.get)
    print(f'worst parameter {worst}: {errs[worst]:.2e} over {len(errs)} parameters')
    bad = {k: v for k, v in errs.items() if not v < (SCALAR_STEP_TOL if g_off[k].numel() == 1 else GRAD_TOL)}
    assert not bad, bad


# A noise strength's gradient is one scalar, sum_p dnoise[p] * noise_const[p] over up to 512^2 pixels of random sign: the sum cancels to
# ~1/500 of the sum of its terms' magnitudes, so the ~1e-6 by which two fp32 computations of dz differ grows to ~1e-3 of the result (measured
# 1.7e-3 at 512^2, full spec; the per-layer float64 tests above hold the same gradient to 1.4e-6).  Every tensor gradient keeps GRAD_TOL.
SCALAR_STEP_TOL = 1e-2


def test_tuning_step_tiny_spec_uses_no_aten_convolution():
    G = _generator({}).to(DEV)
    ws, c, jit = _pivot(G, 1, 0)
    with torch.no_grad():
        target = torch.randn_like(G.synthesis(ws, c=c, noise_mode='const', force_fp32=True, ray_jitter=jit))
    before = _calls()
    g_on, names_on = _tuning_step(G, ws, c, jit, target, True)
    after = _calls()
    for k in NEW_CALLS + ('head_weight_grad',):
        assert after[k] > before[k], k
    bad = sorted(n for n in names_on if n.startswith(CONV_OPS))
    assert not bad, bad
    g_off, names_off = _tuning_step(G, ws, c, jit, target, False)
    assert any(n.startswith(CONV_OPS) for n in names_off)
    _compare_steps(g_on, g_off)


def test_tuning_step_full_spec_matches_switch_off():
    G = _generator(None).to(DEV)
    ws, c, jit = _pivot(G, 1, 2)
    with torch.no_grad():
        target = torch.randn_like(G.synthesis(ws, c=c, noise_mode='const', force_fp32=True, ray_jitter=jit))
    g_on, names = _tuning_step(G, ws, c, jit, target, True)
    assert not any(n.startswith(CONV_OPS) for n in names)
    g_off, _ = _tuning_step(G, ws, c, jit, target, False)
    _compare_steps(g_on, g_off)


# Same construction as section 5.10's check of d ws: a central finite difference of the oracle's mixed-precision forward along the unit
# direction of the gradient under test, step 1e-3 in parameter space.
ORACLE_FD_TOL = 1e-2


def test_parameter_gradient_tiny_spec_against_oracle_finite_difference():
    from oracle import generator as ogen, ops as oops
    from training import networks
    G = _generator({})
    sd = {k: v.detach().clone() for k, v in G.state_dict().items()}
    ws, c, jit = _pivot(G, 1, 3)
    sp = G.spec
    P = torch.randn(1, sp.img_channels, sp.img_resolution, sp.img_resolution, generator=torch.Generator().manual_seed(4))
    Gd = copy.deepcopy(G).to(DEV)
    # conv weights, biases, noise strengths, head weights: the parameters this path computes directly
    sel = {}
    for mname, m in Gd.synthesis.named_modules():
        if isinstance(m, (networks.SynthesisLayer, networks.ToRGBLayer)):
            for pname in ('weight', 'bias', 'noise_strength'):
                if getattr(m, pname, None) is not None:
                    sel[f'synthesis.{mname}.{pname}'] = getattr(m, pname)
    for p in sel.values():
        p.requires_grad_(True)
    before = _calls()
    img = Gd.synthesis(ws.to(DEV), c=c.to(DEV), noise_mode='const', ray_jitter=jit.to(DEV))
    (img * P.to(DEV)).sum().backward()
    assert _calls()['modconv_weight_grad'] > before['modconv_weight_grad']
    d = {k: p.grad.detach().cpu().double() for k, p in sel.items()}
    norm = float(torch.sqrt(sum((v * v).sum() for v in d.values())))
    v = {k: g / norm for k, g in d.items()}

    def loss(eps):
        sd2 = dict(sd)
        for k, dv in v.items():
            sd2[k] = (sd[k].double() + eps * dv).to(sd[k].dtype)
        out = ogen.synthesis(sd2, sp, ws.double(), c, jitter=jit, ops=oops)
        return float((out['image'].double() * P.double()).sum())

    eps = 1e-3
    fd = (loss(eps) - loss(-eps)) / (2 * eps)
    e = abs(fd - norm) / norm
    print(f'tiny spec parameter gradient vs oracle finite difference: {e:.2e} (directional derivative {norm:.4e})')
    assert e < ORACLE_FD_TOL


# ---- exclusive residency ---------------------------------------------------------------------------------------------------------------

def _pk_victim_lib():
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'native', '_bin', 'libpk_victim.so')
    if not os.path.isfile(path):
        import sys
        sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
        import __graft_entry__
        path = __graft_entry__.build_test_natives()
    if not os.path.isfile(path):
        pytest.skip('tests/native/pk_victim.hip could not be built here (hipcc output above)')
    lib = ctypes.CDLL(path)
    lib.pk_victim_launch.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p]
    lib.pk_aggressor_launch.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p]
    return lib


def test_foreign_packed_fp32_victim_beside_the_weight_gradient(gpu_device):
    """the weight-gradient kernel's LDS-fed bf16 matrix loop must not share a SIMD with a foreign wave.  The foreign
    packed-fp32 victim of tests/native/pk_victim.hip runs 1500 times beside it per neighbour and must equal its lone result bit for bit."""
    from torch_utils import hip_plugin
    lib = _pk_victim_lib()
    dev = gpu_device
    g = torch.Generator().manual_seed(41)
    rn = lambda *sh: torch.randn(*sh, generator=g).to(dev)
    K, BLOCKS, REPS = 512, 64, 1500
    A = rn(BLOCKS * 32, K); xv = rn(K)
    ref = torch.empty(BLOCKS * 32, device=dev)
    ys = torch.empty(REPS, BLOCKS * 32, device=dev)
    spin = torch.empty(1024 * 256, device=dev)
    sa, sb = torch.cuda.Stream(dev), torch.cuda.Stream(dev)
    torch.cuda.synchronize(dev)

    def victim(out, stream):
        assert lib.pk_victim_launch(A.data_ptr(), xv.data_ptr(), out.data_ptr(), K, BLOCKS, stream.cuda_stream) == 0

    victim(ref, sb)
    torch.cuda.synchronize(dev)

    def changed_launches(neighbour, every=25):
        ys.zero_()
        torch.cuda.synchronize(dev)
        for i in range(REPS):
            if i % every == 0:
                with torch.cuda.stream(sa):
                    neighbour()
            victim(ys[i], sb)
        torch.cuda.synchronize(dev)
        return int((ys != ref[None]).any(dim=1).sum())

    control = changed_launches(lambda: lib.pk_aggressor_launch(spin.data_ptr(), 1500, 1024, sa.cuda_stream), every=40)
    if control == 0:
        pytest.skip('the stand-alone aggressor does not disturb the packed-fp32 victim on this device: nothing to protect against')
    assert changed_launches(lambda: None) == 0, 'the victim must be stable on its own'
    record = {}
    for mode, cin, cout, h in ((0, 128, 128, 128), (2, 256, 128, 64)):
        gh = h if mode == 0 else 2 * h + 1
        gg, x, s, d = rn(2, cout, gh, gh), rn(2, cin, h, h), rn(2, cin) + 1, rn(2, cout).abs() + 0.5
        fn = lambda gg=gg, x=x, s=s, d=d, mode=mode: hip_plugin.ModconvGradPlugin.weight_grad(gg, x, s, d, mode=mode, arith=6)
        fn()
        record[f'weight_grad mode {mode} {cin}->{cout} @{h} [bf16x6]'] = changed_launches(fn)
    print(record, f'positive control {control} of {REPS}')
    assert hip_plugin.exclusive_violations()[0] == 0
    hit = {k: v for k, v in record.items() if v}
    assert not hit, f'foreign packed-fp32 victim disturbed beside: {hit}'
