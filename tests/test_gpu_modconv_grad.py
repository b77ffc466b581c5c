"""Frozen-generator gradients of the synthesis convolutions (training/networks.py `hip_conv_grad`: ide3d_modconv2d + csrc/modconv_bwd.hip)
with respect to the layer inputs, the styles and, through the affines, ws.  `pytest -m gpu`.

Reference: float64 CPU autograd through the layers' own definitions (the differentiable ATen path of the same modules, parameters cast to
float64).  Loss = sum(y * P) with a fixed random projection P.  Errors are the max-abs difference as a fraction of the reference
gradient's max-abs, bounded by GRAD_TOL.
"""

import copy

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

GRAD_TOL = 1e-4
DEV = torch.device('cuda', 0)

NEW_CALLS = ('modconv_act_backward', 'modconv_scale_dot', 'head_weight_grad')


def _calls():
    from torch_utils import hip_plugin
    return {k: hip_plugin.CALLS.get(k, 0) for k in NEW_CALLS + ('modconv2d',)}


def _err(actual, expected):
    a = actual.detach().cpu().double(); e = expected.detach().cpu().double()
    assert a.shape == e.shape, f'shape {tuple(a.shape)} != {tuple(e.shape)}'
    return float((a - e).abs().max()) / (float(e.abs().max()) + 1e-30)


def _frozen(mod):
    for p in mod.parameters():
        p.requires_grad_(False)
    return mod


def _layer(cin, cout, res, up, seed, act='lrelu', clamp=None, noise_strength=0.3, w_dim=32):
    from training import networks
    torch.manual_seed(seed)
    lay = networks.SynthesisLayer(cin, cout, w_dim=w_dim, resolution=res, up=up, activation=act, conv_clamp=clamp)
    with torch.no_grad():
        lay.bias.normal_(0, 0.5)
        lay.noise_strength.fill_(noise_strength)
        lay.affine.bias.normal_(1, 0.3)
    return _frozen(lay)


def _double(mod):
    """A float64 copy of `mod` on the CPU; resample filters stay float32 (what upfirdn2d / conv2d_resample take)."""
    ref = copy.deepcopy(mod).double()
    for m in ref.modules():
        if getattr(m, 'resample_filter', None) is not None:
            m.resample_filter = m.resample_filter.float()
    return ref


def _inputs(n, cin, res_in, w_dim, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, cin, res_in, res_in, generator=g) * scale
    w = torch.randn(n, w_dim, generator=g)
    return x, w


def _run_layer(lay, x, w, P, noise_mode, dev):
    """-> (y, dx, dws) of `lay(x, w)` with loss sum(y * P), on `dev` in the dtype of x."""
    x = x.to(dev).requires_grad_(True)
    w = w.to(dev).requires_grad_(True)
    y = lay(x, w, noise_mode=noise_mode)
    (y * P.to(dev, y.dtype)).sum().backward()
    return y.detach(), x.grad, w.grad


def _away_from_kinks(ref, x, w, P, noise_mode):
    """P with zeros where the float64 pre-activation lies within 1e-5 of its max-abs of the lrelu kink or of the clamp: there an fp32 forward
    may take the other side (its rounding error is ~1e-7 of the max), and act' differs by 5x, which no arithmetic could match."""
    with torch.no_grad():
        y = ref(x, w, noise_mode=noise_mode)
    u = y / ref.act_gain
    if ref.activation == 'lrelu':
        u = torch.where(u > 0, u, u / 0.2)
    tol = 1e-5 * float(u.abs().max())
    near = u.abs() < tol
    if ref.conv_clamp is not None:
        near |= (y.abs() - ref.conv_clamp).abs() < 1e-5 * ref.conv_clamp
    return torch.where(near, torch.zeros_like(P), P.double()).float()


def _run_styles(lay, x, styles, P, noise_mode, dev, hip):
    """-> (y, dx, dstyles) of the layer with the styles as a leaf: `_synthesis_layer_grad` on the GPU (hip), the ATen definition otherwise."""
    from torch_utils.ops import bias_act
    from training import networks
    x = x.to(dev).requires_grad_(True)
    s = styles.to(dev).requires_grad_(True)
    noise = None
    if lay.use_noise and noise_mode == 'const':
        noise = (lay.noise_const * lay.noise_strength).to(x.dtype)
    gain = lay.act_gain
    if hip:
        y = networks._synthesis_layer_grad(lay, x, s, None, noise, gain, lay.conv_clamp)
        assert y is not None, 'the layer declined the gradient path'
    else:
        y = networks.modulated_conv2d(x=x, weight=lay.weight, styles=s, noise=noise, up=lay.up, padding=lay.padding,
                                      resample_filter=(lay.resample_filter if lay.up > 1 else None), flip_weight=(lay.up == 1))
        y = bias_act.bias_act(y, lay.bias.to(x.dtype), act=lay.activation, gain=gain, clamp=lay.conv_clamp)
    (y * P.to(dev, y.dtype)).sum().backward()
    return y.detach(), x.grad, s.grad


# (cin, cout, resolution of the output, up, batch, extra) — the widths and maps of the full spec's layers, batch 1-4
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


@pytest.mark.parametrize('case', sorted(LAYERS))
def test_layer_gradients_against_float64(case):
    from training import networks
    cin, cout, res, up, n, extra = LAYERS[case]
    extra = dict(extra)
    noise_mode, scale = extra.pop('noise_mode', 'const'), extra.pop('scale', 1.0)
    lay = _layer(cin, cout, res, up, seed=sum(map(ord, case)) % 1000, **extra)
    x, w = _inputs(n, cin, res // up, 32, seed=1, scale=scale)
    P = torch.randn(n, cout, res, res, generator=torch.Generator().manual_seed(2))
    ref = _double(lay)
    P = _away_from_kinks(ref, x.double(), w.double(), P, noise_mode)
    yr, dxr, dwr = _run_layer(ref, x.double(), w.double(), P, noise_mode, 'cpu')
    gpu = copy.deepcopy(lay).to(DEV)
    before = _calls()
    y, dx, dw = _run_layer(gpu, x, w, P, noise_mode, DEV)
    after = _calls()
    assert after['modconv_act_backward'] > before['modconv_act_backward'] and after['modconv_scale_dot'] > before['modconv_scale_dot']
    assert _err(y, yr) < GRAD_TOL
    e_dx, e_dw = _err(dx, dxr), _err(dw, dwr)
    assert e_dx < GRAD_TOL, f'dx {e_dx:.2e}'
    assert e_dw < GRAD_TOL, f'dws {e_dw:.2e}'
    # d styles with the styles as the leaf
    with torch.no_grad():
        styles = lay.affine(w)
    _, dxr2, dsr = _run_styles(ref, x.double(), styles.double(), P, noise_mode, 'cpu', hip=False)
    _, dx2, ds = _run_styles(gpu, x, styles, P, noise_mode, DEV, hip=True)
    e_dx2, e_ds = _err(dx2, dxr2), _err(ds, dsr)
    assert e_dx2 < GRAD_TOL and e_ds < GRAD_TOL, f'dx {e_dx2:.2e} dstyles {e_ds:.2e}'
    print(f'{case}: dx {e_dx:.2e}  dws {e_dw:.2e}  dstyles {e_ds:.2e}')
    assert networks.hip_conv_grad


def _inference_launches(lay, x, styles, dcoefs, noise):
    """What SynthesisLayer.forward launches without grad for these styles and dcoefs."""
    from torch_utils.ops import bias_act
    from training import networks
    spec = bias_act.activation_funcs[lay.activation]
    networks._modconv_init()
    with torch.no_grad():
        if lay.up == 1:
            return networks._modconv_bias_act(x, lay.weight, styles, True, noise, 1.0, lay.bias, lay.activation, lay.act_gain, lay.conv_clamp,
                                              dcoefs=dcoefs)
        yt = networks._modconv_plugin.modconv2d(x.contiguous(), lay.weight.contiguous(), styles.contiguous(), dcoefs, None, 0.0, None, 1, 0.0,
                                                1.0, -1.0, mode=2, pad_rows=True)
        return networks._upfirdn_plugin().upfirdn2d_ex(yt, lay.resample_filter, 1, 1, 1, 1, 1, 1, 1, 1, False, 4.0, noise=noise, noise_strength=1.0,
                                                       bias=lay.bias, act=spec.cuda_idx, alpha=spec.def_alpha, act_gain=lay.act_gain,
                                                       clamp=-1.0 if lay.conv_clamp is None else lay.conv_clamp)


@pytest.mark.parametrize('case', ['s1_128_32_b2', 'up_128_64_64_b3', 's1_40_24_linear_b1'])
def test_forward_is_the_inference_launch_and_backward_is_deterministic(case):
    """Under grad the output is bit-identical to the no-grad launch for the same styles and dcoefs; two backward passes are bit-identical."""
    from training import networks
    cfg = {'s1_128_32_b2': (128, 128, 32, 1, 2, 'lrelu'), 'up_128_64_64_b3': (128, 64, 64, 2, 3, 'lrelu'),
           's1_40_24_linear_b1': (40, 40, 24, 1, 1, 'linear')}[case]
    cin, cout, res, up, n, act = cfg
    lay = _layer(cin, cout, res, up, seed=5, act=act).to(DEV)
    x, w = _inputs(n, cin, res // up, 32, seed=6)
    x, w = x.to(DEV), w.to(DEV)
    noise = (lay.noise_const * lay.noise_strength).detach()
    grads = []
    for _ in range(2):
        xg, wg = x.clone().requires_grad_(True), w.clone().requires_grad_(True)
        styles = lay.affine(wg)
        dcoefs = networks._demod_coefs(lay.weight, styles)
        y = networks._synthesis_layer_grad(lay, xg, styles, dcoefs, noise, lay.act_gain, lay.conv_clamp)
        assert y is not None and 'Modconv' in type(y.grad_fn).__name__, type(y.grad_fn).__name__
        y0 = _inference_launches(lay, x, styles.detach(), dcoefs.detach(), noise)
        assert torch.equal(y.detach(), y0)
        (y * torch.cos(y.detach())).sum().backward()
        grads.append((xg.grad.clone(), wg.grad.clone()))
    assert torch.equal(grads[0][0], grads[1][0]) and torch.equal(grads[0][1], grads[1][1])


@pytest.mark.parametrize('act,clamp', [('lrelu', -1.0), ('lrelu', 4.0), ('linear', 1.5)])
def test_dz_is_bit_equal_to_bias_act_grad(act, clamp):
    from torch_utils import hip_plugin
    from torch_utils.ops import bias_act
    spec = bias_act.activation_funcs[act]
    g = torch.Generator().manual_seed(3)
    y = (torch.randn(2, 24, 16, 16, generator=g) * 3).to(DEV)
    dy = torch.randn(2, 24, 16, 16, generator=g).to(DEV)
    gain = spec.def_gain
    dz, _ = hip_plugin.ModconvGradPlugin.act_backward(dy, y, spec.cuda_idx, spec.def_alpha, gain, clamp)
    empty = torch.empty([0], device=DEV)
    ref = hip_plugin.BiasActPlugin.bias_act(dy, empty, empty, y, empty, 1, 1, spec.cuda_idx, spec.def_alpha, gain, clamp)
    assert torch.equal(dz, ref)


@pytest.mark.parametrize('rows,cin,res,n', [(192, 128, 64, 2), (22, 64, 128, 1), (22, 128, 32, 4), (8, 16, 16, 3)])
def test_dual_head_gradients_against_float64(rows, cin, res, n):
    from training import networks
    torch.manual_seed(rows + cin)
    co = 3 if rows == 22 else rows // 2
    tr = _frozen(networks.ToRGBLayer(cin, co, w_dim=32, conv_clamp=256.0))
    ts = _frozen(networks.ToRGBLayer(cin, rows - co, w_dim=32, conv_clamp=256.0))
    with torch.no_grad():
        for h in (tr, ts):
            h.bias.normal_(0, 0.5); h.affine.bias.normal_(1, 0.3)
    x, w = _inputs(n, cin, res, 32, seed=7)
    P = torch.randn(n, rows, res, res, generator=torch.Generator().manual_seed(8))

    def run(trm, tsm, dev, dtype):
        xx = x.to(dev, dtype).requires_grad_(True); ww = w.to(dev, dtype).requires_grad_(True)
        if dev == 'cpu':
            y = torch.cat([trm(xx, ww), tsm(xx, ww)], dim=1)
        else:
            heads = networks._dual_head(xx, trm, tsm, ww)
            assert heads is not None
            y = torch.cat(heads, dim=1)
        (y * P.to(dev, dtype)).sum().backward()
        return y.detach(), xx.grad, ww.grad

    yr, dxr, dwr = run(_double(tr), _double(ts), 'cpu', torch.float64)
    before = _calls()['head_weight_grad']
    y, dx, dw = run(copy.deepcopy(tr).to(DEV), copy.deepcopy(ts).to(DEV), DEV, torch.float32)
    assert _calls()['head_weight_grad'] > before
    assert _err(y, yr) < GRAD_TOL
    e_dx, e_dw = _err(dx, dxr), _err(dw, dwr)
    assert e_dx < GRAD_TOL and e_dw < GRAD_TOL, f'dx {e_dx:.2e} dws {e_dw:.2e}'


def test_head_weight_grad_kernel_against_float64():
    from torch_utils import hip_plugin
    g = torch.Generator().manual_seed(9)
    for n, rows, cin, hw in ((2, 192, 96, (33, 17)), (1, 22, 130, (64, 64)), (3, 5, 7, (3, 5))):
        dy = torch.randn(n, rows, *hw, generator=g); x = torch.randn(n, cin, *hw, generator=g)
        ref = torch.einsum('nop,nip->noi', dy.double().flatten(2), x.double().flatten(2))
        out = hip_plugin.ModconvGradPlugin.head_weight_grad(dy.to(DEV), x.to(DEV))
        assert _err(out, ref) < 1e-5


# ---- the projector step --------------------------------------------------------------------------------------------------------------

def _generator(spec_kwargs, seed=0):
    from training import triplane
    torch.manual_seed(seed)
    spec = triplane.tiny_spec(**spec_kwargs) if spec_kwargs is not None else triplane.GeneratorSpec()
    G = _frozen(triplane.TriPlaneGenerator(spec).eval())
    return G


def _projector_step(G, ws0, c, jit, target, switch):
    """d ws of one projector step (L2 loss against `target`) with `networks.hip_conv_grad = switch`, and the op names of its backward.
    The ray jitter is the fixed tensor `jit`: without it the renderer draws new depths on every call."""
    from training import networks
    old = networks.hip_conv_grad
    networks.hip_conv_grad = switch
    try:
        ws = ws0.clone().requires_grad_(True)
        img = G.synthesis(ws, c=c, noise_mode='const', ray_jitter=jit)
        loss = (img - target).square().mean()
        with torch.profiler.profile(activities=[torch.profiler.ProfilerActivity.CPU]) as prof:
            loss.backward()
    finally:
        networks.hip_conv_grad = old
    names = {e.name for e in prof.events()}
    return ws.grad, names


def _ws_camera_jitter(G, n, seed):
    from training import triplane
    g = np.random.RandomState(seed)
    dev = G.mapping.fc0.weight.device
    z = torch.from_numpy(g.randn(n, G.z_dim)).float().to(dev)
    c = torch.cat([triplane.camera_label(float(g.uniform(-0.4, 0.4))) for _ in range(n)]).float().to(dev)
    jit = torch.from_numpy(g.rand(n, G.synthesis.render_size ** 2, G.spec.num_steps)).float().to(dev)
    with torch.no_grad():
        ws = G.mapping(z, c)
    return ws, c, jit


# Whole projector steps, switch on against switch off, same ray jitter: two fp32 computations of the same gradient (split-bf16 MFMA
# convolutions and the new kernels against MIOpen).  Measured 1.0e-6 (tiny spec, batch 2) and 6.6e-6 .. 6.9e-6 (full spec, batch 1).
TINY_STEP_TOL = 1e-4
FULL_STEP_TOL = 1e-4


def test_projector_step_tiny_spec_uses_no_aten_convolution():
    G = _generator({}).to(DEV)
    ws, c, jit = _ws_camera_jitter(G, 2, 0)
    with torch.no_grad():
        target = torch.randn_like(G.synthesis(ws, c=c, noise_mode='const', ray_jitter=jit))
    before = _calls()
    d_on, names_on = _projector_step(G, ws, c, jit, target, True)
    after = _calls()
    for k in NEW_CALLS:
        assert after[k] > before[k], k
    bad = sorted(n for n in names_on if n.startswith(('aten::convolution', 'aten::miopen_', 'aten::cudnn_', 'aten::_convolution')))
    assert not bad, bad
    d_off, names_off = _projector_step(G, ws, c, jit, target, False)
    assert any(n.startswith(('aten::convolution', 'aten::_convolution', 'aten::miopen_')) for n in names_off)
    e = _err(d_on, d_off)
    print(f'tiny projector d ws: on vs off {e:.2e}')
    assert e < TINY_STEP_TOL


# The oracle (oracle/generator.py) computes its convolutions in fp32 (`weight.float()`, F.conv2d) around float64 element-wise ops, so
# its gradient can only be probed by a finite difference of that mixed-precision forward: along the unit direction of the gradient
# under test, central, step 1e-3 in ws.  Its own noise (fp32 rounding over the step, lrelu kinks crossed by it) was measured at
# 2.2e-3 of the directional derivative with CPU autograd through the ATen definition; a wrong scale or a wrong sign in any layer's
# gradient moves it by far more.
ORACLE_FD_TOL = 1e-2


def test_projector_gradient_tiny_spec_against_oracle_finite_difference():
    from oracle import generator as ogen, ops as oops
    G = _generator({})
    sd = {k: v.detach().clone() for k, v in G.state_dict().items()}
    ws, c, jit = _ws_camera_jitter(G, 1, 3)
    sp = G.spec
    P = torch.randn(1, sp.img_channels, sp.img_resolution, sp.img_resolution, generator=torch.Generator().manual_seed(4))
    Gd = copy.deepcopy(G).to(DEV)
    wsg = ws.to(DEV).requires_grad_(True)
    before = _calls()
    img = Gd.synthesis(wsg, c=c.to(DEV), noise_mode='const', ray_jitter=jit.to(DEV))
    (img * P.to(DEV)).sum().backward()
    assert _calls()['modconv_act_backward'] > before['modconv_act_backward']
    d = wsg.grad.detach().cpu().double()

    def loss(w):
        out = ogen.synthesis(sd, sp, w, c, jitter=jit, ops=oops)
        return float((out['image'].double() * P.double()).sum())

    v = d / d.norm()
    eps = 1e-3
    fd = (loss(ws.double() + eps * v) - loss(ws.double() - eps * v)) / (2 * eps)
    e = abs(fd - float(d.norm())) / float(d.norm())
    print(f'tiny projector d ws vs oracle finite difference: {e:.2e}')
    assert e < ORACLE_FD_TOL


def test_backbone_gradients_tiny_spec_against_cpu():
    """d ws of the tri-plane backbone (3x3, up-sampling and head layers of every voxel block, dcoefs under grad, the const-input block)
    against CPU autograd through the ATen definition of the same module.  The blocks compute in float32 by construction (float64 cannot
    be pushed through them), so this reference is float32; the per-layer tests above hold the float64 comparison."""
    G = _generator({})
    syn = G.synthesis
    ws, _, _ = _ws_camera_jitter(G, 2, 1)
    g = torch.Generator()

    def run(s, wsx, dev):
        wsx = wsx.detach().clone().to(dev).requires_grad_(True)
        vws, _ = s.split_ws(wsx)
        img_v, seg_v = s.backbone(vws, noise_mode='const')
        Pi = torch.randn(img_v.shape, generator=g.manual_seed(5)).to(dev, img_v.dtype)
        Ps = torch.randn(seg_v.shape, generator=g.manual_seed(6)).to(dev, seg_v.dtype)
        ((img_v * Pi).sum() + (seg_v * Ps).sum()).backward()
        return wsx.grad

    ref = run(copy.deepcopy(syn), ws, 'cpu')
    before = _calls()
    got = run(copy.deepcopy(syn).to(DEV), ws, DEV)
    after = _calls()
    assert after['modconv_act_backward'] > before['modconv_act_backward'] and after['head_weight_grad'] > before['head_weight_grad']
    e = _err(got, ref)
    print(f'tiny backbone d ws vs CPU: {e:.2e}')
    assert e < GRAD_TOL


def test_projector_step_full_spec_matches_switch_off():
    G = _generator(None).to(DEV)
    ws, c, jit = _ws_camera_jitter(G, 1, 2)
    with torch.no_grad():
        target = torch.randn_like(G.synthesis(ws, c=c, noise_mode='const', ray_jitter=jit))
    d_on, names = _projector_step(G, ws, c, jit, target, True)
    assert not any(n.startswith(('aten::convolution', 'aten::miopen_', 'aten::cudnn_')) for n in names)
    d_off, _ = _projector_step(G, ws, c, jit, target, False)
    e = _err(d_on, d_off)
    print(f'full-spec projector d ws: on vs off {e:.2e}')
    assert e < FULL_STEP_TOL


# ---- routing -------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('param', ['weight', 'bias', 'affine.weight', 'noise_strength'])
def test_trainable_parameter_declines_and_keeps_its_gradient(param):
    from training import networks
    lay = _layer(64, 64, 16, 1, seed=12).to(DEV)
    x, w = _inputs(2, 64, 16, 32, seed=13)
    x, w = x.to(DEV), w.to(DEV)
    mod, name = (lay.affine, 'weight') if param == 'affine.weight' else (lay, param)
    getattr(mod, name).requires_grad_(True)
    results = []
    for switch in (True, False):
        networks.hip_conv_grad = switch
        try:
            getattr(mod, name).grad = None
            before = _calls()['modconv_act_backward']
            y = lay(x, w.clone().requires_grad_(True), noise_mode='const')
            y.square().sum().backward()
            assert _calls()['modconv_act_backward'] == before
            results.append(getattr(mod, name).grad.clone())
        finally:
            networks.hip_conv_grad = True
    assert torch.equal(results[0], results[1])


def test_random_noise_and_switch_off_never_reach_the_new_entry_points():
    from training import networks
    lay = _layer(64, 64, 16, 1, seed=14).to(DEV)
    up = _layer(64, 32, 32, 2, seed=15).to(DEV)
    x, w = _inputs(2, 64, 16, 32, seed=16)
    x, w = x.to(DEV).requires_grad_(True), w.to(DEV).requires_grad_(True)
    before = _calls()
    (lay(x, w, noise_mode='random').sum() + up(x, w, noise_mode='random').sum()).backward()
    networks.hip_conv_grad = False
    try:
        (lay(x, w, noise_mode='const').sum() + up(x, w, noise_mode='const').sum()).backward()
    finally:
        networks.hip_conv_grad = True
    after = _calls()
    for k in NEW_CALLS:
        assert after[k] == before[k], k
