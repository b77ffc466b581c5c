"""The plain-convolution regime of `ide3d_modconv2d` - styles == NULL, dcoefs == NULL, bias + ReLU / bias / nothing - that the loss networks
(training/lpips.py, training/parse_loss.py, training/id_loss.py) run about 150 times per projector step, launch by launch against float64
(DESIGN.md section 5.18):

 * every stand-in of tests/loss_conv_launches.py (one per plan class of the workload set + the edge launches) in the default arithmetic and
   in fp32: `max |y - ref| <= TOL max |pre-activation ref|` with TOL of tests/test_gpu_conv_arith.py, exact zeros behind the ReLU, two runs
   and a run on NaN-filled free blocks bit-equal;
 * the wrappers `parse_loss._conv` / `_conv_grad` (shared by `id_loss`) and LPIPS's backward convolution per layer kind against a float64
   copy of the module and its autograd vjp;
 * the adjoint identity <A x, dy> == <x, A^T dy> between a forward launch and its gradient launch;
 * the streaming passes of csrc/parse_loss.hip / csrc/lpips.hip on more than 65535 planes and on more than 256 CUs x 8 x 256 pixels,
   where their grids wrap.

Measured on an MI355X (all 260 cases pass, the file takes 5 s; no launch needed the wider 4 x ATen bound): worst max error of a stand-in as
a fraction of TOL max |pre-activation|: 0.424 in the default arithmetic (bf16x6; 9 x 256 -> 512 @ 17 x 20, 3x3, no epilogue: the 16 x 16
tile without split-K) and 0.224 in fp32 (9 x 64 -> 64 @ 114 x 228); every other launch is below 0.30.  The wrappers: 0.251 forward, 0.141
gradient; LPIPS's backward convolution 0.054; the adjoint identity's two sides differ by at most 1.0e-3 of their bound."""

import math

import pytest
import torch
import torch.nn.functional as F

import loss_conv_launches as L
from test_gpu_conv_arith import TOL                      # the project's bound of the fp32 and bf16x6 arithmetics: 4e-6 of max |ref|
from test_gpu_parse_loss import _aten_vjp, _dirty, _within

pytestmark = pytest.mark.gpu

ARITHS = {'default': 0, 'fp32': 1}


def _mc():
    from torch_utils import hip_plugin
    hip_plugin.load()
    return hip_plugin.ModconvPlugin.modconv2d


def _tol(arith):
    from torch_utils import hip_plugin
    return TOL['fp32'] if arith == 1 else TOL[hip_plugin.conv_arithmetic()]


def _id(launch):
    n, cin, cout, h, w, k, mode, epi = launch
    return f'{n}x{cin}to{cout}@{h}x{w}k{k}m{mode}{epi}'


def _operands(launch, dev, seed=11, zero_border=False):
    """x: ReLU-ed noise (about half zeros, like real activations); w: randn / sqrt(cin k k); bias: 0.5 randn, against pre-activations of
    standard deviation sqrt(1 / 2), so that the ReLU cuts about half of the outputs."""
    n, cin, cout, h, w, k, mode, epi = launch
    g = torch.Generator().manual_seed(seed + 7919 * cin + 31 * cout + h)
    x = torch.randn(n, cin, h, w, generator=g).clamp_min(0)
    if zero_border:
        x[:, :, 0], x[:, :, -1], x[:, :, :, 0], x[:, :, :, -1] = 0, 0, 0, 0
    wt = torch.randn(cout, cin, k, k, generator=g) / math.sqrt(cin * k * k)
    bias = None if epi == 'grad' else 0.5 * torch.randn(cout, generator=g)
    return x.to(dev), wt.to(dev), (None if bias is None else bias.to(dev))


def _ref64(x, wt, bias, mode):
    """The pre-activation in float64 on the fp32 operands (ATen on the GPU, as tests/test_gpu_conv_arith.py runs it)."""
    x, wt = x.double(), wt.double()
    b = None if bias is None else bias.double()
    if mode == 0:
        return F.conv2d(x, wt, b, padding=wt.shape[2] // 2)
    if mode == 1:
        return F.conv2d(x, wt, b, stride=2)
    return F.conv_transpose2d(x, wt.transpose(0, 1), b, stride=2)


def _launch(x, wt, bias, launch, arith):
    return _mc()(x, wt, None, None, None, 0.0, bias, 3 if launch[7] == 'relu' else 1, 0.0, 1.0, -1.0, mode=launch[6], arith=arith)


# ---- 3a: every stand-in against float64 ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('arith', list(ARITHS), ids=list(ARITHS))
@pytest.mark.parametrize('launch', [l for l, _ in L.STAND_INS], ids=_id)
def test_stand_in_against_float64(gpu_device, launch, arith):
    """One launch of the table against the float64 convolution + bias + ReLU of the same fp32 operands."""
    code = ARITHS[arith]
    x, wt, bias = _operands(launch, gpu_device, zero_border=launch in L.ZERO_BORDER)
    pre = _ref64(x, wt, bias, launch[6])
    ref = pre.clamp_min(0) if launch[7] == 'relu' else pre
    y = _launch(x, wt, bias, launch, code)
    assert tuple(y.shape) == (launch[0], launch[2]) + L.out_size(launch)
    scale, tol = float(pre.abs().max()), _tol(code)
    err = (y.double() - ref).abs()
    ratio = float(err.max()) / (tol * scale)
    print(f'{_id(launch)} [{arith}]: max err {float(err.max()):.3e} = {ratio:.3f} x TOL max |pre-activation| ({scale:.3e})')
    if launch[7] == 'relu':
        cut = float((pre < 0).double().mean())
        assert cut >= 1 / 3, f'the ReLU cuts only {cut:.2f} of the outputs'
        assert bool((y[pre < -tol * scale] == 0).all()), 'a ReLU output whose float64 pre-activation is clearly negative must be exactly 0'
    if ratio > 1:           # where it sits: a row, a column, a channel block or a K tail is a bug, a uniform spread is rounding
        e = err / (tol * scale)
        print('worst per output channel', e.amax(dim=(0, 2, 3)).topk(min(4, e.shape[1])), 'per row', e.amax(dim=(0, 1, 3)).topk(min(4, e.shape[2])),
              'per column', e.amax(dim=(0, 1, 2)).topk(min(4, e.shape[3])), 'per image', e.amax(dim=(1, 2, 3)))
    assert ratio <= 1
    assert torch.equal(_launch(x, wt, bias, launch, code), y), 'two runs differ'
    _dirty(gpu_device)
    assert torch.equal(_launch(x, wt, bias, launch, code), y), 'the launch read memory it had not written'


# ---- 3c: the adjoint identity ---------------------------------------------------------------------------------------------------------------------
def _adjoint_of(launch):
    """(the launch of A^T, its weights from A's) of a forward launch A, as `networks._grad_weight` derives them: mode 0 on the transposed,
    flipped weights; mode 2 on the transposed weights for the stride-2 convolution (on an input of (2 ho + 1) x (2 wo + 1) pixels, so that
    the transposed convolution's output is exactly the input's gradient), and mode 1 for a transposed convolution."""
    from training import networks
    n, cin, cout, h, w, k, mode, epi = launch
    oh, ow = L.out_size(launch)
    if mode == 0:
        return (n, cout, cin, h, w, k, 0, 'grad'), lambda wt: networks._grad_weight(wt, True)
    return (n, cout, cin, oh, ow, k, 2 if mode == 1 else 1, 'grad'), lambda wt: networks._grad_weight(wt, False)


ADJOINT_CASES = [(2, 147, 64, 9, 15, 1, 0, 'grad'), (1, 128, 128, 6, 7, 1, 0, 'grad'), (2, 3, 64, 13, 18, 3, 0, 'grad'), (1, 64, 128, 12, 12, 3, 0, 'grad'),
                 (2, 32, 128, 13, 17, 3, 1, 'grad'), (1, 512, 512, 15, 15, 3, 1, 'grad'), (1, 128, 64, 9, 18, 3, 2, 'grad'), (1, 512, 256, 2, 3, 3, 2, 'grad')]


@pytest.mark.parametrize('arith', list(ARITHS), ids=list(ARITHS))
@pytest.mark.parametrize('launch', ADJOINT_CASES, ids=_id)
def test_adjoint_identity(gpu_device, launch, arith):
    """<A x, dy> == <x, A^T dy>, both sides in float64 from the kernels' fp32 outputs.  Each launch is within TOL max |its output| of the
    exact map per element, so the two sides differ by at most TOL (max |A x| sum |dy| + max |A^T dy| sum |x|)."""
    code = ARITHS[arith]
    x, wt, _ = _operands(launch, gpu_device, seed=23)
    back, derive = _adjoint_of(launch)
    assert back[3:5] == L.out_size(launch) and L.out_size(back) == launch[3:5], 'mode 1 / 2 pairs need an odd-sided stride-2 input'
    g = torch.Generator().manual_seed(29)
    dy = torch.randn(launch[0], launch[2], *L.out_size(launch), generator=g).to(gpu_device)
    ax = _launch(x, wt, None, launch, code)
    aty = _launch(dy, derive(wt), None, back, code)
    lhs, rhs = float((ax.double() * dy.double()).sum()), float((x.double() * aty.double()).sum())
    tol = _tol(code)
    bound = tol * (float(ax.abs().max()) * float(dy.abs().double().sum()) + float(aty.abs().max()) * float(x.abs().double().sum()))
    print(f'{_id(launch)} [{arith}]: <Ax, dy> {lhs:.9e}, <x, A^T dy> {rhs:.9e}, difference {abs(lhs - rhs):.3e} = {abs(lhs - rhs) / bound:.2e} x bound')
    assert abs(lhs - rhs) <= bound
    # the reference satisfies it by construction; the forward launch against it, so that a pair that is wrong the same way does not pass
    ref = _ref64(x, wt, None, launch[6])
    assert float((ax.double() - ref).abs().max()) <= tol * float(ref.abs().max())


# ---- 3b: the wrappers at layer level ----------------------------------------------------------------------------------------------------------------
# (k, stride, padding, BatchNorm, relu) of BiSeNet (training/face_parsing.py) and of the IR-SE backbone (training/id_loss.py) -> (cin, cout), maps
LAYER_KINDS = {
    'parse': [((7, 2, 3, True, True), (3, 64), [(64, 64), (32, 96)]),                      # the stem: unfolded patches, K = 147
              ((3, 1, 1, True, True), (64, 64), [(2, 2), (5, 7)]),
              ((3, 1, 1, True, False), (128, 128), [(2, 2), (5, 7)]),
              ((3, 2, 1, True, True), (64, 128), [(4, 4), (6, 10)]),
              ((1, 2, 0, True, False), (64, 128), [(4, 4), (6, 10)]),
              ((1, 1, 0, True, True), (512, 128), [(1, 1)]),                                # conv_avg on the global mean
              ((1, 1, 0, True, True), (384, 256), [(8, 8), (5, 7)]),                        # the fusion block
              ((1, 1, 0, True, False), (128, 128), [(1, 1)]),                               # an attention gate
              ((1, 1, 0, False, True), (256, 64), [(1, 1)]),
              ((1, 1, 0, False, False), (64, 256), [(1, 1)]),
              ((1, 1, 0, False, False), (256, 19), [(8, 8), (5, 7)])],                      # the logits
    'id': [((3, 1, 1, True, False), (3, 64), [(7, 7), (12, 13)]),                           # the input layer
           ((3, 1, 1, False, False), (64, 128), [(7, 7), (14, 14)]),
           ((3, 1, 1, True, False), (256, 256), [(7, 7)]),
           ((3, 2, 1, True, False), (128, 128), [(14, 14), (7, 9)]),                        # 14 -> 7; an odd map: the crop keeps rows 1 .. h of h + 2
           ((1, 2, 0, True, False), (256, 512), [(14, 14), (6, 10)])],
}
LAYER_CASES = [(net, kind, ch, size) for net, kinds in LAYER_KINDS.items() for kind, ch, sizes in kinds for size in sizes]


def _layer(kind, ch, dev, seed):
    k, s, p, with_bn, relu = kind
    g = torch.Generator().manual_seed(seed)
    conv = torch.nn.Conv2d(ch[0], ch[1], k, s, p, bias=False)
    conv.weight.data = torch.randn(ch[1], ch[0], k, k, generator=g) / math.sqrt(ch[0] * k * k)
    bn = None
    if with_bn:
        bn = torch.nn.BatchNorm2d(ch[1])
        bn.weight.data, bn.bias.data = torch.rand(ch[1], generator=g) + 0.5, 0.5 * torch.randn(ch[1], generator=g)
        bn.running_mean.data, bn.running_var.data = 0.2 * torch.randn(ch[1], generator=g), torch.rand(ch[1], generator=g) + 0.5
    mods = [m.eval().requires_grad_(False) for m in ((conv, bn) if bn is not None else (conv,))]
    import copy
    m64 = [copy.deepcopy(m).double().to(dev) for m in mods]
    mods = [m.to(dev) for m in mods]
    return mods[0], (mods[1] if with_bn else None), (lambda t: m64[1](m64[0](t)) if with_bn else m64[0](t))


@pytest.mark.parametrize('net,kind,ch,size', LAYER_CASES, ids=[f'{n}-k{k[0]}s{k[1]}{"bn" if k[3] else ""}{"relu" if k[4] else ""}-{c[0]}to{c[1]}@{s[0]}x{s[1]}'
                                                                for n, k, c, s in LAYER_CASES])
def test_wrapper_layer_against_float64(gpu_device, net, kind, ch, size):
    """`_conv` against relu(bn(conv(x.double()))) of a float64 copy of the module, `_conv_grad` (the stem: `stem_backward`, as the fused
    pass computes it) against the float64 autograd vjp: the unfolded stem, the explicit padding and the crop of the stride-2 3x3, the
    decimation of the stride-2 1x1 and its half-resolution gradient after the join has scattered it to the even positions."""
    from training import id_loss, networks, parse_loss
    assert networks._modconv_init() and networks._modconv_grad_init()
    ops = (parse_loss if net == 'parse' else id_loss)._HipOps.get()
    P = parse_loss._HipOps.get().P
    k, s, p, with_bn, relu = kind
    conv, bn, f64 = _layer(kind, ch, gpu_device, seed=41 + k + 3 * s + ch[0])
    g = torch.Generator().manual_seed(43)
    x = torch.randn(2, ch[0], *size, generator=g).clamp_min(0).to(gpu_device)
    pre = f64(x.double())
    ref = pre.clamp_min(0) if relu else pre
    tol = _tol(0)
    y = parse_loss._conv(ops, x, conv, bn, relu)
    assert y.shape == ref.shape
    e = float((y.double() - ref).abs().max())
    print(f'forward: max err {e:.3e} = {e / (tol * float(pre.abs().max())):.3f} x TOL max |pre-activation|')
    assert e <= tol * float(pre.abs().max())
    dz = torch.randn(*pre.shape, generator=g).to(gpu_device)
    want = _aten_vjp(f64, torch.zeros_like(x).double(), dz.double())
    if k == 7:
        from training import face_parsing
        got = P.stem_backward(dz, face_parsing._folded(conv, bn)[0], size)
    else:
        got = parse_loss._conv_grad(ops, dz, conv, bn, size=size)
        if (k, s) == (1, 2):
            assert tuple(got.shape[2:]) == ((size[0] + 1) // 2, (size[1] + 1) // 2)
            got = P.join([torch.zeros_like(x), (got.contiguous(), True)])
    assert got.shape == want.shape
    e = float((got.double() - want).abs().max())
    print(f'gradient: max err {e:.3e} = {e / (tol * float(want.abs().max())):.3f} x TOL max |gradient|')
    assert e <= tol * float(want.abs().max())


@pytest.mark.parametrize('shape', [(2, 64, 3, 13, 18), (1, 128, 64, 5, 7), (1, 512, 512, 2, 2)], ids=lambda s: 'x'.join(map(str, s)))
def test_lpips_backward_convolution_against_float64(gpu_device, shape):
    """training/lpips.py's input gradient of a 3x3 layer: a forward launch on `_grad_weight(weight, True)` against the float64 vjp."""
    from training import networks
    assert networks._modconv_init()
    n, cout, cin, h, w = shape
    g = torch.Generator().manual_seed(47)
    weight = (torch.randn(cout, cin, 3, 3, generator=g) / math.sqrt(cin * 9)).to(gpu_device)
    dz = torch.randn(n, cout, h, w, generator=g).clamp_min(0).to(gpu_device)
    got = _mc()(dz, networks._grad_weight(weight, True), None, None, None, 0.0, None, 1, 0.0, 1.0, -1.0)
    want = _aten_vjp(lambda t: F.conv2d(t, weight.double(), padding=1), torch.zeros(n, cin, h, w, dtype=torch.float64, device=gpu_device), dz.double())
    e = float((got.double() - want).abs().max())
    print(f'max err {e:.3e} = {e / (_tol(0) * float(want.abs().max())):.3f} x TOL max |gradient|')
    assert e <= _tol(0) * float(want.abs().max())


# ---- 3d: the streaming passes where their grids wrap -------------------------------------------------------------------------------------------------
def _rand(shape, seed, dev):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)).to(dev)


# more planes than gridDim.y may hold (65535: `pl_grid`), and more pixels in a plane than 256 CUs x 8 workgroups x 256 threads (`stream_grid`)
WRAP = {'planes': (1, 65539, 2, 2), 'pixels': (1, 1, 725, 725)}


# the join's 16-byte form takes 4 pixels per thread: 1452 x 1452 / 4 is more than its grid holds
JOIN_WRAP = dict(WRAP, pixels_by_four=(1, 1, 1452, 1452))


@pytest.mark.parametrize('what', list(JOIN_WRAP))
def test_join_and_plane_sums_where_the_grid_wraps(gpu_device, what):
    from torch_utils import hip_plugin
    P = hip_plugin.ParseLossPlugin
    shape = JOIN_WRAP[what]
    a, b, dy = (_rand(shape, s, gpu_device) for s in (51, 52, 53))
    D = lambda t: t.double()
    y = P.join([a, b], post=1)
    assert _within(y, F.relu(D(a) + D(b)), F.relu(a + b), 'relu(a + b)')
    assert torch.equal(y, F.relu(a + b)), 'one fp32 addition and a maximum: bit-equal to ATen'
    assert _within(P.join([dy], y=y, post=2), D(dy) * (y > 0), dy * (y > 0), 'dy (y > 0)')
    gain = 1.0 / (shape[2] * shape[3])
    mean = P.plane_sums(a, None, gain)
    assert _within(mean, D(a).mean(dim=(2, 3), keepdim=True), a.mean(dim=(2, 3), keepdim=True), 'mean')
    dot = P.plane_sums(dy, a)
    assert _within(dot, (D(dy) * D(a)).sum(dim=(2, 3), keepdim=True), (dy * a).sum(dim=(2, 3), keepdim=True), 'dot')
    assert torch.equal(P.plane_sums(a, None, gain), mean) and torch.equal(P.plane_sums(dy, a), dot) and torch.equal(P.join([a, b], post=1), y)


@pytest.mark.parametrize('what', list(WRAP))
def test_pools_where_the_grid_wraps(gpu_device, what):
    """maxpool3s2 + its backward and LPIPS's maxpool2, bit-equal to ATen as in tests/test_gpu_parse_loss.py / test_gpu_lpips.py.  On a
    725 x 725 plane the backward's grid (over the input's pixels) wraps; the forward pools' grids run over the outputs, so a 1451 x 1451
    plane, with 726 x 726 and 725 x 725 of them, is run as well."""
    from torch_utils import hip_plugin
    P, Q = hip_plugin.ParseLossPlugin, hip_plugin.LpipsPlugin
    for shape in ([(1, 65539, 3, 3)] if what == 'planes' else [WRAP[what], (1, 1, 1451, 1451)]):
        x = _rand(shape, 54, gpu_device)
        y, idx = P.maxpool(x)
        assert torch.equal(y, F.max_pool2d(x, 3, 2, 1))
        dy = _rand(tuple(y.shape), 55, gpu_device)
        want = _aten_vjp(lambda t: F.max_pool2d(t, 3, 2, 1), x, dy)
        dx = P.maxpool_backward(dy, idx, shape[2:])
        assert torch.equal(dx, want)
        assert torch.equal(P.maxpool_backward(dy, idx, shape[2:], mask=x), want * (x > 0))
        assert torch.equal(P.maxpool_backward(dy, idx, shape[2:]), dx)
        assert torch.equal(Q.maxpool2(x), F.max_pool2d(x, 2))


@pytest.mark.parametrize('shape,size', [((1, 65539, 2, 2), (3, 3)), ((1, 1, 91, 91), (725, 725))], ids=list(WRAP))
def test_resize_where_the_grid_wraps(gpu_device, shape, size):
    """The forward wraps over the planes / the 725 x 725 output pixels; the adjoint over the planes, and over the pixels of its own output
    in the other direction (725 x 725 -> 91 x 91 reads every pixel; 91 x 91 <- 725 x 725 as the gradient of an up-sampling)."""
    from torch_utils import hip_plugin
    P = hip_plugin.ParseLossPlugin
    x, dy = _rand(shape, 57, gpu_device), _rand(shape[:2] + size, 58, gpu_device)
    up = lambda t: F.interpolate(t, size, mode='bilinear', align_corners=True)
    y = P.resize(x, size)
    assert _within(y, up(x.double()), up(x), 'resize')
    dx = P.resize_backward(dy, shape[2:])
    assert _within(dx, _aten_vjp(up, x.double(), dy.double()), _aten_vjp(up, x, dy), 'adjoint')
    assert torch.equal(P.resize_backward(dy, shape[2:]), dx) and torch.equal(P.resize(x, size), y)
    if shape[1] == 1:          # the adjoint's own grid: a 725 x 725 input gradient of a down-sampling to 91 x 91
        down = lambda t: F.interpolate(t, shape[2:], mode='bilinear', align_corners=True)
        big, g = _rand((1, 1) + size, 59, gpu_device), _rand(shape, 60, gpu_device)
        assert _within(P.resize(big, shape[2:]), down(big.double()), down(big), 'down-sampling')
        assert _within(P.resize_backward(g, size), _aten_vjp(down, big.double(), g.double()), _aten_vjp(down, big, g), 'its adjoint')


def test_loss_head_on_more_pixels_than_a_grid_holds(gpu_device):
    """[1, 20, 91, 91] logits against 725 x 725 labels: 2054 workgroups of 256 pixels, whose partial sums the finishing launch adds."""
    from torch_utils import hip_plugin
    P = hip_plugin.ParseLossPlugin
    lg = _rand((1, 20, 91, 91), 61, gpu_device)
    lab = torch.randint(0, 20, (1, 725, 725), generator=torch.Generator().manual_seed(62)).to(gpu_device)
    ce = lambda t: F.cross_entropy(F.interpolate(t, (725, 725), mode='bilinear', align_corners=True), lab)
    loss, lse = P.ce(lg, lab)
    assert _within(loss, ce(lg.double()), ce(lg), 'loss')
    dloss = torch.tensor([0.7], device=gpu_device)
    dl = P.ce_backward(lg, lab, lse, dloss)
    want = _aten_vjp(ce, lg.double(), torch.tensor(0.7, dtype=torch.float64, device=gpu_device))
    assert _within(dl, want, _aten_vjp(ce, lg, dloss[0]), 'dlogits')
    loss2, lse2 = P.ce(lg, lab)
    assert torch.equal(loss2, loss) and torch.equal(lse2, lse) and torch.equal(P.ce_backward(lg, lab, lse, dloss), dl)
