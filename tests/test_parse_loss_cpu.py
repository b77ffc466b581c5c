"""The face parser's cross-entropy loss (training/parse_loss.py) without a GPU: the definition against the fixture written from the
reference's own BiSeNet (scripts/make_parse_loss_golden.py), the orchestration of the fused pass - run here on a float64 torch restatement
of every launch (tests/parse_loss_ref.py `TorchOps`) - against autograd, the weight orientation of the stride-2 gradient, the projector
closure, the C ABI of csrc/parse_loss.hip and the convolution plan of the pass at 512 x 512."""

import ctypes
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import parse_loss_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _ulp(v):
    return float(np.spacing(np.float32(abs(float(v)))))


_nets = {}


def _net(dtype=torch.float32):
    if dtype not in _nets:
        _nets[dtype] = R.parser(dtype=dtype)
    return _nets[dtype]


@pytest.mark.parametrize('case', [0, 1])
def test_definition_against_the_reference_fixture(case):
    """Bound: 4 x the difference between this project's BiSeNet in float32 and in float64 on the same input, plus one fp32 ulp of the largest
    magnitude (the fixture is the reference's float32 run: another summation order inside the same 32 convolutions)."""
    from training import parse_loss
    img, lab, want_loss, want_grad = R.fixture(case)
    assert tuple(img.shape) == R.CASES[case] and lab.dtype == torch.int64 and int(lab.min()) >= 0 and int(lab.max()) <= 19
    leaf = img.clone().requires_grad_(True)
    loss = parse_loss.cross_entropy(_net(), leaf, lab)
    (grad,) = torch.autograd.grad(loss, [leaf])
    assert loss.ndim == 0 and loss.dtype == torch.float32
    l64, g64 = R.definition(_net(torch.float64), img.double(), lab)
    bound_l = 4 * abs(float(loss.detach()) - float(l64)) + _ulp(l64)
    bound_g = 4 * float((grad.double() - g64).abs().max()) + _ulp(g64.abs().max())
    err_l, err_g = abs(float(loss.detach()) - float(want_loss)), float((grad - want_grad).abs().max())
    print(f'loss {float(loss.detach()):.6f}: |own - fixture| {err_l:.3e} (bound {bound_l:.3e}); gradient max |own - fixture| {err_g:.3e} (bound {bound_g:.3e})')
    assert err_l <= bound_l and err_g <= bound_g
    assert float(want_grad.abs().max()) > 0


@pytest.mark.parametrize('case', [0, 1])
def test_fused_orchestration_against_autograd(case):
    """`_fused_forward` / `_fused_backward` - what the HIP path runs - with every launch restated in float64 torch: the loss and the image
    gradient equal autograd through the float64 definition up to the float32 folding of the BatchNorms (1e-5 relative; a wrong crop, a
    dropped branch or a mis-scaled mean gradient is 1e-2 or more)."""
    from training import parse_loss
    img, lab, _, _ = R.fixture(case)
    l64, g64 = R.definition(_net(torch.float64), img.double(), lab)
    ops = R.TorchOps(torch.float64)
    with torch.no_grad():
        loss, sv = parse_loss._fused_forward(ops, _net(), img.double(), lab)
        grad = parse_loss._fused_backward(ops, _net(), sv, torch.full([1], 0.5, dtype=torch.float64))
    assert abs(float(loss) - float(l64)) <= 1e-5 * float(l64)
    assert float((grad - 0.5 * g64).norm() / (0.5 * g64).norm()) <= 1e-5


@pytest.mark.parametrize('k,stride', [(3, 2), (1, 2), (3, 1), (1, 1)])
def test_conv_grad_is_the_adjoint_of_conv(k, stride):
    """`parse_loss._conv_grad` against autograd through `parse_loss._conv`, both on the torch restatement of the kernel's three modes
    (tests/test_gpu_ops.py pins mode 2 to conv_transpose2d(x, w_given.transpose(0, 1), stride=2)): the weight orientation of the mode 1 /
    mode 2 pair and the crop to rows and columns 1..h for 3x3 stride 2, the half-resolution gradient for 1x1 stride 2 (scattered to the
    even positions by the join), the transposed and flipped weights for stride 1.  A BatchNorm is folded in."""
    from training import parse_loss
    torch.manual_seed(k * 10 + stride)
    conv, bn = torch.nn.Conv2d(3, 5, k, stride, k // 2, bias=False), torch.nn.BatchNorm2d(5).eval()
    with torch.no_grad():
        bn.running_mean.normal_(); bn.running_var.uniform_(0.5, 1.5); bn.weight.normal_(); bn.bias.normal_()
    for m in (conv, bn):
        m.requires_grad_(False)
    ops = R.TorchOps(torch.float64)
    x = torch.randn(2, 3, 8, 12, dtype=torch.float64, requires_grad=True)
    y = parse_loss._conv(ops, x, conv, bn)
    assert float((y.detach() - bn.double()(conv.double()(x.detach()))).abs().max()) <= 1e-5          # (folded in float32)
    conv.float(); bn.float()
    dy = torch.randn(y.shape, dtype=torch.float64)
    (want,) = torch.autograd.grad(y, [x], dy)
    with torch.no_grad():
        got = parse_loss._conv_grad(ops, dy, conv, bn, size=(8, 12))
    if (k, stride) == (1, 2):
        assert tuple(got.shape) == (2, 3, 4, 6)
        got = ops.join([torch.zeros_like(want), (got, True)])
    assert got.shape == want.shape
    assert float((got - want).abs().max()) <= 1e-12 * max(float(want.abs().max()), 1.0)


def test_labels_equal_the_parsing_img_spelling():
    from training import face_parsing, parse_loss
    img = R.fixture(1)[0]
    lab = parse_loss.labels(_net(), img)
    assert lab.dtype == torch.int64 and tuple(lab.shape) == (1, 96, 64) and not lab.requires_grad
    assert torch.equal(lab, face_parsing.parsing_img(_net(), img, argmax=True, return_mask=False, remap=False)[1].squeeze(1))


def test_parse_distance_with_a_base_is_the_hand_written_sum():
    from training import parse_loss, projection
    img, lab, _, _ = R.fixture(1)
    images = (img + 1) * 127.5
    other = torch.rand(1, 3, 96, 64, generator=torch.Generator().manual_seed(3)) * 255
    base = projection.l2_distance(other)
    d = parse_loss.parse_distance(lab, _net(), weight=0.25, base=base)
    want = 0.25 * F.cross_entropy(_net()(images / 127.5 - 1)[0], lab) + base(images)
    assert torch.equal(d(images), want)
    # an image target: its labels are computed once, by `labels`
    d_img = parse_loss.parse_distance(other, _net())
    assert torch.equal(d_img(images), F.cross_entropy(_net()(images / 127.5 - 1)[0], parse_loss.labels(_net(), other / 127.5 - 1)))
    leaf = images.clone().requires_grad_(True)
    (g,) = torch.autograd.grad(d(leaf), [leaf])
    assert bool(torch.isfinite(g).all()) and float(g.abs().max()) > 0


def test_switches_and_cpu_routing():
    from training import parse_loss
    assert isinstance(parse_loss.fused, bool) and parse_loss.arith == 0
    assert not parse_loss._on_hip(_net(), torch.zeros(1, 3, 64, 64)), 'CPU tensors take the PyTorch definition'
    assert parse_loss._sides_ok(64, 96) and not parse_loss._sides_ok(72, 72) and not parse_loss._sides_ok(32, 64)


def test_project_with_parse_distance_on_cpu_tensors():
    from training import parse_loss, projection, triplane
    torch.manual_seed(0)
    G = triplane.TriPlaneGenerator(triplane.tiny_spec()).eval()
    c = triplane.camera_label(0.2)
    target = torch.rand(3, G.img_resolution, G.img_resolution, generator=torch.Generator().manual_seed(1)) * 255
    d = parse_loss.parse_distance(target[None], _net(), weight=0.1, base=projection.l2_distance(target[None]))
    p = projection.Projector(G, target, c, num_steps=2, w_avg_samples=32, distance=d)
    start = p.pivot().clone()
    losses = [float(p.step(i)) for i in range(2)]
    assert all(v == v and abs(v) != float('inf') for v in losses)
    assert bool(torch.isfinite(p.pivot()).all()) and not torch.equal(p.pivot(), start)


# ---- the C ABI ---------------------------------------------------------------------------------------------------------------------------------
def _header():
    return re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'ide3d_hip.h')).read(), flags=re.S)


SIGNATURES = (
    'int ide3d_resize_bilinear(const float* x, float* y, int64_t planes, int32_t h, int32_t w, int32_t H, int32_t W, void* stream);',
    'int ide3d_resize_bilinear_backward(const float* dy, float* dx, int64_t planes, int32_t h, int32_t w, int32_t H, int32_t W, void* stream);',
    'int64_t ide3d_parse_ce_workspace_bytes(int32_t n, int32_t C, int32_t h, int32_t w, int32_t H, int32_t W);',
    'int ide3d_parse_ce(const float* logits, const int64_t* labels, int32_t n, int32_t C, int32_t h, int32_t w, int32_t H, int32_t W, '
    'double* lse, float* workspace, int64_t workspace_bytes, float* loss, void* stream);',
    'int ide3d_parse_ce_backward(const float* logits, const int64_t* labels, const double* lse, const float* dloss, float* dlogits, '
    'int32_t n, int32_t C, int32_t h, int32_t w, int32_t H, int32_t W, void* stream);',
    'int ide3d_maxpool3s2(const float* x, float* y, uint8_t* idx, int64_t planes, int32_t h, int32_t w, void* stream);',
    'int ide3d_maxpool3s2_backward(const float* dy, const uint8_t* idx, const float* mask, float* dx, int64_t planes, int32_t h, int32_t w, '
    'void* stream);',
    'int ide3d_parse_join(const ide3d_parse_join_params* p, void* stream);',
    'int ide3d_plane_sums(const float* a, const float* b, float* out, int64_t planes, int64_t hw, float gain, void* stream);',
    'int ide3d_parse_stem_backward(const float* dz, const float* weight, float* dx, int32_t n, int32_t cout, int32_t H, int32_t W, void* stream);',
)


def test_entry_points_are_declared_listed_and_exported():
    from torch_utils import hip_plugin
    h = re.sub(r'\s+', ' ', _header())
    path = hip_plugin.lib_path()
    assert os.path.isfile(path), f'{path} missing: run __graft_entry__.build()'
    lib = ctypes.CDLL(path)
    for sig in SIGNATURES:
        assert sig in h, sig
        name = re.search(r'(ide3d_\w+)\(', sig).group(1)
        assert name in hip_plugin.EXPORTED_SYMBOLS and hasattr(lib, name), name
    assert hip_plugin._ABI_VERSION == 8 and lib.ide3d_abi_version() == 8
    assert hip_plugin.PLUGINS['parse_loss_plugin'] is hip_plugin.ParseLossPlugin
    # the ctypes prototypes: one argument type per parameter of the header
    loaded = hip_plugin.load()
    for sig in SIGNATURES:
        name = re.search(r'(ide3d_\w+)\(', sig).group(1)
        params = sig[sig.index('(') + 1:sig.rindex(')')].split(',')
        fn = getattr(loaded, name)
        assert len(fn.argtypes) == len(params), name
        assert fn.restype is (ctypes.c_int64 if sig.startswith('int64_t') else ctypes.c_int), name
        for a, decl in zip(fn.argtypes, params):
            want = ctypes.c_int32 if 'int32_t' in decl and '*' not in decl else ctypes.c_int64 if 'int64_t' in decl and '*' not in decl else \
                ctypes.c_float if decl.strip().startswith('float ') else None
            assert (a is want) if want is not None else ('*' in decl), (name, decl)


def test_join_struct_matches_header():
    from torch_utils import hip_plugin

    def names(struct):
        body = re.search(r'typedef struct %s \{(.*?)\} %s;' % (struct, struct), _header(), re.S).group(1)
        return [n for d in body.split(';') if d.strip() for n in re.findall(r'([A-Za-z_][A-Za-z0-9_]*)(?:\[\w+\])?\s*(?:,|$)', d.strip())]
    assert names('ide3d_parse_term') == [f[0] for f in hip_plugin._ParseTerm._fields_] == ['p', 'batch_stride', 'plane_stride', 'row_pitch', 'half']
    assert names('ide3d_parse_join_params') == [f[0] for f in hip_plugin._ParseJoinParams._fields_]
    assert ctypes.sizeof(hip_plugin._ParseTerm) == 32 and ctypes.sizeof(hip_plugin._ParseJoinParams) == 152
    assert hip_plugin._ParseJoinParams.scale.offset == 96 and hip_plugin._ParseJoinParams.n.offset == 128
    assert int(re.search(r'#define IDE3D_PARSE_JOIN_TERMS (\d+)', _header()).group(1)) == hip_plugin.PARSE_JOIN_TERMS


def test_workspace_query_and_argument_checks():
    """8 bytes per loss-head workgroup of 256 image pixels; bad arguments are refused before anything is launched."""
    from torch_utils import hip_plugin
    lib = hip_plugin.load()
    assert lib.ide3d_parse_ce_workspace_bytes(4, 20, 64, 64, 512, 512) == 4 * 512 * 512 // 256 * 8
    assert lib.ide3d_parse_ce_workspace_bytes(1, 20, 8, 8, 64, 65) == (64 * 65 + 255) // 256 * 8
    assert lib.ide3d_parse_ce_workspace_bytes(1, 0, 8, 8, 64, 64) == -1 and lib.ide3d_parse_ce_workspace_bytes(1, 20, 8, 8, 1, 64) == -1
    assert lib.ide3d_parse_ce(None, None, 1, 20, 8, 8, 64, 64, None, None, 0, None, None) == -1 and b'null pointer' in lib.ide3d_last_error()
    assert lib.ide3d_parse_ce(16, 16, 1, 20, 8, 8, 64, 64, 16, 16, 8, 16, None) == -1 and b'workspace' in lib.ide3d_last_error()
    assert lib.ide3d_resize_bilinear(16, 16, 1, 4, 4, 1, 8, None) == -1 and b'H, W >= 2' in lib.ide3d_last_error()
    assert lib.ide3d_resize_bilinear_backward(16, 16, 0, 4, 4, 8, 8, None) == -1
    assert lib.ide3d_maxpool3s2(None, 16, None, 1, 4, 4, None) == -1
    assert lib.ide3d_maxpool3s2_backward(16, None, None, 16, 1, 4, 4, None) == -1
    assert lib.ide3d_plane_sums(16, None, 16, 0, 4, 1.0, None) == -1
    assert lib.ide3d_parse_stem_backward(16, 16, 16, 1, 65, 64, 64, None) == -1 and b'cout' in lib.ide3d_last_error()
    p = hip_plugin._ParseJoinParams()
    assert lib.ide3d_parse_join(ctypes.byref(p), None) == -1
    p.out, p.n, p.c, p.h, p.w = 16, 1, 2, 4, 4
    p.term[0].p, p.term[0].batch_stride, p.term[0].plane_stride, p.term[0].row_pitch = 16, 32, 16, 3
    assert lib.ide3d_parse_join(ctypes.byref(p), None) == -1 and b'row pitch' in lib.ide3d_last_error()
    p.term[0].row_pitch, p.post = 4, 2
    assert lib.ide3d_parse_join(ctypes.byref(p), None) == -1 and b'post' in lib.ide3d_last_error()


# ---- the convolution plan ------------------------------------------------------------------------------------------------------------------------
class _RecordingOps(R.TorchOps):
    """TorchOps that notes every convolution launch: (cin, cout, h, w, k, mode, epilogue)."""

    def __init__(self):
        super().__init__(torch.float32)
        self.launches = []

    def conv(self, x, w, bias, relu, mode=0):
        self.launches.append((x.shape[1], w.shape[0], x.shape[2], x.shape[3], w.shape[2], mode, 'relu' if relu else ('bias' if bias is not None else 'grad')))
        return super().conv(x, w, bias, relu, mode)


def launches_at(side, base=64):
    """The convolution launches of one forward + backward at side x side: recorded at base x base, where every map but the global averages
    (1 x 1 at every size) scales with the image; the stride-2 mode reads the map padded by one pixel on every side."""
    from training import parse_loss
    net, ops = _net(), _RecordingOps()
    img, lab = torch.zeros(1, 3, base, base), torch.zeros(1, base, base, dtype=torch.int64)
    with torch.no_grad():
        loss, sv = parse_loss._fused_forward(ops, net, img, lab)
        forward = len(ops.launches)
        parse_loss._fused_backward(ops, net, sv, torch.ones(1))
    f = side // base

    def scaled(v, mode):
        return v if v == 1 else ((v - 2) * f + 2 if mode == 1 else v * f)
    out = [(cin, cout, scaled(h, mode), scaled(w, mode), k, mode, ep) for cin, cout, h, w, k, mode, ep in ops.launches]
    return out[:forward], out[forward:]


def test_every_convolution_launch_at_512_has_a_kernel():
    """The 32 convolutions of the parser and the 31 of its input gradient that are ide3d_modconv2d launches (the 32nd, the stem's, is
    ide3d_parse_stem_backward) at 512 x 512, batch 1 and 4, in bf16x6 and fp32."""
    from torch_utils import hip_plugin
    fwd, bwd = launches_at(512)
    assert len(fwd) == 32 and len(bwd) == 31
    assert fwd[0] == (147, 64, 256, 256, 1, 0, 'relu'), 'the stem: a 1x1 convolution over its unfolded 7x7 patches'
    assert sum(1 for l in fwd if l[5] == 1) == 3 and sum(1 for l in bwd if l[5] == 2) == 3
    assert all(l[6] == 'grad' for l in bwd)
    kinds = set()
    for cin, cout, h, w, k, mode, ep in fwd + bwd:
        for n in (1, 4):
            for arith in (6, 1):
                plan = hip_plugin.modconv_plan(n, cin, cout, h, w, k=k, mode=mode, arith=arith, epilogue=ep)
                assert plan['workgroups'] > 0, (cin, cout, h, w, k, mode, ep, n, arith)
                kinds.add(plan['kind'])
    assert 'split' in kinds or 'split_teams' in kinds, 'the wide 3x3 layers take the split-bf16 family in bf16x6'
