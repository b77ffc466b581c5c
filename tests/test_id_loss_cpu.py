"""The ArcFace identity loss (training/id_loss.py) without a GPU: the net's keys and the definition against the fixture written from the
reference's own classes (scripts/make_id_loss_golden.py), the orchestration of the fused pass - run here on a float64 torch restatement of
every launch (tests/id_loss_ref.py `TorchOps`) - against float64 autograd of an independent functional restatement, the reference's triple,
the projector closure, the routing rules, the overlay of `inversion.criteria.id_loss` and the C ABI of csrc/id_loss.hip."""

import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import id_loss_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _ulp(v):
    return float(np.spacing(np.float32(abs(float(v)))))


_memo = {}


def _idloss(spec='IR_SE50', dtype=torch.float32):
    if (spec, dtype) not in _memo:
        _memo[(spec, dtype)] = R.idloss(getattr(R, spec), dtype=dtype)
    return _memo[(spec, dtype)]


def _float64(case):
    """The float64 restatement on the fixture's inputs, computed once: (loss, gradient, e(y_hat), e(y))."""
    if case not in _memo:
        fx = R.fixture(case)
        _memo[case] = R.loss64(_idloss().facenet, fx['y_hat'], fx['y'], R.IR_SE50['units'])
    return _memo[case]


def test_state_dict_keys_and_order_equal_the_reference():
    from training import id_loss
    keys = R.fixture_keys()
    net = id_loss.Backbone(112, 50, mode='ir_se', drop_ratio=0.6)
    assert list(net.state_dict().keys()) == keys and len(keys) == 397
    sd = R.synthetic_state_dict({k: list(v.shape) for k, v in net.state_dict().items()})
    assert list(sd.keys()) == keys
    net.load_state_dict(sd, strict=True)
    crit = id_loss.IDLoss(weights=sd)
    assert not crit.facenet.training and not any(p.requires_grad for p in crit.parameters())
    assert torch.equal(crit.facenet.state_dict()['body.23.res_layer.5.fc2.weight'], sd['body.23.res_layer.5.fc2.weight'])
    crit.train()
    assert not crit.facenet.training
    # the block plan: every stage's first block has stride 2; the width decides the shortcut kind
    assert [b.stride for b in net.body] == [2, 1, 1, 2, 1, 1, 1, 2] + [1] * 13 + [2, 1, 1]
    assert isinstance(net.body[0].shortcut_layer, torch.nn.MaxPool2d) and isinstance(net.body[3].shortcut_layer, torch.nn.Sequential)


@pytest.mark.parametrize('case', [0, 1])
def test_definition_against_the_reference_fixture(case):
    """The module's PyTorch definition in fp32 against the fixture (the reference's fp32 run).  Bound per quantity, by the triangle
    inequality: 4 x the distance of this module's fp32 result to float64 + the fixture's own distance to float64, with a floor of one fp32
    ulp of the largest magnitude.  The gradient is exactly zero outside the crop."""
    fx = R.fixture(case)
    assert tuple(fx['y_hat'].shape) == R.CASES[case]
    crit = _idloss()
    l64, g64, e64, t64 = _float64(case)
    leaf = fx['y_hat'].clone().requires_grad_(True)
    loss, sim, logs = crit(leaf, fx['y'], fx['y'])
    (grad,) = torch.autograd.grad(loss, [leaf])
    f = R.CASES[case][2] // 256
    outside = grad.clone()
    outside[:, :, 35 * f:223 * f, 32 * f:220 * f] = 0
    assert float(outside.abs().max()) == 0.0 and float(grad.abs().max()) > 0
    feats_hat, feats = crit.features(fx['y_hat']), crit.features(fx['y'])

    def check(what, own, fixture, want):
        own, fixture, want = (torch.as_tensor(t).double() for t in (own, fixture, want))
        e_own, e_fix = float((own - want).abs().max()), float((fixture - want).abs().max())
        floor = _ulp(want.abs().max())
        err = float((own - fixture).abs().max())
        print(f'case {case} {what}: |own - fixture| {err:.3e}; own error {e_own:.3e}, fixture error {e_fix:.3e}, one ulp of the largest magnitude {floor:.3e}')
        assert err <= max(4 * e_own, floor) + e_fix, what
    check('embeddings of y_hat', feats_hat, fx['feats_hat'], e64)
    check('embeddings of y', feats, fx['feats'], t64)
    check('loss', loss.detach(), fx['loss'], l64)
    check('sim_improvement', sim, fx['sim'], l64 * -1.0)
    check('gradient samples', R.crop_samples(grad), fx['grad_samples'], R.crop_samples(g64))
    check('gradient sum', grad.double().sum(), fx['grad_sum'], g64.sum())
    check('gradient norm', grad.double().norm(), fx['grad_norm'], g64.norm())


@pytest.mark.parametrize('spec,shape', [('NARROW', (2, 3, 256, 256)), ('SHORT', (1, 3, 512, 512))])
def test_fused_orchestration_against_float64_autograd(spec, shape):
    """`_fused_forward` / `_fused_backward` - what the HIP path runs - with every launch restated in float64 torch: loss, embeddings and
    image gradient equal float64 autograd of the functional restatement up to the float32 folding of the BatchNorms (1e-5 relative; a wrong
    crop, a dropped shortcut or a mis-scaled mean gradient is 1e-2 or more)."""
    from training import id_loss
    crit = _idloss(spec)
    y_hat, y = R.to_float(R.smooth_images(shape, 3)), R.to_float(R.smooth_images(shape, 4))
    l64, g64, e64, t64 = R.loss64(crit.facenet, y_hat, y, getattr(R, spec)['units'])
    ops = R.TorchOps(torch.float64)
    with torch.no_grad():
        loss, e, sv = id_loss._fused_forward(ops, crit.facenet, y_hat.double(), t64)
        grad = id_loss._fused_backward(ops, crit.facenet, sv, torch.full([1], 0.5, dtype=torch.float64))
        assert id_loss._fused_forward(ops, crit.facenet, y.double(), None)[0] is None
    assert float((e - e64).abs().max()) <= 1e-5
    assert abs(float(loss) - l64) <= 1e-5 * l64
    assert float((grad - 0.5 * g64).norm() / (0.5 * g64).norm()) <= 1e-5
    assert tuple(grad.shape) == shape


def test_forward_returns_the_reference_triple_and_distance_to_its_loss():
    from training import id_loss
    crit = _idloss('NARROW')
    y_hat, y, x = (R.to_float(R.smooth_images((2, 3, 256, 256), s)) for s in (5, 6, 7))
    loss, sim, logs = crit(y_hat, y, x)
    e_hat, e_y, e_x = (crit.extract_feats(t) for t in (y_hat, y, x))
    assert float((e_hat.norm(dim=1) - 1).abs().max()) <= 1e-6
    assert isinstance(sim, float) and len(logs) == 2 and all(set(d) == {'diff_target', 'diff_input', 'diff_views'} for d in logs)
    want, want_sim = 0, 0
    for i in range(2):                                               # the reference's loop (id_loss.py:37-47)
        dt, di, dv = e_hat[i].dot(e_y[i]), e_hat[i].dot(e_x[i]), e_y[i].dot(e_x[i])
        assert logs[i]['diff_target'] == pytest.approx(float(dt), abs=1e-6) and logs[i]['diff_input'] == pytest.approx(float(di), abs=1e-6)
        assert logs[i]['diff_views'] == pytest.approx(float(dv), abs=1e-6)
        want, want_sim = want + 1 - dt, want_sim + float(dt) - float(dv)
    assert float(loss) == pytest.approx(float(want / 2), abs=1e-6) and sim == pytest.approx(want_sim / 2, abs=1e-6)
    feats = crit.features(y)
    assert not feats.requires_grad and torch.equal(feats, e_y)
    assert torch.equal(crit.distance_to(y_hat, feats), loss)
    # x is y: the features are computed once
    calls = []
    hook = crit.facenet.register_forward_hook(lambda *a: calls.append(1))
    crit(y_hat, y, y)
    hook.remove()
    assert len(calls) == 2
    # the gradient flows to y_hat only
    a, b = y_hat.clone().requires_grad_(True), y.clone().requires_grad_(True)
    crit(a, b, b)[0].backward()
    assert a.grad is not None and float(a.grad.abs().max()) > 0 and b.grad is None
    assert 'RANDOMLY INITIALISED' in id_loss.IDLoss.__doc__ and 'RANDOMLY INITIALISED' in id_loss.__doc__


def test_id_distance_with_a_base_is_the_hand_written_sum():
    from training import id_loss, projection
    crit = _idloss('SHORT')
    target, images, other = (torch.from_numpy(R.smooth_images((1, 3, 256, 256), s)).float() for s in (8, 9, 10))
    base = projection.l2_distance(other)
    d = id_loss.id_distance(target, crit, weight=0.25, base=base)
    want = 0.25 * crit.distance_to(images / 127.5 - 1, crit.features(target / 127.5 - 1)) + base(images)
    assert torch.equal(d(images), want)
    assert torch.equal(id_loss.id_distance(target, crit)(images), crit.distance_to(images / 127.5 - 1, crit.features(target / 127.5 - 1)))
    leaf = images.clone().requires_grad_(True)
    (g,) = torch.autograd.grad(d(leaf), [leaf])
    assert bool(torch.isfinite(g).all()) and float(g.abs().max()) > 0


def test_project_with_id_distance_on_cpu_tensors():
    from training import id_loss, projection, triplane
    torch.manual_seed(0)
    G = triplane.TriPlaneGenerator(triplane.tiny_spec()).eval()
    c = triplane.camera_label(0.2)
    target = torch.rand(3, G.img_resolution, G.img_resolution, generator=torch.Generator().manual_seed(1)) * 255
    d = id_loss.id_distance(target[None], _idloss('SHORT'), weight=0.1, base=projection.l2_distance(target[None]))
    p = projection.Projector(G, target, c, num_steps=3, w_avg_samples=32, distance=d)
    start = p.pivot().clone()
    losses = [float(p.step(i)) for i in range(3)]
    assert all(v == v and abs(v) != float('inf') for v in losses)
    assert bool(torch.isfinite(p.pivot()).all()) and not torch.equal(p.pivot(), start)


def test_switches_and_cpu_routing():
    """Without a GPU everything takes the PyTorch definition; `_on_hip` refuses what the fused route does not cover whatever the device."""
    from training import id_loss
    assert isinstance(id_loss.fused, bool) and id_loss.arith == 0
    crit = _idloss('SHORT')
    net = crit.facenet
    img = R.to_float(R.smooth_images((1, 3, 256, 256), 12))
    assert not id_loss._on_hip(net, img), 'CPU tensors'
    assert not id_loss._on_hip(net, img.half()) and not id_loss._on_hip(net, torch.zeros(1, 3, 256, 512)) and not id_loss._on_hip(net, torch.zeros(1, 3, 384, 384))
    want = crit._definition(img)
    assert torch.equal(crit.extract_feats(img), want)
    old = id_loss.fused
    id_loss.fused = False
    try:
        assert torch.equal(crit.extract_feats(img), want)
    finally:
        id_loss.fused = old
    # other sizes go through the reference's poolings (the first one only when the HEIGHT is not 256, as the reference tests); H = 384 and H != W
    for shape in ((1, 3, 384, 384), (1, 3, 256, 320)):
        x = torch.rand(shape, generator=torch.Generator().manual_seed(13)) * 2 - 1
        e = crit.extract_feats(x)
        assert tuple(e.shape) == (1, 512) and torch.equal(e, net(crit.face_pool((crit.pool(x) if shape[2] != 256 else x)[:, :, 35:223, 32:220])))
    # mode='ir' builds the block without a gate and runs the definition
    ir = R.idloss(R.SHORT, mode='ir')
    assert not any('fc1' in k for k in ir.facenet.state_dict()) and tuple(ir.extract_feats(img).shape) == (1, 512)
    assert not id_loss._on_hip(ir.facenet, img)
    # a trainable parameter: the definition, and its gradient exists
    p = net.input_layer[0].weight
    p.requires_grad_(True)
    try:
        assert not id_loss._on_hip(net, img)
        crit.distance_to(img, crit.features(img.flip(3))).backward()
        assert p.grad is not None
    finally:
        p.requires_grad_(False)
        p.grad = None


def _reference_root():
    from oracle import ref_import
    return ref_import.REFERENCE_ROOT


@pytest.mark.skipif(not os.path.isdir(os.path.join(_reference_root(), 'inversion', 'criteria')),
                    reason='needs the reference tree for the modules the overlay does not replace')
def test_overlay_replaces_id_loss_and_nothing_else(tmp_path):
    """In a fresh interpreter with this package in front of the reference on sys.path: `inversion.criteria.id_loss.IDLoss` is this
    package's and loads `paths_config.ir_se50` in its constructor; `inversion.criteria.l2_loss` still comes from the reference."""
    ref = _reference_root()
    weights = tmp_path / 'w.pth'
    code = f'''
import sys, types
sys.path[:0] = [{os.path.join(ROOT, "ide-3d_amd")!r}, {ref!r}]
sys.modules.setdefault('cv2', types.ModuleType('cv2'))
import torch
import inversion.criteria.id_loss as m, inversion.criteria.l2_loss as l2, inversion.configs.paths_config as pc
from training import id_loss
assert m.__file__.startswith({os.path.join(ROOT, "ide-3d_amd")!r}), m.__file__
assert l2.__file__.startswith({ref!r}), l2.__file__
assert issubclass(m.IDLoss, id_loss.IDLoss)
torch.manual_seed(0)
sd = id_loss.Backbone().state_dict()
torch.save(sd, {str(weights)!r})
pc.ir_se50 = {str(weights)!r}
crit = m.IDLoss()
assert torch.equal(crit.facenet.state_dict()['output_layer.3.weight'], sd['output_layer.3.weight']) and not crit.facenet.training
print('overlay ok')
'''
    out = subprocess.run([sys.executable, '-c', code], capture_output=True, text=True)
    assert out.returncode == 0 and 'overlay ok' in out.stdout, out.stderr[-2000:]


# ---- the C ABI ---------------------------------------------------------------------------------------------------------------------------------
def _header():
    return re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'ide3d_hip.h')).read(), flags=re.S)


NAMES = ('ide3d_id_prep', 'ide3d_id_prep_backward', 'ide3d_prelu', 'ide3d_prelu_backward', 'ide3d_se_gate', 'ide3d_se_gate_backward',
         'ide3d_linear_workspace_bytes', 'ide3d_linear_backward_input_workspace_bytes', 'ide3d_linear', 'ide3d_linear_backward_input',
         'ide3d_id_head', 'ide3d_id_head_backward')


def test_entry_points_are_declared_listed_and_exported():
    """Every entry point csrc/id_loss.hip defines is declared in the header, listed by the binding and exported, and the reverse; the
    ctypes prototype has one argument type per parameter of the declaration."""
    from torch_utils import hip_plugin
    h = re.sub(r'\s+', ' ', _header())
    src = open(os.path.join(ROOT, 'ide-3d_amd', 'csrc', 'id_loss.hip')).read()
    defined = set(re.findall(r'extern "C" \w+ (ide3d_\w+)\(', src))
    assert defined == set(NAMES)
    path = hip_plugin.lib_path()
    assert os.path.isfile(path), f'{path} missing: run __graft_entry__.build()'
    lib, loaded = ctypes.CDLL(path), hip_plugin.load()
    for name in NAMES:
        m = re.search(r'(int64_t|int) %s\(([^)]*)\);' % name, h)
        assert m, f'{name} is not declared in the header'
        assert name in hip_plugin.EXPORTED_SYMBOLS and hasattr(lib, name), name
        params = m.group(2).split(',')
        fn = getattr(loaded, name)
        assert len(fn.argtypes) == len(params), name
        assert fn.restype is (ctypes.c_int64 if m.group(1) == 'int64_t' else ctypes.c_int), name
        for a, decl in zip(fn.argtypes, params):
            want = ctypes.c_int32 if 'int32_t' in decl and '*' not in decl else ctypes.c_int64 if 'int64_t' in decl and '*' not in decl else None
            assert (a is want) if want is not None else ('*' in decl), (name, decl)
    assert hip_plugin._ABI_VERSION == 8 and lib.ide3d_abi_version() == 8
    assert hip_plugin.PLUGINS['id_loss_plugin'] is hip_plugin.IdLossPlugin


def test_workspace_queries_and_argument_checks():
    """One float per slice of 2048 columns (forward) or 64 rows (input gradient), image and output; what the kernels do not cover is
    declined, and bad arguments are refused before anything is launched."""
    from torch_utils import hip_plugin
    lib = hip_plugin.load()
    assert lib.ide3d_linear_workspace_bytes(4, 25088, 512) == 13 * 4 * 512 * 4
    assert lib.ide3d_linear_workspace_bytes(1, 784, 8) == 8 * 4
    assert lib.ide3d_linear_backward_input_workspace_bytes(3, 3136, 40) == 3 * 3136 * 4 and lib.ide3d_linear_backward_input_workspace_bytes(4, 25088, 512) == 8 * 4 * 25088 * 4
    assert lib.ide3d_linear_workspace_bytes(9, 784, 8) == -1 and lib.ide3d_linear_workspace_bytes(1, 786, 8) == -1 and lib.ide3d_linear_workspace_bytes(1, 784, 0) == -1
    assert lib.ide3d_linear(16, 16, None, 16, 1, 784, 8, 16, 16, None) == -1 and b'workspace' in lib.ide3d_last_error()
    assert lib.ide3d_linear(16, 16, None, 16, 9, 784, 8, 16, 1 << 20, None) == -1
    assert lib.ide3d_linear(16, 20, None, 16, 1, 784, 8, 16, 1 << 20, None) == -1 and b'aligned' in lib.ide3d_last_error()
    assert lib.ide3d_linear_backward_input(16, 16, 16, 1, 786, 8, 16, 1 << 20, None) == -1
    assert lib.ide3d_id_prep(None, 16, 1, 1, None) == -1 and b'null pointer' in lib.ide3d_last_error()
    assert lib.ide3d_id_prep(16, 16, 1, 0, None) == -1 and lib.ide3d_id_prep_backward(16, 16, 0, 1, None) == -1
    assert lib.ide3d_prelu(16, None, 16, 1, 1, 4, 4, None) == -1
    assert lib.ide3d_prelu_backward(16, 32, 16, 3, 16, 16, 16, 1, 2, 4, 4, None) == -1 and b'row pitch' in lib.ide3d_last_error()
    assert lib.ide3d_se_gate(16, 16, 16, 16, 1, 513, 32, None) == -1 and lib.ide3d_se_gate(16, 16, 16, 16, 1, 512, 33, None) == -1
    assert lib.ide3d_se_gate_backward(16, 16, 16, 16, None, 16, 1, 16, 1, None) == -1
    assert lib.ide3d_id_head(16, 16, 16, 16, None, 1, 8, None) == -1 and lib.ide3d_id_head_backward(16, 16, 16, None, 16, 1, 8, None) == -1
