"""C ABI of the frozen-generator convolution backward (csrc/modconv_bwd.hip, include/ide3d_hip.h): declarations, EXPORTED_SYMBOLS, the built
library's exports, the ctypes mirror of ide3d_act_bwd_params; and the routing rules of training/networks.py that need no GPU."""
import ctypes
import os
import re

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NEW_SYMBOLS = ('ide3d_act_bwd_workspace_bytes', 'ide3d_modconv_act_backward', 'ide3d_modconv_scale_dot', 'ide3d_head_wgrad_workspace_bytes',
               'ide3d_head_weight_grad')


def _header():
    return re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'ide3d_hip.h')).read(), flags=re.S)


def test_entry_points_declared_listed_and_exported():
    from torch_utils import hip_plugin
    h = _header()
    assert re.search(r'int64_t ide3d_act_bwd_workspace_bytes\(int32_t n, int32_t c, int32_t h, int32_t w\);', h)
    assert re.search(r'int ide3d_modconv_act_backward\(const ide3d_act_bwd_params\* p, void\* stream\);', h)
    assert re.search(r'int ide3d_modconv_scale_dot\(const float\* x, const float\* t, const float\* styles, float\* dx, float\* dstyles,\s*'
                     r'int32_t n, int32_t c, int32_t h, int32_t w, float\* workspace, int64_t workspace_bytes, void\* stream\);', h)
    assert re.search(r'int64_t ide3d_head_wgrad_workspace_bytes\(int32_t n, int32_t rows, int32_t cin, int32_t h, int32_t w\);', h)
    assert re.search(r'int ide3d_head_weight_grad\(const float\* dy, const float\* x, float\* dw, int32_t n, int32_t rows, int32_t cin, '
                     r'int32_t h, int32_t w,\s*float\* workspace, int64_t workspace_bytes, void\* stream\);', h)
    path = hip_plugin.lib_path()
    assert os.path.isfile(path), f'{path} missing: run __graft_entry__.build()'
    lib = ctypes.CDLL(path)
    for name in NEW_SYMBOLS:
        assert name in hip_plugin.EXPORTED_SYMBOLS
        assert hasattr(lib, name), name
    assert hip_plugin._ABI_VERSION == 8


def test_act_bwd_params_struct_matches_header():
    from torch_utils import hip_plugin
    body = re.search(r'typedef struct ide3d_act_bwd_params \{(.*?)\} ide3d_act_bwd_params;', _header(), re.S).group(1)
    names = []
    for decl in body.split(';'):
        decl = decl.strip()
        if decl:
            names += [re.search(r'([A-Za-z_][A-Za-z0-9_]*)\s*$', part).group(1) for part in decl.split(',')]
    cls = hip_plugin._ActBwdParams
    assert names == [f[0] for f in cls._fields_]
    offsets = {f[0]: getattr(cls, f[0]).offset for f in cls._fields_}
    assert offsets == {'dy': 0, 'y': 8, 'dz': 16, 'noise': 24, 'noise_strength': 32, 'bias': 40, 'dcoefs': 48, 'ddcoefs': 56,
                       'n': 64, 'c': 68, 'h': 72, 'w': 76, 'y_pitch': 80, 'act': 84, 'alpha': 88, 'gain': 92, 'clamp': 96,
                       'workspace': 104, 'workspace_bytes': 112}
    assert ctypes.sizeof(cls) == 120


def test_workspace_sizes_without_gpu():
    from torch_utils import hip_plugin
    lib = hip_plugin.load()
    assert lib.ide3d_act_bwd_workspace_bytes(2, 3, 64, 64) == 2 * 3 * 1 * 4
    assert lib.ide3d_act_bwd_workspace_bytes(1, 4, 256, 256) == 4 * 16 * 4
    assert lib.ide3d_act_bwd_workspace_bytes(0, 4, 8, 8) < 0
    assert lib.ide3d_head_wgrad_workspace_bytes(1, 192, 128, 4, 4) == 1 * 1 * 192 * 128 * 4
    assert lib.ide3d_head_wgrad_workspace_bytes(1, 22, 64, 0, 4) < 0


def test_switch_and_cpu_routing():
    """The module switch exists and is on; CPU tensors never take the new path (layers and heads keep the ATen definition)."""
    from training import networks
    assert networks.hip_conv_grad is True
    torch.manual_seed(0)
    lay = networks.SynthesisLayer(8, 8, w_dim=4, resolution=8).requires_grad_(False)
    x = torch.randn(1, 8, 8, 8, requires_grad=True)
    w = torch.randn(1, 4, requires_grad=True)
    styles = lay.affine(w)
    assert not networks._conv_grad_ok(x, styles, *networks._layer_params(lay))
    assert networks._synthesis_layer_grad(lay, x, styles, None, None, lay.act_gain, None) is None
    y = lay(x, w, noise_mode='const')
    assert y.grad_fn is not None and 'ModconvActGrad' not in type(y.grad_fn).__name__
    y.sum().backward()
    assert x.grad is not None and w.grad is not None
    tr = networks.ToRGBLayer(8, 3, w_dim=4).requires_grad_(False)
    ts = networks.ToRGBLayer(8, 5, w_dim=4).requires_grad_(False)
    assert networks._dual_head(x, tr, ts, w) is None
