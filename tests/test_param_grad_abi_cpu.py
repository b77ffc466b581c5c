"""C ABI of the parameter gradients of the synthesis convolutions (ide3d_modconv_weight_grad, ide3d_bias_noise_grad in csrc/modconv_bwd.hip,
include/ide3d_hip.h): declarations, EXPORTED_SYMBOLS, the built library's exports, the ctypes mirror of ide3d_wgrad_params, the workspace
queries; and the routing switch of training/networks.py, which needs no GPU."""
import ctypes
import os
import re

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NEW_SYMBOLS = ('ide3d_wgrad_workspace_bytes', 'ide3d_modconv_weight_grad', 'ide3d_bias_noise_workspace_bytes', 'ide3d_bias_noise_grad')


def _header():
    return re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'ide3d_hip.h')).read(), flags=re.S)


def test_entry_points_declared_listed_and_exported():
    from torch_utils import hip_plugin
    h = _header()
    assert re.search(r'int64_t ide3d_wgrad_workspace_bytes\(int32_t n, int32_t cin, int32_t cout, int32_t h, int32_t w\);', h)
    assert re.search(r'int ide3d_modconv_weight_grad\(const ide3d_wgrad_params\* p, void\* stream\);', h)
    assert re.search(r'int64_t ide3d_bias_noise_workspace_bytes\(int32_t n, int32_t c, int32_t h, int32_t w\);', h)
    assert re.search(r'int ide3d_bias_noise_grad\(const float\* dz, float\* db, float\* dnoise, int32_t n, int32_t c, int32_t h, int32_t w,\s*'
                     r'float\* workspace, int64_t workspace_bytes, void\* stream\);', h)
    lib = ctypes.CDLL(hip_plugin.lib_path())
    for name in NEW_SYMBOLS:
        assert name in hip_plugin.EXPORTED_SYMBOLS
        assert hasattr(lib, name), name
    assert hip_plugin._ABI_VERSION == 8
    assert ctypes.sizeof(hip_plugin._ActBwdParams) == 120


def test_wgrad_params_struct_matches_header():
    from torch_utils import hip_plugin
    body = re.search(r'typedef struct ide3d_wgrad_params \{(.*?)\} ide3d_wgrad_params;', _header(), re.S).group(1)
    names = []
    for decl in body.split(';'):
        decl = decl.strip()
        if decl:
            names += [re.search(r'([A-Za-z_][A-Za-z0-9_]*)\s*$', part).group(1) for part in decl.split(',')]
    cls = hip_plugin._WgradParams
    assert names == [f[0] for f in cls._fields_]
    offsets = {f[0]: getattr(cls, f[0]).offset for f in cls._fields_}
    assert offsets == {'g': 0, 'x': 8, 'styles': 16, 'dcoefs': 24, 'dw': 32, 'n': 40, 'cin': 44, 'cout': 48, 'h': 52, 'w': 56,
                       'mode': 60, 'arith': 64, 'workspace': 72, 'workspace_bytes': 80}
    assert ctypes.sizeof(cls) == 88


def test_workspace_sizes_without_gpu():
    from torch_utils import hip_plugin
    lib = hip_plugin.load()
    # one pixel split: 512 x 512 at 4^2 (576 tiles x taps fill the device already)
    assert lib.ide3d_wgrad_workspace_bytes(1, 512, 512, 4, 4) == 1 * 1 * 512 * 512 * 9 * 4
    # several splits per image at 512^2: at least 512 pixels per split, a whole number of splits
    b = lib.ide3d_wgrad_workspace_bytes(2, 64, 64, 512, 512)
    per_slice = 64 * 64 * 9 * 4
    assert b % per_slice == 0 and 2 * 2 <= b // per_slice <= 2 * 256
    assert lib.ide3d_wgrad_workspace_bytes(1, 8, 8, 0, 4) < 0
    assert lib.ide3d_wgrad_workspace_bytes(0, 8, 8, 4, 4) < 0
    # bias / noise: per plane 4 partials per 1024-pixel block, per 32-plane group one noise row
    assert lib.ide3d_bias_noise_workspace_bytes(2, 64, 32, 32) == (2 * 64 * 1 * 4 + 4 * 1024) * 4
    assert lib.ide3d_bias_noise_workspace_bytes(1, 3, 0, 4) < 0


def test_switch_exists_off_and_cpu_never_takes_the_path():
    from training import networks
    assert networks.hip_param_grad is False
    torch.manual_seed(0)
    lay = networks.SynthesisLayer(8, 8, w_dim=4, resolution=8)
    x = torch.randn(1, 8, 8, 8)
    w = torch.randn(1, 4)
    old = networks.hip_param_grad
    networks.hip_param_grad = True
    try:
        styles = lay.affine(w)
        assert not networks._conv_grad_ok(x, styles, *networks._layer_params(lay))
        assert networks._synthesis_layer_grad(lay, x, styles, None, None, lay.act_gain, None) is None
        y = lay(x, w, noise_mode='const')
        assert y.grad_fn is not None and 'Modconv' not in type(y.grad_fn).__name__
        y.square().sum().backward()
        assert lay.weight.grad is not None and lay.bias.grad is not None and lay.noise_strength.grad is not None
        tr = networks.ToRGBLayer(8, 3, w_dim=4)
        ts = networks.ToRGBLayer(8, 5, w_dim=4)
        assert networks._dual_head(x, tr, ts, w) is None
    finally:
        networks.hip_param_grad = old
