"""C ABI of the trainable plain convolutions: mode 1 of ide3d_modconv_weight_grad (csrc/modconv_bwd.hip) and
ide3d_linear_weight_grad (csrc/linear_wgrad.hip) and ide3d_residual_join (csrc/res_join.hip): declarations, EXPORTED_SYMBOLS, the built library's exports, the host-side argument checks
(which return before anything is launched, so they need no GPU), the unchanged workspace query; and the routing switch of
training/networks.py."""
import ctypes
import os
import re

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -1


def _header():
    return re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'ide3d_hip.h')).read(), flags=re.S)


def test_entry_points_declared_listed_and_exported():
    from torch_utils import hip_plugin
    h = _header()
    assert re.search(r'int ide3d_linear_weight_grad\(const float\* dy, const float\* x, float\* dw, int32_t n, int32_t K, int32_t M, void\* stream\);', h)
    assert re.search(r'int64_t ide3d_wgrad_workspace_bytes\(int32_t n, int32_t cin, int32_t cout, int32_t h, int32_t w\);', h)
    lib = hip_plugin.load()
    assert re.search(r'int ide3d_residual_join\(const float\* a, const float\* b, float\* out, int64_t count, float gain, void\* stream\);', h)
    for name in ('ide3d_linear_weight_grad', 'ide3d_residual_join', 'ide3d_modconv_weight_grad', 'ide3d_wgrad_workspace_bytes'):
        assert name in hip_plugin.EXPORTED_SYMBOLS
        assert hasattr(lib, name), name
    assert len(re.findall(r'\bide3d_linear_weight_grad\(', h)) == 1
    assert hip_plugin._ABI_VERSION == 8 and lib.ide3d_abi_version() == 8
    assert hasattr(hip_plugin.IdLossPlugin, 'linear_weight_grad') and hasattr(hip_plugin.IdLossPlugin, 'residual_join')


def _wgrad_params(hip_plugin, mode, n, cin, cout, h, w, ws_bytes, null=()):
    """Params whose pointers are never dereferenced on the host: the checks under test return before the launch."""
    dummy = ctypes.create_string_buffer(64)
    p = hip_plugin._WgradParams()
    for name in ('g', 'x', 'dw', 'workspace'):
        setattr(p, name, None if name in null else ctypes.addressof(dummy))
    p.n, p.cin, p.cout, p.h, p.w, p.mode, p.arith = n, cin, cout, h, w, mode, 1
    p.workspace_bytes = ws_bytes
    return p, dummy


def test_mode_1_host_checks_return_einval_without_a_gpu():
    from torch_utils import hip_plugin
    lib = hip_plugin.load()
    need = lib.ide3d_wgrad_workspace_bytes(2, 24, 40, 4, 3)          # the grid of g for an x of 9 x 7
    assert need == 2 * 1 * 40 * 24 * 9 * 4
    for null in ('g', 'x', 'dw', 'workspace'):
        p, keep = _wgrad_params(hip_plugin, 1, 2, 24, 40, 9, 7, need, null=(null,))
        assert lib.ide3d_modconv_weight_grad(ctypes.byref(p), None) == EINVAL, null
    p, keep = _wgrad_params(hip_plugin, 1, 2, 24, 40, 9, 7, need - 4)
    assert lib.ide3d_modconv_weight_grad(ctypes.byref(p), None) == EINVAL
    assert b'workspace too small' in lib.ide3d_last_error()
    # an x smaller than the 3 x 3 window, a mode that does not exist
    for mode, h, w in ((1, 2, 7), (1, 9, 2), (3, 9, 7)):
        p, keep = _wgrad_params(hip_plugin, mode, 2, 24, 40, h, w, 1 << 30)
        assert lib.ide3d_modconv_weight_grad(ctypes.byref(p), None) == EINVAL, (mode, h, w)
    # sizes whose element counts leave 32 (and 64) bits are refused, not wrapped
    p, keep = _wgrad_params(hip_plugin, 1, 2, 24, 40, 2 ** 31 - 1, 2 ** 31 - 1, 2 ** 62)
    assert lib.ide3d_modconv_weight_grad(ctypes.byref(p), None) == EINVAL
    assert lib.ide3d_wgrad_workspace_bytes(2, 24, 40, 2 ** 31 - 1, 2 ** 31 - 1) < 0
    assert lib.ide3d_modconv_weight_grad(None, None) == EINVAL


def test_linear_weight_grad_host_checks_return_einval_without_a_gpu():
    from torch_utils import hip_plugin
    lib = hip_plugin.load()
    buf = ctypes.create_string_buffer(256)
    a = (ctypes.addressof(buf) + 15) & ~15
    vp = ctypes.c_void_p
    assert lib.ide3d_linear_weight_grad(vp(a), vp(a), vp(a), 9, 8, 5, None) == EINVAL        # n > 8
    assert lib.ide3d_linear_weight_grad(vp(a), vp(a), vp(a), 1, 6, 5, None) == EINVAL        # K % 4 != 0
    assert lib.ide3d_linear_weight_grad(vp(a), vp(a), vp(a), 0, 8, 5, None) == EINVAL
    assert lib.ide3d_linear_weight_grad(vp(a), vp(a), vp(a), 1, 8, 0, None) == EINVAL
    assert lib.ide3d_linear_weight_grad(None, vp(a), vp(a), 1, 8, 5, None) == EINVAL
    assert lib.ide3d_linear_weight_grad(vp(a), None, vp(a), 1, 8, 5, None) == EINVAL
    assert lib.ide3d_linear_weight_grad(vp(a), vp(a), None, 1, 8, 5, None) == EINVAL
    assert lib.ide3d_linear_weight_grad(vp(a), vp(a + 4), vp(a), 1, 8, 5, None) == EINVAL    # x not 16-byte aligned
    assert lib.ide3d_linear_weight_grad(vp(a), vp(a), vp(a + 8), 1, 8, 5, None) == EINVAL    # dw not 16-byte aligned


def test_residual_join_host_checks_return_einval_without_a_gpu():
    from torch_utils import hip_plugin
    lib = hip_plugin.load()
    buf = ctypes.create_string_buffer(256)
    a = (ctypes.addressof(buf) + 15) & ~15
    vp, f = ctypes.c_void_p, ctypes.c_float
    assert lib.ide3d_residual_join(None, vp(a), vp(a + 64), 4, f(1.0), None) == EINVAL
    assert lib.ide3d_residual_join(vp(a), vp(a + 32), None, 4, f(1.0), None) == EINVAL
    assert lib.ide3d_residual_join(vp(a), None, vp(a + 64), 0, f(1.0), None) == EINVAL
    assert lib.ide3d_residual_join(vp(a), None, vp(a + 64), 2 ** 40, f(1.0), None) == EINVAL
    assert lib.ide3d_residual_join(vp(a + 2), None, vp(a + 64), 4, f(1.0), None) == EINVAL     # not a float's address
    assert lib.ide3d_residual_join(vp(a), vp(a + 33), vp(a + 64), 4, f(1.0), None) == EINVAL


def test_projector_gate_mirrors_the_entry_points_limits():
    from training import encoders
    lib = __import__('torch_utils.hip_plugin', fromlist=['load']).load()
    for n, K, M in ((1, 8192, 512), (8, 8192, 5120), (9, 8192, 512), (0, 8, 4), (1, 6, 4), (1, 2 ** 24 + 4, 4), (1, 8, 65535 * 8 + 1), (1, 2 ** 24, 2 ** 17)):
        covered = lib.ide3d_linear_workspace_bytes(n, K, M) >= 0 and lib.ide3d_linear_backward_input_workspace_bytes(n, K, M) >= 0
        assert encoders._linear_covers(n, K, M) == covered, (n, K, M)


def _wgrad_bytes(n, cin, cout, h, w):
    """The workspace query as it was before mode 1 (csrc/modconv_bwd.hip, wt_geom), restated."""
    cdiv = lambda a, b: -(-a // b)
    kpix = h * w
    s = max(1, min(cdiv(2048, n * 9 * cdiv(cout, 64) * cdiv(cin, 64)), cdiv(kpix, 512), 256))
    per = cdiv(cdiv(kpix, s), 32) * 32
    return n * cdiv(kpix, per) * cout * cin * 9 * 4


def test_workspace_query_is_unchanged_for_modes_0_and_2():
    from torch_utils import hip_plugin
    lib = hip_plugin.load()
    assert lib.ide3d_wgrad_workspace_bytes(1, 512, 512, 4, 4) == 1 * 1 * 512 * 512 * 9 * 4
    b = lib.ide3d_wgrad_workspace_bytes(2, 64, 64, 512, 512)
    assert b % (64 * 64 * 9 * 4) == 0 and 2 * 2 <= b // (64 * 64 * 9 * 4) <= 2 * 256
    assert lib.ide3d_wgrad_workspace_bytes(1, 8, 8, 0, 4) < 0
    assert lib.ide3d_wgrad_workspace_bytes(0, 8, 8, 4, 4) < 0
    for args in ((1, 512, 512, 4, 4), (2, 64, 64, 512, 512), (4, 512, 512, 16, 16), (1, 32, 32, 256, 256), (2, 24, 40, 9, 7), (3, 3, 32, 65, 65),
                 (8, 128, 256, 64, 64), (1, 64, 64, 1, 1)):
        assert lib.ide3d_wgrad_workspace_bytes(*args) == _wgrad_bytes(*args), args


def test_switch_exists_off_and_cpu_never_takes_the_path():
    from training import encoders, networks
    assert networks.hip_plain_conv_grad is False
    torch.manual_seed(0)
    blk = encoders.EncoderResBlock(8, 8)
    proj = encoders.EqualConv2d(8, 4, 4, padding=0, bias=False)
    x = torch.randn(2, 8, 8, 8, requires_grad=True)
    networks.hip_plain_conv_grad = True
    try:
        for lay in (blk.conv1, blk.conv2, blk.skip):
            assert networks._plain_conv_form(lay, x) is None
        y = proj(blk(x))
        assert 'PlainConvGrad' not in type(y.grad_fn).__name__ and 'ProjectorGrad' not in type(y.grad_fn).__name__
        y.square().sum().backward()
        assert x.grad is not None and all(p.grad is not None for p in list(blk.parameters()) + list(proj.parameters()))
    finally:
        networks.hip_plain_conv_grad = False
