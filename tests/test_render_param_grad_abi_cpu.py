"""C ABI of the fused renderer's backward with decoder-parameter gradients (ide3d_render_rays_backward_params, include/ide3d_hip.h): the
ctypes mirror of ide3d_render_param_grads, the declarations, EXPORTED_SYMBOLS and the built library's exports, the workspace query (host
arithmetic only), and the routing rules of TriplaneRenderer under `triplane.fused_render_param_grad` that need no GPU.  No GPU needed."""
import contextlib
import ctypes
import os
import re

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header():
    return re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'ide3d_hip.h')).read(), flags=re.S)


@contextlib.contextmanager
def _switch(on):
    from training import triplane
    old = triplane.fused_render_param_grad
    triplane.fused_render_param_grad = on
    try:
        yield
    finally:
        triplane.fused_render_param_grad = old


def test_render_param_grads_struct_matches_header():
    from torch_utils import hip_plugin
    body = re.search(r'typedef struct ide3d_render_param_grads \{(.*?)\} ide3d_render_param_grads;', _header(), re.S).group(1)
    names = []
    for decl in body.split(';'):
        decl = decl.strip()
        if decl:
            names.append(re.search(r'([A-Za-z_][A-Za-z0-9_]*)\s*$', decl).group(1))
    cls = hip_plugin._RenderParamGrads
    assert names == [f[0] for f in cls._fields_]
    offsets = {f[0]: getattr(cls, f[0]).offset for f in cls._fields_}
    assert offsets == {'grad_geo_w0': 0, 'grad_geo_b0': 8, 'grad_geo_w1': 16, 'grad_geo_b1': 24, 'grad_tex_w0': 32, 'grad_tex_b0': 40,
                       'grad_tex_w1': 48, 'grad_tex_b1': 56, 'workspace': 64, 'workspace_bytes': 72}
    assert ctypes.sizeof(cls) == 80
    assert ctypes.sizeof(hip_plugin._RenderGrads) == 104, 'ide3d_render_grads keeps its layout'


def test_entry_points_are_declared_listed_and_exported():
    from torch_utils import hip_plugin
    h = _header()
    assert re.search(r'int ide3d_render_rays_backward_params\(const ide3d_render_params\* p, const ide3d_render_grads\* g, '
                     r'const ide3d_render_param_grads\* q, void\* stream\);', h)
    assert re.search(r'int64_t ide3d_render_param_grad_workspace_bytes\(const ide3d_render_params\* p\);', h)
    assert hip_plugin._ABI_VERSION == 8
    path = hip_plugin.lib_path()
    assert os.path.isfile(path), f'{path} missing: run __graft_entry__.build()'
    lib = ctypes.CDLL(path)
    for name in ('ide3d_render_rays_backward_params', 'ide3d_render_param_grad_workspace_bytes'):
        assert name in hip_plugin.EXPORTED_SYMBOLS
        assert hasattr(lib, name)
    assert lib.ide3d_abi_version() == 8


def test_workspace_query():
    """One slice per wave of the launch (8 waves x min(rays / 8, 256) workgroups at the product's 96 steps), each the eight tensors' sizes
    rounded up to 16 bytes; 0 where there is no compiled form."""
    from torch_utils import hip_plugin
    lib = ctypes.CDLL(hip_plugin.lib_path())
    fn = lib.ide3d_render_param_grad_workspace_bytes
    fn.restype, fn.argtypes = ctypes.c_int64, [ctypes.POINTER(hip_plugin._RenderParams)]

    def query(C, hid, feat, seg, n=4, rays=4096, steps=96):
        p = hip_plugin._RenderParams()
        p.n, p.rays_per_img, p.steps, p.C, p.hidden, p.feat_ch, p.seg_ch = n, rays, steps, C, hid, feat, seg
        return fn(ctypes.byref(p))

    def slice_floats(C, hid, feat, seg):
        total = 2 * hid * C + 2 * hid + (1 + seg + feat) * (hid + 1)
        return (total + 3) // 4 * 4

    assert query(32, 64, 32, 19) == 2048 * slice_floats(32, 64, 32, 19) * 4
    assert query(16, 32, 8, 5) == 2048 * slice_floats(16, 32, 8, 5) * 4
    assert query(32, 64, 32, 19, n=1, rays=24) == 24 * slice_floats(32, 64, 32, 19) * 4          # 3 workgroups of 8 waves
    assert query(24, 40, 8, 5) == 0
    assert query(32, 64, 32, 19, steps=100000) == 0


def _renderer(trainable):
    from training import triplane
    R = triplane.TriplaneRenderer(triplane.tiny_spec())
    R.decoder.requires_grad_(trainable)
    return R


def test_switch_is_off_by_default_and_then_a_trainable_decoder_is_refused():
    from training import triplane
    assert triplane.fused_render_param_grad is False
    R = _renderer(True)
    tex = torch.zeros(1, 48, 8, 8, requires_grad=True)
    geo = torch.zeros(1, 48, 8, 8)
    cam = torch.eye(4)[None]
    assert not R._fused_grad_ok(tex, geo, cam, None, None)


def test_cpu_tensors_never_take_the_fused_path_with_the_switch_on():
    cam = torch.eye(4)[None]
    with _switch(True):
        for trainable in (True, False):
            R = _renderer(trainable)
            tex = torch.zeros(1, 48, 8, 8, requires_grad=True)
            geo = torch.zeros(1, 48, 8, 8)
            assert not R._fused_grad_ok(tex, geo, cam, None, None)
            assert not R._fused_grad_ok(tex.detach(), geo, cam, None, None)


def test_rules_with_the_switch_on():
    """The rule itself, on stand-ins for CUDA tensors (only device type, dtype and requires_grad are read)."""
    class T:
        def __init__(self, requires_grad=False, device='cuda', dtype=torch.float32):
            self.requires_grad, self.device, self.dtype = requires_grad, torch.device(device), dtype

    class Dec:
        def __init__(self, ps):
            self.ps = ps

        def parameters(self):
            return iter(self.ps)

    from training import triplane

    class R:
        _fused_grad_ok = triplane.TriplaneRenderer._fused_grad_ok
        _fused_param_grad_ok = triplane.TriplaneRenderer._fused_param_grad_ok

    def ok(planes=(False, False), params=(False,) * 8, cam=T(), jit=None, noise=None, pdev='cuda', pdtype=torch.float32):
        r = R()
        r.decoder = Dec([T(g, pdev, pdtype) for g in params])
        return r._fused_grad_ok(T(planes[0]), T(planes[1]), cam, jit, noise)

    one = (False,) * 7 + (True,)
    with _switch(True):
        assert ok(planes=(True, False))
        assert ok(params=one), 'one trainable decoder parameter and detached planes'
        assert ok(planes=(True, True), params=(True,) * 8)
        assert not ok(), 'nothing requires grad'
        assert not ok(params=one, cam=T(True))
        assert not ok(params=one, jit=T(True))
        assert not ok(params=one, noise=T(True))
        assert not ok(params=one, pdev='cpu')
        assert not ok(params=one, pdtype=torch.float64)
        with torch.no_grad():
            assert not ok(params=one)
    with _switch(False):
        assert ok(planes=(True, False))
        assert not ok(params=one)
        assert not ok(planes=(True, True), params=one), 'switch off: a trainable decoder stays step-wise'
