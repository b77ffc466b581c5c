"""C ABI of the fused renderer's backward with the camera gradient (ide3d_render_rays_backward_camera, include/ide3d_hip.h): the ctypes
mirror of ide3d_render_camera_grads, the declarations, EXPORTED_SYMBOLS and the built library's exports, the workspace query (host
arithmetic only), the binding's argument order, and the routing rules of TriplaneRenderer under `triplane.fused_render_camera_grad` that
need no GPU.  No GPU needed."""
import contextlib
import ctypes
import os
import re

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header():
    return re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'ide3d_hip.h')).read(), flags=re.S)


@contextlib.contextmanager
def _switches(camera, params=False):
    from training import triplane
    old = triplane.fused_render_camera_grad, triplane.fused_render_param_grad
    triplane.fused_render_camera_grad, triplane.fused_render_param_grad = camera, params
    try:
        yield
    finally:
        triplane.fused_render_camera_grad, triplane.fused_render_param_grad = old


def test_render_camera_grads_struct_matches_header():
    from torch_utils import hip_plugin
    body = re.search(r'typedef struct ide3d_render_camera_grads \{(.*?)\} ide3d_render_camera_grads;', _header(), re.S).group(1)
    names = [re.search(r'([A-Za-z_][A-Za-z0-9_]*)\s*$', d.strip()).group(1) for d in body.split(';') if d.strip()]
    cls = hip_plugin._RenderCameraGrads
    assert names == [f[0] for f in cls._fields_] == ['grad_cam2world', 'workspace', 'workspace_bytes']
    assert {f[0]: getattr(cls, f[0]).offset for f in cls._fields_} == {'grad_cam2world': 0, 'workspace': 8, 'workspace_bytes': 16}
    assert ctypes.sizeof(cls) == 24
    assert ctypes.sizeof(hip_plugin._RenderGrads) == 104 and ctypes.sizeof(hip_plugin._RenderParamGrads) == 80, 'the older structs keep their layout'


def test_entry_points_are_declared_listed_and_exported():
    from torch_utils import hip_plugin
    h = re.sub(r'\s+', ' ', _header())
    assert re.search(r'int ide3d_render_rays_backward_camera\(const ide3d_render_params\* p, const ide3d_render_grads\* g, '
                     r'const ide3d_render_param_grads\* q, const ide3d_render_camera_grads\* c, void\* stream\);', h)
    assert re.search(r'int64_t ide3d_render_camera_grad_workspace_bytes\(const ide3d_render_params\* p\);', h)
    # the two older entry points keep their signatures
    assert re.search(r'int ide3d_render_rays_backward\(const ide3d_render_params\* p, const ide3d_render_grads\* g, void\* stream\);', h)
    assert re.search(r'int ide3d_render_rays_backward_params\(const ide3d_render_params\* p, const ide3d_render_grads\* g, '
                     r'const ide3d_render_param_grads\* q, void\* stream\);', h)
    assert hip_plugin._ABI_VERSION == 8
    path = hip_plugin.lib_path()
    assert os.path.isfile(path), f'{path} missing: run __graft_entry__.build()'
    lib = ctypes.CDLL(path)
    for name in ('ide3d_render_rays_backward_camera', 'ide3d_render_camera_grad_workspace_bytes'):
        assert name in hip_plugin.EXPORTED_SYMBOLS
        assert hasattr(lib, name)
    assert lib.ide3d_abi_version() == 8


def test_binding_argument_order_matches_the_header():
    from torch_utils import hip_plugin
    lib = hip_plugin.load()
    P = ctypes.POINTER
    assert lib.ide3d_render_rays_backward_camera.argtypes == [P(hip_plugin._RenderParams), P(hip_plugin._RenderGrads), P(hip_plugin._RenderParamGrads),
                                                              P(hip_plugin._RenderCameraGrads), ctypes.c_void_p]
    assert lib.ide3d_render_rays_backward_camera.restype == ctypes.c_int
    assert lib.ide3d_render_camera_grad_workspace_bytes.argtypes == [P(hip_plugin._RenderParams)]
    assert lib.ide3d_render_camera_grad_workspace_bytes.restype == ctypes.c_int64


def _query(lib, C, hid, n=4, rays=4096, steps=96):
    from torch_utils import hip_plugin
    p = hip_plugin._RenderParams()
    p.n, p.rays_per_img, p.steps, p.C, p.hidden, p.feat_ch, p.seg_ch = n, rays, steps, C, hid, 8, 5
    return lib.ide3d_render_camera_grad_workspace_bytes(ctypes.byref(p))


def test_workspace_query():
    """12 floats per image per wave of the launch (8 waves x min(rays / 8, 256) workgroups at the product's 96 steps); 0 where the backward
    has no compiled form or the steps do not fit."""
    from torch_utils import hip_plugin
    lib = hip_plugin.load()
    assert _query(lib, 32, 64) == 2048 * 4 * 12 * 4
    assert _query(lib, 16, 32) == 2048 * 4 * 12 * 4
    assert _query(lib, 32, 64, n=1, rays=24) == 24 * 12 * 4
    assert _query(lib, 16, 32, n=3, rays=144, steps=17) == 432 * 3 * 12 * 4          # 54 workgroups of 8 waves, 3 images
    assert _query(lib, 24, 40) == 0
    assert _query(lib, 32, 64, steps=100000) == 0
    assert lib.ide3d_render_camera_grad_workspace_bytes(None) == 0


def test_nothing_requested_is_an_argument_error():
    from torch_utils import hip_plugin
    lib = hip_plugin.load()
    p, g = hip_plugin._RenderParams(), hip_plugin._RenderGrads()
    assert lib.ide3d_render_rays_backward_camera(ctypes.byref(p), ctypes.byref(g), None, None, None) == -1          # IDE3D_EINVAL
    assert b'no gradient requested' in lib.ide3d_last_error()


def _renderer():
    from training import triplane
    R = triplane.TriplaneRenderer(triplane.tiny_spec())
    R.decoder.requires_grad_(False)
    return R


def test_switch_is_off_by_default():
    from training import triplane
    assert triplane.fused_render_camera_grad is False


def test_cpu_tensors_stay_step_wise_with_the_switch_on():
    R = _renderer()
    cam = torch.eye(4)[None].clone().requires_grad_(True)
    tex, geo = torch.zeros(1, 48, 8, 8), torch.zeros(1, 48, 8, 8)
    for params in (False, True):
        with _switches(True, params):
            assert not R._fused_grad_ok(tex, geo, cam, None, None)
            assert not R._fused_grad_ok(tex.clone().requires_grad_(True), geo, cam, None, None)


def test_rules_on_stand_ins():
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

    def ok(planes=(False, False), params=(False,) * 8, cam=None, jit=None, noise=None):
        r = R()
        r.decoder = Dec([T(g) for g in params])
        return r._fused_grad_ok(T(planes[0]), T(planes[1]), cam or T(), jit, noise)

    one = (False,) * 7 + (True,)
    for params_switch in (False, True):
        with _switches(True, params_switch):
            assert ok(cam=T(True)), 'a camera that requires grad is reason enough'
            assert ok(planes=(True, False), cam=T(True))
            assert ok(planes=(True, False)), 'no camera gradient: as before'
            assert not ok(), 'nothing requires grad'
            assert not ok(cam=T(True), jit=T(True))
            assert not ok(cam=T(True), noise=T(True))
            assert not ok(cam=T(True, dtype=torch.float64))
            assert not ok(cam=T(True, device='cpu'))
            assert ok(cam=T(True), params=one) == params_switch, 'a trainable decoder still needs its own switch'
            with torch.no_grad():
                assert not ok(cam=T(True))
        with _switches(False, params_switch):
            assert not ok(cam=T(True))
            assert not ok(planes=(True, True), cam=T(True)), 'switch off: a camera that requires grad stays step-wise'
            assert ok(planes=(True, False))


def test_camera_label_reaches_the_renderer_with_its_graph():
    """G.synthesis derives cam2world from c with tensor ops: a c that requires grad gets a gradient on its 12 pose entries (CPU, step-wise)."""
    from training import triplane
    torch.manual_seed(0)
    G = triplane.TriPlaneGenerator(triplane.tiny_spec()).eval().requires_grad_(False)
    seen = {}
    G.synthesis.renderer.register_forward_pre_hook(lambda m, args: seen.update(cam=args[2]))
    c = triplane.camera_label(0.2).clone().requires_grad_(True)
    with torch.no_grad():
        ws = G.mapping(torch.randn(1, G.z_dim), triplane.conditioning_label())
    img = G.synthesis(ws, c=c, noise_mode='const')
    assert seen['cam'].requires_grad and seen['cam'].dtype == torch.float32 and seen['cam'].shape == (1, 4, 4)
    (gc,) = torch.autograd.grad(img.square().sum(), [c])
    assert float(gc[:, :12].abs().max()) > 0 and float(gc[:, 12:].abs().max()) == 0
