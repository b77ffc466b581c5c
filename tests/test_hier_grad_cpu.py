"""The merged march's backward (`ide3d_render_rays_merged_backward`), what can be checked without a GPU: the C
boundary of the two new entry points, their host-side argument rules and workspace query, the routing of `TriplaneRenderer.forward` under
`triplane.fused_hierarchical_grad`, and the float64 reference of tests/hier_grad_ref.py against central differences."""

import ctypes
import os
import re

import numpy as np
import torch

import hier_grad_ref
import hier_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ('ide3d_render_merged_param_grad_workspace_bytes', 'ide3d_render_rays_merged_backward')
EINVAL, ENOKERNEL = -1, -2


def _lib():
    from torch_utils import hip_plugin
    path = hip_plugin.lib_path()
    assert os.path.isfile(path), f'{path} missing: run __graft_entry__.build()'
    lib = ctypes.CDLL(path)
    vp, i32 = ctypes.c_void_p, ctypes.c_int32
    P = ctypes.POINTER(hip_plugin._RenderParams)
    lib.ide3d_render_rays_merged_backward.argtypes = [P, vp, vp, vp, i32, ctypes.POINTER(hip_plugin._RenderGrads),
                                                      ctypes.POINTER(hip_plugin._RenderParamGrads), vp]
    lib.ide3d_render_rays_merged_backward.restype = ctypes.c_int
    for name in ('ide3d_render_merged_param_grad_workspace_bytes', 'ide3d_render_param_grad_workspace_bytes'):
        getattr(lib, name).argtypes = [P]
        getattr(lib, name).restype = ctypes.c_int64
    lib.ide3d_last_error.restype = ctypes.c_char_p
    return lib


def test_entry_points_declared_listed_exported_and_workspace_query():
    """Both symbols in the header, in EXPORTED_SYMBOLS, in the plugin's prototypes and in the built library.  The workspace query is host
    arithmetic: 0 without a compiled (C, hidden) form or outside 3 .. 1024 steps, else one slice per wave of the launch planned for
    T = 2 * steps samples, i.e. what the plain query answers for 2 * steps.  (The slice count is waves per workgroup x workgroups, capped by
    the chip, so the byte count follows the launch plan of T; it is not monotonic in the step count.)"""
    from torch_utils import hip_plugin
    h = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'ide3d_hip.h')).read(), flags=re.S)
    assert re.search(r'int64_t ide3d_render_merged_param_grad_workspace_bytes\(const ide3d_render_params\* p\);', h)
    assert re.search(r'int ide3d_render_rays_merged_backward\(const ide3d_render_params\* p, const float\* z_all, const int32_t\* src, '
                     r'const float\* z_fine,\s*int32_t total_steps, const ide3d_render_grads\* g, const ide3d_render_param_grads\* q, '
                     r'void\* stream\);', h)
    assert hip_plugin._ABI_VERSION == 8
    lib = _lib()
    for name in NEW:
        assert name in hip_plugin.EXPORTED_SYMBOLS
        assert hasattr(lib, name), f'{name} not exported'
    assert lib.ide3d_abi_version() == 8
    assert callable(hip_plugin.VolumeRenderPlugin.render_rays_merged_backward)

    def query(fn, C, hid, feat, seg, n=4, rays=4096, steps=96):
        p = hip_plugin._RenderParams()
        p.n, p.rays_per_img, p.steps, p.C, p.hidden, p.feat_ch, p.seg_ch = n, rays, steps, C, hid, feat, seg
        return fn(ctypes.byref(p))

    merged, plain = lib.ide3d_render_merged_param_grad_workspace_bytes, lib.ide3d_render_param_grad_workspace_bytes
    assert merged(None) == 0
    assert query(merged, 24, 40, 8, 5) == 0, 'no compiled form'
    assert query(merged, 8, 16, 4, 2) == 0, 'no compiled form'
    for steps in (2, 1025, 0):
        assert query(merged, 32, 64, 32, 19, steps=steps) == 0, 'outside the hierarchical pass\'s step range'
    for form in ((32, 64, 32, 19), (16, 32, 8, 5)):
        for n, rays in ((4, 4096), (1, 20)):
            for steps in (3, 48, 96, 512, 1024):
                got = query(merged, *form, n=n, rays=rays, steps=steps)
                assert got > 0 and got % 16 == 0
                assert got == query(plain, *form, n=n, rays=rays, steps=2 * steps), (form, n, rays, steps)
    # sized by 2 * steps, not by steps: 20 rays at 96 steps run 8 waves per workgroup in the plain march (24 slices), 4 in the merged one (20)
    assert query(merged, 32, 64, 32, 19, n=1, rays=20, steps=96) != query(plain, 32, 64, 32, 19, n=1, rays=20, steps=96)


def _params(hip_plugin, backing, steps=12, C=16, hidden=32, last_back=0, channels_last=True):
    """An ide3d_render_params whose pointers all name `backing` (16-byte aligned host memory: nothing here may reach a launch)."""
    p = hip_plugin._RenderParams()
    addr = backing.ctypes.data
    assert addr % 16 == 0
    for f in ('rays_d_cam', 'z_lin', 'cam2world', 'tex_planes', 'geo_planes', *hip_plugin.VolumeRenderPlugin.MLP_KEYS):
        setattr(p, f, addr)
    H = W = 8
    strides = (3 * C * H * W, 1, W * 3 * C, 3 * C) if channels_last else (3 * C * H * W, H * W, W, 1)
    p.tex_stride = p.geo_stride = (ctypes.c_int64 * 4)(*strides)
    p.n, p.rays_per_img, p.steps = 1, 4, steps
    p.C, p.H, p.W, p.hidden, p.feat_ch, p.seg_ch = C, H, W, hidden, 4, 2
    p.clamp_mode, p.last_back = 0, last_back
    return p


def _grads(hip_plugin, backing, C=16, channels_last=True, planes=True):
    g = hip_plugin._RenderGrads()
    if planes:
        g.grad_tex_planes = g.grad_geo_planes = backing.ctypes.data
    H = W = 8
    strides = (3 * C * H * W, 1, W * 3 * C, 3 * C) if channels_last else (3 * C * H * W, H * W, W, 1)
    g.grad_tex_stride = g.grad_geo_stride = (ctypes.c_int64 * 4)(*strides)
    return g


def test_host_side_argument_checks():
    """Null pointers and a total_steps other than 2 * steps are IDE3D_EINVAL; steps outside 3 .. 1024, last_back, planes or gradient buffers
    that are not channels_last and a (C, hidden) pair without a compiled form are IDE3D_ENOKERNEL with an error text: all decided on the
    host, before any device call (this test runs without a GPU)."""
    from torch_utils import hip_plugin
    lib = _lib()
    fn = lib.ide3d_render_rays_merged_backward
    buf = np.zeros(4096 + 16, dtype=np.uint8)
    off = (-buf.ctypes.data) % 16
    backing = buf[off:off + 4096]
    a = backing.ctypes.data
    ok, g = _params(hip_plugin, backing), _grads(hip_plugin, backing)
    assert fn(None, a, a, a, 24, ctypes.byref(g), None, None) == EINVAL
    assert fn(ctypes.byref(ok), a, a, a, 24, None, None, None) == EINVAL
    for args in ((None, a, a), (a, None, a), (a, a, None)):
        assert fn(ctypes.byref(ok), *args, 24, ctypes.byref(g), None, None) == EINVAL
    assert fn(ctypes.byref(ok), a, a, a, 23, ctypes.byref(g), None, None) == EINVAL, 'total_steps must be 2 * steps'
    assert fn(ctypes.byref(ok), a, a, a, 12, ctypes.byref(g), None, None) == EINVAL
    bad = _params(hip_plugin, backing)
    bad.geo_w1 = None
    assert fn(ctypes.byref(bad), a, a, a, 24, ctypes.byref(g), None, None) == EINVAL
    bad = _params(hip_plugin, backing)
    bad.z_lin = None
    assert fn(ctypes.byref(bad), a, a, a, 24, ctypes.byref(g), None, None) == EINVAL
    # planes only: both plane gradient buffers are required
    none = _grads(hip_plugin, backing, planes=False)
    assert fn(ctypes.byref(ok), a, a, a, 24, ctypes.byref(none), None, None) == EINVAL
    # with q: its eight outputs are required
    q = hip_plugin._RenderParamGrads()
    assert fn(ctypes.byref(ok), a, a, a, 24, ctypes.byref(g), ctypes.byref(q), None) == EINVAL
    # declines, each with a text that names the entry point
    for kw in (dict(steps=2), dict(steps=1025), dict(last_back=1), dict(channels_last=False), dict(C=8, hidden=16)):
        p = _params(hip_plugin, backing, **kw)
        assert fn(ctypes.byref(p), a, a, a, 2 * p.steps, ctypes.byref(_grads(hip_plugin, backing, C=p.C)), None, None) == ENOKERNEL, kw
        assert b'render_rays_merged_backward' in lib.ide3d_last_error(), kw
    nchw = _grads(hip_plugin, backing, channels_last=False)
    assert fn(ctypes.byref(ok), a, a, a, 24, ctypes.byref(nchw), None, None) == ENOKERNEL
    assert b'channels_last' in lib.ide3d_last_error()
    p = _params(hip_plugin, backing, steps=1025)
    assert fn(ctypes.byref(p), a, a, a, 2050, ctypes.byref(g), None, None) == ENOKERNEL
    assert b'1025' in lib.ide3d_last_error()


# ---- routing ------------------------------------------------------------------------------------------------

def test_switch_defaults_off_and_cpu_tensors_stay_step_wise(monkeypatch):
    from training import triplane
    from training import volumetric_rendering as vr
    assert triplane.fused_hierarchical_grad is False
    calls = []
    monkeypatch.setattr(vr, 'render_triplane_hierarchical', lambda *a, **k: calls.append(k))
    R = triplane.TriplaneRenderer(triplane.tiny_spec()).requires_grad_(False)
    g = torch.Generator().manual_seed(1)
    tex = (torch.randn(1, 48, 8, 8, generator=g) * 0.7).requires_grad_(True)
    geo = torch.randn(1, 48, 8, 8, generator=g) * 0.7
    cam = triplane.camera_label(0.3)[:, :16].reshape(1, 4, 4)
    kw = dict(jitter=torch.rand(1, 64, 12, generator=g), hierarchical=True, importance_u=torch.rand(64, 12, generator=g))
    base = R(tex, geo, cam, **kw)
    monkeypatch.setattr(triplane, 'fused_hierarchical_grad', True)
    on = R(tex, geo, cam, **kw)
    assert not calls, 'CPU tensors reached the fused pass'
    for x, y in zip(on, base):
        assert x.requires_grad and torch.equal(x, y)
    # with the device test out of the way: sigma_noise_fine keeps the call step-wise; without it the call goes to the new path once, and a
    # None from there ("no kernel") falls through to the step-wise result
    monkeypatch.setattr(triplane, '_all_fp32_cuda', lambda *tensors: True)
    R(tex, geo, cam, sigma_noise_fine=torch.zeros(1, 64, 24), **kw)
    assert not calls
    R(tex, geo, cam.clone().requires_grad_(True), **kw)
    assert not calls, 'a camera that requires grad reached the fused pass'
    R(tex, geo, cam, **dict(kw, jitter=kw['jitter'].clone().requires_grad_(True)))
    assert not calls, 'a jitter that requires grad reached the fused pass'
    R(tex, geo, cam, **dict(kw, importance_u=kw['importance_u'].clone().requires_grad_(True)))
    assert not calls, 'pdf draws that require grad reached the fused pass'
    R(tex, geo, cam, jitter=kw['jitter'], hierarchical=False)
    assert not calls, 'the plain render reached the fused pass'
    out = R(tex, geo, cam, **kw)
    assert len(calls) == 1 and calls[0]['importance_u'] is kw['importance_u'] and calls[0]['jitter'] is kw['jitter']
    for x, y in zip(out, base):
        assert torch.equal(x, y)
    (ga,), (gb,) = torch.autograd.grad(out[0].sum(), [tex]), torch.autograd.grad(base[0].sum(), [tex])
    assert torch.equal(ga, gb)
    with torch.no_grad():
        R(tex, geo, cam, **kw)
    assert len(calls) == 1, 'grad mode off: nothing to differentiate'
    # fused_hierarchical stays independent: its own switch, its own rule
    assert triplane.fused_hierarchical is False


def test_rules_with_the_switch_on():
    """The rule itself, on stand-ins for CUDA tensors (only device type, dtype and requires_grad are read)."""
    from training import triplane

    class T:
        def __init__(self, requires_grad=False, device='cuda', dtype=torch.float32):
            self.requires_grad, self.device, self.dtype = requires_grad, torch.device(device), dtype

    class Dec:
        def __init__(self, ps):
            self.ps = ps

        def parameters(self):
            return iter(self.ps)

    class R:
        _fused_hier_grad_ok = triplane.TriplaneRenderer._fused_hier_grad_ok

    def ok(planes=(False, False), params=(False,) * 8, cam=T(), jit=None, noise=None, u=None, pdev='cuda', pdtype=torch.float32,
           tdtype=torch.float32):
        r = R()
        r.decoder = Dec([T(g, pdev, pdtype) for g in params])
        return r._fused_hier_grad_ok(T(planes[0], dtype=tdtype), T(planes[1], dtype=tdtype), cam, jit, noise, u)

    one = (False,) * 7 + (True,)
    old = triplane.fused_render_param_grad
    try:
        triplane.fused_render_param_grad = False
        assert ok(planes=(True, False)) and ok(planes=(False, True), jit=T(), noise=T(), u=T())
        assert not ok(), 'nothing requires grad'
        assert not ok(params=one) and not ok(planes=(True, True), params=one), 'a trainable decoder needs fused_render_param_grad'
        assert not ok(planes=(True, False), cam=T(True))
        assert not ok(planes=(True, False), jit=T(True))
        assert not ok(planes=(True, False), noise=T(True))
        assert not ok(planes=(True, False), u=T(True))
        assert not ok(planes=(True, False), tdtype=torch.float16)
        assert not ok(planes=(True, False), cam=T(device='cpu'))
        with torch.no_grad():
            assert not ok(planes=(True, False))
        triplane.fused_render_param_grad = True
        assert ok(planes=(True, False)) and ok(params=one) and ok(planes=(True, True), params=(True,) * 8)
        assert not ok(params=one, cam=T(True)) and not ok(params=one, jit=T(True)) and not ok(params=one, u=T(True))
        assert not ok(params=one, pdev='cpu') and not ok(params=one, pdtype=torch.float64)
        old_cam = triplane.fused_render_camera_grad
        try:
            triplane.fused_render_camera_grad = True
            assert not ok(planes=(True, False), cam=T(True)), 'the merged march has no camera gradient under any switch'
        finally:
            triplane.fused_render_camera_grad = old_cam
    finally:
        triplane.fused_render_param_grad = old


# ---- the reference ---------------------------------------------------------------------------------------------

def test_reference_autograd_equals_central_differences():
    """hier_grad_ref's float64 autograd against float64 central differences (h = 1e-6: truncation ~h^2, rounding ~1e-16 / h, both far below
    the 1e-6 of the gradient's max-abs asked here) on a dozen plane entries and a dozen decoder entries of a tiny scene with forced ties."""
    from training import triplane
    C, size, S, n = 16, 3, 5, 2
    sp = triplane.tiny_spec(render_size=size, num_steps=S)
    torch.manual_seed(3)
    R0 = triplane.TriplaneRenderer(sp)
    with torch.no_grad():
        for p in R0.parameters():
            if p.ndim == 1:
                p.copy_(torch.randn_like(p) * 0.2)
    sd = {'synthesis.renderer.' + k: v for k, v in R0.state_dict().items()}
    R64 = hier_grad_ref.renderer64(sp, sd)
    R64.decoder.requires_grad_(True)
    g = torch.Generator().manual_seed(4)
    planes = (torch.randn(n, 6 * C, 8, 8, generator=g) * 0.7).double().requires_grad_(True)
    cam = torch.cat([triplane.camera_label(0.4), triplane.camera_label(-0.3, pitch=1.4)])[:, :16].reshape(n, 4, 4)
    rays = size * size
    jit = torch.rand(n, rays, S, generator=g)
    z_lin = torch.linspace(sp.ray_start, sp.ray_end, S)
    z_coarse = (z_lin + (jit - 0.5) * (z_lin[1] - z_lin[0])).reshape(n * rays, S)
    z_fine = torch.rand(n * rays, S, generator=g) * (sp.ray_end - sp.ray_start) + sp.ray_start
    z_fine[:, 0] = z_coarse[:, 2]                        # ties: delta = 0 between a fine sample and the coarse one at the same depth
    z_all, src = hier_ref.merge(z_fine, z_coarse)
    P = (torch.randn(n, sp.feature_channels + sp.seg_channels, size, size, generator=g).double(),
         torch.randn(n, 1, size, size, generator=g).double(), torch.randn(n, 1, size, size, generator=g).double())

    def value():
        out = hier_grad_ref.merged_outputs(R64, planes[:, :3 * C], planes[:, 3 * C:], cam, sp.fov, size, S, sp.ray_start, sp.ray_end, jit,
                                           z_all, src, z_fine, clamp_mode='softplus', white_back=True, max_depth=3.75)
        return hier_grad_ref.loss(*out, P)

    leaves = [planes] + list(R64.decoder.parameters())
    grads = torch.autograd.grad(value(), leaves)
    assert all(float(x.abs().max()) > 0 for x in grads)
    h, pick = 1e-6, torch.Generator().manual_seed(5)
    worst = 0.0
    for leaf, grad in zip(leaves, grads):
        # the plane entries that matter are the ones a ray touches: take the largest gradients' positions and some at random
        flat = grad.reshape(-1)
        idx = torch.cat([flat.abs().topk(min(6, flat.numel())).indices, torch.randint(flat.numel(), (6,), generator=pick)]) if leaf is planes \
            else torch.randint(flat.numel(), (2,), generator=pick)
        for i in idx.tolist():
            with torch.no_grad():
                view = leaf.view(-1)
                keep = float(view[i])
                view[i] = keep + h; up = float(value())
                view[i] = keep - h; down = float(value())
                view[i] = keep
            fd = (up - down) / (2 * h)
            worst = max(worst, abs(fd - float(flat[i])) / float(flat.abs().max()))
    print(f'[hier-grad-ref] autograd vs central differences: worst {worst:.2e} of each gradient\'s max-abs')
    assert worst <= 1e-6
