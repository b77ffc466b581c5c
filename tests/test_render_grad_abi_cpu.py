"""C ABI of the fused renderer's backward (ide3d_render_rays_backward, include/ide3d_hip.h): the ctypes mirror of ide3d_render_grads, the
declaration, EXPORTED_SYMBOLS and the built library's export; and the routing rules of TriplaneRenderer that need no GPU.  No GPU needed."""
import ctypes
import os
import re

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header():
    return re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'ide3d_hip.h')).read(), flags=re.S)


def test_render_grads_struct_matches_header():
    from torch_utils import hip_plugin
    body = re.search(r'typedef struct ide3d_render_grads \{(.*?)\} ide3d_render_grads;', _header(), re.S).group(1)
    names = []
    for decl in body.split(';'):
        decl = decl.strip()
        if decl:
            names.append(re.search(r'([A-Za-z_][A-Za-z0-9_]*)\s*(\[\d+\])?\s*$', decl).group(1))
    cls = hip_plugin._RenderGrads
    assert names == [f[0] for f in cls._fields_]
    offsets = {f[0]: getattr(cls, f[0]).offset for f in cls._fields_}
    assert offsets == {'grad_feat': 0, 'grad_depth': 8, 'grad_wsum': 16, 'grad_tex_planes': 24, 'grad_geo_planes': 32,
                       'grad_tex_stride': 40, 'grad_geo_stride': 72}
    assert ctypes.sizeof(cls) == 104


def test_render_rays_backward_is_declared_listed_and_exported():
    from torch_utils import hip_plugin
    assert re.search(r'int ide3d_render_rays_backward\(const ide3d_render_params\* p, const ide3d_render_grads\* g, void\* stream\);', _header())
    assert 'ide3d_render_rays_backward' in hip_plugin.EXPORTED_SYMBOLS
    assert hip_plugin._ABI_VERSION == 8
    path = hip_plugin.lib_path()
    assert os.path.isfile(path), f'{path} missing: run __graft_entry__.build()'
    assert hasattr(ctypes.CDLL(path), 'ide3d_render_rays_backward')


def test_fused_gradient_routing_rules_on_cpu():
    """CPU planes never take the fused gradient path; the module switch exists and is on by default."""
    from training import triplane
    assert triplane.fused_render_grad is True
    R = triplane.TriplaneRenderer(triplane.tiny_spec())
    for p in R.decoder.parameters():
        p.requires_grad_(False)
    tex = torch.zeros(1, 48, 8, 8, requires_grad=True)
    geo = torch.zeros(1, 48, 8, 8)
    cam = torch.eye(4)[None]
    assert not R._fused_grad_ok(tex, geo, cam, None, None)
