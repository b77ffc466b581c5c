"""C ABI of the fused 3x3 layer + dual heads entry point (ide3d_modconv2d_heads, include/ide3d_hip.h): the ctypes mirror of
ide3d_modconv_head_epilogue and the exported symbol.  No GPU needed."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_head_epilogue_struct_matches_header():
    from torch_utils import hip_plugin
    src = open(os.path.join(ROOT, 'include', 'ide3d_hip.h')).read()
    body = re.search(r'typedef struct ide3d_modconv_head_epilogue \{(.*?)\} ide3d_modconv_head_epilogue;', src, re.S).group(1)
    body = re.sub(r'/\*.*?\*/', '', body, flags=re.S)
    names = [re.search(r'([A-Za-z_][A-Za-z0-9_]*)\s*$', d.strip()).group(1) for d in body.split(';') if d.strip()]
    cls = hip_plugin._ModconvHeadEpilogue
    assert names == [f[0] for f in cls._fields_]
    # natural alignment on LP64: three pointers, three 4-byte fields (+ 4 bytes of padding), pointer, int64
    offsets = {f[0]: getattr(cls, f[0]).offset for f in cls._fields_}
    assert offsets == {'w': 0, 'bias': 8, 'y': 16, 'rows': 24, 'clamp': 28, 'no_activation_output': 32, 'workspace': 40, 'workspace_bytes': 48}
    assert ctypes.sizeof(cls) == 56


def test_modconv2d_heads_is_exported():
    from torch_utils import hip_plugin
    assert 'ide3d_modconv2d_heads' in hip_plugin.EXPORTED_SYMBOLS
    src = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'ide3d_hip.h')).read(), flags=re.S)
    assert re.search(r'int ide3d_modconv2d_heads\(const ide3d_modconv_params\* p, const ide3d_modconv_head_epilogue\* heads, void\* stream\);', src)
    path = hip_plugin.lib_path()
    assert os.path.isfile(path), f'{path} missing: run __graft_entry__.build()'
    assert hasattr(ctypes.CDLL(path), 'ide3d_modconv2d_heads')
