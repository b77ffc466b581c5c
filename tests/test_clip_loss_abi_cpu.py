"""The C ABI of csrc/clip_loss.hip without a GPU: the header, the binding and the built library agree on the new entry points, and their
host-side argument checks refuse bad arguments before anything is launched (no device access)."""

import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NAMES = ('ide3d_clip_prep', 'ide3d_clip_prep_backward', 'ide3d_vit_embed', 'ide3d_vit_embed_backward', 'ide3d_layernorm', 'ide3d_layernorm_backward',
         'ide3d_vit_attention', 'ide3d_vit_attention_backward', 'ide3d_quickgelu', 'ide3d_quickgelu_backward', 'ide3d_clip_head',
         'ide3d_clip_head_backward')


def _header():
    return re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'ide3d_hip.h')).read(), flags=re.S)


def test_entry_points_are_declared_listed_and_exported():
    """Every entry point csrc/clip_loss.hip defines is declared in the header, listed by the binding and exported, and the reverse; the
    ctypes prototype has one argument type per parameter of the declaration.  The ABI version stays 8: entry points are only added."""
    from torch_utils import hip_plugin
    h = re.sub(r'\s+', ' ', _header())
    src = open(os.path.join(ROOT, 'ide-3d_amd', 'csrc', 'clip_loss.hip')).read()
    assert set(re.findall(r'extern "C" \w+ (ide3d_\w+)\(', src)) == set(NAMES)
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
        assert fn.restype is ctypes.c_int, name
        for a, decl in zip(fn.argtypes, params):
            want = (ctypes.c_int32 if 'int32_t' in decl and '*' not in decl else ctypes.c_int64 if 'int64_t' in decl and '*' not in decl
                    else ctypes.c_float if 'float' in decl and '*' not in decl else None)
            assert (a is want) if want is not None else ('*' in decl), (name, decl)
    assert hip_plugin._ABI_VERSION == 8 and lib.ide3d_abi_version() == 8
    assert hip_plugin.PLUGINS['clip_loss_plugin'] is hip_plugin.ClipLossPlugin
    P = hip_plugin.ClipLossPlugin
    assert (P.SIDE, P.MAX_TOKENS, P.MAX_HEAD_DIM) == (224, 64, 64)
    for method in ('prep', 'prep_backward', 'embed', 'embed_backward', 'layernorm', 'layernorm_backward', 'attention', 'attention_backward', 'quickgelu',
                   'quickgelu_backward', 'head', 'head_backward'):
        assert callable(getattr(P, method))


def test_argument_checks_refuse_before_any_launch():
    from torch_utils import hip_plugin
    lib = hip_plugin.load()
    f = ctypes.c_float
    err = lambda: lib.ide3d_last_error()
    # prep: null pointers, mean without std, k and p out of range
    assert lib.ide3d_clip_prep(None, None, None, 16, 1, 1, 32, None) == -1 and b'null pointer' in err()
    assert lib.ide3d_clip_prep(16, 16, None, 16, 1, 1, 32, None) == -1 and b'mean and std' in err()
    assert lib.ide3d_clip_prep(16, None, None, 16, 1, 0, 32, None) == -1 and lib.ide3d_clip_prep(16, None, None, 16, 1, 257, 32, None) == -1
    assert lib.ide3d_clip_prep(16, None, None, 16, 1, 1, 48, None) == -1 and b'dividing 224' in err()
    assert lib.ide3d_clip_prep(16, None, None, 16, 0, 1, 32, None) == -1
    assert lib.ide3d_clip_prep_backward(16, None, None, 1, 1, 32, None) == -1 and lib.ide3d_clip_prep_backward(16, None, 16, 1, 1, 0, None) == -1
    # embed and LayerNorm
    assert lib.ide3d_vit_embed(16, 16, 16, 16, 16, 16, None, 1, 8, 5, f(1e-5), None) == -1 and b'null pointer' in err()
    assert lib.ide3d_vit_embed(16, 16, 16, 16, 16, 16, 16, 1, 8, 1, f(1e-5), None) == -1 and b'T >= 2' in err()
    assert lib.ide3d_vit_embed_backward(16, 16, 16, 16, 16, 16, 16, 0, 8, 5, None) == -1
    assert lib.ide3d_layernorm(16, 16, 16, 16, 16, 16, 1, 8, 5, 4, f(1e-5), None) == -1 and b'pitch' in err()
    assert lib.ide3d_layernorm(16, 16, 16, 16, 16, 16, 1, 0, 5, 5, f(1e-5), None) == -1 and lib.ide3d_layernorm(16, 16, 16, 16, 16, 16, 1, 8, 5, 5, f(-1.0), None) == -1
    assert lib.ide3d_layernorm_backward(16, 16, 16, 16, 16, None, None, 1, 8, 5, 5, None) == -1 and b'null pointer' in err()
    assert lib.ide3d_layernorm_backward(16, 16, 16, 16, 16, None, 16, 1, 8, 6, 5, None) == -1
    # attention: T and d past 64, d no multiple of 4
    assert lib.ide3d_vit_attention(16, 16, 1, 2, 32, 65, f(1.0), None) == -1 and b'T <= 64' in err()
    assert lib.ide3d_vit_attention(16, 16, 1, 2, 68, 50, f(1.0), None) == -1 and lib.ide3d_vit_attention(16, 16, 1, 2, 6, 50, f(1.0), None) == -1
    assert lib.ide3d_vit_attention(16, None, 1, 2, 32, 50, f(1.0), None) == -1
    assert lib.ide3d_vit_attention_backward(16, 16, 16, 1, 0, 32, 50, f(1.0), None) == -1 and lib.ide3d_vit_attention_backward(16, None, 16, 1, 2, 32, 50, f(1.0), None) == -1
    # QuickGELU: count, alignment to a float
    assert lib.ide3d_quickgelu(16, 16, 0, None) == -1 and lib.ide3d_quickgelu(16, 16, 2 ** 40, None) == -1 and lib.ide3d_quickgelu(18, 16, 4, None) == -1
    assert lib.ide3d_quickgelu_backward(None, 16, 16, 4, None) == -1 and lib.ide3d_quickgelu_backward(16, 16, None, 4, None) == -1
    # head
    assert lib.ide3d_clip_head(16, None, 16, 16, 16, 16, 16, 16, 16, 1, 8193, 1, None) == -1 and lib.ide3d_clip_head(16, None, 16, 16, 16, 16, 16, 16, 16, 1, 8, 0, None) == -1
    assert lib.ide3d_clip_head(16, None, None, 16, 16, 16, 16, 16, 16, 1, 8, 1, None) == -1 and b'null pointer' in err()
    assert lib.ide3d_clip_head(16, None, 16, 16, 16, 16, 16, 20, 16, 1, 8, 1, None) == -1 and b'8-byte' in err()
    assert lib.ide3d_clip_head_backward(16, 16, 16, 16, None, 16, 1, 8, 1, None) == -1
