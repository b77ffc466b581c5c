"""The C ABI of csrc/adv_loss.hip without a GPU: the header, the binding and the built library agree on the new entry points, and their
host-side argument checks refuse bad arguments with their text before anything is launched (no device access)."""

import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NAMES = ('ide3d_minibatch_std', 'ide3d_minibatch_std_backward', 'ide3d_adv_head', 'ide3d_adv_head_backward')


def _header():
    return re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'ide3d_hip.h')).read(), flags=re.S)


def test_entry_points_are_declared_listed_and_exported():
    """Every entry point csrc/adv_loss.hip defines is declared in the header, listed by the binding and exported, and the reverse; the
    ctypes prototype has one argument type per parameter of the declaration.  The ABI version stays 8: entry points are only added."""
    from torch_utils import hip_plugin
    h = re.sub(r'\s+', ' ', _header())
    src = open(os.path.join(ROOT, 'ide-3d_amd', 'csrc', 'adv_loss.hip')).read()
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
            want = ctypes.c_int32 if 'int32_t' in decl and '*' not in decl else None
            assert (a is want) if want is not None else ('*' in decl), (name, decl)
    assert hip_plugin._ABI_VERSION == 8 and lib.ide3d_abi_version() == 8
    assert hip_plugin.PLUGINS['adv_loss_plugin'] is hip_plugin.AdvLossPlugin
    for method in ('minibatch_std', 'minibatch_std_backward', 'head', 'head_backward'):
        assert callable(getattr(hip_plugin.AdvLossPlugin, method))
    assert hip_plugin.AdvLossPlugin.MAX_M == 8192


def test_argument_checks_refuse_before_any_launch():
    from torch_utils import hip_plugin
    lib = hip_plugin.load()
    err = lambda: lib.ide3d_last_error()
    std, bwd = lib.ide3d_minibatch_std, lib.ide3d_minibatch_std_backward
    # minibatch_std (x, y, n, c, h, w, group, features): null pointers, a batch that is no multiple of the group, channels that are no
    # multiple of the features, a negative group, no features, an empty tensor
    assert std(None, 16, 4, 4, 4, 4, 2, 1, None) == -1 and b'minibatch_std: null pointer' in err()
    assert std(16, None, 4, 4, 4, 4, 2, 1, None) == -1 and b'null pointer' in err()
    assert std(16, 16, 6, 4, 4, 4, 4, 1, None) == -1 and b'not a multiple of the group size 4' in err()
    assert std(16, 16, 3, 4, 4, 4, 4, 1, None) == -1 and b'group size' in err(), 'a group larger than the batch'
    assert std(16, 16, 4, 5, 4, 4, 2, 2, None) == -1 and b'not a multiple of features = 2' in err()
    assert std(16, 16, 4, 4, 4, 4, -1, 1, None) == -1 and b'group >= 0' in err()
    assert std(16, 16, 4, 4, 4, 4, 2, 0, None) == -1 and std(16, 16, 0, 4, 4, 4, 0, 1, None) == -1 and std(16, 16, 4, 4, 0, 4, 2, 1, None) == -1
    assert std(16, 16, 4, 4, 1 << 15, 1 << 15, 2, 1, None) == -1 and b'too large' in err()
    assert bwd(16, 16, None, 4, 4, 4, 4, 2, 1, None) == -1 and b'minibatch_std_backward: null pointer' in err()
    assert bwd(16, None, 16, 4, 4, 4, 4, 2, 1, None) == -1 and bwd(None, 16, 16, 4, 4, 4, 4, 2, 1, None) == -1
    assert bwd(16, 16, 16, 6, 4, 4, 4, 4, 1, None) == -1 and b'minibatch_std_backward: the batch n = 6 is not a multiple of the group size 4' in err()
    assert bwd(16, 16, 16, 4, 5, 4, 4, 2, 2, None) == -1 and b'not a multiple of features' in err()
    # adv_head (o, cmap, logit, loss, n, M, sign): null pointers, a sign that is not -1 or +1, M past the limit, no cmap with M != 1, no image
    head, hb = lib.ide3d_adv_head, lib.ide3d_adv_head_backward
    assert head(None, 16, 16, 16, 2, 8, -1, None) == -1 and b'adv_head: null pointer' in err()
    assert head(16, 16, None, 16, 2, 8, -1, None) == -1 and head(16, 16, 16, None, 2, 8, -1, None) == -1
    assert head(16, 16, 16, 16, 2, 8, 0, None) == -1 and b'sign must be -1 or +1' in err()
    assert head(16, 16, 16, 16, 2, 8, 2, None) == -1 and b'sign' in err()
    assert head(16, 16, 16, 16, 2, 8193, 1, None) == -1 and b'M <= 8192' in err()
    assert head(16, None, 16, 16, 2, 8, 1, None) == -1 and b'without cmap M must be 1' in err()
    assert head(16, 16, 16, 16, 0, 8, 1, None) == -1 and head(16, 16, 16, 16, 2, 0, 1, None) == -1
    # adv_head_backward (o, cmap, logit, dloss, do, n, M, sign)
    assert hb(16, 16, 16, None, 16, 2, 8, 1, None) == -1 and b'adv_head_backward: null pointer' in err()
    assert hb(16, 16, None, 16, 16, 2, 8, 1, None) == -1 and hb(16, 16, 16, 16, None, 2, 8, 1, None) == -1 and hb(None, 16, 16, 16, 16, 2, 8, 1, None) == -1
    assert hb(16, 16, 16, 16, 16, 2, 8, 3, None) == -1 and b'sign must be -1 or +1' in err()
    assert hb(16, None, 16, 16, 16, 2, 8, 1, None) == -1 and b'without cmap M must be 1' in err()
    assert hb(16, 16, 16, 16, 16, 2, 8193, -1, None) == -1 and hb(16, 16, 16, 16, 16, 65536, 8, -1, None) == -1
