"""training/projection.py without a GPU: the torch definitions of the noise regulariser and the noise normaliser against the float64
restatement (tests/noise_ref.py) and against values worked out by hand, `project()` on CPU tensors, and the C ABI of csrc/noise_reg.hip
(declared in the header, listed, exported by the built library, ABI version unchanged)."""
import copy
import ctypes
import os
import re

import pytest
import torch

import noise_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header():
    return re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'ide3d_hip.h')).read(), flags=re.S)


def test_hand_computed_4x4():
    """n[y][x] = x.  n * left: 0*3, 1*0, 2*1, 3*2 -> mean 2; n * up = x^2 -> mean 3.5; one level: 2^2 + 3.5^2 = 16.25."""
    from training import projection
    n = torch.arange(4.0).repeat(4, 1)
    assert float(projection.noise_regularization([n])) == 16.25
    assert float(noise_ref.reg64([n])) == 16.25


def test_hand_computed_16x16_has_the_levels_16_and_8():
    """Columns 2, 2, 0, 0 repeating.  Level 16: n * left = 0, 4, 0, 0 -> mean 1; n * up = n^2 -> mean 2: 1 + 4.  Level 8: columns 2, 0
    repeating: n * left = 0; n * up -> mean 2: 0 + 4.  Total 9.  (A 4 x 4 level would be all ones and add 2.)"""
    from training import projection
    n = torch.tensor([2.0, 2.0, 0.0, 0.0]).repeat(16, 4)
    assert n.shape == (16, 16)
    assert float(projection.noise_regularization([n])) == 9.0
    assert float(noise_ref.reg64([n])) == 9.0


@pytest.mark.parametrize('shapes', [[(4, 4)], [(8, 8), (16, 16), (64, 64)], [(12, 12)], [(16, 32)], [(32, 32), (12, 12), (16, 32)]])
def test_torch_regulariser_and_its_gradient_against_float64(shapes):
    from training import projection
    g = torch.Generator().manual_seed(len(shapes) + shapes[0][0])
    maps = [torch.randn(*s, generator=g) + 0.3 for s in shapes]
    want, want_g = noise_ref.reg64_with_grads(maps)
    leaves = [m.clone().requires_grad_(True) for m in maps]
    got = projection.noise_regularization(leaves)
    got.backward()
    assert got.dtype == torch.float32 and got.ndim == 0
    assert abs(float(got.detach()) - float(want)) <= 1e-5 * float(want)
    for leaf, wg in zip(leaves, want_g):
        assert float((leaf.grad.double() - wg).abs().max()) <= 1e-5 * float(wg.abs().max())


def test_empty_list_and_switch():
    from training import projection
    assert projection.fused_noise_ops is True
    z = projection.noise_regularization([])
    assert z.ndim == 0 and float(z) == 0.0
    assert projection.normalize_noise_([]) == []


def test_torch_normaliser_against_float64():
    from training import projection
    g = torch.Generator().manual_seed(5)
    maps = [0.3 + 1.2 * torch.randn(s, s, generator=g) for s in (4, 8, 16, 12, 64)] + [torch.randn(16, 32, generator=g)]
    want = noise_ref.normalize64(maps)
    leaves = [m.clone().requires_grad_(True) for m in maps]           # leaves that require grad: the function brings its own no_grad
    versions = [t._version for t in leaves]
    out = projection.normalize_noise_(leaves)
    assert all(a is b for a, b in zip(out, leaves))
    for t, v, w in zip(leaves, versions, want):
        assert t._version > v
        assert float((t.detach().double() - w).abs().max()) <= 1e-6
        assert abs(float(t.detach().double().mean())) <= 1e-6 and abs(float(t.detach().double().square().mean()) - 1) <= 1e-5


def test_project_on_cpu_tensors():
    from training import projection, triplane
    torch.manual_seed(0)
    G = triplane.TriPlaneGenerator(triplane.tiny_spec()).eval()
    with torch.no_grad():
        for name, p in G.synthesis.named_parameters():
            if name.endswith('noise_strength'):
                p.fill_(0.3)
    state = {k: v.detach().clone() for k, v in G.state_dict().items()}
    flags = {k: p.requires_grad for k, p in G.named_parameters()}
    c = triplane.camera_label(0.2)
    target = torch.rand(3, G.img_resolution, G.img_resolution, generator=torch.Generator().manual_seed(1)) * 255
    w, info = projection.project(G, target, c, num_steps=3, w_avg_samples=32, return_info=True)
    assert tuple(w.shape) == (1, G.num_ws, G.w_dim) and not w.requires_grad
    assert len(info['losses']) == 3 and all(v == v for v in info['losses'])
    assert len(info['noise_maps']) == len(projection.noise_maps(G)) > 0
    for n in info['noise_maps']:
        assert abs(float(n.double().mean())) <= 1e-5 and abs(float(n.double().square().mean()) - 1) <= 1e-5
    # the caller's generator: same values, same flags, maps still plain buffers
    for k, v in G.state_dict().items():
        assert torch.equal(v, state[k]), k
    assert {k: p.requires_grad for k, p in G.named_parameters()} == flags
    assert not any(b.requires_grad for b in projection.noise_maps(G))
    # W+: a per-layer start is optimised per layer
    w_plus = projection.project(G, target, c, num_steps=1, w_avg_samples=8, initial_w=w + torch.arange(G.num_ws)[None, :, None] * 0.01)
    assert tuple(w_plus.shape) == (1, G.num_ws, G.w_dim) and not torch.equal(w_plus[:, 0], w_plus[:, 1])


def test_trainable_noise_map_on_the_cpu_keeps_the_aten_definition():
    """CPU tensors never take the HIP gradient path, with `hip_noise_grad` on (the default) as before it."""
    from training import networks
    assert networks.hip_noise_grad is True
    torch.manual_seed(2)
    lay = networks.SynthesisLayer(8, 8, w_dim=16, resolution=8).requires_grad_(False)
    with torch.no_grad():
        lay.noise_strength.fill_(0.3)
    lay.noise_const.requires_grad_(True)
    y = lay(torch.randn(2, 8, 8, 8), torch.randn(2, 16), noise_mode='const')
    assert 'Modconv' not in type(y.grad_fn).__name__
    y.square().sum().backward()
    assert lay.noise_const.grad is not None and float(lay.noise_const.grad.abs().max()) > 0


def test_entry_points_are_declared_listed_and_exported():
    from torch_utils import hip_plugin
    h = _header()
    table = r'const ide3d_noise_map\* table, const int32_t\* sides, int32_t k'
    assert re.search(r'typedef struct ide3d_noise_map \{\s*float\*\s+data;\s*int32_t\s+side;\s*int32_t\s+reserved;\s*\} ide3d_noise_map;', h)
    assert re.search(r'int ide3d_noise_reg\(' + table + r', float\* workspace, int64_t workspace_bytes,\s*float\* means, float\* loss, '
                     r'void\* stream\);', h)
    assert re.search(r'int ide3d_noise_reg_backward\(' + table + r', const float\* workspace, int64_t workspace_bytes,\s*const float\* means, '
                     r'const float\* dloss, float\* grad, void\* stream\);', h)
    assert re.search(r'int ide3d_noise_normalize\(' + table + r', float\* workspace, int64_t workspace_bytes,\s*void\* stream\);', h)
    assert ctypes.sizeof(hip_plugin._NoiseMap) == 16 and hip_plugin._NoiseMap.side.offset == 8
    assert hip_plugin._ABI_VERSION == 8
    path = hip_plugin.lib_path()
    assert os.path.isfile(path), f'{path} missing: run __graft_entry__.build()'
    lib = ctypes.CDLL(path)
    for name in ('ide3d_noise_reg', 'ide3d_noise_reg_backward', 'ide3d_noise_normalize', 'ide3d_noise_reg_workspace_bytes',
                 'ide3d_noise_reg_levels', 'ide3d_noise_normalize_workspace_bytes'):
        assert name in hip_plugin.EXPORTED_SYMBOLS
        assert hasattr(lib, name)
    assert lib.ide3d_abi_version() == 8


def test_layout_queries():
    """Host arithmetic only.  Levels: side, side / 2, ..., 8 (one for side <= 8).  Workspace: the pooled levels plus two partial sums (two fp32 words each) per
    (level, 64 x 64 tile); the normaliser: two such sums per tile.  Sides that are not powers of two in 4..512 are refused."""
    from torch_utils import hip_plugin
    lib = ctypes.CDLL(hip_plugin.lib_path())
    i32p = ctypes.POINTER(ctypes.c_int32)
    lib.ide3d_noise_reg_workspace_bytes.restype = lib.ide3d_noise_normalize_workspace_bytes.restype = ctypes.c_int64
    for fn in (lib.ide3d_noise_reg_workspace_bytes, lib.ide3d_noise_normalize_workspace_bytes, lib.ide3d_noise_reg_levels):
        fn.argtypes = [i32p, ctypes.c_int32]

    def q(fn, sides):
        return fn((ctypes.c_int32 * len(sides))(*sides), len(sides))

    assert q(lib.ide3d_noise_reg_levels, [4]) == 1 and q(lib.ide3d_noise_reg_levels, [8]) == 1 and q(lib.ide3d_noise_reg_levels, [16]) == 2
    assert q(lib.ide3d_noise_reg_levels, [4, 8, 8, 16, 32, 128, 512]) == 1 + 1 + 1 + 2 + 3 + 5 + 7
    assert q(lib.ide3d_noise_reg_workspace_bytes, [8]) == 4 * 4
    assert q(lib.ide3d_noise_reg_workspace_bytes, [16]) == 4 * (64 + 2 * 4)
    assert q(lib.ide3d_noise_reg_workspace_bytes, [128]) == 4 * (64 * 64 + 32 * 32 + 16 * 16 + 8 * 8 + 4 * 5 * 4)
    assert q(lib.ide3d_noise_normalize_workspace_bytes, [512, 4]) == 4 * 4 * (64 + 1)
    for bad in ([2], [1024], [12], [0], []):
        assert q(lib.ide3d_noise_reg_workspace_bytes, bad) == -1 and q(lib.ide3d_noise_normalize_workspace_bytes, bad) == -1
        assert q(lib.ide3d_noise_reg_levels, bad) == -1
