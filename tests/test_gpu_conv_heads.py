"""The dual heads fused into the epilogue of the 3x3 layer in front of them (ide3d_modconv2d_heads, csrc/modconv.hip HeadEpi).

 * at the three real shapes (backbone 128 -> 192 @256, super-resolution 128 -> 22 @256 and 64 -> 22 @512), batch 4 and 1: the heads and the
   layer's own output are bit-equal to the two ide3d_modconv2d calls they replace;
 * the entry point declines (IDE3D_ENOKERNEL -> None) shapes and arithmetics it has no form for, and the knob turns it off;
 * the full generator is bit-equal with the fusion on and off, eager and replayed from a hipGraph, and the fused launch did run;
 * a foreign packed-fp32 kernel beside the fused kernel is never disturbed (exclusive residency).
"""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SHAPES = [  # n, cin, cout, h, w, head rows
    (4, 128, 128, 256, 256, 192), (4, 128, 128, 256, 256, 22), (4, 64, 64, 512, 512, 22),
    (1, 128, 128, 256, 256, 192), (1, 128, 128, 256, 256, 22), (1, 64, 64, 512, 512, 22),
]


def _problem(dev, n, cin, cout, h, w, rows, seed=0):
    g = torch.Generator().manual_seed(seed)
    rn = lambda *sh: torch.randn(*sh, generator=g).to(dev)
    x = rn(n, cin, h, w)
    wt = rn(cout, cin, 3, 3)
    styles = rn(n, cin) * 0.5 + 1
    dcoefs = (wt[None] * styles[:, None, :, None, None]).square().sum(dim=(2, 3, 4)).add(1e-8).rsqrt()
    noise = rn(h, w) * 0.1
    bias = rn(cout) * 0.1
    head_w = rn(n, rows, cout, 1, 1) / np.sqrt(cout)
    head_b = rn(rows) * 0.1
    return x, wt, styles.contiguous(), dcoefs.contiguous(), noise, bias, head_w, head_b


def _fused(mc, x, wt, styles, dcoefs, noise, bias, head_w, head_b, clamp=256.0, gain=float(np.sqrt(2)), **kw):
    return mc.modconv2d_heads(x, wt, styles, dcoefs, noise, 1.0, bias, 3, 0.2, gain, clamp, head_w, head_b, clamp, **kw)


def _unfused(mc, x, wt, styles, dcoefs, noise, bias, head_w, head_b, clamp=256.0):
    y = mc.modconv2d(x, wt, styles, dcoefs, noise, 1.0, bias, 3, 0.2, float(np.sqrt(2)), clamp)
    heads = mc.modconv2d(y, head_w, None, None, None, 0.0, head_b, 1, 0.0, 1.0, clamp)
    return y, heads


@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_fused_heads_bit_equal_to_two_launches(gpu_device, shape):
    from torch_utils import hip_plugin
    mc = hip_plugin.ModconvPlugin
    args = _problem(gpu_device, *shape)
    y_ref, h_ref = _unfused(mc, *args)
    before = hip_plugin.CALLS.get('modconv2d_heads', 0)
    out = _fused(mc, *args, want_x=True)
    n, cin, cout, h, w, rows = shape
    if hip_plugin.modconv_plan(n, cout, rows, h, w, k=1, per_image=True, epilogue='head')['kind'] not in ('head_split', 'head_resident'):
        assert out is None        # (batch 1, 22 rows: too few workgroups for the split-bf16 heads, which run on the fp32 loop)
        return
    assert out is not None, hip_plugin.load().ide3d_last_error().decode()
    y, heads = out
    assert torch.equal(y, y_ref), 'layer output differs'
    assert torch.equal(heads, h_ref), f'heads differ: max |d| {(heads - h_ref).abs().max().item():.3e}'
    # without the layer's own output: the heads are the same
    y2, heads2 = _fused(mc, *args, want_x=False)
    assert y2 is None and torch.equal(heads2, h_ref)
    assert hip_plugin.CALLS.get('modconv2d_heads', 0) == before + 2
    assert hip_plugin.exclusive_violations()[0] == 0


def test_fused_heads_decline(gpu_device, monkeypatch):
    """No fused form: more than one row block (256 channels), a split-K plan (128 channels @64 at batch 1), the fp32 arithmetic, the knob.
    A declined shape is remembered by the plugin; the library is asked once."""
    from torch_utils import hip_plugin
    mc = hip_plugin.ModconvPlugin
    lib = hip_plugin.load()
    assert _fused(mc, *_problem(gpu_device, 2, 128, 256, 64, 64, 22)) is None
    assert b'all channels of a tile' in lib.ide3d_last_error()
    assert hip_plugin.modconv_plan(1, 128, 128, 64, 64)['split_k'] > 1
    assert _fused(mc, *_problem(gpu_device, 1, 128, 128, 64, 64, 22)) is None
    assert b'all channels of a tile' in lib.ide3d_last_error()
    assert (1, 128, 128, 64, 64, 22, 6) in mc._heads_declined
    args = _problem(gpu_device, 4, 128, 128, 256, 256, 22)
    assert _fused(mc, *args, arith=1) is None
    assert b'bf16x6 only' in lib.ide3d_last_error()
    monkeypatch.setenv('IDE3D_MODCONV_NO_HEAD_FUSION', '1')
    assert _fused(mc, *args) is None
    monkeypatch.delenv('IDE3D_MODCONV_NO_HEAD_FUSION')
    assert _fused(mc, *args) is not None           # (the knob is not remembered as a decline)


def _generator(dev):
    from training import triplane
    torch.manual_seed(0)
    return triplane.TriPlaneGenerator().eval().requires_grad_(False).to(dev)


# (h, head rows) -> blocks fused per pass: vb256 (192 rows @256) and b512 (22 @512) at both batch sizes; b256 (22 @256) at batch 4 only — at
# batch 1 its heads have too few workgroups for the split-bf16 loop and run on the fp32 one, so the library declines
FUSED_BLOCKS = {1: {(256, 192), (512, 22)}, 4: {(256, 192), (256, 22), (512, 22)}}


@pytest.mark.parametrize('batch', [1, 4])
def test_generator_bit_equal_with_and_without_fusion(gpu_device, batch, monkeypatch):
    """Eager synthesis: image, segmentation and both tri-planes are the same (a) fused, (b) with the knob set (the two launches made by
    networks._conv1_dual_head) and (c) on the path the blocks took before the fusion existed (SynthesisLayer.forward + _dual_head); every
    block that has a fused form used it."""
    from torch_utils import hip_plugin
    from training import networks, triplane
    monkeypatch.setenv('IDE3D_AUTO_GRAPH', '0')      # eager passes: a replayed graph would not see the knob or the patched router
    G = _generator(gpu_device)
    z = torch.from_numpy(np.stack([np.random.RandomState(s).randn(G.z_dim) for s in range(batch)])).float().to(gpu_device)
    cams = torch.cat([triplane.camera_label(y) for y in np.linspace(-0.4, 0.4, batch)]).to(gpu_device)
    cond = triplane.conditioning_label().repeat(batch, 1).to(gpu_device)
    fused_shapes = []
    real = hip_plugin.ModconvPlugin.modconv2d_heads

    def recording(x, *args, **kw):
        out = real(x, *args, **kw)
        if out is not None:
            fused_shapes.append((x.shape[-1], out[1].shape[1], out[0] is None))
        return out
    monkeypatch.setattr(hip_plugin.ModconvPlugin, 'modconv2d_heads', staticmethod(recording))

    def run():
        with torch.no_grad():
            ws = G.mapping(z, cond)
            planes = G.synthesis.planes(ws)
            img, seg = G.synthesis(ws, c=cams, noise_mode='const', ray_jitter=False, return_seg=True)
        return [t.clone() for t in (img, seg, *planes)]

    on = run()
    assert {(h, r) for h, r, _ in fused_shapes} == FUSED_BLOCKS[batch], fused_shapes
    # the last blocks of backbone and superres (vb256, b512) do not write their unused activation
    assert all(no_x for h, r, no_x in fused_shapes if (h, r) in ((256, 192), (512, 22)))
    fused_shapes.clear()
    monkeypatch.setenv('IDE3D_MODCONV_NO_HEAD_FUSION', '1')
    knob = run()
    assert not fused_shapes
    monkeypatch.delenv('IDE3D_MODCONV_NO_HEAD_FUSION')
    monkeypatch.setattr(networks, '_conv1_dual_head', lambda *a, **k: None)
    before = run()
    for name, a, b, c in zip(('image', 'image_seg', 'tex plane', 'seg plane'), on, knob, before):
        assert torch.equal(a, b), f'{name} differs with the knob set'
        assert torch.equal(a, c), f'{name} differs from the unfused path'
    assert hip_plugin.exclusive_violations()[0] == 0


def test_graphed_renderer_bit_equal_with_and_without_fusion(gpu_device, monkeypatch):
    """GraphedRenderer at batch 4: the replayed graph with the fused launches equals the one captured with the fusion off."""
    from torch_utils import hip_plugin
    from training import triplane
    G = _generator(gpu_device)
    B = 4
    z = torch.from_numpy(np.stack([np.random.RandomState(s).randn(G.z_dim) for s in range(B)])).float().to(gpu_device)
    cams = torch.cat([triplane.camera_label(y) for y in (-0.3, -0.1, 0.1, 0.3)]).to(gpu_device)
    cond = triplane.conditioning_label().repeat(B, 1).to(gpu_device)
    before = hip_plugin.CALLS.get('modconv2d_heads', 0)
    run = triplane.GraphedRenderer(G, B, gpu_device, ray_jitter=False)
    img_on, seg_on = [t.clone() for t in run(z, cond, cams)]
    assert hip_plugin.CALLS.get('modconv2d_heads', 0) > before, 'the captured pass did not use the fused launch'
    del run
    monkeypatch.setenv('IDE3D_MODCONV_NO_HEAD_FUSION', '1')
    run = triplane.GraphedRenderer(G, B, gpu_device, ray_jitter=False)
    img_off, seg_off = [t.clone() for t in run(z, cond, cams)]
    assert torch.equal(img_on, img_off) and torch.equal(seg_on, seg_off)


def test_foreign_packed_fp32_victim_beside_fused_heads(gpu_device):
    """tests/native/pk_victim.hip (packed fp32 on operands straight from global loads) on a second stream while the fused kernels run:
    every victim launch equals its result computed alone."""
    import ctypes
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'native', '_bin', 'libpk_victim.so')
    if not os.path.isfile(path):
        import sys
        sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
        import __graft_entry__
        path = __graft_entry__.build_test_natives()
    if not os.path.isfile(path):
        pytest.skip('tests/native/pk_victim.hip could not be built here')
    lib = ctypes.CDLL(path)
    lib.pk_victim_launch.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p]
    lib.pk_aggressor_launch.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p]
    from torch_utils import hip_plugin
    mc = hip_plugin.ModconvPlugin
    dev = gpu_device
    g = torch.Generator().manual_seed(12)
    K, BLOCKS, REPS = 512, 64, 600
    A = torch.randn(BLOCKS * 32, K, generator=g).to(dev); xv = torch.randn(K, generator=g).to(dev)
    ref = torch.empty(BLOCKS * 32, device=dev)
    ys = torch.empty(REPS, BLOCKS * 32, device=dev)
    sa, sb = torch.cuda.Stream(dev), torch.cuda.Stream(dev)
    torch.cuda.synchronize(dev)
    assert lib.pk_victim_launch(A.data_ptr(), xv.data_ptr(), ref.data_ptr(), K, BLOCKS, sb.cuda_stream) == 0
    torch.cuda.synchronize(dev)
    bad = {}
    for shape in SHAPES[:3]:
        args = _problem(dev, *shape)
        ys.zero_()
        torch.cuda.synchronize(dev)
        for i in range(REPS):
            if i % 25 == 0:
                with torch.cuda.stream(sa), torch.no_grad():
                    assert _fused(mc, *args, want_x=False) is not None
            assert lib.pk_victim_launch(A.data_ptr(), xv.data_ptr(), ys[i].data_ptr(), K, BLOCKS, sb.cuda_stream) == 0
        torch.cuda.synchronize(dev)
        bad['x'.join(map(str, shape))] = int((ys != ref[None]).any(dim=1).sum())
    assert not any(bad.values()), f'victim launches disturbed beside the fused kernel: {bad}'
    assert hip_plugin.exclusive_violations()[0] == 0
