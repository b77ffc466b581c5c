"""The low-resolution block group (csrc/lowres.hip, `ide3d_lowres_group`) against the per-layer HIP path it replaces and against a float64
definition of the same blocks (reference semantics: inversion/networks.py:966-1139 `SegSynthesisBlock`, :330-514 `SynthesisLayer`,
:670-713 `ToRGBLayer`; conv2d_resample.py:112-129 for the up-sampling layers)."""

import os

import numpy as np
import pytest
import torch

# the blocks in float64 (tests/blocks64.py): plain torch operations, none of the product's code paths
from blocks64 import blocks64 as _blocks64, layer64 as _layer64, styles64 as _styles64

pytestmark = pytest.mark.gpu


def _blocks(C, nblocks, w_dim, device, img_ch=12, seg_ch=8, conv_clamp=None, seed=0, res0=4):
    from training import triplane
    torch.manual_seed(seed)
    blocks = []
    for i in range(nblocks):
        res = res0 << i
        b = triplane.VoxelBlock(0 if i == 0 else C, C, w_dim=w_dim, resolution=res, img_channels=img_ch, seg_channels=seg_ch, is_last=False,
                                architecture='skip', conv_clamp=conv_clamp, layer_name='training.networks.SynthesisLayer')
        for lay in ([b.conv1] if i == 0 else [b.conv0, b.conv1]):
            lay.noise_strength.data.fill_(0.37)
            lay.bias.data.normal_(0, 0.3)
        b.torgb.bias.data.normal_(0, 0.2)
        b.toseg.bias.data.normal_(0, 0.2)
        blocks.append(b.eval().requires_grad_(False).to(device))
    return blocks


def _split(blocks, ws):
    out, idx = [], 0
    for b in blocks:
        out.append(ws.narrow(1, idx, b.num_conv + b.num_torgb))
        idx += b.num_conv
    return out


def _run(blocks, ws_list, group, start_state=None):
    """-> (x, img, seg) after all blocks, with / without the group launch; also how many blocks the group covered"""
    from training import networks
    old = os.environ.get('IDE3D_NO_LOWRES_GROUP')
    try:
        os.environ.pop('IDE3D_NO_LOWRES_GROUP', None)
        if not group:
            os.environ['IDE3D_NO_LOWRES_GROUP'] = '1'
        x = img = seg = None
        start, resume, info = 0, False, None
        with torch.no_grad():
            grp = networks.lowres_group_forward(blocks, ws_list, noise_mode='const')
            if grp is not None:
                x, img, seg, start, resume = grp
                info = (start, resume, x.clone(), img.clone(), seg.clone())
            for i, (b, w) in enumerate(zip(blocks, ws_list)):
                if i < start:
                    continue
                extra = dict(_resume_after_conv0=True) if (resume and i == start) else {}
                x, img, seg = b(x, img, w, condition_img=seg, noise_mode='const', **extra)
        return x, img, seg, info
    finally:
        if old is None:
            os.environ.pop('IDE3D_NO_LOWRES_GROUP', None)
        else:
            os.environ['IDE3D_NO_LOWRES_GROUP'] = old


def _rel(a, b):
    return float((a.double() - b.double()).abs().max() / b.double().abs().max().clamp_min(1e-30))


@pytest.mark.parametrize('C,nblocks,n', [(64, 3, 1), (64, 4, 3), (512, 4, 1), (512, 3, 4), (512, 3, 2), (128, 2, 8)])
def test_group_equals_per_layer_path(gpu_device, C, nblocks, n):
    from torch_utils import hip_plugin
    assert hip_plugin.conv_arithmetic() == 'bf16x6'
    w_dim = 64
    blocks = _blocks(C, nblocks, w_dim, gpu_device)
    ws = torch.randn([n, sum(b.num_conv for b in blocks) + 1, w_dim], device=gpu_device)
    ws_list = _split(blocks, ws)
    before = hip_plugin.CALLS.get('lowres_group', 0)
    xg, ig, sg, info = _run(blocks, ws_list, True)
    assert info is not None, 'the group launch did not apply'
    assert hip_plugin.CALLS.get('lowres_group', 0) == before + 1
    xr, ir, sr, none = _run(blocks, ws_list, False)
    assert none is None
    # same arithmetic (bf16x6 products, fp32 accumulation), different summation order: a few ulp of the tensor's scale
    assert _rel(xg, xr) < 1e-5, _rel(xg, xr)
    assert _rel(ig, ir) < 1e-5 and _rel(sg, sr) < 1e-5, (_rel(ig, ir), _rel(sg, sr))
    assert hip_plugin.exclusive_violations() == (0, '')


def test_group_with_clamp_and_in_bf16x3(gpu_device):
    """conv_clamp active in every layer and head (the fp16-block setting of a released pickle, inversion/networks.py:1058-1060), and the two-piece
    arithmetic (bf16x3: PARTS = 2 instantiation of every phase) — each against the per-layer path in the same setting."""
    from torch_utils import hip_plugin
    for arith, tol in (('bf16x6', 1e-5), ('bf16x3', 2e-4)):
        hip_plugin.conv_arithmetic(arith)
        try:
            blocks = _blocks(512, 3, 64, gpu_device, conv_clamp=0.6, seed=3)
            ws_list = _split(blocks, torch.randn([2, sum(b.num_conv for b in blocks) + 1, 64], device=gpu_device))
            xg, ig, sg, info = _run(blocks, ws_list, True)
            assert info is not None
            assert float(xg.abs().max()) <= 0.6 * 1.0000001 and float(info[3].abs().max()) > 0.3          # the clamp bites (act gain sqrt 2 on unit-variance data)
            xr, ir, sr, _ = _run(blocks, ws_list, False)
            assert _rel(xg, xr) < tol and _rel(ig, ir) < tol and _rel(sg, sr) < tol, (arith, _rel(xg, xr), _rel(ig, ir), _rel(sg, sr))
        finally:
            hip_plugin.conv_arithmetic('default')


def test_group_outputs_at_its_own_boundary(gpu_device):
    """What leaves the group (x in front of the next block / conv0's output inside it, the skip images) against the per-layer path cut at the
    same place — a whole-backbone tolerance would hide an O(1) error of a sub-stage behind later layers."""
    from training import networks
    C, w_dim = 512, 64
    for n, nblocks in ((1, 5), (4, 4)):
        blocks = _blocks(C, nblocks, w_dim, gpu_device, seed=1)
        ws = torch.randn([n, sum(b.num_conv for b in blocks) + 1, w_dim], device=gpu_device)
        ws_list = _split(blocks, ws)
        _, _, _, info = _run(blocks, ws_list, True)
        start, resume, xg, ig, sg = info
        assert start >= 2
        os.environ['IDE3D_NO_LOWRES_GROUP'] = '1'
        try:
            with torch.no_grad():
                x = img = seg = None
                for i in range(start):
                    x, img, seg = blocks[i](x, img, ws_list[i], condition_img=seg, noise_mode='const')
                if resume:
                    x = blocks[start].conv0(x, ws_list[start][:, 0], noise_mode='const')
        finally:
            os.environ.pop('IDE3D_NO_LOWRES_GROUP')
        assert xg.shape == x.shape and ig.shape == img.shape and sg.shape == seg.shape
        assert _rel(xg, x) < 5e-6 and _rel(ig, img) < 5e-6 and _rel(sg, seg) < 5e-6, (n, _rel(xg, x), _rel(ig, img), _rel(sg, seg))


def test_group_against_float64_definition(gpu_device):
    """The blocks' mathematics in float64 (modulate, 3x3 conv / transposed conv + FIR, demodulate, noise, bias, lrelu, heads, skip up-sampling)."""
    C, w_dim, n = 64, 32, 1          # (batch 1: all three blocks fit the group)
    blocks = _blocks(C, 3, w_dim, gpu_device, seed=2)
    ws = torch.randn([n, sum(b.num_conv for b in blocks) + 1, w_dim], device=gpu_device)
    ws_list = _split(blocks, ws)
    xg, ig, sg, info = _run(blocks, ws_list, True)
    assert info is not None and info[0] == 3
    x, img, seg = _blocks64(blocks, ws_list)
    assert _rel(xg, x) < 4e-6 and _rel(ig, img) < 4e-6 and _rel(sg, seg) < 4e-6, (_rel(xg, x), _rel(ig, img), _rel(sg, seg))


def test_backbone_uses_the_group_and_replays_bit_equal(gpu_device):
    """Full-size backbone: the group launch is taken (batch 1 and 4), agrees with the per-layer path, and a hipGraph replay of it is bit-equal
    to the eager launches."""
    from torch_utils import hip_plugin
    from training import triplane, graph_cache
    torch.manual_seed(0)
    G = triplane.TriPlaneGenerator().eval().requires_grad_(False).to(gpu_device)
    syn = G.synthesis
    for n in (1, 4):
        ws = torch.randn([n, G.num_ws, G.w_dim], device=gpu_device)
        try:
            graph_cache.reset(syn)
            graph_cache.STATS.clear()
            before = hip_plugin.CALLS.get('lowres_group', 0)
            with graph_cache.disabled():
                a = syn.planes(ws)
            assert hip_plugin.CALLS.get('lowres_group', 0) == before + 1
            os.environ['IDE3D_NO_LOWRES_GROUP'] = '1'
            with graph_cache.disabled():
                b = syn.planes(ws)
            os.environ.pop('IDE3D_NO_LOWRES_GROUP')
            for u, v in zip(a, b):
                assert _rel(u, v) < 1e-5
            outs = [syn.planes(ws) for _ in range(4)]          # eager, capture, replay, replay
            assert graph_cache.STATS['replay'] >= 2
            for o in outs:
                for u, v in zip(o, a):
                    assert torch.equal(u, v)
        finally:
            os.environ.pop('IDE3D_NO_LOWRES_GROUP', None)


def test_hooks_and_other_arithmetics_keep_the_per_layer_path(gpu_device):
    from torch_utils import hip_plugin
    from training import networks
    blocks = _blocks(64, 2, 32, gpu_device)
    ws_list = _split(blocks, torch.randn([1, 4, 32], device=gpu_device))
    with torch.no_grad():
        assert networks.lowres_group_forward(blocks, ws_list, noise_mode='const') is not None
        assert networks.lowres_group_forward(blocks, ws_list, noise_mode='random') is None
        h = blocks[1].conv0.register_forward_hook(lambda m, i, o: None)
        got = networks.lowres_group_forward(blocks, ws_list, noise_mode='const')
        h.remove()
        assert got is None or got[3] == 1          # the hooked block stays out of the group
        try:
            hip_plugin.conv_arithmetic('fp32')
            assert networks.lowres_group_forward(blocks, ws_list, noise_mode='const') is None
        finally:
            hip_plugin.conv_arithmetic('default')


# ---- the group at its edges against the float64 definition ---------------------------------------------------------------------------

def _stop_of(fit):
    """(next block, resume) after the first `fit` layers of [b0.conv1, b1.conv0, b1.conv1, b2.conv0, ...]"""
    bi, conv0 = fit // 2, fit % 2 == 0
    return (bi, True) if conv0 else (bi + 1, False)


def _group_twice(run):
    """run() twice: the group sums in a fixed order, so two launches on the same inputs must be bit-equal"""
    from torch_utils import hip_plugin
    before = hip_plugin.CALLS.get('lowres_group', 0)
    a, b = run(), run()
    assert hip_plugin.CALLS.get('lowres_group', 0) == before + 2, 'the group launch did not run'
    for u, v in zip(a, b):
        assert torch.equal(u, v), 'two runs of the group differ'
    assert hip_plugin.exclusive_violations() == (0, '')
    return a


_SERIES = [dict(C=512, nblocks=4, n=n) for n in range(1, 9)]                                           # the benchmark's width, n = 4 its batch
_SERIES += [dict(C=512, nblocks=4, n=n, arith='bf16x3') for n in (1, 2, 3)]                            # n = 2: up@32 with two images
_SERIES += [dict(C=32, nblocks=3, n=2), dict(C=96, nblocks=3, n=3), dict(C=1024, nblocks=4, n=1)]      # one slab; CB = S = 3; 32 slabs
_SERIES += [dict(C=64, nblocks=3, n=2, img=3, seg=19), dict(C=512, nblocks=4, n=4, img=96, seg=96), dict(C=64, nblocks=3, n=3, img=3, seg=2)]
_SERIES += [dict(C=128, nblocks=3, n=2, clamp=0.6), dict(C=512, nblocks=4, n=2, clamp=0.6), dict(C=64, nblocks=3, n=3, noise_mode='none')]
_SERIES += [dict(C=64, nblocks=3, n=2, adversarial=True), dict(C=512, nblocks=4, n=1, adversarial=True)]


def _case_id(c):
    return '-'.join(f'{k}{v}' if not isinstance(v, bool) else k for k, v in c.items())


@pytest.mark.parametrize('case', _SERIES, ids=[_case_id(c) for c in _SERIES])
def test_group_edges_against_float64(gpu_device, case):
    """x, img and seg where the group stops — at the stop point `ide3d_lowres_layers_supported` gives for the case — against the float64
    definition.  Run twice, bit-equal run to run."""
    from torch_utils import hip_plugin
    from training import networks
    C, nblocks, n = case['C'], case['nblocks'], case['n']
    arith, clamp, noise_mode = case.get('arith', 'bf16x6'), case.get('clamp'), case.get('noise_mode', 'const')
    w_dim = 64
    blocks = _blocks(C, nblocks, w_dim, gpu_device, img_ch=case.get('img', 12), seg_ch=case.get('seg', 8), conv_clamp=clamp, seed=C + n)
    if case.get('adversarial'):
        # styles 2^k per input channel, k over [-21, 21]: the group's activations x styles span 40+ octaves in every layer
        g = torch.Generator().manual_seed(C + n)
        for b in blocks:
            for lay in ([b.conv1] if b.in_channels == 0 else [b.conv0, b.conv1]):
                k = torch.randint(-21, 22, (C,), generator=g)
                k[:2] = torch.tensor([-21, 21])
                sign = torch.randint(0, 2, (C,), generator=g) * 2 - 1
                lay.affine.weight.data.mul_(2.0 ** -24)
                lay.affine.bias.data.copy_((sign * 2.0 ** k.double() * (1 + 0.25 * torch.rand(C, generator=g, dtype=torch.float64))).float())
    ws_list = _split(blocks, torch.randn([n, sum(b.num_conv for b in blocks) + 1, w_dim], device=gpu_device))
    ups = [1] + [2, 1] * (nblocks - 1)
    fit = hip_plugin.LowresPlugin.layers_supported(n, C, 4, ups, 6 if arith == 'bf16x6' else 3)
    want_stop = _stop_of(fit)
    if C == 512 and nblocks == 4:          # tests/test_plan_cpu.py::test_lowres_group_extent_by_batch_size
        assert want_stop == ((3, True) if n == 1 or (n == 2 and arith == 'bf16x3') else (2, True) if n <= 5 or arith == 'bf16x3' else (1, True))

    def run():
        with torch.no_grad():
            grp = networks.lowres_group_forward(blocks, ws_list, noise_mode=noise_mode)
        assert grp is not None
        assert grp[3:] == want_stop, (grp[3:], want_stop)
        return grp[:3]
    hip_plugin.conv_arithmetic(arith)
    try:
        xg, ig, sg = _group_twice(run)
    finally:
        hip_plugin.conv_arithmetic('default')
    with torch.no_grad():
        x, img, seg = _blocks64(blocks, ws_list, want_stop, noise_mode=noise_mode)
    assert xg.shape == x.shape and ig.shape == img.shape and sg.shape == seg.shape
    if clamp is not None:
        assert float(xg.abs().max()) <= float(np.float32(clamp)) and float((x.abs() == clamp).double().mean()) > 0.01          # the clamp bites
    if case.get('adversarial'):
        s = _styles64(blocks[1].conv1.affine, ws_list[1][:, 1]).abs()
        assert float((s.max() / s.min()).log2()) >= 40
    tol = 2e-4 if arith == 'bf16x3' else 4e-6 if C <= 128 else 1e-5
    errs = (_rel(xg, x), _rel(ig, img), _rel(sg, seg))
    print(f'lowres-f64 {_case_id(case)} stop={want_stop} x={errs[0]:.2e} img={errs[1]:.2e} seg={errs[2]:.2e} bound={tol:.0e}')
    assert max(errs) < tol, errs


def _abi_layer(lay, w, head=-1):
    """an ide3d_lowres_layer's inputs, formed in fp32 torch operations from the module (styles, demodulation, noise x strength)"""
    s = w @ (lay.affine.weight * lay.affine.weight_gain).t() + lay.affine.bias * lay.affine.bias_gain
    d = ((lay.weight[None] * s[:, None, :, None, None]).square().sum(dim=[2, 3, 4]) + 1e-8).rsqrt()
    return dict(weight=lay.weight, styles=s, dcoefs=d, noise=lay.noise_const * lay.noise_strength, bias=lay.bias, act_gain=lay.act_gain,
                clamp=-1.0 if lay.conv_clamp is None else lay.conv_clamp, up=lay.up, head=head)


def _abi_heads(b, w):
    ts = [t.weight[None, :, :, 0, 0] * ((w @ (t.affine.weight * t.affine.weight_gain).t() + t.affine.bias * t.affine.bias_gain) * t.weight_gain)[:, None]
          for t in (b.torgb, b.toseg)]
    return dict(w=torch.cat(ts, dim=1).contiguous(), bias=torch.cat([b.torgb.bias, b.toseg.bias]), clamp=-1.0)


@pytest.mark.parametrize('n,arith', [(1, 'bf16x6'), (2, 'bf16x3')])
def test_group_with_a_per_image_input_through_the_abi(gpu_device, n, arith):
    """x0 given per image (x0_batch_stride != 0) at res0 = 8, layers up = [1, 2, 1] with a head after the first and the last: the group's input is
    not the learned constant, and the second head adds the first one's up-sampled skip.  (conv1@16 reads n x 18^2 slots: two images fit LDS in
    bf16x3 only.)"""
    from torch_utils import hip_plugin
    C, w_dim = 64, 32
    blocks = _blocks(C, 2, w_dim, gpu_device, img_ch=3, seg_ch=19, seed=7, res0=8)
    ws_list = _split(blocks, torch.randn([n, 4, w_dim], device=gpu_device))
    x0 = torch.randn([n, C, 8, 8], device=gpu_device)
    b0, b1 = blocks
    with torch.no_grad():
        layers = [_abi_layer(b0.conv1, ws_list[0][:, 0], 0), _abi_layer(b1.conv0, ws_list[1][:, 0]), _abi_layer(b1.conv1, ws_list[1][:, 1], 1)]
        heads = [_abi_heads(b0, ws_list[0][:, 1]), _abi_heads(b1, ws_list[1][:, 2])]
        assert hip_plugin.LowresPlugin.layers_supported(n, C, 8, [1, 2, 1], 6 if arith == 'bf16x6' else 3) == 3
        hip_plugin.conv_arithmetic(arith)
        try:
            xg, k0, k1 = _group_twice(lambda: _flat(hip_plugin.LowresPlugin.group(x0, layers, heads, b0.resample_filter)))
        finally:
            hip_plugin.conv_arithmetic('default')
        x, img, seg = _blocks64(blocks, ws_list, x0=x0)
        _, img0, seg0 = _blocks64(blocks, ws_list, (1, False), x0=x0)
    errs = (_rel(xg, x), _rel(k1, torch.cat([img, seg], 1)), _rel(k0, torch.cat([img0, seg0], 1)))
    tol = 4e-6 if arith == 'bf16x6' else 2e-4
    print(f'lowres-f64 abi-per-image-x0 n{n}-{arith} x={errs[0]:.2e} skip1={errs[1]:.2e} skip0={errs[2]:.2e} bound={tol:.0e}')
    assert max(errs) < tol, errs


def _flat(out):
    x, skips = out
    return (x, *skips)


# ---- gradients: the group and the per-layer fast paths read parameters by pointer, so they must step aside for anything trainable ---------

_TRAINABLE = {
    'conv_affine': lambda bl, ws: list(bl[1].conv1.affine.parameters()),
    'noise_strength': lambda bl, ws: [bl[0].conv1.noise_strength],
    'torgb_affine': lambda bl, ws: list(bl[1].torgb.affine.parameters()),
    'toseg_bias': lambda bl, ws: [bl[1].toseg.bias],
    'later_block_ws': lambda bl, ws: [ws[2]],
}


def _backbone_like(blocks, ws_list):
    """training/triplane.py `backbone`: the group where it applies, then the blocks from where it stopped"""
    from training import networks
    x = img = seg = None
    start, resume = 0, False
    grp = networks.lowres_group_forward(blocks, ws_list, noise_mode='const')
    if grp is not None:
        x, img, seg, start, resume = grp
    for i, (b, w) in enumerate(zip(blocks, ws_list)):
        if i < start:
            continue
        extra = dict(_resume_after_conv0=True) if (resume and i == start) else {}
        x, img, seg = b(x, img, w, condition_img=seg, noise_mode='const', **extra)
    return x, img, seg, (None if grp is None else grp[3:])


def _grad_case(gpu_device, C, nblocks, n, pick, seed):
    """-> (stop of the group or None, gradients on the GPU, gradients of the float64 definition on a CPU copy)"""
    import copy
    blocks = _blocks(C, nblocks, 32, gpu_device, seed=seed)
    ws = torch.randn([n, sum(b.num_conv for b in blocks) + 1, 32], device=gpu_device)
    ws_list = [w.clone() for w in _split(blocks, ws)]          # separate tensors: one block's ws can be made trainable alone
    cpu_blocks = [copy.deepcopy(b).cpu().double() for b in blocks]
    cpu_ws = [w.detach().cpu().double() for w in ws_list]
    params, cpu_params = pick(blocks, ws_list), pick(cpu_blocks, cpu_ws)
    for p in params + cpu_params:
        p.requires_grad_(True)
    g = torch.Generator().manual_seed(seed)
    x, img, seg, stop = _backbone_like(blocks, ws_list)
    proj = [torch.randn(t.shape, generator=g, dtype=torch.float64) for t in (x, img, seg)]
    loss = sum((t * p.to(gpu_device, torch.float32)).sum() for t, p in zip((x, img, seg), proj))
    got = [g_.cpu() for g_ in torch.autograd.grad(loss, params)]
    x6, img6, seg6 = _blocks64(cpu_blocks, cpu_ws)
    want = torch.autograd.grad(sum((t * p).sum() for t, p in zip((x6, img6, seg6), proj)), cpu_params)
    return stop, got, want


@pytest.mark.parametrize('what', list(_TRAINABLE))
def test_trainable_block_parameters_are_differentiated(gpu_device, what):
    """Everything frozen but one affine, one noise strength, a head's affine, a head's bias, or the ws of a later block (a tensor of its own):
    the group ends in front of the block that owns it (block 0 for the noise strength: no group), the per-layer fast paths decline, and the
    gradients equal those of the float64 definition run on a CPU copy."""
    stop, got, want = _grad_case(gpu_device, 64, 3, 2, _TRAINABLE[what], seed=11)
    assert stop == (None if what == 'noise_strength' else (2, False) if what == 'later_block_ws' else (1, False)), stop
    for a, b in zip(got, want):
        assert a is not None and a.shape == b.shape
        print(f'lowres-grad {what} rel={_rel(a, b):.2e} bound=1e-04')
        assert _rel(a, b) < 1e-4, (what, _rel(a, b))


def test_group_runs_when_only_a_block_after_it_is_trainable(gpu_device):
    """Control: at batch 4 the group covers conv1@4 .. up@16 (4 layers); trainable heads of block 3 (32^2) leave it where it is.  (Heads: no lrelu
    between them and the outputs, whose kink would turn fp32-sized differences of a pre-activation near 0 into O(1 / sqrt(pixels)) gradient
    differences.)"""
    from torch_utils import hip_plugin
    before = hip_plugin.CALLS.get('lowres_group', 0)
    stop, got, want = _grad_case(gpu_device, 64, 4, 4, lambda bl, ws: [bl[3].torgb.bias, *bl[3].toseg.affine.parameters()], seed=12)
    assert stop == (2, True) and hip_plugin.CALLS.get('lowres_group', 0) == before + 1
    for a, b in zip(got, want):
        print(f'lowres-grad control rel={_rel(a, b):.2e} bound=1e-04')
        assert _rel(a, b) < 1e-4, _rel(a, b)


@pytest.mark.parametrize('n,C,arith', [(2, 2080, 'bf16x3'), (1, 4128, 'bf16x6')])
def test_wide_up_layer_whose_fill_rule_band_would_overflow_lds(gpu_device, n, C, arith):
    """One up-sampling layer 16^2 -> 32^2 at the narrowest widths where n x C / 32 > 128 gives phase R 2 bands of 16 rows: their scratch (146,048 B)
    would not fit behind the weight slice (126,976 B in bf16x3, 108,544 B in bf16x6), so the layer runs 3 bands (107,392 B).  Per-image x0,
    against the float64 definition."""
    from torch_utils import hip_plugin
    from training import networks
    assert hip_plugin.LowresPlugin.phase_r_plan(n, C, 16, [2], 3 if arith == 'bf16x3' else 6) == [(3, 107392)]
    torch.manual_seed(C)
    lay = networks.SynthesisLayer(C, C, 32, resolution=32, up=2).eval().requires_grad_(False)
    lay.noise_strength.data.fill_(0.37)
    lay.bias.data.normal_(0, 0.3)
    lay = lay.to(gpu_device)
    w = torch.randn([n, 32], device=gpu_device)
    x0 = torch.randn([n, C, 16, 16], device=gpu_device)
    with torch.no_grad():
        layers = [_abi_layer(lay, w)]
        x64 = _layer64(lay, x0, w)
        hip_plugin.conv_arithmetic(arith)
        try:
            (xg,) = _group_twice(lambda: _flat(hip_plugin.LowresPlugin.group(x0, layers, [], lay.resample_filter)))
        finally:
            hip_plugin.conv_arithmetic('default')
    tol = 2e-4 if arith == 'bf16x3' else 1e-5
    print(f'lowres-f64 wide-up n{n}-C{C}-{arith} x={_rel(xg, x64):.2e} bound={tol:.0e}')
    assert _rel(xg, x64) < tol, _rel(xg, x64)
