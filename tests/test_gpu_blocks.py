"""The blocks past the low-resolution group — the remaining tri-plane blocks and the super-resolution blocks, run layer by layer through
`SegSynthesisBlock.forward` (training/networks.py) — driven as the generator drives them and compared after EVERY block with the float64
definition of tests/blocks64.py (pinned to the reference's own run by tests/test_oracle_golden.py, without a GPU).

What is under test is the glue between the kernels: `act_gain * gain` and `conv_clamp * gain`, the cached noise product and demodulation
coefficients, prefetched styles, pitched outputs handed to the FIR epilogue, deferred and merged skip images, `skip_channels_last`, `_x_unused`,
`_resume_after_conv0`, fp16-storage blocks, and the decline path of `_conv1_dual_head`.  Each case asserts by launch counter
(`hip_plugin.CALLS`) or output property that the route it is about really ran.

Error measure: max |error| over max |float64 value| per tensor.  Bounds (the project's own for block chains of this depth): 4e-6 up to 128
channels, 1e-5 above (512), 2e-4 in bf16x3; f16x3 and fp32 take the bound of bf16x6.  A case that misses its bound also reports what the same
definition run in ATen float32 loses against float64 on that case (`f32def`): the yardstick for float32 rounding on it."""

import collections
import contextlib
import os

import numpy as np
import pytest
import torch

import blocks64

pytestmark = pytest.mark.gpu

W_DIM = 64
_COUNTED = ('modconv2d', 'modconv2d_heads', 'upfirdn2d', 'skip_upsample_add_cl', 'bias_act', 'style_demod', 'fold_heads', 'style_demod_batch',
            'fold_heads_batch', 'lowres_group', 'bilinear_up2_split')


def _rel(a, b):
    return float((a.double() - b.double()).abs().max() / b.double().abs().max().clamp_min(1e-30))


@contextlib.contextmanager
def _env(**values):
    """environment variables for the duration of a run (None: unset), restored afterwards"""
    old = {k: os.environ.get(k) for k in values}
    try:
        for k, v in values.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _calls():
    from torch_utils import hip_plugin
    return collections.Counter({k: hip_plugin.CALLS.get(k, 0) for k in _COUNTED})


def _delta(before):
    now = _calls()
    return {k: now[k] - before[k] for k in _COUNTED}


def _chain(device, widths, res0, img_ch, seg_ch, conv_clamp=None, seed=0, use_fp16=False, is_last=False, skip_cl=False):
    """blocks widths[i] -> widths[i + 1] at res0 << i, as tests/test_gpu_lowres.py `_blocks` builds them: non-zero noise strength, random biases,
    eval(), frozen.  `is_last` / `skip_cl` go to the last block."""
    from training import triplane
    torch.manual_seed(seed)
    blocks = []
    for i in range(len(widths) - 1):
        last = i == len(widths) - 2
        b = triplane.VoxelBlock(widths[i], widths[i + 1], w_dim=W_DIM, resolution=res0 << i, img_channels=img_ch, seg_channels=seg_ch,
                                is_last=(is_last and last), architecture='skip', conv_clamp=conv_clamp, use_fp16=use_fp16,
                                layer_name='training.networks.SynthesisLayer')
        for lay in (b.conv0, b.conv1):
            lay.noise_strength.data.fill_(0.37)
            lay.bias.data.normal_(0, 0.3)
        b.torgb.bias.data.normal_(0, 0.2)
        b.toseg.bias.data.normal_(0, 0.2)
        if skip_cl and last:
            b.skip_channels_last = True
        blocks.append(b.eval().requires_grad_(False).to(device))
    return blocks


def _split(blocks, ws):
    out, idx = [], 0
    for b in blocks:
        out.append(ws.narrow(1, idx, b.num_conv + b.num_torgb))
        idx += b.num_conv
    return out


def _make_adversarial(blocks, seed):
    """styles 2^k per input channel, k over [-21, 21], on the up-sampling layer and the plain layer of every block (the construction of
    tests/test_gpu_lowres.py::test_group_edges_against_float64)"""
    g = torch.Generator().manual_seed(seed)
    for b in blocks:
        for lay in (b.conv0, b.conv1):
            C = lay.affine.weight.shape[0]
            k = torch.randint(-21, 22, (C,), generator=g)
            k[:2] = torch.tensor([-21, 21])
            sign = torch.randint(0, 2, (C,), generator=g) * 2 - 1
            lay.affine.weight.data.mul_(2.0 ** -24)
            lay.affine.bias.data.copy_((sign * 2.0 ** k.double() * (1 + 0.25 * torch.rand(C, generator=g, dtype=torch.float64))).float())


def _drive(blocks, ws_list, x, img, seg, *, noise_mode='const', gain=None, noises=None, resume=False, x_unused=False, force_fp32=False,
           prefetch=False, arena=False):
    """The blocks as `backbone` / `superres` call them -> [(x, img, seg) in front of block i], [(x, img, seg) after block i]."""
    from training import networks
    ins, outs = [], []
    side = None
    scope = networks.amax_arena(ws_list[0].shape[0], ws_list[0].device) if arena else contextlib.nullcontext()
    with torch.no_grad(), scope:
        try:
            if prefetch:
                side = networks.side_stream(ws_list[0].device)
                networks.prefetch_styles(list(zip(blocks, ws_list)), side)
            for i, (b, w) in enumerate(zip(blocks, ws_list)):
                extra = {}
                if gain is not None:
                    extra['gain'] = gain
                if noises is not None:
                    extra['block_noise'] = noises[i]
                if resume and i == 0:
                    extra['_resume_after_conv0'] = True
                if x_unused and i == len(blocks) - 1:
                    extra['_x_unused'] = True
                if force_fp32:
                    extra['force_fp32'] = True
                ins.append((x, img, seg))
                x, img, seg = b(x, img, w, condition_img=seg, noise_mode=noise_mode, **extra)
                outs.append((x, img, seg))
        finally:
            if side is not None:
                networks.finish_prefetch(side)
    torch.cuda.synchronize()
    return ins, outs


# ---- the series -----------------------------------------------------------------------------------------------------------------------------
# n: batch; w: channel widths along the chain (w[0] is the width of the chain's input x at res / 2); res: resolution of the first block;
# heads: (image, semantic) head widths.  Everything else names the route or edge the case is about.

_SERIES = [
    # shapes: batch 1 / 3 / 4 / 5, widths off the kernels' row and K tiles, the four pairs of head widths
    dict(id='n1-w24-40-72-h3+19', n=1, w=[24, 40, 72], res=32, heads=(3, 19)),
    dict(id='n3-w72-96-96-h12+8-prefetch-nomerge', n=3, w=[72, 96, 96], res=32, heads=(12, 8), variants=('prefetch', 'nomerge')),
    dict(id='n5-w96-96-h3+2-skipcl-declined', n=5, w=[96, 96], res=32, heads=(3, 2), skip_cl=True),
    dict(id='n4-w40-40-h12+8-skipcl', n=4, w=[40, 40], res=32, heads=(12, 8), skip_cl=True),
    dict(id='n1-w96-96-h96+96-skipcl', n=1, w=[96, 96], res=32, heads=(96, 96), skip_cl=True),
    dict(id='n3-w128-64-narrows-is_last', n=3, w=[128, 64], res=64, heads=(3, 19), is_last=True),
    # clamp: bites in the layers and in the heads; then with gain != 1 (conv_clamp * gain, act_gain * gain)
    dict(id='n3-w64-clamp0.6', n=3, w=[64, 64, 64], res=32, heads=(12, 8), clamp=0.6),
    dict(id='n3-w64-clamp0.6-gain0.7', n=3, w=[64, 64, 64], res=32, heads=(12, 8), clamp=0.6, gain=0.7),
    dict(id='n4-w40-72-clamp0.6-gain1.5-h3+19', n=4, w=[40, 72], res=32, heads=(3, 19), clamp=0.6, gain=1.5),
    # noise
    dict(id='n4-w40-noise-none', n=4, w=[40, 40], res=32, heads=(3, 2), noise_mode='none'),
    dict(id='n1-w24-tiled-noise', n=1, w=[24, 24, 24], res=32, heads=(3, 19), tiled=True),
    dict(id='n3-w40-72-block-noise', n=3, w=[40, 72], res=32, heads=(12, 8), block_noise=True),
    # routes
    dict(id='n4-w64-hook-on-conv1', n=4, w=[64, 64], res=32, heads=(12, 8), hook=True),
    dict(id='n3-w72-resume-after-conv0', n=3, w=[72, 72, 40], res=32, heads=(3, 19), resume=True),
    # arithmetics
    dict(id='n3-w72-96-fp32', n=3, w=[72, 96], res=32, heads=(3, 19), arith='fp32'),
    dict(id='n4-w64-f16x3-arena', n=4, w=[64, 64, 64], res=32, heads=(12, 8), arith='f16x3'),
    dict(id='n5-w96-bf16x3', n=5, w=[96, 96], res=32, heads=(3, 2), arith='bf16x3'),
    dict(id='n2-w512-bf16x6', n=2, w=[512, 512], res=32, heads=(96, 96)),
    # fp16-storage blocks (checked block by block from the device's own input), force_fp32 bit-equal to fp32 blocks
    dict(id='n3-w64-fp16-blocks', n=3, w=[64, 64, 64], res=32, heads=(3, 19), clamp=256, fp16=True, variants=('force_fp32',)),
    # adversarial styles on an up-sampling and a plain layer
    dict(id='n3-w64-adversarial', n=3, w=[64, 64], res=32, heads=(12, 8), adversarial=True),
    # the benchmark's widths at batch 4: the last tri-plane block (128 @ 256^2, heads 96 + 96, channels-last tri-planes) and the two
    # super-resolution blocks (32 -> 128 @ 256^2, 128 -> 64 @ 512^2, heads 3 + 19); strip plan, row-parity pairs, resident-weight heads, the
    # heads in the convolution's epilogue.  `x_unused`: x comes back None, img / seg bit-equal; `nofusion`: the decline path, bit-equal
    dict(id='n4-w128-128-r256-h96+96-skipcl', n=4, w=[128, 128], res=256, heads=(96, 96), skip_cl=True, fused=(0,), variants=('x_unused', 'nofusion')),
    dict(id='n4-w32-128-64-r256-r512-h3+19-is_last', n=4, w=[32, 128, 64], res=256, heads=(3, 19), is_last=True, fused=(0, 1),
         variants=('x_unused', 'nofusion')),
    dict(id='n1-w128-64-r512-clamp0.6-gain0.7', n=1, w=[128, 64], res=512, heads=(3, 19), clamp=0.6, gain=0.7, is_last=True, fused=(0,)),
]


def _expected_launches(case, blocks, variant):
    """what the route of the case launches, from reading SegSynthesisBlock.forward: a case that falls back to ATen, or takes another route than
    the one it is about, fails here"""
    e = collections.Counter()
    last = len(blocks) - 1
    fused = set(case.get('fused', ())) if variant != 'nofusion' else set()
    per_call = case.get('block_noise', False)
    off_single_launch = per_call or (case.get('tiled', False) and case.get('noise_mode', 'const') == 'const')
    for i, b in enumerate(blocks):
        if not (case.get('resume') and i == 0):
            e['modconv2d'] += 1                                    # conv0: the transposed convolution ...
            e['upfirdn2d'] += 1                                    # ... and its FIR
            e['style_demod'] += 1
            if per_call:
                e['bias_act'] += 1
        if i in fused:
            e['modconv2d_heads'] += 1                              # conv1 + both heads in one launch
        else:
            e['modconv2d'] += 2                                    # conv1; both heads
        e['style_demod'] += 1
        e['fold_heads'] += 1
        if off_single_launch:
            e['bias_act'] += 1
        c_img, c_seg = case['heads']
        if case.get('skip_cl') and i == last:
            for c in (c_img, c_seg):
                e['skip_upsample_add_cl' if c % 4 == 0 else 'upfirdn2d'] += 1
        elif (case.get('is_last') and i == last) or variant == 'nomerge':
            e['upfirdn2d'] += 2
        else:
            e['upfirdn2d'] += 1                                    # both skip images in one up-sample + add
    if variant == 'prefetch':
        e['style_demod'] = e['fold_heads'] = 0
        e['style_demod_batch'] = e['fold_heads_batch'] = 1
    return e


def _assert_launches(case, blocks, variant, got):
    want = _expected_launches(case, blocks, variant)
    keys = ['modconv2d', 'modconv2d_heads', 'skip_upsample_add_cl', 'bias_act', 'fold_heads', 'style_demod_batch', 'fold_heads_batch', 'lowres_group']
    if not case.get('block_noise'):
        keys.append('upfirdn2d')                                   # (per-call noise: the plain FIR op may take several launches)
    keys.append('style_demod')
    for k in keys:
        assert got[k] == want[k], f'{case["id"]} [{variant}]: {k} launched {got[k]} times, the route of this case makes {want[k]} ({got})'


def _tol(case):
    return 2e-4 if case.get('arith') == 'bf16x3' else 4e-6 if max(case['w']) <= 128 else 1e-5


def _f32def(fn):
    """the figure a missed bound is judged by: the same definition in ATen float32 against its float64 run"""
    with torch.no_grad():
        a, b = fn(torch.float32), fn(torch.float64)
    return tuple(_rel(u, v) for u, v in zip(a, b) if u is not None)


@pytest.mark.parametrize('case', _SERIES, ids=[c['id'] for c in _SERIES])
def test_block_chains_against_float64(gpu_device, case):
    """x, img and seg after every block of a short chain, against the float64 definition run (a) from the chain's inputs and (b) for every
    block from the device's own inputs to that block."""
    from torch_utils import hip_plugin
    from training import networks
    n, widths, res, (c_img, c_seg) = case['n'], case['w'], case['res'], case['heads']
    arith, clamp, gain, noise_mode = case.get('arith', 'bf16x6'), case.get('clamp'), case.get('gain'), case.get('noise_mode', 'const')
    fp16, variants = case.get('fp16', False), case.get('variants', ())
    seed = sum(widths) + n
    build = lambda **kw: _chain(gpu_device, widths, res, c_img, c_seg, conv_clamp=clamp, seed=seed, is_last=case.get('is_last', False),
                                skip_cl=case.get('skip_cl', False), **kw)
    blocks = build(use_fp16=fp16)
    if case.get('adversarial'):
        _make_adversarial(blocks, seed)
    g = torch.Generator().manual_seed(seed)
    rn = lambda *shape: torch.randn(*shape, generator=g).to(gpu_device)
    ws_list = _split(blocks, rn(n, sum(b.num_conv for b in blocks) + 1, W_DIM))
    h0 = res // 2
    w0 = h0 * (2 if case.get('tiled') else 1)                      # tiled: every map twice as wide as the block's noise_const
    x0, both0 = rn(n, widths[0], h0, w0), rn(n, c_img + c_seg, h0, w0)
    img0, seg0 = both0[:, :c_img], both0[:, c_img:]                # channel ranges of one tensor, as the group and `bilinear_up2_split` hand them over
    noises = [rn(n, 2, (res << i), (res << i)) for i in range(len(blocks))] if case.get('block_noise') else None
    kw64 = dict(noise_mode=noise_mode, gain=(1 if gain is None else gain))
    if case.get('resume'):
        # the chain starts inside its first block: x0 becomes the float64 definition's conv0 output, rounded to float32
        with torch.no_grad():
            x0 = blocks64.block64(blocks[0], x0, None, None, ws_list[0], only_conv0=True, **kw64)[0].float()
    hook_calls = []
    hooks = [b.conv1.register_forward_hook(lambda m, i, o: hook_calls.append(m)) for b in blocks] if case.get('hook') else []

    def run(variant=None, chain=blocks):
        env = dict(IDE3D_NO_LOWRES_GROUP='1', IDE3D_NO_SKIP_MERGE=('1' if variant == 'nomerge' else None),
                   IDE3D_MODCONV_NO_HEAD_FUSION=('1' if variant == 'nofusion' else None))
        before = _calls()
        with _env(**env):
            ins, outs = _drive(chain, ws_list, x0, img0, seg0, noise_mode=noise_mode, gain=gain, noises=noises, resume=case.get('resume', False),
                               x_unused=(variant == 'x_unused'), force_fp32=(variant == 'force_fp32'), prefetch=(variant == 'prefetch'),
                               arena=(arith == 'f16x3'))
        return ins, outs, _delta(before)

    hip_plugin.conv_arithmetic(arith)
    try:
        ins, outs, launched = run()
        varied = {v: run(v) for v in variants}
        twin = run(chain=build(use_fp16=False)) if 'force_fp32' in variants else None
    finally:
        hip_plugin.conv_arithmetic('default')
        for h in hooks:
            h.remove()

    # ---- the float64 side: the whole chain from its inputs, and every block from the device's own inputs
    def chain64(dtype):
        x, img, seg = x0, img0, seg0
        res_ = []
        for i, (b, w) in enumerate(zip(blocks, ws_list)):
            x, img, seg = blocks64.block64(b, x, img, seg, w, block_noise=(None if noises is None else noises[i]),
                                           resume_after_conv0=(case.get('resume', False) and i == 0), dtype=dtype, **kw64)
            res_.append((x, img, seg))
        return res_

    def block64_from_device(i, dtype=torch.float64):
        return blocks64.block64(blocks[i], *ins[i], ws_list[i], block_noise=(None if noises is None else noises[i]),
                                resume_after_conv0=(case.get('resume', False) and i == 0), dtype=dtype, **kw64)

    with torch.no_grad():
        want_chain = chain64(torch.float64)
        want_block = [want_chain[0]] + [block64_from_device(i) for i in range(1, len(blocks))]
    tol = _tol(case)
    errs_chain, errs_block = [], []
    for i, (got, wc, wb) in enumerate(zip(outs, want_chain, want_block)):
        for u, v in zip(got, wc):
            assert u.shape == v.shape
        errs_block.append(tuple(_rel(u, v) for u, v in zip(got[1:] if fp16 else got, wb[1:] if fp16 else wb)))
        if not fp16:          # (a one-ulp float16 difference of x is not to be carried through the later blocks of a chain)
            errs_chain.append(tuple(_rel(u, v) for u, v in zip(got, wc)))
    worst = [max(e[j] for e in errs_chain + errs_block) for j in range(len(errs_block[0]))]
    names = ('img', 'seg') if fp16 else ('x', 'img', 'seg')
    line = f'blocks-f64 {case["id"]} ' + ' '.join(f'{k}={v:.2e}' for k, v in zip(names, worst)) + f' bound={tol:.0e}'
    if max(worst) >= tol:
        f32 = _f32def(lambda dt: [t for r in chain64(dt) for t in r])
        line += f' f32def={max(f32):.2e}'
    print(line)
    print(f'blocks-f64 {case["id"]} per block, from the device\'s own inputs: ' + ' | '.join(' '.join(f'{v:.1e}' for v in e) for e in errs_block))
    assert max(worst) < tol, line

    if fp16:
        # derived, not measured: the half-ulp of float16 rounding (2^-11 relative, 2^-25 in the subnormal range) on top of the fp32 chain bound
        for i, (got, wb) in enumerate(zip(outs, want_block)):
            assert got[0].dtype == torch.float16 and got[1].dtype == got[2].dtype == torch.float32
            x64 = wb[0]
            excess = (got[0].double() - x64).abs() - (2.0 ** -11 * x64.abs() + 2.0 ** -25 + tol * x64.abs().max())
            print(f'blocks-f64 {case["id"]} block {i} x16: max excess over the float16 bound {float(excess.max()):.2e} (<= 0 required)')
            assert float(excess.max()) <= 0, (i, float(excess.max()))
        f_ins, f_outs, _ = varied['force_fp32']
        for (a, b_) in zip(f_outs, twin[1]):
            assert a[0].dtype == torch.float32
            for u, v in zip(a, b_):
                assert torch.equal(u, v), 'force_fp32 on fp16 blocks differs from the same blocks built with use_fp16=False'

    # ---- the clamp bites, in the layers and in the heads
    if clamp is not None and not fp16:
        c = clamp * (1 if gain is None else gain)
        for (xg, _, _), (x64, _, _) in zip(outs, want_chain):
            assert float(xg.abs().max()) <= float(np.float32(c)), (float(xg.abs().max()), c)
            assert float((x64.abs() == c).double().mean()) > 0.01, 'the clamp does not bite in the layers'
        with torch.no_grad():
            y = blocks64.head64(blocks[-1].torgb, want_chain[-1][0], ws_list[-1][:, 2])
        assert float((y.abs() == clamp).double().mean()) > 0.001, 'the clamp does not bite in the heads'
    if case.get('adversarial'):
        for lay, col in ((blocks[0].conv0, 0), (blocks[0].conv1, 1)):
            s = blocks64.styles64(lay.affine, ws_list[0][:, col]).abs()
            assert float((s.max() / s.min()).log2()) >= 40

    # ---- the route of the case really ran
    _assert_launches(case, blocks, None, launched)
    xl, il, sl = outs[-1]
    if case.get('hook'):
        assert len(hook_calls) == len(blocks) * (1 + len(variants)), 'the hooked conv1 was not called as a module'
    if case.get('skip_cl'):
        for t, c in ((il, c_img), (sl, c_seg)):
            if c % 4 == 0:
                assert t.is_contiguous(memory_format=torch.channels_last) and t.stride(1) == 1, (t.shape, t.stride())
            else:
                assert t.is_contiguous(), (t.shape, t.stride())      # the channels-last kernel declined: the NCHW route, not a misread
    elif case.get('is_last'):
        assert networks._adjacent_views(il, sl) is None and il.is_contiguous() and sl.is_contiguous()      # the network's outputs: dense tensors of their own
    else:
        assert networks._adjacent_views(il, sl) is not None, 'the merged skip up-sampler did not run'
    if arith == 'f16x3':
        assert networks._amax_of(xl) is not None, 'no amax travelled with the activation: the f16x3 loops cannot have run'

    # ---- variants of the same chain
    for v, (v_ins, v_outs, v_launched) in varied.items():
        _assert_launches(case, blocks, v, v_launched)
        if v == 'force_fp32':
            continue
        for i, (a, b_) in enumerate(zip(v_outs, outs)):
            if v == 'x_unused' and i == len(blocks) - 1:
                assert a[0] is None, '_x_unused: the fused launch still wrote x'
                a, b_ = a[1:], b_[1:]
            if v == 'nomerge':
                # no promise of bit-equality between the one-launch and the two-launch skip up-sampler: the bound, against float64
                assert networks._adjacent_views(a[1], a[2]) is None
                e = tuple(_rel(u, w_) for u, w_ in zip(a, want_chain[i]))
                print(f'blocks-f64 {case["id"]} [nomerge] block {i} ' + ' '.join(f'{x:.2e}' for x in e)
                      + f' bit-equal to merged: {all(torch.equal(u, w_) for u, w_ in zip(a, b_))}')
                assert max(e) < tol, (v, i, e)
            else:
                for u, w_ in zip(a, b_):
                    assert torch.equal(u, w_), f'{case["id"]} [{v}]: block {i} is not bit-equal to the plain run'
    assert hip_plugin.exclusive_violations() == (0, '')


def test_benchmark_width_cases_reach_the_forms_they_are_about():
    """Host-only planner query: the shapes of the three batch-4 / 512^2 cases get the strip plan for their transposed layers, the 16 x 16 x
    128-row (row-parity pair) and 32 x 16 forms, and resident-weight heads."""
    from torch_utils import hip_plugin
    plan = lambda **kw: hip_plugin.modconv_plan(arith=6, **kw)
    up = plan(n=4, cin=128, cout=128, h=128, w=128, mode=2, epilogue='plain')
    assert up['strip'] == 1 and (up['tile_h'], up['tile_w'], up['rows']) == (16, 16, 128)
    up = plan(n=4, cin=128, cout=64, h=256, w=256, mode=2, epilogue='plain')
    assert up['strip'] == 1 and up['workgroups'] == 1024
    assert plan(n=4, cin=64, cout=64, h=512, w=512)['tile_h'] == 32
    for rows, res, c in ((192, 256, 128), (22, 256, 128), (22, 512, 64)):
        assert plan(n=4, cin=c, cout=rows, h=res, w=res, k=1, per_image=True, epilogue='head')['kind'] == 'head_resident'


# ---- whole modules ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('group', [True, False], ids=['group-hand-over', 'no-group'])
def test_backbone_and_superres_against_float64(gpu_device, group):
    """`TriplaneSynthesisNetwork.backbone` and `.superres` of a small spec (five tri-plane blocks 4^2 .. 64^2 of 64 / 64 / 64 / 64 / 32 channels,
    super-resolution blocks 8 -> 64 @ 32^2 and 64 -> 32 @ 64^2) at batch 3.  With the group allowed, the per-layer blocks take over where the group
    stops (widths are multiples of 32: the group takes no others); `superres` starts from a random feature map, so `bilinear_up2_split`'s adjacent
    outputs feed the first block's merged skip up-sampler."""
    from torch_utils import hip_plugin
    from training import triplane
    assert hip_plugin.conv_arithmetic() == 'bf16x6'
    torch.manual_seed(5)
    spec = triplane.tiny_spec(channel_max=64, channel_base=2048, plane_resolution=64)
    syn = triplane.TriplaneSynthesisNetwork(spec)
    for m in syn.modules():
        if hasattr(m, 'noise_strength'):
            m.noise_strength.data.fill_(0.37)
            m.bias.data.normal_(0, 0.3)
        if hasattr(m, 'torgb'):
            m.torgb.bias.data.normal_(0, 0.2)
            m.toseg.bias.data.normal_(0, 0.2)
    syn = syn.eval().requires_grad_(False).to(gpu_device)
    n = 3
    ws = torch.randn([n, syn.num_ws, spec.w_dim], device=gpu_device)
    feat = torch.randn([n, spec.feature_channels + spec.seg_channels, spec.render_size, spec.render_size], device=gpu_device)
    voxel_ws, block_ws = syn.split_ws(ws)
    before = _calls()
    with _env(IDE3D_NO_LOWRES_GROUP=(None if group else '1')), torch.no_grad():
        img_v, seg_v = syn.backbone(voxel_ws, noise_mode='const', force_fp32=False)
        mid = _delta(before)
        img, seg = syn.superres(feat, block_ws, noise_mode='const', force_fp32=False)
    torch.cuda.synchronize()
    launched = _delta(before)
    with torch.no_grad():
        img_v64, seg_v64 = blocks64.backbone64(syn, voxel_ws)
        img64, seg64 = blocks64.superres64(syn, feat, block_ws)
    errs = (_rel(img_v, img_v64), _rel(seg_v, seg_v64), _rel(img, img64), _rel(seg, seg64))
    tol = 4e-6
    tag = 'group' if group else 'no-group'
    line = f'blocks-f64 whole-modules-{tag} img_v={errs[0]:.2e} seg_v={errs[1]:.2e} img={errs[2]:.2e} seg={errs[3]:.2e} bound={tol:.0e}'
    if max(errs) >= tol:
        f32 = _f32def(lambda dt: [*blocks64.backbone64(syn, voxel_ws, dtype=dt), *blocks64.superres64(syn, feat, block_ws, dtype=dt)])
        line += f' f32def={max(f32):.2e}'
    print(line)
    assert max(errs) < tol, line
    # routes: the group ran (or did not) and handed over to per-layer blocks; tri-planes channels-last from the fused skip kernel; the entrance of
    # superres in one launch, its first block's skip images in one up-sample + add, the last block's as dense tensors of their own
    assert mid['lowres_group'] == (1 if group else 0)
    assert mid['modconv2d'] > 0 and mid['skip_upsample_add_cl'] == 2
    for t in (img_v, seg_v):
        assert t.is_contiguous(memory_format=torch.channels_last) and t.shape == (n, 3 * spec.plane_channels, 64, 64)
    assert launched['bilinear_up2_split'] == 1
    assert launched['upfirdn2d'] - mid['upfirdn2d'] == 2 + 1 + 2          # two FIRs of conv0, one merged skip launch, two of the last block
    assert img.shape == (n, 3, 64, 64) and seg.shape == (n, spec.seg_channels, 64, 64) and img.is_contiguous() and seg.is_contiguous()
    assert hip_plugin.exclusive_violations() == (0, '')
