"""The synthesis blocks in float64 (reference semantics: inversion/networks.py:330-514 SynthesisLayer, :670-713 ToRGBLayer, :966-1139
SegSynthesisBlock; conv2d_resample.py:112-129; upfirdn2d.py:313-349): plain torch operations on the modules' device, differentiable (the
gradient tests run it on a float64 CPU copy of the blocks).  None of the product's code paths is used: only the modules' parameters, buffers
and constructor attributes are read.

Every function takes `dtype` (default float64).  With `dtype=torch.float32` the same definition runs in ATen float32 arithmetic: its distance
from the float64 run is what float32 rounding alone costs on a case, the yardstick the GPU tests fall back on where a starting bound is missed."""

import torch
import torch.nn.functional as F

F64 = torch.float64


def styles64(aff, w, dtype=F64):
    return (w.to(dtype) @ aff.weight.to(dtype).t()) * aff.weight_gain + aff.bias.to(dtype) * aff.bias_gain


def clamp64(y, clamp):
    return y if clamp is None else y.clamp(-clamp, clamp)


def fir64(x, f, gain):
    """true 2-D convolution of the (already padded) x with the 4x4 filter f, times gain: out[y, x] = sum_ab x[y + a, x + b] f[3 - a, 3 - b]"""
    f = f.to(x.dtype) * gain
    h, w = x.shape[-2] - 3, x.shape[-1] - 3
    out = 0
    for a in range(4):
        for b in range(4):
            out = out + x[..., a:a + h, b:b + w] * f[3 - a, 3 - b]
    return out


def up2_f64(x, f):
    """upsample2d(x, f) (upfirdn2d.py:313-349) in x's dtype: zero insertion x 2, pad (2, 1), true convolution with f, gain 4"""
    n, c, h, w = x.shape
    xu = torch.zeros([n, c, 2 * h, 2 * w], dtype=x.dtype, device=x.device)
    xu[:, :, ::2, ::2] = x
    return fir64(F.pad(xu, [2, 1, 2, 1]), f, 4)


def bilinear_up2_64(x, dtype=F64):
    """the entrance of `superres`: F.interpolate(scale 2, bilinear, align_corners=False)"""
    return F.interpolate(x.to(dtype), scale_factor=2, mode='bilinear', align_corners=False)


def layer64(lay, x, w, noise_mode='const', gain=1, input_noise=None, dtype=F64):
    """SynthesisLayer: styles, weights modulated and demodulated per image, 3x3 conv (up = 1) or stride-2 transposed conv + pad 1 + 4x4 FIR x 4
    (up = 2); noise x strength (`input_noise` [n, 1, H, W] when given, else the constant map, tiled along the width where it is narrower than
    the output: inversion/networks.py:451-456), bias, lrelu 0.2, act gain x gain, conv clamp x gain"""
    assert noise_mode in ('const', 'none'), 'random noise has no definition to compare with'
    s = styles64(lay.affine, w, dtype)
    wm = lay.weight.to(dtype)[None] * s[:, None, :, None, None]
    wm = wm * (wm.square().sum(dim=[2, 3, 4]) + 1e-8).rsqrt()[:, :, None, None, None]
    x = x.to(dtype)
    ys = []
    for i in range(x.shape[0]):
        if lay.up == 2:
            y = F.conv_transpose2d(x[i:i + 1], wm[i].transpose(0, 1), stride=2)
            ys.append(fir64(F.pad(y, [1, 1, 1, 1]), lay.resample_filter, 4))
        else:
            ys.append(F.conv2d(x[i:i + 1], wm[i], padding=1))
    y = torch.cat(ys)
    if lay.use_noise and input_noise is not None:
        y = y + input_noise.to(dtype) * lay.noise_strength.to(dtype)
    elif lay.use_noise and noise_mode == 'const':
        noise = lay.noise_const.to(dtype) * lay.noise_strength.to(dtype)
        if noise.shape[-1] < y.shape[-1]:
            assert y.shape[-1] % noise.shape[-1] == 0
            noise = noise.repeat(1, y.shape[-1] // noise.shape[-1])
        y = y + noise
    y = F.leaky_relu(y + lay.bias.to(dtype)[None, :, None, None], 0.2) * (lay.act_gain * gain)
    return clamp64(y, None if lay.conv_clamp is None else lay.conv_clamp * gain)


def head64(t, x, w, dtype=F64):
    """ToRGBLayer: 1x1 modulated conv without demodulation, bias, conv clamp"""
    s = styles64(t.affine, w, dtype) * t.weight_gain
    y = torch.einsum('oc,nc,nchw->nohw', t.weight.to(dtype)[:, :, 0, 0], s, x.to(dtype)) + t.bias.to(dtype)[None, :, None, None]
    return clamp64(y, t.conv_clamp)


def block64(b, x, img, seg, ws, noise_mode='const', gain=1, block_noise=None, x0=None, resume_after_conv0=False, only_conv0=False, dtype=F64):
    """One SegSynthesisBlock from given inputs: (x, img, seg, ws [n, num_conv + num_torgb, w_dim]) -> (x, img, seg).  x is ignored by a block
    that starts at its constant (`x0`: a per-image input in its place); img / seg None: no skip images yet.  Heads: 'skip' blocks and `is_last`
    blocks of either architecture.  `resume_after_conv0`: x already is conv0's output; `only_conv0`: -> (conv0's output, img, seg) unchanged.
    block_noise [n, 2, H, W]: channel 0 is conv0's noise, channel 1 conv1's (in place of the constant maps)."""
    kw = dict(noise_mode=noise_mode, gain=gain, dtype=dtype)
    if b.in_channels == 0:
        x = x0.to(dtype) if x0 is not None else b.const.to(dtype)[None].expand(ws.shape[0], -1, -1, -1)
    else:
        if not resume_after_conv0:
            x = layer64(b.conv0, x, ws[:, 0], input_noise=(None if block_noise is None else block_noise[:, 0:1]), **kw)
        if only_conv0:
            return x, img, seg
    x = x.to(dtype)
    if not b.use_single_layer:
        x = layer64(b.conv1, x, ws[:, b.num_conv - 1], input_noise=(None if block_noise is None else block_noise[:, 1:2]), **kw)
    if b.is_last or b.architecture == 'skip':
        wh = ws[:, b.num_conv]
        yi, ys = head64(b.torgb, x, wh, dtype), head64(b.toseg, x, wh, dtype)
        if img is not None:
            up = img.shape[-1] * 2 == x.shape[-1]
            assert up or img.shape[-1] == x.shape[-1]
            img, seg = img.to(dtype), seg.to(dtype)
            img, seg = ((up2_f64(img, b.resample_filter), up2_f64(seg, b.resample_filter)) if up else (img, seg))
            img, seg = img + yi, seg + ys
        else:
            img, seg = yi, ys
    return x, img, seg


def blocks64(blocks, ws_list, stop=None, x0=None, noise_mode='const', dtype=F64, **block_kwargs):
    """-> (x, img, seg) in float64 at `stop` = (next block, resume) (None: after all blocks): x in front of blocks[next block], or that block's
    conv0 output when resume; img / seg after the last complete block.  x0: a per-image input [n, C, r, r] of blocks[0] in place of its constant."""
    nb, resume = stop if stop is not None else (len(blocks), False)
    x = img = seg = None
    for bi, (b, w) in enumerate(zip(blocks, ws_list)):
        if bi > nb or (bi == nb and not resume):
            break
        x, img, seg = block64(b, x, img, seg, w, noise_mode=noise_mode, x0=(x0 if bi == 0 else None), only_conv0=(bi == nb), dtype=dtype,
                              **block_kwargs)
    return x, img, seg


def backbone64(syn, voxel_ws, noise_mode='const', dtype=F64):
    """TriplaneSynthesisNetwork.backbone: ws slices -> (texture tri-plane, semantic tri-plane)"""
    _, img, seg = blocks64([getattr(syn, f'vb{r}') for r in syn.voxel_block_resolutions], voxel_ws, noise_mode=noise_mode, dtype=dtype)
    return img, seg


def superres64(syn, feat, block_ws, noise_mode='const', dtype=F64):
    """TriplaneSynthesisNetwork.superres: composited features [n, feature_channels + seg_channels, r, r] -> (img, seg): bilinear x 2 of the
    features (x), of their first img_channels (img) and of the semantic channels (seg), then the super-resolution blocks"""
    fc = syn.spec.feature_channels
    up = bilinear_up2_64(feat, dtype)
    x, img, seg = up[:, :fc], up[:, :syn.img_channels], up[:, fc:]
    for r, w in zip(syn.block_resolutions, block_ws):
        x, img, seg = block64(getattr(syn, f'b{r}'), x, img, seg, w, noise_mode=noise_mode, dtype=dtype)
    return img, seg
