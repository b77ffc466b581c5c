"""The face parser's cross-entropy loss with a HIP forward and image gradient.

Reference: the one term that keeps a re-rendered image's semantic mask on the target's mask in the hybrid encoder's training and per-image
fine-tuning (apps/train_hybrid_encoder.py:279-283, 324-328, apps/finetune_hybrid_encoder.py:170-174):

    _, seg = parsing_img(bisNet, img, argmax=False, return_mask=False, with_grad=True, remap=False)        # the parser's logits
    loss = torch.nn.CrossEntropyLoss()(seg, target)                                                        # target: int64 parser class ids

i.e. the mean over N H W of logsumexp_c(logits) - logits[target], back-propagated through the frozen BiSeNet (training/face_parsing.py) into
the image.  `cross_entropy(bisNet, img, target)` is that value; `labels(bisNet, img)` gives the parser's own class ids (what the apps
compute for the target image); `parse_distance(...)` is the closure `training.projection.project(distance=...)` takes.

`fused` (module switch): float32 CUDA images, a `face_parsing.BiSeNet` in eval mode whose parameters are all frozen, and an image whose
sides are multiples of 32 and at least 64 run on the HIP path: one autograd Function whose forward launches the 32 convolutions exactly as
`face_parsing.conv_bn_act` does in inference (ide3d_modconv2d on BatchNorm-folded weights, ReLU fused) with the passes of
csrc/parse_loss.hip between them, and whose backward launches 31 x ide3d_modconv2d on derived weights (stride 1: transposed and flipped,
mode 0; 3x3 stride 2: transposed, mode 2, cropped; 1x1 stride 2: transposed, at half resolution), the direct stem gradient, 10 x
ide3d_modconv_act_backward and the same passes' adjoints; it returns the image gradient only.  Everything else - CPU tensors, trainable
parameters, other sizes, `fused = False` - is the plain PyTorch definition through the unchanged `BiSeNet.forward`.
`arith` (module switch): the per-call arithmetic of the convolutions on the HIP path (0 = the process default, see
`hip_plugin.conv_arithmetic`).
"""

import torch
import torch.nn.functional as F
from torch.autograd.function import once_differentiable

from training import face_parsing, networks

# True: what the HIP path takes (see above) runs on it.  False: always the PyTorch definition.  Shipped value: see DESIGN.md section 5.16.
fused = True
arith = 0


# ---- the fused pass, written against an `ops` object: `_HipOps` here, a float64 torch restatement in tests/parse_loss_ref.py -----------------
class _HipOps:
    """The launches of the fused pass.  conv: [n, cin, h, w] x folded weights -> ide3d_modconv2d; everything else: csrc/parse_loss.hip."""

    _instance = None

    @classmethod
    def get(cls):
        if cls._instance is None:
            cls._instance = cls()
        return cls._instance

    def __init__(self):
        from torch_utils import hip_plugin
        self.P = hip_plugin.ParseLossPlugin
        self.resize, self.resize_backward = self.P.resize, self.P.resize_backward
        self.ce, self.ce_backward = self.P.ce, self.P.ce_backward
        self.maxpool, self.maxpool_backward = self.P.maxpool, self.P.maxpool_backward
        self.join, self.plane_sums, self.stem_backward = self.P.join, self.P.plane_sums, self.P.stem_backward
        self.relu_backward = networks.relu_backward

    @staticmethod
    def conv(x, w, bias, relu, mode=0):
        return networks.plain_conv(x, w, bias, relu, mode, arith)


def _conv(ops, x, conv, bn=None, relu=False):
    """relu?(bn?(conv(x))) as `face_parsing.conv_bn_act` launches it: folded weights; 3x3 stride 2 = explicit padding + the kernel's stride-2
    mode, 1x1 stride 2 on the decimated input, the 7x7 stem as a 1x1 convolution over its unfolded patches."""
    w, b = face_parsing._folded(conv, bn)
    k, s, p = conv.kernel_size[0], conv.stride[0], conv.padding[0]
    mode = 0
    if (k, s) == (3, 2):
        x, mode = F.pad(x, [1, 1, 1, 1]), 1
    elif (k, s) == (1, 2):
        x = x[:, :, ::2, ::2]
    elif k == 7:
        n, c, h, wd = x.shape
        ho, wo = (h + 2 * p - k) // s + 1, (wd + 2 * p - k) // s + 1
        x = F.unfold(x, k, padding=p, stride=s).reshape(n, c * k * k, ho, wo)
        w = networks._wgrad_cache.get((w,), lambda: w.reshape(w.shape[0], -1, 1, 1), key='parse_stem_1x1')
    return ops.conv(x.contiguous(), w, b, relu, mode)


def _conv_grad(ops, dz, conv, bn=None, size=None):
    """The input gradient of `_conv` (before its activation) from dz.  Stride 1: mode 0 on the transposed, flipped weights.  3x3 stride 2:
    mode 2 on the transposed weights gives the gradient of the PADDED input, (2 ho + 1) x (2 wo + 1) = (h + 1) x (w + 1) for even h, w; rows
    and columns 1..h are the input's (the last padded row and column are never read by the floor-stride convolution): a view, not a copy.
    1x1 stride 2: the 1x1 gradient at half resolution; the caller scatters it to the even positions (`half` term of the join)."""
    w, _ = face_parsing._folded(conv, bn)
    k, s = conv.kernel_size[0], conv.stride[0]
    if (k, s) == (3, 2):
        g = ops.conv(dz, networks._grad_weight(w, False), None, False, 2)
        return g[:, :, 1:size[0] + 1, 1:size[1] + 1]
    return ops.conv(dz, networks._grad_weight(w, True), None, False, 0)


def _sides_ok(H, W):
    return H % 32 == 0 and W % 32 == 0 and H >= 64 and W >= 64


def _fused_forward(ops, net, x, target):
    """-> (loss, saved): the forward of the fused pass; `saved` is what `_fused_backward` reads."""
    cp, rn = net.cp, net.cp.resnet
    s = _conv(ops, x, rn.conv1, rn.bn1, relu=True)
    h, pidx = ops.maxpool(s)
    blocks, feats = [], []
    for layer in (rn.layer1, rn.layer2, rn.layer3, rn.layer4):
        for blk in layer:
            y1 = _conv(ops, h, blk.conv1, blk.bn1, relu=True)
            y2 = _conv(ops, y1, blk.conv2, blk.bn2)
            sc = h if blk.downsample is None else _conv(ops, h, blk.downsample[0], blk.downsample[1])
            out = ops.join([sc, y2], post=1)
            blocks.append((blk, tuple(h.shape[2:]), y1, out))
            h = out
        feats.append(h)
    feat8, feat16, feat32 = feats[1:]

    def area(t):
        return t.shape[2] * t.shape[3]
    avg = _conv(ops, ops.plane_sums(feat32, None, 1.0 / area(feat32)), cp.conv_avg.conv, cp.conv_avg.bn, relu=True)
    f32c = _conv(ops, feat32, cp.arm32.conv.conv, cp.arm32.conv.bn, relu=True)
    a32 = torch.sigmoid(_conv(ops, ops.plane_sums(f32c, None, 1.0 / area(f32c)), cp.arm32.conv_atten, cp.arm32.bn_atten))
    u32 = ops.join([f32c], scale=a32, bias=avg)
    up32 = _conv(ops, ops.resize(u32, feat16.shape[2:]), cp.conv_head32.conv, cp.conv_head32.bn, relu=True)
    f16c = _conv(ops, feat16, cp.arm16.conv.conv, cp.arm16.conv.bn, relu=True)
    a16 = torch.sigmoid(_conv(ops, ops.plane_sums(f16c, None, 1.0 / area(f16c)), cp.arm16.conv_atten, cp.arm16.bn_atten))
    u16 = ops.join([f16c, up32], scale=a16)
    up16 = _conv(ops, ops.resize(u16, feat8.shape[2:]), cp.conv_head16.conv, cp.conv_head16.bn, relu=True)
    ffm = net.ffm
    ff = _conv(ops, torch.cat([feat8, up16], dim=1), ffm.convblk.conv, ffm.convblk.bn, relu=True)
    t1 = _conv(ops, ops.plane_sums(ff, None, 1.0 / area(ff)), ffm.conv1, relu=True)
    g = torch.sigmoid(_conv(ops, t1, ffm.conv2))
    fo = ops.join([ff, ff], scale=g)                                     # feat * atten + feat
    o1 = _conv(ops, fo, net.conv_out.conv.conv, net.conv_out.conv.bn, relu=True)
    logits = _conv(ops, o1, net.conv_out.conv_out)
    loss, lse = ops.ce(logits, target)
    saved = dict(size=tuple(x.shape[2:]), s=s, pidx=pidx, blocks=blocks, avg=avg, f32c=f32c, a32=a32, up32=up32, f16c=f16c, a16=a16, up16=up16,
                 ff=ff, t1=t1, g=g, o1=o1, logits=logits, lse=lse, target=target,
                 sizes=(tuple(feat8.shape[2:]), tuple(feat16.shape[2:]), tuple(feat32.shape[2:])), c8=feat8.shape[1])
    return loss, saved


def _fused_backward(ops, net, sv, dloss):
    """-> d loss / d image.  Every `join` with post=2 is (the sum of the gradients that meet at a tensor) * (the tensor > 0)."""
    cp, rn, ffm = net.cp, net.cp.resnet, net.ffm
    size8, size16, size32 = sv['sizes']
    dl = ops.ce_backward(sv['logits'], sv['target'], sv['lse'], dloss)
    dz = ops.relu_backward(_conv_grad(ops, dl, net.conv_out.conv_out), sv['o1'])
    dfo = _conv_grad(ops, dz, net.conv_out.conv.conv, net.conv_out.conv.bn)
    # feature fusion: fo = ff * g + ff, g = sigmoid(conv2(relu(conv1(mean ff))))
    ff, g = sv['ff'], sv['g']
    dg = ops.plane_sums(dfo, ff) * (g * (1 - g))
    dt1 = _conv_grad(ops, dg.contiguous(), ffm.conv2) * (sv['t1'] > 0)
    dmean = _conv_grad(ops, dt1.contiguous(), ffm.conv1)
    dz = ops.join([dfo, dfo], scale=g, bias=dmean, bias_gain=1.0 / (size8[0] * size8[1]), y=ff, post=2)
    dcat = _conv_grad(ops, dz, ffm.convblk.conv, ffm.convblk.bn)
    c8 = sv['c8']
    # context path, 1/8 -> 1/16: up16 = relu(conv_head16(resize(u16))), u16 = f16c * a16 + up32
    dz = ops.join([dcat[:, c8:]], y=sv['up16'], post=2)
    du16 = ops.resize_backward(_conv_grad(ops, dz, cp.conv_head16.conv, cp.conv_head16.bn), size16)
    f16c, a16 = sv['f16c'], sv['a16']
    da = ops.plane_sums(du16, f16c) * (a16 * (1 - a16))
    dmean = _conv_grad(ops, da.contiguous(), cp.arm16.conv_atten, cp.arm16.bn_atten)
    dz = ops.join([du16], scale=a16, bias=dmean, bias_gain=1.0 / (size16[0] * size16[1]), y=f16c, post=2)
    dfeat16 = _conv_grad(ops, dz, cp.arm16.conv.conv, cp.arm16.conv.bn)
    # 1/16 -> 1/32: up32 = relu(conv_head32(resize(u32))), u32 = f32c * a32 + avg
    dz = ops.relu_backward(du16, sv['up32'])
    du32 = ops.resize_backward(_conv_grad(ops, dz, cp.conv_head32.conv, cp.conv_head32.bn), size32)
    f32c, a32 = sv['f32c'], sv['a32']
    da = ops.plane_sums(du32, f32c) * (a32 * (1 - a32))
    dmean = _conv_grad(ops, da.contiguous(), cp.arm32.conv_atten, cp.arm32.bn_atten)
    dz = ops.join([du32], scale=a32, bias=dmean, bias_gain=1.0 / (size32[0] * size32[1]), y=f32c, post=2)
    dfeat32 = _conv_grad(ops, dz, cp.arm32.conv.conv, cp.arm32.conv.bn)
    davg = ops.plane_sums(du32) * (sv['avg'] > 0)
    dmean32 = _conv_grad(ops, davg.contiguous(), cp.conv_avg.conv, cp.conv_avg.bn)          # the global average of feat32
    # the ResNet, last block first: `terms` (+ a broadcast mean gradient) are what meets at the block's output
    terms, bias, gain = [dfeat32], dmean32, 1.0 / (size32[0] * size32[1])
    blocks = sv['blocks']
    for i in reversed(range(len(blocks))):
        blk, in_size, y1, out = blocks[i]
        if i == 5:
            terms.append(dfeat16)
        elif i == 3:
            terms.append(dcat[:, :c8])
        dz = ops.join(terms, bias=bias, bias_gain=gain, y=out, post=2)
        bias, gain = None, 1.0
        dz1 = ops.relu_backward(_conv_grad(ops, dz, blk.conv2, blk.bn2), y1)
        g1 = _conv_grad(ops, dz1, blk.conv1, blk.bn1, size=in_size)
        if blk.downsample is None:
            terms = [g1, dz]
        else:
            terms = [g1, (_conv_grad(ops, dz, blk.downsample[0], blk.downsample[1]), True)]
    dp = ops.join(terms)
    ds = ops.maxpool_backward(dp, sv['pidx'], sv['s'].shape[2:], mask=sv['s'])
    return ops.stem_backward(ds, face_parsing._folded(rn.conv1, rn.bn1)[0], sv['size'])


class _FusedParseLoss(torch.autograd.Function):
    """The parser, the loss head and the image gradient back through all of it on the HIP entry points.  The only differentiable input is
    the image; the backward is differentiable once.  The activations it keeps are the pass's own outputs (nothing a caller holds), so they
    live on the context rather than in `save_for_backward`."""

    @staticmethod
    def forward(ctx, img, net, target):
        loss, ctx.sv = _fused_forward(_HipOps.get(), net, img, target)
        ctx.net = net
        return loss

    @staticmethod
    @once_differentiable
    def backward(ctx, dloss):
        return _fused_backward(_HipOps.get(), ctx.net, ctx.sv, dloss.to(torch.float32).reshape(1).contiguous()), None, None


def _on_hip(bisNet, img):
    if not (fused and isinstance(img, torch.Tensor) and img.is_cuda and img.dtype == torch.float32 and img.ndim == 4 and img.shape[1] == 3
            and _sides_ok(img.shape[2], img.shape[3]) and type(bisNet) is face_parsing.BiSeNet and not bisNet.training):
        return False
    params = list(bisNet.parameters())
    if any(p.requires_grad or p.dtype != torch.float32 or p.device != img.device for p in params):
        return False
    return networks.use_hip_modconv and networks._modconv_init() and networks._modconv_grad_init()


def labels(bisNet, img):
    """The parser's argmax class ids of `img` ([N, 3, H, W] in -1..1), int64 [N, H, W], no remap, no gradient: what
    `parsing_img(bisNet, img, argmax=True, return_mask=False, remap=False)[1].squeeze(1)` returns."""
    with torch.no_grad():
        return bisNet(img)[0].argmax(1)


def cross_entropy(bisNet, img, target):
    """`torch.nn.CrossEntropyLoss()(bisNet(img)[0], target)`, differentiable with respect to `img` ([N, 3, H, W] in -1..1); target: int64
    [N, H, W] in 0..n_classes-1.  EVERY label must lie in that range: the HIP path does not look at the values (a check would wait for the
    device), and a label outside it - `CrossEntropyLoss`'s ignore_index -100 included, which the PyTorch path drops from the mean - would
    contribute its pixel's log-sum-exp and stay in the N H W mean.  `parse_distance` checks its labels once."""
    if _on_hip(bisNet, img) and target.dtype == torch.int64 and target.device == img.device and tuple(target.shape) == (img.shape[0], *img.shape[2:]):
        return _FusedParseLoss.apply(img.contiguous(), bisNet, target.contiguous())
    return F.cross_entropy(bisNet(img)[0], target)


def parse_distance(target, bisNet, weight=1.0, base=None):
    """The `distance` of `projection.project` that keeps the rendered image's semantic mask on `target`: images (0..255) are mapped to -1..1
    (`x / 127.5 - 1`, as the reference does in front of its parser) and the closure returns `weight * cross_entropy(bisNet, x, labels)`
    (+ `base(images)` when given, e.g. `l2_distance(...)` or `lpips_distance(...)`).  target: int64 labels [1, H, W] in parser class ids (an
    edited mask), or an image [1, 3, H, W] in 0..255 whose labels are computed once with `labels`."""
    if target.dtype == torch.int64:
        lab = target.detach()
        n_classes = bisNet.conv_out.conv_out.out_channels if hasattr(bisNet, 'conv_out') else None
        if n_classes is not None and lab.numel() and not (0 <= int(lab.min()) and int(lab.max()) < n_classes):          # once, not per step
            raise ValueError(f'parse_distance: labels must lie in 0..{n_classes - 1} (no ignore_index), got {int(lab.min())}..{int(lab.max())}')
    else:
        lab = labels(bisNet, target.detach().to(torch.float32) / 127.5 - 1)

    def distance(images):
        d = weight * cross_entropy(bisNet, images / 127.5 - 1, lab.to(images.device))
        return d + base(images) if base is not None else d
    return distance
