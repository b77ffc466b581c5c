"""The ArcFace identity loss with a HIP forward and image gradient.

Reference: the identity term of the hybrid encoder's training step (apps/train_hybrid_encoder.py:235-237, 305-335,
inversion/criteria/id_loss.py): one minus the cosine between the embeddings that a frozen face-recognition net - the IR-SE50 `Backbone` of
inversion/psp/encoders/model_irse.py / helpers.py - gives for the re-rendered and for the real image,

    feats(x) = l2_norm(facenet(face_pool(pool(x)[:, :, 35:223, 32:220])))        # pool: to 256 x 256 unless already, face_pool: to 112 x 112
    loss     = mean_i (1 - feats(y_hat)_i . feats(y)_i)

back-propagated through the net into `y_hat`.  `Backbone` here is written from that definition with the reference's module and parameter
names, so `model_ir_se50.pth` loads unchanged; `IDLoss` has the reference's `extract_feats` / `forward` and, for a training step,
`features` + `distance_to` (the same loss against cached embeddings, without the host synchronisation of `forward`'s logs);
`id_distance(...)` is the closure `training.projection.project(distance=...)` takes.  Nothing here downloads: WITHOUT LOADED WEIGHTS THE
NET IS RANDOMLY INITIALISED and the loss measures nothing; pass `weights=` (a path or a state dict) or call `facenet.load_state_dict`.

`fused` (module switch): float32 CUDA images [n, 3, 256 f, 256 f] with an integer f >= 1 and an `ir_se` backbone of input size 112 in eval
mode whose parameters are all frozen run on the HIP path: one autograd Function whose forward launches ide3d_id_prep, the convolutions as
ide3d_modconv2d on BatchNorm-folded weights (a block's leading BatchNorm is an explicit affine pass: its shift would meet the zero padding),
ide3d_prelu, ide3d_plane_sums + ide3d_se_gate + one gated join per block, ide3d_linear on the output layer with both its BatchNorms folded
in, and ide3d_id_head; the backward launches the same convolutions on derived weights (as `parse_loss._conv_grad` derives them) and the
adjoints of the other passes, and returns the image gradient only.  Everything else - CPU tensors, other dtypes and sizes, trainable
parameters, `mode='ir'`, `fused = False` - is the plain PyTorch definition.
`arith` (module switch): the per-call arithmetic of the convolutions on the HIP path (0 = the process default, see
`hip_plugin.conv_arithmetic`).
"""

import torch
import torch.nn as nn
from torch.autograd.function import once_differentiable

from training import networks
from training.parse_loss import _conv, _conv_grad

# True: what the HIP path takes (see above) runs on it.  False: always the PyTorch definition.  Shipped value: see DESIGN.md section 5.17.
fused = True
arith = 0

CROP = (35, 223, 32, 220)          # rows, columns of the 256 x 256 frame (id_loss.py:21)


# ---- the net (model_irse.py, helpers.py) -------------------------------------------------------------------------------------------------------
class Flatten(nn.Module):
    def forward(self, x):
        return x.reshape(x.shape[0], -1)


def l2_norm(x, axis=1):
    return x / torch.norm(x, 2, axis, True)


class SEModule(nn.Module):
    """x * sigmoid(fc2(relu(fc1(mean over the pixels of x)))) (helpers.py:61-78)."""

    def __init__(self, channels, reduction):
        super().__init__()
        self.avg_pool = nn.AdaptiveAvgPool2d(1)
        self.fc1 = nn.Conv2d(channels, channels // reduction, kernel_size=1, padding=0, bias=False)
        self.relu = nn.ReLU(inplace=True)
        self.fc2 = nn.Conv2d(channels // reduction, channels, kernel_size=1, padding=0, bias=False)
        self.sigmoid = nn.Sigmoid()

    def forward(self, x):
        return x * self.sigmoid(self.fc2(self.relu(self.fc1(self.avg_pool(x)))))


class bottleneck_IR(nn.Module):
    """BatchNorm -> 3x3 -> PReLU -> 3x3 (stride) -> BatchNorm, plus the shortcut: the decimated input when the width stays, else 1x1 (stride)
    -> BatchNorm (helpers.py:81-99)."""

    def __init__(self, in_channel, depth, stride, se=False):
        super().__init__()
        self.in_channel, self.depth, self.stride = in_channel, depth, stride
        if in_channel == depth:
            self.shortcut_layer = nn.MaxPool2d(1, stride)
        else:
            self.shortcut_layer = nn.Sequential(nn.Conv2d(in_channel, depth, (1, 1), stride, bias=False), nn.BatchNorm2d(depth))
        layers = [nn.BatchNorm2d(in_channel), nn.Conv2d(in_channel, depth, (3, 3), (1, 1), 1, bias=False), nn.PReLU(depth),
                  nn.Conv2d(depth, depth, (3, 3), stride, 1, bias=False), nn.BatchNorm2d(depth)]
        self.res_layer = nn.Sequential(*layers, *([SEModule(depth, 16)] if se else []))

    def forward(self, x):
        return self.res_layer(x) + self.shortcut_layer(x)


class bottleneck_IR_SE(bottleneck_IR):
    """The same with a squeeze-excite gate at the end of the residual branch (helpers.py:102-123)."""

    def __init__(self, in_channel, depth, stride):
        super().__init__(in_channel, depth, stride, se=True)


UNITS = {50: (3, 4, 14, 3), 100: (3, 13, 30, 3), 152: (3, 8, 36, 3)}


class Backbone(nn.Module):
    """The IR / IR-SE face net (model_irse.py:9-48): `input_layer` (3x3, BatchNorm, PReLU), `body` (a flat Sequential of blocks, four
    stages whose first block has stride 2), `output_layer` (BatchNorm2d, Dropout, Flatten, Linear to 512, BatchNorm1d), l2_norm.
    `state_dict()` has the reference's keys in the reference's order.  `widths` / `units`: the stages' widths and block counts (narrow,
    short nets for tests); the defaults are the reference's."""

    def __init__(self, input_size=112, num_layers=50, mode='ir_se', drop_ratio=0.6, affine=True, widths=(64, 128, 256, 512), units=None):
        super().__init__()
        assert input_size in (112, 224), 'input_size should be 112 or 224'
        assert mode in ('ir', 'ir_se'), 'mode should be ir or ir_se'
        if units is None:
            assert num_layers in UNITS, 'num_layers should be 50, 100 or 152'
            units = UNITS[num_layers]
        assert len(widths) == 4 and len(units) == 4
        self.input_size, self.mode = input_size, mode
        unit = bottleneck_IR_SE if mode == 'ir_se' else bottleneck_IR
        self.input_layer = nn.Sequential(nn.Conv2d(3, widths[0], (3, 3), 1, 1, bias=False), nn.BatchNorm2d(widths[0]), nn.PReLU(widths[0]))
        side = input_size // 16
        self.output_layer = nn.Sequential(nn.BatchNorm2d(widths[3]), nn.Dropout(drop_ratio), Flatten(), nn.Linear(widths[3] * side * side, 512),
                                          nn.BatchNorm1d(512, affine=affine))
        modules, cin = [], widths[0]
        for depth, count in zip(widths, units):
            modules += [unit(cin, depth, 2)] + [unit(depth, depth, 1) for _ in range(count - 1)]
            cin = depth
        self.body = nn.Sequential(*modules)

    def forward(self, x):
        return l2_norm(self.output_layer(self.body(self.input_layer(x))))


# ---- the fused pass, written against an `ops` object: `_HipOps` here, a float64 torch restatement in tests/id_loss_ref.py ---------------------
class _HipOps:
    """The launches of the fused pass.  conv: ide3d_modconv2d; join, plane_sums: csrc/parse_loss.hip; everything else: csrc/id_loss.hip."""

    _instance = None

    @classmethod
    def get(cls):
        if cls._instance is None:
            cls._instance = cls()
        return cls._instance

    def __init__(self):
        from torch_utils import hip_plugin
        P, Q = hip_plugin.IdLossPlugin, hip_plugin.ParseLossPlugin
        self.prep, self.prep_backward, self.prelu, self.prelu_backward = P.prep, P.prep_backward, P.prelu, P.prelu_backward
        self.se_gate, self.se_gate_backward, self.linear, self.linear_backward_input = P.se_gate, P.se_gate_backward, P.linear, P.linear_backward_input
        self.head, self.head_backward = P.head, P.head_backward
        self.join, self.plane_sums = Q.join, Q.plane_sums

    @staticmethod
    def conv(x, w, bias, relu, mode=0):
        return networks.plain_conv(x, w, bias, relu, mode, arith)          # (this module's own `arith`, hence not parse_loss's method)


def _bn_affine(bn):
    """(scale, shift) of an eval-mode BatchNorm, float64."""
    scale = (bn.running_var.double() + bn.eps).rsqrt()
    if bn.weight is not None:
        scale = scale * bn.weight.detach().double()
    shift = -bn.running_mean.double() * scale
    return scale, (shift + bn.bias.detach().double() if bn.bias is not None else shift)


def _affine(bn, n):
    """(scale, shift) of a block's leading BatchNorm as [n, c] float32 tensors (what the join reads), cached."""
    def build():
        scale, shift = _bn_affine(bn)
        return tuple(t.float()[None].expand(n, -1).contiguous() for t in (scale, shift))
    return networks._wgrad_cache.get((bn.weight, bn.bias, bn.running_mean, bn.running_var), build, key=('id_affine', n), extra=bn.eps)


def _folded_linear(net):
    """(weight [512, c * 49], bias [512]) of the output layer as one linear layer: BatchNorm2d in front (no padding is involved, so its
    shift folds exactly into the bias) and BatchNorm1d behind, folded in float64; Dropout is the identity in eval mode.  Cached."""
    bn2, lin, bn1 = net.output_layer[0], net.output_layer[3], net.output_layer[4]

    def build():
        s2, t2 = _bn_affine(bn2)
        s1, t1 = _bn_affine(bn1)
        w = lin.weight.detach().double()
        per = w.shape[1] // s2.numel()
        b = lin.bias.detach().double() + w @ t2.repeat_interleave(per)
        w = w * s2.repeat_interleave(per)[None]
        return (w * s1[:, None]).float().contiguous(), (b * s1 + t1).float().contiguous()
    sources = [lin.weight, lin.bias, bn2.weight, bn2.bias, bn2.running_mean, bn2.running_var, bn1.running_mean, bn1.running_var]
    sources += [bn1.weight, bn1.bias] if bn1.weight is not None else []
    return networks._wgrad_cache.get(tuple(sources), build, key='id_linear', extra=(bn2.eps, bn1.eps))


def _slope(prelu):
    return prelu.weight.detach()


def _fused_forward(ops, net, x, target):
    """-> (loss or None, e, saved): x [n, 3, 256 f, 256 f]; target: unit embeddings [n, 512] or None (embeddings only).  `saved` is what
    `_fused_backward` reads."""
    n = x.shape[0]
    il = net.input_layer
    z0 = _conv(ops, ops.prep(x), il[0], il[1])
    h = ops.prelu(z0, _slope(il[2]))
    blocks = []
    for blk in net.body:
        res = blk.res_layer
        scale, shift = _affine(res[0], n)
        z1 = _conv(ops, ops.join([h], scale=scale, bias=shift), res[1])
        z2 = _conv(ops, ops.prelu(z1, _slope(res[2])), res[3], res[4])
        mean = ops.plane_sums(z2, None, 1.0 / (z2.shape[2] * z2.shape[3]))
        g = ops.se_gate(mean, res[5].fc1.weight.detach(), res[5].fc2.weight.detach())
        if blk.in_channel == blk.depth:
            sc = h if blk.stride == 1 else h[:, :, ::blk.stride, ::blk.stride].contiguous()
        else:
            sc = _conv(ops, h, blk.shortcut_layer[0], blk.shortcut_layer[1])
        h = ops.join([z2, sc], scale=g)
        blocks.append((blk, z1, z2, mean, g))
    w, b = _folded_linear(net)
    e, norm, loss = ops.head(ops.linear(h.reshape(n, -1), w, b), target)
    return loss, e, dict(size=tuple(x.shape[2:]), z0=z0, blocks=blocks, top=tuple(h.shape), e=e, norm=norm, target=target)


def _fused_backward(ops, net, sv, dloss):
    """-> d loss / d image.  dloss: one element on the device."""
    n = sv['e'].shape[0]
    df = ops.head_backward(sv['e'], sv['target'], sv['norm'], dloss)
    dh = ops.linear_backward_input(df, _folded_linear(net)[0]).reshape(sv['top'])
    for blk, z1, z2, mean, g in reversed(sv['blocks']):
        res = blk.res_layer
        # out = z2 * g + shortcut, g = gate(mean of z2): the gradient of z2 is dh * g + the mean's broadcast gradient
        dg = ops.plane_sums(dh, z2)
        dmean = ops.se_gate_backward(mean, res[5].fc1.weight.detach(), res[5].fc2.weight.detach(), g, dg)
        dz2 = ops.join([dh], scale=g, bias=dmean, bias_gain=1.0 / (z2.shape[2] * z2.shape[3]))
        dz1 = ops.prelu_backward(_conv_grad(ops, dz2, res[3], res[4], size=tuple(z1.shape[2:])), z1, _slope(res[2]))
        da = _conv_grad(ops, dz1, res[1])
        half = blk.stride == 2
        if blk.in_channel == blk.depth:
            short = (dh, True) if half else dh
        else:
            short = _conv_grad(ops, dh, blk.shortcut_layer[0], blk.shortcut_layer[1])
            short = (short, True) if half else short
        dh = ops.join([da, short], scale=_affine(res[0], n)[0])
    il = net.input_layer
    dz0 = ops.prelu_backward(dh, sv['z0'], _slope(il[2]))
    return ops.prep_backward(_conv_grad(ops, dz0, il[0], il[1]), sv['size'])


class _FusedIdLoss(torch.autograd.Function):
    """Embedding, loss and the image gradient back through the net on the HIP entry points -> (loss, embeddings); only the loss is
    differentiable, only with respect to the image; the backward is differentiable once.  The activations it keeps are the pass's own
    outputs, so they live on the context rather than in `save_for_backward`."""

    @staticmethod
    def forward(ctx, img, net, feats):
        loss, e, ctx.sv = _fused_forward(_HipOps.get(), net, img, feats)
        ctx.net = net
        ctx.mark_non_differentiable(e)
        return loss, e

    @staticmethod
    @once_differentiable
    def backward(ctx, dloss, _de):
        return _fused_backward(_HipOps.get(), ctx.net, ctx.sv, dloss.to(torch.float32).reshape(1).contiguous()), None, None


def _on_hip(net, img):
    if not (fused and isinstance(img, torch.Tensor) and img.is_cuda and img.dtype == torch.float32 and img.ndim == 4 and img.shape[1] == 3
            and img.shape[2] == img.shape[3] and img.shape[2] >= 256 and img.shape[2] % 256 == 0 and type(net) is Backbone
            and net.mode == 'ir_se' and net.input_size == 112 and not net.training):
        return False
    if any(p.requires_grad or p.dtype != torch.float32 or p.device != img.device for p in net.parameters()):
        return False
    return networks.use_hip_modconv and networks._modconv_init() and networks._modconv_grad_init()


class IDLoss(nn.Module):
    """`inversion/criteria/id_loss.py::IDLoss` without its weights file: `.facenet` is the IR-SE50 `Backbone` in eval mode, frozen.  Nothing
    is downloaded or loaded unless `weights` (a path or a state dict, `model_ir_se50.pth`) is given: WITHOUT LOADED WEIGHTS THE NET IS
    RANDOMLY INITIALISED.  `facenet`: another `Backbone` to use instead (tests build narrow ones)."""

    def __init__(self, weights=None, facenet=None):
        super().__init__()
        self.facenet = facenet if facenet is not None else Backbone(input_size=112, num_layers=50, drop_ratio=0.6, mode='ir_se')
        if weights is not None:
            self.facenet.load_state_dict(torch.load(weights, map_location='cpu') if isinstance(weights, (str, bytes)) or hasattr(weights, '__fspath__') else weights)
        self.pool = nn.AdaptiveAvgPool2d((256, 256))
        self.face_pool = nn.AdaptiveAvgPool2d((112, 112))
        self.facenet.eval().requires_grad_(False)

    def train(self, mode=True):
        """The face net stays in eval mode (the reference calls `facenet.eval()` once and trains nothing of it)."""
        super().train(mode)
        self.facenet.eval()
        return self

    def extract_feats(self, x):
        """The unit embeddings [n, 512] of images in -1..1 (id_loss.py:18-24), differentiable with respect to x on the PyTorch path only;
        on the HIP path (see the module) no gradient is recorded: use `distance_to` for one."""
        if _on_hip(self.facenet, x) and not (torch.is_grad_enabled() and x.requires_grad):
            with torch.no_grad():
                return _fused_forward(_HipOps.get(), self.facenet, x.contiguous(), None)[1]
        return self._definition(x)

    def _definition(self, x):
        if x.shape[2] != 256:
            x = self.pool(x)
        x = x[:, :, CROP[0]:CROP[1], CROP[2]:CROP[3]]
        return self.facenet(self.face_pool(x))

    def features(self, y):
        """Detached unit embeddings of `y` for caching (the target of `distance_to`)."""
        with torch.no_grad():
            return self.extract_feats(y.detach()).detach()

    def _distance(self, y_hat, feats):
        """-> (mean_i (1 - e(y_hat)_i . feats_i), e(y_hat)); the gradient flows to y_hat only."""
        feats = feats.detach()
        if _on_hip(self.facenet, y_hat) and feats.is_cuda and feats.device == y_hat.device and feats.dtype == torch.float32 \
                and tuple(feats.shape) == (y_hat.shape[0], 512):
            return _FusedIdLoss.apply(y_hat.contiguous(), self.facenet, feats.contiguous())
        e = self._definition(y_hat)
        return (1 - (e * feats.to(e.dtype)).sum(dim=1)).mean(), e

    def distance_to(self, y_hat, feats):
        """The scalar mean_i (1 - e(y_hat)_i . feats_i) against cached `features(y)`, without any host synchronisation: what a training
        step should call."""
        return self._distance(y_hat, feats)[0]

    def forward(self, y_hat, y, x):
        """The reference's triple (loss, sim_improvement, id_logs) (id_loss.py:26-47): id_logs holds Python floats, so this waits for the
        device as the reference does.  When `x is y` the features are computed once."""
        y_feats = self.features(y)
        x_feats = y_feats if x is y else self.features(x)
        loss, e = self._distance(y_hat, y_feats)
        e = e.detach()
        rows = torch.stack([(e * y_feats).sum(1), (e * x_feats).sum(1), (y_feats * x_feats).sum(1)], dim=1).double().cpu().tolist()
        id_logs = [{'diff_target': t, 'diff_input': i, 'diff_views': v} for t, i, v in rows]
        sim_improvement = sum(t - v for t, _, v in rows) / len(rows)
        return loss, sim_improvement, id_logs


def id_distance(target, idloss, weight=1.0, base=None):
    """The `distance` of `projection.project` that keeps the rendered image's identity on `target`'s ([n, 3, H, W], 0..255): images
    (0..255) are mapped to -1..1 (`x / 127.5 - 1`) and the closure returns `weight * idloss.distance_to(x, features(target))`
    (+ `base(images)` when given, e.g. `l2_distance(...)` or `lpips_distance(...)`)."""
    feats = idloss.features(target.detach().to(torch.float32) / 127.5 - 1)

    def distance(images):
        d = weight * idloss.distance_to(images / 127.5 - 1, feats.to(images.device))
        return d + base(images) if base is not None else d
    return distance
