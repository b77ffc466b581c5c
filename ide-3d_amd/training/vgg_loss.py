"""The VGG19 feature loss of the hybrid encoder's training step, with a HIP forward and image gradient.

Reference: `VGGLoss` of apps/train_hybrid_encoder.py:120-152 (used at :305).  Written from the definition:

    s, t = (source + 1) / 2, (target + 1) / 2                        no ImageNet z-score
    a_k  = VGG19 activations relu1_1, relu2_1, relu3_1, relu4_1, relu5_1: torchvision's `vgg19().features[:30]` (3x3 convolutions with
           padding 1 + ReLU at positions 0, 2, 5, 7, 10, 12, 14, 16, 19, 21, 23, 25, 28; MaxPool2d(2, 2) at 4, 9, 18, 27) cut into the
           slices [0, 2) [2, 7) [7, 12) [12, 21) [21, 30), a_k the output of slice k
    loss = sum_k weights[k] * mean_{n c h w} |a_k(s) - a_k(t)|       weights (1, 1, 1, 1, 1); `n_layers` in 1..5 keeps the first slices;
                                                                     the target is evaluated without gradient

Every tap is a ReLU output that feeds the next convolution directly; every pool follows a ReLU that is no tap.  Module names equal the
reference class's (`layers.{slice}.{position}.{weight,bias}`), so a `state_dict` saved from it loads as is; `load_torchvision_state_dict`
takes torchvision's `features.N.*` keys.  Nothing here downloads: WITHOUT LOADED WEIGHTS THE NET IS RANDOMLY INITIALISED.  An image side
below 16 leaves the fourth pool without a window and raises ValueError on every path (whatever `n_layers`).

`fused` (module switch): fp32 CUDA images, dense NCHW, 3 channels, frozen parameters on the image's device and (for `distance_to`) dense
fp32 cached features without grad run on the HIP path, one autograd Function that returns the image gradient only:

    forward    lpips_prep (f = 1, x * 0.5 + 0.5, mean 0, std 1: bit-equal to (x + 1) / 2) -> 13 x modconv2d (bias, ReLU), 4 x maxpool2
               -> feat_l1
    backward   tap 5: feat_l1_tap_backward(g = None) -> modconv2d on the transposed-flipped weights
               behind a pool (conv4_4, conv3_4, conv2_2, conv1_2): maxpool2_relu_backward -> modconv2d likewise
               interior (conv4_3, conv4_2, conv3_3, conv3_2): modconv_act_backward -> modconv2d likewise
               taps 4..1: feat_l1_tap_backward(g) -> modconv2d likewise
               lpips_prep_backward

Everything else — CPU, other dtypes, `fused = False`, parameters that require grad — takes the torch definition in this file.  `fused` ships
True: on an MI355X the HIP path is faster than the ATen path of this module at 256 x 256 and 512 x 512, batch 1 and 4 (DESIGN.md section
5.22, scripts/bench_vgg_loss.py).
"""

import torch
import torch.nn as nn
import torch.nn.functional as F

from training import networks

# True: what the HIP path takes (see above) runs on it.  False: always the torch definition.
fused = True

VGG19_WIDTHS = (64, 128, 256, 512, 512)
STAGES = (2, 2, 4, 4, 1)                                             # convolutions per stage of features[:30]; a pool between stages
CONV_INDEX = (0, 2, 5, 7, 10, 12, 14, 16, 19, 21, 23, 25, 28)        # their positions in torchvision's vgg19().features
POOL_INDEX = (4, 9, 18, 27)
SLICE_ENDS = (2, 7, 12, 21, 30)                                      # the reference's `feature_layers`
MIN_SIDE = 16                                                        # four 2x2 pools leave 1 x 1


def _layout(widths):
    """{position: module} of features[:30] at the given channels per stage."""
    mods, cin, pos = {}, 3, 0
    for s, (count, cout) in enumerate(zip(STAGES, widths)):
        if s > 0:
            mods[pos] = nn.MaxPool2d(kernel_size=2, stride=2); pos += 1
        for _ in range(count):
            mods[pos], mods[pos + 1] = nn.Conv2d(cin, cout, 3, 1, 1), nn.ReLU()
            cin, pos = cout, pos + 2
    assert pos == 30 and tuple(i for i in sorted(mods) if isinstance(mods[i], nn.Conv2d)) == CONV_INDEX
    assert tuple(i for i in sorted(mods) if isinstance(mods[i], nn.MaxPool2d)) == POOL_INDEX
    return mods


class VGG19Features(nn.Module):
    """torchvision's `vgg19().features[:30]` in the reference's five `Sequential` slices (train_hybrid_encoder.py:124-136), so that the keys
    of its `state_dict()` are `layers.{slice}.{position}.{weight,bias}`.  `widths`: channels per stage (the default is VGG19; tests build
    narrow nets); `n_layers` in 1..5 keeps the first slices.  Randomly initialised, frozen."""

    def __init__(self, widths=VGG19_WIDTHS, n_layers=5):
        super().__init__()
        assert len(widths) == len(STAGES) and 1 <= int(n_layers) <= len(SLICE_ENDS)
        self.widths, self.n_layers = tuple(int(w) for w in widths), int(n_layers)
        mods = _layout(self.widths)
        self.layers = nn.ModuleList()
        prev = 0
        for end in SLICE_ENDS[:self.n_layers]:
            piece = nn.Sequential()
            for pos in range(prev, end):
                piece.add_module(str(pos), mods[pos])
            self.layers.append(piece)
            prev = end
        # mean 0 and std 1 of ide3d_lpips_prep (device constants; not part of the state dict)
        self.register_buffer('_prep_mean', torch.zeros(3), persistent=False)
        self.register_buffer('_prep_std', torch.ones(3), persistent=False)
        self.requires_grad_(False)

    def plan(self):
        """[(kind, module)] in launch order, kind in 'conv' (a convolution + its ReLU), 'pool', 'tap' (the end of a slice)."""
        out = []
        for piece in self.layers:
            for m in piece:
                if isinstance(m, nn.Conv2d):
                    out.append(('conv', m))
                elif isinstance(m, nn.MaxPool2d):
                    out.append(('pool', m))
            out.append(('tap', None))
        return out

    def taps(self, z):
        """The slice outputs of an image already mapped to [0, 1] (torch definition)."""
        out, h = [], z
        for piece in self.layers:
            h = piece(h)
            out.append(h)
        return out

    def forward(self, x):
        """x in [-1, 1] -> the raw taps (torch definition)."""
        return self.taps((x + 1) / 2)


def _hip_taps(net, x):
    """-> (the output of every convolution + ReLU in order, the indices of the taps among them) on the HIP entry points."""
    from torch_utils import hip_plugin
    P, conv2d = hip_plugin.LpipsPlugin, networks._modconv_plugin.modconv2d
    h = P.prep(x, net._prep_mean, net._prep_std, 1, 0.5, 0.5)
    acts, tap_at = [], []
    for kind, m in net.plan():
        if kind == 'conv':
            h = conv2d(h, m.weight, None, None, None, 0.0, m.bias, 3, 0.0, 1.0, -1.0)
            acts.append(h)
        elif kind == 'pool':
            h = P.maxpool2(h)
        else:
            tap_at.append(len(acts) - 1)
    return acts, tap_at


class _FusedVggLoss(torch.autograd.Function):
    """prep -> 13 convolutions, 4 pools -> L1 head, and the image gradient back through all of it, on the HIP entry points.  The only
    differentiable input is the image."""

    @staticmethod
    def forward(ctx, x, net, feats):
        from torch_utils import hip_plugin
        acts, tap_at = _hip_taps(net, x)
        loss = hip_plugin.VggLossPlugin.feat_l1([acts[i] for i in tap_at], feats, net.weights[:len(tap_at)])
        ctx.save_for_backward(*acts)
        ctx.net, ctx.feats = net, feats
        return loss

    @staticmethod
    def backward(ctx, dloss):
        from torch_utils import hip_plugin
        P, V, conv2d = hip_plugin.LpipsPlugin, hip_plugin.VggLossPlugin, networks._modconv_plugin.modconv2d
        acts, net = ctx.saved_tensors, ctx.net
        dloss = dloss.to(torch.float32)
        # walk the plan backwards; `behind` is what follows the convolution whose ReLU gradient is due: a tap, a pool or the next convolution
        j, k, g, behind = len(acts), len(ctx.feats), None, None
        for kind, m in reversed(net.plan()):
            if kind != 'conv':
                behind = kind
                if kind == 'tap':
                    k -= 1
                continue
            j -= 1
            if behind == 'tap':
                dz = V.feat_l1_tap_backward(acts[j], ctx.feats[k], g, dloss, net.weights[k])
            elif behind == 'pool':
                dz = V.maxpool2_relu_backward(acts[j], g)
            else:
                dz, _ = networks._modconv_grad_plugin.act_backward(g, acts[j], 3, 0.0, 1.0, -1.0)
            g = conv2d(dz, networks._grad_weight(m.weight, True), None, None, None, 0.0, None, 1, 0.0, 1.0, -1.0)
            behind = 'conv'
        return P.prep_backward(g, net._prep_std, 1, 0.5), None, None


class VGGLoss(VGG19Features):
    """`VGGLoss(device)(source, target)` -> scalar, both [N, 3, H, W] in [-1, 1] with H, W >= 16: the reference class
    (train_hybrid_encoder.py:120-152) with `.layers` (the slices) and `.weights` as there.  `features` / `distance_to` are the cached-target
    form the other losses of this package offer.  No download: the weights are random until a state dict is loaded (`load_state_dict` of one
    saved from the reference class, or `load_torchvision_state_dict`)."""

    def __init__(self, device=None, n_layers=5, widths=VGG19_WIDTHS):
        super().__init__(widths, n_layers)
        self.weights = (1.0, 1.0, 1.0, 1.0, 1.0)
        if device is not None:
            self.to(device)

    def load_torchvision_state_dict(self, features):
        """`features`: a state dict with torchvision's keys (`features.N.weight`, `features.N.bias`, or without the prefix; other keys, such
        as the classifier's or the layers behind position 29, are ignored)."""
        sd, prev = {}, 0
        for s, end in enumerate(SLICE_ENDS[:self.n_layers]):
            for i in (i for i in CONV_INDEX if prev <= i < end):
                for name in ('weight', 'bias'):
                    key = f'features.{i}.{name}' if f'features.{i}.{name}' in features else f'{i}.{name}'
                    sd[f'layers.{s}.{i}.{name}'] = features[key]
            prev = end
        self.load_state_dict(sd)
        return self

    def _frozen(self):
        return not any(p.requires_grad for p in self.parameters())

    def _on_hip(self, x, feats=None):
        if not (fused and isinstance(x, torch.Tensor) and x.is_cuda and x.dtype == torch.float32 and x.ndim == 4 and x.shape[1] == 3
                and x.is_contiguous() and self._frozen() and all(p.dtype == torch.float32 and p.device == x.device for p in self.parameters())
                and self._prep_std.device == x.device):
            return False
        if feats is not None and not all(t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and not t.requires_grad for t in feats):
            return False
        return networks._modconv_init() and networks._modconv_grad_init()

    @staticmethod
    def _check_sides(x):
        h, w = x.shape[2], x.shape[3]
        if h < MIN_SIDE or w < MIN_SIDE:
            raise ValueError(f'the VGG19 feature loss needs image sides of at least {MIN_SIDE}, got {h} x {w}: '
                             'the fourth MaxPool2d(2, 2) would have no window')

    def features(self, target):
        """The raw taps of target (in [-1, 1]), without grad: what a caller caches for a fixed target."""
        self._check_sides(target)
        with torch.no_grad():
            if self._on_hip(target):
                acts, tap_at = _hip_taps(self, target)
                return [acts[i] for i in tap_at]
            return [t.detach() for t in self.taps((target + 1) / 2)]

    def distance_to(self, source, feats):
        """The loss for feats = features(target): the same value as forward(source, target)."""
        self._check_sides(source)
        feats = list(feats)
        assert len(feats) == len(self.layers)
        if self._on_hip(source, feats):
            return _FusedVggLoss.apply(source, self, feats)
        total = None
        for a, t, wt in zip(self.taps((source + 1) / 2), feats, self.weights):
            d = wt * F.l1_loss(a, t)
            total = d if total is None else total + d
        return total

    def forward(self, source, target):
        return self.distance_to(source, self.features(target))


def vgg_distance(target, vggloss, weight=1.0, base=None):
    """The `distance` of `projection.project` that keeps the rendered image's VGG19 features on `target`'s ([n, 3, H, W], 0..255): images
    (0..255) are mapped to -1..1 (`x / 127.5 - 1`) and the closure returns `weight * vggloss.distance_to(x, features(target))`
    (+ `base(images)` when given, e.g. `l2_distance(...)` or `lpips_distance(...)`)."""
    feats = vggloss.features((target.detach().to(torch.float32) / 127.5 - 1).contiguous())

    def distance(images):
        d = weight * vggloss.distance_to((images / 127.5 - 1).contiguous(), [t.to(images.device) for t in feats])
        return d + base(images) if base is not None else d
    return distance
