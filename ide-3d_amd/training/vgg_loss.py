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

The chain of launches is run by the walkers of training/feature_loss.py over `VGG19Features.plan()`; `_fused_backward` here holds the tap /
pool / interior choice as the walker's `relu_grad`.
Everything else — CPU, other dtypes, `fused = False`, parameters that require grad — takes the torch definition in this file.  `fused` ships
True: on an MI355X the HIP path is faster than the ATen path of this module at 256 x 256 and 512 x 512, batch 1 and 4 (DESIGN.md section
5.22, scripts/bench_vgg_loss.py).
"""

import torch
import torch.nn as nn
import torch.nn.functional as F

from training import feature_loss

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
            out += feature_loss.sequential_plan(piece, ()) + [('tap', None)]
        return out

    def taps(self, z):
        """The slice outputs of an image already mapped to [0, 1] (torch definition)."""
        return feature_loss.torch_taps(self.plan(), z)

    def forward(self, x):
        """x in [-1, 1] -> the raw taps (torch definition)."""
        return self.taps((x + 1) / 2)


# ---- the fused pass over the walkers of training/feature_loss.py, written against an `ops` object (tests/feature_loss_ref.py) -------------
def _fused_taps(ops, net, x):
    """-> what `forward_walk` returns for x in [-1, 1]: (the output of every convolution + ReLU, the positions of the taps among them, ...)."""
    return feature_loss.forward_walk(ops, feature_loss.plan_of(net), lambda: ops.prep(x, net._prep_mean, net._prep_std, 1, 0.5, 0.5), False)


def _fused_forward(ops, net, x, feats):
    """-> (loss, saved)."""
    saved = _fused_taps(ops, net, x)
    return ops.feat_l1(feature_loss.tapped(saved), feats, net.weights[:len(saved[1])]), saved


def _fused_backward(ops, net, saved, feats, dloss):
    """-> the image gradient.  What follows a ReLU picks its gradient pass: a tap (the L1 term joins the next convolution's input gradient,
    None behind the last tap), a pool (routed to the window's first maximum) or the next convolution."""
    acts = saved[0]

    def relu_grad(j, behind, k, g):
        if behind == 'tap':
            return ops.feat_l1_tap_backward(acts[j], feats[k], g, dloss, net.weights[k])
        if behind == 'pool':
            return ops.maxpool2_relu_backward(acts[j], g)
        return ops.relu_backward(g, acts[j])
    return ops.prep_backward(feature_loss.backward_walk(ops, feature_loss.plan_of(net), saved, relu_grad), net._prep_std, 1, 0.5)


class _FusedVggLoss(torch.autograd.Function):
    """prep -> 13 convolutions, 4 pools -> L1 head, and the image gradient back through all of it, on the HIP entry points.  The only
    differentiable input is the image."""

    @staticmethod
    def forward(ctx, x, net, feats):
        loss, (acts, tap_at, _, sizes) = _fused_forward(feature_loss.HipOps.get(), net, x, feats)
        ctx.save_for_backward(*acts)
        ctx.net, ctx.feats, ctx.walk = net, feats, (tap_at, sizes)
        return loss

    @staticmethod
    def backward(ctx, dloss):
        tap_at, sizes = ctx.walk
        saved = (ctx.saved_tensors, tap_at, (), sizes)
        return _fused_backward(feature_loss.HipOps.get(), ctx.net, saved, ctx.feats, dloss.to(torch.float32)), None, None


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
        names = {int(pos): f'layers.{s}.{pos}' for s, piece in enumerate(self.layers) for pos, m in piece.named_children() if isinstance(m, nn.Conv2d)}
        self.load_state_dict(feature_loss.torchvision_convs(features, names))
        return self

    def _on_hip(self, x, feats=None):
        return feature_loss.on_hip(fused, x, feats, self.parameters(), True, (self._prep_std,), True)

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
                return feature_loss.tapped(_fused_taps(feature_loss.HipOps.get(), self, target))
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
