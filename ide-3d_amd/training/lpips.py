"""The VGG16 LPIPS distance of the reference's projectors and coaches, with a HIP forward and image gradient.

Reference: `inversion/criteria/lpips/{lpips,networks,utils}.py` (the class the coaches minimise next to L2, base_coach.py:152-171) and the
`vgg16.pt` TorchScript of the projectors (w_projector_ide3d.py:66-75, 104-111).  Written from the definition:

    z   = (x - mean) / std                        mean (-.030, -.088, -.188), std (.458, .448, .450); x in [-1, 1]
    a_k = VGG16 activations relu1_2, relu2_2, relu3_3, relu4_3, relu5_3 of z (3x3 convolutions with padding 1 + ReLU in stages of
          2, 2, 3, 3, 3; a 2x2 max-pool with floor in front of stages 2..5)
    u_k = a_k / (sqrt(sum_c a_k^2) + 1e-10)
    d_k = mean_{h,w} sum_c lin_k[c] (u_k(x) - u_k(y))^2
    LPIPS(x, y) = sum_k sum_n d_k[n] / N

Parameter and buffer names equal the reference class's (`net.layers.{0,2,5,...,28}.{weight,bias}`, `net.mean`, `net.std`,
`lin.{0..4}.1.weight`), so a `state_dict` saved from its `LPIPS('vgg')` loads as is; `load_torchvision_state_dict` takes torchvision's
`features.N.*` keys and the five `lin` tensors.  Nothing here downloads: WITHOUT LOADED WEIGHTS THE NET IS RANDOMLY INITIALISED and the
value is not LPIPS.  Only 'vgg' exists in this module: AlexNet and SqueezeNet need 11x11, 5x5 and strided convolutions, which the
convolution kernel of this library does not have.  The AlexNet form (the reference's default) is `training.lpips_alex.LPIPS()`, which runs
those convolutions as 1x1 launches over unfolded patches.

One deliberate difference from the reference: at a pixel whose tap is zero in every channel, the reference's autograd returns NaN (the
derivative of sqrt at 0).  Here the gradient of that pixel's norm is DEFINED as 0 — in the kernels and in the torch definition below alike,
both of which use the closed form  da_c = g_c / (n + eps) - a_c (sum_k g_k a_k) / (n (n + eps)^2)  with the second term 0 where n = 0,
never autograd through sqrt.

`fused` (module switch): fp32 CUDA images, dense NCHW, frozen parameters, every map side >= 1 after the four pools and (for
`lpips_distance`) an integer area factor run on the HIP path: one autograd Function around ide3d_lpips_prep, 13 x ide3d_modconv2d (bias and
ReLU fused), 4 x ide3d_maxpool2, ide3d_lpips_head forward, and ide3d_lpips_head_backward, 5 x ide3d_lpips_stage_backward, 13 x
ide3d_modconv2d on the transposed-flipped weights, 8 x ide3d_modconv_act_backward, ide3d_lpips_prep_backward backward; it returns the
image gradient only (the weights are frozen).  Everything else — CPU, other dtypes, `fused = False`, parameters that require grad — takes the
torch definition in this file, differentiable by autograd except for the closed-form normalisation.  The chain of launches is run by the
walkers of training/feature_loss.py over `VGG16Features.plan()`; this module adds the prep, the head and `LPIPS._relu_grad`.
"""

import torch
import torch.nn as nn
import torch.nn.functional as F

from training import feature_loss, networks

# True: what the HIP path takes (see above) runs on it.  False: always the torch definition.
fused = True

STAGES = (2, 2, 3, 3, 3)                                             # convolutions per stage
CONV_INDEX = (0, 2, 5, 7, 10, 12, 14, 17, 19, 21, 24, 26, 28)        # their positions in torchvision's vgg16().features
TAP_INDEX = (3, 8, 15, 22, 29)                                       # the last ReLU of every stage (relu1_2 .. relu5_3)
VGG16_WIDTHS = (64, 128, 256, 512, 512)
MEAN, STD = (-.030, -.088, -.188), (.458, .448, .450)
EPS = 1e-10


class _Normalize(torch.autograd.Function):
    """u = a / (sqrt(sum_c a^2) + eps) with the closed-form gradient (0 for the norm's part where the norm is 0)."""

    @staticmethod
    def forward(ctx, a):
        n = a.square().sum(dim=1, keepdim=True).sqrt()
        ctx.save_for_backward(a, n)
        return a / (n + EPS)

    @staticmethod
    def backward(ctx, g):
        a, n = ctx.saved_tensors
        dot = (g * a).sum(dim=1, keepdim=True)
        den = n * (n + EPS).square()
        coef = torch.where(n > 0, dot / torch.where(n > 0, den, torch.ones_like(den)), torch.zeros_like(n))
        return g / (n + EPS) - a * coef


class VGG16Features(nn.Module):
    """torchvision's `vgg16().features[:30]` by layout (so its keys load) + the z-score buffers: the reference's `VGG16(BaseNet)`
    (networks.py:35-62, 87-95).  `widths`: channels per stage (the default is VGG16; tests build narrow nets).  Randomly initialised."""

    def __init__(self, widths=VGG16_WIDTHS):
        super().__init__()
        assert len(widths) == len(STAGES)
        self.widths = tuple(int(w) for w in widths)
        layers, cin = [], 3
        for s, (count, cout) in enumerate(zip(STAGES, self.widths)):
            if s > 0:
                layers.append(nn.MaxPool2d(kernel_size=2, stride=2))
            for _ in range(count):
                layers += [nn.Conv2d(cin, cout, 3, 1, 1), nn.ReLU()]
                cin = cout
        self.layers = nn.Sequential(*layers)
        assert tuple(i for i, m in enumerate(self.layers) if isinstance(m, nn.Conv2d)) == CONV_INDEX
        self.register_buffer('mean', torch.tensor(MEAN)[None, :, None, None])
        self.register_buffer('std', torch.tensor(STD)[None, :, None, None])
        self.requires_grad_(False)

    def plan(self):
        """[(kind, module)] in launch order (training/feature_loss.py): a tap behind the last ReLU of every stage."""
        return feature_loss.sequential_plan(self.layers, TAP_INDEX)

    def taps(self, z):
        """The five stage outputs of an already z-scored image (torch definition)."""
        return feature_loss.torch_taps(self.plan(), z)

    def forward(self, x):
        """x in [-1, 1] -> the five normalised taps (torch definition)."""
        return [_Normalize.apply(a) for a in self.taps((x - self.mean) / self.std)]


def _prep_torch(x, net, f, in_scale, in_shift):
    if f > 1:
        x = F.avg_pool2d(x, f)
    if in_scale != 1.0 or in_shift != 0.0:
        x = x * in_scale + in_shift
    return (x - net.mean) / net.std


# ---- the fused pass over the walkers of training/feature_loss.py, written against an `ops` object (tests/feature_loss_ref.py) -------------
def _fused_features(ops, lp, y, f, in_scale, in_shift):
    net = lp.net
    saved = feature_loss.forward_walk(ops, feature_loss.plan_of(net), lambda: ops.prep(y, net.mean, net.std, f, in_scale, in_shift), False)
    return ops.normalize(feature_loss.tapped(saved))


def _fused_forward(ops, lp, x, feats, lins, f, in_scale, in_shift):
    """-> (loss, saved): prep -> the net's chain -> head; `saved` is what `forward_walk` returns."""
    net = lp.net
    saved = feature_loss.forward_walk(ops, feature_loss.plan_of(net), lambda: ops.prep(x, net.mean, net.std, f, in_scale, in_shift), True)
    return ops.head(feature_loss.tapped(saved), feats, lins), saved


def _fused_backward(ops, lp, saved, feats, lins, f, in_scale, dloss):
    """-> the image gradient: head backward -> the chain backwards with the net's ReLU-gradient passes -> prep backward."""
    dtaps = ops.head_backward(feature_loss.tapped(saved), feats, lins, dloss)
    g = feature_loss.backward_walk(ops, feature_loss.plan_of(lp.net), saved, lp._relu_grad(ops, saved, dtaps))
    return ops.prep_backward(g, lp.net.std, f, in_scale)


class _FusedLpips(torch.autograd.Function):
    """prep -> the convolutions and pools of `lp.net` -> head, and the image gradient back through all of it, on the HIP entry points.  The
    only differentiable input is the image."""

    @staticmethod
    def forward(ctx, x, lp, feats, f, in_scale, in_shift):
        lins = lp._lin_vectors()
        loss, (acts, tap_at, idxs, sizes) = _fused_forward(feature_loss.HipOps.get(), lp, x, feats, lins, f, in_scale, in_shift)
        ctx.save_for_backward(*acts, *idxs)
        ctx.lp, ctx.feats, ctx.lins, ctx.prep, ctx.walk = lp, feats, lins, (f, in_scale), (tap_at, sizes)
        return loss

    @staticmethod
    def backward(ctx, dloss):
        (tap_at, sizes), (f, in_scale) = ctx.walk, ctx.prep
        acts, idxs = ctx.saved_tensors[:len(sizes)], ctx.saved_tensors[len(sizes):]
        dx = _fused_backward(feature_loss.HipOps.get(), ctx.lp, (acts, tap_at, idxs, sizes), ctx.feats, ctx.lins, f, in_scale,
                             dloss.to(torch.float32))
        return dx, None, None, None, None, None


class LPIPS(nn.Module):
    """`LPIPS('vgg')(x, y)` -> scalar, x and y [N, 3, H, W] in [-1, 1] (reference lpips.py:8-35).  `.net`: VGG16Features, `.lin`: five
    [1, C, 1, 1] non-negative weights without bias, in the reference's `Sequential(Identity, Conv2d)` layout.  No download: the weights are
    random until a state dict is loaded (`load_state_dict` of one saved from the reference class, or `load_torchvision_state_dict`).
    `training.lpips_alex.LPIPS` derives from this class: what a net sets is `_make_net`, `_on_hip`, `_sides_ok`, `_check_sides` and
    `_relu_grad`."""

    def __init__(self, net_type='vgg', version='0.1', widths=VGG16_WIDTHS):
        super().__init__()
        assert version in ['0.1'], 'v0.1 is only supported now'
        self.net = self._make_net(net_type, widths)
        self.lin = nn.ModuleList([nn.Sequential(nn.Identity(), nn.Conv2d(c, 1, 1, 1, 0, bias=False)) for c in self.net.widths])
        with torch.no_grad():
            for l in self.lin:
                l[1].weight.uniform_(0, 1)          # (the trained weights are non-negative)
        self.requires_grad_(False)

    @staticmethod
    def _make_net(net_type, widths):
        if net_type in ('alex', 'squeeze'):
            raise NotImplementedError(f"net_type '{net_type}' is not supported: AlexNet and SqueezeNet need 11x11, 5x5 and strided "
                                      "convolutions, which the HIP convolution kernel does not have; use 'vgg'")
        if net_type != 'vgg':
            raise NotImplementedError('choose net_type from [vgg].')
        return VGG16Features(widths)

    def load_torchvision_state_dict(self, features, lin):
        """`features`: a state dict with torchvision's keys (`features.N.weight`, `features.N.bias`, or without the prefix; other keys, such
        as the classifier's, are ignored); `lin`: the five lin tensors ([1, C, 1, 1] or [C]) in tap order."""
        sd = feature_loss.torchvision_convs(features, {i: f'net.layers.{i}' for i, m in enumerate(self.net.layers) if isinstance(m, nn.Conv2d)})
        assert len(lin) == len(self.lin)
        for k, w in enumerate(lin):
            sd[f'lin.{k}.1.weight'] = torch.as_tensor(w).reshape(1, -1, 1, 1)
        sd['net.mean'], sd['net.std'] = self.net.mean, self.net.std
        self.load_state_dict(sd)
        return self

    def _lin_vectors(self):
        return [networks._wgrad_cache.get((l[1].weight,), lambda w=l[1].weight: w.detach().reshape(-1).float().contiguous(), key='lpips_lin')
                for l in self.lin]

    def _on_hip(self, x, feats=None):
        return feature_loss.on_hip(fused, x, feats, self.parameters(), False, (), True)

    @staticmethod
    def _sides_ok(h, w):
        return (h >> 4) >= 1 and (w >> 4) >= 1

    def _check_sides(self, x, f):
        """A net with a minimum side raises ValueError here, on every path; this one leaves a small image to the torch definition."""

    def _relu_grad(self, ops, saved, dtaps):
        """The ReLU gradients of `backward_walk`: a stage's last ReLU is a tap with (but for the last stage) a pool behind it."""
        acts = saved[0]

        def relu_grad(j, behind, k, g):
            return ops.stage_backward(acts[j], g, dtaps[k]) if behind == 'tap' else ops.relu_backward(g, acts[j])
        return relu_grad

    def _takes_hip(self, x, feats, f):
        H, W = x.shape[2:]
        return self._on_hip(x, feats) and H % f == 0 and W % f == 0 and self._sides_ok(H // f, W // f)

    def features(self, y):
        """The five normalised taps of y (in [-1, 1]), detached: what a projector caches for its target."""
        return self._features(y, 1, 1.0, 0.0)

    def _features(self, y, f, in_scale, in_shift):
        self._check_sides(y, f)
        with torch.no_grad():
            if self._takes_hip(y, None, f):
                return _fused_features(feature_loss.HipOps.get(), self, y, f, in_scale, in_shift)
            z = _prep_torch(y, self.net, f, in_scale, in_shift)
            return [_Normalize.apply(a).detach() for a in self.net.taps(z)]

    def distance_to(self, x, feats):
        """LPIPS(x, y) for feats = features(y): the same value as forward(x, y)."""
        return self._distance(x, feats, 1, 1.0, 0.0)

    def _distance(self, x, feats, f, in_scale, in_shift):
        self._check_sides(x, f)
        if self._takes_hip(x, feats, f):
            return _FusedLpips.apply(x, self, list(feats), f, in_scale, in_shift)
        z = _prep_torch(x, self.net, f, in_scale, in_shift)
        total = None
        for a, t, l in zip(self.net.taps(z), feats, self.lin):
            d = ((_Normalize.apply(a) - t).square() * l[1].weight).sum(dim=1).mean(dim=(1, 2)).sum()
            total = d if total is None else total + d
        return total / x.shape[0]

    def forward(self, x, y):
        return self.distance_to(x, self.features(y))


def lpips_distance(target, lpips, size=256):
    """The `distance` of `projection.project` that measures LPIPS to `target` ([1, 3, H, W], 0..255): images (0..255) are area-down-sampled to
    `size` when larger (w_projector_ide3d.py:73-74, 106-107), mapped to [-1, 1] and compared with the target's cached features by
    `lpips.distance_to`, so the closure returns LPIPS itself.  The reference projector measures the squared distance of the `vgg16.pt`
    TorchScript's `return_lpips=True` features (:108-111); the reference class (inversion/criteria/lpips) is the same definition — the same
    net, taps, normalisation and lin weights (that script folds sqrt(lin / (h w)) into its feature vector) — hence the same quantity.
    On the HIP path the down-sampling, the rescaling and the z-score are one launch; that needs an integer area factor."""
    def small(img):
        """(image, area factor still to apply): a square integer factor is left to the distance's first pass, any other is resized here."""
        h, w = img.shape[2:]
        if h <= size:                                    # (the reference's test: `if img.shape[2] > 256`)
            return img, 1
        if h % size == 0 and w == h:
            return img, h // size
        return F.interpolate(img, size=(size, size), mode='area'), 1

    with torch.no_grad():
        t, f = small(target.detach())
        feats = lpips._features(t.contiguous(), f, 2.0 / 255.0, -1.0)

    def distance(images):
        img, f = small(images)
        return lpips._distance(img.contiguous(), feats, f, 2.0 / 255.0, -1.0)
    return distance
