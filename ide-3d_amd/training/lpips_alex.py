"""The AlexNet LPIPS distance — the reference's default perceptual loss — with a HIP forward and image gradient.

Reference: `inversion/criteria/lpips/{lpips,networks,utils}.py` with `net_type='alex'`, the default of the class (lpips.py:16): what the
hybrid encoder's training step builds (apps/train_hybrid_encoder.py:235), what the PTI coaches minimise (`lpips_type = 'alex'`,
inversion/configs/hyperparameters.py, base_coach.py:44) and what apps/calc_losses_on_images.py measures.  The z-score, the normalisation,
the `lin` head and the final sum are those of the VGG16 form (training/lpips.py, where the formulas stand); the feature net is
torchvision's `alexnet().features[:12]` with a tap behind every ReLU (networks.py:76-84):

    0  Conv2d(3,   64, 11, stride 4, padding 2) + ReLU   -> tap 1
       MaxPool2d(3, 2)                                      (no padding, floor)
    3  Conv2d(64, 192, 5, padding 2) + ReLU              -> tap 2
       MaxPool2d(3, 2)
    6  Conv2d(192, 384, 3, padding 1) + ReLU             -> tap 3
    8  Conv2d(384, 256, 3, padding 1) + ReLU             -> tap 4
    10 Conv2d(256, 256, 3, padding 1) + ReLU             -> tap 5

Parameter and buffer names equal the reference class's (`net.layers.{0,3,6,8,10}.{weight,bias}`, `net.mean`, `net.std`,
`lin.{0..4}.1.weight`); `load_torchvision_state_dict` takes torchvision's `features.N.*` keys and the five `lin` tensors, as a list or under
the `lin{k}.model.1.weight` keys of the file the reference reads from `pretrained_models/alex.pth`.  Nothing here downloads: WITHOUT LOADED
WEIGHTS THE NET IS RANDOMLY INITIALISED and the value is not LPIPS.  The gradient of the norm at an all-zero pixel is 0 as in
training/lpips.py.  An image side below 31 (after the area factor) leaves the second pool without a window and raises ValueError on
every path.

`fused` (module switch): fp32 CUDA images, dense NCHW, frozen parameters and (for `lpips_distance`) an integer area factor run on the HIP
path, one autograd Function that returns the image gradient only.  The convolution kernel has k = 1 and k = 3 at stride 1, so the 11x11
stride-4 stem and the 5x5 layer run as a patch unfolding followed by a 1x1 launch (the face parser's 7x7 stem does the same), their input
gradients as a 1x1 launch on the transposed weight followed by the unfolding's adjoint:

    forward    prep -> unfold2d(11, 4, 2) -> modconv2d 1x1 (363 -> c1, bias, ReLU)                       tap 1
               maxpool3s2p0 (+idx) -> unfold2d(5, 1, 2) -> modconv2d 1x1 (25 c1 -> c2, bias, ReLU)       tap 2
               maxpool3s2p0 (+idx) -> 3 x modconv2d 3x3 (bias, ReLU)                                     taps 3..5
               lpips_head
    backward   lpips_head_backward
               tap 5: lpips_tap_backward(g = None)       -> modconv2d 3x3 on the transposed-flipped weights
               tap 4, 3: lpips_tap_backward(g as it is)  -> modconv2d 3x3 likewise
               tap 2: lpips_tap_backward(g, idx)         -> modconv2d 1x1 on the transposed weight (c2 -> 25 c1) -> fold2d(5, 1, 2)
               tap 1: lpips_tap_backward(g, idx)         -> modconv2d 1x1 (c1 -> 363) -> fold2d(11, 4, 2)
               lpips_prep_backward

Every ReLU gradient sits at a tap, so ide3d_modconv_act_backward is not called.  Everything else — CPU, other dtypes, `fused = False`,
parameters that require grad — takes the torch definition in this file.
"""

import torch
import torch.nn as nn
import torch.nn.functional as F

from training import lpips, networks
from training.lpips import MEAN, STD, _Normalize, _prep_torch

# True: what the HIP path takes (see above) runs on it.  False: always the torch definition.
fused = True

ALEX_WIDTHS = (64, 192, 384, 256, 256)
CONV_INDEX = (0, 3, 6, 8, 10)                                        # positions in torchvision's alexnet().features
GEOMETRY = ((11, 4, 2), (5, 1, 2), (3, 1, 1), (3, 1, 1), (3, 1, 1))  # (kernel, stride, padding) per convolution
POOL_BEHIND = (True, True, False, False, False)                      # a MaxPool2d(3, 2) between this tap and the next convolution
MIN_SIDE = 31                                                        # stem (H - 7) // 4 + 1 >= 7, so that two pools leave 1 x 1


class AlexNetFeatures(nn.Module):
    """torchvision's `alexnet().features[:12]` by layout (so its keys load) + the z-score buffers: the reference's `AlexNet(BaseNet)`
    (networks.py:35-62, 76-84; its layer 12, the last pool, is never run).  `widths`: channels per tap (the default is AlexNet; tests build
    narrow nets).  Randomly initialised."""

    def __init__(self, widths=ALEX_WIDTHS):
        super().__init__()
        assert len(widths) == len(GEOMETRY)
        self.widths = tuple(int(w) for w in widths)
        layers, cin = [], 3
        for cout, (k, s, p), pool in zip(self.widths, GEOMETRY, POOL_BEHIND):
            layers += [nn.Conv2d(cin, cout, k, s, p), nn.ReLU()]
            if pool:
                layers.append(nn.MaxPool2d(kernel_size=3, stride=2))
            cin = cout
        self.layers = nn.Sequential(*layers)
        assert tuple(i for i, m in enumerate(self.layers) if isinstance(m, nn.Conv2d)) == CONV_INDEX and len(self.layers) == 12
        self.register_buffer('mean', torch.tensor(MEAN)[None, :, None, None])
        self.register_buffer('std', torch.tensor(STD)[None, :, None, None])
        self.requires_grad_(False)

    def convs(self):
        return [self.layers[i] for i in CONV_INDEX]

    def taps(self, z):
        """The five ReLU outputs of an already z-scored image (torch definition)."""
        out, h = [], z
        for conv, pool in zip(self.convs(), POOL_BEHIND):
            h = F.relu(conv(h))
            out.append(h)
            if pool:
                h = F.max_pool2d(h, 3, 2)
        return out

    def forward(self, x):
        """x in [-1, 1] -> the five normalised taps (torch definition)."""
        return [_Normalize.apply(a) for a in self.taps((x - self.mean) / self.std)]


def _weight_1x1(conv, transposed):
    """A k x k convolution's weight as the 1x1 weight over its unfolded patches, [cout, cin k k, 1, 1], or that of its input gradient,
    [cin k k, cout, 1, 1]; a 3x3 convolution's own weight, or its transposed-flipped one.  Cached per weight tensor, so that the packed
    copies in the convolution's workspace are reused across steps."""
    w = conv.weight
    if conv.kernel_size[0] == 3:
        return networks._grad_weight(w, True) if transposed else w
    if transposed:
        return networks._wgrad_cache.get((w,), lambda: w.detach().reshape(w.shape[0], -1).t().contiguous()[:, :, None, None], key='alex_1x1_t')
    return networks._wgrad_cache.get((w,), lambda: w.detach().reshape(w.shape[0], -1, 1, 1), key='alex_1x1')


def _hip_taps(net, z, want_idx):
    """-> (the five ReLU outputs, the two pools' winner bytes or Nones, the input size of every convolution) on the HIP entry points."""
    from torch_utils import hip_plugin
    A, conv2d = hip_plugin.LpipsAlexPlugin, networks._modconv_plugin.modconv2d
    acts, idxs, sizes, h = [], [], [], z
    for conv, (k, s, p), pool in zip(net.convs(), GEOMETRY, POOL_BEHIND):
        sizes.append(tuple(h.shape[2:]))
        if k != 3:
            h = A.unfold2d(h, k, s, p)
        h = conv2d(h, _weight_1x1(conv, False), None, None, None, 0.0, conv.bias, 3, 0.0, 1.0, -1.0)
        acts.append(h)
        if pool:
            h, idx = A.maxpool3s2p0(h, want_idx)
            idxs.append(idx)
    return acts, idxs, sizes


class _FusedLpipsAlex(torch.autograd.Function):
    """prep -> 5 convolutions (2 of them over unfolded patches), 2 pools -> head, and the image gradient back through all of it, on the HIP
    entry points.  The only differentiable input is the image."""

    @staticmethod
    def forward(ctx, x, lp, feats, f, in_scale, in_shift):
        from torch_utils import hip_plugin
        P, net = hip_plugin.LpipsPlugin, lp.net
        acts, idxs, sizes = _hip_taps(net, P.prep(x, net.mean, net.std, f, in_scale, in_shift), True)
        lins = lp._lin_vectors()
        loss = P.head(acts, feats, lins)
        ctx.save_for_backward(*acts, *idxs)
        ctx.lp, ctx.feats, ctx.lins, ctx.prep, ctx.sizes = lp, feats, lins, (f, in_scale), sizes
        return loss

    @staticmethod
    def backward(ctx, dloss):
        from torch_utils import hip_plugin
        P, A, conv2d = hip_plugin.LpipsPlugin, hip_plugin.LpipsAlexPlugin, networks._modconv_plugin.modconv2d
        acts, idxs = ctx.saved_tensors[:len(GEOMETRY)], list(ctx.saved_tensors[len(GEOMETRY):])
        net = ctx.lp.net
        dtaps = P.head_backward(list(acts), ctx.feats, ctx.lins, dloss.to(torch.float32))
        g = None
        for j in reversed(range(len(GEOMETRY))):
            k, s, p = GEOMETRY[j]
            dz = A.tap_backward(acts[j], g, idxs.pop() if POOL_BEHIND[j] else None, dtaps[j])
            g = conv2d(dz, _weight_1x1(net.convs()[j], True), None, None, None, 0.0, None, 1, 0.0, 1.0, -1.0)
            if k != 3:
                g = A.fold2d(g, ctx.sizes[j], k, s, p)
        f, in_scale = ctx.prep
        return P.prep_backward(g, net.std, f, in_scale), None, None, None, None, None


class LPIPS(lpips.LPIPS):
    """`LPIPS()(x, y)` -> scalar, x and y [N, 3, H, W] in [-1, 1] with H, W >= 31: the reference class at its default `net_type='alex'`
    (lpips.py:8-35).  `.net`: AlexNetFeatures, `.lin`: five [1, C, 1, 1] non-negative weights without bias, in the reference's
    `Sequential(Identity, Conv2d)` layout.  The public and closure surface is that of `training.lpips.LPIPS` (`features`, `distance_to`,
    `forward` are inherited), so `training.lpips.lpips_distance(target, m)` and `projection.project(distance=...)` take it as they take the
    VGG16 form.  No download: the weights are random until a state dict is loaded."""

    def __init__(self, net_type='alex', version='0.1', widths=ALEX_WIDTHS):
        nn.Module.__init__(self)
        assert version in ['0.1'], 'v0.1 is only supported now'
        if net_type == 'vgg':
            raise NotImplementedError("net_type 'vgg' is training.lpips.LPIPS('vgg'); this module holds the AlexNet form")
        if net_type == 'squeeze':
            raise NotImplementedError("net_type 'squeeze' is not supported: SqueezeNet's fire modules are not built; use 'alex' or "
                                      "training.lpips.LPIPS('vgg')")
        if net_type != 'alex':
            raise NotImplementedError('choose net_type from [alex].')
        self.net = AlexNetFeatures(widths)
        self.lin = nn.ModuleList([nn.Sequential(nn.Identity(), nn.Conv2d(c, 1, 1, 1, 0, bias=False)) for c in self.net.widths])
        with torch.no_grad():
            for l in self.lin:
                l[1].weight.uniform_(0, 1)          # (the trained weights are non-negative)
        self.requires_grad_(False)

    def load_torchvision_state_dict(self, features, lin):
        """`features`: a state dict with torchvision's keys (`features.N.weight`, `features.N.bias`, or without the prefix; other keys, such
        as the classifier's, are ignored); `lin`: the five lin tensors ([1, C, 1, 1] or [C]) in tap order, or the state dict of the
        reference's `alex.pth` (`lin{k}.model.1.weight`)."""
        sd = {}
        for i in CONV_INDEX:
            for name in ('weight', 'bias'):
                key = f'features.{i}.{name}' if f'features.{i}.{name}' in features else f'{i}.{name}'
                sd[f'net.layers.{i}.{name}'] = features[key]
        if isinstance(lin, dict):
            lin = [lin[f'lin{k}.model.1.weight'] for k in range(len(GEOMETRY))]
        assert len(lin) == len(GEOMETRY)
        for k, w in enumerate(lin):
            sd[f'lin.{k}.1.weight'] = torch.as_tensor(w).reshape(1, -1, 1, 1)
        sd['net.mean'], sd['net.std'] = self.net.mean, self.net.std
        self.load_state_dict(sd)
        return self

    def _on_hip(self, x, feats=None):
        if not (fused and isinstance(x, torch.Tensor) and x.is_cuda and x.dtype == torch.float32 and x.ndim == 4 and x.shape[1] == 3
                and x.is_contiguous() and self._frozen() and next(self.parameters()).dtype == torch.float32
                and next(self.parameters()).device == x.device):
            return False
        if feats is not None and not all(t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and not t.requires_grad for t in feats):
            return False
        return networks._modconv_init()

    @staticmethod
    def _sides_ok(h, w):
        return h >= MIN_SIDE and w >= MIN_SIDE

    def _check_sides(self, x, f):
        h, w = x.shape[2] // f, x.shape[3] // f
        if not self._sides_ok(h, w):
            raise ValueError(f'AlexNet LPIPS needs image sides of at least {MIN_SIDE} (after the area factor), got {h} x {w}: '
                             'the second MaxPool2d(3, 2) would have no window')

    def _features(self, y, f, in_scale, in_shift):
        self._check_sides(y, f)
        with torch.no_grad():
            if self._on_hip(y) and y.shape[2] % f == 0 and y.shape[3] % f == 0:
                from torch_utils import hip_plugin
                P = hip_plugin.LpipsPlugin
                return P.normalize(_hip_taps(self.net, P.prep(y, self.net.mean, self.net.std, f, in_scale, in_shift), False)[0])
            z = _prep_torch(y, self.net, f, in_scale, in_shift)
            return [_Normalize.apply(a).detach() for a in self.net.taps(z)]

    def _distance(self, x, feats, f, in_scale, in_shift):
        self._check_sides(x, f)
        if self._on_hip(x, feats) and x.shape[2] % f == 0 and x.shape[3] % f == 0:
            return _FusedLpipsAlex.apply(x, self, list(feats), f, in_scale, in_shift)
        z = _prep_torch(x, self.net, f, in_scale, in_shift)
        total = None
        for a, t, l in zip(self.net.taps(z), feats, self.lin):
            d = ((_Normalize.apply(a) - t).square() * l[1].weight).sum(dim=1).mean(dim=(1, 2)).sum()
            total = d if total is None else total + d
        return total / x.shape[0]
