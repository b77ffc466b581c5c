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
parameters that require grad — takes the torch definition of training/lpips.py, whose fused pass this is too: the walkers of
training/feature_loss.py over `AlexNetFeatures.plan()` make the launches above (the unfold / 1x1 / fold bracketing is theirs).
"""

import torch
import torch.nn as nn

from training import feature_loss, lpips
from training.lpips import MEAN, STD, _Normalize

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

    def plan(self):
        """[(kind, module)] in launch order (training/feature_loss.py): a tap behind every convolution."""
        return feature_loss.sequential_plan(self.layers, [i + 1 for i in CONV_INDEX])

    def taps(self, z):
        """The five ReLU outputs of an already z-scored image (torch definition)."""
        return feature_loss.torch_taps(self.plan(), z)

    def forward(self, x):
        """x in [-1, 1] -> the five normalised taps (torch definition)."""
        return [_Normalize.apply(a) for a in self.taps((x - self.mean) / self.std)]


class LPIPS(lpips.LPIPS):
    """`LPIPS()(x, y)` -> scalar, x and y [N, 3, H, W] in [-1, 1] with H, W >= 31: the reference class at its default `net_type='alex'`
    (lpips.py:8-35).  `.net`: AlexNetFeatures, `.lin`: five [1, C, 1, 1] non-negative weights without bias, in the reference's
    `Sequential(Identity, Conv2d)` layout.  The public and closure surface is that of `training.lpips.LPIPS` (`features`, `distance_to`,
    `forward` are inherited, and so are the fused pass and the torch definition behind them), so `training.lpips.lpips_distance(target, m)`
    and `projection.project(distance=...)` take it as they take the VGG16 form.  No download: the weights are random until a state dict is
    loaded."""

    def __init__(self, net_type='alex', version='0.1', widths=ALEX_WIDTHS):
        super().__init__(net_type, version, widths)

    @staticmethod
    def _make_net(net_type, widths):
        if net_type == 'vgg':
            raise NotImplementedError("net_type 'vgg' is training.lpips.LPIPS('vgg'); this module holds the AlexNet form")
        if net_type == 'squeeze':
            raise NotImplementedError("net_type 'squeeze' is not supported: SqueezeNet's fire modules are not built; use 'alex' or "
                                      "training.lpips.LPIPS('vgg')")
        if net_type != 'alex':
            raise NotImplementedError('choose net_type from [alex].')
        return AlexNetFeatures(widths)

    def load_torchvision_state_dict(self, features, lin):
        """`features`, `lin`: as `training.lpips.LPIPS.load_torchvision_state_dict` takes them; `lin` may also be the state dict of the
        reference's `alex.pth` (`lin{k}.model.1.weight`)."""
        if isinstance(lin, dict):
            lin = [lin[f'lin{k}.model.1.weight'] for k in range(len(self.lin))]
        return super().load_torchvision_state_dict(features, lin)

    def _on_hip(self, x, feats=None):
        return feature_loss.on_hip(fused, x, feats, self.parameters(), False, (), False)

    @staticmethod
    def _sides_ok(h, w):
        return h >= MIN_SIDE and w >= MIN_SIDE

    def _check_sides(self, x, f):
        h, w = x.shape[2] // f, x.shape[3] // f
        if not self._sides_ok(h, w):
            raise ValueError(f'AlexNet LPIPS needs image sides of at least {MIN_SIDE} (after the area factor), got {h} x {w}: '
                             'the second MaxPool2d(3, 2) would have no window')

    def _relu_grad(self, ops, saved, dtaps):
        """The ReLU gradients of `backward_walk`: every ReLU output is a tap; the first two have a 3x3 pool behind them, whose gradient is
        routed through the winner bytes."""
        acts, _, idxs, _ = saved

        def relu_grad(j, behind, k, g):
            return ops.tap_backward(acts[j], g, idxs[sum(POOL_BEHIND[:j])] if POOL_BEHIND[j] else None, dtaps[k])
        return relu_grad
