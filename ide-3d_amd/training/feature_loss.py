"""What the three tapped feature-net losses share (training/lpips.py, training/lpips_alex.py, training/vgg_loss.py).

Each of them is a prep pass, a chain of `convolution + ReLU` launches with max-pools between them and taps at some ReLU outputs, a loss head
over the taps, and the same chain backwards.  A net describes its chain as a plan, `net.plan()`: [(kind, module)] in launch order with kind
in 'conv' (an `nn.Conv2d` and its ReLU), 'pool' (an `nn.MaxPool2d`: 2x2 stride 2, or 3x3 stride 2 without padding) and 'tap' (the ReLU
output in front of it is a tap).  `forward_walk` and `backward_walk` run a plan on an `ops` object: `HipOps` here, a float64 torch
restatement in tests/feature_loss_ref.py, so the walkers are checked against autograd without a GPU.  What differs between the losses on the
way back is the ReLU-gradient pass of each convolution, which the loss hands to `backward_walk` as `relu_grad`.
"""

import torch
import torch.nn as nn
import torch.nn.functional as F

from training import networks


class HipOps:
    """The launches of the fused passes.  conv, relu_backward: ide3d_modconv2d, ide3d_modconv_act_backward (training/networks.py);
    everything else: the plugin methods over csrc/lpips.hip, csrc/lpips_alex.hip and csrc/vgg_loss.hip."""

    _instance = None

    @classmethod
    def get(cls):
        if cls._instance is None:
            cls._instance = cls()
        return cls._instance

    def __init__(self):
        from torch_utils import hip_plugin
        P, A, V = hip_plugin.LpipsPlugin, hip_plugin.LpipsAlexPlugin, hip_plugin.VggLossPlugin
        self.prep, self.prep_backward, self.maxpool2, self.stage_backward = P.prep, P.prep_backward, P.maxpool2, P.stage_backward
        self.normalize, self.head, self.head_backward = P.normalize, P.head, P.head_backward
        self.unfold2d, self.fold2d, self.maxpool3s2p0, self.tap_backward = A.unfold2d, A.fold2d, A.maxpool3s2p0, A.tap_backward
        self.feat_l1, self.feat_l1_tap_backward, self.maxpool2_relu_backward = V.feat_l1, V.feat_l1_tap_backward, V.maxpool2_relu_backward
        self.conv, self.relu_backward = networks.plain_conv, networks.relu_backward


def on_hip(fused, x, feats, params, every, buffers, grad_plugin):
    """The gate of the HIP path: `fused` (the calling module's switch), a dense fp32 CUDA image [n, 3, H, W], frozen `params` (an iterator,
    walked once) of which the first - with `every`, each - is fp32 on the image's device, `buffers` on that device, dense fp32 CUDA cached
    features without grad (when given), and the plugins: the convolution's, and the activation gradient's when `grad_plugin` (a loss whose
    every ReLU gradient sits at a tap does not need it)."""
    if not (fused and isinstance(x, torch.Tensor) and x.is_cuda and x.dtype == torch.float32 and x.ndim == 4 and x.shape[1] == 3
            and x.is_contiguous() and all(b.device == x.device for b in buffers)):
        return False
    check = True
    for p in params:
        if p.requires_grad or (check and not (p.dtype == torch.float32 and p.device == x.device)):
            return False
        check = every
    if feats is not None and not all(t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and not t.requires_grad for t in feats):
        return False
    return networks._modconv_init() and (not grad_plugin or networks._modconv_grad_init())


def torchvision_convs(features, prefix_of):
    """{f'{prefix_of[i]}.weight' / '.bias': tensor} from a state dict with torchvision's keys (`features.N.weight`, `features.N.bias`, or
    without the prefix; other keys, such as the classifier's, are ignored).  `prefix_of`: {position N: the module's name here}."""
    sd = {}
    for i, prefix in prefix_of.items():
        for name in ('weight', 'bias'):
            key = f'features.{i}.{name}'
            sd[f'{prefix}.{name}'] = features[key if key in features else f'{i}.{name}']
    return sd


def _weight_1x1(w, transposed):
    """A k x k convolution that is not 3x3 runs as a 1x1 launch over its unfolded patches, on [cout, cin k k, 1, 1], its input gradient on
    [cin k k, cout, 1, 1].  Cached per weight tensor, so that the packed copies in the convolution's workspace are reused across steps."""
    if transposed:
        return networks._wgrad_cache.get((w,), lambda: w.detach().reshape(w.shape[0], -1).t().contiguous()[:, :, None, None], key='alex_1x1_t')
    return networks._wgrad_cache.get((w,), lambda: w.detach().reshape(w.shape[0], -1, 1, 1), key='alex_1x1')


def sequential_plan(layers, tap_relus):
    """The plan of an `nn.Sequential` of Conv2d, ReLU and MaxPool2d modules; `tap_relus`: the positions of the ReLUs whose outputs are taps."""
    kinds = {nn.Conv2d: 'conv', nn.MaxPool2d: 'pool'}
    return [(kinds.get(type(m), 'tap'), m) for i, m in enumerate(layers) if type(m) in kinds or i in tap_relus]


def plan_of(net):
    """`net.plan()`, built on first use and kept on the net (its modules never change), so that a call does not pay for it."""
    if '_plan' not in net.__dict__:
        net.__dict__['_plan'] = net.plan()
    return net.__dict__['_plan']


def tapped(saved):
    """The taps among the ReLU outputs that `forward_walk` returned."""
    acts, tap_at = saved[:2]
    return [acts[i] for i in tap_at]


def torch_taps(plan, z):
    """The taps of the prepped image z by the torch definition (differentiable by autograd)."""
    out, h = [], z
    for kind, m in plan:
        if kind == 'tap':
            out.append(h)
        else:
            h = F.relu(m(h)) if kind == 'conv' else m(h)
    return out


def forward_walk(ops, plan, z, want_idx):
    """The chain on the prepped image -> (the ReLU output of every convolution, the positions of the taps among them, the 3x3 pools' winner
    bytes (Nones without `want_idx`), the input size of every convolution): what `backward_walk` reads.  `z` is a call that returns the
    prepped image: an argument would stay alive in the caller's frame for the whole walk, this way it is released behind the first
    convolution."""
    acts, tap_at, idxs, sizes, h = [], [], [], [], z()
    for kind, m in plan:
        if kind == 'conv':
            k, w = m.kernel_size[0], m.weight
            sizes.append(tuple(h.shape[2:]))
            if k != 3:
                h, w = ops.unfold2d(h, k, m.stride[0], m.padding[0]), _weight_1x1(w, False)
            h = ops.conv(h, w, m.bias, True)
            acts.append(h)
        elif kind == 'pool':
            if m.kernel_size == 2:
                h = ops.maxpool2(h)
            else:
                h, idx = ops.maxpool3s2p0(h, want_idx)
                idxs.append(idx)
        else:
            tap_at.append(len(acts) - 1)
    return acts, tap_at, idxs, sizes


def backward_walk(ops, plan, saved, relu_grad):
    """The chain backwards -> the gradient of the prepped image.  For every convolution j, last to first: `relu_grad(j, behind, k, g)` gives
    the gradient in front of its ReLU from g, the gradient of the next convolution's input (None behind the last one; still pooled where a
    pool lies between), then the convolution runs on the derived weight and folds where the forward pass unfolded.  `behind` is what follows
    the ReLU directly ('tap', 'pool' or 'conv'), k the tap's index when that is a tap, else None."""
    acts, tap_at, _, sizes = saved
    j, k, g, behind = len(acts), len(tap_at), None, None
    for kind, m in reversed(plan):
        if kind != 'conv':
            behind = kind
            k -= kind == 'tap'
            continue
        j -= 1
        dz = relu_grad(j, behind, k if behind == 'tap' else None, g)
        if m.kernel_size[0] == 3:
            g = ops.conv(dz, networks._grad_weight(m.weight, True), None, False)
        else:
            g = ops.fold2d(ops.conv(dz, _weight_1x1(m.weight, True), None, False), sizes[j], m.kernel_size[0], m.stride[0], m.padding[0])
        behind = 'conv'
    return g
