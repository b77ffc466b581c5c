"""The StyleGAN2 discriminator's adversarial loss with a HIP forward and image gradient.

Reference: the adversarial term of the hybrid encoder's training step (apps/train_hybrid_encoder.py:100-117, 198, 211, 302, 313),

    rec_pred = D(torch.cat([rec_real_img, rec_real_img_raw], 1), real_label)        # training.discriminator.Discriminator
    adv_loss = g_nonsaturating_loss(rec_pred)                                       # softplus(-rec_pred).mean()

back-propagated through the discriminator into the rendered images, and the discriminator's own logistic loss with its R1 penalty.
`ADVLoss(D)` wraps a discriminator: `logits`, `cmap` (the mapped label: it does not depend on the image, so a caller with a fixed label
computes it once and passes `cmap=`), `generator_loss` (= `forward`), `discriminator_loss`; `adv_distance(...)` is the closure
`training.projection.project(distance=...)` takes; `d_logistic_loss`, `g_nonsaturating_loss` and `d_r1_loss` are the training app's three
functions on logits (R1 differentiates twice, through the PyTorch definition).

PRECISION: the loss evaluates D in fp32 on both of its paths (`force_fp32=True`, the default).  Pickled discriminators carry
`num_fp16_res=4` with `conv_clamp=256`: the clamp stays, the fp16 casts of the four highest resolutions go, so values differ from an fp16
evaluation by fp16 rounding.  `force_fp32=False` keeps the blocks' own dtypes and always takes the PyTorch definition.

`fused` (module switch): the HIP path is taken when every parameter of D is frozen, D is a `resnet` discriminator whose layers all have
the covered form (lrelu or linear, a 2-D square resample filter, no clamp behind a linear activation), the image is a dense float32 CUDA
tensor [n, img_channels, R, R] with n <= 8 and `cmap` does not require grad.  Then one autograd Function runs, per block, `fromrgb` (first
block), the skip branch (FIR decimation + a 1x1 launch), `conv0`, `conv1` (FIR + the stride-2 launch) and the join, then
ide3d_minibatch_std, the epilogue convolution, ide3d_linear + a leaky-ReLU ide3d_bias_act, ide3d_linear for `out` and ide3d_adv_head; its
backward mirrors this with ide3d_adv_head_backward, ide3d_linear_backward_input, ide3d_modconv_act_backward, ide3d_minibatch_std_backward,
the convolutions on derived weights, the FIR adjoints and one ide3d_residual_join per block, and returns the image gradient only.
Everything else - CPU tensors, a trainable D, other dtypes, n > 8, the other architectures, a label that requires grad, R1,
`fused = False` - is the PyTorch definition.  `last_path` of the module says which ran.
`arith` (module switch): the per-call arithmetic of the convolutions on the HIP path (0 = the process default, see
`hip_plugin.conv_arithmetic`).
"""

import numpy as np
import torch
import torch.nn.functional as F
from torch.autograd.function import once_differentiable

from torch_utils.ops import bias_act
from training import networks
from training.discriminator import Discriminator

# True: what the HIP path takes (see above) runs on it.  False: always the PyTorch definition.  Shipped value: see DESIGN.md section 5.38.
fused = True
arith = 0

MAX_BATCH = 8          # the rows of one ide3d_linear launch


# ---- the training app's three functions (apps/train_hybrid_encoder.py:100-117) ----------------------------------------------------------------
def d_logistic_loss(real_pred, fake_pred):
    """softplus(-D(real)).mean() + softplus(D(fake)).mean()."""
    return F.softplus(-real_pred).mean() + F.softplus(fake_pred).mean()


def g_nonsaturating_loss(fake_pred):
    """softplus(-D(fake)).mean()."""
    return F.softplus(-fake_pred).mean()


def d_r1_loss(real_pred, real_img):
    """The R1 penalty mean_i |d sum(real_pred) / d real_img_i|^2, itself differentiable (`create_graph=True`): `real_pred` must come from the
    PyTorch definition (`Discriminator.forward`, or `ADVLoss.logits` on an image that requires grad)."""
    grad, = torch.autograd.grad(outputs=real_pred.sum(), inputs=real_img, create_graph=True)
    return grad.square().reshape(grad.shape[0], -1).sum(1).mean()


# ---- the fused pass ----------------------------------------------------------------------------------------------------------------------------
def _form(lay):
    """The `_plain_conv_launch` form of a discriminator layer, or None when the walker does not cover it."""
    k = lay.weight.shape[-1]
    if not (lay.up == 1 and lay.down in (1, 2) and k in (1, 3) and lay.weight.shape[-2] == k and lay.activation in ('linear', 'lrelu')):
        return None
    # bias_act's linear activation passes the gradient through the clamp unmasked, ide3d_modconv_act_backward masks it (networks._plain_conv_form)
    if lay.conv_clamp is not None and lay.activation == 'linear':
        return None
    if lay.down == 1:
        return 'conv'
    f = lay.resample_filter
    if f.ndim != 2 or f.shape[0] != f.shape[1]:
        return None
    return 'fir_conv1' if k == 1 else 'fir_conv3'


def _conv(lay, x, gain=1):
    """-> (y, record for `_conv_grad`): a frozen Conv2dLayer as its inference branches launch it."""
    k = lay.weight.shape[-1]
    ws = networks._scaled_weight(lay.weight, lay.weight_gain)
    clamp = lay.conv_clamp * gain if lay.conv_clamp is not None else None
    pads = networks._plain_fir_pads(lay, k) if lay.down == 2 else (0, 0)
    _, y = networks._plain_conv_launch(x, ws, lay.bias, _form(lay), lay.resample_filter, pads, lay.activation, lay.act_gain * gain, clamp, arith)
    return y, (lay, ws, pads, lay.act_gain * gain, clamp, y, tuple(x.shape[2:]))


def _conv_grad(dy, rec):
    lay, ws, pads, gain, clamp, y, x_size = rec
    dz = networks._plain_conv_act_grad(dy, y, lay.activation, gain, clamp)
    return networks._plain_conv_input_grad(dz, ws, _form(lay), lay.resample_filter, pads, x_size, arith)


def _fc_params(lay):
    w = networks._scaled_weight(lay.weight, lay.weight_gain)
    b = lay.bias
    if b is not None and lay.bias_gain != 1:
        b = networks._scaled_weight(b, lay.bias_gain)
    return w, (b.detach() if b is not None else None)


def _plugins():
    from torch_utils import hip_plugin
    return hip_plugin.AdvLossPlugin, hip_plugin.IdLossPlugin


def _fused_forward(D, img, cmap, sign):
    """-> (loss, logits [n, 1], saved)."""
    A, L = _plugins()
    n = img.shape[0]
    x, blocks = img, []
    for res in D.block_resolutions:
        blk = getattr(D, f'b{res}')
        rgb = None
        if blk.in_channels == 0:
            x, rgb = _conv(blk.fromrgb, x)
        ys, r_skip = _conv(blk.skip, x, gain=np.sqrt(0.5))
        x0, r0 = _conv(blk.conv0, x)
        x1, r1 = _conv(blk.conv1, x0, gain=np.sqrt(0.5))
        x = L.residual_join(ys, x1, 1.0)
        blocks.append((rgb, r_skip, r0, r1))
    ep = D.b4
    top = x
    if ep.mbstd is not None:
        x = A.minibatch_std(top, ep.mbstd.group_size, ep.mbstd.num_channels)
    xc, rc = _conv(ep.conv, x)
    w_fc, b_fc = _fc_params(ep.fc)
    h = bias_act.bias_act(L.linear(xc.reshape(n, -1), w_fc), b_fc, act=ep.fc.activation)
    w_out, b_out = _fc_params(ep.out)
    o = L.linear(h, w_out, b_out)
    logits, loss = A.head(o, cmap, sign)
    return loss, logits, dict(blocks=blocks, top=top, rc=rc, conv_shape=tuple(xc.shape), h=h, o=o, cmap=cmap, logits=logits, sign=sign)


def _fused_backward(D, sv, dloss):
    """-> d loss / d image.  dloss: one element on the device."""
    A, L = _plugins()
    ep = D.b4
    n = sv['o'].shape[0]
    do = A.head_backward(sv['o'], sv['cmap'], sv['logits'], dloss, sv['sign'])
    dh = L.linear_backward_input(do, _fc_params(ep.out)[0])
    spec = bias_act.activation_funcs[ep.fc.activation]
    h4 = sv['h'].reshape(n, -1, 1, 1)
    dpre = networks._modconv_grad_plugin.act_backward(dh.reshape(h4.shape), h4, spec.cuda_idx, spec.def_alpha, spec.def_gain, -1.0)[0]
    dxc = L.linear_backward_input(dpre.reshape(n, -1), _fc_params(ep.fc)[0]).reshape(sv['conv_shape'])
    dx = _conv_grad(dxc, sv['rc'])
    if ep.mbstd is not None:
        dx = A.minibatch_std_backward(sv['top'], dx.contiguous(), ep.mbstd.group_size, ep.mbstd.num_channels)
    for rgb, r_skip, r0, r1 in reversed(sv['blocks']):
        # out = skip(x) + conv1(conv0(x)): both branches receive dx, their input gradients meet at x
        dx = L.residual_join(_conv_grad(_conv_grad(dx, r1), r0).contiguous(), _conv_grad(dx, r_skip).contiguous(), 1.0)
        if rgb is not None:
            dx = _conv_grad(dx, rgb)
    return dx


class _FusedAdvLoss(torch.autograd.Function):
    """softplus(sign * D(img)).mean() and the image gradient back through a frozen discriminator on the HIP entry points -> (loss,
    logits); only the loss is differentiable, only with respect to the image; the backward is differentiable once.  The activations it keeps
    are the pass's own outputs, so they live on the context rather than in `save_for_backward`."""

    @staticmethod
    def forward(ctx, img, D, cmap, sign):
        loss, logits, ctx.sv = _fused_forward(D, img, cmap, sign)
        ctx.D = D
        ctx.mark_non_differentiable(logits)
        return loss, logits

    @staticmethod
    @once_differentiable
    def backward(ctx, dloss, _dlogits):
        return _fused_backward(ctx.D, ctx.sv, dloss.to(torch.float32).reshape(1).contiguous()), None, None, None


def _layers(D):
    for res in D.block_resolutions:
        blk = getattr(D, f'b{res}')
        yield from ((blk.fromrgb,) if blk.in_channels == 0 else ()) + (blk.skip, blk.conv0, blk.conv1)
    yield D.b4.conv


def _on_hip(D, img, cmap):
    if not (fused and isinstance(img, torch.Tensor) and img.is_cuda and img.dtype == torch.float32 and img.ndim == 4 and img.is_contiguous()
            and type(D) is Discriminator and D.b4.architecture == 'resnet' and 1 <= img.shape[0] <= MAX_BATCH
            and tuple(img.shape[1:]) == (D.img_channels, D.img_resolution, D.img_resolution) and D.img_resolution >= 8):
        return False
    if any(p.requires_grad or p.dtype != torch.float32 or p.device != img.device for p in D.parameters()):
        return False
    if any(b.device != img.device or (b.is_floating_point() and b.dtype != torch.float32) for b in D.buffers()):
        return False
    if any(getattr(D, f'b{res}').architecture != 'resnet' for res in D.block_resolutions) or any(_form(lay) is None for lay in _layers(D)):
        return False
    ep = D.b4
    if ep.fc.activation != 'lrelu' or ep.out.activation != 'linear' or ep.in_channels % 4 != 0:
        return False
    if (cmap is None) != (ep.cmap_dim == 0):
        return False
    if cmap is not None and not (cmap.is_cuda and cmap.device == img.device and cmap.dtype == torch.float32 and not cmap.requires_grad
                                 and tuple(cmap.shape) == (img.shape[0], ep.cmap_dim) and ep.cmap_dim <= 8192):
        return False
    if ep.cmap_dim == 0 and ep.final_channels != 1:
        return False
    return networks.use_hip_modconv and networks._modconv_init() and networks._modconv_grad_init()


class ADVLoss(torch.nn.Module):
    """The adversarial loss through the discriminator `D` (a `training.discriminator.Discriminator`, left as it is given: freeze it -
    `D.eval().requires_grad_(False)` - for the HIP path).  D is evaluated in fp32 (see the module); `force_fp32=False` keeps the blocks'
    own dtypes and the PyTorch definition.  `last_path`: 'hip' or 'torch', the path of the last evaluation."""

    def __init__(self, D, force_fp32=True):
        super().__init__()
        self.D = D
        self.force_fp32 = bool(force_fp32)
        self.last_path = None

    def cmap(self, c):
        """The mapped label [n, cmap_dim] (None for an unconditional D): independent of the image, so a caller with a fixed `c` caches it."""
        return self.D.mapping(None, c) if self.D.c_dim > 0 else None

    def _check_batch(self, img):
        """The minibatch-std layer's rule, before any launch on either path."""
        mb = self.D.b4.mbstd
        if mb is not None and isinstance(img, torch.Tensor) and img.ndim == 4 and img.shape[0] % mb.group(img.shape[0]) != 0:
            raise ValueError(f'ADVLoss: the batch ({img.shape[0]}) is not a multiple of the minibatch-std group size ({mb.group(img.shape[0])})')

    def _definition(self, img, c, cmap):
        self.last_path = 'torch'
        return self.D(img, c, cmap=cmap, force_fp32=True) if self.force_fp32 else self.D(img, c, cmap=cmap)

    def _loss(self, img, c, cmap, sign):
        """-> softplus(sign * D(img, c)).mean()."""
        self._check_batch(img)
        if cmap is None:
            cmap = self.cmap(c)
        if self.force_fp32 and _on_hip(self.D, img, cmap):
            self.last_path = 'hip'
            return _FusedAdvLoss.apply(img, self.D, None if cmap is None else cmap.contiguous(), sign)[0]
        return F.softplus(sign * self._definition(img, c, cmap)).mean()

    def logits(self, img, c=None, cmap=None):
        """D(img, c) [n, 1]; differentiable (twice) on the PyTorch path, which an image that requires grad always takes."""
        self._check_batch(img)
        if cmap is None:
            cmap = self.cmap(c)
        if self.force_fp32 and not (torch.is_grad_enabled() and img.requires_grad) and _on_hip(self.D, img, cmap):
            self.last_path = 'hip'
            with torch.no_grad():
                return _fused_forward(self.D, img, None if cmap is None else cmap.contiguous(), -1)[1]
        return self._definition(img, c, cmap)

    def generator_loss(self, img, c=None, cmap=None):
        """softplus(-D(img, c)).mean(): `g_nonsaturating_loss` of the logits."""
        return self._loss(img, c, cmap, -1)

    def discriminator_loss(self, real, fake, c_real=None, c_fake=None, cmap_real=None, cmap_fake=None):
        """softplus(-D(real, c_real)).mean() + softplus(D(fake, c_fake)).mean(): `d_logistic_loss` of the two logits."""
        return self._loss(real, c_real, cmap_real, -1) + self._loss(fake, c_fake, cmap_fake, +1)

    def forward(self, img, c=None, cmap=None):
        return self.generator_loss(img, c, cmap)


def adv_distance(c, advloss, weight=1.0, base=None):
    """The `distance` of `projection.project` that pulls the rendered image towards what the discriminator takes for real under the label
    `c` ([1, c_dim] or [n, c_dim]; None for an unconditional D): images (0..255) are mapped to -1..1 (`x / 127.5 - 1`) and the closure
    returns `weight * advloss.generator_loss(x, cmap=cmap(c))` (+ `base(images)` when given); the label is mapped once."""
    with torch.no_grad():
        cm = advloss.cmap(c) if c is not None else None

    def distance(images):
        m = None if cm is None else cm.to(images.device).expand(images.shape[0], -1).contiguous()
        d = weight * advloss.generator_loss(images / 127.5 - 1, cmap=m)
        return d + base(images) if base is not None else d
    return distance
