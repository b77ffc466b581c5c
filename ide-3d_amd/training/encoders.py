"""Image / segmentation -> latent encoders of the interactive editing loop (reference inversion/networks.py:1507-1665,
used by apps/train_hybrid_encoder.py:208 and Painter/run_UI.py:193-199): the inverse half of "edit -> re-render".

`HybridEncoder(img, seg) -> ws [B, n_latents_geo + n_latents_app, w_dim]`: two identical residual conv towers (one on
the RGB image, one on the 19-channel segmentation), each halving the resolution down to 4x4 and projecting with a 4x4
convolution.  Every convolution is a `Conv2dLayer` (training/networks.py), so on the GPU the stride-1 convolutions run on
the MFMA kernel of csrc/modconv.hip, the low-pass filter of the down-sampling layers on csrc/upfirdn2d.hip and the
bias / activation on csrc/bias_act.hip; module and parameter names equal the reference's, state dicts interchange.
"""

import math

import torch
from torch.autograd.function import once_differentiable

from torch_utils import custom_ops
from torch_utils import persistence
from training import networks
from training.networks import Conv2dLayer


def tower_channels(resolution: int) -> int:
    """Feature width at a given resolution (reference table, inversion/networks.py:1564-1574)."""
    return {4: 512, 8: 512, 16: 512, 32: 512, 64: 256, 128: 128, 256: 64, 512: 32, 1024: 16}[resolution]


@persistence.persistent_class
class EncoderResBlock(torch.nn.Module):
    """3x3 conv, 3x3 down-2 conv and a 1x1 down-2 skip, summed and scaled by 1/sqrt(2) (reference :1507-1521)."""

    def __init__(self, in_channel, out_channel, blur_kernel=(1, 3, 3, 1)):
        super().__init__()
        self.conv1 = Conv2dLayer(in_channel, in_channel, 3, activation='lrelu')
        self.conv2 = Conv2dLayer(in_channel, out_channel, 3, down=2, activation='lrelu')
        self.skip = Conv2dLayer(in_channel, out_channel, 1, down=2, activation='linear', bias=False)

    def forward(self, x):
        y, s = self.conv2(self.conv1(x)), self.skip(x)
        if (networks.hip_plain_conv_grad and networks.use_hip_modconv and torch.is_grad_enabled() and (y.requires_grad or s.requires_grad) and y.shape == s.shape
                and 0 < y.numel() < 2 ** 40 and all(t.is_cuda and t.dtype == torch.float32 for t in (y, s)) and y.device == s.device):
            return _ResidualJoin.apply(y, s, 1 / math.sqrt(2))
        return (y + s) * (1 / math.sqrt(2))


class _ResidualJoin(torch.autograd.Function):
    """(a + b) * gain as one launch (ide3d_residual_join), bit-equal to the two element-wise operators; both branches
    receive dy * gain, one launch and one tensor."""

    @staticmethod
    def forward(ctx, a, b, gain):
        ctx.gain = gain
        return _id_plugin().residual_join(a.contiguous(), b.contiguous(), gain)

    @staticmethod
    @once_differentiable
    def backward(ctx, dy):
        d = _id_plugin().residual_join(dy.contiguous(), None, ctx.gain) if any(ctx.needs_input_grad[:2]) else None
        return (d if ctx.needs_input_grad[0] else None), (d if ctx.needs_input_grad[1] else None), None


def _id_plugin():
    return custom_ops.get_plugin(module_name='id_loss_plugin', sources=['id_loss.hip', 'linear_wgrad.hip', 'res_join.hip'])


class _ProjectorGrad(torch.autograd.Function):
    """An `EqualConv2d` whose kernel covers its whole input, as the linear layer it is: y = x2 ws^T with
    x2 = x.reshape(n, -1) and ws = (weight * scale).reshape(M, -1) (ide3d_linear); dx2 = dy ws (ide3d_linear_backward_input),
    d weight = scale * dy^T x2 (ide3d_linear_weight_grad)."""

    @staticmethod
    def forward(ctx, x, weight, scale):
        P = _id_plugin()
        x2 = x.reshape(x.shape[0], -1).contiguous()
        ws = networks._scaled_weight(weight, scale).reshape(weight.shape[0], -1)
        y = P.linear(x2, ws)
        ctx.save_for_backward(x2)
        ctx.ws, ctx.scale, ctx.x_shape, ctx.w_shape = ws, scale, tuple(x.shape), tuple(weight.shape)
        return y.reshape(x.shape[0], weight.shape[0], 1, 1)

    @staticmethod
    @once_differentiable
    def backward(ctx, dy):
        P = _id_plugin()
        x2, = ctx.saved_tensors
        dy2 = dy.reshape(x2.shape[0], -1).contiguous()
        dx = P.linear_backward_input(dy2, ctx.ws).reshape(ctx.x_shape) if ctx.needs_input_grad[0] else None
        dw = (P.linear_weight_grad(dy2, x2) * ctx.scale).reshape(ctx.w_shape) if ctx.needs_input_grad[1] else None
        return dx, dw, None


def _linear_covers(n, K, M):
    """The limits of ide3d_linear, ide3d_linear_backward_input and ide3d_linear_weight_grad (csrc/id_loss.hip `id_linear_ok`, csrc/linear_wgrad.hip
    `linear_wgrad_ok`), restated so that a projector outside them keeps F.conv2d instead of raising."""
    return 1 <= n <= 8 and K >= 4 and K % 4 == 0 and K <= 2 ** 24 and 1 <= M <= 65535 * 8 and K * M < 2 ** 40


@persistence.persistent_class
class EqualConv2d(torch.nn.Module):
    """Plain conv with equalised learning rate: weight * 1/sqrt(fan_in) at run time (reference :1524-1556)."""

    def __init__(self, in_channel, out_channel, kernel_size, stride=1, padding=0, bias=True):
        super().__init__()
        self.weight = torch.nn.Parameter(torch.randn(out_channel, in_channel, kernel_size, kernel_size))
        self.scale = 1 / math.sqrt(in_channel * kernel_size ** 2)
        self.stride, self.padding = stride, padding
        self.bias = torch.nn.Parameter(torch.zeros(out_channel)) if bias else None

    def forward(self, x):
        k = self.weight.shape[-1]
        if (networks.hip_plain_conv_grad and networks.use_hip_modconv and torch.is_grad_enabled() and (x.requires_grad or self.weight.requires_grad)
                and self.bias is None and self.padding == 0 and self.stride == 1 and x.ndim == 4 and tuple(x.shape[2:]) == (k, k)
                and x.shape[1] == self.weight.shape[1] and _linear_covers(x.shape[0], x.shape[1] * k * k, self.weight.shape[0])
                and x.is_cuda and x.dtype == torch.float32 and self.weight.is_cuda and self.weight.dtype == torch.float32
                and x.device == self.weight.device):
            return _ProjectorGrad.apply(x, self.weight, self.scale)
        return torch.nn.functional.conv2d(x, self.weight * self.scale, bias=self.bias, stride=self.stride, padding=self.padding)

    def extra_repr(self):
        o, i, k, _ = self.weight.shape
        return f'{i}, {o}, {k}, stride={self.stride}, padding={self.padding}'


def _tower(input_dim: int, size: int):
    """1x1 stem at `size`, then residual blocks down to 4x4 -> (Sequential, channels at 4x4)."""
    layers = [Conv2dLayer(input_dim, tower_channels(size), 1)]
    ch = tower_channels(size)
    res = size
    while res > 4:
        res //= 2
        layers.append(EncoderResBlock(ch, tower_channels(res)))
        ch = tower_channels(res)
    return torch.nn.Sequential(*layers), ch


@persistence.persistent_class
class Encoder(torch.nn.Module):
    """Single-tower encoder (reference :1559-1601)."""

    def __init__(self, size, n_latents, w_dim=512, add_dim=0, input_dim=3, **unused):
        super().__init__()
        self.w_dim, self.add_dim, self.n_latents = w_dim, add_dim, n_latents
        self.convs, ch = _tower(input_dim, size)
        self.projector = EqualConv2d(ch, n_latents * w_dim + add_dim, 4, padding=0, bias=False)

    def forward(self, x):
        out = self.projector(self.convs(x))
        if self.add_dim == 0:
            return out.view(len(x), self.n_latents, self.w_dim)
        # like the reference, the extra head is read from the last two channels whatever add_dim says
        return out[:, :-2].view(len(x), self.n_latents, self.w_dim), out[:, -2:].view(len(x), self.add_dim)


@persistence.persistent_class
class HybridEncoder(torch.nn.Module):
    """Appearance tower on the image + geometry tower on the segmentation (reference :1604-1665); output rows are
    [geometry latents | appearance latents]."""

    def __init__(self, size, n_latents_app, n_latents_geo, w_dim=512, add_dim=0, input_img_dim=3, input_seg_dim=19, **unused):
        super().__init__()
        self.w_dim, self.add_dim = w_dim, add_dim
        self.n_latents_app, self.n_latents_geo = n_latents_app, n_latents_geo
        self.convs_img, ch = _tower(input_img_dim, size)
        self.projector_img = EqualConv2d(ch, n_latents_app * w_dim + add_dim, 4, padding=0, bias=False)
        self.convs_seg, ch = _tower(input_seg_dim, size)
        self.projector_seg = EqualConv2d(ch, n_latents_geo * w_dim, 4, padding=0, bias=False)

    def forward(self, img, seg):
        b = img.size(0)
        out_img = self.projector_img(self.convs_img(img))
        out_seg = self.projector_seg(self.convs_seg(seg)).view(b, self.n_latents_geo, self.w_dim)
        if self.add_dim == 0:
            return torch.cat([out_seg, out_img.view(b, self.n_latents_app, self.w_dim)], 1)
        ws_img, extra = out_img[:, :-2], out_img[:, -2:]
        return torch.cat([out_seg, ws_img.view(b, self.n_latents_app, self.w_dim)], 1), extra.view(b, self.add_dim)
