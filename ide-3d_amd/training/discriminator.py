"""The StyleGAN2 discriminator (reference inversion/networks.py:1271-1502), which the hybrid encoder's training step loads as `network['D']`
beside `G_ema` (apps/train_hybrid_encoder.py:198, 211) for its adversarial term.

`DiscriminatorBlock`, `MinibatchStdLayer`, `DiscriminatorEpilogue` and `Discriminator` are written from that definition with the reference's
constructor arguments, attribute names and parameter / buffer names, so `D.state_dict()` of a reference discriminator loads with
`strict=True`; they are built from this package's `Conv2dLayer`, `FullyConnectedLayer` and `MappingNetwork` and are reachable as
`training.networks.<name>` too (the path pickles and `dnnlib.util.construct_class_by_name` use).

A residual block at resolution R maps [n, C, R, R] (the first block: the image through `fromrgb`) to [n, C', R / 2, R / 2]:
    resnet:  sqrt(1/2) * (skip(x) + conv1(conv0(x)))      skip: FIR + decimation + 1x1, linear, no bias; conv1: FIR + 3x3 of stride 2
    orig:    conv1(conv0(x));   skip: the same, with `fromrgb` of the (FIR-decimated) image added to x in every block
and the epilogue at 4 x 4 appends the minibatch standard deviation, runs one 3x3 convolution and two dense layers, and projects the result
on the mapped label: logit = out . cmap / sqrt(cmap_dim) (no label: `out` has one feature, the logit).

Everything here is differentiable twice through ATen whenever a gradient is recorded (R1's `create_graph=True` goes through
`Discriminator.forward`); the frozen layers run this package's HIP inference launches under `no_grad`, `MinibatchStdLayer` included.  The HIP
forward and image gradient of the adversarial loss through a frozen discriminator is `training.adv_loss`.
"""

import numpy as np
import torch

from torch_utils import misc
from torch_utils import persistence
from torch_utils.ops import upfirdn2d
from training.networks import Conv2dLayer, FullyConnectedLayer, MappingNetwork

ARCHITECTURES = ('orig', 'skip', 'resnet')


@persistence.persistent_class
class DiscriminatorBlock(torch.nn.Module):
    """One resolution of the discriminator (reference networks.py:1271-1355).  `in_channels = 0` marks the first block, which reads the
    image; `freeze_layers` (Freeze-D) registers the first layers of the network as buffers: layer `first_layer_idx + i` of this block, in
    the order fromrgb, conv0, conv1, skip, trains when its index is at least `freeze_layers`."""

    def __init__(self, in_channels, tmp_channels, out_channels, resolution, img_channels, first_layer_idx, architecture='resnet',
                 activation='lrelu', resample_filter=[1, 3, 3, 1], conv_clamp=None, use_fp16=False, fp16_channels_last=False, freeze_layers=0):
        assert in_channels in [0, tmp_channels]
        assert architecture in ARCHITECTURES
        super().__init__()
        self.in_channels = in_channels
        self.resolution = resolution
        self.img_channels = img_channels
        self.first_layer_idx = first_layer_idx
        self.architecture = architecture
        self.use_fp16 = use_fp16
        self.channels_last = use_fp16 and fp16_channels_last
        self.register_buffer('resample_filter', upfirdn2d.setup_filter(resample_filter))
        self.num_layers = 0

        def layer(cin, cout, k, **kwargs):
            trainable = self.first_layer_idx + self.num_layers >= freeze_layers
            self.num_layers += 1
            return Conv2dLayer(cin, cout, kernel_size=k, trainable=trainable, channels_last=self.channels_last, **kwargs)

        if in_channels == 0 or architecture == 'skip':
            self.fromrgb = layer(img_channels, tmp_channels, 1, activation=activation, conv_clamp=conv_clamp)
        self.conv0 = layer(tmp_channels, tmp_channels, 3, activation=activation, conv_clamp=conv_clamp)
        self.conv1 = layer(tmp_channels, out_channels, 3, activation=activation, down=2, resample_filter=resample_filter, conv_clamp=conv_clamp)
        if architecture == 'resnet':
            self.skip = layer(tmp_channels, out_channels, 1, bias=False, down=2, resample_filter=resample_filter)

    def forward(self, x, img, force_fp32=False, downsampler=None):
        half = self.use_fp16 and not force_fp32
        dtype = torch.float16 if half else torch.float32
        memory_format = torch.channels_last if self.channels_last and not force_fp32 else torch.contiguous_format
        if x is not None:
            misc.assert_shape(x, [None, self.in_channels, self.resolution, self.resolution])
            x = x.to(dtype=dtype, memory_format=memory_format)
        if self.in_channels == 0 or self.architecture == 'skip':
            misc.assert_shape(img, [None, self.img_channels, self.resolution, self.resolution])
            img = img.to(dtype=dtype, memory_format=memory_format)
            y = self.fromrgb(img)
            x = y if x is None else x + y
            if self.architecture != 'skip':
                img = None                     # only the first block reads the image
            elif downsampler is not None:
                img = downsampler(img, 2)
            else:
                img = upfirdn2d.downsample2d(img, self.resample_filter)
        if self.architecture == 'resnet':
            y = self.skip(x, gain=np.sqrt(0.5))
            x = self.conv1(self.conv0(x), gain=np.sqrt(0.5))
            x = y + x
        else:
            x = self.conv1(self.conv0(x))
        assert x.dtype == dtype
        return x, img


@persistence.persistent_class
class MinibatchStdLayer(torch.nn.Module):
    """Appends `num_channels` planes holding the standard deviation over groups of the minibatch, averaged over a feature's channels and the
    pixels (reference networks.py:1360-1381).  Groups have G = min(group_size, n) members (None: n) and are interleaved: sample g * (n / G)
    + j is member g of group j.  A batch that is no multiple of G, or channels that are no multiple of `num_channels`, raise ValueError
    (where the reference's `reshape` raises).  Frozen fp32 CUDA inference under `no_grad` is one launch of ide3d_minibatch_std; whenever a
    gradient is recorded it is the PyTorch definition."""

    def __init__(self, group_size, num_channels=1):
        super().__init__()
        self.group_size = group_size
        self.num_channels = num_channels

    def group(self, n):
        return n if self.group_size is None else min(int(self.group_size), n)

    def forward(self, x):
        n, c, h, w = x.shape
        G, F = self.group(n), self.num_channels
        if n % G != 0:
            raise ValueError(f'MinibatchStdLayer: the batch ({n}) is not a multiple of the group size ({G})')
        if c % F != 0:
            raise ValueError(f'MinibatchStdLayer: the channels ({c}) are not a multiple of num_channels ({F})')
        if x.is_cuda and x.dtype == torch.float32 and x.is_contiguous() and not (torch.is_grad_enabled() and x.requires_grad):
            from torch_utils import hip_plugin
            return hip_plugin.AdvLossPlugin.minibatch_std(x, G, F)
        y = x.reshape(G, n // G, F, c // F, h, w)
        y = y - y.mean(dim=0)
        y = (y.square().mean(dim=0) + 1e-8).sqrt()                  # [n / G, F, c / F, h, w]
        y = y.mean(dim=[2, 3, 4]).reshape(n // G, F, 1, 1)
        return torch.cat([x, y.repeat(G, 1, h, w)], dim=1)


@persistence.persistent_class
class DiscriminatorEpilogue(torch.nn.Module):
    """The 4 x 4 end of the discriminator (reference networks.py:1386-1441), always fp32: (`fromrgb` of the image added, 'skip' only,)
    `mbstd`, `conv`, `fc`, `out`, and with a label the projection on `cmap` [n, cmap_dim]."""

    def __init__(self, in_channels, cmap_dim, resolution, img_channels, architecture='resnet', mbstd_group_size=4, mbstd_num_channels=1,
                 activation='lrelu', conv_clamp=None, final_channels=1):
        assert architecture in ARCHITECTURES
        super().__init__()
        self.in_channels = in_channels
        self.final_channels = final_channels
        self.cmap_dim = cmap_dim
        self.resolution = resolution
        self.img_channels = img_channels
        self.architecture = architecture
        if architecture == 'skip':
            self.fromrgb = Conv2dLayer(img_channels, in_channels, kernel_size=1, activation=activation)
        self.mbstd = MinibatchStdLayer(group_size=mbstd_group_size, num_channels=mbstd_num_channels) if mbstd_num_channels > 0 else None
        self.conv = Conv2dLayer(in_channels + mbstd_num_channels, in_channels, kernel_size=3, activation=activation, conv_clamp=conv_clamp)
        self.fc = FullyConnectedLayer(in_channels * (resolution ** 2), in_channels, activation=activation)
        self.out = FullyConnectedLayer(in_channels, final_channels if cmap_dim == 0 else cmap_dim)

    def forward(self, x, img, cmap, force_fp32=False):
        misc.assert_shape(x, [None, self.in_channels, self.resolution, self.resolution])
        x = x.to(dtype=torch.float32, memory_format=torch.contiguous_format)
        if self.architecture == 'skip':
            misc.assert_shape(img, [None, self.img_channels, self.resolution, self.resolution])
            x = x + self.fromrgb(img.to(dtype=torch.float32, memory_format=torch.contiguous_format))
        if self.mbstd is not None:
            x = self.mbstd(x)
        x = self.out(self.fc(self.conv(x).flatten(1)))
        if self.cmap_dim > 0:
            misc.assert_shape(cmap, [None, self.cmap_dim])
            x = (x * cmap).sum(dim=1, keepdim=True) * (1 / np.sqrt(self.cmap_dim))
        assert x.dtype == torch.float32
        return x


@persistence.persistent_class
class Discriminator(torch.nn.Module):
    """The StyleGAN2 discriminator (reference networks.py:1446-1502): blocks `b<res>` from `img_resolution` down to 8, `mapping` (label ->
    cmap, only with `c_dim > 0`) and the epilogue `b4`.  A block at resolution `res` has min(channel_base // res, channel_max) channels;
    the `num_fp16_res` highest resolutions run in fp16 unless `force_fp32=True` is passed to `forward`.  -> logits [n, 1]."""

    def __init__(self, c_dim, img_resolution, img_channels, architecture='resnet', channel_base=32768, channel_max=512, num_fp16_res=0,
                 conv_clamp=None, cmap_dim=None, block_kwargs={}, mapping_kwargs={}, epilogue_kwargs={}):
        super().__init__()
        self.c_dim = c_dim
        self.img_resolution = img_resolution
        self.img_resolution_log2 = int(np.log2(img_resolution))
        self.img_channels = img_channels
        self.block_resolutions = [2 ** i for i in range(self.img_resolution_log2, 2, -1)]
        channels = {res: min(channel_base // res, channel_max) for res in self.block_resolutions + [4]}
        fp16_resolution = max(2 ** (self.img_resolution_log2 + 1 - num_fp16_res), 8)
        if cmap_dim is None:
            cmap_dim = channels[4]
        if c_dim == 0:
            cmap_dim = 0
        common = dict(img_channels=img_channels, architecture=architecture, conv_clamp=conv_clamp)
        layer_idx = 0
        for res in self.block_resolutions:
            block = DiscriminatorBlock(channels[res] if res < img_resolution else 0, channels[res], channels[res // 2], resolution=res,
                                       first_layer_idx=layer_idx, use_fp16=(res >= fp16_resolution), **block_kwargs, **common)
            setattr(self, f'b{res}', block)
            layer_idx += block.num_layers
        if c_dim > 0:
            self.mapping = MappingNetwork(z_dim=0, c_dim=c_dim, w_dim=cmap_dim, num_ws=None, w_avg_beta=None, **mapping_kwargs)
        self.b4 = DiscriminatorEpilogue(channels[4], cmap_dim=cmap_dim, resolution=4, **epilogue_kwargs, **common)

    def features(self, img, **block_kwargs):
        """-> (x [n, C, 4, 4], img or None): the blocks in front of the epilogue."""
        if isinstance(img, dict):
            img = img['img']
        x = None
        for res in self.block_resolutions:
            x, img = getattr(self, f'b{res}')(x, img, **block_kwargs)
        return x, img

    def forward(self, img, c, cmap=None, **block_kwargs):
        """`cmap`: the mapped label `self.mapping(None, c)` when the caller has it already (it does not depend on the image)."""
        x, img = self.features(img, **block_kwargs)
        if self.c_dim > 0 and cmap is None:
            cmap = self.mapping(None, c)
        return self.b4(x, img, cmap)
