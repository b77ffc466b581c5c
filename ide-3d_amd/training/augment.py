"""The augmentation pipeline of adaptive discriminator augmentation (Karras et al., "Training Generative Adversarial Networks with
Limited Data"), with the geometric and colour stages in HIP (csrc/augment.hip).

Surface of the reference module (training/augment.py): `wavelets`, `matrix`, the `translate / scale / rotate` helpers with their `_inv`
forms and `AugmentPipe` with the reference's constructor arguments, defaults and buffers (`p`, `Hz_geom`, `Hz_fbank`), so a state dict
interchanges.  `forward(images, debug_percentile=None)` has the reference's meaning stage by stage: pixel blitting, general geometry,
colour, image-space filter, noise, cutout.

What the reference can only express by re-running `forward`:

    params = pipe.sample_params(N, C, H, W, device)      every draw and matrix product as batch-sized ops on `device`, no host read
    out    = pipe.apply(images, params, noise=None)       the stages on given parameters; forward == apply(images, sample_params(...))
    geometric_transform(images, G_inv, Hz_geom=None)      the geometric stage alone, any channel count
    color_transform(images, C)                            the colour stage alone, 3 channels or 1

so an image and its 19-channel mask receive the same warp:

    params = pipe.sample_params(*img.shape, img.device); img = pipe.apply(img, params)
    mask = augment.geometric_transform(mask, params.G_inv, pipe.Hz_geom)

Two definitions live here.  The PyTorch definition is built from this package's upfirdn2d, grid_sample_gradfix and conv2d_gradfix like
the reference's; it pads with Python ints, so it reads the margins back and synchronises.  It serves CPU tensors, dtypes other than
float32, a `G_inv` or `C` that requires grad, `fused = False`, and always the image-filter, noise and cutout stages.  The HIP path serves
float32 CUDA images (made contiguous if they are not) for the geometric and colour stages, forward and backward with respect to the
images, under one pair of autograd Functions (the map and its transpose, each the other's backward, so a gradient taken with
`create_graph=True` differentiates again): the margins stay on the device as four int32, the matrix chain of reference lines 292-301 is folded
in float64 on the device into one map from output-grid pixels to up-sampled pixels, and one launch does the rest.  Its backward
accumulates with float atomic adds: two backward runs agree to rounding, not bit for bit.
"""

import dataclasses
from typing import Optional

import numpy as np
import torch

from torch_utils import persistence
from torch_utils.ops import upfirdn2d
from torch_utils.ops import grid_sample_gradfix
from torch_utils.ops import conv2d_gradfix

# True: what the HIP path takes (see above) runs on it.  False: always the PyTorch definition.
fused = True

MAX_SIDE = 16384

#----------------------------------------------------------------------------
# Low-pass decomposition filters of the two wavelets the pipeline uses (the same numbers as PyWavelets' `dec_lo`).

wavelets = {
    'sym2': [-0.12940952255092145, 0.22414386804185735, 0.836516303737469, 0.48296291314469025],
    'sym6': [0.015404109327027373, 0.0034907120842174702, -0.11799011114819057, -0.048311742585633, 0.4910559419267466, 0.787641141030194,
             0.3379294217276218, -0.07263752278646252, -0.021060292512300564, 0.04472490177066578, 0.0017677118642428036, -0.007800708325034148],
}

#----------------------------------------------------------------------------
# Homogeneous matrices from scalars and batch tensors.


_consts = {}


def _device_key(device):
    """'cuda' and 'cuda:0' name one device: one cache entry."""
    d = torch.device('cpu' if device is None else device)
    return (d.type, d.index if d.index is not None or d.type != 'cuda' else torch.cuda.current_device())


def _const(value, shape=None, dtype=torch.float32, device=None):
    """A constant tensor, made once per (value, dtype, device), kept for the life of the process (a few dozen tensors of at most 16
    elements) and never written.  The FIRST use on a device copies from the host; later uses copy nothing, so the matrix code can run
    inside a stream capture after one eager call."""
    arr = np.asarray(value, dtype=np.float64)
    key = (arr.tobytes(), arr.shape, dtype, _device_key(device))
    t = _consts.get(key)
    if t is None:
        t = _consts[key] = torch.as_tensor(arr, dtype=dtype, device=device)
    return t if shape is None else t.expand(shape)


def matrix(*rows, device=None):
    """A matrix from rows of entries.  Entries are Python scalars or tensors of one common shape B; the result is B + (rows, columns),
    on the tensors' device and in their dtype, or a plain float32 constant on `device` when every entry is a scalar."""
    width = len(rows[0])
    if any(len(row) != width for row in rows):
        raise ValueError('matrix: rows of unequal length')
    batch = next((v for row in rows for v in row if isinstance(v, torch.Tensor)), None)
    if batch is None:
        return _const(rows, device=device)
    if device is not None and torch.device(device) != batch.device:
        raise ValueError(f'matrix: device {device} given, but the entries live on {batch.device}')
    lift = lambda v: v if isinstance(v, torch.Tensor) else _const(v, batch.shape, batch.dtype, batch.device)
    return torch.stack([torch.stack([lift(v) for v in row], dim=-1) for row in rows], dim=-2)


def translate2d(tx, ty, **kwargs):
    return matrix([1, 0, tx], [0, 1, ty], [0, 0, 1], **kwargs)


def translate3d(tx, ty, tz, **kwargs):
    return matrix([1, 0, 0, tx], [0, 1, 0, ty], [0, 0, 1, tz], [0, 0, 0, 1], **kwargs)


def scale2d(sx, sy, **kwargs):
    return matrix([sx, 0, 0], [0, sy, 0], [0, 0, 1], **kwargs)


def scale3d(sx, sy, sz, **kwargs):
    return matrix([sx, 0, 0, 0], [0, sy, 0, 0], [0, 0, sz, 0], [0, 0, 0, 1], **kwargs)


def rotate2d(theta, **kwargs):
    return matrix([torch.cos(theta), torch.sin(-theta), 0], [torch.sin(theta), torch.cos(theta), 0], [0, 0, 1], **kwargs)


def rotate3d(v, theta, **kwargs):
    """Rotation by `theta` about the unit axis `v` (Rodrigues)."""
    x, y, z = v[..., 0], v[..., 1], v[..., 2]
    s, c = torch.sin(theta), torch.cos(theta)
    k = 1 - c
    return matrix([x * x * k + c, x * y * k - z * s, x * z * k + y * s, 0],
                  [y * x * k + z * s, y * y * k + c, y * z * k - x * s, 0],
                  [z * x * k - y * s, z * y * k + x * s, z * z * k + c, 0],
                  [0, 0, 0, 1], **kwargs)


def translate2d_inv(tx, ty, **kwargs):
    return translate2d(-tx, -ty, **kwargs)


def translate3d_inv(tx, ty, tz, **kwargs):
    return translate3d(-tx, -ty, -tz, **kwargs)


def scale2d_inv(sx, sy, **kwargs):
    return scale2d(1 / sx, 1 / sy, **kwargs)


def scale3d_inv(sx, sy, sz, **kwargs):
    return scale3d(1 / sx, 1 / sy, 1 / sz, **kwargs)


def rotate2d_inv(theta, **kwargs):
    return rotate2d(-theta, **kwargs)


def rotate3d_inv(v, theta, **kwargs):
    return rotate3d(v, -theta, **kwargs)

#----------------------------------------------------------------------------
# The geometric stage.

_default_taps = {}


def _geom_taps(Hz_geom, device):
    if Hz_geom is None:
        key = _device_key(device)
        if key not in _default_taps:
            _default_taps[key] = upfirdn2d.setup_filter(wavelets['sym6'], device=device)
        Hz_geom = _default_taps[key]
    if not (isinstance(Hz_geom, torch.Tensor) and Hz_geom.ndim == 1 and Hz_geom.numel() == 12):
        raise ValueError('the geometric filter must be a 1-D tensor of 12 taps')
    return Hz_geom


def _check_images(images, what):
    if not (isinstance(images, torch.Tensor) and images.ndim == 4):
        raise ValueError(f'{what}: images must be a [N, C, H, W] tensor')
    if not images.dtype.is_floating_point:
        raise ValueError(f'{what}: images must have a floating-point dtype (got {images.dtype})')
    n, c, h, w = images.shape
    if min(n, c, h, w) < 1:
        raise ValueError(f'{what}: empty axis in {list(images.shape)}')
    return n, c, h, w


def _check_geometric(images, G_inv):
    n, c, h, w = _check_images(images, 'geometric_transform')
    if h < 2 or w < 2:
        raise ValueError(f'geometric_transform: reflect padding needs a height and a width of at least 2 (got {h} x {w})')
    if h > MAX_SIDE or w > MAX_SIDE:
        raise ValueError(f'geometric_transform: a side above {MAX_SIDE} (got {h} x {w})')
    if not (isinstance(G_inv, torch.Tensor) and tuple(G_inv.shape) == (n, 3, 3) and G_inv.dtype.is_floating_point):
        raise ValueError(f'geometric_transform: G_inv must be a floating-point [{n}, 3, 3] tensor')
    if G_inv.device != images.device:
        raise ValueError('geometric_transform: G_inv and the images must share a device')
    return n, c, h, w


def margins(G_inv, height, width, taps=12):
    """(mx0, my0, mx1, my1), int32 [4] on G_inv's device: how far the transformed corners of the image, plus the filter's reach, leave it;
    batch-wide, clamped to [0, side - 1] (reference lines 278-288).  No host read."""
    return _margin_values(G_inv, height, width, taps).ceil().to(torch.int32)


def _margin_values(G_inv, height, width, taps=12):
    dev, dt = G_inv.device, G_inv.dtype
    cx, cy = (width - 1) / 2, (height - 1) / 2
    corners = _const([[-cx, -cy, 1], [cx, -cy, 1], [cx, cy, 1], [-cx, cy, 1]], dtype=dt, device=dev)
    moved = G_inv @ corners.t()                                        # [N, xyz, corner]
    xy = moved[:, :2, :].permute(1, 0, 2).flatten(1)                   # [xy, N * corner]
    reach = torch.cat([-xy, xy]).max(dim=1).values                     # x0, y0, x1, y1
    pad = taps // 4 * 2
    reach = reach + _const([pad - cx, pad - cy] * 2, dtype=dt, device=dev)
    reach = reach.max(_const([0, 0] * 2, dtype=dt, device=dev))
    return reach.min(_const([width - 1, height - 1] * 2, dtype=dt, device=dev))


def sample_coords(G_inv, m, height, width, taps=12):
    """[N, 6] float32: reference lines 292-301 and the unnormalisations of affine_grid / grid_sample (align_corners=False) folded, in
    float64 on the device, into the map from pixel (j, i) of the 2 (H + 6) x 2 (W + 6) sampling grid to pixel coordinates of the
    up-sampled padded image: ix = a0 j + a1 i + a2, iy = a3 j + a4 i + a5."""
    dev = G_inv.device
    md = m.to(torch.float64)
    mx0, my0, mx1, my1 = md[0], md[1], md[2], md[3]
    pad = taps // 4 * 2
    ws, hs = 2 * (width + pad), 2 * (height + pad)
    wu, hu = 2 * (width + mx0 + mx1), 2 * (height + my0 + my1)
    k = dict(device=dev)
    half = _const(0.5, dtype=torch.float64, device=dev)
    two = _const(2.0, dtype=torch.float64, device=dev)
    G = translate2d((mx0 - mx1) / 2, (my0 - my1) / 2) @ G_inv.detach().to(torch.float64)
    G = scale2d(two, two) @ G @ scale2d(half, half)
    G = translate2d(-half, -half) @ G @ translate2d(half, half)
    G = translate2d((wu - 1) / 2, (hu - 1) / 2) @ G @ translate2d(_const(-(ws - 1) / 2, dtype=torch.float64, **k), _const(-(hs - 1) / 2, dtype=torch.float64, **k))
    return G[:, :2, :].reshape(-1, 6).to(torch.float32).contiguous()


def _geometric_torch(images, G_inv, Hz_geom):
    """The PyTorch definition (reference lines 277-306).  Reads the margins back: pads are Python ints."""
    n, c, h, w = images.shape
    dev = images.device
    pad = Hz_geom.shape[0] // 4
    mx0, my0, mx1, my1 = (int(v) for v in margins(G_inv, h, w, Hz_geom.shape[0]).tolist())
    f = Hz_geom.to(torch.float32)
    x = torch.nn.functional.pad(images, [mx0, mx1, my0, my1], mode='reflect')
    G = translate2d((mx0 - mx1) / 2, (my0 - my1) / 2, device=dev).to(G_inv.dtype) @ G_inv
    x = upfirdn2d.upsample2d(x=x, f=f, up=2)
    G = scale2d(2, 2, device=dev).to(G.dtype) @ G @ scale2d_inv(2, 2, device=dev).to(G.dtype)
    G = translate2d(-0.5, -0.5, device=dev).to(G.dtype) @ G @ translate2d_inv(-0.5, -0.5, device=dev).to(G.dtype)
    shape = [n, c, (h + pad * 2) * 2, (w + pad * 2) * 2]
    G = scale2d(2 / x.shape[3], 2 / x.shape[2], device=dev).to(G.dtype) @ G @ scale2d_inv(2 / shape[3], 2 / shape[2], device=dev).to(G.dtype)
    grid = torch.nn.functional.affine_grid(theta=G[:, :2, :].to(x.dtype), size=shape, align_corners=False)
    x = grid_sample_gradfix.grid_sample(x, grid)
    return upfirdn2d.downsample2d(x=x, f=f, down=2, padding=-pad * 2, flip_filter=True)


def _color_rows(C, num_channels):
    """[N, 4, 4] -> [N, 12]: the 3 x 4 rows for RGB; for one channel the grey form of reference lines 367-368 as row 0 = (scale, 0, 0, offset)."""
    if num_channels == 3:
        return C[:, :3, :].reshape(-1, 12)
    if num_channels == 1:
        grey = C[:, :3, :].mean(dim=1)                                 # [N, 4]
        rows = torch.zeros([C.shape[0], 12], dtype=C.dtype, device=C.device)
        rows[:, 0] = grey[:, :3].sum(dim=1)
        rows[:, 3] = grey[:, 3]
        return rows
    raise ValueError('Image must be RGB (3 channels) or L (1 channel)')


def _color_torch(images, C):
    n, c, h, w = images.shape
    rows = _color_rows(C, c).to(images.dtype)
    x = images.reshape(n, c, h * w)
    if c == 3:
        m = rows.reshape(n, 3, 4)
        x = m[:, :, :3] @ x + m[:, :, 3:]
    else:
        x = x * rows[:, 0].reshape(n, 1, 1) + rows[:, 3].reshape(n, 1, 1)
    return x.reshape(n, c, h, w)


def _check_color(images, C):
    n, c, h, w = _check_images(images, 'color_transform')
    if c not in (1, 3):
        raise ValueError('Image must be RGB (3 channels) or L (1 channel)')
    if not (isinstance(C, torch.Tensor) and tuple(C.shape) == (n, 4, 4) and C.dtype.is_floating_point and C.device == images.device):
        raise ValueError(f'color_transform: C must be a floating-point [{n}, 4, 4] tensor on the images\' device')


def _takes_hip(images, *params):
    return fused and images.is_cuda and images.dtype == torch.float32 and not any(p is not None and p.requires_grad for p in params)


def _launch(x, coords, m, taps, color, transpose):
    """One launch of the linear map (coords given: the geometric stage with the colour matrix as its epilogue; coords None: the colour
    matrix alone) or of its transpose with respect to the images."""
    from torch_utils import hip_plugin
    x = x.contiguous()
    if coords is None:
        return hip_plugin.AugmentPlugin.color(x, torch.empty_like(x), color, transpose=transpose)
    if transpose:
        return hip_plugin.AugmentPlugin.geometric_backward(x, torch.zeros_like(x), coords, m, taps, color)
    return hip_plugin.AugmentPlugin.geometric(x, torch.empty_like(x), coords, m, taps, color)


class _FusedMap(torch.autograd.Function):
    """y = L x + b: ide3d_augment_geometric (or ide3d_augment_color when there is no geometric stage).  Its backward is `_FusedMapT`, so
    a gradient taken with `create_graph=True` (the R1 penalty through the pipe) stays on the tape."""

    @staticmethod
    def forward(ctx, images, coords, m, taps, color):
        ctx.save_for_backward(coords, m, taps, color)
        return _launch(images, coords, m, taps, color, False)

    @staticmethod
    def backward(ctx, grad_out):
        return _FusedMapT.apply(grad_out, *ctx.saved_tensors), None, None, None, None


class _FusedMapT(torch.autograd.Function):
    """g -> L^T g: the transposed launch.  The map is linear, so its own backward is the forward launch without the colour offset."""

    @staticmethod
    def forward(ctx, grad_out, coords, m, taps, color):
        ctx.save_for_backward(coords, m, taps, color)
        return _launch(grad_out, coords, m, taps, color, True)

    @staticmethod
    def backward(ctx, grad_grad):
        coords, m, taps, color = ctx.saved_tensors
        linear = None if color is None else color * _const([1, 1, 1, 0] * 3, dtype=color.dtype, device=color.device)
        return _FusedMap.apply(grad_grad, coords, m, taps, linear), None, None, None, None


def _fused_rows(C, num_channels):
    return _color_rows(C.detach().to(torch.float32), num_channels).contiguous()


def _geometric_color(images, G_inv, C, Hz_geom):
    """The geometric stage, then the colour stage; either may be None."""
    if G_inv is not None:
        n, c, h, w = _check_geometric(images, G_inv)
        Hz_geom = _geom_taps(Hz_geom, images.device)
    if C is not None:
        _check_color(images, C)
    if _takes_hip(images, G_inv, C):
        c = images.shape[1]
        rows = _fused_rows(C, c) if C is not None else None
        if G_inv is None:
            return images if rows is None else _FusedMap.apply(images, None, None, None, rows)
        m = margins(G_inv.detach(), h, w, Hz_geom.shape[0])
        coords = sample_coords(G_inv, m, h, w, Hz_geom.shape[0])
        return _FusedMap.apply(images, coords, m, Hz_geom.detach().to(torch.float32).contiguous(), rows)
    if G_inv is not None:
        images = _geometric_torch(images, G_inv, Hz_geom)
    if C is not None:
        images = _color_torch(images, C)
    return images


def geometric_transform(images, G_inv, Hz_geom=None):
    """Warp `images` [N, C, H, W] (any C) by the inverse pixel-space transforms `G_inv` [N, 3, 3] as the pipeline's geometric stage does:
    reflect padding by the batch-wide margins, 2x up-sampling with `Hz_geom` (sym6 by default), bilinear resampling, 2x decimation."""
    return _geometric_color(images, G_inv, None, Hz_geom)


def color_transform(images, C):
    """`C[:, :3, :3] @ rgb + C[:, :3, 3]` per pixel for 3 channels, the grey form for 1; anything else raises a ValueError."""
    return _geometric_color(images, None, C, None)

#----------------------------------------------------------------------------


@dataclasses.dataclass
class AugmentParams:
    """What one call of the pipeline drew.  A field is None when no stage that sets it is configured."""
    G_inv: Optional[torch.Tensor] = None            # [N, 3, 3] float32: inverse pixel-space transform, before any padding adjustment
    C: Optional[torch.Tensor] = None                # [N, 4, 4] float32: homogeneous colour transform
    Hz_prime: Optional[torch.Tensor] = None         # [N, 43]: the image-space filter of every sample
    noise_sigma: Optional[torch.Tensor] = None      # [N, 1, 1, 1]
    cutout_size: Optional[torch.Tensor] = None      # [N, 2, 1, 1, 1], relative to the image
    cutout_center: Optional[torch.Tensor] = None    # [N, 2, 1, 1, 1], relative to the image


@persistence.persistent_class
class AugmentPipe(torch.nn.Module):
    """Every augmentation is off by default; a probability multiplier of 1 switches one on.  `p` scales all of them."""

    def __init__(self,
        xflip=0, rotate90=0, xint=0, xint_max=0.125,
        scale=0, rotate=0, aniso=0, xfrac=0, scale_std=0.2, rotate_max=1, aniso_std=0.2, xfrac_std=0.125,
        brightness=0, contrast=0, lumaflip=0, hue=0, saturation=0, brightness_std=0.2, contrast_std=0.5, hue_max=1, saturation_std=1,
        imgfilter=0, imgfilter_bands=[1, 1, 1, 1], imgfilter_std=1,
        noise=0, cutout=0, noise_std=0.1, cutout_size=0.5,
    ):
        super().__init__()
        self.register_buffer('p', torch.ones([]))
        # pixel blitting
        self.xflip, self.rotate90, self.xint, self.xint_max = float(xflip), float(rotate90), float(xint), float(xint_max)
        # general geometry (scales are log2 standard deviations, rotate_max = 1 is a full circle, xfrac_std is relative to the side)
        self.scale, self.rotate, self.aniso, self.xfrac = float(scale), float(rotate), float(aniso), float(xfrac)
        self.scale_std, self.rotate_max, self.aniso_std, self.xfrac_std = float(scale_std), float(rotate_max), float(aniso_std), float(xfrac_std)
        # colour
        self.brightness, self.contrast, self.lumaflip, self.hue, self.saturation = float(brightness), float(contrast), float(lumaflip), float(hue), float(saturation)
        self.brightness_std, self.contrast_std, self.hue_max, self.saturation_std = float(brightness_std), float(contrast_std), float(hue_max), float(saturation_std)
        # image-space filter
        self.imgfilter, self.imgfilter_bands, self.imgfilter_std = float(imgfilter), list(imgfilter_bands), float(imgfilter_std)
        # corruptions
        self.noise, self.cutout, self.noise_std, self.cutout_size = float(noise), float(cutout), float(noise_std), float(cutout_size)

        self.register_buffer('Hz_geom', upfirdn2d.setup_filter(wavelets['sym6']))

        # four-band filter bank from sym2: each level up-samples the bank by zero insertion, smooths every row with the half-band low-pass
        # and adds the half-band high-pass to the new band's centre
        lo = np.asarray(wavelets['sym2'])
        hi = lo * ((-1) ** np.arange(lo.size))
        lo2 = np.convolve(lo, lo[::-1]) / 2
        hi2 = np.convolve(hi, hi[::-1]) / 2
        bank = np.eye(4, 1)
        for band in range(1, 4):
            stuffed = np.zeros([4, bank.shape[1] * 2 - 1])
            stuffed[:, ::2] = bank
            bank = np.stack([np.convolve(row, lo2) for row in stuffed])
            mid = bank.shape[1] // 2
            bank[band, mid - hi2.size // 2: mid - hi2.size // 2 + hi2.size] += hi2
        self.register_buffer('Hz_fbank', torch.as_tensor(bank, dtype=torch.float32))

    # ---- parameters ----

    def sample_params(self, batch_size, num_channels, height, width, device, debug_percentile=None):
        """Draw the parameters of one call: batch-sized PyTorch ops on `device`, nothing is copied to the host."""
        N, dev = batch_size, torch.device(device)
        pct = None if debug_percentile is None else torch.as_tensor(debug_percentile, dtype=torch.float32, device=dev)
        p = self.p.to(dev)
        rand = lambda *shape: torch.rand(list(shape), device=dev)
        randn = lambda *shape: torch.randn(list(shape), device=dev)

        def gated(value, neutral, prob, *gate_shape):
            return torch.where(rand(*gate_shape) < prob, value, torch.full_like(value, neutral))

        def normal_pct():
            return torch.erfinv(pct * 2 - 1)

        out = AugmentParams()

        # ---- pixel blitting and general geometry: G_inv @ pixel_out -> pixel_in ----
        G = None
        def push(M):
            nonlocal G
            G = M if G is None else G @ M
        if self.xflip > 0:
            i = gated(torch.floor(rand(N) * 2), 0, self.xflip * p, N)
            if pct is not None:
                i = torch.full_like(i, 1) * torch.floor(pct * 2)
            push(scale2d_inv(1 - 2 * i, 1))
        if self.rotate90 > 0:
            i = gated(torch.floor(rand(N) * 4), 0, self.rotate90 * p, N)
            if pct is not None:
                i = torch.full_like(i, 1) * torch.floor(pct * 4)
            push(rotate2d_inv(-np.pi / 2 * i))
        if self.xint > 0:
            t = gated((rand(N, 2) * 2 - 1) * self.xint_max, 0, self.xint * p, N, 1)
            if pct is not None:
                t = torch.full_like(t, 1) * ((pct * 2 - 1) * self.xint_max)
            push(translate2d_inv(torch.round(t[:, 0] * width), torch.round(t[:, 1] * height)))
        if self.scale > 0:
            s = gated(torch.exp2(randn(N) * self.scale_std), 1, self.scale * p, N)
            if pct is not None:
                s = torch.full_like(s, 1) * torch.exp2(normal_pct() * self.scale_std)
            push(scale2d_inv(s, s))
        p_rot = 1 - torch.sqrt((1 - self.rotate * p).clamp(0, 1))          # P(pre or post) = rotate * p
        if self.rotate > 0:
            theta = gated((rand(N) * 2 - 1) * np.pi * self.rotate_max, 0, p_rot, N)
            if pct is not None:
                theta = torch.full_like(theta, 1) * ((pct * 2 - 1) * np.pi * self.rotate_max)
            push(rotate2d_inv(-theta))
        if self.aniso > 0:
            s = gated(torch.exp2(randn(N) * self.aniso_std), 1, self.aniso * p, N)
            if pct is not None:
                s = torch.full_like(s, 1) * torch.exp2(normal_pct() * self.aniso_std)
            push(scale2d_inv(s, 1 / s))
        if self.rotate > 0:
            theta = gated((rand(N) * 2 - 1) * np.pi * self.rotate_max, 0, p_rot, N)
            if pct is not None:
                theta = torch.zeros_like(theta)
            push(rotate2d_inv(-theta))
        if self.xfrac > 0:
            t = gated(randn(N, 2) * self.xfrac_std, 0, self.xfrac * p, N, 1)
            if pct is not None:
                t = torch.full_like(t, 1) * (normal_pct() * self.xfrac_std)
            push(translate2d_inv(t[:, 0] * width, t[:, 1] * height))
        out.G_inv = G

        # ---- colour: C @ colour_in -> colour_out ----
        C = None
        def push_left(M):
            nonlocal C
            C = M if C is None else M @ C
        eye4 = torch.eye(4, device=dev)
        luma = _const(np.asarray([1, 1, 1, 0]) / np.sqrt(3), device=dev)
        vv = torch.outer(luma, luma)
        if self.brightness > 0:
            b = gated(randn(N) * self.brightness_std, 0, self.brightness * p, N)
            if pct is not None:
                b = torch.full_like(b, 1) * (normal_pct() * self.brightness_std)
            push_left(translate3d(b, b, b))
        if self.contrast > 0:
            c = gated(torch.exp2(randn(N) * self.contrast_std), 1, self.contrast * p, N)
            if pct is not None:
                c = torch.full_like(c, 1) * torch.exp2(normal_pct() * self.contrast_std)
            push_left(scale3d(c, c, c))
        if self.lumaflip > 0:
            i = gated(torch.floor(rand(N, 1, 1) * 2), 0, self.lumaflip * p, N, 1, 1)
            if pct is not None:
                i = torch.full_like(i, 1) * torch.floor(pct * 2)
            push_left(eye4 - 2 * vv * i)                                    # Householder reflection about the luma axis
        if self.hue > 0 and num_channels > 1:
            theta = gated((rand(N) * 2 - 1) * np.pi * self.hue_max, 0, self.hue * p, N)
            if pct is not None:
                theta = torch.full_like(theta, 1) * ((pct * 2 - 1) * np.pi * self.hue_max)
            push_left(rotate3d(luma, theta))
        if self.saturation > 0 and num_channels > 1:
            s = gated(torch.exp2(randn(N, 1, 1) * self.saturation_std), 1, self.saturation * p, N, 1, 1)
            if pct is not None:
                s = torch.full_like(s, 1) * torch.exp2(normal_pct() * self.saturation_std)
            push_left(vv + (eye4 - vv) * s)
        out.C = C

        # ---- image-space filter: per-band gains, power-normalised, folded into one 43-tap filter per sample ----
        if self.imgfilter > 0:
            bands = self.Hz_fbank.shape[0]
            assert len(self.imgfilter_bands) == bands
            power = _const(np.array([10, 1, 1, 1]) / 13, device=dev)       # expected 1/f power per band
            g = torch.ones([N, bands], device=dev)
            for k, strength in enumerate(self.imgfilter_bands):
                t_k = gated(torch.exp2(randn(N) * self.imgfilter_std), 1, self.imgfilter * p * strength, N)
                if pct is not None:
                    t_k = torch.full_like(t_k, 1) * torch.exp2(normal_pct() * self.imgfilter_std) if strength > 0 else torch.ones_like(t_k)
                t = torch.ones([N, bands], device=dev)
                t[:, k] = t_k
                g = g * (t / (power * t.square()).sum(dim=-1, keepdim=True).sqrt())
            out.Hz_prime = g @ self.Hz_fbank.to(dev)

        # ---- corruptions ----
        if self.noise > 0:
            sigma = gated(randn(N, 1, 1, 1).abs() * self.noise_std, 0, self.noise * p, N, 1, 1, 1)
            if pct is not None:
                sigma = torch.full_like(sigma, 1) * (torch.erfinv(pct) * self.noise_std)
            out.noise_sigma = sigma
        if self.cutout > 0:
            size = gated(torch.full([N, 2, 1, 1, 1], self.cutout_size, device=dev), 0, self.cutout * p, N, 1, 1, 1, 1)
            center = rand(N, 2, 1, 1, 1)
            if pct is not None:
                size = torch.full_like(size, self.cutout_size)
                center = torch.full_like(center, 1) * pct
            out.cutout_size, out.cutout_center = size, center
        return out

    # ---- execution ----

    def apply(self, images, params=None, noise=None):
        """Run the stages on given parameters.  `noise`: the [N, C, H, W] standard-normal draw of the noise stage (drawn here when None)."""
        if callable(images) and params is None:            # `torch.nn.Module.apply(fn)`, which this method shadows (a parent's `.apply(init_fn)`)
            return super().apply(images)
        if params is None:
            raise TypeError('AugmentPipe.apply(images, params, noise=None): params (from sample_params) is missing')
        n, c, h, w = _check_images(images, 'AugmentPipe.apply')
        dev = images.device
        if params.G_inv is not None or params.C is not None:
            images = _geometric_color(images, params.G_inv, params.C, self.Hz_geom)
        if params.Hz_prime is not None:
            taps = params.Hz_prime.to(images.dtype)
            k = taps.shape[1] // 2
            taps = taps.unsqueeze(1).repeat([1, c, 1]).reshape([n * c, 1, -1])
            x = images.reshape([1, n * c, h, w])
            x = torch.nn.functional.pad(input=x, pad=[k, k, k, k], mode='reflect')
            x = conv2d_gradfix.conv2d(input=x, weight=taps.unsqueeze(2), groups=n * c)
            x = conv2d_gradfix.conv2d(input=x, weight=taps.unsqueeze(3), groups=n * c)
            images = x.reshape([n, c, h, w])
        if params.noise_sigma is not None:
            if noise is None:
                noise = torch.randn([n, c, h, w], device=dev)
            images = images + noise * params.noise_sigma
        if params.cutout_size is not None:
            size, center = params.cutout_size, params.cutout_center
            xs = torch.arange(w, device=dev).reshape([1, 1, 1, -1])
            ys = torch.arange(h, device=dev).reshape([1, 1, -1, 1])
            keep_x = ((xs + 0.5) / w - center[:, 0]).abs() >= size[:, 0] / 2
            keep_y = ((ys + 0.5) / h - center[:, 1]).abs() >= size[:, 1] / 2
            images = images * torch.logical_or(keep_x, keep_y).to(torch.float32)
        return images

    def forward(self, images, debug_percentile=None):
        n, c, h, w = _check_images(images, 'AugmentPipe')
        return self.apply(images, self.sample_params(n, c, h, w, images.device, debug_percentile=debug_percentile))

#----------------------------------------------------------------------------
