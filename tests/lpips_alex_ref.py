"""float64 restatement of the AlexNet LPIPS distance (training/lpips_alex.py) and of the streaming passes of csrc/lpips_alex.hip, written out
from the formulas so that it shares no code with the definitions under test, and a synthetic state dict that is a function of the parameter
names, the widths and a seed.  Used by test_lpips_alex_cpu.py and test_gpu_lpips_alex.py."""

import zlib

import torch
import torch.nn.functional as F

ALEX = (64, 192, 384, 256, 256)
CONV_INDEX = (0, 3, 6, 8, 10)
GEOMETRY = ((11, 4, 2), (5, 1, 2), (3, 1, 1), (3, 1, 1), (3, 1, 1))          # (kernel, stride, padding)
POOL_BEHIND = (True, True, False, False, False)
MEAN = (-.030, -.088, -.188)
STD = (.458, .448, .450)
EPS = 1e-10


def state_dict_keys():
    """The reference class's keys in the order its `state_dict()` lists them: a module's own buffers come before its children."""
    keys = ['net.mean', 'net.std']
    keys += [f'net.layers.{i}.{n}' for i in CONV_INDEX for n in ('weight', 'bias')]
    return keys + [f'lin.{k}.1.weight' for k in range(5)]


def _gen(name, seed):
    return torch.Generator().manual_seed(zlib.crc32(f'{name}/{seed}'.encode()))


def synthetic_state_dict(widths=ALEX, seed=0, bias_shift=None):
    """He-scaled normal weights, biases 0.1 * normal, lin uniform in [0, 1): every tensor a function of its key, its shape and the seed.
    bias_shift: {conv index: number added to that layer's bias} (a large negative one makes a tap zero everywhere)."""
    sd = {'net.mean': torch.tensor(MEAN)[None, :, None, None], 'net.std': torch.tensor(STD)[None, :, None, None]}
    cin = 3
    for i, cout, (k, _, _) in zip(CONV_INDEX, widths, GEOMETRY):
        sd[f'net.layers.{i}.weight'] = torch.randn(cout, cin, k, k, generator=_gen(f'net.layers.{i}.weight', seed)) * (2.0 / (cin * k * k)) ** 0.5
        sd[f'net.layers.{i}.bias'] = torch.randn(cout, generator=_gen(f'net.layers.{i}.bias', seed)) * 0.1 + (bias_shift or {}).get(i, 0.0)
        cin = cout
    for k, c in enumerate(widths):
        sd[f'lin.{k}.1.weight'] = torch.rand(1, c, 1, 1, generator=_gen(f'lin.{k}.1.weight', seed))
    return sd


class _Unit(torch.autograd.Function):
    """u[c] = a[c] / (|a| + eps) per pixel; backward by the closed form, the norm's part 0 where |a| = 0."""

    @staticmethod
    def forward(ctx, a):
        norm = (a * a).sum(1, keepdim=True) ** 0.5
        ctx.save_for_backward(a, norm)
        return a / (norm + EPS)

    @staticmethod
    def backward(ctx, g):
        a, norm = ctx.saved_tensors
        first = g / (norm + EPS)
        inner = (g * a).sum(1, keepdim=True)
        second = torch.zeros_like(a)
        nz = (norm > 0).expand_as(a)
        second[nz] = (a * inner / (norm * (norm + EPS) ** 2).masked_fill(norm == 0, 1.0))[nz]
        return first - second


def windows(x, k, stride, pad):
    """[n, c, k, k, ho, wo]: entry (ky, kx, oy, ox) = x[oy stride + ky - pad, ox stride + kx - pad], 0 outside — by slicing the padded image."""
    n, c, h, w = x.shape
    ho, wo = (h + 2 * pad - k) // stride + 1, (w + 2 * pad - k) // stride + 1
    xp = torch.zeros(n, c, h + 2 * pad, w + 2 * pad, dtype=x.dtype)
    xp[:, :, pad:pad + h, pad:pad + w] = x
    rows = []
    for ky in range(k):
        rows.append(torch.stack([xp[:, :, ky:ky + (ho - 1) * stride + 1:stride, kx:kx + (wo - 1) * stride + 1:stride] for kx in range(k)], dim=2))
    return torch.stack(rows, dim=2)


def conv64(x, weight, bias, k, stride, pad):
    """A strided, padded convolution from its definition: sum over (ci, ky, kx) of weight * window."""
    return torch.einsum('ncklyx,ockl->noyx', windows(x, k, stride, pad), weight) + bias[None, :, None, None]


def pool64(x):
    """3x3 stride-2 maximum without padding (floor): the maximum over the nine shifted, strided slices."""
    n, c, h, w = x.shape
    oh, ow = (h - 3) // 2 + 1, (w - 3) // 2 + 1
    return windows(x, 3, 2, 0).reshape(n, c, 9, oh, ow).amax(dim=2)


def taps64(sd, z):
    out, h = [], z
    for i, (k, s, p), pool in zip(CONV_INDEX, GEOMETRY, POOL_BEHIND):
        h = conv64(h, sd[f'net.layers.{i}.weight'].double(), sd[f'net.layers.{i}.bias'].double(), k, s, p).clamp_min(0)
        out.append(h)
        if pool:
            h = pool64(h)
    return out


def unit_taps64(sd, x):
    z = (x.double() - sd['net.mean'].double()) / sd['net.std'].double()
    return [_Unit.apply(a) for a in taps64(sd, z)]


def lpips64(sd, x, y):
    """LPIPS(x, y) in float64 (differentiable in x)."""
    ux, uy = unit_taps64(sd, x), [u.detach() for u in unit_taps64(sd, y)]
    total = torch.zeros([], dtype=torch.float64)
    for k, (a, b) in enumerate(zip(ux, uy)):
        lin = sd[f'lin.{k}.1.weight'].double().reshape(1, -1, 1, 1)
        per_image = (lin * (a - b) ** 2).sum(1).sum(dim=(1, 2)) / (a.shape[2] * a.shape[3])
        total = total + per_image.sum()
    return total / x.shape[0]


def lpips64_with_grad(sd, x, y):
    """(value, d value / d x) in float64 on the CPU."""
    leaf = x.detach().cpu().double().requires_grad_(True)
    v = lpips64(sd, leaf, y.detach().cpu())
    (g,) = torch.autograd.grad(v, [leaf])
    return v.detach(), g


def images(shape, seed):
    """(x, y) in [-1, 1]."""
    g = torch.Generator().manual_seed(seed)
    return torch.rand(*shape, generator=g) * 2 - 1, torch.rand(*shape, generator=g) * 2 - 1


# ---- the streaming passes -------------------------------------------------------------------------------------------------------------------
def fold64(dcol, size, k, stride, pad):
    """The adjoint of the unfolding in float64, by scattering every patch entry back to the pixel it was read from."""
    n, ckk, ho, wo = dcol.shape
    c, (h, w) = ckk // (k * k), size
    d = dcol.double().reshape(n, c, k, k, ho, wo)
    xp = torch.zeros(n, c, h + 2 * pad + stride, w + 2 * pad + stride, dtype=torch.float64)
    for ky in range(k):
        for kx in range(k):
            xp[:, :, ky:ky + (ho - 1) * stride + 1:stride, kx:kx + (wo - 1) * stride + 1:stride] += d[:, :, ky, kx]
    return xp[:, :, pad:pad + h, pad:pad + w]


def tap_backward64(y, g, dtap, pooled):
    """(route(g) + dtap) * [y > 0]: autograd through ATen's float64 pool + an explicit mask."""
    total = dtap.double().clone()
    if g is not None and pooled:
        leaf = y.double().clone().requires_grad_(True)
        (routed,) = torch.autograd.grad(F.max_pool2d(leaf, 3, 2), [leaf], g.double())
        total = total + routed
    elif g is not None:
        total = total + g.double()
    return total * (y > 0)
