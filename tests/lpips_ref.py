"""float64 restatement of the VGG16 LPIPS distance (training/lpips.py) and of the streaming passes of csrc/lpips.hip, written out from the
formulas so that it shares no code with the definitions under test, and a synthetic state dict that is a function of the parameter names.
Used by test_lpips_cpu.py and test_gpu_lpips.py."""

import zlib

import torch
import torch.nn.functional as F

STAGES = (2, 2, 3, 3, 3)
CONV_INDEX = (0, 2, 5, 7, 10, 12, 14, 17, 19, 21, 24, 26, 28)
VGG16 = (64, 128, 256, 512, 512)
MEAN = (-.030, -.088, -.188)
STD = (.458, .448, .450)
EPS = 1e-10


def state_dict_keys():
    """The reference class's keys in the order its `state_dict()` lists them: a module's own buffers come before its children."""
    keys = ['net.mean', 'net.std']
    keys += [f'net.layers.{i}.{n}' for i in CONV_INDEX for n in ('weight', 'bias')]
    return keys + [f'lin.{k}.1.weight' for k in range(5)]


def _gen(name):
    return torch.Generator().manual_seed(zlib.crc32(name.encode()))


def synthetic_state_dict(widths=VGG16, bias_shift=None):
    """He-scaled normal weights, biases 0.1 * normal, lin uniform in [0, 1): every tensor a function of its key (and shape) alone.
    bias_shift: {conv index: number added to that layer's bias} (a large negative one makes a tap zero everywhere)."""
    sd = {'net.mean': torch.tensor(MEAN)[None, :, None, None], 'net.std': torch.tensor(STD)[None, :, None, None]}
    cin, convs = 3, iter(CONV_INDEX)
    for count, cout in zip(STAGES, widths):
        for _ in range(count):
            i = next(convs)
            sd[f'net.layers.{i}.weight'] = torch.randn(cout, cin, 3, 3, generator=_gen(f'net.layers.{i}.weight')) * (2.0 / (cin * 9)) ** 0.5
            sd[f'net.layers.{i}.bias'] = torch.randn(cout, generator=_gen(f'net.layers.{i}.bias')) * 0.1 + (bias_shift or {}).get(i, 0.0)
            cin = cout
    for k, c in enumerate(widths):
        sd[f'lin.{k}.1.weight'] = torch.rand(1, c, 1, 1, generator=_gen(f'lin.{k}.1.weight'))
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


def pool64(x):
    """2x2 stride-2 maximum with floor on odd sides, by reshaping."""
    n, c, h, w = x.shape
    return x[:, :, :h // 2 * 2, :w // 2 * 2].reshape(n, c, h // 2, 2, w // 2, 2).amax(dim=(3, 5))


def taps64(sd, z):
    out, h, convs = [], z, iter(CONV_INDEX)
    for s, count in enumerate(STAGES):
        if s > 0:
            h = pool64(h)
        for _ in range(count):
            i = next(convs)
            h = F.conv2d(h, sd[f'net.layers.{i}.weight'].double(), sd[f'net.layers.{i}.bias'].double(), padding=1).clamp_min(0)
        out.append(h)
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
def prep64(x, f, in_scale, in_shift):
    n, c, H, W = x.shape
    v = x.double().reshape(n, c, H // f, f, W // f, f).sum(dim=(3, 5)) / (f * f)
    return (v * in_scale + in_shift - torch.tensor(MEAN).double()[None, :, None, None]) / torch.tensor(STD).double()[None, :, None, None]


def prep_backward64(dy, f, in_scale):
    k = in_scale / (f * f) / torch.tensor(STD).double()[None, :, None, None]
    return (dy.double() * k).repeat_interleave(f, dim=2).repeat_interleave(f, dim=3)


def stage_backward64(y, dpool, dtap):
    """(route(dpool) + dtap) * [y > 0]: autograd through the float64 pool + an explicit mask."""
    total = dtap.double().clone()
    if dpool is not None:
        leaf = y.double().clone().requires_grad_(True)
        (routed,) = torch.autograd.grad(F.max_pool2d(leaf, 2), [leaf], dpool.double())
        total = total + routed
    return total * (y > 0)


def head64(a, t, lin):
    """sum_n mean_{h,w} sum_c lin (u - t)^2 / N of one tap in float64 (differentiable in a)."""
    u = _Unit.apply(a)
    return (lin.double().reshape(1, -1, 1, 1) * (u - t.double()) ** 2).sum(1).mean(dim=(1, 2)).sum() / a.shape[0]
