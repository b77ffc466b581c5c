"""float64 restatement of the VGG19 feature loss (training/vgg_loss.py), written out from the formulas so that it shares no code with the
definition under test, a synthetic state dict that is a function of the parameter names, the widths and a seed, and the kink margins of
the end-to-end cases.  Used by test_vgg_loss_cpu.py and test_gpu_vgg_loss.py.

    s, t = (x + 1) / 2, (y + 1) / 2
    13 convolutions 3x3 padding 1 + ReLU in stages of 2, 2, 4, 4, 1; a 2x2 stride-2 maximum (floor) between the stages
    taps: the ReLU outputs of the first convolution of every stage (relu1_1 .. relu5_1)
    loss = sum_k weight_k * sum |a_k(s) - a_k(t)| / (n c_k h_k w_k)
"""

import zlib

import torch

VGG19 = (64, 128, 256, 512, 512)
STAGES = (2, 2, 4, 4, 1)
CONV_INDEX = (0, 2, 5, 7, 10, 12, 14, 16, 19, 21, 23, 25, 28)
SLICE_OF = (0, 1, 1, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4)          # the reference's slice that holds each convolution
NARROW = (16, 32, 64, 64, 64)
# the end-to-end cases of the GPU test, (widths, n_layers, shape, seed); test_vgg_loss_cpu.py proves the kink margin of each seed
E2E_CASES = [(NARROW, 5, (2, 3, 32, 32), 79), (NARROW, 5, (1, 3, 40, 24), 5), (VGG19, 5, (1, 3, 32, 32), 210), (NARROW, 3, (1, 3, 16, 16), 2)]


def convs_of(n_layers):
    """The convolutions (index into CONV_INDEX) that the first n_layers slices hold."""
    return [j for j, s in enumerate(SLICE_OF) if s < n_layers]


def state_dict_keys(n_layers=5):
    return [f'layers.{SLICE_OF[j]}.{CONV_INDEX[j]}.{n}' for j in convs_of(n_layers) for n in ('weight', 'bias')]


def _gen(name, seed):
    return torch.Generator().manual_seed(zlib.crc32(f'{name}/{seed}'.encode()))


def synthetic_state_dict(widths=VGG19, seed=0, n_layers=5):
    """He-scaled normal weights, biases 0.1 * normal: every tensor a function of its key, its shape and the seed."""
    sd, cin, j = {}, 3, 0
    for count, cout in zip(STAGES, widths):
        for _ in range(count):
            if SLICE_OF[j] < n_layers:
                key = f'layers.{SLICE_OF[j]}.{CONV_INDEX[j]}'
                sd[key + '.weight'] = torch.randn(cout, cin, 3, 3, generator=_gen(key + '.weight', seed)) * (2.0 / (cin * 9)) ** 0.5
                sd[key + '.bias'] = torch.randn(cout, generator=_gen(key + '.bias', seed)) * 0.1
            cin, j = cout, j + 1
    return sd


def images(shape, seed):
    """(x, y) in [-1, 1]."""
    g = torch.Generator().manual_seed(seed)
    return torch.rand(*shape, generator=g) * 2 - 1, torch.rand(*shape, generator=g) * 2 - 1


def conv3(x, weight, bias):
    """A 3x3 convolution with zero padding 1 from its definition: the sum over the nine shifted slices of the padded image."""
    n, c, h, w = x.shape
    xp = torch.zeros(n, c, h + 2, w + 2, dtype=x.dtype)
    xp[:, :, 1:h + 1, 1:w + 1] = x
    out = bias[None, :, None, None].expand(n, weight.shape[0], h, w).clone()
    for ky in range(3):
        for kx in range(3):
            out = out + torch.einsum('nchw,oc->nohw', xp[:, :, ky:ky + h, kx:kx + w], weight[:, :, ky, kx])
    return out


def pool2(x):
    """2x2 stride-2 maximum with floor: the maximum of the four strided slices."""
    h2, w2 = x.shape[2] // 2 * 2, x.shape[3] // 2 * 2
    return torch.stack([x[:, :, dy:h2:2, dx:w2:2] for dy in (0, 1) for dx in (0, 1)]).amax(dim=0)


def walk(sd, z, n_layers=5, dtype=torch.float64):
    """-> (pre-activations of every convolution run, taps) of an image already in [0, 1], in `dtype` on the CPU."""
    pre, taps, h, j = [], [], z.to(dtype), 0
    for s, count in enumerate(STAGES):
        if s >= n_layers:
            break
        if s > 0:
            h = pool2(h)
        for i in range(count):
            if SLICE_OF[j] < n_layers:
                key = f'layers.{SLICE_OF[j]}.{CONV_INDEX[j]}'
                u = conv3(h, sd[key + '.weight'].to(dtype), sd[key + '.bias'].to(dtype))
                pre.append(u)
                h = u.clamp_min(0)
                if i == 0:
                    taps.append(h)
            j += 1
    return pre, taps


def vgg64(sd, x, y, n_layers=5, weights=(1.0,) * 5):
    """The loss in float64 (differentiable in x)."""
    ax = walk(sd, (x.double() + 1) / 2, n_layers)[1]
    ay = [t.detach() for t in walk(sd, (y.double() + 1) / 2, n_layers)[1]]
    total = torch.zeros([], dtype=torch.float64)
    for a, b, wt in zip(ax, ay, weights):
        total = total + wt * (a - b).abs().sum() / a.numel()
    return total


def vgg64_with_grad(sd, x, y, n_layers=5):
    """(value, d value / d x) in float64 on the CPU."""
    leaf = x.detach().cpu().double().requires_grad_(True)
    v = vgg64(sd, leaf, y.detach().cpu(), n_layers)
    (g,) = torch.autograd.grad(v, [leaf])
    return v.detach(), g


def aten_walk32(sd, z, n_layers=5):
    """The same walk by ATen in fp32 on the CPU (the yardstick of the kink margins): (pre-activations, taps)."""
    import torch.nn.functional as F
    pre, taps, h, j = [], [], z.float(), 0
    for s, count in enumerate(STAGES):
        if s >= n_layers:
            break
        if s > 0:
            h = F.max_pool2d(h, 2)
        for i in range(count):
            if SLICE_OF[j] < n_layers:
                key = f'layers.{SLICE_OF[j]}.{CONV_INDEX[j]}'
                u = F.conv2d(h, sd[key + '.weight'], sd[key + '.bias'], padding=1)
                pre.append(u)
                h = F.relu(u)
                if i == 0:
                    taps.append(h)
            j += 1
    return pre, taps


def kink_margins(sd, x, y, n_layers=5):
    """The distance of the source x (the image that is differentiated) from every kink of the loss, in float64:
      'conv': per convolution (m_l, the smallest |pre-activation|): the ReLU;
      'pool': per pool (m_l of the convolution in front of it, the smallest gap between the two largest values of a window whose maximum
              is positive): the winner of a 2x2 maximum;
      'tap':  per tap (m_l, the smallest non-zero |a - t| against the target y): the L1 distance.
    m_l = 8 x the largest error of the fp32 CPU ATen evaluation of that layer against float64 on the same inputs (for a tap: of the tap
    difference, so both images count).  The target's own pre-activations and pool winners are not restricted: y is not differentiated, and
    ReLU and the maximum are continuous, so a sign or a winner that differs there moves t by no more than the rounding error itself."""
    out = {'conv': [], 'pool': [], 'tap': []}
    px, ax = walk(sd, (x.double() + 1) / 2, n_layers)
    ay = walk(sd, (y.double() + 1) / 2, n_layers)[1]
    qx, bx = aten_walk32(sd, (x + 1) / 2, n_layers)
    by = aten_walk32(sd, (y + 1) / 2, n_layers)[1]
    for u, p in zip(px, qx):
        out['conv'].append((8 * float((p.double() - u).abs().max()), float(u.abs().min())))
    ends, last = [], -1
    for count in STAGES[:-1]:
        last += count
        ends.append(last)                                    # the convolution in front of each pool
    for j in ends:
        if j + 1 >= len(px):                                 # (a pool is run only if a convolution follows it)
            break
        h = px[j].clamp_min(0)
        h2, w2 = h.shape[2] // 2 * 2, h.shape[3] // 2 * 2
        top = torch.stack([h[:, :, dy:h2:2, dx:w2:2] for dy in (0, 1) for dx in (0, 1)]).topk(2, dim=0).values
        gap = (top[0] - top[1])[top[0] > 0]
        out['pool'].append((out['conv'][j][0], float(gap.min()) if gap.numel() else float('inf')))
    for a, t, a32, t32 in zip(ax, ay, bx, by):
        d = a - t
        m = 8 * float(((a32.double() - t32.double()) - d).abs().max())
        nz = d[d != 0].abs()
        out['tap'].append((m, float(nz.min()) if nz.numel() else float('inf')))
    return out
