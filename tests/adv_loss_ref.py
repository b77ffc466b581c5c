"""float64 restatement of the StyleGAN2 discriminator's adversarial loss (training/discriminator.py, training/adv_loss.py; DESIGN.md section
5.38), in plain torch and written from the formulas: the whole function on a state dict (the reference class casts to fp32 inside its
blocks and cannot run in float64), the two passes of csrc/adv_loss.hip with their analytic adjoints, and the shared end-to-end cases.
Not a test module."""

import math
import os

import numpy as np
import torch
import torch.nn.functional as F

SQRT2 = math.sqrt(2.0)
SQRT_HALF = math.sqrt(0.5)

# The end-to-end cases.  `seed` picks weights and inputs whose float64 pre-activations keep clear of every kink (test_adv_loss_cpu.py asserts
# it): a condition that chooses the seed, not a measurement.
CASES = {
    # the reference-run fixture's configuration: n = 4 in two interleaved groups, a mapped label
    'fixture': dict(kwargs=dict(c_dim=25, img_resolution=16, img_channels=6, channel_base=128, channel_max=16, conv_clamp=256,
                                epilogue_kwargs=dict(mbstd_group_size=2)), n=4, seed=1),
    # no label (the logit is `out`'s one feature), n = 1 so G = 1, three blocks
    'uncond': dict(kwargs=dict(c_dim=0, img_resolution=32, img_channels=3, channel_base=256, channel_max=16, conv_clamp=256), n=1, seed=2),
    # two statistic planes, n = 8 in groups of 4, and a clamp that is active on more than 1 % of the activations
    'clamped': dict(kwargs=dict(c_dim=25, img_resolution=16, img_channels=3, channel_base=128, channel_max=16, conv_clamp=1.0,
                                epilogue_kwargs=dict(mbstd_group_size=4, mbstd_num_channels=2)), n=8, seed=3),
}


def synthetic_state_dict(shapes, seed):
    """Weights for a discriminator from its state dict's {name: shape}: standard normal weights (what the layers' constructors draw),
    biases 0.2 * normal (the constructors' zeros would leave them untested); the `resample_filter` buffers are not included."""
    g = torch.Generator().manual_seed(seed)
    out = {}
    for name, shape in shapes.items():
        if name.endswith('resample_filter'):
            continue
        t = torch.randn(list(shape), generator=g)
        if name.endswith('.bias'):
            t = t * 0.2
        elif name.startswith('mapping.fc'):
            t = t * 100.0            # FullyConnectedLayer(lr_multiplier=0.01) draws randn / lr_multiplier
        out[name] = t
    return out


def case_inputs(name):
    """-> (img [n, C, R, R] float32 in about -1..1, c [n, c_dim] float32 or None) of a case."""
    case = CASES[name]
    kw = case['kwargs']
    g = torch.Generator().manual_seed(1000 + case['seed'])
    img = torch.randn([case['n'], kw['img_channels'], kw['img_resolution'], kw['img_resolution']], generator=g).mul(0.5).clamp(-1, 1)
    c = torch.randn([case['n'], kw['c_dim']], generator=g) if kw['c_dim'] > 0 else None
    return img, c


def fixture():
    """tests/golden/discriminator.npz (scripts/make_discriminator_golden.py: the reference's own class on the CPU) -> (the arrays, the state
    dict as tensors)."""
    d = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'discriminator.npz'))
    return d, {k[3:]: torch.from_numpy(d[k]) for k in d.files if k.startswith('sd/')}


def build(name, cls):
    """A discriminator of class `cls` for a case with its synthetic weights, in eval mode and frozen."""
    D = cls(**CASES[name]['kwargs'])
    sd = synthetic_state_dict({k: tuple(v.shape) for k, v in D.state_dict().items()}, CASES[name]['seed'])
    D.load_state_dict(sd, strict=False)
    return D.eval().requires_grad_(False)


# ---- the two passes of csrc/adv_loss.hip --------------------------------------------------------------------------------------------------------
def members(n, G, j):
    """The samples of group j: interleaved with stride n / G."""
    return [g * (n // G) + j for g in range(G)]


def mbstd64(x, group, features, grouping=members):
    """x [n, c, h, w] float64 -> [n, c + features, h, w]; group: G (None or 0: the batch)."""
    n, c, h, w = x.shape
    G = n if not group else min(group, n)
    cf = c // features
    stat = x.new_zeros([n, features, h, w])
    for j in range(n // G):
        idx = grouping(n, G, j)
        xs = x[idx]                                                        # [G, c, h, w]
        sd = ((xs - xs.mean(0, keepdim=True)).square().mean(0) + 1e-8).sqrt()          # [c, h, w]
        for f in range(features):
            stat[idx, f] = sd[f * cf:(f + 1) * cf].mean()
    return torch.cat([x, stat], dim=1)


def mbstd64_backward(x, dy, group, features):
    """-> (dx, term): dx = dy[:, :c] + term, term = D[j, f] / (c / F h w) * (x - mean_G) / (G std)."""
    n, c, h, w = x.shape
    G = n if not group else min(group, n)
    cf = c // features
    term = torch.zeros_like(x)
    for j in range(n // G):
        idx = members(n, G, j)
        xs = x[idx]
        dev = xs - xs.mean(0, keepdim=True)
        sd = (dev.square().mean(0) + 1e-8).sqrt()
        for f in range(features):
            Dsum = dy[idx, c + f].sum()
            ch = slice(f * cf, (f + 1) * cf)
            term[idx, ch] = Dsum / (cf * h * w) * dev[:, ch] / (G * sd[ch])
    return dy[:, :c] + term, term


def softplus64(z):
    return z.clamp(min=0) + torch.log1p(torch.exp(-z.abs()))


def head64(o, cmap, sign):
    """-> (logit [n], loss)."""
    logit = (o * cmap).sum(1) / math.sqrt(o.shape[1]) if cmap is not None else o[:, 0]
    return logit, softplus64(sign * logit).mean()


def head64_backward(o, cmap, logit, dloss, sign):
    k = dloss * sign * torch.sigmoid(sign * logit) / o.shape[0]
    return k[:, None] * cmap / math.sqrt(o.shape[1]) if cmap is not None else k[:, None]


# ---- the whole function ----------------------------------------------------------------------------------------------------------------------------
def _fir(x, f, pad, down):
    """upfirdn2d without up-sampling: zero padding, a true convolution with f, decimation."""
    c = x.shape[1]
    y = F.conv2d(F.pad(x, [pad, pad, pad, pad]), f.flip(0, 1)[None, None].repeat(c, 1, 1, 1), groups=c)
    return y[:, :, ::down, ::down]


def _act(u, act, gain, clamp, taps, name):
    y = (torch.where(u >= 0, u, 0.2 * u) * SQRT2 if act == 'lrelu' else u) * gain
    bound = None if clamp is None else clamp * gain
    if taps is not None:
        taps.append(dict(name=name, act=act, u=u.detach(), y=y.detach(), clamp=bound))
    return y if bound is None else y.clamp(-bound, bound)


def _conv(sd, name, x, act, down=1, gain=1.0, clamp=None, taps=None):
    w = sd[name + '.weight'].double()
    k = w.shape[-1]
    w = w / math.sqrt(w.shape[1] * k * k)
    if down == 2:
        f = sd[name + '.resample_filter'].double()
        fw = f.shape[-1]
        pad = k // 2 + (fw - down + 1) // 2
        assert pad == k // 2 + (fw - down) // 2, 'an even filter pads both sides alike'
        u = F.conv2d(_fir(x, f, pad, 2), w) if k == 1 else F.conv2d(_fir(x, f, pad, 1), w, stride=2)
    else:
        u = F.conv2d(x, w, padding=k // 2)
    b = sd.get(name + '.bias')
    if b is not None:
        u = u + b.double()[None, :, None, None]
    return _act(u, act, gain, clamp, taps, name)


def _fc(sd, name, x, act, lr=1.0, taps=None):
    w = sd[name + '.weight'].double()
    u = x @ (w * (lr / math.sqrt(w.shape[1]))).t() + sd[name + '.bias'].double() * lr
    return _act(u, act, 1.0, None, taps, name)


def cmap64(sd, c):
    """The mapped label: embed, second-moment normalisation, eight leaky-ReLU layers of lr multiplier 0.01."""
    x = _fc(sd, 'mapping.embed', c.double(), 'linear')
    x = x * (x.square().mean(1, keepdim=True) + 1e-8).rsqrt()
    i = 0
    while f'mapping.fc{i}.weight' in sd:
        x = _fc(sd, f'mapping.fc{i}', x, 'lrelu', lr=0.01)
        i += 1
    return x


def logits64(sd, kwargs, img, cmap, taps=None):
    """D(img) [n] in float64 for a `resnet` discriminator's state dict (with its resample_filter buffers); cmap [n, M] float64 or None."""
    clamp = kwargs.get('conv_clamp')
    ep = kwargs.get('epilogue_kwargs', {})
    res = kwargs['img_resolution']
    x = _conv(sd, f'b{res}.fromrgb', img, 'lrelu', clamp=clamp, taps=taps)
    while res > 4:
        y = _conv(sd, f'b{res}.skip', x, 'linear', down=2, gain=SQRT_HALF, taps=taps)
        x = _conv(sd, f'b{res}.conv0', x, 'lrelu', clamp=clamp, taps=taps)
        x = _conv(sd, f'b{res}.conv1', x, 'lrelu', down=2, gain=SQRT_HALF, clamp=clamp, taps=taps)
        x = y + x
        res //= 2
    features = ep.get('mbstd_num_channels', 1)
    if features > 0:
        x = mbstd64(x, ep.get('mbstd_group_size', 4), features)
    x = _conv(sd, 'b4.conv', x, 'lrelu', clamp=clamp, taps=taps)
    x = _fc(sd, 'b4.fc', x.flatten(1), 'lrelu', taps=taps)
    o = _fc(sd, 'b4.out', x, 'linear')
    return head64(o, cmap, -1)[0]


def loss64(sd, kwargs, img, c, sign=-1, taps=None):
    """-> (loss, image gradient, logits), float64: softplus(sign * D(img, c)).mean() and its gradient by float64 autograd."""
    sd = {k: v.detach() for k, v in sd.items()}
    leaf = img.detach().double().requires_grad_(True)
    cmap = cmap64(sd, c) if c is not None else None
    logit = logits64(sd, kwargs, leaf, cmap, taps)
    loss = softplus64(sign * logit).mean()
    (grad,) = torch.autograd.grad(loss, [leaf])
    return float(loss.detach()), grad, logit.detach()


def kink_margin(taps):
    """The smallest distance of a leaky-ReLU pre-activation from its kink at 0, and of an (unclamped) output from an active clamp, over the
    layer's RMS pre-activation."""
    worst = math.inf
    for t in taps:
        if t['act'] != 'lrelu':
            continue
        rms = float(t['u'].square().mean().sqrt())
        worst = min(worst, float(t['u'].abs().min()) / rms)
        if t['clamp'] is not None:
            worst = min(worst, float((t['y'].abs() - t['clamp']).abs().min()) / rms)
    return worst


def clamp_share(taps):
    """The share of the clamped layers' activations that sit on the clamp."""
    on = total = 0
    for t in taps:
        if t['clamp'] is not None:
            on += int((t['y'].abs() > t['clamp']).sum())
            total += t['y'].numel()
    return on / max(total, 1)


def rel_l2(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


def to_numpy_state(sd):
    return {k: np.ascontiguousarray(v.detach().cpu().numpy()) for k, v in sd.items()}
