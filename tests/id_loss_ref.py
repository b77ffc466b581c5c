"""Test helpers for training/id_loss.py: weights that are a function of the parameter names, the fixture, a float64 functional restatement of
the loss (independent of the module: plain `torch.nn.functional` calls on a state dict), and `TorchOps`, a restatement in plain torch of
every launch the fused pass makes, so that `id_loss._fused_forward` / `_fused_backward` - the orchestration the HIP path runs - can be
checked against autograd on the CPU, and each HIP pass against float64 on the GPU."""

import os
import zlib

import numpy as np
import torch
import torch.nn.functional as F

import parse_loss_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ((2, 3, 256, 256), (1, 3, 512, 512))
IR_SE50 = dict(widths=(64, 128, 256, 512), units=(3, 4, 14, 3))
NARROW = dict(widths=(16, 32, 48, 64), units=(2, 2, 1, 1))          # all three shortcut kinds and a stride-1 SE block
SHORT = dict(widths=(16, 32, 48, 64), units=(1, 1, 1, 1))
GRAD_STEP = 4                                                       # the fixture keeps every 4th row and column of the gradient inside the crop


def synthetic_state_dict(shapes):
    """{name: tensor} for {name: shape}: every tensor is drawn from a generator seeded with the CRC of its NAME, in a range chosen by the
    name, so that the net stays well conditioned through its 24 residual blocks (with BatchNorm weights in 0.5..1.5 everywhere the
    activations grow from 0.24 to 2300 and an fp32 gradient means nothing):
        trailing BatchNorm of the residual branch (res_layer.4.weight) 0.15..0.30, shortcut BatchNorm weights 0.8..1.2, other BatchNorm
        weights 0.5..1.5, running variances 0.5..1.5, running means and biases +-0.1, PReLU slopes 0.1..0.4, convolution and linear
        weights uniform with variance 1 / fan-in.
    Measured with the reference's IR-SE50 on the fixture's first case: the input layer's and every block's output standard deviation stays within
    0.24..0.38 (both fixture cases); ATen's fp32 CPU image gradient is 1.1e-6 of the largest gradient magnitude away from float64, the loss
    1.2e-7."""
    out = {}
    for name, shape in shapes.items():
        g = torch.Generator().manual_seed(zlib.crc32(name.encode()))

        def uniform(lo, hi):
            return torch.rand(*shape, generator=g, dtype=torch.float64) * (hi - lo) + lo
        leaf = name.rsplit('.', 1)[1]
        if leaf == 'num_batches_tracked':
            t = torch.zeros(shape, dtype=torch.int64)
        elif leaf == 'running_var':
            t = uniform(0.5, 1.5)
        elif leaf in ('running_mean', 'bias'):
            t = uniform(-0.1, 0.1)
        elif len(shape) >= 2:                                        # convolution / linear weights
            bound = (3.0 / float(np.prod(shape[1:]))) ** 0.5
            t = uniform(-bound, bound)
        elif name.endswith(('input_layer.2.weight', 'res_layer.2.weight')):
            t = uniform(0.1, 0.4)                                    # PReLU
        elif name.endswith('res_layer.4.weight'):
            t = uniform(0.15, 0.30)
        elif 'shortcut_layer' in name:
            t = uniform(0.8, 1.2)
        else:
            t = uniform(0.5, 1.5)
        out[name] = t if t.dtype == torch.int64 else t.float()
    return out


def backbone(spec=IR_SE50, device='cpu', dtype=torch.float32, mode='ir_se'):
    from training import id_loss
    torch.manual_seed(5)
    net = id_loss.Backbone(112, 50, mode=mode, drop_ratio=0.6, **spec)
    net.load_state_dict(synthetic_state_dict({k: list(v.shape) for k, v in net.state_dict().items()}))
    return net.to(device=device, dtype=dtype).eval().requires_grad_(False)


def idloss(spec=IR_SE50, device='cpu', dtype=torch.float32, mode='ir_se'):
    from training import id_loss
    return id_loss.IDLoss(facenet=backbone(spec, device, dtype, mode))


def smooth_images(shape, seed):
    """uint8 images (value = u8 / 127.5 - 1) that compress: a smooth closed-form pattern plus a seeded term of one quantisation step that is
    constant over 16 x 16 blocks, quantised to multiples of 12 (what the fixture generator draws; the fixture is authoritative)."""
    n, c, h, w = shape
    yy, xx = np.meshgrid(np.arange(h) / h, np.arange(w) / w, indexing='ij')
    rng = np.random.RandomState(seed)
    out = np.empty(shape, dtype=np.uint8)
    q, blk, fs = 12, 16, 0.3
    for i in range(n):
        for ch in range(c):
            a, b, ph = (1.5 + i + 0.5 * ch + 0.1 * seed) * fs, (2.5 - 0.7 * ch + 0.3 * i) * fs, 0.9 * ch + 0.4 * seed
            v = 128 + 70 * np.sin(2 * np.pi * (a * yy + 0.3 * xx) + ph) * np.cos(2 * np.pi * b * xx - ph) + 30 * np.cos(2 * np.pi * (yy - xx) * (1 + ch) * fs)
            v = v + np.kron(rng.randint(-1, 2, size=(h // blk, w // blk)), np.ones((blk, blk))) * q
            out[i, ch] = np.clip(np.rint(v / q) * q, 0, 255).astype(np.uint8)
    return out


def to_float(u8):
    return torch.from_numpy(np.asarray(u8)).to(torch.float32) / 127.5 - 1


_npz = {}


def fixture(i):
    """Case i of tests/golden/id_loss.npz -> dict(y_hat, y (float32 images), feats_hat, feats, loss, sim, grad_samples, grad_sum, grad_norm)."""
    if 'd' not in _npz:
        _npz['d'] = np.load(os.path.join(ROOT, 'tests', 'golden', 'id_loss.npz'))
    d = _npz['d']
    t = lambda k: torch.from_numpy(d[f'{i}/{k}'])
    return dict(y_hat=to_float(d[f'{i}/y_hat']), y=to_float(d[f'{i}/y']), feats_hat=t('feats_hat'), feats=t('feats'), loss=float(d[f'{i}/loss']),
                sim=float(d[f'{i}/sim_improvement']), grad_samples=t('grad_samples'), grad_sum=float(d[f'{i}/grad_sum']), grad_norm=float(d[f'{i}/grad_norm']))


def fixture_keys():
    if 'd' not in _npz:
        _npz['d'] = np.load(os.path.join(ROOT, 'tests', 'golden', 'id_loss.npz'))
    return [str(k) for k in _npz['d']['keys']]


def crop_samples(grad):
    """Every 4th row and column of an image gradient inside the crop (rows 35 f .. 223 f - 1, columns 32 f .. 220 f - 1)."""
    f = grad.shape[2] // 256
    return grad[:, :, 35 * f:223 * f:GRAD_STEP, 32 * f:220 * f:GRAD_STEP]


# ---- the loss from a state dict, functionally ----------------------------------------------------------------------------------------------------
def _bn(sd, p, x):
    return F.batch_norm(x, sd[p + '.running_mean'], sd[p + '.running_var'], sd.get(p + '.weight'), sd.get(p + '.bias'), False, 0.0, 1e-5)


def embed(sd, x, units):
    """Unit embeddings of images x in -1..1 from the state dict `sd`, in the dtype of both."""
    if x.shape[2] != 256:
        x = F.adaptive_avg_pool2d(x, 256)
    x = F.adaptive_avg_pool2d(x[:, :, 35:223, 32:220], 112)
    x = F.prelu(_bn(sd, 'input_layer.1', F.conv2d(x, sd['input_layer.0.weight'], padding=1)), sd['input_layer.2.weight'])
    firsts = {sum(units[:i]) for i in range(4)}
    for i in range(sum(units)):
        s, p = (2 if i in firsts else 1), f'body.{i}.'
        r = F.conv2d(_bn(sd, p + 'res_layer.0', x), sd[p + 'res_layer.1.weight'], padding=1)
        r = F.conv2d(F.prelu(r, sd[p + 'res_layer.2.weight']), sd[p + 'res_layer.3.weight'], stride=s, padding=1)
        r = _bn(sd, p + 'res_layer.4', r)
        g = torch.sigmoid(F.conv2d(F.relu(F.conv2d(r.mean(dim=(2, 3), keepdim=True), sd[p + 'res_layer.5.fc1.weight'])), sd[p + 'res_layer.5.fc2.weight']))
        if p + 'shortcut_layer.0.weight' in sd:
            sc = _bn(sd, p + 'shortcut_layer.1', F.conv2d(x, sd[p + 'shortcut_layer.0.weight'], stride=s))
        else:
            sc = x[:, :, ::s, ::s]
        x = r * g + sc
    x = F.linear(_bn(sd, 'output_layer.0', x).flatten(1), sd['output_layer.3.weight'], sd['output_layer.3.bias'])
    x = _bn(sd, 'output_layer.4', x)
    return x / x.norm(dim=1, keepdim=True)


def loss64(net, y_hat, y, units):
    """float64: (loss, d loss / d y_hat, e(y_hat), e(y)) of the restatement with the parameters of `net`."""
    sd = {k: (v.double() if v.is_floating_point() else v).cpu() for k, v in net.state_dict().items()}
    leaf = y_hat.double().cpu().clone().requires_grad_(True)
    with torch.no_grad():
        t = embed(sd, y.double().cpu(), units)
    e = embed(sd, leaf, units)
    loss = (1 - (e * t).sum(1)).mean()
    (g,) = torch.autograd.grad(loss, [leaf])
    return float(loss.detach()), g, e.detach(), t


def _vjp(fn, x, dy):
    leaf = x.detach().clone().requires_grad_(True)
    with torch.enable_grad():
        (g,) = torch.autograd.grad(fn(leaf), [leaf], dy)
    return g


def prep_definition(x):
    if x.shape[2] != 256:
        x = F.adaptive_avg_pool2d(x, 256)
    return F.adaptive_avg_pool2d(x[:, :, 35:223, 32:220], 112)


class TorchOps(parse_loss_ref.TorchOps):
    """The `ops` of id_loss._fused_forward / _fused_backward in torch, computing in `dtype` (conv, join, plane_sums: parse_loss_ref)."""

    def prep(self, x):
        return prep_definition(x.to(self.dtype))

    def prep_backward(self, dy, size):
        return _vjp(prep_definition, torch.zeros(dy.shape[0], 3, *size, dtype=dy.dtype, device=dy.device), dy)

    def prelu(self, x, slope):
        return F.prelu(x, slope.to(x.dtype))

    def prelu_backward(self, dy, x, slope):
        return torch.where(x > 0, dy, slope.to(x.dtype).reshape(1, -1, 1, 1) * dy)

    def se_gate(self, s, w1, w2):
        return torch.sigmoid(F.conv2d(F.relu(F.conv2d(s, w1.to(s.dtype))), w2.to(s.dtype)))

    def se_gate_backward(self, s, w1, w2, g, dg):
        return _vjp(lambda t: self.se_gate(t, w1, w2), s, dg)

    def linear(self, x, w, b=None):
        return F.linear(x.to(self.dtype), w.to(self.dtype), None if b is None else b.to(self.dtype))

    def linear_backward_input(self, dy, w):
        return dy.to(self.dtype) @ w.to(self.dtype)

    def head(self, f, target=None):
        norm = f.norm(dim=1)
        e = f / norm[:, None]
        return e, norm, (None if target is None else (1 - (e * target.to(e.dtype)).sum(1)).mean())

    def head_backward(self, e, target, norm, dloss):
        g = -dloss.reshape([]).to(e.dtype) * target.to(e.dtype) / e.shape[0]
        return (g - e * (e * g).sum(1, keepdim=True)) / norm[:, None]
