"""Test helpers for training/parse_loss.py: the parser with name-derived weights, the fixture, and `TorchOps`, a restatement in plain torch
(any dtype, any device) of every launch the fused pass makes, so that `parse_loss._fused_forward` / `_fused_backward` - the orchestration
the HIP path runs - can be checked against autograd on the CPU, and each HIP pass against float64 on the GPU."""

import os

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ((2, 3, 64, 64), (1, 3, 96, 64))


def parser(device='cpu', dtype=torch.float32):
    from oracle import face_parsing as ofp
    from training import face_parsing
    torch.manual_seed(5)
    net = face_parsing.BiSeNet(n_classes=20)
    net.load_state_dict(ofp.synthetic_state_dict({k: list(v.shape) for k, v in net.state_dict().items()}))
    return net.to(device=device, dtype=dtype).eval().requires_grad_(False)


def fixture(i):
    """-> (image, labels int64, loss, grad) of case i of tests/golden/parse_loss.npz."""
    d = np.load(os.path.join(ROOT, 'tests', 'golden', 'parse_loss.npz'))
    return (torch.from_numpy(d[f'{i}/image']), torch.from_numpy(d[f'{i}/labels'].astype(np.int64)), torch.from_numpy(d[f'{i}/loss']),
            torch.from_numpy(d[f'{i}/grad']))


def definition(net, img, target):
    """(loss, d loss / d img) of the module's definition through autograd, in the dtype of `img`."""
    leaf = img.clone().requires_grad_(True)
    loss = F.cross_entropy(net(leaf)[0], target)
    (g,) = torch.autograd.grad(loss, [leaf])
    return loss.detach(), g


def _vjp(fn, x, dy):
    leaf = x.detach().clone().requires_grad_(True)
    with torch.enable_grad():
        (g,) = torch.autograd.grad(fn(leaf), [leaf], dy)
    return g


class TorchOps:
    """The `ops` of parse_loss._fused_forward / _fused_backward in torch, computing in `dtype`."""

    def __init__(self, dtype=torch.float64):
        self.dtype = dtype

    def conv(self, x, w, bias, relu, mode=0):
        x, w = x.to(self.dtype), w.to(self.dtype)
        bias = None if bias is None else bias.to(self.dtype)
        if mode == 0:
            y = F.conv2d(x, w, bias, padding=w.shape[2] // 2)
        elif mode == 1:
            y = F.conv2d(x, w, bias, stride=2)
        else:
            y = F.conv_transpose2d(x, w.transpose(0, 1), bias, stride=2)
        return F.relu(y) if relu else y

    @staticmethod
    def relu_backward(dy, y):
        return dy * (y > 0)

    @staticmethod
    def maxpool(x, want_index=True):
        return F.max_pool2d(x, 3, 2, 1, return_indices=True)

    @staticmethod
    def maxpool_backward(dy, idx, size, mask=None):
        n, c = dy.shape[:2]
        dx = torch.zeros(n, c, size[0] * size[1], dtype=dy.dtype, device=dy.device).scatter_add_(2, idx.reshape(n, c, -1), dy.reshape(n, c, -1))
        dx = dx.reshape(n, c, *size)
        return dx * (mask > 0) if mask is not None else dx

    @staticmethod
    def join(terms, scale=None, bias=None, bias_gain=1.0, y=None, post=0):
        terms = [t if isinstance(t, tuple) else (t, False) for t in terms]
        v = terms[0][0] * scale.reshape(*terms[0][0].shape[:2], 1, 1) if scale is not None else terms[0][0].clone()
        for t, half in terms[1:]:
            if half:
                v[:, :, ::2, ::2] += t
            else:
                v = v + t
        if bias is not None:
            v = v + bias.reshape(*v.shape[:2], 1, 1) * bias_gain
        return F.relu(v) if post == 1 else (v * (y > 0) if post == 2 else v)

    @staticmethod
    def plane_sums(a, b=None, gain=1.0):
        return (a if b is None else a * b).sum(dim=(2, 3), keepdim=True) * gain

    @staticmethod
    def resize(x, size):
        return F.interpolate(x, tuple(size), mode='bilinear', align_corners=True)

    @staticmethod
    def resize_backward(dy, size):
        n, c, H, W = dy.shape
        return _vjp(lambda x: TorchOps.resize(x, (H, W)), torch.zeros(n, c, *size, dtype=dy.dtype, device=dy.device), dy)

    @staticmethod
    def ce(logits, labels):
        return F.cross_entropy(TorchOps.resize(logits, labels.shape[1:]), labels), None

    @staticmethod
    def ce_backward(logits, labels, lse, dloss):
        return _vjp(lambda x: TorchOps.ce(x, labels)[0], logits, dloss.reshape([]).to(logits.dtype))

    def stem_backward(self, dz, weight, size):
        w = weight.to(dz.dtype)
        return _vjp(lambda x: F.conv2d(x, w, stride=2, padding=3), torch.zeros(dz.shape[0], 3, *size, dtype=dz.dtype, device=dz.device), dz)
