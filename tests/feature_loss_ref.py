"""Test helpers for training/feature_loss.py: `TorchOps`, a restatement in plain torch (any dtype, on the CPU) of every launch the fused passes
of training/lpips.py, training/lpips_alex.py and training/vgg_loss.py make, so that the shared walkers - the orchestration the HIP path runs -
can be checked against autograd without a GPU.  Every method is a vjp of ATen calls or the closed form of the modules' docstrings; none calls
the code under test.  `RecordingOps` also lists the launches in order, under the names `hip_plugin.CALLS` counts them by."""

import torch
import torch.nn.functional as F

EPS = 1e-10

# method of the `ops` object -> the entry point it stands for, as `hip_plugin.CALLS` names it
ENTRY = {'prep': 'lpips_prep', 'prep_backward': 'lpips_prep_backward', 'maxpool2': 'maxpool2', 'maxpool3s2p0': 'maxpool3s2p0',
         'unfold2d': 'unfold2d', 'fold2d': 'fold2d', 'conv': 'modconv2d', 'relu_backward': 'modconv_act_backward',
         'stage_backward': 'lpips_stage_backward', 'tap_backward': 'lpips_tap_backward', 'feat_l1_tap_backward': 'feat_l1_tap_backward',
         'maxpool2_relu_backward': 'maxpool2_relu_backward', 'normalize': 'lpips_head', 'head': 'lpips_head',
         'head_backward': 'lpips_head_backward', 'feat_l1': 'feat_l1'}


def _vjp(fn, x, dy):
    leaf = x.detach().clone().requires_grad_(True)
    with torch.enable_grad():
        (g,) = torch.autograd.grad(fn(leaf), [leaf], dy)
    return g


class TorchOps:
    """The `ops` of `feature_loss.forward_walk` / `backward_walk` and of the three losses' `_fused_*` functions in torch, computing in `dtype`."""

    def __init__(self, dtype=torch.float64):
        self.dtype = dtype

    def prep(self, x, mean, std, f=1, in_scale=1.0, in_shift=0.0):
        v = F.avg_pool2d(x.to(self.dtype), f) * in_scale + in_shift
        return (v - mean.to(self.dtype).reshape(1, 3, 1, 1)) / std.to(self.dtype).reshape(1, 3, 1, 1)

    def prep_backward(self, dy, std, f=1, in_scale=1.0):
        n, _, h, w = dy.shape
        return _vjp(lambda x: TorchOps.prep(self, x, torch.zeros(3), std, f, in_scale, 0.0), torch.zeros(n, 3, h * f, w * f, dtype=self.dtype), dy)

    @staticmethod
    def maxpool2(x):
        return F.max_pool2d(x, 2)

    @staticmethod
    def maxpool3s2p0(x, want_idx=True):
        """-> (pooled, winner bytes ky * 3 + kx of the window anchored at (2 oy, 2 ox), from ATen's flat indices)."""
        y, flat = F.max_pool2d(x, 3, 2, return_indices=True)
        if not want_idx:
            return y, None
        oy = torch.arange(y.shape[2])[:, None]
        ox = torch.arange(y.shape[3])[None, :]
        ky, kx = flat // x.shape[3] - 2 * oy, flat % x.shape[3] - 2 * ox
        assert bool(((ky >= 0) & (ky < 3) & (kx >= 0) & (kx < 3)).all())
        return y, (ky * 3 + kx).to(torch.uint8)

    @staticmethod
    def unfold2d(x, k, stride, pad):
        n, c, h, w = x.shape
        ho, wo = (h + 2 * pad - k) // stride + 1, (w + 2 * pad - k) // stride + 1
        return F.unfold(x, k, padding=pad, stride=stride).reshape(n, c * k * k, ho, wo)

    @staticmethod
    def fold2d(dcol, size, k, stride, pad):
        n, c = dcol.shape[0], dcol.shape[1] // (k * k)
        return _vjp(lambda x: TorchOps.unfold2d(x, k, stride, pad), torch.zeros(n, c, *size, dtype=dcol.dtype), dcol)

    def conv(self, x, w, bias=None, relu=False, mode=0, arith=0):
        assert mode == 0 and arith == 0
        y = F.conv2d(x.to(self.dtype), w.to(self.dtype), None if bias is None else bias.to(self.dtype), padding=w.shape[2] // 2)
        return F.relu(y) if relu else y

    @staticmethod
    def relu_backward(dy, y):
        return dy * (y > 0)

    @staticmethod
    def _route2(y, dpool):
        return _vjp(lambda v: F.max_pool2d(v, 2), y, dpool)

    @staticmethod
    def stage_backward(y, dpool, dtap):
        return (dtap if dpool is None else dtap + TorchOps._route2(y, dpool)) * (y > 0)

    @staticmethod
    def maxpool2_relu_backward(y, dpool):
        return TorchOps._route2(y, dpool) * (y > 0)

    @staticmethod
    def tap_backward(y, g, idx, dtap):
        """idx given: g is routed to the pixel (2 oy + ky, 2 ox + kx) that each winner byte names; idx None: g (or nothing) is added as it is."""
        total = dtap
        if idx is not None:
            n, c, h, w = y.shape
            assert idx.dtype == torch.uint8 and idx.shape == g.shape
            oy = torch.arange(g.shape[2])[:, None]
            ox = torch.arange(g.shape[3])[None, :]
            flat = (2 * oy + idx.long() // 3) * w + 2 * ox + idx.long() % 3
            total = total + torch.zeros(n, c, h * w, dtype=g.dtype).scatter_add_(2, flat.reshape(n, c, -1), g.reshape(n, c, -1)).reshape(y.shape)
        elif g is not None:
            total = total + g
        return total * (y > 0)

    @staticmethod
    def feat_l1_tap_backward(a, t, g, dloss, weight):
        l1 = torch.sign(a - t) * (dloss.reshape([]) * weight / a.numel())
        return (l1 if g is None else g + l1) * (a > 0)

    @staticmethod
    def _unit(a):
        return a / (a.square().sum(dim=1, keepdim=True).sqrt() + EPS)

    @staticmethod
    def normalize(acts):
        return [TorchOps._unit(a) for a in acts]

    def head(self, acts, targets, lins):
        total = torch.zeros([], dtype=self.dtype)
        for u, t, lin in zip(map(self._unit, acts), targets, lins):
            total = total + (lin.to(self.dtype).reshape(1, -1, 1, 1) * (u - t).square()).sum(dim=1).mean(dim=(1, 2)).sum() / u.shape[0]
        return total

    def head_backward(self, acts, targets, lins, dloss):
        """The closed form of training/lpips.py: da = g / (|a| + eps) - a (sum_c g a) / (|a| (|a| + eps)^2), the second term 0 where |a| = 0,
        for g = d loss / d u = dloss 2 lin (u - t) / (h w N)."""
        out = []
        for a, u, t, lin in zip(acts, map(self._unit, acts), targets, lins):
            n, _, h, w = a.shape
            g = dloss.reshape([]) * 2 * lin.to(self.dtype).reshape(1, -1, 1, 1) * (u - t) / (h * w * n)
            norm = a.square().sum(dim=1, keepdim=True).sqrt()
            coef = (g * a).sum(dim=1, keepdim=True) / (norm * (norm + EPS).square()).masked_fill(norm == 0, 1.0)
            out.append(g / (norm + EPS) - a * coef.masked_fill(norm == 0, 0.0))
        return out

    def feat_l1(self, acts, targets, weights):
        total = torch.zeros([], dtype=self.dtype)
        for a, t, wt in zip(acts, targets, weights):
            total = total + wt * (a - t).abs().mean()
        return total


class RecordingOps(TorchOps):
    """`TorchOps` that appends the name of every launch to `.log`."""

    def __init__(self, dtype=torch.float64):
        super().__init__(dtype)
        self.log = []
        for name in ENTRY:
            setattr(self, name, self._recorded(name, getattr(super(), name)))

    def _recorded(self, name, fn):
        def call(*args, **kwargs):
            self.log.append(name)
            return fn(*args, **kwargs)
        return call
