"""float64 restatements of the projector's noise regulariser and noise normaliser (training/projection.py), written with explicit index
arithmetic so that they share no code with the definitions under test.  Used by test_projection_cpu.py and test_gpu_noise_reg.py."""

import torch


def reg64(maps):
    """sum over maps and levels of mean(n * n[left])^2 + mean(n * n[up])^2 in float64 (differentiable); levels: the map, then 2x2 block
    means while the height is above 8; neighbours wrap around."""
    total = torch.zeros([], dtype=torch.float64)
    for n in maps:
        a = n.double()
        while True:
            h, w = a.shape
            left = a[:, (torch.arange(w) - 1) % w]
            up = a[(torch.arange(h) - 1) % h, :]
            total = total + (a * left).sum().div(h * w) ** 2 + (a * up).sum().div(h * w) ** 2
            if h <= 8:
                break
            a = a.reshape(h // 2, 2, w // 2, 2).sum(dim=(1, 3)) / 4
    return total


def reg64_with_grads(maps, upstream=1.0):
    """(loss, [d (upstream * loss) / d map]) in float64 on the CPU."""
    leaves = [m.detach().cpu().double().requires_grad_(True) for m in maps]
    loss = reg64(leaves)
    grads = torch.autograd.grad(loss * upstream, leaves)
    return loss.detach(), list(grads)


def normalize64(maps):
    """n - mean(n), then divided by the root mean square of THAT, in float64 on the CPU."""
    out = []
    for m in maps:
        a = m.detach().cpu().double()
        a = a - a.sum() / a.numel()
        out.append(a / (a * a).sum().div(a.numel()).sqrt())
    return out


def correlated(side, seed):
    """z + 0.6 roll(z, 1, 0) + 0.6 roll(z, 1, 1) with z standard normal: neighbouring pixels correlate, so the level-0 means are about 0.6
    (of a variance of 1.72) and do not cancel."""
    z = torch.randn(side, side, generator=torch.Generator().manual_seed(seed))
    return z + 0.6 * torch.roll(z, 1, 0) + 0.6 * torch.roll(z, 1, 1)


def white(side, seed):
    return torch.randn(side, side, generator=torch.Generator().manual_seed(seed))
