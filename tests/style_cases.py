"""The cases of the style kernels' edge suite (tests/test_gpu_style.py, tests/test_mapping_style_ref_cpu.py): shapes, the route each is built
for, seeded inputs.  A misaligned affine weight is a contiguous view one float into a larger buffer (allocations are at least 16-byte
aligned): 16-byte loads are then impossible and `affine_rows` must take its scalar path although w_dim is a multiple of 4."""

import itertools
import math

import torch

import style_ref

# (n, cin, cout, wdim), misaligned affine weight?, route: vec path, passes of the demodulation over the channels, demodulation launches
STYLE_CASES = [
    ((1, 1, 1, 4), False, dict(vec=True, chunks=1, groups=1)),
    ((2, 7, 5, 30), False, dict(vec=False, chunks=1, groups=1)),             # scalar path, fewer than 64 columns
    ((3, 33, 33, 260), False, dict(vec=True, chunks=1, groups=1)),           # one row / column past a block, one float4 in the second slab
    ((2, 65, 31, 100), True, dict(vec=False, chunks=1, groups=1)),           # scalar path by alignment
    ((8, 520, 40, 64), False, dict(vec=True, chunks=2, groups=1)),           # the second c0 chunk
    ((9, 520, 40, 64), False, dict(vec=True, chunks=2, groups=2)),           # the demodulation splits 8 + 1
    ((17, 48, 1, 36), False, dict(vec=True, chunks=1, groups=3)),
    ((4, 96, 64, 1024), False, dict(vec=True, chunks=1, groups=1)),
    ((5, 64, 0, 512), False, dict(vec=True, chunks=1, groups=0)),            # cout 0: no demodulation (the call passes no wsq_t)
]
VARIANTS = list(itertools.product((True, False), (1.0, 0.37), ('contiguous', 'column', 'expanded')))     # affine_b?, bias_gain, form of w

FOLD_CASES = [(cin, heads, wdim, mis0) for cin in (1, 63, 65, 130) for heads in ((3, 19), (1, 1)) for wdim in (30, 260) for mis0 in (False, True)]
FOLD_N = 3

# job lists of the batch forms: (cin, cout (0 = no demodulation), affine bias?) per job; all at one (n, wdim)
_CYCLE = [(7, 5, True), (33, 33, True), (48, 1, True), (64, 0, True)]
BATCH_LISTS = {
    'jobs24': (4, 36, _CYCLE * 6),
    'jobs25': (4, 36, _CYCLE * 6 + [(33, 33, True)]),
    'first_plain': (4, 36, [(64, 0, True), (33, 33, True), (7, 5, True)]),
    'last_plain': (4, 36, [(33, 33, True), (7, 5, True), (64, 0, True)]),
    'all_plain': (4, 36, [(64, 0, True), (7, 0, True), (33, 0, False)]),
    'no_bias_mixed': (3, 260, [(33, 33, False), (7, 5, True), (65, 31, False), (64, 0, False)]),
    'max_cin': (4, 64, [(1, 1, True), (33, 33, True), (520, 40, True), (33, 5, True)]),
    'n8': (8, 36, [(33, 33, True), (520, 40, True), (64, 0, True)]),
}


def route(shape, affine_ptr=0):
    n, cin, cout, wdim = shape
    return dict(vec=style_ref.is_vec(wdim, affine_ptr), chunks=style_ref.demod_chunks(cin), groups=style_ref.demod_groups(n) if cout else 0)


def _offset(t, misaligned, device='cpu'):
    """A contiguous tensor with t's values whose storage starts 4 bytes (misaligned) or 0 bytes into a fresh buffer on `device`."""
    buf = torch.empty(t.numel() + 4, dtype=t.dtype, device=device)
    out = buf[1 if misaligned else 0:][:t.numel()].view(t.shape)
    out.copy_(t)
    return out


def latent(form, n, wdim, g):
    """w [n, wdim] in one of three forms: contiguous, a column ws[:, 1] of a [n, 3, wdim] tensor (row stride 3 wdim), one latent expanded
    over the batch (row stride 0)."""
    if form == 'contiguous':
        return torch.randn(n, wdim, generator=g)
    if form == 'column':
        return torch.randn(n, 3, wdim, generator=g)[:, 1]
    return torch.randn(wdim, generator=g).expand(n, wdim)


def latent_to(w, device):
    """Move keeping the strides (`.to` may materialise an expanded tensor)."""
    if w.stride(0) == 0:
        return w[0].to(device).expand(w.shape[0], -1)
    if not w.is_contiguous():
        base = torch.zeros(w.shape[0], 3, w.shape[1], device=device)
        base[:, 1] = w.to(device)
        return base[:, 1]
    return w.to(device)


def style_inputs(shape, has_bias, form, seed=0):
    n, cin, cout, wdim = shape
    g = torch.Generator().manual_seed(7000 + seed + 31 * cin + 7 * wdim + n)
    w = latent(form, n, wdim, g)
    A = torch.randn(cin, wdim, generator=g)
    b = torch.randn(cin, generator=g) + 1 if has_bias else None
    wsq_t = None
    if cout:
        W = torch.randn(cout, cin, 3, 3, generator=g)
        wsq_t = W.double().square().sum(dim=[2, 3]).t().contiguous().float()
    return w, A, b, wsq_t, 1 / math.sqrt(wdim)


def fold_inputs(cin, heads, wdim, seed=0):
    g = torch.Generator().manual_seed(9000 + seed + 13 * cin + wdim + heads[1])
    w = latent('column', FOLD_N, wdim, g)
    A0, A1 = torch.randn(cin, wdim, generator=g), torch.randn(cin, wdim, generator=g)
    b0, b1 = torch.randn(cin, generator=g) + 1, torch.randn(cin, generator=g) + 1
    W0, W1 = torch.randn(heads[0], cin, generator=g), torch.randn(heads[1], cin, generator=g)
    return w, 1 / math.sqrt(wdim), A0, b0, W0, 1 / math.sqrt(cin), A1, b1, W1, 0.5 / math.sqrt(cin)


def batch_inputs(name):
    """-> (n, wdim, [(w, A, b, a_gain, b_gain, wsq_t)]) on the CPU; every job reads its own column of one ws tensor."""
    n, wdim, specs = BATCH_LISTS[name]
    g = torch.Generator().manual_seed(11000 + len(specs) + wdim)
    ws = torch.randn(n, len(specs), wdim, generator=g)
    jobs = []
    for k, (cin, cout, has_b) in enumerate(specs):
        A = torch.randn(cin, wdim, generator=g)
        b = torch.randn(cin, generator=g) + 1 if has_b else None
        wsq = (torch.rand(cin, cout, generator=g) + 0.1) if cout else None
        jobs.append((ws[:, k], A, b, 1 / math.sqrt(wdim), 0.37 if k % 2 else 1.0, wsq))
    return n, wdim, ws, jobs
