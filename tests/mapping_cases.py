"""The plugin-level cases of the mapping kernels' edge suite (tests/test_gpu_mapping.py, tests/test_mapping_style_ref_cpu.py): shapes, the
route each is built for (the host and kernel conditions of csrc/mapping.hip, restated), seeded inputs, the telescoped run and its check.

Telescoping: for a case with L layers the entry point is called with the first l layers, l = 1 .. L, `num_ws = 1`, `psi = 1`.  The l-layer
result is the kernel's own activation x_l (exact bits: the kernel is deterministic for fixed shapes), and row [:, 0] of the (l + 1)-layer
result is held to the ONE-layer bound of `mapping_ref.layer` applied to x_l: every layer of a deep launch is checked, with its barrier and
weight prefetch, by a bound that does not grow with depth.

`python tests/mapping_cases.py OUT.npz` runs every case and four truncation combinations on cuda:0 and writes all results to OUT.npz: the
per-layer form (`IDE3D_MAPPING_PER_LAYER`, read once per process) is compared with the default form across two such processes."""

import math
import os
import sys

import numpy as np
import torch

import mapping_ref

WGS, WAVES, RB, NB = 64, 4, 2, 4               # workgroups, waves per workgroup, rows per wave block, images per register block
LR, ALPHA, GAIN = 0.01, 0.2, math.sqrt(2)      # MappingNetwork's lr_multiplier; lrelu's def_alpha and def_gain


def case(name, n, z_dim, c_dim, embed, widths, embed_bias=True, fc_bias=None, route=None):
    return dict(name=name, n=n, z_dim=z_dim, c_dim=c_dim, embed=embed, widths=list(widths), embed_bias=embed_bias,
                fc_bias=[True] * len(widths) if fc_bias is None else list(fc_bias), route=route or {})


def _g(n, with_bias):
    return [case(f'g1{s}', n[0], 0, 3, 8, [8], embed_bias=b, route=dict(one_block=[True], idle=[56]))
            for s, b in with_bias] + \
           [case(f'g2{s}', n[1], 10, 1, 6, [16], embed_bias=b, route=dict(one_block=[True], idle=[48])) for s, b in with_bias] + \
           [case(f'g3{s}', n[2], 512, 25, 512, [512], embed_bias=b, route=dict(one_block=[True], idle=[0])) for s, b in with_bias]


# route: one_block per layer, idle workgroups per layer, and where it is the point of the case: per (rows per workgroup) and blocks
# (register blocks of images in gemv_rows)
CASES = [
    case('a', 1, 4, 0, 0, [4], route=dict(one_block=[True], idle=[60], per=[1])),
    case('b', 4, 32, 0, 0, [36, 40, 32], route=dict(one_block=[True] * 3, idle=[28, 24, 32], per=[1, 1, 1])),
    case('c', 3, 64, 0, 0, [132, 68], route=dict(one_block=[True] * 2, idle=[20, 30], per=[3, 2])),
    case('d', 2, 516, 0, 0, [516, 512, 516, 512], route=dict(one_block=[False, True, False, True], idle=[6, 0, 6, 0], per=[9, 8, 9, 8])),
    case('e8', 8, 1024, 0, 0, [1024, 1024], route=dict(one_block=[False] * 2, idle=[0, 0], per=[16, 16], blocks=2)),
    case('e5', 5, 1024, 0, 0, [1024, 1024], route=dict(one_block=[False] * 2, idle=[0, 0], per=[16, 16], blocks=2)),
    case('e4', 4, 1024, 0, 0, [1024, 1024], route=dict(one_block=[False] * 2, idle=[0, 0], per=[16, 16], blocks=1)),
    case('f', 5, 256, 0, 0, [512, 512], route=dict(one_block=[False] * 2, idle=[0, 0], per=[8, 8], blocks=2)),
    *_g((2, 2, 4), (('', True), ('_nob', False))),
    case('h1', 4, 32, 0, 0, [36, 40, 32], fc_bias=[True, False, True], route=dict(one_block=[True] * 3, idle=[28, 24, 32])),
    case('h0', 4, 32, 0, 0, [36, 40, 32], fc_bias=[False] * 3, route=dict(one_block=[True] * 3, idle=[28, 24, 32])),
    case('i', 1, 8, 0, 0, [8] * 16, route=dict(one_block=[True] * 16, idle=[56] * 16)),
    # n = 3 (one partial register block) in gemv_rows with an odd row count per workgroup, then a one_block layer
    case('j', 3, 64, 0, 0, [516, 132], route=dict(one_block=[False, True], idle=[6, 20], per=[9, 3], blocks=1)),
]
BY_NAME = {c['name']: c for c in CASES}

PSI_BELOW_HALF = float(np.nextafter(np.float32(0.5), np.float32(0)))
# (num_ws, psi, cutoff) of the truncation combinations that the two-process comparison carries (on case b); the in-process test runs the full cross
TRUNC_COMBOS = [(18, 0.7, None), (18, PSI_BELOW_HALF, 1), (18, -0.5, 17), (1, 1.5, 4)]


def cdiv(a, b):
    return -(-a // b)


def route(c):
    """What `mapping_kernel` / `mapping_layer_kernel` do with this shape: per layer, whether a wave owns one block of RB rows and all images
    one register block (`one_block`: cdiv(O, 64) <= 4 waves x RB rows and n <= NB), how many of the 64 workgroups have no row (r0 >= r1),
    rows per workgroup; and the register blocks of images of `gemv_rows`."""
    per = [cdiv(o, WGS) for o in c['widths']]
    return dict(one_block=[p <= WAVES * RB and c['n'] <= NB for p in per],
                idle=[WGS - cdiv(o, p) for o, p in zip(c['widths'], per)],
                per=per, blocks=cdiv(c['n'], NB))


def tensors(c, seed=0):
    """Seeded float32 CPU inputs; weights randn / lr_multiplier as the layers initialise them, biases randn (the layers' zeros would
    hide a misplaced bias row)."""
    g = torch.Generator().manual_seed(1000 + seed + sum(map(ord, c['name'])))
    n, z_dim, c_dim, embed = c['n'], c['z_dim'], c['c_dim'], c['embed']
    t = dict(z=torch.randn(n, z_dim, generator=g), c=None, embed_w=None, embed_b=None, embed_wgain=1.0, embed_bgain=1.0, fc_w=[], fc_b=[])
    if embed:
        t['c'] = torch.randn(n, c_dim, generator=g)
        t['embed_w'] = torch.randn(embed, c_dim, generator=g)
        t['embed_b'] = torch.randn(embed, generator=g) if c['embed_bias'] else None
        t['embed_wgain'] = 1 / math.sqrt(c_dim)
    k = z_dim + embed
    for o, has_b in zip(c['widths'], c['fc_bias']):
        t['fc_w'].append(torch.randn(o, k, generator=g) / LR)
        bias = torch.randn(o, generator=g)
        t['fc_b'].append(bias if has_b else None)
        k = o
    t['w_avg'] = torch.randn(k, generator=g) * 0.3
    return t


def to_device(t, device):
    mv = lambda v: v.to(device) if torch.is_tensor(v) else ([mv(e) for e in v] if isinstance(v, list) else v)
    return {k: mv(v) for k, v in t.items()}


def launch(td, layers=None, num_ws=1, psi=1.0, cutoff=None, w_avg=None):
    """One call of the native entry point with the first `layers` layers of the device tensors `td`."""
    from torch_utils import hip_plugin
    L = len(td['fc_w']) if layers is None else layers
    return hip_plugin.MappingPlugin.mapping(td['z'], td['c'], td['embed_w'], td['embed_b'], td['embed_wgain'], td['embed_bgain'],
                                            td['fc_w'][:L], td['fc_b'][:L], LR, ALPHA, GAIN, num_ws, w_avg, psi, cutoff)


def run(c, device):
    """The telescoped run: [x_1, ..., x_L] as float32 numpy arrays [n, O_l]."""
    td = to_device(tensors(c), device)
    return [launch(td, layers=l)[:, 0].cpu().numpy() for l in range(1, len(c['widths']) + 1)]


def check(c, acts):
    """`acts`: the telescoped results (or a model's) -> worst error / bound per layer."""
    t = tensors(c)
    x, e = mapping_ref.input_stage(t['z'], t['c'], t['embed_w'], t['embed_b'], t['embed_wgain'], t['embed_bgain'])
    ratios = []
    for w, b, got in zip(t['fc_w'], t['fc_b'], acts):
        ref, bound = mapping_ref.layer(x, w, b, LR, ALPHA, GAIN, e_in=e)
        g64 = torch.from_numpy(np.ascontiguousarray(got)).double()
        assert g64.shape == ref.shape, (c['name'], g64.shape, ref.shape)
        assert bool(torch.isfinite(g64).all()), f"case {c['name']}: non-finite activation"
        ratios.append(float(((g64 - ref).abs() / bound).max()))
        x, e = g64, None
    return ratios


def check_truncation(x_last, w_avg, got, num_ws, psi, cutoff):
    """got [n, num_ws, w] float32 numpy -> worst error / bound over the truncated rows; rows outside must be copies of x_last."""
    ref, bound, trunc = mapping_ref.truncate(torch.from_numpy(x_last), w_avg, psi, cutoff, num_ws)
    g = torch.from_numpy(np.ascontiguousarray(got))
    assert tuple(g.shape) == tuple(ref.shape)
    keep = ~trunc
    assert torch.equal(g[:, keep], torch.from_numpy(x_last)[:, None, :].expand(-1, int(keep.sum()), -1)), \
        f'num_ws {num_ws} psi {psi} cutoff {cutoff}: a row outside the cut-off is not a copy of the last activation'
    if not bool(trunc.any()):
        return 0.0
    err = (g.double() - ref).abs()[:, trunc]
    return float((err / (bound[:, trunc] + mapping_ref.TINY)).max())


def run_all(device):
    """Every case telescoped, then the truncation combinations on case b -> {key: array}."""
    out = {}
    for c in CASES:
        for l, a in enumerate(run(c, device)):
            out[f"{c['name']}/{l}"] = a
    b = BY_NAME['b']
    td = to_device(tensors(b), device)
    for i, (num_ws, psi, cutoff) in enumerate(TRUNC_COMBOS):
        out[f'trunc/{i}'] = launch(td, num_ws=num_ws, psi=psi, cutoff=cutoff, w_avg=td['w_avg']).cpu().numpy()
    return out


def check_all(out):
    """The bounds on a `run_all` result -> {case: worst ratio}."""
    worst = {}
    for c in CASES:
        worst[c['name']] = max(check(c, [out[f"{c['name']}/{l}"] for l in range(len(c['widths']))]))
    b = BY_NAME['b']
    x_last = out[f"b/{len(b['widths']) - 1}"]
    w_avg = tensors(b)['w_avg']
    worst['trunc'] = max(check_truncation(x_last, w_avg, out[f'trunc/{i}'], *combo) for i, combo in enumerate(TRUNC_COMBOS))
    return worst


if __name__ == '__main__':
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for p in (os.path.join(root, 'ide-3d_amd'), root):
        if p not in sys.path:
            sys.path.insert(0, p)
    from torch_utils import hip_plugin
    torch.set_grad_enabled(False)
    res = run_all(torch.device('cuda:0'))
    torch.cuda.synchronize()
    assert hip_plugin.CALLS.get('mapping', 0) == sum(len(c['widths']) for c in CASES) + len(TRUNC_COMBOS), hip_plugin.CALLS
    np.savez(sys.argv[1], **res)
