"""The plain convolutions of the loss networks (training/lpips.py, training/parse_loss.py, training/id_loss.py), launch by launch: which
`ide3d_modconv2d` calls one forward + backward of a loss's fused pass makes, the plan class of a launch, and `STAND_INS`, the small
launches that tests/test_gpu_loss_convs.py runs against float64 in place of the workload's.

A launch is `(n, cin, cout, h, w, k, mode, epilogue)`: h, w are what the kernel receives (after the wrappers' padding, decimation or
unfolding); epilogue is 'relu' (bias + ReLU), 'bias' (bias only) or 'grad' (nothing: an input gradient, or a convolution without
BatchNorm), the vocabulary of `hip_plugin.modconv_plan`.  The parser's `ffm.conv1` (ReLU without a bias) is listed as 'relu': the
planner does not look at the bias of a mode-0 launch and the kernel's finish adds 0 for a missing one (csrc/modconv.hip, `s_bi`)."""

import torch

import id_loss_ref
import lpips_ref

ARITHS = (6, 1)          # bf16x6 (the default arithmetic) and fp32 (tests/test_gpu_conv_arith.py: ARITH)


class _Recorder(id_loss_ref.TorchOps):
    """The `ops` of both fused passes with a shape-only convolution: `conv` notes its launch and returns zeros of the output's shape; the
    streaming passes are the float32 torch restatements (on zeros: element-wise work only)."""

    def __init__(self):
        super().__init__(torch.float32)
        self.launches = []

    def conv(self, x, w, bias, relu, mode=0):
        n, cin, h, wd = x.shape
        cout, cin2, k, k2 = w.shape
        assert cin == cin2 and k == k2 and k in (1, 3) and x.is_contiguous(), (tuple(x.shape), tuple(w.shape))
        self.launches.append((n, cin, cout, h, wd, k, mode, 'relu' if relu else ('bias' if bias is not None else 'grad')))
        oh, ow = (2 * h + 1, 2 * wd + 1) if mode == 2 else (((h - 3) // 2 + 1, (wd - 3) // 2 + 1) if mode == 1 else (h, wd))
        return torch.zeros(n, cout, oh, ow)


_cache = {}


def _pair(size):
    return (size, size) if isinstance(size, int) else tuple(size)


def launches(loss, spec, n, size):
    """The convolution launches of one forward + backward of `loss` at batch n:
    'parse': spec = the number of classes (None: 20), size = the image's (H, W) or side;
    'id':    spec = dict(widths=, units=) of the IR-SE backbone (None: IR-SE50), size = the image's side (256 f; the net sees its 112 x 112 crop);
    'lpips': spec = the five VGG widths (None: VGG16), size = the (H, W) or side the feature net sees."""
    key = (loss, repr(spec), n, _pair(size))
    if key not in _cache:
        _cache[key] = tuple(_enumerate(loss, spec, n, _pair(size)))
    return list(_cache[key])


def _enumerate(loss, spec, n, size):
    if loss == 'lpips':
        out, back, cin, (h, w) = [], [], 3, size
        for s, (count, cout) in enumerate(zip(lpips_ref.STAGES, spec or lpips_ref.VGG16)):
            if s > 0:
                h, w = h // 2, w // 2
            for _ in range(count):
                out.append((n, cin, cout, h, w, 3, 0, 'relu'))
                back.append((n, cout, cin, h, w, 3, 0, 'grad'))
                cin = cout
        return out + back[::-1]
    ops = _Recorder()
    with torch.no_grad():
        if loss == 'parse':
            from training import face_parsing, parse_loss
            net = face_parsing.BiSeNet(n_classes=spec or 20).eval().requires_grad_(False)
            x, target = torch.zeros(n, 3, *size), torch.zeros(n, *size, dtype=torch.int64)
            _, saved = parse_loss._fused_forward(ops, net, x, target)
            parse_loss._fused_backward(ops, net, saved, torch.ones(1))
        elif loss == 'id':
            from training import id_loss
            net = id_loss.Backbone(112, 50, mode='ir_se', **(spec or id_loss_ref.IR_SE50)).eval().requires_grad_(False)
            x, target = torch.zeros(n, 3, *size), torch.zeros(n, 512)
            target[:, 0] = 1
            _, _, saved = id_loss._fused_forward(ops, net, x, target)
            id_loss._fused_backward(ops, net, saved, torch.ones(1))
        else:
            raise ValueError(loss)
    return ops.launches


# (loss, spec, batch, size): what a projector step runs
WORKLOADS = (('parse', None, 1, 512), ('lpips', None, 1, 256), ('lpips', None, 4, 256), ('id', None, 1, 256), ('id', None, 4, 256))


def workload_launches():
    """Every distinct launch of the workload set, in order of first appearance."""
    seen = {}
    for wl in WORKLOADS:
        for l in launches(*wl):
            seen.setdefault(l, wl)
    return list(seen)


def out_size(launch):
    n, cin, cout, h, w, k, mode, epi = launch
    return (2 * h + 1, 2 * w + 1) if mode == 2 else (((h - 3) // 2 + 1, (w - 3) // 2 + 1) if mode == 1 else (h, w))


def plan(launch, arith):
    from torch_utils import hip_plugin
    n, cin, cout, h, w, k, mode, epi = launch
    return hip_plugin.modconv_plan(n, cin, cout, h, w, k=k, mode=mode, arith=arith, epilogue=epi)


PLAN_FIELDS = ('kind', 'tile_h', 'tile_w', 'images_per_tile', 'rows', 'waves', 'parts')


def plan_class(launch, arith):
    """(k, mode, epilogue, kind, tile_h, tile_w, images_per_tile, rows, waves, parts, split_k > 1, strip, transposed_all_class) of the
    plan + the predicates on which the kernels' staging and finish (csrc/modconv.hip) take another path in this regime:
      cin % 32 != 0, cout < 64       the two the issue names;
      cin % KC != 0                  a K tail: the last chunk's channels beyond cin are staged as zeros (`live` / `sty[k]`: fp32 loop lines
                                     444-455 with KC = 4 for 3x3, 16 for 1x1, `ModeCfg`; split loop lines 945-946 with KC = 16);
      cout % rows != 0               rows of the last M block beyond cout are skipped by the finish (`co >= p.cout`, lines 276 and 309);
      n % images_per_tile != 0       a tile's images beyond n are staged as zeros and skipped (lines 385, 251, 299);
      a ragged store tail            the vector finish stores 4 pixels of a row at once unless `ox + 3 >= ow` (lines 251, 281-284): ow % 4
                                     != 0; under split-K the reduction kernel takes 16-byte accesses only if oh * ow % 4 == 0 (line 1764).
    The flattened form of a 1x1 launch (`flatten_pointwise`: h * w % 4 == 0 and >= 128) shows as the 1 x 128 tile."""
    n, cin, cout, h, w, k, mode, epi = launch
    p = plan(launch, arith)
    oh, ow = out_size(launch)
    kc = 16 if (p['parts'] or k == 1) else 4
    tail = (oh * ow) % 4 != 0 if p['split_k'] > 1 else ow % 4 != 0
    return (k, mode, epi) + tuple(p[f] for f in PLAN_FIELDS) + (p['split_k'] > 1, p['strip'], p['transposed_all_class'],
            cin % 32 != 0, cout < 64, cin % kc != 0, cout % p['rows'] != 0, n % p['images_per_tile'] != 0, tail)


def classes_of(launch_list):
    """{(arith, plan class): [launches]}"""
    out = {}
    for l in launch_list:
        for a in ARITHS:
            out.setdefault((a, plan_class(l, a)), []).append(l)
    return out


# ---- the stand-ins -------------------------------------------------------------------------------------------------------------------------------
# (launch, the arithmetics in which it stands for a plan class of the workload set): for every (arithmetic, plan class) of WORKLOADS the
# cheapest launch of that class found by a search over n in 1..9, the channel counts 3 .. 512 of the nets and maps of 1 .. 258 pixels a side
# (h x h, h x (h + 1), h x (h + 3), h x 2h).  tests/test_loss_conv_plans_cpu.py holds the table to the planner in both directions.
CLASS_STAND_INS = (
    ((1, 32, 128, 8, 16, 1, 0, 'bias'), (6, 1)),
    ((1, 128, 128, 1, 1, 1, 0, 'bias'), (6, 1)),
    ((1, 128, 128, 6, 7, 1, 0, 'bias'), (6, 1)),
    ((1, 128, 128, 8, 16, 1, 0, 'bias'), (6, 1)),
    ((2, 128, 128, 6, 7, 1, 0, 'bias'), (6, 1)),
    ((1, 3, 128, 8, 16, 1, 0, 'grad'), (6, 1)),
    ((1, 32, 128, 1, 1, 1, 0, 'grad'), (6, 1)),
    ((1, 128, 3, 8, 16, 1, 0, 'grad'), (6, 1)),
    ((1, 128, 64, 1, 1, 1, 0, 'grad'), (6, 1)),
    ((1, 128, 64, 8, 16, 1, 0, 'grad'), (6, 1)),
    ((1, 128, 128, 1, 1, 1, 0, 'grad'), (6, 1)),
    ((1, 128, 128, 6, 7, 1, 0, 'grad'), (6, 1)),
    ((1, 128, 128, 8, 16, 1, 0, 'grad'), (6, 1)),
    ((2, 128, 128, 6, 7, 1, 0, 'grad'), (6, 1)),
    ((1, 3, 64, 8, 16, 1, 0, 'relu'), (6, 1)),
    ((1, 128, 64, 1, 1, 1, 0, 'relu'), (6, 1)),
    ((1, 128, 128, 1, 1, 1, 0, 'relu'), (6, 1)),
    ((1, 128, 128, 8, 16, 1, 0, 'relu'), (6, 1)),
    ((1, 3, 64, 12, 12, 3, 0, 'bias'), (6, 1)),
    ((1, 32, 64, 12, 12, 3, 0, 'bias'), (1,)),
    ((1, 32, 128, 6, 7, 3, 0, 'bias'), (1,)),
    ((1, 32, 128, 12, 12, 3, 0, 'bias'), (1,)),
    ((1, 64, 64, 12, 12, 3, 0, 'bias'), (6,)),
    ((1, 256, 128, 1, 1, 3, 0, 'bias'), (6,)),
    ((1, 256, 128, 1, 4, 3, 0, 'bias'), (6,)),
    ((2, 32, 128, 6, 7, 3, 0, 'bias'), (1,)),
    ((1, 32, 3, 12, 12, 3, 0, 'grad'), (6, 1)),
    ((1, 32, 3, 256, 256, 3, 0, 'grad'), (6, 1)),
    ((1, 32, 64, 12, 12, 3, 0, 'grad'), (1,)),
    ((1, 32, 64, 256, 256, 3, 0, 'grad'), (1,)),
    ((1, 32, 128, 6, 7, 3, 0, 'grad'), (1,)),
    ((1, 32, 128, 12, 12, 3, 0, 'grad'), (1,)),
    ((1, 64, 64, 12, 12, 3, 0, 'grad'), (6,)),
    ((1, 64, 128, 12, 12, 3, 0, 'grad'), (6,)),
    ((1, 256, 64, 1, 4, 3, 0, 'grad'), (6,)),
    ((1, 256, 128, 1, 1, 3, 0, 'grad'), (6,)),
    ((1, 256, 128, 1, 4, 3, 0, 'grad'), (6,)),
    ((2, 32, 128, 6, 7, 3, 0, 'grad'), (1,)),
    ((4, 512, 512, 18, 18, 3, 0, 'grad'), (6,)),
    ((9, 32, 512, 33, 36, 3, 0, 'grad'), (1,)),
    ((9, 64, 64, 114, 228, 3, 0, 'grad'), (6,)),
    ((9, 256, 512, 17, 20, 3, 0, 'grad'), (6,)),
    ((1, 3, 64, 12, 12, 3, 0, 'relu'), (6, 1)),
    ((1, 32, 64, 12, 12, 3, 0, 'relu'), (1,)),
    ((1, 32, 64, 256, 256, 3, 0, 'relu'), (1,)),
    ((1, 32, 128, 12, 12, 3, 0, 'relu'), (1,)),
    ((1, 64, 64, 12, 12, 3, 0, 'relu'), (6,)),
    ((1, 64, 128, 12, 12, 3, 0, 'relu'), (6,)),
    ((1, 256, 128, 1, 4, 3, 0, 'relu'), (6,)),
    ((4, 512, 512, 18, 18, 3, 0, 'relu'), (6,)),
    ((9, 32, 512, 33, 36, 3, 0, 'relu'), (1,)),
    ((9, 64, 64, 114, 228, 3, 0, 'relu'), (6,)),
    ((9, 256, 512, 17, 20, 3, 0, 'relu'), (6,)),
    ((1, 32, 64, 25, 25, 3, 1, 'bias'), (6, 1)),
    ((1, 32, 128, 13, 16, 3, 1, 'bias'), (6, 1)),
    ((1, 32, 128, 25, 25, 3, 1, 'bias'), (6, 1)),
    ((2, 32, 128, 13, 16, 3, 1, 'bias'), (6, 1)),
    ((1, 32, 128, 25, 25, 3, 1, 'relu'), (6, 1)),
    ((1, 32, 64, 4, 4, 3, 2, 'grad'), (1,)),
    ((1, 32, 64, 16, 17, 3, 2, 'grad'), (6,)),
    ((1, 128, 64, 9, 18, 3, 2, 'grad'), (6,)),
    ((1, 128, 128, 4, 4, 3, 2, 'grad'), (6,)),
)


def _edges():
    out = []
    # [n, c, 1, 1] maps of the attention / squeeze-excite / global-average branches and their gradients
    for n in (1, 3, 9):
        for cin, cout, epi in ((512, 128, 'relu'), (256, 64, 'relu'), (64, 256, 'bias'), (64, 4, 'relu'), (4, 64, 'bias')):
            out += [(n, cin, cout, 1, 1, 1, 0, epi), (n, cout, cin, 1, 1, 1, 0, 'grad')]
    # the unfolded 7x7 stem: a ragged K of 147 on 180 pixels (flattened: 128 + 52) and on 135 pixels (not a multiple of 4: 8 x 8 tiles)
    out += [(1, 147, 64, 12, 15, 1, 0, 'relu'), (1, 147, 64, 9, 15, 1, 0, 'relu')]
    out += [(2, 3, 64, 13, 18, 3, 0, 'relu'), (2, 64, 3, 13, 18, 3, 0, 'grad')]
    out += [(1, 256, 19, 12, 15, 1, 0, 'bias'), (1, 19, 256, 12, 15, 1, 0, 'grad')]
    out += [(1, 512, 256, h, w, 3, 2, 'grad') for h, w in ((1, 1), (2, 3), (7, 7))]
    return tuple(out)


EDGE_LAUNCHES = _edges()
# mode 1 on an input whose one-pixel border is zero (what F.pad hands to the kernel): 4 x 4 -> 1 x 1 and 16 x 16 -> 7 x 7
ZERO_BORDER = ((2, 64, 128, 4, 4, 3, 1, 'bias'), (1, 512, 512, 16, 16, 3, 1, 'bias'))
STAND_INS = CLASS_STAND_INS + tuple((l, ()) for l in EDGE_LAUNCHES + ZERO_BORDER)
