"""csrc/augment.hip on the GPU against the float64 restatement of tests/augment_ref.py: the geometric stage under
per-sample matrices, the colour stage, guarded buffers, the golden file end to end, backward, graph capture, peak memory, the fallbacks and
the C ABI's refusals.  Every bound is n 2^-24 absval + coordinate term, with the counts stated in augment_ref."""
import numpy as np
import pytest
import torch

import augment_ref as R
from training import augment

pytestmark = pytest.mark.gpu

GUARD = 0xA5


def P():
    from torch_utils import hip_plugin
    return hip_plugin.AugmentPlugin


def calls():
    from torch_utils import hip_plugin
    return dict(hip_plugin.CALLS)


def guarded(nbytes, dev, pad=4096):
    big = torch.full([nbytes + 2 * pad], GUARD, dtype=torch.uint8, device=dev)
    return big, big[pad:pad + nbytes]


def untouched_outside(big, nbytes, pad=4096):
    return bool((big[:pad] == GUARD).all()) and bool((big[pad + nbytes:] == GUARD).all())


# ---- per-sample matrices ------------------------------------------------------------------------------------------------------------

def T(tx, ty):
    return np.array([[1, 0, tx], [0, 1, ty], [0, 0, 1.0]])


def S(sx, sy):
    return np.diag([sx, sy, 1.0])


def Rot(t):
    return np.array([[np.cos(t), -np.sin(t), 0], [np.sin(t), np.cos(t), 0], [0, 0, 1.0]])


BAND_SCALE = 0.38        # zoom-out: G_inv scales by 2.63; a 42 x 42 sampling tile then spans 112 texels of U, past the LDS budget (86)


def matrices(H, W):
    """name -> G_inv (output pixel -> input pixel, about the image centre)."""
    return {
        'identity': np.eye(3),
        'xflip': S(-1, 1),
        'rot90': Rot(np.pi / 2),
        'shift_int': T(3, -2),
        'shift_frac': T(2.37, -1.61),
        'rot45': Rot(np.pi / 4),
        'rot0.3': Rot(0.3),
        'scale0.5': S(2, 2),
        'scale2.0': S(0.5, 0.5),
        'band': S(1 / BAND_SCALE, 1 / BAND_SCALE) @ Rot(0.1),
        'aniso1.7': S(1 / 1.7, 1.7),
        'beyond': T(1.4 * W + 0.3, -1.2 * H - 0.6),
    }


def anchor():
    """A sample whose corners reach past every other matrix's (but the two that clamp anyway) by a non-integer amount on all four sides, so the
    batch-wide margins are those of one well-conditioned sample: the margin condition holds whatever exact matrix shares its batch."""
    return S(2.2231, 2.2231) @ Rot(0.3) @ T(0.413, -0.271)


SHAPES = [(1, 1, 2, 2), (3, 3, 5, 7), (2, 3, 17, 33), (2, 19, 16, 33), (4, 1, 40, 24)]      # tile side 16: 5 and 7 below, 16 at, 17, 33 and 40 above


def batches():
    out = []
    names = list(matrices(8, 8))
    for shape in SHAPES:
        n = shape[0]
        per = n if n == 1 else n - 1
        for lo in range(0, len(names), per):
            out.append((shape, tuple(names[lo:lo + per])))
    return out


def batch_matrices(shape, names):
    n, c, h, w = shape
    ms = matrices(h, w)
    G = [ms[k] for k in names]
    while len(G) < n:
        G.append(anchor())
    return np.stack(G).astype(np.float32)


def images(shape, seed):
    return np.random.RandomState(seed).uniform(-1, 1, size=shape).astype(np.float32)


def check_margins(geo, G32, h, w, dev):
    dist = R.margin_distance(geo.raw, h, w)
    print(f'margins {geo.m.tolist()} from {np.round(geo.raw, 4).tolist()}: distance to an integer {dist:.4f}')
    assert dist >= R.MARGIN_CLEARANCE
    m = augment.margins(torch.from_numpy(G32).to(dev), h, w)
    assert m.dtype == torch.int32 and m.is_cuda and m.cpu().tolist() == geo.m.tolist()
    return m


@pytest.mark.parametrize('shape,names', batches(), ids=lambda v: 'x'.join(map(str, v)) if isinstance(v[0], int) else '+'.join(v))
def test_geometric_transform(gpu_device, shape, names):
    n, c, h, w = shape
    G32 = batch_matrices(shape, names)
    geo = R.Geometry(G32.astype(np.float64), h, w, n_c=R.NC_KERNEL)
    m = check_margins(geo, G32, h, w, gpu_device)
    x = images(shape, 31 + h)
    want, absval, ct = geo.forward(x)
    xd, Gd = torch.from_numpy(x).to(gpu_device), torch.from_numpy(G32).to(gpu_device)
    before, loops = calls().get('augment_geometric', 0), P().band_loops(gpu_device)
    got = augment.geometric_transform(xd, Gd)
    assert calls().get('augment_geometric', 0) == before + 1
    assert R.report(f'geometric {shape} {names}', got.cpu().numpy(), want, R.bound(absval, ct))
    looped = P().band_loops(gpu_device) - loops
    if 'band' in names and min(h, w) >= 16:
        assert looped > 0, 'the window of U under a tile exceeds the LDS budget at this scale: the workgroup must have looped over bands'
    # straight through the plugin into a guarded buffer; a second run is bit-equal; the strided input takes the same path
    nbytes = 4 * x.size
    coords = augment.sample_coords(Gd, m, h, w)
    taps = torch.from_numpy(R.taps_f32().astype(np.float32)).to(gpu_device)
    big, view = guarded(nbytes, gpu_device)
    out = view.view(torch.float32).view(n, c, h, w)
    P().geometric(xd, out, coords, m, taps)
    torch.cuda.synchronize()
    assert untouched_outside(big, nbytes)
    assert torch.equal(out, got)
    wide = torch.zeros([n, c, h, w + 3], device=gpu_device); wide[..., :w] = xd
    assert torch.equal(augment.geometric_transform(wide[..., :w], Gd), got)


@pytest.mark.parametrize('shape', [(2, 3, 17, 33), (3, 1, 5, 7)])
def test_color_transform(gpu_device, shape):
    n, c, h, w = shape
    C = np.stack([R.debug_matrices(p, c, h, w)[1] for p in (0.1, 0.62, 0.9)[:n]]).astype(np.float32)
    x = images(shape, 5)
    # colour alone: 3 multiplications + 3 additions
    zero = np.zeros(shape)
    want, absval, _ = R.color(x.astype(np.float64), np.abs(x).astype(np.float64), zero, C.astype(np.float64))
    before = calls().get('augment_color', 0)
    nbytes = 4 * x.size
    big, view = guarded(nbytes, gpu_device)
    xd, Cd = torch.from_numpy(x).to(gpu_device), torch.from_numpy(C).to(gpu_device)
    got = augment.color_transform(xd, Cd)
    assert calls().get('augment_color', 0) == before + 1
    # 6 operations of the kernel + the float32 fold of the grey row (3 additions, a division, a sum) for one channel
    assert R.report(f'colour {shape}', got.cpu().numpy(), want, R.bound(absval, zero, n=12))
    P().color(xd, view.view(torch.float32).view(shape), augment._fused_rows(Cd, c))
    torch.cuda.synchronize()
    assert untouched_outside(big, nbytes) and torch.equal(view.view(torch.float32).view(shape), got)
    # backward: the transposed matrix without the offset
    xg = xd.clone().requires_grad_(True)
    wgt = images(shape, 6)
    (augment.color_transform(xg, Cd) * torch.from_numpy(wgt).to(gpu_device)).sum().backward()
    gw, ga = R.color_transpose(wgt.astype(np.float64), C.astype(np.float64))
    assert R.report('colour backward', xg.grad.cpu().numpy(), gw, R.bound(ga, zero, n=12))


@pytest.mark.parametrize('si,pi', [(si, pi) for si in range(len(R.SHAPES)) for pi in range(len(R.PERCENTILES))])
def test_end_to_end_golden(gpu_device, si, pi):
    x, gold, want, tol, geo, Gn, Cn = R.golden_case(si, pi, R.NC_KERNEL)
    pipe = augment.AugmentPipe(**R.BGC).to(gpu_device)
    before = calls()
    out = pipe(torch.from_numpy(x).to(gpu_device), debug_percentile=R.PERCENTILES[pi])
    after = calls()
    assert after.get('augment_geometric', 0) == before.get('augment_geometric', 0) + 1, 'one fused launch, the colour stage its epilogue'
    assert after.get('augment_color', 0) == before.get('augment_color', 0)
    assert after.get('upfirdn2d', 0) == before.get('upfirdn2d', 0), 'no upfirdn2d launch'
    assert R.report('fused pipeline vs golden', out.cpu().numpy(), gold.astype(np.float64), tol)
    assert R.report('fused pipeline vs restatement', out.cpu().numpy(), want, tol)


@pytest.mark.parametrize('shape', [(2, 3, 17, 33), (2, 19, 5, 7)])
def test_backward(gpu_device, shape):
    n, c, h, w = shape
    G32 = np.stack([matrices(h, w)['rot0.3'] @ S(1.1, 0.8), anchor()]).astype(np.float32)
    C32 = np.stack([R.debug_matrices(p, 3, h, w)[1] for p in (0.3, 0.9)]).astype(np.float32) if c == 3 else None
    geo = R.Geometry(G32.astype(np.float64), h, w, n_c=R.NC_KERNEL)
    check_margins(geo, G32, h, w, gpu_device)
    pipe = augment.AugmentPipe(**R.BGC).to(gpu_device)
    prm = augment.AugmentParams(G_inv=torch.from_numpy(G32).to(gpu_device), C=None if C32 is None else torch.from_numpy(C32).to(gpu_device))
    x, wgt = images(shape, 41), images(shape, 42)
    wd = torch.from_numpy(wgt).to(gpu_device)
    grads = []
    before = calls().get('augment_geometric_backward', 0)
    for _ in range(2):
        xd = torch.from_numpy(x).to(gpu_device).requires_grad_(True)
        (pipe.apply(xd, prm) * wd).sum().backward()
        grads.append(xd.grad.cpu().numpy().astype(np.float64))
    assert calls().get('augment_geometric_backward', 0) == before + 2
    g, ga = (wgt.astype(np.float64), np.abs(wgt).astype(np.float64)) if C32 is None else R.color_transpose(wgt.astype(np.float64), C32.astype(np.float64))
    want, _, _ = geo.transpose(g)
    _, absval, ct = geo.transpose(ga)
    tol = R.bound(absval, ct)
    assert R.report(f'backward {shape}', grads[0], want, tol)
    assert R.report('second run', grads[1], want, tol)
    assert R.report('two runs', grads[0], grads[1], tol)


@pytest.mark.parametrize('shape', [(2, 3, 17, 33), (2, 19, 5, 7), (2, 1, 5, 7)])
def test_second_order(gpu_device, shape):
    """The R1 penalty's path through the fused Functions: a gradient taken with create_graph=True stays on the tape, and
    d/dw of sum(v * grad_x sum(w * apply(x))) is the linear part of apply on v (the forward launch without the colour offset)."""
    n, c, h, w = shape
    G32 = np.stack([matrices(h, w)['rot0.3'] @ S(1.1, 0.8), anchor()]).astype(np.float32)
    C32 = np.stack([R.debug_matrices(p, c, h, w)[1] for p in (0.3, 0.9)]).astype(np.float32) if c in (1, 3) else None
    with_geometry = c != 1                                 # the one-channel case: the colour launch alone
    prm = augment.AugmentParams(G_inv=torch.from_numpy(G32).to(gpu_device) if with_geometry else None,
                                C=None if C32 is None else torch.from_numpy(C32).to(gpu_device))
    pipe = augment.AugmentPipe(**R.BGC).to(gpu_device)
    x = torch.from_numpy(images(shape, 51)).to(gpu_device).requires_grad_(True)
    wgt = torch.from_numpy(images(shape, 52)).to(gpu_device).requires_grad_(True)
    v = images(shape, 53)
    before = calls()
    (g,) = torch.autograd.grad((pipe.apply(x, prm) * wgt).sum(), x, create_graph=True)
    assert g.requires_grad and g.grad_fn is not None
    (gw,) = torch.autograd.grad((g * torch.from_numpy(v).to(gpu_device)).sum(), wgt)
    key = 'augment_geometric' if with_geometry else 'augment_color'
    assert calls().get(key, 0) == before.get(key, 0) + (2 if with_geometry else 3), 'forward, then the second order: the forward launch again'
    v64 = v.astype(np.float64)
    if with_geometry:
        geo = R.Geometry(G32.astype(np.float64), h, w, n_c=R.NC_KERNEL)
        triple = geo.forward(v)
    else:
        triple = (v64, np.abs(v64), np.zeros(shape))
    want, absval, ct = triple if C32 is None else R.color_linear(*triple, C32.astype(np.float64))
    assert R.report(f'second order {shape}', gw.cpu().numpy(), want, R.bound(absval, ct))


def test_graph_capture_needs_no_host_read(gpu_device):
    shape = (2, 3, 17, 33)
    n, c, h, w = shape
    pipe = augment.AugmentPipe(**R.BGC).to(gpu_device)
    cases = []
    for seed, pct in ((1, 0.3), (2, 0.62)):
        G, C = R.debug_matrices(pct, c, h, w)
        cases.append((torch.from_numpy(images(shape, seed)).to(gpu_device), torch.from_numpy(np.stack([G, anchor()]).astype(np.float32)).to(gpu_device),
                      torch.from_numpy(np.stack([C, np.eye(4)]).astype(np.float32)).to(gpu_device)))
    eager = [pipe.apply(x, augment.AugmentParams(G_inv=G, C=C)).clone() for x, G, C in cases]
    assert not torch.equal(eager[0], eager[1])
    x, G, C = (t.clone() for t in cases[0])
    prm = augment.AugmentParams(G_inv=G, C=C)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        pipe.apply(x, prm)                                # warm-up: constants and the counter exist before the capture
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                         # a host read inside would raise here
        out = pipe.apply(x, prm)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager[0])
    x.copy_(cases[1][0]); G.copy_(cases[1][1]); C.copy_(cases[1][2])
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager[1]), 'the margins and the matrices are read on the device at replay'


def test_no_intermediate_in_device_memory(gpu_device):
    shape = (4, 3, 64, 64)
    G = torch.from_numpy(np.stack([S(3.1, 3.1) @ Rot(0.2)] * 4).astype(np.float32)).to(gpu_device)
    assert augment.margins(G, 64, 64).cpu().tolist() == [63] * 4, 'margins clamped: the padded image is 190 x 190, the up-sampled one 380 x 380'
    x = torch.from_numpy(images(shape, 3)).to(gpu_device)
    augment.geometric_transform(x, G)                     # warm-up: constants, the default taps
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = augment.geometric_transform(x, G)
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - base
    print(f'peak rise {rise} bytes for an output of {out.numel() * 4}')
    assert rise <= 2 * out.numel() * 4 + (1 << 20)


def test_fallbacks_take_the_pytorch_definition(gpu_device):
    shape = (2, 3, 17, 33)
    n, c, h, w = shape
    G32 = np.stack([matrices(h, w)['rot0.3'], anchor()]).astype(np.float32)
    geo = R.Geometry(G32.astype(np.float64), h, w, n_c=R.NC_KERNEL)
    x = images(shape, 8)
    want, absval, ct = geo.forward(x)
    tol = R.bound(absval, ct)
    xd, Gd = torch.from_numpy(x).to(gpu_device), torch.from_numpy(G32).to(gpu_device)
    before = calls()
    moved = lambda: {k: v for k, v in calls().items() if k.startswith('augment') and v != before.get(k, 0)}
    Gg = Gd.clone().requires_grad_(True)
    out = augment.geometric_transform(xd, Gg)
    assert out.requires_grad and R.report('G_inv requires grad', out.detach().cpu().numpy(), want, tol)
    augment.fused = False
    try:
        assert R.report('fused = False', augment.geometric_transform(xd, Gd).cpu().numpy(), want, tol)
    finally:
        augment.fused = True
    half = augment.geometric_transform(xd.half(), Gd)
    assert half.dtype == torch.float16
    # float16: every operation of the chain rounds to 11 bits instead of 24, and so does the input
    want16, abs16, ct16 = geo.forward(xd.half().float().cpu().numpy())
    assert R.report('float16', half.float().cpu().numpy(), want16, R.bound(abs16, ct16) * 2.0 ** 13 + 2.0 ** -11 * np.abs(want16))
    assert moved() == {}, 'none of the three took the HIP path'


def test_c_abi_refusals(gpu_device):
    x = torch.zeros(2, 3, 8, 8, device=gpu_device)
    G = torch.eye(3, device=gpu_device).expand(2, 3, 3).contiguous()
    m = augment.margins(G, 8, 8)
    coords = augment.sample_coords(G, m, 8, 8)
    taps = torch.from_numpy(R.taps_f32().astype(np.float32)).to(gpu_device)
    ok = torch.empty_like(x)
    P().geometric(x, ok, coords, m, taps)
    for bad in (dict(out=torch.empty(2 * 3 * 8 * 8 - 1, device=gpu_device)), dict(x=torch.zeros(2, 3, 1, 8, device=gpu_device), out=torch.empty(48, device=gpu_device)),
                dict(x=x.double()), dict(coords=coords[:1]), dict(m=m[:3]), dict(m=m.float()), dict(taps=taps[:8]),
                dict(color=torch.zeros(2, 11, device=gpu_device)), dict(x=torch.zeros(2, 3, 0, 8, device=gpu_device))):
        args = dict(x=x, out=ok, coords=coords, m=m, taps=taps, color=None); args.update(bad)
        with pytest.raises(RuntimeError):
            P().geometric(args['x'], args['out'], args['coords'], args['m'], args['taps'], args['color'])
    x2 = torch.zeros(2, 2, 8, 8, device=gpu_device)
    with pytest.raises(RuntimeError, match='3 channels or 1'):
        P().geometric(x2, torch.empty_like(x2), coords, m, taps, torch.zeros(2, 12, device=gpu_device))
    with pytest.raises(RuntimeError):
        P().color(x2, torch.empty_like(x2), torch.zeros(2, 12, device=gpu_device))
    with pytest.raises(RuntimeError):
        P().geometric_backward(x, torch.empty(5, device=gpu_device), coords, m, taps)
    torch.cuda.synchronize()
