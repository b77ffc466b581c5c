"""training/augment.py without a GPU: the buffers and the PyTorch definition against the reference-run golden file and the float64
restatement of tests/augment_ref.py, the parameter draws, `apply`, the mask warp, backward and the refusals.
Every bound is n 2^-24 absval + coordinate term, with the counts stated in augment_ref."""
import numpy as np
import pytest
import torch

import augment_ref as R
from training import augment

CASES = [(si, pi) for si in range(len(R.SHAPES)) for pi in range(len(R.PERCENTILES))]


@pytest.fixture(scope='module')
def pipe():
    return augment.AugmentPipe(**R.BGC)


def test_names_resolve():
    for name in ('wavelets', 'matrix', 'translate2d', 'translate3d', 'scale2d', 'scale3d', 'rotate2d', 'rotate3d', 'translate2d_inv', 'translate3d_inv',
                 'scale2d_inv', 'scale3d_inv', 'rotate2d_inv', 'rotate3d_inv', 'AugmentPipe', 'geometric_transform', 'color_transform'):
        assert hasattr(augment, name), name
    assert set(augment.wavelets) >= {'sym2', 'sym6'} and augment.fused is True
    import sys
    assert 'scipy' not in augment.__dict__ and not any(getattr(v, '__name__', '').startswith('scipy') for v in vars(augment).values() if isinstance(v, type(sys)))


def test_buffers_match_golden(pipe):
    g = R.golden()
    sd = pipe.state_dict()
    assert set(sd) == {'p', 'Hz_geom', 'Hz_fbank'}
    assert sd['p'].shape == () and float(sd['p']) == 1.0 and tuple(sd['Hz_geom'].shape) == (12,) and tuple(sd['Hz_fbank'].shape) == (4, 43)
    for name in ('Hz_geom', 'Hz_fbank'):
        got, want = sd[name].numpy().astype(np.float64), g[name].astype(np.float64)
        assert (np.abs(got - want) <= 1e-7 * np.abs(want)).all(), name
    assert np.array_equal(R.taps_f32(), g['Hz_geom'].astype(np.float64))


@pytest.mark.parametrize('si,pi', CASES)
def test_golden_bgc(pipe, si, pi):
    x, gold, want, tol, geo, Gn, Cn = R.golden_case(si, pi, R.NC_KERNEL)
    n, c, h, w = R.SHAPES[si]
    dist = R.margin_distance(geo.raw, h, w)
    print(f'margins {geo.m.tolist()} from {geo.raw.tolist()}: distance to an integer {dist:.4f}')
    assert dist >= R.MARGIN_CLEARANCE
    prm = pipe.sample_params(n, c, h, w, 'cpu', debug_percentile=R.PERCENTILES[pi])
    m = augment.margins(prm.G_inv, h, w)
    assert m.dtype == torch.int32 and m.tolist() == geo.m.tolist()
    if h <= 7:
        assert m.tolist() == [w - 1, h - 1, w - 1, h - 1], 'the tiny cases clamp, so the zero border of the sampler is exercised'
    assert R.report('restatement vs golden', gold, want, tol)
    out = pipe(torch.from_numpy(x), debug_percentile=R.PERCENTILES[pi])
    assert out.dtype == torch.float32 and tuple(out.shape) == (n, c, h, w)
    assert R.report('PyTorch definition vs golden', out.numpy(), gold.astype(np.float64), tol)
    assert R.report('PyTorch definition vs restatement', out.numpy(), want, tol)


def test_golden_filter_cutout():
    g = R.golden()
    fc = augment.AugmentPipe(imgfilter=1, cutout=1)
    x = g['fc_x']
    out = fc(torch.from_numpy(x), debug_percentile=0.8).numpy()
    # the 43-tap separable filter: 2 x (43 + 42) operations on |x| <= 1 with taps whose absolute sum is s per axis
    prm = fc.sample_params(*x.shape, 'cpu', debug_percentile=0.8)
    s = float(prm.Hz_prime.abs().sum(dim=1).max())
    tol = 170 * R.U * s * s
    err = float(np.abs(out.astype(np.float64) - g['fc_out']).max())
    print(f'filter + cutout: largest error {err:.3e}, bound {tol:.3e}, ratio {err / tol:.3f}')
    assert err <= tol
    assert (out == 0).any() and prm.G_inv is None and prm.C is None and prm.noise_sigma is None
    assert tuple(prm.Hz_prime.shape) == (2, 43) and tuple(prm.cutout_size.shape) == (2, 2, 1, 1, 1) and tuple(prm.cutout_center.shape) == (2, 2, 1, 1, 1)


def test_sample_params_identity_at_p0(pipe):
    full = augment.AugmentPipe(**R.BGC, imgfilter=1, noise=1, cutout=1)
    full.p.fill_(0)
    prm = full.sample_params(5, 3, 16, 16, 'cpu')
    assert torch.equal(prm.G_inv, torch.eye(3).expand(5, 3, 3)) and torch.equal(prm.C, torch.eye(4).expand(5, 4, 4))
    assert prm.G_inv.dtype == torch.float32 and prm.C.dtype == torch.float32
    assert torch.equal(prm.noise_sigma, torch.zeros(5, 1, 1, 1)) and torch.equal(prm.cutout_size, torch.zeros(5, 2, 1, 1, 1))
    assert tuple(prm.Hz_prime.shape) == (5, 43)
    delta = torch.zeros(43); delta[21] = 1
    assert (prm.Hz_prime - delta).abs().max() < 1e-6, 'unit gains fold the bank into a unit impulse'


@pytest.mark.parametrize('si,pi', [(0, 1), (1, 4), (3, 2)])
def test_sample_params_match_restatement(pipe, si, pi):
    n, c, h, w = R.SHAPES[si]
    prm = pipe.sample_params(n, c, h, w, 'cpu', debug_percentile=R.PERCENTILES[pi])
    G, C = R.debug_matrices(R.PERCENTILES[pi], c, h, w)
    # float32 chains of at most 8 products of 3 x 3 (5 operations an entry) over erfinv / exp2 / sin / cos of a few ulp each: 64 ulp of the
    # largest entry
    for got, want in ((prm.G_inv, G), (prm.C[:, :3], C[:3])):
        tol = 64 * R.U * max(1.0, float(np.abs(want).max()))
        err = float(np.abs(got.numpy().astype(np.float64) - want).max())
        print(f'largest error {err:.3e}, bound {tol:.3e}')
        assert tuple(got.shape)[0] == n and err <= tol


def test_sample_params_none_fields_and_seed():
    geo_only = augment.AugmentPipe(xflip=1, scale=1)
    prm = geo_only.sample_params(3, 3, 8, 8, 'cpu')
    assert tuple(prm.G_inv.shape) == (3, 3, 3) and prm.C is None and prm.Hz_prime is None and prm.noise_sigma is None and prm.cutout_size is None and prm.cutout_center is None
    col_only = augment.AugmentPipe(brightness=1, hue=1)
    prm = col_only.sample_params(3, 3, 8, 8, 'cpu')
    assert prm.G_inv is None and tuple(prm.C.shape) == (3, 4, 4)
    noise_only = augment.AugmentPipe(noise=1)
    prm = noise_only.sample_params(3, 3, 8, 8, 'cpu')
    assert prm.G_inv is None and prm.C is None and tuple(prm.noise_sigma.shape) == (3, 1, 1, 1) and prm.cutout_size is None
    nothing = augment.AugmentPipe().sample_params(3, 3, 8, 8, 'cpu')
    assert all(v is None for v in vars(nothing).values())
    x = torch.randn(3, 3, 8, 8)
    assert augment.AugmentPipe()(x) is x
    full = augment.AugmentPipe(**R.BGC, imgfilter=1, noise=1, cutout=1)
    torch.manual_seed(7); a = full.sample_params(4, 3, 12, 10, 'cpu')
    torch.manual_seed(7); b = full.sample_params(4, 3, 12, 10, 'cpu')
    torch.manual_seed(8); c = full.sample_params(4, 3, 12, 10, 'cpu')
    for k in vars(a):
        assert torch.equal(getattr(a, k), getattr(b, k)), k
    assert not torch.equal(a.G_inv, c.G_inv)


def test_apply_twice_and_noise():
    full = augment.AugmentPipe(**R.BGC, imgfilter=1, noise=1, cutout=1)
    torch.manual_seed(3)
    x = torch.rand(2, 3, 24, 26) * 2 - 1
    prm = full.sample_params(2, 3, 24, 26, 'cpu')
    prm.noise_sigma = prm.noise_sigma + 0.05          # (so the stage shows for every sample)
    noise = torch.randn(2, 3, 24, 26)
    a, b = full.apply(x, prm, noise=noise), full.apply(x, prm, noise=noise)
    assert torch.equal(a, b)
    base = full.apply(x, prm, noise=torch.zeros_like(noise))
    keep = (base != 0) | (a != 0)
    cut = full.apply(torch.ones_like(x), augment.AugmentParams(cutout_size=prm.cutout_size, cutout_center=prm.cutout_center))
    want = base + noise * prm.noise_sigma * cut
    assert (a - want).abs().max() <= 4 * R.U * (base.abs() + (noise * prm.noise_sigma).abs()).max() and keep.any()
    torch.manual_seed(11); c = full.apply(x, prm)
    torch.manual_seed(11); d = full.apply(x, prm, noise=torch.randn(2, 3, 24, 26))
    assert torch.equal(c, d), 'noise=None draws the same normal tensor'


def test_mask_warp_matches_concatenation(pipe):
    torch.manual_seed(5)
    img, mask = torch.rand(2, 3, 17, 33), torch.rand(2, 19, 17, 33)
    prm = pipe.sample_params(2, 3, 17, 33, 'cpu')
    both = augment.geometric_transform(torch.cat([img, mask], dim=1), prm.G_inv, pipe.Hz_geom)
    assert torch.equal(augment.geometric_transform(mask, prm.G_inv, pipe.Hz_geom), both[:, 3:])
    assert torch.equal(augment.geometric_transform(img, prm.G_inv), both[:, :3]), 'sym6 is the default filter'
    out = pipe.apply(img, prm)
    assert torch.equal(out, augment.color_transform(both[:, :3], prm.C))


@pytest.mark.parametrize('shape', [(2, 3, 17, 33), (2, 1, 5, 7)])
def test_backward_is_the_transposed_map(pipe, shape):
    n, c, h, w = shape
    rng = np.random.RandomState(9)
    x = torch.from_numpy(rng.uniform(-1, 1, size=shape).astype(np.float32)).requires_grad_(True)
    wgt = rng.uniform(-1, 1, size=shape).astype(np.float32)
    Gs, Cs = zip(*[R.debug_matrices(p, c, h, w) for p in (0.3, 0.62)])
    G, C = np.stack(Gs), np.stack(Cs)
    prm = augment.AugmentParams(G_inv=torch.from_numpy(G.astype(np.float32)), C=torch.from_numpy(C.astype(np.float32)))
    (pipe.apply(x, prm) * torch.from_numpy(wgt)).sum().backward()
    G32, C32 = prm.G_inv.numpy().astype(np.float64), prm.C.numpy().astype(np.float64)
    geo = R.Geometry(G32, h, w, n_c=R.NC_KERNEL)
    assert R.margin_distance(geo.raw, h, w) >= R.MARGIN_CLEARANCE
    g, ga = R.color_transpose(wgt.astype(np.float64), C32)
    want, _, _ = geo.transpose(g)
    _, absval, ct = geo.transpose(ga)
    assert R.report('backward of the PyTorch definition', x.grad.numpy(), want, R.bound(absval, ct))


def test_refusals(pipe):
    G = torch.eye(3).expand(2, 3, 3)
    for bad in (torch.zeros(2, 3, 1, 8), torch.zeros(2, 3, 8, 1), torch.zeros(2, 3, 0, 8), torch.zeros(0, 3, 8, 8), torch.zeros(2, 0, 8, 8), torch.zeros(2, 3, 8),
                torch.zeros(2, 3, 8, 8, dtype=torch.int32), torch.zeros(2, 3, 2, augment.MAX_SIDE + 1)):
        with pytest.raises(ValueError):
            augment.geometric_transform(bad, torch.eye(3).expand(bad.shape[0], 3, 3))
    x = torch.zeros(2, 3, 8, 8)
    for bad_G in (torch.eye(3), torch.eye(3).expand(3, 3, 3), torch.eye(4).expand(2, 4, 4), torch.eye(3).expand(2, 3, 3).to(torch.int64)):
        with pytest.raises(ValueError):
            augment.geometric_transform(x, bad_G)
    with pytest.raises(ValueError):
        augment.geometric_transform(x, G, torch.ones(8))
    C = torch.eye(4).expand(2, 4, 4)
    with pytest.raises(ValueError, match='RGB'):
        augment.color_transform(torch.zeros(2, 2, 8, 8), C)
    with pytest.raises(ValueError):
        augment.color_transform(x, torch.eye(4))
    with pytest.raises(ValueError, match='RGB'):
        augment.AugmentPipe(brightness=1)(torch.zeros(2, 2, 8, 8))
    assert tuple(augment.color_transform(torch.zeros(2, 1, 8, 8), C).shape) == (2, 1, 8, 8)


def test_module_apply_still_reaches_children(pipe):
    """`AugmentPipe.apply(images, params)` shadows `torch.nn.Module.apply(fn)`: a callable alone is passed on."""
    parent = torch.nn.Sequential(augment.AugmentPipe(xflip=1), torch.nn.Linear(2, 2))
    seen = []
    parent.apply(lambda mod: seen.append(type(mod).__name__))
    assert len(seen) == 3 and any('AugmentPipe' in name for name in seen)
    with pytest.raises(TypeError):
        parent[0].apply(torch.zeros(1, 3, 4, 4))


def test_second_order_through_the_pytorch_definition(pipe):
    """The R1 penalty's path: a gradient taken with create_graph=True differentiates again.  d/dw of sum(v * grad_x sum(w * apply(x)))
    is the linear part of apply on v."""
    shape = (2, 3, 17, 33)
    n, c, h, w = shape
    rng = np.random.RandomState(12)
    Gs, Cs = zip(*[R.debug_matrices(p, c, h, w) for p in (0.3, 0.62)])
    G32, C32 = np.stack(Gs).astype(np.float32), np.stack(Cs).astype(np.float32)
    prm = augment.AugmentParams(G_inv=torch.from_numpy(G32), C=torch.from_numpy(C32))
    x = torch.from_numpy(rng.uniform(-1, 1, size=shape).astype(np.float32)).requires_grad_(True)
    wgt = torch.from_numpy(rng.uniform(-1, 1, size=shape).astype(np.float32)).requires_grad_(True)
    v = rng.uniform(-1, 1, size=shape).astype(np.float32)
    from torch_utils.ops import grid_sample_gradfix
    grid_sample_gradfix.enabled = True                     # as the reference's training loop sets it: ATen's own backward does not differentiate
    try:
        (g,) = torch.autograd.grad((pipe.apply(x, prm) * wgt).sum(), x, create_graph=True)
        assert g.requires_grad
        (gw,) = torch.autograd.grad((g * torch.from_numpy(v)).sum(), wgt)
    finally:
        grid_sample_gradfix.enabled = False
    geo = R.Geometry(G32.astype(np.float64), h, w, n_c=R.NC_KERNEL)
    want, absval, ct = R.color_linear(*geo.forward(v), C32.astype(np.float64))
    assert R.report('second order, PyTorch definition', gw.numpy(), want, R.bound(absval, ct))
