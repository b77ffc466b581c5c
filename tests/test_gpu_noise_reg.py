"""The projector's noise regulariser and noise normaliser as batched HIP launches (csrc/noise_reg.hip through training/projection.py, DESIGN.md
section 5.13) against the float64 restatement of tests/noise_ref.py.  `pytest -m gpu`.

Sizes: maps of side 4, 8, 8, 16, 32, 128 and 512 in one call (the duplicate side is deliberate) and each size alone: the one-level maps, the
first pooled level, a tile seam (128 = 2 x 2 tiles of 64) and the wrap at the largest size the kernels take."""

import pytest
import torch

import noise_ref

pytestmark = pytest.mark.gpu

DEV = torch.device('cuda', 0)
SIDES = (4, 8, 8, 16, 32, 128, 512)
SETS = {'all': SIDES, **{f'side{s}': (s,) for s in sorted(set(SIDES))}}
KERNEL_CALLS = ('noise_reg', 'noise_reg_backward', 'noise_normalize')

_cache = {}


def _calls():
    from torch_utils import hip_plugin
    return {k: hip_plugin.CALLS.get(k, 0) for k in KERNEL_CALLS}


def _maps(kind, sides):
    """CPU maps and their float64 loss and gradients: computed once per (kind, sides), shared, never modified."""
    key = (kind, tuple(sides))
    if key not in _cache:
        make = noise_ref.correlated if kind == 'correlated' else noise_ref.white
        maps = [make(s, 100 + 10 * i + s) for i, s in enumerate(sides)]
        _cache[key] = (maps, *noise_ref.reg64_with_grads(maps))
    return _cache[key]


def _device_run(maps, fn=None, upstream=None):
    """(loss, grads) of `fn` (default: projection.noise_regularization) on device copies of `maps`."""
    from training import projection
    leaves = [m.to(DEV).requires_grad_(True) for m in maps]
    loss = (fn or projection.noise_regularization)(leaves)
    (loss if upstream is None else upstream(loss, leaves)).backward()
    return loss.detach(), [t.grad for t in leaves]


def _loss_err(loss, want):
    return abs(float(loss.double().cpu()) - float(want)) / float(want)


def _grad_errs(grads, want):
    return [float((g.double().cpu() - w).abs().max()) / float(w.abs().max()) for g, w in zip(grads, want)]


@pytest.mark.parametrize('name', sorted(SETS))
def test_correlated_maps_against_float64(name):
    """Neighbouring pixels correlate (0.6 of the variance in each direction), so the level-0 means do not cancel and the fixed bound of the
    fixed-order fp32 sums holds: 1e-5 for the loss (relative) and for each map's gradient (of its float64 max-abs)."""
    sides = SETS[name]
    maps, want, want_g = _maps('correlated', sides)
    for m in maps:                                   # the premise, on the CPU: means of about 0.6 on the maps large enough to show it
        if m.shape[0] >= 128:
            a = m.double()
            assert abs(float((a * torch.roll(a, 1, 1)).mean()) - 0.6) < 0.1 and abs(float((a * torch.roll(a, 1, 0)).mean()) - 0.6) < 0.1
    before = _calls()
    loss, grads = _device_run(maps)
    after = _calls()
    assert after['noise_reg'] == before['noise_reg'] + 1 and after['noise_reg_backward'] == before['noise_reg_backward'] + 1
    e_loss, e_g = _loss_err(loss, want), _grad_errs(grads, want_g)
    print(f'{name}: loss {e_loss:.2e}  grads {max(e_g):.2e}')
    assert e_loss <= 1e-5
    assert max(e_g) <= 1e-5, e_g


def test_white_noise_maps_are_no_worse_than_twice_eager_fp32():
    """White noise: every mean cancels to about 1/R of its terms, so no fixed bound follows from the arithmetic.  The yardstick is the eager
    fp32 torch definition on the same device and maps: the kernels' error against float64 must be at most twice its error, for the loss and
    for the gradients (the largest per-map error as a fraction of that map's float64 max-abs)."""
    from training import projection
    maps, want, want_g = _maps('white', SIDES)
    loss_k, grads_k = _device_run(maps)
    loss_t, grads_t = _device_run(maps, fn=projection._noise_regularization_torch)
    ek, et = _loss_err(loss_k, want), _loss_err(loss_t, want)
    gk, gt = max(_grad_errs(grads_k, want_g)), max(_grad_errs(grads_t, want_g))
    print(f'white noise: loss error kernel {ek:.2e} eager {et:.2e}; gradient error kernel {gk:.2e} eager {gt:.2e}')
    assert ek <= 2 * et, f'loss: kernel {ek:.2e}, eager fp32 {et:.2e}'
    assert gk <= 2 * gt, f'gradients: kernel {gk:.2e}, eager fp32 {gt:.2e}'


def test_upstream_gradient_scales_exactly_and_stays_on_the_device():
    """loss * 1e5 + another differentiable term of the same maps: the regulariser's share of every gradient is exactly 1e5 times its
    gradient under an upstream of 1 (the kernel multiplies the finished value once), and the backward is one more launch of the entry
    point with the upstream scalar read on the device."""
    maps, _, _ = _maps('correlated', SIDES)
    _, g1 = _device_run(maps)
    before = _calls()
    _, g2 = _device_run(maps, upstream=lambda loss, leaves: loss * 1e5 + sum((t * 0.5).sum() for t in leaves))
    after = _calls()
    assert after['noise_reg_backward'] == before['noise_reg_backward'] + 1 and after['noise_reg'] == before['noise_reg'] + 1
    for a, b in zip(g1, g2):
        assert torch.equal(a * 1e5 + 0.5, b)


def test_two_calls_are_bit_identical():
    maps, _, _ = _maps('white', SIDES)
    l1, g1 = _device_run(maps)
    l2, g2 = _device_run(maps)
    assert torch.equal(l1, l2) and all(torch.equal(a, b) for a, b in zip(g1, g2))


def test_empty_list_gives_zero():
    from training import projection
    before = _calls()
    z = projection.noise_regularization([])
    assert z.ndim == 0 and float(z) == 0.0 and _calls() == before


def test_other_shapes_take_the_torch_definition():
    """12 x 12, 16 x 32 and a non-contiguous view are not the kernels' to take; a single one of them sends the whole call to torch."""
    g = torch.Generator().manual_seed(3)
    wide = torch.randn(16, 64, generator=g) + 0.3
    cases = {'12x12': [torch.randn(12, 12, generator=g) + 0.3], '16x32': [torch.randn(16, 32, generator=g) + 0.3],
             'view': [wide[:, ::4]], 'mixed': [torch.randn(16, 16, generator=g) + 0.3, torch.randn(12, 12, generator=g) + 0.3]}
    for name, maps in cases.items():
        want, want_g = noise_ref.reg64_with_grads(maps)
        leaves = [m.to(DEV) for m in maps]
        if name == 'view':
            leaves = [wide.to(DEV)[:, ::4]]
            assert not leaves[0].is_contiguous()
        leaves = [t.requires_grad_(True) if t.is_leaf else t.detach().requires_grad_(True) for t in leaves]
        before = _calls()
        from training import projection
        loss = projection.noise_regularization(leaves)
        loss.backward()
        assert _calls() == before, name
        assert _loss_err(loss.detach(), want) <= 1e-5, name
        assert max(_grad_errs([t.grad for t in leaves], want_g)) <= 1e-5, name


def test_switch_off_takes_the_torch_definition():
    from training import projection
    maps, want, want_g = _maps('correlated', (16, 32))
    projection.fused_noise_ops = False
    try:
        before = _calls()
        loss, grads = _device_run(maps)
        assert _calls() == before
    finally:
        projection.fused_noise_ops = True
    assert _loss_err(loss, want) <= 1e-5 and max(_grad_errs(grads, want_g)) <= 1e-5


# ---- normalize_noise_ ------------------------------------------------------------------------------------------------------------------

def _norm_inputs():
    """0.3 + 1.2 * white noise: a mean and a scale to remove.  |n| stays below 8, so one fp32 rounding is at most 2^-22 * 1/2 = 2.4e-7:
    the subtraction, the multiplication and the two coefficients (each correctly rounded from float64 sums) stay within 1e-6 together."""
    return [0.3 + 1.2 * noise_ref.white(s, 200 + i) for i, s in enumerate(SIDES)]


def test_normalize_against_float64():
    from training import projection
    maps = _norm_inputs()
    want = noise_ref.normalize64(maps)
    leaves = [m.to(DEV).requires_grad_(True) for m in maps]          # leaves that require grad, as in the projector
    versions = [t._version for t in leaves]
    before = _calls()
    with torch.no_grad():
        projection.normalize_noise_(leaves)
    assert _calls()['noise_normalize'] == before['noise_normalize'] + 1
    for t, v, w in zip(leaves, versions, want):
        assert t._version > v, 'the version counter did not advance'
        got = t.detach().double().cpu()
        assert float((got - w).abs().max()) <= 1e-6
        assert abs(float(got.mean())) <= 1e-6 and abs(float(got.square().mean()) - 1) <= 1e-6
    # the switch off: the torch definition, same result within the same bound
    again = [m.to(DEV).requires_grad_(True) for m in maps]
    projection.fused_noise_ops = False
    try:
        before = _calls()
        projection.normalize_noise_(again)
        assert _calls() == before
    finally:
        projection.fused_noise_ops = True
    for a, b, w in zip(again, leaves, want):
        assert float((a.detach() - b.detach()).abs().max()) <= 1e-6
        assert float((a.detach().double().cpu() - w).abs().max()) <= 1e-6


def test_normalize_binding_refuses_a_leaf_that_requires_grad_under_grad():
    from torch_utils import hip_plugin
    t = torch.randn(16, 16, device=DEV, requires_grad=True)
    with pytest.raises(RuntimeError):
        hip_plugin.NoisePlugin.noise_normalize([t])
    with torch.no_grad():
        hip_plugin.NoisePlugin.noise_normalize([t])
    assert t._version == 1


def test_normalized_maps_invalidate_the_scaled_noise_cache():
    """`_scaled_const_noise` caches noise_const * noise_strength per (tensor, version): after the raw-pointer update the product is new."""
    from training import networks, projection
    n = torch.randn(16, 16, device=DEV) + 2
    s = torch.full([], 0.5, device=DEV)
    with torch.no_grad():
        a = networks._scaled_const_noise(n, s).clone()
        projection.normalize_noise_([n])
        b = networks._scaled_const_noise(n, s)
    assert not torch.equal(a, b) and torch.equal(b, n * s)


# ---- project() ---------------------------------------------------------------------------------------------------------------------------

def test_project_tiny_generator():
    from training import projection, triplane
    torch.manual_seed(0)
    G = triplane.TriPlaneGenerator(triplane.tiny_spec()).eval().requires_grad_(False)
    with torch.no_grad():
        for name, p in G.synthesis.named_parameters():
            if name.endswith('noise_strength'):
                p.fill_(0.3)
    G = G.to(DEV)
    state = {k: v.detach().clone() for k, v in G.state_dict().items()}
    c = triplane.camera_label(0.2).to(DEV)
    with torch.no_grad():
        z = torch.randn(1, G.z_dim, generator=torch.Generator().manual_seed(1)).to(DEV)
        target = (G.synthesis(G.mapping(z, c), c=c, noise_mode='const')[0] + 1) * (255 / 2)
    before = _calls()
    w, info = projection.project(G, target, c, num_steps=8, w_avg_samples=256, return_info=True)
    after = _calls()
    assert after['noise_reg'] == before['noise_reg'] + 8 and after['noise_reg_backward'] == before['noise_reg_backward'] + 8
    assert after['noise_normalize'] == before['noise_normalize'] + 8
    assert tuple(w.shape) == (1, G.num_ws, G.w_dim)
    print('project: losses', [f'{v:.4g}' for v in info['losses']])
    assert info['losses'][-1] < info['losses'][0]
    for k, v in G.state_dict().items():
        assert torch.equal(v, state[k]), k
    assert not any(b.requires_grad for b in projection.noise_maps(G))
    for n in info['noise_maps']:
        a = n.double()
        assert abs(float(a.mean())) <= 1e-5 and abs(float(a.square().mean()) - 1) <= 1e-5
