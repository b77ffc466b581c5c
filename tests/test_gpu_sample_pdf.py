"""`ide3d_sample_pdf` (csrc/sample_pdf.hip) on the boundaries of its lane runs and of its grid-stride loop, and on draws placed on the edges
of the sampled function, against float64 (tests/pdf_ref.py; the table's margins are checked without a GPU in
tests/test_composite_cases_cpu.py).  Needs an MI355X.

On the table every element is held to both checks, none left out: the project's cdf property |cdf64(sample) - u| <= 2e-5 + steepest * 5e-7,
and 5e-6 against the float32 definition `oracle_ops.sample_pdf` (which the CPU test ties to the float64 inverse cdf within the same 5e-6)."""

import pytest
import torch

import pdf_ref
from oracle import ops as oracle_ops

pytestmark = pytest.mark.gpu


def _calls():
    from torch_utils import hip_plugin
    return hip_plugin.CALLS.get('sample_pdf', 0)


def _sample(bins, w, u, dev):
    from training import volumetric_rendering as vr
    before = _calls()
    got = vr.sample_pdf(bins.to(dev), w.to(dev), u.shape[-1], u=u.to(dev))
    assert _calls() == before + 1
    assert got.shape == (w.shape[0], u.shape[-1]) and got.dtype == torch.float32
    return got.cpu()


@pytest.mark.parametrize('case', pdf_ref.CASES, ids=[c.name for c in pdf_ref.CASES])
def test_table_against_float64_everywhere(gpu_device, case):
    bins, w, u = case.inputs()
    got = _sample(bins, w, u, gpu_device)
    ue = pdf_ref.expand(u, case.rays)
    f, tol = pdf_ref.cdf_at(bins, w, got)
    dev_cdf = (f - ue.double()).abs()
    want = oracle_ops.sample_pdf(bins, w, ue)
    err = (got - want).abs()
    print(f'{case.name}: worst cdf deviation / tolerance {float((dev_cdf / tol).max()):.3f}, worst distance to the float32 definition {float(err.max()):.3e}, '
          f'to the float64 inverse cdf {float((got.double() - pdf_ref.inverse_cdf64(bins, w, u)).abs().max()):.3e}')
    assert bool((dev_cdf <= tol).all()), f'cdf(sample) != u at {int((dev_cdf > tol).sum())} of {got.numel()} elements'
    assert bool((err <= 5e-6).all()), f'{int((err > 5e-6).sum())} of {got.numel()} elements differ from the definition, worst {float(err.max()):.3e}'
    assert bool((got >= bins[:, :1]).all() and (got <= bins[:, -1:]).all())
    if case.rays > 8192:          # the rays of the second grid-stride trip, by themselves: they are the last three
        assert bool((err[8192:] <= 5e-6).all()) and bool((dev_cdf[8192:] <= tol[8192:]).all())


def test_sorted_draws_give_sorted_samples(gpu_device):
    for case in pdf_ref.CASES:
        if case.rays > 8192 or case.n < 7:
            continue
        bins, w, u = case.inputs()
        got = _sample(bins, w, torch.sort(u, -1)[0], gpu_device)
        assert bool((got[:, 1:] >= got[:, :-1]).all()), case.name          # away from the knots not even rounding can swap two samples


def test_placed_draws(gpu_device):
    """Draws at 0, at 1, outside [0, 1], on cdf knots and inside runs of zero-weight bins (pdf_ref.placed_case), where two correct
    evaluations may take different bins or branches: the properties that hold on either."""
    bins, w, u = pdf_ref.placed_case()
    k = w.shape[1]
    assert bool((u[:, 1:] >= u[:, :-1]).all()) and bool((w[0] == 0).all()) and bool((w[1, 40:50] == 0).all())
    got = _sample(bins, w, u, gpu_device)
    # a float32 ulp of the depth (2.4e-7 at 3.3) on either side: t * (b1 - b0) is rounded twice on the way to b1
    slack = 5e-7
    assert bool((got >= bins[:, :1] - slack).all() and (got <= bins[:, -1:] + slack).all()), 'samples stay inside [bins[0], bins[k]]'
    lo, hi = u <= 0, u > 1 + 1e-6
    assert int(lo.sum()) == 2 * w.shape[0] and int(hi.sum()) == w.shape[0]
    assert torch.equal(got[lo], bins[:, :1].expand_as(got)[lo]), 'u <= 0 gives bins[0] exactly'
    assert torch.equal(got[hi], bins[:, k:].expand_as(got)[hi]), 'u > cdf[k] gives bins[k] exactly'
    # cdf(sample) = u for the draws clamped to the cdf's range; the tolerance already holds the mass eps of a bin on the `denom -> 1` branch
    f, tol = pdf_ref.cdf_at(bins, w, got.clamp(bins[:, :1], bins[:, -1:]))
    dev_cdf = (f - u.double().clamp(0, 1)).abs()
    print(f'placed draws: worst cdf deviation / tolerance {float((dev_cdf / tol).max()):.3f}')
    assert bool((dev_cdf <= tol).all()), f'cdf(sample) != u at {(dev_cdf > tol).nonzero().tolist()}'
    assert bool((got[:, 1:] >= got[:, :-1] - slack).all()), 'sorted draws give sorted samples'
    # the same edges as draws shared by all rays
    us = torch.tensor([-0.5, 0.0, 0.25, 0.5, 1.0, 1.5])
    gs = _sample(bins, w, us, gpu_device)
    assert torch.equal(gs[:, :2], bins[:, :1].expand(-1, 2)) and torch.equal(gs[:, 5], bins[:, k])
    f, tol = pdf_ref.cdf_at(bins, w, gs.clamp(bins[:, :1], bins[:, -1:]))
    assert bool(((f - us.double().clamp(0, 1)[None]).abs() <= tol).all())
    assert bool((gs[:, 1:] >= gs[:, :-1] - slack).all())
