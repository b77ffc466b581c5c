"""`mapping_kernel` / `mapping_layer_kernel` (csrc/mapping.hip) at their edges against the float64 definition, one layer at a time.
Needs a real MI355X: `pytest -m gpu`.

The cases, the route each is built for and the telescoped run are in tests/mapping_cases.py; the reference and the derivation of every
bound constant in tests/mapping_ref.py (one layer: 24 u of gain * (wg * sum |x W| + bg * |b|); input stage: 12 u relative for z, (c_dim + 3) u
of the embedding's magnitude carried through its normalisation; truncation: 4 u).  tests/test_mapping_style_ref_cpu.py shows on the CPU that
a correct implementation with the kernels' summation order stays inside these bounds and that a dropped tail slab, a bias row off by one, a
skipped lane and a wrong image clamp leave them by more than 100 x.

Which route a layer takes (`one_block` or `gemv_rows`, idle workgroups, an odd number of rows per workgroup) cannot be seen from a result; the
case table restates the kernel's conditions and the CPU test asserts them.  Which FORM a process took cannot be seen either: `ide3d_mapping`
launches the one-launch kernel where `mapping_resident()` finds its 64 workgroups co-resident with a 2 x margin.  From the code, a 256-CU
MI355X with at least one resident 256-thread, 32.5 KB-LDS workgroup per CU gives 256 >= 128: the one-launch form is what the default process
runs there, and IDE3D_MAPPING_PER_LAYER=1 (read once per process) selects the other.  Both forms run every case in a child process of
their own and must agree bit for bit.

Every test prints its worst error / bound and checks `hip_plugin.CALLS` for the native call.
"""

import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import mapping_cases
import mapping_ref
from util import assert_close

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD_TIMEOUT = 240         # seconds per child process: import, library load and ~60 small launches take ~15 s


def _calls():
    from torch_utils import hip_plugin
    return hip_plugin.CALLS.get('mapping', 0)


@pytest.mark.parametrize('name', [c['name'] for c in mapping_cases.CASES])
def test_every_layer_within_its_one_layer_bound(gpu_device, name):
    c = mapping_cases.BY_NAME[name]
    before = _calls()
    with torch.no_grad():
        acts = mapping_cases.run(c, gpu_device)
    assert _calls() == before + len(c['widths'])
    ratios = mapping_cases.check(c, acts)
    print(f'mapping {name}: worst error / bound per layer {[round(r, 3) for r in ratios]}')
    assert max(ratios) <= 1.0, f'case {name}: {max(ratios):.3f} x the bound at layer {int(np.argmax(ratios))}'


def test_full_launch_equals_the_telescoped_last_activation(gpu_device):
    """The premise of the telescoped check: x_l of a deeper launch has the bits of the l-layer launch.  The L-layer launch with num_ws > 1
    broadcasts exactly the telescoped x_L to every row."""
    for name in ('b', 'd', 'i'):
        c = mapping_cases.BY_NAME[name]
        td = mapping_cases.to_device(mapping_cases.tensors(c), gpu_device)
        with torch.no_grad():
            x_last = mapping_cases.launch(td)[:, 0]
            again = mapping_cases.launch(td)[:, 0]
            ws = mapping_cases.launch(td, num_ws=5)
        assert torch.equal(x_last, again), f'case {name}: two launches of one shape differ'
        assert torch.equal(ws, x_last[:, None, :].expand(-1, 5, -1)), f'case {name}: the broadcast rows are not copies'


@pytest.mark.parametrize('num_ws', [1, 18])
def test_truncation_and_broadcast(gpu_device, num_ws):
    c = mapping_cases.BY_NAME['b']
    t = mapping_cases.tensors(c)
    td = mapping_cases.to_device(t, gpu_device)
    worst, before, runs = 0.0, _calls(), 0
    with torch.no_grad():
        x_last = mapping_cases.launch(td)[:, 0].cpu().numpy()
        for psi in (1, 0.7, 0.5, mapping_cases.PSI_BELOW_HALF, 0.3, 0, -0.5, 1.5):
            for cutoff in (None, 0, 1, num_ws - 1, num_ws, num_ws + 3):
                got = mapping_cases.launch(td, num_ws=num_ws, psi=psi, cutoff=cutoff, w_avg=td['w_avg']).cpu().numpy()
                runs += 1
                worst = max(worst, mapping_cases.check_truncation(x_last, t['w_avg'], got, num_ws, psi, cutoff))
    assert _calls() == before + 1 + runs
    print(f'mapping truncation num_ws {num_ws}: worst error / bound {worst:.3f} over {runs} (psi, cut-off) pairs')
    assert worst <= 1.0


def test_negative_cutoff_is_a_slice_at_plugin_level(gpu_device):
    """`MappingPlugin.mapping` gives a negative cut-off the meaning of `ws[:, :cutoff]`."""
    c = mapping_cases.BY_NAME['b']
    t = mapping_cases.tensors(c)
    td = mapping_cases.to_device(t, gpu_device)
    with torch.no_grad():
        x_last = mapping_cases.launch(td)[:, 0].cpu().numpy()
        for num_ws in (1, 18):
            for cutoff in (-1, -2, -num_ws + 1, -num_ws, -num_ws - 3):
                got = mapping_cases.launch(td, num_ws=num_ws, psi=0.7, cutoff=cutoff, w_avg=td['w_avg']).cpu().numpy()
                assert mapping_cases.check_truncation(x_last, t['w_avg'], got, num_ws, 0.7, cutoff) <= 1.0
                k = mapping_ref.slice_cutoff(cutoff, num_ws)
                assert all(not np.array_equal(got[:, j], x_last) for j in range(k)), f'cut-off {cutoff}: a row inside the slice was not truncated'


@pytest.mark.parametrize('cutoff', [-1, -11, -12, -15])
def test_module_negative_cutoff_truncates_the_rows_of_the_slice(gpu_device, cutoff):
    """`MappingNetwork.forward(truncation_cutoff=k)` with k < 0 on the GPU == the CPU module (whose `ws[:, :k]` is a Python slice), and the
    truncated rows are exactly those of the slice: the others carry the bits of the psi = 1 result."""
    from training import networks
    torch.manual_seed(3)
    M = networks.MappingNetwork(32, 25, 32, 12, num_layers=2).eval()
    with torch.no_grad():
        M.w_avg.copy_(torch.randn(32) * 0.3)
    Mg = networks.MappingNetwork(32, 25, 32, 12, num_layers=2).eval()
    Mg.load_state_dict(M.state_dict()); Mg = Mg.to(gpu_device)
    g = torch.Generator().manual_seed(4)
    z, c = torch.randn(3, 32, generator=g), torch.randn(3, 25, generator=g)
    before = _calls()
    with torch.no_grad():
        got = Mg(z.to(gpu_device), c.to(gpu_device), truncation_psi=0.7, truncation_cutoff=cutoff).cpu()
        plain = Mg(z.to(gpu_device), c.to(gpu_device)).cpu()
        want = M(z, c, truncation_psi=0.7, truncation_cutoff=cutoff)
    assert _calls() == before + 2, 'the fused mapping kernel must have run'
    inside = torch.zeros(12, dtype=torch.bool)
    inside[:cutoff] = True
    truncated = torch.tensor([not torch.equal(got[:, j], plain[:, j]) for j in range(12)])
    assert torch.equal(truncated, inside), f'cut-off {cutoff}: truncated rows {truncated.nonzero().flatten().tolist()}, the slice is {inside.nonzero().flatten().tolist()}'
    assert_close(got, want, rtol=1e-4, atol=1e-5, what=f'module, cut-off {cutoff}')


def test_narrow_launch_after_a_wide_one_on_one_workspace(gpu_device):
    """Case e (1024 wide, 8 images) and then case a (4 wide, 1 image) on the same cached workspace: the stale wider activations must not
    reach the narrow launch."""
    a, e = mapping_cases.BY_NAME['a'], mapping_cases.BY_NAME['e8']
    with torch.no_grad():
        first = mapping_cases.run(a, gpu_device)
        mapping_cases.run(e, gpu_device)
        after = mapping_cases.run(a, gpu_device)
    assert all(np.array_equal(x, y) for x, y in zip(first, after))
    assert max(mapping_cases.check(a, after)) <= 1.0


# ---- both forms of the entry point, a fresh process each ---------------------------------------------------------------------------------

@pytest.fixture(scope='module')
def forms(gpu_device, tmp_path_factory):
    """{'one_launch' | 'per_layer': results of `python tests/mapping_cases.py`} - the default form and IDE3D_MAPPING_PER_LAYER=1.  A child that
    fails or runs out of time raises here, and nothing further is started."""
    out = {}
    tmp = tmp_path_factory.mktemp('mapping_forms')
    for form, flag in (('one_launch', None), ('per_layer', '1')):
        env = dict(os.environ)
        env.pop('IDE3D_MAPPING_PER_LAYER', None)
        if flag:
            env['IDE3D_MAPPING_PER_LAYER'] = flag
        path = str(tmp / f'{form}.npz')
        subprocess.run([sys.executable, os.path.join(ROOT, 'tests', 'mapping_cases.py'), path], check=True, env=env, timeout=CHILD_TIMEOUT)
        with np.load(path) as d:
            out[form] = {k: d[k] for k in d.files}
    return out


def test_per_layer_form_is_bit_equal_and_both_are_within_the_bounds(forms):
    one, per = forms['one_launch'], forms['per_layer']
    assert sorted(one) == sorted(per) and len(one) == sum(len(c['widths']) for c in mapping_cases.CASES) + len(mapping_cases.TRUNC_COMBOS)
    for key in one:
        assert np.array_equal(one[key], per[key]), f'{key}: the per-layer form differs from the one-launch form'
    for form, res in forms.items():
        worst = mapping_cases.check_all(res)
        print(f'mapping {form}: worst error / bound per case {({k: round(v, 3) for k, v in worst.items()})}')
        assert max(worst.values()) <= 1.0, (form, worst)


def test_narrow_case_is_what_a_fresh_process_computes(gpu_device, forms):
    """Case a in this process - after every wider case of this module has used the workspace, and once more right after case e - has the
    bits of case a run FIRST in a fresh process (the children run it before any other launch)."""
    a, e = mapping_cases.BY_NAME['a'], mapping_cases.BY_NAME['e8']
    with torch.no_grad():
        mapping_cases.run(e, gpu_device)
        here = mapping_cases.run(a, gpu_device)
    assert mapping_cases.CASES[0] is a
    assert np.array_equal(here[0], forms['one_launch']['a/0'])


# ---- refusals ----------------------------------------------------------------------------------------------------------------------------

def _refused(td, **kw):
    before = _calls()
    with pytest.raises(RuntimeError):
        mapping_cases.launch(td, **kw)
    assert _calls() == before, 'a refused call must not count as a launch'


def test_refusals_raise_and_launch_nothing(gpu_device):
    dev = gpu_device
    mk = lambda n, widths, z_dim=8: mapping_cases.to_device(mapping_cases.tensors(mapping_cases.case('r', n, z_dim, 0, 0, widths)), dev)
    _refused(mk(9, [8]))                                                     # n = 9
    _refused(mk(1, [1028]))                                                  # a width of 1028
    _refused(mk(1, [6]))                                                     # a width of 6
    _refused(mk(1, [8] * 17))                                                # 17 layers
    td = mapping_cases.to_device(mapping_cases.tensors(mapping_cases.BY_NAME['g2']), dev)
    td['c'] = td['c'][:1].contiguous()
    _refused(td)                                                             # c with the wrong batch
    td = mk(2, [8, 12])
    _refused(td, num_ws=3, psi=0.7, w_avg=td['w_avg'][:-1].contiguous())     # w_avg one element short
    _refused(td, num_ws=3, psi=0.7, w_avg=None)                              # truncation without w_avg
    td['fc_w'][1] = torch.randn(12, 12, device=dev)
    _refused(td)                                                             # widths that do not chain
    ok = mk(2, [8, 12])
    before = _calls()
    mapping_cases.launch(ok)
    assert _calls() == before + 1
