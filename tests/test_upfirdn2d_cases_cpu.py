"""The upfirdn2d case table (tests/upfirdn2d_cases.py) without a GPU: which of the thirteen launchable forms of csrc/upfirdn2d.hip every case
takes, through the host-only query `ide3d_upfirdn2d_plan` (the launch goes through the same function, the tile kernel through the same
staging predicate); that the table reaches every form, every tile instance with both staging paths, and both sides of every condition of
`fir44_applies`, `fir_up2_applies` and `cell_applies`; and that its two references stand: the float64 tap loop of oracle/ops.py equals
the tensor definition `_upfirdn2d_ref` in float64, and the float32 definition stays inside the bound the GPU suite uses, so that suite
measures the kernel and not the table."""
import ctypes
import os
import re

import pytest
import torch

import upfirdn2d_cases as uc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

LEAN_CONDITIONS = {
    # condition of fir44_applies reachable with a tensor -> the case fields that may differ between the two cases of its pair
    'fir44': {'dtype': {'dtype'}, 'x_stride[3] != 1': {'layout'}, 'add': {'epi'}, 'out_w <= 64': {'shape'}, 'out_w % 4': {'shape'}, 'pitch % 4': {'layout'},
              'x_row_floats': {'layout'}, 'x alignment': {'layout'}, 'x plane stride % 4': {'layout'}, 'noise alignment': {'epi'}},
    'fir_up2': {'dtype': {'dtype'}, 'x_stride[3] != 1': {'layout'}, 'out_w % 4': {'pad'}, 'in_w % 4': {'shape'}, 'pad_x0 odd': {'pad'}, 'pitch % 4': {'layout'},
                'x alignment': {'layout'}, 'x plane stride % 4': {'layout'}, 'add_stride[3] != 1': {'epi'}, 'add alignment': {'epi'}, 'add plane stride % 4': {'epi'},
                'add pitch % 4': {'epi'}, 'noise alignment': {'epi'}},
    'cell': {'up_x != up_y': {'up'}, 'up not 2 or 4': {'up'}, 'down != 1': {'down'}, 'y_amax': {'epi'}, 'taps < 36': {'filt', 'pad'}, 'LDS': {'filt', 'pad'}},
}


def _hp():
    from torch_utils import hip_plugin
    return hip_plugin


def _plan_of(case, ts=None):
    ts = ts or case.tensors()
    return _hp().upfirdn2d_plan(ts['x'], tuple(ts['f'].shape), *case.call_args(), **case.plan_kwargs(ts))


def _stated(p):
    return dict(form=p['form'], instance=p['instance'], staging=p['staging'], cell_u=p['cell_u'], c_fastest=p['c_fastest'], tiles=(p['tiles_x'], p['tiles_y']))


def _spec(shape, stride=None, dtype=torch.float32, align=0, row_floats=0):
    n, c, h, w = shape
    return dict(shape=shape, stride=stride or (c * h * w, h * w, w, 1), dtype=dtype, align=align, row_floats=row_floats)


def test_upfirdn2d_plan_abi_cpu():
    """Declared in the header, listed, exported, mirrored field for field, and outside the launch counters."""
    hp = _hp()
    src = open(os.path.join(ROOT, 'include', 'ide3d_hip.h')).read()
    assert re.search(r'\bint ide3d_upfirdn2d_plan\(const ide3d_upfirdn2d_params\* p, const ide3d_upfirdn2d_epilogue\* ep, ide3d_upfirdn2d_plan_info\* out\);', src)
    body = re.search(r'typedef struct ide3d_upfirdn2d_plan_info \{(.*?)\} ide3d_upfirdn2d_plan_info;', src, re.S).group(1)
    body = re.sub(r'/\*.*?\*/', '', body, flags=re.S)
    ctype = {'int32_t': ctypes.c_int32, 'int64_t': ctypes.c_int64}
    fields = [(name.strip(), ctype[m.group(1)]) for m in re.finditer(r'(int32_t|int64_t)\s+([\w\s,]+);', body) for name in m.group(2).split(',')]
    assert fields == list(hp._UpfirdnPlanInfo._fields_)
    enum = re.findall(r'IDE3D_UPFIRDN_([A-Z0-9_]+) = (\d)', src)
    assert [(n.lower(), int(v)) for n, v in enum] == list(zip(hp.UPFIRDN_FORMS, range(5)))
    assert 'ide3d_upfirdn2d_plan' in hp.EXPORTED_SYMBOLS
    assert hasattr(ctypes.CDLL(hp.lib_path()), 'ide3d_upfirdn2d_plan')
    assert hp._ABI_VERSION == 8
    hp.CALLS.clear()
    hp.upfirdn2d_plan(torch.zeros(1, 2, 5, 6), (4, 4), padx0=1, padx1=1, pady0=1, pady1=1)
    assert not hp.CALLS, 'a plan query is not a launch'


def test_every_case_takes_the_form_instance_and_staging_the_table_states():
    for c in uc.CASES:
        ts = c.tensors()
        x = ts['x']
        st, off, numel = uc.layout_of(c.layout, c.shape)
        assert tuple(x.stride()) == st and x.storage_offset() == off and x.untyped_storage().nbytes() == numel * x.element_size(), c.name
        assert x.untyped_storage().data_ptr() % 16 == 0 and torch.equal(x.contiguous(), c.values('x')), c.name          # the view keeps the alignment it claims
        assert _stated(_plan_of(c, ts)) == c.stated_plan(), (c.name, c.why, _plan_of(c, ts))
        # the same plan from the shape, strides and alignment alone
        e = c.epi
        add = None if ts['add'] is None else dict(shape=tuple(ts['add'].shape), stride=ts['add'].stride(), dtype=ts['add'].dtype, align=ts['add'].data_ptr() % 16)
        spec = dict(shape=c.shape, stride=st, dtype=c.torch_dtype, align=off * x.element_size() % 16, row_floats=_hp()._row_floats_readable(x))
        kw = dict(c.plan_kwargs(ts), add=add, noise=None if 'noise' not in e else e['noise'] * 4 % 16)
        assert _hp().upfirdn2d_plan(spec, tuple(ts['f'].shape), *c.call_args(), **kw) == _plan_of(c, ts), c.name
        assert c.out_shape[2] * c.out_shape[3] * c.shape[0] * c.shape[1] <= 1100000, c.name          # the table stays small


def test_every_form_instance_and_staging_is_reached():
    assert {c.form for c in uc.CASES} == {'generic', 'cell', 'tile', 'fir44', 'fir_up2'}
    assert {c.cell_u for c in uc.CELL_CASES} == {2, 4}
    assert {c.c_fastest for c in uc.CASES if c.form == 'generic'} == {0, 1}
    tiled = {}
    for c in uc.CASES:
        if c.form in ('tile', 'fir44', 'fir_up2'):
            tiled.setdefault((c.form, c.instance), []).append(c)
    assert set(tiled) == {('tile', i) for i in uc.TILE_INSTANCES} | {('fir44', uc.T128), ('fir_up2', uc.TUP2)}
    for (form, inst), cases in tiled.items():
        if form == 'tile':          # every instance holds few enough 16-byte loads to stage that way: both paths exist for all ten
            assert {c.staging for c in cases if c.dtype == 'f32'} >= {0, 1}, inst
        else:
            assert {c.staging for c in cases} == {1}
        # one and at least two tiles per axis (the 64-wide instance exists for out_w <= 64: one tile column by definition)
        assert any(c.tiles[0] == 1 for c in cases) and (inst == uc.T64 or any(c.tiles[0] >= 2 for c in cases)), (form, inst)
        assert any(c.tiles[1] == 1 for c in cases) and any(c.tiles[1] >= 2 for c in cases), (form, inst)
        # xcd_remap off and on the multiples of 8
        grids = {c.tiles[0] * c.tiles[1] * c.shape[0] * c.shape[1] for c in cases}
        assert grids >= {7, 8, 9, 13}, (form, inst)
    # mixed staging is pinned, not spread: the two cases whose only difference from a lean case is the plane stride (plane 0 aligned, plane 1 not)
    assert {c.name for c in uc.CASES if c.staging == 2} == {'t128_planes_off', 'tup2_planes_off'}
    # the storage types: fp16 and bf16 through every form that takes them, float64 through the generic kernel
    for dt in ('f16', 'bf16'):
        assert {(c.form, c.instance) for c in uc.CASES if c.dtype == dt} >= {('tile', uc.T64), ('tile', uc.T128), ('tile', uc.TUP2), ('tile', uc.TDN2), ('cell', None), ('generic', None)}, dt
    assert {c.form for c in uc.CASES if c.dtype == 'f64'} == {'generic'}
    # the grid-stride loops take a second trip
    assert any(c.form == 'generic' and c.shape[0] * c.shape[1] * c.out_shape[2] * c.out_shape[3] > 2048 * 256 for c in uc.CASES)
    assert any(c.form == 'cell' and c.shape[0] * c.shape[1] * c.tiles[1] * c.cell_u * c.tiles[0] > 2048 * 256 for c in uc.CASES)
    # y_amax after every form that accepts it; the generic form on both sides of its 64-image LDS path
    am = {(c.form, c.instance) for c in uc.AMAX_CASES}
    assert am >= {('generic', None), ('tile', uc.T64), ('tile', uc.T128), ('tile', uc.TUP2), ('fir44', uc.T128), ('fir_up2', uc.TUP2)}
    assert {c.shape[0] for c in uc.AMAX_CASES if c.form == 'generic'} >= {64, 65}
    # epilogues: the tile forms with 16-byte and scalar add / noise rows, the cell and generic forms with the scalar apply_epilogue
    for form in ('generic', 'cell', 'tile', 'fir44', 'fir_up2'):
        keys = set().union(*(set(c.epi) for c in uc.CASES if c.form == form))
        assert keys >= ({'noise', 'bias', 'act'} if form == 'fir44' else {'add', 'noise', 'bias', 'act'}), form
    alphas = {(c.form, c.epi.get('alpha')) for c in uc.CASES if c.epi.get('act') == 3}
    assert alphas >= {(f, a) for f in ('fir44',) for a in (0.0, 0.2, 1.0, 1.5, -0.2)} and ('fir_up2', 1.5) in alphas and ('fir_up2', 0.2) in alphas
    assert {bool(c.epi.get('clamp', -1) >= 0) for c in uc.CASES if c.form == 'fir44' and 'act' in c.epi} == {True, False}


def test_every_dispatch_condition_is_hit_on_both_sides_by_a_pair_that_differs_in_it_alone():
    seen = {k: set() for k in LEAN_CONDITIONS}
    for c in uc.CASES:
        if c.vs is None:
            continue
        other, cond = uc.BY_NAME[c.vs[0]], c.vs[1]
        assert c.form != other.form, c.name
        a, b = c.fields(), other.fields()
        diff = {k for k in a if a[k] != b[k]}
        if other.form in LEAN_CONDITIONS:
            assert cond in LEAN_CONDITIONS[other.form], (c.name, cond)
            assert diff and diff <= LEAN_CONDITIONS[other.form][cond], (c.name, cond, diff)
            seen[other.form].add(cond)
            # a case the lean kernel declines runs the tile instance it reproduces, unless the condition takes it out of the tiled forms
            if other.form in ('fir44', 'fir_up2') and cond not in ('x_stride[3] != 1', 'out_w <= 64'):
                assert c.form == 'tile' and c.instance == other.instance, c.name
        else:
            assert diff == {'dtype'} and cond == 'dtype' and c.form == 'generic', c.name          # the 12-tap instances are fp32 only
    for form, conds in LEAN_CONDITIONS.items():
        assert seen[form] == set(conds), (form, set(conds) - seen[form])
    assert any(c.vs and uc.BY_NAME[c.vs[0]].instance == uc.X_UP for c in uc.CASES) and any(c.vs and uc.BY_NAME[c.vs[0]].instance == uc.Y_UP for c in uc.CASES)


def test_conditions_no_tensor_of_the_table_reaches(monkeypatch):
    """The knobs, overlapping rows and the 2^31-byte plane limits of the lean kernels; the x-stride limit of the cell kernel."""
    hp = _hp()
    base44 = lambda **kw: hp.upfirdn2d_plan(_spec((1, 2, 32, 128), **kw), (4, 4), 1, 1, 1, 1, 2, 1, 2, 1)['form']
    base_up2 = lambda **kw: hp.upfirdn2d_plan(_spec((1, 2, 8, 8), **kw), (4, 4), 2, 2, 1, 1, 2, 1, 2, 1)['form']
    cell = lambda: hp.upfirdn2d_plan(_spec((1, 2, 8, 8)), (6, 6), 2, 2, 1, 1, 3, 2, 3, 2)['form']
    assert (base44(), base_up2(), cell()) == ('fir44', 'fir_up2', 'cell')
    monkeypatch.setenv('IDE3D_FIR_NO_LEAN', '1')
    assert (base44(), base_up2(), cell()) == ('tile', 'tile', 'cell')
    monkeypatch.delenv('IDE3D_FIR_NO_LEAN')
    monkeypatch.setenv('IDE3D_FIR_NO_CELL', '1')
    assert (base44(), base_up2(), cell()) == ('fir44', 'fir_up2', 'generic')
    monkeypatch.delenv('IDE3D_FIR_NO_CELL')
    # rows that overlap (pitch < round_up(in_w, 4)) and rows of pitch 0
    assert base44(stride=(32 * 64, 32 * 64, 64, 1)) == 'tile' and base44(stride=(128, 128, 0, 1)) == 'tile'
    assert base_up2(stride=(32, 32, 4, 1)) == 'tile' and base_up2(stride=(8, 8, 0, 1)) == 'tile'
    # planes of 2^31 bytes
    for shape, lean in (((1, 1, 2 ** 14, 2 ** 15 - 4), 'fir44'), ((1, 1, 2 ** 14, 2 ** 15), 'tile')):
        assert hp.upfirdn2d_plan(_spec(shape), (4, 4), 1, 1, 1, 1, 2, 1, 2, 1)['form'] == lean
    for shape, lean in (((1, 1, 2 ** 13, 2 ** 14 - 4), 'fir_up2'), ((1, 1, 2 ** 13, 2 ** 14), 'tile')):          # the output plane has four times the elements
        assert hp.upfirdn2d_plan(_spec(shape), (4, 4), 2, 2, 1, 1, 2, 1, 2, 1)['form'] == lean
    # x_stride[3] * in_w at 2^31 elements
    for k, form in ((2 ** 27 - 1, 'cell'), (2 ** 27, 'generic')):
        assert hp.upfirdn2d_plan(_spec((1, 1, 2, 16), stride=(2 ** 32, 2 ** 32, 2 ** 31, k)), (6, 6), 2, 2, 1, 1, 3, 2, 3, 2)['form'] == form


def test_the_tile_kernel_and_the_plan_share_one_staging_predicate():
    """The staging choice is made on the device; the plan reports it.  Both call tile_stage16_instance / tile_stage16_plane, and neither
    spells the conditions out again (the two stagings are bit-equal by design, so no output could show a drift)."""
    src = open(os.path.join(ROOT, 'ide-3d_amd', 'csrc', 'upfirdn2d.hip')).read()
    src = re.sub(r'//[^\n]*', '', src)
    kernel = src[src.index('upfirdn2d_tile_kernel(ide3d_upfirdn2d_params p'):src.index('fir44_kernel(ide3d_upfirdn2d_params p')]
    host = src[src.index('static int tile_staging('):src.index('static int upfirdn2d_plan(')]
    for part in (kernel, host):
        assert part.count('tile_stage16_plane(') == 1 and part.count('tile_stage16_instance(') == 1
        assert part.count('x_row_floats') == 1 and '& 15' not in part.replace('reinterpret_cast<uintptr_t>(yr + ox0) & 15', '')
    assert re.search(r'tile_stage16_plane\(pitch, p\.in_w, p\.x_row_floats, reinterpret_cast<uintptr_t>\(xp\)\)', kernel)
    assert re.search(r'tile_stage16_plane\(p\.x_stride\[2\], p\.in_w, p\.x_row_floats,\s*reinterpret_cast<uintptr_t>\(p\.x\) \+', host)
    assert 'tile_stage16_instance((int)sizeof(T), G::NLD4)' in kernel and 'tile_stage16_instance(4, G::NLD4)' in host


def test_plan_reports_the_launch_geometry():
    hp = _hp()
    # the 513 -> 512 FIR behind the generator's last transposed convolution: rows of 513 floats in a pitch of 516, noise + bias + lrelu
    x = _spec((4, 64, 513, 513), stride=(64 * 513 * 516, 513 * 516, 516, 1), row_floats=516)
    p = hp.upfirdn2d_plan(x, (4, 4), 1, 1, 1, 1, 1, 1, 1, 1, False, 4.0, noise=True, bias=True, act=3, alpha=0.2, act_gain=2 ** 0.5, y_amax=True)
    assert p == dict(form='fir44', instance=uc.T128, cell_u=0, staging=1, c_fastest=0, tiles_x=4, tiles_y=16, grid=4 * 64 * 64, lds_bytes=0)
    # its skip-image upsample 256 -> 512 with the add
    p = hp.upfirdn2d_plan(_spec((4, 3, 256, 256)), (4, 4), 2, 2, 1, 1, 2, 1, 2, 1, False, 4.0, add=_spec((4, 3, 512, 512)))
    assert p == dict(form='fir_up2', instance=uc.TUP2, cell_u=0, staging=1, c_fastest=0, tiles_x=4, tiles_y=16, grid=4 * 3 * 64, lds_bytes=0)
    # odd pads shift the cells: 129 output columns from pad_x0 = 3 need 66 cells of 2, 33 rows from pad_y0 = 1 need 17
    p = hp.upfirdn2d_plan(_spec((1, 1, 16, 64)), (4, 4), 2, 2, 1, 1, 3, 1, 1, 3)
    assert (p['form'], p['tiles_x'], p['tiles_y'], p['grid']) == ('tile', 2, 2, 4)
    # the viewer's 47 x 47 filter at up 4 (513 outputs from cell -7 to cell 121): 13 x 4 rows of 64 floats of padded filter; the streaming grids stop at 8 workgroups per CU
    p = hp.upfirdn2d_plan(_spec((1, 3, 128, 128)), (47, 47), 4, 4, 1, 1, 25, 22, 25, 22, False, 16.0)
    assert p == dict(form='cell', instance=None, cell_u=4, staging=-1, c_fastest=0, tiles_x=129, tiles_y=129, grid=-(-3 * 129 * 4 * 129 // 256), lds_bytes=64 * 52 * 4)
    assert hp.upfirdn2d_plan(_spec((1, 3, 512, 512)), (47, 47), 4, 4, 1, 1, 25, 22, 25, 22)['grid'] == 2048
    p = hp.upfirdn2d_plan(_spec((2, 3, 20, 22), dtype=torch.float64), (4, 4), 2, 2, 1, 1, 2, 1, 2, 1)
    assert p == dict(form='generic', instance=None, cell_u=0, staging=-1, c_fastest=0, tiles_x=0, tiles_y=0, grid=-(-2 * 3 * 40 * 44 // 256), lds_bytes=0)
    # down 2: 128 x 16 outputs per tile
    p = hp.upfirdn2d_plan(_spec((1, 2, 512, 512), dtype=torch.float16), (4, 4), 1, 1, 2, 2, 1, 1, 1, 1)
    assert (p['form'], p['instance'], p['staging'], p['tiles_x'], p['tiles_y']) == ('tile', uc.TDN2, 0, 2, 16)


def test_plan_refuses_what_the_launch_refuses():
    hp = _hp()
    ok = lambda **kw: hp.upfirdn2d_plan(_spec((1, 2, 5, 6)), (4, 4), **dict(dict(padx0=1, padx1=1, pady0=1, pady1=1), **kw))
    assert ok()['form'] == 'tile'
    for kw in (dict(upx=0), dict(upy=0), dict(downx=0), dict(downy=-1), dict(act=2), dict(act=9), dict(padx0=-9), dict(pady1=-9)):
        with pytest.raises(RuntimeError):
            ok(**kw)
    for shape in ((0, 2, 5, 6), (1, 0, 5, 6), (1, 2, 0, 6)):
        with pytest.raises(RuntimeError):
            hp.upfirdn2d_plan(_spec(shape, stride=(60, 30, 6, 1)), (4, 4), padx0=4, padx1=4, pady0=4, pady1=4)
    with pytest.raises(RuntimeError):
        hp.upfirdn2d_plan(_spec((1, 2, 5, 6)), (0, 4), padx0=1, padx1=1)
    # straight through the C ABI: null pointers and a storage type that does not exist
    lib = hp.load()

    def raw(**over):
        p, _, _ = hp._upfirdn_params((1, 2, 5, 6), (60, 30, 6, 1), torch.float32, 4096, 0, (4, 4), (4, 1), 4096, 1, 1, 1, 1, 1, 1, 1, 1, False, 1.0)
        p.y, p.y_stride = 4096, hp._i64x4((40, 20, 5, 1))
        for k, v in over.items():
            setattr(p, k, v)
        info = hp._UpfirdnPlanInfo()
        return lib.ide3d_upfirdn2d_plan(ctypes.byref(p), None, ctypes.byref(info)), info

    rc, info = raw()
    assert rc == 0 and hp.UPFIRDN_FORMS[info.form] == 'tile'          # a null epilogue is the plain call
    for over in (dict(x=None), dict(f=None), dict(y=None), dict(dtype=4), dict(dtype=-1), dict(out_w=0)):
        assert raw(**over)[0] == -1, over
        assert lib.ide3d_last_error()
    assert lib.ide3d_upfirdn2d_plan(None, None, ctypes.byref(hp._UpfirdnPlanInfo())) == -1
    p, _, _ = hp._upfirdn_params((1, 2, 5, 6), (60, 30, 6, 1), torch.float32, 4096, 0, (4, 4), (4, 1), 4096, 1, 1, 1, 1, 1, 1, 1, 1, False, 1.0)
    assert lib.ide3d_upfirdn2d_plan(ctypes.byref(p), None, None) == -1
    # more tiles than a grid holds
    with pytest.raises(RuntimeError, match='grid too large'):
        hp.upfirdn2d_plan(_spec((2 ** 15, 2 ** 15, 33, 65), stride=(0, 0, 65, 1)), (4, 4), 1, 1, 1, 1, 2, 1, 2, 1)


@pytest.mark.parametrize('case', uc.CASES, ids=[c.name for c in uc.CASES])
def test_the_two_references_agree_and_the_float32_definition_is_within_the_bound(case):
    from torch_utils.ops import upfirdn2d as up
    r = uc.reference(case)
    x, f = case.values('x'), case.filter()
    kw = dict(up=list(case.up), down=list(case.down), padding=list(case.pad), flip_filter=case.flip, gain=case.gain)
    # (the definition scales the float32 taps by the gain in float32; the oracle takes the gain in float64: the gain is applied outside here,
    # and the float32 run below keeps the definition's own rounding of f * gain, which the bound counts)
    def64 = up._upfirdn2d_ref(x.double(), f, **dict(kw, gain=1)) * case.gain
    assert def64.dtype == r['fir'].dtype == torch.float64 and tuple(def64.shape) == tuple(r['fir'].shape) == case.out_shape
    # both in float64: what is left is the order of the sums, 2^-53 per tap of the sum of absolute products
    bound64 = r['tol_fir'] * (2.0 ** -53 / uc.EPS[case.dtype])
    assert bool(((def64 - r['fir']).abs() <= bound64).all()), float(((def64 - r['fir']).abs() / bound64.clamp_min(1e-300)).max())
    if case.dtype != 'f64':          # the definition with float accumulation on the stored values: inside the bound the GPU suite applies to the FIR
        def32 = up._upfirdn2d_ref(x.float(), f, **kw)
        ratio = ((def32.double() - r['fir']).abs() / r['tol_fir'].clamp_min(1e-300))
        assert float(ratio.max()) <= 1.0, float(ratio.max())
    assert bool(torch.isfinite(r['y']).all()) and bool((r['tol'] >= 0).all())
    # the ratio the GPU suite takes: 0 for the reference itself, infinite for a NaN (a leaked pad column holds one)
    bad = r['y'].clone()
    bad.view(-1)[0] = float('nan')
    assert uc.worst_ratio(r['y'], case) == 0.0 and uc.worst_ratio(bad, case) == float('inf')


def test_twins_carry_equal_values_through_different_staging_paths():
    assert len(uc.TWINS) >= 10
    for a, b in uc.TWINS:
        fa, fb = a.fields(), b.fields()
        assert {k for k in fa if fa[k] != fb[k]} == {'layout'}, (a.name, b.name)
        assert torch.equal(a.values('x'), b.values('x'))
        if a.form == b.form == 'tile':
            assert {a.staging, b.staging} == {0, 1} and a.instance == b.instance, (a.name, b.name)
        else:          # a lean case (16-byte by construction) against the scalar staging of the instance it reproduces
            assert {a.form, b.form} in ({'fir44', 'tile'}, {'fir_up2', 'tile'}) and a.instance == b.instance and {a.staging, b.staging} == {0, 1}
    assert {a.instance for a, _ in uc.TWINS} == set(uc.TILE_INSTANCES)
