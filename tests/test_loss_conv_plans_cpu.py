"""Plan coverage of the loss networks' plain convolutions without a GPU (tests/loss_conv_launches.py): every plan
class that `ide3d_modconv_plan` gives a launch of the workload set - the parser at 512 x 512, LPIPS with VGG16 at 256 x 256, the identity
net's IR-SE50 at its 112 x 112 crop, in bf16x6 and fp32 - is the class of a stand-in of `STAND_INS`, which tests/test_gpu_loss_convs.py
runs against float64; every stand-in's class still occurs in the workload set; the edge launches are in the table."""

import time

import loss_conv_launches as L


def test_launch_lists_of_the_fused_passes():
    """The shape-only recorder sees what the fused passes launch: 32 + 31 convolutions of the parser (the stem's
    gradient is a pass of its own), 13 + 13 of VGG16, and for IR-SE50 1 + 24 x 2 + 4 shortcuts forward and as many backward."""
    t0 = time.time()
    parse = L.launches('parse', None, 1, 512)
    assert len(parse) == 32 + 31
    assert parse[0] == (1, 147, 64, 256, 256, 1, 0, 'relu'), 'the 7x7 stem as a 1x1 convolution over unfolded patches'
    assert (1, 256, 20, 64, 64, 1, 0, 'grad') in parse and (1, 20, 256, 64, 64, 1, 0, 'grad') in parse
    assert (1, 512, 128, 1, 1, 1, 0, 'relu') in parse and (1, 256, 64, 1, 1, 1, 0, 'relu') in parse and (1, 64, 256, 1, 1, 1, 0, 'grad') in parse
    lp = L.launches('lpips', None, 4, 256)
    assert len(lp) == 26 and lp[0] == (4, 3, 64, 256, 256, 3, 0, 'relu') and lp[-1] == (4, 64, 3, 256, 256, 3, 0, 'grad')
    ident = L.launches('id', None, 4, 256)
    assert len(ident) == 2 * (1 + 24 * 2 + 3)          # the first stage keeps its width: its stride-2 shortcut is a decimation
    assert ident[0] == (4, 3, 64, 112, 112, 3, 0, 'bias') and ident[-1] == (4, 64, 3, 112, 112, 3, 0, 'grad')
    assert (4, 64, 64, 114, 114, 3, 1, 'bias') in ident, 'stride 2: explicit padding + mode 1'
    assert (4, 512, 512, 7, 7, 3, 2, 'grad') in ident and (4, 256, 512, 7, 7, 1, 0, 'bias') in ident
    assert time.time() - t0 < 30, 'the shape-only enumeration must stay in seconds'


def _table():
    return {(a, L.plan_class(l, a)): l for l, ariths in L.STAND_INS for a in ariths}


def test_every_plan_class_of_the_workload_has_a_stand_in():
    want = L.classes_of(L.workload_launches())
    have = _table()
    missing = {k: v[0] for k, v in want.items() if k not in have}
    print(f'{len(want)} plan classes in the workload set, {len(L.CLASS_STAND_INS)} stand-ins')
    assert not missing, f'{len(missing)} plan classes of the workload set have no stand-in (class: a workload launch of it): {missing}'


def test_every_stand_in_class_occurs_in_the_workload():
    want = L.classes_of(L.workload_launches())
    stale = [(l, a) for l, ariths in L.CLASS_STAND_INS for a in ariths if (a, L.plan_class(l, a)) not in want]
    assert not stale, f'stand-ins whose plan class no launch of the workload set has any more: {stale}'
    assert all(ariths and set(ariths) <= set(L.ARITHS) for _, ariths in L.CLASS_STAND_INS)
    assert len({l for l, _ in L.STAND_INS}) == len(L.STAND_INS), 'a launch is listed twice'


def test_the_edge_launches_are_in_the_table():
    table = {l for l, _ in L.STAND_INS}
    for n in (1, 3, 9):
        for cin, cout, epi in ((512, 128, 'relu'), (256, 64, 'relu'), (64, 256, 'bias'), (64, 4, 'relu'), (4, 64, 'bias')):
            assert (n, cin, cout, 1, 1, 1, 0, epi) in table and (n, cout, cin, 1, 1, 1, 0, 'grad') in table
    stem = [l for l in table if l[1:3] == (147, 64) and l[5:] == (1, 0, 'relu')]
    assert any(L.plan(l, 6)['tile_w'] == 128 and (l[3] * l[4]) % 128 != 0 for l in stem), 'K = 147 on a ragged flattened map'
    assert any(L.plan(l, 6)['tile_w'] == 8 and (l[3] % 8 != 0 or l[4] % 8 != 0) for l in stem), 'K = 147 on ragged 8 x 8 tiles (not flattened)'
    assert any(l[1:3] == (3, 64) and l[5:] == (3, 0, 'relu') and l[3] < 64 for l in table)
    assert any(l[1:3] == (64, 3) and l[5:] == (3, 0, 'grad') and l[3] < 64 for l in table)
    assert any(l[1:3] == (256, 19) and l[5:] == (1, 0, 'bias') for l in table) and any(l[1:3] == (19, 256) and l[5:] == (1, 0, 'grad') for l in table)
    for hw in ((1, 1), (2, 3), (7, 7)):
        assert (1, 512, 256) + hw + (3, 2, 'grad') in table
    for l in L.ZERO_BORDER:
        assert l in table and l[6] == 1
    assert {L.out_size(l) for l in L.ZERO_BORDER} == {(1, 1), (7, 7)} and {l[3:5] for l in L.ZERO_BORDER} == {(4, 4), (16, 16)}
