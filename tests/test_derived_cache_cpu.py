"""The rules of the two host caches that keep memory alive between calls, stated once, against the helpers that use them:
`torch_utils.misc.DerivedCache` (tensors derived from parameters: training/networks.py, training/face_parsing.py) and
`torch_utils.hip_plugin._Workspaces` (launch workspaces and the packed-weight copies inside them).
  1. an entry is valid only for the very tensor object it was made from, at the same `_version`, device and storage address;
  2. a live entry is never freed (a captured hipGraph holds raw pointers into it): only entries whose source is gone are dropped, and
     only once the table has outgrown its limit;
  3. with grad enabled and a source that requires grad nothing is cached: the caller gets the differentiable expression.
CPU tensors only; the shared library is not needed."""

import gc

import torch

from torch_utils import hip_plugin, misc
from training import face_parsing, networks


def _param(*shape):
    return torch.nn.Parameter(torch.randn(*shape), requires_grad=False)


def test_scaled_weight_is_valid_for_one_object_version_address_and_gain():
    w = _param(4, 3, 3, 3)
    a = networks._scaled_weight(w, 0.5)
    assert torch.equal(a, w * 0.5) and networks._scaled_weight(w, 0.5) is a
    with torch.no_grad():
        w.mul_(2)                                    # in-place edit: `_version` moves
    b = networks._scaled_weight(w, 0.5)
    assert b is not a and torch.equal(b, w * 0.5) and networks._scaled_weight(w, 0.5) is b
    w.data = w.data.clone()                          # same object, same version, other storage (what `Module.to()` does)
    c = networks._scaled_weight(w, 0.5)
    assert c is not b and torch.equal(c, b) and networks._scaled_weight(w, 0.5) is c
    d = networks._scaled_weight(w, 0.25)
    assert d is not c and torch.equal(d, w * 0.25)
    w2 = torch.nn.Parameter(w.detach().clone(), requires_grad=False)       # another object with equal contents ...
    assert networks._scaled_weight(w2, 0.25) is not d
    assert networks._scaled_weight(w, 0.25) is d     # ... has an entry of its own


def test_cat_cached_sees_both_sources_and_steps_aside_for_autograd():
    a, b = _param(5), _param(7)
    with torch.no_grad():
        y = networks._cat_cached(a, b)
        assert torch.equal(y, torch.cat([a, b])) and networks._cat_cached(a, b) is y
        b.add_(1.0)                                  # only the second source changed
        y2 = networks._cat_cached(a, b)
        assert y2 is not y and torch.equal(y2, torch.cat([a, b])) and networks._cat_cached(a, b) is y2
        b2 = torch.nn.Parameter(b.detach().clone(), requires_grad=False)
        assert networks._cat_cached(a, b2) is not y2       # another object in second place
    y3 = networks._cat_cached(a, b2)                 # grad mode alone is no reason to step aside: nothing here requires grad
    assert networks._cat_cached(a, b2) is y3 and y3.grad_fn is None
    b2.requires_grad_(True)
    table = networks._cat_cache.table
    before = dict(table)
    z = networks._cat_cached(a, b2)
    assert z.grad_fn is not None and z is not y3
    assert table.keys() == before.keys() and all(table[k] is v for k, v in before.items())      # nothing stored
    with torch.no_grad():
        assert networks._cat_cached(a, b2) is y3     # inference with the same tensors: the cached one again


def test_scaled_const_noise_steps_aside_for_autograd():
    const, strength = torch.randn(8, 8), _param(1)
    n = networks._scaled_const_noise(const, strength)
    assert torch.equal(n, const * strength) and networks._scaled_const_noise(const, strength) is n
    strength.requires_grad_(True)
    assert networks._scaled_const_noise(const, strength).grad_fn is not None
    with torch.no_grad():
        assert networks._scaled_const_noise(const, strength) is n


def test_grad_weight_keeps_both_orientations_of_one_weight():
    w = _param(6, 4, 3, 3)
    f, p = networks._grad_weight(w, True), networks._grad_weight(w, False)
    assert networks._grad_weight(w, True) is f and networks._grad_weight(w, False) is p
    assert tuple(p.shape) == (4, 6, 3, 3) and p.is_contiguous() and f.is_contiguous()
    assert torch.equal(p, w.transpose(0, 1)) and torch.equal(f, p.flip(2, 3)) and not torch.equal(f, p)
    with torch.no_grad():
        w.add_(1.0)                                  # an optimiser step: both are re-made
    assert networks._grad_weight(w, True) is not f and networks._grad_weight(w, False) is not p
    assert torch.equal(networks._grad_weight(w, True), w.transpose(0, 1).flip(2, 3))


def test_wsq_follows_the_weight():
    w = _param(6, 4, 3, 3)
    s = networks._wsq_t(w)
    assert tuple(s.shape) == (4, 6) and torch.allclose(s, w.square().sum(dim=[2, 3]).t()) and networks._wsq_t(w) is s
    with torch.no_grad():
        w.mul_(3)
    assert networks._wsq_t(w) is not s and torch.allclose(networks._wsq_t(w), s * 9)


def test_folded_batchnorm_follows_running_statistics():
    torch.manual_seed(0)
    conv, bn = torch.nn.Conv2d(3, 5, 3, bias=False), torch.nn.BatchNorm2d(5).eval()
    with torch.no_grad():
        bn.running_var.uniform_(0.5, 2.0); bn.running_mean.normal_(); bn.weight.normal_(); bn.bias.normal_()
    w, b = face_parsing._folded(conv, bn)
    w_again, b_again = face_parsing._folded(conv, bn)
    assert w_again is w and b_again is b
    x = torch.randn(2, 3, 9, 9)
    with torch.no_grad():
        assert torch.allclose(torch.nn.functional.conv2d(x, w, b), bn(conv(x)), atol=1e-5)
        bn.running_var.mul_(4.0)                     # a buffer edited in place
        w2, b2 = face_parsing._folded(conv, bn)
        assert w2 is not w and torch.allclose(torch.nn.functional.conv2d(x, w2, b2), bn(conv(x)), atol=1e-5)
        assert face_parsing._folded(conv, bn)[0] is w2
        other = torch.nn.Conv2d(3, 5, 3, bias=False)             # another convolution in front of the same BatchNorm
        w4, b4 = face_parsing._folded(other, bn)
        assert torch.allclose(torch.nn.functional.conv2d(x, w4, b4), bn(other(x)), atol=1e-5) and face_parsing._folded(conv, bn)[0] is w2
    plain = torch.nn.Conv2d(3, 5, 1, bias=False)
    w3, b3 = face_parsing._folded(plain, None)
    assert b3 is None and torch.equal(w3, plain.weight) and face_parsing._folded(plain, None)[0] is w3


def test_eviction_drops_dead_entries_only_and_only_past_the_limit():
    cache = misc.DerivedCache(limit=4)
    sources = [_param(3) for _ in range(4)]
    values = [cache.get((s,), lambda s=s: s * 2.0) for s in sources]
    del sources[0], sources[0]                       # two of the four sources die
    gc.collect()
    live = [_param(3)]
    values.append(cache.get((live[0],), lambda: live[0] * 2.0))
    assert len(cache.table) == 5                     # the table was AT its limit, not past it, when this entry came: the dead ones stay
    live.append(_param(3))
    values.append(cache.get((live[1],), lambda: live[1] * 2.0))
    assert len(cache.table) == 4                     # past the limit: the two dead entries are gone ...
    for s, v in zip(sources + live, values[2:]):     # ... and every live one is the very object it was
        assert cache.get((s,), lambda: None) is v
    assert len(cache.table) == 4
    # nothing but live entries: the table grows past its limit rather than free one
    more = [_param(3) for _ in range(3)]
    for s in more:
        cache.get((s,), lambda s=s: s * 2.0)
    assert len(cache.table) == 7
    for s, v in zip(sources + live, values[2:]):
        assert cache.get((s,), lambda: None) is v
    # an entry goes when its FIRST source is gone; one whose second source died stays until then
    first, second = _param(3), _param(3)
    pair = cache.get((first, second), lambda: torch.cat([first, second]))
    del second
    gc.collect()
    cache.get((_param(3),), lambda: torch.zeros(1))
    assert cache.table[id(first)][2] is pair


def test_workspaces_drop_by_domain_and_packed_stamp():
    ws = hip_plugin._Workspaces(limit=2)
    mine, theirs = ('owner', 1), ('stream', 7)
    made = []
    alloc = lambda: made.append(torch.zeros(4)) or made[-1]
    e1 = ws.entry((11, 0, mine, 6), alloc)
    e2 = ws.entry((12, 0, theirs, 6), alloc)
    ws.entry((0, mine), alloc)
    assert len(made) == 3 and ws.entry((11, 0, mine, 6), alloc) is e1 and len(made) == 3 and e1[0] is made[0]
    ws.drop(mine)
    assert list(ws.table) == [(12, 0, theirs, 6)] and ws.entry((12, 0, theirs, 6), alloc) is e2
    w, v = _param(4, 4, 3, 3), _param(4, 4, 3, 3)
    assert ws.packed(e2, [w]) == [False]             # a fresh entry holds no packed copy
    ws.mark_packed(e2, [w])
    assert ws.packed(e2, [w]) == [True]
    twin = torch.nn.Parameter(w.detach().clone(), requires_grad=False)
    assert ws.packed(e2, [twin]) == [False]          # equal contents, another object
    with torch.no_grad():
        w.mul_(2)
    assert ws.packed(e2, [w]) == [False]             # edited in place since the copy was made
    ws.mark_packed(e2, [w, v])
    with torch.no_grad():
        v.add_(1)
    assert ws.packed(e2, [w, v]) == [True, False]    # per weight
    ws.mark_packed(e2, [])                           # per-image weights: never "packed"
    assert ws.packed(e2, []) == []
    # past the limit only entries whose packed weight is gone are dropped; unmarked ones (per-image weights) stay
    a, b = _param(2), _param(2)
    ea, eb = ws.entry(('a',), alloc), ws.entry(('b',), alloc)
    ws.mark_packed(ea, [a]); ws.mark_packed(eb, [b])
    del a
    gc.collect()
    ec = ws.entry(('c',), alloc)
    assert set(ws.table) == {(12, 0, theirs, 6), ('b',), ('c',)} and ws.entry(('b',), alloc) is eb and ws.entry(('c',), alloc) is ec
    # a plugin without a limit (the mapping network's) never drops anything by itself
    assert hip_plugin.MappingPlugin._ws.limit is None and hip_plugin.ModconvPlugin._ws.limit == 1024 and hip_plugin.LowresPlugin._ws.limit == 64
