"""The plane gate: the last backbone block's launches skip the output tiles under which no needed cell lies.

Operator level, hand-made maps — empty, full, one cell in each corner, a checkerboard of cells, one plane set and the other two empty — on
the 256^2 block's own channel counts (128 -> 128 + dual heads of 192 rows; 96-channel skip accumulation): under every set cell the gated
launch is BIT-EQUAL to the dense one, the full map equals dense everywhere, and what lies under no live tile keeps the sentinel the output
was filled with (the empty map touches nothing).  Shapes: the fused conv1 + heads form exists from 4 x 128^2 on (256 workgroups; below
that the layer's plan is split-K and the library declines the fusion, gate or not), so the convolution runs at batch 4 on 128^2 — 8 x 8
tiles of 16 x 16, image index 0..3 — and the skip accumulation at batch 2, 32^2 -> 64^2.

End to end, a reduced generator whose last backbone block still takes the fused form (128 channels at 128^2 planes of 3 x 32 channels, batch 4;
`tiny_spec`'s 16-channel blocks have none): `G.synthesis(..., return_seg=True)` with the gate and with IDE3D_NO_PLANE_GATE set gives
bit-equal images and segmentations, eagerly and replayed from the graph cache with a different camera on consecutive replays; with
`return_dict=True` the planes are the dense ones everywhere (the dense route was kept)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SENTINEL = 12345.0


def _maps(n, ch, cw, dev):
    """name -> uint8 [n, 3, ch, cw]"""
    z = lambda: torch.zeros([n, 3, ch, cw], dtype=torch.uint8)
    corners = z()
    for i, (y, x) in enumerate(((0, 0), (0, cw - 1), (ch - 1, 0), (ch - 1, cw - 1))):
        corners[i % n, i % 3, y, x] = 1                       # a different image and plane per corner
    checker = z()
    yy, xx = torch.meshgrid(torch.arange(ch), torch.arange(cw), indexing='ij')
    for i in range(n):
        for pl in range(3):
            # a checkerboard of cells inside a checkerboard of 4 x 4-cell blocks (= the convolution's 16 x 16 tiles), shifted per image;
            # plane 2 is shifted by a block as well, so the union of the planes and a single plane tell different stories
            checker[i, pl] = (((yy + xx) % 2 == 0) & ((yy // 4 + xx // 4 + i + pl // 2) % 2 == 0) & ((pl < 2) | (yy < ch // 2))).to(torch.uint8)
    one_plane = z()
    one_plane[:, 1] = 1
    one_plane[n - 1, 1, ch // 2:] = 0                          # ... and only half of it in the last image
    maps = dict(empty=z(), full=z() + 1, corners=corners, checker=checker, one_plane=one_plane)
    return {k: v.to(dev) for k, v in maps.items()}


def _texel_mask(cells, h, w):
    """[n, 3, ch, cw] cells -> bool [n, 3, h, w]: the texels under set cells."""
    return cells.bool().repeat_interleave(4, dim=2).repeat_interleave(4, dim=3)[:, :, :h, :w]


def _tile_mask(texels, th, tw):
    """bool [n, h, w] -> bool [n, h, w]: the th x tw tiles that hold a set texel."""
    n, h, w = texels.shape
    t = texels.reshape(n, h // th, th, w // tw, tw).any(dim=4).any(dim=2)
    return t.repeat_interleave(th, dim=1).repeat_interleave(tw, dim=2)


MAP_NAMES = ('empty', 'full', 'corners', 'checker', 'one_plane')


@pytest.fixture(scope='module')
def conv_problem(gpu_device):
    """The 256^2 block's conv1 + heads at the smallest size with a fused form, and its dense result (computed once, never written to)."""
    from torch_utils import hip_plugin
    from test_gpu_conv_heads import _problem, _fused
    args = _problem(gpu_device, 4, 128, 128, 128, 128, 192, seed=3)
    dense = _fused(hip_plugin.ModconvPlugin, *args, want_x=False)
    assert dense is not None, hip_plugin.load().ide3d_last_error().decode()
    return args, dense[1]


@pytest.mark.parametrize('listed', [False, True], ids=['per_tile', 'listed'])
@pytest.mark.parametrize('name', MAP_NAMES)
def test_conv1_heads_under_a_map(gpu_device, conv_problem, name, listed):
    """`listed`: the launch is handed the compacted list of its live tiles (ide3d_plane_tile_list) and packs them to the front of its grid;
    otherwise every workgroup keeps its tile and looks at the cells under it.  Same results."""
    from torch_utils import hip_plugin
    from test_gpu_conv_heads import _fused
    args, dense = conv_problem
    n, rows, h, w = dense.shape
    cells = _maps(n, h // 4, w // 4, gpu_device)[name]
    gate = cells
    if listed:
        tiles = hip_plugin.plane_tile_list(cells, h, w, 16, 16)
        want = torch.nonzero(cells.bool().any(dim=1).reshape(n, h // 16, 4, w // 16, 4).any(dim=4).any(dim=2).flatten()).flatten().int()
        assert tiles[0].item() == want.numel() and torch.equal(tiles[1:1 + want.numel()], want), 'the live tiles, in ascending order'
        gate = (cells, tiles, (16, 16))
    out = torch.full_like(dense, SENTINEL)
    before = hip_plugin.CALLS.get('modconv2d_heads', 0)
    y, heads = _fused(hip_plugin.ModconvPlugin, *args, want_x=False, gate=gate, heads_out=out)
    assert y is None and heads is out and hip_plugin.CALLS.get('modconv2d_heads', 0) == before + 1
    needed = _texel_mask(cells, h, w).any(dim=1)                           # union of the three planes
    live = _tile_mask(needed, 16, 16)
    print(name, 'needed texels', needed.float().mean().item(), 'live 16 x 16 tiles', live.float().mean().item())
    m = needed[:, None].expand_as(dense)
    assert torch.equal(out[m], dense[m]), 'a texel under a set cell differs from the dense launch'
    lm = live[:, None].expand_as(dense)
    assert torch.equal(out[lm], dense[lm]), 'live tiles are computed whole'
    assert (out[~lm] == SENTINEL).all(), 'a tile without a set cell was written'
    if name == 'full':
        assert torch.equal(out, dense)
    if name == 'empty':
        assert (out == SENTINEL).all()
    assert hip_plugin.exclusive_violations()[0] == 0


def test_conv1_heads_gate_switch_and_checks(gpu_device, conv_problem, monkeypatch):
    """IDE3D_NO_PLANE_GATE: the gated entry point runs dense.  A map of the wrong shape is refused before anything is launched."""
    from torch_utils import hip_plugin
    from test_gpu_conv_heads import _fused
    args, dense = conv_problem
    n, rows, h, w = dense.shape
    cells = _maps(n, h // 4, w // 4, gpu_device)['empty']
    monkeypatch.setenv('IDE3D_NO_PLANE_GATE', '1')
    out = torch.full_like(dense, SENTINEL)
    _fused(hip_plugin.ModconvPlugin, *args, want_x=False, gate=cells, heads_out=out)
    assert torch.equal(out, dense)
    monkeypatch.delenv('IDE3D_NO_PLANE_GATE')
    with pytest.raises(RuntimeError, match='plane gate'):
        _fused(hip_plugin.ModconvPlugin, *args, want_x=False, gate=cells[:, :, :-1], heads_out=out)


@pytest.fixture(scope='module')
def skip_problem(gpu_device):
    from torch_utils import hip_plugin
    g = torch.Generator().manual_seed(5)
    lo = torch.randn(2, 96, 32, 32, generator=g).to(gpu_device)
    add = torch.randn(2, 96, 64, 64, generator=g).to(gpu_device)
    return lo, add, hip_plugin.ResamplePlugin.skip_upsample_add_cl(lo, add)


@pytest.mark.parametrize('name', MAP_NAMES)
def test_skip_accumulation_under_a_map(gpu_device, skip_problem, name):
    """Gated per plane: the 32-channel group cg of an 8 x 32 tile is live iff a cell of plane cg lies under it."""
    from torch_utils import hip_plugin
    lo, add, dense = skip_problem
    n, c, h, w = dense.shape
    cells = _maps(n, h // 4, w // 4, gpu_device)[name]
    out = torch.full_like(dense, SENTINEL)                                 # (channels_last like `dense`)
    got = hip_plugin.ResamplePlugin.skip_upsample_add_cl(lo, add, gate=cells, out=out)
    assert got is out
    needed = _texel_mask(cells, h, w)                                      # [n, 3, h, w]
    for pl in range(3):
        ch = slice(32 * pl, 32 * pl + 32)
        m = needed[:, pl, None].expand(n, 32, h, w)
        assert torch.equal(out[:, ch][m], dense[:, ch][m]), f'plane {pl}: a texel under a set cell differs from the dense launch'
        lm = _tile_mask(needed[:, pl], 8, 32)[:, None].expand(n, 32, h, w)
        assert torch.equal(out[:, ch][lm], dense[:, ch][lm])
        assert (out[:, ch][~lm] == SENTINEL).all(), f'plane {pl}: a tile without a set cell of its plane was written'
    if name == 'full':
        assert torch.equal(out, dense)
    if name == 'empty':
        assert (out == SENTINEL).all()


def test_skip_accumulation_refuses_other_channel_counts(gpu_device):
    from torch_utils import hip_plugin
    lo = torch.zeros(1, 64, 8, 8, device=gpu_device)
    add = torch.zeros(1, 64, 16, 16, device=gpu_device)
    with pytest.raises(RuntimeError, match='96-channel'):
        hip_plugin.ResamplePlugin.skip_upsample_add_cl(lo, add, gate=torch.ones(1, 3, 4, 4, dtype=torch.uint8, device=gpu_device))


# ---- end to end -------------------------------------------------------------------------------------------------------------------------

def _spec():
    from training import triplane
    # vb128 is 128 -> 128 at 128^2 with 2 x 96 head rows: at batch 4 the fused conv1 + heads launch takes it (256 workgroups of 16 x 16)
    return triplane.GeneratorSpec(z_dim=32, w_dim=32, mapping_layers=2, channel_base=16384, channel_max=128, plane_resolution=128,
                                  plane_channels=32, decoder_hidden=64, feature_channels=32, seg_channels=19, render_size=16, num_steps=12,
                                  img_resolution=128, sr_channels={64: 32, 128: 16})


@pytest.fixture(scope='module')
def reduced(gpu_device):
    from training import triplane
    torch.manual_seed(0)
    G = triplane.TriPlaneGenerator(_spec()).eval().requires_grad_(False).to(gpu_device)
    n = 4
    z = torch.from_numpy(np.stack([np.random.RandomState(s).randn(G.z_dim) for s in range(n)])).float().to(gpu_device)
    cond = triplane.conditioning_label().repeat(n, 1).to(gpu_device)
    with torch.no_grad():
        ws = G.mapping(z, cond)
    cams = [torch.cat([triplane.camera_label(y) for y in yaws]).to(gpu_device)
            for yaws in ((-0.5, 0.0, 0.5, 0.25), (0.4, -0.3, 0.1, -0.6))]
    jit = torch.rand(n, 16 * 16, 12, generator=torch.Generator().manual_seed(1)).to(gpu_device)
    return G, ws, cams, jit


def _gated_calls(monkeypatch):
    """Record, per heads / skip launch, whether it ran under a map."""
    from torch_utils import hip_plugin
    seen = []
    real_h, real_s = hip_plugin.ModconvPlugin.modconv2d_heads, hip_plugin.ResamplePlugin.skip_upsample_add_cl

    def heads(*a, **k):
        out = real_h(*a, **k)
        if out is not None:
            seen.append(("heads", a[0].shape[-1], k.get("gate") is not None))
        return out

    def skip(*a, **k):
        seen.append(('skip', a[1].shape[-1], k.get('gate') is not None))
        return real_s(*a, **k)
    monkeypatch.setattr(hip_plugin.ModconvPlugin, 'modconv2d_heads', staticmethod(heads))
    monkeypatch.setattr(hip_plugin.ResamplePlugin, 'skip_upsample_add_cl', staticmethod(skip))
    return seen


def test_synthesis_eager_bit_equal_with_and_without_the_gate(reduced, monkeypatch):
    from torch_utils import hip_plugin
    G, ws, cams, jit = reduced
    monkeypatch.setenv('IDE3D_AUTO_GRAPH', '0')
    seen = _gated_calls(monkeypatch)

    def run(c, **kw):
        with torch.no_grad():
            return G.synthesis(ws, c=c, noise_mode='const', ray_jitter=jit, return_seg=True, **kw)
    for c in cams:
        seen.clear()
        before = hip_plugin.CALLS.get('plane_cells', 0)
        img, seg = run(c)
        assert hip_plugin.CALLS.get('plane_cells', 0) == before + 1
        assert ('heads', 128, True) in seen and seen.count(('skip', 128, True)) == 2, seen      # the gated launches did run
        monkeypatch.setenv('IDE3D_NO_PLANE_GATE', '1')
        seen.clear()
        img0, seg0 = run(c)
        assert not any(g for *_x, g in seen) and hip_plugin.CALLS.get('plane_cells', 0) == before + 1
        d = run(c, return_dict=True)
        planes_knob = [p.clone() for p in d['planes']]
        monkeypatch.delenv('IDE3D_NO_PLANE_GATE')
        assert torch.equal(img, img0) and torch.equal(seg, seg0), 'the gate changed an output'
        # planes that leave the call are dense: no map, and equal to the ones computed with the switch set
        seen.clear()
        d = run(c, return_dict=True)
        assert not any(g for *_x, g in seen), seen
        assert all(torch.equal(a, b) for a, b in zip(d['planes'], planes_knob))
        assert torch.equal(d['image'], img) and torch.equal(d['image_seg'], seg)
        with torch.no_grad():
            planes = G.synthesis.planes(ws)
        assert all(torch.equal(a, b) for a, b in zip(planes, planes_knob)), '`planes()` must stay dense'
    # the cameras see part of the volume: the gate has something to skip
    cells = G.synthesis.renderer.needed_cells(cams[0][:, :16].reshape(-1, 4, 4), (128, 128))
    share = cells.any(dim=1).float().reshape(4, 8, 4, 8, 4).amax(dim=(2, 4)).mean().item()
    print('live 16 x 16 tiles of the reduced generator:', share)
    assert 0.1 < share < 0.7
    assert hip_plugin.exclusive_violations()[0] == 0


def test_synthesis_replayed_with_two_cameras(reduced, monkeypatch):
    """One captured graph, a different camera on consecutive replays: the map is rebuilt on the device inside the graph."""
    from training import graph_cache
    G, ws, cams, jit = reduced
    monkeypatch.delenv('IDE3D_AUTO_GRAPH', raising=False)

    def run(c):
        with torch.no_grad():
            return [t.clone() for t in G.synthesis(ws, c=c, noise_mode='const', ray_jitter=jit, return_seg=True)]
    monkeypatch.setenv('IDE3D_NO_PLANE_GATE', '1')
    with graph_cache.disabled():
        want = [run(c) for c in cams]
    monkeypatch.delenv('IDE3D_NO_PLANE_GATE')
    graph_cache.reset(G.synthesis)
    before = dict(graph_cache.STATS)
    c_buf = cams[0].clone()
    got = []
    for i in (0, 0, 0, 1, 0, 1):                      # eager, capture, then replays that alternate the camera
        c_buf.copy_(cams[i])
        got.append((i, run(c_buf)))
    d = {k: graph_cache.STATS[k] - before.get(k, 0) for k in ('eager', 'capture', 'replay')}
    assert d == {'eager': 1, 'capture': 1, 'replay': 5}, d            # (the capturing call returns its result by a replay, too)
    for i, (img, seg) in got:
        assert torch.equal(img, want[i][0]) and torch.equal(seg, want[i][1]), f'camera {i}: a replay under the gate differs from the dense pass'
    # the switch is part of the signature: setting it does not replay the gated graph
    monkeypatch.setenv('IDE3D_NO_PLANE_GATE', '1')
    caps = graph_cache.STATS['capture']
    run(c_buf); run(c_buf)
    assert graph_cache.STATS['capture'] == caps + 1
    graph_cache.reset(G.synthesis)
