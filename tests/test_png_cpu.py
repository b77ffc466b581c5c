"""PNG files without a GPU: the host definition of training/png.py through the independent decoder of
tests/png_ref.py (and PIL where it is installed), its adaptive filter choice, tokens, code lengths and sizes against plain restatements
and zlib, `save_image` against torchvision's formulas, the files' writers and the C ABI with its refusals."""
import ctypes
import io
import os
import re
import zlib

import numpy as np
import pytest
import torch

import png_cases
import png_ref
from training import png

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_files = {}


def host_file(name):
    """The host definition's file of a case, computed once and never modified."""
    if name not in _files:
        frame, filt, seg = png_cases.CASES[name]
        _files[name] = png.encode_png(torch.from_numpy(frame), filt, seg)[0]
    return _files[name]


def segments(name):
    frame, filt, seg = png_cases.CASES[name]
    stream, _ = png.filter_rows(frame, png.FILTERS[filt])
    return [stream[o:o + seg] for o in range(0, stream.shape[0], seg)]


# ---- round trips ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('name', sorted(png_cases.CASES))
def test_round_trip(name):
    frame, filt, seg = png_cases.CASES[name]
    img, types, z = png_ref.decode(host_file(name))
    assert img.shape == frame.shape and np.array_equal(img, frame)
    if filt != 'adaptive':
        assert (types == png.FILTERS[filt]).all()
    assert z[:2] == b'\x78\x01'
    # a segment never takes more than its bytes + 5
    F = frame.shape[0] * (frame.shape[1] * frame.shape[2] + 1)
    assert len(z) <= png.worst_case_bytes(*frame.shape, seg) == F + 5 * -(-F // seg) + 6


@pytest.mark.parametrize('name', sorted(png_cases.CASES))
def test_round_trip_pil(name):
    Image = pytest.importorskip('PIL.Image')
    frame = png_cases.CASES[name][0]
    im = Image.open(io.BytesIO(host_file(name)))
    assert im.mode == ('L' if frame.shape[2] == 1 else 'RGB')
    assert np.array_equal(np.asarray(im).reshape(frame.shape), frame)


def test_cases_cover_what_they_claim():
    c = png_cases.CASES
    assert {c[k][0].shape[1] * c[k][0].shape[2] % 4 for k in ('rowbytes_4k', 'rowbytes_4k+1', 'rowbytes_4k+3')} == {0, 1, 3}
    assert c['boundary_5x1366x3'][0].shape == (5, 1366, 3) and (1366 * 3 + 1) % 1024 != 0
    for name, (frame, filt, seg) in c.items():
        assert frame.dtype == np.uint8 and frame.ndim == 3 and (seg == 1024 or name == 'length_limit')
    assert all(len(segments(k)) > 1 for k in ('constant', 'zeros', 'boundary_5x1366x3', 'runs', 'alternating', 'random', 'forced_paeth'))
    assert len(segments('length_limit')) == 1


# ---- rows -------------------------------------------------------------------------------------------------------------------------

def _filter_row_plain(t, cur, prev, C):
    out = []
    for x in range(len(cur)):
        a = int(cur[x - C]) if x >= C else 0
        b = int(prev[x])
        c = int(prev[x - C]) if x >= C else 0
        if t == 4:
            p = a + b - c
            pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
            pred = a if pa <= pb and pa <= pc else (b if pb <= pc else c)
        else:
            pred = (0, a, b, (a + b) // 2)[t]
        out.append((int(cur[x]) - pred) & 255)
    return out


@pytest.mark.parametrize('name', ['1x37x3', 'rowbytes_4k+1', 'boundary_5x1366x3', 'flat_labels', 'constant_adaptive', 'forced_average'])
def test_adaptive_choice_is_the_brute_force_minimum(name):
    frame = png_cases.CASES[name][0]
    H, W, C = frame.shape
    stream, types = png.filter_rows(frame, 5)
    rows = stream.reshape(H, W * C + 1)
    flat = frame.reshape(H, W * C)
    for y in range(0, H, max(1, H // 6)):
        prev = flat[y - 1] if y else np.zeros(W * C, np.uint8)
        cand = [_filter_row_plain(t, flat[y], prev, C) for t in range(5)]
        cost = [sum(min(v, 256 - v) for v in row) for row in cand]
        best = min(range(5), key=lambda t: (cost[t], t))
        assert types[y] == best == rows[y, 0]
        assert rows[y, 1:].tolist() == cand[best]


# ---- tokens -----------------------------------------------------------------------------------------------------------------------

def _tokens_plain(data):
    """The token rule as a sequential scan."""
    out, i, n = [], 0, len(data)
    while i < n:
        e = i
        while e < n and data[e] == data[i]:
            e += 1
        out.append((int(data[i]), 0))
        m = e - i - 1
        while m >= 3:
            out.append((int(data[i]), min(m, 258)))
            m -= min(m, 258)
        out += [(int(data[i]), 0)] * m
        i = e
    return out


@pytest.mark.parametrize('name', ['runs', 'constant', 'zeros', 'alternating', 'boundary_5x1366x3', 'flat_labels'])
def test_tokens_are_the_sequential_rule(name):
    for seg in segments(name):
        value, length = png.segment_tokens(seg)
        assert list(zip(value.tolist(), length.tolist())) == _tokens_plain(seg.tolist())


def test_run_lengths_case_holds_exactly_those_runs():
    want = {1: [0], 2: [0, 0], 3: [0, 0, 0], 4: [0, 3], 258: [0, 257], 259: [0, 258], 260: [0, 258, 0], 261: [0, 258, 0, 0], 262: [0, 258, 3],
            516: [0, 258, 257], 517: [0, 258, 258]}
    seen = {}
    for seg in segments('runs'):
        assert seg.shape[0] == 1024 and seg[0] == 0
        value, length = png.segment_tokens(seg)
        for v in np.unique(value):
            if 10 < v < 200:
                seen[int((seg == v).sum())] = length[value == v].tolist()
    assert seen == want
    value, length = png.segment_tokens(segments('alternating')[0])
    assert (length == 0).all() and not png.segment_plan(segments('alternating')[0])['has_match']


def test_length_codes_are_rfc_1951():
    base = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
    extra = [0] * 8 + [1] * 4 + [2] * 4 + [3] * 4 + [4] * 4 + [5] * 4 + [0]
    for length in range(3, 259):
        k = max(i for i in range(29) if base[i] <= length) if length < 258 else 28
        assert (png.LENGTH_SYMBOL[length], png.LENGTH_EXTRA_BITS[length], png.LENGTH_EXTRA_VALUE[length]) == (257 + k, extra[k], length - base[k])


# ---- codes ------------------------------------------------------------------------------------------------------------------------

def _kraft(lens):
    return sum(2.0 ** -int(l) for l in lens if l)


@pytest.mark.parametrize('name', sorted(png_cases.CASES))
def test_code_lengths_are_complete_and_limited(name):
    for seg in segments(name):
        p = png.segment_plan(seg)
        assert p['hist'][256] == 1 and p['hist'].sum() == p['value'].shape[0] + 1
        assert ((p['lens'] > 0) == (p['hist'] > 0)).all() and p['lens'].max() <= 15 and _kraft(p['lens']) == 1.0
        assert ((p['cl_lens'] > 0) == (p['cl_hist'] > 0)).all() and p['cl_lens'].max() <= 7 and _kraft(p['cl_lens']) == 1.0
        assert 257 <= p['hlit'] <= 286 and 4 <= p['hclen'] <= 19
        # the run-length coded header expands to the lengths it stands for
        seq = []
        for s, e in p['cl_tokens']:
            seq += [s] if s < 16 else [seq[-1]] * (e + 3) if s == 16 else [0] * (e + (3 if s == 17 else 11))
        assert seq == p['lens'][:p['hlit']].tolist() + [1 if p['has_match'] else 0]


def test_code_lengths_are_optimal_below_the_limit():
    """Where no depth passes the limit the lengths cost what a plain heap-built Huffman code costs."""
    import heapq
    rng = np.random.RandomState(3)
    for trial in range(20):
        freq = (rng.randint(0, 50, size=286) * (rng.rand(286) < 0.4)).astype(np.int64)
        freq[256] = 1
        heap = [(int(f), i) for i, f in enumerate(freq) if f]
        heapq.heapify(heap)
        cost = 0
        while len(heap) > 1:
            a, b = heapq.heappop(heap), heapq.heappop(heap)
            cost += a[0] + b[0]
            heapq.heappush(heap, (a[0] + b[0], 1000 + len(heap) + trial))
        lens = png.code_lengths(freq, 15)
        assert png.leaf_depth_counts(freq)[1].__len__() - 1 <= 15
        assert int((lens * freq).sum()) == cost and _kraft(lens) == 1.0


def test_length_limit_case_exercises_the_limiter():
    (seg,) = segments('length_limit')
    p = png.segment_plan(seg)
    assert seg.shape[0] == 28655
    assert sorted(p['hist'][p['hist'] > 0].tolist()) == sorted([1] + list(png_cases.FIBONACCI))
    assert p['unlimited_depth'] == 20 > 15 and not p['has_match'] and (p['length'] == 0).all()
    assert p['lens'].max() == 15 and _kraft(p['lens']) == 1.0
    # the block is a dynamic one, not the stored fallback
    assert png.dynamic_size(p['bits'], True) < seg.shape[0] + 5
    assert png.deflate_segment(seg, True)[0] & 7 == 0b101


def test_canonical_codes_follow_the_rfc_example():
    # RFC 1951 3.2.2: lengths (3, 3, 3, 3, 3, 2, 4, 4) -> codes 010 011 100 101 110 00 1110 1111
    codes = png.canonical_codes([3, 3, 3, 3, 3, 2, 4, 4])
    want = ['010', '011', '100', '101', '110', '00', '1110', '1111']
    assert [format(int(c), '0%db' % len(w))[::-1] for c, w in zip(codes, want)] == want


# ---- sizes ------------------------------------------------------------------------------------------------------------------------

def test_random_bytes_are_stored():
    for name in png_cases.STORED_CASES:
        frame, filt, seg = png_cases.CASES[name]
        segs = segments(name)
        for k, s in enumerate(segs):
            block = png.deflate_segment(s, k == len(segs) - 1)
            assert block[0] == (1 if k == len(segs) - 1 else 0) and len(block) == s.shape[0] + 5 and block[5:] == s.tobytes()
        F = sum(s.shape[0] for s in segs)
        assert len(host_file(name)) == F + 5 * len(segs) + 6 + 57          # zlib framing 6, PNG container 8 + 25 + 12 + 12


def realistic_stream():
    """The filtered stream of a 96 x 1024 x 3 frame like the renderer's: a smooth noisy RGB half beside a flat 19-colour label half."""
    rng = np.random.RandomState(0)
    y, x = np.mgrid[0:96, 0:512]
    rgb = np.stack([128 + 80 * np.sin(x / 90.0 + c) * np.cos(y / 70.0) + rng.normal(0, 2.0, size=x.shape) for c in range(3)], axis=2)
    labels = ((x // 37 + y // 29) % 19).astype(np.uint8)
    palette = rng.randint(0, 256, size=[19, 3]).astype(np.uint8)
    frame = np.concatenate([np.clip(rgb, 0, 255).astype(np.uint8), palette[labels]], axis=1)
    return png.filter_rows(frame, 5)[0]


def test_size_against_zlib_rle_at_the_same_boundaries():
    stream = realistic_stream()
    seg = 32768
    assert stream.shape[0] >= 8 * seg
    ours = 0
    comp = zlib.compressobj(6, zlib.DEFLATED, -15, 8, zlib.Z_RLE)
    ref = 0
    for o in range(0, stream.shape[0], seg):
        last = o + seg >= stream.shape[0]
        ours += len(png.deflate_segment(stream[o:o + seg], last))
        ref += len(comp.compress(stream[o:o + seg].tobytes())) + len(comp.flush(zlib.Z_FINISH if last else zlib.Z_FULL_FLUSH))
    print(f'host definition {ours} bytes, zlib Z_RLE flushed every {seg} bytes {ref} bytes: {100.0 * (ours - ref) / ref:+.2f} %')
    assert ours <= ref * 1.01
    assert ours < stream.shape[0] / 2


# ---- save_image -------------------------------------------------------------------------------------------------------------------

def test_save_image_grid_and_bytes(tmp_path):
    g = torch.Generator().manual_seed(0)
    t = torch.rand(5, 3, 6, 7, generator=g) * 2.4 - 1.2
    grid = png.image_grid_u8(t, nrow=3, padding=2, normalize=True, value_range=(-1, 1), pad_value=0.25)
    assert grid.shape == ((6 + 2) * 2 + 2, (7 + 2) * 3 + 2, 3) and grid.dtype == torch.uint8
    want = np.full(grid.shape, int(np.floor(255 * 0.25 + 0.5)), np.uint8)
    x = (np.clip(t.numpy().astype(np.float32), -1, 1) + 1) / np.float32(2)
    for k in range(5):
        r, c = divmod(k, 3)
        want[r * 8 + 2:r * 8 + 8, c * 9 + 2:c * 9 + 9] = np.floor(np.clip(255 * x[k] + 0.5, 0, 255)).astype(np.uint8).transpose(1, 2, 0)
    assert np.array_equal(grid.numpy(), want)
    # a batch of one image is written as it is; a single channel is replicated; without value_range the tensor's own range is used
    one = png.image_grid_u8(t[:1, :1], normalize=True)
    lo, hi = float(t[0, 0].min()), float(t[0, 0].max())
    q = np.floor(np.clip(255 * ((t[0, 0].numpy() - lo) / max(hi - lo, 1e-5)) + 0.5, 0, 255)).astype(np.uint8)
    assert one.shape == (6, 7, 3) and all(np.array_equal(one[..., c].numpy(), q) for c in range(3))
    assert png.image_grid_u8(t[0]).shape == (6, 7, 3)
    raw = png.image_grid_u8(torch.tensor([[[-0.5, 0.0, 0.001, 0.5, 1.0, 1.7]]]))
    assert raw[0, :, 0].tolist() == [0, 0, 0, 128, 255, 255]
    # the call of gen_images.py:115-116
    path = tmp_path / 'seed0000.png'
    png.save_image(t, str(path), normalize=True, range=(-1, 1))
    img = png_ref.decode(path.read_bytes())[0]
    assert np.array_equal(img, png.image_grid_u8(t, normalize=True, value_range=(-1, 1)).numpy())
    with pytest.raises(ValueError):
        png.image_grid_u8(torch.zeros(2, 4, 5, 5))


def test_writers(tmp_path):
    from training import video_render
    frames = [torch.from_numpy(png_cases.noisy_gradient(12, 20, 3, s)) for s in range(5)]
    assert video_render.write_png_sequence(iter(frames), str(tmp_path / 'f%03d.png'), batch=2) == 5
    for k, f in enumerate(frames):
        assert np.array_equal(png_ref.decode((tmp_path / f'f{k:03d}.png').read_bytes())[0], f.numpy())
    png.save_png(frames[0], tmp_path / 'one.png')
    assert (tmp_path / 'one.png').read_bytes() == png.encode_png(frames[0])[0] == png.encode_png(torch.stack(frames))[0]
    with pytest.raises(ValueError):
        png.save_png(torch.stack(frames), ['a.png'])
    for bad in (torch.zeros(4, 4, 2, dtype=torch.uint8), torch.zeros(4, 4, 3), torch.zeros(0, 4, 3, dtype=torch.uint8)):
        with pytest.raises(ValueError):
            png.encode_png(bad)
    for seg in (512, 65536, 3000):
        with pytest.raises(ValueError):
            png.encode_png(frames[0], segment_bytes=seg)
    with pytest.raises(ValueError):
        png.encode_png(frames[0], filter='best')


def test_integration_note_names_the_patch():
    with open(os.path.join(ROOT, 'INTEGRATION.md')) as f:
        text = f.read()
    assert 'from training.png import save_image' in text and 'gen_images.py' in text


# ---- C ABI ------------------------------------------------------------------------------------------------------------------------

def test_c_abi_and_refusals():
    from torch_utils import hip_plugin
    with open(os.path.join(ROOT, 'include', 'ide3d_hip.h')) as f:
        h = f.read()
    assert re.search(r'int64_t ide3d_png_workspace_bytes\(int32_t n, int32_t h, int32_t w, int32_t c, int32_t segment_bytes\);', h)
    assert re.search(r'int64_t ide3d_png_out_bytes\(int32_t n, int32_t h, int32_t w, int32_t c, int32_t segment_bytes\);', h)
    assert re.search(r'int ide3d_png_encode\(const uint8_t\* frames, int32_t n, int32_t h, int32_t w, int32_t c, int32_t filter_mode, int32_t segment_bytes,\s*'
                     r'void\* workspace, int64_t workspace_bytes, uint8_t\* out, int64_t out_capacity, int64_t\* offsets, void\* stream\);', h)
    assert 'gen_images.py:115-116' in h
    path = hip_plugin.lib_path()
    assert os.path.isfile(path), f'{path} missing: run __graft_entry__.build()'
    lib, loaded = ctypes.CDLL(path), hip_plugin.load()
    for name in ('ide3d_png_workspace_bytes', 'ide3d_png_out_bytes', 'ide3d_png_encode'):
        assert name in hip_plugin.EXPORTED_SYMBOLS and hasattr(lib, name), name
        m = re.search(r'(int64_t|int) %s\(([^)]*)\);' % name, h)
        assert len(getattr(loaded, name).argtypes) == len(m.group(2).split(',')), name
    assert hip_plugin._ABI_VERSION == 8 and lib.ide3d_abi_version() == 8
    assert hip_plugin.PLUGINS['png_plugin'] is hip_plugin.PngPlugin
    # host arithmetic only
    ws, ob = loaded.ide3d_png_workspace_bytes, loaded.ide3d_png_out_bytes
    F = 512 * 3073
    assert ob(4, 512, 1024, 3, 32768) == 4 * (F + 5 * 49 + 6) == 4 * png.worst_case_bytes(512, 1024, 3, 32768)
    assert ws(4, 512, 1024, 3, 32768) == 4 * F + 4 * 49 * (32768 + 32) + 4 * 49 * 16 + 4 * 49 * 8          # F is a multiple of 16 here
    assert ob(1, 1, 1, 1, 1024) == 2 + 5 + 6 and ws(1, 1, 1, 1, 1024) == 16 + 1056 + 16 + 16
    for bad in ((0, 8, 8, 3, 1024), (1, 0, 8, 3, 1024), (1, 8, 8, 2, 1024), (1, 8, 8, 4, 1024), (1, 8, 8, 3, 512), (1, 8, 8, 3, 65536),
                (1, 8, 8, 3, 1025), (4, 32768, 16384, 3, 32768), (1, 65536, 32768, 1, 32768)):
        assert ws(*bad) == -1 and ob(*bad) == -1, bad
    # every refusal comes before the first launch, so it needs no GPU; the pointers are never read
    buf = (ctypes.c_uint8 * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    enc = loaded.ide3d_png_encode
    big = 1 << 30
    refused = [enc(p, 1, 8, 8, 2, 5, 1024, p, big, p, big, p, None), enc(p, 1, 8, 8, 3, 5, 2000, p, big, p, big, p, None),
               enc(p, 1, 8, 8, 3, 6, 1024, p, big, p, big, p, None), enc(p, 1, 8, 8, 3, -1, 1024, p, big, p, big, p, None),
               enc(p, 1, 8, 8, 3, 5, 1024, p, ws(1, 8, 8, 3, 1024) - 1, p, big, p, None),
               enc(p, 1, 8, 8, 3, 5, 1024, p, big, p, ob(1, 8, 8, 3, 1024) - 1, p, None), enc(p, 1, 8, 8, 3, 5, 1024, p, big, p, 1 << 31, p, None),
               enc(None, 1, 8, 8, 3, 5, 1024, p, big, p, big, p, None), enc(p, 4, 32768, 16384, 3, 5, 32768, p, big, p, big, p, None)]
    assert refused == [-1] * len(refused)
    assert b'png_encode' in loaded.ide3d_last_error()
