"""JPEG files and Motion-JPEG AVI without a GPU: the host definition of training/jpeg.py through the independent
decoder of tests/jpeg_ref.py and through Pillow, what every case of tests/jpeg_cases.py is there for, its tables against Pillow's, the
colour matrix on all 2^24 values, the DCT's error bound and the quantiser's rounding against float64, quality and size against Pillow's
encoder, the AVI container and its writers, and the C ABI with its refusals."""
import ctypes
import io
import os
import re

import numpy as np
import pytest
import torch
from PIL import Image

import jpeg_cases
import jpeg_ref
from training import jpeg, video_render

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_files, _parsed = {}, {}


def host_file(name):
    """The host definition's file of a case, computed once and never modified."""
    if name not in _files:
        frame, q, sub, ri = jpeg_cases.CASES[name]
        _files[name] = jpeg.encode_jpeg(torch.from_numpy(frame), q, sub, ri)[0]
    return _files[name]


def parsed(name):
    if name not in _parsed:
        _parsed[name] = jpeg_ref.parse(host_file(name))
    return _parsed[name]


def psnr(a, b):
    mse = np.mean((a.astype(np.float64) - b.astype(np.float64)) ** 2)
    return 10 * np.log10(255.0 ** 2 / mse) if mse > 0 else np.inf


# ---- round trips ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('name', sorted(jpeg_cases.CASES))
def test_round_trip(name):
    frame, q, sub, ri = jpeg_cases.CASES[name]
    H, W, C = frame.shape
    p = parsed(name)
    assert (p['height'], p['width'], len(p['components'])) == (H, W, C)
    assert p['markers'] == ['SOI', 0xE0] + [0xDB] * (1 if C == 1 else 2) + [0xC0] + [0xC4] * (2 if C == 1 else 4) + [0xDD, 0xDA]
    sub_eff = '4:4:4' if C == 1 else sub
    assert p['dri'] == (jpeg.default_restart_interval(C, sub_eff) if ri is None else ri)
    assert p['components'][0][1:3] == ((2, 2) if sub_eff == '4:2:0' else (1, 1))
    # the decoder's quantised coefficients are the host definition's, exactly
    zz, comp = jpeg.quantised_blocks(frame, q, sub_eff)
    assert len(p['scan_blocks']) == zz.shape[0]
    for k, (ci, nat) in enumerate(p['scan_blocks']):
        assert ci == comp[k]
        want = np.zeros([8, 8], np.int64)
        for i, cell in enumerate(jpeg_ref._ZZ):
            want[cell] = zz[k, i]
        assert np.array_equal(nat, want), (name, k)
    m, my, mx = jpeg.mcu_grid(H, W, C, sub_eff)
    assert len(p['rst']) == -(-(my * mx) // p['dri']) - 1 and p['rst'] == [i % 8 for i in range(len(p['rst']))]
    assert len(host_file(name)) - len(p['scan']) < 700 and len(p['scan']) <= jpeg.worst_case_bytes(H, W, C, sub_eff, p['dri'])
    # Pillow opens and fully loads it
    im = Image.open(io.BytesIO(host_file(name)))
    im.load()
    assert im.size == (W, H) and im.mode == ('L' if C == 1 else 'RGB')
    # the float64 decoder and Pillow's integer one agree on the picture (chroma up-sampling differs: replication here)
    mine = jpeg_ref.decode(host_file(name))[0]
    if sub_eff == '4:4:4':
        assert np.abs(mine.astype(int) - np.asarray(im).reshape(mine.shape).astype(int)).max() <= 2
    if sub_eff == '4:4:4' and q >= 85 and name not in ('stuffing', 'ac_max', 'dc_swing', 'zrl_no_eob'):          # only the quantiser's loss
        assert psnr(mine.reshape(frame.shape), frame) > 28, psnr(mine.reshape(frame.shape), frame)


def test_cases_cover_what_they_claim():
    cats = lambda name, kind: [t[1] for toks in parsed(name)['tokens'] for t in toks if t[0] == kind]
    dc = cats('dc_swing', 'dc')
    assert dc.count(11) >= 6
    scan_dc = [int(nat[0, 0]) for _, nat in parsed('dc_swing')['scan_blocks']]
    assert max(np.diff(scan_dc)) >= 1024 and min(np.diff(scan_dc)) <= -1024, 'category 11 with both signs'
    assert any(rs & 15 == 10 for rs in cats('ac_max', 'ac'))
    for toks in parsed('zrl_no_eob')['tokens']:
        ac = [t[1] for t in toks if t[0] == 'ac']
        assert ac.count(0xF0) == 3 and 0x00 not in ac and len(ac) == 4 and ac[-1] >> 4 == 14, ac
    assert all(nat[7, 7] != 0 for _, nat in parsed('zrl_no_eob')['scan_blocks'])
    assert b'\xff\x00' in parsed('stuffing')['scan']
    assert parsed('restart_wrap')['rst'] == [0, 1, 2, 3, 4, 5, 6, 7, 0, 1, 2]          # 12 intervals: indices 0..7 and 0..3, the last ends in EOI
    assert parsed('restart_wrap')['dri'] == 1
    p = parsed('restart_ragged')
    assert p['dri'] == 5 and len(p['rst']) == 2 and len(p['scan_blocks']) == 12 * 6
    # flat: after the first MCU of an interval nothing but DC-0 + EOB; intervals end mid-byte and are padded with 1-bits
    p = parsed('flat')
    per = 3 * p['dri']
    for k, toks in enumerate(p['tokens']):
        if k % per >= 3:
            assert toks == [('dc', 0), ('ac', 0)], (k, toks)
    assert any(n > 0 for n in p['pad_bits'])
    # the clamps of the tables
    assert max(parsed('q1')['qtables'][0]) == 255 and min(parsed('q1')['qtables'][0]) == 255 and set(parsed('q100')['qtables'][1]) == {1}
    # intervals longer than one pass of the device
    assert parsed('restart_long')['dri'] * 6 > jpeg.CHUNK_BLOCKS and parsed('one_interval')['rst'] == []


# ---- tables -----------------------------------------------------------------------------------------------------------------------

def _pillow_file(frame, **kw):
    buf = io.BytesIO()
    Image.fromarray(frame[..., 0] if frame.shape[2] == 1 else frame).save(buf, 'JPEG', **kw)
    return buf.getvalue()


@pytest.mark.parametrize('q', [1, 25, 50, 75, 90, 100])
def test_quantisation_tables_equal_pillows(q):
    frame = jpeg_cases.CASES['rgb_realistic'][0]
    theirs = Image.open(io.BytesIO(_pillow_file(frame, quality=q))).quantization
    assert list(theirs[0]) == jpeg.quant_table(jpeg.LUMA_Q, q).tolist()          # Pillow >= 8.3 returns natural order
    assert list(theirs[1]) == jpeg.quant_table(jpeg.CHROMA_Q, q).tolist()
    ours = Image.open(io.BytesIO(jpeg.encode_jpeg(torch.from_numpy(frame), q)[0])).quantization
    assert {k: list(v) for k, v in ours.items()} == {k: list(v) for k, v in theirs.items()}


def test_huffman_tables_equal_pillows():
    frame = jpeg_cases.CASES['rgb_realistic'][0]
    theirs = jpeg_ref.parse(_pillow_file(frame, quality=90, optimize=False))['dht']
    ours = parsed('rgb_realistic')['dht']
    assert sorted(ours) == [(0, 0), (0, 1), (1, 0), (1, 1)] and ours == theirs
    for name, key in (('dc_luma', (0, 0)), ('dc_chroma', (0, 1)), ('ac_luma', (1, 0)), ('ac_chroma', (1, 1))):
        assert (list(jpeg.STD_HUFFMAN[name][0]), list(jpeg.STD_HUFFMAN[name][1])) == theirs[key]


# ---- colour -----------------------------------------------------------------------------------------------------------------------

def test_colour_is_within_one_of_the_float64_formula_everywhere():
    g, b = np.meshgrid(np.arange(256), np.arange(256), indexing='ij')
    worst = 0
    for r in range(256):
        rgb = np.stack([np.full_like(g, r), g, b], axis=-1).astype(np.uint8)
        got = jpeg.rgb_to_ycbcr(rgb)
        R, G, B = float(r), g.astype(np.float64), b.astype(np.float64)
        want = np.stack([0.299 * R + 0.587 * G + 0.114 * B,
                         -0.168735892 * R - 0.331264108 * G + 0.5 * B + 128,
                         0.5 * R - 0.418687589 * G - 0.081312411 * B + 128], axis=-1)          # T.871: Cb = (B - Y) / 1.772 + 128, Cr = (R - Y) / 1.402 + 128
        want = np.clip(np.floor(want + 0.5), 0, 255)
        assert got.min() >= 0 and got.max() <= 255
        worst = max(worst, int(np.abs(got - want).max()))
    assert worst <= 1, worst


# ---- DCT and quantisation ---------------------------------------------------------------------------------------------------------

def _blocks():
    rng = np.random.RandomState(0)
    checker = np.where((np.arange(8)[:, None] + np.arange(8)[None, :]) & 1, 127, -128)
    d = jpeg_ref._idct_matrix()
    signs = [np.where(np.outer(d[v], d[u]) >= 0, 127, -128) for v in range(8) for u in range(8)]          # the extreme block of every coefficient
    smooth = np.rint(np.clip(60 * rng.randn(2000, 1, 1) + 25 * rng.randn(2000, 8, 1).cumsum(axis=1) + 3 * rng.randn(2000, 8, 8), -128, 127))
    return np.concatenate([rng.randint(-128, 128, size=[20000, 8, 8]), smooth, [np.full([8, 8], 127), np.full([8, 8], -128), checker, -1 - checker], signs]).astype(np.int64)


def test_dct_error_bound_and_quantiser_rounding():
    E = jpeg.DCT_ERROR_BOUND
    assert 0 < E <= 1
    blocks = _blocks()
    F = jpeg_ref.fdct_f64(blocks)
    F8 = jpeg.fdct8(blocks)
    err = np.abs(F8 / 8.0 - F).max()
    print(f'largest DCT error {err:.4f}, bound E = {E:.4f}')
    assert err <= E
    assert np.abs(F8).max() < 2 ** 15 and np.abs(F[:, 1:, 1:]).max() <= 1020 + 1e-9
    for q in (1, 2, 3, 7, 16, 99, 255):
        k = jpeg.quantise(F8.reshape(-1, 64), np.full(64, q))
        assert np.abs(k - F.reshape(-1, 64) / q).max() <= 0.5 + E / q          # for every coefficient of every block: a derived bound
    # half away from zero, on integers
    assert jpeg.quantise(np.array([4, -4, 3, -3, 12, -12, 11, -11, 0]), np.ones(9, np.int64)).tolist() == [1, -1, 0, 0, 2, -2, 1, -1, 0]
    assert jpeg.quantise(np.array([24, -24, 23, -23]), np.full(4, 3)).tolist() == [1, -1, 1, -1]
    assert jpeg.quantise(np.array([12, -12, 11, -11]), np.full(4, 3)).tolist() == [1, -1, 0, 0]


# ---- against Pillow's encoder -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('size', ['64x96', '128x256'])
@pytest.mark.parametrize('sub', ['4:4:4', '4:2:0'])
@pytest.mark.parametrize('q', [50, 90, 100])
def test_quality_and_size_against_pillows_encoder(size, sub, q):
    frame = jpeg_cases.CASES['rgb_realistic'][0] if size == '64x96' else jpeg_cases.realistic(128, 256, 3, 13)
    ri = jpeg.default_restart_interval(3, sub)
    ours = jpeg.encode_jpeg(torch.from_numpy(frame), q, sub)[0]
    theirs = _pillow_file(frame, quality=q, subsampling=sub, optimize=False, restart_marker_blocks=ri)
    assert jpeg_ref.parse(theirs)['dri'] == ri if size == '64x96' else True
    dec = lambda data: np.asarray(Image.open(io.BytesIO(data)))
    p_ours, p_theirs = psnr(dec(ours), frame), psnr(dec(theirs), frame)
    print(f'{size} {sub} q{q}: PSNR {p_ours:.3f} dB (Pillow {p_theirs:.3f}, {p_ours - p_theirs:+.3f}), {len(ours)} bytes (Pillow {len(theirs)}, '
          f'{100.0 * len(ours) / len(theirs) - 100:+.2f} %)')
    assert p_ours >= p_theirs - 0.1
    assert len(ours) <= len(theirs) * 1.01


# ---- container --------------------------------------------------------------------------------------------------------------------

def _five_frames():
    frames = [jpeg_cases.realistic(40, 56, 3, 20 + k) for k in range(5)]
    sizes = [len(f) for f in jpeg.encode_jpeg(torch.from_numpy(np.stack(frames)), 80, '4:2:0')]
    if not any(s & 1 for s in sizes):          # one frame with an odd JPEG length: a little more noise moves the size
        for seed in range(100, 200):
            frames[2] = jpeg_cases.realistic(40, 56, 3, seed)
            if len(jpeg.encode_jpeg(torch.from_numpy(frames[2]), 80, '4:2:0')[0]) & 1:
                break
    return [torch.from_numpy(f) for f in frames]


def test_avi_container(tmp_path):
    frames = _five_frames()
    files = jpeg.encode_jpeg(torch.stack(frames), 80, '4:2:0')
    assert any(len(f) & 1 for f in files) and any(not len(f) & 1 for f in files)
    path = str(tmp_path / 'a.avi')
    assert video_render.write_avi(frames, path, fps=24, quality=80, batch=2) == 5
    with open(path, 'rb') as f:
        data = f.read()
    a = jpeg_ref.parse_avi(data)
    assert a['riff_size'] == len(data) - 8
    assert a['avih'][4] == 5 and a['strh']['length'] == 5 and a['avih'][0] == 1000000 // 24
    assert (a['strh']['type'], a['strh']['handler'], a['strh']['scale'], a['strh']['rate']) == (b'vids', b'MJPG', 1, 24)
    assert a['avih'][8:10] == (56, 40) and a['strf'][1:6] == (56, 40, 1, 24, b'MJPG') and a['strh']['frame'] == (0, 0, 56, 40)
    assert [k for k, _, _ in a['lists']] == [b'hdrl', b'strl', b'movi']
    chunks = [c for c in a['chunks'] if c[1] == b'00dc']
    assert len(chunks) == 5 and len(a['idx1']) == 5 and len(a['chunks']) == 5
    for (cid, flags, at, size), (pos, _, csize), want in zip(a['idx1'], chunks, files):
        assert cid == b'00dc' and flags == 0x10 and a['movi'] + at == pos and size == csize == len(want)
        assert pos % 2 == 0, 'chunks start on even offsets'
        body = data[pos + 8:pos + 8 + size]
        assert body[:2] == b'\xff\xd8' and body[-2:] == b'\xff\xd9' and body == want
    info, got = video_render.read_avi(path)
    assert info == dict(width=56, height=40, fps=24.0, frames=5) and got == files
    for k, g in enumerate(got):
        im = Image.open(io.BytesIO(g)); im.load()
        theirs = _pillow_file(frames[k].numpy(), quality=80, subsampling='4:2:0', optimize=False)
        assert psnr(np.asarray(im), frames[k].numpy()) >= psnr(np.asarray(Image.open(io.BytesIO(theirs))), frames[k].numpy()) - 0.1


def test_writers_give_the_same_file(tmp_path):
    frames = _five_frames()
    a, b, c = (str(tmp_path / n) for n in ('a.avi', 'b.avi', 'c.avi'))
    video_render.write_avi(frames, a, fps=30, quality=80)
    with video_render.get_writer(b, mode='I', fps=30, codec='libx264', bitrate='10M', quality=80, batch=3) as w:
        for k, f in enumerate(frames):
            w.append_data(f.numpy() if k % 2 else f)          # numpy and tensor frames
    with pytest.raises(ValueError):
        w.append_data(frames[0])
    assert video_render.mimwrite(c, [f.numpy() for f in frames], fps=30, quality=8) == 5
    data = [open(p, 'rb').read() for p in (a, b, c)]
    assert data[0] == data[1] == data[2]
    # imageio's 0..10 scale -> 10 * quality clamped to 1..100
    for iq, jq in ((0, 1), (5, 50), (10, 100), (9.5, 95)):
        video_render.mimwrite(c, frames[:1], quality=iq)
        assert video_render.read_avi(c)[1][0] == jpeg.encode_jpeg(frames[0], jq)[0]
    grey = str(tmp_path / 'g.avi')
    assert video_render.write_avi([f[..., 0] for f in frames[:2]], grey) == 2
    assert Image.open(io.BytesIO(video_render.read_avi(grey)[1][1])).mode == 'L'
    with pytest.raises(ValueError):
        video_render.write_avi([frames[0], frames[0][:8]], grey)


def test_two_gib_guard(tmp_path, monkeypatch):
    frames = _five_frames()
    path = str(tmp_path / 'big.avi')
    video_render.write_avi(frames, path, quality=80, batch=1)
    size = os.path.getsize(path)
    monkeypatch.setattr(video_render, 'AVI_MAX_BYTES', size)
    video_render.write_avi(frames, path, quality=80, batch=1)          # exactly at the limit: written
    monkeypatch.setattr(video_render, 'AVI_MAX_BYTES', size - 1)
    with pytest.raises(ValueError, match='2 GiB'):
        video_render.write_avi(frames, path, quality=80, batch=1)
    info, got = video_render.read_avi(path)                            # what was written before the guard is a whole file
    assert info['frames'] == 4 and len(got) == 4 and jpeg_ref.parse_avi(open(path, 'rb').read())['riff_size'] == os.path.getsize(path) - 8


def test_arguments():
    f = torch.from_numpy(jpeg_cases.CASES['rgb_realistic'][0])
    for kw in (dict(quality=0), dict(quality=101), dict(subsampling='4:2:2'), dict(restart_interval=0), dict(restart_interval=65536)):
        with pytest.raises(ValueError):
            jpeg.encode_jpeg(f, **kw)
    for bad in (f.float(), f[..., :2], f[:0], torch.zeros([1, 1, 1, 1, 3], dtype=torch.uint8)):
        with pytest.raises(ValueError):
            jpeg.encode_jpeg(bad)
    assert jpeg.encode_jpeg(f[None])[0] == jpeg.encode_jpeg(f)[0]
    assert jpeg.worst_case_bytes(512, 1024, 3, '4:2:0', 5) == 409 * (2 * ((1658 * 30 + 7) // 8) + 2) + (2 * ((1658 * 18 + 7) // 8) + 2)


def test_save_jpeg(tmp_path):
    f = torch.from_numpy(np.stack([jpeg_cases.CASES['rgb_realistic'][0]] * 2))
    paths = [str(tmp_path / f'{k}.jpg') for k in range(2)]
    jpeg.save_jpeg(f, paths, quality=70)
    assert [open(p, 'rb').read() for p in paths] == jpeg.encode_jpeg(f, 70)
    jpeg.save_jpeg(f[0], paths[0])
    assert Image.open(paths[0]).size == (96, 64)
    with pytest.raises(ValueError):
        jpeg.save_jpeg(f, paths[:1])


def test_integration_note_names_the_patch():
    with open(os.path.join(ROOT, 'INTEGRATION.md')) as f:
        text = f.read()
    assert 'from training.video_render import get_writer, mimwrite' in text and 'gen_videos.py' in text and 'imageio.get_writer' in text


# ---- C ABI ------------------------------------------------------------------------------------------------------------------------

def test_c_abi_and_refusals():
    from torch_utils import hip_plugin
    with open(os.path.join(ROOT, 'include', 'ide3d_hip.h')) as f:
        h = f.read()
    six = r'\(int32_t n, int32_t h, int32_t w, int32_t c, int32_t subsampling, int32_t restart_interval\);'
    assert re.search(r'int64_t ide3d_jpeg_workspace_bytes' + six, h) and re.search(r'int64_t ide3d_jpeg_out_bytes' + six, h)
    assert re.search(r'int ide3d_jpeg_encode\(const uint8_t\* frames, int32_t n, int32_t h, int32_t w, int32_t c, int32_t quality, int32_t subsampling,\s*'
                     r'int32_t restart_interval, void\* workspace, int64_t workspace_bytes, uint8_t\* out, int64_t out_capacity,\s*'
                     r'int64_t\* offsets, void\* stream\);', h)
    assert 'gen_videos.py:108,131' in h
    path = hip_plugin.lib_path()
    assert os.path.isfile(path), f'{path} missing: run __graft_entry__.build()'
    lib, loaded = ctypes.CDLL(path), hip_plugin.load()
    for name in ('ide3d_jpeg_workspace_bytes', 'ide3d_jpeg_out_bytes', 'ide3d_jpeg_encode'):
        assert name in hip_plugin.EXPORTED_SYMBOLS and hasattr(lib, name), name
        m = re.search(r'(int64_t|int) %s\(([^)]*)\);' % name, h)
        assert len(getattr(loaded, name).argtypes) == len(m.group(2).split(',')), name
    assert hip_plugin.PLUGINS['jpeg_plugin'] is hip_plugin.JpegPlugin
    # host arithmetic only
    ws, ob = loaded.ide3d_jpeg_workspace_bytes, loaded.ide3d_jpeg_out_bytes
    for H, W, C, sub, ri in ((512, 1024, 3, '4:2:0', 5), (512, 1024, 3, '4:4:4', 10), (61, 45, 1, '4:4:4', 32), (17, 33, 3, '4:2:0', 65535), (96, 8, 3, '4:4:4', 1)):
        assert ob(3, H, W, C, jpeg.SUBSAMPLINGS[sub], ri) == 3 * jpeg.worst_case_bytes(H, W, C, sub, ri), (H, W, C, sub, ri)
    slot = (2 * ((1658 * 30 + 7) // 8) + 2 + 15) // 16 * 16
    T = 4 * 410
    assert ws(4, 512, 1024, 3, 420, 5) == T * slot + T * 4 + T * 8          # T * 4 is a multiple of 16 here
    assert ws(1, 1, 1, 1, 444, 65535) == 432 + 16 + 16                      # one block: 2 * 208 + 2 -> 432
    for bad in ((0, 8, 8, 3, 444, 1), (1, 0, 8, 3, 444, 1), (1, 8, 0, 3, 444, 1), (1, 8, 8, 2, 444, 1), (1, 8, 8, 4, 444, 1), (1, 8, 8, 3, 422, 1),
                (1, 8, 8, 1, 420, 1), (1, 8, 8, 3, 444, 0), (1, 8, 8, 3, 444, 65536), (1, 65536, 8, 3, 444, 1), (1, 8, 65536, 3, 444, 1),
                (1, 65535, 65535, 1, 444, 1), (64, 4096, 4096, 3, 420, 5)):
        assert ws(*bad) == -1 and ob(*bad) == -1, bad
    # every refusal comes before the first launch, so it needs no GPU; the pointers are never read
    buf = (ctypes.c_uint8 * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    enc = loaded.ide3d_jpeg_encode
    big = 1 << 30
    ok = (1, 8, 8, 3, 90, 444, 1)
    refused = {
        'channels': enc(p, 1, 8, 8, 2, 90, 444, 1, p, big, p, big, p, None), 'quality0': enc(p, 1, 8, 8, 3, 0, 444, 1, p, big, p, big, p, None),
        'quality101': enc(p, 1, 8, 8, 3, 101, 444, 1, p, big, p, big, p, None), 'subsampling': enc(p, 1, 8, 8, 3, 90, 422, 1, p, big, p, big, p, None),
        'grey420': enc(p, 1, 8, 8, 1, 90, 420, 1, p, big, p, big, p, None), 'restart0': enc(p, 1, 8, 8, 3, 90, 444, 0, p, big, p, big, p, None),
        'restart_big': enc(p, 1, 8, 8, 3, 90, 444, 65536, p, big, p, big, p, None), 'empty': enc(p, 1, 0, 8, 3, 90, 444, 1, p, big, p, big, p, None),
        'side': enc(p, 1, 8, 65536, 3, 90, 444, 1, p, big, p, big, p, None),
        'workspace': enc(p, *ok, p, ws(1, 8, 8, 3, 444, 1) - 1, p, big, p, None), 'out': enc(p, *ok, p, big, p, ob(1, 8, 8, 3, 444, 1) - 1, p, None),
        'out_2gib': enc(p, *ok, p, big, p, 1 << 31, p, None), 'null': enc(None, *ok, p, big, p, big, p, None),
        'huge': enc(p, 64, 4096, 4096, 3, 90, 420, 5, p, big, p, big, p, None),
    }
    assert all(rc == -1 for rc in refused.values()), refused
    assert b'jpeg_encode' in loaded.ide3d_last_error()
