"""csrc/png.hip on the GPU against the host definition of training/png.py: every case of tests/png_cases.py
byte for byte and through the independent decoder of tests/png_ref.py, batches, repeatability, buffer guards, the refusals and one
end-to-end frame of the tiny generator."""
import ctypes

import numpy as np
import pytest
import torch

import png_cases
import png_ref
from training import png

pytestmark = pytest.mark.gpu

_host = {}


def host_file(name):
    """The host definition's file of a case, computed once."""
    if name not in _host:
        frame, filt, seg = png_cases.CASES[name]
        _host[name] = png.encode_png(torch.from_numpy(frame), filt, seg)[0]
    return _host[name]


@pytest.mark.parametrize('name', sorted(png_cases.CASES))
def test_case_equals_host_definition_and_decodes(gpu_device, name):
    from torch_utils import hip_plugin
    frame, filt, seg = png_cases.CASES[name]
    before = hip_plugin.CALLS.get('png_encode', 0)
    got = png.encode_png(torch.from_numpy(frame).to(gpu_device), filt, seg)
    assert hip_plugin.CALLS.get('png_encode', 0) == before + 1
    assert len(got) == 1
    img, types, _ = png_ref.decode(got[0])
    assert np.array_equal(img, frame)
    if filt != 'adaptive':
        assert (types == png.FILTERS[filt]).all()
    assert got[0] == host_file(name)


def _three_frames():
    rng = np.random.RandomState(11)
    a = png_cases.noisy_gradient(33, 70, 3, 8)
    b = np.repeat(np.repeat(rng.randint(0, 19, size=[3, 7, 1]).astype(np.uint8) * 11, 11, axis=0), 10, axis=1).repeat(3, axis=2)
    c = rng.randint(0, 256, size=[33, 70, 3]).astype(np.uint8)
    return np.stack([a, b, c])


def test_batch_equals_single_calls_and_repeats(gpu_device):
    frames = torch.from_numpy(_three_frames()).to(gpu_device)
    batch = png.encode_png(frames, 'adaptive', 1024)
    single = [png.encode_png(frames[k], 'adaptive', 1024)[0] for k in range(3)]
    assert batch == single
    assert png.encode_png(frames, 'adaptive', 1024) == batch
    for k in range(3):
        assert np.array_equal(png_ref.decode(batch[k])[0], frames[k].cpu().numpy())
        assert batch[k] == png.encode_png(frames[k].cpu(), 'adaptive', 1024)[0]


def test_buffers_are_written_only_inside_their_views(gpu_device):
    from torch_utils import hip_plugin
    frames = torch.from_numpy(_three_frames()).to(gpu_device)
    N, H, W, C = frames.shape
    lib = hip_plugin.load()
    ws_bytes, out_bytes = lib.ide3d_png_workspace_bytes(N, H, W, C, 1024), lib.ide3d_png_out_bytes(N, H, W, C, 1024)
    assert out_bytes == N * (H * (W * C + 1) + 5 * -(-H * (W * C + 1) // 1024) + 6)
    pad, mis = 4096, 16 + 5          # the out view starts 5 bytes past a 16-byte boundary
    big_ws = torch.full([ws_bytes + 2 * pad], 0xA5, dtype=torch.uint8, device=gpu_device)
    big_out = torch.full([out_bytes + 2 * pad + mis], 0xA5, dtype=torch.uint8, device=gpu_device)
    big_off = torch.full([N + 1 + 8], -7, dtype=torch.int64, device=gpu_device)
    ws, out, off = big_ws[pad:pad + ws_bytes], big_out[pad + mis:pad + mis + out_bytes], big_off[4:4 + N + 1]
    hip_plugin.PngPlugin.launch(frames, 5, 1024, ws, out, off)
    torch.cuda.synchronize()
    assert bool((big_ws[:pad] == 0xA5).all()) and bool((big_ws[pad + ws_bytes:] == 0xA5).all())
    assert bool((big_out[:pad + mis] == 0xA5).all()) and bool((big_out[pad + mis + out_bytes:] == 0xA5).all())
    assert bool((big_off[:4] == -7).all()) and bool((big_off[4 + N + 1:] == -7).all())
    ends = off.tolist()
    assert ends[0] == 0 and ends[-1] <= out_bytes
    assert bool((out[ends[-1]:] == 0xA5).all()), 'nothing is written past the last stream'
    raw = out[:ends[-1]].cpu().numpy().tobytes()
    want = png.encode_zlib(frames.cpu(), 'adaptive', 1024)
    assert [raw[ends[k]:ends[k + 1]] for k in range(N)] == want


def _guarded_streams(frames, mode, seg):
    """PngPlugin.launch into views of buffers filled with a pattern, the out view 5 bytes past a 16-byte boundary -> the streams, after
    checking that nothing outside the views or past the last stream was written."""
    from torch_utils import hip_plugin
    N, H, W, C = frames.shape
    lib = hip_plugin.load()
    ws_bytes, out_bytes = lib.ide3d_png_workspace_bytes(N, H, W, C, seg), lib.ide3d_png_out_bytes(N, H, W, C, seg)
    pad, mis = 4096, 16 + 5
    big_ws = torch.full([ws_bytes + 2 * pad], 0xA5, dtype=torch.uint8, device=frames.device)
    big_out = torch.full([out_bytes + 2 * pad + mis], 0xA5, dtype=torch.uint8, device=frames.device)
    big_off = torch.full([N + 1 + 8], -7, dtype=torch.int64, device=frames.device)
    ws, out, off = big_ws[pad:pad + ws_bytes], big_out[pad + mis:pad + mis + out_bytes], big_off[4:4 + N + 1]
    assert out.data_ptr() % 16 == 5
    hip_plugin.PngPlugin.launch(frames, mode, seg, ws, out, off)
    torch.cuda.synchronize()
    assert bool((big_ws[:pad] == 0xA5).all()) and bool((big_ws[pad + ws_bytes:] == 0xA5).all())
    assert bool((big_out[:pad + mis] == 0xA5).all()) and bool((big_out[pad + mis + out_bytes:] == 0xA5).all())
    assert bool((big_off[:4] == -7).all()) and bool((big_off[4 + N + 1:] == -7).all())
    ends = off.tolist()
    assert ends[0] == 0 and ends[-1] <= out_bytes and ends == sorted(ends)
    assert bool((out[ends[-1]:] == 0xA5).all()), 'nothing is written past the last stream'
    raw = out[:ends[-1]].cpu().numpy().tobytes()
    return [raw[ends[k]:ends[k + 1]] for k in range(N)]


def test_more_segments_than_scan_threads(gpu_device):
    """3 frames of 361 x 1024 x 1, filter 'none', segments of 1024 bytes: a frame's filtered stream is 361 x 1025 bytes = 362 segments, the
    batch 1086: two sizes per thread of the position scan, its last threads idle; a single frame is one size per thread.  The batch equals
    the single calls, every stream inflates to the frame's filtered rows, one equals the host definition, and the guards hold."""
    import zlib
    frames_np = np.stack([png_cases.noisy_gradient(361, 1024, 1, 20 + k) for k in range(3)])
    assert -(-361 * 1025 // 1024) == 362 and 3 * 362 > 1024 and (3 * 362) % 1024 != 0
    frames = torch.from_numpy(frames_np).to(gpu_device)
    batch = _guarded_streams(frames, png.FILTERS['none'], 1024)
    single = [_guarded_streams(frames[k:k + 1].contiguous(), png.FILTERS['none'], 1024)[0] for k in range(3)]
    assert batch == single
    for k in range(3):
        assert zlib.decompress(batch[k]) == png.filter_rows(frames_np[k], png.FILTERS['none'])[0].tobytes()
    assert batch[1] == png.zlib_stream(frames_np[1], png.FILTERS['none'], 1024)


def test_refusals_launch_nothing(gpu_device):
    from torch_utils import hip_plugin
    lib = hip_plugin.load()
    frames = torch.zeros([2, 8, 8, 3], dtype=torch.uint8, device=gpu_device)
    ws_bytes, out_bytes = lib.ide3d_png_workspace_bytes(2, 8, 8, 3, 1024), lib.ide3d_png_out_bytes(2, 8, 8, 3, 1024)
    ws = torch.full([ws_bytes + 16], 0xA5, dtype=torch.uint8, device=gpu_device)
    out = torch.full([out_bytes], 0xA5, dtype=torch.uint8, device=gpu_device)
    off = torch.full([3], -7, dtype=torch.int64, device=gpu_device)
    p = lambda t, o=0: ctypes.c_void_p(t.data_ptr() + o)

    def call(n=2, h=8, w=8, c=3, mode=5, seg=1024, wsp=None, wsb=ws_bytes, outb=out_bytes):
        return lib.ide3d_png_encode(p(frames), n, h, w, c, mode, seg, p(ws) if wsp is None else wsp, wsb, p(out), outb, p(off), None)

    bad = dict(channels=call(c=2), channels4=call(c=4), seg_small=call(seg=512), seg_large=call(seg=65536), seg_pow2=call(seg=3000),
               mode=call(mode=6), empty=call(h=0), workspace=call(wsb=ws_bytes - 1), out=call(outb=out_bytes - 1), aligned=call(wsp=p(ws, 8)),
               huge=call(n=4, h=32768, w=16384))
    assert all(rc == -1 for rc in bad.values()), bad
    assert lib.ide3d_png_workspace_bytes(4, 32768, 16384, 3, 32768) == -1 and lib.ide3d_png_out_bytes(1, 8, 8, 2, 1024) == -1
    torch.cuda.synchronize()
    assert bool((ws == 0xA5).all()) and bool((out == 0xA5).all()) and bool((off == -7).all())
    assert call() == 0
    with pytest.raises(RuntimeError):
        hip_plugin.PngPlugin.encode(frames[..., :2].contiguous(), 5, 1024)
    with pytest.raises(ValueError):
        png.encode_png(frames, 'adaptive', 2048 + 1)


def test_generator_frames_to_files(gpu_device, tmp_path):
    """`frames_u8` of the tiny generator -> `save_png` -> the files decode to the tensor."""
    from training import distributed_render as dr, triplane
    torch.manual_seed(0)
    G = triplane.TriPlaneGenerator(triplane.tiny_spec()).eval().to(gpu_device)
    z = torch.from_numpy(np.random.RandomState(0).randn(2, G.z_dim)).to(gpu_device)
    c = torch.cat([triplane.camera_label(-0.4), triplane.camera_label(0.3)]).to(gpu_device)
    with torch.no_grad():
        ws = G.mapping(z, triplane.conditioning_label(gpu_device).repeat(2, 1))
        img, seg = G.synthesis(ws, c=c, noise_mode='const', return_seg=True)
    frames = dr.frames_u8(img, seg)
    assert frames.dtype == torch.uint8 and frames.ndim == 4 and frames.shape[0] == 2 and frames.shape[3] == 3
    paths = [str(tmp_path / f'seed{k:04d}.png') for k in range(2)]
    png.save_png(frames, paths)
    for k, path in enumerate(paths):
        with open(path, 'rb') as f:
            data = f.read()
        assert np.array_equal(png_ref.decode(data)[0], frames[k].cpu().numpy())
        assert data == png.encode_png(frames[k].cpu())[0]
