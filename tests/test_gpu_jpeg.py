"""csrc/jpeg.hip on the GPU against the host definition of training/jpeg.py: every case of tests/jpeg_cases.py
byte for byte and through Pillow, batches, repeatability, buffer guards, the refusals and one benchmark-sized frame through `write_avi`."""
import ctypes
import io

import numpy as np
import pytest
import torch
from PIL import Image

import jpeg_cases
from training import jpeg, video_render

pytestmark = pytest.mark.gpu

_host = {}


def host_file(name):
    """The host definition's file of a case, computed once."""
    if name not in _host:
        frame, q, sub, ri = jpeg_cases.CASES[name]
        _host[name] = jpeg.encode_jpeg(torch.from_numpy(frame), q, sub, ri)[0]
    return _host[name]


def psnr(a, b):
    mse = np.mean((a.astype(np.float64) - b.astype(np.float64)) ** 2)
    return 10 * np.log10(255.0 ** 2 / mse) if mse > 0 else np.inf


@pytest.mark.parametrize('name', sorted(jpeg_cases.CASES))
def test_case_equals_host_definition_and_decodes(gpu_device, name):
    from torch_utils import hip_plugin
    frame, q, sub, ri = jpeg_cases.CASES[name]
    before = hip_plugin.CALLS.get('jpeg_encode', 0)
    got = jpeg.encode_jpeg(torch.from_numpy(frame).to(gpu_device), q, sub, ri)
    assert hip_plugin.CALLS.get('jpeg_encode', 0) == before + 1
    assert len(got) == 1
    im = Image.open(io.BytesIO(got[0]))
    im.load()
    assert im.size == (frame.shape[1], frame.shape[0]) and im.mode == ('L' if frame.shape[2] == 1 else 'RGB')
    assert got[0] == host_file(name)


def _three_frames():
    return np.stack([jpeg_cases.realistic(33, 70, 3, 31), np.random.RandomState(32).randint(0, 256, size=[33, 70, 3]).astype(np.uint8),
                     np.full([33, 70, 3], 77, np.uint8)])


@pytest.mark.parametrize('sub,ri', [('4:2:0', None), ('4:4:4', 7)])
def test_batch_equals_single_calls_and_repeats(gpu_device, sub, ri):
    frames = torch.from_numpy(_three_frames()).to(gpu_device)
    batch = jpeg.encode_jpeg(frames, 92, sub, ri)
    single = [jpeg.encode_jpeg(frames[k], 92, sub, ri)[0] for k in range(3)]
    assert batch == single
    assert jpeg.encode_jpeg(frames, 92, sub, ri) == batch
    assert batch == jpeg.encode_jpeg(frames.cpu(), 92, sub, ri)


def test_buffers_are_written_only_inside_their_views(gpu_device):
    from torch_utils import hip_plugin
    frame, q, sub, ri = jpeg_cases.CASES['stuffing']          # noise at quality 100: the case nearest the worst-case slot
    frames = torch.from_numpy(np.stack([frame, frame[::-1].copy(), frame[:, ::-1].copy()])).to(gpu_device)
    N, H, W, C = frames.shape
    ri = jpeg.default_restart_interval(C, sub)
    lib = hip_plugin.load()
    args = (N, H, W, C, jpeg.SUBSAMPLINGS[sub], ri)
    ws_bytes, out_bytes = lib.ide3d_jpeg_workspace_bytes(*args), lib.ide3d_jpeg_out_bytes(*args)
    assert out_bytes == N * jpeg.worst_case_bytes(H, W, C, sub, ri)
    pad, mis = 4096, 16 + 5          # the out view starts 5 bytes past a 16-byte boundary
    big_ws = torch.full([ws_bytes + 2 * pad], 0xA5, dtype=torch.uint8, device=gpu_device)
    big_out = torch.full([out_bytes + 2 * pad + mis], 0xA5, dtype=torch.uint8, device=gpu_device)
    big_off = torch.full([N + 1 + 8], -7, dtype=torch.int64, device=gpu_device)
    ws, out, off = big_ws[pad:pad + ws_bytes], big_out[pad + mis:pad + mis + out_bytes], big_off[4:4 + N + 1]
    hip_plugin.JpegPlugin.launch(frames, q, jpeg.SUBSAMPLINGS[sub], ri, ws, out, off)
    torch.cuda.synchronize()
    assert bool((big_ws[:pad] == 0xA5).all()) and bool((big_ws[pad + ws_bytes:] == 0xA5).all())
    assert bool((big_out[:pad + mis] == 0xA5).all()) and bool((big_out[pad + mis + out_bytes:] == 0xA5).all())
    assert bool((big_off[:4] == -7).all()) and bool((big_off[4 + N + 1:] == -7).all())
    ends = off.tolist()
    assert ends[0] == 0 and ends[-1] <= out_bytes
    assert bool((out[ends[-1]:] == 0xA5).all()), 'nothing is written past the last scan'
    raw = out[:ends[-1]].cpu().numpy().tobytes()
    want = jpeg.encode_scans(frames.cpu(), q, sub, ri)
    assert [raw[ends[k]:ends[k + 1]] for k in range(N)] == want
    assert sum(s.count(b'\xff\x00') for s in want) > 20


@pytest.mark.parametrize('N', [1, 2])
def test_more_intervals_than_scan_threads(gpu_device, N):
    """Grey frames of 8 x 8800 with a restart interval of one MCU: 1100 intervals per frame, so one frame is more intervals than the
    position scan has threads (not a multiple of them) and two frames are three sizes per thread, with the marker term (2 bytes per RSTm)
    and the frame term both live.  Every interval is copied to a destination of its own residue modulo 16 (the out view starts 5 bytes
    past a 16-byte boundary).  The scans equal the host definition, `offsets` their running lengths, and the guards hold."""
    from torch_utils import hip_plugin
    frames = torch.from_numpy(np.stack([jpeg_cases.realistic(8, 8800, 1, 40 + k) for k in range(N)])).to(gpu_device)
    q, sub, ri = 90, '4:4:4', 1
    lib = hip_plugin.load()
    args = (N, 8, 8800, 1, jpeg.SUBSAMPLINGS[sub], ri)
    ws_bytes, out_bytes = lib.ide3d_jpeg_workspace_bytes(*args), lib.ide3d_jpeg_out_bytes(*args)
    pad, mis = 4096, 16 + 5
    big_ws = torch.full([ws_bytes + 2 * pad], 0xA5, dtype=torch.uint8, device=gpu_device)
    big_out = torch.full([out_bytes + 2 * pad + mis], 0xA5, dtype=torch.uint8, device=gpu_device)
    big_off = torch.full([N + 1 + 8], -7, dtype=torch.int64, device=gpu_device)
    ws, out, off = big_ws[pad:pad + ws_bytes], big_out[pad + mis:pad + mis + out_bytes], big_off[4:4 + N + 1]
    assert out.data_ptr() % 16 == 5
    hip_plugin.JpegPlugin.launch(frames, q, jpeg.SUBSAMPLINGS[sub], ri, ws, out, off)
    torch.cuda.synchronize()
    assert bool((big_ws[:pad] == 0xA5).all()) and bool((big_ws[pad + ws_bytes:] == 0xA5).all())
    assert bool((big_out[:pad + mis] == 0xA5).all()) and bool((big_out[pad + mis + out_bytes:] == 0xA5).all())
    assert bool((big_off[:4] == -7).all()) and bool((big_off[4 + N + 1:] == -7).all())
    want = jpeg.encode_scans(frames.cpu(), q, sub, ri)
    assert all(s.count(b'\xff\xd0') + s.count(b'\xff\xd7') >= 2 * (1100 // 8) for s in want)          # the restart markers are there
    ends = off.tolist()
    assert ends == [sum(len(s) for s in want[:k]) for k in range(N + 1)]
    assert bool((out[ends[-1]:] == 0xA5).all()), 'nothing is written past the last scan'
    raw = out[:ends[-1]].cpu().numpy().tobytes()
    assert [raw[ends[k]:ends[k + 1]] for k in range(N)] == want


def test_refusals_launch_nothing(gpu_device):
    from torch_utils import hip_plugin
    lib = hip_plugin.load()
    frames = torch.zeros([2, 8, 8, 3], dtype=torch.uint8, device=gpu_device)
    ws_bytes, out_bytes = lib.ide3d_jpeg_workspace_bytes(2, 8, 8, 3, 444, 1), lib.ide3d_jpeg_out_bytes(2, 8, 8, 3, 444, 1)
    ws = torch.full([ws_bytes + 16], 0xA5, dtype=torch.uint8, device=gpu_device)
    out = torch.full([out_bytes], 0xA5, dtype=torch.uint8, device=gpu_device)
    off = torch.full([3], -7, dtype=torch.int64, device=gpu_device)
    p = lambda t, o=0: ctypes.c_void_p(t.data_ptr() + o)

    def call(n=2, h=8, w=8, c=3, q=90, sub=444, ri=1, wsp=None, wsb=ws_bytes, outb=out_bytes):
        return lib.ide3d_jpeg_encode(p(frames), n, h, w, c, q, sub, ri, p(ws) if wsp is None else wsp, wsb, p(out), outb, p(off), None)

    bad = dict(channels=call(c=2), channels4=call(c=4), quality0=call(q=0), quality101=call(q=101), subsampling=call(sub=422), grey420=call(c=1, sub=420),
               restart0=call(ri=0), restart_big=call(ri=65536), empty=call(h=0), side=call(w=65536), workspace=call(wsb=ws_bytes - 1),
               out=call(outb=out_bytes - 1), aligned=call(wsp=p(ws, 8)), huge=call(n=64, h=4096, w=4096, sub=420, ri=5))
    assert all(rc == -1 for rc in bad.values()), bad
    torch.cuda.synchronize()
    assert bool((ws == 0xA5).all()) and bool((out == 0xA5).all()) and bool((off == -7).all())
    assert call() == 0
    torch.cuda.synchronize()
    with pytest.raises(RuntimeError):
        hip_plugin.JpegPlugin.encode(frames[..., :2].contiguous(), 90, 444, 1)
    with pytest.raises(ValueError):
        jpeg.encode_jpeg(frames, quality=0)


def test_benchmark_frame_through_write_avi(gpu_device, tmp_path):
    """A frame of the benchmark generator (512 x 1024 x 3: RGB beside the palette-coloured segmentation) -> write_avi -> read_avi ->
    Pillow: as good as Pillow's own encoding of the frame to 0.1 dB, and the device's bytes are the host definition's."""
    from training import distributed_render as dr, triplane
    torch.manual_seed(0)
    G = triplane.TriPlaneGenerator().eval().to(gpu_device)
    z = torch.from_numpy(np.random.RandomState(0).randn(1, G.z_dim)).float().to(gpu_device)
    with torch.no_grad():
        img, seg = G.synthesis(G.mapping(z, triplane.conditioning_label(gpu_device)), c=triplane.camera_label(0.3, device=gpu_device), noise_mode='const',
                               return_seg=True)
    frame = dr.frames_u8(img, seg, dr.palette_tensor(G.spec.seg_channels, gpu_device))[0]
    assert tuple(frame.shape) == (512, 1024, 3) and frame.dtype == torch.uint8
    path = str(tmp_path / 'frame.avi')
    assert video_render.write_avi([frame], path) == 1
    info, files = video_render.read_avi(path)
    assert info == dict(width=1024, height=512, fps=60.0, frames=1) and len(files) == 1
    host = frame.cpu()
    assert files[0] == jpeg.encode_jpeg(host)[0]
    ours = np.asarray(Image.open(io.BytesIO(files[0])))
    buf = io.BytesIO()
    Image.fromarray(host.numpy()).save(buf, 'JPEG', quality=90, subsampling='4:2:0', optimize=False, restart_marker_blocks=jpeg.default_restart_interval(3, '4:2:0'))
    theirs = np.asarray(Image.open(io.BytesIO(buf.getvalue())))
    p_ours, p_theirs = psnr(ours, host.numpy()), psnr(theirs, host.numpy())
    print(f'PSNR {p_ours:.3f} dB (Pillow {p_theirs:.3f}), {len(files[0])} bytes (Pillow {len(buf.getvalue())}), raw {host.numel()}')
    assert p_ours >= p_theirs - 0.1
