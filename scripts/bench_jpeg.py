"""Frames -> JPEG files and Motion-JPEG AVI on one GPU (csrc/jpeg.hip): `frames_u8` frames of the benchmark
generator (512 x 1024 x 3: RGB beside the palette-coloured segmentation) at quality 90, 4:2:0, batch 1 / 4 / 16: ms per frame of the three
launches (device events) and of `encode_jpeg` as a caller sees it (the two copies to the host and the markers included), bytes copied to
the host per frame against the raw frame; a 240-frame turntable of those frames through `write_avi` against `write_y4m`; beside it on
this host Pillow's `save(..., 'JPEG')` on one core.  Every timing is the median of BLOCKS blocks of REPS calls after warm-up, with the
spread (min, max) of the blocks.  Prints one JSON line and writes it to profiles/jpeg/bench_jpeg.json."""
import io, json, os, statistics, sys, tempfile, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'ide-3d_amd')); sys.path.insert(0, ROOT)
import numpy as np
import torch
from training import distributed_render as dr, jpeg, triplane, video_render
from torch_utils import hip_plugin

dev = torch.device('cuda:0')
REPS, BLOCKS = 20, 5
QUALITY, SUB = 90, '4:2:0'
RI = jpeg.default_restart_interval(3, SUB)


def blocks(fn, clock):
    """[median, min, max] of BLOCKS blocks of REPS calls, ms per call; `clock`: 'device' (events) or 'wall' (host clock, device idle at both ends)."""
    for _ in range(5):
        fn()
    out = []
    for _ in range(BLOCKS):
        if clock == 'device':
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize(); a.record()
            for _ in range(REPS):
                fn()
            b.record(); torch.cuda.synchronize()
            out.append(a.elapsed_time(b) / REPS)
        else:
            torch.cuda.synchronize(); t0 = time.perf_counter()
            for _ in range(REPS):
                fn()
            torch.cuda.synchronize()
            out.append((time.perf_counter() - t0) / REPS * 1e3)
    return [round(statistics.median(out), 4), round(min(out), 4), round(max(out), 4)]


def host_blocks(fn, reps=3):
    out = []
    for _ in range(reps):
        t0 = time.perf_counter(); fn(); out.append((time.perf_counter() - t0) * 1e3)
    return [round(statistics.median(out), 3), round(min(out), 3), round(max(out), 3)]


torch.manual_seed(0)
G = triplane.TriPlaneGenerator().eval().to(dev)
palette = dr.palette_tensor(G.spec.seg_channels, dev)
cond = triplane.conditioning_label(dev).repeat(4, 1)
chunks = []
with torch.no_grad():
    for k in range(4):
        z = torch.from_numpy(np.stack([np.random.RandomState(4 * k + j).randn(G.spec.z_dim) for j in range(4)])).float().to(dev)
        cams = torch.cat([triplane.camera_label(y, device=dev) for y in (-0.45, -0.15, 0.15, 0.45)])
        img, seg = G.synthesis(G.mapping(z, cond), c=cams, noise_mode='const', return_seg=True)
        chunks.append(dr.frames_u8(img, seg, palette))
frames = torch.cat(chunks).contiguous()
raw = int(frames[0].numel())
res = {'frames': list(frames.shape), 'quality': QUALITY, 'subsampling': SUB, 'restart_interval': RI, 'raw_bytes_per_frame': raw}

for batch in (1, 4, 16):
    fb = frames[:batch].contiguous()
    files = jpeg.encode_jpeg(fb, QUALITY, SUB)
    scans = jpeg.encode_scans(fb, QUALITY, SUB)
    copied = sum(len(s) for s in scans) / batch + 8 * (batch + 1) / batch
    r = {'bytes_per_frame': round(sum(len(f) for f in files) / batch, 1), 'bytes_copied_to_host_per_frame': round(copied, 1),
         'raw_over_copied': round(raw / copied, 1),
         'launches_ms_per_frame': [round(v / batch, 5) for v in blocks(lambda: hip_plugin.JpegPlugin.encode(fb, QUALITY, 420, RI), 'device')],
         'encode_jpeg_wall_ms_per_frame': [round(v / batch, 5) for v in blocks(lambda: jpeg.encode_jpeg(fb, QUALITY, SUB), 'wall')]}
    r['frames_per_s_wall'] = round(1e3 / r['encode_jpeg_wall_ms_per_frame'][0], 1)
    res[f'batch{batch}'] = r

# the same bytes as the host definition, and Pillow reads them
f0 = frames[0].cpu()
dev_file = jpeg.encode_jpeg(frames[:1], QUALITY, SUB)[0]
res['equals_host_definition'] = dev_file == jpeg.encode_jpeg(f0, QUALITY, SUB)[0]
from PIL import Image
psnr = lambda a, b: float(10 * np.log10(255.0 ** 2 / np.mean((a.astype(np.float64) - b.astype(np.float64)) ** 2)))
im = Image.fromarray(f0.numpy())
def save():
    buf = io.BytesIO(); im.save(buf, 'JPEG', quality=QUALITY, subsampling=SUB, optimize=False, restart_marker_blocks=RI); return buf.getvalue()
res['host_pillow_one_core'] = {'bytes': len(save()), 'ms': host_blocks(save, reps=9), 'psnr_db': round(psnr(np.asarray(Image.open(io.BytesIO(save()))), f0.numpy()), 3)}
res['device_file_psnr_db'] = round(psnr(np.asarray(Image.open(io.BytesIO(dev_file))), f0.numpy()), 3)

# a 240-frame turntable: the 16 frames in turn, through both video sinks (host clock, file writes included)
turntable = [frames[k % 16] for k in range(240)]
with tempfile.TemporaryDirectory() as tmp:
    for name, fn in (('write_avi', lambda p: video_render.write_avi(turntable, p)), ('write_avi_batch16', lambda p: video_render.write_avi(turntable, p, batch=16)),
                     ('write_y4m', lambda p: video_render.write_y4m(turntable, p))):
        path = os.path.join(tmp, name)
        fn(path)                                     # warm-up
        ms = []
        for _ in range(3):
            torch.cuda.synchronize(); t0 = time.perf_counter(); fn(path); torch.cuda.synchronize(); ms.append((time.perf_counter() - t0) * 1e3)
        res[f'turntable240_{name}'] = {'ms': [round(statistics.median(ms), 1), round(min(ms), 1), round(max(ms), 1)], 'file_bytes': os.path.getsize(path)}

def clock_under_load():
    """GPU 0's clocks as `rocm-smi --showclocks --json` reads them while batch-16 encodes are queued (read only; None without the tool)."""
    import shutil, subprocess
    exe = shutil.which('rocm-smi') or '/opt/rocm/bin/rocm-smi'
    if not os.path.exists(exe):
        return None
    try:
        fb = frames[:16].contiguous()
        for _ in range(300):
            hip_plugin.JpegPlugin.encode(fb, QUALITY, 420, RI)
        out = subprocess.run([exe, '--showclocks', '--json'], capture_output=True, text=True, timeout=20)
        torch.cuda.synchronize()
        card = next(iter(json.loads(out.stdout).values()))
        return {k.lower().split()[0] + '_mhz': v.strip('()').replace('Mhz', '').replace('MHz', '') for k, v in card.items()
                if ('sclk' in k.lower() or 'mclk' in k.lower()) and 'speed' in k.lower()}
    except Exception as e:      # noqa: BLE001 - diagnostics only
        return {'error': f'{type(e).__name__}: {e}'[:120]}


res['gpu_clock'] = clock_under_load()
line = json.dumps(dict(metric='frames -> JPEG files / Motion-JPEG AVI', device=torch.cuda.get_device_name(0), reps=REPS, blocks=BLOCKS,
                       timing='[median, min, max] of the blocks', **res, native_launches={k: c for k, c in hip_plugin.CALLS.items() if k.startswith('jpeg')}))
print(line)
outdir = os.path.join(ROOT, 'profiles', 'jpeg')
os.makedirs(outdir, exist_ok=True)
with open(os.path.join(outdir, 'bench_jpeg.json'), 'w') as f:
    f.write(line + '\n')
