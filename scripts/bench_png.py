"""Frames -> PNG files on one GPU (csrc/png.hip): `frames_u8` frames of the benchmark generator (512 x 1024 x 3:
RGB beside the palette-coloured segmentation) at batch 1 / 4 / 16 with segments of 16 and 32 KiB: ms per frame of the four launches
(device events), of `encode_png` as a caller sees it (the two copies to the host, CRC-32 and container included) and of the CRC-32 alone,
bytes per frame; beside it on this host PIL at compress levels 1 and 6 (skipped when PIL is absent) and zlib Z_RLE on the same filtered
stream.  Every timing is the median of BLOCKS blocks of REPS calls after warm-up, with the spread (min, max) of the blocks.
Prints one JSON line and writes it to profiles/png/bench_png.json."""
import io, json, os, statistics, sys, time, zlib
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'ide-3d_amd')); sys.path.insert(0, ROOT)
import numpy as np
import torch
from training import distributed_render as dr, png, triplane
from torch_utils import hip_plugin

dev = torch.device('cuda:0')
REPS, BLOCKS = 20, 5


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
res = {'frames': list(frames.shape), 'raw_bytes_per_frame': int(frames[0].numel())}

for seg_bytes in (16384, 32768):
    for batch in (1, 4, 16):
        fb = frames[:batch].contiguous()
        files = png.encode_png(fb, segment_bytes=seg_bytes)
        idat = [f[41:-16] for f in files]
        r = {'bytes_per_frame': round(sum(len(f) for f in files) / batch, 1),
             'launches_ms_per_frame': [round(v / batch, 5) for v in blocks(lambda: hip_plugin.PngPlugin.encode(fb, 5, seg_bytes), 'device')],
             'encode_png_wall_ms_per_frame': [round(v / batch, 5) for v in blocks(lambda: png.encode_png(fb, segment_bytes=seg_bytes), 'wall')],
             'crc32_ms_per_frame': [round(v / batch, 5) for v in host_blocks(lambda: [zlib.crc32(b'IDAT' + d) for d in idat], reps=9)]}
        r['frames_per_s_wall'] = round(1e3 / r['encode_png_wall_ms_per_frame'][0], 1)
        res[f'seg{seg_bytes // 1024}k_batch{batch}'] = r

# the same bytes as the host definition, and the frame back, on one frame (the host definition takes seconds at this size)
f0 = frames[0].cpu()
stream0, types0 = png.filter_rows(f0.numpy(), 5)
dev_file = png.encode_png(frames[:1])[0]
res['decodes_to_the_filtered_stream'] = zlib.decompress(dev_file[41:-16]) == stream0.tobytes()
res['equals_host_definition'] = dev_file == png.encode_png(f0)[0]
res['filter_types_share'] = [round(float((types0 == t).mean()), 3) for t in range(5)]

raw0 = stream0.tobytes()
def z_rle():
    c = zlib.compressobj(6, zlib.DEFLATED, 15, 8, zlib.Z_RLE)
    return c.compress(raw0) + c.flush()
res['host_zlib_rle_filtered_stream'] = {'bytes': len(z_rle()), 'ms': host_blocks(z_rle)}
res['host_zlib_level6_filtered_stream'] = {'bytes': len(zlib.compress(raw0, 6)), 'ms': host_blocks(lambda: zlib.compress(raw0, 6))}
try:
    from PIL import Image
except ImportError:
    Image = None
if Image is not None:
    im = Image.fromarray(f0.numpy())
    for level in (1, 6):
        def save():
            buf = io.BytesIO(); im.save(buf, format='png', compress_level=level); return buf.getvalue()
        res[f'host_pil_level{level}'] = {'bytes': len(save()), 'ms': host_blocks(save)}
    res['pil_reads_the_device_file'] = bool(np.array_equal(np.asarray(Image.open(io.BytesIO(dev_file))), f0.numpy()))
else:
    res['host_pil'] = 'PIL is not installed'

line = json.dumps(dict(metric='frames -> PNG files', device=torch.cuda.get_device_name(0), reps=REPS, blocks=BLOCKS, timing='[median, min, max] of the blocks',
                       **res, native_launches={k: c for k, c in hip_plugin.CALLS.items() if k.startswith('png')}))
print(line)
outdir = os.path.join(ROOT, 'profiles', 'png')
os.makedirs(outdir, exist_ok=True)
with open(os.path.join(outdir, 'bench_png.json'), 'w') as f:
    f.write(line + '\n')
