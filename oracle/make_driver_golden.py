"""Generate tests/golden/drivers.npz by running the REFERENCE's untouched driver code on the overlay (build container only).

    python oracle/make_driver_golden.py [reference checkout, default $IDE3D_REFERENCE or /root/reference]

Two child interpreters with `sys.path = [overlay, reference]`, i.e. `torch_utils` / `training` / `dnnlib` resolve to this repository and
everything the overlay does not carry (`legacy`, `dnnlib.seg_tools`, `gen_videos`, `extract_shapes`, ...) to the reference checkout:

  * the REFERENCE's `legacy.load_network_pkl` (legacy.py:22-42) loads `scripts/make_random_init_pkl.py --tiny`, and the call sequence
    of gen_images.py:85-111 runs verbatim on it (2 seeds x 3 yaws): `seq_cam` (the camera labels it builds), `seq_img_*` / `seq_seg_*`
    (a fixed quarter of every render's values, see `reduce`);
  * gen_videos.py:66-139 (2 frames of a 2 x 2 `image_seg` grid) and extract_shapes.py:99-150 (32^3 cube, and its sample lattice) on
    `--tiny52`, without stratified jitter: `video_frames`, `cube`, `lattice_*` (the lattice as a SHA-256 of its bytes), `lattice_origin`,
    `lattice_voxel_size`.

How the reference's modules bind to the overlay (which package each import resolves to, the face parser behind dnnlib/seg_tools.py, the
video writer's arguments) is asserted here, while the fixtures are made.  tests/test_reference_drivers_cpu.py compares the product with
the stored outputs.  Modules the image lacks and the drivers import at module level (cv2, torchvision, imageio, plyfile, mrcfile,
skimage, numpy-1 private modules) are stubbed as oracle/ref_import.py does.  TEST INFRASTRUCTURE ONLY.
"""

import os
import subprocess
import sys
import tempfile
import textwrap

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, 'tests', 'golden', 'drivers.npz')
SEQ_SAMPLE_FRACTION = 4          # one in four values of every recorded render is stored

STUBS = r'''
import math, os, sys, types
overlay, ref, pkl, out = sys.argv[1], sys.argv[2], sys.argv[3], sys.argv[4]
sys.path[:0] = [overlay, ref]
import numpy as np, numpy.lib
for name, attrs in (('arraysetops', dict(isin=np.isin)), ('function_base', dict(angle=np.angle, iterable=np.iterable))):
    m = types.ModuleType('numpy.lib.' + name)
    for k, v in attrs.items():
        setattr(m, k, v)
    sys.modules['numpy.lib.' + name] = m; setattr(numpy.lib, name, m)
cv2 = types.ModuleType('cv2'); cv2.normalize = None; sys.modules['cv2'] = cv2
tv = types.ModuleType('torchvision'); tv.transforms = types.ModuleType('torchvision.transforms'); tv.utils = types.ModuleType('torchvision.utils')
tv.utils.save_image = None
sys.modules.update({'torchvision': tv, 'torchvision.transforms': tv.transforms, 'torchvision.utils': tv.utils})
'''

CHILD_SEQUENCE = STUBS + r'''
import torch
import dnnlib, legacy                                     # legacy.py is the reference's file; dnnlib the overlay (extended over the reference)
from training.volumetric_rendering import sample_camera_positions, create_cam2world_matrix     # gen_images.py:12
from dnnlib.seg_tools import *                            # gen_images.py:14 -> the REFERENCE's module through the extended package path
assert legacy.__file__.startswith(ref) and dnnlib.__file__.startswith(overlay)
assert sys.modules['dnnlib.seg_tools'].__file__.startswith(ref)
# dnnlib/seg_tools.py:10 `from inversion.BiSeNet import BiSeNet` finds the overlay's face parser; the rest of `inversion` stays the reference's
import inversion.BiSeNet, inversion.networks
assert inversion.BiSeNet.__file__.startswith(overlay) and inversion.networks.__file__.startswith(ref)
assert sys.modules['dnnlib.seg_tools'].BiSeNet.__module__ == 'training.face_parsing'
_net = BiSeNet(n_classes=20).eval()
_lab = face_parsing(torch.zeros(1, 3, 64, 64), _net)          # the REFERENCE's face_parsing / parsing_img / id_remap / scatter (seg_tools.py:100-123) on it
assert _lab.shape == (1, 19, 512, 512) and float(_lab.sum(1).min()) == 1.0
import training.networks, training.triplane, torch_utils.ops.upfirdn2d
for mod in (training.networks, training.triplane, torch_utils.ops.upfirdn2d, sys.modules['training.volumetric_rendering']):
    assert mod.__file__.startswith(overlay), mod.__file__

device = torch.device('cpu')
with dnnlib.util.open_url(pkl) as f:                      # gen_images.py:81-82
    G = legacy.load_network_pkl(f)['G_ema'].to(device)
assert type(G).__module__ == 'training.triplane'

truncation_psi, noise_mode = 0.7, 'const'
cs = torch.tensor([1,0,0,0, 0,1,0,0, 0,0,1,2.7, 0,0,0,1, 4.2647, 0, 0.5, 0, 4.2647, 0.5, 0, 0, 1]).float().to(device).reshape(1,-1)
imgs, segs, cams = [], [], []
for seed in (0, 1):
    torch.manual_seed(seed)
    z = torch.from_numpy(np.random.RandomState(seed).randn(1, G.z_dim)).to(device)
    ws = G.mapping(z=z, c=cs, truncation_psi=truncation_psi)
    for k, yaw in enumerate([-0.5, 0, 0.5]):
        render_params = {"h_mean": yaw+math.pi*0.5, "v_mean": math.pi * 0.5, "h_stddev": 0., "v_stddev": 0., "fov": 18, "num_steps": 12}
        camera_points, phi, theta = sample_camera_positions(device, n=1, r=2.7, horizontal_mean=yaw+math.pi*0.5, vertical_mean=math.pi * 0.5, mode=None)
        c = create_cam2world_matrix(-camera_points, camera_points, device=device)
        c = c.reshape(1,-1)
        c = torch.cat((c, torch.tensor([4.2647, 0, 0.5, 0, 4.2647, 0.5, 0, 0, 1]).reshape(1, -1).to(c)), -1)
        torch.manual_seed(1000 + k)                       # the stratified jitter is drawn inside synthesis
        img, seg = G.synthesis(ws, c=c, render_params=render_params, noise_mode=noise_mode, return_seg=True)
        col = (mask2color(seg) / 255. - 0.5) / 0.5
        assert img.shape == (1, 3, G.img_resolution, G.img_resolution) and col.shape == img.shape
        imgs.append(img.detach().numpy()); segs.append(seg.detach().numpy())
        if seed == 0:
            cams.append(c.numpy())
np.savez(out, seq_img=np.stack(imgs), seq_seg=np.stack(segs), seq_cam=np.concatenate(cams))
print('DRIVER_SEQUENCE_OK')
'''

CHILD_LOOPS = STUBS + r'''
# the video writer's stub records the frames it is given; nothing else of these modules is on the recorded path
for name in ('plyfile', 'mrcfile', 'skimage', 'skimage.measure'):
    sys.modules[name] = types.ModuleType(name)
sys.modules['skimage'].measure = sys.modules['skimage.measure']
written = {}
class _Writer:
    def __init__(self, path, **kw): self.path, self.kw, self.frames = path, kw, []; written[path] = self
    def append_data(self, frame): self.frames.append(np.array(frame))
    def close(self): self.closed = True
imageio = types.ModuleType('imageio'); imageio.get_writer = lambda path, **kw: _Writer(path, **kw); sys.modules['imageio'] = imageio

import torch
import dnnlib, legacy
import gen_videos, extract_shapes                          # the REFERENCE's files
assert gen_videos.__file__.startswith(ref) and extract_shapes.__file__.startswith(ref)

device = torch.device('cpu')
with dnnlib.util.open_url(pkl) as f:
    G = legacy.load_network_pkl(f)['G_ema'].to(device)
# neither driver can pass jitter draws: render without stratified jitter (keyword injected in front of G.synthesis)
G.synthesis.register_forward_pre_hook(lambda mod, args, kwargs: (args, {**kwargs, 'ray_jitter': False}), with_kwargs=True)

# gen_videos.py:66-139, 2 x 2 grid of four seeds, image_seg frames, 2 frames
seeds, w_frames = [0, 1, 2, 3], 2
gen_videos.gen_interp_video(G=G, mp4='grid.mp4', seeds=seeds, w_frames=w_frames, grid_dims=(2, 2), image_mode='image_seg', device=device)
wr = written['grid.mp4']
assert wr.kw.get('codec') == 'libx264' and wr.kw.get('fps') == 60 and getattr(wr, 'closed', False)     # gen_videos.py:108,139
frames = np.stack(wr.frames)
res = G.img_resolution
assert frames.shape == (w_frames, 2 * res, 2 * 2 * res, 3) and frames.dtype == np.uint8

# extract_shapes.py:99-150 at voxel_resolution 32 (driver arguments of extract_shapes.py:166-189)
label = torch.tensor([1,0,0,0, 0,1,0,0, 0,0,1,2.7, 0,0,0,1, 4.2647, 0, 0.5, 0, 4.2647, 0.5, 0, 0, 1])[None].float()
render_params = {"h_stddev": 0., "v_stddev": 0., "num_steps": 96}
z = torch.from_numpy(np.random.RandomState(5).randn(1, G.z_dim))
cube = extract_shapes.sample_generator_ide3d(G, None, z, label, cube_length=0.3, voxel_resolution=32, psi=1.0, max_batch=10000, **render_params)
assert cube.shape == (32, 32, 32)
s, o, v = extract_shapes.create_samples(32, [0, 0, 0], 0.3)
assert s.dtype == torch.float32 and s.is_contiguous()
np.savez(out, video_frames=frames, cube=np.asarray(cube), lattice_samples=s.numpy(), lattice_origin=np.asarray(o),
         lattice_voxel_size=np.asarray(v, dtype=np.float64))
print('DRIVER_LOOPS_OK')
'''


def run_child(code, ref, pkl_flag, tmp):
    pkl = os.path.join(tmp, f'random-init{pkl_flag}.pkl')
    subprocess.run([sys.executable, os.path.join(ROOT, 'scripts', 'make_random_init_pkl.py'), pkl_flag, '--out', pkl], check=True)
    child, out = os.path.join(tmp, 'child.py'), os.path.join(tmp, 'out.npz')
    with open(child, 'w') as f:
        f.write(textwrap.dedent(code))
    env = {k: v for k, v in os.environ.items() if k != 'PYTHONPATH'}
    subprocess.run([sys.executable, child, os.path.join(ROOT, 'ide-3d_amd'), ref, pkl, out], env=env, cwd=tmp, check=True, timeout=1200)
    return dict(np.load(out))


def reduce(a):
    """Keep the fixture small: of each recorded render, the values at SEQ_SAMPLE_FRACTION of its positions (fixed, seeded, ascending; the
    positions are stored next to them); of the lattice, its SHA-256 (float32 bytes, C order), shape, first and last rows."""
    import hashlib
    out = {k: v for k, v in a.items() if not k.startswith(('seq_img', 'seq_seg', 'lattice_samples'))}
    rs = np.random.RandomState(0)
    for key in ('seq_img', 'seq_seg'):
        flat = a[key].reshape(a[key].shape[0], -1)
        idx = np.sort(rs.choice(flat.shape[1], flat.shape[1] // SEQ_SAMPLE_FRACTION, replace=False)).astype(np.int32)
        out[key + '_index'], out[key + '_sample'] = idx, flat[:, idx]
    lat = np.ascontiguousarray(a['lattice_samples'], dtype=np.float32)
    out['lattice_sha256'] = np.frombuffer(hashlib.sha256(lat.tobytes()).digest(), dtype=np.uint8)
    out['lattice_shape'] = np.asarray(lat.shape, dtype=np.int64)
    out['lattice_first_last'] = lat.reshape(-1, 3)[[0, -1]]
    return out


def main():
    ref = sys.argv[1] if len(sys.argv) > 1 else os.environ.get('IDE3D_REFERENCE', '/root/reference')
    assert os.path.isdir(os.path.join(ref, 'torch_utils')), f'reference checkout not found at {ref}'
    ref = os.path.abspath(ref)
    arrays = {}
    with tempfile.TemporaryDirectory() as tmp:
        arrays.update(run_child(CHILD_SEQUENCE, ref, '--tiny', tmp))
        arrays.update(run_child(CHILD_LOOPS, ref, '--tiny52', tmp))
    stored = reduce(arrays)
    np.savez_compressed(OUT, **stored)
    print(f'{os.path.relpath(OUT, ROOT)}: {", ".join(f"{k} {v.shape}" for k, v in stored.items())}, {os.path.getsize(OUT) / 1024:.1f} KiB')


if __name__ == '__main__':
    main()
