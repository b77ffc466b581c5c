"""The reference's UNTOUCHED driver code on top of the overlay (INTEGRATION.md option A), in this container on CPU tensors, against
tests/golden/drivers.npz — the outputs of those drivers (of the gen_images.py renders a fixed quarter of their values), recorded by
oracle/make_driver_golden.py, which also asserts how the reference's modules bind to the overlay (`legacy`, `dnnlib.seg_tools`,
`gen_videos`, `extract_shapes` from the reference, everything else from here):

  * `scripts/make_random_init_pkl.py` writes `dict(G_ema=G)`, which unpickles into the product's `training.triplane` module;
  * the call sequence of gen_images.py:85-111 on the loaded generator (`G.mapping(z=, c=, truncation_psi=)`, `sample_camera_positions`,
    `create_cam2world_matrix`, `G.synthesis(ws, c=c, render_params=..., noise_mode=..., return_seg=True)`) equals the product called
    directly;
  * the viewer pattern of viz/renderer.py:410-441 (a forward hook on every sub-module, `force_fp32=` keyword) works on the module tree;
  * gen_videos.py:66-139 and extract_shapes.py:99-150 equal training/video_render.py / training/shape_extraction.py called directly.
"""

import hashlib
import math
import os
import subprocess
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'drivers.npz')


def _load_pkl(tmp_path, flag):
    """The pickle the drivers load (`dnnlib.util.open_url` + unpickling, as legacy.load_network_pkl does), written by the product's script."""
    import pickle
    from dnnlib import util
    pkl = tmp_path / f'random-init{flag}.pkl'
    res = subprocess.run([sys.executable, os.path.join(ROOT, 'scripts', 'make_random_init_pkl.py'), flag, '--out', str(pkl)],
                         stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert res.returncode == 0, res.stdout
    with util.open_url(str(pkl)) as f:
        G = pickle.load(f)['G_ema'].to(torch.device('cpu'))
    assert type(G).__module__ == 'training.triplane'
    return G


def test_untouched_reference_driver_sequence(tmp_path):
    from training import triplane
    d = np.load(GOLDEN)
    G = _load_pkl(tmp_path, '--tiny')
    cs = torch.tensor([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 2.7, 0, 0, 0, 1, 4.2647, 0, 0.5, 0, 4.2647, 0.5, 0, 0, 1]).float().reshape(1, -1)
    for k, yaw in enumerate([-0.5, 0, 0.5]):      # the camera labels the sequence builds (pose helpers + intrinsics) == the product's
        assert torch.allclose(triplane.camera_label(yaw), torch.from_numpy(d['seq_cam'][k:k + 1]), atol=1e-6), yaw
    i = 0
    for seed in (0, 1):
        torch.manual_seed(seed)
        z = torch.from_numpy(np.random.RandomState(seed).randn(1, G.z_dim))
        ws = G.mapping(z=z, c=cs, truncation_psi=0.7)
        for k, yaw in enumerate([-0.5, 0, 0.5]):
            torch.manual_seed(1000 + k)           # the stratified jitter is drawn inside synthesis, as in the recorded sequence
            img, seg = G.synthesis(ws, c=triplane.camera_label(yaw), noise_mode='const', return_seg=True)
            assert img.shape == (1, 3, G.img_resolution, G.img_resolution)
            for name, got in (('img', img), ('seg', seg)):      # the recorded quarter of the render's values (oracle/make_driver_golden.py)
                got = got.reshape(-1)[torch.from_numpy(d[f'seq_{name}_index']).long()]
                want = torch.from_numpy(d[f'seq_{name}_sample'][i])
                assert torch.allclose(got, want, atol=1e-5), (name, seed, yaw, float((got - want).abs().max()))
            assert math.isfinite(float(img.abs().mean())) and float(img.abs().mean()) > 0
            i += 1

    # viz/renderer.py:410-441 pattern: hooks on every sub-module, force_fp32 keyword, dict output
    names = {mod: name for name, mod in G.named_modules()}
    seen = []
    hooks = [m.register_forward_hook(lambda mod, _i, out: seen.append(names[mod])) for m in G.modules()]
    out = G.synthesis(ws, c=triplane.camera_label(0.5), noise_mode='const', force_fp32=True, return_dict=True)
    for h in hooks:
        h.remove()
    assert set(out) >= {'image', 'image_depth', 'image_raw'}
    assert any(n.startswith('synthesis.vb') for n in seen) and any(n.startswith('synthesis.b') and 'torgb' in n for n in seen) and 'synthesis.renderer' in seen


def test_reference_gen_videos_and_extract_shapes_loops(tmp_path):
    """gen_videos.py:66-139 (2 frames of a 2 x 2 `image_seg` grid) and extract_shapes.py:99-150 (32^3 cube) as recorded from the REFERENCE's
    files on the overlay, without stratified jitter; training/video_render.py / training/shape_extraction.py called directly reproduce them."""
    import training.video_render as video_render
    import training.shape_extraction as shape_extraction
    d = np.load(GOLDEN)
    G = _load_pkl(tmp_path, '--tiny52')
    G.synthesis.register_forward_pre_hook(lambda mod, args, kwargs: (args, {**kwargs, 'ray_jitter': False}), with_kwargs=True)
    device = torch.device('cpu')

    seeds, w_frames = [0, 1, 2, 3], 2
    ref_frames = d['video_frames']
    res = G.img_resolution
    assert ref_frames.shape == (w_frames, 2 * res, 2 * 2 * res, 3) and ref_frames.dtype == np.uint8
    ours = np.stack([f.cpu().numpy() for f in video_render.gen_interp_frames(G, seeds, w_frames=w_frames, grid_dims=(2, 2), image_mode='image_seg', device=device)])
    assert ours.shape == ref_frames.shape
    # the product renders the four cells of a frame in one batch from cached tri-planes; the reference one by one from scratch: identical
    # up to fp32 summation order inside ATen's CPU convolutions, i.e. isolated uint8 roundings / argmax flips
    diff = ours.astype(np.int32) - ref_frames.astype(np.int32)
    rgb = np.concatenate([diff[:, :, :res], diff[:, :, 2 * res:3 * res]], axis=2)            # the RGB halves of the two grid columns
    assert np.abs(rgb).max() <= 2 and (diff != 0).mean() < 5e-3, (int(np.abs(rgb).max()), float((diff != 0).mean()))

    label = torch.tensor([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 2.7, 0, 0, 0, 1, 4.2647, 0, 0.5, 0, 4.2647, 0.5, 0, 0, 1])[None].float()
    render_params = {"h_stddev": 0., "v_stddev": 0., "num_steps": 96}
    z = torch.from_numpy(np.random.RandomState(5).randn(1, G.z_dim))
    cube_ref = d['cube']
    cube = shape_extraction.sample_generator_ide3d(G, None, z, label, cube_length=0.3, voxel_resolution=32, psi=1.0, max_batch=10000, **render_params)
    assert cube_ref.shape == (32, 32, 32) and cube.shape == cube_ref.shape
    assert np.allclose(cube, cube_ref, rtol=1e-4, atol=1e-5 * np.abs(cube_ref).max()), float(np.abs(cube - cube_ref).max())
    # the lattice the reference builds == the product's
    s, o, v = shape_extraction.create_samples(32, [0, 0, 0], 0.3)
    assert s.dtype == torch.float32 and list(s.shape) == d['lattice_shape'].tolist()
    assert torch.equal(s.reshape(-1, 3)[[0, -1]], torch.from_numpy(d['lattice_first_last']))
    assert hashlib.sha256(s.contiguous().numpy().tobytes()).digest() == d['lattice_sha256'].tobytes()      # every point, bit for bit
    assert np.array_equal(o, d['lattice_origin']) and v == float(d['lattice_voxel_size'])
