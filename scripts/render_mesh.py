"""The reference's render_mesh.py on the device: density cube (`.npy` of extract_shapes.py) -> marching cubes -> 512^2 turntable video,
with the rasterizer of csrc/raster.hip in place of pyrender / trimesh.  Same options as the reference:

    python scripts/render_mesh.py --fname out/1.npy --size 256 --sigma-threshold 10 --w-frames 240 --outdir out

writes <outdir>/render.y4m (`ffmpeg -i render.y4m render.mp4` makes the reference's file), or with `--format avi` <outdir>/render.avi:
Motion-JPEG compressed on the device (`video_render.write_avi`).  `--size` is the reference's cube side: the
vertices are divided by it (render_mesh.py:32).  With `--colors` or `--labels` and a generator pickle in `--fname` the mesh comes from
`extract_mesh(vertex_attributes=True)` at `--size`^3 instead of a cube file, and the frames show the vertex colours or the semantic
labels' palette.  The shading is ambient + diffuse Lambert, not pyrender's metallic-roughness model."""
import argparse, os, pickle, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'ide-3d_amd')); sys.path.insert(0, ROOT)
import numpy as np
import torch
from training import mesh_extraction, mesh_render, video_render


def label_palette(num=19, seed=0):
    """One fixed colour per semantic label (uint8 [num, 3])."""
    return torch.from_numpy(np.random.RandomState(seed).randint(32, 256, size=[num, 3]).astype(np.uint8))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--fname', required=True, help='density cube (.npy), or a network pickle with --colors / --labels')
    ap.add_argument('--size', type=int, default=256, help='side of the cube')
    ap.add_argument('--sigma-threshold', type=float, default=10.0, help='sigma threshold during marching cubes')
    ap.add_argument('--w-frames', type=int, default=240, help='number of frames of the turntable')
    ap.add_argument('--outdir', required=True)
    ap.add_argument('--colors', action='store_true', help='generator pickle: shade with the vertex colours')
    ap.add_argument('--labels', action='store_true', help='generator pickle: shade with the semantic labels\' palette')
    ap.add_argument('--seed', type=int, default=0, help='generator pickle: the latent\'s seed')
    ap.add_argument('--image-size', type=int, default=512)
    ap.add_argument('--format', choices=['y4m', 'avi'], default='y4m', help='y4m: raw 4:4:4 frames; avi: Motion-JPEG (quality 90, 4:2:0), 60 fps both')
    ap.add_argument('--device', default='cuda:0' if torch.cuda.is_available() else 'cpu')
    args = ap.parse_args()
    dev = torch.device(args.device)
    if args.colors or args.labels:
        from training import triplane
        with open(args.fname, 'rb') as f:
            G = pickle.load(f)['G_ema'].eval().requires_grad_(False).to(dev)
        z = torch.from_numpy(np.random.RandomState(args.seed).randn(1, G.z_dim)).float().to(dev)
        mesh = mesh_extraction.extract_mesh(G, z, triplane.conditioning_label(dev), voxel_resolution=args.size, threshold=args.sigma_threshold,
                                            normals=True, vertex_attributes=True)
        if args.labels:
            mesh['colors'] = label_palette().to(dev)[mesh['labels'].clamp(0, 18)]
    else:
        mesh = mesh_render.mesh_from_cube_file(args.fname, threshold=args.sigma_threshold, device=dev, normals=True, side=args.size)
    os.makedirs(args.outdir, exist_ok=True)
    path = os.path.join(args.outdir, 'render.' + args.format)
    frames = mesh_render.render_turntable(mesh, num_frames=args.w_frames, size=args.image_size)
    count = (video_render.write_avi if args.format == 'avi' else video_render.write_y4m)(frames, path)
    print(f'{count} frames of {mesh["triangles"].shape[0]} triangles -> {path}')


if __name__ == '__main__':
    main()
