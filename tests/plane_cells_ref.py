"""float64 numpy reference of the plane gate's needed-cell map (ide3d_plane_cells, csrc/camera.hip), and the
cameras its tests use.  Shared by tests/test_plane_cells_cpu.py and tests/test_gpu_plane_cells.py.

A cell is a 4 x 4 block of texels of one plane (0: xy, 1: yz, 2: xz) of an H x W tri-plane.  The renderer's sample of ray r at step i with
jitter draw j sits at depth z_i + (j - 0.5) * dz along the camera-space direction d_r, is moved to the world by cam2world, and reads the
2 x 2 texels (floor(u), floor(u) + 1) x (floor(v), floor(v) + 1) of every plane, u = ((x + 1) * W - 1) / 2.  A tap outside the plane has
weight zero, but the marcher still LOADS it, from the address clamped into the plane (csrc/triplane_tap.h `tap_addr`).

    exact(jitters)   cells that hold an in-bounds tap of a sample at one of the given draws
    reads(jitters)   cells that hold an address the marcher forms for those samples: `exact` plus the clamped ones (the border texels that
                     a tap outside the plane is loaded from; a zero weight does not make an Inf or a NaN found there harmless)
    hull()           cells met by the continuous segments j in [0, 1] (sampled every 1 / 32 of a segment: at most 0.1 texel at the sizes
                     used here, and a subset of the true hull, which only makes the cap below stricter), addresses clamped like `reads`

The device map must contain `reads` for every draw, and must be contained in `hull` dilated by one cell.
"""
import math

import numpy as np

CELL = 4


def camera_rays(fov, size):
    """training.volumetric_rendering._camera_rays in float64: [size * size, 3], x fastest, y flipped."""
    x = np.linspace(-1.0, 1.0, size)
    y = np.linspace(1.0, -1.0, size)
    gx, gy = np.meshgrid(x, y, indexing='xy')                 # row = y, column = x
    z = -np.ones_like(gx) / np.tan((2 * math.pi * fov / 360) / 2)
    d = np.stack([gx.ravel(), gy.ravel(), z.ravel()], -1)
    return d / np.linalg.norm(d, axis=-1, keepdims=True)


def _plane_uv(cam2world, fov, size, steps, t0, t1, jitter, H, W):
    """Continuous texel coordinates (u, v) of every plane for draws `jitter` [n, R, S, K] -> float64 [n, R, S, K, 3, 2]."""
    M = np.asarray(cam2world, dtype=np.float64).reshape(-1, 4, 4)
    d = camera_rays(fov, size)                                 # [R, 3]
    z = np.linspace(t0, t1, steps)
    dz = z[1] - z[0] if steps > 1 else 0.0
    depth = z[None, None, :, None] + (jitter - 0.5) * dz       # [n, R, S, K]
    p = d[None, :, None, None, :] * depth[..., None]           # camera space
    w = np.einsum('nij,nrskj->nrski', M[:, :3, :3], p) + M[:, None, None, None, :3, 3]
    planes = np.stack([w[..., [0, 1]], w[..., [1, 2]], w[..., [0, 2]]], axis=-2)      # [n, R, S, K, 3, 2] (x coordinate, y coordinate)
    size_xy = np.array([W, H], dtype=np.float64)
    return ((planes + 1.0) * size_xy - 1.0) / 2.0


def _mark(cells, n_idx, pl_idx, x, y, ok):
    cells[n_idx[ok], pl_idx[ok], y[ok] // CELL, x[ok] // CELL] = 1


def _cells_of(uv, H, W, clamped):
    n = uv.shape[0]
    cells = np.zeros([n, 3, -(-H // CELL), -(-W // CELL)], dtype=np.uint8)
    # the marcher saturates floor() into [-2, size + 1] before the integer conversion (make_tap)
    ix0 = np.clip(np.floor(uv[..., 0]), -2, W + 1).astype(np.int64)
    iy0 = np.clip(np.floor(uv[..., 1]), -2, H + 1).astype(np.int64)
    n_idx = np.broadcast_to(np.arange(n).reshape(n, 1, 1, 1, 1), ix0.shape)
    pl_idx = np.broadcast_to(np.arange(3).reshape(1, 1, 1, 1, 3), ix0.shape)
    for dx in (0, 1):
        for dy in (0, 1):
            x, y = ix0 + dx, iy0 + dy
            if clamped:
                _mark(cells, n_idx, pl_idx, np.clip(x, 0, W - 1), np.clip(y, 0, H - 1), np.ones(x.shape, dtype=bool))
            else:
                _mark(cells, n_idx, pl_idx, x, y, (x >= 0) & (x < W) & (y >= 0) & (y < H))
    return cells


def _draws(jitters, n, rays, steps, seed):
    """[n, R, S, K]: the given constant draws and, for every None among them, one uniform draw per sample."""
    rng = np.random.RandomState(seed)
    cols = [rng.uniform(0.0, 1.0, size=[n, rays, steps]) if j is None else np.full([n, rays, steps], float(j)) for j in jitters]
    return np.stack(cols, axis=-1)


EXACT_DRAWS = (0.0, 0.5, 1.0 - 2.0 ** -24, None)               # None: one random draw per sample


def exact(cam2world, fov, size, steps, t0, t1, H, W, jitters=EXACT_DRAWS, seed=0):
    n = np.asarray(cam2world).reshape(-1, 4, 4).shape[0]
    return _cells_of(_plane_uv(cam2world, fov, size, steps, t0, t1, _draws(jitters, n, size * size, steps, seed), H, W), H, W, clamped=False)


def reads(cam2world, fov, size, steps, t0, t1, H, W, jitters=EXACT_DRAWS, seed=0):
    n = np.asarray(cam2world).reshape(-1, 4, 4).shape[0]
    return _cells_of(_plane_uv(cam2world, fov, size, steps, t0, t1, _draws(jitters, n, size * size, steps, seed), H, W), H, W, clamped=True)


def hull(cam2world, fov, size, steps, t0, t1, H, W, per_segment=33):
    n = np.asarray(cam2world).reshape(-1, 4, 4).shape[0]
    t = np.broadcast_to(np.linspace(0.0, 1.0, per_segment), [n, size * size, steps, per_segment])
    return _cells_of(_plane_uv(cam2world, fov, size, steps, t0, t1, t, H, W), H, W, clamped=True)


def dilate(cells):
    """Every cell whose 3 x 3 neighbourhood (same plane, same image) holds a set cell."""
    p = np.pad(cells, ((0, 0), (0, 0), (1, 1), (1, 1)))
    out = np.zeros_like(cells)
    h, w = cells.shape[2:]
    for dy in range(3):
        for dx in range(3):
            out |= p[:, :, dy:dy + h, dx:dx + w]
    return out


# ---- the cameras of the tests: 16 x 16 rays x 12 steps on 64^2 planes ------------------------------------------------------------------

SIZE, STEPS, PLANE = 16, 12, 64
T0, T1 = 2.25, 3.3


def _look_at(origin, target):
    """cam2world of training.volumetric_rendering.create_cam2world_matrix(normalize(target - origin), origin), float64 -> float32."""
    o, t = np.asarray(origin, np.float64), np.asarray(target, np.float64)
    f = (t - o) / np.linalg.norm(t - o)
    left = np.cross([0.0, 1.0, 0.0], f); left /= np.linalg.norm(left)
    up = np.cross(f, left); up /= np.linalg.norm(up)
    m = np.eye(4)
    m[:3, 0], m[:3, 1], m[:3, 2], m[:3, 3] = -left, up, -f, o
    return m.astype(np.float32)


def _orbit(yaw, pitch=math.pi / 2, radius=2.7):
    """The gen_images.py pose: a camera on a sphere of `radius` looking at the origin (training.triplane.camera_label)."""
    theta, phi = yaw + math.pi / 2, min(max(pitch, 1e-5), math.pi - 1e-5)
    o = radius * np.array([math.sin(phi) * math.cos(theta), math.cos(phi), math.sin(phi) * math.sin(theta)])
    return _look_at(o, [0.0, 0.0, 0.0])


# name -> (cam2world [n, 4, 4] float32, fov)
CASES = {
    'yaw0': (np.stack([_orbit(0.0)]), 18.0),
    'yaw_pm05': (np.stack([_orbit(-0.5), _orbit(0.5)]), 18.0),               # two images: the image index of the map
    'steep_pitch': (np.stack([_orbit(0.3, pitch=0.35)]), 18.0),
    'close_leaves_volume': (np.stack([_orbit(0.2, radius=1.2)]), 18.0),      # the far samples are behind the volume: taps outside the planes
    'fov60': (np.stack([_orbit(0.0)]), 60.0),
    'plane_corner': (np.stack([_look_at([0.9, 0.9, 2.7], [0.9, 0.9, 0.0])]), 18.0),   # the xy plane's (+1, +1) corner: last row and column
}
