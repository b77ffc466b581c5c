"""Rendering the extracted mesh: the step render_mesh.py:36-61 delegates to pyrender / trimesh (OpenGL), as a triangle rasterizer on the
device (csrc/raster.hip).  One perspective camera per frame (yfov 18 degrees, render_mesh.py:48), one directional
light at the camera pose (:57), white background (:47).

Definition (the kernels' header comment states it in full; `project_host`, `depth_host` and `shade_host` below are the same integers
and the same float32 operations in the same order, in numpy):

  * camera space p_cam = R p + t with (R | t) = the inverse of `cam2world`, inverted here in float64 and rounded to float32; view depth
    d = -z_cam; pixel coordinates px = ((fx x_cam) / d) sx + ox, py = oy - ((fy y_cam) / d) sy; fy = 1 / tan(fov / 2), fx = fy / (W / H);
    snapped to 24.8 fixed point X = rint(256 px).  Pixel (r, c) is sampled at (256 c + 128, 256 r + 128).
    `align_corners=False` (default): sx = ox = W / 2, pixel centres at c + 0.5 like OpenGL.  `align_corners=True`: sx = (W - 1) / 2,
    ox = W / 2, so that column c sits at ndc = -1 + 2 c / (W - 1), the ray grid of `get_initial_rays_trig`: the mesh depth map then lies
    on the ray-marcher's pixels (square images).
  * coverage by int64 edge functions with the top-left rule, perspective-correct float32 view depth, nearest wins, equal depths go to the
    lower triangle index.  The device resolves this with one 64-bit integer atomic minimum per covered sample on the key
    (depth bits << 32 | triangle index): a minimum does not depend on order, so two runs are bit-equal.
  * NO clipping: a triangle with a vertex behind `near` or outside the guard band (|px|, |py| <= 16384) is dropped whole, as are
    degenerate triangles and triangles with an index outside [0, V).  `validate=True` raises on the cases a user would not expect.
  * shading: image = clamp(base (ambient + diffuse max(0, n . l))), l = the camera's +z axis in world space.  This is NOT pyrender's
    metallic-roughness model (metallicFactor 0.2, roughnessFactor 0.6, ambient [5, 5, 5], light intensity 3: render_mesh.py:36-49),
    which is not available to compare against; `ambient` and `diffuse` are this package's own parameters.
"""

import math

import numpy as np
import torch

GUARD = 16384.0
BEHIND, OUTSIDE = 1, 2                      # vertex flags
BAD_INDEX, DROPPED = 1, 2                   # status bits
CULL = ('none', 'back', 'front')
AMBIENT, DIFFUSE = 0.3, 0.7
_HOST_LANE_BOX = 64                         # host definition only: boxes up to this many samples are walked for all triangles at once


# ---- camera -------------------------------------------------------------------------------------------------------------------

def _size(size):
    H, W = (size, size) if isinstance(size, int) else size
    assert 1 <= int(H) <= 16384 and 1 <= int(W) <= 16384, 'render_mesh: images of 1..16384 pixels a side'
    return int(H), int(W)


def view_constants(H, W, fov=18.0, align_corners=False):
    """(fx, fy, sx, ox, sy, oy) as float32 values: what `ide3d_raster_project` takes."""
    fy = 1.0 / math.tan(math.radians(fov) / 2)
    fx = fy / (W / H)
    if align_corners:
        sx, sy = (W - 1) / 2, (H - 1) / 2
    else:
        sx, sy = W / 2, H / 2
    return tuple(np.float32(v) for v in (fx, fy, sx, W / 2, sy, H / 2))


def camera_matrices(cam2world):
    """cam2world [N, 4, 4] or [N, 16] (any device, e.g. `c[:, :16]`) -> (world2cam [N, 3, 4] float32, light [N, 3] float32) as numpy:
    the float64 inverse rounded once, and the camera's +z axis in world space."""
    c = cam2world.detach().cpu().double().numpy() if isinstance(cam2world, torch.Tensor) else np.asarray(cam2world, dtype=np.float64)
    c = c.reshape(-1, 4, 4)
    return np.ascontiguousarray(np.linalg.inv(c)[:, :3, :].astype(np.float32)), np.ascontiguousarray(c[:, :3, 2].astype(np.float32))


# ---- host definition ----------------------------------------------------------------------------------------------------------

def project_host(vertices, world2cam, view, near=0.05):
    """float32 vertices [V, 3], world2cam [N, 3, 4], `view_constants(...)` -> records [N, V, 4] int32: X, Y, float bits of d, flags."""
    v = np.ascontiguousarray(vertices, dtype=np.float32).reshape(-1, 3)
    m = np.ascontiguousarray(world2cam, dtype=np.float32).reshape(-1, 3, 4)
    fx, fy, sx, ox, sy, oy = (np.float32(a) for a in view)
    x, y, z = v[None, :, 0], v[None, :, 1], v[None, :, 2]
    with np.errstate(all='ignore'):
        cam = [((m[:, k, 0, None] * x + m[:, k, 1, None] * y) + m[:, k, 2, None] * z) + m[:, k, 3, None] for k in range(3)]
        d = -cam[2]
        front = d >= np.float32(near)
        px = ((fx * cam[0]) / d) * sx + ox
        py = oy - ((fy * cam[1]) / d) * sy
        inside = front & (np.abs(px) <= np.float32(GUARD)) & (np.abs(py) <= np.float32(GUARD))
        X = np.where(inside, np.rint(np.where(inside, px, np.float32(0)) * np.float32(256)), 0).astype(np.int32)
        Y = np.where(inside, np.rint(np.where(inside, py, np.float32(0)) * np.float32(256)), 0).astype(np.int32)
    flags = np.where(~front, BEHIND, np.where(~inside, OUTSIDE, 0)).astype(np.int32)
    return np.ascontiguousarray(np.stack([X, Y, np.ascontiguousarray(d, dtype=np.float32).view(np.int32), flags], axis=-1))


def _corners(rec, tri):
    """records [V, 4] and index triples [n, 3] (all valid) -> X [n, 3] int64, Y [n, 3] int64, d [n, 3] float32, flags [n, 3]."""
    r = rec[tri]
    return r[..., 0].astype(np.int64), r[..., 1].astype(np.int64), np.ascontiguousarray(r[..., 2]).view(np.float32), r[..., 3]


def _edge_values(X, Y, s, r, c):
    """Per sample: corner coordinates [n, 3], area sign [n], pixel (r, c) -> (w [n, 3] int64 with sum = |doubled area|, covered [n])."""
    px, py = 256 * c.astype(np.int64) + 128, 256 * r.astype(np.int64) + 128
    w, covered = [], np.ones(X.shape[0], dtype=bool)
    for a, b in ((1, 2), (2, 0), (0, 1)):                       # the edge opposite corner 0, 1, 2
        dx, dy = s * (X[:, b] - X[:, a]), s * (Y[:, b] - Y[:, a])
        e = dx * (py - Y[:, a]) - dy * (px - X[:, a])
        covered &= (e > 0) | ((e == 0) & ((dy < 0) | ((dy == 0) & (dx > 0))))          # top-left rule
        w.append(e)
    return np.stack(w, axis=1), covered


def _view_depth(w, d):
    """q_i = float32(w_i) / d_i, their sum in corner order, and the view depth float32(|A2|) / sum."""
    with np.errstate(all='ignore'):
        q = w.astype(np.float32) / d
        qs = (q[:, 0] + q[:, 1]) + q[:, 2]
        return q, qs, w.sum(axis=1).astype(np.float32) / qs


def depth_host(records, triangles, H, W, cull='none'):
    """records [N, V, 4], triangles [T, 3] -> (z-buffer [N, H, W] uint64, all ones = background; status bits)."""
    assert cull in CULL
    rec_all = np.asarray(records, dtype=np.int32)
    tri_all = np.asarray(triangles, dtype=np.int32).reshape(-1, 3)
    N, V = rec_all.shape[:2]
    zbuf = np.full([N, H * W], np.iinfo(np.uint64).max, dtype=np.uint64)
    ok = ((tri_all >= 0) & (tri_all < V)).all(axis=1)
    status = 0 if ok.all() else BAD_INDEX
    for n in range(N):
        ids = np.flatnonzero(ok)
        X, Y, d, fl = _corners(rec_all[n], tri_all[ids])
        bad = fl != 0
        part = bad.any(axis=1) & ~bad.all(axis=1)
        if part.any():                                           # dropped whole; reported when what is left of it spans a box that meets the screen
            big = np.int64(1) << 40
            x0, x1 = np.where(bad, big, X)[part].min(axis=1), np.where(bad, -big, X)[part].max(axis=1)
            y0, y1 = np.where(bad, big, Y)[part].min(axis=1), np.where(bad, -big, Y)[part].max(axis=1)
            if ((x1 >= 128) & (x0 <= 256 * W - 128) & (y1 >= 128) & (y0 <= 256 * H - 128)).any():
                status |= DROPPED
        area2 = (X[:, 1] - X[:, 0]) * (Y[:, 2] - Y[:, 0]) - (Y[:, 1] - Y[:, 0]) * (X[:, 2] - X[:, 0])
        keep = ~bad.any(axis=1) & (area2 != 0)
        if cull == 'back':
            keep &= area2 < 0
        elif cull == 'front':
            keep &= area2 > 0
        c0, c1 = np.maximum((X.min(axis=1) + 127) >> 8, 0), np.minimum((X.max(axis=1) - 128) >> 8, W - 1)
        r0, r1 = np.maximum((Y.min(axis=1) + 127) >> 8, 0), np.minimum((Y.max(axis=1) - 128) >> 8, H - 1)
        keep &= (c0 <= c1) & (r0 <= r1)
        ids, X, Y, d, s = ids[keep], X[keep], Y[keep], d[keep], np.where(area2[keep] > 0, 1, -1).astype(np.int64)
        c0, bw, r0, bh = c0[keep], (c1 - c0 + 1)[keep], r0[keep], (r1 - r0 + 1)[keep]
        # candidate samples (triangle, r, c): small boxes offset by offset for all triangles at once, large boxes one triangle at a time
        small = bw * bh <= _HOST_LANE_BOX
        ks, rs, cs = [], [], []
        if small.any():
            for dy in range(int(bh[small].max())):
                for dx in range(int(bw[small].max())):
                    k = np.flatnonzero(small & (bh > dy) & (bw > dx))
                    ks.append(k); rs.append(r0[k] + dy); cs.append(c0[k] + dx)
        for k in np.flatnonzero(~small):
            rr, cc = np.meshgrid(np.arange(r0[k], r0[k] + bh[k]), np.arange(c0[k], c0[k] + bw[k]), indexing='ij')
            ks.append(np.full(rr.size, k)); rs.append(rr.reshape(-1)); cs.append(cc.reshape(-1))
        if not ks:
            continue
        k, r, c = np.concatenate(ks), np.concatenate(rs), np.concatenate(cs)
        w, covered = _edge_values(X[k], Y[k], s[k], r, c)
        k, r, c, w = k[covered], r[covered], c[covered], w[covered]
        _, _, depth = _view_depth(w, d[k])
        key = (np.ascontiguousarray(depth).view(np.uint32).astype(np.uint64) << np.uint64(32)) | ids[k].astype(np.uint64)
        np.minimum.at(zbuf[n], r * W + c, key)
    return zbuf.reshape(N, H, W), status


def shade_host(zbuf, records, vertices, triangles, light, normals=None, colors=None, labels=None, two_sided=True, ambient=AMBIENT,
               diffuse=DIFFUSE, base_color=(1.0, 1.0, 1.0), bg=1.0):
    """z-buffer of `depth_host` -> dict of numpy arrays: depth [N, 1, H, W], triangle [N, H, W] int32, image [N, 3, H, W][, label]."""
    N, H, W = zbuf.shape
    f32 = np.float32
    v = np.ascontiguousarray(vertices, dtype=f32).reshape(-1, 3)
    tri_all = np.asarray(triangles, dtype=np.int32).reshape(-1, 3)
    out = {'depth': np.full([N, 1, H, W], np.inf, dtype=f32), 'triangle': np.full([N, H, W], -1, dtype=np.int32),
           'image': np.full([N, 3, H, W], f32(bg), dtype=f32)}
    if labels is not None:
        out['label'] = np.full([N, H, W], -1, dtype=np.int32)
    for n in range(N):
        r, c = np.nonzero(zbuf[n] != np.iinfo(np.uint64).max)
        if r.size == 0:
            continue
        key = zbuf[n][r, c]
        t = (key & np.uint64(0xffffffff)).astype(np.int64)
        idx = tri_all[t]
        X, Y, d, _ = _corners(np.asarray(records[n], dtype=np.int32), idx)
        area2 = (X[:, 1] - X[:, 0]) * (Y[:, 2] - Y[:, 0]) - (Y[:, 1] - Y[:, 0]) * (X[:, 2] - X[:, 0])
        s = np.where(area2 > 0, 1, -1).astype(np.int64)
        w, _ = _edge_values(X, Y, s, r, c)
        q, qs, _ = _view_depth(w, d)
        with np.errstate(all='ignore'):
            b = q / qs[:, None]
            out['depth'][n, 0, r, c] = (key >> np.uint64(32)).astype(np.uint32).view(f32)
            out['triangle'][n, r, c] = t
            if labels is not None:
                best = np.where((b[:, 2] > b[:, 0]) & (b[:, 2] > b[:, 1]), 2, np.where(b[:, 1] > b[:, 0], 1, 0))
                out['label'][n, r, c] = np.asarray(labels, dtype=np.int32)[idx[np.arange(idx.shape[0]), best]]
            if normals is not None:
                nv = np.ascontiguousarray(normals, dtype=f32).reshape(-1, 3)[idx]                  # [n, 3 corners, 3]
                nn = (b[:, 0, None] * nv[:, 0] + b[:, 1, None] * nv[:, 1]) + b[:, 2, None] * nv[:, 2]
            else:
                e1, e2 = v[idx[:, 1]] - v[idx[:, 0]], v[idx[:, 2]] - v[idx[:, 0]]
                nn = np.stack([e1[:, (k + 1) % 3] * e2[:, (k + 2) % 3] - e1[:, (k + 2) % 3] * e2[:, (k + 1) % 3] for k in range(3)], axis=1)
            length = np.sqrt((nn[:, 0] * nn[:, 0] + nn[:, 1] * nn[:, 1]) + nn[:, 2] * nn[:, 2])
            nn = np.where(length[:, None] > 0, nn / np.where(length > 0, length, f32(1))[:, None], f32(0))
            if two_sided:
                nn = np.where((s > 0)[:, None], -nn, nn)                                             # back-facing: turned toward the camera
            l = np.asarray(light, dtype=f32).reshape(-1, 3)[n]
            ndl = np.maximum((nn[:, 0] * l[0] + nn[:, 1] * l[1]) + nn[:, 2] * l[2], f32(0))
            shade = f32(ambient) + f32(diffuse) * ndl
            for k in range(3):
                if colors is not None:
                    cv = np.asarray(colors, dtype=np.uint8).reshape(-1, 3)[idx, k].astype(f32)     # [n, 3 corners]
                    base = ((b[:, 0] * cv[:, 0] + b[:, 1] * cv[:, 1]) + b[:, 2] * cv[:, 2]) / f32(255)
                else:
                    base = f32(base_color[k])
                out['image'][n, k, r, c] = np.minimum(np.maximum(base * shade, f32(0)), f32(1))
    return out


# ---- public surface -----------------------------------------------------------------------------------------------------------

def _raise_on(status):
    if status & BAD_INDEX:
        raise ValueError('render_mesh: a triangle index is outside [0, V)')
    if status & DROPPED:
        raise ValueError('render_mesh: a triangle that reaches the screen has a vertex behind `near` or outside the guard band; there is no '
                         'clipping, it would be dropped whole (validate=False renders without it)')


def _on_device(vertices):
    return isinstance(vertices, torch.Tensor) and vertices.is_cuda


def _host_array(t, dtype):
    if t is None:
        return None
    return np.ascontiguousarray(t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else t).astype(dtype)


def project_vertices(vertices, cam2world, *, size=512, fov=18.0, near=0.05, align_corners=False):
    """The records of the projection, int32 [N, V, 4]: X, Y (24.8 fixed point), the float bits of the view depth, flags (1: behind `near`,
    2: outside the guard band).  CUDA float32 vertices run `ide3d_raster_project`, anything else `project_host`; the two agree bit for bit."""
    H, W = _size(size)
    w2c, _ = camera_matrices(cam2world)
    view = view_constants(H, W, fov, align_corners)
    if _on_device(vertices):
        from torch_utils import hip_plugin
        v = vertices.detach().float().contiguous()
        ws = hip_plugin.RasterPlugin.project(v, torch.from_numpy(w2c).to(v.device), H, W, view, near)
        return hip_plugin.RasterPlugin.records(ws, w2c.shape[0], v.shape[0])
    return torch.from_numpy(project_host(_host_array(vertices, np.float32), w2c, view, near))


def render_mesh(vertices, triangles, cam2world, *, size=512, fov=18.0, near=0.05, normals=None, colors=None, labels=None, cull='none',
                align_corners=False, ambient=AMBIENT, diffuse=DIFFUSE, base_color=(1.0, 1.0, 1.0), bg=1.0, validate=True, large_min=None):
    """Render N cameras of one mesh -> dict: depth [N, 1, H, W] float32 (view depth, +inf on the background), triangle [N, H, W] int32
    (-1), image [N, 3, H, W] float32 in [0, 1] (`bg`), and with `labels` label [N, H, W] int32 (the label of the corner with the largest
    barycentric, -1 on the background).

    vertices [V, 3], triangles [T, 3], optional per-vertex normals [V, 3], colors [V, 3] uint8, labels [V] (what `extract_mesh` returns);
    cam2world [N, 4, 4] or [N, 16] (`c[:, :16]`); size: int or (H, W); cull: 'none' (two-sided: normals are turned toward the camera on
    back-facing triangles), 'back' or 'front' (front = the geometric normal (v1 - v0) x (v2 - v0) points toward the camera).
    Without normals the flat face normal is used.  `align_corners=True` puts the samples on the ray grid of `get_initial_rays_trig`.

    There is NO clipping: triangles with a vertex behind `near` or outside the guard band are dropped whole.  `validate=True` (one device
    reduction, one host read) raises ValueError on an out-of-range triangle index and on a dropped triangle whose remaining vertices span
    a box that meets the screen; `validate=False` is for meshes that come straight from `marching_cubes`.  The shading is ambient + diffuse
    Lambert with the light along the camera axis (render_mesh.py:57), NOT pyrender's metallic-roughness model.

    Float32 CUDA vertices run csrc/raster.hip (no fallback: an unusable library raises); CPU tensors run the numpy host definition,
    which computes the same integers and the same float32 operations.  `large_min` forces the device's lane / wave split (tests)."""
    H, W = _size(size)
    assert cull in CULL, f'cull must be one of {CULL}'
    w2c, light = camera_matrices(cam2world)
    N = w2c.shape[0]
    view = view_constants(H, W, fov, align_corners)
    shade_kw = dict(two_sided=cull == 'none', ambient=ambient, diffuse=diffuse, base_color=tuple(base_color), bg=bg)
    if _on_device(vertices):
        from torch_utils import hip_plugin
        rp = hip_plugin.RasterPlugin
        dev = vertices.device
        v = vertices.detach().float().contiguous()
        t = triangles.detach().to(device=dev, dtype=torch.int32).reshape(-1, 3).contiguous()
        ws = rp.project(v, torch.from_numpy(w2c).to(dev), H, W, view, near)
        rp.depth(ws, v, t, N, H, W, cull=cull, large_min=large_min)
        if validate:
            _raise_on(rp.status(ws))
        return rp.shade(ws, v, t, N, H, W, torch.from_numpy(light).to(dev),
                        normals=None if normals is None else normals.detach().to(device=dev, dtype=torch.float32).contiguous(),
                        colors=None if colors is None else colors.detach().to(device=dev, dtype=torch.uint8).contiguous(),
                        labels=None if labels is None else labels.detach().to(device=dev, dtype=torch.int32).contiguous(), **shade_kw)
    v, t = _host_array(vertices, np.float32), _host_array(triangles, np.int32)
    rec = project_host(v, w2c, view, near)
    zbuf, status = depth_host(rec, t, H, W, cull)
    if validate:
        _raise_on(status)
    out = shade_host(zbuf, rec, v, t, light, normals=_host_array(normals, np.float32), colors=_host_array(colors, np.uint8),
                     labels=_host_array(labels, np.int32), **shade_kw)
    dev = vertices.device if isinstance(vertices, torch.Tensor) else None
    return {k: torch.from_numpy(a).to(dev) for k, a in out.items()}


def turntable_cameras(num_frames, radius=2.7, device=None):
    """cam2world [num_frames, 4, 4] of the sweep of render_mesh.py:45-46, 52-53: yaw = pi (0.5 + 0.15 cos(2 pi i / n)),
    pitch = pi (0.5 - 0.05 sin(2 pi i / n)), the camera on the sphere of `radius` looking at the origin.  (The reference then moves the
    camera by +0.5 along every axis, line 55, because its mesh lives in [0, 1]^3: `mesh_from_cube_file` moves the mesh by -0.5 instead.)"""
    from training.volumetric_rendering import create_cam2world_matrix, sample_camera_positions
    poses = []
    for i in range(num_frames):
        yaw = math.pi * (0.5 + 0.15 * math.cos(2 * math.pi * i / num_frames))
        pitch = math.pi * (0.5 - 0.05 * math.sin(2 * math.pi * i / num_frames))
        points, _, _ = sample_camera_positions(device=device, n=1, r=radius, horizontal_mean=yaw, vertical_mean=pitch, mode=None)
        poses.append(create_cam2world_matrix(-points, points, device=device).reshape(-1, 4, 4))
    return torch.cat(poses) if poses else torch.zeros([0, 4, 4], device=device)


def render_turntable(mesh, num_frames=240, size=512, chunk=8, radius=2.7, **kw):
    """Generator of uint8 [H, W, 3] frames of the turntable (render_mesh.py:44-68), `chunk` cameras per `render_mesh` call, ready for
    `video_render.write_y4m`.  `mesh`: dict with vertices, triangles and optionally normals, colors (what `extract_mesh` /
    `mesh_from_cube_file` return); further keywords go to `render_mesh`."""
    v = mesh['vertices']
    cams = turntable_cameras(num_frames, radius=radius, device=v.device if isinstance(v, torch.Tensor) else None)
    kw.setdefault('validate', False)
    for key in ('normals', 'colors'):
        if mesh.get(key) is not None:
            kw.setdefault(key, mesh[key])
    for i in range(0, num_frames, chunk):
        image = render_mesh(v, mesh['triangles'], cams[i:i + chunk], size=size, **kw)['image']
        frames = (image * 255 + 0.5).clamp_(0, 255).to(torch.uint8).permute(0, 2, 3, 1).contiguous()
        yield from frames


def mesh_from_cube_file(path, threshold=10.0, device=None, normals=False, side=None):
    """render_mesh.py:29-32 for the `.npy` density cube extract_shapes.py writes: `np.maximum(cube, 0)`, marching cubes at `threshold`,
    vertices in index units divided by the cube side (`side`: the reference's `--size` when it differs from the file's), and the +0.5
    camera shift of line 55 carried as a vertex offset of -0.5, so that `turntable_cameras` applies unchanged
    -> dict(vertices, triangles[, normals])."""
    from training import mesh_extraction
    cube = np.maximum(np.load(path), 0)
    assert cube.ndim == 3, 'mesh_from_cube_file: a [X, Y, Z] density cube'
    res = mesh_extraction.marching_cubes(torch.from_numpy(np.ascontiguousarray(cube, dtype=np.float32)).to(device), threshold, normals=normals)
    out = {'vertices': res[0] / float(side or cube.shape[0]) - 0.5, 'triangles': res[1]}
    if normals:
        out['normals'] = res[2]
    return out
