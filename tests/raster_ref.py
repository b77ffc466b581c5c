"""The rasterizer of csrc/raster.hip / training/mesh_render.py restated as plain loops: the projection in float64, coverage on the
snapped integers in Python ints with an independently written top-left rule, float64 depth and shading at one pixel of one triangle,
and the small meshes the tests share.  Nothing here imports the code under test except `marching_cubes_host` for the sphere."""
import math

import numpy as np

# float32 view depth against float64 on the same snapped integers and the same float32 vertex depths: int64 -> float32 of w_i (2^-24
# each, one per term), q_i = w_i / d_i (2^-24), two additions of positive terms (2^-24 each, no cancellation), float32(|A2|) (2^-24)
# and the last division (2^-24): (1 + 1 + 2 + 1 + 1) 2^-24 = 6 * 2^-24 relative.  Two depths can swap order when they are closer
# than twice that.
DEPTH_REL = 6 * 2.0 ** -24
NEAR_TIE_REL = 2 * DEPTH_REL


# ---- projection -----------------------------------------------------------------------------------------------------------------

def project64(vertices, cam2world, H, W, fov=18.0, align_corners=False):
    """float64 pixel coordinates and view depth of every vertex for every camera -> (px [N, V], py [N, V], d [N, V])."""
    v = np.asarray(vertices, dtype=np.float64).reshape(-1, 3)
    c = np.asarray(cam2world, dtype=np.float64).reshape(-1, 4, 4)
    fy = 1.0 / math.tan(math.radians(fov) / 2)
    fx = fy / (W / H)
    sx, sy = ((W - 1) / 2, (H - 1) / 2) if align_corners else (W / 2, H / 2)
    px, py, d = (np.zeros([c.shape[0], v.shape[0]]) for _ in range(3))
    for n in range(c.shape[0]):
        m = np.linalg.inv(c[n])
        for i in range(v.shape[0]):
            x, y, z = (m[k, 0] * v[i, 0] + m[k, 1] * v[i, 1] + m[k, 2] * v[i, 2] + m[k, 3] for k in range(3))
            d[n, i] = -z
            if -z > 0:
                px[n, i] = fx * x / -z * sx + W / 2
                py[n, i] = H / 2 - fy * y / -z * sy
    return px, py, d


def record_depths(records):
    """records [V, 4] int32 -> the float32 view depths as float64 [V]."""
    return np.ascontiguousarray(np.asarray(records, dtype=np.int32)[:, 2]).view(np.float32).astype(np.float64)


# ---- coverage on the integers ---------------------------------------------------------------------------------------------------

def _oriented(records, tri):
    """Snapped corners of one triangle as Python ints, re-ordered so that the interior is where every edge value is positive
    -> ([(X, Y)] * 3 in the ORIGINAL corner order, sign) with sign = +1 / -1 the orientation, or None for a degenerate triangle."""
    p = [(int(records[i][0]), int(records[i][1])) for i in tri]
    area2 = (p[1][0] - p[0][0]) * (p[2][1] - p[0][1]) - (p[1][1] - p[0][1]) * (p[2][0] - p[0][0])
    if area2 == 0:
        return None
    return p, (1 if area2 > 0 else -1)


def edge_values(p, sign, r, c):
    """Python-int edge value of the sample of pixel (r, c) against the edge opposite each corner, positive inside; and the edge value's
    rate of change along +x and +y (what decides a sample that lies exactly on the edge)."""
    sx, sy = 256 * c + 128, 256 * r + 128
    out = []
    for a, b in ((1, 2), (2, 0), (0, 1)):
        ex, ey = p[b][0] - p[a][0], p[b][1] - p[a][1]
        w = sign * (ex * (sy - p[a][1]) - ey * (sx - p[a][0]))
        out.append((w, -sign * ey, sign * ex))
    return out


def covers(p, sign, r, c):
    """The sample belongs to the triangle iff the point moved by (eps, eps^2), eps -> 0+, is strictly inside: a point on a left edge
    moves in, on a right edge out; on a horizontal edge only the move along +y (down) counts.  In integers: (w, dw/dx, dw/dy) is
    lexicographically positive for every edge."""
    return all(e > (0, 0, 0) for e in edge_values(p, sign, r, c))


def facing_front(sign):
    """Pixel y points down: the geometric normal (v1 - v0) x (v2 - v0) faces the camera iff the doubled area in pixel coordinates is negative."""
    return sign < 0


def coverage_int(records, triangles, H, W, cull='none'):
    """records [V, 4] (X, Y, depth bits, flags) of ONE camera, triangles [T, 3] -> {(r, c): [triangle, ...]} of the covering triangles.
    Skipped like the definition says: an index outside [0, V), a flagged vertex, zero area, the culling mode."""
    V = len(records)
    cover = {}
    for t, tri in enumerate(np.asarray(triangles).reshape(-1, 3).tolist()):
        if any(i < 0 or i >= V for i in tri) or any(int(records[i][3]) != 0 for i in tri):
            continue
        o = _oriented(records, tri)
        if o is None:
            continue
        p, sign = o
        if (cull == 'back' and not facing_front(sign)) or (cull == 'front' and facing_front(sign)):
            continue
        xs, ys = [q[0] for q in p], [q[1] for q in p]
        for r in range(max(min(ys) // 256 - 1, 0), min(max(ys) // 256 + 1, H - 1) + 1):
            for c in range(max(min(xs) // 256 - 1, 0), min(max(xs) // 256 + 1, W - 1) + 1):
                if covers(p, sign, r, c):
                    cover.setdefault((r, c), []).append(t)
    return cover


def barycentrics64(records, tri, r, c):
    """Perspective-correct barycentrics (float64) of the sample and the view depth: b_i ~ w_i / d_i, depth = |A2| / sum(w_i / d_i)."""
    p, sign = _oriented(records, tri)
    d = record_depths(records)
    w = [e[0] for e in edge_values(p, sign, r, c)]
    q = [w[k] / d[tri[k]] for k in range(3)]
    s = q[0] + q[1] + q[2]
    return [x / s for x in q], sum(w) / s, sign


def depth64(records, tri, r, c):
    return barycentrics64(records, tri, r, c)[1]


def shade64(records, vertices, tri, r, c, light, normals=None, colors=None, labels=None, two_sided=True, ambient=0.3, diffuse=0.7,
            base_color=(1.0, 1.0, 1.0)):
    """-> (rgb [3], label or None, barycentrics [3]) of one pixel of one triangle in float64."""
    b, _, sign = barycentrics64(records, tri, r, c)
    v = np.asarray(vertices, dtype=np.float64)
    if normals is not None:
        n = sum(b[k] * np.asarray(normals, dtype=np.float64)[tri[k]] for k in range(3))
    else:
        n = np.cross(v[tri[1]] - v[tri[0]], v[tri[2]] - v[tri[0]])
    length = math.sqrt(float(n @ n))
    n = n / length if length > 0 else n * 0
    if two_sided and not facing_front(sign):
        n = -n
    shade = ambient + diffuse * max(0.0, float(n @ np.asarray(light, dtype=np.float64)))
    if colors is not None:
        base = sum(b[k] * np.asarray(colors, dtype=np.float64)[tri[k]] for k in range(3)) / 255
    else:
        base = np.asarray(base_color, dtype=np.float64)
    label = None if labels is None else int(np.asarray(labels)[tri[int(np.argmax(b))]])
    return np.clip(base * shade, 0, 1), label, b


def check_triangle_map(tri_map, records, triangles, H, W, cull='none'):
    """The winner of every pixel against coverage_int and depth64 -> (covered pixels, pixels that used the near-tie allowance).
    A pixel nobody covers must be -1.  The winner must be the covering triangle of least float64 depth (the lowest index among exactly
    equal depths); another COVERING triangle is allowed only when its float64 depth is within NEAR_TIE_REL of the least."""
    cover = coverage_int(records, triangles, H, W, cull)
    tris = np.asarray(triangles).reshape(-1, 3).tolist()
    used = 0
    for r in range(H):
        for c in range(W):
            got, cands = int(tri_map[r][c]), cover.get((r, c))
            if not cands:
                assert got == -1, f'pixel ({r}, {c}): triangle {got} where nothing covers'
                continue
            depths = {t: depth64(records, tris[t], r, c) for t in cands}
            best = min(cands, key=lambda t: (depths[t], t))
            if got != best:
                assert got in depths, f'pixel ({r}, {c}): triangle {got} does not cover it (covering: {cands})'
                assert depths[got] <= depths[best] * (1 + NEAR_TIE_REL), f'pixel ({r}, {c}): {got} at {depths[got]} beats {best} at {depths[best]}'
                used += 1
    return len(cover), used


# float32 shading against shade64 on the same integers, u = 2^-24, per pixel (every quantity below comes from the float64 side):
#   barycentrics  q_i = float(w_i) / d_i: 2u; their sum: + 2u; b_i = q_i / sum: + u -> 7u relative, b_i <= 1 so 7u absolute.
#   smooth normal sum b_i n_i, |n_i| <= 1: (7u + u) per product, two additions: 26u per component, sqrt(3) 26u = 45u as a vector,
#                 45u / |sum| relative to its length.
#   flat normal   e = v_b - v_a: u relative; each product of the cross product 3u, the difference u: 7u |e1| |e2| per component,
#                 sqrt(3) 7u = 12.2u as a vector, 12.2u / sin(angle between the edges) relative to |e1 x e2|.
#   unit normal   twice the relative error above (direction, then length) + 5u for the squares, sums, root and division.
#   n . l         error of n times |l| (<= 1.001) + 5u;  shade = ambient + diffuse n.l: diffuse times that + 2u.
#   base          interpolated colours: 255 (8u per product, 3 products, 2u for the sums) / 255 + u = 27u; a constant colour: u.
#   pixel         d_shade * base + d_base * shade + u  <=  d_shade + d_base (ambient + diffuse) + u      (base <= 1)
U24 = 2.0 ** -24


def shading_bound(records, vertices, tri, r, c, normals, colors, ambient, diffuse):
    v = np.asarray(vertices, dtype=np.float64)
    if normals is not None:
        b = barycentrics64(records, tri, r, c)[0]
        rel = 45 * U24 / np.linalg.norm(sum(b[k] * np.asarray(normals, dtype=np.float64)[tri[k]] for k in range(3)))
    else:
        e1, e2 = v[tri[1]] - v[tri[0]], v[tri[2]] - v[tri[0]]
        rel = 12.2 * U24 / (np.linalg.norm(np.cross(e1, e2)) / (np.linalg.norm(e1) * np.linalg.norm(e2)))
    d_shade = diffuse * ((2 * rel + 5 * U24) * 1.001 + 5 * U24) + 2 * U24
    return d_shade + (27 * U24 if colors is not None else U24) * (ambient + diffuse) + U24


def check_shading(out, records, vertices, triangles, light, normals=None, colors=None, labels=None, two_sided=True, ambient=0.3,
                  diffuse=0.7, base_color=(1.0, 1.0, 1.0)):
    """`out`: depth [1, H, W], triangle [H, W], image [3, H, W][, label [H, W]] of ONE camera.  Every foreground pixel against depth64
    (DEPTH_REL) and shade64 (shading_bound); labels exactly, after checking in float64 that the two largest barycentrics of the pixel are
    further apart than their float32 error (2 * 7u) -> worst error / bound over the image (for the record)."""
    tris = np.asarray(triangles).reshape(-1, 3).tolist()
    worst = 0.0
    for r, c in zip(*np.nonzero(out['triangle'] >= 0)):
        tri = tris[int(out['triangle'][r, c])]
        want = depth64(records, tri, int(r), int(c))
        assert abs(float(out['depth'][0, r, c]) - want) <= DEPTH_REL * want, (r, c)
        rgb, label, b = shade64(records, vertices, tri, int(r), int(c), light, normals=normals, colors=colors, labels=labels, two_sided=two_sided,
                                ambient=ambient, diffuse=diffuse, base_color=base_color)
        bound = shading_bound(records, vertices, tri, int(r), int(c), normals, colors, ambient, diffuse)
        err = float(np.abs(out['image'][:, r, c].astype(np.float64) - rgb).max())
        assert err <= bound, f'pixel ({r}, {c}): image error {err:.3e} > bound {bound:.3e}'
        worst = max(worst, err / bound)
        if labels is not None:
            top = sorted(b)
            assert top[2] - top[1] > 14 * U24, f'pixel ({r}, {c}): the test input has a barycentric tie'
            assert int(out['label'][r, c]) == label, (r, c)
    bgd = out['triangle'] < 0
    assert np.isinf(out['depth'][0][bgd]).all() and (labels is None or (out['label'][bgd] == -1).all())
    return worst


# ---- meshes ---------------------------------------------------------------------------------------------------------------------
# The small meshes are laid out on the SCREEN of `head_on_camera` with fov = 90 degrees (f = 1 exactly) and power-of-two image sizes
# and depths, so that a vertex meant to sit on a multiple of 1/8 pixel is there exactly after the float32 projection.

FOV_EXACT = 90.0


def head_on_camera(distance, shift=(0.0, 0.0)):
    """cam2world of a camera at (shift, distance) looking down -z, y up (a small `shift` takes the samples off a mesh's symmetry planes)."""
    c = np.eye(4)
    c[0, 3], c[1, 3], c[2, 3] = shift[0], shift[1], distance
    return c[None]


def looking_away_camera(distance):
    """The same position, turned by 180 degrees about y: everything is behind it."""
    c = np.diag([-1.0, 1.0, -1.0, 1.0])
    c[2, 3] = distance
    return c[None]


def screen_to_world(px, py, d, H, W, distance=4.0):
    """World point that `head_on_camera(distance)` with fov 90 sees at pixel coordinates (px, py) (align_corners=False) at view depth d."""
    return [(px - W / 2) / (W / 2) * d, -(py - H / 2) / (H / 2) * d, distance - d]


def offsets64():
    """The 64 sub-pixel offsets (i / 8, j / 8): (4/8, 4/8) puts vertices laid out on x.0 coordinates exactly on sample points."""
    return [(i / 8, j / 8) for j in range(8) for i in range(8)]


def split_quad(ox=0.0, oy=0.0, H=16, W=16):
    """An 8 x 8 pixel square with corners on half-pixel coordinates + (ox, oy), split along the diagonal A-C, corner depths 1, 2, 2, 1:
    at offset (0, 0) all four corners and the diagonal lie exactly on sample points -> (vertices, triangles, (x0, y0, x1, y1))."""
    x0, y0, x1, y1 = 2.5 + ox, 2.5 + oy, 10.5 + ox, 10.5 + oy
    pts = [(x0, y0, 1.0), (x1, y0, 2.0), (x1, y1, 2.0), (x0, y1, 1.0)]
    v = np.array([screen_to_world(px, py, d, H, W) for px, py, d in pts], dtype=np.float32)
    return v, np.array([[0, 1, 2], [0, 2, 3]], dtype=np.int32), (x0, y0, x1, y1)


def closed_fan(ox=0.0, oy=0.0, H=16, W=16, k=7):
    """k triangles around a centre at (8.5, 8.5) + (ox, oy) (on a sample point at offset (0, 0)), the ring on multiples of 1/8 pixel near
    a circle of radius 6 -> (vertices, triangles, ring polygon in pixel coordinates)."""
    ring = [(round((8.5 + 6 * math.cos(2 * math.pi * i / k + 0.3)) * 8) / 8 + ox, round((8.5 + 6 * math.sin(2 * math.pi * i / k + 0.3)) * 8) / 8 + oy)
            for i in range(k)]
    pts = [(8.5 + ox, 8.5 + oy, 1.0)] + [(x, y, 2.0) for x, y in ring]
    v = np.array([screen_to_world(px, py, d, H, W) for px, py, d in pts], dtype=np.float32)
    t = np.array([[0, 1 + i, 1 + (i + 1) % k] for i in range(k)], dtype=np.int32)
    return v, t, ring


def interpenetrating_pair(H=32, W=32):
    """Two triangles that cross in depth along a line through the image."""
    pts = [(3.2, 4.1, 1.0), (29.3, 6.7, 3.0), (9.6, 28.4, 2.2), (28.1, 27.3, 1.1), (2.7, 25.2, 2.9), (17.4, 2.3, 2.1)]
    v = np.array([screen_to_world(px, py, d, H, W) for px, py, d in pts], dtype=np.float32)
    return v, np.array([[0, 1, 2], [3, 4, 5]], dtype=np.int32)


SPHERE_N, SPHERE_VOXELS = 24, 8.0
SPHERE_RADIUS = SPHERE_VOXELS / SPHERE_N          # world units


def sphere_mesh():
    """A sphere of radius 8 voxels meshed at 24^3 by `marching_cubes_host`, centred at the origin, one voxel = 1 / 24
    -> (vertices float32, triangles int32, normals float32)."""
    from training import mesh_extraction as me
    g = np.mgrid[0:SPHERE_N, 0:SPHERE_N, 0:SPHERE_N].astype(np.float64)
    vol = SPHERE_VOXELS - np.sqrt(((g - (SPHERE_N - 1) / 2) ** 2).sum(0))
    v, t, n = me.marching_cubes_host(vol.astype(np.float32), 0.0, normals=True)
    return ((v - (SPHERE_N - 1) / 2) / SPHERE_N).astype(np.float32), t, n.astype(np.float32)


def tiny_triangles(count, H, W, seed=0, depth_range=(1.0, 3.0)):
    """`count` random triangles of 1-3 pixels on the screen of `head_on_camera` (fov 90)."""
    rng = np.random.default_rng(seed)
    centre = rng.uniform(1, [W - 1, H - 1], size=[count, 1, 2])
    corner = centre + rng.uniform(-1.5, 1.5, size=[count, 3, 2])
    d = rng.uniform(*depth_range, size=[count, 3])
    w = np.stack([(corner[..., 0] - W / 2) / (W / 2) * d, -(corner[..., 1] - H / 2) / (H / 2) * d, 4.0 - d], axis=-1)
    return w.reshape(-1, 3).astype(np.float32), np.arange(3 * count, dtype=np.int32).reshape(-1, 3)
