"""Marching cubes as plain loops in float64: the yardstick of tests/test_mesh_cpu.py and tests/test_gpu_mesh.py.

Independent of the vectorised code in training/mesh_extraction.py except for the case table itself (`case_table()`, whose
properties test_mesh_cpu.py checks exhaustively): vertices live in a dict keyed on grid edges, cells are visited one by one.
Also the mesh measurements the tests share (half-edge closure, Euler characteristic, signed volume, canonical forms) and the
three test volumes."""
import numpy as np


def reference_mesh(volume, iso, table, edges):
    """-> (vertices [V, 3] float64, triangles [T, 3] int64); `table` = case_table(), `edges` = the 12 corner pairs."""
    vol = np.asarray(volume, dtype=np.float64)
    X, Y, Z = vol.shape
    corner = [((c >> 0) & 1, (c >> 1) & 1, (c >> 2) & 1) for c in range(8)]
    ids, verts, tris = {}, [], []
    for i in range(X - 1):
        for j in range(Y - 1):
            for k in range(Z - 1):
                case = 0
                for c, (dx, dy, dz) in enumerate(corner):
                    if vol[i + dx, j + dy, k + dz] > iso:
                        case |= 1 << c
                for tri in table[case]:
                    out = []
                    for e in tri:
                        a, b = edges[e]
                        pa = (i + corner[a][0], j + corner[a][1], k + corner[a][2])
                        pb = (i + corner[b][0], j + corner[b][1], k + corner[b][2])
                        if (pa, pb) not in ids:
                            va, vb = vol[pa], vol[pb]
                            t = (iso - va) / (vb - va)
                            ids[(pa, pb)] = len(verts)
                            verts.append([pa[n] + t * (pb[n] - pa[n]) for n in range(3)])
                        out.append(ids[(pa, pb)])
                    tris.append(out)
    return np.array(verts, dtype=np.float64).reshape(-1, 3), np.array(tris, dtype=np.int64).reshape(-1, 3)


# ---- the test volumes ----------------------------------------------------------------------------------------------------------

SPHERE_N, SPHERE_R = 24, 9.0
SPHERE_CENTRE = (SPHERE_N - 1) / 2 + np.array([0.13, -0.21, 0.37])


def sphere_volume(n=SPHERE_N, radius=SPHERE_R, offset=(0.13, -0.21, 0.37)):
    """radius - r around (n - 1) / 2 + offset: inside (high) within the sphere, iso 0."""
    g = np.mgrid[0:n, 0:n, 0:n].astype(np.float64)
    c = (n - 1) / 2 + np.array(offset)
    return radius - np.sqrt(((g - c[:, None, None, None]) ** 2).sum(0))


def torus_volume(n=24, major=7.0, minor=3.0):
    g = np.mgrid[0:n, 0:n, 0:n].astype(np.float64)
    c = (n - 1) / 2 + np.array([0.13, -0.21, 0.37])
    q = np.sqrt((g[0] - c[0]) ** 2 + (g[1] - c[1]) ** 2) - major
    return minor - np.sqrt(q ** 2 + (g[2] - c[2]) ** 2)


def noise_volume(shape=(14, 14, 14), seed=0, border=-5.0):
    """Seeded normal noise; with `border` every border face is set to that (outside) value."""
    v = np.random.default_rng(seed).standard_normal(shape)
    if border is not None:
        v[0] = v[-1] = border
        v[:, 0] = v[:, -1] = border
        v[:, :, 0] = v[:, :, -1] = border
    return v


# ---- measurements --------------------------------------------------------------------------------------------------------------

def half_edges(tris):
    he = {}
    for t in np.asarray(tris).tolist():
        for a, b in ((t[0], t[1]), (t[1], t[2]), (t[2], t[0])):
            he[(a, b)] = he.get((a, b), 0) + 1
    return he


def is_closed(tris):
    """Every directed half-edge appears once and its reverse once."""
    he = half_edges(tris)
    return all(n == 1 and he.get((b, a), 0) == 1 for (a, b), n in he.items())


def open_half_edges(tris):
    """Half-edges whose reverse is missing (every half-edge must still be unique)."""
    he = half_edges(tris)
    assert all(n == 1 for n in he.values())
    return [(a, b) for (a, b) in he if (b, a) not in he]


def euler(num_vertices, tris):
    """V - E + F of a closed mesh."""
    he = half_edges(tris)
    return num_vertices - len(he) // 2 + len(tris)


def signed_volume(verts, tris):
    v, t = np.asarray(verts, dtype=np.float64), np.asarray(tris)
    return float(np.einsum('ij,ij->i', v[t[:, 0]], np.cross(v[t[:, 1]], v[t[:, 2]])).sum() / 6)


def match_vertices(ref, got, tol):
    """The vertex SETS are equal within tol: a one-to-one assignment got[n] -> ref[idx[n]] with max |difference| <= tol per coordinate
    (asserted).  Found through a hash of ref on a 1e-3 grid, so no sort order can flip where two roundings disagree."""
    ref, got = np.asarray(ref, dtype=np.float64).reshape(-1, 3), np.asarray(got, dtype=np.float64).reshape(-1, 3)
    assert ref.shape == got.shape, f'{got.shape[0]} vertices, reference has {ref.shape[0]}'
    h, cells = 1e-3, {}
    for i, key in enumerate(map(tuple, np.floor(ref / h).astype(np.int64).tolist())):
        cells.setdefault(key, []).append(i)
    lo, hi = np.floor((got - tol) / h).astype(np.int64).tolist(), np.floor((got + tol) / h).astype(np.int64).tolist()
    used, idx = np.zeros(ref.shape[0], dtype=bool), np.empty(got.shape[0], dtype=np.int64)
    for n, (l, u) in enumerate(zip(lo, hi)):
        best, dist = -1, np.inf
        for kx in range(l[0], u[0] + 1):
            for ky in range(l[1], u[1] + 1):
                for kz in range(l[2], u[2] + 1):
                    for i in cells.get((kx, ky, kz), ()):
                        d = np.abs(ref[i] - got[n]).max()
                        if not used[i] and d < dist:
                            best, dist = i, d
        assert best >= 0 and dist <= tol, f'vertex {n} {got[n]} has no reference vertex within {tol} (nearest unused: {dist})'
        used[best], idx[n] = True, best
    return idx


def triangle_keys(verts, tris, decimals=4):
    """Triangles as position triples, rotated so the smallest corner comes first (winding kept), sorted."""
    v = np.round(np.asarray(verts, dtype=np.float64), decimals)
    keys = []
    for t in np.asarray(tris).tolist():
        p = [tuple(v[i]) for i in t]
        k = min(range(3), key=lambda n: p[n])
        keys.append((p[k], p[(k + 1) % 3], p[(k + 2) % 3]))
    return sorted(keys)
