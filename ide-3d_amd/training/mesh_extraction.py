"""Iso-surface meshes from the density cube: the `mcubes.marching_cubes(volume, threshold)` step of render_mesh.py:31 and
dnnlib/geometry.py:281-291 (`extract_geometry`), which the reference delegates to PyMCubes.

The case table is GENERATED (`case_table()`), not typed in.  Conventions: cell corner c = x + 2y + 4z (bit 0 is the step along
volume axis 0), corner bit set <=> value > threshold (strict), the 12 edges are the corner pairs that differ in one bit in
ascending (a, b) order.  Construction: on each of the 6 faces, taken counter-clockwise as seen from outside the cell, every
maximal run of inside corners is cut off by ONE directed segment from the edge where the run starts to the edge where it ends.
On a face with four crossings the two inside corners are therefore always separated, and because the rule reads the face's
corner signs only, the two cells that share a face draw the same segments in opposite directions: the mesh has no cracks.  The
segments chain into closed loops over edge ids; each loop is fan-triangulated from its first edge.  This gives at most 5
triangles per case, 820 over the 256 cases, and triangles whose normals point toward LOWER values (outward for a density;
`flip=True` reverses the winding for signed-distance-style volumes).  PyMCubes' own winding cannot be checked here (the package
is not available to compare against): a consumer that depends on it should test its orientation once and pass `flip`.

Vertices lie on grid edges: p_a + t (p_b - p_a), t = (threshold - v_a) / (v_b - v_a).  Every crossing edge is owned by its
lower end point (the +x, +y, +z edges of a grid point), vertices are numbered by owning point in memory order, x before y
before z, and triangles by cell in memory order, then table order: the output order is a function of the grid shape and the
data only.  `marching_cubes` runs csrc/mesh.hip for float32 CUDA volumes and the vectorised host
definition below otherwise; both produce the same vertices and triangles in the same order.
"""

import functools
import os

import numpy as np
import torch

CORNERS = tuple(((c >> 0) & 1, (c >> 1) & 1, (c >> 2) & 1) for c in range(8))
EDGES = tuple((a, b) for a in range(8) for b in range(a + 1, 8) if bin(a ^ b).count('1') == 1)
EDGE_AXIS = tuple((a ^ b).bit_length() - 1 for a, b in EDGES)          # 0: along volume axis 0 (x), 1: y, 2: z
_EDGE_ID = {e: i for i, e in enumerate(EDGES)}


def _edge_id(a, b):
    return _EDGE_ID[(min(a, b), max(a, b))]


def cell_faces():
    """The 6 faces as 4 corner ids each, counter-clockwise as seen from outside the cell; order: -x, +x, -y, +y, -z, +z."""
    faces = []
    for axis in range(3):
        u, v = ((1, 2), (2, 0), (0, 1))[axis]                         # u x v = +axis
        for side in (0, 1):
            cyc = []
            for du, dv in ((0, 0), (1, 0), (1, 1), (0, 1)):           # counter-clockwise seen from +axis
                p = [0, 0, 0]
                p[axis], p[u], p[v] = side, du, dv
                cyc.append(p[0] + 2 * p[1] + 4 * p[2])
            faces.append(tuple(cyc[::-1] if side == 0 else cyc))      # the outside of the low face is -axis
    return tuple(faces)


def face_segments(case, face):
    """Directed segments (from edge id, to edge id) the case draws on one face (4 corner ids, counter-clockwise from outside)."""
    s = [(case >> c) & 1 for c in face]
    segs = []
    for i in range(4):
        if s[i] == 0 and s[(i + 1) % 4] == 1:                         # a run of inside corners starts behind face edge i
            j = (i + 1) % 4
            while s[(j + 1) % 4] == 1:
                j = (j + 1) % 4
            segs.append((_edge_id(face[i], face[(i + 1) % 4]), _edge_id(face[j], face[(j + 1) % 4])))
    return segs


@functools.lru_cache(maxsize=None)
def case_table():
    """256 tuples of triangles; a triangle is 3 edge ids (indices into EDGES)."""
    faces = cell_faces()
    table = []
    for case in range(256):
        nxt = {}
        for face in faces:
            for a, b in face_segments(case, face):
                assert a not in nxt
                nxt[a] = b
        tris, seen = [], set()
        for start in nxt:
            if start in seen:
                continue
            loop, k = [start], nxt[start]
            seen.add(start)
            while k != start:
                loop.append(k)
                seen.add(k)
                k = nxt[k]
            tris += [(loop[0], loop[t], loop[t + 1]) for t in range(1, len(loop) - 1)]
        table.append(tuple(tris))
    return tuple(table)


@functools.lru_cache(maxsize=None)
def case_table_bytes():
    """The table as the kernels read it: uint8 [256, 16], byte 0 = number of triangles, bytes 1..15 = their edge ids."""
    out = np.zeros([256, 16], dtype=np.uint8)
    for case, tris in enumerate(case_table()):
        out[case, 0] = len(tris)
        out[case, 1:1 + 3 * len(tris)] = np.array(tris, dtype=np.uint8).reshape(-1)
    out.setflags(write=False)
    return out


# ---- host definition ---------------------------------------------------------------------------------------------------------

def _gradient_at(v, idx):
    """Central differences of v at integer points idx [n, 3], one-sided at the border (0 along an axis of length 1) -> [n, 3]."""
    g = np.zeros([idx.shape[0], 3], dtype=v.dtype)
    for ax in range(3):
        n = v.shape[ax]
        hi, lo = idx.copy(), idx.copy()
        hi[:, ax] = np.minimum(idx[:, ax] + 1, n - 1)
        lo[:, ax] = np.maximum(idx[:, ax] - 1, 0)
        d = v[hi[:, 0], hi[:, 1], hi[:, 2]] - v[lo[:, 0], lo[:, 1], lo[:, 2]]
        g[:, ax] = np.where(hi[:, ax] - lo[:, ax] == 2, d * v.dtype.type(0.5), d)
    return g


def marching_cubes_host(volume, threshold, normals=False, flip=False, lattice=None):
    """The definition on numpy arrays, in the volume's own floating-point type (float32 or float64) ->
    (vertices [V, 3], triangles [T, 3] int32, normals [V, 3] or None)."""
    v = np.ascontiguousarray(volume)
    if v.dtype not in (np.float32, np.float64):
        v = v.astype(np.float32)
    assert v.ndim == 3, 'volume must be [X, Y, Z]'
    ft = v.dtype.type
    iso = ft(threshold)
    X, Y, Z = v.shape
    ins = v > iso
    # owned crossing edges of every grid point: [X, Y, Z, 3]; flat index = point * 3 + axis is the vertex order
    cross = np.zeros([X, Y, Z, 3], dtype=bool)
    cross[:-1, :, :, 0] = ins[:-1] != ins[1:]
    cross[:, :-1, :, 1] = ins[:, :-1] != ins[:, 1:]
    cross[:, :, :-1, 2] = ins[:, :, :-1] != ins[:, :, 1:]
    flat = np.flatnonzero(cross)
    if flat.size >= 2 ** 31:
        raise RuntimeError(f'marching_cubes: {flat.size} vertices do not fit int32 indices')
    point, axis = flat // 3, flat % 3
    pa = np.stack(np.unravel_index(point, (X, Y, Z)), axis=1)
    pb = pa.copy()
    pb[np.arange(pa.shape[0]), axis] += 1
    va, vb = v[pa[:, 0], pa[:, 1], pa[:, 2]], v[pb[:, 0], pb[:, 1], pb[:, 2]]
    t = (iso - va) / (vb - va)
    verts = pa.astype(v.dtype)
    verts[np.arange(pa.shape[0]), axis] += t
    nrm = None
    if normals:
        ga, gb = _gradient_at(v, pa), _gradient_at(v, pb)
        g = ga + t[:, None] * (gb - ga)
        if not flip:
            g = -g
        length = np.sqrt((g * g).sum(axis=1, keepdims=True))
        nrm = np.where(length > 0, g / np.where(length > 0, length, 1), 0).astype(v.dtype)
    if lattice is not None:
        voxel_size, corner, scale = lattice
        c = np.array([corner[2], corner[1], corner[0]], dtype=np.float32).astype(v.dtype)      # axis order of shape_extraction.lattice_points
        verts = (verts * ft(np.float32(voxel_size)) + c) * ft(np.float32(scale))
    # triangles
    tris = np.zeros([0, 3], dtype=np.int32)
    if min(X, Y, Z) >= 2 and flat.size:
        case = np.zeros([X - 1, Y - 1, Z - 1], dtype=np.uint8)
        for c, (dx, dy, dz) in enumerate(CORNERS):
            case |= ins[dx:X - 1 + dx, dy:Y - 1 + dy, dz:Z - 1 + dz].astype(np.uint8) << c
        table = case_table_bytes()
        cells = np.flatnonzero(table[:, 0][case])
        if cells.size:
            cc = case.reshape(-1)[cells]
            cxyz = np.stack(np.unravel_index(cells, case.shape), axis=1)
            edges = table[cc, 1:].reshape(-1, 5, 3).astype(np.int64)
            keep = np.arange(5)[None, :] < table[cc, 0][:, None]
            corner_a = np.array([a for a, _ in EDGES])[edges]                                    # [n, 5, 3]
            own = cxyz[:, None, None, :] + np.array(CORNERS)[corner_a]                           # [n, 5, 3, 3]
            own_flat = ((own[..., 0] * Y + own[..., 1]) * Z + own[..., 2]) * 3 + np.array(EDGE_AXIS)[edges]
            own_flat = own_flat[keep]                                                            # cell-major, then table order
            if own_flat.shape[0] >= 2 ** 31:
                raise RuntimeError(f'marching_cubes: {own_flat.shape[0]} triangles do not fit int32 indices')
            vid = np.cumsum(cross.reshape(-1), dtype=np.int32) - 1                               # vertex id of every crossing edge
            tris = vid[own_flat].astype(np.int32)
    if flip:
        tris = tris[:, [0, 2, 1]]
    return verts, np.ascontiguousarray(tris), nrm


def marching_cubes(volume, threshold, *, normals=False, flip=False, lattice=None):
    """`mcubes.marching_cubes(volume, threshold)` on a torch tensor [X, Y, Z] ->
    (vertices [V, 3] float32, triangles [T, 3] int32[, normals [V, 3] float32]) on the volume's device.

    Vertices are in index units (what PyMCubes returns), or, with `lattice=(voxel_size, corner, scale)`, in the world coordinates
    of `shape_extraction.density_cube`: scale * (index * voxel_size + corner) with volume axes 0, 1, 2 taking corner[2], corner[1],
    corner[0] like `shape_extraction.lattice_points`.  Triangle normals (and `normals=True` vertex normals: the normalised,
    interpolated central-difference gradient, zero where the gradient is zero) point toward lower values; `flip=True` reverses both.
    A float32 CUDA volume runs the HIP kernels (no fallback: an unusable library raises); anything else runs `marching_cubes_host`
    in the volume's precision (float64 volumes are meshed in float64 and rounded once at the end)."""
    assert isinstance(volume, torch.Tensor) and volume.ndim == 3, 'volume must be a [X, Y, Z] tensor'
    if volume.is_cuda and volume.dtype == torch.float32:
        from torch_utils import hip_plugin
        hip_plugin.load()
        v, t, n = hip_plugin.MeshPlugin.marching_cubes(volume, float(threshold), torch.from_numpy(case_table_bytes().copy()), normals=normals, flip=flip, lattice=lattice)
    else:
        src = volume.detach().cpu()
        if not src.dtype.is_floating_point or src.dtype in (torch.float16, torch.bfloat16):
            src = src.float()
        v, t, n = marching_cubes_host(src.numpy(), threshold, normals=normals, flip=flip, lattice=lattice)
        v = torch.from_numpy(v.astype(np.float32)).to(volume.device)
        t = torch.from_numpy(t).to(volume.device)
        n = torch.from_numpy(n.astype(np.float32)).to(volume.device) if normals else None
    return (v, t, n) if normals else (v, t)


# ---- generator -> mesh -------------------------------------------------------------------------------------------------------

def extract_mesh(G, z_or_ws, c=None, *, voxel_resolution=256, voxel_origin=(0, 0, 0), cube_length=2.0, threshold=10.0, psi=0.5,
                 noise_mode='const', normals=False, flip=False, vertex_attributes=False, max_batch=None):
    """Generator -> density cube -> mesh in world coordinates without leaving the device (extract_shapes.py:99-150 followed by
    dnnlib/geometry.py:281-291).  `z_or_ws`: z [1, z_dim] (mapped with `c` and `psi`) or ws [1, num_ws, w_dim].

    The vertices use the lattice of `density_cube`: corner = voxel_origin - cube_length / 2, voxel_size = cube_length / (N - 1) and
    the 0.9 scale, axes as in `lattice_points`.  The reference evaluates the density at points whose second and third index are
    not floored (a sub-voxel shear, kept by `density_cube` for parity); vertex positions here use the integer lattice, so that
    shear is NOT reproduced in them.

    Returns a dict: vertices [V, 3] float32, triangles [T, 3] int32, optionally normals [V, 3]; with `vertex_attributes=True` one
    `renderer.sample_voxel` call at the vertices adds colors [V, 3] uint8 (the first three feature channels, [-1, 1] -> [0, 255])
    and labels [V] int64 (argmax of the semantic logits)."""
    from training import shape_extraction as se
    with torch.no_grad():
        if z_or_ws.ndim == 3:
            ws = z_or_ws
        else:
            ws = G.mapping(z_or_ws, c, truncation_psi=psi)
        assert ws.shape[0] == 1, 'extract_mesh: one generator sample at a time'
        img_v, seg_v = se.triplanes_from_ws(G.synthesis, ws, noise_mode=noise_mode)
        renderer = G.synthesis.renderer
        scale = 0.9
        cube = se.density_cube(renderer, img_v, seg_v, voxel_resolution=voxel_resolution, max_batch=max_batch, voxel_origin=voxel_origin,
                               cube_length=cube_length, scale=scale)[0]
        corner = np.array(voxel_origin) - cube_length / 2
        voxel_size = cube_length / (voxel_resolution - 1)
        res = marching_cubes(cube, threshold, normals=normals, flip=flip, lattice=(voxel_size, corner, scale))
        out = {'vertices': res[0], 'triangles': res[1]}
        if normals:
            out['normals'] = res[2]
        if vertex_attributes:
            out.update(vertex_attributes_at(renderer, img_v, seg_v, out['vertices']))
    return out


def vertex_attributes_at(renderer, img_v, seg_v, vertices):
    """One `renderer.sample_voxel` call at world points [V, 3] -> {'colors': [V, 3] uint8, 'labels': [V] int64}."""
    dec = renderer.decoder
    if vertices.shape[0] == 0:
        return {'colors': torch.zeros([0, 3], dtype=torch.uint8, device=vertices.device),
                'labels': torch.zeros([0], dtype=torch.int64, device=vertices.device)}
    feat = renderer.sample_voxel(img_v, seg_v, vertices.unsqueeze(0))
    colors = (feat[:, :3] * 127.5 + 128).clamp(0, 255).to(torch.uint8)
    labels = feat[:, dec.feature_channels:dec.feature_channels + dec.seg_channels].argmax(dim=1)
    return {'colors': colors, 'labels': labels}


# ---- files -------------------------------------------------------------------------------------------------------------------

def _np(a, dtype):
    if isinstance(a, torch.Tensor):
        a = a.detach().cpu().numpy()
    return np.ascontiguousarray(a, dtype=dtype)


def write_ply(path, vertices, triangles, normals=None, colors=None, labels=None):
    """Binary little-endian PLY: vertex x y z [nx ny nz] [red green blue] [label], face vertex_indices (uchar count, int index)."""
    v, f = _np(vertices, '<f4').reshape(-1, 3), _np(triangles, '<i4').reshape(-1, 3)
    fields, cols = [('x', '<f4'), ('y', '<f4'), ('z', '<f4')], [v[:, 0], v[:, 1], v[:, 2]]
    if normals is not None:
        n = _np(normals, '<f4').reshape(-1, 3)
        fields += [('nx', '<f4'), ('ny', '<f4'), ('nz', '<f4')]
        cols += [n[:, 0], n[:, 1], n[:, 2]]
    if colors is not None:
        c = _np(colors, 'u1').reshape(-1, 3)
        fields += [('red', 'u1'), ('green', 'u1'), ('blue', 'u1')]
        cols += [c[:, 0], c[:, 1], c[:, 2]]
    if labels is not None:
        fields += [('label', '<i4')]
        cols += [_np(labels, '<i4').reshape(-1)]
    assert all(col.shape[0] == v.shape[0] for col in cols), 'write_ply: per-vertex arrays must have one row per vertex'
    names = {'<f4': 'float', 'u1': 'uchar', '<i4': 'int'}
    header = ['ply', 'format binary_little_endian 1.0', f'element vertex {v.shape[0]}']
    header += [f'property {names[t]} {name}' for name, t in fields]
    header += [f'element face {f.shape[0]}', 'property list uchar int vertex_indices', 'end_header']
    vrec = np.empty(v.shape[0], dtype=fields)
    for (name, _), col in zip(fields, cols):
        vrec[name] = col
    frec = np.empty(f.shape[0], dtype=[('n', 'u1'), ('idx', '<i4', (3,))])
    frec['n'], frec['idx'] = 3, f
    with open(path, 'wb') as fh:
        fh.write(('\n'.join(header) + '\n').encode('ascii'))
        fh.write(vrec.tobytes())
        fh.write(frec.tobytes())


def read_ply(path):
    """Inverse of `write_ply` (triangle faces only) -> dict of numpy arrays: vertices, triangles and whichever of normals, colors,
    labels the file has."""
    types = {'float': '<f4', 'uchar': 'u1', 'int': '<i4'}
    with open(path, 'rb') as fh:
        assert fh.readline().strip() == b'ply'
        assert fh.readline().strip() == b'format binary_little_endian 1.0', 'read_ply: binary little-endian files only'
        counts, fields, element = {}, [], None
        while True:
            line = fh.readline().decode('ascii').split()
            if line[0] == 'end_header':
                break
            if line[0] == 'element':
                element = line[1]
                counts[element] = int(line[2])
            elif line[0] == 'property' and element == 'vertex':
                fields.append((line[2], types[line[1]]))
            elif line[0] == 'property' and element == 'face':
                assert line[1:] == ['list', 'uchar', 'int', 'vertex_indices']
        vrec = np.frombuffer(fh.read(counts['vertex'] * np.dtype(fields).itemsize), dtype=fields)
        fdt = np.dtype([('n', 'u1'), ('idx', '<i4', (3,))])
        frec = np.frombuffer(fh.read(counts['face'] * fdt.itemsize), dtype=fdt)
    assert (frec['n'] == 3).all(), 'read_ply: triangles only'
    out = {'vertices': np.stack([vrec['x'], vrec['y'], vrec['z']], axis=1), 'triangles': frec['idx'].copy()}
    have = {name for name, _ in fields}
    if 'nx' in have:
        out['normals'] = np.stack([vrec['nx'], vrec['ny'], vrec['nz']], axis=1)
    if 'red' in have:
        out['colors'] = np.stack([vrec['red'], vrec['green'], vrec['blue']], axis=1)
    if 'label' in have:
        out['labels'] = vrec['label'].copy()
    return out


def save_mesh(outdir, name, vertices, triangles, normals=None, colors=None, labels=None):
    """`<outdir>/<name>.ply` (the file extract_shapes.py:195-219 writes through plyfile) -> its path."""
    os.makedirs(outdir, exist_ok=True)
    path = os.path.join(outdir, f'{name}.ply')
    write_ply(path, vertices, triangles, normals=normals, colors=colors, labels=labels)
    return path
