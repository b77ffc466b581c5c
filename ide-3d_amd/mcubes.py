"""Stand-in for the PyMCubes module the reference imports (`import mcubes`: render_mesh.py:4,31 and dnnlib/geometry.py:282,286).

With this package's directory in front on `sys.path`, `mcubes.marching_cubes(u, isovalue)` resolves here, so
`dnnlib.geometry.extract_geometry` and render_mesh.py up to its line 31 run unchanged.  Only the one function the reference
calls is provided.  Like PyMCubes it takes a numpy array (any real dtype, meshed in float64) and returns numpy arrays in index
coordinates: vertices float64 [V, 3] and triangles int64 [T, 3].  A float32 CUDA tensor is meshed by the HIP kernels
(training/mesh_extraction.py) and copied back.  Triangle normals point toward lower values; PyMCubes' own winding could not be
compared (see training/mesh_extraction.py)."""

import numpy as np
import torch

from training import mesh_extraction


def marching_cubes(u, isovalue):
    if isinstance(u, torch.Tensor) and u.is_cuda and u.dtype == torch.float32:
        vertices, triangles = mesh_extraction.marching_cubes(u, isovalue)
        return vertices.cpu().numpy().astype(np.float64), triangles.cpu().numpy().astype(np.int64)
    if isinstance(u, torch.Tensor):
        u = u.detach().cpu().numpy()
    vertices, triangles, _ = mesh_extraction.marching_cubes_host(np.asarray(u, dtype=np.float64), isovalue)
    return vertices, triangles.astype(np.int64)
