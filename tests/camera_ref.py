"""The three pose functions of training/volumetric_rendering.py (sample_camera_positions after its draw, create_cam2world_matrix,
LookAtPoseSampler.sample after its draw) restated for explicit inputs of any dtype on any device: in float64 on the CPU they are the reference
of tests/test_gpu_camera.py, in fp32 on the device its ATen comparison.  tests/test_camera_resample_cases_cpu.py pins them to the product's
own chain."""

import math

import torch


def sphere_ref(theta, pitch, r, pitch_is_v=False):
    p = torch.clamp(pitch, 1e-5, math.pi - 1e-5)
    if pitch_is_v:
        p = torch.arccos(1 - 2 * (p / math.pi))
    return torch.cat([r * torch.sin(p) * torch.cos(theta), r * torch.cos(p), r * torch.sin(p) * torch.sin(theta)], dim=-1), p


def _normalize(v):
    return v / torch.norm(v, dim=-1, keepdim=True)


def cam2world_ref(forward, origin):
    f = _normalize(forward)
    up = torch.tensor([0.0, 1.0, 0.0], dtype=f.dtype, device=f.device).expand_as(f)
    left = _normalize(torch.cross(up, f, dim=-1))
    up = _normalize(torch.cross(f, left, dim=-1))
    n = f.shape[0]
    rot = torch.eye(4, dtype=f.dtype, device=f.device).repeat(n, 1, 1)
    rot[:, :3, :3] = torch.stack((-left, up, -f), dim=-1)
    trans = torch.eye(4, dtype=f.dtype, device=f.device).repeat(n, 1, 1)
    trans[:, :3, 3] = origin
    return trans @ rot          # a product: a NaN of the rotation reaches its whole column, the last row included


def lookat_ref(h, v, lookat, radius):
    origins, _ = sphere_ref(h, v, radius, pitch_is_v=True)
    return cam2world_ref(_normalize(lookat - origins), origins)
