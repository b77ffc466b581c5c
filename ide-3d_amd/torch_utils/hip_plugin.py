"""ctypes binding of libide3d_hip.so (C ABI: include/ide3d_hip.h).

This is the host half of the drop-in boundary.  The reference loads one pybind11 module per op
through `torch_utils.custom_ops.get_plugin` (custom_ops.py:59) and calls `_plugin.<fn>(tensors...)`
(bias_act.py:150, upfirdn2d.py:242, filtered_lrelu.py:217,228).  Here the same call shapes are kept:
every `*Plugin` class below exposes functions with the reference plugin's argument order, validates
like the reference's TORCH_CHECKs, allocates outputs with torch (memory format preserved) and hands
raw device pointers + the current HIP stream to the C ABI.  PyTorch is only plumbing (device memory,
streams); all arithmetic happens in the hand-written HIP kernels.

There is deliberately NO fallback in this file: if the shared library is missing, was built for a
different arch, or a launch fails, a RuntimeError is raised.
"""

import ctypes
import math
import os
import threading
import weakref

import torch

_LIB_ENV = 'IDE3D_HIP_LIB'          # override path of libide3d_hip.so
_ABI_VERSION = 8
AMAX_SLOTS, AMAX_STRIDE = 32, 64     # = IDE3D_AMAX_SLOTS / _STRIDE (include/ide3d_hip.h): slot k of an image's `amax` row is element k * 64
AMAX_FLOATS = AMAX_SLOTS * AMAX_STRIDE

_DTYPE_CODE = {torch.float32: 0, torch.float16: 1, torch.bfloat16: 2, torch.float64: 3}

_lock = threading.Lock()
_lib = None

# number of successful C-ABI launches per entry point (tests assert the native path really ran)
CALLS = {}


def lib_path():
    env = os.environ.get(_LIB_ENV)
    if env:
        return env
    here = os.path.dirname(os.path.abspath(__file__))
    return os.path.join(os.path.dirname(here), 'lib', 'libide3d_hip.so')


class _UpfirdnParams(ctypes.Structure):
    _fields_ = [
        ('x', ctypes.c_void_p), ('f', ctypes.c_void_p), ('y', ctypes.c_void_p),
        ('dtype', ctypes.c_int32),
        ('n', ctypes.c_int32), ('c', ctypes.c_int32), ('in_h', ctypes.c_int32), ('in_w', ctypes.c_int32),
        ('out_h', ctypes.c_int32), ('out_w', ctypes.c_int32),
        ('x_stride', ctypes.c_int64 * 4), ('y_stride', ctypes.c_int64 * 4),
        ('f_h', ctypes.c_int32), ('f_w', ctypes.c_int32),
        ('f_stride', ctypes.c_int64 * 2),
        ('up_x', ctypes.c_int32), ('up_y', ctypes.c_int32), ('down_x', ctypes.c_int32), ('down_y', ctypes.c_int32),
        ('pad_x0', ctypes.c_int32), ('pad_y0', ctypes.c_int32),
        ('flip', ctypes.c_int32), ('gain', ctypes.c_float), ('x_row_floats', ctypes.c_int32),
    ]


def _row_floats_readable(x):
    """Elements readable from the start of the row of `x` that starts last in its storage (every other row has at least as many): what
    `ide3d_upfirdn2d_params.x_row_floats` promises.  0 (no promise) for anything but positive-stride rank-4 tensors."""
    if x.ndim != 4 or any(st <= 0 for st in x.stride()):
        return 0
    last_row = x.storage_offset() + sum((x.shape[i] - 1) * x.stride(i) for i in range(3))
    total = x.untyped_storage().nbytes() // x.element_size()
    return int(max(0, min(total - last_row, 2 ** 31 - 1)))


class _UpfirdnEpilogue(ctypes.Structure):
    _fields_ = [
        ('add', ctypes.c_void_p), ('add_stride', ctypes.c_int64 * 4),
        ('noise', ctypes.c_void_p), ('noise_strength', ctypes.c_float),
        ('bias', ctypes.c_void_p),
        ('fused_act', ctypes.c_int32), ('act', ctypes.c_int32),
        ('alpha', ctypes.c_float), ('act_gain', ctypes.c_float), ('clamp', ctypes.c_float),
        ('y_amax', ctypes.c_void_p),
    ]


class _FlreluParams(ctypes.Structure):
    _fields_ = [
        ('x', ctypes.c_void_p), ('y', ctypes.c_void_p), ('b', ctypes.c_void_p), ('s', ctypes.c_void_p),
        ('fu', ctypes.c_void_p), ('fd', ctypes.c_void_p),
        ('dtype', ctypes.c_int32),
        ('n', ctypes.c_int32), ('c', ctypes.c_int32), ('in_h', ctypes.c_int32), ('in_w', ctypes.c_int32),
        ('out_h', ctypes.c_int32), ('out_w', ctypes.c_int32),
        ('x_stride', ctypes.c_int64 * 4), ('y_stride', ctypes.c_int64 * 4),
        ('fu_w', ctypes.c_int32), ('fu_h', ctypes.c_int32), ('fd_w', ctypes.c_int32), ('fd_h', ctypes.c_int32),
        ('fu_stride', ctypes.c_int64 * 2), ('fd_stride', ctypes.c_int64 * 2),
        ('up', ctypes.c_int32), ('down', ctypes.c_int32),
        ('pad_x0', ctypes.c_int32), ('pad_y0', ctypes.c_int32),
        ('s_w_bytes', ctypes.c_int32), ('s_h', ctypes.c_int32),
        ('s_ofs_x', ctypes.c_int32), ('s_ofs_y', ctypes.c_int32),
        ('sw_limit', ctypes.c_int32), ('sign_mode', ctypes.c_int32),
        ('flip', ctypes.c_int32),
        ('gain', ctypes.c_float), ('slope', ctypes.c_float), ('clamp', ctypes.c_float),
    ]


class _RenderGrads(ctypes.Structure):
    _fields_ = [
        ('grad_feat', ctypes.c_void_p), ('grad_depth', ctypes.c_void_p), ('grad_wsum', ctypes.c_void_p),
        ('grad_tex_planes', ctypes.c_void_p), ('grad_geo_planes', ctypes.c_void_p),
        ('grad_tex_stride', ctypes.c_int64 * 4), ('grad_geo_stride', ctypes.c_int64 * 4),
    ]


class _RenderParamGrads(ctypes.Structure):
    """ide3d_render_param_grads (include/ide3d_hip.h): the decoder gradients of ide3d_render_rays_backward_params."""
    _fields_ = [
        ('grad_geo_w0', ctypes.c_void_p), ('grad_geo_b0', ctypes.c_void_p), ('grad_geo_w1', ctypes.c_void_p), ('grad_geo_b1', ctypes.c_void_p),
        ('grad_tex_w0', ctypes.c_void_p), ('grad_tex_b0', ctypes.c_void_p), ('grad_tex_w1', ctypes.c_void_p), ('grad_tex_b1', ctypes.c_void_p),
        ('workspace', ctypes.c_void_p), ('workspace_bytes', ctypes.c_int64),
    ]


class _RenderCameraGrads(ctypes.Structure):
    """ide3d_render_camera_grads (include/ide3d_hip.h): the camera gradient of ide3d_render_rays_backward_camera."""
    _fields_ = [('grad_cam2world', ctypes.c_void_p), ('workspace', ctypes.c_void_p), ('workspace_bytes', ctypes.c_int64)]


class _Lattice(ctypes.Structure):
    _fields_ = [('n', ctypes.c_int32), ('voxel_size', ctypes.c_float), ('corner', ctypes.c_float * 3), ('scale', ctypes.c_float)]


class _RenderParams(ctypes.Structure):
    _fields_ = [
        ('rays_d_cam', ctypes.c_void_p), ('z_lin', ctypes.c_void_p), ('cam2world', ctypes.c_void_p),
        ('jitter', ctypes.c_void_p), ('sigma_noise', ctypes.c_void_p),
        ('tex_planes', ctypes.c_void_p), ('geo_planes', ctypes.c_void_p),
        ('tex_stride', ctypes.c_int64 * 4), ('geo_stride', ctypes.c_int64 * 4),
        ('geo_w0', ctypes.c_void_p), ('geo_b0', ctypes.c_void_p), ('geo_w1', ctypes.c_void_p), ('geo_b1', ctypes.c_void_p),
        ('tex_w0', ctypes.c_void_p), ('tex_b0', ctypes.c_void_p), ('tex_w1', ctypes.c_void_p), ('tex_b1', ctypes.c_void_p),
        ('n', ctypes.c_int32), ('rays_per_img', ctypes.c_int32), ('steps', ctypes.c_int32),
        ('C', ctypes.c_int32), ('H', ctypes.c_int32), ('W', ctypes.c_int32),
        ('hidden', ctypes.c_int32), ('feat_ch', ctypes.c_int32), ('seg_ch', ctypes.c_int32),
        ('clamp_mode', ctypes.c_int32), ('last_back', ctypes.c_int32), ('white_back', ctypes.c_int32),
        ('max_depth', ctypes.c_float),
        ('out_feat', ctypes.c_void_p), ('out_depth', ctypes.c_void_p), ('out_wsum', ctypes.c_void_p),
    ]


class _ModconvParams(ctypes.Structure):
    _fields_ = [
        ('x', ctypes.c_void_p), ('w', ctypes.c_void_p), ('styles', ctypes.c_void_p), ('dcoefs', ctypes.c_void_p),
        ('noise', ctypes.c_void_p), ('bias', ctypes.c_void_p), ('y', ctypes.c_void_p),
        ('n', ctypes.c_int32), ('cin', ctypes.c_int32), ('cout', ctypes.c_int32),
        ('h', ctypes.c_int32), ('w_', ctypes.c_int32), ('k', ctypes.c_int32),
        ('noise_strength', ctypes.c_float),
        ('act', ctypes.c_int32), ('alpha', ctypes.c_float), ('gain', ctypes.c_float), ('clamp', ctypes.c_float),
        ('mode', ctypes.c_int32), ('weights_packed', ctypes.c_int32),
        ('workspace', ctypes.c_void_p), ('workspace_bytes', ctypes.c_int64),
        ('w_batch_stride', ctypes.c_int64), ('arith', ctypes.c_int32),
        ('x_amax', ctypes.c_void_p), ('y_amax', ctypes.c_void_p), ('y_pitch', ctypes.c_int32),
    ]


class _ActBwdParams(ctypes.Structure):
    """ide3d_act_bwd_params (include/ide3d_hip.h): K1 of the convolution backward (ide3d_modconv_act_backward)."""
    _fields_ = [
        ('dy', ctypes.c_void_p), ('y', ctypes.c_void_p), ('dz', ctypes.c_void_p),
        ('noise', ctypes.c_void_p), ('noise_strength', ctypes.c_float), ('bias', ctypes.c_void_p),
        ('dcoefs', ctypes.c_void_p), ('ddcoefs', ctypes.c_void_p),
        ('n', ctypes.c_int32), ('c', ctypes.c_int32), ('h', ctypes.c_int32), ('w', ctypes.c_int32), ('y_pitch', ctypes.c_int32),
        ('act', ctypes.c_int32), ('alpha', ctypes.c_float), ('gain', ctypes.c_float), ('clamp', ctypes.c_float),
        ('workspace', ctypes.c_void_p), ('workspace_bytes', ctypes.c_int64),
    ]


class _WgradParams(ctypes.Structure):
    """ide3d_wgrad_params (include/ide3d_hip.h): the direct weight gradient of a modulated 3x3 convolution (ide3d_modconv_weight_grad)."""
    _fields_ = [
        ('g', ctypes.c_void_p), ('x', ctypes.c_void_p), ('styles', ctypes.c_void_p), ('dcoefs', ctypes.c_void_p), ('dw', ctypes.c_void_p),
        ('n', ctypes.c_int32), ('cin', ctypes.c_int32), ('cout', ctypes.c_int32), ('h', ctypes.c_int32), ('w', ctypes.c_int32),
        ('mode', ctypes.c_int32), ('arith', ctypes.c_int32), ('workspace', ctypes.c_void_p), ('workspace_bytes', ctypes.c_int64),
    ]


class _ModconvHeadEpilogue(ctypes.Structure):
    """ide3d_modconv_head_epilogue (include/ide3d_hip.h): the dual heads fused behind a 3x3 layer (ide3d_modconv2d_heads)."""
    _fields_ = [
        ('w', ctypes.c_void_p), ('bias', ctypes.c_void_p), ('y', ctypes.c_void_p),
        ('rows', ctypes.c_int32), ('clamp', ctypes.c_float), ('no_activation_output', ctypes.c_int32),
        ('workspace', ctypes.c_void_p), ('workspace_bytes', ctypes.c_int64),
    ]


class _ModconvPlanInfo(ctypes.Structure):
    """ide3d_modconv_plan_info (include/ide3d_hip.h): what ide3d_modconv2d would launch."""
    _fields_ = [
        ('kind', ctypes.c_int32), ('tile_h', ctypes.c_int32), ('tile_w', ctypes.c_int32), ('images_per_tile', ctypes.c_int32),
        ('rows', ctypes.c_int32), ('waves', ctypes.c_int32), ('parts', ctypes.c_int32), ('f16', ctypes.c_int32),
        ('split_k', ctypes.c_int32), ('strip', ctypes.c_int32), ('transposed_all_class', ctypes.c_int32), ('reserved', ctypes.c_int32),
        ('workgroups', ctypes.c_int64),
    ]


class _CompositePlanInfo(ctypes.Structure):
    """ide3d_composite_plan_info (include/ide3d_hip.h): what ide3d_composite would launch."""
    _fields_ = [('form', ctypes.c_int32), ('workgroup', ctypes.c_int32), ('grid', ctypes.c_int64), ('lds_bytes', ctypes.c_int64)]


COMPOSITE_FORMS = ('fallback', 'lds8', 'lds20', 'lds40')     # IDE3D_COMPOSITE_*


class _UpfirdnPlanInfo(ctypes.Structure):
    """ide3d_upfirdn2d_plan_info (include/ide3d_hip.h): what ide3d_upfirdn2d / ide3d_upfirdn2d_ex would launch."""
    _fields_ = [('form', ctypes.c_int32),
                ('ux', ctypes.c_int32), ('uy', ctypes.c_int32), ('dx', ctypes.c_int32), ('dy', ctypes.c_int32),
                ('fw', ctypes.c_int32), ('fh', ctypes.c_int32), ('cx', ctypes.c_int32), ('cy', ctypes.c_int32),
                ('cell_u', ctypes.c_int32), ('staging', ctypes.c_int32), ('c_fastest', ctypes.c_int32),
                ('tiles_x', ctypes.c_int32), ('tiles_y', ctypes.c_int32), ('grid', ctypes.c_int64), ('lds_bytes', ctypes.c_int64)]


UPFIRDN_FORMS = ('generic', 'cell', 'tile', 'fir44', 'fir_up2')     # IDE3D_UPFIRDN_*

PLAN_KINDS = ('fp32', 'split', 'split_teams', 'head_split', 'head_resident', 'head_small')     # IDE3D_PLAN_*

STYLE_BATCH_MAX = 24        # IDE3D_STYLE_BATCH_MAX


class _StyleJob(ctypes.Structure):
    _fields_ = [
        ('w', ctypes.c_void_p), ('w_stride', ctypes.c_int64),
        ('affine_w', ctypes.c_void_p), ('affine_b', ctypes.c_void_p),
        ('wsq_t', ctypes.c_void_p),
        ('cin', ctypes.c_int32), ('cout', ctypes.c_int32),
        ('affine_gain', ctypes.c_float), ('bias_gain', ctypes.c_float),
        ('styles', ctypes.c_void_p), ('dcoefs', ctypes.c_void_p),
    ]


class _FoldJob(ctypes.Structure):
    _fields_ = [
        ('w', ctypes.c_void_p), ('w_stride', ctypes.c_int64),
        ('cin', ctypes.c_int32), ('affine_gain', ctypes.c_float),
        ('a0', ctypes.c_void_p), ('b0', ctypes.c_void_p), ('w0', ctypes.c_void_p), ('cout0', ctypes.c_int32), ('gain0', ctypes.c_float),
        ('a1', ctypes.c_void_p), ('b1', ctypes.c_void_p), ('w1', ctypes.c_void_p), ('cout1', ctypes.c_int32), ('gain1', ctypes.c_float),
        ('out', ctypes.c_void_p),
    ]


LOWRES_MAX_LAYERS, LOWRES_MAX_HEADS = 8, 4          # IDE3D_LOWRES_MAX_*


class _LowresLayer(ctypes.Structure):
    _fields_ = [('weight', ctypes.c_void_p), ('styles', ctypes.c_void_p), ('dcoefs', ctypes.c_void_p), ('noise', ctypes.c_void_p), ('bias', ctypes.c_void_p),
                ('act_gain', ctypes.c_float), ('clamp', ctypes.c_float), ('up', ctypes.c_int32), ('head', ctypes.c_int32),
                ('weights_packed', ctypes.c_int32), ('reserved', ctypes.c_int32)]


class _LowresHead(ctypes.Structure):
    _fields_ = [('w', ctypes.c_void_p), ('bias', ctypes.c_void_p), ('skip', ctypes.c_void_p), ('clamp', ctypes.c_float), ('O', ctypes.c_int32)]


class _LowresParams(ctypes.Structure):
    _fields_ = [('x0', ctypes.c_void_p), ('x0_batch_stride', ctypes.c_int64), ('fir', ctypes.c_void_p), ('x_out', ctypes.c_void_p),
                ('workspace', ctypes.c_void_p), ('workspace_bytes', ctypes.c_int64),
                ('n', ctypes.c_int32), ('C', ctypes.c_int32), ('res0', ctypes.c_int32), ('nlayers', ctypes.c_int32), ('nheads', ctypes.c_int32),
                ('arith', ctypes.c_int32), ('reserved0', ctypes.c_int32), ('reserved', ctypes.c_int32),
                ('layers', _LowresLayer * LOWRES_MAX_LAYERS), ('heads', _LowresHead * LOWRES_MAX_HEADS)]


class _MappingParams(ctypes.Structure):
    _fields_ = [
        ('z', ctypes.c_void_p), ('c', ctypes.c_void_p), ('embed_w', ctypes.c_void_p), ('embed_b', ctypes.c_void_p),
        ('fc_w', ctypes.c_void_p * 16), ('fc_b', ctypes.c_void_p * 16), ('fc_out', ctypes.c_int32 * 16),
        ('w_avg', ctypes.c_void_p), ('ws', ctypes.c_void_p),
        ('workspace', ctypes.c_void_p), ('workspace_bytes', ctypes.c_int64),
        ('n', ctypes.c_int32), ('z_dim', ctypes.c_int32), ('c_dim', ctypes.c_int32), ('embed', ctypes.c_int32),
        ('layers', ctypes.c_int32), ('num_ws', ctypes.c_int32),
        ('embed_weight_gain', ctypes.c_float), ('embed_bias_gain', ctypes.c_float), ('lr_multiplier', ctypes.c_float),
        ('alpha', ctypes.c_float), ('act_gain', ctypes.c_float), ('truncation_psi', ctypes.c_float),
        ('truncation_cutoff', ctypes.c_int32),
    ]


LPIPS_MAX_TAPS = 8          # IDE3D_LPIPS_MAX_TAPS


class _LpipsTap(ctypes.Structure):
    """Mirror of ide3d_lpips_tap."""
    _fields_ = [
        ('a', ctypes.c_void_p), ('t', ctypes.c_void_p), ('lin', ctypes.c_void_p), ('out', ctypes.c_void_p),
        ('c', ctypes.c_int32), ('h', ctypes.c_int32), ('w', ctypes.c_int32), ('reserved', ctypes.c_int32),
    ]


class _FeatL1Tap(ctypes.Structure):
    """Mirror of ide3d_feat_l1_tap."""
    _fields_ = [
        ('a', ctypes.c_void_p), ('t', ctypes.c_void_p), ('weight', ctypes.c_float),
        ('c', ctypes.c_int32), ('h', ctypes.c_int32), ('w', ctypes.c_int32),
    ]


PARSE_JOIN_TERMS = 3          # IDE3D_PARSE_JOIN_TERMS


class _ParseTerm(ctypes.Structure):
    """Mirror of ide3d_parse_term."""
    _fields_ = [
        ('p', ctypes.c_void_p), ('batch_stride', ctypes.c_int64), ('plane_stride', ctypes.c_int64), ('row_pitch', ctypes.c_int32),
        ('half', ctypes.c_int32),
    ]


class _ParseJoinParams(ctypes.Structure):
    """Mirror of ide3d_parse_join_params."""
    _fields_ = [
        ('term', _ParseTerm * PARSE_JOIN_TERMS), ('scale', ctypes.c_void_p), ('bias', ctypes.c_void_p), ('y', ctypes.c_void_p),
        ('out', ctypes.c_void_p), ('n', ctypes.c_int32), ('c', ctypes.c_int32), ('h', ctypes.c_int32), ('w', ctypes.c_int32),
        ('post', ctypes.c_int32), ('bias_gain', ctypes.c_float),
    ]


def _hip_runtimes_mapped():
    """Paths of every libamdhip64 mapped into this process (there must be exactly one)."""
    paths = set()
    try:
        with open('/proc/self/maps') as f:
            for line in f:
                if 'libamdhip64' in line:
                    paths.add(line.split()[-1])
    except OSError:
        pass
    return paths


def load():
    """dlopen libide3d_hip.so once and declare the prototypes.  Raises RuntimeError if unusable."""
    global _lib
    if _lib is not None:
        return _lib
    with _lock:
        if _lib is not None:
            return _lib
        path = lib_path()
        if not os.path.isfile(path):
            raise RuntimeError(
                f'libide3d_hip.so not found at {path}. Build it with `python -c "import __graft_entry__ as g; g.build()"` '
                f'or `make -C ide-3d_amd/csrc`, or point ${_LIB_ENV} at it. There is no CPU/eager fallback for CUDA tensors.')
        # torch ships its own libamdhip64.so (soname libamdhip64.so.7); make sure it is the one already mapped
        # so that our kernels share torch's HIP runtime, streams and allocations.
        torch.cuda.is_available()
        try:
            lib = ctypes.CDLL(path, mode=ctypes.RTLD_LOCAL)
        except OSError as e:
            raise RuntimeError(f'failed to load {path}: {e}') from e
        rts = _hip_runtimes_mapped()
        if len(rts) > 1:
            raise RuntimeError(f'two HIP runtimes mapped in one process ({sorted(rts)}); import torch before loading the plugin')
        vp, i32, i64, f32 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_float
        lib.ide3d_last_error.restype = ctypes.c_char_p
        lib.ide3d_last_error.argtypes = []
        lib.ide3d_abi_version.restype = ctypes.c_int
        lib.ide3d_build_arch.restype = ctypes.c_char_p
        if lib.ide3d_abi_version() != _ABI_VERSION:
            raise RuntimeError(f'{path}: ABI version {lib.ide3d_abi_version()} != expected {_ABI_VERSION}; rebuild')
        # a library built with timing-only experiment knobs (wrong results by design) or without exclusive residency must never be
        # mistaken for the product: it loads only when the experimenter says so
        lib.ide3d_build_flags.restype = ctypes.c_char_p
        lib.ide3d_build_flags.argtypes = []
        flags = lib.ide3d_build_flags().decode('ascii', 'replace').split()
        unsafe = [f for f in flags if f.startswith('!')]
        if unsafe and os.environ.get('IDE3D_ALLOW_EXPERIMENT_BUILD') != '1':
            raise RuntimeError(f'{path} was built with experiment knobs that change results or drop a safety property ({" ".join(unsafe)}); '
                               'rebuild without EXTRA=..., or set IDE3D_ALLOW_EXPERIMENT_BUILD=1 for timing experiments')
        protos = {
            'ide3d_bias_act': [vp, vp, vp, vp, vp, vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, f32, f32, f32, i64, i64, i64, vp],
            'ide3d_upfirdn2d': [ctypes.POINTER(_UpfirdnParams), vp],
            'ide3d_upfirdn2d_ex': [ctypes.POINTER(_UpfirdnParams), ctypes.POINTER(_UpfirdnEpilogue), vp],
            'ide3d_upfirdn2d_plan': [ctypes.POINTER(_UpfirdnParams), ctypes.POINTER(_UpfirdnEpilogue), ctypes.POINTER(_UpfirdnPlanInfo)],
            'ide3d_filtered_lrelu': [ctypes.POINTER(_FlreluParams), vp],
            'ide3d_filtered_lrelu_act': [vp, vp, ctypes.c_int, i32, i32, i32, i32, ctypes.POINTER(i64 * 4),
                                         i32, i32, i32, i32, f32, f32, f32, ctypes.c_int, vp],
            'ide3d_triplane_sample': [vp, ctypes.POINTER(i64 * 4), i32, i32, i32, i32, vp, i64, vp, vp],
            'ide3d_triplane_sample_rays': [vp, ctypes.POINTER(i64 * 4), i32, i32, i32, i32, vp, i64, vp, i32, i32, i32, vp],
            'ide3d_triplane_taps': [i32, i32, vp, i64, vp, vp],
            'ide3d_triplane_tile_masks': [i32, i32, vp, i32, i32, i32, i32, vp, vp],
            'ide3d_triplane_sample_backward': [vp, vp, ctypes.POINTER(i64 * 4), i32, i32, i32, i32, vp, i64,
                                               vp, ctypes.POINTER(i64 * 4), vp, vp],
            'ide3d_composite': [vp, vp, vp, vp, i64, i32, i32, ctypes.c_int, ctypes.c_int, ctypes.c_int, f32,
                                ctypes.c_int, vp, vp, vp, vp],
            'ide3d_composite_plan': [vp, i64, i32, i32, ctypes.POINTER(_CompositePlanInfo)],
            'ide3d_sample_pdf': [vp, vp, vp, i64, i64, i32, i32, f32, vp, vp],
            'ide3d_render_rays': [ctypes.POINTER(_RenderParams), vp],
            'ide3d_render_ray_weights': [ctypes.POINTER(_RenderParams), vp, vp, vp, vp, vp],
            'ide3d_merge_depths': [vp, vp, i64, i32, i32, vp, vp, vp],
            'ide3d_render_rays_merged': [ctypes.POINTER(_RenderParams), vp, vp, vp, i32, vp],
            'ide3d_render_rays_backward': [ctypes.POINTER(_RenderParams), ctypes.POINTER(_RenderGrads), vp],
            'ide3d_render_param_grad_workspace_bytes': [ctypes.POINTER(_RenderParams)],
            'ide3d_render_rays_backward_params': [ctypes.POINTER(_RenderParams), ctypes.POINTER(_RenderGrads), ctypes.POINTER(_RenderParamGrads), vp],
            'ide3d_render_camera_grad_workspace_bytes': [ctypes.POINTER(_RenderParams)],
            'ide3d_render_rays_backward_camera': [ctypes.POINTER(_RenderParams), ctypes.POINTER(_RenderGrads), ctypes.POINTER(_RenderParamGrads),
                                                  ctypes.POINTER(_RenderCameraGrads), vp],
            'ide3d_render_merged_param_grad_workspace_bytes': [ctypes.POINTER(_RenderParams)],
            'ide3d_render_rays_merged_backward': [ctypes.POINTER(_RenderParams), vp, vp, vp, i32, ctypes.POINTER(_RenderGrads),
                                                  ctypes.POINTER(_RenderParamGrads), vp],
            'ide3d_sample_voxel': [ctypes.POINTER(_RenderParams), vp, i64, vp, vp, ctypes.c_int, vp],
            'ide3d_lattice_points': [ctypes.POINTER(_Lattice), i64, i64, vp, vp],
            'ide3d_density_lattice': [ctypes.POINTER(_RenderParams), ctypes.POINTER(_Lattice), i64, i64, vp, vp],
            'ide3d_mesh_workspace_bytes': [i32, i32, i32],
            'ide3d_mesh_count': [vp, i32, i32, i32, f32, vp, vp, i64, vp],
            'ide3d_mesh_emit': [vp, i32, i32, i32, f32, vp, ctypes.POINTER(_Lattice), i32, vp, i64, i64, i64, vp, vp, vp, vp],
            'ide3d_raster_workspace_bytes': [i32, i64, i32, i32],
            'ide3d_raster_project': [vp, i64, vp, i32, i32, i32, f32, f32, f32, f32, f32, f32, f32, vp, i64, vp],
            'ide3d_raster_depth': [vp, i64, i64, i32, i32, i32, i32, i32, vp, i64, vp],
            'ide3d_raster_shade': [vp, vp, i64, i32, i32, i32, vp, vp, vp, vp, i32, f32, f32, ctypes.POINTER(ctypes.c_float * 3), f32, vp, i64, vp, vp, vp, vp, vp],
            'ide3d_png_workspace_bytes': [i32, i32, i32, i32, i32],
            'ide3d_png_out_bytes': [i32, i32, i32, i32, i32],
            'ide3d_png_encode': [vp, i32, i32, i32, i32, i32, i32, vp, i64, vp, i64, vp, vp],
            'ide3d_jpeg_workspace_bytes': [i32, i32, i32, i32, i32, i32],
            'ide3d_jpeg_out_bytes': [i32, i32, i32, i32, i32, i32],
            'ide3d_jpeg_encode': [vp, i32, i32, i32, i32, i32, i32, i32, vp, i64, vp, i64, vp, vp],
            'ide3d_metrics_workspace_bytes': [i32, i64, i64, i32, i32],
            'ide3d_feature_moments': [vp, i64, i32, i64, vp, vp, vp],
            'ide3d_poly_kernel_sums': [vp, i64, i64, vp, i64, i64, i32, vp, vp, i32, i32, vp, i64, vp, vp],
            'ide3d_knn_radii': [vp, i64, i32, i64, i32, vp, i64, vp, vp],
            'ide3d_manifold_inside': [vp, i64, i64, vp, i64, i64, i32, vp, vp, i64, vp, vp],
            'ide3d_ppl_prep': [vp, vp, vp, vp, i32, i32, i32, i32, i32, i32, i32, i32, f32, f32, vp],
            'ide3d_lpips_pair_workspace_bytes': [ctypes.POINTER(_LpipsTap), i32, i32],
            'ide3d_lpips_pair_distances': [ctypes.POINTER(_LpipsTap), i32, i32, f32, vp, i64, vp, vp],
            'ide3d_trimmed_mean': [vp, i64, i64, i64, vp, vp],
            'ide3d_inception_score_workspace_bytes': [i64, i32, i32],
            'ide3d_inception_score': [vp, i64, i32, i64, i32, vp, i64, vp, vp],
            'ide3d_label_iou': [vp, vp, i32, i32, i64, vp, i32, i32, vp, vp, vp],
            'ide3d_augment_geometric': [vp, vp, i32, i32, i32, i32, i64, i64, vp, vp, vp, vp, vp, vp],
            'ide3d_augment_geometric_backward': [vp, vp, i32, i32, i32, i32, i64, i64, vp, vp, vp, vp, vp],
            'ide3d_augment_color': [vp, vp, i32, i32, i64, i64, i64, vp, i32, vp],
            'ide3d_modconv2d': [ctypes.POINTER(_ModconvParams), vp],
            'ide3d_modconv2d_heads': [ctypes.POINTER(_ModconvParams), ctypes.POINTER(_ModconvHeadEpilogue), vp],
            'ide3d_modconv2d_heads_gated': [ctypes.POINTER(_ModconvParams), ctypes.POINTER(_ModconvHeadEpilogue), ctypes.POINTER(_PlaneGate), vp],
            'ide3d_plane_cells': [vp, vp, vp, i32, i32, i32, i32, i32, vp, vp],
            'ide3d_plane_tile_list': [ctypes.POINTER(_PlaneGate), i32, i32, i32, i32, i32, vp, vp],
            'ide3d_skip_upsample_add_cl_gated': [vp, ctypes.POINTER(i64 * 4), vp, ctypes.POINTER(i64 * 4), i32, i32, i32, i32, vp, ctypes.POINTER(_PlaneGate), vp],
            'ide3d_modconv_plan': [ctypes.POINTER(_ModconvParams), ctypes.POINTER(_ModconvPlanInfo)],
            'ide3d_modconv_workspace_bytes': [i32, i32, i32, i32, i32, i32, i32, i32],
            'ide3d_act_bwd_workspace_bytes': [i32, i32, i32, i32],
            'ide3d_modconv_act_backward': [ctypes.POINTER(_ActBwdParams), vp],
            'ide3d_modconv_scale_dot': [vp, vp, vp, vp, vp, i32, i32, i32, i32, vp, i64, vp],
            'ide3d_head_wgrad_workspace_bytes': [i32, i32, i32, i32, i32],
            'ide3d_head_weight_grad': [vp, vp, vp, i32, i32, i32, i32, i32, vp, i64, vp],
            'ide3d_wgrad_workspace_bytes': [i32, i32, i32, i32, i32],
            'ide3d_modconv_weight_grad': [ctypes.POINTER(_WgradParams), vp],
            'ide3d_bias_noise_workspace_bytes': [i32, i32, i32, i32],
            'ide3d_bias_noise_grad': [vp, vp, vp, i32, i32, i32, i32, vp, i64, vp],
            'ide3d_noise_reg_workspace_bytes': [ctypes.POINTER(i32), i32],
            'ide3d_noise_reg_levels': [ctypes.POINTER(i32), i32],
            'ide3d_noise_reg': [vp, ctypes.POINTER(i32), i32, vp, i64, vp, vp, vp],
            'ide3d_noise_reg_backward': [vp, ctypes.POINTER(i32), i32, vp, i64, vp, vp, vp, vp],
            'ide3d_noise_normalize_workspace_bytes': [ctypes.POINTER(i32), i32],
            'ide3d_noise_normalize': [vp, ctypes.POINTER(i32), i32, vp, i64, vp],
            'ide3d_lpips_prep': [vp, vp, vp, vp, i32, i32, i32, i32, f32, f32, vp],
            'ide3d_lpips_prep_backward': [vp, vp, vp, i32, i32, i32, i32, f32, vp],
            'ide3d_maxpool2': [vp, vp, i64, i32, i32, vp],
            'ide3d_lpips_stage_backward': [vp, vp, vp, vp, i64, i32, i32, vp],
            'ide3d_lpips_head_workspace_bytes': [ctypes.POINTER(_LpipsTap), i32, i32],
            'ide3d_lpips_head': [ctypes.POINTER(_LpipsTap), i32, i32, vp, i64, vp, vp],
            'ide3d_lpips_head_backward': [ctypes.POINTER(_LpipsTap), i32, i32, vp, vp],
            'ide3d_unfold2d': [vp, vp, i32, i32, i32, i32, i32, i32, i32, vp],
            'ide3d_fold2d': [vp, vp, i32, i32, i32, i32, i32, i32, i32, vp],
            'ide3d_maxpool3s2p0': [vp, vp, vp, i64, i32, i32, vp],
            'ide3d_lpips_tap_backward': [vp, vp, vp, vp, vp, i64, i32, i32, i32, vp],
            'ide3d_feat_l1_workspace_bytes': [ctypes.POINTER(_FeatL1Tap), i32, i32],
            'ide3d_feat_l1': [ctypes.POINTER(_FeatL1Tap), i32, i32, vp, i64, vp, vp],
            'ide3d_feat_l1_tap_backward': [vp, vp, vp, vp, vp, f32, i64, i32, i32, i64, vp],
            'ide3d_maxpool2_relu_backward': [vp, vp, vp, i64, i32, i32, vp],
            'ide3d_resize_bilinear': [vp, vp, i64, i32, i32, i32, i32, vp],
            'ide3d_resize_bilinear_backward': [vp, vp, i64, i32, i32, i32, i32, vp],
            'ide3d_parse_ce_workspace_bytes': [i32, i32, i32, i32, i32, i32],
            'ide3d_parse_ce': [vp, vp, i32, i32, i32, i32, i32, i32, vp, vp, i64, vp, vp],
            'ide3d_parse_ce_backward': [vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, i32, vp],
            'ide3d_maxpool3s2': [vp, vp, vp, i64, i32, i32, vp],
            'ide3d_maxpool3s2_backward': [vp, vp, vp, vp, i64, i32, i32, vp],
            'ide3d_parse_join': [ctypes.POINTER(_ParseJoinParams), vp],
            'ide3d_plane_sums': [vp, vp, vp, i64, i64, f32, vp],
            'ide3d_parse_stem_backward': [vp, vp, vp, i32, i32, i32, i32, vp],
            'ide3d_id_prep': [vp, vp, i32, i32, vp],
            'ide3d_id_prep_backward': [vp, vp, i32, i32, vp],
            'ide3d_prelu': [vp, vp, vp, i32, i32, i32, i32, vp],
            'ide3d_prelu_backward': [vp, i64, i64, i32, vp, vp, vp, i32, i32, i32, i32, vp],
            'ide3d_se_gate': [vp, vp, vp, vp, i32, i32, i32, vp],
            'ide3d_se_gate_backward': [vp, vp, vp, vp, vp, vp, i32, i32, i32, vp],
            'ide3d_linear_workspace_bytes': [i32, i32, i32],
            'ide3d_linear_backward_input_workspace_bytes': [i32, i32, i32],
            'ide3d_linear': [vp, vp, vp, vp, i32, i32, i32, vp, i64, vp],
            'ide3d_linear_backward_input': [vp, vp, vp, i32, i32, i32, vp, i64, vp],
            'ide3d_linear_weight_grad': [vp, vp, vp, i32, i32, i32, vp],
            'ide3d_residual_join': [vp, vp, vp, i64, f32, vp],
            'ide3d_id_head': [vp, vp, vp, vp, vp, i32, i32, vp],
            'ide3d_id_head_backward': [vp, vp, vp, vp, vp, i32, i32, vp],
            'ide3d_clip_prep': [vp, vp, vp, vp, i32, i32, i32, vp],
            'ide3d_clip_prep_backward': [vp, vp, vp, i32, i32, i32, vp],
            'ide3d_vit_embed': [vp, vp, vp, vp, vp, vp, vp, i32, i32, i32, f32, vp],
            'ide3d_vit_embed_backward': [vp, vp, vp, vp, vp, vp, vp, i32, i32, i32, vp],
            'ide3d_layernorm': [vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, f32, vp],
            'ide3d_layernorm_backward': [vp, vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, vp],
            'ide3d_vit_attention': [vp, vp, i32, i32, i32, i32, f32, vp],
            'ide3d_vit_attention_backward': [vp, vp, vp, i32, i32, i32, i32, f32, vp],
            'ide3d_quickgelu': [vp, vp, i64, vp],
            'ide3d_quickgelu_backward': [vp, vp, vp, i64, vp],
            'ide3d_clip_head': [vp, vp, vp, vp, vp, vp, vp, vp, vp, i32, i32, i32, vp],
            'ide3d_clip_head_backward': [vp, vp, vp, vp, vp, vp, i32, i32, i32, vp],
            'ide3d_minibatch_std': [vp, vp, i32, i32, i32, i32, i32, i32, vp],
            'ide3d_minibatch_std_backward': [vp, vp, vp, i32, i32, i32, i32, i32, i32, vp],
            'ide3d_adv_head': [vp, vp, vp, vp, i32, i32, i32, vp],
            'ide3d_adv_head_backward': [vp, vp, vp, vp, vp, i32, i32, i32, vp],
            'ide3d_set_conv_arithmetic': [i32],
            'ide3d_get_conv_arithmetic': [],
            'ide3d_frame_u8': [vp, vp, vp, i32, i32, i32, i32, vp, vp],
            'ide3d_sphere_points': [vp, vp, i32, ctypes.c_float, i32, vp, vp, vp],
            'ide3d_cam2world': [vp, vp, vp, i32, i32, vp, vp],
            'ide3d_style_demod': [vp, i64, vp, vp, vp, i32, i32, i32, i32, f32, f32, vp, vp, vp],
            'ide3d_fold_heads': [vp, i64, i32, i32, i32, f32, vp, vp, vp, i32, f32, vp, vp, vp, i32, f32, vp, vp],
            'ide3d_style_demod_batch': [ctypes.POINTER(_StyleJob), i32, i32, i32, vp],
            'ide3d_fold_heads_batch': [ctypes.POINTER(_FoldJob), i32, i32, i32, vp],
            'ide3d_mapping': [ctypes.POINTER(_MappingParams), vp],
            'ide3d_mapping_workspace_bytes': [],
            'ide3d_mapping_supported': [],
            'ide3d_skip_upsample_add_cl': [vp, ctypes.POINTER(i64 * 4), vp, ctypes.POINTER(i64 * 4), i32, i32, i32, i32, vp, vp],
            'ide3d_bilinear_up2_split': [vp, i32, i32, i32, i32, ctypes.POINTER(vp * 3), ctypes.POINTER(i32 * 3), ctypes.POINTER(i32 * 3), ctypes.POINTER(ctypes.c_int64 * 3), vp],
            'ide3d_lowres_layers_supported': [i32, i32, i32, ctypes.POINTER(i32), i32, i32],
            'ide3d_lowres_workspace_bytes': [ctypes.POINTER(_LowresParams)],
            'ide3d_lowres_group': [ctypes.POINTER(_LowresParams), vp],
        }
        for name, argtypes in protos.items():
            fn = getattr(lib, name)          # AttributeError here = header / library mismatch
            fn.restype = ctypes.c_int64 if name.endswith('_bytes') else ctypes.c_int
            fn.argtypes = argtypes
        _lib = lib
        return _lib


EXPORTED_SYMBOLS = (
    'ide3d_last_error', 'ide3d_abi_version', 'ide3d_build_arch', 'ide3d_build_flags', 'ide3d_exclusive_violations', 'ide3d_exclusive_violation_text', 'ide3d_bias_act', 'ide3d_upfirdn2d', 'ide3d_upfirdn2d_ex', 'ide3d_upfirdn2d_plan',
    'ide3d_filtered_lrelu', 'ide3d_filtered_lrelu_act', 'ide3d_triplane_sample', 'ide3d_triplane_sample_rays', 'ide3d_triplane_taps', 'ide3d_triplane_tile_masks',
    'ide3d_triplane_sample_backward', 'ide3d_composite', 'ide3d_composite_plan', 'ide3d_sample_pdf', 'ide3d_render_rays', 'ide3d_render_rays_backward', 'ide3d_sample_voxel',
    'ide3d_lattice_points', 'ide3d_density_lattice',
    'ide3d_modconv2d', 'ide3d_modconv2d_heads', 'ide3d_modconv_workspace_bytes', 'ide3d_modconv_plan', 'ide3d_set_conv_arithmetic', 'ide3d_get_conv_arithmetic', 'ide3d_frame_u8', 'ide3d_sphere_points', 'ide3d_cam2world', 'ide3d_style_demod', 'ide3d_fold_heads',
    'ide3d_style_demod_batch', 'ide3d_fold_heads_batch',
    'ide3d_skip_upsample_add_cl', 'ide3d_bilinear_up2_split', 'ide3d_mapping', 'ide3d_mapping_workspace_bytes', 'ide3d_mapping_supported',
    'ide3d_lowres_layers_supported', 'ide3d_lowres_phase_r_plan', 'ide3d_lowres_workspace_bytes', 'ide3d_lowres_group',
    'ide3d_act_bwd_workspace_bytes', 'ide3d_modconv_act_backward', 'ide3d_modconv_scale_dot', 'ide3d_head_wgrad_workspace_bytes',
    'ide3d_head_weight_grad', 'ide3d_wgrad_workspace_bytes', 'ide3d_modconv_weight_grad', 'ide3d_bias_noise_workspace_bytes',
    'ide3d_bias_noise_grad', 'ide3d_render_param_grad_workspace_bytes', 'ide3d_render_rays_backward_params',
    'ide3d_noise_reg_workspace_bytes', 'ide3d_noise_reg_levels', 'ide3d_noise_reg', 'ide3d_noise_reg_backward',
    'ide3d_noise_normalize_workspace_bytes', 'ide3d_noise_normalize',
    'ide3d_render_camera_grad_workspace_bytes', 'ide3d_render_rays_backward_camera',
    'ide3d_lpips_prep', 'ide3d_lpips_prep_backward', 'ide3d_maxpool2', 'ide3d_lpips_stage_backward', 'ide3d_lpips_head_workspace_bytes',
    'ide3d_lpips_head', 'ide3d_lpips_head_backward',
    'ide3d_unfold2d', 'ide3d_fold2d', 'ide3d_maxpool3s2p0', 'ide3d_lpips_tap_backward',
    'ide3d_feat_l1_workspace_bytes', 'ide3d_feat_l1', 'ide3d_feat_l1_tap_backward', 'ide3d_maxpool2_relu_backward',
    'ide3d_resize_bilinear', 'ide3d_resize_bilinear_backward', 'ide3d_parse_ce_workspace_bytes', 'ide3d_parse_ce', 'ide3d_parse_ce_backward',
    'ide3d_maxpool3s2', 'ide3d_maxpool3s2_backward', 'ide3d_parse_join', 'ide3d_plane_sums', 'ide3d_parse_stem_backward',
    'ide3d_id_prep', 'ide3d_id_prep_backward', 'ide3d_prelu', 'ide3d_prelu_backward', 'ide3d_se_gate', 'ide3d_se_gate_backward',
    'ide3d_linear_workspace_bytes', 'ide3d_linear_backward_input_workspace_bytes', 'ide3d_linear', 'ide3d_linear_backward_input',
    'ide3d_linear_weight_grad', 'ide3d_residual_join', 'ide3d_id_head', 'ide3d_id_head_backward',
    'ide3d_mesh_workspace_bytes', 'ide3d_mesh_count', 'ide3d_mesh_emit',
    'ide3d_render_ray_weights', 'ide3d_merge_depths', 'ide3d_render_rays_merged',
    'ide3d_render_merged_param_grad_workspace_bytes', 'ide3d_render_rays_merged_backward',
    'ide3d_raster_workspace_bytes', 'ide3d_raster_project', 'ide3d_raster_depth', 'ide3d_raster_shade',
    'ide3d_plane_cells', 'ide3d_plane_tile_list', 'ide3d_modconv2d_heads_gated', 'ide3d_skip_upsample_add_cl_gated',
    'ide3d_png_workspace_bytes', 'ide3d_png_out_bytes', 'ide3d_png_encode',
    'ide3d_jpeg_workspace_bytes', 'ide3d_jpeg_out_bytes', 'ide3d_jpeg_encode',
    'ide3d_metrics_workspace_bytes', 'ide3d_feature_moments', 'ide3d_poly_kernel_sums', 'ide3d_knn_radii', 'ide3d_manifold_inside',
    'ide3d_augment_geometric', 'ide3d_augment_geometric_backward', 'ide3d_augment_color',
    'ide3d_clip_prep', 'ide3d_clip_prep_backward', 'ide3d_vit_embed', 'ide3d_vit_embed_backward', 'ide3d_layernorm', 'ide3d_layernorm_backward',
    'ide3d_vit_attention', 'ide3d_vit_attention_backward', 'ide3d_quickgelu', 'ide3d_quickgelu_backward', 'ide3d_clip_head', 'ide3d_clip_head_backward',
    'ide3d_minibatch_std', 'ide3d_minibatch_std_backward', 'ide3d_adv_head', 'ide3d_adv_head_backward',
    'ide3d_ppl_prep', 'ide3d_lpips_pair_workspace_bytes', 'ide3d_lpips_pair_distances', 'ide3d_trimmed_mean',
    'ide3d_inception_score_workspace_bytes', 'ide3d_inception_score', 'ide3d_label_iou',
)


def exclusive_violations():
    """(count, text): kernels with an LDS-fed bf16 / fp16 matrix loop that would NOT be alone on their CU on this device (their launches are
    refused with a RuntimeError); (0, '') everywhere the library is supported.  See ide3d_exclusive_violations (include/ide3d_hip.h)."""
    lib = load()
    lib.ide3d_exclusive_violations.restype = ctypes.c_int
    lib.ide3d_exclusive_violation_text.restype = ctypes.c_char_p
    return int(lib.ide3d_exclusive_violations()), lib.ide3d_exclusive_violation_text().decode('utf-8', 'replace')


def _check(rc, what):
    if rc == 0:
        CALLS[what] = CALLS.get(what, 0) + 1
    if rc != 0:
        msg = load().ide3d_last_error().decode('utf-8', 'replace')
        raise RuntimeError(f'{what} failed (code {rc}): {msg}')


# Host cost per launch matters for the drop-in loop shape (batch 1, eager: ~75 launches of 10-40 us of GPU work each; bench.py
# `dropin_eager_b1`): the raw stream handle comes from torch's C entry point (no `Stream` object), and the device guard is a no-op when the
# tensor's device is already current (the common single-GPU case).
_raw_stream = getattr(torch._C, '_cuda_getCurrentRawStream', None)


def _stream_handle(device):
    if _raw_stream is not None:
        return _raw_stream(device.index if device.index is not None else torch.cuda.current_device())
    return torch.cuda.current_stream(device).cuda_stream


def _stream(t):
    return ctypes.c_void_p(_stream_handle(t.device))


# ---- streams of our own ----------------------------------------------------------------------------------------------------------
# `torch.cuda.Stream()` hands out one of 32 pooled handles per device, round-robin: the 33rd stream an application (or this library) asks
# for IS the first one again.  A hipGraph capture whose capture stream happens to be the style side stream, or a stream the caller renders
# on, is malformed (round 5: a host-side segfault in hipGraphLaunch at the 33rd capture of a process, scripts/micro/r5_graph_churn.py).
# The streams this library forks work to - the capture stream of training/graph_cache.py and triplane.GraphedRenderer, the style
# prefetch side stream - are therefore created from the HIP runtime directly, once per (device, purpose), and never collide with a pooled one.
_private_streams = {}


def _hip_runtime():
    paths = _hip_runtimes_mapped()
    if len(paths) != 1:
        raise RuntimeError(f'expected exactly one HIP runtime mapped in this process, found {sorted(paths)}')
    rt = ctypes.CDLL(next(iter(paths)))          # the path that is already mapped: the same instance torch uses
    rt.hipStreamCreateWithFlags.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_uint]
    rt.hipStreamCreateWithFlags.restype = ctypes.c_int
    return rt


def private_stream(device, purpose):
    """A `torch.cuda.ExternalStream` around a HIP stream created for (device, purpose) and kept for the life of the process."""
    device = torch.device(device)
    idx = device.index if device.index is not None else torch.cuda.current_device()
    key = (idx, purpose)
    st = _private_streams.get(key)
    if st is None:
        with _lock:
            st = _private_streams.get(key)
            if st is None:
                torch.cuda.init()
                h = ctypes.c_void_p()
                with torch.cuda.device(idx):
                    rc = _hip_runtime().hipStreamCreateWithFlags(ctypes.byref(h), 1)          # hipStreamNonBlocking, like torch's pooled streams
                if rc != 0 or not h.value:
                    raise RuntimeError(f'hipStreamCreateWithFlags failed ({rc})')
                st = _private_streams[key] = torch.cuda.ExternalStream(h.value, device=torch.device('cuda', idx))
    return st


capture_lock = threading.RLock()          # one hipGraph capture at a time per process (they share the capture stream of their device)


class _NoGuard:
    def __enter__(self):
        return self

    def __exit__(self, *exc):
        return False


_NO_GUARD = _NoGuard()


def _dev_guard(device):
    """`with _dev_guard(t.device):` does what `with torch.cuda.device(t.device):` does, minus the context switch when that device is current."""
    if device is None:
        return _NO_GUARD
    idx = device.index if isinstance(device, torch.device) else device
    if idx is None or idx == torch.cuda.current_device():
        return _NO_GUARD
    return torch.cuda.device(idx)


# ---- who owns a launch's scratch memory ------------------------------------------------------------------------------------------
# Split-K partials, packed weights and the mapping kernel's barrier counter live in workspaces that belong to ONE launch at a time.
# Eager callers are told apart by their stream (two streams never share a workspace).  A stream HANDLE is not an identity, though:
# PyTorch hands pooled handles out round-robin and a hipGraph is replayed on whatever stream is current, so a captured graph owns its
# workspaces through `workspace_scope(owner)` instead: everything launched inside the scope is keyed by the owner object (one
# `GraphedRenderer`), and the entries are dropped when the owner is garbage-collected.  Two graphs therefore never share scratch
# memory with each other or with eager callers; replays of ONE graph must be serialised (they share its static buffers anyway).
_scope = threading.local()
_scope_finalizers = {}


class _Workspaces:
    """The workspaces of one plugin: key (built by the caller, with `_ws_domain(device)` in it) -> [buffer, packed-weight stamp].  The stamp is
    one (weakref(weight), weight._version) per weight whose packed copy the buffer holds, written after a successful launch: a packed copy is
    valid only for the very tensor object (and version) it was made from — the key pins address, shape and device, but the allocator
    recycles a data_ptr for another weight of the same shape.  Per-image weights are never "packed": their stamp stays empty."""

    def __init__(self, limit=None):
        self.limit, self.table = limit, {}

    def entry(self, key, alloc):
        ent = self.table.get(key)
        if ent is None:
            if self.limit is not None and len(self.table) > self.limit:
                # only those with a packed weight whose tensor is gone (nothing can launch with them again): a captured hipGraph holds raw pointers into the live ones
                for dead in [k for k, e in self.table.items() if any(ref() is None for ref, _ in e[1])]:
                    del self.table[dead]
            ent = self.table[key] = [alloc(), ()]
        return ent

    def packed(self, ent, weights):
        """Per weight: does the entry hold the packed copy of this very tensor at its current version?  (A fresh entry: of none.)"""
        return [ref() is w and ver == w._version for (ref, ver), w in zip(ent[1], weights)] or [False] * len(weights)

    def mark_packed(self, ent, weights):
        ent[1] = [(weakref.ref(w), w._version) for w in weights]

    def drop(self, domain):
        for k in [k for k in self.table if domain in k]:
            del self.table[k]


def _drop_owner(domain):
    _scope_finalizers.pop(domain, None)
    for plugin in (ModconvPlugin, MappingPlugin, LowresPlugin, VolumeRenderPlugin, VggLossPlugin, MeshPlugin, RasterPlugin):
        plugin._ws.drop(domain)


class workspace_scope:
    """`with workspace_scope(owner): ...` — launches inside use workspaces owned by `owner` (any weak-referenceable object)."""

    def __init__(self, owner):
        self.domain = ('owner', id(owner))
        if self.domain not in _scope_finalizers:
            _scope_finalizers[self.domain] = weakref.finalize(owner, _drop_owner, self.domain)

    def __enter__(self):
        self.prev = getattr(_scope, 'domain', None)
        _scope.domain = self.domain
        return self

    def __exit__(self, *exc):
        _scope.domain = self.prev
        return False


def _ws_domain(device):
    """Key component that separates workspaces of concurrent launch sequences: the owner of the active scope, else the current stream."""
    dom = getattr(_scope, 'domain', None)
    return dom if dom is not None else ('stream', _stream_handle(device))


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if (t is not None and t.numel() > 0) else ctypes.c_void_p(0)


def _i64x4(vals):
    return (ctypes.c_int64 * 4)(*[int(v) for v in vals])


def _require(cond, msg):
    if not cond:
        raise RuntimeError(msg)


def _dense(t):
    return t.is_contiguous() or (t.ndim == 4 and t.is_contiguous(memory_format=torch.channels_last))


# ------------------------------------------------------------------------------------------------
# bias_act_plugin
# ------------------------------------------------------------------------------------------------

class BiasActPlugin:
    """`bias_act_plugin` of the reference (bias_act.cpp:32-97)."""

    @staticmethod
    def bias_act(x, b, xref, yref, dy, grad, dim, act, alpha, gain, clamp):
        _require(x.is_cuda, 'x must reside on CUDA device')
        for name, t in (('b', b), ('xref', xref), ('yref', yref), ('dy', dy)):
            if t.numel():
                _require(t.device == x.device, f'{name} must reside on the same device as x')
                _require(t.dtype == x.dtype, f'{name} must have the same dtype as x')
        _require(x.dtype in _DTYPE_CODE, 'x must be float16, bfloat16, float32 or float64')
        _require(b.numel() == 0 or (b.ndim == 1 and 0 <= dim < x.ndim and b.shape[0] == x.shape[dim]),
                 'b must be a vector matching dimension `dim` of x')
        _require(b.numel() == 0 or b.is_contiguous(), 'b must be contiguous')
        for name, t in (('xref', xref), ('yref', yref), ('dy', dy)):
            _require(t.numel() == 0 or (t.shape == x.shape and t.stride() == x.stride()),
                     f'{name} must have the same shape and layout as x')
        _require(grad >= 0, 'grad must be non-negative')
        _require(_dense(x) or x.numel() == 0 or x.is_non_overlapping_and_dense(), 'x must be non-overlapping and dense')
        y = torch.empty_like(x)
        _require(y.stride() == x.stride(), 'internal: output layout differs from input layout')
        if x.numel() == 0:
            return y
        step_b = x.stride(dim) if b.numel() else 1
        with _dev_guard(x.device):
            rc = load().ide3d_bias_act(_ptr(x), _ptr(b), _ptr(xref), _ptr(yref), _ptr(dy), _ptr(y),
                                       _DTYPE_CODE[x.dtype], int(grad), int(act), float(alpha), float(gain), float(clamp),
                                       x.numel(), max(b.numel(), 1), int(step_b), _stream(x))
        _check(rc, 'bias_act')
        return y


# ------------------------------------------------------------------------------------------------
# upfirdn2d_plugin
# ------------------------------------------------------------------------------------------------

def _upfirdn_params(x_shape, x_stride, dtype, x_ptr, row_floats, f_shape, f_stride, f_ptr, upx, upy, downx, downy, padx0, padx1, pady0, pady1, flip, gain):
    """The `_UpfirdnParams` of one call, all but the output's address and strides -> (params, output shape, channels_last output?).
    `Upfirdn2dPlugin.upfirdn2d_ex` and the host-only `upfirdn2d_plan` both build their parameters here."""
    _require(f_shape[0] >= 1 and f_shape[1] >= 1, 'f must be at least 1x1')
    _require(upx >= 1 and upy >= 1, 'upsampling factor must be at least 1')
    _require(downx >= 1 and downy >= 1, 'downsampling factor must be at least 1')
    n, c, ih, iw = x_shape
    ow = (iw * upx + padx0 + padx1 - f_shape[1] + downx) // downx
    oh = (ih * upy + pady0 + pady1 - f_shape[0] + downy) // downy
    _require(ow >= 1 and oh >= 1, 'output must be at least 1x1')
    cl = x_stride[1] == 1 and c > 1
    p = _UpfirdnParams()
    p.x, p.f = x_ptr, f_ptr
    p.dtype = _DTYPE_CODE[dtype]
    p.n, p.c, p.in_h, p.in_w, p.out_h, p.out_w = n, c, ih, iw, oh, ow
    p.x_stride = _i64x4(x_stride)
    p.f_h, p.f_w = f_shape
    p.f_stride = (ctypes.c_int64 * 2)(f_stride[0], f_stride[1])
    p.up_x, p.up_y, p.down_x, p.down_y = upx, upy, downx, downy
    p.pad_x0, p.pad_y0 = padx0, pady0
    p.flip, p.gain = int(bool(flip)), float(gain)
    p.x_row_floats = row_floats
    return p, (n, c, oh, ow), cl


class Upfirdn2dPlugin:
    """`upfirdn2d_plugin` of the reference (upfirdn2d.cpp:16-105)."""

    @staticmethod
    def upfirdn2d(x, f, upx, upy, downx, downy, padx0, padx1, pady0, pady1, flip, gain):
        return Upfirdn2dPlugin.upfirdn2d_ex(x, f, upx, upy, downx, downy, padx0, padx1, pady0, pady1, flip, gain)

    @staticmethod
    def upfirdn2d_ex(x, f, upx, upy, downx, downy, padx0, padx1, pady0, pady1, flip, gain,
                     add=None, noise=None, noise_strength=1.0, bias=None, act=None, alpha=0.0, act_gain=1.0, clamp=-1.0, y_amax=None):
        """upfirdn2d with the optional fused epilogue  y = bias_act(FIR(x) + add + noise * noise_strength)
        (`act` None = no bias/activation stage; 1 linear, 3 lrelu)."""
        _require(x.is_cuda, 'x must reside on CUDA device')
        _require(f.device == x.device, 'f must reside on the same device as x')
        _require(f.dtype == torch.float32, 'f must be float32')
        _require(x.dtype in _DTYPE_CODE, 'x must be float16, bfloat16, float32 or float64')
        _require(x.numel() > 0, 'x has zero size')
        _require(f.numel() > 0, 'f has zero size')
        _require(x.ndim == 4, 'x must be rank 4')
        _require(f.ndim == 2, 'f must be rank 2')
        p, (n, c, oh, ow), cl = _upfirdn_params(tuple(x.shape), x.stride(), x.dtype, x.data_ptr(), _row_floats_readable(x), tuple(f.shape), f.stride(), f.data_ptr(),
                                                upx, upy, downx, downy, padx0, padx1, pady0, pady1, flip, gain)
        y = torch.empty([n, c, oh, ow], dtype=x.dtype, device=x.device,
                        memory_format=torch.channels_last if cl else torch.contiguous_format)
        p.y, p.y_stride = y.data_ptr(), _i64x4(y.stride())
        plain = add is None and noise is None and act is None and y_amax is None
        with _dev_guard(x.device):
            if plain:
                rc = load().ide3d_upfirdn2d(ctypes.byref(p), _stream(x))
            else:
                ep = _UpfirdnEpilogue()
                keep = []
                if y_amax is not None:     # [n, AMAX_FLOATS] float32, zeroed by the caller: row max = max |y| per image (f16x3 scale of the consumer)
                    _require(y_amax.is_cuda and y_amax.device == x.device and y_amax.dtype == torch.float32 and tuple(y_amax.shape) == (n, AMAX_FLOATS)
                             and y_amax.is_contiguous() and x.dtype == torch.float32, 'y_amax must be a contiguous float32 [n, AMAX_FLOATS] tensor on the device of a float32 x')
                    ep.y_amax = y_amax.data_ptr()
                if add is not None:
                    _require(add.shape == y.shape and add.dtype == x.dtype and add.device == x.device, 'add must match the output')
                    ep.add, ep.add_stride = add.data_ptr(), _i64x4(add.stride())
                if noise is not None:
                    noise = noise.to(torch.float32).contiguous(); keep.append(noise)
                    _require(tuple(noise.shape[-2:]) == (oh, ow) and noise.numel() == oh * ow, 'noise must be [out_h, out_w]')
                    ep.noise, ep.noise_strength = noise.data_ptr(), float(noise_strength)
                if act is not None:
                    ep.fused_act, ep.act = 1, int(act)
                    ep.alpha, ep.act_gain, ep.clamp = float(alpha), float(act_gain), float(clamp)
                    if bias is not None:
                        bias = bias.to(x.dtype).contiguous(); keep.append(bias)
                        _require(bias.numel() == c, 'bias must have one entry per channel')
                        ep.bias = bias.data_ptr()
                rc = load().ide3d_upfirdn2d_ex(ctypes.byref(p), ctypes.byref(ep), _stream(x))
        _check(rc, 'upfirdn2d')
        return y


# ------------------------------------------------------------------------------------------------
# filtered_lrelu_plugin
# ------------------------------------------------------------------------------------------------

class FilteredLReluPlugin:
    """`filtered_lrelu_plugin` of the reference (filtered_lrelu.cpp:16-298)."""

    @staticmethod
    def filtered_lrelu(x, fu, fd, b, si, up, down, px0, px1, py0, py1, sx, sy, gain, slope, clamp, flip_filters, write_signs):
        _require(x.is_cuda, 'x must reside on CUDA device')
        _require(fu.device == x.device and fd.device == x.device and b.device == x.device,
                 'all input tensors must reside on the same device')
        _require(fu.dtype == torch.float32 and fd.dtype == torch.float32, 'fu and fd must be float32')
        _require(b.dtype == x.dtype, 'x and b must have the same dtype')
        _require(x.dtype in (torch.float16, torch.float32, torch.bfloat16), 'x and b must be float16, bfloat16 or float32')
        _require(x.ndim == 4, 'x must be rank 4')
        _require(x.numel() > 0, 'x is empty')
        _require(fu.ndim in (1, 2) and fd.ndim in (1, 2), 'fu and fd must be rank 1 or 2')
        _require(fu.numel() > 0, 'fu is empty')
        _require(fd.numel() > 0, 'fd is empty')
        _require(b.ndim == 1 and b.shape[0] == x.shape[1], 'b must be a vector with the same number of channels as x')
        _require(up >= 1 and down >= 1, 'up and down must be at least 1')
        n, c, xh, xw = x.shape
        fut_w, fut_h = fu.shape[-1] - 1, fu.shape[0] - 1
        fdt_w, fdt_h = fd.shape[-1] - 1, fd.shape[0] - 1
        cw = xw * up + (px0 + px1) - fut_w
        ch = xh * up + (py0 + py1) - fut_h
        _require(cw > fdt_w and ch > fdt_h, 'upsampled buffer must be at least the size of downsampling filter')
        yw = (cw - fdt_w + (down - 1)) // down
        yh = (ch - fdt_h + (down - 1)) // down
        _require(yw > 0 and yh > 0, 'output must be at least 1x1')
        read_signs = si.numel() > 0
        so = torch.empty([0], dtype=torch.uint8, device=x.device)
        s = si
        sw_active = 0
        if write_signs:
            sw_active = yw * down - (down - 1) + fdt_w
            sh = yh * down - (down - 1) + fdt_h
            sw = (sw_active + 15) & ~15
            s = so = torch.empty([n, c, sh, sw >> 2], dtype=torch.uint8, device=x.device)
        elif read_signs:
            sw_active = s.shape[3] << 2
        if read_signs or write_signs:
            _require(s.is_contiguous(), 'signs must be contiguous')
            _require(s.dtype == torch.uint8, 'signs must be uint8')
            _require(s.device == x.device, 'signs must reside on the same device as x')
            _require(s.ndim == 4, 'signs must be rank 4')
            _require(s.shape[0] == n and s.shape[1] == c, 'signs must have same batch & channels as x')
        cl = x.stride(1) == 1 and c > 1
        y = torch.empty([n, c, yh, yw], dtype=x.dtype, device=x.device,
                        memory_format=torch.channels_last if cl else torch.contiguous_format)
        p = _FlreluParams()
        p.x, p.y, p.b = x.data_ptr(), y.data_ptr(), b.contiguous().data_ptr()
        p.s = s.data_ptr() if (read_signs or write_signs) else 0
        p.fu, p.fd = fu.data_ptr(), fd.data_ptr()
        p.dtype = _DTYPE_CODE[x.dtype]
        p.n, p.c, p.in_h, p.in_w, p.out_h, p.out_w = n, c, xh, xw, yh, yw
        p.x_stride, p.y_stride = _i64x4(x.stride()), _i64x4(y.stride())
        p.fu_w, p.fu_h = fu.shape[-1], (fu.shape[0] if fu.ndim == 2 else 0)
        p.fd_w, p.fd_h = fd.shape[-1], (fd.shape[0] if fd.ndim == 2 else 0)
        p.fu_stride = (ctypes.c_int64 * 2)(fu.stride(0) if fu.ndim == 2 else 0, fu.stride(-1))
        p.fd_stride = (ctypes.c_int64 * 2)(fd.stride(0) if fd.ndim == 2 else 0, fd.stride(-1))
        p.up, p.down, p.pad_x0, p.pad_y0 = up, down, px0, py0
        p.s_w_bytes, p.s_h = (s.shape[3], s.shape[2]) if (read_signs or write_signs) else (0, 0)
        p.s_ofs_x, p.s_ofs_y = sx, sy
        p.sw_limit = (sw_active + 3) >> 2
        p.sign_mode = 1 if write_signs else (2 if read_signs else 0)
        p.flip = int(bool(flip_filters))
        p.gain, p.slope, p.clamp = float(gain), float(slope), float(min(clamp, 3.0e38))
        with _dev_guard(x.device):
            rc = load().ide3d_filtered_lrelu(ctypes.byref(p), _stream(x))
        if rc == -2:     # IDE3D_ENOKERNEL: same contract as the reference's return_code = -1
            return torch.empty([0], device=x.device), torch.empty([0], device=x.device), -1
        _check(rc, 'filtered_lrelu')
        return y, so, 0

    @staticmethod
    def filtered_lrelu_act_(x, si, sx, sy, gain, slope, clamp, write_signs):
        _require(x.is_cuda, 'x must reside on CUDA device')
        _require(x.ndim == 4, 'x must be rank 4')
        _require(x.numel() > 0, 'x is empty')
        _require(x.dtype in _DTYPE_CODE, 'x must be float16, bfloat16, float32 or float64')
        n, c, h, w = x.shape
        read_signs = si.numel() > 0
        so = torch.empty([0], dtype=torch.uint8, device=x.device)
        s = si
        if write_signs:
            sw = (w + 15) & ~15
            s = so = torch.empty([n, c, h, sw >> 2], dtype=torch.uint8, device=x.device)
        if read_signs or write_signs:
            _require(s.is_contiguous(), 'signs must be contiguous')
            _require(s.dtype == torch.uint8, 'signs must be uint8')
            _require(s.device == x.device, 'signs must reside on the same device as x')
            _require(s.ndim == 4, 'signs must be rank 4')
            _require(s.shape[0] == n and s.shape[1] == c, 'signs must have same batch & channels as x')
        s_w, s_h = ((s.shape[3] << 2), s.shape[2]) if (read_signs or write_signs) else (0, 0)
        with _dev_guard(x.device):
            rc = load().ide3d_filtered_lrelu_act(
                _ptr(x), _ptr(s) if (read_signs or write_signs) else ctypes.c_void_p(0), _DTYPE_CODE[x.dtype],
                n, c, h, w, ctypes.byref(_i64x4(x.stride())), s_w, s_h, sx, sy,
                float(gain), float(slope), float(min(clamp, 3.0e38)),
                1 if write_signs else (2 if read_signs else 0), _stream(x))
        _check(rc, 'filtered_lrelu_act_')
        return so


# ------------------------------------------------------------------------------------------------
# tri-plane gather / compositing / fused renderer / modulated conv / frame conversion
# ------------------------------------------------------------------------------------------------

class TriplanePlugin:
    @staticmethod
    def sample(planes, coords, ray_grid=None):
        """planes [n, 3C, H, W] float32 (any strides), coords [n, m, 3] float32 -> [n*m, C].

        ray_grid = (rays_h, rays_w, steps) tells the library that coords is [n, rays_h, rays_w, steps, 3] flattened (what
        the ray-marcher produces): a grouping hint for the LDS-staged kernel, results do not depend on it."""
        _require(planes.is_cuda and coords.device == planes.device, 'planes and coords must be on the same CUDA device')
        _require(planes.dtype == torch.float32 and coords.dtype == torch.float32, 'planes and coords must be float32')
        _require(planes.ndim == 4 and planes.shape[1] % 3 == 0, 'planes must be [n, 3*C, H, W]')
        _require(coords.ndim == 3 and coords.shape[2] == 3 and coords.shape[0] == planes.shape[0], 'coords must be [n, m, 3]')
        n, c3, H, W = planes.shape
        C = c3 // 3
        coords = coords.contiguous()
        m = coords.shape[1]
        out = torch.empty([n * m, C], dtype=torch.float32, device=planes.device)
        if m == 0:
            return out
        if ray_grid is not None:
            rh, rw, steps = (int(v) for v in ray_grid)
            _require(rh * rw * steps == m, 'ray_grid does not match the number of samples')
            with _dev_guard(planes.device):
                rc = load().ide3d_triplane_sample_rays(_ptr(planes), ctypes.byref(_i64x4(planes.stride())), n, C, H, W,
                                                       _ptr(coords), m, _ptr(out), rh, rw, steps, _stream(planes))
            _check(rc, 'triplane_sample_rays')
            return out
        with _dev_guard(planes.device):
            rc = load().ide3d_triplane_sample(_ptr(planes), ctypes.byref(_i64x4(planes.stride())), n, C, H, W,
                                              _ptr(coords), m, _ptr(out), _stream(planes))
        _check(rc, 'triplane_sample')
        return out

    @staticmethod
    def taps(H, W, coords):
        coords = coords.contiguous().reshape(-1, 3)
        _require(coords.is_cuda and coords.dtype == torch.float32, 'coords must be float32 on a CUDA device')
        taps = torch.empty([coords.shape[0], 3, 3], dtype=torch.int32, device=coords.device)
        if coords.shape[0]:
            with _dev_guard(coords.device):
                rc = load().ide3d_triplane_taps(H, W, _ptr(coords), coords.shape[0], _ptr(taps), _stream(coords))
            _check(rc, 'triplane_taps')
        return taps

    @staticmethod
    def tile_masks(H, W, coords, ray_grid):
        """coords [n, rays_h * rays_w * steps, 3] -> int32 [n, tiles, steps / 4]: the planes `sample(..., ray_grid=)` stages in LDS per
        chunk (bit p = plane p), from the gather kernel's own region-table code.  Parity hook for the tests."""
        rh, rw, steps = (int(v) for v in ray_grid)
        coords = coords.contiguous()
        _require(coords.is_cuda and coords.dtype == torch.float32, 'coords must be float32 on a CUDA device')
        _require(coords.ndim == 3 and coords.shape[2] == 3 and coords.shape[1] == rh * rw * steps, 'coords must be [n, rays_h * rays_w * steps, 3]')
        _require(rh > 0 and rw > 0 and steps > 0 and rh % 8 == 0 and rw % 8 == 0 and steps % 4 == 0, 'ray_grid must be made of 8 x 8-ray tiles and 4-step chunks')
        n = coords.shape[0]
        masks = torch.empty([n, (rh // 8) * (rw // 8), steps // 4], dtype=torch.int32, device=coords.device)
        if n:
            with _dev_guard(coords.device):
                rc = load().ide3d_triplane_tile_masks(H, W, _ptr(coords), n, rh, rw, steps, _ptr(masks), _stream(coords))
            _check(rc, 'triplane_tile_masks')
        return masks

    @staticmethod
    def sample_backward(grad_out, planes, coords, need_coord_grad):
        n, c3, H, W = planes.shape
        C = c3 // 3
        coords = coords.contiguous()
        grad_out = grad_out.contiguous()
        m = coords.shape[1]
        grad_planes = torch.zeros_like(planes)
        grad_coords = torch.zeros_like(coords) if need_coord_grad else None
        if m:
            with _dev_guard(planes.device):
                rc = load().ide3d_triplane_sample_backward(
                    _ptr(grad_out), _ptr(planes), ctypes.byref(_i64x4(planes.stride())), n, C, H, W,
                    _ptr(coords), m, _ptr(grad_planes), ctypes.byref(_i64x4(grad_planes.stride())),
                    _ptr(grad_coords), _stream(planes))
            _check(rc, 'triplane_sample_backward')
        return grad_planes, grad_coords


class VolumeRenderPlugin:
    _ws = _Workspaces()          # (kind, bytes, device index, launch domain) -> the per-wave partial sums of render_rays_backward_params / _camera
    MLP_KEYS = ('geo_w0', 'geo_b0', 'geo_w1', 'geo_b1', 'tex_w0', 'tex_b0', 'tex_w1', 'tex_b1')        # the decoder tensors of `mlp`, in the order of the C structs

    @staticmethod
    def composite(rgb_sigma, z_vals, dir_norm, noise, clamp_mode, last_back, white_back, max_depth, fill_mode,
                  want_weights=True):
        """rgb_sigma [rays, steps, ch+1], z_vals [rays, steps], dir_norm [rays], noise [rays, steps] | None."""
        _require(rgb_sigma.is_cuda and rgb_sigma.dtype == torch.float32, 'rgb_sigma must be float32 on a CUDA device')
        rays, steps, row = rgb_sigma.shape
        ch = row - 1
        rgb_sigma, z_vals, dir_norm = rgb_sigma.contiguous(), z_vals.contiguous(), dir_norm.contiguous()
        if noise is not None:
            noise = noise.contiguous()
        dev = rgb_sigma.device
        rgb = torch.empty([rays, ch], dtype=torch.float32, device=dev)
        depth = torch.empty([rays], dtype=torch.float32, device=dev)
        weights = torch.empty([rays, steps], dtype=torch.float32, device=dev) if want_weights else None
        with _dev_guard(dev):
            rc = load().ide3d_composite(_ptr(rgb_sigma), _ptr(z_vals), _ptr(dir_norm), _ptr(noise), rays, steps, ch,
                                        int(clamp_mode), int(bool(last_back)), int(bool(white_back)), float(max_depth or 0.0),
                                        int(fill_mode), _ptr(rgb), _ptr(depth), _ptr(weights), _stream(rgb_sigma))
        _check(rc, 'composite')
        return rgb, depth, weights

    @staticmethod
    def sample_pdf(bins, weights, u, eps=1e-5):
        """bins [rays, k+1], weights [rays, k], u [n_importance] (shared) or [rays, n_importance] -> [rays, n_importance]."""
        _require(weights.is_cuda and weights.dtype == torch.float32 and weights.ndim == 2, 'weights must be 2-D float32 on a CUDA device')
        rays, k = weights.shape
        _require(bins.shape == (rays, k + 1) and bins.dtype == torch.float32 and bins.device == weights.device,
                 'bins must be [rays, k + 1] float32 next to weights')
        _require(u.dtype == torch.float32 and u.device == weights.device and u.ndim in (1, 2) and (u.ndim == 1 or u.shape[0] == rays),
                 'u must be [n_importance] or [rays, n_importance] float32 next to weights')
        bins, weights, u = bins.contiguous(), weights.contiguous(), u.contiguous()
        n_imp = u.shape[-1]
        out = torch.empty([rays, n_imp], dtype=torch.float32, device=weights.device)
        with _dev_guard(weights.device):
            rc = load().ide3d_sample_pdf(_ptr(bins), _ptr(weights), _ptr(u), 0 if u.ndim == 1 else n_imp, rays, k, n_imp,
                                         float(eps), _ptr(out), _stream(weights))
        _check(rc, 'sample_pdf')
        return out

    @staticmethod
    def _fill_render_params(p, tex_planes, geo_planes, mlp):
        p.tex_planes, p.geo_planes = tex_planes.data_ptr(), geo_planes.data_ptr()
        p.tex_stride, p.geo_stride = _i64x4(tex_planes.stride()), _i64x4(geo_planes.stride())
        for k in VolumeRenderPlugin.MLP_KEYS:
            t = mlp[k]
            _require(t.is_cuda and t.dtype == torch.float32 and t.is_contiguous(), f'{k} must be contiguous float32 on GPU')
            setattr(p, k, t.data_ptr())
            _require(t.device == tex_planes.device, f'{k} must reside on the same device as the tri-planes')
        n, c3, H, W = tex_planes.shape
        _require(geo_planes.shape == tex_planes.shape, 'texture and geometry tri-planes must have the same shape')
        _require(geo_planes.device == tex_planes.device, 'texture and geometry tri-planes must reside on the same device')
        _require(c3 % 3 == 0, 'tri-planes must be [n, 3*C, H, W]')
        C = c3 // 3
        _require(mlp['geo_w0'].ndim == 2 and mlp['geo_w1'].ndim == 2 and mlp['tex_w0'].ndim == 2 and mlp['tex_w1'].ndim == 2,
                 'decoder weights must be [out, in] matrices')
        hidden = mlp['geo_w0'].shape[0]
        nout_geo, nout_tex = mlp['geo_w1'].shape[0], mlp['tex_w1'].shape[0]
        # the kernel indexes w0[row * C + col], b0[row], w1[row * hidden + col], b1[row] for the compiled (C, hidden): every
        # tensor must have exactly that shape, and both branches the same hidden width
        for k, shape in (('geo_w0', (hidden, C)), ('tex_w0', (hidden, C)), ('geo_b0', (hidden,)), ('tex_b0', (hidden,)),
                         ('geo_w1', (nout_geo, hidden)), ('tex_w1', (nout_tex, hidden)), ('geo_b1', (nout_geo,)), ('tex_b1', (nout_tex,))):
            _require(tuple(mlp[k].shape) == shape, f'{k} must be {list(shape)} (C={C}, hidden={hidden}), got {list(mlp[k].shape)}')
        _require(nout_geo >= 1, 'geo_w1 must have at least the sigma row')
        p.n, p.C, p.H, p.W = n, C, H, W
        p.hidden = hidden
        p.seg_ch = nout_geo - 1
        p.feat_ch = nout_tex

    @staticmethod
    def check_render_shapes(n, rays_per_img, steps, rays_d_cam, z_lin, cam2world, jitter=None, sigma_noise=None):
        """Host-only shape rules of `render_rays`, checked before anything is launched.  The kernel reads rays_d_cam[r * 3 + k],
        z_lin[s], cam2world[image * 16 + k] and jitter / sigma_noise[ray * steps + s] for every ray of all n images: a shorter
        buffer would be read past its end."""
        _require(rays_d_cam.numel() == rays_per_img * 3, f'render_rays: rays_d_cam must be [{rays_per_img}, 3], got {list(rays_d_cam.shape)}')
        _require(z_lin.numel() == steps, f'render_rays: z_lin must hold {steps} depths, got {list(z_lin.shape)}')
        _require(cam2world.numel() == n * 16,
                 f'render_rays: cam2world must be [{n}, 4, 4] (one camera per image), got {list(cam2world.shape)}')
        for name, t in (('jitter', jitter), ('sigma_noise', sigma_noise)):
            if t is not None:
                _require(t.numel() == n * rays_per_img * steps,
                         f'render_rays: {name} must be [{n}, {rays_per_img}, {steps}] (images, rays, steps), got {list(t.shape)}')

    @staticmethod
    def _ray_params(rays_d_cam, z_lin, cam2world, jitter, sigma_noise, tex_planes, geo_planes, mlp, clamp_mode, last_back, white_back,
                    max_depth):
        """-> (ide3d_render_params without outputs, tensors that must stay alive while it is in use)"""
        dev = tex_planes.device
        _require(tex_planes.ndim == 4, 'render_rays: tri-planes must be [n, 3*C, H, W]')
        VolumeRenderPlugin.check_render_shapes(tex_planes.shape[0], rays_d_cam.shape[0], z_lin.shape[0], rays_d_cam, z_lin, cam2world,
                                               jitter, sigma_noise)
        for t in (rays_d_cam, z_lin, cam2world, tex_planes, geo_planes):
            _require(t.is_cuda and t.dtype == torch.float32, 'render_rays: float32 CUDA tensors required')
        for t in (jitter, sigma_noise):
            _require(t is None or (t.dtype == torch.float32 and t.device == dev), 'render_rays: jitter / sigma_noise must be float32 next to the tri-planes')
        rays_d_cam, z_lin = rays_d_cam.contiguous(), z_lin.contiguous()
        cam2world = cam2world.reshape(-1, 16).contiguous()
        p = _RenderParams()
        VolumeRenderPlugin._fill_render_params(p, tex_planes, geo_planes, mlp)
        p.rays_d_cam, p.z_lin, p.cam2world = rays_d_cam.data_ptr(), z_lin.data_ptr(), cam2world.data_ptr()
        p.rays_per_img, p.steps = rays_d_cam.shape[0], z_lin.shape[0]
        keep = [rays_d_cam, z_lin, cam2world]
        if jitter is not None:
            jitter = jitter.contiguous(); keep.append(jitter); p.jitter = jitter.data_ptr()
        if sigma_noise is not None:
            sigma_noise = sigma_noise.contiguous(); keep.append(sigma_noise); p.sigma_noise = sigma_noise.data_ptr()
        p.clamp_mode, p.last_back, p.white_back = int(clamp_mode), int(bool(last_back)), int(bool(white_back))
        p.max_depth = float(max_depth or 0.0)
        return p, keep

    @staticmethod
    def _ray_outputs(p, dev):
        """Allocates (feat [n, feat+seg, rays], depth [n, rays], wsum [n, rays]) of a march and points `p`'s outputs at them."""
        n, R = p.n, p.rays_per_img
        feat = torch.empty([n, p.feat_ch + p.seg_ch, R], dtype=torch.float32, device=dev)
        depth = torch.empty([n, R], dtype=torch.float32, device=dev)
        wsum = torch.empty([n, R], dtype=torch.float32, device=dev)
        p.out_feat, p.out_depth, p.out_wsum = feat.data_ptr(), depth.data_ptr(), wsum.data_ptr()
        return feat, depth, wsum

    @staticmethod
    def _merged_samples(what, p, dev, merged):
        """(z_all, src, z_fine) of the merged march, checked against `p`'s shape -> the three, contiguous."""
        rays, S = p.n * p.rays_per_img, p.steps
        shapes = (('z_all', (rays, 2 * S), torch.float32), ('src', (rays, 2 * S), torch.int32), ('z_fine', (rays, S), torch.float32))
        for t_, (name, shape, dt) in zip(merged, shapes):
            _require(t_.dtype == dt and t_.device == dev and tuple(t_.shape) == shape,
                     f'{what}: {name} must be {list(shape)} {dt} next to the tri-planes, got {list(t_.shape)} {t_.dtype}')
        return tuple(t_.contiguous() for t_ in merged)

    @staticmethod
    def render_rays(rays_d_cam, z_lin, cam2world, jitter, sigma_noise, tex_planes, geo_planes, mlp,
                    clamp_mode, last_back, white_back, max_depth):
        dev = tex_planes.device
        p, keep = VolumeRenderPlugin._ray_params(rays_d_cam, z_lin, cam2world, jitter, sigma_noise, tex_planes, geo_planes, mlp,
                                                 clamp_mode, last_back, white_back, max_depth)
        feat, depth, wsum = VolumeRenderPlugin._ray_outputs(p, dev)
        with _dev_guard(dev):
            rc = load().ide3d_render_rays(ctypes.byref(p), _stream(tex_planes))
        if rc == -2:        # IDE3D_ENOKERNEL: configuration not covered by the fused kernel
            return None
        _check(rc, 'render_rays')
        return feat, depth, wsum

    @staticmethod
    def render_ray_weights(rays_d_cam, z_lin, cam2world, jitter, sigma_noise, tex_planes, geo_planes, mlp, clamp_mode,
                           want=('weights', 'z_vals', 'pdf_bins', 'pdf_weights'), last_back=False):
        """First pass of the hierarchical renderer (`ide3d_render_ray_weights`): the geometry branch only.  -> (weights [n*R, S], z_vals
        [n*R, S], pdf_bins [n*R, S-1], pdf_weights [n*R, S-2]), None in place of what `want` does not name (not computed); None when the
        library has no kernel for the configuration (IDE3D_ENOKERNEL: what `render_rays` declines, and S < 3 or S > 1024)."""
        dev = tex_planes.device
        p, keep = VolumeRenderPlugin._ray_params(rays_d_cam, z_lin, cam2world, jitter, sigma_noise, tex_planes, geo_planes, mlp,
                                                 clamp_mode, last_back, False, None)
        rays, S = p.n * p.rays_per_img, p.steps
        outs = [torch.empty([rays, max(S - k, 0)], dtype=torch.float32, device=dev) if name in want else None
                for name, k in (('weights', 0), ('z_vals', 0), ('pdf_bins', 1), ('pdf_weights', 2))]
        with _dev_guard(dev):
            rc = load().ide3d_render_ray_weights(ctypes.byref(p), *(_ptr(o) for o in outs), _stream(tex_planes))
        if rc == -2:        # IDE3D_ENOKERNEL
            return None
        _check(rc, 'render_ray_weights')
        return tuple(outs)

    @staticmethod
    def merge_depths(z_fine, z_coarse):
        """z_fine [rays, Sf], z_coarse [rays, Sc] -> (z_all [rays, Sf+Sc] float32, src [rays, Sf+Sc] int32): per ray the stable ascending order
        of cat([z_fine, z_coarse], 1) (`ide3d_merge_depths`); src indexes the concatenation."""
        _require(z_fine.is_cuda and z_fine.dtype == torch.float32 and z_fine.ndim == 2, 'merge_depths: z_fine must be 2-D float32 on a CUDA device')
        _require(z_coarse.dtype == torch.float32 and z_coarse.ndim == 2 and z_coarse.device == z_fine.device and z_coarse.shape[0] == z_fine.shape[0],
                 'merge_depths: z_coarse must be [rays, steps] float32 next to z_fine')
        z_fine, z_coarse = z_fine.contiguous(), z_coarse.contiguous()
        rays, sf, sc = z_fine.shape[0], z_fine.shape[1], z_coarse.shape[1]
        z_all = torch.empty([rays, sf + sc], dtype=torch.float32, device=z_fine.device)
        src = torch.empty([rays, sf + sc], dtype=torch.int32, device=z_fine.device)
        with _dev_guard(z_fine.device):
            rc = load().ide3d_merge_depths(_ptr(z_fine), _ptr(z_coarse), rays, sf, sc, _ptr(z_all), _ptr(src), _stream(z_fine))
        _check(rc, 'merge_depths')
        return z_all, src

    @staticmethod
    def render_rays_merged(rays_d_cam, z_lin, cam2world, jitter, tex_planes, geo_planes, mlp, clamp_mode, white_back, max_depth,
                           z_all, src, z_fine, last_back=False):
        """Merged march of the hierarchical renderer (`ide3d_render_rays_merged`): `render_rays` over the 2 S samples of each ray in the order
        `merge_depths(z_fine, z_vals)` gave (z_all, src [n*R, 2S]; z_fine [n*R, S]), no density noise.  -> (feat, depth, wsum) like
        `render_rays`, or None (IDE3D_ENOKERNEL, as `render_ray_weights`)."""
        dev = tex_planes.device
        p, keep = VolumeRenderPlugin._ray_params(rays_d_cam, z_lin, cam2world, jitter, None, tex_planes, geo_planes, mlp,
                                                 clamp_mode, last_back, white_back, max_depth)
        z_all, src, z_fine = VolumeRenderPlugin._merged_samples('render_rays_merged', p, dev, (z_all, src, z_fine))
        feat, depth, wsum = VolumeRenderPlugin._ray_outputs(p, dev)
        with _dev_guard(dev):
            rc = load().ide3d_render_rays_merged(ctypes.byref(p), _ptr(z_all), _ptr(src), _ptr(z_fine), 2 * p.steps, _stream(tex_planes))
        if rc == -2:        # IDE3D_ENOKERNEL
            return None
        _check(rc, 'render_rays_merged')
        return feat, depth, wsum

    @staticmethod
    def _render_backward(what, ray_args, upstream, plane_grads, param_grads, camera_grad, merged=None):
        """The one backward call behind the four public methods: `what` names the entry point (C symbol `ide3d_<what>`, error texts,
        `CALLS`), `ray_args` are the forward's twelve arguments, `upstream` is (grad_feat, grad_depth, grad_wsum) -> (dtex, dgeo, grads,
        dcam) with None for what was not asked; None when the library has no kernel for the configuration (IDE3D_ENOKERNEL).  `merged`:
        (z_all, src, z_fine) of the merged march (`render_rays_merged_backward` only)."""
        tex_planes, geo_planes, mlp = ray_args[5:8]
        dev = tex_planes.device
        p, keep = VolumeRenderPlugin._ray_params(*ray_args)
        n, R, nch = p.n, p.rays_per_img, p.feat_ch + p.seg_ch
        if merged is not None:
            merged = VolumeRenderPlugin._merged_samples(what, p, dev, merged)
        g = _RenderGrads()
        for name, t, shape in zip(('grad_feat', 'grad_depth', 'grad_wsum'), upstream, ((n, nch, R), (n, R), (n, R))):
            if t is not None:
                _require(t.numel() == math.prod(shape), f'{what}: {name} must hold {list(shape)} values, got {list(t.shape)}')
                t = t.to(device=dev, dtype=torch.float32).contiguous()
                keep.append(t)
                setattr(g, name, t.data_ptr())
        dtex = dgeo = grads = dcam = None
        if plane_grads:
            dtex = torch.empty(tex_planes.shape, dtype=torch.float32, device=dev, memory_format=torch.channels_last).zero_()
            dgeo = torch.empty(geo_planes.shape, dtype=torch.float32, device=dev, memory_format=torch.channels_last).zero_()
            g.grad_tex_planes, g.grad_geo_planes = dtex.data_ptr(), dgeo.data_ptr()
            g.grad_tex_stride, g.grad_geo_stride = _i64x4(dtex.stride()), _i64x4(dgeo.stride())
        lib = load()

        def workspace(kind, nbytes):
            key = (kind, nbytes, dev.index, _ws_domain(dev))
            return VolumeRenderPlugin._ws.entry(key, lambda: torch.empty([nbytes // 4], dtype=torch.float32, device=dev))[0].data_ptr()

        q_ref = c_ref = None
        if camera_grad:
            cbytes = lib.ide3d_render_camera_grad_workspace_bytes(ctypes.byref(p))
            if cbytes <= 0:        # no compiled form for (C, hidden), or too many steps: what the launch would answer with IDE3D_ENOKERNEL
                return None
            c = _RenderCameraGrads()
            dcam = torch.empty([n, 4, 4], dtype=torch.float32, device=dev)
            c.grad_cam2world, c.workspace, c.workspace_bytes = dcam.data_ptr(), workspace('render_camera_grad', cbytes), cbytes
            c_ref = ctypes.byref(c)
        if param_grads:
            query = lib.ide3d_render_param_grad_workspace_bytes if merged is None else lib.ide3d_render_merged_param_grad_workspace_bytes
            nbytes = query(ctypes.byref(p))
            if nbytes <= 0:        # as above
                return None
            q = _RenderParamGrads()
            grads = {k: torch.empty_like(mlp[k]) for k in VolumeRenderPlugin.MLP_KEYS}
            for k, t in grads.items():
                setattr(q, 'grad_' + k, t.data_ptr())
            q.workspace, q.workspace_bytes = workspace('render_param_grad', nbytes), nbytes
            q_ref = ctypes.byref(q)
        with _dev_guard(dev):
            if merged is not None:
                rc = lib.ide3d_render_rays_merged_backward(ctypes.byref(p), *(_ptr(t_) for t_ in merged), 2 * p.steps, ctypes.byref(g), q_ref,
                                                           _stream(tex_planes))
            else:
                extra = {'render_rays_backward': (), 'render_rays_backward_params': (q_ref,), 'render_rays_backward_camera': (q_ref, c_ref)}[what]
                rc = getattr(lib, 'ide3d_' + what)(ctypes.byref(p), ctypes.byref(g), *extra, _stream(tex_planes))
        if rc == -2:        # IDE3D_ENOKERNEL
            return None
        _check(rc, what)
        return dtex, dgeo, grads, dcam

    @staticmethod
    def render_rays_backward(rays_d_cam, z_lin, cam2world, jitter, sigma_noise, tex_planes, geo_planes, mlp, clamp_mode, last_back,
                             white_back, max_depth, grad_feat, grad_depth, grad_wsum):
        """Gradients of `render_rays` with respect to the two tri-planes: the same arguments as the forward, then dL/dfeat [n, feat+seg,
        rays], dL/ddepth [n, rays], dL/dwsum [n, rays] (each may be None = zero) -> (dL/dtex_planes, dL/dgeo_planes), channels_last
        float32 of the planes' shape; None when the library has no backward kernel for the configuration (IDE3D_ENOKERNEL)."""
        res = VolumeRenderPlugin._render_backward('render_rays_backward', (rays_d_cam, z_lin, cam2world, jitter, sigma_noise, tex_planes,
                                                  geo_planes, mlp, clamp_mode, last_back, white_back, max_depth),
                                                  (grad_feat, grad_depth, grad_wsum), True, False, False)
        return None if res is None else res[:2]

    @staticmethod
    def render_rays_backward_params(rays_d_cam, z_lin, cam2world, jitter, sigma_noise, tex_planes, geo_planes, mlp, clamp_mode, last_back,
                                    white_back, max_depth, grad_feat, grad_depth, grad_wsum, plane_grads=True):
        """`render_rays_backward` with the gradients of the eight decoder tensors of `mlp` as well (ide3d_render_rays_backward_params) ->
        (dL/dtex_planes | None, dL/dgeo_planes | None, {key of mlp: gradient of that gain-folded tensor}); None when the library has no
        kernel for the configuration.  `plane_grads=False`: no plane buffer is allocated and the kernel skips the tap scatter (decoder-only
        training on detached planes).  The decoder gradients are bit-reproducible from run to run; the per-wave partial sums live in a
        workspace of this plugin's cache (one per shape and launch domain, see `workspace_scope`)."""
        res = VolumeRenderPlugin._render_backward('render_rays_backward_params', (rays_d_cam, z_lin, cam2world, jitter, sigma_noise,
                                                  tex_planes, geo_planes, mlp, clamp_mode, last_back, white_back, max_depth),
                                                  (grad_feat, grad_depth, grad_wsum), plane_grads, True, False)
        return None if res is None else res[:3]

    @staticmethod
    def render_rays_backward_camera(rays_d_cam, z_lin, cam2world, jitter, sigma_noise, tex_planes, geo_planes, mlp, clamp_mode, last_back,
                                    white_back, max_depth, grad_feat, grad_depth, grad_wsum, plane_grads=True, param_grads=False):
        """The backward of `render_rays` with the gradient of the camera pose (ide3d_render_rays_backward_camera) -> (dL/dtex_planes | None,
        dL/dgeo_planes | None, {key of mlp: gradient} | None, dL/dcam2world [n, 4, 4] with a zero last row); None when the library has no
        kernel for the configuration.  `plane_grads=False`: no plane buffer is allocated, the tap scatter is skipped; `param_grads=True`:
        the eight decoder gradients as well.  The camera gradient (like the decoder's) is summed in a fixed order: bit-reproducible from
        run to run, and the same whatever else the call computes.  Both workspaces come from this plugin's cache."""
        return VolumeRenderPlugin._render_backward('render_rays_backward_camera', (rays_d_cam, z_lin, cam2world, jitter, sigma_noise,
                                                   tex_planes, geo_planes, mlp, clamp_mode, last_back, white_back, max_depth),
                                                   (grad_feat, grad_depth, grad_wsum), plane_grads, param_grads, True)

    @staticmethod
    def render_rays_merged_backward(rays_d_cam, z_lin, cam2world, jitter, tex_planes, geo_planes, mlp, clamp_mode, white_back, max_depth,
                                    z_all, src, z_fine, grad_feat, grad_depth, grad_wsum, plane_grads=True, param_grads=False,
                                    last_back=False):
        """Gradients of `render_rays_merged` (ide3d_render_rays_merged_backward): its arguments, then dL/dfeat, dL/ddepth, dL/dwsum (each may
        be None = zero) -> (dL/dtex_planes | None, dL/dgeo_planes | None, {key of mlp: gradient} | None); None when the library has no
        kernel for the configuration (IDE3D_ENOKERNEL: what `render_rays_merged` and `render_rays_backward` decline).  z_all, src and
        z_fine are constants of the backward, like jitter and the camera.  `plane_grads=False` (with `param_grads=True`): the tap scatter is
        skipped; `param_grads=True`: the eight decoder gradients, bit-reproducible, their partial sums in a workspace of this plugin's
        cache."""
        _require(plane_grads or param_grads, 'render_rays_merged_backward: no gradient requested')
        res = VolumeRenderPlugin._render_backward('render_rays_merged_backward', (rays_d_cam, z_lin, cam2world, jitter, None, tex_planes,
                                                  geo_planes, mlp, clamp_mode, last_back, white_back, max_depth),
                                                  (grad_feat, grad_depth, grad_wsum), plane_grads, param_grads, False, (z_all, src, z_fine))
        return None if res is None else res[:3]

    @staticmethod
    def sample_voxel(tex_planes, geo_planes, mlp, pts, sigma_only=False):
        dev = tex_planes.device
        pts = pts.contiguous()
        _require(pts.is_cuda and pts.dtype == torch.float32 and pts.ndim == 3 and pts.shape[2] == 3, 'pts must be [n, m, 3] float32')
        p = _RenderParams()
        VolumeRenderPlugin._fill_render_params(p, tex_planes, geo_planes, mlp)
        n, m = pts.shape[0], pts.shape[1]
        _require(n == p.n, 'pts batch must match the tri-plane batch')
        width = p.feat_ch + p.seg_ch + 1
        out = None if sigma_only else torch.empty([n * m, width], dtype=torch.float32, device=dev)
        sig = torch.empty([n * m], dtype=torch.float32, device=dev) if sigma_only else None
        if m:
            with _dev_guard(dev):
                rc = load().ide3d_sample_voxel(ctypes.byref(p), _ptr(pts), m, _ptr(out), _ptr(sig), int(sigma_only), _stream(pts))
            if rc == -2:
                return None
            _check(rc, 'sample_voxel')
        return sig if sigma_only else out


    @staticmethod
    def _lattice(n, voxel_size, corner, scale):
        lat = _Lattice()
        lat.n, lat.voxel_size, lat.scale = int(n), float(voxel_size), float(scale)
        for i in range(3):
            lat.corner[i] = float(corner[i])
        return lat

    @staticmethod
    def lattice_points(n, voxel_size, corner, scale, first, count, device):
        """Points [first, first + count) of the extract_shapes lattice (see ide3d_lattice in the header) -> [count, 3]."""
        device = torch.device(device)
        _require(device.type == 'cuda', 'lattice_points: CUDA device required')
        pts = torch.empty([count, 3], dtype=torch.float32, device=device)
        lat = VolumeRenderPlugin._lattice(n, voxel_size, corner, scale)
        with _dev_guard(device):
            rc = load().ide3d_lattice_points(ctypes.byref(lat), int(first), int(count), _ptr(pts), _stream(pts))
        _check(rc, 'lattice_points')
        return pts

    @staticmethod
    def density_lattice(tex_planes, geo_planes, mlp, n, voxel_size, corner, scale, first, count):
        """sigma of lattice points [first, first + count) for every image -> [batch * count]; None if no fused kernel."""
        p = _RenderParams()
        VolumeRenderPlugin._fill_render_params(p, tex_planes, geo_planes, mlp)
        lat = VolumeRenderPlugin._lattice(n, voxel_size, corner, scale)
        sig = torch.empty([p.n * int(count)], dtype=torch.float32, device=tex_planes.device)
        if count:
            with _dev_guard(tex_planes.device):
                rc = load().ide3d_density_lattice(ctypes.byref(p), ctypes.byref(lat), int(first), int(count), _ptr(sig), _stream(tex_planes))
            if rc == -2:
                return None
            _check(rc, 'density_lattice')
        return sig


class ModconvPlugin:
    _ws = _Workspaces(limit=1024)
    _heads_declined = set()      # (n, cin, cout, h, w, rows, arith) that ide3d_modconv2d_heads has no fused form for

    @staticmethod
    def _workspace(lib, x, w, n, cin, cout, h, wd, k, mode, per_image, arith):
        """The workspace entry of (weight, problem shape, device, launch domain, arithmetic)."""
        # one workspace per (weight, problem shape, device, launch domain): the split-K partials inside it belong to one launch at a
        # time; the domain is the current stream for eager callers and the owning GraphedRenderer inside `workspace_scope`
        # ... and per arithmetic: the packed weights of the split-bf16 loops differ from the fp32 loop's
        key = (0 if per_image else w.data_ptr(), tuple(w.shape), n, h, wd, mode, x.device.index, _ws_domain(x.device), arith)
        def alloc():
            nbytes = lib.ide3d_modconv_workspace_bytes(n, cin, cout, h, wd, k, mode, int(per_image))
            _require(nbytes >= 0, 'modconv2d: unsupported configuration')
            return torch.empty([max(nbytes // 4, 1)], dtype=torch.float32, device=x.device)
        return ModconvPlugin._ws.entry(key, alloc)

    @staticmethod
    def _params(lib, x, w, y, styles, dcoefs, noise, noise_strength, bias, act, alpha, gain, clamp, mode, arith, x_amax, y_amax):
        """ide3d_modconv_params of one modconv2d call (y_pitch left 0) -> (params, workspace entry, tensors to keep alive)."""
        n, cin, h, wd = x.shape
        per_image = (w.ndim == 5)
        cout, _, k, _ = w.shape[-4:]
        ent = ModconvPlugin._workspace(lib, x, w, n, cin, cout, h, wd, k, mode, per_image, arith)
        p = _ModconvParams()
        p.x, p.w, p.y = x.data_ptr(), w.data_ptr(), (y.data_ptr() if y is not None else None)
        keep = []
        for name, t in (('styles', styles), ('dcoefs', dcoefs), ('noise', noise), ('bias', bias)):
            if t is not None:
                t = t.contiguous(); keep.append(t)
                _require(t.is_cuda and t.dtype == torch.float32, f'modconv2d: {name} must be float32 on GPU')
                _require(t.device == x.device, f'modconv2d: {name} must reside on the same device as x')
                setattr(p, name, t.data_ptr())
        p.n, p.cin, p.cout, p.h, p.w_, p.k = n, cin, cout, h, wd, k
        p.noise_strength = float(noise_strength)
        p.act, p.alpha, p.gain, p.clamp = int(act), float(alpha), float(gain), float(clamp)
        p.mode = mode
        p.weights_packed = int((not per_image) and ModconvPlugin._ws.packed(ent, (w,))[0])
        p.w_batch_stride = (cout * cin * k * k) if per_image else 0
        p.arith = arith
        for name, t in (('x_amax', x_amax), ('y_amax', y_amax)):
            if t is not None:
                _require(t.is_cuda and t.device == x.device and t.dtype == torch.float32 and tuple(t.shape) == (n, AMAX_FLOATS) and t.is_contiguous(),
                         f'modconv2d: {name} must be a contiguous float32 [n, AMAX_FLOATS] tensor on the device of x')
                setattr(p, name, t.data_ptr())
        p.workspace, p.workspace_bytes = ent[0].data_ptr(), ent[0].numel() * 4
        return p, ent, keep

    @staticmethod
    def modconv2d(x, w, styles, dcoefs, noise, noise_strength, bias, act, alpha, gain, clamp, mode=0, arith=0, x_amax=None, y_amax=None, pad_rows=False):
        """arith: 0 = process default (`conv_arithmetic`), 1 = fp32 MFMA, 3 = bf16x3, 6 = bf16x6, 16 = f16x3 (include/ide3d_hip.h).
        x_amax [n, AMAX_FLOATS]: row max = bound of max |x| per image (the f16x3 arithmetic needs it; else it runs bf16x6);
        y_amax [n, AMAX_FLOATS], zeroed: its row maxima receive max |finite y| per image.
        mode 0: stride-1 k x k (modulated) conv, "same" padding, fused epilogue; mode 1: 3x3 stride-2 conv without padding
        (output ((h-3)//2+1) x ((w-3)//2+1)); mode 2: 3x3 transposed stride-2 conv (output (2h+1) x (2w+1)).
        styles / dcoefs / noise / bias may be None."""
        for t in (x, w):
            _require(t.is_cuda and t.dtype == torch.float32 and t.is_contiguous(), 'modconv2d: contiguous float32 CUDA tensors required')
        _require(w.device == x.device, 'modconv2d: w must reside on the same device as x')
        n, cin, h, wd = x.shape
        per_image = (w.ndim == 5)             # [n, cout, cin, k, k]: styles already folded into per-image weights
        if per_image:
            _require(w.shape[0] == n and styles is None, 'modconv2d: per-image weights need w.shape[0] == batch and styles=None')
        cout, cin2, k, k2 = w.shape[-4:]
        _require(cin == cin2 and k == k2 and k in (1, 3), 'modconv2d: weight must be [cout, cin, k, k] with k in {1, 3}')
        _require(mode in (0, 1, 2), 'modconv2d: mode must be 0, 1 or 2')
        _require(mode != 1 or (k == 3 and h >= 3 and wd >= 3), 'modconv2d: mode 1 is a 3x3 stride-2 convolution on an input of at least 3x3')
        oh, ow = (2 * h + 1, 2 * wd + 1) if mode == 2 else (((h - 3) // 2 + 1, (wd - 3) // 2 + 1) if mode == 1 else (h, wd))
        # pad_rows (mode 2): rows of the (2w + 1)-wide result padded to a multiple of 4 floats — returned as a view [..., :ow] of the padded
        # storage — so that the FIR that reads it next stages 16-byte aligned rows
        pitch = (ow + 3) // 4 * 4 if (pad_rows and mode == 2) else ow
        y = torch.empty([n, cout, oh, pitch], dtype=torch.float32, device=x.device)
        lib = load()
        arith = int(arith) or int(lib.ide3d_get_conv_arithmetic())
        if arith == 16 and x_amax is None:
            arith = 6          # f16x3 needs the bound on |x|; decided here so that the workspace (packed weights) is the bf16x6 one
        p, ent, keep = ModconvPlugin._params(lib, x, w, y, styles, dcoefs, noise, noise_strength, bias, act, alpha, gain, clamp, mode, arith, x_amax, y_amax)
        p.y_pitch = pitch if pitch != ow else 0
        with _dev_guard(x.device):
            rc = lib.ide3d_modconv2d(ctypes.byref(p), _stream(x))
        _check(rc, 'modconv2d')
        ModconvPlugin._ws.mark_packed(ent, () if per_image else (w,))
        return y if pitch == ow else y[..., :ow]

    @staticmethod
    def modconv2d_heads(x, w, styles, dcoefs, noise, noise_strength, bias, act, alpha, gain, clamp, head_w, head_bias, head_clamp,
                        want_x=True, arith=0, gate=None, heads_out=None):
        """A stride-1 3x3 `modconv2d` and the dual heads that read its output (`modconv2d(y, head_w, None, None, None, 0.0, head_bias, 1,
        0.0, 1.0, head_clamp)`, head_w [n, rows, cin, 1, 1] per-image) in one launch (ide3d_modconv2d_heads) -> (y or None, heads
        [n, rows, h, w]), bit-equal to the two calls; None when the fused form does not apply (the caller then makes the two calls).
        want_x=False: y is not written.  `gate` (plane_cells' map [n, 3, ceil(h / 4), ceil(w / 4)]): a workgroup with no set cell under its
        tile writes nothing, so the outputs hold defined values only under set cells (ide3d_modconv2d_heads_gated); or (map, plane_tile_list(map, h, w,
        th, tw), (th, tw)) with the launch's tile size (16 x 16 for 128 output channels, 32 x 16 for 64): the live tiles packed to the front of the grid.  `heads_out`: the contiguous
        [n, rows, h, w] tensor the heads are written into instead of a fresh one."""
        for t in (x, w, head_w):
            _require(t.is_cuda and t.dtype == torch.float32 and t.is_contiguous(), 'modconv2d_heads: contiguous float32 CUDA tensors required')
        n, cin, h, wd = x.shape
        cout = w.shape[0]
        _require(w.ndim == 4 and tuple(w.shape[1:]) == (cin, 3, 3), 'modconv2d_heads: w must be [cout, cin, 3, 3]')
        _require(head_w.ndim == 5 and head_w.shape[0] == n and head_w.shape[2] == cout and tuple(head_w.shape[3:]) == (1, 1),
                 'modconv2d_heads: head_w must be [n, rows, cout, 1, 1]')
        lib = load()
        arith = int(arith) or int(lib.ide3d_get_conv_arithmetic())
        if arith == 16:
            arith = 6          # (no x_amax here: what modconv2d runs without one)
        rows = head_w.shape[1]
        # the library's decision depends on the shape, the arithmetic and the knob only: a declined shape is remembered, so that callers that
        # try every dual-path block (the 512-channel ones always decline) pay for the allocations and parameter blocks once
        shape_key = (n, cin, cout, h, wd, rows, arith)
        knob_off = 'IDE3D_MODCONV_NO_HEAD_FUSION' in os.environ
        if knob_off or shape_key in ModconvPlugin._heads_declined:
            return None
        y = torch.empty([n, cout, h, wd], dtype=torch.float32, device=x.device) if want_x else None
        heads = torch.empty([n, rows, h, wd], dtype=torch.float32, device=x.device) if heads_out is None else heads_out
        _require(heads.dtype == torch.float32 and heads.device == x.device and tuple(heads.shape) == (n, rows, h, wd) and heads.is_contiguous(),
                 'modconv2d_heads: heads_out must be a contiguous float32 [n, rows, h, w] tensor on the device of x')
        p, ent, keep = ModconvPlugin._params(lib, x, w, y, styles, dcoefs, noise, noise_strength, bias, act, alpha, gain, clamp, 0, arith, None, None)
        hent = ModconvPlugin._workspace(lib, heads, head_w, n, cout, rows, h, wd, 1, 0, True, arith)
        e = _ModconvHeadEpilogue()
        e.w, e.y, e.rows, e.clamp, e.no_activation_output = head_w.data_ptr(), heads.data_ptr(), rows, float(head_clamp), int(not want_x)
        if head_bias is not None:
            head_bias = head_bias.contiguous()
            _require(head_bias.is_cuda and head_bias.dtype == torch.float32 and head_bias.numel() == rows, 'modconv2d_heads: head_bias must be float32 [rows] on GPU')
            e.bias = head_bias.data_ptr()
        e.workspace, e.workspace_bytes = hent[0].data_ptr(), hent[0].numel() * 4
        with _dev_guard(x.device):
            if gate is not None:
                rc = lib.ide3d_modconv2d_heads_gated(ctypes.byref(p), ctypes.byref(e), ctypes.byref(_plane_gate(gate, n, h, wd)), _stream(x))
            else:
                rc = lib.ide3d_modconv2d_heads(ctypes.byref(p), ctypes.byref(e), _stream(x))
        if rc == -2:        # IDE3D_ENOKERNEL
            ModconvPlugin._heads_declined.add(shape_key)
            return None
        _check(rc, 'modconv2d_heads')
        ModconvPlugin._ws.mark_packed(ent, (w,))          # (the 3x3 layer's entry only: `hent` belongs to per-image weights)
        return y, heads


class ModconvGradPlugin:
    """The streaming and reduction passes of the frozen-generator convolution backward (csrc/modconv_bwd.hip);
    the matrix work of that backward is `ModconvPlugin.modconv2d`."""

    @staticmethod
    def _f32(t, name, dev, shape=None):
        _require(t.is_cuda and t.dtype == torch.float32 and t.device == dev, f'{name} must be float32 on the device of the gradient')
        if shape is not None:
            _require(tuple(t.shape) == tuple(shape), f'{name} must be {list(shape)}, got {list(t.shape)}')
        return t

    @staticmethod
    def act_backward(dy, y, act, alpha, gain, clamp, noise=None, noise_strength=1.0, bias=None, dcoefs=None):
        """K1 (ide3d_modconv_act_backward) -> (dz or None, ddcoefs or None).  act 1 / 3: dz = bias_act's grad = 1 form with yref = y (clamp < 0:
        none); with `dcoefs`: ddcoefs = sum_p dz * (u - noise_strength * noise - bias) / dcoefs, u recovered from y.  act 0: the dot-only form,
        ddcoefs = sum_p dy * y / dcoefs, no dz.  dy [n, c, h, w] dense; y of that shape (rows may be padded: a view [..., :w] of wider rows)."""
        dev = dy.device
        ModconvGradPlugin._f32(dy, 'dy', dev)
        _require(dy.ndim == 4 and dy.is_contiguous(), 'act_backward: dy must be a contiguous [n, c, h, w] tensor')
        n, c, h, w = dy.shape
        ModconvGradPlugin._f32(y, 'y', dev, dy.shape)
        _require(y.stride(3) == 1 and y.stride(2) >= w and y.stride(1) == h * y.stride(2) and y.stride(0) == c * y.stride(1),
                 'act_backward: y must be dense apart from padded rows')
        _require(act in (0, 1, 3), 'act_backward: act must be 0 (dot only), 1 (linear) or 3 (lrelu)')
        _require(act != 0 or dcoefs is not None, 'act_backward: the dot-only form needs dcoefs')
        lib = load()
        p = _ActBwdParams()
        keep = []
        p.dy, p.y = dy.data_ptr(), y.data_ptr()
        p.y_pitch = y.stride(2) if y.stride(2) != w else 0
        dz = torch.empty_like(dy) if act != 0 else None
        if dz is not None:
            p.dz = dz.data_ptr()
        if noise is not None:
            noise = ModconvGradPlugin._f32(noise, 'noise', dev).contiguous(); keep.append(noise)
            _require(noise.numel() == h * w, 'act_backward: noise must be [h, w]')
            p.noise = noise.data_ptr()
        p.noise_strength = float(noise_strength)
        if bias is not None:
            bias = ModconvGradPlugin._f32(bias, 'bias', dev, (c,)).contiguous(); keep.append(bias)
            p.bias = bias.data_ptr()
        dd = ws = None
        if dcoefs is not None:
            dcoefs = ModconvGradPlugin._f32(dcoefs, 'dcoefs', dev, (n, c)).contiguous(); keep.append(dcoefs)
            dd = torch.empty([n, c], dtype=torch.float32, device=dev)
            nbytes = lib.ide3d_act_bwd_workspace_bytes(n, c, h, w)
            _require(nbytes > 0, 'act_backward: unsupported shape')
            ws = torch.empty([nbytes // 4], dtype=torch.float32, device=dev)
            p.dcoefs, p.ddcoefs, p.workspace, p.workspace_bytes = dcoefs.data_ptr(), dd.data_ptr(), ws.data_ptr(), nbytes
        p.n, p.c, p.h, p.w = n, c, h, w
        p.act, p.alpha, p.gain, p.clamp = int(act), float(alpha), float(gain), float(clamp)
        with _dev_guard(dev):
            rc = lib.ide3d_modconv_act_backward(ctypes.byref(p), _stream(dy))
        _check(rc, 'modconv_act_backward')
        return dz, dd

    @staticmethod
    def scale_dot(x, t, styles):
        """K2 (ide3d_modconv_scale_dot): (dx = styles[n, c] * t, dstyles = sum_p x * t) for x, t [n, c, h, w], styles [n, c]."""
        dev = t.device
        ModconvGradPlugin._f32(t, 't', dev)
        _require(t.ndim == 4 and t.is_contiguous(), 'scale_dot: t must be a contiguous [n, c, h, w] tensor')
        n, c, h, w = t.shape
        x = ModconvGradPlugin._f32(x, 'x', dev, t.shape).contiguous()
        styles = ModconvGradPlugin._f32(styles, 'styles', dev, (n, c)).contiguous()
        lib = load()
        dx = torch.empty_like(t)
        ds = torch.empty([n, c], dtype=torch.float32, device=dev)
        nbytes = lib.ide3d_act_bwd_workspace_bytes(n, c, h, w)
        _require(nbytes > 0, 'scale_dot: unsupported shape')
        ws = torch.empty([nbytes // 4], dtype=torch.float32, device=dev)
        with _dev_guard(dev):
            rc = lib.ide3d_modconv_scale_dot(_ptr(x), _ptr(t), _ptr(styles), _ptr(dx), _ptr(ds), n, c, h, w, _ptr(ws), nbytes, _stream(t))
        _check(rc, 'modconv_scale_dot')
        return dx, ds

    @staticmethod
    def head_weight_grad(dy, x):
        """K3 (ide3d_head_weight_grad): dw[n, o, i] = sum_p dy[n, o, p] * x[n, i, p] for dy [n, rows, h, w], x [n, cin, h, w]."""
        dev = dy.device
        ModconvGradPlugin._f32(dy, 'dy', dev)
        _require(dy.ndim == 4 and x.ndim == 4 and x.shape[0] == dy.shape[0] and x.shape[2:] == dy.shape[2:], 'head_weight_grad: dy [n, rows, h, w], x [n, cin, h, w]')
        dy = dy.contiguous()
        x = ModconvGradPlugin._f32(x, 'x', dev).contiguous()
        n, rows, h, w = dy.shape
        cin = x.shape[1]
        lib = load()
        nbytes = lib.ide3d_head_wgrad_workspace_bytes(n, rows, cin, h, w)
        _require(nbytes > 0, 'head_weight_grad: unsupported shape')
        ws = torch.empty([nbytes // 4], dtype=torch.float32, device=dev)
        dw = torch.empty([n, rows, cin], dtype=torch.float32, device=dev)
        with _dev_guard(dev):
            rc = lib.ide3d_head_weight_grad(_ptr(dy), _ptr(x), _ptr(dw), n, rows, cin, h, w, _ptr(ws), nbytes, _stream(dy))
        _check(rc, 'head_weight_grad')
        return dw

    @staticmethod
    def weight_grad(g, x, styles, dcoefs, mode=0, arith=0):
        """ide3d_modconv_weight_grad -> dw [cout, cin, 3, 3], the direct weight gradient of a modulated 3x3 convolution.
        mode 0: g [n, cout, h, w] (dz of a stride-1 layer); mode 2: g [n, cout, 2h + 1, 2w + 1] (the FIR adjoint g_t of an up-sampling layer);
        mode 1: g [n, cout, (h - 3) // 2 + 1, (w - 3) // 2 + 1] (dz of a stride-2 unpadded layer, section 5.19);
        x [n, cin, h, w]; styles [n, cin], dcoefs [n, cout] or None.  arith: 0 = the process arithmetic, 1 fp32, 6 bf16x6."""
        dev = g.device
        ModconvGradPlugin._f32(g, 'g', dev)
        _require(g.ndim == 4 and x.ndim == 4 and x.shape[0] == g.shape[0], 'weight_grad: g [n, cout, gh, gw], x [n, cin, h, w]')
        _require(mode in (0, 1, 2), 'weight_grad: mode must be 0, 1 or 2')
        n, cout = g.shape[:2]
        cin, h, w = x.shape[1:]
        _require(mode != 1 or (h >= 3 and w >= 3), 'weight_grad: mode 1 needs an x of at least 3 x 3')
        gshape = {0: (h, w), 1: ((h - 3) // 2 + 1, (w - 3) // 2 + 1), 2: (2 * h + 1, 2 * w + 1)}[mode]
        _require(tuple(g.shape[2:]) == gshape, f'weight_grad: g must be {gshape[0]} x {gshape[1]} for mode {mode} and an x of {h} x {w}')
        g = g.contiguous()
        x = ModconvGradPlugin._f32(x, 'x', dev).contiguous()
        if styles is not None:
            styles = ModconvGradPlugin._f32(styles, 'styles', dev, (n, cin)).contiguous()
        if dcoefs is not None:
            dcoefs = ModconvGradPlugin._f32(dcoefs, 'dcoefs', dev, (n, cout)).contiguous()
        lib = load()
        nbytes = lib.ide3d_wgrad_workspace_bytes(n, cin, cout, *(gshape if mode == 1 else (h, w)))      # (the grid the sum runs over)
        _require(nbytes > 0, 'weight_grad: unsupported shape')
        ws = torch.empty([nbytes // 4], dtype=torch.float32, device=dev)
        dw = torch.empty([cout, cin, 3, 3], dtype=torch.float32, device=dev)
        p = _WgradParams()
        p.g, p.x, p.dw = g.data_ptr(), x.data_ptr(), dw.data_ptr()
        p.styles = styles.data_ptr() if styles is not None else None
        p.dcoefs = dcoefs.data_ptr() if dcoefs is not None else None
        p.n, p.cin, p.cout, p.h, p.w, p.mode, p.arith = n, cin, cout, h, w, int(mode), int(arith)
        p.workspace, p.workspace_bytes = ws.data_ptr(), nbytes
        with _dev_guard(dev):
            rc = lib.ide3d_modconv_weight_grad(ctypes.byref(p), _stream(g))
        _check(rc, 'modconv_weight_grad')
        return dw

    @staticmethod
    def bias_noise_grad(dz, noise=False):
        """ide3d_bias_noise_grad -> (db [c], dnoise [h, w] or None): db = sum_{n,p} dz, dnoise = sum_{n,c} dz for dz [n, c, h, w]."""
        dev = dz.device
        ModconvGradPlugin._f32(dz, 'dz', dev)
        _require(dz.ndim == 4, 'bias_noise_grad: dz must be [n, c, h, w]')
        dz = dz.contiguous()
        n, c, h, w = dz.shape
        lib = load()
        nbytes = lib.ide3d_bias_noise_workspace_bytes(n, c, h, w)
        _require(nbytes > 0, 'bias_noise_grad: unsupported shape')
        ws = torch.empty([nbytes // 4], dtype=torch.float32, device=dev)
        db = torch.empty([c], dtype=torch.float32, device=dev)
        dn = torch.empty([h, w], dtype=torch.float32, device=dev) if noise else None
        with _dev_guard(dev):
            rc = lib.ide3d_bias_noise_grad(dz.data_ptr(), db.data_ptr(), _ptr(dn), n, c, h, w, ws.data_ptr(), nbytes, _stream(dz))
        _check(rc, 'bias_noise_grad')
        return db, dn


class _NoiseMap(ctypes.Structure):
    _fields_ = [('data', ctypes.c_void_p), ('side', ctypes.c_int32), ('reserved', ctypes.c_int32)]


class NoisePlugin:
    """The projector's noise regulariser and noise normaliser, batched over all maps of a call (csrc/noise_reg.hip).
    `maps`: a non-empty list of contiguous float32 [R, R] tensors on one device, R a power of two in 4..512."""

    MIN_SIDE, MAX_SIDE, MAX_MAPS = 4, 512, 1024
    _tables = {}          # (device, ((data_ptr, side), ...)) -> _Table: the device table is uploaded once per set of maps

    class _Table:
        pass

    @staticmethod
    def supported(t):
        """One map the kernels take (the callers' dispatch rule)."""
        return (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float32 and t.ndim == 2 and t.shape[0] == t.shape[1]
                and NoisePlugin.MIN_SIDE <= t.shape[0] <= NoisePlugin.MAX_SIDE and (t.shape[0] & (t.shape[0] - 1)) == 0 and t.is_contiguous())

    @staticmethod
    def _table(maps, what):
        _require(0 < len(maps) <= NoisePlugin.MAX_MAPS, f'{what}: 1..{NoisePlugin.MAX_MAPS} maps')
        dev = maps[0].device
        for t in maps:
            _require(NoisePlugin.supported(t) and t.device == dev,
                     f'{what}: every map must be a contiguous float32 [R, R] tensor on one device, R a power of two in 4..512')
        key = (dev, tuple((t.data_ptr(), t.shape[0]) for t in maps))
        tab = NoisePlugin._tables.get(key)
        if tab is None:
            lib = load()
            k = len(maps)
            tab = NoisePlugin._Table()
            tab.k = k
            tab.sides = (ctypes.c_int32 * k)(*[t.shape[0] for t in maps])
            host = (_NoiseMap * k)()
            for i, t in enumerate(maps):
                host[i].data, host[i].side = t.data_ptr(), t.shape[0]
            tab.device = torch.frombuffer(bytearray(bytes(host)), dtype=torch.uint8).to(dev)
            tab.reg_bytes = lib.ide3d_noise_reg_workspace_bytes(tab.sides, k)
            tab.levels = lib.ide3d_noise_reg_levels(tab.sides, k)
            tab.norm_bytes = lib.ide3d_noise_normalize_workspace_bytes(tab.sides, k)
            _require(tab.reg_bytes > 0 and tab.levels > 0 and tab.norm_bytes > 0, f'{what}: unsupported maps')
            tab.numels = [t.numel() for t in maps]
            if len(NoisePlugin._tables) >= 16:
                NoisePlugin._tables.clear()
            NoisePlugin._tables[key] = tab
        return tab, dev

    @staticmethod
    def noise_reg(maps):
        """ide3d_noise_reg -> (loss [] float32, means [levels, 2], workspace): the last two are what `noise_reg_backward` reads."""
        tab, dev = NoisePlugin._table(maps, 'noise_reg')
        ws = torch.empty([tab.reg_bytes // 4], dtype=torch.float32, device=dev)
        means = torch.empty([tab.levels, 2], dtype=torch.float32, device=dev)
        loss = torch.empty([], dtype=torch.float32, device=dev)
        with _dev_guard(dev):
            rc = load().ide3d_noise_reg(_ptr(tab.device), tab.sides, tab.k, _ptr(ws), tab.reg_bytes, _ptr(means), _ptr(loss), _stream(ws))
        _check(rc, 'noise_reg')
        return loss, means, ws

    @staticmethod
    def noise_reg_backward(maps, ws, means, dloss):
        """ide3d_noise_reg_backward -> [d loss / d map for every map] (views of one buffer); `dloss`: the upstream gradient, a one-element
        float32 tensor on the maps' device (read by the kernel, never by the host)."""
        tab, dev = NoisePlugin._table(maps, 'noise_reg_backward')
        _require(ws.is_cuda and ws.dtype == torch.float32 and ws.device == dev and ws.numel() * 4 >= tab.reg_bytes and ws.is_contiguous(),
                 'noise_reg_backward: workspace of another call')
        _require(means.dtype == torch.float32 and means.device == dev and tuple(means.shape) == (tab.levels, 2) and means.is_contiguous(),
                 'noise_reg_backward: means of another call')
        _require(dloss.dtype == torch.float32 and dloss.device == dev and dloss.numel() == 1, 'noise_reg_backward: dloss must be one float32 on the device')
        dloss = dloss.contiguous()
        grad = torch.empty([sum(tab.numels)], dtype=torch.float32, device=dev)
        with _dev_guard(dev):
            rc = load().ide3d_noise_reg_backward(_ptr(tab.device), tab.sides, tab.k, _ptr(ws), tab.reg_bytes, _ptr(means), _ptr(dloss), _ptr(grad),
                                                 _stream(grad))
        _check(rc, 'noise_reg_backward')
        return [g.view_as(t) for g, t in zip(grad.split(tab.numels), maps)]

    @staticmethod
    def noise_normalize(maps):
        """ide3d_noise_normalize, in place: n -= mean(n); n *= rsqrt(mean(n^2)) for every map.  The kernels write through raw pointers, so the
        version counter of every map is advanced here, as a torch in-place op would (caches and graph signatures keyed on versions go stale);
        like a torch in-place op it refuses a leaf that requires grad unless grad mode is off."""
        tab, dev = NoisePlugin._table(maps, 'noise_normalize')
        if torch.is_grad_enabled():
            _require(not any(t.requires_grad for t in maps), 'noise_normalize: an in-place update of a tensor that requires grad needs torch.no_grad()')
        ws = torch.empty([tab.norm_bytes // 4], dtype=torch.float32, device=dev)
        with _dev_guard(dev):
            rc = load().ide3d_noise_normalize(_ptr(tab.device), tab.sides, tab.k, _ptr(ws), tab.norm_bytes, _stream(ws))
        _check(rc, 'noise_normalize')
        for t in maps:
            torch.autograd.graph.increment_version(t)
        return maps


class LpipsPlugin:
    """The streaming passes of the VGG16 LPIPS distance and its image gradient (csrc/lpips.hip).  Every tensor is a
    contiguous float32 CUDA tensor on one device."""

    @staticmethod
    def _f32(t, name, dev=None, shape=None):
        _require(isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and (dev is None or t.device == dev),
                 f'lpips: {name} must be a contiguous float32 CUDA tensor on the device of the other arguments')
        if shape is not None:
            _require(tuple(t.shape) == tuple(shape), f'lpips: {name} must be {list(shape)}, got {list(t.shape)}')
        return t

    @staticmethod
    def prep(x, mean, std, f=1, in_scale=1.0, in_shift=0.0):
        """ide3d_lpips_prep: x [n, 3, H, W] -> ((f x f area mean) * in_scale + in_shift - mean) / std, [n, 3, H / f, W / f]."""
        LpipsPlugin._f32(x, 'x')
        _require(x.ndim == 4 and x.shape[1] == 3 and f >= 1 and x.shape[2] % f == 0 and x.shape[3] % f == 0, 'lpips prep: x [n, 3, H, W], f divides H and W')
        mean = LpipsPlugin._f32(mean.reshape(-1), 'mean', x.device, (3,))
        std = LpipsPlugin._f32(std.reshape(-1), 'std', x.device, (3,))
        n, _, H, W = x.shape
        y = torch.empty([n, 3, H // f, W // f], dtype=torch.float32, device=x.device)
        with _dev_guard(x.device):
            rc = load().ide3d_lpips_prep(_ptr(x), _ptr(y), _ptr(mean), _ptr(std), n, H, W, int(f), float(in_scale), float(in_shift), _stream(x))
        _check(rc, 'lpips_prep')
        return y

    @staticmethod
    def prep_backward(dy, std, f=1, in_scale=1.0):
        """ide3d_lpips_prep_backward: dy [n, 3, h, w] -> dx [n, 3, h f, w f]."""
        LpipsPlugin._f32(dy, 'dy')
        _require(dy.ndim == 4 and dy.shape[1] == 3 and f >= 1, 'lpips prep_backward: dy [n, 3, h, w]')
        std = LpipsPlugin._f32(std.reshape(-1), 'std', dy.device, (3,))
        n, _, h, w = dy.shape
        dx = torch.empty([n, 3, h * f, w * f], dtype=torch.float32, device=dy.device)
        with _dev_guard(dy.device):
            rc = load().ide3d_lpips_prep_backward(_ptr(dy), _ptr(dx), _ptr(std), n, h * f, w * f, int(f), float(in_scale), _stream(dy))
        _check(rc, 'lpips_prep_backward')
        return dx

    @staticmethod
    def maxpool2(x):
        """ide3d_maxpool2: [n, c, h, w] -> [n, c, h // 2, w // 2], bit-equal to F.max_pool2d(x, 2)."""
        LpipsPlugin._f32(x, 'x')
        _require(x.ndim == 4 and x.shape[2] >= 2 and x.shape[3] >= 2, 'maxpool2: x [n, c, h, w] with h, w >= 2')
        n, c, h, w = x.shape
        y = torch.empty([n, c, h // 2, w // 2], dtype=torch.float32, device=x.device)
        with _dev_guard(x.device):
            rc = load().ide3d_maxpool2(_ptr(x), _ptr(y), n * c, h, w, _stream(x))
        _check(rc, 'maxpool2')
        return y

    @staticmethod
    def stage_backward(y, dpool, dtap):
        """ide3d_lpips_stage_backward -> dz = (route(dpool) + dtap) where y > 0, else 0; dpool [n, c, h // 2, w // 2] or None."""
        LpipsPlugin._f32(y, 'y')
        _require(y.ndim == 4, 'lpips stage_backward: y [n, c, h, w]')
        n, c, h, w = y.shape
        LpipsPlugin._f32(dtap, 'dtap', y.device, y.shape)
        if dpool is not None:
            LpipsPlugin._f32(dpool, 'dpool', y.device, (n, c, h // 2, w // 2))
        dz = torch.empty_like(y)
        with _dev_guard(y.device):
            rc = load().ide3d_lpips_stage_backward(_ptr(y), _ptr(dpool), _ptr(dtap), _ptr(dz), n * c, h, w, _stream(y))
        _check(rc, 'lpips_stage_backward')
        return dz

    @staticmethod
    def _taps(acts, targets, lins, outs):
        k = len(acts)
        _require(1 <= k <= LPIPS_MAX_TAPS, f'lpips: 1..{LPIPS_MAX_TAPS} taps')
        dev, n = acts[0].device, acts[0].shape[0]
        taps = (_LpipsTap * k)()
        for i, a in enumerate(acts):
            LpipsPlugin._f32(a, 'tap', dev)
            _require(a.ndim == 4 and a.shape[0] == n, 'lpips: every tap must be [n, c, h, w]')
            taps[i].a, (taps[i].c, taps[i].h, taps[i].w) = a.data_ptr(), a.shape[1:]
            if targets is not None:
                taps[i].t = LpipsPlugin._f32(targets[i], 'target', dev, a.shape).data_ptr()
                taps[i].lin = LpipsPlugin._f32(lins[i], 'lin', dev, (a.shape[1],)).data_ptr()
            if outs is not None:
                taps[i].out = outs[i].data_ptr()
        return taps, k, n, dev

    @staticmethod
    def normalize(acts):
        """The normalise-only form of ide3d_lpips_head: [a / (sqrt(sum_c a^2) + 1e-10) for a in acts]."""
        outs = [torch.empty_like(a) for a in acts]
        taps, k, n, dev = LpipsPlugin._taps(acts, None, None, outs)
        with _dev_guard(dev):
            rc = load().ide3d_lpips_head(taps, k, n, None, 0, None, _stream(acts[0]))
        _check(rc, 'lpips_head')
        return outs

    @staticmethod
    def head(acts, targets, lins):
        """ide3d_lpips_head -> loss [] float32: sum over taps and images of mean_{h,w} sum_c lin[c] (u - t)^2, over n.  lins: [c] each."""
        taps, k, n, dev = LpipsPlugin._taps(acts, targets, lins, None)
        lib = load()
        nbytes = lib.ide3d_lpips_head_workspace_bytes(taps, k, n)
        _require(nbytes > 0, 'lpips head: unsupported taps')
        ws = torch.empty([nbytes // 8], dtype=torch.float64, device=dev)
        loss = torch.empty([], dtype=torch.float32, device=dev)
        with _dev_guard(dev):
            rc = lib.ide3d_lpips_head(taps, k, n, _ptr(ws), nbytes, _ptr(loss), _stream(acts[0]))
        _check(rc, 'lpips_head')
        return loss

    @staticmethod
    def head_backward(acts, targets, lins, dloss):
        """ide3d_lpips_head_backward -> [d loss / d a for a in acts]; dloss: a one-element float32 tensor on the device."""
        outs = [torch.empty_like(a) for a in acts]
        taps, k, n, dev = LpipsPlugin._taps(acts, targets, lins, outs)
        _require(dloss.is_cuda and dloss.dtype == torch.float32 and dloss.device == dev and dloss.numel() == 1, 'lpips head_backward: dloss must be one float32 on the device')
        dloss = dloss.contiguous()
        with _dev_guard(dev):
            rc = load().ide3d_lpips_head_backward(taps, k, n, _ptr(dloss), _stream(acts[0]))
        _check(rc, 'lpips_head_backward')
        return outs


class LpipsAlexPlugin:
    """The streaming passes of the AlexNet LPIPS distance and its image gradient beside `LpipsPlugin` (csrc/lpips_alex.hip, DESIGN.md
    section 5.20).  Every tensor is a contiguous float32 CUDA tensor on one device (the winner bytes: uint8)."""

    @staticmethod
    def _geometry(h, w, k, stride, pad):
        _require(1 <= k <= 16 and 1 <= stride <= k and 0 <= pad < k and h + 2 * pad >= k and w + 2 * pad >= k,
                 'lpips_alex: 1 <= k <= 16, 1 <= stride <= k, 0 <= pad < k and at least one window per side')
        return (h + 2 * pad - k) // stride + 1, (w + 2 * pad - k) // stride + 1

    @staticmethod
    def unfold2d(x, k, stride, pad):
        """ide3d_unfold2d: x [n, c, h, w] -> [n, c k k, ho, wo], bit-equal to F.unfold(x, k, padding=pad, stride=stride).reshape(...)."""
        LpipsPlugin._f32(x, 'x')
        _require(x.ndim == 4, 'unfold2d: x [n, c, h, w]')
        n, c, h, w = x.shape
        ho, wo = LpipsAlexPlugin._geometry(h, w, k, stride, pad)
        col = torch.empty([n, c * k * k, ho, wo], dtype=torch.float32, device=x.device)
        with _dev_guard(x.device):
            rc = load().ide3d_unfold2d(_ptr(x), _ptr(col), n, c, h, w, int(k), int(stride), int(pad), _stream(x))
        _check(rc, 'unfold2d')
        return col

    @staticmethod
    def fold2d(dcol, size, k, stride, pad):
        """ide3d_fold2d: dcol [n, c k k, ho, wo] -> dx [n, c, h, w] for size = (h, w): the adjoint of `unfold2d`."""
        LpipsPlugin._f32(dcol, 'dcol')
        h, w = (int(v) for v in size)
        ho, wo = LpipsAlexPlugin._geometry(h, w, k, stride, pad)
        _require(dcol.ndim == 4 and dcol.shape[1] % (k * k) == 0 and tuple(dcol.shape[2:]) == (ho, wo),
                 f'fold2d: dcol must be [n, c * {k * k}, {ho}, {wo}], got {list(dcol.shape)}')
        n, c = dcol.shape[0], dcol.shape[1] // (k * k)
        dx = torch.empty([n, c, h, w], dtype=torch.float32, device=dcol.device)
        with _dev_guard(dcol.device):
            rc = load().ide3d_fold2d(_ptr(dcol), _ptr(dx), n, c, h, w, int(k), int(stride), int(pad), _stream(dcol))
        _check(rc, 'fold2d')
        return dx

    @staticmethod
    def maxpool3s2p0(x, want_idx=True):
        """ide3d_maxpool3s2p0: [n, c, h, w] -> (y [n, c, (h-3)//2+1, (w-3)//2+1] bit-equal to F.max_pool2d(x, 3, 2), winner bytes or None)."""
        LpipsPlugin._f32(x, 'x')
        _require(x.ndim == 4 and x.shape[2] >= 3 and x.shape[3] >= 3, 'maxpool3s2p0: x [n, c, h, w] with h, w >= 3')
        n, c, h, w = x.shape
        y = torch.empty([n, c, (h - 3) // 2 + 1, (w - 3) // 2 + 1], dtype=torch.float32, device=x.device)
        idx = torch.empty(y.shape, dtype=torch.uint8, device=x.device) if want_idx else None
        with _dev_guard(x.device):
            rc = load().ide3d_maxpool3s2p0(_ptr(x), _ptr(y), _ptr(idx), n * c, h, w, _stream(x))
        _check(rc, 'maxpool3s2p0')
        return y, idx

    @staticmethod
    def tap_backward(y, g, idx, dtap):
        """ide3d_lpips_tap_backward -> dz = (route(g) + dtap) where y > 0, else 0.  idx given: g is the gradient of the 3x3 stride-2 pool of
        y, routed through the winner bytes; idx None: g has y's shape and is added as it is, or is None."""
        LpipsPlugin._f32(y, 'y')
        _require(y.ndim == 4, 'lpips tap_backward: y [n, c, h, w]')
        n, c, h, w = y.shape
        LpipsPlugin._f32(dtap, 'dtap', y.device, y.shape)
        pooled = idx is not None
        if pooled:
            _require(g is not None and h >= 3 and w >= 3, 'lpips tap_backward: winner bytes need a pooled gradient and h, w >= 3')
            ps = (n, c, (h - 3) // 2 + 1, (w - 3) // 2 + 1)
            LpipsPlugin._f32(g, 'g', y.device, ps)
            _require(idx.is_cuda and idx.dtype == torch.uint8 and idx.is_contiguous() and idx.device == y.device and tuple(idx.shape) == ps,
                     f'lpips tap_backward: idx must be a contiguous uint8 CUDA tensor {list(ps)}')
        elif g is not None:
            LpipsPlugin._f32(g, 'g', y.device, y.shape)
        dz = torch.empty_like(y)
        with _dev_guard(y.device):
            rc = load().ide3d_lpips_tap_backward(_ptr(y), _ptr(g), _ptr(idx), _ptr(dtap), _ptr(dz), n * c, h, w, int(pooled), _stream(y))
        _check(rc, 'lpips_tap_backward')
        return dz


class VggLossPlugin:
    """The streaming passes of the VGG19 feature loss and its image gradient beside `LpipsPlugin` (csrc/vgg_loss.hip, DESIGN.md section
    5.22).  Every tensor is a contiguous float32 CUDA tensor on one device."""

    _ws = _Workspaces()          # (bytes, device index, launch domain) -> the per-workgroup partial sums of feat_l1

    @staticmethod
    def feat_l1(acts, targets, weights):
        """ide3d_feat_l1 -> loss [] float32: sum_k weights[k] * mean |acts[k] - targets[k]|."""
        k = len(acts)
        _require(1 <= k <= LPIPS_MAX_TAPS and len(targets) == k and len(weights) == k, f'feat_l1: 1..{LPIPS_MAX_TAPS} taps, a target and a weight for each')
        dev, n = acts[0].device, acts[0].shape[0]
        taps = (_FeatL1Tap * k)()
        for i, (a, t, wt) in enumerate(zip(acts, targets, weights)):
            LpipsPlugin._f32(a, 'tap', dev)
            _require(a.ndim == 4 and a.shape[0] == n, 'feat_l1: every tap must be [n, c, h, w]')
            taps[i].a, taps[i].t = a.data_ptr(), LpipsPlugin._f32(t, 'target', dev, a.shape).data_ptr()
            taps[i].weight, (taps[i].c, taps[i].h, taps[i].w) = float(wt), a.shape[1:]
        lib = load()
        nbytes = lib.ide3d_feat_l1_workspace_bytes(taps, k, n)
        _require(nbytes > 0, 'feat_l1: unsupported taps')
        ws = VggLossPlugin._ws.entry((nbytes, dev.index, _ws_domain(dev)), lambda: torch.empty([nbytes // 8], dtype=torch.float64, device=dev))[0]
        loss = torch.empty([], dtype=torch.float32, device=dev)
        with _dev_guard(dev):
            rc = lib.ide3d_feat_l1(taps, k, n, _ptr(ws), nbytes, _ptr(loss), _stream(acts[0]))
        _check(rc, 'feat_l1')
        return loss

    @staticmethod
    def feat_l1_tap_backward(a, t, g, dloss, weight):
        """ide3d_feat_l1_tap_backward -> dz = (g + s sign(a - t)) where a > 0, else 0, s = fp32(double(dloss) * weight / a.numel()); g: the
        next convolution's input gradient, or None at the last tap; dloss: a one-element float32 tensor on the device."""
        LpipsPlugin._f32(a, 'a')
        _require(a.ndim == 4, 'feat_l1_tap_backward: a [n, c, h, w]')
        n, c, h, w = a.shape
        LpipsPlugin._f32(t, 't', a.device, a.shape)
        if g is not None:
            LpipsPlugin._f32(g, 'g', a.device, a.shape)
        _require(dloss.is_cuda and dloss.dtype == torch.float32 and dloss.device == a.device and dloss.numel() == 1,
                 'feat_l1_tap_backward: dloss must be one float32 on the device')
        dloss = dloss.contiguous()
        dz = torch.empty_like(a)
        with _dev_guard(a.device):
            rc = load().ide3d_feat_l1_tap_backward(_ptr(a), _ptr(t), _ptr(g), _ptr(dz), _ptr(dloss), float(weight), n * c, h, w, a.numel(), _stream(a))
        _check(rc, 'feat_l1_tap_backward')
        return dz

    @staticmethod
    def maxpool2_relu_backward(y, dpool):
        """ide3d_maxpool2_relu_backward -> dz = dpool routed to the first maximum of its 2x2 window where y > 0, else 0; y a ReLU output
        [n, c, h, w], dpool [n, c, h // 2, w // 2]."""
        LpipsPlugin._f32(y, 'y')
        _require(y.ndim == 4 and y.shape[2] >= 2 and y.shape[3] >= 2, 'maxpool2_relu_backward: y [n, c, h, w] with h, w >= 2')
        n, c, h, w = y.shape
        LpipsPlugin._f32(dpool, 'dpool', y.device, (n, c, h // 2, w // 2))
        dz = torch.empty_like(y)
        with _dev_guard(y.device):
            rc = load().ide3d_maxpool2_relu_backward(_ptr(y), _ptr(dpool), _ptr(dz), n * c, h, w, _stream(y))
        _check(rc, 'maxpool2_relu_backward')
        return dz


class MeshPlugin:
    """Marching cubes on a float32 CUDA volume (csrc/mesh.hip): `mcubes.marching_cubes` of render_mesh.py:31 /
    dnnlib/geometry.py:286.  The one host read is the pair of totals that sizes the outputs."""

    _ws = _Workspaces()          # (bytes, device index, launch domain) -> totals + per-workgroup pairs + one int32 per grid point
    _tables = {}                 # device index -> the case table on that device

    @staticmethod
    def _table(table, dev):
        t = MeshPlugin._tables.get(dev.index)
        if t is None:
            _require(tuple(table.shape) == (256, 16) and table.dtype == torch.uint8, 'marching_cubes: the case table is uint8 [256, 16]')
            t = MeshPlugin._tables[dev.index] = table.to(dev).contiguous()
        return t

    @staticmethod
    def _grid(volume):
        _require(volume.is_cuda and volume.dtype == torch.float32 and volume.ndim == 3 and volume.is_contiguous(),
                 'marching_cubes: volume must be a contiguous [X, Y, Z] float32 CUDA tensor')
        dev = volume.device if volume.device.index is not None else torch.device('cuda', torch.cuda.current_device())
        return dev, tuple(volume.shape)

    @staticmethod
    def count(volume, threshold, table):
        """ide3d_mesh_count -> (workspace, number of vertices, number of triangles).  Reading the two totals is the only synchronisation."""
        dev, (X, Y, Z) = MeshPlugin._grid(volume)
        lib = load()
        nbytes = lib.ide3d_mesh_workspace_bytes(X, Y, Z)
        _require(nbytes > 0, f'marching_cubes: unsupported grid {X} x {Y} x {Z} (1..1024 points per axis)')
        ws = MeshPlugin._ws.entry((nbytes, dev.index, _ws_domain(dev)), lambda: torch.empty([(nbytes + 7) // 8], dtype=torch.int64, device=dev))[0]
        with _dev_guard(dev):
            rc = lib.ide3d_mesh_count(_ptr(volume), X, Y, Z, float(threshold), _ptr(MeshPlugin._table(table, dev)), _ptr(ws), ws.numel() * 8, _stream(volume))
        _check(rc, 'mesh_count')
        nv, nt = (int(v) for v in ws[:2].tolist())
        _require(nv < 2 ** 31 and nt < 2 ** 31, f'marching_cubes: {nv} vertices / {nt} triangles do not fit int32 indices')
        return ws, nv, nt

    @staticmethod
    def emit(volume, threshold, table, ws, nv, nt, normals=False, flip=False, lattice=None):
        """ide3d_mesh_emit with the workspace and totals of `count` on the same volume and threshold -> (vertices, triangles, normals or None)."""
        dev, (X, Y, Z) = MeshPlugin._grid(volume)
        lat = VolumeRenderPlugin._lattice(max(X, Y, Z), *lattice) if lattice is not None else None
        vertices = torch.empty([nv, 3], dtype=torch.float32, device=dev)
        triangles = torch.empty([nt, 3], dtype=torch.int32, device=dev)
        nrm = torch.empty([nv, 3], dtype=torch.float32, device=dev) if normals else None
        with _dev_guard(dev):
            rc = load().ide3d_mesh_emit(_ptr(volume), X, Y, Z, float(threshold), _ptr(MeshPlugin._table(table, dev)),
                                        ctypes.byref(lat) if lat is not None else None, int(bool(flip)), _ptr(ws), ws.numel() * 8, nv, nt,
                                        _ptr(vertices), _ptr(triangles), _ptr(nrm), _stream(volume))
        _check(rc, 'mesh_emit')
        return vertices, triangles, nrm

    @staticmethod
    def marching_cubes(volume, threshold, table, normals=False, flip=False, lattice=None):
        """-> (vertices [V, 3] float32, triangles [T, 3] int32, normals [V, 3] float32 or None); `table`: mesh_extraction.case_table_bytes() as a
        tensor, `lattice`: None (index units) or (voxel_size, corner[3], scale) as in ide3d_lattice."""
        volume = volume.detach().contiguous()
        ws, nv, nt = MeshPlugin.count(volume, threshold, table)
        return MeshPlugin.emit(volume, threshold, table, ws, nv, nt, normals=normals, flip=flip, lattice=lattice)


class _StreamPlugin:
    """What the two stream encoders share: the frame and buffer checks, the workspace cache, the allocation of `out` and
    `offsets`.  A subclass gives `_name` (of its entry point), `_limits` (what it supports, for the refusal), `_ws`, and its two C calls:
    `_sizes(lib, N, H, W, C, *args)` -> (workspace bytes, worst-case output bytes) and `_run(lib, frames, N, H, W, C, args, buffers)` -> rc,
    `args` being the encoder's own arguments as integers."""

    @classmethod
    def _shape(cls, frames, args):
        _require(frames.is_cuda and frames.dtype == torch.uint8 and frames.ndim == 4 and frames.is_contiguous(),
                 f'{cls._name}: frames must be a contiguous [N, H, W, C] uint8 CUDA tensor')
        N, H, W, C = (int(v) for v in frames.shape)
        ws_bytes, out_bytes = cls._sizes(load(), N, H, W, C, *args)
        _require(ws_bytes > 0 and 0 < out_bytes < 2 ** 31, f'{cls._name}: unsupported call: {N} frames of {H} x {W} x {C}, arguments {args} ({cls._limits})')
        return (N, H, W, C), ws_bytes, out_bytes

    @classmethod
    def _launch(cls, frames, args, workspace, out, offsets):
        (N, H, W, C), _, _ = cls._shape(frames, args)
        for t, dt in ((workspace, torch.uint8), (out, torch.uint8), (offsets, torch.int64)):
            _require(t.is_cuda and t.device == frames.device and t.dtype == dt and t.is_contiguous(), f'{cls._name}: workspace / out are uint8, offsets int64, on the frames\' device')
        _require(offsets.numel() == N + 1, f'{cls._name}: offsets holds N + 1 values')
        with _dev_guard(frames.device):
            rc = cls._run(load(), _ptr(frames), N, H, W, C, args, (_ptr(workspace), workspace.numel(), _ptr(out), out.numel(), _ptr(offsets), _stream(frames)))
        _check(rc, cls._name)

    @classmethod
    def _encode(cls, frames, args):
        (N, H, W, C), ws_bytes, out_bytes = cls._shape(frames, args)
        dev = frames.device if frames.device.index is not None else torch.device('cuda', torch.cuda.current_device())
        ws = cls._ws.entry((ws_bytes, dev.index, _ws_domain(dev)), lambda: torch.empty([ws_bytes], dtype=torch.uint8, device=dev))[0]
        out = torch.empty([out_bytes], dtype=torch.uint8, device=dev)
        offsets = torch.empty([N + 1], dtype=torch.int64, device=dev)
        cls._launch(frames, args, ws, out, offsets)
        return out, offsets


class PngPlugin(_StreamPlugin):
    """Row filters + deflate of uint8 CUDA frames (csrc/png.hip): the compression inside `save_image` of
    gen_images.py:115-116.  `training.png` holds the host definition of the same bytes and the container."""

    _name = 'png_encode'
    _limits = '(filter mode, segment bytes): 1 or 3 channels, a power of two in [1024, 32768], below 2 GiB per call'
    _ws = _Workspaces()          # (bytes, device index, launch domain) -> filtered streams + segment slots + segment records

    @staticmethod
    def _sizes(lib, N, H, W, C, filter_mode, segment_bytes):
        return lib.ide3d_png_workspace_bytes(N, H, W, C, segment_bytes), lib.ide3d_png_out_bytes(N, H, W, C, segment_bytes)

    @staticmethod
    def _run(lib, frames, N, H, W, C, args, buffers):
        return lib.ide3d_png_encode(frames, N, H, W, C, *args, *buffers)

    @staticmethod
    def launch(frames, filter_mode, segment_bytes, workspace, out, offsets):
        """ide3d_png_encode into the caller's buffers (uint8 workspace and out, int64 offsets [N + 1], all on the frames' device)."""
        PngPlugin._launch(frames, (int(filter_mode), int(segment_bytes)), workspace, out, offsets)

    @staticmethod
    def encode(frames, filter_mode, segment_bytes):
        """-> (out uint8 [worst case], offsets int64 [N + 1]) on the device: stream k is out[offsets[k]:offsets[k + 1]]."""
        return PngPlugin._encode(frames, (int(filter_mode), int(segment_bytes)))


class JpegPlugin(_StreamPlugin):
    """Colour conversion, DCT, quantiser and Huffman coding of uint8 CUDA frames (csrc/jpeg.hip): the compression
    of the Motion-JPEG video sink.  `training.jpeg` holds the host definition of the same bytes and the markers."""

    _name = 'jpeg_encode'
    _limits = '(quality, subsampling, restart interval): 1 or 3 channels, sides 1..65535, 444 or 420 (RGB only), 1..65535 MCUs, below 2 GiB per call'
    _ws = _Workspaces()          # (bytes, device index, launch domain) -> interval slots + their sizes and positions

    @staticmethod
    def _sizes(lib, N, H, W, C, quality, subsampling, restart_interval):
        return (lib.ide3d_jpeg_workspace_bytes(N, H, W, C, subsampling, restart_interval), lib.ide3d_jpeg_out_bytes(N, H, W, C, subsampling, restart_interval))

    @staticmethod
    def _run(lib, frames, N, H, W, C, args, buffers):
        return lib.ide3d_jpeg_encode(frames, N, H, W, C, *args, *buffers)

    @staticmethod
    def launch(frames, quality, subsampling, restart_interval, workspace, out, offsets):
        """ide3d_jpeg_encode into the caller's buffers (uint8 workspace and out, int64 offsets [N + 1], all on the frames' device)."""
        JpegPlugin._launch(frames, (int(quality), int(subsampling), int(restart_interval)), workspace, out, offsets)

    @staticmethod
    def encode(frames, quality, subsampling, restart_interval):
        """-> (out uint8 [worst case], offsets int64 [N + 1]) on the device: scan k is out[offsets[k]:offsets[k + 1]]."""
        return JpegPlugin._encode(frames, (int(quality), int(subsampling), int(restart_interval)))


class MetricsPlugin:
    """Float64 moments and the fp32 pair engine's three epilogues on float32 CUDA features (csrc/metrics.hip): what
    calc_metrics.py does with a detector's features.  `training.metrics` holds the host definitions, the formulas on top and the routing.
    Every function works in the caller's buffers, on the current stream."""

    POLY, RADII, INSIDE = 0, 1, 2

    @staticmethod
    def _features(x, what):
        _require(isinstance(x, torch.Tensor) and x.is_cuda and x.dtype == torch.float32 and x.ndim == 2 and x.shape[0] > 0 and x.shape[1] > 0
                 and x.stride(1) == 1 and x.stride(0) >= x.shape[1], f'{what}: features must be a [n, d] float32 CUDA tensor with contiguous rows')
        return int(x.shape[0]), int(x.shape[1]), int(x.stride(0))

    @staticmethod
    def _buffer(t, dtype, numel, dev, what):
        _require(t.is_cuda and t.device == dev and t.dtype == dtype and t.is_contiguous() and t.numel() >= numel, f'{what}: needs a contiguous {dtype} buffer of {numel} elements on {dev}')

    @staticmethod
    def workspace_bytes(op, rows, cols, d, k_or_subsets):
        nbytes = load().ide3d_metrics_workspace_bytes(int(op), int(rows), int(cols), int(d), int(k_or_subsets))
        _require(nbytes >= 0, f'metrics: unsupported call (op {op}, {rows} x {cols} pairs, d = {d}, k or subsets = {k_or_subsets}): '
                 '1 <= d <= 8192, 1 <= n <= 2^22, 1 <= k <= 7 < n, 2 <= m <= 4096, 1 <= subsets <= 4096')
        return nbytes

    @staticmethod
    def workspace(op, rows, cols, d, k_or_subsets, device):
        return torch.empty([max(16, MetricsPlugin.workspace_bytes(op, rows, cols, d, k_or_subsets))], dtype=torch.uint8, device=device)

    @staticmethod
    def feature_moments(x, raw_mean, raw_cov):
        """raw_mean [d] += column sums of x, raw_cov [d, d] += x^T x, in float64, in place."""
        n, d, stride = MetricsPlugin._features(x, 'feature_moments')
        MetricsPlugin._buffer(raw_mean, torch.float64, d, x.device, 'feature_moments: raw_mean')
        MetricsPlugin._buffer(raw_cov, torch.float64, d * d, x.device, 'feature_moments: raw_cov')
        with _dev_guard(x.device):
            rc = load().ide3d_feature_moments(_ptr(x), n, d, stride, _ptr(raw_mean), _ptr(raw_cov), _stream(x))
        _check(rc, 'feature_moments')

    @staticmethod
    def poly_kernel_sums(x, y, xi, yi, workspace, sums):
        """sums float64 [subsets, 3] <- the three polynomial-kernel sums of every subset; xi, yi int32 [subsets, m]."""
        nx, d, sx = MetricsPlugin._features(x, 'poly_kernel_sums')
        ny, dy, sy = MetricsPlugin._features(y, 'poly_kernel_sums')
        _require(d == dy and y.device == x.device, 'poly_kernel_sums: x and y must share the feature width and the device')
        _require(xi.ndim == 2 and xi.shape == yi.shape, 'poly_kernel_sums: xi and yi must be [subsets, m]')
        subsets, m = int(xi.shape[0]), int(xi.shape[1])
        MetricsPlugin._buffer(xi, torch.int32, subsets * m, x.device, 'poly_kernel_sums: xi')
        MetricsPlugin._buffer(yi, torch.int32, subsets * m, x.device, 'poly_kernel_sums: yi')
        MetricsPlugin._buffer(sums, torch.float64, subsets * 3, x.device, 'poly_kernel_sums: sums')
        MetricsPlugin._buffer(workspace, torch.uint8, 0, x.device, 'poly_kernel_sums: workspace')
        with _dev_guard(x.device):
            rc = load().ide3d_poly_kernel_sums(_ptr(x), nx, sx, _ptr(y), ny, sy, d, _ptr(xi), _ptr(yi), subsets, m, _ptr(workspace), workspace.numel(), _ptr(sums), _stream(x))
        _check(rc, 'poly_kernel_sums')

    @staticmethod
    def knn_radii(f, k, workspace, radii_sq):
        """radii_sq float32 [n] <- the squared distance of every row to its k-th nearest other row."""
        n, d, stride = MetricsPlugin._features(f, 'knn_radii')
        MetricsPlugin._buffer(radii_sq, torch.float32, n, f.device, 'knn_radii: radii_sq')
        MetricsPlugin._buffer(workspace, torch.uint8, 0, f.device, 'knn_radii: workspace')
        with _dev_guard(f.device):
            rc = load().ide3d_knn_radii(_ptr(f), n, d, stride, int(k), _ptr(workspace), workspace.numel(), _ptr(radii_sq), _stream(f))
        _check(rc, 'knn_radii')

    @staticmethod
    def manifold_inside(probes, manifold, radii_sq, workspace, inside):
        """inside uint8 [np] <- 1 where the probe lies within the radius of some manifold row."""
        n_p, d, sp = MetricsPlugin._features(probes, 'manifold_inside')
        n_m, dm, sm = MetricsPlugin._features(manifold, 'manifold_inside')
        _require(d == dm and manifold.device == probes.device, 'manifold_inside: probes and manifold must share the feature width and the device')
        MetricsPlugin._buffer(radii_sq, torch.float32, n_m, probes.device, 'manifold_inside: radii_sq')
        MetricsPlugin._buffer(inside, torch.uint8, n_p, probes.device, 'manifold_inside: inside')
        MetricsPlugin._buffer(workspace, torch.uint8, 0, probes.device, 'manifold_inside: workspace')
        with _dev_guard(probes.device):
            rc = load().ide3d_manifold_inside(_ptr(probes), n_p, sp, _ptr(manifold), n_m, sm, d, _ptr(radii_sq), _ptr(workspace), workspace.numel(), _ptr(inside),
                                              _stream(probes))
        _check(rc, 'manifold_inside')


class MetricsEvalPlugin:
    """The arithmetic between the networks of PPL, Inception Score and mIoU (csrc/metrics_eval.hip).
    `training.metrics` holds the host definitions and the routing.  Every function works in the caller's buffers, on the current stream;
    an output or workspace passed as None is allocated here."""

    LABEL_DTYPES = {torch.int64: 0, torch.uint8: 1}

    @staticmethod
    def _buffer(t, dtype, numel, dev, what):
        _require(isinstance(t, torch.Tensor) and t.is_cuda and t.device == dev and t.dtype == dtype and t.is_contiguous() and t.numel() >= numel,
                 f'{what}: needs a contiguous {dtype} buffer of {numel} elements on {dev}')
        return t

    @staticmethod
    def ppl_prep(x, mean, std, window=None, f=1, in_scale=1.0, in_shift=0.0, out=None):
        """ide3d_ppl_prep: x [n, 3, H, W] -> ((f x f area mean inside window (y0, x0, h, w)) * in_scale + in_shift - mean) / std."""
        LpipsPlugin._f32(x, 'x')
        _require(x.ndim == 4 and x.shape[1] == 3, 'ppl_prep: x must be [n, 3, H, W]')
        n, _, H, W = (int(v) for v in x.shape)
        y0, x0, h, w = (int(v) for v in (window if window is not None else (0, 0, H, W)))
        f = int(f)
        _require(f >= 1 and h >= 1 and w >= 1 and h % f == 0 and w % f == 0 and 0 <= y0 and y0 + h <= H and 0 <= x0 and x0 + w <= W,
                 f'ppl_prep: the window ({y0}, {x0}, {h}, {w}) must lie inside the {H} x {W} image and f = {f} must divide it')
        mean = LpipsPlugin._f32(mean.reshape(-1), 'mean', x.device, (3,))
        std = LpipsPlugin._f32(std.reshape(-1), 'std', x.device, (3,))
        if out is None:
            out = torch.empty([n, 3, h // f, w // f], dtype=torch.float32, device=x.device)
        MetricsEvalPlugin._buffer(out, torch.float32, n * 3 * (h // f) * (w // f), x.device, 'ppl_prep: out')
        with _dev_guard(x.device):
            rc = load().ide3d_ppl_prep(_ptr(x), _ptr(out), _ptr(mean), _ptr(std), n, H, W, y0, x0, h, w, f, float(in_scale), float(in_shift), _stream(x))
        _check(rc, 'ppl_prep')
        return out

    @staticmethod
    def _pair_taps(acts, lins):
        k = len(acts)
        _require(1 <= k <= LPIPS_MAX_TAPS and len(lins) == k, f'lpips_pair_distances: 1..{LPIPS_MAX_TAPS} taps, one lin vector each')
        dev, n2 = acts[0].device, int(acts[0].shape[0])
        _require(n2 >= 2 and n2 % 2 == 0, 'lpips_pair_distances: every tap must hold 2 n images')
        taps = (_LpipsTap * k)()
        for i, (a, l) in enumerate(zip(acts, lins)):
            LpipsPlugin._f32(a, 'tap', dev)
            _require(a.ndim == 4 and a.shape[0] == n2, 'lpips_pair_distances: every tap must be [2 n, c, h, w]')
            taps[i].a, (taps[i].c, taps[i].h, taps[i].w) = a.data_ptr(), a.shape[1:]
            taps[i].lin = LpipsPlugin._f32(l, 'lin', dev, (a.shape[1],)).data_ptr()
        return taps, k, n2 // 2, dev

    @staticmethod
    def pair_workspace_bytes(acts, lins):
        taps, k, n, _ = MetricsEvalPlugin._pair_taps(acts, lins)
        nbytes = load().ide3d_lpips_pair_workspace_bytes(taps, k, n)
        _require(nbytes > 0, 'lpips_pair_distances: unsupported taps')
        return nbytes

    @staticmethod
    def lpips_pair_distances(acts, lins, scale, workspace=None, dist=None):
        """ide3d_lpips_pair_distances -> dist float32 [n]: scale * LPIPS(image i, image i + n) from the raw taps [2 n, c, h, w]."""
        taps, k, n, dev = MetricsEvalPlugin._pair_taps(acts, lins)
        lib = load()
        if workspace is None:
            nbytes = lib.ide3d_lpips_pair_workspace_bytes(taps, k, n)
            _require(nbytes > 0, 'lpips_pair_distances: unsupported taps')
            workspace = torch.empty([nbytes], dtype=torch.uint8, device=dev)
        MetricsEvalPlugin._buffer(workspace, torch.uint8, 0, dev, 'lpips_pair_distances: workspace')
        if dist is None:
            dist = torch.empty([n], dtype=torch.float32, device=dev)
        MetricsEvalPlugin._buffer(dist, torch.float32, n, dev, 'lpips_pair_distances: dist')
        with _dev_guard(dev):
            rc = lib.ide3d_lpips_pair_distances(taps, k, n, float(scale), _ptr(workspace), workspace.numel(), _ptr(dist), _stream(acts[0]))
        _check(rc, 'lpips_pair_distances')
        return dist

    @staticmethod
    def trimmed_mean(x, lo_rank, hi_rank, out=None):
        """ide3d_trimmed_mean -> out float64 [4] = (mean of the x between the two order statistics, lo, hi, count)."""
        _require(isinstance(x, torch.Tensor) and x.is_cuda and x.dtype == torch.float32 and x.ndim == 1 and x.is_contiguous() and x.numel() > 0,
                 'trimmed_mean: x must be a contiguous float32 CUDA vector')
        if out is None:
            out = torch.empty([4], dtype=torch.float64, device=x.device)
        MetricsEvalPlugin._buffer(out, torch.float64, 4, x.device, 'trimmed_mean: out')
        with _dev_guard(x.device):
            rc = load().ide3d_trimmed_mean(_ptr(x), x.numel(), int(lo_rank), int(hi_rank), _ptr(out), _stream(x))
        _check(rc, 'trimmed_mean')
        return out

    @staticmethod
    def inception_workspace_bytes(n, d, splits):
        nbytes = load().ide3d_inception_score_workspace_bytes(int(n), int(d), int(splits))
        _require(nbytes >= 0, f'inception_score: unsupported call ({n} x {d} probabilities in {splits} splits): 1 <= d <= 8192, 1 <= splits <= 4096, splits <= n <= 2^22')
        return nbytes

    @staticmethod
    def inception_score(p, splits, workspace=None, kl=None):
        """ide3d_inception_score -> kl float64 [splits]: per split the mean over its rows of sum_j p (log p - log mean_j)."""
        n, d, stride = MetricsPlugin._features(p, 'inception_score')
        if workspace is None:
            workspace = torch.empty([max(16, MetricsEvalPlugin.inception_workspace_bytes(n, d, splits))], dtype=torch.uint8, device=p.device)
        MetricsEvalPlugin._buffer(workspace, torch.uint8, 0, p.device, 'inception_score: workspace')
        if kl is None:
            kl = torch.empty([int(splits)], dtype=torch.float64, device=p.device)
        MetricsEvalPlugin._buffer(kl, torch.float64, int(splits), p.device, 'inception_score: kl')
        with _dev_guard(p.device):
            rc = load().ide3d_inception_score(_ptr(p), n, d, stride, int(splits), _ptr(workspace), workspace.numel(), _ptr(kl), _stream(p))
        _check(rc, 'inception_score')
        return kl

    @staticmethod
    def label_iou(a, b, classes, remap=None, counts=None, iou=None):
        """ide3d_label_iou -> (iou float32 [n], counts int32 [n, classes, 2]) of two label maps [n, ...] (int64 or uint8, one dtype)."""
        _require(isinstance(a, torch.Tensor) and isinstance(b, torch.Tensor) and a.is_cuda and b.device == a.device and a.dtype == b.dtype
                 and a.dtype in MetricsEvalPlugin.LABEL_DTYPES and a.shape == b.shape and a.ndim >= 2 and a.is_contiguous() and b.is_contiguous()
                 and a.numel() > 0, 'label_iou: two contiguous int64 or uint8 CUDA label maps [n, ...] of one shape, dtype and device')
        n, classes = int(a.shape[0]), int(classes)
        hw = a.numel() // n
        _require(1 <= classes <= 32, f'label_iou: classes must be 1..32, got {classes}')
        n_in = 0
        if remap is not None:
            MetricsEvalPlugin._buffer(remap, torch.int32, 1, a.device, 'label_iou: remap')
            n_in = remap.numel()
        if counts is None:
            counts = torch.empty([n, classes, 2], dtype=torch.int32, device=a.device)
        if iou is None:
            iou = torch.empty([n], dtype=torch.float32, device=a.device)
        MetricsEvalPlugin._buffer(counts, torch.int32, n * classes * 2, a.device, 'label_iou: counts')
        MetricsEvalPlugin._buffer(iou, torch.float32, n, a.device, 'label_iou: iou')
        with _dev_guard(a.device):
            rc = load().ide3d_label_iou(_ptr(a), _ptr(b), MetricsEvalPlugin.LABEL_DTYPES[a.dtype], n, hw, _ptr(remap), n_in, classes, _ptr(counts), _ptr(iou),
                                        _stream(a))
        _check(rc, 'label_iou')
        return iou, counts


class AugmentPlugin:
    """The geometric and colour stages of the ADA pipeline on float32 CUDA images (csrc/augment.hip): what
    training/augment.py:290-306 and 363-368 do, as one launch each way.  `training.augment` draws the parameters, folds the matrices and
    holds the PyTorch definition.  Every function works in the caller's buffers, on the current stream, and reads nothing back."""

    _band_loops = {}         # device index -> int32 [1]: workgroups whose window of U exceeded the LDS budget (they looped over pieces)

    @staticmethod
    def _images(x, what):
        _require(isinstance(x, torch.Tensor) and x.is_cuda and x.dtype == torch.float32 and x.ndim == 4 and x.is_contiguous(),
                 f'{what}: images must be a contiguous [n, c, h, w] float32 CUDA tensor')
        return [int(v) for v in x.shape]

    @staticmethod
    def _buffer(t, dtype, numel, dev, what):
        _require(isinstance(t, torch.Tensor) and t.is_cuda and t.device == dev and t.dtype == dtype and t.is_contiguous() and t.numel() >= numel,
                 f'{what}: needs a contiguous {dtype} buffer of {numel} elements on {dev}')

    @staticmethod
    def _counter(dev):
        key = dev.index if dev.index is not None else torch.cuda.current_device()
        t = AugmentPlugin._band_loops.get(key)
        if t is None:
            t = AugmentPlugin._band_loops[key] = torch.zeros([1], dtype=torch.int32, device=dev)
        return t

    @staticmethod
    def band_loops(device):
        """Workgroups of `geometric` on `device` so far that split their tile because its window exceeded the LDS budget (reads the device)."""
        return int(AugmentPlugin._counter(torch.device(device)).item())

    @staticmethod
    def _common(x, out, coords, margins, taps, color, what):
        n, c, h, w = AugmentPlugin._images(x, what)
        _require(isinstance(out, torch.Tensor) and out.is_cuda and out.dtype == torch.float32 and out.is_contiguous() and out.device == x.device,
                 f'{what}: the output must be a contiguous float32 buffer on {x.device}')
        AugmentPlugin._buffer(coords, torch.float32, n * 6, x.device, f'{what}: coords')
        AugmentPlugin._buffer(margins, torch.int32, 4, x.device, f'{what}: margins')
        AugmentPlugin._buffer(taps, torch.float32, 12, x.device, f'{what}: taps')
        _require(taps.numel() == 12, f'{what}: the geometric filter must have 12 taps (got {taps.numel()})')
        if color is not None:
            AugmentPlugin._buffer(color, torch.float32, n * 12, x.device, f'{what}: color')
        return n, c, h, w

    @staticmethod
    def geometric(x, out, coords, margins, taps, color=None):
        """out [n, c, h, w] <- the geometric stage of x under coords [n, 6] and the device margins [4]; then the colour matrix [n, 12] if given."""
        n, c, h, w = AugmentPlugin._common(x, out, coords, margins, taps, color, 'augment_geometric')
        with _dev_guard(x.device):
            rc = load().ide3d_augment_geometric(_ptr(x), _ptr(out), n, c, h, w, x.numel(), out.numel(), _ptr(coords), _ptr(margins), _ptr(taps), _ptr(color),
                                                _ptr(AugmentPlugin._counter(x.device)), _stream(x))
        _check(rc, 'augment_geometric')
        return out

    @staticmethod
    def geometric_backward(grad_out, grad_images, coords, margins, taps, color=None):
        """grad_images (zero-filled by the caller) += the transpose of `geometric` applied to grad_out."""
        n, c, h, w = AugmentPlugin._common(grad_out, grad_images, coords, margins, taps, color, 'augment_geometric_backward')
        with _dev_guard(grad_out.device):
            rc = load().ide3d_augment_geometric_backward(_ptr(grad_out), _ptr(grad_images), n, c, h, w, grad_out.numel(), grad_images.numel(), _ptr(coords),
                                                         _ptr(margins), _ptr(taps), _ptr(color), _stream(grad_out))
        _check(rc, 'augment_geometric_backward')
        return grad_images

    @staticmethod
    def color(x, out, color, transpose=False):
        """out <- color[:, :3, :3] @ x + color[:, :3, 3] per pixel (3 channels; row 0 as scale and offset for 1); transpose: the backward."""
        n, c, h, w = AugmentPlugin._images(x, 'augment_color')
        _require(isinstance(out, torch.Tensor) and out.is_cuda and out.dtype == torch.float32 and out.is_contiguous() and out.device == x.device,
                 f'augment_color: the output must be a contiguous float32 buffer on {x.device}')
        AugmentPlugin._buffer(color, torch.float32, n * 12, x.device, 'augment_color: color')
        with _dev_guard(x.device):
            rc = load().ide3d_augment_color(_ptr(x), _ptr(out), n, c, h * w, x.numel(), out.numel(), _ptr(color), int(bool(transpose)), _stream(x))
        _check(rc, 'augment_color')
        return out


class RasterPlugin:
    """Triangle rasterizer on float32 CUDA meshes (csrc/raster.hip): the pyrender step of render_mesh.py:36-61.
    `training.mesh_render` prepares the arguments (camera inversion in float64, the pixel grid) and holds the host definition."""

    _ws = _Workspaces()          # (bytes, device index, launch domain) -> status word + vertex records + z-buffer
    CULL = {'none': 0, 'back': 1, 'front': 2}

    @staticmethod
    def _workspace(dev, N, V, H, W):
        nbytes = load().ide3d_raster_workspace_bytes(N, V, H, W)
        _require(nbytes > 0, f'render_mesh: unsupported shape: {N} cameras, {V} vertices, {H} x {W} pixels')
        return RasterPlugin._ws.entry((nbytes, dev.index, _ws_domain(dev)), lambda: torch.empty([(nbytes + 15) // 16, 2], dtype=torch.int64, device=dev))[0]

    @staticmethod
    def _mesh(vertices, triangles):
        _require(vertices.is_cuda and vertices.dtype == torch.float32 and vertices.ndim == 2 and vertices.shape[1] == 3 and vertices.is_contiguous(),
                 'render_mesh: vertices must be a contiguous [V, 3] float32 CUDA tensor')
        dev = vertices.device if vertices.device.index is not None else torch.device('cuda', torch.cuda.current_device())
        if triangles is not None:
            _require(triangles.dtype == torch.int32 and triangles.ndim == 2 and triangles.shape[1] == 3 and triangles.is_contiguous() and triangles.device == vertices.device,
                     'render_mesh: triangles must be a contiguous [T, 3] int32 tensor on the vertices\' device')
        return dev

    @staticmethod
    def project(vertices, world2cam, H, W, view, near):
        """ide3d_raster_project -> the workspace; `view` = (fx, fy, sx, ox, sy, oy) as float32 values, world2cam [N, 3, 4] float32 on the device."""
        dev = RasterPlugin._mesh(vertices, None)
        N, V = int(world2cam.shape[0]), int(vertices.shape[0])
        _require(world2cam.dtype == torch.float32 and tuple(world2cam.shape) == (N, 3, 4) and world2cam.is_contiguous() and world2cam.device == vertices.device,
                 'render_mesh: world2cam must be a contiguous [N, 3, 4] float32 tensor on the vertices\' device')
        ws = RasterPlugin._workspace(dev, N, V, H, W)
        with _dev_guard(dev):
            rc = load().ide3d_raster_project(_ptr(vertices), V, _ptr(world2cam), N, H, W, *[float(v) for v in view], float(near), _ptr(ws), ws.numel() * 8,
                                             _stream(vertices))
        _check(rc, 'raster_project')
        return ws

    @staticmethod
    def records(ws, N, V):
        """The projected-vertex records of `project` as an int32 tensor [N, V, 4]: X, Y, float bits of the view depth, flags (a copy)."""
        return ws.view(torch.int32).reshape(-1)[4:4 + N * V * 4].reshape(N, V, 4).clone()

    @staticmethod
    def depth(ws, vertices, triangles, N, H, W, cull='none', large_min=None):
        """ide3d_raster_depth on the records in `ws`: clears and fills the z-buffer."""
        dev = RasterPlugin._mesh(vertices, triangles)
        _require(cull in RasterPlugin.CULL, f'render_mesh: cull must be one of {sorted(RasterPlugin.CULL)}')
        with _dev_guard(dev):
            rc = load().ide3d_raster_depth(_ptr(triangles), int(triangles.shape[0]), int(vertices.shape[0]), N, H, W, RasterPlugin.CULL[cull],
                                           -1 if large_min is None else int(large_min), _ptr(ws), ws.numel() * 8, _stream(vertices))
        _check(rc, 'raster_depth')

    @staticmethod
    def status(ws):
        """The status word `depth` left (IDE3D_RASTER_BAD_INDEX | IDE3D_RASTER_DROPPED): one host read."""
        return int(ws.view(torch.int32).reshape(-1)[0].item())

    @staticmethod
    def shade(ws, vertices, triangles, N, H, W, light, normals=None, colors=None, labels=None, two_sided=True, ambient=0.3, diffuse=0.7,
              base_color=(1.0, 1.0, 1.0), bg=1.0):
        """ide3d_raster_shade -> dict(depth [N, 1, H, W], triangle [N, H, W] int32, image [N, 3, H, W][, label [N, H, W] int32])."""
        dev = RasterPlugin._mesh(vertices, triangles)
        V = int(vertices.shape[0])
        _require(light.dtype == torch.float32 and tuple(light.shape) == (N, 3) and light.is_contiguous() and light.device == vertices.device, 'render_mesh: light must be float32 [N, 3]')
        for name, t, dt in (('normals', normals, torch.float32), ('colors', colors, torch.uint8)):
            _require(t is None or (t.dtype == dt and tuple(t.shape) == (V, 3) and t.is_contiguous() and t.device == vertices.device),
                     f'render_mesh: {name} must be a contiguous [V, 3] {dt} tensor on the vertices\' device')
        _require(labels is None or (labels.dtype == torch.int32 and tuple(labels.shape) == (V,) and labels.is_contiguous() and labels.device == vertices.device),
                 'render_mesh: labels must be a contiguous [V] int32 tensor on the vertices\' device')
        out = {'depth': torch.empty([N, 1, H, W], dtype=torch.float32, device=dev), 'triangle': torch.empty([N, H, W], dtype=torch.int32, device=dev),
               'image': torch.empty([N, 3, H, W], dtype=torch.float32, device=dev)}
        if labels is not None:
            out['label'] = torch.empty([N, H, W], dtype=torch.int32, device=dev)
        base = (ctypes.c_float * 3)(*[float(v) for v in base_color])
        if labels is not None and V == 0:          # nothing to look up: every pixel is background
            out['label'].fill_(-1)
            labels = None
        with _dev_guard(dev):
            rc = load().ide3d_raster_shade(_ptr(vertices), _ptr(triangles), V, N, H, W, _ptr(normals), _ptr(colors), _ptr(labels), _ptr(light),
                                           int(bool(two_sided)), float(ambient), float(diffuse), ctypes.byref(base), float(bg), _ptr(ws), ws.numel() * 8,
                                           _ptr(out['depth']), _ptr(out['triangle']), _ptr(out['image']), _ptr(out['label'] if labels is not None else None), _stream(vertices))
        _check(rc, 'raster_shade')
        return out


class ParseLossPlugin:
    """The passes between the convolutions of the face parser's cross-entropy loss and its image gradient (csrc/parse_loss.hip, DESIGN.md
    section 5.16).  Tensors are float32 CUDA tensors; dense NCHW unless a method says otherwise."""

    @staticmethod
    def _f32(t, name, dev=None, shape=None):
        _require(isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and (dev is None or t.device == dev),
                 f'parse_loss: {name} must be a contiguous float32 CUDA tensor on the device of the other arguments')
        if shape is not None:
            _require(tuple(t.shape) == tuple(shape), f'parse_loss: {name} must be {list(shape)}, got {list(t.shape)}')
        return t

    @staticmethod
    def resize(x, size):
        """ide3d_resize_bilinear: F.interpolate(x, size, mode='bilinear', align_corners=True) for x [n, c, h, w]."""
        ParseLossPlugin._f32(x, 'x')
        _require(x.ndim == 4, 'resize: x [n, c, h, w]')
        n, c, h, w = x.shape
        H, W = int(size[0]), int(size[1])
        y = torch.empty([n, c, H, W], dtype=torch.float32, device=x.device)
        with _dev_guard(x.device):
            rc = load().ide3d_resize_bilinear(_ptr(x), _ptr(y), n * c, h, w, H, W, _stream(x))
        _check(rc, 'resize_bilinear')
        return y

    @staticmethod
    def resize_backward(dy, size):
        """ide3d_resize_bilinear_backward: dy [n, c, H, W] -> the gradient of `resize`'s input of spatial `size`."""
        ParseLossPlugin._f32(dy, 'dy')
        _require(dy.ndim == 4, 'resize_backward: dy [n, c, H, W]')
        n, c, H, W = dy.shape
        h, w = int(size[0]), int(size[1])
        dx = torch.empty([n, c, h, w], dtype=torch.float32, device=dy.device)
        with _dev_guard(dy.device):
            rc = load().ide3d_resize_bilinear_backward(_ptr(dy), _ptr(dx), n * c, h, w, H, W, _stream(dy))
        _check(rc, 'resize_bilinear_backward')
        return dx

    @staticmethod
    def _ce_args(logits, labels):
        ParseLossPlugin._f32(logits, 'logits')
        _require(logits.ndim == 4 and labels.ndim == 3 and labels.shape[0] == logits.shape[0], 'parse_ce: logits [n, C, h, w], labels [n, H, W]')
        _require(labels.is_cuda and labels.device == logits.device and labels.dtype == torch.int64 and labels.is_contiguous(),
                 'parse_ce: labels must be a contiguous int64 tensor on the device of the logits')
        return (*logits.shape, labels.shape[1], labels.shape[2])

    @staticmethod
    def ce(logits, labels):
        """ide3d_parse_ce -> (loss [] float32, lse [n, H, W] float64): CrossEntropyLoss()(resize(logits, labels.shape[1:]), labels)."""
        n, C, h, w, H, W = ParseLossPlugin._ce_args(logits, labels)
        lib = load()
        nbytes = lib.ide3d_parse_ce_workspace_bytes(n, C, h, w, H, W)
        _require(nbytes > 0, 'parse_ce: unsupported shape')
        dev = logits.device
        ws = torch.empty([nbytes // 8], dtype=torch.float64, device=dev)
        lse = torch.empty([n, H, W], dtype=torch.float64, device=dev)
        loss = torch.empty([], dtype=torch.float32, device=dev)
        with _dev_guard(dev):
            rc = lib.ide3d_parse_ce(_ptr(logits), _ptr(labels), n, C, h, w, H, W, _ptr(lse), _ptr(ws), nbytes, _ptr(loss), _stream(logits))
        _check(rc, 'parse_ce')
        return loss, lse

    @staticmethod
    def ce_backward(logits, labels, lse, dloss):
        """ide3d_parse_ce_backward -> dlogits; dloss: a one-element float32 tensor on the device."""
        n, C, h, w, H, W = ParseLossPlugin._ce_args(logits, labels)
        dev = logits.device
        _require(lse.is_cuda and lse.device == dev and lse.dtype == torch.float64 and lse.is_contiguous() and tuple(lse.shape) == (n, H, W),
                 'parse_ce_backward: lse must be the float64 [n, H, W] tensor ce() returned')
        _require(dloss.is_cuda and dloss.dtype == torch.float32 and dloss.device == dev and dloss.numel() == 1, 'parse_ce_backward: dloss must be one float32 on the device')
        dl = torch.empty_like(logits)
        with _dev_guard(dev):
            rc = load().ide3d_parse_ce_backward(_ptr(logits), _ptr(labels), _ptr(lse), _ptr(dloss), _ptr(dl), n, C, h, w, H, W, _stream(logits))
        _check(rc, 'parse_ce_backward')
        return dl

    @staticmethod
    def maxpool(x, want_index=True):
        """ide3d_maxpool3s2 -> (F.max_pool2d(x, 3, 2, 1), winner bytes [n, c, oh, ow] uint8 or None)."""
        ParseLossPlugin._f32(x, 'x')
        _require(x.ndim == 4, 'maxpool3s2: x [n, c, h, w]')
        n, c, h, w = x.shape
        oh, ow = (h - 1) // 2 + 1, (w - 1) // 2 + 1
        y = torch.empty([n, c, oh, ow], dtype=torch.float32, device=x.device)
        idx = torch.empty([n, c, oh, ow], dtype=torch.uint8, device=x.device) if want_index else None
        with _dev_guard(x.device):
            rc = load().ide3d_maxpool3s2(_ptr(x), _ptr(y), _ptr(idx), n * c, h, w, _stream(x))
        _check(rc, 'maxpool3s2')
        return y, idx

    @staticmethod
    def maxpool_backward(dy, idx, size, mask=None):
        """ide3d_maxpool3s2_backward -> dx [n, c, *size]; mask [n, c, *size]: the gradient is zeroed where mask <= 0."""
        ParseLossPlugin._f32(dy, 'dy')
        _require(dy.ndim == 4, 'maxpool3s2_backward: dy [n, c, oh, ow]')
        n, c, oh, ow = dy.shape
        h, w = int(size[0]), int(size[1])
        _require((oh, ow) == ((h - 1) // 2 + 1, (w - 1) // 2 + 1), 'maxpool3s2_backward: dy does not belong to an input of that size')
        _require(idx.is_cuda and idx.device == dy.device and idx.dtype == torch.uint8 and idx.is_contiguous() and idx.shape == dy.shape,
                 'maxpool3s2_backward: idx must be the uint8 tensor maxpool() returned')
        if mask is not None:
            ParseLossPlugin._f32(mask, 'mask', dy.device, (n, c, h, w))
        dx = torch.empty([n, c, h, w], dtype=torch.float32, device=dy.device)
        with _dev_guard(dy.device):
            rc = load().ide3d_maxpool3s2_backward(_ptr(dy), _ptr(idx), _ptr(mask), _ptr(dx), n * c, h, w, _stream(dy))
        _check(rc, 'maxpool3s2_backward')
        return dx

    @staticmethod
    def join(terms, scale=None, bias=None, bias_gain=1.0, y=None, post=0):
        """ide3d_parse_join -> post(terms[0] * scale[n, c] + terms[1] + terms[2] + bias[n, c] * bias_gain), dense [n, c, h, w].
        terms: 1..3 entries, each a [n, c, h, w] tensor or view with contiguous rows, or (tensor [n, c, (h+1)//2, (w+1)//2], True) for a
        half-resolution map added at the even positions; terms[0] is full size.  post: 0 none, 1 relu, 2 zero where y <= 0."""
        terms = [t if isinstance(t, tuple) else (t, False) for t in terms]
        _require(1 <= len(terms) <= PARSE_JOIN_TERMS and not terms[0][1], f'parse_join: 1..{PARSE_JOIN_TERMS} terms, the first at full size')
        t0 = terms[0][0]
        _require(t0.ndim == 4, 'parse_join: terms are [n, c, h, w]')
        n, c, h, w = t0.shape
        dev = t0.device
        p = _ParseJoinParams()
        for i, (t, half) in enumerate(terms):
            want = (n, c, (h + 1) // 2, (w + 1) // 2) if half else (n, c, h, w)
            _require(t.is_cuda and t.device == dev and t.dtype == torch.float32 and tuple(t.shape) == want and (t.stride(3) == 1 or want[3] == 1),
                     f'parse_join: term {i} must be a float32 CUDA tensor {list(want)} with contiguous rows')
            q = p.term[i]
            q.p, q.batch_stride, q.plane_stride, q.row_pitch, q.half = t.data_ptr(), t.stride(0), t.stride(1), max(t.stride(2), want[3]), int(half)
        for name, t in (('scale', scale), ('bias', bias)):
            if t is not None:
                ParseLossPlugin._f32(t, name, dev)
                _require(t.numel() == n * c, f'parse_join: {name} must hold n * c values')
                setattr(p, name, t.data_ptr())
        if y is not None:
            p.y = ParseLossPlugin._f32(y, 'y', dev, (n, c, h, w)).data_ptr()
        out = torch.empty([n, c, h, w], dtype=torch.float32, device=dev)
        p.out, p.n, p.c, p.h, p.w, p.post, p.bias_gain = out.data_ptr(), n, c, h, w, int(post), float(bias_gain)
        with _dev_guard(dev):
            rc = load().ide3d_parse_join(ctypes.byref(p), _stream(t0))
        _check(rc, 'parse_join')
        return out

    @staticmethod
    def plane_sums(a, b=None, gain=1.0):
        """ide3d_plane_sums -> [n, c, 1, 1]: gain * sum over the pixels of a (* b)."""
        ParseLossPlugin._f32(a, 'a')
        _require(a.ndim == 4, 'plane_sums: a [n, c, h, w]')
        if b is not None:
            ParseLossPlugin._f32(b, 'b', a.device, a.shape)
        n, c, h, w = a.shape
        out = torch.empty([n, c, 1, 1], dtype=torch.float32, device=a.device)
        with _dev_guard(a.device):
            rc = load().ide3d_plane_sums(_ptr(a), _ptr(b), _ptr(out), n * c, h * w, float(gain), _stream(a))
        _check(rc, 'plane_sums')
        return out

    @staticmethod
    def stem_backward(dz, weight, size):
        """ide3d_parse_stem_backward: the input gradient [n, 3, *size] of conv2d(x, weight [cout, 3, 7, 7], stride=2, padding=3)."""
        ParseLossPlugin._f32(dz, 'dz')
        H, W = int(size[0]), int(size[1])
        _require(dz.ndim == 4 and tuple(dz.shape[2:]) == ((H - 1) // 2 + 1, (W - 1) // 2 + 1), 'stem_backward: dz [n, cout, (H-1)//2+1, (W-1)//2+1]')
        n, cout = dz.shape[:2]
        ParseLossPlugin._f32(weight, 'weight', dz.device, (cout, 3, 7, 7))
        dx = torch.empty([n, 3, H, W], dtype=torch.float32, device=dz.device)
        with _dev_guard(dz.device):
            rc = load().ide3d_parse_stem_backward(_ptr(dz), _ptr(weight), _ptr(dx), n, cout, H, W, _stream(dz))
        _check(rc, 'parse_stem_backward')
        return dx


class IdLossPlugin:
    """The passes of the ArcFace identity loss and its image gradient that are not convolutions, joins or plane sums (csrc/id_loss.hip,
    DESIGN.md section 5.17).  Tensors are contiguous float32 CUDA tensors unless a method says otherwise."""

    LINEAR_MAX_ROWS = 8          # kLinMaxN: images per launch of the linear layer (more are launched in groups)

    @staticmethod
    def _f32(t, name, dev=None, shape=None):
        _require(isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and (dev is None or t.device == dev),
                 f'id_loss: {name} must be a contiguous float32 CUDA tensor on the device of the other arguments')
        if shape is not None:
            _require(tuple(t.shape) == tuple(shape), f'id_loss: {name} must be {list(shape)}, got {list(t.shape)}')
        return t

    @staticmethod
    def _factor(shape):
        _require(len(shape) == 4 and shape[1] == 3 and shape[2] == shape[3] and shape[2] >= 256 and shape[2] % 256 == 0,
                 'id_prep: images are [n, 3, 256 f, 256 f] with an integer f >= 1')
        return shape[2] // 256

    @staticmethod
    def prep(x):
        """ide3d_id_prep: x [n, 3, 256 f, 256 f] -> [n, 3, 112, 112]: average pooling by f, the crop [35:223, 32:220], adaptive pooling to 112."""
        IdLossPlugin._f32(x, 'x')
        f = IdLossPlugin._factor(x.shape)
        y = torch.empty([x.shape[0], 3, 112, 112], dtype=torch.float32, device=x.device)
        with _dev_guard(x.device):
            rc = load().ide3d_id_prep(_ptr(x), _ptr(y), x.shape[0], f, _stream(x))
        _check(rc, 'id_prep')
        return y

    @staticmethod
    def prep_backward(dy, size):
        """ide3d_id_prep_backward: dy [n, 3, 112, 112] -> the gradient of `prep`'s input of spatial `size`."""
        n = dy.shape[0]
        IdLossPlugin._f32(dy, 'dy', None, (n, 3, 112, 112))
        f = IdLossPlugin._factor((n, 3, int(size[0]), int(size[1])))
        dx = torch.empty([n, 3, 256 * f, 256 * f], dtype=torch.float32, device=dy.device)
        with _dev_guard(dy.device):
            rc = load().ide3d_id_prep_backward(_ptr(dy), _ptr(dx), n, f, _stream(dy))
        _check(rc, 'id_prep_backward')
        return dx

    @staticmethod
    def prelu(x, slope):
        """ide3d_prelu: F.prelu(x, slope) for x [n, c, h, w], slope [c]."""
        IdLossPlugin._f32(x, 'x')
        _require(x.ndim == 4, 'prelu: x [n, c, h, w]')
        n, c, h, w = x.shape
        IdLossPlugin._f32(slope, 'slope', x.device, (c,))
        y = torch.empty_like(x)
        with _dev_guard(x.device):
            rc = load().ide3d_prelu(_ptr(x), _ptr(slope), _ptr(y), n, c, h, w, _stream(x))
        _check(rc, 'prelu')
        return y

    @staticmethod
    def prelu_backward(dy, x, slope):
        """ide3d_prelu_backward -> dx; x: the pre-activation; dy: [n, c, h, w], possibly a view with contiguous rows."""
        IdLossPlugin._f32(x, 'x')
        _require(x.ndim == 4, 'prelu_backward: x [n, c, h, w]')
        n, c, h, w = x.shape
        IdLossPlugin._f32(slope, 'slope', x.device, (c,))
        _require(dy.is_cuda and dy.device == x.device and dy.dtype == torch.float32 and dy.shape == x.shape and (dy.stride(3) == 1 or w == 1),
                 'prelu_backward: dy must be a float32 CUDA tensor of the shape of x with contiguous rows')
        dx = torch.empty_like(x)
        with _dev_guard(x.device):
            rc = load().ide3d_prelu_backward(ctypes.c_void_p(dy.data_ptr()), dy.stride(0), dy.stride(1), max(dy.stride(2), w), _ptr(x), _ptr(slope),
                                             _ptr(dx), n, c, h, w, _stream(x))
        _check(rc, 'prelu_backward')
        return dx

    @staticmethod
    def _se_args(s, w1, w2):
        IdLossPlugin._f32(s, 's')
        n, c = s.shape[0], s.numel() // max(s.shape[0], 1)
        r = w1.shape[0]
        IdLossPlugin._f32(w1, 'w1', s.device)
        IdLossPlugin._f32(w2, 'w2', s.device)
        _require(w1.numel() == r * c and w2.numel() == c * r and w2.shape[0] == c, 'se_gate: s [n, c], w1 [r, c], w2 [c, r]')
        return n, c, r

    @staticmethod
    def se_gate(s, w1, w2):
        """ide3d_se_gate: s [n, c(, 1, 1)] spatial means, w1 [r, c(, 1, 1)], w2 [c, r(, 1, 1)] -> sigmoid(w2 relu(w1 s)) in the shape of s."""
        n, c, r = IdLossPlugin._se_args(s, w1, w2)
        g = torch.empty_like(s)
        with _dev_guard(s.device):
            rc = load().ide3d_se_gate(_ptr(s), _ptr(w1), _ptr(w2), _ptr(g), n, c, r, _stream(s))
        _check(rc, 'se_gate')
        return g

    @staticmethod
    def se_gate_backward(s, w1, w2, g, dg):
        """ide3d_se_gate_backward: dg (the gradient of `se_gate`'s result g) -> ds, in the shape of s."""
        n, c, r = IdLossPlugin._se_args(s, w1, w2)
        IdLossPlugin._f32(g, 'g', s.device)
        IdLossPlugin._f32(dg, 'dg', s.device)
        _require(g.numel() == n * c and dg.numel() == n * c, 'se_gate_backward: g and dg hold n * c values')
        ds = torch.empty_like(s)
        with _dev_guard(s.device):
            rc = load().ide3d_se_gate_backward(_ptr(s), _ptr(w1), _ptr(w2), _ptr(g), _ptr(dg), _ptr(ds), n, c, r, _stream(s))
        _check(rc, 'se_gate_backward')
        return ds

    @staticmethod
    def _linear(x, weight, bias, backward):
        lib = load()
        IdLossPlugin._f32(x, 'dy' if backward else 'x')
        IdLossPlugin._f32(weight, 'weight', x.device)
        _require(x.ndim == 2 and weight.ndim == 2 and x.shape[1] == weight.shape[0 if backward else 1], 'linear: x [n, K], weight [M, K], dy [n, M]')
        M, K = weight.shape
        if bias is not None:
            IdLossPlugin._f32(bias, 'bias', x.device, (M,))
        out = torch.empty([x.shape[0], K if backward else M], dtype=torch.float32, device=x.device)
        query = lib.ide3d_linear_backward_input_workspace_bytes if backward else lib.ide3d_linear_workspace_bytes
        what = 'linear_backward_input' if backward else 'linear'
        step = IdLossPlugin.LINEAR_MAX_ROWS
        for i in range(0, x.shape[0], step):
            xs, ys = x[i:i + step], out[i:i + step]
            nbytes = query(xs.shape[0], K, M)
            _require(nbytes > 0, f'{what}: unsupported shape n = {xs.shape[0]}, K = {K}, M = {M} (K must be a multiple of 4)')
            ws = torch.empty([nbytes // 4], dtype=torch.float32, device=x.device)
            with _dev_guard(x.device):
                if backward:
                    rc = lib.ide3d_linear_backward_input(_ptr(xs), _ptr(weight), _ptr(ys), xs.shape[0], K, M, _ptr(ws), nbytes, _stream(x))
                else:
                    rc = lib.ide3d_linear(_ptr(xs), _ptr(weight), _ptr(bias), _ptr(ys), xs.shape[0], K, M, _ptr(ws), nbytes, _stream(x))
            _check(rc, what)
        return out

    @staticmethod
    def linear(x, weight, bias=None):
        """ide3d_linear: F.linear(x [n, K], weight [M, K], bias [M]); the weight is read once per 8 images."""
        return IdLossPlugin._linear(x, weight, bias, False)

    @staticmethod
    def linear_backward_input(dy, weight):
        """ide3d_linear_backward_input: dy [n, M] @ weight [M, K]."""
        return IdLossPlugin._linear(dy, weight, None, True)

    @staticmethod
    def linear_weight_grad(dy, x):
        """ide3d_linear_weight_grad: dy [n, M]^T @ x [n, K] -> [M, K], summed over the images in ascending order (n <= 8, K % 4 == 0)."""
        IdLossPlugin._f32(dy, 'dy')
        IdLossPlugin._f32(x, 'x', dy.device)
        _require(dy.ndim == 2 and x.ndim == 2 and dy.shape[0] == x.shape[0], 'linear_weight_grad: dy [n, M], x [n, K]')
        dy, x = dy.contiguous(), x.contiguous()
        (n, M), K = dy.shape, x.shape[1]
        dw = torch.empty([M, K], dtype=torch.float32, device=dy.device)
        with _dev_guard(dy.device):
            rc = load().ide3d_linear_weight_grad(_ptr(dy), _ptr(x), _ptr(dw), n, K, M, _stream(dy))
        _check(rc, 'linear_weight_grad')
        return dw

    @staticmethod
    def residual_join(a, b, gain):
        """ide3d_residual_join -> (a + b) * gain, or a * gain when b is None, in the shape of a: one launch, bit-equal to the element-wise definition."""
        IdLossPlugin._f32(a, 'a')
        _require(a.numel() > 0, 'residual_join: empty operand')
        a = a.contiguous()
        if b is not None:
            IdLossPlugin._f32(b, 'b', a.device)
            _require(b.shape == a.shape, 'residual_join: a and b must have one shape')
            b = b.contiguous()
        out = torch.empty(a.shape, dtype=torch.float32, device=a.device)
        with _dev_guard(a.device):
            rc = load().ide3d_residual_join(_ptr(a), _ptr(b), _ptr(out), a.numel(), float(gain), _stream(a))
        _check(rc, 'residual_join')
        return out

    @staticmethod
    def head(f, target=None):
        """ide3d_id_head -> (e [n, M] = f / |f|, norm [n], loss [] or None): loss = mean_i (1 - e_i . target_i) when target [n, M] is given."""
        IdLossPlugin._f32(f, 'f')
        _require(f.ndim == 2, 'id_head: f [n, M]')
        n, M = f.shape
        if target is not None:
            IdLossPlugin._f32(target, 'target', f.device, (n, M))
        e, norm = torch.empty_like(f), torch.empty([n], dtype=torch.float32, device=f.device)
        loss = torch.empty([], dtype=torch.float32, device=f.device) if target is not None else None
        with _dev_guard(f.device):
            rc = load().ide3d_id_head(_ptr(f), _ptr(target), _ptr(e), _ptr(norm), _ptr(loss), n, M, _stream(f))
        _check(rc, 'id_head')
        return e, norm, loss

    @staticmethod
    def head_backward(e, target, norm, dloss):
        """ide3d_id_head_backward -> df; dloss: a one-element float32 tensor on the device."""
        IdLossPlugin._f32(e, 'e')
        n, M = e.shape
        IdLossPlugin._f32(target, 'target', e.device, (n, M))
        IdLossPlugin._f32(norm, 'norm', e.device, (n,))
        _require(dloss.is_cuda and dloss.dtype == torch.float32 and dloss.device == e.device and dloss.numel() == 1, 'id_head_backward: dloss must be one float32 on the device')
        df = torch.empty_like(e)
        with _dev_guard(e.device):
            rc = load().ide3d_id_head_backward(_ptr(e), _ptr(target), _ptr(norm), _ptr(dloss), _ptr(df), n, M, _stream(e))
        _check(rc, 'id_head_backward')
        return df


class ClipLossPlugin:
    """The passes of the CLIP image-text loss and its image gradient that are not dense products (csrc/clip_loss.hip, DESIGN.md section
    5.37).  Tensors are contiguous float32 CUDA tensors unless a method says otherwise; token maps are channel-major, [n, C, T]."""

    SIDE = 224               # kClipSide: what the reference's Upsample(7) + AvgPool2d(S / 32) produce
    MAX_TOKENS = 64          # kAttMaxT
    MAX_HEAD_DIM = 64        # kAttMaxD
    EPS = 1e-5               # LayerNorm

    @staticmethod
    def _f32(t, name, dev=None, shape=None):
        _require(isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and (dev is None or t.device == dev),
                 f'clip_loss: {name} must be a contiguous float32 CUDA tensor on the device of the other arguments')
        if shape is not None:
            _require(tuple(t.shape) == tuple(shape), f'clip_loss: {name} must be {list(shape)}, got {list(t.shape)}')
        return t

    @staticmethod
    def _prep_args(shape, p, mean, std, dev):
        _require(len(shape) == 4 and shape[1] == 3 and shape[2] == shape[3] and shape[2] >= 32 and shape[2] % 32 == 0,
                 'clip_prep: images are [n, 3, 32 k, 32 k] with an integer k >= 1')
        _require(1 <= p <= ClipLossPlugin.SIDE and ClipLossPlugin.SIDE % p == 0, 'clip_prep: the patch size must divide 224')
        _require((mean is None) == (std is None), 'clip_prep: mean and std come together')
        for name, t in (('mean', mean), ('std', std)):
            if t is not None:
                ClipLossPlugin._f32(t, name, dev, (3,))
        return shape[2] // 32

    @staticmethod
    def prep(x, p, mean=None, std=None):
        """ide3d_clip_prep: x [n, 3, S, S] -> col [n, 3 p p, 224 / p, 224 / p]: Upsample(7), AvgPool2d(S / 32), ((v + 1) / 2 - mean) / std
        when mean and std (float32 [3] on the device) are given, unfolded into p x p patches."""
        ClipLossPlugin._f32(x, 'x')
        k = ClipLossPlugin._prep_args(x.shape, p, mean, std, x.device)
        g = ClipLossPlugin.SIDE // p
        col = torch.empty([x.shape[0], 3 * p * p, g, g], dtype=torch.float32, device=x.device)
        with _dev_guard(x.device):
            rc = load().ide3d_clip_prep(_ptr(x), _ptr(mean), _ptr(std), _ptr(col), x.shape[0], k, p, _stream(x))
        _check(rc, 'clip_prep')
        return col

    @staticmethod
    def prep_backward(dcol, size, p, std=None):
        """ide3d_clip_prep_backward: dcol [n, 3 p p, 224 / p, 224 / p] -> the gradient of `prep`'s input of spatial `size`."""
        ClipLossPlugin._f32(dcol, 'dcol')
        n = dcol.shape[0]
        k = ClipLossPlugin._prep_args((n, 3, int(size[0]), int(size[1])), p, std, std, dcol.device)
        g = ClipLossPlugin.SIDE // p
        _require(tuple(dcol.shape) == (n, 3 * p * p, g, g), 'clip_prep_backward: dcol [n, 3 p p, 224 / p, 224 / p]')
        dx = torch.empty([n, 3, 32 * k, 32 * k], dtype=torch.float32, device=dcol.device)
        with _dev_guard(dcol.device):
            rc = load().ide3d_clip_prep_backward(_ptr(dcol), _ptr(std), _ptr(dx), n, k, p, _stream(dcol))
        _check(rc, 'clip_prep_backward')
        return dx

    @staticmethod
    def embed(patches, table, gamma, beta):
        """ide3d_vit_embed: patches [n, C, T - 1] (any trailing shape with T - 1 elements), table [C, T] -> (ln_pre(tokens) [n, C, T], mean
        [n, T], rstd [n, T])."""
        ClipLossPlugin._f32(patches, 'patches')
        ClipLossPlugin._f32(table, 'table', patches.device)
        _require(patches.ndim >= 3 and table.ndim == 2, 'vit_embed: patches [n, C, T - 1], table [C, T]')
        n, C = patches.shape[:2]
        T = table.shape[1]
        _require(table.shape[0] == C and patches.numel() == n * C * (T - 1) and T >= 2, 'vit_embed: patches [n, C, T - 1], table [C, T]')
        ClipLossPlugin._f32(gamma, 'gamma', patches.device, (C,))
        ClipLossPlugin._f32(beta, 'beta', patches.device, (C,))
        y = torch.empty([n, C, T], dtype=torch.float32, device=patches.device)
        mean, rstd = (torch.empty([n, T], dtype=torch.float32, device=patches.device) for _ in range(2))
        with _dev_guard(patches.device):
            rc = load().ide3d_vit_embed(_ptr(patches), _ptr(table), _ptr(gamma), _ptr(beta), _ptr(y), _ptr(mean), _ptr(rstd), n, C, T,
                                        ClipLossPlugin.EPS, _stream(patches))
        _check(rc, 'vit_embed')
        return y, mean, rstd

    @staticmethod
    def embed_backward(dy, patches, table, gamma, mean, rstd):
        """ide3d_vit_embed_backward -> the gradient of the patch tokens, in the shape of `patches`."""
        ClipLossPlugin._f32(dy, 'dy')
        _require(dy.ndim == 3, 'vit_embed_backward: dy [n, C, T]')
        n, C, T = dy.shape
        dev = dy.device
        ClipLossPlugin._f32(patches, 'patches', dev)
        _require(patches.shape[:2] == dy.shape[:2] and patches.numel() == n * C * (T - 1) and T >= 2, 'vit_embed_backward: patches [n, C, T - 1]')
        ClipLossPlugin._f32(table, 'table', dev, (C, T))
        ClipLossPlugin._f32(gamma, 'gamma', dev, (C,))
        ClipLossPlugin._f32(mean, 'mean', dev, (n, T))
        ClipLossPlugin._f32(rstd, 'rstd', dev, (n, T))
        dp = torch.empty_like(patches)
        with _dev_guard(dev):
            rc = load().ide3d_vit_embed_backward(_ptr(dy), _ptr(patches), _ptr(table), _ptr(gamma), _ptr(mean), _ptr(rstd), _ptr(dp), n, C, T, _stream(dy))
        _check(rc, 'vit_embed_backward')
        return dp

    @staticmethod
    def layernorm(x, gamma, beta, tokens=None):
        """ide3d_layernorm: x [n, C, T] -> (y [n, C, tokens], mean [n, tokens], rstd [n, tokens]): LayerNorm over C of the first `tokens`
        tokens (default: all; 1 = the class token, read in place)."""
        ClipLossPlugin._f32(x, 'x')
        _require(x.ndim == 3, 'layernorm: x [n, C, T]')
        n, C, pitch = x.shape
        T = pitch if tokens is None else int(tokens)
        _require(1 <= T <= pitch, 'layernorm: 1 <= tokens <= T')
        ClipLossPlugin._f32(gamma, 'gamma', x.device, (C,))
        ClipLossPlugin._f32(beta, 'beta', x.device, (C,))
        y = torch.empty([n, C, T], dtype=torch.float32, device=x.device)
        mean, rstd = (torch.empty([n, T], dtype=torch.float32, device=x.device) for _ in range(2))
        with _dev_guard(x.device):
            rc = load().ide3d_layernorm(_ptr(x), _ptr(gamma), _ptr(beta), _ptr(y), _ptr(mean), _ptr(rstd), n, C, T, pitch, ClipLossPlugin.EPS, _stream(x))
        _check(rc, 'layernorm')
        return y, mean, rstd

    @staticmethod
    def layernorm_backward(dy, x, gamma, mean, rstd, add=None):
        """ide3d_layernorm_backward: dy [n, C, tokens] -> dx in the shape of x [n, C, T] (+ add [n, C, T]); an exact 0 past `tokens`."""
        ClipLossPlugin._f32(dy, 'dy')
        ClipLossPlugin._f32(x, 'x', dy.device)
        _require(dy.ndim == 3 and x.ndim == 3 and dy.shape[:2] == x.shape[:2] and dy.shape[2] <= x.shape[2], 'layernorm_backward: dy [n, C, tokens], x [n, C, T]')
        n, C, T = dy.shape
        pitch = x.shape[2]
        ClipLossPlugin._f32(gamma, 'gamma', dy.device, (C,))
        ClipLossPlugin._f32(mean, 'mean', dy.device, (n, T))
        ClipLossPlugin._f32(rstd, 'rstd', dy.device, (n, T))
        if add is not None:
            ClipLossPlugin._f32(add, 'add', dy.device, x.shape)
        dx = torch.empty_like(x)
        with _dev_guard(dy.device):
            rc = load().ide3d_layernorm_backward(_ptr(dy), _ptr(x), _ptr(gamma), _ptr(mean), _ptr(rstd), _ptr(add), _ptr(dx), n, C, T, pitch, _stream(dy))
        _check(rc, 'layernorm_backward')
        return dx

    @staticmethod
    def _att_args(qkv, heads):
        ClipLossPlugin._f32(qkv, 'qkv')
        _require(qkv.ndim == 3 and heads >= 1 and qkv.shape[1] % (3 * heads) == 0, 'vit_attention: qkv [n, 3 heads d, T]')
        n, C3, T = qkv.shape
        d = C3 // (3 * heads)
        _require(d % 4 == 0 and 4 <= d <= ClipLossPlugin.MAX_HEAD_DIM and 1 <= T <= ClipLossPlugin.MAX_TOKENS,
                 f'vit_attention: head dimension a multiple of 4 and <= {ClipLossPlugin.MAX_HEAD_DIM}, T <= {ClipLossPlugin.MAX_TOKENS}')
        return n, d, T

    @staticmethod
    def attention(qkv, heads):
        """ide3d_vit_attention: qkv [n, 3 C, T] -> [n, C, T], softmax(q k^T / sqrt(d)) v per head."""
        n, d, T = ClipLossPlugin._att_args(qkv, heads)
        out = torch.empty([n, heads * d, T], dtype=torch.float32, device=qkv.device)
        with _dev_guard(qkv.device):
            rc = load().ide3d_vit_attention(_ptr(qkv), _ptr(out), n, heads, d, T, float(d) ** -0.5, _stream(qkv))
        _check(rc, 'vit_attention')
        return out

    @staticmethod
    def attention_backward(qkv, dout, heads):
        """ide3d_vit_attention_backward: dout [n, C, T] -> dqkv [n, 3 C, T]."""
        n, d, T = ClipLossPlugin._att_args(qkv, heads)
        ClipLossPlugin._f32(dout, 'dout', qkv.device, (n, heads * d, T))
        dqkv = torch.empty_like(qkv)
        with _dev_guard(qkv.device):
            rc = load().ide3d_vit_attention_backward(_ptr(qkv), _ptr(dout), _ptr(dqkv), n, heads, d, T, float(d) ** -0.5, _stream(qkv))
        _check(rc, 'vit_attention_backward')
        return dqkv

    @staticmethod
    def quickgelu(x):
        """ide3d_quickgelu: x * sigmoid(1.702 x), in the shape of x."""
        ClipLossPlugin._f32(x, 'x')
        _require(x.numel() > 0, 'quickgelu: empty operand')
        y = torch.empty_like(x)
        with _dev_guard(x.device):
            rc = load().ide3d_quickgelu(_ptr(x), _ptr(y), x.numel(), _stream(x))
        _check(rc, 'quickgelu')
        return y

    @staticmethod
    def quickgelu_backward(dy, x):
        """ide3d_quickgelu_backward -> dx; x: the pre-activation."""
        ClipLossPlugin._f32(x, 'x')
        ClipLossPlugin._f32(dy, 'dy', x.device, x.shape)
        _require(x.numel() > 0, 'quickgelu_backward: empty operand')
        dx = torch.empty_like(x)
        with _dev_guard(x.device):
            rc = load().ide3d_quickgelu_backward(_ptr(dy), _ptr(x), _ptr(dx), x.numel(), _stream(x))
        _check(rc, 'quickgelu_backward')
        return dx

    @staticmethod
    def head(f, text, base=None):
        """ide3d_clip_head: f [n, D], text [T, D], base [n, D] or None -> (out [n, T] = 1 - cos(f - base, text), e [n, D], norm [n], tnorm [T],
        mean [] = the mean of out, summed in float64 before its values are rounded)."""
        ClipLossPlugin._f32(f, 'f')
        _require(f.ndim == 2, 'clip_head: f [n, D]')
        n, D = f.shape
        ClipLossPlugin._f32(text, 'text', f.device)
        _require(text.ndim == 2 and text.shape[1] == D and text.shape[0] >= 1, 'clip_head: text [T, D]')
        T = text.shape[0]
        if base is not None:
            ClipLossPlugin._f32(base, 'base', f.device, (n, D))
        e = torch.empty_like(f)
        norm, tnorm = torch.empty([n], dtype=torch.float32, device=f.device), torch.empty([T], dtype=torch.float32, device=f.device)
        out = torch.empty([n, T], dtype=torch.float32, device=f.device)
        rowsum, mean = torch.empty([n], dtype=torch.float64, device=f.device), torch.empty([], dtype=torch.float32, device=f.device)
        with _dev_guard(f.device):
            rc = load().ide3d_clip_head(_ptr(f), _ptr(base), _ptr(text), _ptr(e), _ptr(norm), _ptr(tnorm), _ptr(out), _ptr(rowsum), _ptr(mean), n, D, T,
                                        _stream(f))
        _check(rc, 'clip_head')
        return out, e, norm, tnorm, mean

    @staticmethod
    def head_backward(e, text, norm, tnorm, dout):
        """ide3d_clip_head_backward: dout [n, T] on the device -> df [n, D]."""
        ClipLossPlugin._f32(e, 'e')
        n, D = e.shape
        ClipLossPlugin._f32(text, 'text', e.device)
        T = text.shape[0]
        _require(tuple(text.shape) == (T, D), 'clip_head_backward: text [T, D]')
        ClipLossPlugin._f32(norm, 'norm', e.device, (n,))
        ClipLossPlugin._f32(tnorm, 'tnorm', e.device, (T,))
        ClipLossPlugin._f32(dout, 'dout', e.device, (n, T))
        df = torch.empty_like(e)
        with _dev_guard(e.device):
            rc = load().ide3d_clip_head_backward(_ptr(e), _ptr(text), _ptr(norm), _ptr(tnorm), _ptr(dout), _ptr(df), n, D, T, _stream(e))
        _check(rc, 'clip_head_backward')
        return df


class AdvLossPlugin:
    """The passes of the discriminator's adversarial loss and its image gradient that are not convolutions, FIR passes, joins or linear
    layers (csrc/adv_loss.hip).  Tensors are contiguous float32 CUDA tensors."""

    MAX_M = 8192             # kAdvMaxM

    @staticmethod
    def _f32(t, name, dev=None, shape=None):
        _require(isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and (dev is None or t.device == dev),
                 f'adv_loss: {name} must be a contiguous float32 CUDA tensor on the device of the other arguments')
        if shape is not None:
            _require(tuple(t.shape) == tuple(shape), f'adv_loss: {name} must be {list(shape)}, got {list(t.shape)}')
        return t

    @staticmethod
    def _group(n, group_size):
        """The `group` argument of the entry points for a layer's `group_size` (None: the whole batch): min(group_size, n)."""
        return n if group_size is None else min(int(group_size), n)

    @staticmethod
    def minibatch_std(x, group_size, features=1):
        """ide3d_minibatch_std: x [n, c, h, w] -> [n, c + features, h, w], `MinibatchStdLayer(group_size, features)(x)`."""
        AdvLossPlugin._f32(x, 'x')
        _require(x.ndim == 4, 'minibatch_std: x [n, c, h, w]')
        n, c, h, w = x.shape
        y = torch.empty([n, c + features, h, w], dtype=torch.float32, device=x.device)
        with _dev_guard(x.device):
            rc = load().ide3d_minibatch_std(_ptr(x), _ptr(y), n, c, h, w, AdvLossPlugin._group(n, group_size), features, _stream(x))
        _check(rc, 'minibatch_std')
        return y

    @staticmethod
    def minibatch_std_backward(x, dy, group_size, features=1):
        """ide3d_minibatch_std_backward: dy [n, c + features, h, w] -> dx [n, c, h, w]; x: the layer's input."""
        AdvLossPlugin._f32(x, 'x')
        _require(x.ndim == 4, 'minibatch_std_backward: x [n, c, h, w]')
        n, c, h, w = x.shape
        AdvLossPlugin._f32(dy, 'dy', x.device, (n, c + features, h, w))
        dx = torch.empty_like(x)
        with _dev_guard(x.device):
            rc = load().ide3d_minibatch_std_backward(_ptr(x), _ptr(dy), _ptr(dx), n, c, h, w, AdvLossPlugin._group(n, group_size), features, _stream(x))
        _check(rc, 'minibatch_std_backward')
        return dx

    @staticmethod
    def head(o, cmap, sign):
        """ide3d_adv_head -> (logit [n, 1], loss []): logit = (o * cmap).sum(1) / sqrt(M) (cmap None: o is [n, 1] and logit = o),
        loss = softplus(sign * logit).mean()."""
        AdvLossPlugin._f32(o, 'o')
        _require(o.ndim == 2, 'adv_head: o [n, M]')
        n, M = o.shape
        if cmap is not None:
            AdvLossPlugin._f32(cmap, 'cmap', o.device, (n, M))
        logit = torch.empty([n, 1], dtype=torch.float32, device=o.device)
        loss = torch.empty([], dtype=torch.float32, device=o.device)
        with _dev_guard(o.device):
            rc = load().ide3d_adv_head(_ptr(o), _ptr(cmap), _ptr(logit), _ptr(loss), n, M, int(sign), _stream(o))
        _check(rc, 'adv_head')
        return logit, loss

    @staticmethod
    def head_backward(o, cmap, logit, dloss, sign):
        """ide3d_adv_head_backward -> do [n, M]; dloss: a one-element float32 tensor on the device."""
        AdvLossPlugin._f32(o, 'o')
        n, M = o.shape
        if cmap is not None:
            AdvLossPlugin._f32(cmap, 'cmap', o.device, (n, M))
        AdvLossPlugin._f32(logit, 'logit', o.device, (n, 1))
        _require(dloss.is_cuda and dloss.dtype == torch.float32 and dloss.device == o.device and dloss.numel() == 1,
                 'adv_head_backward: dloss must be one float32 on the device')
        do = torch.empty_like(o)
        with _dev_guard(o.device):
            rc = load().ide3d_adv_head_backward(_ptr(o), _ptr(cmap), _ptr(logit), _ptr(dloss), _ptr(do), n, M, int(sign), _stream(o))
        _check(rc, 'adv_head_backward')
        return do


def modconv_plan(n, cin, cout, h, w, k=3, mode=0, per_image=False, arith=0, epilogue='conv', x_amax=False):
    """Host-only (works without a GPU): the kernel family, tile and grid `modconv2d` would launch for this shape -> dict of the
    ide3d_modconv_plan_info fields, `kind` as a name from PLAN_KINDS.  epilogue: 'conv' (noise, bias, lrelu, gain sqrt(2): the 3x3 layers),
    'plain' (demodulation only: the up-sampling layers, whose FIR carries the rest), 'head' (bias, clamp 256, linear), 'relu' (an unmodulated
    convolution + bias + ReLU: the feature nets), 'bias' (unmodulated + bias, linear: a convolution with its BatchNorm folded in) or 'grad'
    (unmodulated, no epilogue: the input gradient of one).  x_amax: the
    caller passes the producer's bound on |x| (what the f16x3 arithmetic needs)."""
    p = _ModconvParams()
    p.n, p.cin, p.cout, p.h, p.w_, p.k, p.mode = n, cin, cout, h, w, k, mode
    p.arith = int(arith)
    p.w_batch_stride = cout * cin * k * k if per_image else 0
    dummy = 256                                  # non-null, 16-byte aligned, never dereferenced
    p.x = p.w = p.y = dummy
    if not per_image and epilogue not in ('relu', 'bias', 'grad'):
        p.styles = p.dcoefs = dummy
    if epilogue == 'relu':               # an unmodulated convolution + bias + ReLU (training/lpips.py, training/face_parsing.py)
        p.bias, p.act, p.alpha, p.gain, p.clamp = dummy, 3, 0.0, 1.0, -1.0
    elif epilogue == 'bias':
        p.bias, p.act, p.gain, p.clamp = dummy, 1, 1.0, -1.0
    elif epilogue == 'grad':             # the input gradient of one: unmodulated, no epilogue
        p.act, p.gain, p.clamp = 1, 1.0, -1.0
    elif epilogue == 'conv':
        p.noise, p.bias, p.noise_strength, p.act, p.alpha, p.gain, p.clamp = dummy, dummy, 1.0, 3, 0.2, math.sqrt(2.0), -1.0
    elif epilogue == 'plain':
        p.act, p.gain, p.clamp = 1, 1.0, -1.0
    elif epilogue == 'head':
        p.bias, p.act, p.gain, p.clamp = dummy, 1, 1.0, 256.0
    else:
        raise ValueError(epilogue)
    if x_amax:
        p.x_amax = dummy
    info = _ModconvPlanInfo()
    rc = load().ide3d_modconv_plan(ctypes.byref(p), ctypes.byref(info))       # (not a launch: stays out of CALLS)
    if rc != 0:
        raise RuntimeError(f'modconv_plan failed (code {rc}): ' + load().ide3d_last_error().decode('utf-8', 'replace'))
    out = {name: getattr(info, name) for name, _ in _ModconvPlanInfo._fields_ if name != 'reserved'}
    out['kind'] = PLAN_KINDS[info.kind]
    return out


def composite_plan(rgb_sigma, rays=None, steps=None, ch=None):
    """Host-only (works without a GPU): the kernel form `VolumeRenderPlugin.composite` would launch -> dict of the ide3d_composite_plan_info
    fields, `form` as a name from COMPOSITE_FORMS.  rgb_sigma: a [rays, steps, ch + 1] tensor on any device (its shape and the 16-byte
    alignment of its address count; `.contiguous()` is applied as the launch does), or an address / alignment as an int next to rays,
    steps and ch."""
    if torch.is_tensor(rgb_sigma):
        rays, steps, row = rgb_sigma.shape
        ch, rgb_sigma = row - 1, rgb_sigma.contiguous().data_ptr()
    info = _CompositePlanInfo()
    rc = load().ide3d_composite_plan(ctypes.c_void_p(int(rgb_sigma)), rays, steps, ch, ctypes.byref(info))       # (not a launch: stays out of CALLS)
    if rc != 0:
        raise RuntimeError(f'composite_plan failed (code {rc}): ' + load().ide3d_last_error().decode('utf-8', 'replace'))
    return dict(form=COMPOSITE_FORMS[info.form], grid=info.grid, workgroup=info.workgroup, lds_bytes=info.lds_bytes)


def upfirdn2d_plan(x, f, upx=1, upy=1, downx=1, downy=1, padx0=0, padx1=0, pady0=0, pady1=0, flip=False, gain=1.0,
                   add=None, noise=None, bias=False, act=None, alpha=0.0, act_gain=1.0, clamp=-1.0, y_amax=False):
    """Host-only (works without a GPU): the kernel form `Upfirdn2dPlugin.upfirdn2d_ex` would launch for these arguments -> dict of the
    ide3d_upfirdn2d_plan_info fields: `form` as a name from UPFIRDN_FORMS, `instance` = (ux, uy, dx, dy, fw, fh, cx, cy) (None unless the
    form is tiled), `cell_u`, `staging`, `c_fastest`, `tiles_x`, `tiles_y`, `grid`, `lds_bytes`.
    x: a rank-4 tensor on any device (shape, strides, dtype, the 16-byte alignment of its address and the readable row length count), or a
    dict(shape=, stride=, dtype=, align=0, row_floats=0) (`align` = address modulo 16).  f: a rank-2 tensor or its shape.  add: None, a tensor
    or such a dict; noise: None / False, True (aligned), a tensor or an address modulo 16; bias, y_amax: present or not.  The output is laid
    out as the call lays it out, on a 16-byte aligned address (as device allocations are)."""
    base = 4096          # a non-null, 16-byte aligned stand-in address: the query never dereferences

    def spec(v):
        if torch.is_tensor(v):
            return tuple(v.shape), tuple(v.stride()), v.dtype, base + v.data_ptr() % 16, _row_floats_readable(v)
        return tuple(v['shape']), tuple(v['stride']), v['dtype'], base + int(v.get('align', 0)), int(v.get('row_floats', 0))

    x_shape, x_stride, dtype, x_ptr, row_floats = spec(x)
    _require(dtype in _DTYPE_CODE, 'x must be float16, bfloat16, float32 or float64')
    _require(len(x_shape) == 4, 'x must be rank 4')
    f_shape, f_stride = (tuple(f.shape), tuple(f.stride())) if torch.is_tensor(f) else (tuple(f), (f[1], 1))
    _require(len(f_shape) == 2, 'f must be rank 2')
    p, oshape, cl = _upfirdn_params(x_shape, x_stride, dtype, x_ptr, row_floats, f_shape, f_stride, base, upx, upy, downx, downy, padx0, padx1, pady0, pady1, flip, gain)
    y = torch.empty(oshape, dtype=dtype, device='meta', memory_format=torch.channels_last if cl else torch.contiguous_format)
    p.y, p.y_stride = base, _i64x4(y.stride())
    ep = _UpfirdnEpilogue()
    if add is not None:
        a_shape, a_stride, a_dtype, a_ptr, _ = spec(add)
        _require(a_shape == tuple(oshape) and a_dtype == dtype, 'add must match the output')
        ep.add, ep.add_stride = a_ptr, _i64x4(a_stride)
    if noise is not None and noise is not False:
        ep.noise = base + (0 if noise is True else noise.data_ptr() % 16 if torch.is_tensor(noise) else int(noise))
    if act is not None:
        ep.fused_act, ep.act = 1, int(act)
        ep.alpha, ep.act_gain, ep.clamp = float(alpha), float(act_gain), float(clamp)
        if bias:
            ep.bias = base
    if y_amax:
        ep.y_amax = base
    info = _UpfirdnPlanInfo()
    rc = load().ide3d_upfirdn2d_plan(ctypes.byref(p), ctypes.byref(ep), ctypes.byref(info))       # (not a launch: stays out of CALLS)
    if rc != 0:
        raise RuntimeError(f'upfirdn2d_plan failed (code {rc}): ' + load().ide3d_last_error().decode('utf-8', 'replace'))
    form = UPFIRDN_FORMS[info.form]
    return dict(form=form, instance=(info.ux, info.uy, info.dx, info.dy, info.fw, info.fh, info.cx, info.cy) if form in ('tile', 'fir44', 'fir_up2') else None,
                cell_u=info.cell_u, staging=info.staging, c_fastest=info.c_fastest, tiles_x=info.tiles_x, tiles_y=info.tiles_y,
                grid=info.grid, lds_bytes=info.lds_bytes)


_ARITH_NAMES = {'fp32': 1, 'bf16x3': 3, 'bf16x6': 6, 'f16x3': 16, 'default': 0}


def conv_arithmetic(name=None):
    """Get (no argument) or set the process-wide arithmetic of the shared-weight 3x3 convolutions (the per-image heads and the decoder MLPs of
    the ray-marcher follow it): 'bf16x6' (the default: every fp32 operand as 3 bf16 pieces, the 6 products above 2^-24 on the bf16 matrix
    pipe, fp32 accumulation - fp32-grade, measured as accurate as the fp32 matrix instruction against float64), 'fp32' (exact fp32
    products on v_mfma_f32_32x32x2_f32, 1.5x slower end to end), 'f16x3' (2 fp16 pieces, 3 products, power-of-two range scales from the
    producers' `amax`: ~2^-21 per product relative to the row / image maxima; the fastest fp32-grade mode), 'bf16x3' (2 bf16 pieces, 3
    products, ~2^-17 per product) or 'default' (back to the IDE3D_CONV_ARITH environment default, else bf16x6).  Returns the name in force.

    Safety beside other kernels: on MI355X a packed-fp32 instruction of ANOTHER kernel's wave returns wrong values
    while a wave on the same SIMD runs a loop of LDS reads + bf16 / fp16 MFMAs.  Every kernel of this library with such a loop keeps
    foreign waves off its SIMDs while the loop runs (8-wave workgroups that fill the register file of their SIMDs, or waves that claim
    all 512 registers), so every arithmetic may run beside kernels of other libraries, RCCL or another stream
    (tests/test_gpu_conv_arith.py::test_foreign_packed_fp32_victim_beside_every_matrix_loop)."""
    lib = load()
    if name is not None:
        _require(name in _ARITH_NAMES, f'conv_arithmetic: one of {sorted(_ARITH_NAMES)}')
        _check(lib.ide3d_set_conv_arithmetic(_ARITH_NAMES[name]), 'set_conv_arithmetic')
    code = int(lib.ide3d_get_conv_arithmetic())
    return {1: 'fp32', 3: 'bf16x3', 6: 'bf16x6', 16: 'f16x3'}[code]


class StylePlugin:
    @staticmethod
    def style_demod(w, affine_w, affine_b, affine_gain, bias_gain, wsq_t=None):
        """w [n, wdim] (rows may be strided), affine_w [cin, wdim], wsq_t [cin, cout] | None -> (styles [n, cin], dcoefs [n, cout] | None)."""
        _require(w.is_cuda and w.dtype == torch.float32 and w.ndim == 2 and w.stride(1) == 1, 'style_demod: w must be float32 [n, wdim] with unit inner stride')
        n, wdim = w.shape
        cin = affine_w.shape[0]
        _require(affine_w.is_contiguous() and affine_w.dtype == torch.float32 and affine_w.shape[1] == wdim, 'style_demod: bad affine weight')
        for name, t in (('affine_w', affine_w), ('affine_b', affine_b), ('wsq_t', wsq_t)):
            _require(t is None or t.device == w.device, f'style_demod: {name} must reside on the same device as w')
        styles = torch.empty([n, cin], dtype=torch.float32, device=w.device)
        dcoefs = None
        cout = 0
        if wsq_t is not None:
            _require(wsq_t.is_contiguous() and wsq_t.shape[0] == cin, 'style_demod: wsq_t must be contiguous [cin, cout]')
            cout = wsq_t.shape[1]
            dcoefs = torch.empty([n, cout], dtype=torch.float32, device=w.device)
        with _dev_guard(w.device):
            rc = load().ide3d_style_demod(_ptr(w), w.stride(0), _ptr(affine_w), _ptr(affine_b), _ptr(wsq_t), n, cin, cout, wdim,
                                          float(affine_gain), float(bias_gain), _ptr(styles), _ptr(dcoefs), _stream(w))
        _check(rc, 'style_demod')
        return styles, dcoefs

    @staticmethod
    def fold_heads(w, affine_gain, a0, b0, w0, gain0, a1, b1, w1, gain1):
        """-> per-image folded head weights [n, cout0 + cout1, cin, 1, 1]."""
        _require(w.is_cuda and w.dtype == torch.float32 and w.ndim == 2 and w.stride(1) == 1, 'fold_heads: w must be float32 [n, wdim]')
        n, wdim = w.shape
        cout0, cin = w0.shape[0], w0.shape[1]
        cout1 = w1.shape[0]
        for t in (a0, b0, w0, a1, b1, w1):
            _require(t.is_cuda and t.dtype == torch.float32 and t.is_contiguous(), 'fold_heads: contiguous float32 CUDA tensors required')
            _require(t.device == w.device, 'fold_heads: all tensors must reside on the same device as w')
        out = torch.empty([n, cout0 + cout1, cin, 1, 1], dtype=torch.float32, device=w.device)
        with _dev_guard(w.device):
            rc = load().ide3d_fold_heads(_ptr(w), w.stride(0), n, cin, wdim, float(affine_gain), _ptr(a0), _ptr(b0), _ptr(w0), cout0, float(gain0),
                                         _ptr(a1), _ptr(b1), _ptr(w1), cout1, float(gain1), _ptr(out), _stream(w))
        _check(rc, 'fold_heads')
        return out

    @staticmethod
    def style_demod_batch(jobs):
        """All modulated layers of a pass in two launches.  jobs: [(w, affine_w, affine_b, affine_gain, bias_gain, wsq_t or None)]
        with w [n, wdim] (unit inner stride) -> [(styles [n, cin], dcoefs [n, cout] or None)], views of two buffers.  Same per-layer
        code as `style_demod`: bit-identical.  Returns None when the batch form does not apply (n > 8, > STYLE_BATCH_MAX layers handled
        by chunking)."""
        if not jobs:
            return []
        w0 = jobs[0][0]
        n, wdim = w0.shape
        if n > 8:
            return None
        dev = w0.device
        tot_s = sum(j[1].shape[0] for j in jobs)
        tot_d = sum(j[5].shape[1] for j in jobs if j[5] is not None)
        sbuf = torch.empty([n * tot_s], dtype=torch.float32, device=dev)
        dbuf = torch.empty([max(n * tot_d, 1)], dtype=torch.float32, device=dev)
        arr = (_StyleJob * len(jobs))()
        outs, so, do = [], 0, 0
        for k, (w, aw, ab, again, bgain, wsq_t) in enumerate(jobs):
            _require(w.is_cuda and w.dtype == torch.float32 and w.ndim == 2 and w.stride(1) == 1 and tuple(w.shape) == (n, wdim) and w.device == dev,
                     'style_demod_batch: every w must be float32 [n, wdim] with unit inner stride on one device')
            cin = aw.shape[0]
            _require(aw.is_contiguous() and aw.shape[1] == wdim and aw.dtype == torch.float32 and aw.device == dev, 'style_demod_batch: affine weight must be contiguous float32 [cin, wdim]')
            _require(ab is None or (ab.is_contiguous() and ab.numel() == cin and ab.device == dev), 'style_demod_batch: affine bias must be contiguous [cin]')
            styles = sbuf[so:so + n * cin].view(n, cin); so += n * cin
            dco, cout = None, 0
            if wsq_t is not None:
                _require(wsq_t.is_contiguous() and wsq_t.shape[0] == cin and wsq_t.device == dev, 'style_demod_batch: wsq_t must be contiguous [cin, cout]')
                cout = wsq_t.shape[1]
                dco = dbuf[do:do + n * cout].view(n, cout); do += n * cout
            j = arr[k]
            j.w, j.w_stride = w.data_ptr(), w.stride(0)
            j.affine_w, j.affine_b = aw.data_ptr(), (ab.data_ptr() if ab is not None else None)
            j.wsq_t = wsq_t.data_ptr() if wsq_t is not None else None
            j.cin, j.cout, j.affine_gain, j.bias_gain = cin, cout, float(again), float(bgain)
            j.styles, j.dcoefs = styles.data_ptr(), (dco.data_ptr() if dco is not None else None)
            outs.append((styles, dco))
        lib = load()
        with _dev_guard(dev):
            for k0 in range(0, len(jobs), STYLE_BATCH_MAX):
                cnt = min(STYLE_BATCH_MAX, len(jobs) - k0)
                rc = lib.ide3d_style_demod_batch(ctypes.cast(ctypes.byref(arr, k0 * ctypes.sizeof(_StyleJob)), ctypes.POINTER(_StyleJob)),
                                                 cnt, n, wdim, _stream(w0))
                _check(rc, 'style_demod_batch')
        return outs

    @staticmethod
    def fold_heads_batch(jobs):
        """All dual heads of a pass in one launch.  jobs: [(w, affine_gain, a0, b0, w0, gain0, a1, b1, w1, gain1)] (arguments of
        `fold_heads`) -> [out [n, cout0 + cout1, cin, 1, 1]], views of one buffer; bit-identical to `fold_heads`."""
        if not jobs:
            return []
        w_0 = jobs[0][0]
        n, wdim = w_0.shape
        dev = w_0.device
        sizes = [(j[4].shape[0] + j[8].shape[0]) * j[4].shape[1] for j in jobs]
        buf = torch.empty([n * sum(sizes)], dtype=torch.float32, device=dev)
        arr = (_FoldJob * len(jobs))()
        outs, off = [], 0
        for k, (w, again, a0, b0, w0, g0, a1, b1, w1, g1) in enumerate(jobs):
            _require(w.is_cuda and w.dtype == torch.float32 and w.ndim == 2 and w.stride(1) == 1 and tuple(w.shape) == (n, wdim) and w.device == dev,
                     'fold_heads_batch: every w must be float32 [n, wdim] with unit inner stride on one device')
            for t in (a0, b0, w0, a1, b1, w1):
                _require(t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and t.device == dev, 'fold_heads_batch: contiguous float32 CUDA tensors required')
            cout0, cin = w0.shape[0], w0.shape[1]
            cout1 = w1.shape[0]
            _require(w1.shape[1] == cin and a0.shape == (cin, wdim) and a1.shape == (cin, wdim), 'fold_heads_batch: head shapes do not agree')
            out = buf[off:off + n * sizes[k]].view(n, cout0 + cout1, cin, 1, 1); off += n * sizes[k]
            j = arr[k]
            j.w, j.w_stride, j.cin, j.affine_gain = w.data_ptr(), w.stride(0), cin, float(again)
            j.a0, j.b0, j.w0, j.cout0, j.gain0 = a0.data_ptr(), b0.data_ptr(), w0.data_ptr(), cout0, float(g0)
            j.a1, j.b1, j.w1, j.cout1, j.gain1 = a1.data_ptr(), b1.data_ptr(), w1.data_ptr(), cout1, float(g1)
            j.out = out.data_ptr()
            outs.append(out)
        lib = load()
        with _dev_guard(dev):
            for k0 in range(0, len(jobs), STYLE_BATCH_MAX):
                cnt = min(STYLE_BATCH_MAX, len(jobs) - k0)
                rc = lib.ide3d_fold_heads_batch(ctypes.cast(ctypes.byref(arr, k0 * ctypes.sizeof(_FoldJob)), ctypes.POINTER(_FoldJob)),
                                                cnt, n, wdim, _stream(w_0))
                _check(rc, 'fold_heads_batch')
        return outs


class FramePlugin:
    @staticmethod
    def frame_u8(img, seg, palette, out=None):
        img, seg = img.contiguous(), seg.contiguous()
        _require(img.is_cuda and img.dtype == torch.float32 and seg.dtype == torch.float32, 'frame_u8: float32 CUDA tensors required')
        n, _, H, W = img.shape
        classes = seg.shape[1]
        _require(palette.dtype == torch.uint8 and palette.shape == (classes, 3) and palette.is_cuda, 'palette must be uint8 [classes, 3] on GPU')
        if out is None:
            out = torch.empty([n, H, 2 * W, 3], dtype=torch.uint8, device=img.device)
        _require(out.dtype == torch.uint8 and tuple(out.shape) == (n, H, 2 * W, 3) and out.is_contiguous() and out.device == img.device,
                 'frame_u8: out must be a contiguous uint8 [N, H, 2W, 3] tensor on the image device')
        with _dev_guard(img.device):
            rc = load().ide3d_frame_u8(_ptr(img), _ptr(seg), _ptr(palette.contiguous()), n, classes, H, W, _ptr(out), _stream(img))
        _check(rc, 'frame_u8')
        return out


class CameraPlugin:
    """The pose helpers of training/volumetric_rendering.py as two launches (csrc/camera.hip)."""

    @staticmethod
    def applies(*tensors):
        """float32 CUDA tensors outside autograd (the drivers' poses; a differentiable pose keeps the tensor operations)."""
        return all(torch.is_tensor(t) and t.is_cuda and t.dtype == torch.float32 and not t.requires_grad for t in tensors)

    @staticmethod
    def sphere_points(theta, pitch, r, pitch_is_v=False):
        """theta, pitch [n, 1] -> (pos [n, 3], phi [n, 1]) (include/ide3d_hip.h: ide3d_sphere_points)."""
        _require(theta.is_cuda and theta.dtype == torch.float32 and pitch.dtype == torch.float32 and pitch.device == theta.device and theta.numel() == pitch.numel(),
                 'sphere_points: float32 CUDA tensors of one size required')
        theta, pitch = theta.contiguous(), pitch.contiguous()
        n = theta.numel()
        pos = torch.empty([n, 3], dtype=torch.float32, device=theta.device)
        phi = torch.empty_like(pitch)
        with _dev_guard(theta.device):
            rc = load().ide3d_sphere_points(_ptr(theta), _ptr(pitch), n, float(r), int(bool(pitch_is_v)), _ptr(pos), _ptr(phi), _stream(theta))
        _check(rc, 'sphere_points')
        return pos, phi

    @staticmethod
    def cam2world(forward, origin, lookat=None):
        """forward [n, 3] | None, origin [n, 3], lookat [3] / [1, 3] / [n, 3] | None -> [n, 4, 4] (ide3d_cam2world)."""
        _require(origin.is_cuda and origin.dtype == torch.float32 and origin.ndim == 2 and origin.shape[1] == 3, 'cam2world: origin must be float32 [n, 3] on a CUDA device')
        origin = origin.contiguous()
        n = origin.shape[0]
        stride = 0
        if lookat is not None:
            _require(lookat.dtype == torch.float32 and lookat.device == origin.device and lookat.numel() in (3, 3 * n), 'cam2world: lookat must hold 3 or 3 n float32 values on the same device')
            lookat = lookat.contiguous()
            stride = 3 if (lookat.numel() == 3 * n and n > 1) else 0
        else:
            _require(forward is not None and forward.dtype == torch.float32 and forward.device == origin.device and tuple(forward.shape) == (n, 3),
                     'cam2world: forward must be float32 [n, 3] on the same device')
            forward = forward.contiguous()
        out = torch.empty([n, 4, 4], dtype=torch.float32, device=origin.device)
        with _dev_guard(origin.device):
            rc = load().ide3d_cam2world(_ptr(forward if lookat is None else None), _ptr(origin), _ptr(lookat), stride, n, _ptr(out), _stream(origin))
        _check(rc, 'cam2world')
        return out


class MappingPlugin:
    MAX_N, MAX_WIDTH, MAX_LAYERS = 8, 1024, 16
    _ws = _Workspaces()          # (device index, launch domain) -> per-layer activations + barrier counter (zero-filled once); see workspace_scope

    @staticmethod
    def supports(n, z_dim, embed, widths, device=None):
        """`device`: the device the launch will run on (the residency answer is per device; None = the current one)."""
        k0 = z_dim + embed
        if not (1 <= n <= MappingPlugin.MAX_N and 0 < k0 <= MappingPlugin.MAX_WIDTH and k0 % 4 == 0 and 1 <= len(widths) <= MappingPlugin.MAX_LAYERS
                and all(0 < w <= MappingPlugin.MAX_WIDTH and w % 4 == 0 for w in widths)):
            return False
        with _dev_guard(device):                              # None: no-op guard
            return bool(load().ide3d_mapping_supported())            # the kernel's grid barrier needs its 64 workgroups co-resident

    @staticmethod
    def mapping(z, c, embed_w, embed_b, embed_wgain, embed_bgain, fc_ws, fc_bs, lr_multiplier, alpha, act_gain, num_ws, w_avg, psi, cutoff, trusted=False):
        """z [n, z_dim], c [n, c_dim] | None, raw parameters of the embed / fc layers -> ws [n, num_ws, w_dim] (one launch).
        `cutoff` has the meaning it has in `MappingNetwork._truncate`'s `ws[:, :cutoff]`, a Python slice: None truncates every row, a value
        k >= 0 the first min(k, num_ws) rows, a negative value the first max(num_ws + k, 0) rows (truncation applies where psi != 1 only).
        `trusted`: the caller has passed these very parameter objects (and this batch size) through the checks before; only z / c are checked."""
        dev = z.device
        if trusted:
            _require(z.is_cuda and z.dtype == torch.float32 and z.is_contiguous() and (c is None or (c.device == dev and c.dtype == torch.float32 and c.is_contiguous()
                                                                                                 and tuple(c.shape) == (z.shape[0], embed_w.shape[1]))),
                     'mapping: z / c must be contiguous float32 tensors on one CUDA device, c [n, c_dim]')
            return MappingPlugin._launch(z, c, embed_w, embed_b, embed_wgain, embed_bgain, fc_ws, fc_bs, lr_multiplier, alpha, act_gain, num_ws, w_avg, psi, cutoff)
        f32c = lambda t: t is None or (t.is_cuda and t.device == dev and t.dtype == torch.float32 and t.is_contiguous())
        _require(all(f32c(t) for t in (z, c, embed_w, embed_b, w_avg, *fc_ws, *fc_bs)), 'mapping: contiguous float32 tensors on one CUDA device required')
        n, z_dim = z.shape
        embed = 0 if embed_w is None else embed_w.shape[0]
        _require(MappingPlugin.supports(n, z_dim, embed, [w.shape[0] for w in fc_ws], device=dev), 'mapping: unsupported shape')
        # the kernel indexes c as [n, c_dim] and w_avg as [w_dim]: a smaller conditioning batch (torch.cat would raise in the
        # reference, networks.py:302) or a short w_avg must not become an out-of-bounds read
        _require((embed_w is None) or (c is not None and embed_w.ndim == 2 and tuple(c.shape) == (n, embed_w.shape[1])),
                 f'mapping: c must be [{n}, {None if embed_w is None else embed_w.shape[1]}] (got {None if c is None else tuple(c.shape)})')
        _require(embed_b is None or (embed_w is not None and tuple(embed_b.shape) == (embed,)), 'mapping: embed bias must be [embed]')
        _require(w_avg is None or w_avg.numel() == fc_ws[-1].shape[0], 'mapping: w_avg must have w_dim elements')
        _require(num_ws >= 1, 'mapping: num_ws must be positive')
        k = z_dim + embed
        for w, b in zip(fc_ws, fc_bs):
            _require(w.ndim == 2 and w.shape[1] == k and (b is None or tuple(b.shape) == (w.shape[0],)), 'mapping: layer widths do not chain')
            k = w.shape[0]
        return MappingPlugin._launch(z, c, embed_w, embed_b, embed_wgain, embed_bgain, fc_ws, fc_bs, lr_multiplier, alpha, act_gain, num_ws, w_avg, psi, cutoff)

    @staticmethod
    def _launch(z, c, embed_w, embed_b, embed_wgain, embed_bgain, fc_ws, fc_bs, lr_multiplier, alpha, act_gain, num_ws, w_avg, psi, cutoff):
        dev = z.device
        n, z_dim = z.shape
        embed = 0 if embed_w is None else embed_w.shape[0]
        k = fc_ws[-1].shape[0]
        lib = load()
        wsp = MappingPlugin._ws.entry((dev.index, _ws_domain(dev)), lambda: torch.zeros([lib.ide3d_mapping_workspace_bytes() // 4 + 4], dtype=torch.float32, device=dev))[0]
        out = torch.empty([n, num_ws, k], dtype=torch.float32, device=dev)
        p = _MappingParams()
        p.z, p.c = z.data_ptr(), (c.data_ptr() if c is not None else 0)
        p.embed_w, p.embed_b = (embed_w.data_ptr() if embed_w is not None else 0), (embed_b.data_ptr() if embed_b is not None else 0)
        for i, (w, b) in enumerate(zip(fc_ws, fc_bs)):
            p.fc_w[i], p.fc_b[i], p.fc_out[i] = w.data_ptr(), (b.data_ptr() if b is not None else 0), w.shape[0]
        p.w_avg = w_avg.data_ptr() if w_avg is not None else 0
        p.ws, p.workspace, p.workspace_bytes = out.data_ptr(), wsp.data_ptr(), wsp.numel() * 4
        p.n, p.z_dim, p.c_dim, p.embed, p.layers, p.num_ws = n, z_dim, (c.shape[1] if c is not None else 0), embed, len(fc_ws), num_ws
        p.embed_weight_gain, p.embed_bias_gain, p.lr_multiplier = float(embed_wgain), float(embed_bgain), float(lr_multiplier)
        p.alpha, p.act_gain, p.truncation_psi = float(alpha), float(act_gain), float(psi)
        # `ws[:, :cutoff]` is a Python slice: a negative cut-off counts from the end.  The ABI reads every negative value as "all rows".
        p.truncation_cutoff = -1 if cutoff is None else (int(cutoff) if cutoff >= 0 else max(num_ws + int(cutoff), 0))
        with _dev_guard(dev):
            rc = lib.ide3d_mapping(ctypes.byref(p), _stream(z))
        _check(rc, 'mapping')
        return out


class _PlaneGate(ctypes.Structure):
    """ide3d_plane_gate"""
    _fields_ = [('cells', ctypes.c_void_p), ('cells_h', ctypes.c_int32), ('cells_w', ctypes.c_int32),
                ('tile_list', ctypes.c_void_p), ('tile_h', ctypes.c_int32), ('tile_w', ctypes.c_int32)]


def _plane_gate(gate, n, h, w):
    """The C struct of a needed-cell map [n, 3, ceil(h / 4), ceil(w / 4)] (uint8, contiguous) for an h x w output.  `gate`: the map, or
    (map, plane_tile_list's output, (tile_h, tile_w))."""
    cells, tiles, tile_hw = gate if isinstance(gate, tuple) else (gate, None, None)
    _require(cells.is_cuda and cells.dtype == torch.uint8 and cells.is_contiguous() and tuple(cells.shape) == (n, 3, (h + 3) // 4, (w + 3) // 4),
             f'plane gate: cells must be a contiguous uint8 CUDA tensor [{n}, 3, {(h + 3) // 4}, {(w + 3) // 4}], got {list(cells.shape)} {cells.dtype}')
    g = _PlaneGate()
    g.cells, g.cells_h, g.cells_w = cells.data_ptr(), cells.shape[2], cells.shape[3]
    if tiles is not None:
        th, tw = tile_hw
        _require(tiles.is_cuda and tiles.dtype == torch.int32 and tiles.is_contiguous() and tiles.device == cells.device
                 and tiles.numel() == 1 + n * (-(-h // th)) * (-(-w // tw)), 'plane gate: the tile list must be plane_tile_list(cells, h, w, tile_h, tile_w)')
        g.tile_list, g.tile_h, g.tile_w = tiles.data_ptr(), th, tw
    return g


def plane_tile_list(cells, h, w, tile_h, tile_w):
    """int32 [1 + n * tiles]: the number of tile_h x tile_w tiles of an h x w output with a set cell of `cells` under them, then their indices
    (ide3d_plane_tile_list).  Handed to a gated launch with that tile size beside the map, it spreads the live tiles evenly over the device."""
    n = cells.shape[0]
    g = _plane_gate(cells, n, h, w)
    out = torch.empty([1 + n * (-(-h // tile_h)) * (-(-w // tile_w))], dtype=torch.int32, device=cells.device)
    with _dev_guard(cells.device):
        rc = load().ide3d_plane_tile_list(ctypes.byref(g), n, int(h), int(w), int(tile_h), int(tile_w), _ptr(out), _stream(cells))
    _check(rc, 'plane_tile_list')
    return out


def plane_cells(rays_d_cam, z_lin, cam2world, H, W):
    """The needed-cell map of an H x W tri-plane for the cameras `cam2world` [n, 4, 4] of a render with the camera-space ray directions
    `rays_d_cam` [R, 3] and the depth ramp `z_lin` [S] (the fused renderer's own arguments) -> uint8 [n, 3, ceil(H / 4), ceil(W / 4)]: 1 where a
    sample can address a texel of the 4 x 4 cell, whatever the jitter draw (ide3d_plane_cells, csrc/camera.hip)."""
    for t in (rays_d_cam, z_lin, cam2world):
        _require(t.is_cuda and t.dtype == torch.float32 and t.is_contiguous(), 'plane_cells: contiguous float32 CUDA tensors required')
    _require(rays_d_cam.ndim == 2 and rays_d_cam.shape[1] == 3 and z_lin.ndim == 1 and cam2world.ndim == 3 and tuple(cam2world.shape[1:]) == (4, 4),
             'plane_cells: rays_d_cam [R, 3], z_lin [S], cam2world [n, 4, 4]')
    n = cam2world.shape[0]
    cells = torch.empty([n, 3, (H + 3) // 4, (W + 3) // 4], dtype=torch.uint8, device=cam2world.device)
    with _dev_guard(cells.device):
        rc = load().ide3d_plane_cells(_ptr(rays_d_cam), _ptr(z_lin), _ptr(cam2world), n, rays_d_cam.shape[0], z_lin.shape[0], int(H), int(W),
                                      _ptr(cells), _stream(cells))
    _check(rc, 'plane_cells')
    return cells


class ResamplePlugin:
    @staticmethod
    def skip_upsample_add_cl(lo, add, gate=None, out=None):
        """upsample2d(lo, [1,3,3,1]) + add -> [n, c, 2h, 2w] in channels_last memory format (lo / add: any strides).  `gate` (plane_cells' map
        [n, 3, ceil(2h / 4), ceil(2w / 4)], c a multiple of 96): only the 8 x 32 tiles with a set cell of their own plane under them are
        written (ide3d_skip_upsample_add_cl_gated).  `out`: the channels_last tensor to write into instead of a fresh one."""
        _require(lo.is_cuda and lo.dtype == torch.float32 and add.dtype == torch.float32 and add.device == lo.device,
                 'skip_upsample_add_cl: float32 CUDA tensors on one device required')
        n, c, h, w = lo.shape
        _require(tuple(add.shape) == (n, c, 2 * h, 2 * w), 'skip_upsample_add_cl: add must be [n, c, 2h, 2w]')
        _require(c % 4 == 0, 'skip_upsample_add_cl: channel count must be a multiple of 4')
        if out is None:
            out = torch.empty([n, c, 2 * h, 2 * w], dtype=torch.float32, device=lo.device, memory_format=torch.channels_last)
        _require(out.dtype == torch.float32 and out.device == lo.device and tuple(out.shape) == (n, c, 2 * h, 2 * w)
                 and out.is_contiguous(memory_format=torch.channels_last), 'skip_upsample_add_cl: out must be a channels_last float32 [n, c, 2h, 2w] tensor')
        with _dev_guard(lo.device):
            if gate is not None:
                rc = load().ide3d_skip_upsample_add_cl_gated(_ptr(lo), ctypes.byref(_i64x4(lo.stride())), _ptr(add), ctypes.byref(_i64x4(add.stride())),
                                                             n, c, h, w, _ptr(out), ctypes.byref(_plane_gate(gate, n, 2 * h, 2 * w)), _stream(lo))
            else:
                rc = load().ide3d_skip_upsample_add_cl(_ptr(lo), ctypes.byref(_i64x4(lo.stride())), _ptr(add), ctypes.byref(_i64x4(add.stride())),
                                                       n, c, h, w, _ptr(out), _stream(lo))
        _check(rc, 'skip_upsample_add_cl')
        return out

    @staticmethod
    def bilinear_up2_split(x, ranges, adjacent=None):
        """x [n, c, h, w] -> one [n, count, 2h, 2w] tensor per (begin, count) in `ranges` (at most 3), bilinear, align_corners=False.
        `adjacent=(i, j)`: outputs i and j = i + 1 are the two channel ranges of ONE [n, count_i + count_j, 2h, 2w] tensor (views)."""
        _require(x.is_cuda and x.dtype == torch.float32, 'bilinear_up2_split: float32 CUDA tensor required')
        _require(1 <= len(ranges) <= 3, 'bilinear_up2_split: one to three channel ranges')
        x = x.contiguous()
        n, c, h, w = x.shape
        outs = [None if (adjacent and k in adjacent) else torch.empty([n, cnt, 2 * h, 2 * w], dtype=torch.float32, device=x.device) for k, (_b, cnt) in enumerate(ranges)]
        bs = [0, 0, 0]
        if adjacent:
            i, j = adjacent
            _require(j == i + 1 and 0 <= i and j < len(ranges), 'bilinear_up2_split: adjacent outputs must be consecutive')
            ci, cj = ranges[i][1], ranges[j][1]
            both = torch.empty([n, ci + cj, 2 * h, 2 * w], dtype=torch.float32, device=x.device)
            outs[i], outs[j] = both[:, :ci], both[:, ci:]
            bs[i] = bs[j] = (ci + cj) * 4 * h * w
        dst = (ctypes.c_void_p * 3)(*([o.data_ptr() for o in outs] + [0] * (3 - len(outs))))
        bsa = (ctypes.c_int64 * 3)(*bs)
        beg = (ctypes.c_int32 * 3)(*([int(b) for b, _c in ranges] + [0] * (3 - len(outs))))
        cnt = (ctypes.c_int32 * 3)(*([int(c_) for _b, c_ in ranges] + [0] * (3 - len(outs))))
        with _dev_guard(x.device):
            rc = load().ide3d_bilinear_up2_split(_ptr(x), n, c, h, w, ctypes.byref(dst), ctypes.byref(beg), ctypes.byref(cnt), ctypes.byref(bsa), _stream(x))
        _check(rc, 'bilinear_up2_split')
        return outs


class LowresPlugin:
    """The low-resolution block group of the backbone in one launch (csrc/lowres.hip, include/ide3d_hip.h `ide3d_lowres_group`)."""
    _ws = _Workspaces(limit=64)          # buffers zero-filled once: the halo slots of the activation images are never written

    @staticmethod
    def layers_supported(n, C, res0, ups, arith=0):
        arr = (ctypes.c_int32 * len(ups))(*[int(u) for u in ups])
        return int(load().ide3d_lowres_layers_supported(int(n), int(C), int(res0), arr, len(ups), int(arith)))

    @staticmethod
    def phase_r_plan(n, C, res0, ups, arith=0):
        """[(row bands, LDS scratch bytes of the largest band)] of phase R for each layer the group accepts (host only)"""
        arr = (ctypes.c_int32 * len(ups))(*[int(u) for u in ups])
        bands, scratch = (ctypes.c_int32 * len(ups))(), (ctypes.c_int64 * len(ups))()
        fit = int(load().ide3d_lowres_phase_r_plan(int(n), int(C), int(res0), arr, len(ups), int(arith), bands, scratch))
        return [(int(bands[l]), int(scratch[l])) for l in range(fit)]

    @staticmethod
    def group(x0, layers, heads, fir, arith=0):
        """x0 [C, r, r] (shared by the batch) or [n, C, r, r]; layers: dicts(weight [C, C, 3, 3], styles [n, C], dcoefs [n, C], noise [res, res] | None
        (x noise_strength already), bias [C] | None, act_gain, clamp (< 0: none), up (1 | 2), head (index | -1)); heads: dicts(w [n, O, C], bias [O] |
        None, clamp).  Returns (x_out [n, C, res, res], [skip_k [n, O, res_k, res_k]])."""
        lib = load()
        n, C = layers[0]['styles'].shape
        dev = x0.device
        _require(1 <= len(layers) <= LOWRES_MAX_LAYERS and len(heads) <= LOWRES_MAX_HEADS, 'lowres_group: too many layers / heads')
        _require(x0.is_cuda and x0.dtype == torch.float32 and x0.is_contiguous() and x0.shape[-3] == C and x0.shape[-1] == x0.shape[-2], 'lowres_group: x0 must be contiguous float32 [C, r, r] or [n, C, r, r]')
        _require(fir.is_cuda and fir.dtype == torch.float32 and fir.is_contiguous() and tuple(fir.shape) == (4, 4) and fir.device == dev, 'lowres_group: fir must be a float32 [4, 4] filter on the device of x0')
        arith = int(arith) or int(lib.ide3d_get_conv_arithmetic())
        p = _LowresParams()
        p.x0, p.x0_batch_stride = x0.data_ptr(), (x0.stride(0) if x0.ndim == 4 else 0)
        p.fir = fir.data_ptr()
        p.n, p.C, p.res0, p.nlayers, p.nheads, p.arith = n, C, x0.shape[-1], len(layers), len(heads), arith
        keep, res, head_res = [], x0.shape[-1], {}
        for l, L in enumerate(layers):
            q = p.layers[l]
            w = L['weight']
            _require(w.is_cuda and w.dtype == torch.float32 and w.is_contiguous() and tuple(w.shape) == (C, C, 3, 3) and w.device == dev, f'lowres_group: layer {l}: weight must be contiguous float32 [C, C, 3, 3]')
            q.weight = w.data_ptr()
            res = res * 2 if int(L['up']) == 2 else res
            for name, shape in (('styles', (n, C)), ('dcoefs', (n, C)), ('noise', (res, res)), ('bias', (C,))):
                t = L.get(name)
                if t is None:
                    _require(name in ('noise', 'bias'), f'lowres_group: layer {l}: {name} is required')
                    continue
                t = t.contiguous(); keep.append(t)
                _require(t.is_cuda and t.dtype == torch.float32 and tuple(t.shape) == shape and t.device == dev, f'lowres_group: layer {l}: {name} must be float32 {shape} on the device of x0')
                setattr(q, name, t.data_ptr())
            q.act_gain, q.clamp, q.up, q.head = float(L['act_gain']), float(L['clamp']), int(L['up']), int(L.get('head', -1))
            if q.head >= 0:
                head_res[q.head] = res
        key = (tuple(L['weight'].data_ptr() for L in layers), n, C, x0.shape[-1], tuple(int(L['up']) for L in layers), dev.index, _ws_domain(dev), arith)
        def alloc():
            nbytes = lib.ide3d_lowres_workspace_bytes(ctypes.byref(p))
            _require(nbytes > 0, 'lowres_group: unsupported configuration')
            return torch.zeros([nbytes // 4 + 1], dtype=torch.float32, device=dev)
        ent = LowresPlugin._ws.entry(key, alloc)
        weights = [L['weight'] for L in layers]
        for l, packed in enumerate(LowresPlugin._ws.packed(ent, weights)):
            p.layers[l].weights_packed = int(packed)
        p.workspace, p.workspace_bytes = ent[0].data_ptr(), ent[0].numel() * 4
        skips = []
        for k, H in enumerate(heads):
            q = p.heads[k]
            w = H['w'].reshape(n, -1, C)
            _require(w.is_cuda and w.dtype == torch.float32 and w.is_contiguous() and w.device == dev, f'lowres_group: head {k}: folded weights must be contiguous float32 [n, O, C]')
            _require(k in head_res, f'lowres_group: head {k} is not attached to a layer')
            O = w.shape[1]
            keep.append(w)
            q.w, q.O, q.clamp = w.data_ptr(), O, float(H['clamp'])
            b = H.get('bias')
            if b is not None:
                b = b.contiguous(); keep.append(b)
                _require(b.is_cuda and b.dtype == torch.float32 and tuple(b.shape) == (O,) and b.device == dev, f'lowres_group: head {k}: bias must be float32 [O]')
                q.bias = b.data_ptr()
            sk = torch.empty([n, O, head_res[k], head_res[k]], dtype=torch.float32, device=dev)
            q.skip = sk.data_ptr()
            skips.append(sk)
        x_out = torch.empty([n, C, res, res], dtype=torch.float32, device=dev)
        p.x_out = x_out.data_ptr()
        with _dev_guard(dev):
            rc = lib.ide3d_lowres_group(ctypes.byref(p), _stream(x0))
        _check(rc, 'lowres_group')
        LowresPlugin._ws.mark_packed(ent, weights)
        return x_out, skips


PLUGINS = {
    'mesh_plugin': MeshPlugin,
    'raster_plugin': RasterPlugin,
    'png_plugin': PngPlugin,
    'jpeg_plugin': JpegPlugin,
    'metrics_plugin': MetricsPlugin,
    'metrics_eval_plugin': MetricsEvalPlugin,
    'augment_plugin': AugmentPlugin,
    'lowres_plugin': LowresPlugin,
    'bias_act_plugin': BiasActPlugin,
    'upfirdn2d_plugin': Upfirdn2dPlugin,
    'filtered_lrelu_plugin': FilteredLReluPlugin,
    'triplane_plugin': TriplanePlugin,
    'volume_render_plugin': VolumeRenderPlugin,
    'modconv_plugin': ModconvPlugin,
    'modconv_grad_plugin': ModconvGradPlugin,
    'frame_plugin': FramePlugin,
    'camera_plugin': CameraPlugin,
    'style_plugin': StylePlugin,
    'resample_plugin': ResamplePlugin,
    'mapping_plugin': MappingPlugin,
    'lpips_plugin': LpipsPlugin,
    'lpips_alex_plugin': LpipsAlexPlugin,
    'vgg_loss_plugin': VggLossPlugin,
    'parse_loss_plugin': ParseLossPlugin,
    'id_loss_plugin': IdLossPlugin,
    'clip_loss_plugin': ClipLossPlugin,
    'adv_loss_plugin': AdvLossPlugin,
}
