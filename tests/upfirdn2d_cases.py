"""The case table of the upfirdn2d suites: tests/test_upfirdn2d_cases_cpu.py checks the table itself without a GPU (which of the thirteen
launchable forms of csrc/upfirdn2d.hip every case takes, by `hip_plugin.upfirdn2d_plan`; that the table reaches every form, instance,
staging path and both sides of every dispatch condition; that the float64 oracle and the tensor definition agree),
tests/test_gpu_upfirdn2d.py runs `Upfirdn2dPlugin.upfirdn2d_ex` on it.

A case states its inputs AND what it must take: `form` (generic / cell / tile / fir44 / fir_up2), for the tiled forms the template
`instance` (ux, uy, dx, dy, fw, fh, cx, cy), `staging` (1 = 16-byte, 0 = scalar, 2 = mixed, -1 = none), for cell `cell_u`, for generic
`c_fastest`, and the tiles per plane.  `vs = (other case, condition)` marks the declined half of a pair: this case differs from `other`
in the one thing `condition` names, and that sends it to another form.  `twin` names a case with equal values whose rows reach LDS by
the other staging path.

Inputs are seeded by shape and storage type alone (equal shapes = equal values, whatever the layout) and are non-dyadic (normal draws).
Every x (and `add`) is a view into a flat buffer, described by a layout:
  ('dense',)              contiguous
  ('pitch', P, off=0)     rows of pitch P elements, the view starts `off` elements into the row; whole rows belong to the storage
  ('tight', P)            pitch P, but the storage ends with the last element of the last row (`x_row_floats` = in_w)
  ('planes', P, extra)    pitch P, `extra` elements between two planes
  ('cl',)                 channels_last
  ('hstride', k)          every k-th row of a taller dense tensor
  ('wstride', k)          every k-th column of a wider dense tensor
  ('flatoff', off)        contiguous, `off` elements into its buffer
The gaps of a buffer hold NaN: a kernel that lets a pad column in shows it in every output that column reaches.  No view leaves its
storage.

The float64 reference and the error bound of a case (see tests/test_gpu_upfirdn2d.py for the derivation) are computed once per process
and shared (`reference`)."""

import math
import zlib

import numpy as np
import torch

DTYPES = dict(f32=torch.float32, f16=torch.float16, bf16=torch.bfloat16, f64=torch.float64)

T64 = (1, 1, 1, 1, 4, 4, 2, 4)        # 64 x 32 outputs per tile
T128 = (1, 1, 1, 1, 4, 4, 4, 4)       # 128 x 32
TUP2 = (2, 2, 1, 1, 4, 4, 2, 2)       # 64 x 16 cells = 128 x 32 outputs
TDN2 = (1, 1, 2, 2, 4, 4, 4, 2)       # 128 x 16
X_UP = (2, 1, 1, 1, 12, 1, 2, 4)      # 64 cells = 128 outputs x 32 rows
X_DN = (1, 1, 2, 1, 12, 1, 4, 4)      # 128 x 32
X_1 = (1, 1, 1, 1, 12, 1, 4, 4)       # 128 x 32
Y_UP = (1, 2, 1, 1, 1, 12, 4, 2)      # 128 x 16 cells = 32 output rows
Y_DN = (1, 1, 1, 2, 1, 12, 4, 2)      # 128 x 16
Y_1 = (1, 1, 1, 1, 1, 12, 4, 4)       # 128 x 32
TILE_INSTANCES = (T64, T128, TUP2, TDN2, X_UP, X_DN, X_1, Y_UP, Y_DN, Y_1)

A44 = torch.tensor([[1., 2., 3., 4.], [0.5, 3., 3., 1.], [2., 3., 5., 1.], [1., 3., 3., 7.]]) / 40      # asymmetric: a flipped or swapped tap shows
A12 = torch.tensor([0.7, -1.9, 2.3, 4.1, -3.3, 5.9, 6.1, -2.7, 3.7, 1.3, -0.9, 0.3]) / 11                 # asymmetric, no zero tap

SQRT2 = math.sqrt(2.0)
E_ADD = dict(add=('dense',))
E_NOISE = dict(noise=0, strength=0.37)
E_LIN = dict(bias=True, act=1)
E_LRELU = dict(noise=0, strength=0.37, bias=True, act=3, alpha=0.2, act_gain=SQRT2, clamp=1.5)          # the fmaxf form, clamp on
E_LRELU_NC = dict(noise=0, strength=0.7, bias=True, act=3, alpha=0.2, act_gain=SQRT2)                    # clamp off
E_ALPHA0 = dict(bias=True, act=3, alpha=0.0, act_gain=1.25)
E_ALPHA1 = dict(bias=True, act=3, alpha=1.0, act_gain=1.0, clamp=0.9)
E_SEL15 = dict(bias=True, act=3, alpha=1.5, act_gain=1.0)                                                  # the select form
E_SELNEG = dict(noise=0, strength=0.37, bias=True, act=3, alpha=-0.2, act_gain=1.3, clamp=0.8)
E_ALL = dict(add=('dense',), noise=0, strength=0.3, bias=True, act=3, alpha=0.2, act_gain=1.4, clamp=1.1)


def amax(e=None):
    return dict(e or {}, amax=True)


class Case:
    def __init__(self, name, dtype, shape, layout, filt, up, down, pad, form, instance=None, staging=-1, tiles=(0, 0), cell_u=0, c_fastest=0,
                 flip=False, gain=1.0, epi=None, vs=None, twin=None, why=''):
        self.name, self.dtype, self.shape, self.layout, self.filt = name, dtype, tuple(shape), tuple(layout), filt
        self.up, self.down = (up if isinstance(up, tuple) else (up, up)), (down if isinstance(down, tuple) else (down, down))      # (x, y)
        self.pad, self.flip, self.gain, self.epi = tuple(pad), flip, float(gain), dict(epi or {})
        self.form, self.instance, self.staging, self.tiles, self.cell_u, self.c_fastest = form, instance, staging, tuple(tiles), cell_u, c_fastest
        self.vs, self.twin, self.why = vs, twin, why
        self._init = dict(name=name, dtype=dtype, shape=shape, layout=layout, filt=filt, up=up, down=down, pad=pad, form=form, instance=instance, staging=staging,
                          tiles=tiles, cell_u=cell_u, c_fastest=c_fastest, flip=flip, gain=gain, epi=epi, vs=vs, twin=twin, why=why)

    def replace(self, **kw):
        """A case outside the table that differs from this one in the given constructor arguments."""
        return Case(**dict(self._init, **kw))

    # ---- what a case is, as plain values (the coverage checks compare cases field by field) ----
    def fields(self):
        return dict(dtype=self.dtype, shape=self.shape, layout=self.layout, filt=self.filt if not torch.is_tensor(self.filt) else 'tensor', up=self.up,
                    down=self.down, pad=self.pad, flip=self.flip, gain=self.gain, epi=tuple(sorted((k, str(v)) for k, v in self.epi.items())))

    @property
    def torch_dtype(self):
        return DTYPES[self.dtype]

    def filter(self):
        f = self.filt
        if f is None:
            return torch.ones(1, 1)          # what torch_utils.ops.upfirdn2d passes for f = None
        if isinstance(f, str):
            return dict(a44=A44, a12x=A12[None, :], a12y=A12[:, None])[f].clone()
        fh, fw = f
        g = torch.Generator().manual_seed(1000 + 97 * fh + fw)
        return torch.randn(fh, fw, generator=g) / (fh * fw) ** 0.5

    @property
    def out_shape(self):
        n, c, h, w = self.shape
        fh, fw = self.filter().shape
        px0, px1, py0, py1 = self.pad
        return (n, c, (h * self.up[1] + py0 + py1 - fh + self.down[1]) // self.down[1], (w * self.up[0] + px0 + px1 - fw + self.down[0]) // self.down[0])

    def call_args(self):
        """upx, upy, downx, downy, padx0, padx1, pady0, pady1, flip, gain of Upfirdn2dPlugin.upfirdn2d_ex / hip_plugin.upfirdn2d_plan."""
        return (self.up[0], self.up[1], self.down[0], self.down[1]) + self.pad + (self.flip, self.gain)

    def values(self, what='x'):
        """The dense values of an operand on the CPU, in the storage type (x, add, bias) or float32 (noise)."""
        shape = dict(x=self.shape, add=self.out_shape, noise=self.out_shape[2:], bias=(self.shape[1],))[what]
        g = torch.Generator().manual_seed(zlib.crc32(repr((what, shape, self.dtype)).encode()))
        v = torch.randn(*shape, generator=g)
        return v if what == 'noise' else v.to(self.torch_dtype)

    def tensors(self, device='cpu'):
        """The operands of the call as they are passed: dict(x, f, add, noise, bias) (absent operands None)."""
        out = dict(x=strided(self.values('x'), self.layout, device), f=self.filter().to(device), add=None, noise=None, bias=None)
        e = self.epi
        if 'add' in e:
            out['add'] = strided(self.values('add'), e['add'], device)
        if 'noise' in e:          # [out_h, out_w] float32, contiguous, `noise` floats into its buffer (the binding keeps a contiguous float32 view)
            out['noise'] = strided(self.values('noise')[None, None], ('flatoff', e['noise']), device)[0, 0]
        if e.get('bias'):
            out['bias'] = self.values('bias').to(device)
        return out

    def epilogue_kwargs(self, ts, y_amax=None):
        e = self.epi
        kw = {}
        if ts['add'] is not None:
            kw['add'] = ts['add']
        if ts['noise'] is not None:
            kw.update(noise=ts['noise'], noise_strength=e['strength'])
        if 'act' in e:
            kw.update(bias=ts['bias'], act=e['act'], alpha=e.get('alpha', 0.0), act_gain=e.get('act_gain', 1.0), clamp=e.get('clamp', -1.0))
        if y_amax is not None:
            kw['y_amax'] = y_amax
        return kw

    def plan_kwargs(self, ts):
        e = self.epi
        return dict(add=ts['add'], noise=ts['noise'], bias=ts['bias'] is not None, act=e.get('act'), alpha=e.get('alpha', 0.0), act_gain=e.get('act_gain', 1.0),
                    clamp=e.get('clamp', -1.0), y_amax=bool(e.get('amax')))

    def stated_plan(self):
        return dict(form=self.form, instance=self.instance, staging=self.staging, cell_u=self.cell_u, c_fastest=self.c_fastest, tiles=self.tiles)

    def __repr__(self):
        return self.name


def layout_of(layout, shape):
    """-> (strides, storage offset, storage elements) of a view of `shape`."""
    n, c, h, w = shape
    kind = layout[0]
    off, tail = 0, 0
    if kind == 'dense':
        st = (c * h * w, h * w, w, 1)
    elif kind == 'pitch':
        p = layout[1]
        off = layout[2] if len(layout) > 2 else 0
        st, tail = (c * h * p, h * p, p, 1), p - off - w
        assert tail >= 0
    elif kind == 'tight':
        p = layout[1]
        st = (c * h * p, h * p, p, 1)
    elif kind == 'planes':
        p, extra = layout[1], layout[2]
        st, tail = (c * (h * p + extra), h * p + extra, p, 1), p - w
    elif kind == 'cl':
        st = (h * w * c, 1, w * c, c)
    elif kind == 'hstride':
        k = layout[1]
        hh = k * (h - 1) + 1
        st = (c * hh * w, hh * w, k * w, 1)
    elif kind == 'wstride':
        k = layout[1]
        ww = k * (w - 1) + 1
        st = (c * h * ww, h * ww, ww, k)
    elif kind == 'flatoff':
        st, off = (c * h * w, h * w, w, 1), layout[1]
    else:
        raise ValueError(layout)
    numel = off + sum((s - 1) * t for s, t in zip(shape, st)) + 1 + tail
    return st, off, numel


def strided(values, layout, device='cpu'):
    """`values` (dense, CPU) as a view of the given layout on `device`; the rest of the buffer holds NaN."""
    st, off, numel = layout_of(layout, values.shape)
    buf = torch.full((numel,), float('nan'), dtype=values.dtype)
    buf.as_strided(values.shape, st, off).copy_(values)
    return buf.to(device).as_strided(values.shape, st, off)


# ---- the table --------------------------------------------------------------------------------------------------------------------------

CASES = []


def C(*a, **kw):
    c = Case(*a, **kw)
    assert all(c.name != o.name for o in CASES), c.name
    CASES.append(c)
    return c


P1, P21 = (1, 1, 1, 1), (2, 1, 2, 1)

# -- tile 1/1 4x4, the 64-wide instance: out_w in {1, 3, 63, 64}, out_h in {1, 32, 33} --
C('t64_1x1', 'f32', (1, 1, 2, 2), ('dense',), 'a44', 1, 1, P1, 'tile', T64, 0, (1, 1), why='a 1 x 1 output; in_w = 2 < 4: scalar staging')
C('t64_w3_h32', 'f32', (1, 7, 33, 4), ('dense',), 'a44', 1, 1, P1, 'tile', T64, 1, (1, 1), gain=4, why='out 32 x 3, one full tile row; 7 workgroups')
C('t64_w63_h33', 'f32', (1, 4, 34, 64), ('dense',), 'a44', 1, 1, P1, 'tile', T64, 1, (1, 2), gain=4, epi=amax(E_LRELU), why='two tile rows, the second one row high; 8 workgroups')
C('t64_w64_h32', 'f32', (3, 3, 32, 63), ('dense',), 'a44', 1, 1, (2, 2, 2, 1), 'tile', T64, 0, (1, 1), flip=True, epi=E_ADD, why='the widest 64-wide case; odd pitch: scalar; 9 workgroups')
C('t64_h1', 'f32', (1, 13, 4, 5), ('dense',), 'a44', 1, 1, (1, 1, 0, 0), 'tile', T64, 0, (1, 1), epi=amax(), why='out_h = 1; 13 workgroups')
C('t64_f16', 'f16', (2, 2, 33, 40), ('dense',), 'a44', 1, 1, P1, 'tile', T64, 0, (1, 1), gain=4, epi=E_ALL, why='fp16 storage')
C('t64_bf16', 'bf16', (2, 2, 33, 40), ('dense',), 'a44', 1, 1, P1, 'tile', T64, 0, (1, 1), gain=4, epi=E_LRELU_NC, why='bf16 storage')
C('t64_w41_padded', 'f32', (1, 2, 9, 41), ('pitch', 44), 'a44', 1, 1, P21, 'tile', T64, 1, (1, 1), twin='t64_w41_dense', why='in_w % 4 = 1 in padded rows: 16-byte staging')
C('t64_w41_dense', 'f32', (1, 2, 9, 41), ('dense',), 'a44', 1, 1, P21, 'tile', T64, 0, (1, 1), why='the same values from a pitch of 41: scalar staging')

# -- fir44 and, where it declines, the 128-wide instance --
C('f44_base', 'f32', (1, 2, 32, 129), ('pitch', 132), 'a44', 1, 1, P1, 'fir44', T128, 1, (1, 1), gain=4, twin='t128_pitch129', why='out 31 x 128: one ragged tile; in_w % 4 = 1 in padded rows')
C('t128_f16', 'f16', (1, 2, 32, 129), ('pitch', 132), 'a44', 1, 1, P1, 'tile', T128, 0, (1, 1), gain=4, vs=('f44_base', 'dtype'))
C('gen_wstride', 'f32', (1, 2, 32, 129), ('wstride', 2), 'a44', 1, 1, P1, 'generic', gain=4, vs=('f44_base', 'x_stride[3] != 1'), why='a W-strided view')
C('t128_add', 'f32', (1, 2, 32, 129), ('pitch', 132), 'a44', 1, 1, P1, 'tile', T128, 1, (1, 1), gain=4, epi=E_ADD, vs=('f44_base', 'add'), why='16-byte add rows')
C('t64_narrow', 'f32', (1, 2, 32, 65), ('pitch', 132), 'a44', 1, 1, P1, 'tile', T64, 1, (1, 1), gain=4, vs=('f44_base', 'out_w <= 64'))
C('t128_w127_h31', 'f32', (1, 2, 32, 128), ('pitch', 132), 'a44', 1, 1, P1, 'tile', T128, 1, (1, 1), gain=4, vs=('f44_base', 'out_w % 4'), why='odd out_w')
C('t128_pitch129', 'f32', (1, 2, 32, 129), ('dense',), 'a44', 1, 1, P1, 'tile', T128, 0, (1, 1), gain=4, vs=('f44_base', 'pitch % 4'), why='a dense row pitch that is no multiple of 4')
C('t128_tight', 'f32', (1, 2, 32, 129), ('tight', 132), 'a44', 1, 1, P1, 'tile', T128, 0, (1, 1), gain=4, vs=('f44_base', 'x_row_floats'), why='the storage ends with the last row: its quad is not readable')
C('t128_rows_off', 'f32', (1, 2, 32, 129), ('pitch', 132, 1), 'a44', 1, 1, P1, 'tile', T128, 0, (1, 1), gain=4, vs=('f44_base', 'x alignment'), why='a view whose rows start off the 16-byte grid')
C('t128_planes_off', 'f32', (1, 2, 32, 129), ('planes', 132, 2), 'a44', 1, 1, P1, 'tile', T128, 2, (1, 1), gain=4, vs=('f44_base', 'x plane stride % 4'),
  why='the one mixed case: plane 0 stages by 16 bytes, plane 1 (8 bytes off the grid) by scalar loads')
C('f44_noise', 'f32', (1, 2, 32, 129), ('pitch', 132), 'a44', 1, 1, P1, 'fir44', T128, 1, (1, 1), gain=4, epi=amax(E_NOISE))
C('t128_noise_off', 'f32', (1, 2, 32, 129), ('pitch', 132), 'a44', 1, 1, P1, 'tile', T128, 1, (1, 1), gain=4, epi=amax(dict(E_NOISE, noise=1)), vs=('f44_noise', 'noise alignment'),
  why='a misaligned noise pointer: the scalar noise branch of epilogue_row')
C('f44_lin', 'f32', (1, 2, 32, 129), ('pitch', 132), 'a44', 1, 1, P1, 'fir44', T128, 1, (1, 1), gain=4, epi=E_LIN, why='bias + linear')
C('f44_lrelu', 'f32', (1, 2, 32, 129), ('pitch', 132), 'a44', 1, 1, P1, 'fir44', T128, 1, (1, 1), gain=4, flip=True, epi=amax(E_LRELU), why='lrelu by fmaxf, clamp on')
C('f44_lrelu_nc', 'f32', (1, 2, 32, 129), ('pitch', 132), 'a44', 1, 1, P1, 'fir44', T128, 1, (1, 1), gain=4, epi=E_LRELU_NC, why='clamp off')
C('f44_alpha0', 'f32', (1, 2, 32, 129), ('pitch', 132), 'a44', 1, 1, P1, 'fir44', T128, 1, (1, 1), gain=4, epi=E_ALPHA0, why='alpha = 0: the lower edge of the fmaxf form')
C('f44_alpha1', 'f32', (1, 2, 32, 129), ('pitch', 132), 'a44', 1, 1, P1, 'fir44', T128, 1, (1, 1), gain=4, epi=E_ALPHA1, why='alpha = 1: the upper edge')
C('f44_sel15', 'f32', (1, 2, 32, 129), ('pitch', 132), 'a44', 1, 1, P1, 'fir44', T128, 1, (1, 1), gain=4, epi=amax(E_SEL15), why='alpha 1.5: the select form')
C('f44_selneg', 'f32', (1, 2, 32, 129), ('pitch', 132), 'a44', 1, 1, P1, 'fir44', T128, 1, (1, 1), gain=4, epi=E_SELNEG, why='alpha -0.2: the select form, clamp on')
C('f44_w68_h1', 'f32', (1, 3, 4, 68), ('dense',), 'a44', 1, 1, (2, 1, 0, 0), 'fir44', T128, 1, (1, 1), why='out 1 x 68')
C('f44_w132_h33', 'f32', (1, 2, 33, 132), ('dense',), 'a44', 1, 1, P21, 'fir44', T128, 1, (2, 2), flip=True, epi=amax(), why='two tiles on both axes, each second one a sliver')
C('f44_w260_h32', 'f32', (1, 1, 33, 261), ('pitch', 264), 'a44', 1, 1, P1, 'fir44', T128, 1, (3, 1), gain=4, why='three tile columns, one full tile row')
C('f44_pad0330', 'f32', (1, 2, 20, 72), ('dense',), 'a44', 1, 1, (0, 3, 3, 0), 'fir44', T128, 1, (1, 1), why='pad_x0 = 0: the window starts on the 16-byte grid')
C('f44_pad1212', 'f32', (1, 2, 20, 72), ('dense',), 'a44', 1, 1, (1, 2, 1, 2), 'fir44', T128, 1, (1, 1), flip=True, gain=4, why='the pads the backward pass of pad (2, 1, 2, 1) forms: f - pad0 - 1')
C('f44_crop', 'f32', (1, 2, 20, 72), ('dense',), 'a44', 1, 1, (-1, 4, -2, 5), 'fir44', T128, 1, (1, 1), epi=amax(E_LRELU), why='cropping pads')
C('f44_far', 'f32', (1, 2, 5, 8), ('dense',), 'a44', 1, 1, (130, 1, 37, 1), 'fir44', T128, 1, (2, 2), epi=amax(E_NOISE), why='pads beyond a tile: tile row 0 and tile column 0 lie outside the image')
C('t128_far', 'f32', (1, 2, 5, 8), ('dense',), 'a44', 1, 1, (130, 2, 37, 1), 'tile', T128, 1, (2, 2), why='the same with an odd out_w')
C('f44_w130_padded', 'f32', (2, 2, 9, 130), ('pitch', 132), 'a44', 1, 1, (2, 3, 1, 1), 'fir44', T128, 1, (2, 1), why='in_w % 4 = 2 in padded rows; out_w 132')
# the 128-wide instance at its own edges: out_w in {65, 127, 128, 129, 131}, out_h in {31, 32, 33}
C('t128_w65_h33', 'f32', (1, 4, 34, 66), ('dense',), 'a44', 1, 1, P1, 'tile', T128, 0, (1, 2), gain=4, epi=amax(E_LRELU), why='first width past the 64-wide instance; 8 workgroups')
C('t128_w128_bf16', 'bf16', (1, 3, 33, 129), ('dense',), 'a44', 1, 1, P1, 'tile', T128, 0, (1, 1), gain=4, epi=E_ADD, why='one exact tile in bf16')
C('t128_w128_f16', 'f16', (1, 3, 33, 129), ('dense',), 'a44', 1, 1, P1, 'tile', T128, 0, (1, 1), gain=4, flip=True, epi=E_LRELU)
C('t128_w129_h32', 'f32', (1, 7, 33, 130), ('pitch', 132), 'a44', 1, 1, P1, 'tile', T128, 1, (2, 1), gain=4, epi=amax(E_ALL), twin='t128_w129_dense', why='in_w % 4 = 2 in padded rows; one column in tile 1')
C('t128_w129_dense', 'f32', (1, 7, 33, 130), ('dense',), 'a44', 1, 1, P1, 'tile', T128, 0, (2, 1), gain=4, epi=amax(E_ALL))
C('t128_w131_h31', 'f32', (1, 2, 32, 132), ('dense',), 'a44', 1, 1, P1, 'tile', T128, 1, (2, 1), gain=4, epi=dict(add=('pitch', 134, 1)), why='add rows off the 16-byte grid: the scalar add branch')
C('t128_w130_padded', 'f32', (1, 2, 33, 131), ('pitch', 132), 'a44', 1, 1, P1, 'tile', T128, 1, (2, 1), gain=4, twin='t128_w130_dense', why='in_w % 4 = 3 in padded rows')
C('t128_w130_dense', 'f32', (1, 2, 33, 131), ('dense',), 'a44', 1, 1, P1, 'tile', T128, 0, (2, 1), gain=4)
C('t128_inw3', 'f32', (1, 2, 6, 3), ('dense',), 'a44', 1, 1, (40, 40, 1, 1), 'tile', T128, 0, (1, 1), why='in_w < 4, scalar')
C('t128_inw3_padded', 'f32', (1, 2, 6, 3), ('pitch', 4), 'a44', 1, 1, (40, 41, 1, 1), 'tile', T128, 1, (1, 1), why='in_w < 4 in one quad per row: every 16-byte load clamps to column 0')

# -- fir_up2 and, where it declines, tile<2,2,1,1,4,4,2,2> --
for i, pad in enumerate(((2, 1, 2, 1), (2, 1, 3, 0), (0, 3, 1, 2), (4, -1, 2, 1), (-2, 5, 2, 1))):
    C(f'up2_small_p{i}', 'f32', (2, 3, 8, 8), ('dense',), 'a44', 2, 1, pad, 'fir_up2', TUP2, 1, (1, 1), gain=4, flip=bool(i & 1), epi=(E_ADD, amax(), E_ALL, amax(E_NOISE), {})[i])
    C(f'up2_wide_p{i}', 'f32', (1, 2, 17, 68), ('dense',), 'a44', 2, 1, pad, 'fir_up2', TUP2, 1, (2, 2), gain=4, flip=not (i & 1), epi=({}, E_ADD, amax(E_LRELU), {}, E_ADD)[i],
      why='two tiles in x and in y')
C('up2_base', 'f32', (1, 2, 9, 36), ('dense',), 'a44', 2, 1, P21, 'fir_up2', TUP2, 1, (1, 1), gain=4, epi=E_ADD, twin='tup2_pitch38')
C('tup2_f16', 'f16', (1, 2, 9, 36), ('dense',), 'a44', 2, 1, P21, 'tile', TUP2, 0, (1, 1), gain=4, epi=E_ADD, vs=('up2_base', 'dtype'))
C('tup2_bf16', 'bf16', (1, 2, 9, 36), ('dense',), 'a44', 2, 1, P21, 'tile', TUP2, 0, (1, 1), gain=4, epi=E_ADD, vs=('up2_base', 'dtype'))
C('gen_up2_wstride', 'f32', (1, 2, 9, 36), ('wstride', 3), 'a44', 2, 1, P21, 'generic', gain=4, epi=E_ADD, vs=('up2_base', 'x_stride[3] != 1'))
C('tup2_odd_out', 'f32', (1, 2, 9, 36), ('dense',), 'a44', 2, 1, (2, 2, 2, 1), 'tile', TUP2, 1, (1, 1), gain=4, epi=E_ADD, vs=('up2_base', 'out_w % 4'))
C('tup2_inw33', 'f32', (1, 2, 9, 33), ('dense',), 'a44', 2, 1, P21, 'tile', TUP2, 0, (1, 1), gain=4, epi=E_ADD, vs=('up2_base', 'in_w % 4'), why='input width 33')
C('tup2_inw65', 'f32', (1, 2, 5, 65), ('pitch', 68), 'a44', 2, 1, P21, 'tile', TUP2, 1, (2, 1), gain=4, epi=amax(E_ALL), twin='tup2_inw65_dense', why='input width 65 in padded rows: two tiles in x')
C('tup2_inw65_dense', 'f32', (1, 2, 5, 65), ('dense',), 'a44', 2, 1, P21, 'tile', TUP2, 0, (2, 1), gain=4, epi=amax(E_ALL))
C('tup2_odd_pad', 'f32', (1, 2, 9, 36), ('dense',), 'a44', 2, 1, (3, 0, 2, 1), 'tile', TUP2, 1, (1, 1), gain=4, epi=E_ADD, vs=('up2_base', 'pad_x0 odd'))
C('tup2_pitch38', 'f32', (1, 2, 9, 36), ('pitch', 38), 'a44', 2, 1, P21, 'tile', TUP2, 0, (1, 1), gain=4, epi=E_ADD, vs=('up2_base', 'pitch % 4'))
C('tup2_rows_off', 'f32', (1, 2, 9, 36), ('pitch', 40, 3), 'a44', 2, 1, P21, 'tile', TUP2, 0, (1, 1), gain=4, epi=E_ADD, vs=('up2_base', 'x alignment'))
C('tup2_planes_off', 'f32', (1, 2, 9, 36), ('planes', 36, 4 * 9 + 1), 'a44', 2, 1, P21, 'tile', TUP2, 2, (1, 1), gain=4, epi=E_ADD, vs=('up2_base', 'x plane stride % 4'))
C('tup2_add_off', 'f32', (1, 2, 9, 36), ('dense',), 'a44', 2, 1, P21, 'tile', TUP2, 1, (1, 1), gain=4, epi=dict(add=('pitch', 76, 1)), vs=('up2_base', 'add alignment'),
  why='an add view whose rows are not 16-byte aligned')
C('tup2_add_pitch', 'f32', (1, 2, 9, 36), ('dense',), 'a44', 2, 1, P21, 'tile', TUP2, 1, (1, 1), gain=4, epi=dict(add=('pitch', 74)), vs=('up2_base', 'add pitch % 4'))
C('tup2_add_planes', 'f32', (1, 2, 9, 36), ('dense',), 'a44', 2, 1, P21, 'tile', TUP2, 1, (1, 1), gain=4, epi=dict(add=('planes', 72, 2)), vs=('up2_base', 'add plane stride % 4'))
C('tup2_add_wstride', 'f32', (1, 2, 9, 36), ('dense',), 'a44', 2, 1, P21, 'tile', TUP2, 1, (1, 1), gain=4, epi=dict(add=('wstride', 2)), vs=('up2_base', 'add_stride[3] != 1'))
C('up2_noise', 'f32', (1, 2, 9, 36), ('dense',), 'a44', 2, 1, P21, 'fir_up2', TUP2, 1, (1, 1), gain=4, epi=E_NOISE)
C('tup2_noise_off', 'f32', (1, 2, 9, 36), ('dense',), 'a44', 2, 1, P21, 'tile', TUP2, 1, (1, 1), gain=4, epi=dict(E_NOISE, noise=3), vs=('up2_noise', 'noise alignment'))
C('up2_sel15', 'f32', (1, 2, 9, 36), ('dense',), 'a44', 2, 1, P21, 'fir_up2', TUP2, 1, (1, 1), gain=4, epi=amax(E_SEL15))
C('up2_lin', 'f32', (1, 2, 9, 36), ('dense',), 'a44', 2, 1, P21, 'fir_up2', TUP2, 1, (1, 1), gain=4, epi=E_LIN)
C('tup2_odd_pads', 'f32', (1, 4, 35, 19), ('dense',), 'a44', 2, 1, (3, 0, 1, 2), 'tile', TUP2, 0, (1, 3), gain=1, why='odd pads: shifted polyphase cells; three tile rows')

# -- tile down 2: 128 x 16 outputs per tile --
C('dn2_two_tiles', 'f32', (1, 2, 34, 258), ('dense',), 'a44', 1, 2, P1, 'tile', TDN2, 0, (2, 2), twin='dn2_two_tiles_padded', why='out 17 x 129: one row and one column in the second tiles')
C('dn2_two_tiles_padded', 'f32', (1, 2, 34, 258), ('pitch', 260), 'a44', 1, 2, P1, 'tile', TDN2, 1, (2, 2), why='in_w % 4 = 2 in padded rows')
C('dn2_odd', 'f32', (1, 3, 35, 67), ('dense',), 'a44', 1, 2, P1, 'tile', TDN2, 0, (1, 2), flip=True, epi=E_LRELU, why='odd input sizes')
C('dn2_pad0220', 'f32', (1, 2, 21, 64), ('dense',), 'a44', 1, 2, (0, 2, 2, 0), 'tile', TDN2, 1, (1, 1), epi=E_ADD)
C('dn2_crop', 'f32', (2, 2, 25, 72), ('dense',), 'a44', 1, 2, (-1, 3, -2, 2), 'tile', TDN2, 1, (1, 1), gain=2, why='cropping pads')
C('dn2_f16', 'f16', (1, 2, 34, 258), ('dense',), 'a44', 1, 2, P1, 'tile', TDN2, 0, (2, 2), epi=E_ALL)
C('dn2_bf16', 'bf16', (1, 3, 33, 67), ('dense',), 'a44', 1, 2, (0, 2, 2, 0), 'tile', TDN2, 0, (1, 1))

# -- the six 12-tap instances, fp32, called directly with [1, 12] and [12, 1] filters --
#    pads of the augmentation's sym6 calls: up 2 (6, 5) with gain 2 per axis, down 2 (-1, -1), unit rate (6, 5); one odd and one cropping pad each
for tag, filt, inst, up, down, small, large, tiles_large in (
        ('x_up', 'a12x', X_UP, (2, 1), (1, 1), (2, 2, 5, 9), (1, 2, 33, 66), (2, 2)),
        ('x_dn', 'a12x', X_DN, (1, 1), (2, 1), (2, 2, 5, 40), (1, 2, 33, 270), (2, 2)),
        ('x_1', 'a12x', X_1, (1, 1), (1, 1), (2, 2, 5, 21), (1, 2, 33, 130), (2, 2)),
        ('y_up', 'a12y', Y_UP, (1, 2), (1, 1), (2, 2, 9, 5), (1, 2, 17, 129), (2, 2)),
        ('y_dn', 'a12y', Y_DN, (1, 1), (1, 2), (2, 2, 40, 5), (1, 2, 46, 129), (2, 2)),
        ('y_1', 'a12y', Y_1, (1, 1), (1, 1), (2, 2, 21, 5), (1, 2, 33, 129), (2, 2))):
    along_x = filt == 'a12x'
    pads = dict(x_up=((6, 5), (5, 6), (-2, 13)), x_dn=((-1, -1), (5, 6), (-3, 2)), x_1=((6, 5), (5, 6), (-1, 13)))[tag.replace('y_', 'x_')]
    full = lambda q: (q[0], q[1], 0, 0) if along_x else (0, 0, q[0], q[1])
    g = 2.0 if 'up' in tag else 1.0
    C(f'{tag}_small', 'f32', small, ('dense',), filt, up, down, full(pads[0]), 'tile', inst, 1 if small[3] % 4 == 0 else 0, (1, 1), gain=g, why='one tile, the sym6 pads')
    C(f'{tag}_large', 'f32', large, ('dense',), filt, up, down, full(pads[0]), 'tile', inst, 1 if large[3] % 4 == 0 else 0, tiles_large, gain=g, flip=True, epi=E_LRELU,
      twin=f'{tag}_large_other', why='two tiles on both axes')
    other = ('pitch', (large[3] + 7) & ~3) if large[3] % 4 else ('pitch', large[3] + 1)
    C(f'{tag}_large_other', 'f32', large, other, filt, up, down, full(pads[0]), 'tile', inst, 0 if large[3] % 4 == 0 else 1, tiles_large, gain=g, flip=True, epi=E_LRELU,
      why='the same values through the other staging path')
    C(f'{tag}_odd_pad', 'f32', large, ('dense',), filt, up, down, full(pads[1]), 'tile', inst, 1 if large[3] % 4 == 0 else 0, tiles_large, gain=g, epi=E_ADD, why='an odd leading pad')
    C(f'{tag}_crop', 'f32', small, ('pitch', (small[3] + 7) & ~3), filt, up, down, full(pads[2]), 'tile', inst, 1, (1, 1), gain=g, epi=E_NOISE, why='a cropping pad; padded rows')
C('gen_12tap_f16', 'f16', (2, 2, 5, 9), ('dense',), 'a12x', (2, 1), 1, (6, 5, 0, 0), 'generic', gain=2, vs=('x_up_small', 'dtype'), why='the 12-tap instances are fp32 only')
C('gen_12tap_y_bf16', 'bf16', (2, 2, 9, 5), ('dense',), 'a12y', (1, 2), 1, (0, 0, 6, 5), 'generic', gain=2, vs=('y_up_small', 'dtype'))

# -- one tiny single-tile case per tiled form with 7, 8, 9 and 13 workgroups: xcd_remap off and on the multiples of 8 --
_XCD = (('t64', 'a44', (5, 6), 1, 1, P1, 'tile', T64), ('t128', 'a44', (5, 70), 1, 1, P1, 'tile', T128), ('tup2', 'a44', (5, 6), 2, 1, P21, 'tile', TUP2),
        ('tdn2', 'a44', (9, 10), 1, 2, P1, 'tile', TDN2), ('f44', 'a44', (5, 68), 1, 1, P21, 'fir44', T128), ('up2', 'a44', (5, 8), 2, 1, P21, 'fir_up2', TUP2),
        ('x_up', 'a12x', (3, 7), (2, 1), 1, (6, 5, 0, 0), 'tile', X_UP), ('x_dn', 'a12x', (3, 30), 1, (2, 1), (-1, -1, 0, 0), 'tile', X_DN),
        ('x_1', 'a12x', (3, 9), 1, 1, (6, 5, 0, 0), 'tile', X_1), ('y_up', 'a12y', (7, 3), (1, 2), 1, (0, 0, 6, 5), 'tile', Y_UP),
        ('y_dn', 'a12y', (30, 3), 1, (1, 2), (0, 0, -1, -1), 'tile', Y_DN), ('y_1', 'a12y', (9, 3), 1, 1, (0, 0, 6, 5), 'tile', Y_1))
for tag, filt, hw, up, down, pad, form, inst in _XCD:
    for n, c in ((1, 7), (2, 4), (3, 3), (1, 13)):
        C(f'xcd_{tag}_{n * c}', 'f32', (n, c) + hw, ('dense',), filt, up, down, pad, form, inst, 1 if hw[1] % 4 == 0 else 0, (1, 1), epi=amax() if filt == 'a44' and n * c == 9 else None,
          why=f'{n * c} workgroups')

# -- cell, U = 2 and 4 (the shapes of tests/test_gpu_ops.py::test_upfirdn2d_cell_kernel_equals_generic, the images cut down) --
C('cell_47_u4', 'f32', (1, 3, 20, 24), ('dense',), (47, 47), 4, 1, (25, 22, 25, 22), 'cell', cell_u=4, tiles=(25, 21), gain=16, why='upsample2d(f47, up = 4): the viewer')
C('cell_12_u2', 'f32', (2, 5, 37, 29), ('dense',), (12, 12), 2, 1, (6, 5, 6, 5), 'cell', cell_u=2, tiles=(29, 37), gain=4)
C('gen_up24', 'f32', (2, 5, 37, 29), ('dense',), (12, 12), (2, 4), 1, (6, 5, 6, 5), 'generic', gain=4, vs=('cell_12_u2', 'up_x != up_y'))
C('gen_up3_12', 'f32', (2, 5, 37, 29), ('dense',), (12, 12), 3, 1, (6, 5, 6, 5), 'generic', gain=4, vs=('cell_12_u2', 'up not 2 or 4'), why='up 3')
C('gen_up2_dn2', 'f32', (2, 5, 37, 29), ('dense',), (12, 12), 2, 2, (6, 5, 6, 5), 'generic', gain=4, vs=('cell_12_u2', 'down != 1'), why='up 2 and down 2 together')
C('gen_12_amax', 'f32', (2, 5, 37, 29), ('dense',), (12, 12), 2, 1, (6, 5, 6, 5), 'generic', gain=4, epi=amax(), vs=('cell_12_u2', 'y_amax'))
C('cell_9x7_u2', 'f32', (1, 4, 33, 50), ('dense',), (9, 7), 2, 1, (3, 4, 1, 7), 'cell', cell_u=2, tiles=(51, 34), flip=True, why='odd filter sizes')
C('cell_8x16_u4', 'f32', (2, 2, 40, 24), ('dense',), (8, 16), 4, 1, (-3, 9, 11, -2), 'cell', cell_u=4, tiles=(23, 41), gain=2.5, why='negative pads crop')
C('cell_6_u4', 'f32', (1, 3, 16, 16), ('dense',), (6, 6), 4, 1, (0, 0, 0, 0), 'cell', cell_u=4, tiles=(15, 15), why='f_w f_h = 36: the smallest filter')
C('cell_6x7_u2', 'f32', (1, 2, 9, 11), ('dense',), (6, 7), 2, 1, (3, 3, 2, 3), 'cell', cell_u=2, tiles=(12, 9), why='f_w no multiple of U, f_h one')
C('cell_9x8_u4', 'f16', (1, 2, 9, 11), ('dense',), (9, 8), 4, 1, (4, 3, 5, 3), 'cell', cell_u=4, tiles=(11, 10), gain=4, epi=E_ALL, why='f_h no multiple of U, f_w one; fp16')
C('cell_4x9_u2', 'f32', (1, 2, 9, 11), ('dense',), (4, 9), 2, 1, (4, 4, 2, 1), 'cell', cell_u=2, tiles=(11, 9), why='36 taps')
C('gen_5x7_u2', 'f32', (1, 2, 9, 11), ('dense',), (5, 7), 2, 1, (3, 3, 2, 2), 'generic', why='35 taps: below the cell form', vs=('cell_6x7_u2', 'taps < 36'))
C('cell_lds_edge', 'f32', (1, 1, 12, 12), ('dense',), (92, 100), 4, 1, (50, 50, 46, 46), 'cell', cell_u=4, tiles=(13, 13), why='128 x 96 floats of padded filter: 49 152 bytes, the limit')
C('gen_lds_over', 'f32', (1, 1, 12, 12), ('dense',), (93, 100), 4, 1, (50, 50, 46, 47), 'generic', vs=('cell_lds_edge', 'LDS'), why='one filter row more: 51 200 bytes')
C('cell_second_trip', 'f32', (1, 1, 512, 512), ('dense',), (6, 6), 2, 1, (3, 2, 3, 2), 'cell', cell_u=2, tiles=(513, 513), gain=4, why='513 * 2 * 513 cell rows > 2048 * 256')
C('cell_cl', 'f32', (2, 5, 13, 11), ('cl',), (10, 10), 2, 1, (5, 4, 5, 4), 'cell', cell_u=2, tiles=(12, 14), gain=4, epi=E_ALL, why='channels_last, the scalar apply_epilogue')
C('cell_bf16', 'bf16', (2, 4, 20, 20), ('dense',), (10, 10), 2, 1, (5, 4, 5, 4), 'cell', cell_u=2, tiles=(21, 21), gain=4, epi=E_ALL)

# -- generic --
C('gen_up23', 'f32', (2, 3, 9, 11), ('dense',), 'a44', (2, 3), 1, (2, 1, 3, 2), 'generic', gain=6, why='up = (2, 3)')
C('gen_dn32', 'f32', (2, 3, 19, 14), ('dense',), 'a44', 1, (3, 2), (2, 1, 1, 2), 'generic', why='down = (3, 2)')
C('gen_up2_dn2_44', 'f32', (1, 3, 9, 11), ('dense',), 'a44', 2, 2, (2, 1, 2, 1), 'generic', gain=4, epi=E_ALL, why='up 2 and down 2 together')
C('gen_up3', 'f32', (1, 2, 7, 6), ('dense',), (5, 5), 3, 1, (3, 2, 4, 1), 'generic', gain=9, epi=E_ADD, why='factor 3')
C('gen_5x5', 'f32', (1, 2, 21, 30), ('dense',), (5, 5), 1, 1, (2, 2, 2, 2), 'generic', gain=4, epi=E_LRELU)
C('gen_3x7', 'f16', (2, 2, 11, 13), ('dense',), (3, 7), 1, 2, (3, 3, 1, 1), 'generic', flip=True, epi=E_SELNEG, why='fp16')
C('gen_3x7_bf16', 'bf16', (2, 2, 11, 13), ('dense',), (3, 7), 2, 1, (3, 4, 1, 2), 'generic', gain=4, epi=E_ADD)
C('gen_fnone', 'f32', (2, 3, 5, 7), ('dense',), None, 2, 1, (0, 1, 0, 1), 'generic', gain=3, why='f = None: the 1 x 1 filter')
C('tup2_cl_c1', 'f32', (3, 1, 8, 9), ('cl',), 'a44', 2, 1, P21, 'tile', TUP2, 0, (1, 1), gain=4, why='c = 1 in channels_last is w-contiguous: the tile form takes it')
C('gen_cl_c1_5x5', 'f32', (3, 1, 8, 9), ('cl',), (5, 5), 1, 1, (2, 2, 2, 2), 'generic', c_fastest=0, why='c = 1 in channels_last: lanes along w')
C('gen_cl_c2', 'f32', (2, 2, 8, 9), ('cl',), 'a44', 2, 1, P21, 'generic', c_fastest=1, gain=4, epi=E_ALL)
C('gen_cl_c5', 'f16', (2, 5, 8, 9), ('cl',), 'a44', 1, 1, P1, 'generic', c_fastest=1, gain=4, epi=E_LRELU)
C('gen_hstride', 'f32', (1, 2, 9, 12), ('hstride', 2), (5, 5), 1, 1, (2, 2, 2, 2), 'generic', why='an H-strided view')
C('tile_hstride', 'f32', (1, 2, 17, 36), ('hstride', 2), 'a44', 1, 1, P1, 'tile', T64, 1, (1, 1), why='an H-strided view stays w-contiguous: tile, pitch 72')
C('gen_wstride3', 'f32', (1, 2, 9, 12), ('wstride', 3), (5, 5), 2, 1, (3, 2, 3, 2), 'generic', gain=4, why='a W-strided view')
C('gen_f64', 'f64', (2, 3, 20, 22), ('dense',), 'a44', 2, 1, P21, 'generic', gain=4, epi=dict(add=('dense',), bias=True, act=3, alpha=0.2, act_gain=1.5, clamp=2.0), why='float64 never tiles')
C('gen_f64_12', 'f64', (1, 2, 9, 8), ('cl',), (12, 12), 2, 1, (6, 5, 6, 5), 'generic', c_fastest=1, gain=4, why='float64 never takes the cell form')
C('gen_second_trip', 'f32', (1, 2, 513, 515), ('dense',), (3, 3), 1, 1, (1, 1, 1, 1), 'generic', why='528 390 outputs > 2048 * 256: a second grid-stride trip')
C('gen_amax_n64', 'f32', (64, 1, 5, 6), ('dense',), (5, 5), 1, 1, (2, 2, 2, 2), 'generic', epi=amax(E_LRELU_NC), why='y_amax through LDS: n = 64')
C('gen_amax_n65', 'f32', (65, 1, 5, 6), ('dense',), (5, 5), 1, 1, (2, 2, 2, 2), 'generic', epi=amax(E_LRELU_NC), why='y_amax without LDS: n = 65')
C('gen_amax_n65_big', 'f32', (65, 2, 40, 50), ('dense',), (3, 3), 1, 1, (1, 1, 1, 1), 'generic', epi=amax(), why='n = 65 with lanes that cross images')

BY_NAME = {c.name: c for c in CASES}
LEAN_CASES = [c for c in CASES if c.form in ('fir44', 'fir_up2')]
CELL_CASES = [c for c in CASES if c.form == 'cell']
AMAX_CASES = [c for c in CASES if c.epi.get('amax')]
TWINS = [(c, BY_NAME[c.twin]) for c in CASES if c.twin]


# ---- the float64 reference and the bound ------------------------------------------------------------------------------------------------

EPS = dict(f32=2.0 ** -24, f16=2.0 ** -24, bf16=2.0 ** -24, f64=2.0 ** -53)        # unit roundoff of the accumulation (float for fp16 / bf16 storage)
STORE = dict(f32=0.0, f16=2.0 ** -11, bf16=2.0 ** -8, f64=0.0)                      # one rounding to the storage type
SUBNORMAL = dict(f32=0.0, f16=2.0 ** -25, bf16=0.0, f64=0.0)                        # half the fp16 subnormal step

_REF = {}


def f32(v):
    return float(np.float32(v))


def reference(case):
    """-> dict(y: float64 reference of the finished output, tol: its per-element bound, fir / tol_fir: the FIR alone and its bound in the
    accumulation type, k: roundings counted).  Computed once."""
    if case.name in _REF:
        return _REF[case.name]
    from oracle import ops as oracle_ops
    x, f = case.values('x').double(), case.filter()
    kw = dict(up=case.up, down=case.down, padding=list(case.pad), flip_filter=case.flip)
    fir = oracle_ops.upfirdn2d(x, f, gain=case.gain, **kw)
    a = oracle_ops.upfirdn2d(x.abs(), f.abs(), gain=abs(case.gain), **kw)
    fh, fw = f.shape
    k = -(-fh // case.up[1]) * -(-fw // case.up[0]) + 3
    tol_fir = k * EPS[case.dtype] * a          # the plain FIR in the accumulation type, before any storage rounding
    e = case.epi
    v, scale = fir.clone(), 1.0
    if 'add' in e:
        add = case.values('add').double()
        v, a, k = v + add, a + add.abs(), k + 1
    if 'noise' in e:
        nz = case.values('noise').double() * f32(e['strength'])
        v, a, k = v + nz, a + nz.abs(), k + 2
    if 'act' in e:
        if e.get('bias'):
            b = case.values('bias').double()[None, :, None, None]
            v, a, k = v + b, a + b.abs(), k + 1
        if e['act'] == 3:
            alpha = f32(e.get('alpha', 0.0))
            v, k, scale = torch.where(v > 0, v, v * alpha), k + 1, max(1.0, abs(alpha))
        g = f32(e.get('act_gain', 1.0))
        v, k, scale = v * g, k + 1, scale * abs(g)
        cl = f32(e.get('clamp', -1.0))
        if cl >= 0:
            v = v.clamp(-cl, cl)
    tol = k * EPS[case.dtype] * a * scale
    tol = tol * (1 + STORE[case.dtype]) + STORE[case.dtype] * v.abs() + SUBNORMAL[case.dtype]
    _REF[case.name] = dict(y=v, tol=tol, fir=fir, tol_fir=tol_fir, k=k)
    return _REF[case.name]


def worst_ratio(y, case):
    """max |y - ref| / bound over all elements (0 / 0 counts as 0; a NaN or an infinity in y counts as infinitely wrong)."""
    r = reference(case)
    err = (y.detach().cpu().double() - r['y']).abs()
    ratio = torch.where(err == 0, torch.zeros_like(err), err / r['tol'].clamp_min(1e-300))
    return float(torch.nan_to_num(ratio, nan=float('inf')).max())
