"""Write tests/golden/augment.npz from the reference's own AugmentPipe, on the CPU (build container only: needs the reference tree).

    python scripts/make_augment_golden.py

Holds the inputs, `forward(x, debug_percentile=p)` of the bgc configuration for every shape and percentile of tests/test_augment_cpu.py,
one filter + cutout case, and the three buffers.  The reference is imported with the stubs of oracle/ref_import.py."""

import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

SHAPES = [(2, 3, 17, 33), (2, 3, 24, 20), (2, 3, 5, 7), (2, 1, 2, 2)]
PERCENTILES = [0.1, 0.3, 0.37, 0.62, 0.9]
BGC = dict(xflip=1, rotate90=1, xint=1, scale=1, rotate=1, aniso=1, xfrac=1, brightness=1, contrast=1, lumaflip=1, hue=1, saturation=1)
FILTER_CUTOUT = dict(imgfilter=1, cutout=1)
FILTER_CUTOUT_SHAPE, FILTER_CUTOUT_PCT = (2, 3, 32, 40), 0.8


def inputs(shape, seed):
    return np.random.RandomState(seed).uniform(-1, 1, size=shape).astype(np.float32)


def main():
    from oracle import ref_import
    ref_import.install()
    import torch
    from training.augment import AugmentPipe
    assert sys.modules['training.augment'].__file__.startswith(ref_import.REFERENCE_ROOT), 'not the reference module'
    out = {}
    pipe = AugmentPipe(**BGC)
    out['p'], out['Hz_geom'], out['Hz_fbank'] = pipe.p.numpy(), pipe.Hz_geom.numpy(), pipe.Hz_fbank.numpy()
    with torch.no_grad():
        for si, shape in enumerate(SHAPES):
            x = inputs(shape, 100 + si)
            out[f'x_{si}'] = x
            for pi, pct in enumerate(PERCENTILES):
                out[f'bgc_{si}_{pi}'] = pipe(torch.from_numpy(x), debug_percentile=pct).numpy()
        x = inputs(FILTER_CUTOUT_SHAPE, 200)
        out['fc_x'] = x
        out['fc_out'] = AugmentPipe(**FILTER_CUTOUT)(torch.from_numpy(x), debug_percentile=FILTER_CUTOUT_PCT).numpy()
    path = os.path.join(ROOT, 'tests', 'golden', 'augment.npz')
    np.savez_compressed(path, **out)
    print(f'wrote {path}: {os.path.getsize(path)} bytes, {len(out)} arrays')


if __name__ == '__main__':
    main()
