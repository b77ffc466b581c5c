"""Small frames for the JPEG tests (tests/test_jpeg_cpu.py, tests/test_gpu_jpeg.py): name -> (uint8 frame [H, W, C], quality, subsampling,
restart interval in MCUs or None for the default).  Each is there for one thing, said beside it; test_jpeg_cpu.py checks that it does it."""
import numpy as np


def realistic(h, w, c, seed):
    """Smooth fields + a hard-edged patch + sigma = 3 noise."""
    rng = np.random.RandomState(seed)
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    f = np.stack([128 + 90 * np.sin(x / 23.0 + 0.3 * ch) * np.cos(y / 17.0 - 0.2 * ch) + 0.25 * (x - y) * (ch - 1) for ch in range(c)], axis=-1)
    f[h // 4:h // 2, w // 3:2 * w // 3] = np.array([235, 20, 60][:c])
    return np.clip(f + 3.0 * rng.randn(h, w, c) + 0.5, 0, 255).astype(np.uint8)


def _noise(h, w, c, seed):
    return np.random.RandomState(seed).randint(0, 256, size=[h, w, c]).astype(np.uint8)


def _block_pattern(values):
    """Grey frame of one row of 8 x 8 blocks, block k filled with values[k]."""
    return np.concatenate([np.full([8, 8, 1], v, np.uint8) for v in values], axis=1)


def _basis77(amplitude):
    k = np.cos((2 * np.arange(8) + 1) * 7 * np.pi / 16)
    block = np.rint(128 + amplitude * np.outer(k, k)).astype(np.uint8)
    return np.tile(block, (2, 2))[..., None]


_checker = (((np.arange(16)[:, None] + np.arange(24)[None, :]) & 1) * 255).astype(np.uint8)

CASES = {
    # padding on both axes
    '1x1x3': (np.array([[[200, 30, 90]]], np.uint8), 90, '4:4:4', None),
    '8x8x1': (realistic(8, 8, 1, 1), 90, '4:4:4', None),
    '7x9x3': (realistic(7, 9, 3, 2), 90, '4:4:4', None),
    # exactly one 16 x 16 MCU; odd chroma sides
    '16x16x3': (realistic(16, 16, 3, 3), 90, '4:2:0', None),
    '17x33x3': (realistic(17, 33, 3, 4), 85, '4:2:0', None),
    # constant colour: DC-0 + EOB only after an interval's first MCU, intervals end mid-byte and are padded with 1-bits
    'flat': (np.tile(np.array([[[90, 160, 40]]], np.uint8), (32, 40, 1)), 75, '4:4:4', 3),
    # blocks alternately all 0 and all 255 at quality 100: DC differences of category 11 with both signs
    'dc_swing': (_block_pattern([0, 255, 0, 255, 0, 255, 0, 255]), 100, '4:4:4', None),
    # +-checkerboard at quality 100: an AC coefficient of category 10
    'ac_max': (_checker[..., None], 100, '4:4:4', None),
    # a single (7, 7) basis function: three ZRLs, a non-zero 63rd coefficient, no EOB
    'zrl_no_eob': (_basis77(100.0), 50, '4:4:4', None),
    # uniform noise at quality 100: FF bytes inside the scan, the case nearest the worst-case slot
    'stuffing': (_noise(32, 40, 3, 5), 100, '4:4:4', None),
    # 12 intervals of one MCU: RSTm wraps past 7
    'restart_wrap': (realistic(96, 8, 3, 6), 90, '4:4:4', 1),
    # 3 MCUs per row, intervals of 5: they span rows and the last one is short
    'restart_ragged': (realistic(64, 48, 3, 7), 90, '4:2:0', 5),
    # intervals longer than the 32 blocks the device transforms at a time: bits carried from pass to pass (17 MCUs, then 7)
    'restart_long': (realistic(64, 96, 3, 8), 95, '4:2:0', 17),
    'one_interval': (realistic(40, 72, 3, 9), 90, '4:4:4', 65535),
    # table entries clamped at 255 and at 1
    'q1': (realistic(32, 32, 3, 10), 1, '4:2:0', None),
    'q100': (realistic(32, 32, 3, 11), 100, '4:2:0', None),
    'grey_realistic': (realistic(64, 96, 1, 12), 90, '4:4:4', None),
    'rgb_realistic': (realistic(64, 96, 3, 13), 90, '4:2:0', None),
}
