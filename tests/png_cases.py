"""The shared case list of tests/test_png_cpu.py and tests/test_gpu_png.py: name -> (uint8 frame [H, W, C], filter, segment_bytes).
All tiny; `segment_bytes` = 1024 so that small images span several segments (the length-limit case needs one 32 KiB segment)."""
import numpy as np

SEG = 1024
RUN_LENGTHS = (1, 2, 3, 4, 258, 259, 260, 261, 262, 516, 517)
FIBONACCI = (1, 2, 3, 5, 8, 13, 21, 34, 55, 89, 144, 233, 377, 610, 987, 1597, 2584, 4181, 6765, 10946)
LIMIT_STEP = 9551


def _rng(seed):
    return np.random.RandomState(seed)


def noisy_gradient(H, W, C, seed=0):
    y, x = np.mgrid[0:H, 0:W]
    base = (3 * x + 5 * y)[..., None] + 40 * np.arange(C)
    return ((base + _rng(seed).randint(-3, 4, size=[H, W, C])) & 255).astype(np.uint8)


def run_rows():
    """4 x 1023 x 1: with filter 0 every row is exactly one 1024-byte segment [0 | 1023 bytes]; the rows hold runs of exactly
    RUN_LENGTHS bytes (neighbouring runs differ, none is 0 next to the type byte), the rest of a row alternates two values."""
    rows = ((1, 2, 3, 4, 258, 259), (260, 261, 262), (516,), (517,))
    assert sorted(r for row in rows for r in row) == sorted(RUN_LENGTHS)
    out = np.zeros([4, 1023, 1], np.uint8)
    for k, runs in enumerate(rows):
        data, v = [], 1
        for L in runs:
            data += [10 + v] * L
            v += 1
        while len(data) < 1023:
            data.append(200 + (len(data) & 1))
        out[k, :, 0] = data
    return out


def length_limit_frame():
    """1 x 28654 x 1: with filter 0 the stream [0 | data] holds symbol s FIBONACCI[s] times (symbol 0 once: the type byte), the sorted
    stream dealt to positions (i * LIMIT_STEP) mod n, which leaves no run of 3.  With end-of-block's count of 1 the counts are the
    Fibonacci sequence: the unlimited Huffman depth is 20."""
    n = sum(FIBONACCI)
    assert n == 28655 and np.gcd(LIMIT_STEP, n) == 1
    stream = np.zeros([n], np.uint8)
    stream[(np.arange(n, dtype=np.int64) * LIMIT_STEP) % n] = np.repeat(np.arange(20, dtype=np.uint8), FIBONACCI)
    assert stream[0] == 0
    return stream[1:].reshape(1, n - 1, 1).copy()


def _cases():
    c = {}
    for C in (1, 3):
        c[f'1x1x{C}'] = (np.full([1, 1, C], 7, np.uint8), 'adaptive', SEG)
        c[f'1x37x{C}'] = (noisy_gradient(1, 37, C), 'adaptive', SEG)
    c['single_zero'] = (np.zeros([1, 1, 1], np.uint8), 'none', SEG)
    c['rowbytes_4k'] = (noisy_gradient(9, 64, 1, 1), 'adaptive', SEG)           # 64 = 4k
    c['rowbytes_4k+1'] = (noisy_gradient(9, 23, 3, 2), 'adaptive', SEG)         # 69
    c['rowbytes_4k+3'] = (noisy_gradient(9, 21, 3, 3), 'adaptive', SEG)         # 63... 21 * 3 = 63 = 4 * 15 + 3
    c['constant'] = (np.full([7, 500, 3], 93, np.uint8), 'none', SEG)           # one run across rows and segments (sub/up would zero it)
    c['constant_adaptive'] = (np.full([7, 500, 3], 93, np.uint8), 'adaptive', SEG)
    c['zeros'] = (np.zeros([5, 700, 1], np.uint8), 'none', SEG)                 # the type bytes join the run: one literal per segment
    c['boundary_5x1366x3'] = (np.repeat(noisy_gradient(5, 1366 // 2, 3, 4), 2, axis=1), 'adaptive', SEG)   # boundaries inside rows and runs
    c['runs'] = (run_rows(), 'none', SEG)
    c['alternating'] = (np.where((np.arange(3 * 900) & 1).reshape(3, 900, 1) == 1, 17, 91).astype(np.uint8), 'none', SEG)
    c['random'] = (_rng(5).randint(0, 256, size=[3, 700, 3]).astype(np.uint8), 'none', SEG)
    for name in ('none', 'sub', 'up', 'average', 'paeth'):
        c[f'forced_{name}'] = (noisy_gradient(6, 181, 3, 6), name, SEG)
    c['flat_labels'] = (np.repeat(np.repeat(_rng(7).randint(0, 19, size=[6, 9, 1]).astype(np.uint8) * 13, 8, axis=0), 40, axis=1)
                        .repeat(3, axis=2), 'adaptive', SEG)
    c['length_limit'] = (length_limit_frame(), 'none', 32768)
    return c


CASES = _cases()
STORED_CASES = ('random',)          # every segment must fall back to a stored block
