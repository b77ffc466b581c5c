"""Baseline JPEG files from uint8 frames: the stills and, through `video_render.write_avi`, the Motion-JPEG video sink that stands in for
`imageio.get_writer(mp4, mode='I', fps=60, codec='libx264', bitrate='10M')` (gen_videos.py:108,131) with the compression on the device
(csrc/jpeg.hip).

The stream is defined HERE, in integers, and the HIP kernels reproduce it byte for byte (the layering of `training.png`): CUDA frames take
the kernels, CPU frames take the numpy definition below, and the two give the same files.  Baseline sequential DCT (SOF0, 8 bit), JFIF 1.01.

  input     uint8 [H, W, C], C = 1 (grey) or 3 (RGB), sides 1..65535.  The frame is padded to whole MCUs by replicating its last column and
            row (before colour conversion and subsampling, which commute with replication of whole pixels).
  colour    C = 3: full-range JFIF Y'CbCr (ITU-T T.871) in 16-bit fixed point, >> is the arithmetic (floor) shift:
              Y  = ( 19595 R + 38470 G +  7471 B + 32768) >> 16
              Cb = (-11059 R - 21709 G + 32768 B + 8421375) >> 16          8421375 = (128 << 16) + 32767: B = 255 alone gives 255, not 256
              Cr = ( 32768 R - 27439 G -  5329 B + 8421375) >> 16
            Every row of coefficients sums to 65536 (Y) or 0 (Cb, Cr); each sample is within 1 of the float64 formula rounded and lies in
            0..255 without a clamp.  C = 1: Y is the sample.
  chroma    '4:4:4': 8 x 8 MCU, blocks Y Cb Cr (grey: Y).  '4:2:0': 16 x 16 MCU, chroma = (a + b + c + d + 2) >> 2 over each 2 x 2 of the
            Cb / Cr samples, blocks Y00 Y01 Y10 Y11 Cb Cr.  MCUs in raster order.
  DCT       on s = sample - 128, int32 throughout, with the table T[u][x] = round(2^13 c(u) / 2 cos((2 x + 1) u pi / 16)), c(0) = 1/sqrt 2,
            c(u > 0) = 1 (`DCT_TABLE`; the device holds the same 64 integers):
              rows      t[y][u] = (sum_x T[u][x] s[y][x] + 512) >> 10          the 1-D transform of row y with 3 fractional bits
              columns   F8[v][u] = (sum_y T[v][y] t[y][u] + 4096) >> 13        the 2-D coefficient with 3 fractional bits
            Error bound `DCT_ERROR_BOUND` (E, in unscaled coefficient units, F8 / 8 against the real DCT), with d = max_u sum_x
            |T[u][x] / 2^13 - t(u, x)| (table rounding, at most 8 * 0.5 / 2^13) and a = max_u sum_x |t(u, x)| = 2 sqrt 2:
              rows      e1 = 128 d + 1/16                 table rounding on |s| <= 128, then rounding to 1/8
              columns   E  = d (128 a + e1) + a e1 + 1/16   table rounding on |t| <= 128 a + e1, the rows' error through the exact table,
                                                            then rounding to 1/8
            E = 0.4804 with this table (`_dct_error_bound`); the largest error seen over 22 000 random and 68 extreme blocks is 0.375
            (tests/test_jpeg_cpu.py prints it).  |sums| stay below 2^28.
  quantise  ITU-T T.81 Annex K tables scaled by the IJG rule: scale = 5000 // quality below 50, else 200 - 2 quality; entry =
            clamp((base * scale + 50) // 100, 1, 255).  k = sign(F8) * ((|F8| + 4 q) // (8 q)): F8 / 8 / q rounded half away from zero.  AC values
            are clamped to +-1023 (never reached: |AC| <= 1020 + E) so that every amplitude has a code.
  entropy   Annex K's four Huffman tables (`STD_HUFFMAN`).  Per block in zig-zag order: DC difference to the previous block of the same
            component INSIDE the restart interval (0 before the first), category = bit length of |diff| (0..11), the code of the category then
            the amplitude in `category` bits (negative: diff - 1, low bits: ones' complement); per non-zero AC coefficient after a run of
            r zeros: r >> 4 times ZRL (F0), then the code of ((r & 15) << 4 | size) and the amplitude; EOB (00) when the 63rd is zero.
            Bits MSB first.
  restart   DRI = `restart_interval` MCUs (1..65535; default `default_restart_interval`: the MCUs one workgroup of the device encodes in
            one pass, 32 // blocks per MCU = 5 / 10 / 32 for 4:2:0 / 4:4:4 RGB / grey).  It need not divide a row or the frame.  Every
            interval starts with predictors 0, is padded with 1-bits to a byte, every FF byte is followed by 00, then RSTm (FF D0+m),
            m = interval index mod 8, after every interval but the last.
  file      SOI, APP0 JFIF 1.01 (no density, 1:1), DQT luminance (and chrominance), SOF0, the four (grey: two) DHT tables, DRI, SOS,
            the scan, EOI: added on the host by `jpeg_container`.  The standard tables are written out, so a decoder needs no defaults.

Worst case (`worst_case_bytes`): a block is at most 20 bits of DC (9-bit code + 11) and 63 x 26 bits of AC (16-bit code + 10) = 1658 bits;
an interval of b blocks at most 2 ceil(1658 b / 8) bytes (every byte FF and stuffed) plus 2 for RSTm.

Not here: progressive and arithmetic coding, 12-bit samples, 4:2:2, per-frame optimised Huffman tables, rate control, alpha, EXIF, H.264.
"""

import struct

import numpy as np
import torch

from training.stream_io import streams_to_host, write_files

SUBSAMPLINGS = {'4:4:4': 444, '4:2:0': 420}          # the C ABI's codes
MAX_SIDE = 65535
BLOCK_BITS = 20 + 63 * 26                            # worst case of one block
CHUNK_BLOCKS = 32                                    # blocks one workgroup of csrc/jpeg.hip transforms at a time

LUMA_Q = np.array([16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
                   18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99],
                  np.int32)                          # T.81 table K.1, natural order
CHROMA_Q = np.array([17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99]
                    + [99] * 32, np.int32)           # table K.2

# (number of codes of each length 1..16, the symbols in code order): tables K.3 - K.6
STD_HUFFMAN = {
    'dc_luma': ([0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0], list(range(12))),
    'dc_chroma': ([0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0], list(range(12))),
    'ac_luma': ([0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d],
                [0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81, 0x91, 0xa1, 0x08,
                 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a, 0x25, 0x26, 0x27, 0x28,
                 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59,
                 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89,
                 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6,
                 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2,
                 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa]),
    'ac_chroma': ([0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77],
                  [0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08, 0x14, 0x42, 0x91,
                   0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19, 0x1a, 0x26,
                   0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58,
                   0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87,
                   0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4,
                   0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda,
                   0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa]),
}


def _zigzag():
    order = sorted(range(64), key=lambda i: (i // 8 + i % 8, i // 8 if (i // 8 + i % 8) % 2 else i % 8))
    return np.array(order, np.int64)


ZIGZAG = _zigzag()          # ZIGZAG[k] = natural index (8 v + u) of the k-th coefficient of the scan


def _dct_real():
    u, x = np.arange(8)[:, None], np.arange(8)[None, :]
    return np.where(u == 0, np.sqrt(0.5), 1.0) / 2 * np.cos((2 * x + 1) * u * np.pi / 16)


DCT_TABLE = np.floor(_dct_real() * 8192 + 0.5).astype(np.int64)


def _dct_error_bound():
    t = _dct_real()
    d = float(np.abs(DCT_TABLE / 8192.0 - t).sum(axis=1).max())
    a = float(np.abs(t).sum(axis=1).max())
    e1 = 128 * d + 1 / 16
    return d * (128 * a + e1) + a * e1 + 1 / 16


DCT_ERROR_BOUND = _dct_error_bound()


# ---- samples ----------------------------------------------------------------------------------------------------------------------

def rgb_to_ycbcr(rgb):
    """uint8 [..., 3] -> int32 [..., 3] full-range Y'CbCr, the integers of the module's doc string."""
    v = rgb.astype(np.int32)
    r, g, b = v[..., 0], v[..., 1], v[..., 2]
    y = (19595 * r + 38470 * g + 7471 * b + 32768) >> 16
    cb = (-11059 * r - 21709 * g + 32768 * b + 8421375) >> 16
    cr = (32768 * r - 27439 * g - 5329 * b + 8421375) >> 16
    return np.stack([y, cb, cr], axis=-1)


def blocks_per_mcu(C, subsampling):
    return 1 if C == 1 else 3 if subsampling == '4:4:4' else 6


def default_restart_interval(C, subsampling):
    return CHUNK_BLOCKS // blocks_per_mcu(C, subsampling)


def mcu_grid(H, W, C, subsampling):
    """-> (MCU side, MCU rows, MCU columns)."""
    m = 16 if (C == 3 and subsampling == '4:2:0') else 8
    return m, -(-H // m), -(-W // m)


def sample_blocks(frame, subsampling):
    """uint8 [H, W, C] -> (int32 [B, 8, 8] level-shifted samples of every block in scan order, component 0..2 of every block [B])."""
    H, W, C = frame.shape
    m, my, mx = mcu_grid(H, W, C, subsampling)
    padded = np.pad(frame, ((0, my * m - H), (0, mx * m - W), (0, 0)), mode='edge')
    planes = padded.astype(np.int32) if C == 1 else rgb_to_ycbcr(padded)

    def tiles(p, k):          # [my * 8 k, mx * 8 k] -> [my, mx, k * k, 8, 8]
        return p.reshape(my, k, 8, mx, k, 8).transpose(0, 3, 1, 4, 2, 5).reshape(my, mx, k * k, 8, 8)

    if C == 1:
        parts, comp = [tiles(planes[..., 0], 1)], [0]
    elif m == 8:
        parts, comp = [tiles(planes[..., c], 1) for c in range(3)], [0, 1, 2]
    else:
        sub = [(planes[0::2, 0::2, c] + planes[0::2, 1::2, c] + planes[1::2, 0::2, c] + planes[1::2, 1::2, c] + 2) >> 2 for c in (1, 2)]
        parts, comp = [tiles(planes[..., 0], 2), tiles(sub[0], 1), tiles(sub[1], 1)], [0, 0, 0, 0, 1, 2]
    blocks = np.concatenate(parts, axis=2).reshape(-1, 8, 8) - 128
    return blocks.astype(np.int32), np.tile(np.array(comp, np.int32), my * mx)


# ---- transform --------------------------------------------------------------------------------------------------------------------

def fdct8(blocks):
    """int [B, 8, 8] samples - 128 -> int64 [B, 8, 8] F8[v][u]: the DCT coefficients in units of 1/8."""
    s = np.asarray(blocks, np.int64)
    t = (s @ DCT_TABLE.T + 512) >> 10
    return (DCT_TABLE @ t + 4096) >> 13


def quant_table(base, quality):
    scale = 5000 // quality if quality < 50 else 200 - 2 * quality
    return np.clip((base.astype(np.int64) * scale + 50) // 100, 1, 255).astype(np.int32)


def quantise(F8, q):
    """F8 [..., 64] (natural order) by q [64] or [..., 64]: F8 / (8 q) rounded half away from zero."""
    F8, q = np.asarray(F8, np.int64), np.asarray(q, np.int64)
    return np.sign(F8) * ((np.abs(F8) + 4 * q) // (8 * q))


def quantised_blocks(frame, quality, subsampling):
    """-> (int32 [B, 64] quantised coefficients in zig-zag order, blocks in scan order; component of every block [B])."""
    blocks, comp = sample_blocks(frame, subsampling)
    q = np.stack([quant_table(LUMA_Q, quality), quant_table(CHROMA_Q, quality), quant_table(CHROMA_Q, quality)])
    k = quantise(fdct8(blocks).reshape(-1, 64), q[comp])
    k[:, 1:] = np.clip(k[:, 1:], -1023, 1023)
    return k[:, ZIGZAG].astype(np.int32), comp


# ---- entropy coding ---------------------------------------------------------------------------------------------------------------

def huffman_codes(bits, vals):
    """-> (code [256], length [256]) per symbol, 0 length for a symbol without a code (T.81 Annex C)."""
    code, length = np.zeros(256, np.int64), np.zeros(256, np.int64)
    c, k = 0, 0
    for l in range(1, 17):
        for _ in range(bits[l - 1]):
            code[vals[k]], length[vals[k]] = c, l
            c += 1; k += 1
        c <<= 1
    return code, length


def _bit_length(a):
    """Number of bits of non-negative int64 values below 2^15."""
    n = np.zeros(a.shape, np.int64)
    for b in range(15):
        n += a >= (1 << b)
    return n


def block_tokens(zz, comp, interval_of_block):
    """Quantised blocks -> (code, bit count, block) of every token of the scan in stream order (before padding and stuffing)."""
    B = zz.shape[0]
    dc_tab = [huffman_codes(*STD_HUFFMAN[n]) for n in ('dc_luma', 'dc_chroma', 'dc_chroma')]
    ac_tab = [huffman_codes(*STD_HUFFMAN[n]) for n in ('ac_luma', 'ac_chroma', 'ac_chroma')]
    z = zz.astype(np.int64)
    # DC: difference to the previous block of the same component inside the interval
    diff = np.zeros(B, np.int64)
    for c in range(3):
        idx = np.flatnonzero(comp == c)
        if idx.size:
            dc, itv = z[idx, 0], interval_of_block[idx]
            prev = np.concatenate([[0], dc[:-1]])
            prev[np.concatenate([[True], itv[1:] != itv[:-1]])] = 0
            diff[idx] = dc - prev
    cat = _bit_length(np.abs(diff))
    amp = np.where(diff < 0, diff - 1, diff) & ((1 << cat) - 1)
    dcode = np.stack([t[0] for t in dc_tab])[comp, cat]
    dlen = np.stack([t[1] for t in dc_tab])[comp, cat]
    codes, nbits, keys = [(dcode << cat) | amp], [dlen + cat], [np.arange(B) * 512 + 3]
    # AC
    acode, alen = np.stack([t[0] for t in ac_tab]), np.stack([t[1] for t in ac_tab])
    b, p = np.nonzero(z[:, 1:])
    p = p + 1
    first = np.concatenate([[True], b[1:] != b[:-1]]) if b.size else np.zeros(0, bool)
    prev = np.where(first, 0, np.concatenate([[0], p[:-1]]))
    run = p - prev - 1
    v = z[b, p]
    size = _bit_length(np.abs(v))
    vamp = np.where(v < 0, v - 1, v) & ((1 << size) - 1)
    sym = ((run & 15) << 4) | size
    cb = comp[b]
    codes.append((acode[cb, sym] << size) | vamp); nbits.append(alen[cb, sym] + size); keys.append(b * 512 + p * 8 + 3)
    for j in range(3):
        sel = (run >> 4) > j
        codes.append(acode[cb[sel], 0xF0]); nbits.append(alen[cb[sel], 0xF0]); keys.append(b[sel] * 512 + p[sel] * 8 + j)
    eob = np.flatnonzero(z[:, 63] == 0)
    codes.append(acode[comp[eob], 0]); nbits.append(alen[comp[eob], 0]); keys.append(eob * 512 + 63 * 8 + 4)
    codes, nbits, keys = np.concatenate(codes), np.concatenate(nbits), np.concatenate(keys)
    order = np.argsort(keys, kind='stable')
    return codes[order], nbits[order], keys[order] >> 9


def _pack_msb(codes, nbits):
    """MSB-first packing of codes[i] in nbits[i] bits; the total is a multiple of 8."""
    start = np.cumsum(nbits) - nbits
    tok = np.repeat(np.arange(codes.shape[0]), nbits)
    bit = np.arange(tok.shape[0]) - start[tok]
    return np.packbits(((codes[tok] >> (nbits[tok] - 1 - bit)) & 1).astype(np.uint8))


def entropy_scan(zz, comp, bpm, restart_interval):
    """Quantised blocks in scan order -> the entropy-coded scan (what csrc/jpeg.hip writes per frame): uint8 array."""
    B = zz.shape[0]
    per = bpm * restart_interval                                    # blocks per interval
    interval_of_block = np.arange(B) // per
    n_int = -(-B // per)
    codes, nbits, blk = block_tokens(zz, comp, interval_of_block)
    itv = interval_of_block[blk]
    total = np.bincount(itv, weights=nbits, minlength=n_int).astype(np.int64)
    pad = (-total) % 8
    last = np.flatnonzero(np.concatenate([itv[1:] != itv[:-1], [True]]))          # last token of every interval
    codes = np.insert(codes, last + 1, (1 << pad) - 1)
    nbits = np.insert(nbits, last + 1, pad)
    raw = _pack_msb(codes, nbits)
    ends = np.cumsum((total + pad) // 8)                            # interval ends in the unstuffed bytes
    ff = np.flatnonzero(raw == 0xFF)
    stuffed = np.insert(raw, ff + 1, 0)
    ends = ends + np.searchsorted(ff, ends, side='left')            # FF bytes before every end
    out = np.insert(stuffed, np.repeat(ends[:-1], 2), np.stack([np.full(n_int - 1, 0xFF), 0xD0 + np.arange(n_int - 1) % 8], axis=1).reshape(-1))
    return out.astype(np.uint8)


def scan_bytes(frame, quality, subsampling, restart_interval):
    """uint8 [H, W, C] -> the bytes between the SOS header and EOI."""
    zz, comp = quantised_blocks(frame, quality, subsampling)
    return entropy_scan(zz, comp, blocks_per_mcu(frame.shape[2], subsampling), restart_interval).tobytes()


def worst_case_bytes(H, W, C, subsampling, restart_interval):
    """Upper bound of one frame's scan: every block 1658 bits, every byte stuffed, RSTm after every interval."""
    _, my, mx = mcu_grid(H, W, C, subsampling)
    bpm, mcus = blocks_per_mcu(C, subsampling), my * mx
    full, rest = divmod(mcus, restart_interval)
    size = lambda n: 2 * ((BLOCK_BITS * bpm * n + 7) // 8) + 2
    return full * size(restart_interval) + (size(rest) if rest else 0)


# ---- files ------------------------------------------------------------------------------------------------------------------------

def _segment(marker, payload):
    return struct.pack('>BBH', 0xFF, marker, len(payload) + 2) + payload


def jpeg_container(scan, H, W, C, quality, subsampling, restart_interval):
    """SOI, APP0, DQT, SOF0, DHT, DRI, SOS around an entropy-coded scan, EOI."""
    parts = [b'\xff\xd8', _segment(0xE0, b'JFIF\x00\x01\x01\x00' + struct.pack('>HHBB', 1, 1, 0, 0))]
    for i, base in enumerate((LUMA_Q, CHROMA_Q)[:1 if C == 1 else 2]):
        parts.append(_segment(0xDB, bytes([i]) + quant_table(base, quality)[ZIGZAG].astype(np.uint8).tobytes()))
    samp = 0x22 if (C == 3 and subsampling == '4:2:0') else 0x11
    comps = [(1, samp, 0)] if C == 1 else [(1, samp, 0), (2, 0x11, 1), (3, 0x11, 1)]
    parts.append(_segment(0xC0, struct.pack('>BHHB', 8, H, W, len(comps)) + b''.join(bytes(c) for c in comps)))
    for tc_th, name in ((0x00, 'dc_luma'), (0x10, 'ac_luma'), (0x01, 'dc_chroma'), (0x11, 'ac_chroma'))[:2 if C == 1 else 4]:
        bits, vals = STD_HUFFMAN[name]
        parts.append(_segment(0xC4, bytes([tc_th]) + bytes(bits) + bytes(vals)))
    parts.append(_segment(0xDD, struct.pack('>H', restart_interval)))
    sel = [(1, 0x00)] if C == 1 else [(1, 0x00), (2, 0x11), (3, 0x11)]
    parts.append(_segment(0xDA, bytes([len(sel)]) + b''.join(bytes(s) for s in sel) + bytes([0, 63, 0])))
    parts += [bytes(scan), b'\xff\xd9']
    return b''.join(parts)


def _check_args(frames, quality, subsampling, restart_interval):
    if not (isinstance(frames, torch.Tensor) and frames.dtype == torch.uint8 and frames.ndim in (3, 4)):
        raise ValueError('encode_jpeg: frames must be a uint8 tensor [N, H, W, C] or [H, W, C]')
    if frames.ndim == 3:
        frames = frames[None]
    N, H, W, C = frames.shape
    if C not in (1, 3) or min(N, H, W) < 1 or max(H, W) > MAX_SIDE:
        raise ValueError(f'encode_jpeg: {tuple(frames.shape)}: grey (1) or RGB (3) frames with sides 1..{MAX_SIDE} only')
    if subsampling not in SUBSAMPLINGS:
        raise ValueError(f'encode_jpeg: subsampling must be one of {sorted(SUBSAMPLINGS)}')
    if C == 1:
        subsampling = '4:4:4'                     # no chroma to subsample
    quality = int(quality)
    if not 1 <= quality <= 100:
        raise ValueError('encode_jpeg: quality must be 1..100')
    ri = default_restart_interval(C, subsampling) if restart_interval is None else int(restart_interval)
    if not 1 <= ri <= 65535:
        raise ValueError('encode_jpeg: restart_interval must be 1..65535 MCUs')
    if N * worst_case_bytes(H, W, C, subsampling, ri) >= 2 ** 31:
        raise ValueError('encode_jpeg: the worst case of the batch is 2 GiB or more; encode it in parts')
    return frames, quality, subsampling, ri


def encode_scans(frames, quality=90, subsampling='4:2:0', restart_interval=None):
    """The entropy-coded scans of `encode_jpeg` without the markers: list of N `bytes`."""
    frames, quality, subsampling, ri = _check_args(frames, quality, subsampling, restart_interval)
    if not frames.is_cuda:
        return [scan_bytes(f, quality, subsampling, ri) for f in frames.contiguous().numpy()]
    from torch_utils import hip_plugin
    return streams_to_host(*hip_plugin.JpegPlugin.encode(frames.contiguous(), quality, SUBSAMPLINGS[subsampling], ri))


def encode_jpeg(frames, quality=90, subsampling='4:2:0', restart_interval=None):
    """uint8 frames [N, H, W, C] or [H, W, C] (C = 1 grey, C = 3 RGB) on any device -> list of N complete baseline JFIF files as `bytes`.

    CUDA frames are converted, transformed, quantised and entropy-coded by the HIP kernels (3 launches for the whole batch) and reach the
    host compressed, in two copies through a pinned buffer: the N + 1 offsets, then the used bytes.  CPU frames take the numpy definition
    of this module; both give the same bytes.  Grey frames have no chroma: `subsampling` is ignored for them.  The compressed size
    depends on the data and is read on the host, so a call synchronises its stream and cannot be captured into a graph."""
    if frames.ndim == 3:
        frames = frames[None]
    checked, quality, subsampling, ri = _check_args(frames, quality, subsampling, restart_interval)
    scans = encode_scans(checked, quality, subsampling, ri)
    _, H, W, C = checked.shape
    return [jpeg_container(s, H, W, C, quality, subsampling, ri) for s in scans]


def save_jpeg(frames, paths, quality=90, subsampling='4:2:0', restart_interval=None):
    """Write frame k to paths[k] (one path for a single [H, W, C] frame)."""
    write_files(encode_jpeg(frames, quality, subsampling, restart_interval), paths, 'save_jpeg')
