"""PNG files from uint8 frames: the image sink of the reference's `gen_images.py` (`save_image(imgs, 'seed0000.png', normalize=True,
range=(-1, 1))`, gen_images.py:115-116) without torchvision / PIL, and with the compression on the device (csrc/png.hip, DESIGN.md
section 5.32).

The stream is defined HERE, in integers, and the HIP kernels reproduce it byte for byte (the pattern of `mesh_extraction` /
`mesh_render`): CUDA frames take the kernels, CPU frames take the numpy definition below, and the two give the same files.

  rows      PNG filter types 0-4 (PNG spec section 9; bytes left of the row and above the first row are 0).  `adaptive`: per row the type
            with the smallest sum of min(v, 256 - v) over its filtered bytes, the lowest type on a tie.  The filtered stream is
            [type | W * C bytes] per row.
  segments  `segment_bytes` (a power of two, 1024..32768) consecutive bytes of a frame's filtered stream, the last one shorter.  Nothing
            refers across a segment boundary: each segment is one deflate block that ends on a byte boundary.
  tokens    every maximal run of L equal bytes inside a segment: one literal, then with m = L - 1 matches of length min(m, 258) at
            distance 1 while m >= 3, then m < 3 literals (zlib's Z_RLE); then end-of-block.
  codes     `code_lengths`: Huffman lengths by the two-queue merge over (count, symbol)-sorted leaves, leaf first on equal counts; only
            the NUMBER of leaves per depth is kept, depths past the limit (15; 7 for the code-length alphabet) are folded into the limit and
            the Kraft sum repaired by moving one leaf down at a time from the deepest non-empty level; lengths are then dealt out shortest
            first from the most frequent symbol down (the larger symbol first on equal counts).  Canonical codes per RFC 1951 3.2.2.
  header    HLIT = last used literal/length symbol - 256, HDIST = 0 (one distance code: length 1 when the block has a match, else 0),
            the lengths run-length coded with 16 / 17 / 18 by `code_length_tokens`, HCLEN from the last used entry of the RFC's order.
  stored    a segment of n bytes whose dynamic form (the closing empty stored block of a non-final segment included) is not smaller
            than n + 5 bytes is written as one stored block: a segment never takes more than n + 5 bytes.
  closing   a non-final segment ends with an empty stored block (3 zero bits, pad, 00 00 FF FF); the last one sets BFINAL and pads.
  frame     78 01, the segments, Adler-32 (big endian).
"""

import struct
import zlib

import numpy as np
import torch

from training.stream_io import streams_to_host, write_files

FILTERS = {'none': 0, 'sub': 1, 'up': 2, 'average': 3, 'paeth': 4, 'adaptive': 5}
MIN_SEGMENT_BYTES, MAX_SEGMENT_BYTES = 1024, 32768
DEFAULT_SEGMENT_BYTES = 32768          # scripts/bench_png.py compares 16 and 32 KiB (profiles/png/)
STORED_OVERHEAD = 5                    # bytes a stored block adds to its segment: the per-segment worst case
ADLER = 65521
CL_ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)
PNG_SIGNATURE = b'\x89PNG\r\n\x1a\n'


# ---- rows -------------------------------------------------------------------------------------------------------------------------

def _filter_candidates(frame):
    """uint8 [H, W, C] -> uint8 [5, H, W * C]: the five filtered forms of every row."""
    H, W, C = frame.shape
    x = frame.reshape(H, W * C).astype(np.int32)
    a = np.zeros_like(x); a[:, C:] = x[:, :-C] if W > 1 else 0
    b = np.zeros_like(x); b[1:] = x[:-1]
    c = np.zeros_like(x); c[1:, C:] = x[:-1, :-C] if W > 1 else 0
    p = a + b - c
    pa, pb, pc = np.abs(p - a), np.abs(p - b), np.abs(p - c)
    paeth = np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, c))
    return np.stack([x, x - a, x - b, x - ((a + b) >> 1), x - paeth]).astype(np.uint8)


def filter_rows(frame, mode):
    """uint8 [H, W, C] -> (filtered stream uint8 [H * (W * C + 1)], filter type per row uint8 [H])."""
    H, W, C = frame.shape
    cand = _filter_candidates(frame)
    if mode == 5:
        v = cand.astype(np.int64)
        cost = np.minimum(v, 256 - v).sum(axis=2)          # [5, H]
        types = np.argmin(cost, axis=0).astype(np.uint8)   # first minimum = lowest type
    else:
        types = np.full([H], mode, np.uint8)
    out = np.empty([H, W * C + 1], np.uint8)
    out[:, 0] = types
    out[:, 1:] = cand[types, np.arange(H)]
    return out.reshape(-1), types


# ---- tokens -----------------------------------------------------------------------------------------------------------------------

def _length_tables():
    sym, bits, val = np.zeros(259, np.int32), np.zeros(259, np.int32), np.zeros(259, np.int32)
    for length in range(3, 259):
        l = length - 3
        if length == 258:
            s, e = 285, 0
        elif l < 8:
            s, e = 257 + l, 0
        else:
            e = l.bit_length() - 3
            s = 257 + 4 * (e + 1) + ((l >> e) & 3)
        sym[length], bits[length], val[length] = s, e, l & ((1 << e) - 1)
    return sym, bits, val


LENGTH_SYMBOL, LENGTH_EXTRA_BITS, LENGTH_EXTRA_VALUE = _length_tables()


def segment_tokens(data):
    """uint8 [n] -> (value int32 [T], length int32 [T]): length 0 is the literal `value`, else a match of that length at distance 1."""
    n = data.shape[0]
    starts = np.concatenate([[0], np.flatnonzero(data[1:] != data[:-1]) + 1]).astype(np.int64)
    L = np.diff(np.concatenate([starts, [n]]))
    m = L - 1
    full, rem = m // 258, m % 258
    tail_match = (rem >= 3).astype(np.int64)
    count = 1 + full + np.where(rem >= 3, 1, rem)
    run = np.repeat(np.arange(starts.shape[0]), count)
    k = np.arange(run.shape[0]) - np.repeat(np.cumsum(count) - count, count)
    length = np.where((k >= 1) & (k <= full[run]), 258, np.where((k == full[run] + 1) & (tail_match[run] == 1), rem[run], 0))
    return data[starts][run].astype(np.int32), length.astype(np.int32)


def token_histogram(value, length):
    """286 literal/length counts, end-of-block included."""
    sym = np.where(length == 0, value, LENGTH_SYMBOL[length])
    hist = np.bincount(sym, minlength=286).astype(np.int64)
    hist[256] += 1
    return hist


# ---- codes ------------------------------------------------------------------------------------------------------------------------

def leaf_depth_counts(freq):
    """-> (symbols with a count in ascending (count, symbol) order, number of leaves per depth of the unlimited Huffman tree)."""
    freq = np.asarray(freq, np.int64)
    order = [int(s) for s in np.lexsort((np.arange(freq.shape[0]), freq)) if freq[s] > 0]
    n = len(order)
    if n < 2:
        return order, [0, n]
    w = [int(freq[s]) for s in order] + [0] * (n - 1)
    parent = [0] * (2 * n - 1)
    i, j = 0, n
    for k in range(n, 2 * n - 1):
        pair = []
        for _ in range(2):
            if i < n and (j >= k or w[i] <= w[j]):
                pair.append(i); i += 1
            else:
                pair.append(j); j += 1
        w[k] = w[pair[0]] + w[pair[1]]
        parent[pair[0]] = parent[pair[1]] = k
    depth = [0] * (2 * n - 1)
    for x in range(2 * n - 3, -1, -1):
        depth[x] = depth[parent[x]] + 1
    counts = [0] * (max(depth[:n]) + 1)
    for x in range(n):
        counts[depth[x]] += 1
    return order, counts


def code_lengths(freq, limit):
    """Code length per symbol (0: unused), none above `limit`."""
    order, counts = leaf_depth_counts(freq)
    lens = np.zeros(len(freq), np.int32)
    num = [0] * (limit + 1)
    for d, c in enumerate(counts):
        num[min(d, limit)] += c
    if len(counts) - 1 > limit:
        total = sum(num[l] << (limit - l) for l in range(1, limit + 1))
        while total != 1 << limit:
            num[limit] -= 1
            for l in range(limit - 1, 0, -1):
                if num[l]:
                    num[l] -= 1
                    num[l + 1] += 2
                    break
            total -= 1
    j = len(order)
    for l in range(1, limit + 1):
        for _ in range(num[l]):
            j -= 1
            lens[order[j]] = l
    return lens


def canonical_codes(lens):
    """RFC 1951 3.2.2 codes, already bit-reversed for LSB-first packing."""
    lens = np.asarray(lens, np.int64)
    bl = np.bincount(lens, minlength=17)
    bl[0] = 0
    nxt, code = [0] * 17, 0
    for b in range(1, 17):
        code = (code + int(bl[b - 1])) << 1
        nxt[b] = code
    out = np.zeros(lens.shape[0], np.int64)
    for s, l in enumerate(lens):
        if l:
            out[s] = int(format(nxt[l], '0%db' % l)[::-1], 2)
            nxt[l] += 1
    return out


def code_length_tokens(seq):
    """The code-length sequence -> [(symbol 0..18, extra value)]: a zero run takes 18 (11..138) while at least 11 are left, then 17
    (3..10), then single zeros; a run of v > 0 takes v once, then 16 (3..6) while at least 3 are left, then single v."""
    out, i, n = [], 0, len(seq)
    while i < n:
        v, c = seq[i], 1
        while i + c < n and seq[i + c] == v:
            c += 1
        i += c
        if v == 0:
            while c >= 11:
                r = min(c, 138); out.append((18, r - 11)); c -= r
            if c >= 3:
                out.append((17, c - 3)); c = 0
        else:
            out.append((int(v), 0)); c -= 1
            while c >= 3:
                r = min(c, 6); out.append((16, r - 3)); c -= r
        out.extend([(int(v), 0)] * c)
    return out


def segment_plan(data):
    """Everything the dynamic block of one segment is built from (the tests read the histogram, depths and lengths from here)."""
    value, length = segment_tokens(data)
    hist = token_histogram(value, length)
    lens = code_lengths(hist, 15)
    has_match = bool((length > 0).any())
    hlit = int(np.flatnonzero(lens)[-1]) + 1
    seq = [int(v) for v in lens[:hlit]] + [1 if has_match else 0]
    cl_tokens = code_length_tokens(seq)
    cl_hist = np.bincount([t[0] for t in cl_tokens], minlength=19).astype(np.int64)
    cl_lens = code_lengths(cl_hist, 7)
    hclen = max(4, max(i + 1 for i, s in enumerate(CL_ORDER) if cl_lens[s]))
    extra = {16: 2, 17: 3, 18: 7}
    header_bits = 17 + 3 * hclen + sum(int(cl_lens[s]) + extra.get(s, 0) for s, _ in cl_tokens)
    is_match = length > 0
    body_bits = int((hist * lens).sum()) + int(LENGTH_EXTRA_BITS[length[is_match]].sum()) + int(is_match.sum())
    return dict(value=value, length=length, hist=hist, lens=lens, has_match=has_match, hlit=hlit, cl_tokens=cl_tokens, cl_hist=cl_hist,
                cl_lens=cl_lens, hclen=hclen, bits=header_bits + body_bits, unlimited_depth=len(leaf_depth_counts(hist)[1]) - 1)


def _pack(codes, nbits, total_bits):
    """LSB-first packing of `codes[i]` in `nbits[i]` bits -> uint8 [ceil(total_bits / 8)]."""
    codes, nbits = np.asarray(codes, np.int64), np.asarray(nbits, np.int64)
    start = np.cumsum(nbits) - nbits
    tok = np.repeat(np.arange(codes.shape[0]), nbits)
    bit = np.arange(tok.shape[0]) - start[tok]
    bits = np.zeros((total_bits + 7) // 8 * 8, np.uint8)
    bits[:tok.shape[0]] = (codes[tok] >> bit) & 1
    return np.packbits(bits, bitorder='little')


def dynamic_size(bits, final):
    return (bits + 7) // 8 if final else (bits + 3 + 7) // 8 + 4


def deflate_segment(data, final):
    """uint8 [n] -> the bytes of the segment's block(s)."""
    n = data.shape[0]
    p = segment_plan(data)
    if dynamic_size(p['bits'], final) >= n + STORED_OVERHEAD:
        return bytes([1 if final else 0]) + struct.pack('<HH', n, n ^ 0xFFFF) + data.tobytes()
    codes, nbits = [1 if final else 0, 2, p['hlit'] - 257, 0, p['hclen'] - 4], [1, 2, 5, 5, 4]
    for s in CL_ORDER[:p['hclen']]:
        codes.append(int(p['cl_lens'][s])); nbits.append(3)
    cl_codes = canonical_codes(p['cl_lens'])
    extra = {16: 2, 17: 3, 18: 7}
    for s, e in p['cl_tokens']:
        codes.append(int(cl_codes[s]) | (e << int(p['cl_lens'][s]))); nbits.append(int(p['cl_lens'][s]) + extra.get(s, 0))
    lit_codes = canonical_codes(p['lens'])
    value, length = p['value'], p['length']
    sym = np.where(length == 0, value, LENGTH_SYMBOL[length])
    sl = p['lens'][sym].astype(np.int64)
    eb = np.where(length > 0, LENGTH_EXTRA_BITS[length], 0).astype(np.int64)
    # a match: length code, its extra bits, then the one-bit distance code 0
    tok_code = lit_codes[sym] | (np.where(length > 0, LENGTH_EXTRA_VALUE[length], 0).astype(np.int64) << sl)
    tok_bits = sl + eb + (length > 0)
    codes = np.concatenate([np.asarray(codes, np.int64), tok_code, [lit_codes[256]]])
    nbits = np.concatenate([np.asarray(nbits, np.int64), tok_bits, [p['lens'][256]]])
    assert int(nbits.sum()) == p['bits']
    out = _pack(codes, nbits, p['bits'] if final else p['bits'] + 3).tobytes()
    return out if final else out + b'\x00\x00\xff\xff'


def adler32_segment(data):
    """(A, B) of the segment on its own, from (1, 0)."""
    n = data.shape[0]
    d = data.astype(np.int64)
    return int((1 + d.sum()) % ADLER), int((n + (d * (n - np.arange(n))).sum()) % ADLER)


def zlib_stream(frame, mode=5, segment_bytes=DEFAULT_SEGMENT_BYTES):
    """uint8 [H, W, C] -> the frame's zlib stream (what csrc/png.hip writes per frame)."""
    stream, _ = filter_rows(frame, mode)
    F = stream.shape[0]
    parts, A, B = [b'\x78\x01'], 1, 0
    for o in range(0, F, segment_bytes):
        seg = stream[o:o + segment_bytes]
        parts.append(deflate_segment(seg, o + segment_bytes >= F))
        a, b = adler32_segment(seg)
        A, B = (A + a - 1) % ADLER, (B + b + seg.shape[0] * (A - 1)) % ADLER          # X followed by Y of length n
    parts.append(struct.pack('>I', (B << 16) | A))
    return b''.join(parts)


def worst_case_bytes(H, W, C, segment_bytes):
    """Upper bound of one frame's zlib stream: every segment stored."""
    F = H * (W * C + 1)
    return F + STORED_OVERHEAD * ((F + segment_bytes - 1) // segment_bytes) + 6


# ---- files ------------------------------------------------------------------------------------------------------------------------

def _chunk(kind, payload):
    return struct.pack('>I', len(payload)) + kind + payload + struct.pack('>I', zlib.crc32(kind + payload))


def png_container(stream, H, W, C):
    """Signature, IHDR (bit depth 8, colour type 0 or 2), one IDAT, IEND around a zlib stream."""
    ihdr = struct.pack('>IIBBBBB', W, H, 8, 0 if C == 1 else 2, 0, 0, 0)
    return PNG_SIGNATURE + _chunk(b'IHDR', ihdr) + _chunk(b'IDAT', bytes(stream)) + _chunk(b'IEND', b'')


def _check_args(frames, filter, segment_bytes):
    if not (isinstance(frames, torch.Tensor) and frames.dtype == torch.uint8 and frames.ndim in (3, 4)):
        raise ValueError('encode_png: frames must be a uint8 tensor [N, H, W, C] or [H, W, C]')
    if frames.ndim == 3:
        frames = frames[None]
    N, H, W, C = frames.shape
    if C not in (1, 3) or min(N, H, W) < 1:
        raise ValueError(f'encode_png: {C} channels / an empty axis in {tuple(frames.shape)}: grey (1) or RGB (3) images only')
    if filter not in FILTERS:
        raise ValueError(f'encode_png: filter must be one of {sorted(FILTERS)}')
    seg = DEFAULT_SEGMENT_BYTES if segment_bytes is None else int(segment_bytes)
    if seg < MIN_SEGMENT_BYTES or seg > MAX_SEGMENT_BYTES or seg & (seg - 1):
        raise ValueError(f'encode_png: segment_bytes must be a power of two in [{MIN_SEGMENT_BYTES}, {MAX_SEGMENT_BYTES}]')
    if N * worst_case_bytes(H, W, C, seg) >= 2 ** 31:
        raise ValueError('encode_png: the batch is 2 GiB or more; encode it in parts')
    return frames, FILTERS[filter], seg


def encode_zlib(frames, filter='adaptive', segment_bytes=None):
    """The zlib streams of `encode_png` without the container: list of N `bytes`."""
    frames, mode, seg = _check_args(frames, filter, segment_bytes)
    if not frames.is_cuda:
        return [zlib_stream(f, mode, seg) for f in frames.contiguous().numpy()]
    from torch_utils import hip_plugin
    return streams_to_host(*hip_plugin.PngPlugin.encode(frames.contiguous(), mode, seg))


def encode_png(frames, filter='adaptive', segment_bytes=None):
    """uint8 frames [N, H, W, C] or [H, W, C] (C = 1 grey, C = 3 RGB) on any device -> list of N complete PNG files as `bytes`.

    CUDA frames are filtered and compressed by the HIP kernels (4 launches for the whole batch) and reach the host compressed, in two
    copies through a pinned buffer: the N + 1 offsets, then the used bytes.  CPU frames take the numpy definition of this module; both
    give the same bytes.  The chunk CRC-32 is `zlib.crc32` on the host.  The compressed size depends on the data and is read on the host,
    so a call synchronises its stream and cannot be captured into a graph."""
    if frames.ndim == 3:
        frames = frames[None]
    streams = encode_zlib(frames, filter, segment_bytes)
    _, H, W, C = frames.shape
    return [png_container(s, H, W, C) for s in streams]


def save_png(frames, paths, filter='adaptive', segment_bytes=None):
    """Write frame k to paths[k] (one path for a single [H, W, C] frame)."""
    write_files(encode_png(frames, filter, segment_bytes), paths, 'save_png')


def image_grid_u8(tensor, nrow=8, padding=2, normalize=False, value_range=None, pad_value=0.0):
    """torchvision's `make_grid` + the byte conversion of its `save_image` -> uint8 [H', W', 3] on the tensor's device.
    [C, H, W] or [N, C, H, W] with C in {1, 3}; a single channel is replicated to three.  A batch of one image is kept as it is; else
    xmaps = min(nrow, N), ymaps = ceil(N / xmaps), the grid [3, (H + p) ymaps + p, (W + p) xmaps + p] is filled with `pad_value` and image k
    sits at (y (H + p) + p, x (W + p) + p).  `normalize` clamps to `value_range` (default: the tensor's min and max) and maps to
    (x - lo) / max(hi - lo, 1e-5).  Bytes are floor(clamp(255 x + 0.5, 0, 255))."""
    t = tensor.detach()
    if t.ndim == 3:
        t = t[None]
    if t.ndim != 4 or t.shape[1] not in (1, 3):
        raise ValueError(f'save_image: expected [N, C, H, W] or [C, H, W] with 1 or 3 channels, got {tuple(tensor.shape)}')
    t = t.float()
    if t.shape[1] == 1:
        t = t.expand(-1, 3, -1, -1)
    if normalize:
        lo, hi = (float(value_range[0]), float(value_range[1])) if value_range is not None else (float(t.min()), float(t.max()))
        t = (t.clamp(lo, hi) - lo) / max(hi - lo, 1e-5)
    N, _, H, W = t.shape
    if N == 1:
        grid = t[0]
    else:
        xmaps = min(int(nrow), N)
        ymaps = -(-N // xmaps)
        p = int(padding)
        grid = t.new_full([3, (H + p) * ymaps + p, (W + p) * xmaps + p], float(pad_value))
        for k in range(N):
            y, x = divmod(k, xmaps)
            grid[:, y * (H + p) + p:y * (H + p) + p + H, x * (W + p) + p:x * (W + p) + p + W] = t[k]
    return grid.mul(255).add_(0.5).clamp_(0, 255).floor().to(torch.uint8).permute(1, 2, 0).contiguous()


def save_image(tensor, path, nrow=8, padding=2, normalize=False, value_range=None, pad_value=0.0, **kwargs):
    """`torchvision.utils.save_image` as gen_images.py:115-116 calls it (`range=` of older torchvision is accepted as `value_range`),
    writing the PNG with `save_png`."""
    if 'range' in kwargs:
        value_range = kwargs.pop('range')
    if kwargs:
        raise TypeError(f'save_image: unexpected arguments {sorted(kwargs)}')
    save_png(image_grid_u8(tensor, nrow, padding, normalize, value_range, pad_value), path)
