"""An independent PNG decoder for the tests of training/png.py and csrc/png.hip: chunk parsing with every CRC checked by `zlib.crc32`,
IDAT inflated by `zlib.decompress` (the authority on the validity of the Huffman tables and on the Adler-32), rows unfiltered in numpy."""
import struct
import zlib

import numpy as np

SIGNATURE = b'\x89PNG\r\n\x1a\n'


def chunks(data):
    """[(type, payload)] of a PNG file; asserts the signature, every CRC and that nothing follows IEND."""
    assert data[:8] == SIGNATURE
    out, o = [], 8
    while o < len(data):
        n, kind = struct.unpack('>I', data[o:o + 4])[0], data[o + 4:o + 8]
        payload = data[o + 8:o + 8 + n]
        assert len(payload) == n, 'truncated chunk'
        assert struct.unpack('>I', data[o + 8 + n:o + 12 + n])[0] == zlib.crc32(kind + payload), f'bad CRC in {kind!r}'
        out.append((kind, payload))
        o += 12 + n
        if kind == b'IEND':
            break
    assert o == len(data) and out[-1] == (b'IEND', b'')
    return out


def unfilter(stream, H, W, C):
    """The filtered stream [H * (W * C + 1)] -> (uint8 [H, W, C], filter type per row)."""
    rows = np.frombuffer(stream, np.uint8).reshape(H, W * C + 1)
    out = np.zeros([H, W * C], np.int32)
    prev = np.zeros([W * C], np.int32)
    for y in range(H):
        t, f = int(rows[y, 0]), rows[y, 1:].astype(np.int32)
        cur = out[y]
        assert 0 <= t <= 4
        if t == 0:
            cur[:] = f
        elif t == 2:
            cur[:] = (f + prev) & 255
        else:
            for x in range(W * C):
                a = int(cur[x - C]) if x >= C else 0
                b = int(prev[x])
                c = int(prev[x - C]) if x >= C else 0
                if t == 1:
                    pred = a
                elif t == 3:
                    pred = (a + b) // 2
                else:
                    p = a + b - c
                    pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
                    pred = a if pa <= pb and pa <= pc else (b if pb <= pc else c)
                cur[x] = (int(f[x]) + pred) & 255
        prev = cur
    return out.astype(np.uint8).reshape(H, W, C), rows[:, 0].copy()


def decode(data):
    """PNG file bytes -> (uint8 [H, W, C], filter types [H], the zlib stream of IDAT)."""
    ch = chunks(data)
    assert [k for k, _ in ch] == [b'IHDR', b'IDAT', b'IEND']
    W, H, depth, colour, comp, filt, interlace = struct.unpack('>IIBBBBB', ch[0][1])
    assert depth == 8 and colour in (0, 2) and (comp, filt, interlace) == (0, 0, 0)
    C = 1 if colour == 0 else 3
    stream = zlib.decompress(ch[1][1])
    assert len(stream) == H * (W * C + 1)
    img, types = unfilter(stream, H, W, C)
    return img, types, ch[1][1]
