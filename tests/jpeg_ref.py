"""An independent baseline JPEG decoder and AVI parser for the tests (it shares no code with training/jpeg.py or training/video_render.py):
markers, Huffman decoding from the file's own DHT segments, restart handling, the quantised coefficients of every block, and a float64
dequantise + inverse DCT + colour path.  Plain loops: for the small frames of tests/jpeg_cases.py only."""
import struct

import numpy as np

# the zig-zag sequence of T.81 figure 5: position in the scan -> (row, column)
_ZZ = []
for _d in range(15):
    _cells = [(i, _d - i) for i in range(8) if 0 <= _d - i < 8]
    _ZZ += _cells if _d % 2 else _cells[::-1]


class _Bits:
    def __init__(self, data, pos):
        self.data, self.pos, self.acc, self.n = data, pos, 0, 0

    def bit(self):
        if self.n == 0:
            b = self.data[self.pos]
            self.pos += 1
            if b == 0xFF:
                assert self.data[self.pos] == 0x00, 'a marker inside an interval'
                self.pos += 1
            self.acc, self.n = b, 8
        self.n -= 1
        return (self.acc >> self.n) & 1

    def bits(self, k):
        v = 0
        for _ in range(k):
            v = (v << 1) | self.bit()
        return v

    def symbol(self, table):
        code, length = 0, 0
        while True:
            code = (code << 1) | self.bit()
            length += 1
            if (length, code) in table:
                return table[(length, code)]
            assert length < 16, 'no such code'

    def end_interval(self):
        """The rest of the byte must be 1-bits; -> how many there were."""
        n = self.n
        assert self.bits(n) == (1 << n) - 1, 'an interval is padded with 1-bits'
        return n


def _extend(v, size):
    return v if size == 0 or v >> (size - 1) else v - (1 << size) + 1


def parse(data):
    """-> dict: width, height, components [(id, h, v, tq)], qtables {id: [64] natural order}, dht {(class, id): (bits, vals)}, dri, markers
    (in order), coefficients {component index: int array [blocks down, blocks across, 8, 8]} (quantised, padded grid), tokens (list of
    ('dc', category) / ('ac', run-size byte) per block in scan order), scan_blocks [(component index, [8, 8] quantised)] in scan order, rst (the restart
    markers met, in order), pad_bits (the 1-bits that closed every interval)."""
    assert data[:2] == b'\xff\xd8'
    pos, out = 2, dict(qtables={}, dht={}, dri=0, markers=['SOI'], tokens=[], rst=[], scan_blocks=[])
    while True:
        assert data[pos] == 0xFF, hex(data[pos])
        marker = data[pos + 1]
        length = struct.unpack('>H', data[pos + 2:pos + 4])[0]
        body = data[pos + 4:pos + 2 + length]
        pos += 2 + length
        out['markers'].append(marker)
        if marker == 0xE0:
            assert body[:5] == b'JFIF\x00' and body[5:7] == b'\x01\x01'
        elif marker == 0xDB:
            while body:
                assert body[0] >> 4 == 0
                t = np.zeros(64, np.int64)
                for k in range(64):
                    t[_ZZ[k][0] * 8 + _ZZ[k][1]] = body[1 + k]
                out['qtables'][body[0] & 15] = t
                body = body[65:]
        elif marker == 0xC0:
            p, h, w, n = struct.unpack('>BHHB', body[:6])
            assert p == 8
            out['height'], out['width'] = h, w
            out['components'] = [(body[6 + 3 * i], body[7 + 3 * i] >> 4, body[7 + 3 * i] & 15, body[8 + 3 * i]) for i in range(n)]
        elif marker == 0xC4:
            while body:
                bits, total = list(body[1:17]), sum(body[1:17])
                out['dht'][(body[0] >> 4, body[0] & 15)] = (bits, list(body[17:17 + total]))
                body = body[17 + total:]
        elif marker == 0xDD:
            out['dri'] = struct.unpack('>H', body)[0]
        elif marker == 0xDA:
            ns = body[0]
            sel = [(body[1 + 2 * i], body[2 + 2 * i] >> 4, body[2 + 2 * i] & 15) for i in range(ns)]
            assert tuple(body[1 + 2 * ns:]) == (0, 63, 0)
            break
        else:
            raise AssertionError(f'unexpected marker {marker:02x}')
    tables = {}
    for key, (bits, vals) in out['dht'].items():
        t, code, k = {}, 0, 0
        for l in range(1, 17):
            for _ in range(bits[l - 1]):
                t[(l, code)] = vals[k]
                code += 1; k += 1
            code <<= 1
        tables[key] = t
    comps = out['components']
    hmax, vmax = max(c[1] for c in comps), max(c[2] for c in comps)
    mx, my = -(-out['width'] // (8 * hmax)), -(-out['height'] // (8 * vmax))
    coef = {i: np.zeros([my * c[2], mx * c[1], 8, 8], np.int64) for i, c in enumerate(comps)}
    order = [[i for i, c in enumerate(comps) if c[0] == cid][0] for cid, _, _ in sel]
    rd, pred, left = _Bits(data, pos), [0] * len(comps), out['dri']
    out['pad_bits'] = []
    for m in range(mx * my):
        if out['dri'] and left == 0:
            out['pad_bits'].append(rd.end_interval())
            assert data[rd.pos] == 0xFF and 0xD0 <= data[rd.pos + 1] <= 0xD7, 'RSTm expected'
            out['rst'].append(data[rd.pos + 1] - 0xD0)
            rd.pos += 2
            pred, left = [0] * len(comps), out['dri']
        left -= 1
        for ci, (_, td, ta) in zip(order, sel):
            _, h, v, _ = comps[ci]
            for by in range(v):
                for bx in range(h):
                    block, toks = np.zeros(64, np.int64), []
                    size = rd.symbol(tables[(0, td)])
                    toks.append(('dc', size))
                    pred[ci] += _extend(rd.bits(size), size)
                    block[0] = pred[ci]
                    k = 1
                    while k < 64:
                        rs = rd.symbol(tables[(1, ta)])
                        toks.append(('ac', rs))
                        if rs == 0x00:
                            break
                        if rs == 0xF0:
                            k += 16
                            continue
                        k += rs >> 4
                        assert k < 64
                        block[k] = _extend(rd.bits(rs & 15), rs & 15)
                        k += 1
                    nat = np.zeros([8, 8], np.int64)
                    for k in range(64):
                        nat[_ZZ[k]] = block[k]
                    coef[ci][(m // mx) * v + by, (m % mx) * h + bx] = nat
                    out['tokens'].append(toks)
                    out['scan_blocks'].append((ci, nat))
    out['pad_bits'].append(rd.end_interval())
    assert data[rd.pos:rd.pos + 2] == b'\xff\xd9' and rd.pos + 2 == len(data), 'EOI expected right after the scan'
    out['coefficients'] = coef
    out['scan'] = data[pos:rd.pos]
    return out


def _idct_matrix():
    u, x = np.arange(8)[:, None], np.arange(8)[None, :]
    return np.where(u == 0, np.sqrt(0.5), 1.0) / 2 * np.cos((2 * x + 1) * u * np.pi / 16)          # [u, x]


def fdct_f64(blocks):
    """float64 [..., 8, 8] samples - 128 -> the real DCT coefficients F[v][u]."""
    d = _idct_matrix()
    return d @ np.asarray(blocks, np.float64) @ d.T


def decode(data):
    """-> (uint8 [H, W] or [H, W, 3], the parse): float64 dequantise + inverse DCT, chroma replicated 2 x 2, JFIF colour."""
    p = parse(data)
    d = _idct_matrix()
    comps = p['components']
    hmax, vmax = max(c[1] for c in comps), max(c[2] for c in comps)
    planes = []
    for i, (_, h, v, tq) in enumerate(comps):
        c = p['coefficients'][i] * p['qtables'][tq].reshape(8, 8)
        px = d.T @ c.astype(np.float64) @ d + 128.0
        plane = px.transpose(0, 2, 1, 3).reshape(px.shape[0] * 8, px.shape[1] * 8)
        planes.append(np.repeat(np.repeat(plane, vmax // v, axis=0), hmax // h, axis=1))
    H, W = p['height'], p['width']
    if len(planes) == 1:
        return np.clip(np.rint(planes[0][:H, :W]), 0, 255).astype(np.uint8), p
    y, cb, cr = (q[:H, :W] for q in planes)
    rgb = np.stack([y + 1.402 * (cr - 128), y - 0.344136 * (cb - 128) - 0.714136 * (cr - 128), y + 1.772 * (cb - 128)], axis=-1)
    return np.clip(np.rint(rgb), 0, 255).astype(np.uint8), p


def parse_avi(data):
    """RIFF walk of an AVI 1.0 file -> dict: avih (14 ints), strh (dict), strf (tuple), movi (offset of the 'movi' fourcc), chunks [(offset of
    the chunk header in the file, id, size)], idx1 [(id, flags, offset, size)], sizes_consistent."""
    assert data[:4] == b'RIFF' and data[8:12] == b'AVI '
    riff_size = struct.unpack('<I', data[4:8])[0]
    out = dict(chunks=[], idx1=[], riff_size=riff_size, file_size=len(data), lists=[])

    def walk(lo, hi, depth):
        pos = lo
        while pos < hi:
            cid, size = data[pos:pos + 4], struct.unpack('<I', data[pos + 4:pos + 8])[0]
            assert pos + 8 + size <= hi, (cid, pos, size, hi)
            if cid == b'LIST':
                kind = data[pos + 8:pos + 12]
                out['lists'].append((kind, pos, size))
                if kind == b'movi':
                    out['movi'] = pos + 8
                walk(pos + 12, pos + 8 + size, depth + 1)
            elif cid == b'avih':
                out['avih'] = struct.unpack('<14I', data[pos + 8:pos + 8 + size])
            elif cid == b'strh':
                v = struct.unpack('<4s4sIHHIIIIIIII4H', data[pos + 8:pos + 8 + size])
                out['strh'] = dict(type=v[0], handler=v[1], scale=v[6], rate=v[7], length=v[9], frame=v[13:17])
            elif cid == b'strf':
                out['strf'] = struct.unpack('<IiiHH4sIiiII', data[pos + 8:pos + 8 + size])
            elif cid == b'idx1':
                out['idx1'] = [struct.unpack('<4sIII', data[pos + 8 + 16 * k:pos + 24 + 16 * k]) for k in range(size // 16)]
            else:
                out['chunks'].append((pos, cid, size))
            pos += 8 + size + (size & 1)
        assert pos == hi, 'chunks (with their padding) fill their list exactly'

    walk(12, 8 + riff_size, 0)
    return out
