"""A baseline JPEG writer from chosen coefficients, pure Python and numpy: what lets a test put one non-zero coefficient at a
chosen zigzag position, three distinct quantisation tables or a restart interval of one into a file that libjpeg and the
library both decode.  SOI, DQT, SOF0 (SOF1 where a table is 16-bit), DHT, an optional DRI, one interleaved SOS, EOI.

The Huffman tables are the typical ones of ITU-T T.81 Annex K.3: DC categories 0..11 and AC sizes 1..10, so a quantised AC
coefficient lies in -1023..1023 and a DC difference in -2047..2047; the writer asserts it.  The zigzag order is derived here
from the diagonal walk, not copied from the library's tables, so that the two pin each other."""
import struct

import numpy as np

import jpeg_ref

# natural (row-major) index of zigzag position k: diagonals r + c = s, walked towards row 0 when s is even
NATURAL = [r * 8 + c for r, c in sorted(((r, c) for r in range(8) for c in range(8)), key=lambda p: (p[0] + p[1], p[0] if (p[0] + p[1]) % 2 else -p[0]))]

# Annex K.3: (code lengths 1..16, symbols); the AC symbols are run << 4 | size
_AC_TAIL = [r << 4 | s for r in range(16) for s in range(1, 11)]
_DC = bytes(range(12))
_AC_LUMA = bytes.fromhex("01020300041105122131410613516107227114328191a1082342b1c11552d1f02433627282090a161718191a25262728292a3435363738393a43"
                         "4445464748494a535455565758595a636465666768696a737475767778797a838485868788898a92939495969798999aa2a3a4a5a6a7a8a9aab2"
                         "b3b4b5b6b7b8b9bac2c3c4c5c6c7c8c9cad2d3d4d5d6d7d8d9dae1e2e3e4e5e6e7e8e9eaf1f2f3f4f5f6f7f8f9fa")
_AC_CHROMA = bytes.fromhex("000102031104052131061241510761711322328108144291a1b1c109233352f0156272d10a162434e125f11718191a262728292a35363738"
                           "393a434445464748494a535455565758595a636465666768696a737475767778797a82838485868788898a92939495969798999aa2a3a4a5a6"
                           "a7a8a9aab2b3b4b5b6b7b8b9bac2c3c4c5c6c7c8c9cad2d3d4d5d6d7d8d9dae2e3e4e5e6e7e8e9eaf2f3f4f5f6f7f8f9fa")
HUFFMAN = {(0, 0): ([0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0], _DC),
           (0, 1): ([0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0], _DC),
           (1, 0): ([0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 125], _AC_LUMA),
           (1, 1): ([0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 119], _AC_CHROMA)}   # (class, table) -> (bits, symbols)
assert all(sum(b) == len(v) for b, v in HUFFMAN.values()) and sorted(_AC_LUMA) == sorted(_AC_CHROMA) == sorted(_AC_TAIL + [0x00, 0xf0])


def _codes(bits, vals):
    """symbol -> (code, length) of the canonical code"""
    out, code, k = {}, 0, 0
    for length, n in enumerate(bits, 1):
        for _ in range(n):
            out[vals[k]] = (code, length)
            code, k = code + 1, k + 1
        code <<= 1
    return out


_CODE = {key: _codes(*t) for key, t in HUFFMAN.items()}


def seg(marker, payload):
    return bytes([0xff, marker]) + struct.pack(">H", len(payload) + 2) + payload


class _Bits:
    def __init__(self):
        self.acc, self.n = 0, 0

    def put(self, value, length):
        self.acc, self.n = self.acc << length | value, self.n + length

    def coefficient(self, code, v):
        """the Huffman code of a symbol whose low nibble is the size of v, then v's magnitude bits"""
        size = abs(v).bit_length()
        self.put(*code)
        if size:
            self.put(v if v > 0 else v + (1 << size) - 1, size)

    def flush(self):
        """pads the last byte with ones -> the bytes so far, 0xFF stuffed"""
        self.put((1 << (-self.n % 8)) - 1, -self.n % 8)
        out = self.acc.to_bytes(self.n // 8, "big").replace(b"\xff", b"\xff\x00")
        self.acc, self.n = 0, 0
        return out


def _block(bits, zz, pred, dc, ac):
    diff = zz[0] - pred
    assert abs(diff) < 2048, "a DC difference of %d needs category 12" % diff
    bits.coefficient(dc[abs(diff).bit_length()], diff)
    run, last = 0, max([k for k in range(1, 64) if zz[k]], default=0)
    for k in range(1, last + 1):
        if zz[k] == 0:
            run += 1
            continue
        assert abs(zz[k]) < 1024, "an AC coefficient of %d needs size 11" % zz[k]
        for _ in range(run >> 4):
            bits.put(*ac[0xf0])
        bits.coefficient(ac[(run & 15) << 4 | abs(zz[k]).bit_length()], zz[k])
        run = 0
    if last < 63:
        bits.put(*ac[0x00])
    return zz[0]


def write(coef_q, width, height, sampling, quant, restart_interval=0, table_ids=None, extra_segments=b""):
    """coef_q: [blocks, 64] quantised coefficients, natural order, blocks component-major over planes padded to whole MCUs
    (jpeg_ref.geometry); quant: one [64] table per component, natural order, a value above 255 makes its DQT entry 16-bit;
    table_ids: the tables' ids, 0 / 1 / 2 unless given; extra_segments: bytes placed right behind SOI -> the file"""
    ncomp, dims, (hmax, vmax) = jpeg_ref.geometry(width, height, sampling)
    coef_q, quant = np.asarray(coef_q, np.int64), [np.asarray(q, np.int64).reshape(64) for q in quant]
    table_ids = list(table_ids if table_ids is not None else range(ncomp))
    assert coef_q.shape == (jpeg_ref.num_blocks(width, height, sampling), 64) and len(quant) == len(table_ids) == ncomp
    out = b"\xff\xd8" + extra_segments
    for tq, q in zip(table_ids, quant):
        assert q.min() >= 1 and q.max() <= 65535
        wide = bool(q.max() > 255)
        out += seg(0xdb, bytes([wide << 4 | tq]) + struct.pack(">64H" if wide else "64B", *(int(q[n]) for n in NATURAL)))
    factors = [(hmax, vmax)] + [(1, 1)] * (ncomp - 1)
    out += seg(0xc1 if any(q.max() > 255 for q in quant) else 0xc0, struct.pack(">BHHB", 8, height, width, ncomp) +
               b"".join(bytes([c + 1, h << 4 | v, tq]) for c, ((h, v), tq) in enumerate(zip(factors, table_ids))))
    for (klass, table), (bits, vals) in sorted(HUFFMAN.items()):
        if table < min(ncomp, 2):
            out += seg(0xc4, bytes([klass << 4 | table]) + bytes(bits) + vals)
    if restart_interval:
        out += seg(0xdd, struct.pack(">H", restart_interval))
    out += seg(0xda, bytes([ncomp]) + b"".join(bytes([c + 1, 0x11 * min(c, 1)]) for c in range(ncomp)) + bytes([0, 63, 0]))
    zz = coef_q[:, NATURAL].tolist()
    blk0 = np.cumsum([0] + [bw * bh for bw, bh in dims]).tolist()
    bits, pred, (mcux, mcuy) = _Bits(), [0] * ncomp, dims[-1]          # the last plane has one block per MCU
    for mcu in range(mcux * mcuy):
        if restart_interval and mcu and mcu % restart_interval == 0:
            out += bits.flush() + bytes([0xff, 0xd0 + (mcu // restart_interval - 1) % 8])
            pred = [0] * ncomp
        my, mx = divmod(mcu, mcux)
        for c, (h, v) in enumerate(factors):
            for b in (blk0[c] + (my * v + j) * dims[c][0] + mx * h + i for j in range(v) for i in range(h)):
                pred[c] = _block(bits, zz[b], pred[c], _CODE[0, min(c, 1)], _CODE[1, min(c, 1)])
    return out + bits.flush() + b"\xff\xd9"
