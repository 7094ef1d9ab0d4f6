"""The baseline JPEG encoder restated in numpy (include/rfd.h, "JPEG encode"): BGR pixels -> YCbCr -> edge replication and
downsampling -> libjpeg's accurate integer forward DCT -> quantisation -> dummy blocks -> the whole file.  Integer arithmetic
throughout (int64, so nothing wraps); the judge of every rule here is libjpeg-turbo's default compressor through Pillow
(tests/test_jpeg_encode_cpu.py compares byte for byte).  The entropy coder is the test-side writer of tests/jpeg_write.py, the
geometry is tests/jpeg_ref.py's; the header is written here, because libjpeg orders its segments its own way.

Layout of the coefficients, as rfd_debug_jpeg_encode_blocks returns them: [blocks, 64] i16 in natural (row-major) order, the
blocks component-major, each component's plane padded to whole MCUs and walked row by row (rfd_debug_jpeg_coefficients)."""
import struct

import numpy as np

import jpeg_ref
import jpeg_write
from jpeg_ref import GRAY, S420, S422, S444  # noqa: F401
from jpeg_write import HUFFMAN, NATURAL, seg

_F = jpeg_ref._F
_CONST_BITS, _PASS1_BITS = 13, 2

# ITU-T T.81 Annex K.1, natural order
BASE_LUMA = [16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
             18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99]
BASE_CHROMA = [17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99] + [99] * 32


def fix(x):
    return int(x * 65536 + 0.5)


def ycc(bgr):
    """[H, W, 3] u8 BGR -> Y, Cb, Cr as [H, W] i64 (jccolor.c)"""
    p = np.asarray(bgr).astype(np.int64)
    b, g, r = p[..., 0], p[..., 1], p[..., 2]
    y = (fix(.299) * r + fix(.587) * g + fix(.114) * b + 32768) >> 16
    cb = (-fix(.16874) * r - fix(.33126) * g + fix(.5) * b + (128 << 16) + 32767) >> 16
    cr = (fix(.5) * r - fix(.41869) * g - fix(.08131) * b + (128 << 16) + 32767) >> 16
    return y, cb, cr


def tables(quality):
    """-> the luma and the chroma quantisation table, natural order (jpeg_set_quality with force_baseline)"""
    q = min(max(int(quality), 1), 100)
    scale = 5000 // q if q < 50 else 200 - 2 * q
    return [np.clip((np.asarray(base, np.int64) * scale + 50) // 100, 1, 255) for base in (BASE_LUMA, BASE_CHROMA)]


def real_blocks(width, height, sampling):
    """-> [(wb, hb)] per component: the blocks that hold samples of the image"""
    ncomp, _, (hmax, vmax) = jpeg_ref.geometry(width, height, sampling)
    out = []
    for c in range(ncomp):
        h, v = (hmax, vmax) if c == 0 else (1, 1)
        cw, ch = -(-width * h // hmax), -(-height * v // vmax)
        out.append((-(-cw // 8), -(-ch // 8)))
    return out


def _extend(p, rows, cols):
    """repeats the last row and the last column up to rows x cols"""
    p = np.concatenate([p] + [p[-1:]] * (rows - p.shape[0]), 0) if rows > p.shape[0] else p
    return np.concatenate([p] + [p[:, -1:]] * (cols - p.shape[1]), 1) if cols > p.shape[1] else p


def component_plane(p, fx, fy, wb, hb):
    """one full-size component [H, W] -> its samples [hb * 8, wb * 8], fx x fy input samples each (jcprepct.c, jcsample.c):
    the columns of the INPUT are extended to wb * 8 * fx, its rows only to a whole row group (a multiple of fy); the
    DOWNSAMPLED rows are then repeated down to hb * 8"""
    p = _extend(p, -(-p.shape[0] // fy) * fy, wb * 8 * fx)
    x = np.arange(wb * 8, dtype=np.int64)
    if (fx, fy) == (2, 2):
        p = (p[0::2, 0::2] + p[0::2, 1::2] + p[1::2, 0::2] + p[1::2, 1::2] + (1 + (x & 1))) >> 2
    elif (fx, fy) == (2, 1):
        p = (p[:, 0::2] + p[:, 1::2] + (x & 1)) >> 1
    else:
        assert (fx, fy) == (1, 1)
    return _extend(p, hb * 8, wb * 8)


def _fdct_1d(d, first):
    """d: eight arrays (samples 0..7) -> eight arrays (frequencies 0..7); jfdctint.c, the row pass when `first`"""
    F = _F
    desc = lambda x, n: (x + (1 << (n - 1))) >> n
    tmp0, tmp7, tmp1, tmp6 = d[0] + d[7], d[0] - d[7], d[1] + d[6], d[1] - d[6]
    tmp2, tmp5, tmp3, tmp4 = d[2] + d[5], d[2] - d[5], d[3] + d[4], d[3] - d[4]
    tmp10, tmp13, tmp11, tmp12 = tmp0 + tmp3, tmp0 - tmp3, tmp1 + tmp2, tmp1 - tmp2
    n = _CONST_BITS - _PASS1_BITS if first else _CONST_BITS + _PASS1_BITS
    out = [None] * 8
    if first:
        out[0], out[4] = (tmp10 + tmp11) << _PASS1_BITS, (tmp10 - tmp11) << _PASS1_BITS
    else:
        out[0], out[4] = desc(tmp10 + tmp11, _PASS1_BITS), desc(tmp10 - tmp11, _PASS1_BITS)
    z1 = (tmp12 + tmp13) * F["f0541"]
    out[2] = desc(z1 + tmp13 * F["f0765"], n)
    out[6] = desc(z1 - tmp12 * F["f1847"], n)
    z1, z2, z3, z4 = tmp4 + tmp7, tmp5 + tmp6, tmp4 + tmp6, tmp5 + tmp7
    z5 = (z3 + z4) * F["f1175"]
    tmp4, tmp5, tmp6, tmp7 = tmp4 * F["f0298"], tmp5 * F["f2053"], tmp6 * F["f3072"], tmp7 * F["f1501"]
    z1, z2, z3, z4 = -z1 * F["f0899"], -z2 * F["f2562"], -z3 * F["f1961"] + z5, -z4 * F["f0390"] + z5
    out[7], out[5], out[3], out[1] = desc(tmp4 + z1 + z3, n), desc(tmp5 + z2 + z4, n), desc(tmp6 + z2 + z3, n), desc(tmp7 + z1 + z4, n)
    return out


def fdct(samples):
    """[blocks, 8, 8] samples 0..255 -> [blocks, 8, 8] i64: the DCT scaled by 8"""
    s = np.asarray(samples, np.int64) - 128
    rows = np.stack(_fdct_1d([s[:, :, k] for k in range(8)], True), 2)
    return np.stack(_fdct_1d([rows[:, r, :] for r in range(8)], False), 1)


def quantise(coef, table):
    """[blocks, 8, 8] scaled coefficients, [64] table -> [blocks, 64]: (|c| + divisor / 2) / divisor with the sign put back"""
    d = 8 * np.asarray(table, np.int64).reshape(1, 64)
    c = coef.reshape(-1, 64)
    return np.sign(c) * ((np.abs(c) + d // 2) // d)


def blocks(bgr, quality, sampling, y_plane=None):
    """-> [blocks, 64] i16 quantised coefficients, natural order, dummy blocks included.  y_plane: the grey samples themselves,
    where the judge is handed an `L` image"""
    H, W = np.asarray(bgr).shape[:2] if y_plane is None else y_plane.shape
    ncomp, dims, (hmax, vmax) = jpeg_ref.geometry(W, H, sampling)
    full = [np.asarray(y_plane, np.int64)] if y_plane is not None else list(ycc(bgr))[:ncomp]
    tq = tables(quality)
    out = []
    for c, ((bw, bh), (wb, hb)) in enumerate(zip(dims, real_blocks(W, H, sampling))):
        h, v = (hmax, vmax) if c == 0 else (1, 1)
        plane = component_plane(full[c], hmax // h, vmax // v, wb, hb)
        px = plane.reshape(hb, 8, wb, 8).transpose(0, 2, 1, 3).reshape(-1, 8, 8)
        real = quantise(fdct(px), tq[min(c, 1)]).reshape(hb, wb, 64)
        q = np.zeros((bh, bw, 64), np.int64)
        q[:hb, :wb] = real
        # jccoefct.c: a dummy block has the DC of the block before it in its MCU's block order; in a dummy row that is, for
        # every block, the last block of the row above within the MCU
        for by in range(bh):
            for bx in range(bw):
                if by < hb and bx < wb:
                    continue
                if by < hb:
                    q[by, bx, 0] = q[by, bx - 1, 0]
                else:
                    q[by, bx, 0] = q[by - 1, bx // h * h + h - 1, 0]
        out.append(q.reshape(-1, 64))
    return np.concatenate(out, 0).astype(np.int16)


def restart_interval(width, height, sampling, restart_rows):
    """MCUs per interval: restart_rows MCU rows, 0 = no markers"""
    _, dims, _ = jpeg_ref.geometry(width, height, sampling)
    return int(restart_rows) * dims[-1][0]


def header(width, height, quality, sampling, restart_rows=0):
    """SOI .. SOS in libjpeg's order: APP0, DQT 0 [1], SOF0, DHT DC0 AC0 [DC1 AC1], [DRI], SOS"""
    ncomp, _, (hmax, vmax) = jpeg_ref.geometry(width, height, sampling)
    out = b"\xff\xd8" + seg(0xe0, b"JFIF\0" + bytes([1, 1, 0, 0, 1, 0, 1, 0, 0]))
    for t, q in enumerate(tables(quality)[:min(ncomp, 2)]):
        out += seg(0xdb, bytes([t]) + bytes(int(q[n]) for n in NATURAL))
    out += seg(0xc0, struct.pack(">BHHB", 8, height, width, ncomp) +
               b"".join(bytes([c + 1, (hmax << 4 | vmax) if c == 0 else 0x11, min(c, 1)]) for c in range(ncomp)))
    for table in range(min(ncomp, 2)):
        for klass in (0, 1):
            bits, vals = HUFFMAN[klass, table]
            out += seg(0xc4, bytes([klass << 4 | table]) + bytes(bits) + vals)
    ri = restart_interval(width, height, sampling, restart_rows)
    if ri:
        assert ri <= 65535
        out += seg(0xdd, struct.pack(">H", ri))
    return out + seg(0xda, bytes([ncomp]) + b"".join(bytes([c + 1, 0x11 * min(c, 1)]) for c in range(ncomp)) + bytes([0, 63, 0]))


def scan_of(file_bytes):
    """the bytes behind the SOS segment of a file, EOI included"""
    at = 2
    while True:
        assert file_bytes[at] == 0xff
        marker, n = file_bytes[at + 1], struct.unpack(">H", file_bytes[at + 2:at + 4])[0]
        at += 2 + n
        if marker == 0xda:
            return file_bytes[at:]


def file_from_blocks(coef, width, height, quality, sampling, restart_rows=0):
    """[blocks, 64] quantised coefficients, natural order -> the file: this header, then the scan jpeg_write.write gives"""
    ncomp = jpeg_ref.geometry(width, height, sampling)[0]
    tq = tables(quality)
    quant = [tq[min(c, 1)] for c in range(ncomp)]
    ri = restart_interval(width, height, sampling, restart_rows)
    written = jpeg_write.write(coef, width, height, sampling, quant, restart_interval=ri, table_ids=[min(c, 1) for c in range(ncomp)])
    return header(width, height, quality, sampling, restart_rows) + scan_of(written)


def encode(bgr, quality=90, sampling=S420, restart_rows=1, y_plane=None):
    """[H, W, 3] u8 BGR -> the bytes of the file, SOI to EOI"""
    H, W = np.asarray(bgr).shape[:2] if y_plane is None else y_plane.shape
    return file_from_blocks(blocks(bgr, quality, sampling, y_plane), W, H, quality, sampling, restart_rows)


def pillow(bgr, quality, sampling, restart_rows=0, y_plane=None):
    """the judge: Pillow's file for the same pixels and settings (libjpeg-turbo's default compressor)"""
    import io

    from PIL import Image
    im = Image.fromarray(np.ascontiguousarray(y_plane, np.uint8), "L") if sampling == GRAY else Image.fromarray(np.ascontiguousarray(np.asarray(bgr)[..., ::-1]))
    kw = dict(quality=int(quality), optimize=False)
    if sampling != GRAY:
        kw["subsampling"] = {S444: 0, S422: 1, S420: 2}[sampling]
    if restart_rows:
        kw["restart_marker_rows"] = int(restart_rows)
    f = io.BytesIO()
    im.save(f, "JPEG", **kw)
    return f.getvalue()
