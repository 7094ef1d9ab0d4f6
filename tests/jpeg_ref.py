"""The parallel half of the baseline JPEG decoder restated in numpy: dequantised coefficients -> libjpeg's accurate integer
IDCT -> fancy (triangle) chroma upsampling -> YCbCr to RGB.  Integer arithmetic throughout (int64, so nothing wraps); the
judge of every formula here is libjpeg-turbo through Pillow (tests/test_jpeg_cpu.py compares byte for byte).

Layout of the coefficients, as rfd_debug_jpeg_coefficients returns them: [blocks, 64] i16 in natural (row-major) order, the
blocks component-major, each component's plane padded to whole MCUs and walked row by row."""
import numpy as np

GRAY, S444, S422, S420 = 0, 1, 2, 3
_LUMA = {GRAY: (1, 1), S444: (1, 1), S422: (2, 1), S420: (2, 2)}   # luma sampling (h, v); chroma is 1 x 1

# jidctint.c: 13-bit constants, 2 extra bits kept by the column pass
_CONST_BITS, _PASS1_BITS = 13, 2
_F = dict(f0298=2446, f0390=3196, f0541=4433, f0765=6270, f0899=7373, f1175=9633, f1501=12299, f1847=15137, f1961=16069,
          f2053=16819, f2562=20995, f3072=25172)


def _idct_1d(x):
    """x: eight arrays (frequencies 0..7) -> eight arrays of sums scaled by 2^13, before the descale"""
    F = _F
    z2, z3 = x[2], x[6]
    z1 = (z2 + z3) * F["f0541"]
    tmp2 = z1 - z3 * F["f1847"]
    tmp3 = z1 + z2 * F["f0765"]
    tmp0 = (x[0] + x[4]) << _CONST_BITS
    tmp1 = (x[0] - x[4]) << _CONST_BITS
    tmp10, tmp13, tmp11, tmp12 = tmp0 + tmp3, tmp0 - tmp3, tmp1 + tmp2, tmp1 - tmp2
    tmp0, tmp1, tmp2, tmp3 = x[7], x[5], x[3], x[1]
    z1, z2, z3, z4 = tmp0 + tmp3, tmp1 + tmp2, tmp0 + tmp2, tmp1 + tmp3
    z5 = (z3 + z4) * F["f1175"]
    tmp0, tmp1, tmp2, tmp3 = tmp0 * F["f0298"], tmp1 * F["f2053"], tmp2 * F["f3072"], tmp3 * F["f1501"]
    z1, z2, z3, z4 = -z1 * F["f0899"], -z2 * F["f2562"], -z3 * F["f1961"] + z5, -z4 * F["f0390"] + z5
    tmp0, tmp1, tmp2, tmp3 = tmp0 + z1 + z3, tmp1 + z2 + z4, tmp2 + z2 + z3, tmp3 + z1 + z4
    return [tmp10 + tmp3, tmp11 + tmp2, tmp12 + tmp1, tmp13 + tmp0, tmp13 - tmp0, tmp12 - tmp1, tmp11 - tmp2, tmp10 - tmp3]


def _descale(x, n):
    return (x + (1 << (n - 1))) >> n


def idct_unclamped(coef):
    """[blocks, 64] dequantised coefficients, natural order -> [blocks, 8, 8] i64 samples before the level shift and the clamp"""
    b = np.asarray(coef, np.int64).reshape(-1, 8, 8)
    ws = np.stack([_descale(v, _CONST_BITS - _PASS1_BITS) for v in _idct_1d([b[:, r, :] for r in range(8)])], 1)   # columns
    return np.stack([_descale(v, _CONST_BITS + _PASS1_BITS + 3) for v in _idct_1d([ws[:, :, k] for k in range(8)])], 2)  # rows


def idct(coef):
    """[blocks, 64] dequantised coefficients, natural order -> [blocks, 8, 8] u8 samples"""
    return np.clip(idct_unclamped(coef) + 128, 0, 255).astype(np.uint8)


def geometry(width, height, sampling):
    """-> (components, [(blocks per row, blocks per column)] per component, (hmax, vmax))"""
    h, v = _LUMA[sampling]
    mx, my = -(-width // (8 * h)), -(-height // (8 * v))
    if sampling == GRAY:
        return 1, [(mx, my)], (1, 1)
    return 3, [(mx * h, my * v), (mx, my), (mx, my)], (h, v)


def num_blocks(width, height, sampling):
    return sum(bw * bh for bw, bh in geometry(width, height, sampling)[1])


def planes(coef, width, height, sampling):
    """the u8 component planes, padded to whole MCUs"""
    _, dims, _ = geometry(width, height, sampling)
    px = idct(coef)
    out, at = [], 0
    for bw, bh in dims:
        p = px[at:at + bw * bh].reshape(bh, bw, 8, 8).transpose(0, 2, 1, 3).reshape(bh * 8, bw * 8)
        out.append(p)
        at += bw * bh
    assert at == px.shape[0], (at, px.shape)
    return out


def _interleave(a, b, axis):
    s = list(a.shape)
    s[axis] *= 2
    return np.stack([a, b], axis + 1).reshape(s)


def upsample_h2v1(c):
    """[rows, dw] -> [rows, 2 dw]: jdsample.c h2v1_fancy_upsample; a plane of one or two samples per row is replicated"""
    c = c.astype(np.int64)
    if c.shape[1] <= 2:
        return np.repeat(c, 2, 1)
    p = np.concatenate([c[:, :1], c[:, :-1]], 1)
    n = np.concatenate([c[:, 1:], c[:, -1:]], 1)
    even, odd = (3 * c + p + 1) >> 2, (3 * c + n + 2) >> 2
    even[:, 0], odd[:, -1] = c[:, 0], c[:, -1]
    return _interleave(even, odd, 1)


def upsample_h2v2(c):
    """[dh, dw] -> [2 dh, 2 dw]: h2v2_fancy_upsample; the rows above the first and below the last are those rows themselves"""
    c = c.astype(np.int64)
    if c.shape[1] <= 2:
        return np.repeat(np.repeat(c, 2, 0), 2, 1)
    up = np.concatenate([c[:1], c[:-1]], 0)
    down = np.concatenate([c[1:], c[-1:]], 0)
    s = _interleave(3 * c + up, 3 * c + down, 0)
    p = np.concatenate([s[:, :1], s[:, :-1]], 1)
    n = np.concatenate([s[:, 1:], s[:, -1:]], 1)
    even, odd = (3 * s + p + 8) >> 4, (3 * s + n + 7) >> 4
    even[:, 0], odd[:, -1] = (4 * s[:, 0] + 8) >> 4, (4 * s[:, -1] + 7) >> 4
    return _interleave(even, odd, 1)


def ycc_to_rgb(y, cb, cr):
    y, cb, cr = y.astype(np.int64), cb.astype(np.int64) - 128, cr.astype(np.int64) - 128
    r = y + ((91881 * cr + 32768) >> 16)
    g = y + ((-22554 * cb - 46802 * cr + 32768) >> 16)
    b = y + ((116130 * cb + 32768) >> 16)
    return np.clip(np.stack([r, g, b], -1), 0, 255).astype(np.uint8)


def decode(coef, width, height, sampling):
    """dequantised coefficients -> what Pillow returns: [H, W, 3] u8 RGB, or [H, W] u8 for a grey file"""
    pl = planes(coef, width, height, sampling)
    if sampling == GRAY:
        return pl[0][:height, :width].copy()
    h, v = _LUMA[sampling]
    dw, dh = -(-width // h), -(-height // v)   # the chroma planes' own size
    chroma = []
    for c in pl[1:]:
        c = c[:dh, :dw]
        if (h, v) == (2, 1):
            c = upsample_h2v1(c)
        elif (h, v) == (2, 2):
            c = upsample_h2v2(c)
        chroma.append(c[:height, :width])
    return ycc_to_rgb(pl[0][:height, :width], chroma[0], chroma[1])


def to_bgr(pixels):
    """the golden pixels as the library's frames hold them: [H, W, 3] u8 BGR (a grey file: B = G = R = Y)"""
    p = np.asarray(pixels)
    return np.repeat(p[..., None], 3, -1) if p.ndim == 2 else p[..., ::-1].copy()
