"""The reduced-size JPEG decode (rfd.h, "JPEG decode, reduced size") restated in numpy beside jpeg_ref.decode: libjpeg's
scale_num / scale_denom = 1 / s for s in 2, 4, 8.  Per component an inverse DCT of its own size (jdmaster.c), the reduced
inverse DCTs of jidctred.c, the upsampling that is left (h2v1 for 4:2:2, fancy at s = 2 and 4, plain replication at s = 8), the
colour conversion of full size.  Integer arithmetic in int64; the judge is libjpeg-turbo through Pillow's draft mode
(tests/test_jpeg_scaled_cpu.py compares byte for byte)."""
import numpy as np

import jpeg_ref
from jpeg_ref import GRAY, _descale

# the frequencies an n-point reduced inverse DCT reads along one axis
READ_SET = {8: (0, 1, 2, 3, 4, 5, 6, 7), 4: (0, 1, 2, 3, 5, 6, 7), 2: (0, 1, 3, 5, 7), 1: (0,)}


def scaled_size(width, height, s):
    return -(-width // s), -(-height // s)


def idct_sizes(sampling, s):
    """-> [n per component], [(horizontal, vertical) upsampling left per component]"""
    ncomp = 1 if sampling == GRAY else 3
    hmax, vmax = jpeg_ref._LUMA[sampling]
    factors = [(hmax, vmax)] + [(1, 1)] * (ncomp - 1)
    m = 8 // s
    ns, ups = [], []
    for h, v in factors:
        n = m
        while n < 8 and (hmax * m) % (h * n * 2) == 0 and (vmax * m) % (v * n * 2) == 0:
            n *= 2
        ns.append(n)
        ups.append((hmax * m // (h * n), vmax * m // (v * n)))
    return ns, ups


def reads(n, nat):
    """does the n x n inverse DCT read the coefficient at natural index nat?"""
    return (nat >> 3) in READ_SET[n] and (nat & 7) in READ_SET[n]


def _idct4_1d(x):
    """x: frequency -> array (0 1 2 3 5 6 7 are used) -> four sums scaled by 2^14"""
    t0 = x[0] << 14
    t2 = 15137 * x[2] - 6270 * x[6]
    t10, t12 = t0 + t2, t0 - t2
    a = -1730 * x[7] + 11893 * x[5] - 17799 * x[3] + 8697 * x[1]
    c = -4176 * x[7] - 4926 * x[5] + 7373 * x[3] + 20995 * x[1]
    return [t10 + c, t12 + a, t12 - a, t10 - c]


def _idct2_1d(x):
    t10 = x[0] << 15
    t0 = -5906 * x[7] + 6967 * x[5] - 10426 * x[3] + 29692 * x[1]
    return [t10 + t0, t10 - t0]


def idct_n(coef, n):
    """[blocks, 64] dequantised coefficients, natural order -> [blocks, n, n] u8 samples of the n x n inverse DCT"""
    b = np.asarray(coef, np.int64).reshape(-1, 8, 8)
    if n == 8:
        return jpeg_ref.idct(coef)
    if n == 1:
        return np.clip(_descale(b[:, 0, 0], 3) + 128, 0, 255).astype(np.uint8).reshape(-1, 1, 1)
    one_d, k1, k2 = (_idct4_1d, 12, 19) if n == 4 else (_idct2_1d, 13, 20)
    # the column pass runs over the columns the row pass reads; the others stay zero and are never looked at
    ws = np.zeros((b.shape[0], n, 8), np.int64)
    for col in READ_SET[n]:
        for r, v in enumerate(one_d({f: b[:, f, col] for f in READ_SET[n]})):
            ws[:, r, col] = _descale(v, k1)
    out = np.stack([_descale(v, k2) for v in one_d({f: ws[:, :, f] for f in READ_SET[n]})], 2)
    return np.clip(out + 128, 0, 255).astype(np.uint8)


def planes(coef, width, height, sampling, s):
    """the u8 component planes of the scaled decode, padded to whole MCUs: n_c samples per block and axis"""
    _, dims, _ = jpeg_ref.geometry(width, height, sampling)
    ns, _ = idct_sizes(sampling, s)
    coef = np.asarray(coef)
    out, at = [], 0
    for (bw, bh), n in zip(dims, ns):
        px = idct_n(coef[at:at + bw * bh], n)
        out.append(px.reshape(bh, bw, n, n).transpose(0, 2, 1, 3).reshape(bh * n, bw * n))
        at += bw * bh
    assert at == coef.shape[0], (at, coef.shape)
    return out


def decode_scaled(coef, width, height, sampling, s):
    """dequantised coefficients -> what Pillow returns in draft mode at 1 / s: [ceil(H / s), ceil(W / s), 3] u8 RGB, or two
    dimensions for a grey file.  s = 1 is jpeg_ref.decode."""
    if s == 1:
        return jpeg_ref.decode(coef, width, height, sampling)
    pl = planes(coef, width, height, sampling, s)
    w, h = scaled_size(width, height, s)
    if sampling == GRAY:
        return pl[0][:h, :w].copy()
    _, ups = idct_sizes(sampling, s)
    chroma = []
    for c, (uh, uv) in zip(pl[1:], ups[1:]):
        assert uv == 1 and uh in (1, 2)          # h2v2 never occurs in a scaled decode
        if uh == 2:
            c = c[:h, :-(-w // 2)]                # the component's own samples
            c = np.repeat(c, 2, 1) if s == 8 else jpeg_ref.upsample_h2v1(c)   # no fancy filter when the smallest IDCT is 1 x 1
        chroma.append(c[:h, :w])
    return jpeg_ref.ycc_to_rgb(pl[0][:h, :w], chroma[0], chroma[1])

