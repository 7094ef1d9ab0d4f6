"""Constructed inputs of the pixel path (csrc/kernels_pre.hip: resize_linear_px, align_warp_px and their callers) with the
exact bytes each must give, derived from the geometry alone.  Pure numpy: no oracle, no library, no GPU.

Resize.  cv::resize(INTER_LINEAR) on 8-bit pixels uses 11-bit coefficients cvRound(f * 2048) (round half to even) and
    v = (((b0 * (r0 >> 4)) >> 16) + ((b1 * (r1 >> 4)) >> 16) + 2) >> 2,   r = t0 * a0 + t1 * a1 per source row.
Where the scale s / d of an axis is a dyadic rational, every step of the coefficient code is exact in f32, so the coefficients
are stated here in integers (exact_axis): position (2 * dx + 1) * p - q over 2 * q, p / q = s / d reduced.  Both factors
exactly 2 take the 2x2 mean instead.  Every case also exists transposed.

Warp.  Key points = template * s (rotated by a multiple of 90 degrees) + t with an integer template whose coordinate sums are
multiples of 5, dyadic s and t: means, sums and quotients of the similarity estimate are exact, the inverse map is
src = s * R * dst + t, and the source coordinate of every crop pixel is an integer number of 1/32 pixels -- exactly what
cv::warpAffine's 10 -> 5 bit fixed point keeps.  warp_int states its 15-bit bilinear sum in integers; whole-pixel maps are
stated once more as a plain gather (gather_int), and the two must agree."""
import math

import numpy as np

PAIRS = [(0, 255), (255, 0), (17, 201), (100, 101), (3, 250)]


# ---- resize --------------------------------------------------------------------------------------------------------------
def _div_round(num, den, half_even=True):
    """num / den (arrays of non-negative integers) rounded to nearest; ties to even, or away from zero -> (value, is a tie)"""
    q, r = np.divmod(num, den)
    tie = 2 * r == den
    up = (2 * r > den) | (tie & ((q % 2 == 1) if half_even else True))
    return q + up, tie


def exact_axis(sn, dn, clamp, half_even=True):
    """One axis of a resize from sn to dn pixels whose scale sn / dn is dyadic -> (first tap [dn], c0 [dn], c1 [dn], tie [dn]).
    clamp: the x axis (the tap is clamped and the fraction dropped); the y axis keeps its coefficients and clamps the two
    rows when they are read (resize_apply)."""
    g = math.gcd(sn, dn)
    p, q = sn // g, dn // g
    assert q & (q - 1) == 0, "scale %d / %d is not dyadic" % (sn, dn)
    assert 1.0 / (dn / sn) == sn / dn, "the double scale factor is not sn / dn"
    d = np.arange(dn, dtype=np.int64)
    num, den = (2 * d + 1) * p - q, 2 * q           # fx = num / den before the floor
    assert np.abs(num).max() < 2 ** 24                # exact as an f32
    s = num // den
    rem = num - s * den
    if clamp:
        lo, hi = s < 0, s >= sn - 1
        rem[lo | hi] = 0
        s[lo] = 0
        s[hi] = sn - 1
    c1, tie = _div_round(rem * 2048, den, half_even)
    c0, _ = _div_round((den - rem) * 2048, den, half_even)
    return s, c0, c1, tie


def is_dyadic(sn, dn):
    """whether exact_axis can state the coefficients of a resize from sn to dn pixels"""
    g = math.gcd(sn, dn)
    p, q = sn // g, dn // g
    return q & (q - 1) == 0 and 1.0 / (dn / sn) == sn / dn and max(abs(p - q), (2 * dn - 1) * p - q) < 2 ** 24


def resize_apply(src, xax, yax):
    """the integer arithmetic of the 8-bit linear resize for given coefficients of the two axes"""
    sx, a0, a1 = xax[:3]
    sy, b0, b1 = yax[:3]
    h, w = src.shape[:2]
    s = src.astype(np.int64)
    rows = s[:, sx] * a0[None, :, None] + s[:, np.minimum(sx + 1, w - 1)] * a1[None, :, None]
    r0, r1 = rows[np.clip(sy, 0, h - 1)], rows[np.clip(sy + 1, 0, h - 1)]
    v = (((b0[:, None, None] * (r0 >> 4)) >> 16) + ((b1[:, None, None] * (r1 >> 4)) >> 16) + 2) >> 2
    assert v.min() >= 0 and v.max() <= 255
    return v.astype(np.uint8)


def resize_exact(src, dh, dw, half_even=True):
    """resize of a source whose two scale factors are dyadic, stated in integers"""
    h, w = src.shape[:2]
    if h == 2 * dh and w == 2 * dw:
        return mean_2x2(src)
    return resize_apply(src, exact_axis(w, dw, True, half_even), exact_axis(h, dh, False, half_even))


def mean_2x2(src):
    s = src.astype(np.int32)
    return ((s[0::2, 0::2] + s[0::2, 1::2] + s[1::2, 0::2] + s[1::2, 1::2] + 2) >> 2).astype(np.uint8)


def noise(seed, h, w):
    return np.random.default_rng(seed).integers(0, 256, size=(h, w, 3), dtype=np.uint8)


def checker(h, w):
    yy, xx = np.mgrid[0:h, 0:w]
    return np.repeat((((yy + xx) & 1) * 255).astype(np.uint8)[:, :, None], 3, 2)


# phase of the output column -> 11-bit weight of the right-hand tap, for a k-fold upscale (fractions 3/4, 1/4; 5/8, 7/8, 1/8, 3/8)
UPSCALE_A1 = {2: [1536, 512], 4: [1280, 1792, 256, 768]}


def _step_upscale(k, along_y=False, w=6, h=3, lo=(10, 200, 33), hi=(250, 7, 160)):
    """a two-level step upscaled k times along x: columns < w / 2 at lo, the others at hi.  along_y: the transposed source
    upscaled along y, where the weights enter after the >> 4 and each tap is shifted down on its own."""
    src = np.zeros((h, w, 3), np.uint8)
    src[:, :w // 2], src[:, w // 2:] = lo, hi
    want = np.zeros((h, k * w, 3), np.uint8)
    for dx in range(k * w):
        j, ph = divmod(dx, k)
        sx = j - 1 if ph < k // 2 else j
        a1 = UPSCALE_A1[k][ph]
        t0, t1 = src[:, min(max(sx, 0), w - 1)].astype(np.int64), src[:, min(max(sx + 1, 0), w - 1)].astype(np.int64)
        if along_y:     # the other axis is the identity: r >> 4 = t * 128; the rows are clamped, the weights are not
            want[:, dx] = ((((2048 - a1) * t0 * 128) >> 16) + ((a1 * t1 * 128) >> 16) + 2) >> 2
        else:           # the tap is clamped and its fraction dropped; b0 = 2048, b1 = 0
            if sx < 0 or sx >= w - 1:
                t0, a1 = src[:, min(max(sx, 0), w - 1)].astype(np.int64), 0
            want[:, dx] = (((t0 * (2048 - a1) + t1 * a1) >> 9) + 2) >> 2
    inner = want[0, k * (w // 2 - 1) + k // 2:k * (w // 2) + k // 2]         # the k columns between the two levels' centres
    assert len({tuple(p) for p in inner}) == k
    if along_y:
        src, want = np.ascontiguousarray(src.transpose(1, 0, 2)), np.ascontiguousarray(want.transpose(1, 0, 2))
    assert np.array_equal(want, resize_exact(src, *want.shape[:2]))
    return src, want


TIE_FAMILIES = {(2, 4096): 2048, (3, 2048): 1366}   # (source, destination) pixels -> columns whose fraction * 2048 ends in .5


def tie_case(sn, dn, along_y=False):
    """A source sn pixels wide (p, q[, p] of every pair, one pair per row) resized to dn columns at the same height: every
    unclamped column has both coefficients on a rounding tie.  along_y: the transposed source resized to dn rows.
    -> (src, want, tied columns, pixels a round-half-away changes)"""
    src = np.zeros((len(PAIRS), sn, 3), np.uint8)
    for r, (p, q) in enumerate(PAIRS):
        src[r, 0::2], src[r, 1::2] = p, q
    to = (len(PAIRS), dn)
    if along_y:
        src, to = np.ascontiguousarray(src.transpose(1, 0, 2)), to[::-1]
    first, _, _, tie = exact_axis(sn, dn, not along_y)
    tie = tie & (first >= 0) & (first < sn - 1)      # along y the clamped rows keep their (tied) weights for one and the same row
    want = resize_exact(src, *to)
    away = resize_exact(src, *to, half_even=False)
    changed = int((want != away).any(2).sum())
    assert int(tie.sum()) == TIE_FAMILIES[(sn, dn)], int(tie.sum())
    assert changed > 0, "rounding half away from zero would pass this case"
    return src, want, int(tie.sum()), changed


def resize_cases():
    """-> list of (name, src [h, w, 3] u8, (dh, dw), want [dh, dw, 3] u8), every case along x and, transposed, along y.  The
    integer arithmetic is not symmetric in the two axes (one shift after the weighted sum along x, one per tap along y), so
    the transposed cases whose weights are not 0, 1024 or 2048 state their own expectation."""
    sym, out = [], []
    n = noise(901, 5, 7)
    sym.append(("identity", n, (5, 7), n.copy()))
    n = noise(902, 6, 10)
    sym.append(("both-2", n, (3, 5), mean_2x2(n)))
    for i, (shape, to) in enumerate([((5, 7), (3, 11)), ((4, 4), (9, 2)), ((1, 1), (6, 5)), ((9, 3), (2, 2))]):
        c = np.empty(shape + (3,), np.uint8)
        c[...] = [(77, 200, 3), (255, 255, 255), (1, 128, 254), (0, 9, 90)][i]
        sym.append(("constant-%dx%d-to-%dx%d" % (shape + to), c, to, np.broadcast_to(c[0, 0], to + (3,)).copy()))
    n = noise(903, 3, 10)                                 # scale_x exactly 2, scale_y 1: NOT the 2x2 mean; both taps weigh 1024
    s = n.astype(np.int32)
    sym.append(("mixed-2-by-1", n, (3, 5), ((s[:, 0::2] + s[:, 1::2] + 1) >> 1).astype(np.uint8)))
    row = noise(904, 1, 4096)                              # the size limit: 4096 -> 1 is the rounded mean of pixels 2047 and 2048
    r = row.astype(np.int32)
    sym.append(("4096-to-1", row, (1, 1), ((r[:, 2047:2048] + r[:, 2048:2049] + 1) >> 1).astype(np.uint8)))
    one = noise(905, 1, 1)
    sym.append(("1-to-4096", one, (1, 4096), np.broadcast_to(one, (1, 4096, 3)).copy()))
    for name, src, to, want in sym:
        srcT, wantT = np.ascontiguousarray(src.transpose(1, 0, 2)), np.ascontiguousarray(want.transpose(1, 0, 2))
        if not name.startswith("constant"):
            assert np.array_equal(want, resize_exact(src, *to)) and np.array_equal(wantT, resize_exact(srcT, *to[::-1])), name
        out += [(name + "-x", src, to, want), (name + "-y", srcT, to[::-1], wantT)]
    for y in (False, True):
        for k in (2, 4):
            src, want = _step_upscale(k, y)
            out.append(("step-upscale-%d-%s" % (k, "xy"[y]), src, want.shape[:2], want))
        for sn, dn in TIE_FAMILIES:
            src, want, _, _ = tie_case(sn, dn, y)
            out.append(("ties-%d-to-%d-%s" % (sn, dn, "xy"[y]), src, want.shape[:2], want))
    return out


# ---- letterbox -----------------------------------------------------------------------------------------------------------
LETTERBOX_NETS = [(32, 32), (96, 64), (64, 96)]   # image_size (w, h)
LETTERBOX_SIDES = list(range(1, 10)) + [31, 32, 33, 63, 64, 65, 95, 96, 97, 127, 128, 129, 191, 192, 193]
LETTERBOX_CLASSES = ("identity", "both-2", "mixed", "upscale", "generic", "empty")


def letterbox_class(h, w, new_h, new_w):
    """the branch of cv::resize a frame of h x w takes when it is letterboxed to new_h x new_w"""
    if new_w <= 0 or new_h <= 0:
        return "empty"
    if new_w == w and new_h == h:
        return "identity"
    x2, y2 = 1.0 / (new_w / w) == 2.0, 1.0 / (new_h / h) == 2.0
    if x2 and y2:
        return "both-2"
    if x2 or y2:
        return "mixed"
    return "upscale" if new_w > w or new_h > h else "generic"


# ---- warp ----------------------------------------------------------------------------------------------------------------
TEMPLATE = np.array([[7, 6], [16, 6], [12, 11], [8, 16], [17, 16]], np.float32)   # sums 60 and 55: the mean is an integer
CROP_W, CROP_H = 24, 20
ROT = [(1, 0), (0, 1), (-1, 0), (0, -1)]          # (cos, sin) of 0, 90, 180, 270 degrees


def gather_int(frame, sx, sy):
    """frame[sy, sx] where that lies inside, 0 elsewhere (BORDER_CONSTANT)"""
    h, w = frame.shape[:2]
    inside = (sx >= 0) & (sx < w) & (sy >= 0) & (sy < h)
    return frame[np.clip(sy, 0, h - 1), np.clip(sx, 0, w - 1)] * inside[..., None].astype(np.uint8)


def warp_int(frame, X32, Y32):
    """cv::warpAffine's bilinear sum for source coordinates given in 1/32 pixel: whole part saturated to a short, 15-bit
    weights (the whole-pixel entry is 32767 + 1 on the diagonal tap), taps outside the frame are 0"""
    sx, sy = np.clip(X32 >> 5, -32768, 32767), np.clip(Y32 >> 5, -32768, 32767)
    fx, fy = X32 & 31, Y32 & 31
    wt = [(32 - fy) * (32 - fx) * 32, (32 - fy) * fx * 32, fy * (32 - fx) * 32, fy * fx * 32]
    whole = (fx == 0) & (fy == 0)
    wt[0] = np.where(whole, 32767, wt[0])
    wt[3] = np.where(whole, 1, wt[3])
    acc = np.zeros(X32.shape + (3,), np.int64)
    for t in range(4):
        acc += gather_int(frame, sx + (t & 1), sy + (t >> 1)).astype(np.int64) * wt[t][..., None]
    return ((acc + (1 << 14)) >> 15).astype(np.uint8)


def warp_case(name, frame, s, rot, t, displaced=None):
    """key points TEMPLATE * s rotated by rot * 90 degrees + t, on `frame` -> dict(name, kps [5, 2] f32, M: the forward 2x3
    matrix (key points -> template), want: the crop [CROP_H, CROP_W, 3]).  displaced: index of one landmark moved off the model"""
    c, sn = ROT[rot]
    R = np.array([[c, -sn], [sn, c]], np.float64)
    kps64 = TEMPLATE.astype(np.float64) @ R.T * s + np.array(t, np.float64)
    kps = kps64.astype(np.float32)
    assert np.array_equal(kps.astype(np.float64), kps64), name
    if displaced is not None:
        kps[displaced] += np.array([11.0, -7.0], np.float32)
    A = s * R                                                    # src = A * dst + t
    yy, xx = np.mgrid[0:CROP_H, 0:CROP_W].astype(np.float64)
    X, Y = 32 * (A[0, 0] * xx + A[0, 1] * yy + t[0]), 32 * (A[1, 0] * xx + A[1, 1] * yy + t[1])
    assert np.array_equal(X, np.rint(X)) and np.array_equal(Y, np.rint(Y)), name
    assert max(np.abs(X).max(), np.abs(Y).max()) * 32 + 16 < 2 ** 31, name     # X0 + adelta stays an int
    X32, Y32 = X.astype(np.int64), Y.astype(np.int64)
    want = warp_int(frame, X32, Y32)
    if not ((X32 | Y32) & 31).any() and np.abs(X32 >> 5).max() < 32767 and np.abs(Y32 >> 5).max() < 32767:
        assert np.array_equal(want, gather_int(frame, X32 >> 5, Y32 >> 5)), name    # a whole-pixel map is a plain copy
    Ainv = R.T / s
    M = np.concatenate([Ainv, -(Ainv @ np.array(t, np.float64))[:, None]], 1)
    return dict(name=name, kps=kps, M=M, want=want, frame=frame)


def warp_cases(frame):
    """every closed-form warp on a frame at least 97 x 131: windows near the frame's far corner, over each of its edges,
    scaled, rotated, saturated, and with one landmark displaced"""
    H, W = frame.shape[:2]
    out = []

    def add(name, s, rot, t, displaced=None):
        out.append(warp_case(name, frame, s, rot, t, displaced))

    add("shift-int", 1.0, 0, (W - 50, H - 40))
    assert np.array_equal(out[-1]["want"], frame[H - 40:H - 20, W - 50:W - 26])
    add("shift-frac-origin", 1.0, 0, (-5.5, -3.25))
    add("shift-frac-far", 1.0, 0, (W - 30.5, H - 25.75))
    for name, t in [("left-partly", (-10, 5)), ("left-wholly", (-40, 5)), ("above-partly", (5, -8)), ("above-wholly", (5, -30)),
                    ("right-partly", (W - 12, 5)), ("right-wholly", (W + 3, 5)), ("below-partly", (5, H - 9)), ("below-wholly", (5, H + 2)),
                    ("left-half-column", (-0.5, 3)), ("right-half-column", (W - 23.5, 3)), ("above-half-row", (3, -0.5)),
                    ("below-half-row", (3, H - 19.5))]:
        add(name, 1.0, 0, t)
        if "wholly" in name:
            assert not out[-1]["want"].any()
    x = out[-3]["want"][:, -1].astype(np.int32)       # right-half-column: the last column is half the frame's last pixel, rounded
    assert np.array_equal(x, (frame[3:3 + CROP_H, W - 1].astype(np.int32) + 1) >> 1)
    add("scale-2", 2.0, 0, (W - 60, H - 50))
    assert np.array_equal(out[-1]["want"], frame[H - 50:H - 10:2, W - 60:W - 12:2])
    add("scale-2-over-the-corner", 2.0, 0, (-7, -3))
    add("scale-half", 0.5, 0, (W - 20, H - 15))
    add("rot-90", 1.0, 1, (W - 5, H - 30))
    add("rot-180", 1.0, 2, (W - 3, H - 2))
    add("rot-270", 1.0, 3, (W - 25, H - 4))
    assert np.array_equal(out[-2]["want"], frame[H - 2 - CROP_H + 1:H - 1, W - 3 - CROP_W + 1:W - 2][::-1, ::-1])
    add("rot-90-frac", 1.0, 1, (W - 5.5, H - 30.25))
    add("rot-270-scale-2", 2.0, 3, (W - 45, H - 3))
    add("saturate-high", 4096.0, 0, (-5, -5))
    add("saturate-low", 4096.0, 2, (W + 4, H + 4))
    assert not out[-1]["want"].any() and not out[-2]["want"].any()
    base = warp_case("base", frame, 1.0, 0, (W - 30.5, H - 25.75))
    for i in range(5):
        add("displaced-%d" % i, 1.0, 0, (W - 30.5, H - 25.75), displaced=i)
        assert np.array_equal(out[-1]["want"], base["want"])
    return out


WIDE_W = 33000   # a frame wider than a short can index: the whole part of a coordinate saturates INSIDE it
WIDE_H = 64      # high enough for the frame to letterbox to at least one row of a 640 x 640 network input


def wide_frame():
    return noise(990, WIDE_H, WIDE_W)


def wide_cases(frame):
    """on a frame wider than 32767 pixels the saturated coordinate still lies inside: columns past 32767 all read pixel 32767"""
    out = [warp_case("saturate-inside-int", frame, 1.0, 0, (32756, 0)), warp_case("saturate-inside-frac", frame, 1.0, 0, (32755.5, WIDE_H - 13.75))]
    w = out[0]["want"]
    assert np.array_equal(w[:, :12], frame[:CROP_H, 32756:32768])
    assert np.array_equal(w[:, 12:], np.repeat(frame[:CROP_H, 32767:32768], CROP_W - 12, 1))
    assert out[1]["want"][:13].any() and not out[1]["want"][14:].any()
    return out
