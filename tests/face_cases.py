"""Constructed inputs of the face stage -- face_select_kernel (csrc/kernels_post.hip) and align_setup_kernel with its LMedS
estimate (csrc/kernels_pre.hip) -- with the decisions each must give, written down from the construction.  Pure numpy and plain
Python floats: no oracle, no library, no GPU.

Selection.  Every comparison of the kernel is put on its boundary and one np.nextafter step outside, on frames and ratios for
which the margins are exact in f32 (DYADIC on 1024 x 512: me = 32, centre band [-256, +128] around 512, "area" >= 4096) and on
the default config where min(50, 0.1 * W) takes the 50.  A case states the class of every row (C: valid and central, V: valid,
X: neither), the selected row and the row of the key points; sel_case asserts the classes with the f32 terms (each step checked
to be exact) and that the stated winner is the first strict maximum of its pool.

Estimate.  Key points are pixel_cases' exact similarities of its integer template (dyadic scale, quarter turns, dyadic shift), so
a two-point model through exact points has f32 errors of exactly 0 at every exact point, the least median is 0, sigma takes its
floor and the inliers are the exact points.  The least squares over four or five exact points is exact in f64 (sums of dyadics,
a division by 4 or, the coordinate sums being multiples of 5, by 5), so the inverted map is s * R | t to the bit; over three
points the mean is rounded, and the expected matrix is ls_from_mask: the written least squares over the STATED mask in plain
Python floats, which neither fuse nor reorder.  That is also how a mask shows on the device, where only the matrix comes back.
Cases with noise (marked noisy) take their mask from the f64 errors of the least-median model only where every error is a factor
of 1.9 or more away from the threshold; their matrix, too, is ls_from_mask of that mask.

Not constructible, and said so in NOT_CONSTRUCTIBLE: the triple of exact points no sampled pair lies inside; a model with fewer
than two inliers.  A fallback ROI of height 0 exists only where f32 absorbs the margin (y1 at 2^30), far below the frame: the
status is -3 either way, and it is the hook's ROI that shows rh = 0."""
import itertools
import operator

import numpy as np

import pixel_cases as pc

F = np.float32

# ---- selection -----------------------------------------------------------------------------------------------------------
MAX_DET = 8
DYADIC = (0.25, 0.125, 0.03125, 2.0 ** -7)     # margin_center_left / right, margin_edge, minimum_face_ratio
DEFAULT = (0.3, 0.3, 0.1, 0.0075)              # FaceSelectionConfig::new
BIG = (512, 1024)                              # (H, W)
TALL = (1024, 512)
VGA = (480, 640)


def _f32(op, a, b, exact=True):
    """a op b in f32; exact: asserted to be the f64 result (f32 operands of these magnitudes are exact in f64)"""
    a, b = F(a), F(b)
    with np.errstate(all="ignore"):
        r = op(a, b)
    if exact and np.isfinite(r):
        assert float(r) == op(float(a), float(b)), (op.__name__, a, b)
    return r


def margins(size, cfg):
    """-> (me, mcl, mcr, x_cen) in f32 as the kernel forms them.  DYADIC: every product is exact; DEFAULT: only me = 50 is"""
    H, W = size
    exact = cfg == DYADIC
    me = min(F(50.0), _f32(operator.mul, cfg[2], W, exact))
    if not exact:
        assert me == F(50.0), "the default config is used where the edge margin is the 50"
    return me, _f32(operator.mul, cfg[0], W, exact), _f32(operator.mul, cfg[1], W, exact), _f32(operator.truediv, W, 2)


def sel_terms(box, size, cfg, exact=True):
    """bcw, bch, ratio = width^2 / (H * W), bcw - x_cen, w + h of a row, in f32; exact: every step is asserted to be exact
    (rows with a NaN or an inf apart; the ratio only under DYADIC, where H * W and the minimum are powers of two)"""
    H, W = size
    d = [F(v) for v in box[:4]]
    wd = _f32(operator.sub, d[2], d[0], exact)
    ratio = _f32(operator.truediv, _f32(operator.mul, wd, wd, exact and cfg == DYADIC), _f32(operator.mul, H, W), exact and cfg == DYADIC)
    bcw = _f32(operator.truediv, _f32(operator.add, d[0], d[2], exact), 2, exact)
    bch = _f32(operator.truediv, _f32(operator.add, d[1], d[3], exact), 2, exact)
    off = _f32(operator.sub, bcw, margins(size, cfg)[3], exact)
    tem = _f32(operator.add, wd, _f32(operator.sub, d[3], d[1], exact), exact)
    return bcw, bch, ratio, off, tem


def classify(box, size, cfg, exact=True):
    H, W = size
    me, mcl, mcr, _ = margins(size, cfg)
    bcw, bch, ratio, off, _ = sel_terms(box, size, cfg, exact)
    with np.errstate(all="ignore"):
        valid = bcw >= me and bcw <= F(W) - me and bch >= me and bch <= F(H) - me and ratio >= F(cfg[3])
        return "X" if not valid else ("C" if -mcl <= off <= mcr else "V")


def row_kps(k):
    """key points that name their row: 100 * (row + 1) + 0 .. 9"""
    return (100.0 * (np.arange(k)[:, None] + 1) + np.arange(10)[None, :]).astype(np.float32)


def sel_case(name, rows, want, size=BIG, cfg=DYADIC, classes=None, kp="same", enroll=False, exact=True):
    """rows: (x1, y1, x2, y2) each; exact: every f32 term of every row is exact (not so one step off a boundary, where only the
    outcome of the comparison counts) -> dict(name, boxes [k, 5], kps [k, 10], size, cfg, enroll, want: the selected row or None,
    kp: the row of the key points or None, found)"""
    k = len(rows)
    assert 1 <= k <= MAX_DET
    boxes = np.zeros((k, 5), np.float32)
    boxes[:, :4] = np.array(rows, np.float32)
    boxes[:, 4] = 0.9 - 0.01 * np.arange(k)
    kp = want if kp == "same" else kp
    with np.errstate(all="ignore"):
        if enroll:
            areas = [_f32(operator.mul, _f32(operator.sub, r[2], r[0]), _f32(operator.sub, r[3], r[1])) for r in boxes]
            pool, size_of = list(range(k)), areas
        else:
            cls = "".join(classify(r, size, cfg, exact) for r in boxes)
            assert cls == classes, (name, cls, classes)
            pool = [i for i in range(k) if cls[i] == "C"] or [i for i in range(k) if cls[i] in "CV"] or list(range(k))
            size_of = [sel_terms(r, size, cfg, exact)[4] for r in boxes]
        best, first = F(0.0), None
        for i in pool:
            if size_of[i] > best:
                best, first = size_of[i], i
    assert first == want, (name, first, want)
    return dict(name=name, boxes=boxes, kps=row_kps(k), size=size, cfg=cfg, enroll=enroll, want=want, kp=kp,
                found=0 if want is None else (1 if kp is None else 3))


def _step(box, coord, toward):
    out = [F(v) for v in box]
    out[coord] = np.nextafter(out[coord], F(toward))
    assert out[coord] != F(box[coord])
    return out


def boundary_pair(name, on, coord, toward, decoy, size, cfg, classes_on, classes_out):
    """row 0: the decoy, smaller; row 1: the box on the boundary (it wins), then the same box with one coordinate one f32 step
    outside (it leaves the pool or its class, and the decoy wins)"""
    return [sel_case(name + "-on", [decoy, on], 1, size, cfg, classes_on),
            sel_case(name + "-step-outside", [decoy, _step(on, coord, toward)], 0, size, cfg, classes_out, exact=False)]


def selection_cases():
    out = []
    inf, nan = np.inf, np.nan
    # ---- enrol mode: the first strict maximum of (x2 - x1) * (y2 - y1) ----
    e = dict(enroll=True, cfg=DEFAULT, size=VGA)
    out.append(sel_case("enrol-equal-areas-keep-the-first", [(0, 0, 10, 10), (100, 100, 200, 150), (300, 300, 350, 400), (5, 5, 105, 55)], 1, **e))
    out.append(sel_case("enrol-winner-in-row-0", [(0, 0, 300, 300)] + [(10 * i, 0, 10 * i + 50, 40 + i) for i in range(1, 5)], 0, **e))
    out.append(sel_case("enrol-winner-in-the-last-row", [(10 * i, 0, 10 * i + 50, 40 + i) for i in range(MAX_DET - 1)] + [(0, 0, 300, 300)], MAX_DET - 1, **e))
    out.append(sel_case("enrol-all-zero-slab", [(0, 0, 0, 0)] * 3, None, **e))
    out.append(sel_case("enrol-both-extents-negative", [(0, 0, 40, 40), (100, 100, 50, 40), (0, 0, 50, 50)], 1, **e))
    out.append(sel_case("enrol-one-extent-negative", [(100, 100, 50, 400), (0, 0, 5, 5)], 1, **e))
    out.append(sel_case("enrol-nan-row-never-chosen", [(nan, 0, 500, 500), (0, 0, 5, 5), (0, nan, 600, 600)], 1, **e))
    out.append(sel_case("enrol-inf-area-has-its-key-points", [(0, 0, 5, 5), (0, 0, inf, 10)], 1, **e))
    # ---- the pool: centre boxes, else valid boxes, else every row ----
    out.append(sel_case("pool-centre", [(800, 100, 1000, 400), (0, 0, 1024, 10), (462, 206, 562, 306)], 2, classes="VXC"))
    out.append(sel_case("pool-valid", [(0, 0, 1024, 10), (850, 200, 950, 300), (-200, 100, 100, 500)], 1, classes="XVX"))
    out.append(sel_case("pool-all-rows", [(0, 0, 10, 10), (-200, 100, 100, 500), (0, 0, 30, 30)], 1, classes="XXX"))
    out.append(sel_case("nan-row-never-chosen", [(nan, 0, 500, 500), (0, 0, 30, 30), (0, 0, 10, nan)], 1, classes="XXX"))
    out.append(sel_case("no-positive-size-nothing-found", [(10, 10, 5, 5), (0, 0, 0, 0)], None, classes="XX"))
    # ---- every comparison on its boundary and one step outside ----
    far, mid = (850, 200, 950, 300), (462, 206, 562, 306)          # decoys: valid but not central; central.  w + h = 200
    out += boundary_pair("bcw-at-me", (-68, 100, 132, 300), 2, -inf, far, BIG, DYADIC, "VV", "VX")
    out += boundary_pair("bcw-at-W-minus-me", (892, 100, 1092, 300), 2, inf, far, BIG, DYADIC, "VV", "VX")
    out += boundary_pair("bch-at-me", (800, -68, 1000, 132), 3, -inf, far, BIG, DYADIC, "VV", "VX")
    out += boundary_pair("bch-at-H-minus-me", (800, 380, 1000, 580), 3, inf, far, BIG, DYADIC, "VV", "VX")
    out += boundary_pair("ratio-at-minimum", (868, 100, 932, 400), 2, -inf, far, BIG, DYADIC, "VV", "VX")
    out += boundary_pair("centre-at-right-margin", (128, 100, 1152, 300), 2, inf, mid, BIG, DYADIC, "CC", "CV")
    out += boundary_pair("centre-at-left-margin", (-512, 100, 1024, 300), 2, -inf, mid, BIG, DYADIC, "CC", "CV")
    # another frame size under the same config (me = 16, centre band [-128, +64] around 256): this box is invalid on 1024 x 512
    out += boundary_pair("bcw-at-me-tall-frame", (-84, 100, 116, 300), 2, -inf, (350, 200, 450, 300), TALL, DYADIC, "VV", "VX")
    small = (530, 200, 590, 260)                                      # default config on 640 x 480: me = 50
    out += boundary_pair("default-bcw-at-50", (-50, 100, 150, 300), 2, -inf, small, VGA, DEFAULT, "VV", "VX")
    out += boundary_pair("default-bcw-at-W-minus-50", (156, 100, 1024, 300), 2, inf, small, VGA, DEFAULT, "VV", "VX")
    out += boundary_pair("default-bch-at-50", (500, -50, 620, 150), 3, -inf, small, VGA, DEFAULT, "VV", "VX")
    out += boundary_pair("default-bch-at-H-minus-50", (500, 340, 620, 520), 3, inf, small, VGA, DEFAULT, "VV", "VX")
    # ---- the "area" is the width squared (sic) ----
    out.append(sel_case("area-is-width-squared", [(880, 100, 920, 400), (800, 240, 1000, 250)], 1, classes="XV"))
    # ---- ties of w + h: the first row of the pool ----
    out.append(sel_case("tie-of-w-plus-h", [(0, 0, 10, 10), (800, 100, 900, 200), (800, 250, 950, 300), (820, 300, 920, 400)], 1, classes="XVVV"))
    out.append(sel_case("tie-of-w-plus-h-all-rows", [(0, 0, 20, 10), (0, 0, 10, 20), (0, 0, 15, 15)], 0, classes="XXX"))
    # ---- key points: the first row within 2 px of the chosen box in all four coordinates ----
    chosen = (600, 150, 800, 350)
    for c, sign in enumerate((1, 1, -1, -1)):                          # the earlier row is smaller: it cannot be chosen itself
        near = list(chosen)
        near[c] += 2 * sign
        out.append(sel_case("two-px-exactly-coord-%d" % c, [(0, 0, 10, 10), near, chosen], 2, classes="XVV", kp=1))
        past = _step(near, c, sign * inf)
        assert abs(float(past[c]) - chosen[c]) > 2.0 and abs(float(F(chosen[c]) - past[c])) > 2.0
        out.append(sel_case("two-px-one-step-more-coord-%d" % c, [(0, 0, 10, 10), past, chosen], 2, classes="XVV", kp=2, exact=False))
    # ---- found == 1: a chosen box with a +inf coordinate matches no row, itself included ----
    out.append(sel_case("inf-box-without-key-points", [(0, 0, 30, 30), (100, 100, inf, 200), (0, 0, 10, 10)], 1, classes="XXX", kp=None))
    names = [c["name"] for c in out]
    assert len(set(names)) == len(names)
    return out


def selection_batch(cases, n):
    """n frames of one call: the cases of one config and mode, cycled with a stride, so that the winning row changes from frame
    to frame in every workgroup of 64"""
    assert len({(c["cfg"], c["enroll"]) for c in cases}) == 1
    stride = next(s for s in (7, 5, 3, 1) if np.gcd(s, len(cases)) == 1)
    picked = [cases[(i * stride) % len(cases)] for i in range(n)]
    for lo in range(0, n, 64):
        assert len({c["want"] for c in picked[lo:lo + 64]}) >= 3 or len(cases) < 3
    return picked


# ---- estimate and set-up -------------------------------------------------------------------------------------------------
LMEDS_PAIRS = [(0, 4), (0, 3), (1, 2), (1, 0), (3, 0), (0, 4), (1, 4), (3, 1), (0, 3), (0, 1), (0, 4), (4, 1), (0, 3)]
INLIER_FACTOR = (2.5 * 1.4826 * (1 + 5.0 / 3)) ** 2            # threshold / least median, above the floor
T_FLOOR = float(F(0.001 * 0.001))                               # (float)(sigma * sigma) at the floor
STANDARD = np.array([[38.2946, 51.6963], [73.5318, 51.5014], [56.0252, 71.7366], [41.5493, 92.3655], [70.7299, 92.2041]], np.float32)
CONFIGS = {                                                     # name -> (image_size (w, h), template)
    "small": ((pc.CROP_W, pc.CROP_H), pc.TEMPLATE),
    "flat": ((pc.CROP_W, pc.CROP_H), np.full((5, 2), 7.0, np.float32)),   # every landmark maps to (7, 7): a model of determinant 0
    "default": ((112, 112), STANDARD),
}
BOX = np.array([0, 0, 10, 10, 0.9], np.float32)
SMALL_FRAME = (97, 131)
NOT_CONSTRUCTIBLE = {
    "two-outliers-exact-2-3-4": "no sampled pair lies inside {2, 3, 4}: no exact model is ever drawn",
    "fewer-than-two-inliers": "none found, and none exists: a model is kept only with a finite least median, the third smallest "
                              "error; the threshold is max(1e-6, 97.7 * that median) >= that median, its rounding to f32 is "
                              "monotonic, and the inlier errors are recomputed from the kept model by the same "
                              "similarity_errors5 on the same inputs, so they are the same values and at least three pass",
}


def coded_frame(h, w):
    """a frame whose bytes encode their own position; no byte is 0, which is what a tap outside the frame reads"""
    yy, xx = np.mgrid[0:h, 0:w]
    return np.stack([xx % 251 + 1, yy % 241 + 1, (xx // 251) * 16 + yy // 241 + 1], 2).astype(np.uint8)


def pair_errors(kps, tmpl, i, j):
    """squared errors (f64) of the similarity through landmarks i and j, in complex arithmetic: a construction check, written
    unlike the code under test on purpose"""
    with np.errstate(all="ignore"):
        z, Z = np.empty(5, np.complex128), np.empty(5, np.complex128)
        z.real, z.imag, Z.real, Z.imag = kps[:, 0], kps[:, 1], tmpl[:, 0], tmpl[:, 1]
        a = (Z[i] - Z[j]) / (z[i] - z[j])
        return np.abs(a * (z - z[i]) + Z[i] - Z) ** 2


def exact_subsets_covered():
    """-> (triples of landmarks a sampled pair lies inside, the others)"""
    pairs = {frozenset(p) for p in LMEDS_PAIRS}
    inside = [t for t in itertools.combinations(range(5), 3) if any(p <= set(t) for p in pairs)]
    return inside, [t for t in itertools.combinations(range(5), 3) if t not in inside]


def ls_from_mask(kps, tmpl, mask):
    """the least-squares similarity over the landmarks of mask, in the written operation order, in plain Python floats
    -> the forward matrix as 6 floats"""
    src = [[float(v) for v in p] for p in kps]
    dst = [[float(v) for v in p] for p in tmpl]
    use = [i for i in range(5) if mask[i]]
    cnt = len(use)
    msx = msy = mdx = mdy = 0.0
    for i in use:
        msx += src[i][0]; msy += src[i][1]
        mdx += dst[i][0]; mdy += dst[i][1]
    msx /= cnt; msy /= cnt; mdx /= cnt; mdy /= cnt
    sxx = sa = sb = 0.0
    for i in use:
        xs, ys = src[i][0] - msx, src[i][1] - msy
        xd, yd = dst[i][0] - mdx, dst[i][1] - mdy
        sxx += xs * xs + ys * ys
        sa += xs * xd + ys * yd
        sb += xs * yd - ys * xd
    assert sxx > 0.0
    a, bb = sa / sxx, sb / sxx
    return [a, -bb, mdx - (a * msx - bb * msy), bb, a, mdy - (bb * msx + a * msy)]


def invert(m):
    """cv::warpAffine's inversion of a forward 2x3 matrix, in the written operation order, in plain Python floats"""
    m = [float(v) for v in m]
    D = m[0] * m[4] - m[1] * m[3]
    D = 1.0 / D if D != 0 else 0.0
    A11, A22 = m[4] * D, m[0] * D
    m[0] = A11; m[1] *= -D; m[3] *= -D; m[4] = A22
    b1 = -m[0] * m[2] - m[1] * m[5]
    b2 = -m[3] * m[2] - m[4] * m[5]
    m[2] = b1; m[5] = b2
    return m


def _check_exact_set(name, kps, tmpl, exact):
    """what an exact-subset case relies on: some sampled pair lies inside the exact set, such a pair's model has errors of
    0 on the set (here: below 1e-18 in f64) and gross ones elsewhere, and every other drawn model has a median far from 0 (or is no model)"""
    inside = [p for p in LMEDS_PAIRS if set(p) <= set(exact)]
    assert inside, (name, "no sampled pair avoids the outliers")
    for i, j in LMEDS_PAIRS:
        e = pair_errors(kps, tmpl, i, j)
        if (i, j) in inside:
            assert all(e[k] < 1e-18 for k in exact) and all(not e[k] <= 1.0 for k in range(5) if k not in exact), (name, i, j, e)
        else:
            with np.errstate(all="ignore"):
                assert not np.sort(e)[2] <= 1e-2, (name, i, j, e)          # third smallest; NaN sorts last


def align_case(name, kps, cfg="small", size=SMALL_FRAME, box=BOX, mode=0, mask=None, Minv=None, exact_M=False, crop=None, roi=None,
               area_fast=0, noisy=False):
    """-> dict.  mask: the inliers (a model exists); Minv: the closed-form inverted map, which M = invert(ls_from_mask) must equal
    in every value if exact_M (a zero of either sign is a zero here; the tests compare the bytes of M), else to 1e-10;
    crop: the closed-form crop or None (the oracle's bytes are the only expectation); roi = (x0, y0, rw, rh) of the fallback"""
    (ow, oh), tmpl = CONFIGS[cfg]
    found = (1 if box is not None else 0) | (2 if kps is not None else 0)
    want_M = None
    if mask is not None:
        want_M = invert(ls_from_mask(kps, tmpl, mask))
        if Minv is not None:
            got, ref = np.array(want_M).reshape(2, 3), np.asarray(Minv, np.float64)
            assert np.array_equal(got, ref) if exact_M else np.allclose(got, ref, rtol=0, atol=1e-10), (name, got, ref)
    scale = (1.0 / (ow / roi[2]), 1.0 / (oh / roi[3])) if mode == 1 else (0.0, 0.0)
    return dict(name=name, kps=None if kps is None else np.asarray(kps, np.float32), box=box, found=found, cfg=cfg, size=size, mode=mode,
                mask=None if mask is None else list(map(bool, mask)), M=want_M, exact_M=exact_M, crop=crop,
                roi=tuple(roi) if roi is not None else (0, 0, 0, 0), scale=scale, area_fast=area_fast, noisy=noisy)


def _exact_model(frame, s=1.0, rot=0, t=None):
    """pixel_cases' exact similarity on frame -> (kps [5, 2], inverted map s * R | t, crop)"""
    H, W = frame.shape[:2]
    t = (W - 30.5, H - 25.75) if t is None else t
    c = pc.warp_case("model", frame, s, rot, t)
    cs, sn = pc.ROT[rot]
    Minv = np.array([[s * cs, -s * sn, t[0]], [s * sn, s * cs, t[1]]], np.float64)
    return c["kps"], Minv, c["want"]


def noisy_mask(name, kps, tmpl):
    """the inliers of a case with noise, from the f64 errors of the least-median model: decided only with every margin wide"""
    with np.errstate(all="ignore"):
        models = {}
        for i, j in LMEDS_PAIRS:
            e = pair_errors(kps, tmpl, i, j)
            med = np.sort(e)[2]                                         # NaN and inf sort last: every NaN above every number
            if med < np.inf:
                models.setdefault(frozenset((i, j)), (med, e))
        ranked = sorted(models.values(), key=lambda m: m[0])
        med, e = ranked[0]
        assert ranked[1][0] > med * 1.01, (name, "two models compete for the least median")
        t = INLIER_FACTOR * med
        assert t > 100 * T_FLOOR, name
        mask = [bool(v <= t) for v in e]
        assert all(v <= t / 1.9 or not v <= t * 1.9 for v in e), (name, e / t)
    return mask


def alignment_cases():
    out = []
    tmpl = pc.TEMPLATE
    frame = coded_frame(*SMALL_FRAME)
    inside, uncovered = exact_subsets_covered()
    assert len(inside) == 9 and uncovered == [(2, 3, 4)]
    assert 2.0 ** -20 < T_FLOOR < 2.0 ** -19 < 2.0 ** -18
    gross = np.array([11.0, -7.0], np.float32)

    def exact_case(name, kps, exact, model, **kw):
        _check_exact_set(name, kps, tmpl, exact)
        mask = [k in exact for k in range(5)]
        out.append(align_case(name, kps, mask=mask, Minv=model[1], exact_M=len(exact) >= 4, crop=model[2], **kw))

    # ---- five exact points, a few similarities: the model every other case displaces ----
    models = {"shift": _exact_model(frame), "rot-90-scale-2": _exact_model(frame, 2.0, 1, (125.0, 40.5)), "rot-180-half": _exact_model(frame, 0.5, 2, (70.25, 60.0))}
    for n, m in models.items():
        exact_case("all-exact-" + n, m[0], (0, 1, 2, 3, 4), m)
    # ---- one gross outlier at each landmark ----
    for n, m in models.items():
        for k in range(5):
            if n != "shift" and k not in (0, 2):
                continue
            kps = m[0].copy()
            kps[k] += gross
            exact_case("one-outlier-at-%d-%s" % (k, n), kps, tuple(i for i in range(5) if i != k), m)
    # ---- two gross outliers: every triple of exact points a sampled pair lies inside ----
    m = models["shift"]
    for tr in inside:
        kps = m[0].copy()
        o1, o2 = [k for k in range(5) if k not in tr]
        kps[o1] += gross
        kps[o2] += np.array([-9.0, 13.0], np.float32)
        exact_case("two-outliers-exact-%d-%d-%d" % tr, kps, tr, m)
    # ---- the sigma floor: min_median = 0, sigma = 0.001, t = (float)1e-6; landmark 2 off the exact model by a squared error of ... ----
    for tag, d, inl in [("2^-20-inlier", (2.0 ** -10, 0.0), True), ("2^-19-outlier", (2.0 ** -10, 2.0 ** -10), False), ("2^-18-outlier", (0.0, 2.0 ** -9), False)]:
        kps = m[0].copy()
        kps[2] += np.array(d, np.float32)
        assert np.array_equal(kps[2].astype(np.float64), m[0][2].astype(np.float64) + np.array(d)), tag       # the step is exact in f32
        e = pair_errors(kps, tmpl, *LMEDS_PAIRS[0])             # the first pair drawn avoids landmark 2; a median of 0 is never replaced
        want = d[0] ** 2 + d[1] ** 2
        assert 2 not in LMEDS_PAIRS[0] and abs(e[2] - want) < 1e-9 * want and (want <= T_FLOOR) == inl and e[[0, 1, 3, 4]].max() < 1e-18
        mask = [True, True, inl, True, True]
        out.append(align_case("sigma-floor-" + tag, kps, mask=mask, Minv=None if inl else m[1], exact_M=not inl, crop=m[2]))
        if inl:     # the matrix shows the decision: it is not the four-point one
            assert out[-1]["M"] != invert(ls_from_mask(kps, tmpl, [True, True, False, True, True]))
    # ---- coincident landmarks ----
    kps = m[0].copy()
    kps[1] = kps[0]
    exact_case("coincident-0-and-1", kps, (0, 2, 3, 4), m)
    same = np.tile(np.array([[60.0, 50.0]], np.float32), (5, 1))
    fb = np.array([62, 52, 100, 60, 0.9], np.float32)
    out.append(align_case("all-five-coincident", same, box=fb, mode=1, roi=(40, 30, 91, 67)))
    # ---- a model of determinant 0: the inversion's D != 0 guard; every crop pixel reads frame (0, 0) ----
    zero = np.zeros((pc.CROP_H, pc.CROP_W), np.int64)
    out.append(align_case("determinant-zero", m[0], cfg="flat", mask=[True] * 5, Minv=np.zeros((2, 3)), exact_M=False, crop=pc.warp_int(frame, zero, zero)))
    assert (out[-1]["crop"] == frame[0, 0]).all() and not np.array(out[-1]["M"]).any()
    # ---- one non-finite landmark, on exact key points ----
    neg_nan, pos_nan = np.array([0xffc00000, 0x7fc00000], np.uint32).view(np.float32)
    bad = [("inf-inf", (np.inf, np.inf)), ("inf-0", (np.inf, 0.0)), ("nan-nan", (pos_nan, pos_nan)), ("negative-nan", (neg_nan, neg_nan))]
    for tag, v in bad:
        kps = m[0].copy()
        kps[2] = v
        exact_case("non-finite-exact-" + tag, kps, (0, 1, 3, 4), m)
    # ---- the found bits ----
    out.append(align_case("found-0", None, box=None, mode=-2))
    out.append(align_case("found-1-no-key-points", None, mode=-1))
    out.append(align_case("found-2-no-box", m[0], box=None, mode=-2))
    # ---- the fallback (all key points coincide): ROI [int(max(x1 - 22, 0)), W) x [int(max(y1 - 22, 0)), int(max(y1 + 22, H))) ----
    def fallback(name, det, size, mode, roi, cfg="small", area_fast=0, crop=None):
        out.append(align_case("fallback-" + name, same, cfg=cfg, size=size, box=np.array(list(det) + [0.9], np.float32), mode=mode, roi=roi,
                              area_fast=area_fast, crop=crop))

    S = (100, 200)                                                      # H, W
    fallback("ends-at-the-right-edge", (62, 52, 178, 70), S, 1, (40, 30, 160, 70))
    fallback("one-pixel-past-the-right-edge", (62, 52, 179, 70), S, -3, (40, 30, 161, 70))
    fallback("bb2-is-a-max-the-roi-runs-to-the-edge", (62, 52, 100, 70), S, 1, (40, 30, 160, 70))
    fallback("ends-at-the-bottom-edge", (62, 78, 100, 90), S, 1, (40, 56, 160, 44))
    fallback("one-pixel-past-the-bottom-edge", (62, 79, 100, 90), S, -3, (40, 57, 160, 44))
    fallback("bb3-reads-det-1-not-det-3", (62, 52, 100, 500), S, 1, (40, 30, 160, 70))
    fallback("rw-zero", (222, 52, 100, 70), S, -3, (200, 30, 0, 70))
    fallback("rw-negative", (230, 52, 100, 70), S, -3, (208, 30, -8, 70))
    # rh = 0 needs y1 = y0: where f32 absorbs the margin.  At 2^30 the spacing is 64 below and 128 above, so y1 - 22 and y1 + 22
    # both round back to 2^30.  Then y0 > H, so the status alone cannot tell rh <= 0 from y0 + rh > H; the hook's ROI can.
    far = 2.0 ** 30
    assert F(far) - F(22.0) == F(far) and F(far) + F(22.0) == F(far) and int(F(far)) == 1073741824 < 2 ** 31
    fallback("rh-zero", (62, far, 100, 70), S, -3, (40, 1073741824, 160, 0))
    fallback("fractions-truncate", (62.75, 52.5, 100, 70), S, 1, (40, 30, 160, 70))
    fallback("clamped-at-zero", (10, 5, 100, 70), S, 1, (0, 0, 200, 100))
    f2 = coded_frame(40, 88)                                            # with no rounding of the margin rh >= 44 unless y0 is clamped at 0
    fallback("exact-2x2-small", (62, 10, 60, 60), (40, 88), 1, (40, 0, 48, 40), area_fast=1, crop=pc.mean_2x2(f2[:, 40:]))
    fallback("not-2x2-small", (62, 10, 60, 60), (41, 88), 1, (40, 0, 48, 41))
    f3 = coded_frame(254, 264)
    fallback("exact-2x2-224-for-112", (62, 52, 100, 100), (254, 264), 1, (40, 30, 224, 224), cfg="default", area_fast=1, crop=pc.mean_2x2(f3[30:, 40:]))
    fallback("not-2x2-224x225", (62, 52, 100, 100), (255, 264), 1, (40, 30, 224, 225), cfg="default")
    # ---- noise of +-1.5 px on 2 * template + (100, 50), default config: the decisions of a real face ----
    base = 2 * STANDARD + np.array([100, 50], np.float32)
    noise = (base + np.random.default_rng(1).uniform(-1.5, 1.5, (5, 2))).astype(np.float32)
    out.append(align_case("noisy-finite", noise, cfg="default", size=(300, 400), mask=noisy_mask("noisy-finite", noise, STANDARD), noisy=True))
    for tag, v in bad:
        kps = noise.copy()
        kps[2] = v
        mask = noisy_mask("noisy-" + tag, kps, STANDARD)
        assert mask == [True, True, False, True, True], (tag, mask)
        out.append(align_case("noisy-non-finite-" + tag, kps, cfg="default", size=(300, 400), mask=mask, noisy=True))
    names = [c["name"] for c in out]
    assert len(set(names)) == len(names) and not set(names) & set(NOT_CONSTRUCTIBLE)
    return out


def alignment_batch(cases, n):
    """n faces of one call under one config, cycled with a stride so that the status changes from face to face"""
    assert len({c["cfg"] for c in cases}) == 1
    stride = next(s for s in (7, 5, 3, 1) if np.gcd(s, len(cases)) == 1)
    picked = [cases[(i * stride) % len(cases)] for i in range(n)]
    for lo in range(0, n, 64):
        assert len({c["mode"] for c in picked[lo:lo + 64]}) >= (4 if lo + 64 <= n else 2)     # the last workgroup is partly filled
    return picked
