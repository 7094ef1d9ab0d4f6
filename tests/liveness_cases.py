"""Constructed inputs of the liveness stage (csrc/kernels_pre.hip: liveness_geometry_kernel, liveness_tensor_kernel), found and
classified on tests/liveness_ref.py alone.  Pure numpy: no oracle, no library, no GPU.

A case is (frame w, frame h, box, found, config); a class is a property of what the restatement does with the case, read off
the f32 values in front of every cast and every comparison (classify).  Hand-written cases come first; where a class needs a
particular rounding a seeded, bounded search over hostile boxes adds cases (searched()).  check() asserts that every class
of CLASSES is reached, and that none is held only by searched cases of a single frame size.

Classes (the names are the keys of the census that tests/test_liveness_cases_cpu.py prints):
  cast.<place>.<kind>   Rust's `as i32` at the crop box's left / right / y / h and at the four ROI corners.  kind: nan (-> 0),
                        max (>= 2^31 -> i32::MAX), min (<= -2^31 -> i32::MIN), big (2147483520, the largest f32 below 2^31,
                        converted and not saturated), frac0 (a value in (-1, 0) -> 0), negfrac (a negative value below -1
                        with a fraction).  A case counts for a class only if the matching MUTATION of the cast changes its
                        ROIs or its status: floor for frac0 / negfrac, a wrapping cast for max / min, NaN -> i32::MIN (what
                        cvttss2si leaves) or -> i32::MAX (what `!(f < 2^31)` leaves) for nan, saturation from 2147483520 on for big -- applied at THAT place alone, every
                        other cast left as Rust's (_only_at).  So every class member would catch that slip at that place.
  wrap.crop.zero / wrap.crop.negative   right - left + 1 leaves the i32 range and wraps to 0 / to a negative width; a case
                        counts only if a saturating subtraction would differ.  wrap.roi.w / wrap.roi.h: the same in the ROI's
                        own spans.
  min.*                 which operand f32::min returns: min.h / min.w / min.ori (strictly the smallest of the three), min.tie
                        (scale_ori equal to a ratio, and that value wins), min.negative, min.inf (a +inf ratio), min.one_nan
                        (one NaN ratio beside a finite one), min.both_nan.
  shift.<set>           the set of `if`s of _get_new_box that fired; shift.top+bottom.valid and shift.left+right.valid: both
                        shifts of an axis and still status 0.
  edge.*                right_bottom_x == w1 exactly (no shift) and one f32 step above (the smallest excess: shift); the same
                        for h1; left_top_x exactly +0.0 (no shift); edge.neg_zero_width: new_width = -0.0.
  roi.only.<clause>     a ROI rejected by exactly one clause of the rule; roi.x<0&h<=0 and roi.y<0&w<=0: the two pairs.
  roi.1x1, roi.1xfull, roi.last, roi.whole.<frame>   accepted ROIs at the rule's edges.
  zero_side.accepted / zero_side.rejected   a crop box with a zero side.
  found.0               no face.

Not reached, and not forced (NEVER; check() asserts that neither a hand-written case nor the search meets them, so that this
text stays true).  The search draws 8000 hostile boxes; a probe of 400000 more from the same generator found none either.
The arguments are about FRAMES, whose sides are at most 320: they use w1, h1 < 2^15.  The library itself does not limit a frame's
side to that, and on a frame with a side near 2^31 some of these classes may well be reachable; no such frame is tested.
  * cast.<ROI corner>.nan: scale is f32::min of scale_ori (finite and positive, checked by the library) and two ratios
    h1 / integer with h1 >= 0, so it is never NaN and never infinite; every corner is a sum of finite products.
  * cast.rbx.max / .big, cast.rby.max / .big: the two clamps leave right_bottom <= w1 (h1) < 2^15.
  * cast.ltx.max / .min / .big, cast.rbx.min, cast.lty.min: a corner beyond +-2^31 needs |new_width| (|new_height|) of that
    order.  new_height gets there through the crop's width wrapping while its height saturates (the last family of _draw);
    the crop's height only saturates and never wraps, so new_width stays below about max(w1, h1), and the y corner that
    would go below -2^31 is caught by the top shift first.
  * left_top_x == -0.0 in front of `< 0.0` (edge.ltx_neg_zero): a - b is -0.0 under round-to-nearest only for a = -0.0 and
    b = +0.0, and center_x = box_w / 2 + x is a sum of two i32 -> f32 conversions, which never give -0.0.  new_width = -0.0
    IS reachable: edge.neg_zero_width.
  * roi.only.x+w>cols (x + w > cols as the only failing clause): the clamp leaves right_bottom_x + 1 <= cols, so the clause
    can fire alone only when the ROI's width wraps to a positive number, which needs left_top_x near i32::MAX (above).
    Its partner roi.only.y+h>rows IS reached, by exactly that wrap, and is one of CLASSES.
"""
import collections
import functools

import numpy as np

import liveness_ref as R

f32 = np.float32
FRAMES = [(320, 240), (200, 300), (64, 64), (3, 2), (2, 2), (1, 50), (50, 1), (1, 1)]   # (w, h)
TINY = FRAMES[3:]

# the configs a case may name: small model inputs next to one of the default's sizes keep the oracle's resize cheap
CONFIGS = {
    "default": (R.DEFAULT_SCALES, [(8, 8), (5, 7), (80, 80), (6, 4)]),
    "three": ([1.5, 3.0, 0.5], [(5, 7), (8, 8), (4, 6)]),
    "one": ([1.0], [(9, 5)]),
}

Case = collections.namedtuple("Case", "name w h box found cfg origin")   # origin: "hand" or "search"

I32_MAX, I32_MIN = 2 ** 31 - 1, -2 ** 31
BIG = 2147483520.0   # 2^31 - 128


# ---- the mutations of the two integer rules -----------------------------------------------------------------------------
def _cast_floor(x):
    x = f32(x)
    return R.as_i32(x) if not np.isfinite(x) else R.as_i32(np.floor(x))


def _cast_wrapping(x):
    x = f32(x)
    return R.wrap_i32(int(x)) if np.isfinite(x) else 0


def _cast_nan_min(x):
    return I32_MIN if np.isnan(f32(x)) else R.as_i32(x)


def _cast_nan_max(x):
    return I32_MAX if np.isnan(f32(x)) else R.as_i32(x)


def _cast_early(x):
    return I32_MAX if f32(x) == f32(BIG) else R.as_i32(x)


def _span_saturating(v):
    return max(I32_MIN, min(I32_MAX, int(v)))


MUTANT_OF = dict(frac0=(_cast_floor,), negfrac=(_cast_floor,), max=(_cast_wrapping,), min=(_cast_wrapping,), nan=(_cast_nan_min, _cast_nan_max),
                 big=(_cast_early,))


PLACES = ("left", "right", "y", "h", "ltx", "lty", "rbx", "rby")


def _only_at(place, mutant):
    """a cast that is `mutant` at one place and Rust's everywhere else.  R.face casts in a fixed order: the crop's left, right, y
    and h once, then left_top_x, left_top_y, right_bottom_x, right_bottom_y for each model"""
    calls = [0]

    def cast(x):
        i = calls[0]
        calls[0] += 1
        here = PLACES[i] if i < 4 else PLACES[4 + (i - 4) % 4]
        return mutant(x) if here == place else R.as_i32(x)
    return cast


def _kind(v):
    v = f32(v)
    if np.isnan(v):
        return "nan"
    if v >= f32(2147483648.0):
        return "max"
    if v <= f32(-2147483648.0):
        return "min"
    if v == f32(BIG):
        return "big"
    if f32(-1.0) < v < f32(0.0):
        return "frac0"
    if v < f32(-1.0) and v != np.trunc(v):
        return "negfrac"
    return None


def run(case, **rules):
    """the restatement on a case (no pixels) -> (result dict, one trace per model)"""
    scales, sizes = CONFIGS[case.cfg]
    traces = []
    r = R.face(np.zeros((case.h, case.w, 3), np.uint8), case.box, case.found, scales, sizes, traces=traces, **rules)
    return r, traces


def _differs(case, base, **rules):
    r, _ = run(case, **rules)
    return r["status"] != base["status"] or not np.array_equal(r["rois"], base["rois"])


def classify(case):
    """-> the set of classes the case belongs to"""
    r, traces = run(case)
    if not (int(case.found) & 1):
        return {"found.0"}
    out = set()
    mutant = {}

    def visible(kind, place):
        if (kind, place) not in mutant:
            mutant[kind, place] = any(_differs(case, r, cast=_only_at(place, m)) for m in MUTANT_OF[kind])
        return mutant[kind, place]

    t0 = traces[0]
    for place, v in zip(("left", "right", "y", "h"), t0["crop"]):
        k = _kind(v)
        if k and visible(k, place):
            out.add("cast.%s.%s" % (place, k))
    left, right = R.as_i32(t0["crop"][0]), R.as_i32(t0["crop"][1])
    raw = right - left + 1
    if raw != R.wrap_i32(raw) and _differs(case, r, wrap=_span_saturating):
        out.add("wrap.crop.zero" if R.wrap_i32(raw) == 0 else "wrap.crop.negative" if R.wrap_i32(raw) < 0 else "wrap.crop.positive")
    bx, by, bw, bh = t0["bbox"]
    if bw == 0 or bh == 0:
        out.add("zero_side.accepted" if r["status"] == 0 else "zero_side.rejected")
    for j, t in enumerate(traces):
        for place, v in zip(("ltx", "lty", "rbx", "rby"), t["corners"]):
            k = _kind(v)
            if k and visible(k, place):
                out.add("cast.%s.%s" % (place, k))
        ltx, lty, rbx, rby = (int(v) for v in r["rois"][j])
        if rbx - ltx + 1 != t["rect"][2]:
            out.add("wrap.roi.w")
        if rby - lty + 1 != t["rect"][3]:
            out.add("wrap.roi.h")
        # f32::min
        rh, rw, so, sc = t["ratio_h"], t["ratio_w"], f32(CONFIGS[case.cfg][0][j]), t["scale"]
        nh, nw = np.isnan(rh), np.isnan(rw)
        if nh and nw:
            out.add("min.both_nan")
        elif nh != nw and np.isfinite(rw if nh else rh):
            out.add("min.one_nan")
        if np.isposinf(rh) or np.isposinf(rw):
            out.add("min.inf")
        if not nh and not nw:
            if rh < rw and rh < so:
                out.add("min.h")
            if rw < rh and rw < so:
                out.add("min.w")
            if so < rh and so < rw:
                out.add("min.ori")
            if sc == so and (rh == so or rw == so):
                out.add("min.tie")
        if sc < 0:
            out.add("min.negative")
        # the shifts and their thresholds
        sh = r["shifts"][j]
        out.add("shift." + ("+".join(sh) if sh else "none"))
        if r["status"] == 0:
            if "top" in sh and "bottom" in sh:
                out.add("shift.top+bottom.valid")
            if "left" in sh and "right" in sh:
                out.add("shift.left+right.valid")
        fx0, fy0, fx1, fy1 = t["first"]
        x1 = fx1 - fx0 if "left" in sh else fx1      # right_bottom_x in front of `> w1`
        y1 = fy1 - fy0 if "top" in sh else fy1
        with np.errstate(all="ignore"):
            if x1 == t["w1"]:
                out.add("edge.rbx_eq_w1")
            if x1 == np.nextafter(t["w1"], f32(np.inf)):
                out.add("edge.rbx_min_excess")
            if y1 == t["h1"]:
                out.add("edge.rby_eq_h1")
            if y1 == np.nextafter(t["h1"], f32(np.inf)):
                out.add("edge.rby_min_excess")
            if fx0 == 0 and not np.signbit(fx0):
                out.add("edge.ltx_pos_zero")
            if fx0 == 0 and np.signbit(fx0):
                out.add("edge.ltx_neg_zero")
            if bw == 0 and sc < 0:
                out.add("edge.neg_zero_width")
        # the ROI rule
        x, y, w, h = t["rect"]
        fails = [n for n, f in (("x<0", x < 0), ("y<0", y < 0), ("w<=0", w <= 0), ("h<=0", h <= 0), ("x+w>cols", x + w > case.w),
                                ("y+h>rows", y + h > case.h)) if f]
        if len(fails) == 1:
            out.add("roi.only." + fails[0])
        elif fails in (["x<0", "h<=0"], ["y<0", "w<=0"]):
            out.add("roi." + "&".join(fails))
        if not fails and r["status"] == 0:
            if (w, h) == (1, 1):
                out.add("roi.1x1")
            if w == 1 and h == case.h and case.h > 1:
                out.add("roi.1xfull")
            if x + w == case.w and y + h == case.h and (w, h) != (case.w, case.h):
                out.add("roi.last")
            if (x, y, w, h) == (0, 0, case.w, case.h) and (case.w, case.h) in TINY:
                out.add("roi.whole.%dx%d" % (case.w, case.h))
    return out


# ---- the classes that must be reached ---------------------------------------------------------------------------------------
_CROP, _ROI = ("left", "right", "y", "h"), ("ltx", "lty", "rbx", "rby")
CAST_UNREACHABLE = ({"cast.%s.nan" % p for p in _ROI} | {"cast.%s.%s" % (p, k) for p in ("rbx", "rby") for k in ("max", "big")} |
                    {"cast.ltx.max", "cast.ltx.min", "cast.ltx.big", "cast.lty.min", "cast.rbx.min"})
CLASSES = sorted(
    ({"cast.%s.%s" % (p, k) for p in _CROP + _ROI for k in MUTANT_OF} - CAST_UNREACHABLE) |
    {"wrap.crop.zero", "wrap.crop.negative"} |
    {"min." + m for m in ("h", "w", "ori", "tie", "negative", "inf", "one_nan", "both_nan")} |
    {"shift." + s for s in ("none", "left", "top", "right", "bottom", "left+top", "left+bottom", "top+right", "right+bottom",
                            "left+right", "left+top+right", "left+right+bottom", "left+top+bottom", "top+bottom.valid")} |
    {"edge." + e for e in ("rbx_eq_w1", "rbx_min_excess", "rby_eq_h1", "rby_min_excess", "ltx_pos_zero", "neg_zero_width")} |
    {"roi.only." + c for c in ("x<0", "y<0", "w<=0", "h<=0", "y+h>rows")} | {"roi.x<0&h<=0", "roi.y<0&w<=0"} |
    {"roi.1x1", "roi.1xfull", "roi.last"} | {"roi.whole.%dx%d" % f for f in TINY} |
    {"zero_side.accepted", "zero_side.rejected", "found.0"})
NEVER = sorted(CAST_UNREACHABLE | {"edge.ltx_neg_zero", "roi.only.x+w>cols"})


# ---- hand-written cases -------------------------------------------------------------------------------------------------------
def _hand():
    H = []

    def add(name, frame, box, found=1, cfg="default"):
        H.append(Case(name, frame[0], frame[1], tuple(float(v) for v in box), found, cfg, "hand"))

    big, port, sq = FRAMES[0], FRAMES[1], FRAMES[2]
    # the cases of test_liveness_cpu.py and test_liveness_gpu.py, on the device at last
    add("known face", big, (100, 60, 180, 160))
    add("left", big, (2, 80, 42, 140))
    add("top", big, (140, 2, 180, 62))
    add("right", big, (278, 80, 318, 140))
    add("bottom", big, (140, 178, 180, 238))
    add("ymax < ymin", big, (100, 100, 180, 90), cfg="one")
    add("zero sides, the point ROI", big, (100, 100, 180, 99), cfg="one")
    add("NaN x", big, (np.nan, 60, 180, 160))
    add("NaN y", big, (100, np.nan, 180, 160))
    add("taller than the frame", big, (0, -200, 320, 600))
    add("width wraps to 0", big, (0, 0, 0, 1e10))
    add("no face", big, (100, 60, 180, 160), found=0)
    add("no face, hostile box", port, (np.nan, np.inf, -np.inf, 1e10), found=0)
    # an exact tie of scale_ori = 2.0 with the height ratio: a frame 203 high is not in FRAMES, so the tie is made where
    # FRAMES allows it: 64 x 64, (64 - 1) / 21 = 3.0 with the config "three" (crop 21 high: ymax - ymin = 20)
    add("tie 63 / 21 = 3.0", sq, (20, 20, 40, 40), cfg="three")
    add("tie 299 / 299 = 1.0", port, (90, 0.5, 110, 298.75), cfg="one")
    # one NaN ratio beside a finite one: w1 = 0 on the 1 x 50 frame and a crop 0 wide (left = 5, right = 4)
    add("0 / 0 beside 49 / -1", FRAMES[5], (5, 10, 5, 8))
    add("0 / 0 beside 49 / 3", FRAMES[5], (0.25, 10, 0.25, 12))
    add("0 / 0 twice", FRAMES[7], (5, 10, 5, 9))
    add("negative zero width", big, (5, 10, 5, 8))
    add("negative zero width", port, (5, 10, 5, 8), cfg="three")
    # a NaN x makes the crop 1 wide (left = right = 0) whatever its height: the only way to a NEGATIVE new_width, and so to a
    # negative right_bottom_x in front of its cast
    add("NaN x, crop 1 x -9", big, (np.nan, 100, 0, 90), cfg="one")
    add("NaN x, crop 1 x -9", port, (np.nan, 100, 0, 90), cfg="one")
    add("NaN x, crop 1 x -255", sq, (np.nan, 10, 0, -246), cfg="one")
    # Boxes about 4.5e9 tall (see _draw's last family): the crop's height saturates, its width wraps to -128, the width ratio
    # w1 / -128 wins, new_height = 2^31 * w1 / -128 and center_y = 2^30 + ymin.  The first two put left_top_y on 2147483520
    # exactly; the third has left_top_y = 595591168 and right_bottom_y below -2^31, so that the ROI's height
    # i32::MIN - 595591168 + 1 leaves the i32 range downwards and wraps to +1551892481: y + h > rows is the ONLY clause that
    # rejects it (the kernel must not add y and h in 32 bits).
    add("left_top_y = 2147483520", big, (126.0, -1602224256.0, 126.0, 2966889984.0), cfg="three")
    add("left_top_y = 2147483520", port, (130.0, -595591296.0, 130.0, 3973522944.0), cfg="three")
    add("ROI height wraps to a positive number", port, (99.0, -3221225472.0, 99.0, 1347888640.0), cfg="three")
    # right_bottom_x one f32 step above w1 = 319 after the left shift (a rounding the search met; kept literally)
    add("right_bottom_x = 319 + 2^-15", big, (38.51584243774414, 425.85418701171875, -20.141263961791992, -199.04434204101562), cfg="one")
    # 2147483520 at the crop's y and h where the early-saturation mutant shows (met by the search; kept literally)
    add("y = 2147483520, visible", port, (3.3220481872558594, BIG, -1375783.375, 0.5))
    add("y = 2147483520, visible", sq, (58877936.0, BIG, 4821.0224609375, -4919111.5), cfg="one")
    add("h = 2147483520, visible", port, (-1e10, -0.5, -np.inf, BIG))
    add("h = 2147483520, visible", big, (3e9, -BIG, 1782020096.0, -0.5), cfg="three")
    # fractions in (-1, 0) and below -1 at the crop's casts, where truncation and floor give another crop:
    # left = -0.25 - 0.47 -> 0 (floor: -1, a crop 2 wide); right = 0.2 - 0.5 -> 0 and h = -0.0638 -> 0 (floor: -1);
    # y = -0.5 -> 0 and y = -3.5 -> -3 at scale 0.5, where no shift hides the row
    add("left in (-1, 0)", big, (-1, 10, 0.5, 11))
    add("right and h in (-1, 0)", big, (0.2, 10, 0.2, 8.9362))
    add("y in (-1, 0)", big, (100, -0.5, 140, 40), cfg="three")
    add("y = -3.5", port, (100, -3.5, 140, 40), cfg="three")
    # NaN x again, the crop 1 x -120 (-150): right_bottom_x = 0.5 + (239 / -120) / 2 = -0.4958 -> 0 (floor: -1)
    add("right_bottom_x in (-1, 0)", big, (np.nan, 150, 0, 29), cfg="one")
    add("right_bottom_x in (-1, 0)", port, (np.nan, 200, 0, 49), cfg="one")
    # the tall family again (met by the search; kept literally): right_bottom_y in (-1, 0), a negative fraction, and
    # right_bottom_y one f32 step above h1 after the top shift (both shifts of y, and still a valid ROI)
    add("right_bottom_y in (-1, 0)", big, (159.0, -1073741376.0, 159.0, 2683558656.0), cfg="three")
    add("right_bottom_y = -456.x", port, (127.0, -1073741824.0, 127.0, 2997563904.0), cfg="three")
    add("left_top_y above 2^31", big, (127.0, 0.0, 127.0, 4569114112.0), cfg="three")
    add("left_top_y above 2^31", port, (66.0, 595591168.0, 66.0, 5164705280.0), cfg="three")
    add("right_bottom_y = 239 + 2^-15", big, (39.615116119384766, -194.17477416992188, 188.0092315673828, 194.60365295410156), cfg="three")
    # the two pairs of failing clauses, and a rejected crop with a zero side (met by the search; kept literally)
    add("x < 0 and h <= 0", port, (130.0, -3221225472.0, 130.0, 282030560.0))
    add("x < 0 and h <= 0", sq, (-493967520.0, 1751320.875, 1353311.25, 1073741824.0), cfg="one")
    add("y < 0 and w <= 0", big, (-1570483.25, 17745.943359375, -BIG, -3e9))
    add("y < 0 and w <= 0", port, (-1484.7591552734375, -BIG, -24043540.0, -24379478016.0), cfg="one")
    add("zero side, rejected", sq, (51.23481750488281, -0.5, 16777216.0, np.inf))
    add("zero side, rejected", big, (-46209212.0, -1.0, 1650927616.0, -1.3151676654815674), cfg="three")
    # cases built so that tests/test_liveness_cases_cpu.py can work them by hand (the derivations are there):
    # 100 * fl(239 / 100) = 239 + 2^-16, the smallest excess over h1, reached exactly after the top shift; the same in x with
    # 93 * fl(199 / 93) = 199 + 2^-16; the issue's own example, a left then a right shift that leave left_top_x = -1/3, and its
    # mirror with the bottom shift; negative sides that leave left_top_x = -86.4; two negative fractions at the crop; the
    # whole 2 x 2 frame; 2147483520 at the crop's y and h where saturating one step early moves the rows; a saturated negative
    # height over a crop whose width wraps to a positive number
    add("new_height = 239 + 2^-16", big, (100, -45, 180, 54))
    add("new_width = 199 + 2^-16", port, (27, 100, 27, 198))
    add("left then right shift, left_top_x = -1/3", port, (99, 50, 99, 46), cfg="one")
    add("left, right and bottom shift", port, (99, 250, 99, 246), cfg="one")
    add("negative sides, left_top_x = -86.4", port, (100, 100, 180, 10.5), cfg="one")
    add("left and right negative fractions", big, (-30.3, 10, -10, 50), cfg="one")
    add("whole 2x2", FRAMES[4], (0, 0, 1, 1.1))
    add("y = 2147483520, crop 385 high", big, (100, BIG, 140, 2147483904.0))
    add("h = 2147483520, rows 64 .. 239", big, (0, 0, 0, BIG))
    add("h saturates low over y = 10", big, (100, 10, 140, -3e9))
    # the whole 3 x 2 frame: crop Rect(1, 0, 2, 1), every ratio 1.0, columns 1 .. 3 shifted left by one
    add("whole 3x2", FRAMES[3], (1.9, 0.1, 1.9, 0.95))
    # the whole 50 x 1 frame: crop Rect(29, 1, -1, 0): 0 / 0 beside 49 / -1, new_width = 49, columns 4 .. 53 shifted left by four
    add("whole 50x1", FRAMES[6], (-15.25, 1.75, 72.25, 0.25), cfg="three")
    # the whole frame, and a box outside it, on every tiny frame
    for fr in TINY:
        add("box covering %dx%d" % fr, fr, (0, 0, fr[0] - 1, fr[1] - 1))
        add("box far outside %dx%d" % fr, fr, (1000, 1000, 1040, 1060))
        add("box left above %dx%d" % fr, fr, (-90, -80, -50, -20), cfg="three")
    for fr in FRAMES[:3]:
        add("box covering %dx%d" % fr, fr, (0, 0, fr[0] - 1, fr[1] - 1))
        add("box far outside %dx%d" % fr, fr, (1000, 1000, 1040, 1060), cfg="three")
    # saturating casts at each crop place, with their plain neighbours
    for fr in (big, port):
        add("left / right saturate", fr, (-3e9, 10, -3e9, 40))
        add("left / right saturate high", fr, (3e9, 10, 3e9, 40))
        add("y saturates low", fr, (100, -3e9, 140, -3e9))
        add("y saturates high", fr, (100, 3e9, 140, 3e9))
        add("h saturates low", fr, (100, 3e9, 140, -3e9))
        add("y = 2147483520", fr, (100, BIG, 140, BIG))
        add("left = right = 2147483520", fr, (BIG, 10, BIG, 10))
        add("h = 2147483520", fr, (0, 0, 0, BIG - 128))
        add("infinite box", fr, (-np.inf, -np.inf, np.inf, np.inf))
    return H


# ---- the seeded search ---------------------------------------------------------------------------------------------------------
SEARCH_SEED, SEARCH_SAMPLES, KEEP_PER_CLASS_AND_FRAME = 20240607, 8000, 1
_SPECIAL = [0.0, -0.0, 0.5, -0.5, 1.0, -1.0, 2.0 ** 31, -2.0 ** 31, BIG, -BIG, 3e9, -3e9, 4.6e9, -4.6e9, 1e10, -1e10, 2.0 ** 24, 2.0 ** 30,
            np.inf, -np.inf, np.nan]


def _draw(rng, w, h):
    """one hostile box on a w x h frame"""
    mode = rng.integers(0, 9)
    if mode < 3:      # around the frame, on a quarter-pixel grid: exact ties and zero fractions happen
        x = np.round(rng.uniform(-0.6 * w - 2, 1.6 * w + 2, 2) * 4) / 4
        y = np.round(rng.uniform(-0.6 * h - 2, 1.6 * h + 2, 2) * 4) / 4
        box = [x.min(), y.min(), x.max(), y.max()]
        if rng.integers(0, 6) == 0:
            box[1], box[3] = box[3], box[1]
    elif mode < 5:    # arbitrary fractions
        x, y = rng.uniform(-w - 2, 2 * w + 2, 2), rng.uniform(-h - 2, 2 * h + 2, 2)
        box = [x[0], y[0], x[1], y[1]]
    elif mode == 5:   # small boxes near the frame's corners
        cx, cy = rng.choice([0.0, w - 1.0]), rng.choice([0.0, h - 1.0])
        d = rng.uniform(-3, 3, 4)
        box = [cx + d[0], cy + d[1], cx + d[2], cy + d[3]]
    elif mode == 6:   # huge and special coordinates
        box = [float(rng.choice(_SPECIAL)) if rng.integers(0, 2) else float(rng.uniform(-1, 1) * 2.0 ** rng.integers(1, 36))
               for _ in range(4)]
    elif mode == 7:   # a NaN x: left = right = 0, so the crop is 1 wide whatever its height; here the height is negative
        y = rng.uniform(-2.0, h + 2.0)
        box = [np.nan, y, rng.uniform(0, w), y - rng.uniform(1.0, 4.0 * h + 8.0)]
    else:
        # The family that takes huge values to the ROI's y corners: a box so tall that the crop's height saturates at
        # i32::MAX while its width 0.94 * height + 1 leaves the i32 range and wraps to a NEGATIVE number.  The width ratio is
        # then negative and wins f32::min, new_height = 2^31 * w1 / width is negative and large, and
        # center_y = 2^30 + (ymin as i32) is steered by ymin: towards 0, towards +-2^31, or so that
        # left_top_y = center_y - new_height / 2 lands near 2^31.
        c = float(rng.choice([0.0, 64.0, 128.0, w / 2.0])) + float(rng.integers(-2, 3))
        a = float(rng.choice([2.0 ** 30 * rng.uniform(1.0, 2.0), 2.0 ** 31 - 128.0 * rng.integers(0, 6)]))   # 0.47 * height
        bw = R.wrap_i32(R.as_i32(f32(c + a)) - R.as_i32(f32(c - a)) + 1)
        half = 2.0 ** 30 * (w - 1) / abs(bw) if bw < 0 else 0.0                                                  # |new_height| / 2
        aim = [0.0, 64.0 * rng.integers(-4, 5), half + 64.0 * rng.integers(-2, 3), -2.0 ** 31, 2.0 ** 30,
               2.0 ** 31 - half + 32.0 * rng.integers(-16, 17)][rng.integers(0, 6)]                              # center_y
        ymin = aim - 2.0 ** 30
        box = [c, ymin, c, ymin + a / 0.47]
    return tuple(float(f32(v)) for v in box)


@functools.lru_cache(maxsize=None)
def searched():
    """-> (cases, samples drawn, how often each class of CLASSES and of NEVER was met)"""
    rng = np.random.default_rng(SEARCH_SEED)
    kept, have, met = [], collections.Counter(), collections.Counter()
    wanted = set(CLASSES) | set(NEVER)
    cfgs = sorted(CONFIGS)
    for i in range(SEARCH_SAMPLES):
        w, h = FRAMES[i % len(FRAMES)]
        c = Case("searched %d" % i, w, h, _draw(rng, w, h), 1, cfgs[(i // len(FRAMES)) % len(cfgs)], "search")
        new = []
        for k in classify(c) & wanted:
            met[k] += 1
            if have[k, (w, h)] < KEEP_PER_CLASS_AND_FRAME:
                new.append(k)
        if new:
            kept.append(c)
            for k in new:
                have[k, (w, h)] += 1
    return tuple(kept), SEARCH_SAMPLES, met


@functools.lru_cache(maxsize=None)
def cases():
    """the whole list: hand-written cases, then the searched ones"""
    return tuple(_hand()) + searched()[0]


@functools.lru_cache(maxsize=None)
def census():
    """class -> list of (case index, origin, frame)"""
    table = collections.defaultdict(list)
    for i, c in enumerate(cases()):
        for k in classify(c):
            table[k].append((i, c.origin, (c.w, c.h)))
    return dict(table)


def check():
    """what the module asserts about itself -> the census"""
    table = census()
    missing = [k for k in CLASSES if k not in table]
    assert not missing, "classes without a case: %s" % missing
    for k in CLASSES:
        rows = table[k]
        hand = any(o == "hand" for _, o, _ in rows)
        assert hand or len({f for _, _, f in rows}) > 1, "class %s is held only by searched cases of one frame size: %s" % (k, rows)
    met = searched()[2]
    assert not [k for k in NEVER if k in table or met[k]], "a class recorded as unreachable was reached: %s" % [k for k in NEVER if k in table or met[k]]
    return table
