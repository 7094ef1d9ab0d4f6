"""tests/liveness_cases.py held against itself and against values worked by hand from the reference's formulas
(src/pipeline/module/face_antispoofing.rs, cited as :line).  No GPU, no library: the restatement tests/liveness_ref.py is the
judge of the device in tests/test_liveness_edges_gpu.py, so it is the restatement that is checked here."""
import collections
import time

import numpy as np

import liveness_cases as LC
import liveness_ref as R

f32 = np.float32
MAX, MIN = 2147483647, -2147483648


def test_every_class_is_reached_and_the_list_is_deterministic():
    for f in (LC.searched, LC.cases, LC.census):            # another test module of the session may have built the list already
        f.cache_clear()
    t0 = time.time()
    LC.cases()
    LC.census()                                             # the whole build: the search, and every case classified
    took = time.time() - t0
    table = LC.check()
    kept, samples, met = LC.searched()
    again = LC.searched.__wrapped__()                       # the search once more, uncached
    assert repr(again[0]) == repr(kept) and again[2] == met, "the seeded search is not deterministic"   # repr: a NaN box equals itself
    hand = [c for c in LC.cases() if c.origin == "hand"]
    assert LC.cases()[:len(hand)] == tuple(hand) and len(hand) >= 80
    print("%d cases (%d hand-written, %d of %d searched samples kept), built in %.1f s" % (len(LC.cases()), len(hand), len(kept), samples, took))
    assert took < 10.0, "the case list takes %.1f s to build" % took
    for k in LC.CLASSES:
        rows = table[k]
        print("%-28s %3d cases (%d hand-written) on %d frame sizes" % (k, len(rows), sum(o == "hand" for _, o, _ in rows), len({f for _, _, f in rows})))
    extra = sorted(set(table) - set(LC.CLASSES))
    print("also met:", {k: len(table[k]) for k in extra})
    print("not reached, by argument and by search:", LC.NEVER)
    assert len(LC.cases()) >= 200 and {(c.w, c.h) for c in LC.cases()} == set(LC.FRAMES)


def test_the_mutation_guards_bite():
    """every member of a cast class changes its ROIs or its status under the matching slip of the cast (that is the class's
    definition); here the same is shown once more from outside, for floor, on every frac0 / negfrac case of the list"""
    table = LC.census()
    n = 0
    for k, rows in table.items():
        if k.startswith("cast.") and k.rsplit(".", 1)[1] in ("frac0", "negfrac"):
            for i, _, _ in rows:
                c = LC.cases()[i]
                base, _ = LC.run(c)
                floor, _ = LC.run(c, cast=LC._only_at(k.split(".")[1], LC._cast_floor))
                assert floor["status"] != base["status"] or not np.array_equal(floor["rois"], base["rois"]), (k, c)
                n += 1
    print("floor instead of truncation changes %d (class, case) pairs" % n)
    assert n >= 40
    # and the guards are not vacuous the other way: on a tame box no mutant changes anything
    tame = LC.Case("tame", 320, 240, (100.0, 60.0, 180.0, 160.0), 1, "default", "hand")
    base, _ = LC.run(tame)
    for mutant in {m for ms in LC.MUTANT_OF.values() for m in ms}:
        r, _ = LC.run(tame, cast=mutant)
        assert r["status"] == base["status"] and np.array_equal(r["rois"], base["rois"])
    assert not LC._differs(tame, base, wrap=LC._span_saturating)


# ---- values worked by hand ----------------------------------------------------------------------------------------------------
# (case name, frame) -> (ROIs per model [ltx, lty, rbx, rby], weights per model, status).  The scales are those of the case's
# config: default 4, 2.7, 2, 1; three 1.5, 3, 0.5; one 1.
S27 = f32(2.7)
HAND = {
    # :253-262 dh = 1, c_x = -0.25, 0.47f * 1 = 0.47: left = (-0.72) as i32 = 0 (toward zero), right = 0.22 as i32 = 0:
    # Rect(0, 10, 1, 2).  :347 both ratios are large, scale = s.  Centre (0.5, 11), new box s x 2s.
    # s = 4: 0.5 - 2 < 0 -> right = 2.5 + 1.5 = 4, left = 0 (:358-361); rows 11 -+ 4.  s = 2.7: 0.5 - 1.35 < 0 -> right = 2.7 -> 2;
    # rows 8.3 .. 13.7.  s = 2: right = 1.5 + 0.5; rows 9 .. 13.  s = 1: 0.5 - 0.5 = 0 is not < 0: columns 0 .. 1, rows 10 .. 12
    ("left in (-1, 0)", (320, 240)): ([[0, 7, 4, 15], [0, 8, 2, 13], [0, 9, 2, 13], [0, 10, 1, 12]], [1, 1, 1, 1], 0),
    # dh = -1.0638, 0.47f * dh = -0.499986: left = 0.699986 as i32 = 0, right = (-0.299986) as i32 = 0, h = (-0.0638) as i32 = 0:
    # Rect(0, 10, 1, 0).  239 / 0 = +inf loses f32::min, scale = s; the new box is s wide and 0 high: the columns of the case
    # above, rows 10 .. 10
    ("right and h in (-1, 0)", (320, 240)): ([[0, 10, 4, 10], [0, 10, 2, 10], [0, 10, 2, 10], [0, 10, 1, 10]], [1, 1, 1, 1], 0),
    # dh = 40.5, 0.47f * 40.5 = 19.035: left = 100, right = 139, y = (-0.5) as i32 = 0, h = 41.5 as i32 = 41: Rect(100, 0, 40, 41),
    # centre (120, 20.5), scale = s.  1.5: 60 x 61.5: columns 90 .. 150; 20.5 - 30.75 < 0 -> bottom = 51.25 + 10.25 = 61.5 (:363-366).
    # 3: 120 x 123: columns 60 .. 180; 20.5 - 61.5 = -41 -> bottom = 82 + 41.  0.5: 20 x 20.5: 110 .. 130, 10.25 .. 30.75
    ("y in (-1, 0)", (320, 240)): ([[90, 0, 150, 61], [60, 0, 180, 123], [110, 10, 130, 30]], [1, 1, 1], 0),
    # dh = 43.5, 0.47f * 43.5 = 20.445: left = 99.555 -> 99, right = 140.445 -> 140, y = (-3.5) as i32 = -3, h = 44: Rect(99, -3, 42, 44),
    # centre (120, 19).  1.5: 63 x 66: 88.5 .. 151.5; 19 - 33 = -14 -> bottom = 52 + 14.  3: 126 x 132: 57 .. 183; 19 - 66 = -47 ->
    # bottom = 85 + 47.  0.5: 21 x 22: 109.5 .. 130.5, 8 .. 30
    ("y = -3.5", (200, 300)): ([[88, 0, 151, 66], [57, 0, 183, 132], [109, 8, 130, 30]], [1, 1, 1], 0),
    # c_x is NaN: left = right = NaN as i32 = 0 (:257-258), Rect(0, 150, 1, -120).  :347 scale = 239 / -120 = -1.99167 (negative, so
    # it wins); new box -1.99167 x 239; centre (0.5, 90): left = 0.5 + 0.99583 = 1.49583 -> 1, right = -0.49583 as i32 = 0;
    # 90 - 119.5 < 0 -> bottom = 209.5 + 29.5 = 239.  Rect(1, 0, 0, 240) :323 is empty: cv::resize :332 fails
    ("right_bottom_x in (-1, 0)", (320, 240)): ([[1, 0, 0, 239]], [0], -3),
    # the same on the portrait frame: Rect(0, 200, 1, -150), scale = 299 / -150, centre (0.5, 125): 125 - 149.5 < 0 -> bottom = 299
    ("right_bottom_x in (-1, 0)", (200, 300)): ([[1, 0, 0, 299]], [0], -3),
    # Rect(0, 100, 1, -9): scale = 239 / -9 = -26.5556, new box -26.5556 x 239, centre (0.5, 95.5): left = 13.78 -> 13,
    # right = -12.78 as i32 = -12 (toward zero); 95.5 - 119.5 = -24 -> bottom = 215 + 24 = 239.  Width -12 - 13 + 1 < 0
    ("NaN x, crop 1 x -9", (320, 240)): ([[13, 0, -12, 239]], [0], -3),
    # w1 = h1 = 0.  dh = -1: left = 5.47 -> 5, right = 4.53 -> 4, h = 0: Rect(5, 10, 0, 0); both ratios are 0 / 0 = NaN and
    # f32::min returns scale_ori (:347); the new box is the point (5, 10): 5 > 0 -> left = 5 - (5 - 1 + 1) = 0, right = 0
    # (:368-371), the same in y: the 1 x 1 frame itself, weight s / s
    ("0 / 0 twice", (1, 1)): ([[0, 0, 0, 0]] * 4, [1, 1, 1, 1], 0),
    # w1 = 0, h1 = 49.  dh = -2: left = 5.94 -> 5, right = 4.06 -> 4, h = -1: Rect(5, 10, 0, -1).  min(49 / -1, min(NaN, s)) = -49;
    # new box (0 * -49 = -0.0) x 49, centre (5, 9.5): 5 + -0.0 > 0 -> left = 5 - (5 - 1 + 1) = 0, right = 0; 9.5 - 24.5 < 0 ->
    # bottom = 34 + 15 = 49, not > 49: the whole frame, with NEGATIVE weights -49 / s (:383)
    ("0 / 0 beside 49 / -1", (1, 50)): ([[0, 0, 0, 49]] * 4, [f32(-49) / f32(4), f32(-49) / S27, f32(-49) / f32(2), f32(-49)], 0),
    # dh = 0.85, 0.47f * 0.85 = 0.3995: left = 1.5005 -> 1, right = 2.2995 -> 2, h = 1.85 -> 1: Rect(1, 0, 2, 1); 1 / 1 = 2 / 2 = 1
    # <= s: scale 1, new box 2 x 1, centre (2, 0.5): columns 1 .. 3, 3 > 2 -> left = 1 - (3 - 3 + 1) = 0, right = 2; rows 0 .. 1
    ("whole 3x2", (3, 2)): ([[0, 0, 2, 1]] * 4, [f32(1) / f32(4), f32(1) / S27, f32(1) / f32(2), 1], 0),
    # dh = -1.5, c_x = 28.5, 0.47f * dh = -0.705: left = 29.205 -> 29, right = 27.795 -> 27, h = (-0.5) as i32 = 0: Rect(29, 1, -1, 0).
    # min(0 / 0, min(49 / -1, s)) = -49: new box 49 x -0.0, centre (28.5, 1): columns 4 .. 53, 53 > 49 -> left = 4 - (53 - 50 + 1) = 0,
    # right = 49; 1 + -0.0 > 0 -> top = 1 - (1 - 1 + 1) = 0, bottom = 0
    ("whole 50x1", (50, 1)): ([[0, 0, 49, 0]] * 3, [f32(-49) / f32(1.5), f32(-49) / f32(3), f32(-49) / f32(0.5)], 0),
    # dh = 20: left = 20.6 -> 20, right = 39.4 -> 39: Rect(20, 20, 20, 21), centre (30, 30.5); 63 / 21 = 3.0 exactly, 63 / 20 = 3.15.
    # 1.5: 30 x 31.5: 15 .. 45, 14.75 .. 46.25.  3: min(3.0, min(3.15, 3.0)) is the tie: 60 x 63: 30 - 30 = 0 is not < 0: 0 .. 60;
    # 30.5 - 31.5 = -1 -> bottom = 62 + 1 = 63, not > 63.  0.5: 10 x 10.5: 25 .. 35, 25.25 .. 35.75
    ("tie 63 / 21 = 3.0", (64, 64)): ([[15, 14, 45, 46], [0, 0, 60, 63], [25, 25, 35, 35]], [1, 1, 1], 0),
    # c_x = -3e9, -+ 14.1 is below its step of 256: left = right = (-3e9) as i32 = i32::MIN (saturated), Rect(MIN, 10, 1, 31),
    # scale = s, centre (0.5 - 2^31 = -2^31, 25.5).  left = -2^31 - s / 2 = -2^31 < 0 -> right = -2^31 - -2^31 = 0, left = 0.
    # Rows: 4: 25.5 - 62 < 0 -> bottom = 87.5 + 36.5; 2.7: 31 * 2.7f = 83.7, 25.5 - 41.85 < 0 -> bottom = 83.7; 2: bottom = 62;
    # 1: 10 .. 41
    ("left / right saturate", (320, 240)): ([[0, 0, 0, 124], [0, 0, 0, 83], [0, 0, 0, 62], [0, 10, 0, 41]], [1, 1, 1, 1], 0),
    # left = right = 3e9 as i32 = i32::MAX, Rect(MAX, 10, 1, 31), center_x = 0.5 + 2^31 = 2^31 = left = right > 319:
    # right - 320 = 2147483328, a tie between 2147483264 and 2147483392 that goes to the even 2147483392; + 1 is lost;
    # left = 2^31 - 2147483392 = 256, right = 319 (:368-371).  Rows as above
    ("left / right saturate high", (320, 240)): ([[256, 0, 319, 124], [256, 0, 319, 83], [256, 0, 319, 62], [256, 10, 319, 41]], [1, 1, 1, 1], 0),
    # Rect(120, i32::MAX, 1, 1), scale = s, centre (120.5, 0.5 + 2^31 = 2^31).  Columns 120.5 -+ s / 2.  top = bottom = 2^31 > 239:
    # bottom - 240 = 2147483408 -> 2147483392 (steps of 128), + 1 is lost; top = 256, bottom = 239: height 239 - 256 + 1 = -16,
    # the only clause that fails
    ("y saturates high", (320, 240)): ([[118, 256, 122, 239], [119, 256, 121, 239], [119, 256, 121, 239], [120, 256, 121, 239]], [0, 0, 0, 0], -3),
    # Rect(120, i32::MIN, 1, 1), center_y = 0.5 - 2^31 = -2^31: top = -2^31 < 0 -> bottom = -2^31 - -2^31 = 0, top = 0: row 0
    ("y saturates low", (320, 240)): ([[118, 0, 122, 0], [119, 0, 121, 0], [119, 0, 121, 0], [120, 0, 121, 0]], [1, 1, 1, 1], 0),
    # dh = -6e9, 0.47f * dh = -2.82e9: left = i32::MAX, right = i32::MIN, width MIN - MAX + 1 = -2^32 + 2 wraps to 2, y = MAX,
    # h = (dh + 1) as i32 = i32::MIN: Rect(MAX, MAX, 2, MIN).  239 / -2^31 is negative and wins for every model; new box
    # (2 * that = -2.2e-7) x (exactly 239); centre (1 + 2^31 = 2^31, -2^30 + 2^31 = 2^30).  Columns as in the case above: 256 .. 319.
    # top = 2^30 - 119.5 -> 1073741696 (steps of 64), bottom = 2^30 + 119.5 -> 1073741952 (steps of 128) > 239:
    # bottom - 240 = 1073741712 -> 1073741696, + 1 is lost, top = 0, bottom = 239
    ("h saturates low", (320, 240)): ([[256, 0, 319, 239]] * 4, [f32(239) / f32(-2147483648) / s for s in (f32(4), S27, f32(2), f32(1))], 0),
    # dh = 2966889984 + 1602224256 = 4569114240 rounds to 4569114112 (steps of 512); 0.47f * dh = 2147483627.2 rounds to 2^31
    # (steps of 128 below it).  left = (126 - 2^31 -> -2147483520) , right = (126 + 2^31 -> 2^31) as i32 = i32::MAX,
    # width = MAX + 2147483520 + 1 = 2^32 - 128 wraps to -128 (:262), h = (dh + 1) as i32 = i32::MAX: Rect(-2147483520, -1602224256, -128, MAX).
    # :347 319 / -128 = -2.4921875 wins.  new box 319 x (2^31 * -2.4921875 = -5351931904).  center_x = -64 - 2147483520 = -2147483584,
    # a tie that rounds to -2^31; center_y = 2^30 - 1602224256 = -528482432.  left = -2^31 - 159.5 -> -2147483904 (steps of 256),
    # right = -2^31 + 159.5 -> -2147483520; left < 0 -> right = 384, left = 0; 384 > 319 -> left = -(384 - 320 + 1) = -65, right = 319.
    # top = -528482432 + 2675965952 = 2147483520 exactly: converted, NOT saturated; bottom = -528482432 - 2675965952 = -3204448384
    # -> i32::MIN.  x < 0: Mat::roi :324 fails
    ("left_top_y = 2147483520", (320, 240)): ([[-65, 2147483520, 319, MIN]] * 3, [0, 0, 0], -3),
    # the same family on the portrait frame: dh = 4569114112 exactly, 0.47f * dh -> 2^31; left = 99 - 2^31 -> -2147483520, right = i32::MAX,
    # width -128, y = (-3 * 2^30) as i32 = i32::MIN, h = i32::MAX.  199 / -128 = -1.5546875 wins: new box 199 x -3338665984.
    # center_x = -2147483584 -> -2^31, center_y = 2^30 - 2^31 = -2^30.  left = -2^31 - 99.5 -> -2^31 (steps of 256), right = -2^31 + 99.5
    # -> -2147483520: left < 0 -> right = 128, left = 0.  top = -2^30 + 1669332992 = 595591168, bottom = -2^30 - 1669332992 =
    # -2743074816 -> i32::MIN.  Rect(0, 595591168, 129, MIN - 595591168 + 1 -> wraps to +1551892481): only y + h > rows fails
    ("ROI height wraps to a positive number", (200, 300)): ([[0, 595591168, 128, MIN]] * 3, [0, 0, 0], -3),
    # y = 0: center_y = 2^30; top = 2^30 + 2675965952 = 3749707776 -> i32::MAX (saturated), bottom = 2^30 - 2675965952 = -1602224128;
    # columns as in the 2147483520 case above
    ("left_top_y above 2^31", (320, 240)): ([[-65, MAX, 319, -1602224128]] * 3, [0, 0, 0], -3),
    # dh = +inf: left = (-inf) as i32 = i32::MIN, right = i32::MAX, width 2^32 wraps to 0, y = (-0.5) as i32 = 0, h = i32::MAX:
    # Rect(MIN, 0, 0, MAX).  63 / 2^31 beats 63 / 0 = +inf and every s: new box 0 x (exactly 63), centre (-2^31, 2^30).
    # left = -2^31 < 0 -> right = 0, left = 0.  top = 2^30 - 31.5 -> 2^30 (steps of 64), bottom = 2^30 + 31.5 -> 2^30 > 63:
    # bottom - 64 = 1073741760, + 1 is lost: top = 64, bottom = 63: height 0, cv::resize :332 fails
    ("zero side, rejected", (64, 64)): ([[0, 64, 0, 63]] * 4, [0, 0, 0, 0], -3),
    # dh = 99, 0.47f * 99 = 46.53: left = 93.47 -> 93, right = 186.53 -> 186: Rect(93, -45, 94, 100), centre (140, 5).
    # 239 / 100 in f32: 239 * 2^22 / 100 = 10024386.56 rounds UP to q = 10024387 * 2^-22, and 100 * q = 239 + 44 * 2^-22 rounds to
    # 239 + 2^-16 (the step at 239; 44 is above half of 64).  s = 4 and 2.7 take q: half height 119.5 + 2^-17; top = 5 - that =
    # -114.5000076 and bottom = 124.5000076 are both exact (steps of 2^-17 below 128); top < 0 -> bottom = 239 + 2^-16, the smallest
    # excess over h1, top = 0 (:363-366); bottom > 239 -> top = 0 - (bottom - 240 + 1) = -2^-16, which `as i32` takes to 0 (floor: -1
    # and Mat::roi fails), bottom = 239 (:373-376).  Width 94 * 2.39 = 224.66: 140 -+ 112.33.  s = 2: 188 x 200: 46 .. 234;
    # 5 - 100 < 0 -> bottom = 105 + 95.  s = 1: 94 x 100: 93 .. 187; 5 - 50 < 0 -> bottom = 55 + 45
    ("new_height = 239 + 2^-16", (320, 240)): ([[27, 0, 252, 239], [27, 0, 252, 239], [46, 0, 234, 200], [93, 0, 187, 100]],
                                                [f32(239) / f32(100) / f32(4), f32(239) / f32(100) / S27, 1, 1], 0),
    # the same in x on the portrait frame (w1 = 199, h1 = 299).  dh = 98, 0.47f * 98 = 46.06: left = (27 - 46.06) as i32 = -19 (toward
    # zero), right = 73.06 -> 73: Rect(-19, 100, 93, 99), centre (27.5, 149.5).  199 * 2^22 / 93 = 8974908.559 rounds UP, and
    # 93 * q = 199 + 41 * 2^-22 rounds to 199 + 2^-16 (41 is above half of 64).  s = 4 and 2.7 take q (2.1398 < 299 / 99): left =
    # 27.5 - 99.5000076 = -72.0000076 and right = 127.0000076, both exact; left < 0 -> right = 199 + 2^-16, left = 0; right > 199 ->
    # left = -2^-16 -> 0, right = 199.  Height 99 * 2.1398 = 211.84: 149.5 -+ 105.92 = 43.58 .. 255.42.  s = 2: 186 x 198:
    # 27.5 - 93 < 0 -> right = 120.5 + 65.5 = 186; 50.5 .. 248.5.  s = 1: 27.5 - 46.5 = -19 -> right = 74 + 19; 100 .. 199
    ("new_width = 199 + 2^-16", (200, 300)): ([[0, 43, 199, 255], [0, 43, 199, 255], [0, 50, 186, 248], [0, 100, 93, 199]],
                                               [f32(199) / f32(93) / f32(4), f32(199) / f32(93) / S27, 1, 1], 0),
    # dh = -4, 0.47f * dh = -1.88: left = 100.88 -> 100, right = 97.12 -> 97, width 97 - 100 + 1 = -2, h = (-3.0) as i32 = -3:
    # Rect(100, 50, -2, -3).  299 / -3 = -99.6667 < 199 / -2 = -99.5: the height ratio wins; new box (-2 * -99.6667 = 199.3333) x
    # (299.0: 3 * 99.66666412 = 298.99999237 rounds to 299), centre (99, 48.5).  left = 99 - 99.6667 = -0.6667 < 0 -> right =
    # 198.6667 + 0.6667 = 199.3333, left = 0; 199.3333 > 199 -> left = 0 - (199.3333 - 200 + 1) = -0.3333 -> 0 (floor: -1), right = 199.
    # 48.5 - 149.5 = -101 -> bottom = 198 + 101 = 299, not > 299.  The whole frame, weight -99.6667 / 1
    ("left then right shift, left_top_x = -1/3", (200, 300)): ([[0, 0, 199, 299]], [f32(299) / f32(-3)], 0),
    # the same crop at y = 250: centre (99, 248.5): 248.5 - 149.5 = 99 is not < 0; 398 > 299 -> top = 99 - (398 - 300 + 1) = 0, bottom = 299
    ("left, right and bottom shift", (200, 300)): ([[0, 0, 199, 299]], [f32(299) / f32(-3)], 0),
    # dh = -89.5, 0.47f * dh = -42.065: left = 182.065 -> 182, right = 97.935 -> 97, width -84, h = (-88.5) as i32 = -88 (toward zero):
    # Rect(182, 100, -84, -88).  299 / -88 = -3.39773 < 199 / -84: new box (84 * 3.39773 = 285.409) x 299, centre (140, 56).
    # left = 140 - 142.7045 < 0 -> right = 282.7045 + 2.7045 = 285.409, left = 0; 56 - 149.5 < 0 -> bottom = 205.5 + 93.5 = 299;
    # 285.409 > 199 -> left = -(285.409 - 200 + 1) = -86.409 -> -86 (floor: -87), right = 199.  x < 0 is the only clause that fails
    ("negative sides, left_top_x = -86.4", (200, 300)): ([[-86, 0, 199, 299]], [0], -3),
    # dh = 40, c_x = -20.15, 0.47f * 40 = 18.8: left = -38.95 -> -38, right = -1.35 -> -1 (floor: -39 and -2): Rect(-38, 10, 38, 41),
    # scale 1, centre (-19, 30.5): left = -38 < 0 -> right = 0 + 38, left = 0; rows 10 .. 51
    ("left and right negative fractions", (320, 240)): ([[0, 10, 38, 51]], [1], 0),
    # w1 = h1 = 1.  dh = 1.1, 0.47f * 1.1f = 0.517: left = (-0.017) as i32 = 0, right = 1.017 -> 1, h = 2.1 -> 2: Rect(0, 0, 2, 2); both
    # ratios are 0.5 < s: new box 1 x 1, centre (1, 1): 0.5 .. 1.5, 1.5 > 1 -> left = 0.5 - (1.5 - 2 + 1) = 0, right = 1; the same in y
    ("whole 2x2", (2, 2)): ([[0, 0, 1, 1]] * 4, [f32(0.5) / f32(4), f32(0.5) / S27, f32(0.5) / f32(2), f32(0.5)], 0),
    # ymax = 2^31 + 256, dh = 384, 0.47f * 384 = 180.48: left = (120 - 180.48) as i32 = -60, right = 300: Rect(-60, 2147483520, 361, 385):
    # y is converted, not saturated.  239 / 385 = 0.62078 wins for every s; new box 224.10 x 239.  center_y = 192.5 + 2147483520 =
    # 2^31 + 64.5 -> 2^31 (steps of 256); top = 2^31 - 119.5 -> 2147483520 (steps of 128 below 2^31), bottom = 2^31 + 119.5 -> 2^31 > 239:
    # bottom - 240 = 2147483408 -> 2147483392, + 1 is lost; top = 2147483520 - 2147483392 = 128, bottom = 239.  (With y saturated
    # to i32::MAX center_y is 2^31 + 192.5 -> 2^31 + 256 and the top comes out at 256.)  Columns 120.5 -+ 112.05
    ("y = 2147483520, crop 385 high", (320, 240)): ([[8, 128, 232, 239]] * 4, [f32(239) / f32(385) / s for s in (f32(4), S27, f32(2), f32(1))], 0),
    # dh = 2147483520, dh + 1 rounds back to it: h = 2147483520 converted.  0.47f * dh = 1009317252.8 -> 1009317248 (steps of 64):
    # Rect(-1009317248, 0, 2018634497, 2147483520).  239 / 2147483520 wins; new box (2018634496 * that = 224.66) x 239; centre
    # (1009317248 - 1009317248 = 0, 2^30 - 64).  left = -112.33 < 0 -> right = 224.66, left = 0.  top = 1073741760 - 119.5 ->
    # 1073741632 (steps of 64), bottom = 1073741879.5 -> 2^30 (steps of 128) > 239: bottom - 240 = 1073741584 -> 1073741568, + 1 is
    # lost: top = 1073741632 - 1073741568 = 64, bottom = 239.  (With h saturated center_y is 2^30 and the top comes out at 0.)
    ("h = 2147483520, rows 64 .. 239", (320, 240)): ([[0, 64, 224, 239]] * 4, [f32(239) / f32(2147483520) / s for s in (f32(4), S27, f32(2), f32(1))], 0),
    # dh = -3e9 (the 10 is below its step of 256), h = (dh + 1) as i32 = i32::MIN; 0.47f * dh -> -1410000000: left = 1410000120 ->
    # 1410000128, right = -1409999880 -> -1409999872, width -2819999999 wraps to +1474967297: Rect(1410000128, 10, 1474967297, MIN).
    # 239 / -2^31 is negative and wins: new box (1474967296 * that = -164.15) x (exactly 239).  center_x = 737483648 + 1410000128 =
    # 2147483776, a tie that goes to 2^31; left = 2^31 + 82.08 -> 2^31, right = 2^31 - 82.08 -> 2147483520 > 319: right - 320 =
    # 2147483200, a tie that goes to 2147483136, + 1 is lost: left = 2^31 - 2147483136 = 512, right = 319.  center_y = -2^30 + 10 ->
    # -2^30; top = -2^30 - 119.5 -> -1073741952 (steps of 128), bottom = -2^30 + 119.5 -> -1073741696 (steps of 64); top < 0 ->
    # bottom = 256, top = 0; 256 > 239 -> top = -(256 - 240 + 1) = -17, bottom = 239.  y < 0 and width 319 - 512 + 1 < 0
    ("h saturates low over y = 10", (320, 240)): ([[512, -17, 319, 239]] * 4, [0, 0, 0, 0], -3),
    # Rect(2147483520, 10, 1, 1), left and right converted, not saturated.  center_x = 0.5 + 2147483520 -> 2147483520 = left = right
    # > 319: right - 320 = 2147483200, a tie that goes to the even 2147483136, + 1 is lost: left = 384, right = 319: width -64.
    # Rows 10.5 -+ s / 2
    ("left = right = 2147483520", (320, 240)): ([[384, 8, 319, 12], [384, 9, 319, 11], [384, 9, 319, 11], [384, 10, 319, 11]], [0, 0, 0, 0], -3),
    # the tall family with center_y = 0.  dh = 4071305728, 0.47f * dh = 1913513687.3 -> 1913513728 (steps of 128): left = 127 - that ->
    # -1913513600, right -> 1913513856, width 3827027457 wraps to -467939839, y = -2^30, h = i32::MAX.  199 / -467939840 wins;
    # new_height = 2^31 * 199 / -467939840 = -913.257, center_y = 2^30 - 2^30 = 0: top = 456.63 -> 456, bottom = -456.63 -> -456
    # (toward zero; floor: -457).  center_x = -233969920 - 1913513600 = -2147483520; left = that - 99.5 -> -2^31, right = that + 99.5 ->
    # -2147483392; left < 0 -> right = 256, left = 0; 256 > 199 -> left = -(256 - 200 + 1) = -57, right = 199.  x < 0 and h <= 0
    ("right_bottom_y = -456.x", (200, 300)): ([[-57, 456, 199, -456]] * 3, [0, 0, 0], -3),
    # the same with y = -2^30 + 448: dh = 3757300032 -> 3757299968 (steps of 256), 0.47f * dh = 1765930980.4 -> 1765931008:
    # left -> -1765930880, right -> 1765931136, width wraps to -763105279.  new_height = 2^31 * 319 / -763105280 = -897.71,
    # center_y = 448: top = 896.855 -> 896, bottom = -0.855 as i32 = 0 (floor: -1).  center_x = -381552640 - 1765930880 =
    # -2147483520; left = that - 159.5 -> -2^31, right = that + 159.5 -> -2147483392: right = 256, left = 0.  Only h <= 0 fails
    ("right_bottom_y in (-1, 0)", (320, 240)): ([[0, 896, 256, 0]] * 3, [0, 0, 0], -3),
}

# The cases tests/test_liveness_cpu.py works by hand are in the list under these names.  Their derivations stay in that file, which
# asserts them on the same restatement; the values it derives are held here too, per model where it derives one model only.
S101 = f32(239.0) / f32(101.0)
FROM_LIVENESS_CPU = {
    "known face": ({0: [28, 0, 252, 239], 1: [28, 0, 252, 239], 2: [45, 9, 235, 211], 3: [93, 60, 188, 161]}, [S101 / f32(4), S101 / S27, 1, 1], 0),
    "left": ({3: [0, 80, 57, 141]}, None, 0),
    "top": ({2: [102, 0, 218, 122]}, None, 0),
    "right": ({3: [261, 80, 319, 141]}, None, 0),
    "bottom": ({2: [102, 117, 218, 239]}, None, 0),
    "ymax < ymin": ({0: [0, -119, 319, 239]}, [0], -3),
    "zero sides, the point ROI": ({0: [140, 100, 140, 100]}, [1], 0),
    "NaN x": ({3: [0, 60, 1, 161]}, None, 0),
    "NaN y": ({3: [0, 0, 1, 0]}, None, 0),
    "taller than the frame": ({j: [48, 0, 272, 239] for j in range(4)}, [f32(239.0) / f32(801.0) / s for s in (f32(4), S27, f32(2), f32(1))], 0),
    "width wraps to 0": ({}, None, 0),
    "no face": ({j: [0, 0, 0, 0] for j in range(4)}, [0, 0, 0, 0], -2),
}


def test_hand_worked_values():
    by_key = {(c.name, (c.w, c.h)): c for c in LC.cases() if c.origin == "hand"}
    covered = set()
    for key, (rois, weights, status) in HAND.items():
        c = by_key[key]
        r, _ = LC.run(c)
        assert r["status"] == status, (key, r["status"])
        assert r["rois"].tolist() == rois, (key, r["rois"].tolist())
        assert np.array_equal(r["weights"].view(np.uint32), np.array(weights, np.float32).view(np.uint32)), (key, r["weights"].tolist())
        covered |= LC.classify(c)
    for name, (rois, weights, status) in FROM_LIVENESS_CPU.items():
        c = by_key[name, (320, 240)]
        r, _ = LC.run(c)
        assert r["status"] == status, (name, r["status"])
        for j, roi in rois.items():
            assert r["rois"][j].tolist() == roi, (name, j, r["rois"].tolist())
        if weights is not None:
            assert np.array_equal(r["weights"].view(np.uint32), np.array(weights, np.float32).view(np.uint32)), (name, r["weights"].tolist())
        covered |= LC.classify(c)
    rest = sorted(set(LC.CLASSES) - covered)
    print("%d of %d classes have a hand-worked case" % (len(LC.CLASSES) - len(rest), len(LC.CLASSES)))
    assert not rest, "classes without a hand-worked case: %s" % rest
    families = collections.Counter(k.split(".")[0] for k in covered)
    assert set(families) == {"cast", "wrap", "min", "shift", "edge", "roi", "zero_side", "found"}, families
    for kind in LC.MUTANT_OF:
        assert any(k.startswith("cast.") and k.endswith("." + kind) for k in covered), kind
