"""Constructed inputs of the annotation (include/rfd.h, "annotation") with the frame after the call WRITTEN DOWN from the
construction, not computed by tests/annotate_ref.py: the restatement is held to them on the CPU (tests/test_annotate_cpu.py) and
every form of the call on the GPU (tests/test_annotate_gpu.py).  The integer geometry of every case -- XA, YA, XB, YB, the mark
centres, PX, PY -- stands in the case as numbers; the helpers below only lay bands, discs given as half widths, and glyph bitmaps
at written positions.  The font is the library's (rfd_debug_annotate_glyph), so the cases are built by cases(font).

A case: frame [H, W, 3] u8; rows (x1, y1, x2, y2, score); lmk: per row five (x, y), missing = NaN; sel / label / value: per row
or None; count: None (the rows), an int, or "above" (more than max_det; the harness fills the unused rows with NaN boxes); cfg:
fields over PLAIN below; want = the frame after the call; applied = the drawn, non-skipped rows.

The list:
  outlines    outline_t1, outline_t2, outline_t16, box_1x1, box_thinner_than_2t, seam_63_64, seam_box_across, leaves_left,
              leaves_right, leaves_top, leaves_bottom, wholly_outside
  coordinates skipped_rows (NaN and +-inf in every coordinate, inverted in x and in y, a NaN product), box_3e9_left, box_3e9_all,
              trunc_minus_half, trunc_w_minus_tenth
  marks       mark_r1, mark_r2, mark_r8, mark_tile_corner, mark_outside_and_edge, mark_nan_landmark
  plate       plate_ya_minus_ph_0, plate_ya_minus_ph_minus_1, plate_px_negative, plate_past_right
  text        text_scale1_0, text_scale4_0, text_2147483647, text_question, text_dashes, text_100, text_999, text_7_50,
              round_below, round_at, round_above
  winner      winner_two_rows, winner_three_rows
  styles      style_first_match, style_no_match, sel_null, count_zero, count_negative, count_above
  alpha       alpha_1, alpha_128, alpha_255, alpha_256"""
import re

import numpy as np

NAMES = re.findall(r"[a-z0-9]+(?:_[a-z0-9]+)+", __doc__.split("The list:")[1])          # every case has an underscore in its name
NONE, ARRAY, SCORE = 0, 1, 2
MINUS, QUESTION, PERCENT, SPACE = 10, 11, 12, 13
NAN, INF = float("nan"), float("inf")
C1, C2, C3, TC = (10, 200, 30), (250, 5, 120), (0, 90, 255), (255, 255, 1)
# outline alone, in C1: no marks, no text
PLAIN = dict(styles=((0, 0, C1),), thickness=1, mark_radius=0, label_source=NONE, value_source=NONE, text_scale=1, text_colour=TC, alpha=256,
             margin_x=0.0, margin_top=0.0, margin_bottom=0.0)
F32 = np.float32
R8 = [0, 3, 5, 6, 6, 7, 7, 7, 8, 7, 7, 7, 6, 6, 5, 3, 0]     # half widths of dx^2 + dy^2 <= 64 for dy = -8 .. 8: 0 15 28 39 48 55 60 63 64
R2 = [0, 1, 2, 1, 0]                                        # <= 4: dy = +-2 -> dx = 0; +-1 -> dx^2 <= 3; 0 -> 2
R3 = [0, 2, 2, 3, 2, 2, 0]                                  # <= 9: dy = +-3 -> 0; +-2 -> dx^2 <= 5; +-1 -> dx^2 <= 8; 0 -> 3
R1 = [0, 1, 0]


def _noise(seed, h, w):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)


def _rect(w, x0, y0, x1, y1, c):
    """the pixels x0 .. x1, y0 .. y1 (inclusive) that lie in the frame"""
    H, W = w.shape[:2]
    x0, y0, x1, y1 = max(x0, 0), max(y0, 0), min(x1, W - 1), min(y1, H - 1)
    if x1 >= x0 and y1 >= y0:
        w[y0:y1 + 1, x0:x1 + 1] = c


def _outline(w, XA, YA, XB, YB, t, c):
    """four bands of t lines, each cut to the box"""
    _rect(w, XA, YA, XB, min(YA + t - 1, YB), c)
    _rect(w, XA, max(YB - t + 1, YA), XB, YB, c)
    _rect(w, XA, YA, min(XA + t - 1, XB), YB, c)
    _rect(w, max(XB - t + 1, XA), YA, XB, YB, c)


def _disc(w, cx, cy, half, c):
    r = len(half) // 2
    for dy in range(-r, r + 1):
        _rect(w, cx - half[dy + r], cy + dy, cx + half[dy + r], cy + dy, c)


def _label(w, font, glyphs, PX, PY, s, c, tc):
    """the plate of s (6 len + 1) x 9 s pixels at (PX, PY), then glyph k's bit (row v, column u) as an s x s square at
    (PX + s (1 + 6 k + u), PY + s (1 + v))"""
    _rect(w, PX, PY, PX + s * (6 * len(glyphs) + 1) - 1, PY + 9 * s - 1, c)
    for k, g in enumerate(glyphs):
        for v in range(7):
            for u in range(5):
                if (font[g][v] >> (4 - u)) & 1:
                    x, y = PX + s * (1 + 6 * k + u), PY + s * (1 + v)
                    _rect(w, x, y, x + s - 1, y + s - 1, tc)


def _digits(text):
    return ["0123456789-?% ".index(ch) for ch in text]


def cases(font):
    CASES = {}

    def case(name, frame, rows, cfg, want, applied, lmk=None, sel=None, label=None, value=None, count=None):
        assert frame.dtype == np.uint8 and want.dtype == np.uint8 and frame.shape == want.shape and name not in CASES
        rows = [list(r) + [0.9] * (5 - len(r)) for r in rows]
        marks = [[(NAN, NAN)] * 5 for _ in rows] if lmk is None else [list(m) + [(NAN, NAN)] * (5 - len(m)) for m in lmk]
        CASES[name] = dict(frame=frame, rows=rows, lmk=marks, sel=sel, label=label, value=value, count=count, cfg=dict(PLAIN, **cfg), want=want,
                           applied=applied)

    # ---- outlines ----
    f = _noise(1, 12, 16)                                     # XA 3, YA 2, XB 9, YB 7
    w = f.copy()
    w[2, 3:10] = w[7, 3:10] = C1
    w[2:8, 3] = w[2:8, 9] = C1
    case("outline_t1", f, [(3.0, 2.0, 9.5, 7.25)], {}, w, 1)
    f = _noise(2, 14, 16)                                     # 2, 2, 11, 10; t = 2
    w = f.copy()
    w[2:4, 2:12] = w[9:11, 2:12] = C1
    w[2:11, 2:4] = w[2:11, 10:12] = C1
    case("outline_t2", f, [(2.0, 2.0, 11.0, 10.0)], dict(thickness=2), w, 1)
    f = _noise(3, 50, 60)                                     # 5, 4, 54, 45; t = 16: x < 21 or x > 38 or y < 20 or y > 29
    w = f.copy()
    w[4:46, 5:55] = C1
    w[20:30, 21:39] = f[20:30, 21:39]
    case("outline_t16", f, [(5.0, 4.0, 54.0, 45.0)], dict(thickness=16), w, 1)
    f = _noise(4, 9, 11)                                      # 5, 4, 5, 4
    w = f.copy()
    w[4, 5] = C1
    case("box_1x1", f, [(5.2, 4.9, 5.8, 4.95)], {}, w, 1)
    f = _noise(5, 16, 12)                                     # 2, 2, 6, 12 with t = 3: five columns < 2 t, the outline fills the box
    w = f.copy()
    w[2:13, 2:7] = C1
    case("box_thinner_than_2t", f, [(2.0, 2.0, 6.0, 12.0)], dict(thickness=3), w, 1)
    f = _noise(6, 70, 70)                                     # 63, 63, 64, 64: one pixel in each of four tiles
    w = f.copy()
    w[63:65, 63:65] = C1
    case("seam_63_64", f, [(63.0, 63.0, 64.0, 64.0)], {}, w, 1)
    w = f.copy()                                              # 61, 61, 66, 66 with t = 2: the inner 63 .. 64 stays
    w[61:67, 61:67] = C1
    w[63:65, 63:65] = f[63:65, 63:65]
    case("seam_box_across", f, [(61.0, 61.0, 66.0, 66.0)], dict(thickness=2), w, 1)
    f = _noise(7, 20, 24)                                     # H 20, W 24: a box leaving a side draws no line along that side
    w = f.copy()                                              # -5, 5, 6, 10
    w[5, 0:7] = w[10, 0:7] = C1
    w[5:11, 6] = C1
    case("leaves_left", f, [(-5.0, 5.0, 6.0, 10.0)], {}, w, 1)
    w = f.copy()                                              # 18, 5, 30, 10
    w[5, 18:24] = w[10, 18:24] = C1
    w[5:11, 18] = C1
    case("leaves_right", f, [(18.0, 5.0, 30.0, 10.0)], {}, w, 1)
    w = f.copy()                                              # 5, -4, 10, 6
    w[6, 5:11] = C1
    w[0:7, 5] = w[0:7, 10] = C1
    case("leaves_top", f, [(5.0, -4.0, 10.0, 6.0)], {}, w, 1)
    w = f.copy()                                              # 5, 14, 10, 25
    w[14, 5:11] = C1
    w[14:20, 5] = w[14:20, 10] = C1
    case("leaves_bottom", f, [(5.0, 14.0, 10.0, 25.0)], {}, w, 1)
    case("wholly_outside", f, [(30.0, 30.0, 40.0, 40.0), (-40.0, 2.0, -30.0, 8.0)], {}, f.copy(), 2)      # drawn rows: they count

    # ---- coordinates ----
    f = _noise(8, 12, 16)
    skipped = [(5.0, 2.0, 4.5, 6.0), (2.0, 6.0, 5.0, 5.5),                                   # inverted in x, in y
               (-3.4e38, 2.0, 3.4e38, 5.0), (2.0, -3.4e38, 5.0, 3.4e38)]                     # bw, bh = +inf; inf * 0 = NaN
    for k in range(4):
        for bad in (NAN, INF, -INF):
            r = [2.0, 3.0, 6.0, 7.0]
            r[k] = bad
            skipped.append(tuple(r))
    w = f.copy()
    w[1, 1] = C1
    case("skipped_rows", f, skipped[:7] + [(1.0, 1.0, 1.5, 1.5)] + skipped[7:], {}, w, 1)
    w = f.copy()                                              # XA = -2^31, YA 2, XB 5, YB 4
    w[2, 0:6] = w[4, 0:6] = C1
    w[2:5, 5] = C1
    case("box_3e9_left", f, [(-3e9, 2.0, 5.0, 4.0)], {}, w, 1)
    case("box_3e9_all", f, [(-3e9, -3e9, 3e9, 3e9), (3e9, 1.0, 3e9, 5.0)], dict(thickness=16), f.copy(), 2)   # around and right of the frame
    f = _noise(9, 5, 20)                                      # W = 20
    w = f.copy()                                              # xa = -0.5 -> XA 0 (not -1): the left line IS column 0; XB 2
    w[1, 0:3] = w[3, 0:3] = C1
    w[1:4, 0] = w[1:4, 2] = C1
    case("trunc_minus_half", f, [(-0.5, 1.0, 2.9, 3.0)], {}, w, 1)
    w = f.copy()                                              # xb = W - 0.1 = 19.9 -> XB 19, the last column; XA 17
    w[1, 17:20] = w[3, 17:20] = C1
    w[1:4, 17] = w[1:4, 19] = C1
    case("trunc_w_minus_tenth", f, [(17.2, 1.0, 19.9, 3.0)], {}, w, 1)

    # ---- marks (no outline; the box is elsewhere) ----
    M = dict(thickness=0)
    f = _noise(10, 30, 40)
    w = f.copy()                                              # centres 5, 4 and 20, 10 (7.9 -> 7: 17.9, 12.9 -> 17, 12)
    _disc(w, 5, 4, R1, C1)
    _disc(w, 17, 12, R1, C1)
    case("mark_r1", f, [(30.0, 20.0, 35.0, 25.0)], dict(M, mark_radius=1), w, 1, lmk=[[(5.0, 4.5), (17.9, 12.9)]])
    w = f.copy()
    _disc(w, 5, 4, R2, C1)
    _disc(w, 17, 12, R2, C1)
    case("mark_r2", f, [(30.0, 20.0, 35.0, 25.0)], dict(M, mark_radius=2), w, 1, lmk=[[(5.0, 4.5), (17.9, 12.9)]])
    w = f.copy()
    _disc(w, 12, 11, R8, C1)
    case("mark_r8", f, [(30.0, 20.0, 35.0, 25.0)], dict(M, mark_radius=8), w, 1, lmk=[[(12.0, 11.0)]])
    f = _noise(11, 70, 70)
    w = f.copy()
    _disc(w, 64, 64, R2, C1)                                  # pixels of all four tiles
    _disc(w, 63, 0, R2, C1)
    case("mark_tile_corner", f, [(1.0, 1.0, 3.0, 3.0)], dict(M, mark_radius=2), w, 1, lmk=[[(64.0, 64.0), (63.5, 0.0)]])
    f = _noise(12, 9, 9)
    w = f.copy()
    w[0, 0] = w[0, 1] = w[1, 0] = C1                          # centre 0, 0; the centres -10, 5 and 8, 20 and 2^31 - 1, 3 paint nothing
    w[8, 8] = C1                                              # centre x 9, y 8 in a 9 x 9 frame: the pixel x 8, y 8 alone (dx = -1)
    case("mark_outside_and_edge", f, [(1.0, 1.0, 3.0, 3.0)], dict(M, mark_radius=1), w, 1,
         lmk=[[(0.0, 0.0), (-10.0, 5.0), (8.0, 20.0), (3e9, 3.0), (9.0, 8.0)]])
    f = _noise(13, 12, 12)
    w = f.copy()
    _disc(w, 6, 6, R1, C1)
    case("mark_nan_landmark", f, [(1.0, 1.0, 3.0, 3.0)], dict(M, mark_radius=1), w, 1,
         lmk=[[(NAN, 5.0), (5.0, INF), (6.0, 6.0), (-INF, NAN), (NAN, NAN)]])

    # ---- plate and text (no outline, no marks): label = ARRAY, the plate in C2, the text in TC ----
    T = dict(thickness=0, label_source=ARRAY, styles=((0, 0, C2),))
    f = _noise(14, 30, 40)
    for name, ya, py in (("plate_ya_minus_ph_0", 9, 0), ("plate_ya_minus_ph_minus_1", 8, 8), ("text_scale1_0", 12, 3)):
        w = f.copy()                                          # s = 1, len 1: PW 7, PH 9; PY = YA - 9 if that is >= 0, else YA
        _label(w, font, [0], 4, py, 1, C2, TC)
        case(name, f, [(4.0, float(ya), 30.0, 25.0)], T, w, 1, label=[0])
    w = f.copy()                                              # PX = -3: columns 0 .. 3 of the plate of 7
    _label(w, font, [8], -3, 3, 1, C2, TC)
    case("plate_px_negative", f, [(-3.0, 12.0, 20.0, 20.0)], T, w, 1, label=[8])
    w = f.copy()                                              # PX = 36 of W = 40: four columns
    _label(w, font, [4], 36, 3, 1, C2, TC)
    case("plate_past_right", f, [(36.0, 12.0, 50.0, 20.0)], T, w, 1, label=[4])
    f = _noise(15, 50, 40)
    w = f.copy()                                              # s = 4: PW 28, PH 36; YA 40 -> PY 4
    _label(w, font, [0], 5, 4, 4, C2, TC)
    case("text_scale4_0", f, [(5.0, 40.0, 30.0, 45.0)], dict(T, text_scale=4), w, 1, label=[0])
    f = _noise(16, 24, 70)
    w = f.copy()                                              # ten glyphs: PW 61, across the tile seam at x = 64
    _label(w, font, _digits("2147483647"), 6, 3, 1, C2, TC)
    case("text_2147483647", f, [(6.0, 12.0, 30.0, 20.0)], T, w, 1, label=[2147483647])
    w = f.copy()
    _label(w, font, [QUESTION], 6, 3, 1, C2, TC)
    case("text_question", f, [(6.0, 12.0, 30.0, 20.0)], T, w, 1, label=[-1])
    V = dict(thickness=0, value_source=ARRAY, styles=((0, 0, C2),), text_scale=2)
    for name, v, text in (("text_dashes", NAN, "--%"), ("text_100", 1.0, "100%"), ("text_999", 50.0, "999%"),
                          # 0.005f * 100 rounds to 0.5 exactly, one ulp less to 0.49999994: + 0.5 gives 1.0 and 0.99999994
                          ("round_below", float(np.nextafter(F32(0.005), F32(0))), "0%"), ("round_at", 0.005, "1%"),
                          ("round_above", float(np.nextafter(F32(0.005), F32(1))), "1%")):
        w = f.copy()                                          # s = 2: PH 18; YA 20 -> PY 2
        _label(w, font, _digits(text), 3, 2, 2, C2, TC)
        case(name, f, [(3.0, 20.0, 30.0, 22.0)], V, w, 1, value=[v])
    w = f.copy()
    _label(w, font, _digits("7 50%"), 3, 2, 2, C2, TC)
    case("text_7_50", f, [(3.0, 20.0, 30.0, 22.0)], dict(V, label_source=ARRAY), w, 1, label=[7], value=[0.5])

    # ---- winner: the rows are laid from the last to the first, each with its four layers in order, by the helpers above ----
    WIN = dict(styles=((3, 0, C1), (3, 1, C2), (0, 0, C3)), thickness=3, mark_radius=3, label_source=ARRAY, text_scale=2)
    f = _noise(17, 80, 90)
    geo = [  # XA, YA, XB, YB, the label, the five mark centres; the plate is PX = XA, PY = YA - 18
        (20, 30, 40, 50, 88, [(26, 36), (44, 31), (27, 38), (21, 40), (60, 70)]),
        (23, 33, 43, 53, 88, [(21, 31), (27, 37), (24, 14), (29, 17), (39, 33)]),
        (30, 20, 60, 60, 11, [(26, 35), (40, 51), (70, 70), (70, 70), (70, 70)]),
    ]

    def lay(w, rows):
        for i in reversed(rows):
            XA, YA, XB, YB, lab, marks = geo[i]
            c = (C1, C2, C3)[i]
            _outline(w, XA, YA, XB, YB, 3, c)
            for cx, cy in marks:
                _disc(w, cx, cy, R3, c)
            if YA - 18 >= 0:
                _label(w, font, _digits(str(lab)), XA, YA - 18, 2, c, TC)
            else:
                _label(w, font, _digits(str(lab)), XA, YA, 2, c, TC)
    for name, rows in (("winner_two_rows", [0, 1]), ("winner_three_rows", [0, 1, 2])):
        w = f.copy()
        lay(w, rows)
        case(name, f, [tuple(float(v) for v in geo[i][:4]) for i in rows], WIN, w, len(rows), label=[geo[i][4] for i in rows],
             lmk=[[(float(x), float(y)) for x, y in geo[i][5]] for i in rows], sel=[i for i in rows])

    # ---- styles and counts ----
    f = _noise(18, 12, 30)
    boxes = [(1.0, 1.0, 5.0, 5.0), (11.0, 1.0, 15.0, 5.0), (21.0, 1.0, 25.0, 5.0)]
    w = f.copy()                                              # words 1, 0, 3 against {mask 1 value 1: C2}, {every word: C3}
    _outline(w, 1, 1, 5, 5, 1, C2)
    _outline(w, 11, 1, 15, 5, 1, C3)
    _outline(w, 21, 1, 25, 5, 1, C2)
    case("style_first_match", f, boxes, dict(styles=((1, 1, C2), (0, 0, C3))), w, 3, sel=[1, 0, 3])
    w = f.copy()                                              # the word 0 matches no style: not drawn, not counted
    _outline(w, 1, 1, 5, 5, 1, C2)
    _outline(w, 21, 1, 25, 5, 1, C3)
    case("style_no_match", f, boxes, dict(styles=((1, 1, C2), (2, 2, C3))), w, 2, sel=[1, 0, 2])
    w = f.copy()                                              # sel NULL: every word is 0, which {mask 1 value 0} matches and {1, 1} does not
    for x in (1, 11, 21):
        _outline(w, x, 1, x + 4, 5, 1, C3)
    case("sel_null", f, boxes, dict(styles=((1, 1, C2), (1, 0, C3))), w, 3)
    case("count_zero", f, boxes, {}, f.copy(), 0, count=0)
    case("count_negative", f, boxes, {}, f.copy(), 0, count=-3)
    w = f.copy()
    for x in (1, 11, 21):
        _outline(w, x, 1, x + 4, 5, 1, C1)
    case("count_above", f, boxes, {}, w, 3, count="above")

    # ---- alpha: source (200, 100, 0) under (0, 255, 255): (a C + (256 - a) P + 128) >> 8 ----
    f = np.empty((8, 8, 3), np.uint8)
    f[:] = (200, 100, 0)
    for a, px in ((1, (199, 101, 1)),            # (51000 + 128) >> 8, (255 + 25500 + 128) >> 8, (255 + 128) >> 8
                  (128, (100, 178, 128)),        # (25600 + 128) >> 8, (32640 + 12800 + 128) >> 8, (32640 + 128) >> 8
                  (255, (1, 254, 254)),          # (200 + 128) >> 8, (65025 + 100 + 128) >> 8, (65025 + 128) >> 8
                  (256, (0, 255, 255))):
        w = f.copy()
        _outline(w, 2, 2, 5, 5, 1, px)
        case("alpha_%d" % a, f, [(2.0, 2.0, 5.0, 5.0)], dict(styles=((0, 0, (0, 255, 255)),), alpha=a), w, 1)
    return CASES


def check(cases_, name, out, applied):
    c = cases_[name]
    assert int(applied) == c["applied"], "%s: applied %d, written %d" % (name, applied, c["applied"])
    assert out.shape == c["want"].shape and out.tobytes() == c["want"].tobytes(), \
        "%s: differs from the written frame at (y, x, channel) %s" % (name, np.argwhere(out != c["want"])[:6].tolist())
