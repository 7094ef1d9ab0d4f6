"""Constructed inputs of the redaction (include/rfd.h, "redaction") with the answer WRITTEN DOWN from the construction, not computed
by tests/redact_ref.py: the restatement is held to them on the CPU (tests/test_redact_cpu.py) and both device forms on the GPU
(tests/test_redact_gpu.py).  A case: frame [H, W, 3] u8, rows (x1, y1, x2, y2, score), cfg fields over the default of the
restatement, want = the frame after the call, applied = the selected, non-skipped rows."""
import numpy as np

FILL, PIXELATE, RECT, ELLIPSE = 0, 1, 0, 1
NAN, INF = float("nan"), float("inf")
CASES = {}
PLAIN = dict(margin_x=0.0, margin_top=0.0, margin_bottom=0.0)          # the region is the box


def _case(name, frame, rows, cfg, want, applied):
    assert frame.dtype == np.uint8 and want.dtype == np.uint8 and frame.shape == want.shape
    CASES[name] = dict(frame=frame, rows=[list(r) + [0.9] for r in rows], cfg=cfg, want=want, applied=applied)


def _noise(seed, h, w):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)


def _art(rows):
    return np.array([[c == "X" for c in r] for r in rows])


# ---- a constant frame: any pixelation leaves it unchanged ----
_f = np.empty((20, 30, 3), np.uint8)
_f[:] = (7, 99, 201)
for _cell in (2, 3, 16):
    for _shape in (RECT, ELLIPSE):
        _case("constant_cell%d_shape%d" % (_cell, _shape), _f, [(4.5, 3.0, 22.0, 15.25), (10, 10, 29, 19)],
              dict(mode=PIXELATE, shape=_shape, cell=_cell), _f.copy(), 2)

# ---- a one-pixel checkerboard, cell 2, 9 x 11 with 255 where x + y is even: a whole 2 x 2 cell holds two 255s, (510 + 2) / 4 = 128; the
#      cells of column 10 are 1 x 2, (255 + 1) / 2 = 128; those of row 8 are 2 x 1, 128 as well; the corner cell is the pixel (8, 10)
#      alone, x + y even, (255 + 0) / 1 = 255 ----
_yy, _xx = np.mgrid[0:9, 0:11]
_f = np.repeat((((_xx + _yy) % 2 == 0) * 255).astype(np.uint8)[:, :, None], 3, axis=2)
_w = np.full((9, 11, 3), 128, np.uint8)
_w[8, 10] = 255
_case("checkerboard_cell2", _f, [(0, 0, 10, 8)], dict(PLAIN, mode=PIXELATE, shape=RECT, cell=2), _w, 1)

# ---- a cell cut by the frame edge: 5 x 7, cell 4; cell (1, 1) is the three pixels y = 4, x = 4 .. 6.  B 10 20 31: (61 + 1) / 3 = 20;
#      G 0 0 1: (1 + 1) / 3 = 0; R 255 255 254: (764 + 1) / 3 = 255.  The box covers the pixel (4, 5) alone ----
_f = _noise(1, 5, 7)
_f[4, 4:7, 0], _f[4, 4:7, 1], _f[4, 4:7, 2] = (10, 20, 31), (0, 0, 1), (255, 255, 254)
_w = _f.copy()
_w[4, 5] = (20, 0, 255)
_case("cell_cut_by_the_frame", _f, [(5.0, 4.0, 5.5, 4.5)], dict(PLAIN, mode=PIXELATE, shape=RECT, cell=4), _w, 1)

# ---- two overlapping boxes that share a cell: 8 x 8, cell 4; cell (0, 0) holds B 0 .. 15 ((120 + 8) / 16 = 8), G 100, R 255 but one 0
#      ((3825 + 8) / 16 = 239).  Box A covers x, y = 0 .. 1, box B x, y = 1 .. 2; the seven pixels of their union get the mean, in
#      either order ----
_f = _noise(2, 8, 8)
_f[0:4, 0:4, 0] = np.arange(16).reshape(4, 4)
_f[0:4, 0:4, 1] = 100
_f[0:4, 0:4, 2] = 255
_f[3, 2, 2] = 0
_w = _f.copy()
_w[0:2, 0:2] = (8, 100, 239)
_w[1:3, 1:3] = (8, 100, 239)
_A, _B = (0.0, 0.0, 1.5, 1.9), (1.25, 1.0, 2.0, 2.75)
_case("overlap_a_b", _f, [_A, _B], dict(PLAIN, mode=PIXELATE, shape=RECT, cell=4), _w, 2)
_case("overlap_b_a", _f, [_B, _A], dict(PLAIN, mode=PIXELATE, shape=RECT, cell=4), _w, 2)

# ---- ellipses pixel by pixel: dx = 2 i + 1 - w is 0 | -1 1 | -2 0 2 | -3 -1 1 3, covered iff dx^2 h^2 + dy^2 w^2 <= w^2 h^2.
#      A side of 1 makes its term 0, and 2 x 2 (4 + 4 <= 16), 3 x 3 (36 + 36 <= 81), 3 x 2 and 4 x 2 (36 + 16 <= 64) are full.  4 x 4
#      loses its corners (144 + 144 > 256, 144 + 16 <= 256), 4 x 3 too (81 + 64 > 144), 3 x 4 too (64 + 81 > 144).  8 x 8 is
#      dx^2 + dy^2 <= 64 over 49 25 9 1: the outer rows keep dx^2 <= 15, the next dx^2 <= 39 ----
ELLIPSES = {
    (1, 1): ["X"], (2, 1): ["XX"], (3, 1): ["XXX"], (4, 1): ["XXXX"],
    (1, 2): ["X", "X"], (1, 3): ["X", "X", "X"], (1, 4): ["X", "X", "X", "X"],
    (2, 2): ["XX", "XX"], (3, 2): ["XXX", "XXX"], (2, 3): ["XX", "XX", "XX"], (3, 3): ["XXX", "XXX", "XXX"],
    (4, 2): ["XXXX", "XXXX"], (2, 4): ["XX", "XX", "XX", "XX"],
    (4, 3): [".XX.", "XXXX", ".XX."], (3, 4): [".X.", "XXX", "XXX", ".X."],
    (4, 4): [".XX.", "XXXX", "XXXX", ".XX."],
    (8, 8): ["..XXXX..", ".XXXXXX.", "XXXXXXXX", "XXXXXXXX", "XXXXXXXX", "XXXXXXXX", ".XXXXXX.", "..XXXX.."],
}
for (_ew, _eh), _rows in ELLIPSES.items():
    _f = np.full((13, 14, 3), 200, np.uint8)
    _w = _f.copy()
    _w[2:2 + _eh, 3:3 + _ew][_art(_rows)] = (1, 2, 3)
    _case("ellipse_%dx%d" % (_ew, _eh), _f, [(3.0, 2.0, 3.0 + _ew - 1, 2.0 + _eh - 1)],
          dict(PLAIN, mode=FILL, shape=ELLIPSE, fill=(1, 2, 3)), _w, 1)

# ---- rows that are skipped: outside the frame on each side, inverted, an infinity or a NaN in each coordinate.  One good row among
#      them paints the pixel (1, 1); applied counts it alone ----
_f = _noise(3, 12, 16)
SKIPPED = [(16.0, 2, 20, 5), (2, 12.0, 5, 20), (-9, 2, -1.0, 5), (2, -9, 5, -1.0),               # right, below, left, above
           (5, 2, 4.5, 6), (2, 6, 5, 5.5)]                                                        # inverted in x, in y
for _k in range(4):
    for _bad in (NAN, INF, -INF):
        _r = [2.0, 3.0, 6.0, 7.0]
        _r[_k] = _bad
        SKIPPED.append(tuple(_r))
_w = _f.copy()
_w[1, 1] = (9, 8, 7)
_case("skipped_rows", _f, SKIPPED[:9] + [(1.0, 1.0, 1.5, 1.5)] + SKIPPED[9:], dict(PLAIN, mode=FILL, shape=RECT, fill=(9, 8, 7)), _w, 1)
_case("skipped_rows_alone", _f, SKIPPED, dict(PLAIN, mode=FILL, shape=ELLIPSE, fill=(9, 8, 7)), _f.copy(), 0)

# ---- margins that push the region past every frame side: 10 x 12, box 4, 4 .. 7, 6 (bw 3, bh 2) with margins 4: xa = 4 - 12, xb = 7 +
#      12, ya = 4 - 8, yb = 6 + 8: the whole frame ----
_f = _noise(4, 10, 12)
_w = np.empty_like(_f)
_w[:] = (0, 255, 17)
_case("margins_past_every_side", _f, [(4, 4, 7, 6)], dict(mode=FILL, shape=RECT, fill=(0, 255, 17), margin_x=4.0, margin_top=4.0, margin_bottom=4.0),
      _w, 1)
# margins alone: box 8, 8 .. 12, 12 (bw = bh = 4) with 0.25 / 0.5 / 0.75: xa = 7, xb = 13, ya = 6, yb = 15 in a 20 x 20 frame
_f = _noise(5, 20, 20)
_w = _f.copy()
_w[6:16, 7:14] = (5, 6, 7)
_case("margins_exact", _f, [(8, 8, 12, 12)], dict(mode=FILL, shape=RECT, fill=(5, 6, 7), margin_x=0.25, margin_top=0.5, margin_bottom=0.75), _w, 1)

# ---- truncation toward zero, W = 20: xa = -0.5 -> column 0 (not -1: the box -3.5 .. -0.5 still paints column 0); xa = 10.7 -> 10, xb =
#      12.2 -> 12; xa = W - 0.1 = 19.9 -> 19, the last column ----
_f = _noise(6, 4, 20)
for _name, _box, _cols in (("trunc_minus_half", (-0.5, 1.0, 2.9, 2.0), (0, 3)), ("trunc_left_of_zero", (-3.5, 1.0, -0.5, 2.0), (0, 1)),
                           ("trunc_10_7", (10.7, 1.0, 12.2, 2.0), (10, 13)), ("trunc_w_minus_tenth", (19.9, 1.0, 25.0, 2.0), (19, 20))):
    _w = _f.copy()
    _w[1:3, _cols[0]:_cols[1]] = (255, 0, 128)
    _case(_name, _f, [_box], dict(PLAIN, mode=FILL, shape=RECT, fill=(255, 0, 128)), _w, 1)


def check(name, out, applied):
    c = CASES[name]
    assert int(applied) == c["applied"], "%s: applied %d, written %d" % (name, applied, c["applied"])
    assert out.shape == c["want"].shape and out.tobytes() == c["want"].tobytes(), \
        "%s: differs from the written frame at (y, x, channel) %s" % (name, np.argwhere(out != c["want"])[:6].tolist())
