"""Constructed inputs of the shot quality (include/rfd.h, "shot quality") with the answer written down from the construction,
not from a run.  A case is dict(frame HxWx3 u8, box [5], lmk [10], cfg fields, want): `want` names parts, "q", "status", "A1",
"A2", "m" (one value every cell mean must have) or "region" with the value that follows from how the frame was made.
tests/test_shot_quality_cpu.py holds the restatement to them, tests/test_shot_quality_gpu.py the library."""
import numpy as np

F = np.float32
STANDARD = [38.2946, 51.6963, 73.5318, 51.5014, 56.0252, 71.7366, 41.5493, 92.3655, 70.7299, 92.2041]   # the 112 x 112 alignment template
# lx 0, rx 4: d = 4; nx 2: yaw 0; ly 0, ry 1: roll 0.25; ey 0.5, my 4.5: v = 4; ny 2.5: (ny - ey) / v = 0.5 = pitch0 below: pitch 0
QUARTER_ROLL = [0, 0, 4, 1, 2, 2.5, 0, 4.5, 4, 4.5]
HALF_CFG = dict(pitch0=0.5)    # with QUARTER_ROLL: t = 0.25, pose = 0.75, all exact
NAN, INF = float("nan"), float("inf")
I32_MIN = -2**31


def grey_frame(g):
    """an HxW array of grey levels as a BGR frame with B = G = R, whose grey is the level itself: (v * 16384 + 8192) >> 14 = v"""
    return np.repeat(np.asarray(g, np.uint8)[:, :, None], 3, axis=2).copy()


def whole(frame, score=0.875):
    h, w = frame.shape[:2]
    return [0, 0, w - 1, h - 1, score]


CASES = {}


def case(name, frame, box, want, lmk=QUARTER_ROLL, **cfg):
    assert name not in CASES
    CASES[name] = dict(frame=frame, box=[float(x) for x in box], lmk=[float(x) for x in lmk], cfg=cfg, want=want)


# ---- a constant frame: every mean is 16 v, no Laplacian; expo at the thresholds.  128 x 128: cells of 4 x 4 = 16 pixels, so one
#      pixel of a cell moved by delta moves m = (16 S + 8) / 16 = S by delta: m = 16 * 30 - 1, 16 * 30, 16 * 30 + 1 ----
def _const(v, delta):
    g = np.full((128, 128), v, np.int64)
    g[::4, ::4] += delta
    return grey_frame(g)


for v, delta, expo in ((30, -1, 0.0), (30, 0, 0.0), (30, 1, 1.0), (225, -1, 1.0), (225, 0, 0.0), (225, 1, 0.0)):
    f = _const(v, delta)
    case("constant_%d_%+d" % (v, delta), f, whole(f), dict(m=16 * v + delta, sharp=0.0, A1=0, A2=0, mean=v + delta / 16.0, expo=expo, status=0, size=128.0,
                                                            pose=0.75, q=0.0), **HALF_CFG)     # sharp 0: q 0 whatever the rest
f = _const(128, 0)
f[:4] = 0                                           # the top row of cells is black: 32 of 1024 cells are dark
case("one_dark_row_of_cells", f, whole(f), dict(expo=1.0 - 32.0 / 1024.0, status=0))
f = _const(100, 0)
case("thresholds_from_the_config", f, whole(f), dict(expo=0.0, m=1600), dark=100, bright=101)
case("thresholds_from_the_config_above", f, whole(f), dict(expo=1.0, m=1600), dark=99, bright=101)

# ---- a pixel checkerboard under a 32 x 32 box: a cell is a pixel, m is 0 or 4080, every interior L is +-4 * 4080 = +-16320, 450 of
#      each sign: A1 = 0, A2 = 900 * 16320^2, sharp = 900 * A2 / 207360000 = 16320^2 / 256 = 1040400.  Every cell is dark or bright ----
yy, xx = np.mgrid[0:48, 0:48]
f = grey_frame(((yy + xx) & 1) * 255)
case("pixel_checkerboard", f, [8, 8, 39, 39, 0.875], dict(sharp=1040400.0, A1=0, A2=900 * 16320 * 16320, expo=0.0, mean=127.5, size=32.0, status=0, q=0.0))

# ---- one bright cell on black: L = 16320 at the cell, -4080 at its four neighbours: A1 = 0, A2 = 16320^2 + 4 * 4080^2 =
#      332928000, sharp = 900 * 332928000 / 207360000 = 1445 ----
g = np.zeros((32, 32), np.int64)
g[10, 20] = 255
f = grey_frame(g)
case("one_bright_cell", f, whole(f), dict(sharp=1445.0, A1=0, A2=332928000, mean=4080.0 / 16384.0, expo=0.0, status=0))
# at the rim of the grid the cell is no interior cell and only one neighbour sees it: A1 = -4080, A2 = 4080^2
g = np.zeros((32, 32), np.int64)
g[0, 5] = 255
f = grey_frame(g)
case("one_bright_cell_at_the_rim", f, whole(f), dict(A1=-4080, A2=4080 * 4080, sharp=(900 * 4080 * 4080 - 4080 * 4080) / 207360000.0, status=0))

# ---- a horizontal ramp: m is linear in the column, so every L is 0.  32 wide: grey 8 x.  64 wide: cells of two pixels 4 x, 4 x + 4
#      ... = grey 2 * column, the pair (4c, 4c + 2) has S = 8 c + 2, m = (16 S + 1) / 2 = 64 c + 16 ----
f = grey_frame(np.tile(np.arange(32) * 8, (32, 1)))
case("ramp_32", f, whole(f), dict(sharp=0.0, A1=0, A2=0, status=0))
f = grey_frame(np.tile(np.arange(64) * 2, (40, 1)))
case("ramp_64", f, whole(f), dict(sharp=0.0, A1=0, A2=0, status=0, size=40.0))

# ---- grey weights: (255 * 1868 + 8192) >> 14 = 29, (255 * 9617 + 8192) >> 14 = 150, (255 * 4899 + 8192) >> 14 = 76, white 255 ----
for name, bgr, g in (("blue", (255, 0, 0), 29), ("green", (0, 255, 0), 150), ("red", (0, 0, 255), 76), ("white", (255, 255, 255), 255)):
    f = np.zeros((40, 40, 3), np.uint8)
    f[:] = bgr
    case("grey_of_" + name, f, whole(f), dict(m=16 * g, mean=float(g), sharp=0.0, status=0))

# ---- cell-mean rounding.  cnt = 2 (64 x 32, cells of 2 x 1) with S odd: 16 S / 2 = 8 S is whole, m = 8 S, no tie there.  A tie
#      needs 16 S / cnt = x.5: cnt = 32 (256 x 128, cells of 8 x 4) with S odd; m = (16 S + 16) / 32 rounds the half up ----
g = np.zeros((32, 64), np.int64)
g[:, ::2] = 21
f = grey_frame(g)
case("cnt_2_S_odd", f, whole(f), dict(m=168, mean=10.5, status=0))
for S, m in ((1, 1), (3, 2), (2, 1)):
    g = np.zeros((128, 256), np.int64)
    g[::4, ::8] = S
    f = grey_frame(g)
    case("tie_cnt_32_S_%d" % S, f, whole(f), dict(m=m, mean=m / 16.0, status=0, size=128.0))

# ---- box sizes on a seeded 100 x 100 frame: a box (x, y, x + w - 1, y + h - 1) has sides w, h; below 32 it is unmeasured ----
NOISE = np.random.default_rng(5).integers(0, 256, size=(100, 100, 3), dtype=np.uint8)
for w in (31, 32, 33, 63, 64, 65, 95):
    for h in (31, 32, 33, 63, 64, 65, 95):
        if w in (32, 33, 95) or h in (32, 33, 95) or (w, h) in ((31, 31), (63, 64), (64, 63), (65, 65)):
            unmeasured = w < 32 or h < 32
            want = dict(status=int(unmeasured), size=float(min(w, h)), region=(3, 2, 3 + w - 1, 2 + h - 1, w, h))
            if unmeasured:
                want.update(sharp=0.0, mean=0.0, expo=0.0, q=0.0, pose=0.75)      # the landmark parts are still computed
            case("box_%dx%d" % (w, h), NOISE, [3.5, 2.25, 3 + w - 1 + 0.75, 2 + h - 1 + 0.5, 0.5], want, **HALF_CFG)
# clipped at each side of the frame, wholly outside, and coordinates that are no pixels
for name, box, reg in (
        ("clip_left", [-10, 20, 50, 70], (0, 20, 50, 70, 51, 51)),
        ("clip_top", [20, -10.5, 70, 50], (20, 0, 70, 50, 51, 51)),
        ("clip_right", [60, 20, 200, 70], (60, 20, 99, 70, 40, 51)),
        ("clip_bottom", [20, 60, 70, 200], (20, 60, 70, 99, 51, 40)),
        ("clip_right_below_32", [69, 20, 200, 70], (69, 20, 99, 70, 31, 51)),
        ("outside_right", [200, 20, 300, 70], (200, 20, 99, 70, -100, 51)),
        ("outside_above", [20, -300, 70, -200], (20, 0, 70, -200, 51, -199)),
        ("inverted", [70, 70, 20, 20], (70, 70, 20, 20, -49, -49)),
        ("x1_nan", [NAN, 20, 50, 70], (0, 20, 50, 70, 51, 51)),
        ("y2_nan", [10, 20, 50, NAN], (10, 20, 50, 0, 41, -19)),
        ("x1_minus_inf_x2_inf", [-INF, 20, INF, 70], (0, 20, 99, 70, 100, 51)),
        ("x2_minus_inf", [10, 20, -INF, 70], (10, 20, I32_MIN, 70, I32_MIN - 10 + 1, 51)),
        ("x1_inf", [INF, 20, 50, 70], (2**31 - 1, 20, 50, 70, 50 - (2**31 - 1) + 1, 51)),
        ("all_huge", [-1e30, -1e30, 1e30, 1e30], (0, 0, 99, 99, 100, 100)),
        ("y1_inf_y2_minus_inf", [10, INF, 50, -INF], (10, 2**31 - 1, 50, I32_MIN, 41, I32_MIN - (2**31 - 1) + 1))):
    w, h = reg[4], reg[5]
    want = dict(region=reg, status=int(w < 32 or h < 32), size=float(F(np.int64(min(w, h)))))
    case("box_" + name, NOISE, box + [0.5], want)

# ---- pose ----
# the template itself: d = 35.2372, yaw = |17.7306 - 17.5066| / d = 0.00636, roll = 0.1949 / d = 0.00553, ey = 51.59885, v = 40.68595,
# (71.7366 - 51.59885) / v = 0.49496: pitch = 0.00004 against 0.495; pose = 1 - (yaw + roll + 2 pitch) = 0.988
case("pose_template", NOISE, [10, 10, 80, 80, 0.5], dict(yaw=(0.0064, 1e-4), roll=(0.0055, 1e-4), pitch=(0.0, 1e-4), pose=(0.988, 1e-3), status=0), lmk=STANDARD)
case("pose_quarter_roll", NOISE, [10, 10, 80, 80, 0.5], dict(yaw=0.0, roll=0.25, pitch=0.0, pose=0.75), **HALF_CFG)
ZERO = dict(yaw=0.0, roll=0.0, pitch=0.0, pose=0.0, q=0.0)
case("pose_d_zero", NOISE, [10, 10, 80, 80, 0.5], ZERO, lmk=[4, 0, 4, 1, 2, 2.5, 0, 4.5, 4, 4.5])
case("pose_d_negative", NOISE, [10, 10, 80, 80, 0.5], ZERO, lmk=[4, 0, 0, 1, 2, 2.5, 0, 4.5, 4, 4.5])
case("pose_v_zero", NOISE, [10, 10, 80, 80, 0.5], ZERO, lmk=[0, 0, 4, 1, 2, 2.5, 0, 0.5, 4, 0.5])
case("pose_v_negative", NOISE, [10, 10, 80, 80, 0.5], ZERO, lmk=[0, 0, 4, 1, 2, 2.5, 0, 0.25, 4, 0.25])
# a NaN in each coordinate: lx, rx -> d; ly, ry, mly, mry -> v: all four terms are 0.  nx -> yaw, ny -> pitch: that term is the
# quiet NaN, t is a NaN, pose 0.  mlx and mrx take no part: the pose of pose_quarter_roll
for k, name in enumerate(("lx", "ly", "rx", "ry", "nx", "ny", "mlx", "mly", "mrx", "mry")):
    l = list(QUARTER_ROLL)
    l[k] = NAN
    want = dict(ZERO)
    if name == "nx":
        want.update(yaw=NAN, roll=0.25)
    if name == "ny":
        want.update(pitch=NAN, roll=0.25)
    if name in ("mlx", "mrx"):
        want = dict(yaw=0.0, roll=0.25, pitch=0.0, pose=0.75)
    case("pose_nan_" + name, NOISE, [10, 10, 80, 80, 0.5], want, lmk=l, **HALF_CFG)
# t exactly 1: roll 0.5 (ry = 2, so ey = 1, my = 5, v = 4), ny = 4: (ny - ey) / v = 0.75, pitch 0.25, t = (0 + 0.5) + 0.25 * 2 = 1: pose 0.
# With w_pitch 1.5 t = 0.875 and pose = 0.125
case("pose_t_exactly_one", NOISE, [10, 10, 80, 80, 0.5], dict(yaw=0.0, roll=0.5, pitch=0.25, pose=0.0, q=0.0), lmk=[0, 0, 4, 2, 2, 4, 0, 5, 4, 5], **HALF_CFG)
case("pose_t_below_one", NOISE, [10, 10, 80, 80, 0.5], dict(yaw=0.0, roll=0.5, pitch=0.25, pose=0.125), lmk=[0, 0, 4, 2, 2, 4, 0, 5, 4, 5], pitch0=0.5, w_pitch=1.5)
# the weights reach t: w_roll 3 with roll 0.25 gives 0.75
case("pose_weights", NOISE, [10, 10, 80, 80, 0.5], dict(roll=0.25, pose=0.25), pitch0=0.5, w_roll=3.0)

# ---- the product.  A 128 x 128 checkerboard of 4 x 4 cells at 64 and 192: m = 1024 / 3072, L = +-4 * 2048: sharp = 8192^2 / 256 =
#      262144 (capped at 1), no cell dark or bright: expo 1, size 128 (capped), pose 0.75: q = 0.75 ----
yy, xx = np.mgrid[0:128, 0:128]
BOARD = grey_frame(64 + 128 * (((yy >> 2) + (xx >> 2)) & 1))
case("quality_product", BOARD, whole(BOARD), dict(sharp=262144.0, expo=1.0, size=128.0, mean=128.0, pose=0.75, q=0.75, status=0), **HALF_CFG)
case("quality_size_ref", BOARD, whole(BOARD), dict(q=0.375), pitch0=0.5, size_ref=256.0)
case("quality_sharp_ref", BOARD, whole(BOARD), dict(q=0.375), pitch0=0.5, sharp_ref=524288.0)
case("quality_times_score", BOARD, whole(BOARD, 0.5), dict(q=0.375), pitch0=0.5, times_score=1)
case("quality_score_unused", BOARD, whole(BOARD, NAN), dict(q=0.75), **HALF_CFG)
case("quality_times_nan_score", BOARD, whole(BOARD, NAN), dict(q=NAN, pose=0.75, status=0), pitch0=0.5, times_score=1)
case("quality_unmeasured_nan_score", BOARD, [0, 0, 30, 127, NAN], dict(q=0.0, status=1, size=31.0), pitch0=0.5, times_score=1)


def check(name, got):
    """got: what shot_quality_ref.measure returns, or q / parts / status of the library alone (then the inner values m, A1, A2 and
    region are not looked at); asserts every written value"""
    import shot_quality_ref as R
    want = CASES[name]["want"]
    parts = dict(zip(R.PARTS, got["parts"]))
    for k, v in want.items():
        if k in ("m", "A1", "A2", "region") and k not in got:
            continue
        if k == "m":
            assert (np.asarray(got["m"]) == v).all(), (name, k)
        elif k in ("A1", "A2", "status", "region"):
            assert got[k] == v, (name, k, got[k], v)
        else:
            g = got["q"] if k == "q" else parts[k]
            if isinstance(v, tuple):
                assert abs(float(g) - v[0]) <= v[1], (name, k, g, v)
            elif v != v:
                assert np.asarray(g, F).view(np.uint32) == 0x7FC00000, (name, k, g)
            else:
                assert F(g) == F(v) and np.signbit(F(g)) == np.signbit(F(v)), (name, k, g, v)
