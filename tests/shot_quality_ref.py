"""The shot quality of include/rfd.h ("shot quality") restated in numpy: int64 for every integer step, np.float32 / np.float64
operations in the written order for the rest, so the library's outputs equal these bit for bit.  The restatement uses the cell
edges (np.add.reduceat over them); the kernel uses the inverse map from a pixel to its cell."""
import numpy as np

F = np.float32
I32_MAX, I32_MIN = 2**31 - 1, -2**31
QNAN = np.frombuffer(np.uint32(0x7FC00000).tobytes(), F)[0]
DEFAULT = dict(dark=30, bright=225, pitch0=0.495, w_yaw=1.0, w_roll=1.0, w_pitch=2.0, sharp_ref=64.0, size_ref=112.0, times_score=0)
PARTS = ("sharp", "mean", "expo", "yaw", "roll", "pitch", "pose", "size")


def config(**fields):
    c = dict(DEFAULT)
    assert set(fields) <= set(c), fields
    c.update(fields)
    return c


def as_i32(f):
    """Rust's `as i32`: toward zero, saturating, NaN -> 0"""
    f = F(f)
    if np.isnan(f):
        return 0
    if f >= F(2147483648.0):
        return I32_MAX
    if f <= F(-2147483648.0):
        return I32_MIN
    return int(np.trunc(f))


def region(box, W, H):
    """-> X0, Y0, X1, Y1, w, h (Python ints, so nothing overflows)"""
    X0, Y0 = max(as_i32(box[0]), 0), max(as_i32(box[1]), 0)
    X1, Y1 = min(as_i32(box[2]), W - 1), min(as_i32(box[3]), H - 1)
    return X0, Y0, X1, Y1, X1 - X0 + 1, Y1 - Y0 + 1


def edges(o, n):
    return np.array([o + (k * n) // 32 for k in range(33)], np.int64)


def grey(bgr):
    p = bgr.astype(np.int64)
    return (p[..., 0] * 1868 + p[..., 1] * 9617 + p[..., 2] * 4899 + 8192) >> 14


def cell_means(frame, X0, Y0, w, h):
    """the 32 x 32 cell means of the region in 8.4 fixed point (int64)"""
    g = grey(frame[Y0:Y0 + h, X0:X0 + w])
    cx, cy = edges(0, w), edges(0, h)
    S = np.add.reduceat(np.add.reduceat(g, cy[:-1], axis=0), cx[:-1], axis=1)
    cnt = np.outer(np.diff(cy), np.diff(cx))
    return (16 * S + cnt // 2) // cnt


def laplacian_sums(m):
    L = 4 * m[1:-1, 1:-1] - m[:-2, 1:-1] - m[2:, 1:-1] - m[1:-1, :-2] - m[1:-1, 2:]
    return int(L.sum()), int((L * L).sum())


def quiet(x):
    return QNAN if np.isnan(x) else F(x)


def pose_terms(lmk, cfg):
    """-> yaw, roll, pitch, pose (np.float32), from the ten landmark coordinates"""
    l = np.asarray(lmk, F).reshape(10)
    lx, ly, rx, ry, nx, ny, mly, mry = l[0], l[1], l[2], l[3], l[4], l[5], l[7], l[9]
    with np.errstate(all="ignore"):
        d = F(rx - lx)
        ey = F(F(ly + ry) * F(0.5))
        my = F(F(mly + mry) * F(0.5))
        v = F(my - ey)
        if not (d > 0) or not (v > 0):
            return F(0), F(0), F(0), F(0)
        yaw = F(np.abs(F(F(nx - lx) - F(rx - nx))) / d)
        roll = F(np.abs(F(ry - ly)) / d)
        pitch = F(np.abs(F(F(F(ny - ey) / v) - F(cfg["pitch0"]))))
        t = F(F(F(yaw * F(cfg["w_yaw"])) + F(roll * F(cfg["w_roll"]))) + F(pitch * F(cfg["w_pitch"])))
        pose = F(F(1) - t) if t < 1 else F(0)
    return yaw, roll, pitch, pose


def min1(a):
    return a if a < 1 else F(1)


def measure(frame, box, lmk, cfg=None):
    """one row -> dict(q, parts [8] f32, status, and for a measured row m [32, 32], A1, A2)"""
    cfg = config() if cfg is None else cfg
    H, W = frame.shape[:2]
    X0, Y0, X1, Y1, w, h = region(box, W, H)
    out = dict(status=0 if (w >= 32 and h >= 32) else 1, region=(X0, Y0, X1, Y1, w, h))
    sharp = mean = expo = F(0)
    if out["status"] == 0:
        m = cell_means(frame, X0, Y0, w, h)
        A1, A2 = laplacian_sums(m)
        V = 900 * A2 - A1 * A1
        assert 0 <= V < 2**53 and abs(A1) < 2**31
        sharp = F(np.float64(V) / np.float64(207360000.0))
        mean = F(np.float64(int(m.sum())) / np.float64(16384.0))
        n = int((m <= 16 * cfg["dark"]).sum()) + int((m >= 16 * cfg["bright"]).sum())
        expo = F(F(1) - F(F(n) / F(1024)))
        out.update(m=m, A1=A1, A2=A2)
    yaw, roll, pitch, pose = pose_terms(lmk, cfg)
    size = F(np.int64(min(w, h)))
    q = F(0)
    if out["status"] == 0:
        with np.errstate(all="ignore"):
            a = F(F(box[4]) * pose) if cfg["times_score"] else pose
            q = F(F(F(a * min1(F(sharp / F(cfg["sharp_ref"])))) * min1(F(size / F(cfg["size_ref"])))) * expo)
    out["q"] = quiet(q)
    out["parts"] = np.array([sharp, mean, expo, quiet(yaw), quiet(roll), quiet(pitch), pose, size], F)
    return out


def run(frames, boxes, lmk, count, cfg, quality, parts, status):
    """the call: frames = list of HxWx3 u8; boxes [n, max_det, 5], lmk [n, max_det, 5, 2] or [n, max_det, 10], count [n]; writes the
    rows below each clamped count into quality [n, max_det], parts [n, max_det, 8], status [n, max_det] and leaves the rest"""
    n, md = boxes.shape[0], boxes.shape[1]
    l = np.asarray(lmk, F).reshape(n, md, 10)
    for b in range(n):
        for i in range(min(max(int(count[b]), 0), md)):
            r = measure(frames[b], boxes[b, i], l[b, i], cfg)
            quality[b, i], parts[b, i], status[b, i] = r["q"], r["parts"], r["status"]
    return quality, parts, status
