"""The redaction rule of include/rfd.h ("redaction") in plain numpy, per pixel: the judge of tests/test_redact_gpu.py.  Every f32
step is one numpy float32 operation in the written order; everything else is integer."""
import numpy as np

F = np.float32
FILL, PIXELATE = 0, 1
RECT, ELLIPSE = 0, 1
DEFAULT = dict(mode=PIXELATE, shape=ELLIPSE, cell=16, fill=(0, 0, 0), margin_x=0.1, margin_top=0.2, margin_bottom=0.1, sel_mask=0, sel_value=0)


def config(**fields):
    assert set(fields) <= set(DEFAULT), fields
    return dict(DEFAULT, **fields)


def as_i32(f):
    """Rust's `as i32`: toward zero, saturating, NaN -> 0"""
    f = float(f)
    if f != f:
        return 0
    if f >= 2147483648.0:
        return 2**31 - 1
    if f <= -2147483648.0:
        return -2**31
    return int(f)


def region(box, cfg, W, H):
    """(X0, Y0, X1, Y1) of a box row in an H x W frame, or None where the row is skipped"""
    x1, y1, x2, y2 = (F(v) for v in box[:4])
    if not all(np.isfinite(v) for v in (x1, y1, x2, y2)):
        return None
    with np.errstate(all="ignore"):
        bw, bh = F(x2 - x1), F(y2 - y1)
        if not bw >= 0 or not bh >= 0:
            return None
        gx, gt, gb = F(bw * F(cfg["margin_x"])), F(bh * F(cfg["margin_top"])), F(bh * F(cfg["margin_bottom"]))
        xa, xb, ya, yb = F(x1 - gx), F(x2 + gx), F(y1 - gt), F(y2 + gb)
    if any(np.isnan(v) for v in (xa, xb, ya, yb)):
        return None
    X0, Y0 = max(as_i32(xa), 0), max(as_i32(ya), 0)
    X1, Y1 = min(as_i32(xb), W - 1), min(as_i32(yb), H - 1)
    if X1 < X0 or Y1 < Y0:
        return None
    return X0, Y0, X1, Y1


def region_cover(reg, shape):
    """the covered pixels of a region as a [h, w] bool array"""
    X0, Y0, X1, Y1 = reg
    w, h = X1 - X0 + 1, Y1 - Y0 + 1
    if shape == RECT:
        return np.ones((h, w), bool)
    dx = (2 * np.arange(w, dtype=np.int64) + 1 - w)[None, :]
    dy = (2 * np.arange(h, dtype=np.int64) + 1 - h)[:, None]
    return dx * dx * (h * h) + dy * dy * (w * w) <= (w * w) * (h * h)      # below 2^61 for sides <= 32768


def selected(sel_row, i, cfg):
    return sel_row is None or (int(sel_row[i]) & int(cfg["sel_mask"])) == int(cfg["sel_value"])


def cover(H, W, boxes, count, sel_row, cfg):
    """-> ([H, W] bool: covered by at least one selected, non-skipped row; applied = how many such rows)"""
    covered = np.zeros((H, W), bool)
    applied = 0
    for i in range(min(max(int(count), 0), len(boxes))):
        if not selected(sel_row, i, cfg):
            continue
        reg = region(boxes[i], cfg, W, H)
        if reg is None:
            continue
        applied += 1
        X0, Y0, X1, Y1 = reg
        covered[Y0:Y1 + 1, X0:X1 + 1] |= region_cover(reg, cfg["shape"])
    return covered, applied


def cell_means(frame, cell):
    """[H, W, 3] u8: at every pixel the mean (S + cnt / 2) / cnt of its frame-anchored cell over the cell's pixels inside the frame"""
    H, W = frame.shape[:2]
    ys, xs = np.arange(0, H, cell), np.arange(0, W, cell)
    S = np.add.reduceat(np.add.reduceat(frame.astype(np.int64), ys, axis=0), xs, axis=1)
    cnt = np.add.reduceat(np.add.reduceat(np.ones((H, W, 1), np.int64), ys, axis=0), xs, axis=1)
    m = (S + cnt // 2) // cnt
    return np.repeat(np.repeat(m, cell, axis=0), cell, axis=1)[:H, :W].astype(np.uint8)


def redact(frame, boxes, count, sel_row, cfg):
    """one frame -> (the redacted frame, a new array; applied)"""
    H, W = frame.shape[:2]
    covered, applied = cover(H, W, boxes, count, sel_row, cfg)
    colour = cell_means(frame, cfg["cell"]) if cfg["mode"] == PIXELATE else np.broadcast_to(np.asarray(cfg["fill"][:3], np.uint8), frame.shape)
    out = frame.copy()
    out[covered] = colour[covered]
    return out, applied


def run(frames, boxes, count, sel, cfg):
    """frames: list of [H, W, 3] u8; boxes [n, max_det, 5]; count [n]; sel [n, max_det] u32 or None -> (list of frames, applied [n] i32)"""
    outs, applied = [], np.zeros(len(frames), np.int32)
    for b, f in enumerate(frames):
        o, applied[b] = redact(f, boxes[b], count[b], None if sel is None else sel[b], cfg)
        outs.append(o)
    return outs, applied
