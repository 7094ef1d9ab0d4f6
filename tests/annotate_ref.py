"""The annotation rule of include/rfd.h ("annotation") in plain numpy, as the LITERAL PAINTER: the rows of a frame in descending
index, each painting its layers 1 -> 4 over whatever is there, the blend last -- so the lowest row ends on top and within a row the
highest layer, by painting order alone.  This is deliberately not the kernel's first-cover structure.  The judge of
tests/test_annotate_gpu.py.  Every f32 step is one numpy float32 operation in the written order; everything else is a Python
integer (unbounded, so "in int64" holds).  The glyph table is passed in: the library holds the only copy of the font."""
import numpy as np

from redact_ref import as_i32

F = np.float32
NONE, ARRAY, SCORE = 0, 1, 2
MINUS, QUESTION, PERCENT, SPACE = 10, 11, 12, 13
DEFAULT = dict(styles=((0, 0, (0, 255, 0)),), thickness=2, mark_radius=2, label_source=NONE, value_source=SCORE, text_scale=2,
               text_colour=(0, 0, 0), alpha=256, margin_x=0.0, margin_top=0.0, margin_bottom=0.0)


def config(**fields):
    assert set(fields) <= set(DEFAULT), fields
    return dict(DEFAULT, **fields)


def box(row, cfg):
    """(XA, YA, XB, YB) of a box row, not clipped, or None where the row is skipped"""
    x1, y1, x2, y2 = (F(v) for v in row[:4])
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
    XA, XB, YA, YB = as_i32(xa), as_i32(xb), as_i32(ya), as_i32(yb)
    if XB < XA or YB < YA:
        return None
    return XA, YA, XB, YB


def style_of(word, cfg):
    """the index of the first style the word matches, or None"""
    for k, (mask, value, _) in enumerate(cfg["styles"]):
        if (int(word) & int(mask)) == int(value):
            return k
    return None


def percent(v):
    """the glyphs of the value part"""
    v = F(v)
    if not np.isfinite(v) or not v >= 0:
        return [MINUS, MINUS, PERCENT]
    with np.errstate(all="ignore"):
        p = min(as_i32(F(F(v * F(100.0)) + F(0.5))), 999)
    return [int(ch) for ch in str(p)] + [PERCENT]


def text(cfg, label, value, score):
    """the glyph indices of a row's string"""
    out = []
    if cfg["label_source"] == ARRAY:
        out += [QUESTION] if int(label) < 0 else [int(ch) for ch in str(int(label))]
    if cfg["value_source"] != NONE:
        if out:
            out.append(SPACE)
        out += percent(value if cfg["value_source"] == ARRAY else score)
    assert len(out) <= 15
    return out


def string(glyphs):
    return "".join("0123456789-?% "[g] for g in glyphs)


def plate(XA, YA, n, s):
    PW, PH = s * (6 * n + 1), 9 * s
    return XA, (YA - PH if YA - PH >= 0 else YA), PW, PH


def _span(lo, hi, size):
    """the integers of [lo, hi] inside 0 .. size - 1 as an int64 array (possibly empty)"""
    lo, hi = max(lo, 0), min(hi, size - 1)
    return np.arange(lo, hi + 1, dtype=np.int64) if hi >= lo else np.zeros(0, np.int64)


def paint_row(colour, layer, bx, marks, glyphs, c_row, cfg, font):
    """one row over the canvas: colour [H, W, 3] u8 and layer [H, W] u8 (0 = not covered) are written where the row covers"""
    H, W = layer.shape
    XA, YA, XB, YB = bx
    t, r, s = cfg["thickness"], cfg["mark_radius"], cfg["text_scale"]

    def put(ys, xs, on, value, col):
        if len(ys) and len(xs) and on.any():
            sub = np.ix_(ys, xs)
            lay, c = layer[sub], colour[sub]
            lay[on], c[on] = value, col
            layer[sub], colour[sub] = lay, c

    if t > 0:                                                                            # layer 1
        xs, ys = _span(XA, XB, W), _span(YA, YB, H)
        on = ((xs < XA + t) | (xs > XB - t))[None, :] | ((ys < YA + t) | (ys > YB - t))[:, None]
        put(ys, xs, on, 1, c_row)
    if r > 0:                                                                            # layer 2
        for lx, ly in marks:
            if not (np.isfinite(F(lx)) and np.isfinite(F(ly))):
                continue
            cx, cy = as_i32(F(lx)), as_i32(F(ly))
            xs, ys = _span(cx - r, cx + r, W), _span(cy - r, cy + r, H)
            put(ys, xs, (xs - cx)[None, :] ** 2 + (ys - cy)[:, None] ** 2 <= r * r, 2, c_row)
    if glyphs:
        PX, PY, PW, PH = plate(XA, YA, len(glyphs), s)
        xs, ys = _span(PX, PX + PW - 1, W), _span(PY, PY + PH - 1, H)
        put(ys, xs, np.ones((len(ys), len(xs)), bool), 3, c_row)                          # layer 3
        fx, fy = ((xs - PX) // s)[None, :], ((ys - PY) // s)[:, None]                     # layer 4
        k, u, v = (fx - 1) // 6, (fx - 1) % 6, fy - 1
        inside = (fx >= 1) & (fy >= 1) & (k < len(glyphs)) & (u < 5) & (v < 7)
        table = np.asarray(font, np.int64)[np.asarray(glyphs, np.int64)]                  # [len, 7]
        bits = table[np.clip(k, 0, len(glyphs) - 1), np.clip(v, 0, 6)] >> (4 - np.clip(u, 0, 4)) & 1
        put(ys, xs, np.broadcast_to(inside & (bits == 1), (len(ys), len(xs))), 4, cfg["text_colour"][:3])


def layers(frame_shape, boxes, lmk, count, sel_row, label_row, value_row, cfg, font):
    """-> (colour [H, W, 3] u8, layer [H, W] u8: 0 not covered else the winning layer, applied)"""
    H, W = frame_shape[:2]
    colour, layer = np.zeros((H, W, 3), np.uint8), np.zeros((H, W), np.uint8)
    applied = 0
    for i in reversed(range(min(max(int(count), 0), len(boxes)))):
        k = style_of(0 if sel_row is None else sel_row[i], cfg)
        if k is None:
            continue
        bx = box(boxes[i], cfg)
        if bx is None:
            continue
        applied += 1
        marks = [] if lmk is None else [(lmk[i][2 * m], lmk[i][2 * m + 1]) for m in range(5)]
        glyphs = text(cfg, 0 if label_row is None else label_row[i], 0 if value_row is None else value_row[i], boxes[i][4])
        paint_row(colour, layer, bx, marks, glyphs, cfg["styles"][k][2][:3], cfg, font)
    return colour, layer, applied


def annotate(frame, boxes, lmk, count, sel_row, label_row, value_row, cfg, font):
    """one frame -> (the annotated frame, a new array; applied)"""
    colour, layer, applied = layers(frame.shape, boxes, lmk, count, sel_row, label_row, value_row, cfg, font)
    a = int(cfg["alpha"])
    blended = colour if a == 256 else ((a * colour.astype(np.int64) + (256 - a) * frame.astype(np.int64) + 128) >> 8).astype(np.uint8)
    out = frame.copy()
    out[layer > 0] = blended[layer > 0]
    return out, applied


def run(frames, boxes, lmk, count, sel, label, value, cfg, font):
    """frames: list of [H, W, 3] u8; boxes [n, max_det, 5]; lmk [n, max_det, 10] or None; count [n]; sel u32, label i32, value f32
    [n, max_det] or None -> (list of frames, applied [n] i32)"""
    outs, applied = [], np.zeros(len(frames), np.int32)
    pick = lambda a, b: None if a is None else a[b]
    for b, f in enumerate(frames):
        o, applied[b] = annotate(f, boxes[b], pick(lmk, b), count[b], pick(sel, b), pick(label, b), pick(value, b), cfg, font)
        outs.append(o)
    return outs, applied
