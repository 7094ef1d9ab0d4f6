"""numpy restatement of the reference's liveness glue, src/pipeline/module/face_antispoofing.rs: _get_scale_image :245-295,
_get_new_box :342-385, the Mat::roi / cv::resize validity rule :323-337, _preprocess :180-217 and _postprocess :219-243.

Every intermediate is an np.float32, so every arithmetic step is one IEEE f32 operation in the order the Rust is written
in; Rust's `as i32` and its wrapping i32 arithmetic (a release build) have helpers of their own.  The pixels come from the
oracle's restated cv::resize.  Test infrastructure only."""
import numpy as np

f32 = np.float32
DEFAULT_SCALES = [4.0, 2.7, 2.0, 1.0]                          # :483
DEFAULT_SIZES = [(80, 80), (80, 80), (256, 256), (128, 128)]   # :477-482, (w, h)

_ERR = dict(over="ignore", invalid="ignore", divide="ignore")


def as_i32(x):
    """Rust `x as i32` for an f32: toward zero, saturating, NaN -> 0"""
    x = f32(x)
    if np.isnan(x):
        return 0
    if x >= f32(2147483648.0):
        return 2147483647
    if x <= f32(-2147483648.0):
        return -2147483648
    return int(x)


def wrap_i32(v):
    """a Python int reduced to what wrapping i32 arithmetic leaves"""
    return (int(v) + 2 ** 31) % 2 ** 32 - 2 ** 31


def i32_as_f32(v):
    return f32(int(v))   # round to nearest even, as Rust's `as f32`


def f32_min(a, b):
    """f32::min: if one operand is NaN the other is returned"""
    if np.isnan(a):
        return b
    if np.isnan(b):
        return a
    return a if a < b else b


def scale_image_box(box, cast=as_i32, wrap=wrap_i32, trace=None):
    """_get_scale_image :249-262 -> Rect (x, y, w, h).  cast / wrap: the two integer rules, replaceable by the mutation guards of
    tests/liveness_cases.py; trace: a dict that receives the four f32 values in front of the casts"""
    with np.errstate(**_ERR):
        xmin, ymin, xmax, ymax = (f32(v) for v in box[:4])
        det_height = ymax - ymin
        c_x = (xmin + xmax) / f32(2.0)
        pre = (c_x - f32(0.47) * det_height, c_x + f32(0.47) * det_height, ymin, ymax - ymin + f32(1.0))
        if trace is not None:
            trace["crop"] = pre
        left, right = cast(pre[0]), cast(pre[1])
        return left, cast(pre[2]), wrap(right - left + 1), cast(pre[3])


def new_box(src_w, src_h, bbox, scale_ori, cast=as_i32, trace=None):
    """_get_new_box :342-385 -> (ltx, lty, rbx, rby, weight, shifts); shifts names the `if`s that fired (for the tests);
    trace: a dict that receives the ratios, the scale and the corners before the shifts and in front of the casts"""
    x, y, box_w, box_h = bbox
    scale_ori = f32(scale_ori)
    with np.errstate(**_ERR):
        w1, h1 = i32_as_f32(src_w) - f32(1.0), i32_as_f32(src_h) - f32(1.0)
        ratio_h, ratio_w = h1 / i32_as_f32(box_h), w1 / i32_as_f32(box_w)
        scale = f32_min(ratio_h, f32_min(ratio_w, scale_ori))
        new_width, new_height = i32_as_f32(box_w) * scale, i32_as_f32(box_h) * scale
        center_x = i32_as_f32(box_w) / f32(2.0) + i32_as_f32(x)
        center_y = i32_as_f32(box_h) / f32(2.0) + i32_as_f32(y)
        ltx, lty = center_x - new_width / f32(2.0), center_y - new_height / f32(2.0)
        rbx, rby = center_x + new_width / f32(2.0), center_y + new_height / f32(2.0)
        shifts, first = [], (ltx, lty, rbx, rby)
        if ltx < f32(0.0):
            rbx = rbx - ltx
            ltx = f32(0.0)
            shifts.append("left")
        if lty < f32(0.0):
            rby = rby - lty
            lty = f32(0.0)
            shifts.append("top")
        if rbx > w1:
            ltx = ltx - (rbx - i32_as_f32(src_w) + f32(1.0))
            rbx = w1
            shifts.append("right")
        if rby > h1:
            lty = lty - (rby - i32_as_f32(src_h) + f32(1.0))
            rby = h1
            shifts.append("bottom")
        if trace is not None:
            trace.update(ratio_h=ratio_h, ratio_w=ratio_w, scale=scale, w1=w1, h1=h1, first=first, corners=(ltx, lty, rbx, rby))
        return cast(ltx), cast(lty), cast(rbx), cast(rby), f32(scale / scale_ori), shifts


def roi_rect(ltx, lty, rbx, rby, wrap=wrap_i32):
    return ltx, lty, wrap(rbx - ltx + 1), wrap(rby - lty + 1)   # :323


def roi_ok(rect, src_w, src_h):
    """Mat::roi accepts 0 <= x, 0 <= w, x + w <= cols (same in y); cv::resize then rejects an empty source"""
    x, y, w, h = rect
    return x >= 0 and y >= 0 and w > 0 and h > 0 and x + w <= src_w and y + h <= src_h


def face(frame, box, found, scales=DEFAULT_SCALES, sizes=DEFAULT_SIZES, oracle=None, cast=as_i32, wrap=wrap_i32, traces=None):
    """One face = a single-image call of the reference.  -> dict(tensors [k] of [3, out_h, out_w] f32 (or None without an
    oracle), weights [k] f32, rois [k, 4] i32, status, shifts [k] lists).  traces: a list that receives one dict per model"""
    k = len(scales)
    src_h, src_w = frame.shape[:2]
    rois, weights, shifts = np.zeros((k, 4), np.int32), np.zeros(k, np.float32), [[] for _ in range(k)]
    status = 0
    if not (int(found) & 1):
        status = -2
    else:
        crop = {}
        bbox = scale_image_box(box, cast, wrap, crop)
        for j in range(k):
            tr = dict(crop, bbox=bbox)
            ltx, lty, rbx, rby, weights[j], shifts[j] = new_box(src_w, src_h, bbox, scales[j], cast, tr)
            rois[j] = wrap_i32(ltx), wrap_i32(lty), wrap_i32(rbx), wrap_i32(rby)   # (only a mutated cast leaves the i32 range)
            tr["rect"] = roi_rect(ltx, lty, rbx, rby, wrap)
            if not roi_ok(tr["rect"], src_w, src_h):
                status = -3   # the reference returns Err for the whole face (:324-337)
            if traces is not None:
                traces.append(tr)
    tensors = None
    if oracle is not None:
        tensors = []
        for j in range(k):
            w, h = sizes[j]
            if status < 0:
                tensors.append(np.zeros((3, h, w), np.float32))
                continue
            ltx, lty, rbx, rby = (int(v) for v in rois[j])
            px = oracle.resize_linear(frame[lty:rby + 1, ltx:rbx + 1], h, w)
            tensors.append(px.transpose(2, 0, 1).astype(np.float32))   # plane c = byte channel c of the frame (:203-212)
    if status < 0:
        weights[:] = 0
        if status == -2:
            rois[:] = 0
    return dict(tensors=tensors, weights=weights, rois=rois, status=status, shifts=shifts)


def batch(frames, boxes, found, scales=DEFAULT_SCALES, sizes=DEFAULT_SIZES, oracle=None):
    """n independent faces -> (tensors [k] of [n, 3, h, w], weights [n, k], rois [n, k, 4], status [n], per-face dicts)"""
    per = [face(f, b, fd, scales, sizes, oracle) for f, b, fd in zip(frames, boxes, found)]
    tensors = None if oracle is None else [np.stack([p["tensors"][j] for p in per]) for j in range(len(scales))]
    return (tensors, np.stack([p["weights"] for p in per]), np.stack([p["rois"] for p in per]),
            np.array([p["status"] for p in per], np.int32), per)


def decide(logits, weights, threshold=0.55):
    """_postprocess :228-238 with the weights it was written for: per face, over the models in order,
    live_score = live_score + column(1) * w; total_weight += w; then one division and `> threshold`.
    logits: k arrays [n, classes]; weights [n, k] -> (score [n] f32, live [n] i32)"""
    n = logits[0].shape[0]
    score, live = np.zeros(n, np.float32), np.zeros(n, np.int32)
    with np.errstate(**_ERR):
        for i in range(n):
            s, total = f32(0.0), f32(0.0)
            for o, w in zip(logits, weights[i]):
                s = s + f32(o[i, 1]) * f32(w)
                total = total + f32(w)
            s = s / total
            score[i] = s
            live[i] = 1 if s > f32(threshold) else 0
    return score, live


def decide_as_written(logits, list_weight_scales, threshold=0.55):
    """_postprocess exactly as written, for one image: zip(outputs, weights) stops at the shorter list, and `call` :77-80 makes
    every list of weights ONE element long -- only the first model's output is used"""
    return decide(logits[:len(list_weight_scales)], np.asarray(list_weight_scales, np.float32)[None, :].repeat(logits[0].shape[0], 0),
                  threshold)
