"""The list rule of the packed face list (include/rfd.h, "every detected face of a frame") restated in numpy: what
face_list_kernel must produce, bit for bit.  No library, no GPU.

For frame b the rows 0 .. count[b]-1 of its slab are walked in the detector's order.  A row passes when
    min(x2 - x1, y2 - y1) >= min_face_px and score >= min_score
with every difference one f32 subtraction and np.minimum carrying a NaN through, so that a NaN anywhere in the row makes a
comparison false.  The first max_faces passing rows are taken; the taken rows of all frames, frame after frame, are the list.
Faces at and past cap are dropped, total and first are not truncated."""
import numpy as np


def row_passes(boxes, min_face_px, min_score):
    """boxes [K, 5] f32 -> bool [K]"""
    b = np.asarray(boxes, np.float32).reshape(-1, 5)
    w = b[:, 2] - b[:, 0]                     # f32 - f32 -> f32: one rounding
    h = b[:, 3] - b[:, 1]
    with np.errstate(invalid="ignore"):
        return (np.minimum(w, h) >= np.float32(min_face_px)) & (b[:, 4] >= np.float32(min_score))


def face_list(dets, max_faces, min_face_px, min_score, cap):
    """dets: list of (boxes [K, 5], kps [K, 5, 2] or [K, 10]) per frame, K = that frame's count.
    -> dict(total, first [n + 1], frame, row, box [v, 5], kps [v, 10]) with v = min(total, cap) rows"""
    first, frame, row, box, kps = [0], [], [], [], []
    for b, (boxes, pts) in enumerate(dets):
        boxes = np.asarray(boxes, np.float32).reshape(-1, 5)
        pts = np.asarray(pts, np.float32).reshape(-1, 10)
        taken = np.flatnonzero(row_passes(boxes, min_face_px, min_score))[:max_faces]
        first.append(first[-1] + len(taken))
        for i in taken:
            frame.append(b)
            row.append(int(i))
            box.append(boxes[i])
            kps.append(pts[i])
    total = first[-1]
    v = min(total, cap)
    return dict(total=total, first=np.array(first, np.int32), frame=np.array(frame[:v], np.int32), row=np.array(row[:v], np.int32),
                box=np.array(box[:v], np.float32).reshape(v, 5), kps=np.array(kps[:v], np.float32).reshape(v, 10))
