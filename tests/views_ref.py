"""Detection over overlapping views (include/rfd.h, "views"), restated for the tests.  The reference has no counterpart -- its
RetinaFaceDetection::call letterboxes one image -- so this is a test-side statement of the rule, built from the oracle's pieces:

  per view   oracle.decode_nms(heads_v, iou_thr = 2.0, det_scale = 1.0): no overlap exceeds 2, so this is every thresholded
             candidate of the view, decoded and clipped in network pixels, in (score descending, anchor ascending) order, with
             its anchor index;
  then, in numpy f32: the inner-edge rule, the map to frame pixels X = x / det_scale + offset (one division, one addition),
  the concatenation of a frame's views, the order (score descending, v * anchors + g ascending), oracle.nms, the max_det cut.

A view is (frame, x, y, w, h, inner) or an object with those attributes; inner: bit 0 left, 1 top, 2 right, 3 bottom."""
import numpy as np

from oracle import oracle as O

LEFT, TOP, RIGHT, BOTTOM = 1, 2, 4, 8
F = np.float32


def view_tuple(v):
    return tuple(int(a) for a in ((v.frame, v.x, v.y, v.w, v.h, v.inner) if hasattr(v, "frame") else v))


def total_anchors(net_h, net_w):
    return sum((net_h // s) * (net_w // s) * O.NUM_ANCHORS for s in O.STRIDES)


def slots(views):
    """position of every view among the views of its frame (the views are sorted by frame)"""
    out, run = [], 0
    for i, v in enumerate(views):
        run = run + 1 if i and view_tuple(views[i - 1])[0] == view_tuple(v)[0] else 0
        out.append(run)
    return out


def sort_bits(scores):
    """the monotone key of the sort: ascending key = descending score, -0.0 as +0.0"""
    s = np.where(scores == 0, F(0), scores).astype(F)
    u = s.view(np.uint32)
    u = u ^ np.where(u >> 31, np.uint32(0xffffffff), np.uint32(0x80000000))
    return ~u


def edge_keep(det, inner, new_w, new_h, margin):
    """the inner-edge rule on clipped boxes [k, >= 4] in network pixels; a comparison with a NaN is false"""
    m = F(margin)
    keep = np.ones(len(det), bool)
    with np.errstate(invalid="ignore"):
        if inner & LEFT:
            keep &= det[:, 0] >= m
        if inner & TOP:
            keep &= det[:, 1] >= m
        if inner & RIGHT:
            keep &= det[:, 2] <= F(new_w - 1) - m
        if inner & BOTTOM:
            keep &= det[:, 3] <= F(new_h - 1) - m
    return keep


def view_candidates(heads_v, view, net_h, net_w, conf_thr, margin):
    """-> rows [k,5] and landmarks [k,5,2] in frame pixels, anchors [k], of the candidates of one view that pass the rule"""
    _, x, y, w, h, inner = view_tuple(view)
    new_w, new_h, scale = O.geometry(h, w, net_w, net_h)
    det, lmk, g, _ = O.decode_nms(heads_v, net_h, net_w, F(conf_thr), 2.0, 1.0)
    keep = edge_keep(det, inner, new_w, new_h, margin)
    det, lmk, g = det[keep].astype(F), lmk[keep].astype(F), g[keep]
    scale, off = F(scale), np.array([x, y], F)
    det[:, 0:4:2] = det[:, 0:4:2] / scale + off[0]
    det[:, 1:4:2] = det[:, 1:4:2] / scale + off[1]
    lmk = lmk / scale + off
    return det, lmk.astype(F), g.astype(np.int64)


def detect_views(heads, views, n_frames, net_h, net_w, conf_thr, iou_thr, margin, max_det):
    """heads: per view, the 9 head arrays [C,h,w].  -> per frame (det [K,5], lmk [K,5,2], gidx [K] = v * anchors + g, total):
    K = min(total, max_det)"""
    na = total_anchors(net_h, net_w)
    per_frame = [[] for _ in range(n_frames)]
    for hv, view, v in zip(heads, views, slots(views)):
        det, lmk, g = view_candidates(hv, view, net_h, net_w, conf_thr, margin)
        per_frame[view_tuple(view)[0]].append((det, lmk, v * na + g))
    out = []
    for parts in per_frame:
        if not parts:
            out.append((np.zeros((0, 5), F), np.zeros((0, 5, 2), F), np.zeros(0, np.int32), 0))
            continue
        det, lmk, vg = (np.concatenate([p[k] for p in parts]) for k in range(3))
        order = np.lexsort((vg, sort_bits(det[:, 4])))
        det, lmk, vg = det[order], lmk[order], vg[order]
        keep = O.nms(det, iou_thr) if len(det) else np.zeros(0, np.int32)
        total = len(keep)
        keep = keep[:max_det]
        out.append((det[keep], lmk[keep], vg[keep].astype(np.int32), total))
    return out
