"""Constructed inputs for detection over views (include/rfd.h, "views") at a 128x128 network (672 anchors): head tensors built
with tests/post_cases.py's heads_from_boxes, so that each view's candidates, and with them the merged frame's kept set, are known
from the construction.  Pure numpy plus the oracle; no GPU.  tests/test_views_ref_cpu.py holds every case against the
restatement tests/views_ref.py, tests/test_views_gpu.py runs the same inputs through the kernels.

A case is a dict: heads (per view, 9 arrays [C,h,w]), views [(frame, x, y, w, h, inner)], n_frames, margin, iou, and `want`:
per frame the list of (index of the view in `views`, index of the target within that view) of the rows the merge must keep, in
kept order, or None where only the total is written down (`count`); anchors: per view, the anchor of each target."""
import functools

import numpy as np

import post_cases as P
import views_ref as V

NET = 128
NA = P.total_anchors(NET, NET)   # 672
CONF = P.CONF
IOU = 0.45
OFF = (37, 11)                   # a view corner that is no multiple of any stride
F = np.float32


def view_heads(targets, scores, seed):
    """heads of one view whose candidates decode to `targets` [k,4] (network pixels) with `scores`; -> heads, anchors"""
    k = len(targets)
    g = P.anchors_for(k, NET, NET, seed)
    return P.heads_from_boxes(np.asarray(targets, np.float64).reshape(-1, 4), np.asarray(scores, F), g, NET, NET, seed), g


def decoded(heads):
    """what the decode makes of a view's heads: rows in (score descending, anchor) order, in network pixels"""
    return V.O.decode_nms(heads, NET, NET, F(CONF), 2.0, 1.0)[0]


def case(heads, views, n_frames, want=None, count=None, margin=4.0, iou=IOU, anchors=None):
    return dict(heads=heads, views=views, n_frames=n_frames, want=want, count=count, margin=margin, iou=iou, anchors=anchors)


@functools.lru_cache(maxsize=None)
def two_tiles(score_a, score_b):
    """One face, whole in two tiles that overlap by 56 px: frame box [90,40,110,70] is [90..110] in tile A at x = 0 and
    [18..38] in tile B at x = 72; both keep it 4 px clear of their inner side.  One row: the better score's; on equal scores
    the lower view's."""
    ha, ga = view_heads([[90, 40, 110, 70]], [score_a], 11)
    hb, gb = view_heads([[18, 40, 38, 70]], [score_b], 12)
    views = [(0, 0, 0, NET, NET, V.RIGHT), (0, 72, 0, NET, NET, V.LEFT)]
    return case([ha, hb], views, 1, want=[[(1, 0) if score_b > score_a else (0, 0)]], anchors=[ga, gb])


@functools.lru_cache(maxsize=None)
def cut_by_an_inner_edge():
    """A face that tile A's right side cuts (clipped to x2 = 127 there) and tile B holds whole, and one that only A holds: A's
    half-box is dropped by the rule, whatever its score; the frame keeps B's row and A's other row."""
    ha, ga = view_heads([[100, 40, 140, 70], [20, 20, 50, 50]], [0.99, 0.8], 21)
    hb, gb = view_heads([[28, 40, 68, 70]], [0.75], 22)
    views = [(0, 0, 0, NET, NET, V.RIGHT), (0, 72, 0, NET, NET, V.LEFT)]
    return case([ha, hb], views, 1, want=[[(0, 1), (1, 0)]], anchors=[ga, gb])


@functools.lru_cache(maxsize=None)
def full_view_and_tile():
    """A 256x256 frame: the full view at scale 1/2 and the tile at (128, 128) at scale 1 both hold the face [160,160,220,230]
    whole (network boxes [80,80,110,115] and [32,32,92,102]); the tile scores higher.  One row, the tile's."""
    hf, gf = view_heads([[80, 80, 110, 115]], [0.8], 31)
    ht, gt = view_heads([[32, 32, 92, 102]], [0.9], 32)
    views = [(0, 0, 0, 256, 256, 0), (0, 128, 128, NET, NET, V.LEFT | V.TOP)]
    return case([hf, ht], views, 1, want=[[(1, 0)]], anchors=[gf, gt])


@functools.lru_cache(maxsize=None)
def frames_3_0_1():
    """Three frames in one call with 3, 0 and 1 views (Vmax = 3: unused slots, a frame without a view).  Frame 0: three views side
    by side without overlap, a box in each, scores ascending with the view; frame 2: two distant boxes in its one view."""
    heads, anchors = [], []
    for v, s in enumerate((0.8, 0.85, 0.9)):
        h, g = view_heads([[30, 30 + 10 * v, 60, 70 + 10 * v]], [s], 41 + v)
        heads.append(h); anchors.append(g)
    h, g = view_heads([[10, 10, 30, 30], [70, 70, 100, 110]], [0.75, 0.95], 44)
    heads.append(h); anchors.append(g)
    views = [(0, OFF[0] + 130 * v, OFF[1], NET, NET, 0) for v in range(3)] + [(2, 5, 3, NET, NET, 0)]
    return case(heads, views, 3, want=[[(2, 0), (1, 0), (0, 0)], [], [(3, 1), (3, 0)]], anchors=anchors)


SIDES = ("left", "top", "right", "bottom")
# the tested side lies closest to its border; with m about 20 the other three sides pass whatever their bits say
SIDE_BOXES = {"left": [20, 40, 80, 85], "top": [40, 20, 85, 80], "right": [40, 40, 107, 85], "bottom": [40, 40, 85, 107]}


@functools.lru_cache(maxsize=None)
def edge_margins(side):
    """-> heads of the one-box view, its anchor, and the three margins (at, inside, outside): with `at` the decoded coordinate
    of the side IS the bound of the rule (kept: the rule is >= / <=); with `inside` it is one f32 step on the kept side of the
    bound, with `outside` one f32 step on the dropped side.  Left / top: the bound is m itself.  Right / bottom: the bound is
    f32(127) - m in f32; m is stepped until the bound has moved by exactly one f32 step."""
    k = SIDES.index(side)
    heads, g = view_heads([SIDE_BOXES[side]], [0.9], 50 + k)
    c = decoded(heads)[0, k]                      # the decoded coordinate, f32
    if k < 2:
        return heads, g, (c, np.nextafter(c, F(-np.inf)), np.nextafter(c, F(np.inf)))
    edge = F(NET - 1)
    at = edge - c
    assert edge - at == c                         # the difference is exact both ways at these magnitudes
    def step(direction, target):
        m = at
        for _ in range(64):
            m = np.nextafter(m, F(direction))
            if edge - m != c:
                assert edge - m == target
                return m
        raise AssertionError("no margin found")
    inside = step(-np.inf, np.nextafter(c, F(np.inf)))      # a smaller margin: the bound one step above the coordinate
    outside = step(np.inf, np.nextafter(c, F(-np.inf)))     # a larger margin: the bound one step below it
    return heads, g, (at, inside, outside)


def edge_case(side, which):
    """Two frames, the same one-box view in each: in frame 0 every side is inner, in frame 1 every side but the tested one (it
    lies on the frame border).  which: 0 at, 1 inside, 2 outside.  Frame 1 always keeps its box; frame 0 drops it for outside."""
    heads, g, margins = edge_margins(side)
    bit = 1 << SIDES.index(side)
    views = [(0, OFF[0], OFF[1], NET, NET, 15), (1, OFF[0], OFF[1], NET, NET, 15 ^ bit)]
    return case([heads, heads], views, 2, want=[[] if which == 2 else [(0, 0)], [(1, 0)]], margin=float(margins[which]), anchors=[g, g])


COUNTS = (1023, 1024, 1025, 2049)


@functools.lru_cache(maxsize=None)
def counted(n):
    """n candidates of one frame over four views that tile a 256x256 frame without overlap, isolated 3 px boxes in each, the
    scores dealt round-robin so that the sorted order interleaves the views: all n are kept.  1023 / 1024 / 1025: one chunk of
    the chunk sort, exactly full, and the first key of a second; 2049: three chunks, merged across views."""
    per = [n // 4 + (1 if v < n % 4 else 0) for v in range(4)]
    scores = P.descending_scores(n)
    heads, anchors = [], []
    for v in range(4):
        boxes, _, _, _ = P.targets_isolated(per[v], NET, NET)
        h, g = view_heads(boxes, scores[v::4][:per[v]], 60 + v)
        heads.append(h); anchors.append(g)
    views = [(0, 128 * (v % 2), 128 * (v // 2), NET, NET, 0) for v in range(4)]
    return case(heads, views, 1, count=[n], anchors=anchors)


@functools.lru_cache(maxsize=None)
def many_views(vmax):
    """vmax views of one frame, 3 px apart along x, so that neighbouring views see the same chains of boxes shifted: 40
    candidates a view, real suppression across views.  vmax = 25: 16 800 candidate slots, the register form of the NMS;
    vmax = 26: 17 472, the streaming form."""
    heads = []
    for v in range(vmax):
        boxes, _, _, _ = P.targets_chain(40, P.GEOM_7_2, NET, NET)
        boxes = boxes + F([0, 9 * (v % 3), 0, 9 * (v % 3)])
        heads.append(view_heads(boxes, P.descending_scores(40, 0.99 - 0.001 * v, 0.72), 100 + v)[0])
    views = [(0, 3 * v, 0, NET, NET, 0) for v in range(vmax)]
    return case(heads, views, 1)


@functools.lru_cache(maxsize=None)
def truncated():
    """30 isolated boxes over two views, for a context with max_det = 7: count 7, total 30, the first seven of the merged order"""
    scores = P.descending_scores(30)
    heads, anchors = [], []
    for v in range(2):
        boxes, _, _, _ = P.targets_isolated(15, NET, NET)
        h, g = view_heads(boxes, scores[v::2], 70 + v)
        heads.append(h); anchors.append(g)
    views = [(0, 0, 0, NET, NET, 0), (0, 128, 0, NET, NET, 0)]
    return case(heads, views, 1, want=[[(k % 2, k // 2) for k in range(7)]], count=[30], anchors=anchors)


def want_gidx(c, frame):
    """the v * anchors + g the case writes down for a frame's kept rows"""
    sl = V.slots(c["views"])
    return np.array([sl[i] * NA + c["anchors"][i][t] for i, t in c["want"][frame]], np.int32)
