"""Constructed inputs for decode -> sort -> NMS (csrc/kernels_post.hip): box sets and head tensors whose candidate count
and kept set are known in closed form, so that a test can put a dependency on a chosen boundary of the kernels instead
of waiting for a seed to do it.  Pure numpy plus the oracle's anchor geometry; no GPU.  tests/test_post_cases_cpu.py holds
every builder against the CPU oracle, tests/test_post_edges_gpu.py runs the same inputs through the kernels.

Patterns (indices are positions in the score-descending order the NMS sees):
  chain      equal boxes in rows, `step` apart: a box overlaps its neighbour above the IoU threshold and its second
             neighbour below it, scores descend along the chain -> greedy NMS keeps the even in-chain positions.  A box
             dropped by an UNKEPT predecessor, or one kept although its kept predecessor sits beyond a tile / wave / chunk
             hand-over, changes the parity of everything behind it.
  triples    chains of three (A, B, C) whose members sit in the first, middle and last quarter of the order, isolated boxes
             between them -> everything but the Bs is kept; a kernel that tests C against the unkept B drops C.
  isolated   no two boxes overlap -> all kept (every tile publishes 64 kept boxes).
  kills      every box overlaps the first -> one kept (the all-removed early-outs).
"""
import functools

import numpy as np

STRIDES = (32, 16, 8)
A = 2
CONF = 0.7                      # the contexts' default confidence threshold
CHAIN_LEN = 129                 # odd and no multiple of 64: both parities cross every 64-aligned boundary
MARGIN = 0.05                   # every constructed IoU stays this far from the threshold

# geometry (box side, step along the chain, IoU threshold it is built for), +1 pixel convention:
#   9 px at step 3: neighbours 54 / 108 = 0.5, second neighbours 27 / 135 = 0.2, third neighbours disjoint
#   7 px at step 2: neighbours 35 / 63 = 0.556, second 21 / 77 = 0.273, third 7 / 91 = 0.077 (fits 16 800 boxes in 640x640)
GEOM_9_3 = (9, 3, 0.4)
GEOM_7_2 = (7, 2, 0.45)
ISOLATED_SIDE = 3               # 3 px boxes, 4 px apart in a row, rows 5 px apart: 16 800 of them fit 640x640 untouching

# sizes of the nms_sorted sweep: every register word of nms_kernel<true> (16 waves x 64 boxes per word: 1024 per word,
# 17 words), its last count 17408 and the first count of nms_kernel<false> 17409, the LDS cache edge of that form (4096)
NMS_SIZES = (1, 63, 64, 65, 1023, 1024, 1025, 4095, 4096, 4097, 5121, 16384, 17408, 17409, 20000)
NMS_PATTERNS = ("chain", "triples", "isolated", "kills")


def iou(a, b):
    """nms.rs:39-54 in f32, row-wise on two [m,4] arrays"""
    a = np.asarray(a, np.float32); b = np.asarray(b, np.float32)
    one = np.float32(1.0)
    w = np.maximum(np.float32(0), np.minimum(a[:, 2], b[:, 2]) - np.maximum(a[:, 0], b[:, 0]) + one)
    h = np.maximum(np.float32(0), np.minimum(a[:, 3], b[:, 3]) - np.maximum(a[:, 1], b[:, 1]) + one)
    inter = w * h
    area = lambda v: (v[:, 2] - v[:, 0] + one) * (v[:, 3] - v[:, 1] + one)
    return inter / (area(a) + area(b) - inter)


def layout(lengths, side, step, width, height=None, splittable=False, edge=2, tall=None):
    """Chains of the given lengths, placed left to right in rows `tall + 2` apart on a canvas `width` wide (boxes `side` wide
    and `tall` high, square unless stated; boxes of one row and one height have the IoU of their 1-D extents): box k of a chain
    sits k * step right of its first box, the next chain starts at least 2 px behind the last box's right edge.  A chain
    that does not fit the rest of a row moves to the next row, or (splittable) is cut there into two chains.  Every box
    keeps `edge` px from the canvas border, so nothing reaches the decode's clip.  Returns boxes [n,4] f32 (x1,y1,x2,y2
    inclusive corners), chain id [n] and in-chain position [n], in placement order."""
    per_row = (width - 2 * edge - side) // step + 1          # start positions in a row
    skip = -(-(side + 1) // step)                            # positions between the last box of a chain and the next chain
    assert per_row >= 1
    tall = side if tall is None else tall
    boxes, cid, pos = [], [], []
    row = col = chain = 0
    for L in lengths:
        left = int(L)
        while left > 0:
            room = per_row - col
            if room < (1 if splittable else left):
                assert col > 0, "a chain of %d does not fit a row of %d" % (left, per_row)
                row, col = row + 1, 0
                continue
            m = min(left, room)
            x1 = edge + step * (col + np.arange(m))
            y1 = edge + (tall + 2) * row
            boxes.append(np.stack([x1, np.full(m, y1), x1 + side - 1, np.full(m, y1 + tall - 1)], 1))
            cid.append(np.full(m, chain)); pos.append(np.arange(m))
            chain += 1
            col += m - 1 + skip
            left -= m
    if not boxes:
        return np.zeros((0, 4), np.float32), np.zeros(0, np.int64), np.zeros(0, np.int64)
    boxes = np.concatenate(boxes).astype(np.float32)
    if height is not None:
        assert boxes[:, 3].max() <= height - 1 - edge, "%d boxes do not fit %dx%d" % (len(boxes), width, height)
    return boxes, np.concatenate(cid), np.concatenate(pos)


def descending_scores(n, hi=0.99, lo=0.71):
    """n distinct f32 scores, strictly descending, all above CONF"""
    s = np.linspace(hi, lo, max(n, 2))[:n].astype(np.float32)
    assert n < 2 or np.all(np.diff(s) < 0)
    return s


def _chain_lengths(n, L=CHAIN_LEN):
    return [L] * (n // L) + ([n % L] if n % L else [])


def targets_chain(n, geom, width, height=None):
    """-> boxes [n,4] in score order, kept positions, chain id, in-chain position"""
    side, step, _ = geom
    boxes, cid, pos = layout(_chain_lengths(n), side, step, width, height, splittable=True)
    return boxes, np.flatnonzero(pos % 2 == 0), cid, pos


def triple_order(n):
    """Score ranks of the triples' members: q = n // 4 triples; A_k at rank k, B_k in the middle, C_k at n - q + k, the
    n - 3q isolated boxes before and behind the Bs.  -> (rank of placed box i, ranks of the Bs)"""
    q = n // 4
    s1 = (n - 3 * q) // 2
    rank = np.empty(n, np.int64)
    k = np.arange(q)
    rank[3 * k] = k                                  # A
    rank[3 * k + 1] = q + s1 + k                     # B
    rank[3 * k + 2] = n - q + k                      # C
    singles = np.concatenate([np.arange(q, q + s1), np.arange(2 * q + s1, n - q)])
    rank[3 * q:] = singles
    return rank, q + s1 + k


def targets_triples(n, geom, width, height=None, tall=None):
    side, step, _ = geom
    q = n // 4
    placed, cid, pos = layout([3] * q + [1] * (n - 3 * q), side, step, width, height, tall=tall)
    rank, b_ranks = triple_order(n)
    boxes = np.empty_like(placed); c = np.empty_like(cid); p = np.empty_like(pos)
    boxes[rank], c[rank], p[rank] = placed, cid, pos
    return boxes, np.setdiff1d(np.arange(n), b_ranks), c, p


def targets_isolated(n, width, height=None):
    boxes, cid, pos = layout([1] * n, ISOLATED_SIDE, 1, width, height)
    return boxes, np.arange(n), cid, pos


def targets_kills(n):
    """100 px boxes, each shifted 0..2 px from the first: IoU with it >= 98*98 / (2*100*100 - 98*98) = 0.92"""
    i = np.arange(n)
    dx, dy = i % 3, (i // 3) % 3
    boxes = np.stack([dx, dy, dx + 99, dy + 99], 1).astype(np.float32)
    return boxes, np.arange(min(n, 1)), np.zeros(n, np.int64), i


@functools.lru_cache(maxsize=None)
def nms_case(pattern, n):
    """-> (rows [n,5] f32 in score-descending order, IoU threshold, kept indices, chain id, in-chain position)"""
    geom = GEOM_9_3
    if pattern == "chain":
        t = targets_chain(n, geom, 2048)
    elif pattern == "triples":
        t = targets_triples(n, geom, 2048)
    elif pattern == "isolated":
        t = targets_isolated(n, 2048)
    elif pattern == "kills":
        t = targets_kills(n)
    else:
        raise ValueError(pattern)
    boxes, kept, cid, pos = t
    rows = np.concatenate([boxes, descending_scores(n)[:, None]], 1).astype(np.float32)
    rows.setflags(write=False)
    return rows, geom[2], kept, cid, pos


def boxes_chain(n):
    return nms_case("chain", n)[0]


def boxes_triples(n):
    return nms_case("triples", n)[0]


def boxes_isolated(n):
    return nms_case("isolated", n)[0]


def boxes_kills(n):
    return nms_case("kills", n)[0]


def boxes_pair_among_isolated(first, second, s, v, n):
    """n rows in score order: isolated 3 px boxes, with `first` at index s and `second` at index v (both [4], placed far
    from the isolated ones: those start at x = 102)"""
    assert 0 <= s < v < n
    iso, _, _, _ = targets_isolated(n, 2048)
    iso = iso + np.float32([100, 0, 100, 0])
    iso[s], iso[v] = first, second
    return np.concatenate([iso, descending_scores(n)[:, None]], 1).astype(np.float32)


# (suppressor index, victim index, rows): victim in lane 0 and in lane 63 of another tile than its suppressor; across the
# wave-ownership hand-over (tile 0 -> tile 16); suppressor in the LDS cache and victim in L2 of the streaming form
PLACEMENTS = [(0, 64, 130), (0, 127, 130), (63, 128, 200), (10, 1087, 1100), (5, 1024, 1100), (4000, 17471, 17472),
              (4095, 17408, 17472)]
PAIR_KINDS = ("equal_survives", "below_equal_suppressed", "degenerate", "nan")


def pair_case(kind, s, v, n):
    """The survivor rule `ovr <= thresh` (nms.rs:58) where one comparison decides it -> (rows, threshold, kept indices).
    [0,0,8,8] and [3,0,11,8] have IoU 54 / 108 = 0.5 exactly in f32: the second survives at 0.5 and is suppressed at the next
    f32 below.  A box with x2 = x1 - 1 has area 0: against an identical later box the overlap is 0 / 0 = NaN, which
    suppresses; against any other box it is 0.  A NaN coordinate makes the box's area, and so every overlap with it, NaN:
    as the first box it suppresses every later box, anywhere else it is itself suppressed by the first kept box."""
    thr = np.float32(0.5)
    first, second = [0, 0, 8, 8], [3, 0, 11, 8]
    everything = np.arange(n)
    if kind == "equal_survives":
        want = everything
    elif kind == "below_equal_suppressed":
        thr = np.nextafter(np.float32(0.5), np.float32(0))
        want = np.delete(everything, v)
    elif kind == "degenerate":
        first = second = [5, 5, 4, 9]
        want = np.delete(everything, v)
    elif kind == "nan":
        first = [np.nan, 0, 8, 8]
        want = everything[:1] if s == 0 else np.delete(everything, s)
    else:
        raise ValueError(kind)
    return boxes_pair_among_isolated(first, second, s, v, n), thr, want


# ---- head tensors whose decode lands on chosen boxes -------------------------------------------------------------------

def total_anchors(net_h, net_w):
    return sum((net_h // s) * (net_w // s) * A for s in STRIDES)


@functools.lru_cache(maxsize=None)
def anchor_table(net_h, net_w):
    """[total_anchors,4] in the order g = level offset + (h*W + w)*A + a, levels 32, 16, 8 (the oracle's geometry)"""
    from oracle import oracle as O
    base = O.anchors_fpn()
    t = np.concatenate([O.anchor_plane(net_h // s, net_w // s, s, base[l]).reshape(-1, 4) for l, s in enumerate(STRIDES)])
    t.setflags(write=False)
    return t


def heads_from_boxes(targets, scores, anchors_g, net_h, net_w, seed=0):
    """9 head tensors [C,h,w] (levels 32, 16, 8 x cls, bbox, lmk) in which anchor anchors_g[k] carries fg score scores[k]
    and the deltas that bbox_pred (face_detection.rs:516-549) turns into targets[k]: ((tx-cx)/bw, (ty-cy)/bh, log(w/bw),
    log(h/bh)).  Every other anchor's fg score is below CONF, its deltas and all landmark deltas are seeded noise: the
    candidate count is exactly len(anchors_g)."""
    targets = np.asarray(targets, np.float64).reshape(-1, 4)
    g = np.asarray(anchors_g, np.int64)
    assert len(g) == len(targets) == len(scores) and len(np.unique(g)) == len(g)
    rng = np.random.default_rng(seed)
    an = anchor_table(net_h, net_w).astype(np.float64)[g]
    bw, bh = an[:, 2] - an[:, 0] + 1.0, an[:, 3] - an[:, 1] + 1.0
    cx, cy = an[:, 0] + 0.5 * (bw - 1.0), an[:, 1] + 0.5 * (bh - 1.0)
    tw, th = targets[:, 2] - targets[:, 0] + 1.0, targets[:, 3] - targets[:, 1] + 1.0
    tcx, tcy = targets[:, 0] + 0.5 * (tw - 1.0), targets[:, 1] + 0.5 * (th - 1.0)
    delta = np.stack([(tcx - cx) / bw, (tcy - cy) / bh, np.log(tw / bw), np.log(th / bh)], 1).astype(np.float32)
    heads, off = [], 0
    for s in STRIDES:
        h, w = net_h // s, net_w // s
        fg = (rng.uniform(0.0, CONF, size=(A, h, w)) * 0.98).astype(np.float32)
        bbox = rng.normal(0, 0.3, size=(4 * A, h, w)).astype(np.float32)
        lmk = rng.normal(0, 0.4, size=(10 * A, h, w)).astype(np.float32)
        sel = np.flatnonzero((g >= off) & (g < off + h * w * A))
        r = g[sel] - off
        a, p = r % A, r // A
        fg[a, p // w, p % w] = np.asarray(scores, np.float32)[sel]
        for c in range(4):
            bbox[4 * a + c, p // w, p % w] = delta[sel, c]
        heads += [np.concatenate([1.0 - fg, fg]).astype(np.float32), bbox, lmk]
        off += h * w * A
    return heads


def anchors_for(n, net_h, net_w, seed, ascending=False):
    """n distinct global anchor indices: a seeded permutation's head, so that score rank is unrelated to anchor order and
    to the order in which the decode kernel's atomic counter hands out slots; ascending for the equal-score pattern"""
    g = np.random.default_rng(seed).permutation(total_anchors(net_h, net_w))[:n]
    return np.sort(g) if ascending else g


@functools.lru_cache(maxsize=None)
def decode_case(pattern, n, net_h=640, net_w=640):
    """-> dict(heads, targets [n,4] in score order, gidx of the kept boxes in kept order, cid, pos, iou_thr).
    pattern: chain | equal (the chain with one score: the order is ascending g) | triples | isolated"""
    geom = GEOM_7_2
    if pattern in ("chain", "equal"):
        boxes, kept, cid, pos = targets_chain(n, geom, net_w, net_h)
    elif pattern == "triples":
        # 7 px wide, 1 px high (y2 = y1): 4200 triples and 4200 single boxes of 7x7 do not fit 640x640
        boxes, kept, cid, pos = targets_triples(n, geom, net_w, net_h, tall=1)
    elif pattern == "isolated":
        boxes, kept, cid, pos = targets_isolated(n, net_w, net_h)
    else:
        raise ValueError(pattern)
    seed = 1000 + n
    g = anchors_for(n, net_h, net_w, seed, ascending=pattern == "equal")
    scores = np.full(n, 0.9, np.float32) if pattern == "equal" else descending_scores(n)
    heads = heads_from_boxes(boxes, scores, g, net_h, net_w, seed)
    for h in heads:
        h.setflags(write=False)
    return dict(heads=heads, targets=boxes, anchors=g, kept_gidx=g[kept].astype(np.int32), cid=cid, pos=pos, iou_thr=geom[2],
                n=n, net=(net_h, net_w))


# the decode_nms cases of tests/test_post_edges_gpu.py, shared with the CPU check of the builders
BATCH_COUNTS = (0, 1, 64, 1024, 1025, 2048, 2049, 16800)        # one batch-8 launch, chain pattern
BATCH2_COUNTS = (63, 65, 1023, 2047, 4095, 4097, 8191, 12673)   # a second one: the remaining exact counts
SINGLE_640 = [(p, n) for p in ("triples", "equal") for n in (2049, 8191, 16800)]
COUNTS_704 = (4095, 4096, 4097, 18432, 18433, 20328)
CASES_704 = [(p, n) for p in ("chain", "equal") for n in COUNTS_704]
TRUNCATION = ("isolated", 16800)
