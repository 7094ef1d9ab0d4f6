"""The builders of tests/post_cases.py against the CPU oracle alone, so that a failure of tests/test_post_edges_gpu.py
points at a kernel and not at a fixture: for every pattern and size the GPU file uses, the candidate count is exact, the
oracle keeps exactly the closed-form set, every constructed IoU (computed on the boxes the oracle decodes) stays
post_cases.MARGIN from the threshold, boxes of different chains do not touch, and no box reaches the decode's clip."""
import numpy as np
import pytest

import post_cases as pc


def _check_geometry(boxes, cid, pos, thr, net=None):
    """boxes [n,4] in any order, with chain id and in-chain position: neighbours in a chain overlap above thr + MARGIN, every
    farther pair of a chain below thr - MARGIN, boxes of different chains have no overlap at all under the +1 pixel convention
    (painted on an integer canvas: every corner is within 0.01 of an integer and the pixel ranges [rint(x1), rint(x2) + 1] of
    two chains never meet, so x1' - x2 >= 2 - 0.02 and the intersection's width x2 - x1' + 1 is negative)."""
    n = len(boxes)
    if n == 0:
        return
    assert np.all(np.isfinite(boxes))
    if net is not None:
        H, W = net
        assert boxes[:, 0].min() > 0 and boxes[:, 1].min() > 0 and boxes[:, 2].max() < W - 1 and boxes[:, 3].max() < H - 1, \
            "a target box touches the clip"
    order = np.lexsort((pos, cid))
    b, c, p = boxes[order], cid[order], pos[order]
    for k in range(1, 6):
        same = (c[k:] == c[:-k]) & (p[k:] == p[:-k] + k)
        if not same.any():
            continue
        v = pc.iou(b[:-k][same], b[k:][same])
        if k == 1:
            assert v.min() >= thr + pc.MARGIN, "neighbour IoU %g" % v.min()
        else:
            assert v.max() <= thr - pc.MARGIN, "IoU %g at in-chain distance %d" % (v.max(), k)
    assert np.abs(boxes - np.rint(boxes)).max() < 0.01
    x0, y0 = np.rint(boxes[:, 0]).astype(int), np.rint(boxes[:, 1]).astype(int)
    x1, y1 = np.rint(boxes[:, 2]).astype(int) + 1, np.rint(boxes[:, 3]).astype(int) + 1
    assert x0.min() >= 0 and y0.min() >= 0
    canvas = np.full((y1.max() + 1, x1.max() + 1), -1, np.int64)
    for i in range(n):
        win = canvas[y0[i]:y1[i] + 1, x0[i]:x1[i] + 1]
        assert np.all((win == -1) | (win == cid[i])), "boxes of chains %d and %d touch" % (cid[i], win.max())
        win[...] = cid[i]


@pytest.mark.parametrize("n", pc.NMS_SIZES)
@pytest.mark.parametrize("pattern", pc.NMS_PATTERNS)
def test_nms_builders(oracle, pattern, n):
    rows, thr, kept, cid, pos = pc.nms_case(pattern, n)
    assert rows.shape == (n, 5) and rows.dtype == np.float32
    assert np.all(np.diff(rows[:, 4]) < 0)
    assert np.array_equal(oracle.nms(rows, thr), kept)
    if pattern == "kills":
        assert n < 2 or pc.iou(np.repeat(rows[:1, :4], n - 1, 0), rows[1:, :4]).min() >= thr + pc.MARGIN
        assert len(kept) == 1
    else:
        _check_geometry(rows[:, :4], cid, pos, thr)
        want = {"chain": int(np.sum(pos % 2 == 0)), "triples": n - n // 4, "isolated": n}[pattern]
        assert len(kept) == want


def test_chain_parities_cross_every_boundary():
    """an odd chain length that is no multiple of 64: at each 64-aligned index of the sorted order (tile, wave-ownership,
    chunk boundaries and the LDS cache edge are all multiples of 64) some case has a kept box just before it and some case a
    kept box just behind it, and the box behind depends on the one before (same chain)"""
    assert pc.CHAIN_LEN % 2 == 1 and pc.CHAIN_LEN % 64 != 0
    _, _, kept, cid, pos = pc.nms_case("chain", 20000)
    kept = set(kept.tolist())
    before = [e for e in range(64, 20000, 64) if cid[e] == cid[e - 1] and (e - 1) in kept]
    behind = [e for e in range(64, 20000, 64) if cid[e] == cid[e - 1] and e in kept]
    assert len(before) > 100 and len(behind) > 100
    for edge in (1024, 4096, 17408):        # word hand-over of the register form, LDS cache edge, last register word
        assert cid[edge] == cid[edge - 1]


def test_triples_sit_in_different_chunks_and_on_both_sides_of_the_lds_edge():
    """A, B, C of a triple in different NMS chunks (nms_chunked_kernel: tpc = ceil(tiles / 4) tiles per chunk) at every
    decode size of the GPU file, and in the streaming form's sweep an A below index 4096 with its B above it"""
    for n in (2049, 8191, 16800):
        rank, b = pc.triple_order(n)
        q = n // 4
        tpc = -(-((n + 63) // 64) // 4)
        chunk = lambda r: (r // 64) // tpc
        a, c = rank[0:3 * q:3], rank[2:3 * q:3]
        assert np.all(chunk(a) < chunk(b)) and np.all(chunk(b) < chunk(c))
    rank, b = pc.triple_order(20000)
    assert np.any((rank[0:15000:3] < 4096) & (b >= 4096)) and np.any(rank[0:15000:3] >= 4096)


DECODE_CASES = ([("chain", n, 640) for n in pc.BATCH_COUNTS + pc.BATCH2_COUNTS] + [(p, n, 640) for p, n in pc.SINGLE_640] +
                [pc.TRUNCATION + (640,)] + [(p, n, 704) for p, n in pc.CASES_704])


@pytest.mark.parametrize("pattern,n,size", DECODE_CASES)
def test_decode_builders(oracle, pattern, n, size):
    case = pc.decode_case(pattern, n, size, size)
    thr = case["iou_thr"]
    assert n <= pc.total_anchors(size, size)
    # the boxes the oracle decodes for the chosen anchors, from the deltas as the head tensors hold them
    g, off, delta = case["anchors"], 0, np.zeros((n, 4), np.float32)
    for l, s in enumerate(pc.STRIDES):
        h, w = size // s, size // s
        sel = np.flatnonzero((g >= off) & (g < off + h * w * pc.A))
        r = g[sel] - off
        for c in range(4):
            delta[sel, c] = case["heads"][3 * l + 1][4 * (r % pc.A) + c, (r // pc.A) // w, (r // pc.A) % w]
        off += h * w * pc.A
    dec = oracle.bbox_pred(pc.anchor_table(size, size)[g], delta)
    assert np.array_equal(dec, oracle.clip_boxes(dec, size, size)), "a decoded box reaches the clip"
    assert np.abs(dec - case["targets"]).max(initial=0) < 1e-3
    _check_geometry(dec, case["cid"], case["pos"], thr, net=(size, size))
    det, _, gidx, ncand = oracle.decode_nms(case["heads"], size, size, pc.CONF, thr, 1.0)
    assert ncand == n
    assert np.array_equal(gidx, case["kept_gidx"])
    if pattern == "equal":
        assert np.all(np.diff(gidx) > 0) and np.all(det[:, 4] == det[0, 4])


def test_equality_and_degenerate_boxes(oracle):
    """the oracle's answers for the survivor rule at equality, 0/0 overlaps and a NaN coordinate"""
    pair = np.array([[0, 0, 8, 8, .9], [3, 0, 11, 8, .8]], np.float32)
    assert pc.iou(pair[:1, :4], pair[1:, :4])[0] == np.float32(0.5)
    assert oracle.nms(pair, 0.5).tolist() == [0, 1]
    assert oracle.nms(pair, np.nextafter(np.float32(0.5), np.float32(0))).tolist() == [0]
    degen = np.array([[5, 5, 4, 9, .9], [5, 5, 4, 9, .8], [50, 50, 60, 60, .7]], np.float32)
    assert oracle.nms(degen, 0.45).tolist() == [0, 2]
    nan = np.array([[np.nan, 0, 8, 8, .9], [100, 100, 110, 110, .8], [300, 300, 310, 310, .7]], np.float32)
    assert oracle.nms(nan, 0.45).tolist() == [0]


@pytest.mark.parametrize("kind,s,v,n", [(k,) + p for p in pc.PLACEMENTS[:5] for k in pc.PAIR_KINDS] +
                         [("below_equal_suppressed",) + pc.PLACEMENTS[5], ("nan",) + pc.PLACEMENTS[6]])
def test_pair_builders(oracle, kind, s, v, n):
    rows, thr, want = pc.pair_case(kind, s, v, n)
    assert v % 64 in (0, 63) and v // 64 != s // 64
    assert np.all(np.diff(rows[:, 4]) < 0)
    assert np.array_equal(oracle.nms(rows, thr), want)
