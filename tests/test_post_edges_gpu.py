"""Decode -> sort -> NMS (csrc/kernels_post.hip) on constructed inputs (tests/post_cases.py) whose candidate count and kept
set are known in closed form, at every count where the kernels take another path.  Each result is compared with the CPU
oracle bit for bit (kept anchor sequence, scores, boxes, landmarks) AND with the closed form; tests/test_post_cases_cpu.py
holds the builders against the oracle without a GPU, so a failure here points at a kernel.

Boundaries and where they are crossed:
  chunk_sort_kernel   minimum bitonic size P = 64: 63 / 64 / 65 candidates; single-chunk fast path against chunk sort + merge:
                      1023 / 1024 / 1025 (test_decode_exact_counts_in_one_launch)
  merge_rank_kernel   second pass of the g0 loop (more than kSortGroup * kSortChunk = 18432 candidates: second LDS group, rank
                      accumulated across groups, own-chunk skip in the later group): 18432 / 18433 / 20328 candidates at
                      704x704 (test_704_streaming_nms_and_second_merge_group); the equal-score cases make the order depend
                      on the low key word (ascending g) across several sort chunks
  nms_chunked_kernel  kNmsChunkMin: 2048 (one workgroup) / 2049 (four); dependency chains across tiles (64), wave ownership
                      (every 16 tiles), chunks (tpc tiles) and the incremental publish of phase A; max_det cutting inside
                      chunk 1 and chunk 3
  nms_kernel<true>    RFD_NMS_CHUNKED=0 contexts on the same heads; nms_sorted up to 17408 boxes = every one of the 17
                      register words
  nms_kernel<false>   kNmsRegCap: 17408 (register form) / 17409 (streaming form) through nms_sorted; kNmsLdsBoxes = 4096:
                      4095 / 4096 / 4097 boxes and candidates, chains and pairs with the suppressor in the LDS cache and the
                      victim in L2; the 64-lane emit prefix (`per` changes at 4096 boxes)
  survivor rule       `ovr <= thresh` at equality, 0/0 overlaps, NaN
The "empty tail chunk" return of nms_chunked_kernel (split && nloc <= 0) cannot be reached (a split image has at least 33
tiles and 3 * ceil(nt / 4) < nt from there on) and has no test.
"""
import numpy as np
import pytest

import post_cases as pc

pytestmark = pytest.mark.gpu

_SCALES = (1.0, 0.625, 1 / 3)
_oracle_cache = {}


def _scale(n):
    return np.float32(_SCALES[n % 3])


def _oracle_decode(oracle, pattern, n, size=640):
    """oracle.decode_nms of a constructed case, computed once per module run"""
    key = (pattern, n, size)
    if key not in _oracle_cache:
        case = pc.decode_case(pattern, n, size, size)
        r = oracle.decode_nms(case["heads"], size, size, pc.CONF, case["iou_thr"], float(_scale(n)))
        assert r[3] == n and np.array_equal(r[2], case["kept_gidx"])      # the fixture itself: closed form == oracle
        _oracle_cache[key] = r
    return _oracle_cache[key]


def _stack(cases):
    return [np.stack([c["heads"][i] for c in cases]) for i in range(9)]


def _run(det, cases):
    heads = _stack(cases)
    sc = np.array([_scale(c["n"]) for c in cases], np.float32)
    got = det.decode_nms(heads, sc, want_gidx=True)
    return got, det.last_total.copy()


def _check(oracle, got, total, cases, patterns, size=640, max_det=None):
    for b, (case, pattern) in enumerate(zip(cases, patterns)):
        n = case["n"]
        odet, olmk, ogidx, _ = _oracle_decode(oracle, pattern, n, size)
        k = len(ogidx) if max_det is None else min(len(ogidx), max_det)
        gdet, glmk, ggidx = got[b]
        what = "%s, %d candidates (slot %d)" % (pattern, n, b)
        assert total[b] == len(case["kept_gidx"]), what
        assert np.array_equal(ggidx, case["kept_gidx"][:k]), "kept sequence differs from the closed form: " + what
        assert np.array_equal(ggidx, ogidx[:k]), "kept sequence differs from the oracle: " + what
        assert np.array_equal(gdet, odet[:k]), "scores / boxes differ: " + what
        assert np.array_equal(glmk, olmk[:k]), "landmarks differ: " + what


def _same(a, b):
    (ga, ta), (gb, tb) = a, b
    assert np.array_equal(ta, tb)
    for x, y in zip(ga, gb):
        for u, v in zip(x, y):
            assert np.array_equal(u, v)


@pytest.fixture(scope="module")
def det8(rfd):
    d = rfd.RetinaFaceDetection(image_size=(640, 640), max_batch_size=8, max_det=16800)
    yield d
    d.close()


@pytest.fixture(scope="module")
def det8_unchunked(rfd):
    """the documented fallback: RFD_NMS_CHUNKED=0 is read when the context is created; one workgroup of nms_kernel<true> per
    image whatever the candidate count"""
    with pytest.MonkeyPatch.context() as mp:
        mp.setenv("RFD_NMS_CHUNKED", "0")
        d = rfd.RetinaFaceDetection(image_size=(640, 640), max_batch_size=8, max_det=16800)
    yield d
    d.close()


@pytest.fixture(scope="module")
def det704(rfd):
    assert pc.total_anchors(704, 704) == 20328
    d = rfd.RetinaFaceDetection(image_size=(704, 704), max_batch_size=1, max_det=20328)
    yield d
    d.close()


# ---- nms_sorted: nms_kernel<true> up to 17408 boxes, nms_kernel<false> beyond ----------------------------------------------

@pytest.mark.parametrize("n", pc.NMS_SIZES)
@pytest.mark.parametrize("pattern", pc.NMS_PATTERNS)
def test_nms_sorted(oracle, det8, pattern, n):
    """chain / triples / isolated / kills at 1, 63 / 64 / 65 (one tile and the next), 1023 / 1024 / 1025 (all 16 waves own a
    tile; the second register word), 4095 / 4096 / 4097 (`per` of the emit prefix), 5121 (register word 5), 16384 and 17408
    (the last register word, full), 17409 and 20000 (streaming form: LDS cache below 4096, L2 above; in the chains a kept
    box at 4095 decides the box at 4096, in the triples an A below the edge drops a B above it)"""
    rows, thr, kept, _, _ = pc.nms_case(pattern, n)
    got = det8.nms_sorted(rows, thr)
    assert np.array_equal(got, kept), "kept set differs from the closed form"
    assert np.array_equal(got, oracle.nms(rows, thr))


@pytest.mark.parametrize("kind", pc.PAIR_KINDS)
@pytest.mark.parametrize("s,v,n", pc.PLACEMENTS)
def test_nms_sorted_equality_and_degenerates(oracle, det8, s, v, n, kind):
    """The survivor rule `ovr <= thresh` at equality (IoU exactly 0.5 at thresholds 0.5 and nextafter(0.5, 0)), a 0 / 0
    overlap and a NaN coordinate (in box 0: everything behind it goes; elsewhere: only that box), with the victim in lane 0 and in lane 63 of another tile than its
    suppressor, behind the wave-ownership hand-over, and in L2 with the suppressor in the LDS cache of the streaming form."""
    rows, thr, want = pc.pair_case(kind, s, v, n)
    got = det8.nms_sorted(rows, thr)
    assert np.array_equal(got, want), "kept set differs from the closed form"
    assert np.array_equal(got, oracle.nms(rows, thr))


# ---- decode_nms at 640x640: nms_chunked_kernel (default) and nms_kernel<true> (RFD_NMS_CHUNKED=0) ----------------------------

@pytest.mark.parametrize("counts", [pc.BATCH_COUNTS, pc.BATCH2_COUNTS], ids=["0-1-64-1024-1025-2048-2049-16800",
                                                                              "63-65-1023-2047-4095-4097-8191-12673"])
def test_decode_exact_counts_in_one_launch(oracle, det8, det8_unchunked, counts):
    """One batch-8 launch of chains with exactly these candidate counts (seeded anchor permutation: rank is unrelated to
    anchor order and to the slots the decode's atomic counter hands out): empty and one-candidate images, P = 64 exactly and
    one more, one sort chunk exactly (1024) and chunk sort + merge (1025), the last unsplit image (2048) and the first split
    one (2049), every anchor (16800).  Twice (the progress words of the first launch carry its epoch and must not satisfy the
    second), then in reversed slot order (other images on other chunk workgroups).  The unchunked context gives the same
    bits."""
    cases = [pc.decode_case("chain", n) for n in counts]
    pat = ["chain"] * len(cases)
    first = _run(det8, cases)
    _check(oracle, *first, cases, pat)
    _same(first, _run(det8, cases))
    _check(oracle, *_run(det8, cases[::-1]), cases[::-1], pat)
    _same(first, _run(det8_unchunked, cases))


@pytest.mark.parametrize("pattern,n", pc.SINGLE_640)
def test_decode_long_range_and_equal_scores(oracle, det8, det8_unchunked, pattern, n):
    """triples: A, B, C of a triple sit in different chunks of nms_chunked_kernel (B is dropped by an A published by an
    earlier chunk, C must survive the unkept B of yet another chunk).  equal: the chain with one score, so the sort is
    decided by the anchor index alone (ascending g) over 3, 8 and 17 sort chunks.  2049 = smallest split image (chunks of 9
    tiles, the last one 6), 8191, 16800 = every anchor."""
    cases = [pc.decode_case(pattern, n)]
    chunked = _run(det8, cases)
    _check(oracle, *chunked, cases, [pattern])
    _same(chunked, _run(det8_unchunked, cases))


@pytest.mark.parametrize("max_det", [5000, 13000])
def test_max_det_cuts_inside_a_chunk(rfd, oracle, max_det):
    """16800 isolated candidates (all kept: every tile of every chunk publishes 64 boxes) in chunks of 66 tiles = 4224 rows:
    max_det = 5000 cuts inside chunk 1, 13000 inside chunk 3.  count = max_det, total = 16800, the rows are the oracle's
    first max_det."""
    pattern, n = pc.TRUNCATION
    case = pc.decode_case(pattern, n)
    d = rfd.RetinaFaceDetection(image_size=(640, 640), max_batch_size=1, max_det=max_det)
    try:
        got, total = _run(d, [case])
    finally:
        d.close()
    assert total.tolist() == [16800] and len(got[0][2]) == max_det
    _check(oracle, got, total, [case], [pattern], max_det=max_det)


# ---- 704x704: 20328 anchors > kNmsRegCap (17408) and > kSortGroup * kSortChunk (18432) ----------------------------------------

@pytest.mark.parametrize("pattern,n", pc.CASES_704)
def test_704_streaming_nms_and_second_merge_group(oracle, det704, pattern, n):
    """nms_kernel<false> runs for every count of this context; 4095 / 4096 / 4097 candidates end at the LDS cache edge
    (kNmsLdsBoxes), 18432 candidates fill the 18 sort chunks of one LDS group of merge_rank_kernel exactly, 18433 and 20328
    (every anchor) need the second pass of its g0 loop: rank accumulated over both groups, the own chunk skipped in the second
    group by the workgroups of chunks 18 and 19.  Chains, and the same chains with one score (order = ascending g)."""
    cases = [pc.decode_case(pattern, n, 704, 704)]
    _check(oracle, *_run(det704, cases), cases, [pattern], size=704)
