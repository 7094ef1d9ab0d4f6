"""The liveness stage and the two small rules beside it on the device (csrc/kernels_pre.hip: liveness_geometry_kernel,
liveness_tensor_kernel, liveness_decide_kernel, quality_decide_kernel, l2_normalize_kernel) at every cast, clamp, ROI clause,
workgroup boundary and tile-table shape, against tests/liveness_ref.py and the restatements in this file.

There is no tolerance anywhere here: weights and scores are compared through view(uint32), ROIs, statuses and tensors as
integers (only a NaN is compared as "is a NaN": IEEE leaves its sign and payload open).  Every output array is allocated with
PAD words behind it and pre-filled with 0xA5 bytes, in host memory for the host forms and in HBM for the device forms, and
what the call does not own must keep the fill.  The cases and their classes are tests/liveness_cases.py;
tests/test_liveness_cases_cpu.py holds them against hand-worked values without a GPU."""
import ctypes as C
import functools
import itertools

import numpy as np
import pytest

import liveness_cases as LC
import liveness_ref as R

pytestmark = pytest.mark.gpu

f32 = np.float32
BATCH = 40
PAD = 64                      # words behind every output array
FILL = 0xA5A5A5A5
THRESHOLD = 0.55


@pytest.fixture(scope="module")
def det(rfd):
    d = rfd.RetinaFaceDetection(image_size=(128, 128), max_batch_size=BATCH, max_det=64)   # no call here needs weights
    yield d
    d.close()


@functools.lru_cache(maxsize=None)
def _frame(w, h):
    return np.random.default_rng(7000 + 1000 * w + h).integers(0, 256, size=(h, w, 3), dtype=np.uint8)


# ---- output arrays with the fill behind them ------------------------------------------------------------------------------
def _host_words(words):
    return np.full(words + PAD, FILL, np.uint32)


def _dev_words(words):
    import torch
    return torch.full(((words + PAD) * 4,), 0xA5, dtype=torch.uint8, device="cuda:0")


def _read(buf):
    return buf if isinstance(buf, np.ndarray) else buf.cpu().numpy().view(np.uint32)


def _ptr(buf):
    return buf.ctypes.data if isinstance(buf, np.ndarray) else buf.data_ptr()


def _owned(buf, words, what):
    """the words the call owns; the PAD words behind them must still hold the fill"""
    a = _read(buf)
    assert a.size == words + PAD and (a[words:] == FILL).all(), "%s: written past its end" % (what,)
    return a[:words]


def _ok(rfd, status):
    assert status == rfd.RFD_OK, rfd.load_library().rfd_last_error()


# ---- the two forms of the tensor call ---------------------------------------------------------------------------------------
def _outputs(alloc, n, k, sizes):
    return dict(tensors=[alloc(n * 3 * h * w) for w, h in sizes], weights=alloc(n * k), rois=alloc(n * k * 4), status=alloc(n))


def _unpack(out, n, k, sizes, what):
    tensors = [_owned(t, n * 3 * h * w, (what, "tensor", j)).view(np.float32).reshape(n, 3, h, w) for j, (t, (w, h)) in enumerate(zip(out["tensors"], sizes))]
    return (tensors, _owned(out["weights"], n * k, (what, "weights")).view(np.float32).reshape(n, k),
            _owned(out["rois"], n * k * 4, (what, "rois")).view(np.int32).reshape(n, k, 4), _owned(out["status"], n, (what, "status")).view(np.int32))


def _boxes5(boxes):
    b = np.zeros((len(boxes), 5), np.float32)
    b[:, :4] = np.asarray(boxes, np.float32)
    b[:, 4] = 0.9
    return b


def _call_host(rfd, det, frames, boxes, found, scales, sizes, what):
    n, k = len(frames), len(scales)
    arr, keep = det._images(frames)
    cfg = rfd.liveness_config(scales, sizes)
    box, fd = _boxes5(boxes), np.ascontiguousarray(found, np.int32)
    out = _outputs(_host_words, n, k, sizes)
    ptrs = (C.c_void_p * k)(*[_ptr(t) for t in out["tensors"]])
    _ok(rfd, rfd.load_library().rfd_liveness_tensors(det._ctx, arr, n, box.ctypes.data, fd.ctypes.data, C.addressof(cfg), ptrs, _ptr(out["weights"]),
                                                    _ptr(out["rois"]), _ptr(out["status"])))
    return _unpack(out, n, k, sizes, (what, "host form"))


@functools.lru_cache(maxsize=None)
def _device_frame(w, h):
    """the frame as a strided view inside a larger buffer of 0xA5 bytes: one row above and below, two pixels left, three right
    -> (the buffer, the address of the frame's first byte, its stride)"""
    import torch
    host = np.full((h + 2, w + 5, 3), 0xA5, np.uint8)
    host[1:h + 1, 2:w + 2] = _frame(w, h)
    buf = torch.from_numpy(host).to("cuda:0")
    stride = (w + 5) * 3
    return buf, buf.data_ptr() + stride + 6, stride


def _call_device(rfd, det, frame_sizes, boxes, found, scales, sizes, what):
    import torch
    n, k = len(frame_sizes), len(scales)
    placed = [_device_frame(w, h) for w, h in frame_sizes]
    d_box, d_found = torch.from_numpy(_boxes5(boxes)).to("cuda:0"), torch.from_numpy(np.ascontiguousarray(found, np.int32)).to("cuda:0")
    out = _outputs(_dev_words, n, k, sizes)
    torch.cuda.synchronize()
    det.liveness_tensors_device([p[1] for p in placed], [(h, w) for w, h in frame_sizes], d_box.data_ptr(), d_found.data_ptr(),
                                [_ptr(t) for t in out["tensors"]], _ptr(out["weights"]), _ptr(out["rois"]), _ptr(out["status"]),
                                cfg=rfd.liveness_config(scales, sizes), strides=[p[2] for p in placed], async_=True)
    det.sync()
    torch.cuda.synchronize()
    return _unpack(out, n, k, sizes, (what, "device form"))


def _check(got, want, what):
    """bit for bit against R.batch's (tensors, weights, rois, status, ...), and the rules a negative status implies"""
    tensors, weights, rois, status = got
    wt, ww, wr, ws = want[:4]
    assert np.array_equal(status, ws), (what, status.tolist(), ws.tolist())
    assert np.array_equal(rois, wr), (what, np.argwhere(rois != wr)[:4].tolist(), rois[rois != wr][:4].tolist(), wr[rois != wr][:4].tolist())
    assert np.array_equal(weights.view(np.uint32), ww.view(np.uint32)), (what, weights.tolist(), ww.tolist())
    for j, (g, w) in enumerate(zip(tensors, wt)):
        assert g.shape == w.shape and np.array_equal(g.view(np.uint32), w.view(np.uint32)), (what, "model", j, np.argwhere(g != w)[:4].tolist())
    for i, st in enumerate(status):
        if st < 0:   # no tensors at all, weight +0.0; a face without a box reports no ROI either
            assert not weights[i].view(np.uint32).any() and not any(t[i].view(np.uint32).any() for t in tensors), (what, i)
        if st == -2:
            assert not rois[i].any(), (what, i)


# ---- every case of liveness_cases.py ----------------------------------------------------------------------------------------
_reference = {}


def _cases_of(cfg, oracle):
    """the cases of one config in batches of at most BATCH, each with its reference (computed once per session)"""
    if cfg not in _reference:
        scales, sizes = LC.CONFIGS[cfg]
        mine = [c for c in LC.cases() if c.cfg == cfg]
        batches = []
        for s in range(0, len(mine), BATCH):
            part = mine[s:s + BATCH]
            want = R.batch([_frame(c.w, c.h) for c in part], [c.box for c in part], [c.found for c in part], scales, sizes, oracle=oracle)
            batches.append((part, want))
        _reference[cfg] = batches
    return _reference[cfg]


@pytest.mark.parametrize("form", ["host", "device"])
@pytest.mark.parametrize("cfg", sorted(LC.CONFIGS))
def test_every_constructed_case(rfd, det, oracle, cfg, form):
    scales, sizes = LC.CONFIGS[cfg]
    seen = set()
    for part, want in _cases_of(cfg, oracle):
        boxes, found = [c.box for c in part], [c.found for c in part]
        what = (cfg, [c.name for c in part])
        if form == "host":
            got = _call_host(rfd, det, [_frame(c.w, c.h) for c in part], boxes, found, scales, sizes, what)
        else:
            got = _call_device(rfd, det, [(c.w, c.h) for c in part], boxes, found, scales, sizes, what)
        _check(got, want, what)
        seen.update(want[3].tolist())
    assert seen == {0, -2, -3} or cfg != "default", seen    # the default config's cases hold every status


# ---- workgroup boundaries of the geometry kernel ------------------------------------------------------------------------------
EDGE_FRAME = (64, 64)
GOOD_BOXES = [(20, 18, 40, 42), (2, 30, 20, 50), (30, 2, 50, 20), (44, 30, 62, 52), (10, 10, 50, 60)]
BAD_BOX = (20, 40, 40, 30)                         # ymax < ymin: rejected by the ROI rule (-3)
EDGE_SCALES, EDGE_SIZES = [4.0, 1.0, 2.0, 2.7], [(6, 4), (8, 8), (5, 7), (3, 2)]
KINDS = {"good": 0, "rejected": -3, "none": -2}


_edge_faces = {}


def _edge_face(kind, i, k, oracle):
    """one face of the boundary test on the reference, computed once per (kind, box, found, k) -> (R.face's dict, its box)"""
    box = BAD_BOX if kind == "rejected" else GOOD_BOXES[i % len(GOOD_BOXES)]
    found = 0 if kind == "none" else 1 + 2 * (i % 2)
    key = (box, found, k)
    if key not in _edge_faces:
        _edge_faces[key] = R.face(_frame(*EDGE_FRAME), box, found, EDGE_SCALES[:k], EDGE_SIZES[:k], oracle=oracle)
    return _edge_faces[key], box


def _arrangements(n):
    """kinds by position: every way of putting a bad face (-3 or -2) beside a good one across 15|16 and across 31|32 (where both
    positions exist; else every kind at the position that does), while positions 0, 17 and n - 1 run through the kinds too"""
    pair = [("rejected", "good"), ("good", "rejected"), ("none", "good"), ("good", "none")]
    single = [("rejected",), ("none",), ("good",)]
    first = pair if n > 16 else single if n > 15 else [()]
    second = pair if n > 32 else single if n > 31 else [()]
    names = list(KINDS)
    for a, (p, q) in enumerate(itertools.product(first, second)):
        kinds = ["good"] * n
        kinds[0], kinds[n - 1] = names[a % 3], names[(a + 1) % 3]
        if n > 17:
            kinds[17] = names[(a + 2) % 3]
        for base, ks in ((15, p), (31, q)):
            for d, kd in enumerate(ks):
                kinds[base + d] = kd
        yield kinds


@pytest.mark.parametrize("k", [1, 3, 4])
def test_geometry_workgroup_boundaries(rfd, det, oracle, k):
    """liveness_geometry_kernel takes 16 faces per workgroup and reduces a face's k validity bits through one LDS flag per face:
    a -3 at position 15 leaves position 16 untouched and the reverse, likewise across 31|32; with k < 4 the idle model slots
    write nothing (the fill behind [n][k] stays)"""
    scales, sizes = EDGE_SCALES[:k], EDGE_SIZES[:k]
    calls = 0
    for n in (15, 16, 17, 32, 33, 40):
        for a, kinds in enumerate(_arrangements(n)):
            per = [_edge_face(kd, i, k, oracle) for i, kd in enumerate(kinds)]
            faces = [p[0] for p in per]
            want = ([np.stack([f["tensors"][j] for f in faces]) for j in range(k)], np.stack([f["weights"] for f in faces]),
                    np.stack([f["rois"] for f in faces]), np.array([f["status"] for f in faces], np.int32))
            assert want[3].tolist() == [KINDS[kd] for kd in kinds]          # the reference rejects what the arrangement says
            boxes, found = [p[1] for p in per], [0 if kd == "none" else 1 + 2 * (i % 2) for i, kd in enumerate(kinds)]
            what = ("n", n, "k", k, kinds)
            _check(_call_device(rfd, det, [EDGE_FRAME] * n, boxes, found, scales, sizes, what), want, what)
            if a == 0:
                _check(_call_host(rfd, det, [_frame(*EDGE_FRAME)] * n, boxes, found, scales, sizes, what), want, what)
            calls += 1
    print("k = %d: %d arrangements" % (k, calls))


def test_found_counts_bit_0_only(rfd, det, oracle):
    found = [0, 1, 2, 3, -1, 0x7ffffffe]
    n = len(found)
    scales, sizes = LC.CONFIGS["default"]
    boxes = [GOOD_BOXES[0]] * n
    want = R.batch([_frame(*EDGE_FRAME)] * n, boxes, found, scales, sizes, oracle=oracle)
    assert want[3].tolist() == [-2, 0, -2, 0, 0, -2]
    _check(_call_host(rfd, det, [_frame(*EDGE_FRAME)] * n, boxes, found, scales, sizes, "found"), want, "found")
    _check(_call_device(rfd, det, [EDGE_FRAME] * n, boxes, found, scales, sizes, "found"), want, "found")


# ---- the flat tile table -----------------------------------------------------------------------------------------------------
TILE_SIZES = [(17, 15), (16, 16), (257, 1), (3, 2)]     # 255 px: a pixel short of a tile; one tile; a tile and a pixel; 6 px


@pytest.mark.parametrize("sizes", [TILE_SIZES, TILE_SIZES[::-1], [(257, 1), (17, 15)]], ids=["ascending", "reversed", "two"])
def test_tile_table(rfd, det, oracle, sizes):
    """live_tiles (face_plan.h) lays the 256-pixel tiles of the models end to end: every plane of every model complete and
    correct whichever model a tile count ends on, a rejected face all zero, nothing behind a model's last pixel"""
    k = len(sizes)
    scales = [1.0, 2.0, 1.5, 4.0][:k]
    boxes = [GOOD_BOXES[0], BAD_BOX, GOOD_BOXES[3], GOOD_BOXES[4], GOOD_BOXES[1]]
    found = [1, 1, 1, 0, 3]
    n = len(boxes)
    want = R.batch([_frame(*EDGE_FRAME)] * n, boxes, found, scales, sizes, oracle=oracle)
    assert want[3].tolist() == [0, -3, 0, -2, 0] and all(t[0].any() and t[4].any() for t in want[0])
    _check(_call_host(rfd, det, [_frame(*EDGE_FRAME)] * n, boxes, found, scales, sizes, sizes), want, sizes)
    _check(_call_device(rfd, det, [EDGE_FRAME] * n, boxes, found, scales, sizes, sizes), want, sizes)


# ---- tiny and thin frames ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg", ["default", "three"])
def test_tiny_and_thin_frames(rfd, det, oracle, cfg):
    """1 x 1, 2 x 2, 3 x 2, 1 x 50 and 50 x 1 with the box covering the frame, inside it and outside it; in the device form each
    frame is a strided view inside a buffer of 0xA5 bytes, so a wide load past a ROI row's end reads bytes the oracle never saw"""
    scales, sizes = LC.CONFIGS[cfg]
    frames, boxes = [], []
    for w, h in LC.TINY:
        for box in ((0, 0, w - 1, h - 1), (-1, -1, w, h), (1000, 1000, 1040, 1060), (-90, -80, -50, -20), (0, 0, 0, 0), (w - 1, h - 1, w - 1, h - 1),
                    (0.25, 0.25, w - 0.5, h - 0.5)):
            frames.append((w, h))
            boxes.append(box)
    n = len(frames)
    assert n <= BATCH
    want = R.batch([_frame(w, h) for w, h in frames], boxes, [1] * n, scales, sizes, oracle=oracle)
    by_frame = {f: [st for g, st in zip(frames, want[3].tolist()) if g == f] for f in LC.TINY}
    assert all(0 in v for v in by_frame.values()), by_frame           # every tiny frame has an accepted face
    _check(_call_host(rfd, det, [_frame(w, h) for w, h in frames], boxes, [1] * n, scales, sizes, cfg), want, cfg)
    _check(_call_device(rfd, det, frames, boxes, [1] * n, scales, sizes, cfg), want, cfg)


# ---- the decision rule ----------------------------------------------------------------------------------------------------------
def _same_f32(got, want, what):
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), (what, np.argwhere(np.isnan(got) != nan)[:4].tolist())
    assert np.array_equal(got.view(np.uint32)[~nan], want.view(np.uint32)[~nan]), (what, np.argwhere((got != want) & ~nan)[:4].tolist())


def _decide_inputs(n, k, seed, last_is_above):
    """last_is_above: whether face n - 1 scores one f32 step above the threshold (live) and face n - 2 exactly the threshold
    (not live), or the other way round"""
    rng = np.random.default_rng(seed)
    logits = [rng.uniform(-0.5, 1.5, size=(n, 3)).astype(np.float32) for _ in range(k)]
    w = rng.uniform(0.05, 1.0, size=(n, k)).astype(np.float32)
    thr, last = f32(THRESHOLD), n - 1                # n = 65: `last` is the one face of the second workgroup
    above = np.nextafter(thr, f32(1.0))
    at_last, before = (above, thr) if last_is_above else (thr, above)
    w[1] = 0.0                                       # the weights sum to +inf under a finite numerator: finite / inf = 0, not live
    w[1, 0] = w[1, k - 1] = f32(3e38)
    for x in logits:
        x[1, 1] = 0.25
    logits[k - 1][2, 1] = np.nan                     # a NaN logit: NaN score, not live
    w[3] = 0.0                                       # a face with a negative status: 0 / 0
    for i, v in ((last, at_last), (last - 1, before), (5, thr), (6, above)):
        w[i] = 0.0
        w[i, 0] = 1.0                                # v * 1 + x * 0 + ... over a weight sum of exactly 1: the score is v
        for x in logits:
            x[i, 1] = v
    return logits, w


def _decide_host(rfd, det, logits, w, n, k):
    ptrs = (C.c_void_p * k)(*[x.ctypes.data for x in logits])
    score, live = _host_words(n), _host_words(n)
    _ok(rfd, rfd.load_library().rfd_liveness_decide(det._ctx, ptrs, k, n, 3, w.ctypes.data, THRESHOLD, _ptr(score), _ptr(live)))
    return _owned(score, n, "score").view(np.float32), _owned(live, n, "live").view(np.int32)


def _decide_device(rfd, det, logits, w, n, k):
    import torch
    dl, dw = [torch.from_numpy(x).to("cuda:0") for x in logits], torch.from_numpy(w).to("cuda:0")
    score, live = _dev_words(n), _dev_words(n)
    torch.cuda.synchronize()
    det.liveness_decide_device([x.data_ptr() for x in dl], n, 3, dw.data_ptr(), _ptr(score), _ptr(live), threshold=THRESHOLD)
    det.sync()
    torch.cuda.synchronize()
    assert np.array_equal(dw.cpu().numpy(), w) and all(np.array_equal(a.cpu().numpy(), b, equal_nan=True) for a, b in zip(dl, logits))   # inputs untouched
    return _owned(score, n, "score").view(np.float32), _owned(live, n, "live").view(np.int32)


@pytest.mark.parametrize("form", ["host", "device"])
@pytest.mark.parametrize("k", [8, 16])
def test_decide_full_chunks_and_two_workgroups(rfd, det, k, form):
    """k = 8 and 16 are exactly one and two launches of kLiveDecideChunk models, n = 64 and 65 one workgroup and one face more.
    With n = 65 face 64 is the second workgroup: it scores exactly the threshold (not live) in the first call and one f32 step
    above it (live) in the third.  The calls follow one another with different n and data: for k = 16 the running sums between
    the two launches must be the call's own"""
    run = _decide_host if form == "host" else _decide_device
    for n, seed, last_is_above in ((65, 1, False), (64, 2, False), (65, 3, True)):
        logits, w = _decide_inputs(n, k, 100 * k + seed, last_is_above)
        score, live = R.decide(logits, w, THRESHOLD)
        last = n - 1
        assert score[1] == 0 and live[1] == 0 and np.isnan(score[2]) and live[2] == 0 and np.isnan(score[3]) and live[3] == 0
        hi, eq = (last, last - 1) if last_is_above else (last - 1, last)
        assert score[eq] == f32(THRESHOLD) and live[eq] == 0 and score[hi] == np.nextafter(f32(THRESHOLD), f32(1.0)) and live[hi] == 1
        assert score[5] == f32(THRESHOLD) and live[5] == 0 and live[6] == 1 and 0 < live.sum() < n
        got_score, got_live = run(rfd, det, logits, w, n, k)
        _same_f32(got_score, score, (form, k, n))
        assert np.array_equal(got_live, live), (form, k, n, np.argwhere(got_live != live)[:4].tolist())


# ---- the quality rule -------------------------------------------------------------------------------------------------------------
def _quality_ref(row, threshold):
    """face_quality.rs:159-168: max_by keeps the last of equal maxima; class 1 below the threshold falls back to class 0"""
    predict = 0
    for i in range(1, len(row)):
        if not row[predict] > row[i]:
            predict = i
    score = row[predict]
    if predict == 1 and score < threshold:
        predict, score = 0, row[0]
    return score, predict


QUALITY_ROWS = {63: [0.7, 0.7, 0.1],      # two-way tie: the last index wins
                64: [0.1, 0.5, 0.2],      # class 1 AT the threshold stays
                65: [0.3, 0.3, 0.1],      # tie won by class 1, then below the threshold
                127: [0.2, 0.9, 0.9],
                128: [0.1, 0.4, 0.2],     # class 1 below the threshold -> class 0
                129: [-1.0, -1.0, -1.0]}


@pytest.mark.parametrize("classes", [1, 2, 3])
def test_quality_rule_in_three_workgroups(rfd, det, classes):
    import torch
    L = rfd.load_library()
    thr = f32(0.5)
    rows = np.random.default_rng(40 + classes).uniform(-1, 1, size=(130, classes)).astype(np.float32)
    for i, r in QUALITY_ROWS.items():
        rows[i] = r[:classes]
    want = [_quality_ref(r, thr) for r in rows]
    w_score, w_klass = np.array([w[0] for w in want], np.float32), np.array([w[1] for w in want], np.int32)
    if classes == 3:
        assert w_klass[[63, 64, 65, 127, 128, 129]].tolist() == [1, 1, 0, 2, 0, 2]
    if classes == 2:
        assert w_klass[[63, 64, 65, 127, 128, 129]].tolist() == [1, 1, 0, 1, 0, 0]

    def host(x):
        score, klass = _host_words(130), _host_words(130)
        st = L.rfd_quality_decide(det._ctx, x.ctypes.data, 130, classes, float(thr), _ptr(score), _ptr(klass))
        return st, _owned(score, 130, "score").view(np.float32), _owned(klass, 130, "klass").view(np.int32)

    def device(x):
        dx, score, klass = torch.from_numpy(x).to("cuda:0"), _dev_words(130), _dev_words(130)
        torch.cuda.synchronize()
        _ok(rfd, L.rfd_quality_decide_device(det._ctx, dx.data_ptr(), 130, classes, float(thr), _ptr(score), _ptr(klass)))
        det.sync()
        torch.cuda.synchronize()
        return _owned(score, 130, "score").view(np.float32), _owned(klass, 130, "klass").view(np.int32)

    st, score, klass = host(rows)
    assert st == rfd.RFD_OK and np.array_equal(klass, w_klass) and np.array_equal(score.view(np.uint32), w_score.view(np.uint32))
    score, klass = device(rows)
    assert np.array_equal(klass, w_klass) and np.array_equal(score.view(np.uint32), w_score.view(np.uint32))
    for first, later in ((64, 100), (129, None)):   # the reference panics on a NaN: the host entry names the FIRST such row
        bad = rows.copy()
        bad[first, classes - 1] = np.nan
        if later is not None:
            bad[later, 0] = np.nan
        st, _, _ = host(bad)
        assert st == rfd.RFD_ERR_INVALID_ARG and ("frame %d hold" % first) in L.rfd_last_error().decode(), L.rfd_last_error()
        score, klass = device(bad)
        nan = np.zeros(130, bool)
        nan[[first] + ([later] if later is not None else [])] = True
        assert (klass[nan] == -1).all() and np.isnan(score[nan]).all()
        assert np.array_equal(klass[~nan], w_klass[~nan]) and np.array_equal(score.view(np.uint32)[~nan], w_score.view(np.uint32)[~nan])


# ---- embedding normalisation, bit for bit -------------------------------------------------------------------------------------------
def _l2_ref(x):
    """the order l2_normalize_kernel documents, in numpy f32 (every array operation is one IEEE rounding per element): lane l
    sums x[i]^2 for i = l, l + 64, ... ascending; s[l] = s[l] + s[l ^ off] for off = 32 .. 1; one sqrt; one division each"""
    n, dim = x.shape
    out = np.zeros_like(x)
    lanes = np.arange(64)
    with np.errstate(all="ignore"):
        for r in range(n):
            s = np.zeros(64, np.float32)
            for i0 in range(0, dim, 64):
                part = x[r, i0:i0 + 64]
                s[:part.size] = s[:part.size] + part * part
            for off in (32, 16, 8, 4, 2, 1):
                s = s + s[lanes ^ off]
            assert (s.view(np.uint32) == s.view(np.uint32)[0]).all() or np.isnan(s).all()    # every lane ends with the same bits
            out[r] = x[r] / np.sqrt(s[0])
    return out


def _l2_rows(n, dim, turn):
    rng = np.random.default_rng(900 + 10 * dim + n)
    x = np.zeros((n, dim), np.float32)
    for r in range(n):
        kind = (r + turn) % 6
        sign = rng.choice([-1.0, 1.0], size=dim)
        if kind == 0:      # full-mantissa normals over six binades
            x[r] = (rng.integers(2 ** 23, 2 ** 24, size=dim) * 2.0 ** rng.integers(-26, -20, size=dim) * sign).astype(np.float32)
        elif kind == 1:    # subnormals: every square underflows to 0, the norm is 0, every output is +-inf
            x[r] = (rng.integers(1, 2 ** 23, size=dim).astype(np.uint32).view(np.float32)) * sign.astype(np.float32)
        elif kind == 2:    # the sum of squares overflows to +inf: every output is +-0
            x[r] = (rng.uniform(2e19, 3e19, size=dim) * sign).astype(np.float32)
        elif kind == 3:    # a zero row: 0 / 0
            x[r] = 0.0
        elif kind == 4:    # one NaN
            x[r] = rng.normal(0, 1, size=dim).astype(np.float32)
            x[r, rng.integers(0, dim)] = np.nan
        else:              # normals whose squares are subnormal
            x[r] = (rng.uniform(1e-21, 4e-20, size=dim) * sign).astype(np.float32)
    return x


@pytest.mark.parametrize("dim", [1, 63, 64, 65, 127, 128, 512, 513])
def test_embedding_normalisation_bits(rfd, det, dim):
    import torch
    L = rfd.load_library()
    turn = [1, 63, 64, 65, 127, 128, 512, 513].index(dim)
    for n in (1, 4, 5, 9):
        x = _l2_rows(n, dim, turn)
        want = _l2_ref(x)
        if n == 9:      # what each operand row must do, on the restatement
            kinds = [(r + turn) % 6 for r in range(n)]
            assert np.isinf(want[kinds.index(1)]).all() and not (want[kinds.index(2)].view(np.uint32) & 0x7fffffff).any()
            assert np.isnan(want[kinds.index(3)]).all() and np.isnan(want[kinds.index(4)]).all() and np.isfinite(want[kinds.index(0)]).all()
        out = _host_words(n * dim)
        _ok(rfd, L.rfd_normalize_embeddings(det._ctx, x.ctypes.data, n, dim, _ptr(out)))
        _same_f32(_owned(out, n * dim, "out").view(np.float32).reshape(n, dim), want, ("host", dim, n))
        buf = _dev_words(n * dim)                  # in place: out == emb
        buf[:n * dim * 4] = torch.from_numpy(x.view(np.uint8).reshape(-1)).to("cuda:0")
        torch.cuda.synchronize()
        _ok(rfd, L.rfd_normalize_embeddings_device(det._ctx, _ptr(buf), n, dim, _ptr(buf)))
        det.sync()
        torch.cuda.synchronize()
        _same_f32(_owned(buf, n * dim, "in place").view(np.float32).reshape(n, dim), want, ("device, in place", dim, n))
