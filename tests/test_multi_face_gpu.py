"""The packed face list on the device (include/rfd.h, "every detected face of a frame": rfd_align_detections,
rfd_detect_align_all_batch, rfd_detect_all_faces_device).

Two references, both exact, so every comparison is of bytes:
  * the list itself (total, first, frame, row, box, kps) against the numpy restatement of the rule, tests/face_list_ref.py;
  * status, crop and tensors of packed face t against rfd_align_faces_tensors on the single frame frame[t] with that face's
    box and key points -- the one-face path, which tests/test_face_tensors_gpu.py and tests/test_alignment_gpu.py hold to the oracle."""
import numpy as np
import pytest

import face_list_ref as R
import helpers

pytestmark = pytest.mark.gpu

MAX_DET = 192
FILL = 0xA5               # every byte of the integer and u8 arrays a caller passes in
NAN_BITS = 0x7FA5A5A5     # every word of its float arrays: a NaN, so that nothing computed compares equal to it


def _prefilled(rfd, n, cap, cfgs, want_crops=True):
    lst = rfd.FaceList(n, cap, cfgs, want_crops=want_crops, fill=FILL)
    for a in [lst.box, lst.kps] + lst.tensors:
        a.view(np.uint32)[...] = NAN_BITS
    return lst


def _same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


@pytest.fixture(scope="module")
def det(rfd):
    d = rfd.RetinaFaceDetection(max_batch_size=8, max_det=MAX_DET)
    d.init_synthetic_weights(1234)
    yield d
    d.close()


@pytest.fixture(scope="module")
def frames8():
    return [helpers.make_image(700 + i, *((240, 320) if i % 2 == 0 else (400, 480)), n_blobs=3) for i in range(8)]


# ---- 1. the list rule on constructed detections ------------------------------------------------------------------------
SIDES = np.array([8.0, 16.0, 31.5, 32.0, 32.5, 48.0, 64.0, 100.25], np.float32)   # dyadic: every x1 + side is exact in f32


def _slab(seed, count, sides=SIDES, nan_rows=()):
    """count rows in descending score: boxes with dyadic corners and sides, key points that name their (seed, row)"""
    rng = np.random.default_rng(seed)
    x1 = rng.integers(0, 400, size=count).astype(np.float32) * np.float32(0.5)
    y1 = rng.integers(0, 300, size=count).astype(np.float32) * np.float32(0.5)
    w, h = rng.choice(sides, size=count), rng.choice(sides, size=count)
    score = np.linspace(0.99, 0.30, count).astype(np.float32) if count else np.zeros(0, np.float32)
    boxes = np.stack([x1, y1, x1 + w, y1 + h, score], 1).astype(np.float32).reshape(count, 5)
    for r, col in nan_rows:
        boxes[r, col] = np.nan
    kps = (np.float32(seed) * 1000 + np.arange(count, dtype=np.float32)[:, None] + np.arange(10, dtype=np.float32)[None, :] / 16).astype(np.float32)
    return boxes, kps.reshape(count, 5, 2)


def _check_list(det, rfd, frames, dets, max_faces, min_face_px, min_score, caps):
    full = R.face_list(dets, max_faces, min_face_px, min_score, 1 << 30)
    T = full["total"]
    lc = rfd.face_list_config(max_faces=max_faces, min_face_px=min_face_px, min_score=min_score)
    for cap in sorted({max(1, c) for c in caps(T)}):
        want = R.face_list(dets, max_faces, min_face_px, min_score, cap)
        got = det.align_detections(frames, dets, cfgs=[], cap=cap, list_cfg=lc, want_crops=False)
        v = min(T, cap)
        tag = (max_faces, min_face_px, min_score, cap, T)
        assert int(got.total[0]) == T and got.valid == v, tag
        assert _same(got.first, want["first"]), tag
        assert _same(got.frame[:v], want["frame"]) and _same(got.row[:v], want["row"]), tag
        assert _same(got.box[:v], want["box"]) and _same(got.kps[:v].reshape(v, 10), want["kps"]), tag
        assert (got.status[:v] >= -3).all() and (got.status[:v] != -1).all() and (got.status[:v] != -2).all(), tag
    return T


def _caps(T):
    return [1, T - 1, T, T + 7]


def test_list_rule_at_the_ballot_word_boundaries(rfd, det, frames8):
    """counts 0, 1, 63, 64, 65, 129, 192: below, at and above one and two 64-bit ballot words, and the full slab; an eighth
    frame whose rows all fail the size floor"""
    counts = [0, 1, 63, 64, 65, 129, MAX_DET]
    dets = [_slab(10 + i, c) for i, c in enumerate(counts)]
    dets.append(_slab(20, 50, sides=SIDES[:3]))                                   # 8, 16, 31.5: nothing reaches 32
    assert not R.row_passes(dets[7][0], 32.0, 0.0).any() and R.row_passes(dets[6][0], 0.0, 0.0).all()
    T = _check_list(det, rfd, frames8, dets, MAX_DET + 1, 0.0, 0.0, _caps)        # every row of the first seven frames
    assert T == sum(counts) + 50
    for mf in (1, 64, 65, 66, MAX_DET - 1, MAX_DET):                             # count - 1, count, count + 1 of the 65- and the 192-row frame
        _check_list(det, rfd, frames8, dets, mf, 0.0, 0.0, _caps)
    T = _check_list(det, rfd, frames8, dets, 32, 32.0, 0.0, _caps)               # the size floor: frame 7 contributes nothing
    assert 0 < T < sum(min(c, 32) for c in counts) + 32
    _check_list(det, rfd, frames8, dets, 40, 32.0, 0.5, _caps)


def test_list_rule_empty_frame_between_full_ones(rfd, det, frames8):
    dets = [_slab(30, MAX_DET), _slab(31, 0), _slab(32, MAX_DET)]
    for mf in (1, 32, MAX_DET, MAX_DET + 1):
        T = _check_list(det, rfd, frames8[:3], dets, mf, 0.0, 0.0, _caps)
        assert T == 2 * min(mf, MAX_DET)
    none = [_slab(33, 0), _slab(34, 40, sides=SIDES[:1])]                        # no face at all: T = 0, nothing written
    assert _check_list(det, rfd, frames8[:2], none, 32, 16.0, 0.0, lambda T: [1, 5]) == 0


def test_list_rule_predicate_edges(rfd, det, frames8):
    """exactly the limit passes, 31.5 against 32 fails, the narrower side decides, a NaN anywhere fails, min_score cuts a prefix"""
    rows = np.array([[10, 10, 42, 74, 0.95],        # 32 x 64: passes at 32
                     [10, 10, 74, 42, 0.94],        # 64 x 32: passes
                     [10, 10, 41.5, 74, 0.93],      # 31.5 x 64: fails
                     [10, 10, 74, 41.5, 0.92],      # 64 x 31.5: fails
                     [np.nan, 10, 74, 74, 0.91],    # NaN x1
                     [10, 10, 74, np.nan, 0.90],    # NaN y2
                     [10, 10, 74, 74, np.nan],      # NaN score
                     [10, 10, 74, 74, 0.5],         # at min_score 0.5: passes
                     [10, 10, 74, 74, 0.25],        # below it
                     [10, 10, 74, 74, 0.125]], np.float32)
    kps = _slab(40, len(rows))[1]
    assert R.row_passes(rows, 32.0, 0.5).tolist() == [True, True, False, False, False, False, False, True, False, False]
    dets = [(rows, kps), _slab(41, 70, nan_rows=[(0, 0), (63, 1), (64, 2), (65, 3), (69, 4)])]
    for mpx, ms in ((32.0, 0.5), (32.0, 0.0), (0.0, 0.5), (0.0, 0.0), (31.5, 0.25)):
        for mf in (1, 3, 32, 70):
            _check_list(det, rfd, frames8[:2], dets, mf, mpx, ms, _caps)
    got = det.align_detections(frames8[:1], dets[:1], cfgs=[], cap=8, list_cfg=rfd.face_list_config(min_face_px=32.0, min_score=0.5), want_crops=False)
    assert got.total[0] == 3 and got.row[:3].tolist() == [0, 1, 7]


# ---- 2. equivalence with the one-face path -----------------------------------------------------------------------------
def _presets(rfd):
    return [rfd.face_tensor_config_quality(), rfd.face_tensor_config_extraction()]


def _sized(rfd, preset, size):
    return rfd.face_tensor_config(size, list(preset.mean), list(preset.scale))


@pytest.fixture(scope="module")
def constructed():
    """Four frames -- a 240x320 one, one without detections, a 400x480 strided view of a wider array, and the first again in a
    second slot -- with 12 faces from helpers.make_face_kps plus the coincident-key-point faces of test_face_tensors_gpu.py
    (crop + resize fallback: status 1; fallback ROI outside the frame: status -3)."""
    small = helpers.make_image(801, 240, 320, n_blobs=5)
    wide = helpers.make_image(802, 400, 520, n_blobs=5)[:, 20:500]
    assert wide.shape == (400, 480, 3) and wide.strides[0] == 520 * 3
    frames = [small, helpers.make_image(803, 400, 480, n_blobs=2), wide, small]
    same = np.tile(np.array([[100.0, 100.0]], np.float32), (5, 1))

    def faces(seeds, h, w, extra=()):
        rows = [helpers.make_face_kps(s, h, w) for s in seeds] + list(extra)
        boxes = np.stack([b for _, b in rows]).astype(np.float32)
        boxes[:, 4] = np.linspace(0.95, 0.6, len(rows)).astype(np.float32)
        return boxes, np.stack([k for k, _ in rows]).astype(np.float32)
    fallback = [(same, np.array([60, 50, 200, 150, 0.9], np.float32)), (same, np.array([60, 50, 470, 150, 0.9], np.float32))]
    dets = [faces(range(900, 905), 240, 320), (np.zeros((0, 5), np.float32), np.zeros((0, 5, 2), np.float32)),
            faces(range(910, 914), 400, 480, fallback), faces(range(920, 923), 240, 320)]
    return frames, dets


@pytest.mark.parametrize("which", ["warp", "resized"])
def test_every_listed_face_equals_the_one_face_path(rfd, det, constructed, which):
    frames, dets = constructed
    q, e = _presets(rfd)
    cfgs = [q, e] if which == "warp" else [_sized(rfd, e, (56, 56)), _sized(rfd, q, (96, 80))]   # written by the warp / resized from crops
    T = sum(len(b) for b, _ in dets)
    assert T == 14
    outs = [det.align_detections(frames, dets, cfgs=cfgs, cap=T + 3, want_crops=wc) for wc in (True, False)]
    lst = outs[0]
    assert lst.valid == T and lst.first.tolist() == [0, 5, 5, 11, 14] and lst.frame[:T].tolist() == [0] * 5 + [2] * 6 + [3] * 3
    seen = set()
    for t in range(T):
        b, r = int(lst.frame[t]), int(lst.row[t])
        assert _same(lst.box[t], dets[b][0][r]) and _same(lst.kps[t], dets[b][1][r])
        crops, status, tensors = det.align_faces_tensors([frames[b]], [(lst.box[t], lst.kps[t])], cfgs)
        seen.add(int(status[0]))
        for o in outs:
            assert int(o.status[t]) == int(status[0]), t
            assert o.crops is None or _same(o.crops[t], crops[0]), t
            for j in range(len(cfgs)):
                assert _same(o.tensors[j][t], tensors[j][0]), (t, j, o.crops is None)
        if status[0] < 0:
            assert not crops[0].any() and not any(x[0].any() for x in tensors)
    assert seen == {0, 1, -3}, seen
    assert _same(outs[0].frame, outs[1].frame) and _same(outs[0].status, outs[1].status)


# ---- 3. the untouched tail, host form ----------------------------------------------------------------------------------
def _arrays(lst):
    return [("frame", lst.frame), ("row", lst.row), ("status", lst.status), ("box", lst.box), ("kps", lst.kps)] + \
           ([("crops", lst.crops)] if lst.crops is not None else []) + [("tensor%d" % j, t) for j, t in enumerate(lst.tensors)]


def _tail_is_untouched(arrays, v):
    for name, a in arrays:
        tail = np.ascontiguousarray(a[v:])
        tail = tail.view(np.uint32) if a.dtype == np.float32 else tail.view(np.uint8)
        assert tail.size and (tail == (NAN_BITS if a.dtype == np.float32 else FILL)).all(), "%s: rows >= %d were written" % (name, v)


def test_rows_past_the_list_stay_as_passed_host_form(rfd, det, constructed):
    frames, dets = constructed
    q = rfd.face_tensor_config_quality()
    cfgs = [q, _sized(rfd, q, (56, 56))]
    T = 14
    ref = det.align_detections(frames, dets, cfgs=cfgs, cap=T)
    big = _prefilled(rfd, len(frames), T + 7, cfgs)
    det.align_detections(frames, dets, cfgs=cfgs, cap=T + 7, out=big)
    assert big.total[0] == T and _same(big.first, ref.first)
    for (name, a), (_, w) in zip(_arrays(big), _arrays(ref)):
        assert _same(a[:T], w), name
    _tail_is_untouched(_arrays(big), T)
    cut = _prefilled(rfd, len(frames), T - 1, cfgs)
    det.align_detections(frames, dets, cfgs=cfgs, cap=T - 1, out=cut)
    assert cut.total[0] == T and cut.valid == T - 1 and _same(cut.first, ref.first)
    for (name, a), (_, w) in zip(_arrays(cut), _arrays(ref)):
        assert _same(a, w[:T - 1]), name


# ---- 4. from the network, and the device form ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def calibrated(rfd, det):
    """Four frames whose detections come from the network, one of them with none and one with more than max_faces.  Random
    weights score arbitrarily, so -- the idiom of test_face_tensors_gpu.py -- the threshold is read off the head tensors: between
    the best foreground score of the quietest flat frame and the 12th best of the busiest frame."""
    busy = [helpers.make_image(500 + i, *((240, 320) if i % 2 == 0 else (400, 480)), n_blobs=6) for i in range(6)]
    quiet = [np.zeros((240, 320, 3), np.uint8), np.full((240, 320, 3), 128, np.uint8), np.full((400, 480, 3), 255, np.uint8),
             np.full((240, 320, 3), 64, np.uint8), np.full((400, 480, 3), 192, np.uint8)]
    fg = []
    for group in (busy, quiet):                                                  # at most max_batch_size frames a pass
        _, tn, _ = det.preprocess(group)
        heads = det.forward(tn)
        fg += list(np.concatenate([heads[3 * l][:, 2:4].reshape(len(group), -1) for l in range(3)], 1))
    fg = np.stack(fg)
    best = fg.max(1)
    kth = -np.sort(-fg[:len(busy)], 1)[:, 11]
    qi = len(busy) + int(np.argmin(best[len(busy):]))
    order = np.argsort(-kth)
    lo, hi = float(best[qi]), float(kth[order[0]])
    print("best score per frame:", best.tolist(), "12th best of the busy frames:", kth.tolist())
    assert lo < hi, "no threshold separates the quiet frame from 12 candidates of a busy one"
    thr = lo + 0.5 * (hi - lo)
    det.set_thresholds(thr, 0.45)
    allf = busy + quiet
    frames = [allf[order[0]], allf[qi], allf[order[1]], allf[order[2]]]
    found = det.call_batch(frames)
    counts = [len(b) for b, _ in found]
    print("threshold %.6f, detections per frame: %s" % (thr, counts))
    assert counts[1] == 0 and max(counts) >= 2, counts
    max_faces = max(1, max(counts) // 2)                                         # so that the busiest frame has more than max_faces
    yield frames, found, max_faces
    det.set_thresholds(0.7, 0.45)


def _host_reference(rfd, det, frames, max_faces, cfgs, cap):
    lc = rfd.face_list_config(max_faces=max_faces)
    found = det.call_batch(frames)
    return det.align_detections(frames, found, cfgs=cfgs, cap=cap, list_cfg=lc), found


def test_fused_host_entry_equals_detect_then_align(rfd, det, calibrated):
    frames, found, max_faces = calibrated
    q, e = _presets(rfd)
    cfgs = [q, e, _sized(rfd, e, (56, 56))]
    lc = rfd.face_list_config(max_faces=max_faces)
    cap = 4 * max_faces
    want, again = _host_reference(rfd, det, frames, max_faces, cfgs, cap)
    assert all(_same(a[0], b[0]) and _same(a[1], b[1]) for a, b in zip(found, again))       # detect() is repeatable
    rule = R.face_list(found, max_faces, 0.0, 0.0, cap)
    T = rule["total"]
    assert T == want.total[0] and max(len(b) for b, _ in found) > max_faces and want.first[2] == want.first[1]
    assert _same(want.first, rule["first"]) and _same(want.row[:want.valid], rule["row"]) and _same(want.box[:want.valid], rule["box"])
    got = det.detect_align_all(frames, cfgs=cfgs, cap=cap, list_cfg=lc)
    assert got.total[0] == T and _same(got.first, want.first)
    for (name, a), (_, w) in zip(_arrays(got), _arrays(want)):
        assert _same(a[:want.valid], w[:want.valid]), name


def _device_list(torch, n, cap, cfgs, want_crops=True):
    """device arrays of an rfd_face_list: integers and crops of FILL bytes, floats (held as their bits) of NAN_BITS"""
    dev = torch.device("cuda", 0)
    i32 = lambda *shape: torch.full(shape, int(np.frombuffer(bytes([FILL]) * 4, np.int32)[0]), dtype=torch.int32, device=dev)
    f32 = lambda *shape: torch.full(shape, NAN_BITS, dtype=torch.int32, device=dev)
    return dict(total=i32(1), first=i32(n + 1), frame=i32(cap), row=i32(cap), status=i32(cap), box=f32(cap, 5), kps=f32(cap, 5, 2),
                crops=torch.full((cap, 112, 112, 3), FILL, dtype=torch.uint8, device=dev) if want_crops else None,
                tensors=[f32(cap, 3, c.out_h, c.out_w) for c in cfgs])


def _device_call(det, z, ptrs, shapes, cfgs, cap, lc, async_):
    det.detect_all_faces_device(ptrs, shapes, cfgs, cap, z["total"].data_ptr(), z["first"].data_ptr(), z["frame"].data_ptr(),
                                z["row"].data_ptr(), z["box"].data_ptr(), z["kps"].data_ptr(), z["status"].data_ptr(),
                                None if z["crops"] is None else z["crops"].data_ptr(), [t.data_ptr() for t in z["tensors"]],
                                list_cfg=lc, async_=async_)


def _device_arrays(z):
    i32 = lambda t: t.cpu().numpy()
    f32 = lambda t: t.cpu().numpy().view(np.float32)
    out = [("frame", i32(z["frame"])), ("row", i32(z["row"])), ("status", i32(z["status"])), ("box", f32(z["box"])), ("kps", f32(z["kps"]))]
    if z["crops"] is not None:
        out.append(("crops", z["crops"].cpu().numpy()))
    out += [("tensor%d" % j, f32(t)) for j, t in enumerate(z["tensors"])]
    return int(i32(z["total"])[0]), i32(z["first"]), out


def test_device_form_back_to_back_and_its_tail(rfd, det, calibrated):
    """rfd_detect_all_faces_device enqueued twice with async = 1, the frames in opposite orders, then one rfd_sync: both equal the
    host form of their order.  cap = T + 7 on FILL-ed device arrays: rows >= T keep every byte; cap = T - 1: all rows valid,
    total = T.  Then the synchronous form without a crops pointer."""
    import torch
    frames, _, max_faces = calibrated
    frames = [np.ascontiguousarray(f) for f in frames]
    q, e = _presets(rfd)
    cfgs = [q, e, _sized(rfd, e, (56, 56))]
    lc = rfd.face_list_config(max_faces=max_faces)
    dev = torch.device("cuda", 0)
    bufs = [torch.from_numpy(f).to(dev) for f in frames]
    orders = [[0, 1, 2, 3], [3, 2, 1, 0]]
    want = [_host_reference(rfd, det, [frames[i] for i in o], max_faces, cfgs, 4 * max_faces)[0] for o in orders]
    Ts = [int(w.total[0]) for w in want]
    assert min(Ts) >= 2 and all(w.valid == T for w, T in zip(want, Ts))
    caps = [Ts[0] + 7, Ts[1] - 1]
    outs = [_device_list(torch, 4, cap, cfgs) for cap in caps]
    torch.cuda.synchronize()
    for o, z, cap in zip(orders, outs, caps):
        _device_call(det, z, [bufs[i].data_ptr() for i in o], [frames[i].shape[:2] for i in o], cfgs, cap, lc, True)
    det.sync()
    torch.cuda.synchronize()
    for o, z, cap, w, T in zip(orders, outs, caps, want, Ts):
        total, first, arrays = _device_arrays(z)
        v = min(T, cap)
        assert total == T and _same(first, w.first), o
        for (name, a), (_, x) in zip(arrays, _arrays(w)):
            assert _same(a[:v], x[:v]), (o, name)
        if cap > T:
            _tail_is_untouched(arrays, T)
    z = _device_list(torch, 4, caps[0], cfgs, want_crops=False)
    torch.cuda.synchronize()
    _device_call(det, z, [bufs[i].data_ptr() for i in orders[0]], [frames[i].shape[:2] for i in orders[0]], cfgs, caps[0], lc, False)
    total, first, arrays = _device_arrays(z)
    assert total == Ts[0] and _same(first, want[0].first)
    for (name, a), (_, x) in zip(arrays, [p for p in _arrays(want[0]) if p[0] != "crops"]):
        assert _same(a[:Ts[0]], x[:Ts[0]]), name
    _tail_is_untouched(arrays, Ts[0])


# ---- 5. argument errors ------------------------------------------------------------------------------------------------
def test_argument_errors_are_named(rfd, det, frames8):
    import torch
    frames, dets = frames8[:2], [_slab(50, 3), _slab(51, 2)]
    q = rfd.face_tensor_config_quality()
    z = _device_list(torch, 2, 4, [q])
    bufs = [torch.from_numpy(f).to(torch.device("cuda", 0)) for f in frames]

    def entries(cfgs, cap, lc, fr=frames, ds=dets):
        yield lambda: det.align_detections(fr, ds, cfgs=cfgs, cap=cap, list_cfg=lc)
        yield lambda: det.detect_align_all(fr, cfgs=cfgs, cap=cap, list_cfg=lc)
        if len(fr) == 2 and len(cfgs) == 1:
            yield lambda: _device_call(det, z, [b.data_ptr() for b in bufs], [f.shape[:2] for f in frames], cfgs, cap, lc, False)
    cases = [([q], 4, rfd.face_list_config(max_faces=0), rfd.RFD_ERR_INVALID_ARG, "max_faces"),
             ([q], 0, rfd.face_list_config(), rfd.RFD_ERR_INVALID_ARG, "cap"),
             ([q], -3, None, rfd.RFD_ERR_INVALID_ARG, "cap"),
             ([q], 4, rfd.face_list_config(min_face_px=-1.0), rfd.RFD_ERR_INVALID_ARG, "min_face_px"),
             ([q], 4, rfd.face_list_config(min_face_px=float("nan")), rfd.RFD_ERR_INVALID_ARG, "min_face_px"),
             ([q], 4, rfd.face_list_config(min_face_px=float("inf")), rfd.RFD_ERR_INVALID_ARG, "min_face_px"),
             ([q], 4, rfd.face_list_config(min_score=float("nan")), rfd.RFD_ERR_INVALID_ARG, "min_score"),
             ([q], 4, rfd.face_list_config(min_score=float("-inf")), rfd.RFD_ERR_INVALID_ARG, "min_score"),
             ([q] * (rfd.MAX_FACE_TENSORS + 1), 4, None, rfd.RFD_ERR_CAPACITY, "RFD_MAX_FACE_TENSORS")]
    for cfgs, cap, lc, status, fragment in cases:
        for call in entries(cfgs, cap, lc):
            with pytest.raises(rfd.RfdError) as err:
                call()
            assert err.value.status == status and fragment in str(err.value), (fragment, str(err.value))
    nine = [frames[0]] * 9                                                       # n is bound by max_batch_size, cap is not
    for call in entries([q], 4, None, nine, [dets[0]] * 9):
        with pytest.raises(rfd.RfdError) as err:
            call()
        assert err.value.status == rfd.RFD_ERR_CAPACITY and "max_batch_size" in str(err.value)
    big = det.align_detections(frames, dets, cfgs=[], cap=5000, want_crops=False)
    assert big.total[0] == 5 and big.first.tolist() == [0, 3, 5]
    total, first, arrays = _device_arrays(z)                                     # no refused call wrote anything
    assert total == np.frombuffer(bytes([FILL]) * 4, np.int32)[0]
    _tail_is_untouched(arrays, 0)
