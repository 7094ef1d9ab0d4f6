"""The tracker on the device (include/rfd.h, "tracker") against tests/tracker_ref.py, bit for bit: track, flags, stats, ended, the
due slab and due_track of every call, and after every call the whole state through rfd_tracker_get_tracks (shot_q by its bits).
There is no tolerance: both sides are the same f32 operations.  The constructed cases of tests/tracker_cases.py are held to
their written values as well."""
import ctypes as C

import numpy as np
import pytest

import helpers
import tracker_cases as TC
import tracker_ref as TR

pytestmark = pytest.mark.gpu

MAX_DET, MAX_BATCH = 1024, 32
FILL = 0xA5
F = np.float32


@pytest.fixture(scope="module")
def det(rfd):
    d = rfd.RetinaFaceDetection(image_size=(128, 128), max_batch_size=MAX_BATCH, max_det=MAX_DET)
    yield d
    d.close()


def _state(tracker, stream):
    return [(t.slot, t.serial, np.asarray(list(t.box), F).tobytes(), t.missed, t.hits, int(np.asarray([t.shot_q], F).view(np.uint32)[0]))
            for t in tracker.tracks(stream)]


class Pair:
    """a tracker of the library and the restatement, fed the same calls and compared after each"""

    def __init__(self, rfd, det, **cfg):
        self.rfd, self.cfg = rfd, cfg
        self.lib = det.tracker(**cfg)
        self.ref = TR.TrackerRef(**cfg)
        self.streams = cfg.get("streams", 1)

    def close(self):
        self.lib.close()

    def reset(self, stream=-1):
        self.lib.reset(stream)
        self.ref.reset(stream)

    def call(self, streams, boxes, lmk, count, q=None, what=""):
        n = len(streams)
        got = self.lib.update(streams, boxes, lmk, count, q, out=self.rfd.TrackOut(n, MAX_DET, self.cfg.get("max_tracks", 64), fill=FILL))
        want = self.ref.update(streams, boxes, lmk, count, q, TR.Out(n, MAX_DET, self.cfg.get("max_tracks", 64), fill=FILL))
        for name, a in got.arrays():
            assert a.tobytes() == getattr(want, name).tobytes(), "%s %s" % (what, name)
        for s in sorted(set(int(x) for x in streams)):
            assert _state(self.lib, s) == self.ref.tracks(s), "%s state of stream %d" % (what, s)
        return got


def _case_slabs(frames):
    with_q = any("q" in f for f in frames)
    return TC.slabs(frames, MAX_DET, with_q)


@pytest.mark.parametrize("name", sorted(TC.CASES))
def test_constructed_cases_one_frame_per_call(rfd, det, name):
    case = TC.CASES[name]
    p = Pair(rfd, det, **case["cfg"])
    streams, boxes, lmk, count, q = _case_slabs(case["frames"])
    for b, f in enumerate(case["frames"]):
        if "reset" in f:
            p.reset(f["reset"])
        got = p.call(streams[b:b + 1], boxes[b:b + 1], lmk[b:b + 1], count[b:b + 1], None if q is None else q[b:b + 1], "%s frame %d" % (name, b))
        k = len(f["rows"])
        assert got.track[0, :k].tolist() == f["track"] and got.flags[0, :k].tolist() == f["flags"], (name, b)
        assert tuple(got.stats[0]) == f["stats"] and got.ended[0, :len(f["ended"])].tolist() == f["ended"], (name, b)
    p.close()


@pytest.mark.parametrize("max_tracks", [64, 128, 256])
def test_1024_rows_over_one_track(rfd, det, max_tracks):
    case = TC.crowd(max_tracks)
    p = Pair(rfd, det, **case["cfg"])
    streams, boxes, lmk, count, _ = _case_slabs(case["frames"])
    got = p.call(streams, boxes, lmk, count, None, "crowd")          # both frames in one call
    assert tuple(got.stats[1]) == (1, max_tracks - 1, 0, 1024 - max_tracks)
    assert got.track[1].tolist() == case["frames"][1]["track"] and got.flags[1].tolist() == case["frames"][1]["flags"]
    assert got.due_count.tolist() == [1, max_tracks - 1]                # min_hits 1: every birth is due; the match is not (0.9 vs 0.9 * 1.1)
    p.close()


def _grid_box(k, score):
    """box k of a 16 x 16 grid of 10 x 10 boxes, 20 apart: no two overlap"""
    x, y = 20 * (k % 16), 20 * (k // 16)
    return [x, y, x + 9, y + 9, score]


SLOTS = [0, 63, 64, 127, 128, 255]


def test_lane_and_word_boundaries(rfd, det):
    """256 births fill slots 0..255 in row order; with max_missed 1 two frames of six rows leave tracks in slots 0, 63, 64, 127,
    128 and 255 alone; frames of 1, 63, 64, 65, 1023 and 1024 rows then carry those six boxes at their ends and in the middle,
    between rows that take no part (low score) and a row that is born; a frame of the six follows each and keeps them alive.
    A count of -1 and one of max_det + 1 are clamped; a count of 0 ages."""
    p = Pair(rfd, det, max_tracks=256, iou_min=0.5, max_missed=1, min_score=0.5, new_score=0.5, min_hits=1, improve=1.1)
    max_missed_keeps = dict(s=0, rows=[_grid_box(k, 0.9) for k in SLOTS])
    frames = [dict(s=0, rows=[_grid_box(k, 0.9) for k in range(256)]), max_missed_keeps, max_missed_keeps]
    streams, boxes, lmk, count, _ = _case_slabs(frames)
    got = p.call(streams, boxes, lmk, count, None, "fill")
    assert [tuple(s) for s in got.stats] == [(0, 256, 0, 0), (6, 0, 0, 0), (6, 0, 250, 0)]
    assert got.ended[2, :250].tolist() == [k + 1 for k in range(256) if k not in SLOTS]     # ascending slot order
    assert [t[0] for t in _state(p.lib, 0)] == SLOTS
    for rows in (1, 63, 64, 65, 1023, 1024):
        body = [[5000, 5000, 5009, 5009, 0.25]] * rows                                    # below min_score
        places = sorted(set([0, rows - 1, rows // 2, 62 % rows, 63 % rows, 64 % rows]))[:6]
        for slot, at in zip(SLOTS, places):
            body[at] = _grid_box(slot, 0.75)
        if rows > 70:
            body[70] = [20 * rows, 3000, 20 * rows + 9, 3009, 0.9]                       # a birth past the first word of rows
        f = [dict(s=0, rows=body), max_missed_keeps]
        streams, boxes, lmk, count, _ = _case_slabs(f)
        got = p.call(streams, boxes, lmk, count, None, "%d rows" % rows)
        for slot, at in zip(SLOTS, places):
            assert got.track[0, at] == slot + 1 and got.flags[0, at] == TR.CONFIRMED, (rows, slot, at)
        assert got.stats[0, 0] == len(places) and got.stats[0, 1] == (1 if rows > 70 else 0)
    # the two clamped counts and an empty frame, on slabs whose every row would match or be born.  -1: no rows, the track born
    # at row 70 of the last frame ends.  max_det + 1: 1024 rows; the six match, 250 births fill the slots, 768 rows are dropped
    # (a slot born in this frame is not open to its later rows).  0: all 256 age, none ends.
    full = [dict(s=0, rows=[_grid_box(k % 256, 0.9) for k in range(1024)])] * 3
    streams, boxes, lmk, count, _ = _case_slabs(full)
    count[:] = [-1, MAX_DET + 1, 0]
    got = p.call(streams, boxes, lmk, count, None, "clamped counts")
    assert [tuple(s) for s in got.stats] == [(0, 0, 1, 0), (6, 250, 0, 768), (0, 0, 0, 0)]
    assert len(_state(p.lib, 0)) == 256 and all(t[3] == 1 for t in _state(p.lib, 0))
    p.close()


def _sequence(seed, n_streams, frames_per_stream, max_rows=10):
    """per stream a list of frames of boxes on a coarse lattice (corners multiples of 4, sides 8 or 12), so that equal IoUs and
    IoUs exactly at iou_min = 0.5 occur by themselves; scores on a lattice around the thresholds; a quality per row"""
    rng = np.random.default_rng(seed)
    seq = []
    for s in range(n_streams):
        pos = rng.integers(0, 12, size=(max_rows, 2)) * 4
        frames = []
        for _ in range(frames_per_stream):
            pos = np.clip(pos + rng.integers(-1, 2, size=pos.shape) * 4, 0, 60)
            k = int(rng.integers(0, max_rows + 1))
            pick = rng.permutation(max_rows)[:k]
            side = rng.choice([7, 11], size=(k, 2))
            score = rng.choice([0.25, 0.5, 0.625, 0.75, 0.875], size=k)
            rows = np.concatenate([pos[pick], pos[pick] + side, score[:, None]], 1).astype(F).reshape(k, 5)
            frames.append((rows, rng.choice([0.25, 0.5, 0.625, 0.78125, 1.0, np.nan], size=k).astype(F)))
        seq.append(frames)
    return seq


def _slab_of(items):
    """items: [(stream, rows [k, 5], q [k])] -> the arrays of a call"""
    n = len(items)
    boxes, lmk = np.zeros((n, MAX_DET, 5), F), np.zeros((n, MAX_DET, 5, 2), F)
    count, q = np.zeros(n, np.int32), np.zeros((n, MAX_DET), F)
    for b, (_, rows, qq) in enumerate(items):
        k = len(rows)
        count[b] = k
        boxes[b, :k], q[b, :k] = rows, qq
        lmk[b, :k] = rows[:, None, :2] + np.arange(10, dtype=F).reshape(1, 5, 2) * F(0.5)    # of the row alone: the same in every split
    return np.asarray([s for s, _, _ in items], np.int32), boxes, lmk, count, q


@pytest.mark.parametrize("max_tracks", [64, 128, 256])
def test_seeded_sequences(rfd, det, max_tracks):
    n_streams, per = 4, 200
    seq = _sequence(100 + max_tracks, n_streams, per)
    p = Pair(rfd, det, streams=n_streams, max_tracks=max_tracks, iou_min=0.5, max_missed=2, min_score=0.5, new_score=0.625, min_hits=2, improve=1.25)
    items = [(s, *seq[s][t]) for t in range(per) for s in range(n_streams)]     # interleaved: eight frames of every stream per call
    seen = np.zeros(3, np.int64)
    for at in range(0, len(items), MAX_BATCH):
        got = p.call(*_slab_of(items[at:at + MAX_BATCH]), what="frames from %d" % at)
        seen += [got.stats[:, 0].sum(), got.stats[:, 2].sum(), got.due_count.sum()]
    assert seen.min() > 100, seen          # matches, endings and due rows all happened
    p.close()


ORDERS = {
    "one_stream": (1, lambda i: 0),
    "two_interleaved": (2, lambda i: i % 2),
    "five_reversed": (5, lambda i: (31 - i) % 5),
    "thirty_two_reversed": (32, lambda i: 31 - i),
    "thirty_one_beside_one": (2, lambda i: 1 if i == 17 else 0),
}


@pytest.mark.parametrize("order", sorted(ORDERS))
def test_streams_and_call_splitting(rfd, det, order):
    """32 frames in a hostile stream order: one call of 32, 32 calls of 1 and an uneven split give identical outputs and state"""
    n_streams, stream_of = ORDERS[order]
    seq = _sequence(7, n_streams, 32, max_rows=6)
    taken = [0] * n_streams
    items = []
    for i in range(32):
        s = stream_of(i)
        items.append((s, *seq[s][taken[s]]))
        taken[s] += 1
    cfg = dict(streams=n_streams, max_tracks=64, iou_min=0.5, max_missed=1, min_score=0.5, new_score=0.5, min_hits=2, improve=1.25)
    outs = []
    for split in ([32], [1] * 32, [5, 1, 19, 7]):
        p = Pair(rfd, det, **cfg)
        parts, at = [], 0
        for m in split:
            parts.append(p.call(*_slab_of(items[at:at + m]), what="%s split %s at %d" % (order, len(split), at)))
            at += m
        names = [k for k, _ in parts[0].arrays()]
        outs.append(([np.concatenate([dict(x.arrays())[k] for x in parts]) for k in names], [_state(p.lib, s) for s in range(n_streams)]))
        p.close()
    for arrays, state in outs[1:]:
        assert state == outs[0][1]
        for a, b in zip(arrays, outs[0][0]):
            assert a.tobytes() == b.tobytes()


def test_default_config_and_argument_errors_on_the_device(rfd, det):
    c = rfd.tracker_config(det)
    thr = float(np.float32(det.cfg.confidence_threshold))
    assert (c.streams, c.max_tracks, c.max_missed, c.min_hits, c.min_score, c.new_score) == (1, 64, 5, 2, thr, thr)
    t = det.tracker(streams=3, min_score=0.5, new_score=0.5, min_hits=1)
    frames = [dict(s=0, rows=[TC.A + [0.9]])]
    streams, boxes, lmk, count, _ = TC.slabs(frames, MAX_DET, False)
    t.update(streams, boxes, lmk, count)
    before = [_state(t, s) for s in range(3)]
    assert len(before[0]) == 1
    L = rfd.load_library()

    def refused(status, text, n=1, stream=0, out=None, dets=None):
        s = np.full(max(n, 1), stream, np.int32)
        o = out if out is not None else rfd.TrackOut(max(n, 1), MAX_DET, 64)
        st = o.struct() if out is None else out
        big = np.zeros((1,), np.float32)
        d = dets if dets is not None else rfd.rfd_dets(big.ctypes.data, big.ctypes.data, big.ctypes.data, None)
        for call in (lambda: L.rfd_tracker_update(t._t, s.ctypes.data, C.byref(d), None, n, C.byref(st)),
                     lambda: L.rfd_tracker_update_device(t._t, s.ctypes.data, C.byref(d), None, n, C.byref(st), 1)):
            assert call() == status
            assert text in L.rfd_last_error().decode(), L.rfd_last_error()
    refused(rfd.RFD_ERR_CAPACITY, "max_batch_size", n=MAX_BATCH + 1)
    refused(rfd.RFD_ERR_INVALID_ARG, "stream[0] = 3", stream=3)
    refused(rfd.RFD_ERR_INVALID_ARG, "stream[0] = -1", stream=-1)
    refused(rfd.RFD_ERR_INVALID_ARG, "dets", dets=rfd.rfd_dets())
    half = rfd.TrackOut(1, MAX_DET, 64).struct()
    half.due.count = None
    refused(rfd.RFD_ERR_INVALID_ARG, "due", out=half)
    none = rfd.rfd_track_out()
    refused(rfd.RFD_ERR_INVALID_ARG, "track", out=none)
    assert L.rfd_tracker_update(t._t, None, None, None, 0, None) == rfd.RFD_OK        # n = 0 is a no-op
    assert L.rfd_tracker_reset(t._t, 3) == rfd.RFD_ERR_INVALID_ARG
    n = C.c_int()
    assert L.rfd_tracker_get_tracks(t._t, 3, None, 0, C.byref(n)) == rfd.RFD_ERR_INVALID_ARG
    assert L.rfd_tracker_get_tracks(t._t, 0, None, 0, C.byref(n)) == rfd.RFD_OK and n.value == 1     # count is not truncated to cap
    assert [_state(t, s) for s in range(3)] == before                                                  # nothing was enqueued
    t.close()


def test_device_flow_equals_the_host_forms(rfd, det):
    """Two 300 x 200 frames, synthetic weights: rfd_detect_batch_device -> rfd_tracker_update_device (async) ->
    rfd_align_detections_device on the due slab, one rfd_sync.  Everything left in HBM equals rfd_tracker_update and
    rfd_align_detections on the same slabs byte for byte, and the rows past every count hold the fill."""
    import torch
    dev = torch.device("cuda", 0)
    det.init_synthetic_weights(1234)
    det.set_thresholds(0.0, 1.0)              # every anchor is a candidate and none is suppressed: the synthetic network has no say
    frames = [helpers.make_image(31, 200, 300), helpers.make_image(32, 200, 300)]
    bufs = [torch.from_numpy(np.ascontiguousarray(f)).to(dev) for f in frames]
    fill32 = int(np.frombuffer(bytes([FILL]) * 4, np.int32)[0])
    t32 = lambda *shape: torch.full(shape, fill32, dtype=torch.int32, device=dev)
    n, cap, max_faces = 2, 16, 6
    d_boxes, d_lmk, d_count, d_total = t32(n, MAX_DET, 5), t32(n, MAX_DET, 10), t32(n), t32(n)
    z = dict(track=t32(n, MAX_DET), flags=t32(n, MAX_DET), stats=t32(n, 4), ended=t32(n, 64), due_boxes=t32(n, MAX_DET, 5),
             due_landmarks=t32(n, MAX_DET, 10), due_count=t32(n), due_total=t32(n), due_track=t32(n, MAX_DET))
    e = rfd.face_tensor_config_extraction()
    lc = rfd.face_list_config(max_faces=max_faces)
    fl = dict(total=t32(1), first=t32(n + 1), frame=t32(cap), row=t32(cap), box=t32(cap, 5), kps=t32(cap, 10), status=t32(cap),
              crops=torch.full((cap, 112, 112, 3), FILL, dtype=torch.uint8, device=dev), tensor=t32(cap, 3, 112, 112))
    cfg = dict(streams=2, max_tracks=64, iou_min=0.3, max_missed=5, min_score=0.0, new_score=0.0, min_hits=1, improve=1.1)
    tracker = det.tracker(**cfg)
    out = rfd.rfd_track_out(z["track"].data_ptr(), z["flags"].data_ptr(), z["stats"].data_ptr(), z["ended"].data_ptr(),
                            rfd.rfd_dets(z["due_boxes"].data_ptr(), z["due_landmarks"].data_ptr(), z["due_count"].data_ptr(), z["due_total"].data_ptr()),
                            z["due_track"].data_ptr())
    lst = rfd.rfd_face_list(fl["total"].data_ptr(), fl["first"].data_ptr(), fl["frame"].data_ptr(), fl["row"].data_ptr(), fl["box"].data_ptr(),
                            fl["kps"].data_ptr(), fl["status"].data_ptr(), fl["crops"].data_ptr())
    lst.tensors[0] = fl["tensor"].data_ptr()
    ptrs, shapes = [b.data_ptr() for b in bufs], [f.shape[:2] for f in frames]
    torch.cuda.synchronize()
    det.detect_device(ptrs, shapes, d_boxes.data_ptr(), d_lmk.data_ptr(), d_count.data_ptr(), d_total.data_ptr(), async_=True)
    tracker.update_device([1, 0], d_boxes.data_ptr(), d_lmk.data_ptr(), d_count.data_ptr(), out, async_=True)
    det.align_detections_device(ptrs, shapes, z["due_boxes"].data_ptr(), z["due_landmarks"].data_ptr(), z["due_count"].data_ptr(), [e], cap, lst,
                                list_cfg=lc, async_=True)
    det.sync()
    torch.cuda.synchronize()
    host = lambda t, dt=np.int32: t.cpu().numpy().view(dt)
    boxes, lmk, count = host(d_boxes, F), host(d_lmk, F).reshape(n, MAX_DET, 5, 2), host(d_count)
    assert count.min() > 64, count                       # more rows than slots: births, then drops
    # the tracker's host form on the same slabs, into arrays of the same fill
    twin = det.tracker(**cfg)
    want = twin.update([1, 0], boxes, lmk, count, out=rfd.TrackOut(n, MAX_DET, 64, fill=FILL))
    for name, a in want.arrays():
        assert host(z[name], a.dtype).reshape(a.shape).tobytes() == a.tobytes(), name
    assert [_state(tracker, s) for s in range(2)] == [_state(twin, s) for s in range(2)]
    assert want.due_count.tolist() == [64, 64] and want.stats[:, 3].min() > 0
    assert (want.track[0, count[0]:] == fill32).all() and (want.due_track[:, 64:] == fill32).all() and (want.due_boxes.view(np.int32)[:, 64:] == fill32).all()
    # the face list's host form on the due slab
    dets = [(want.due_boxes[b, :want.due_count[b]], want.due_landmarks[b, :want.due_count[b]]) for b in range(n)]
    ref = rfd.FaceList(n, cap, [e], fill=FILL)
    det.align_detections(frames, dets, cfgs=[e], cap=cap, list_cfg=lc, out=ref)
    T = int(host(fl["total"])[0])
    assert T == int(ref.total[0]) == 2 * max_faces and host(fl["first"]).tolist() == ref.first.tolist()
    for name, a in (("frame", ref.frame), ("row", ref.row), ("box", ref.box), ("kps", ref.kps), ("status", ref.status), ("crops", ref.crops), ("tensor", ref.tensors[0])):
        assert host(fl[name], a.dtype).reshape(a.shape).tobytes() == a.tobytes(), name      # the listed rows and, past them, the fill
    assert (ref.frame[T:] == fill32).all() and (ref.crops[T:] == FILL).all()
    det.set_thresholds(0.7, 0.45)
    tracker.close()
    twin.close()
