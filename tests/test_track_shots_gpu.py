"""The track shots on the device (include/rfd.h, "track shots") against tests/track_shots_ref.py, byte for byte and with no
tolerance: status, total, first, rec and crops of every call over whole arrays filled with 0xA5 beforehand (every row past the
counts included), and after every call the whole state (rfd_tracker_get_shots of every stream, rfd_tracker_get_shot_crop of every
listed track).  Both forms are held: one tracker is driven through the host forms, a second through the device forms over torch
buffers that lie at a chosen byte offset between guard bytes.  The constructed cases of tests/track_shots_cases.py are held to
their written values as well; they run on trackers without identities except where a case enables them."""
import ctypes as C

import numpy as np
import pytest

import track_identity_ref as IR
import track_shots_cases as SC
import track_shots_ref as SR
import tracker_ref as TR

pytestmark = pytest.mark.gpu

MAX_DET, MAX_BATCH = 1024, 32
FILL, GUARD, PAD = SC.FILL, 0xC3, 64
F = np.float32


@pytest.fixture(scope="module")
def det(rfd):
    d = rfd.RetinaFaceDetection(image_size=(128, 128), max_batch_size=MAX_BATCH, max_det=MAX_DET)
    yield d
    d.close()


def _shots_bytes(tracker, stream):
    return b"".join(bytes(e) for e in tracker.shots(stream))


class Guarded:
    """a numpy array as a torch buffer on the device, `off` bytes behind a 16-byte aligned address, between two guards"""

    def __init__(self, a, off=0):
        import torch
        self.like = a
        raw = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
        host = np.full(PAD + off + raw.size + PAD, GUARD, np.uint8)
        host[PAD + off:PAD + off + raw.size] = raw
        self.lo, self.hi = PAD + off, PAD + off + raw.size
        self.buf = torch.from_numpy(host).to("cuda:0")
        assert self.buf.data_ptr() % 16 == 0
        self.ptr = self.buf.data_ptr() + self.lo

    def back(self):
        """the array as the device left it; the guards on both sides must be whole"""
        host = self.buf.cpu().numpy()
        assert (host[:self.lo] == GUARD).all() and (host[self.hi:] == GUARD).all(), "a guard byte was written"
        return host[self.lo:self.hi].view(self.like.dtype).reshape(self.like.shape)


def _guarded(arrays, offs=None):
    import torch
    g = [None if a is None else Guarded(a, 0 if offs is None else offs[i]) for i, a in enumerate(arrays)]
    torch.cuda.synchronize()
    return g, [None if x is None else x.ptr for x in g]


def _host_at(a, off):
    """a copy of `a` whose bytes lie `off` bytes behind an aligned address, between guards -> (the view, the whole block)"""
    raw = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
    block = np.full(PAD + 16 + raw.size + PAD, GUARD, np.uint8)
    base = (-block.ctypes.data) % 16 + PAD + off
    block[base:base + raw.size] = raw
    return block[base:base + raw.size].view(a.dtype).reshape(a.shape), (block, base, raw.size)


def _host_guards_whole(info):
    block, base, size = info
    return bool((block[:base] == GUARD).all() and (block[base + size:] == GUARD).all())


class PairHarness(SC.Harness):
    """the library twice (host forms, device forms) and the restatement, fed the same calls and compared after each; what the
    cases see is the host form's output.  src_off / dst_off: the byte offsets of the caller's crops and of the records' crops"""
    max_det = MAX_DET
    src_off = dst_off = 0

    def __init__(self, rfd, det):
        self.rfd, self.det, self.libs = rfd, det, []

    def close(self):
        for t in self.libs:
            t.close()
        self.libs = []

    def _start(self, tracker_cfg, shot_cfg, identity_cfg):
        self.close()
        self.libs = [self.det.tracker(**tracker_cfg), self.det.tracker(**tracker_cfg)]
        for t in self.libs:
            if identity_cfg is not None:
                t.enable_identities(**identity_cfg)
            t.enable_shots(**shot_cfg)
        self.tracker = TR.TrackerRef(**tracker_cfg)
        self.ident = None if identity_cfg is None else IR.IdentityRef(self.tracker, MAX_DET, **identity_cfg)
        self.ref = SR.ShotsRef(self.tracker, MAX_DET, ident=self.ident, **shot_cfg)

    def check_state(self, what):
        for s in range(self.n_streams):
            want = self.ref.entries(s)
            for form, t in zip(("host", "device"), self.libs):
                assert _shots_bytes(t, s) == want.tobytes(), "%s: %s form, entries of stream %d" % (what, form, s)
                for e in want if what == "keep" else []:             # only a keep writes a crop
                    ser = int(e["serial"])
                    assert t.shot_crop(s, ser).tobytes() == self.ref.shot_crop(s, ser).tobytes(), "%s: %s form, crop %d of stream %d" % (what, form, ser, s)

    def _update(self, streams, boxes, lmk, count):
        n = len(streams)
        want = self.tracker.update(streams, boxes, lmk, count, None, TR.Out(n, MAX_DET, self.max_tracks, fill=FILL))
        for t in self.libs:
            got = t.update(streams, boxes, lmk, count, None, out=self.rfd.TrackOut(n, MAX_DET, self.max_tracks, fill=FILL))
            for name, a in got.arrays():
                assert a.tobytes() == getattr(want, name).tobytes(), name
        self.check_state("update")
        return got

    def _fuse(self, streams, first, row, serial, emb, weight, total, query, status):
        self.ident.fuse(streams, first, row, serial, emb, weight, total, query, status)
        for t in self.libs:                                          # the identities are tests/test_track_identity_gpu.py's to hold
            t.fuse(streams, first, row, serial, emb, weight, total)

    def _label(self, streams, first, row, serial, scores, rows, ids, status, total):
        self.ident.label(streams, first, row, serial, scores, rows, ids, status, total)
        for t in self.libs:
            t.label(streams, first, row, serial, scores, rows, ids, status, total)

    def _keep(self, streams, stamp, first, row, serial, crops, face_status, q, total, status):
        want = status.copy()
        self.ref.keep(streams, stamp, first, row, serial, crops, face_status, q, total, want)
        tot = None if total is None else np.asarray([total], np.int32)
        g, p = _guarded([tot, first, row, serial, crops, face_status, q, status], offs=[0, 0, 0, 0, self.src_off, 0, 0, 0])
        self.libs[1].keep_shots_device(streams, self.rfd.rfd_track_obs(p[0], p[1], p[2], p[3]), len(row), p[4], p[7], stamp=stamp,
                                       face_status_ptr=p[5], q_ptr=p[6])
        dev = g[7].back()
        for x in g:
            if x is not None:
                x.back()                                             # every guard, the inputs' too
        hc, info = _host_at(crops, self.src_off)
        self.libs[0].keep_shots(streams, first, row, serial, hc, stamp=stamp, face_status=face_status, q=q, total=total, status=status)
        assert _host_guards_whole(info) and hc.tobytes() == crops.tobytes()
        for form, s in (("host", status), ("device", dev)):
            assert s.tobytes() == want.tobytes(), "keep, %s form: status %s, want %s" % (form, s.tolist(), want.tolist())
        self.check_state("keep")

    def _collect(self, streams, stamp, stats, ended, cap, total, first, rec, crops):
        want = [total.copy(), first.copy(), rec.copy(), None if crops is None else crops.copy()]
        self.ref.collect(streams, stamp, stats, ended, cap, *want)
        g, p = _guarded([stats, ended, total, first, rec, crops], offs=[0, 0, 0, 0, 0, self.dst_off])
        self.libs[1].collect_ended_device(streams, p[0], p[1], cap, self.rfd.rfd_track_records(p[2], p[3], p[4], p[5]), stamp=stamp)
        dev = [None if x is None else x.back() for x in g]
        if crops is None:
            self.libs[0].collect_ended(streams, stats, ended, cap, stamp=stamp, total=total, first=first, rec=rec, with_crops=False)
        else:
            hc, info = _host_at(crops, self.dst_off)
            self.libs[0].collect_ended(streams, stats, ended, cap, stamp=stamp, total=total, first=first, rec=rec, crops=hc)
            assert _host_guards_whole(info)
            crops[...] = hc
        for form, got in (("host", [total, first, rec, crops]), ("device", dev[2:])):
            for name, a, b in zip(("total", "first", "rec", "crops"), got, want):
                assert (a is None and b is None) or a.tobytes() == b.tobytes(), "collect, %s form: %s" % (form, name)
        assert dev[0].tobytes() == stats.tobytes() and dev[1].tobytes() == ended.tobytes()
        self.check_state("collect")                                  # collect changes nothing

    def shots(self, stream):
        return np.frombuffer(_shots_bytes(self.libs[0], stream), SR.SHOT)

    def shot_crop(self, stream, serial):
        try:
            return self.libs[0].shot_crop(stream, serial)
        except Exception as e:
            assert "no such track" in str(e), e
            return None


@pytest.fixture
def pair(rfd, det):
    h = PairHarness(rfd, det)
    yield h
    h.close()


@pytest.mark.parametrize("name", sorted(SC.CASES))
def test_constructed_cases(pair, name):
    SC.CASES[name](pair)


def _round(h, crop, tag0=0):
    """three tracks; four crops offered, one superseded in the call; a better and a worse shot later; two tracks end and are
    collected with room to spare and with none"""
    h.start(crop=crop)
    h.frames([(0, [0, 1, 2])])
    obs = [(0, 0, 1), (0, 1, 2), (0, 2, 3), (0, 7, 2)]
    assert h.keep([0], obs, [tag0 + i for i in range(4)], q=[0.5, 0.25, 0.75, 0.5], stamp=[11]).tolist() == [0, 0, 0, 0]
    assert h.keep([0], obs[:2], [tag0 + 4, tag0 + 5], q=[0.75, 0.125], stamp=[12]).tolist() == [0, 3]
    assert h.stored(0, 1, tag0 + 4) and h.stored(0, 2, tag0 + 3) and h.stored(0, 3, tag0 + 2)
    out = h.frames([(0, [1])])
    for cap in (3, 1):
        total, first, rec, crops = h.collect([0], out.stats, out.ended, cap, stamp=[13])
        assert total == 2 and [int(r["serial"]) for r in rec[:min(cap, 2)]] == [1, 3][:cap]
        assert crops[0].tobytes() == h.crop(tag0 + 4).tobytes() and (cap == 1 or crops[1].tobytes() == h.crop(tag0 + 2).tobytes())
        assert SC.untouched(crops[2:]) and SC.untouched(rec[2:])


# 60 x 40 x 3 = 7200 bytes: one whole chunk of the copy kernel and a partial one
@pytest.mark.parametrize("crop", [(1, 1), (5, 5), (16, 16), (112, 112), (60, 40)])
def test_crop_sizes(pair, crop):
    _round(pair, crop)


@pytest.mark.parametrize("src_off,dst_off", [(0, 0), (1, 1), (2, 2), (3, 3), (16, 16), (0, 16), (1, 0), (2, 3), (16, 1), (0, 2)])
@pytest.mark.parametrize("crop", [(5, 5), (16, 16)])
def test_crops_at_any_byte_address(pair, crop, src_off, dst_off):
    """the caller's crops and the records' crops at byte offsets 0 .. 3 and 16 from an aligned base, guard bytes on both sides:
    16 x 16 crops (768 bytes) reach the 16-byte path where both rows are aligned, 5 x 5 crops (75 bytes) never align twice"""
    pair.src_off, pair.dst_off = src_off, dst_off
    _round(pair, crop, tag0=src_off + dst_off)


SLOTS = {64: [0, 31, 63], 128: [0, 63, 64, 127], 256: [0, 63, 64, 127, 128, 255]}


@pytest.mark.parametrize("max_tracks", [64, 128, 256])
def test_every_slot_word(pair, max_tracks):
    """max_tracks births fill the slots in row order and every track keeps a shot (more observations than a wave reads at once);
    a second frame keeps the tracks at the ends of every word of 64 slots alive, so all the others end at once: their records
    come in slot order through more than one round of 64 `ended` entries; the survivors then take a better shot"""
    h = pair
    h.start(max_tracks=max_tracks, crop=(2, 2))
    h.frames([(0, list(range(max_tracks)))])
    obs = [(0, r, r + 1) for r in range(max_tracks)]
    q = [0.25 + (r % 7) / 16 for r in range(max_tracks)]
    assert h.keep([0], obs, [r % 250 for r in range(max_tracks)], q=q, stamp=[1]).tolist() == [0] * max_tracks
    keep = SLOTS[max_tracks]
    out = h.frames([(0, keep)])
    gone = [k + 1 for k in range(max_tracks) if k not in keep]
    assert out.stats[0, 2] == len(gone) and out.ended[0, :len(gone)].tolist() == gone
    total, first, rec, crops = h.collect([0], out.stats, out.ended, max_tracks, stamp=[2])
    assert total == len(gone) and [int(r["serial"]) for r in rec[:total]] == gone
    assert all(crops[i].tobytes() == h.crop((s - 1) % 250).tobytes() for i, s in enumerate(gone))
    assert SC.untouched(rec[total:]) and SC.untouched(crops[total:])
    again = [(0, r, k + 1) for r, k in enumerate(keep)]
    assert h.keep([0], again, [200 + r for r in range(len(keep))], q=[2.0] * len(keep), stamp=[3]).tolist() == [0] * len(keep)
    assert [int(e["slot"]) for e in h.shots(0)] == keep and all(h.stored(0, k + 1, 200 + r) for r, k in enumerate(keep))


def _drive(h, seed, n_streams, calls, frames_per_call, lag, identities=None):
    """a seeded sequence: every call updates the trackers with frames of random streams whose rows come from a small pool of grid
    boxes with scores from a small lattice (max_missed 4: tracks are born, become due again when their score rises, end after five
    misses and are reborn in the same slots), collects what the update ended (directly behind it, with a cap that is sometimes
    too small), then offers the crops of the due rows of the call `lag` updates ago (lag 2: some of their tracks have ended) with
    q on a small lattice, sometimes NaN, and face statuses that are sometimes negative"""
    rng = np.random.default_rng(seed)
    h.start(streams=n_streams, crop=(5, 5), identities=identities, tracker=dict(max_missed=4))
    pending, seen, tag = [], np.zeros(5, np.int64), 0
    for c in range(calls):
        streams = [int(rng.integers(0, n_streams)) for _ in range(frames_per_call)]
        items = [(s, [(k, float(rng.choice([0.6, 0.7, 0.8, 0.9, 1.0]))) for k in sorted(rng.choice(8, size=int(rng.integers(1, 6)), replace=False).tolist())])
                 for s in streams]
        out = h.frames(items)
        stamp = [1000 * c + b for b in range(len(items))]
        cap = int(rng.choice([2, 64]))
        total, first, rec, crops = h.collect(streams, out.stats, out.ended, cap, stamp=stamp, with_crops=bool(c % 5))
        seen[3] += total
        seen[4] += int(out.stats[:, 2].sum())
        pending.append((streams, stamp, out.due_count.copy(), out.due_track.copy()))
        if len(pending) > lag:
            st_, sp_, due_count, due_track = pending.pop(0)
            first = np.concatenate([[0], np.cumsum(due_count)]).astype(np.int32)
            m = int(first[-1])
            if m:
                row = np.concatenate([np.arange(k) for k in due_count]).astype(np.int32)
                crops = np.stack([h.crop((tag + t) % 250) for t in range(m)])
                tag += m
                q = rng.choice([0.125, 0.25, 0.375, 0.5, 0.5, 0.75, np.nan], size=m).astype(F) if c % 4 else None
                fs = rng.choice([0, 0, 0, 1, -1, -3], size=m).astype(np.int32) if c % 3 else None
                total = [None, m, m + 3, max(m - 1, 0)][int(rng.integers(0, 4))]
                status = SC.filled((m,), np.int32)
                h._keep(np.asarray(st_, np.int32), np.asarray(sp_, np.int64) if c % 7 else None, first, row, due_track, crops, fs, q, total, status)
                done = min(max(total, 0), m) if total is not None else m
                seen[:3] += [(status[:done] == 0).sum(), (status[:done] == 1).sum(), (status[:done] >= 2).sum()]
    return seen


@pytest.mark.parametrize("n_streams,lag", [(1, 0), (3, 2)])
def test_seeded_sequences_of_40_calls_of_32_frames(pair, n_streams, lag):
    seen = _drive(pair, 21 + n_streams, n_streams, 40, 32, lag)
    assert seen[0] > 50 and seen[2] > 20 and seen[3] > 10 and seen[4] > seen[3], seen      # kept, refused or passed, records, endings without one
    assert lag == 0 or seen[1] > 5, seen                                                    # late crops of ended tracks


def test_the_same_observations_split_three_ways(pair):
    """twelve observations of three tracks of two streams: one call, one call each, and an uneven split"""
    outs = []
    for split in ([12], [1] * 12, [5, 1, 6]):
        h = pair
        h.start(streams=2, crop=(16, 16))
        h.frames([(0, [0, 1]), (1, [2])])
        rng = np.random.default_rng(3)
        frame_of = sorted(int(x) for x in rng.integers(0, 2, size=12))
        obs = [(b, t, int(rng.integers(1, 3)) if b == 0 else 1) for t, b in enumerate(frame_of)]
        q = rng.choice([0.25, 0.5, 0.75, 1.0], size=12).astype(F)
        sts, at = [], 0
        for k in split:
            sts += h.keep([0, 1], obs[at:at + k], range(at, at + k), q=q[at:at + k], stamp=[7, 8]).tolist()
            at += k
        outs.append((sts, [h.shots(s).tobytes() for s in (0, 1)], [h.shot_crop(0, 1).tobytes(), h.shot_crop(0, 2).tobytes(), h.shot_crop(1, 1).tobytes()]))
    assert outs[0] == outs[1] == outs[2] and 3 in outs[0][0] and 0 in outs[0][0]


def test_argument_errors_on_the_device(rfd, det):
    L = rfd.load_library()
    t = det.tracker(streams=2, **SC.IC.TRACKER)
    s, a = np.zeros(1, np.int32), np.zeros(4096, np.int64)
    p = a.ctypes.data
    o = rfd.rfd_track_obs(None, p, p, p)
    r = rfd.rfd_track_records(p, p, p, None)
    calls = {"keep": lambda n=1, m=1, cap=1, obs=o, rec=r, e=p: L.rfd_tracker_keep_shots(t._t, s.ctypes.data, None, n, C.byref(obs), m, e, None, None, p),
             "keep_device": lambda n=1, m=1, cap=1, obs=o, rec=r, e=p: L.rfd_tracker_keep_shots_device(t._t, s.ctypes.data, None, n, C.byref(obs), m, e, None, None, p, 1),
             "collect": lambda n=1, m=1, cap=1, obs=o, rec=r, e=p: L.rfd_tracker_collect_ended(t._t, s.ctypes.data, None, n, e, p, cap, C.byref(rec)),
             "collect_device": lambda n=1, m=1, cap=1, obs=o, rec=r, e=p: L.rfd_tracker_collect_ended_device(t._t, s.ctypes.data, None, n, e, p, cap, C.byref(rec), 1)}
    cnt = C.c_int()
    for name, call in calls.items():                                    # shots not enabled: every call is refused
        assert call() == rfd.RFD_ERR_INVALID_ARG and b"not enabled" in L.rfd_last_error(), name
    assert L.rfd_tracker_get_shots(t._t, 0, None, 0, C.byref(cnt)) == rfd.RFD_ERR_INVALID_ARG and b"not enabled" in L.rfd_last_error()
    assert L.rfd_tracker_get_shot_crop(t._t, 0, 1, p) == rfd.RFD_ERR_INVALID_ARG and b"not enabled" in L.rfd_last_error()
    cfg = t.enable_shots(crop_w=4, crop_h=4)
    assert L.rfd_tracker_shots_enable(t._t, C.byref(cfg)) == rfd.RFD_ERR_INVALID_ARG and b"already enabled" in L.rfd_last_error()
    for name, call in calls.items():
        assert call(n=MAX_BATCH + 1) == rfd.RFD_ERR_CAPACITY and b"max_batch_size" in L.rfd_last_error(), name
        assert call(n=-1) == rfd.RFD_ERR_INVALID_ARG and b"n < 0" in L.rfd_last_error(), name
        s[0] = 2
        assert call() == rfd.RFD_ERR_INVALID_ARG and b"stream[0] = 2" in L.rfd_last_error(), name
        s[0] = 0
        assert call(e=None) == rfd.RFD_ERR_INVALID_ARG and b"is null" in L.rfd_last_error(), name
        assert call(n=0, e=None) == rfd.RFD_OK, name                    # n = 0 is a no-op
        if "keep" in name:
            assert call(m=-1) == rfd.RFD_ERR_INVALID_ARG and b"m < 0" in L.rfd_last_error(), name
            assert call(m=0, e=None) == rfd.RFD_OK, name
            assert call(obs=rfd.rfd_track_obs(None, p, None, p)) == rfd.RFD_ERR_INVALID_ARG and b"obs" in L.rfd_last_error(), name
        else:
            for cap in (0, -1):
                assert call(cap=cap) == rfd.RFD_ERR_INVALID_ARG and b"cap < 1" in L.rfd_last_error(), (name, cap)
            for rec in (rfd.rfd_track_records(None, p, p, None), rfd.rfd_track_records(p, None, p, None), rfd.rfd_track_records(p, p, None, None)):
                assert call(rec=rec) == rfd.RFD_ERR_INVALID_ARG and b"out" in L.rfd_last_error(), name
    assert L.rfd_tracker_get_shots(t._t, 2, None, 0, C.byref(cnt)) == rfd.RFD_ERR_INVALID_ARG
    assert L.rfd_tracker_get_shots(t._t, 0, None, 1, C.byref(cnt)) == rfd.RFD_ERR_INVALID_ARG
    assert L.rfd_tracker_get_shots(t._t, 0, None, 0, C.byref(cnt)) == rfd.RFD_OK and cnt.value == 0     # nothing was enqueued
    assert L.rfd_tracker_get_shot_crop(t._t, 0, 1, p) == rfd.RFD_ERR_INVALID_ARG and b"no such track" in L.rfd_last_error()
    t.close()
    big = det.tracker(streams=4096, max_tracks=256, **SC.IC.TRACKER)    # 4096 x 256 x 112 x 112 x 3 bytes = 36.75 GiB of crops
    assert L.rfd_tracker_shots_enable(big._t, None) == rfd.RFD_ERR_CAPACITY and b"1 GiB" in L.rfd_last_error()
    big.close()


def test_a_tracker_without_shots_is_what_it_was(rfd, det):
    """the same frames through a tracker that never enables shots and one that does: the same outputs and state"""
    plain, shots = det.tracker(**SC.IC.TRACKER), det.tracker(**SC.IC.TRACKER)
    shots.enable_shots(crop_w=5, crop_h=5)
    boxes, lmk, count = np.zeros((2, MAX_DET, 5), F), np.zeros((2, MAX_DET, 5, 2), F), np.asarray([3, 2], np.int32)
    boxes[0, :3], boxes[1, :2] = [SC.IC.grid_box(k) for k in (0, 1, 2)], [SC.IC.grid_box(k) for k in (1, 4)]
    a = plain.update([0, 0], boxes, lmk, count, out=rfd.TrackOut(2, MAX_DET, 64, fill=FILL))
    b = shots.update([0, 0], boxes, lmk, count, out=rfd.TrackOut(2, MAX_DET, 64, fill=FILL))
    for (name, x), (_, y) in zip(a.arrays(), b.arrays()):
        assert x.tobytes() == y.tobytes(), name
    assert [(t.slot, t.serial, t.hits) for t in plain.tracks(0)] == [(t.slot, t.serial, t.hits) for t in shots.tracks(0)] == [(0, 4, 1), (1, 2, 2)]
    plain.close()
    shots.close()


def test_the_whole_pipeline_in_one_stream_order(rfd, det):
    """Two calls of two 300 x 200 frames of two cameras, synthetic weights, async throughout on ONE stream with a single wait at
    the end of both: detect -> shot quality -> track -> COLLECT -> rfd_align_detections_device on the due slab -> KEEP (q: a
    stand-in quality model, the mean of the face tensor, a torch reduction on the same stream) -> a stand-in ID model -> fuse ->
    rfd_gallery_search_identities_device -> label -> rfd_encode_jpeg_batch_device of the records' crops with records.total as
    count_dev.  The tracker asks for an IoU of 1 and forgives no missed frame, and the second call sees other pictures, so the
    tracks of the first call end in the second.  Afterwards the restatement is fed what the library left for the stages that are
    not under test here (detections, quality, the face list and its crops, q, the embeddings, the search output) and must give the
    library's status, records, crops and state byte for byte; the files must be tests/jpeg_encode_ref.py's encoding of the
    restatement's crops."""
    import torch

    import helpers
    import jpeg_encode_ref as JE
    dev = torch.device("cuda", 0)
    det.init_synthetic_weights(1234)
    det.set_thresholds(0.0, 1.0)              # every anchor is a candidate and none is suppressed: the synthetic network has no say
    n, cap, rcap, max_faces, dim, k, streams = 2, 16, 16, 6, 512, 2, [1, 0]
    calls = [[helpers.make_image(31, 200, 300), helpers.make_image(32, 200, 300)], [helpers.make_image(41, 200, 300), helpers.make_image(42, 200, 300)]]
    stamps = [[1000, 1001], [2000, 2001]]
    fill32 = SC.FILL32
    t32 = lambda *shape: torch.full(shape, fill32, dtype=torch.int32, device=dev)
    u8 = lambda *shape: torch.full(shape, FILL, dtype=torch.uint8, device=dev)
    cb = 112 * 112 * 3
    slot = rfd.jpeg_encode_bound(112, 112)

    def buffers(frames):
        z = dict(frames=[torch.from_numpy(np.ascontiguousarray(f)).to(dev) for f in frames],
                 boxes=t32(n, MAX_DET, 5), lmk=t32(n, MAX_DET, 10), count=t32(n), dtotal=t32(n), quality=t32(n, MAX_DET),
                 track=t32(n, MAX_DET), flags=t32(n, MAX_DET), stats=t32(n, 4), ended=t32(n, 64), due_boxes=t32(n, MAX_DET, 5),
                 due_landmarks=t32(n, MAX_DET, 10), due_count=t32(n), due_total=t32(n), due_track=t32(n, MAX_DET),
                 total=t32(1), first=t32(n + 1), frame=t32(cap), row=t32(cap), box=t32(cap, 5), kps=t32(cap, 10), status=t32(cap),
                 crops=u8(cap, 112, 112, 3), tensor=torch.zeros((cap, 3, 112, 112), dtype=torch.float32, device=dev),
                 q=torch.zeros((cap,), dtype=torch.float32, device=dev), emb=torch.zeros((cap, dim), dtype=torch.float32, device=dev),
                 keep_status=t32(cap), query=t32(cap, dim), fuse_status=t32(cap), scores=t32(cap, k), rows=t32(cap, k), ids=t32(cap, k),
                 rtotal=t32(1), rfirst=t32(n + 1), rec=u8(rcap * 80), rcrops=u8(rcap, 112, 112, 3), files=u8(rcap * slot), sizes=t32(rcap))
        return z

    bufs = [buffers(f) for f in calls]
    gen = torch.Generator(device=dev).manual_seed(5)
    proj = torch.randn((3 * 112 * 112, dim), generator=gen, device=dev, dtype=torch.float32)          # the stand-in ID model
    rng = np.random.default_rng(8)
    enrolled = rng.standard_normal((8, dim)).astype(F)
    enrolled /= np.linalg.norm(enrolled, axis=1, keepdims=True)
    gallery = det.gallery(dim=dim, capacity=64)
    assert gallery.add(enrolled) == 0
    gallery.set_identities([0, 1, 2, 3, 4, 5], [100, 100, 101, 102, 103, 103])
    tcfg = dict(streams=2, max_tracks=64, iou_min=1.0, max_missed=0, min_score=0.0, new_score=0.0, min_hits=1, improve=1.1)
    icfg = dict(dim=dim, accept=-1.0, release=-1.0, margin=0.0)                         # every non-empty top is taken
    e = rfd.face_tensor_config_extraction()
    lc = rfd.face_list_config(max_faces=max_faces)
    jcfg = rfd.jpeg_encode_config()
    tracker = det.tracker(**tcfg)
    tracker.enable_identities(**icfg)
    tracker.enable_shots()
    det.sync()
    torch.cuda.synchronize()
    stream = torch.cuda.Stream(device=dev)
    det.set_stream(stream.cuda_stream)
    try:
        with torch.cuda.stream(stream):
            for z, stamp in zip(bufs, stamps):
                P = lambda name: z[name].data_ptr()
                ptrs, shapes = [b.data_ptr() for b in z["frames"]], [(200, 300)] * n
                out = rfd.rfd_track_out(P("track"), P("flags"), P("stats"), P("ended"), rfd.rfd_dets(P("due_boxes"), P("due_landmarks"), P("due_count"), P("due_total")),
                                        P("due_track"))
                lst = rfd.rfd_face_list(P("total"), P("first"), P("frame"), P("row"), P("box"), P("kps"), P("status"), P("crops"))
                lst.tensors[0] = P("tensor")
                obs = rfd.rfd_track_obs(P("total"), P("first"), P("row"), P("due_track"))
                det.detect_device(ptrs, shapes, P("boxes"), P("lmk"), P("count"), P("dtotal"), async_=True)
                det.shot_quality([(p, h, w) for p, (h, w) in zip(ptrs, shapes)], (P("boxes"), P("lmk"), P("count")), device=True, out=(P("quality"), None, None), async_=True)
                tracker.update_device(streams, P("boxes"), P("lmk"), P("count"), out, quality_ptr=P("quality"), async_=True)
                tracker.collect_ended_device(streams, P("stats"), P("ended"), rcap, rfd.rfd_track_records(P("rtotal"), P("rfirst"), P("rec"), P("rcrops")),
                                             stamp=stamp, async_=True)
                det.align_detections_device(ptrs, shapes, P("due_boxes"), P("due_landmarks"), P("due_count"), [e], cap, lst, list_cfg=lc, async_=True)
                torch.mean(z["tensor"].view(cap, -1), dim=1, out=z["q"])
                tracker.keep_shots_device(streams, obs, cap, P("crops"), P("keep_status"), stamp=stamp, face_status_ptr=P("status"), q_ptr=P("q"), async_=True)
                torch.matmul(z["tensor"].view(cap, -1), proj, out=z["emb"])
                tracker.fuse_device(streams, obs, cap, P("emb"), P("query"), P("fuse_status"), async_=True)
                gallery.search_identities_device(P("query"), cap, k, -np.inf, P("scores"), P("rows"), P("ids"), async_=True)
                tracker.label_device(streams, obs, cap, k, P("scores"), P("rows"), P("ids"), P("fuse_status"), async_=True)
                det.encode_jpeg_device([P("rcrops") + r * cb for r in range(rcap)], [(112, 112)] * rcap, P("files"), slot, P("sizes"), cfg=jcfg,
                                       count_ptr=P("rtotal"), async_=True)
        det.sync()                                                                      # the single wait
    finally:
        det.set_stream(None)
    torch.cuda.synchronize()

    host = lambda t, dt=np.int32: t.cpu().numpy().reshape(-1).view(dt)
    ref_t = TR.TrackerRef(**tcfg)
    ref_i = IR.IdentityRef(ref_t, MAX_DET, **icfg)
    ref = SR.ShotsRef(ref_t, MAX_DET, ident=ref_i)
    listed = []
    for c, (z, stamp) in enumerate(zip(bufs, stamps)):
        boxes, lmk = host(z["boxes"], F).reshape(n, MAX_DET, 5), host(z["lmk"], F).reshape(n, MAX_DET, 5, 2)
        count, quality = host(z["count"]), host(z["quality"], F).reshape(n, MAX_DET)
        want_t = ref_t.update(streams, boxes, lmk, count, quality, TR.Out(n, MAX_DET, 64, fill=FILL))
        for name in ("track", "flags", "stats", "ended", "due_count", "due_track"):
            a = getattr(want_t, name)
            assert host(z[name], a.dtype).reshape(a.shape).tobytes() == a.tobytes(), (c, name)
        # collect, directly behind the update
        w_total, w_first, w_rec, w_crops = SC.filled((1,), np.int32), SC.filled((n + 1,), np.int32), SC.filled((rcap,), SR.RECORD), SC.filled((rcap, 112, 112, 3), np.uint8)
        ref.collect(streams, stamp, want_t.stats, want_t.ended, rcap, w_total, w_first, w_rec, w_crops)
        assert host(z["rtotal"]).tobytes() == w_total.tobytes() and host(z["rfirst"]).tobytes() == w_first.tobytes(), c
        assert host(z["rec"], np.uint8).tobytes() == w_rec.tobytes(), c
        assert host(z["rcrops"], np.uint8).tobytes() == w_crops.tobytes(), c
        T = int(w_total[0])
        listed.append(T)
        # the files of the records' crops; slots at or past the total stay untouched with size 0
        sizes, files = host(z["sizes"]), host(z["files"], np.uint8).reshape(rcap, slot)
        for r in range(rcap):
            if r < min(T, rcap):
                want = JE.encode(w_crops[r], jcfg.quality, jcfg.sampling, jcfg.restart_rows)
                assert sizes[r] == len(want) and files[r, :len(want)].tobytes() == want, (c, r)
            else:
                assert sizes[r] == 0 and (files[r] == FILL).all(), (c, r)
        # keep, fuse and label on what the face list, the stand-in models and the gallery left
        total, first, row = int(host(z["total"])[0]), host(z["first"]), host(z["row"])
        assert total == n * max_faces and first.tolist() == [0, max_faces, 2 * max_faces]
        crops, status, q = host(z["crops"], np.uint8).reshape(cap, 112, 112, 3), host(z["status"]), host(z["q"], F)
        w_keep = SC.filled((cap,), np.int32)
        ref.keep(streams, stamp, first, row, want_t.due_track, crops, status, q, total, w_keep)
        assert host(z["keep_status"]).tobytes() == w_keep.tobytes() and (w_keep[:total] == 0).sum() > 1, (c, w_keep)
        emb = host(z["emb"], F).reshape(cap, dim)
        w_q, w_s = SC.filled((cap, dim), F), SC.filled((cap,), np.int32)
        ref_i.fuse(streams, first, row, want_t.due_track, emb, None, total, w_q, w_s)
        assert host(z["fuse_status"]).tobytes() == w_s.tobytes()
        ref_i.label(streams, first, row, want_t.due_track, host(z["scores"], F).reshape(cap, k), host(z["rows"]).reshape(cap, k), host(z["ids"]).reshape(cap, k), w_s, total)
    assert listed[0] == 0 and 0 < listed[1] <= rcap, listed          # the first call's tracks ended in the second, with their pictures
    named = [int(r["named"]) for r in w_rec[:listed[1]]]
    assert sum(named) > 0 and all(int(r["end_stamp"]) in stamps[1] and int(r["first_stamp"]) in stamps[0] for r in w_rec[:listed[1]]), named
    for s in range(2):
        assert _shots_bytes(tracker, s) == ref.entries(s).tobytes(), s
        for ent in ref.entries(s):
            assert tracker.shot_crop(s, int(ent["serial"])).tobytes() == ref.shot_crop(s, int(ent["serial"])).tobytes(), (s, int(ent["serial"]))
    det.set_thresholds(0.7, 0.45)
    tracker.close()
    gallery.close()
