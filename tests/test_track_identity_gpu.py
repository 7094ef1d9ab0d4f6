"""The track identities on the device (include/rfd.h, "track identities") against tests/track_identity_ref.py, bit for bit: query,
status, who, identity and id_score of every call over whole arrays filled with 0xA5 beforehand, and after every call the whole
state (the entries through rfd_tracker_get_identities, the templates through rfd_tracker_get_template, by their bits).  Both forms
are held: one tracker is driven through the host forms, a second through the device forms over torch buffers.  There is no
tolerance: both sides are the same f32 operations.  The constructed cases of tests/track_identity_cases.py are held to their
written values as well."""
import ctypes as C

import numpy as np
import pytest

import track_identity_cases as IC
import track_identity_ref as IR
import tracker_ref as TR

pytestmark = pytest.mark.gpu

MAX_DET, MAX_BATCH = 1024, 32
FILL = IC.FILL
F = np.float32


@pytest.fixture(scope="module")
def det(rfd):
    d = rfd.RetinaFaceDetection(image_size=(128, 128), max_batch_size=MAX_BATCH, max_det=MAX_DET)
    yield d
    d.close()


def _entries(tracker, stream):
    u = lambda x: int(np.asarray([x], F).view(np.uint32)[0])
    return [(e.slot, e.serial, e.identity, e.row, u(e.score), e.named, e.shots, u(e.weight)) for e in tracker.identities(stream)]


class PairHarness(IC.Harness):
    """the library twice (host forms, device forms) and the restatement, fed the same calls and compared after each; what the
    cases see is the host form's output"""
    max_det = MAX_DET

    def __init__(self, rfd, det):
        self.rfd, self.det, self.libs = rfd, det, []

    def close(self):
        for t in self.libs:
            t.close()
        self.libs = []

    def _start(self, tracker_cfg, identity_cfg):
        self.close()
        self.libs = [self.det.tracker(**tracker_cfg), self.det.tracker(**tracker_cfg)]
        for t in self.libs:
            t.enable_identities(**identity_cfg)
        self.tracker = TR.TrackerRef(**tracker_cfg)
        self.ident = IR.IdentityRef(self.tracker, MAX_DET, **identity_cfg)

    def check_state(self, what):
        for s in range(self.n_streams):
            want = self.ident.entries(s)
            for form, t in zip(("host", "device"), self.libs):
                assert _entries(t, s) == want, "%s: %s form, entries of stream %d" % (what, form, s)
                for e in want if what == "fuse" else []:            # only a fuse writes a template
                    assert t.template(s, e[1]).tobytes() == self.ident.template(s, e[1]).tobytes(), "%s: %s form, template %d of stream %d" % (what, form, e[1], s)

    def _update(self, streams, boxes, lmk, count):
        n = len(streams)
        want = self.tracker.update(streams, boxes, lmk, count, None, TR.Out(n, MAX_DET, self.max_tracks, fill=FILL))
        for t in self.libs:
            got = t.update(streams, boxes, lmk, count, None, out=self.rfd.TrackOut(n, MAX_DET, self.max_tracks, fill=FILL))
            for name, a in got.arrays():
                assert a.tobytes() == getattr(want, name).tobytes(), name
        self.check_state("update")
        return got

    def _device(self, arrays):
        """numpy arrays (or None) as torch buffers on the device"""
        import torch
        bufs = [None if a is None else torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1)).to("cuda:0") for a in arrays]
        torch.cuda.synchronize()
        return bufs, [None if b is None else b.data_ptr() for b in bufs]

    @staticmethod
    def _back(buf, like):
        return buf.cpu().numpy().view(like.dtype).reshape(like.shape)

    def _fuse(self, streams, first, row, serial, emb, weight, total, query, status):
        want_q, want_s = query.copy(), status.copy()
        self.ident.fuse(streams, first, row, serial, emb, weight, total, want_q, want_s)
        m = len(row)
        tot = None if total is None else np.asarray([total], np.int32)
        # the device form, into copies of the filled arrays
        bufs, p = self._device([tot, first, row, serial, emb, weight, query, status])
        self.libs[1].fuse_device(streams, self.rfd.rfd_track_obs(p[0], p[1], p[2], p[3]), m, p[4], p[6], p[7], weight_ptr=p[5])
        dq, ds = self._back(bufs[6], query), self._back(bufs[7], status)
        self.libs[0].fuse(streams, first, row, serial, emb, weight, total, query=query, status=status)
        for form, q, s in (("host", query, status), ("device", dq, ds)):
            assert s.tobytes() == want_s.tobytes(), "fuse, %s form: status %s, want %s" % (form, s.tolist(), want_s.tolist())
            assert q.tobytes() == want_q.tobytes(), "fuse, %s form: query" % form
        self.check_state("fuse")

    def _label(self, streams, first, row, serial, scores, rows, ids, status, total):
        self.ident.label(streams, first, row, serial, scores, rows, ids, status, total)
        tot = None if total is None else np.asarray([total], np.int32)
        bufs, p = self._device([tot, first, row, serial, scores, rows, ids, status])
        self.libs[1].label_device(streams, self.rfd.rfd_track_obs(p[0], p[1], p[2], p[3]), len(row), scores.shape[1], p[4], p[5], p[6], p[7])
        self.libs[0].label(streams, first, row, serial, scores, rows, ids, status, total)
        self.check_state("label")

    def _who(self, streams, track, count, flags, who, identity, id_score):
        in_place = flags is who
        want = [None if flags is None else flags.copy(), who.copy(), identity.copy(), id_score.copy()]
        self.ident.who(streams, track, count, want[0], want[0] if in_place else want[1], want[2], want[3])
        if in_place:
            want[1] = want[0]
        bufs, p = self._device([track, count, flags, None if in_place else who, identity, id_score])
        self.libs[1].who_device(streams, p[0], p[1], p[2] if in_place else p[3], flags_ptr=p[2], identity_ptr=p[4], id_score_ptr=p[5])
        dev = [self._back(bufs[2] if in_place else bufs[3], who), self._back(bufs[4], identity), self._back(bufs[5], id_score)]
        self.libs[0].who(streams, track, count, flags=flags, who=who, identity=identity, id_score=id_score)
        for form, got in (("host", [who, identity, id_score]), ("device", dev)):
            for name, a, b in zip(("who", "identity", "id_score"), got, want[1:]):
                assert a.tobytes() == b.tobytes(), "who, %s form: %s" % (form, name)
        if not in_place:                                                # identity and id_score are optional
            bufs, p = self._device([track, count, flags, IC.filled(who.shape, np.uint32)])
            self.libs[1].who_device(streams, p[0], p[1], p[3], flags_ptr=p[2])
            assert self._back(bufs[3], who).tobytes() == want[1].tobytes(), "who, device form without identity and id_score"
        self.check_state("who")

    def entries(self, stream):
        return _entries(self.libs[0], stream)

    def template(self, stream, serial):
        try:
            return self.libs[0].template(stream, serial)
        except Exception as e:
            assert "no such track" in str(e), e
            return None


@pytest.fixture
def pair(rfd, det):
    h = PairHarness(rfd, det)
    yield h
    h.close()


@pytest.mark.parametrize("name", sorted(IC.CASES))
def test_constructed_cases(pair, name):
    IC.CASES[name](pair)


SLOTS = {64: [0, 31, 63], 128: [0, 63, 64, 127], 256: [0, 63, 64, 127, 128, 255]}


@pytest.mark.parametrize("dim,max_tracks", [(32, 64), (64, 128), (96, 256), (512, 128), (1024, 256)])
def test_every_lane_count_and_slot_word(pair, dim, max_tracks):
    """max_tracks births fill the slots in row order; a second frame keeps the tracks at the ends of every word of 64 slots alive
    (max_missed 0).  Their embeddings are dense, so every lane that owns an element takes part (dim 32: lanes 32..63 own none;
    dim 96: half the lanes own two), twice each with different weights; then names, then who over rows of all of them."""
    h = pair
    h.start(max_tracks=max_tracks, dim=dim)
    h.frames([(0, list(range(max_tracks)))])
    keep = SLOTS[max_tracks]
    track, _, _ = h.frames([(0, keep)])
    assert track[0, :len(keep)].tolist() == [k + 1 for k in keep]
    rng = np.random.default_rng(dim + max_tracks)
    obs = [(0, r, k + 1) for r, k in enumerate(keep)] + [(0, 100 + r, k + 1) for r, k in enumerate(keep)] + [(0, 1023, keep[-1] + 1)]
    m = len(obs)
    emb = rng.standard_normal((m, dim)).astype(F)
    q, st = h.fuse([0], obs, emb, weight=rng.choice([0.25, 0.5, 1.0, 3.0], size=m).astype(F))
    assert st.tolist() == [0] * m
    assert [e[0] for e in h.entries(0)] == keep and [e[6] for e in h.entries(0)] == [2] * (len(keep) - 1) + [3]
    h.label([0], obs[:len(keep)], [[(0.75, 10 + r, 20 + r), (0.25, 3, 4)] for r in range(len(keep))], st[:len(keep)])
    rows = [k + 1 for k in keep] * 3 + [0, max_tracks + 7]
    who, ident, score = h.who([0], [rows], [len(rows)], flags=[[2] * len(rows)])
    assert who[0, :len(rows)].tolist() == [10] * (3 * len(keep)) + [2, 2]
    assert ident[0, :len(keep)].tolist() == [20 + r for r in range(len(keep))]


def _drive(h, seed, n_streams, calls, frames_per_call, lag, dim, max_tracks=64):
    """a seeded sequence: every call updates the trackers with frames of random streams whose rows come from a small pool of grid
    boxes (tracks are born, end and are reborn in the same slots: max_missed 0), then delivers the embeddings of the due rows of
    the call `lag` updates ago (lag 2: some of their tracks have ended), with weights that are sometimes bad, then labels them
    with made-up gallery answers on a lattice around the thresholds, then asks who for every row of the call's frames."""
    rng = np.random.default_rng(seed)
    h.start(streams=n_streams, max_tracks=max_tracks, dim=dim)
    pending, seen = [], np.zeros(4, np.int64)
    for c in range(calls):
        streams = [int(rng.integers(0, n_streams)) for _ in range(frames_per_call)]
        items = [(s, sorted(rng.choice(6, size=int(rng.integers(2, 7)), replace=False).tolist())) for s in streams]
        n, md = len(items), h.max_det
        boxes, lmk, count = np.zeros((n, md, 5), F), np.zeros((n, md, 5, 2), F), np.zeros(n, np.int32)
        for b, (_, ks) in enumerate(items):
            count[b] = len(ks)
            boxes[b, :len(ks)] = [IC.grid_box(k) for k in ks]
        out = h._update(np.asarray(streams, np.int32), boxes, lmk, count)
        pending.append((streams, out.due_count.copy(), out.due_track.copy()))
        if len(pending) > lag:
            st_, due_count, due_track = pending.pop(0)
            first = np.concatenate([[0], np.cumsum(due_count)]).astype(np.int32)
            m = int(first[-1])
            if m:
                row = np.concatenate([np.arange(k) for k in due_count]).astype(np.int32)
                emb = rng.standard_normal((m, dim)).astype(F)
                weight = rng.choice([0.25, 0.5, 1.0, 1.0, 2.0, 0.0, np.nan], size=m).astype(F)
                total = [None, m, m + 3, max(m - 1, 0)][int(rng.integers(0, 4))]
                query, status = IC.filled((m, dim), F), IC.filled((m,), np.int32)
                h._fuse(np.asarray(st_, np.int32), first, row, due_track, emb, weight, total, query, status)
                k = int(rng.integers(1, 4))
                scores = rng.choice([0.125, 0.25, 0.375, 0.5, 0.625, 0.75, np.nan], size=(m, k)).astype(F)
                rows = rng.choice([-1, 0, 1, 2, 3], size=(m, k)).astype(np.int32)
                ids = rng.choice([-1, 5, 6], size=(m, k)).astype(np.int32)
                done = min(max(total, 0), m) if total is not None else m
                h._label(np.asarray(st_, np.int32), first, row, due_track, scores, rows, ids if c % 3 else None, status, total)
                seen += [(status[:done] == 0).sum(), (status[:done] == 1).sum(), (status[:done] == 2).sum(), 0]
        who, identity, id_score = IC.filled((n, md), np.uint32), IC.filled((n, md), np.int32), IC.filled((n, md), F)
        flags = out.flags.copy()
        h._who(np.asarray(streams, np.int32), out.track, count, flags, who, identity, id_score)
        seen[3] += int(((who & 8) != 0)[np.arange(md)[None, :] < count[:, None]].sum())
    return seen


@pytest.mark.parametrize("n_streams,lag", [(1, 0), (3, 2)])
def test_seeded_sequences_of_40_calls(pair, n_streams, lag):
    seen = _drive(pair, 11 + n_streams, n_streams, 40, 3, lag, dim=96)
    assert seen[0] > 20 and seen[2] > 5 and seen[3] > 20, seen          # fused, refused and named rows all happened
    assert lag == 0 or seen[1] > 5, seen                                 # late embeddings of ended tracks did too


def test_32_frames_per_call_of_three_interleaved_streams(pair):
    seen = _drive(pair, 5, 3, 5, 32, 0, dim=512, max_tracks=128)
    assert seen[0] > 20 and seen[1] > 20 and seen[3] > 20, seen


def test_splitting_the_observations_over_calls_gives_the_same_bits(pair):
    """twelve observations of three tracks of two streams: one call, one call each, and an uneven split"""
    outs = []
    for split in ([12], [1] * 12, [5, 1, 6]):
        h = pair
        h.start(streams=2, dim=512)
        h.frames([(0, [0, 1]), (1, [2])])
        rng = np.random.default_rng(3)
        frame_of = sorted(int(x) for x in rng.integers(0, 2, size=12))
        obs = [(b, t, int(rng.integers(1, 3)) if b == 0 else 1) for t, b in enumerate(frame_of)]
        emb, w = rng.standard_normal((12, 512)).astype(F), rng.choice([0.5, 1.0, 3.0], size=12).astype(F)
        qs, at = [], 0
        for k in split:
            part = obs[at:at + k]
            q, st = h.fuse([0, 1], part, emb[at:at + k], weight=w[at:at + k])
            assert st.tolist() == [0] * k
            qs.append(q)
            at += k
        outs.append((np.concatenate(qs).tobytes(), [h.entries(s) for s in (0, 1)], [h.template(0, 1).tobytes(), h.template(0, 2).tobytes(), h.template(1, 1).tobytes()]))
    assert outs[0] == outs[1] == outs[2]


def test_argument_errors_on_the_device(rfd, det):
    L = rfd.load_library()
    t = det.tracker(streams=2, **IC.TRACKER)
    s, a = np.zeros(1, np.int32), np.zeros(4096, np.float32)
    p = a.ctypes.data
    o = rfd.rfd_track_obs(None, p, p, p)
    calls = {"fuse": lambda n=1, m=1, k=1, obs=o, e=p: L.rfd_tracker_fuse(t._t, s.ctypes.data, n, C.byref(obs), m, e, None, p, p),
             "fuse_device": lambda n=1, m=1, k=1, obs=o, e=p: L.rfd_tracker_fuse_device(t._t, s.ctypes.data, n, C.byref(obs), m, e, None, p, p, 1),
             "label": lambda n=1, m=1, k=1, obs=o, e=p: L.rfd_tracker_label(t._t, s.ctypes.data, n, C.byref(obs), m, k, e, p, p, p),
             "label_device": lambda n=1, m=1, k=1, obs=o, e=p: L.rfd_tracker_label_device(t._t, s.ctypes.data, n, C.byref(obs), m, k, e, p, p, p, 1),
             "who": lambda n=1, m=1, k=1, obs=o, e=p: L.rfd_tracker_who(t._t, s.ctypes.data, n, e, p, None, p, None, None),
             "who_device": lambda n=1, m=1, k=1, obs=o, e=p: L.rfd_tracker_who_device(t._t, s.ctypes.data, n, e, p, None, p, None, None, 1)}
    cnt = C.c_int()
    for name, call in calls.items():                                    # identities not enabled: every call is refused
        assert call() == rfd.RFD_ERR_INVALID_ARG and b"not enabled" in L.rfd_last_error(), name
    assert L.rfd_tracker_get_identities(t._t, 0, None, 0, C.byref(cnt)) == rfd.RFD_ERR_INVALID_ARG and b"not enabled" in L.rfd_last_error()
    assert L.rfd_tracker_get_template(t._t, 0, 1, p) == rfd.RFD_ERR_INVALID_ARG and b"not enabled" in L.rfd_last_error()
    cfg = t.enable_identities(dim=64)
    assert L.rfd_tracker_identity_enable(t._t, C.byref(cfg)) == rfd.RFD_ERR_INVALID_ARG and b"already enabled" in L.rfd_last_error()
    for name, call in calls.items():
        assert call(n=MAX_BATCH + 1) == rfd.RFD_ERR_CAPACITY and b"max_batch_size" in L.rfd_last_error(), name
        assert call(n=-1) == rfd.RFD_ERR_INVALID_ARG, name
        s[0] = 2
        assert call() == rfd.RFD_ERR_INVALID_ARG and b"stream[0] = 2" in L.rfd_last_error(), name
        s[0] = 0
        assert call(e=None) == rfd.RFD_ERR_INVALID_ARG, name
        assert call(n=0, e=None) == rfd.RFD_OK, name                    # n = 0 is a no-op
        if "who" not in name:
            assert call(m=-1) == rfd.RFD_ERR_INVALID_ARG and b"m < 0" in L.rfd_last_error(), name
            assert call(m=0, e=None) == rfd.RFD_OK, name
            assert call(obs=rfd.rfd_track_obs(None, p, None, p)) == rfd.RFD_ERR_INVALID_ARG and b"obs" in L.rfd_last_error(), name
        if "label" in name:
            for k in (0, 33, -1):
                assert call(k=k) == rfd.RFD_ERR_INVALID_ARG and b"k = " in L.rfd_last_error(), (name, k)
    assert L.rfd_tracker_get_identities(t._t, 2, None, 0, C.byref(cnt)) == rfd.RFD_ERR_INVALID_ARG
    assert L.rfd_tracker_get_identities(t._t, 0, None, 1, C.byref(cnt)) == rfd.RFD_ERR_INVALID_ARG
    assert L.rfd_tracker_get_identities(t._t, 0, None, 0, C.byref(cnt)) == rfd.RFD_OK and cnt.value == 0     # nothing was enqueued
    assert L.rfd_tracker_get_template(t._t, 0, 1, p) == rfd.RFD_ERR_INVALID_ARG and b"no such track" in L.rfd_last_error()
    t.close()
    big = det.tracker(streams=4096, max_tracks=256, **IC.TRACKER)       # 4096 x 256 x 1024 x 4 bytes = 4 GiB of templates
    c = rfd.track_identity_config(dim=1024)
    assert L.rfd_tracker_identity_enable(big._t, C.byref(c)) == rfd.RFD_ERR_CAPACITY and b"1 GiB" in L.rfd_last_error()
    big.close()


def test_a_tracker_without_identities_is_what_it_was(rfd, det):
    """the same frames through a tracker that never enables identities and one that does: the same outputs and state"""
    plain, named = det.tracker(**IC.TRACKER), det.tracker(**IC.TRACKER)
    named.enable_identities(dim=64)
    boxes, lmk, count = np.zeros((2, MAX_DET, 5), F), np.zeros((2, MAX_DET, 5, 2), F), np.asarray([3, 2], np.int32)
    boxes[0, :3], boxes[1, :2] = [IC.grid_box(k) for k in (0, 1, 2)], [IC.grid_box(k) for k in (1, 4)]
    a = plain.update([0, 0], boxes, lmk, count, out=rfd.TrackOut(2, MAX_DET, 64, fill=FILL))
    b = named.update([0, 0], boxes, lmk, count, out=rfd.TrackOut(2, MAX_DET, 64, fill=FILL))
    for (name, x), (_, y) in zip(a.arrays(), b.arrays()):
        assert x.tobytes() == y.tobytes(), name
    assert [(t.slot, t.serial, t.hits) for t in plain.tracks(0)] == [(t.slot, t.serial, t.hits) for t in named.tracks(0)] == [(0, 4, 1), (1, 2, 2)]
    plain.close()
    named.close()


def test_the_whole_pipeline_in_one_stream_order(rfd, det):
    """Two 300 x 200 frames of two cameras, synthetic weights, async throughout on ONE stream with a single wait at the end:
    detect -> shot quality -> track -> rfd_align_detections_device on the due slab -> a stand-in ID model (a fixed seeded projection
    of the face tensor, a torch matmul on the same stream) -> fuse -> rfd_gallery_search_identities_device -> label -> who ->
    rfd_redact_faces_device of the confirmed rows the gallery did not name.  Afterwards the restatement is fed what the library
    left for the stages that are not under test here (detections, quality, the face list, the embeddings, the search output, so
    the gallery's documented score bound plays no part) and must give the library's query, status, state, who, identity and
    id_score bit for bit; the redacted frames are held against tests/redact_ref.py."""
    import torch

    import helpers
    import redact_ref as RR
    dev = torch.device("cuda", 0)
    det.init_synthetic_weights(1234)
    det.set_thresholds(0.0, 1.0)              # every anchor is a candidate and none is suppressed: the synthetic network has no say
    frames = [helpers.make_image(31, 200, 300), helpers.make_image(32, 200, 300)]
    n, cap, max_faces, dim, k, streams = 2, 16, 6, 512, 2, [1, 0]
    fill32 = IC.FILL32
    t32 = lambda *shape: torch.full(shape, fill32, dtype=torch.int32, device=dev)
    bufs = [torch.from_numpy(np.ascontiguousarray(f)).to(dev) for f in frames]
    dsts = [torch.full((200 * 300 * 3,), 0x5A, dtype=torch.uint8, device=dev) for _ in frames]
    d_boxes, d_lmk, d_count, d_total, d_quality = t32(n, MAX_DET, 5), t32(n, MAX_DET, 10), t32(n), t32(n), t32(n, MAX_DET)
    z = dict(track=t32(n, MAX_DET), flags=t32(n, MAX_DET), stats=t32(n, 4), ended=t32(n, 64), due_boxes=t32(n, MAX_DET, 5),
             due_landmarks=t32(n, MAX_DET, 10), due_count=t32(n), due_total=t32(n), due_track=t32(n, MAX_DET))
    fl = dict(total=t32(1), first=t32(n + 1), frame=t32(cap), row=t32(cap), box=t32(cap, 5), kps=t32(cap, 10), status=t32(cap),
              crops=torch.full((cap, 112, 112, 3), FILL, dtype=torch.uint8, device=dev), tensor=torch.zeros((cap, 3, 112, 112), dtype=torch.float32, device=dev))
    gen = torch.Generator(device=dev).manual_seed(5)
    proj = torch.randn((3 * 112 * 112, dim), generator=gen, device=dev, dtype=torch.float32)          # the stand-in model
    d_emb = torch.zeros((cap, dim), dtype=torch.float32, device=dev)
    d_query, d_status = t32(cap, dim), t32(cap)
    d_scores, d_rows, d_ids = t32(cap, k), t32(cap, k), t32(cap, k)
    d_who, d_identity, d_id_score, d_applied = t32(n, MAX_DET), t32(n, MAX_DET), t32(n, MAX_DET), t32(n)
    rng = np.random.default_rng(8)
    enrolled = rng.standard_normal((8, dim)).astype(F)
    enrolled /= np.linalg.norm(enrolled, axis=1, keepdims=True)
    gallery = det.gallery(dim=dim, capacity=64)
    assert gallery.add(enrolled) == 0
    gallery.set_identities([0, 1, 2, 3, 4, 5], [100, 100, 101, 102, 103, 103])         # rows 6 and 7 stay unlabelled
    tcfg = dict(streams=2, max_tracks=64, iou_min=0.3, max_missed=5, min_score=0.0, new_score=0.0, min_hits=1, improve=1.1)
    icfg = dict(dim=dim, accept=-1.0, release=-1.0, margin=0.0)                         # the rehearsal: every non-empty top is taken
    e = rfd.face_tensor_config_extraction()
    lc = rfd.face_list_config(max_faces=max_faces)
    out = rfd.rfd_track_out(z["track"].data_ptr(), z["flags"].data_ptr(), z["stats"].data_ptr(), z["ended"].data_ptr(),
                            rfd.rfd_dets(z["due_boxes"].data_ptr(), z["due_landmarks"].data_ptr(), z["due_count"].data_ptr(), z["due_total"].data_ptr()),
                            z["due_track"].data_ptr())
    lst = rfd.rfd_face_list(fl["total"].data_ptr(), fl["first"].data_ptr(), fl["frame"].data_ptr(), fl["row"].data_ptr(), fl["box"].data_ptr(),
                            fl["kps"].data_ptr(), fl["status"].data_ptr(), fl["crops"].data_ptr())
    lst.tensors[0] = fl["tensor"].data_ptr()
    obs = rfd.rfd_track_obs(fl["total"].data_ptr(), fl["first"].data_ptr(), fl["row"].data_ptr(), z["due_track"].data_ptr())
    ptrs, shapes = [b.data_ptr() for b in bufs], [f.shape[:2] for f in frames]
    images = [(p, h, w) for p, (h, w) in zip(ptrs, shapes)]
    rcfg = dict(mode=RR.FILL, shape=RR.RECT, fill=(0, 0, 255), sel_mask=rfd.TRACK_NAMED | rfd.TRACK_CONFIRMED, sel_value=rfd.TRACK_CONFIRMED)
    det.sync()
    torch.cuda.synchronize()
    stream = torch.cuda.Stream(device=dev)

    def run(tracker):
        det.set_stream(stream.cuda_stream)
        try:
            with torch.cuda.stream(stream):
                det.detect_device(ptrs, shapes, d_boxes.data_ptr(), d_lmk.data_ptr(), d_count.data_ptr(), d_total.data_ptr(), async_=True)
                det.shot_quality(images, (d_boxes.data_ptr(), d_lmk.data_ptr(), d_count.data_ptr()), device=True,
                                 out=(d_quality.data_ptr(), None, None), async_=True)
                tracker.update_device(streams, d_boxes.data_ptr(), d_lmk.data_ptr(), d_count.data_ptr(), out, quality_ptr=d_quality.data_ptr(), async_=True)
                det.align_detections_device(ptrs, shapes, z["due_boxes"].data_ptr(), z["due_landmarks"].data_ptr(), z["due_count"].data_ptr(), [e], cap, lst,
                                            list_cfg=lc, async_=True)
                torch.matmul(fl["tensor"].view(cap, -1), proj, out=d_emb)
                tracker.fuse_device(streams, obs, cap, d_emb.data_ptr(), d_query.data_ptr(), d_status.data_ptr(), async_=True)
                gallery.search_identities_device(d_query.data_ptr(), cap, k, -np.inf, d_scores.data_ptr(), d_rows.data_ptr(), d_ids.data_ptr(), async_=True)
                tracker.label_device(streams, obs, cap, k, d_scores.data_ptr(), d_rows.data_ptr(), d_ids.data_ptr(), d_status.data_ptr(), async_=True)
                tracker.who_device(streams, z["track"].data_ptr(), d_count.data_ptr(), d_who.data_ptr(), flags_ptr=z["flags"].data_ptr(),
                                   identity_ptr=d_identity.data_ptr(), id_score_ptr=d_id_score.data_ptr(), async_=True)
                det.redact_faces(images, (d_boxes.data_ptr(), d_count.data_ptr()), sel=d_who.data_ptr(), cfg=rfd.redact_config(**rcfg), device=True,
                                 dst=[(t.data_ptr(), h, w) for t, (h, w) in zip(dsts, shapes)], applied=d_applied.data_ptr(), async_=True)
            det.sync()                                                                  # the single wait
        finally:
            det.set_stream(None)
        torch.cuda.synchronize()

    # a rehearsal with accept = -1 shows the top scores this pipeline produces (everything in it is deterministic); accept then
    # goes between the lowest and the highest of them, so that the run under test names some tracks and not others
    rehearsal = det.tracker(**tcfg)
    rehearsal.enable_identities(**icfg)
    run(rehearsal)
    rehearsal.close()
    tops = d_scores.cpu().numpy().view(F).reshape(cap, k)[:n * max_faces, 0]
    tops = tops[np.isfinite(tops)]
    assert len(tops) > 1 and tops.min() < tops.max(), tops
    icfg["accept"] = float(F(np.sort(tops)[len(tops) // 2]))
    tracker = det.tracker(**tcfg)
    tracker.enable_identities(**icfg)
    run(tracker)
    host = lambda t, dt=np.int32: t.cpu().numpy().view(dt)
    boxes, lmk, count, quality = host(d_boxes, F), host(d_lmk, F).reshape(n, MAX_DET, 5, 2), host(d_count), host(d_quality, F)
    assert count.min() > 64, count
    # the tracker, restated on what detection and shot quality left
    ref_t = TR.TrackerRef(**tcfg)
    want_t = ref_t.update(streams, boxes, lmk, count, quality, TR.Out(n, MAX_DET, 64, fill=FILL))
    for name in ("track", "flags", "due_count", "due_track"):
        a = getattr(want_t, name)
        assert host(z[name], a.dtype).reshape(a.shape).tobytes() == a.tobytes(), name
    # the face list and the embeddings as the library and the stand-in model left them
    total, first, row = int(host(fl["total"])[0]), host(fl["first"]), host(fl["row"])
    assert total == n * max_faces and first.tolist() == [0, max_faces, 2 * max_faces]
    emb = host(d_emb, F).reshape(cap, dim)
    assert np.isfinite(emb[:total]).all()
    ref = IR.IdentityRef(ref_t, MAX_DET, **icfg)
    want_q, want_s = IC.filled((cap, dim), F), IC.filled((cap,), np.int32)
    ref.fuse(streams, first, row, want_t.due_track, emb, None, total, want_q, want_s)
    assert host(d_status).tobytes() == want_s.tobytes() and (want_s[:total] == 0).sum() > 1
    assert host(d_query, F).reshape(cap, dim).tobytes() == want_q.tobytes()             # the fused rows and, past the total, the fill
    scores, rows, ids = host(d_scores, F).reshape(cap, k), host(d_rows).reshape(cap, k), host(d_ids).reshape(cap, k)
    ref.label(streams, first, row, want_t.due_track, scores, rows, ids, want_s, total)
    named = 0
    for s in range(2):
        assert _entries(tracker, s) == ref.entries(s), s
        for ent in ref.entries(s):
            assert tracker.template(s, ent[1]).tobytes() == ref.template(s, ent[1]).tobytes(), (s, ent[1])
        named += sum(ent[5] for ent in ref.entries(s))
    assert 0 < named < total, named                                                     # some tracks took a name, some did not
    want_who, want_identity, want_score = IC.filled((n, MAX_DET), np.uint32), IC.filled((n, MAX_DET), np.int32), IC.filled((n, MAX_DET), F)
    ref.who(streams, want_t.track, count, want_t.flags, want_who, want_identity, want_score)
    who = host(d_who, np.uint32).reshape(n, MAX_DET)
    assert who.tobytes() == want_who.tobytes() and host(d_identity).reshape(n, MAX_DET).tobytes() == want_identity.tobytes()
    assert host(d_id_score, F).reshape(n, MAX_DET).tobytes() == want_score.tobytes()
    assert int(((who & rfd.TRACK_NAMED) != 0)[np.arange(MAX_DET)[None, :] < count[:, None]].sum()) == named
    # the redaction of the confirmed rows without a name
    want, applied = RR.run(frames, boxes, count, who, RR.config(**rcfg))
    assert host(d_applied).tolist() == applied.tolist() and applied.min() > 0
    for b in range(n):
        assert (want[b] != frames[b]).any()
        assert dsts[b].cpu().numpy().tobytes() == want[b].tobytes(), "dst %d" % b
        assert bufs[b].cpu().numpy().tobytes() == frames[b].tobytes(), "source %d" % b
    det.set_thresholds(0.7, 0.45)
    tracker.close()
    gallery.close()
