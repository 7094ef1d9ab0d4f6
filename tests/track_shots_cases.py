"""Constructed cases of the track shots (include/rfd.h, "track shots"), each with its answer written down from the construction.
Every crop is filled with a byte pattern that names its observation (crop(tag)), so "which shot is stored" and "which crop is
in the record" are read off the bytes.  A case is a function of a harness: the harness runs the calls (on the restatement alone
in tests/test_track_shots_cpu.py; on the library through its host forms AND its device forms AND the restatement, compared byte
for byte, in tests/test_track_shots_gpu.py) and the case asserts the written answers on what comes back.

The tracker under every case is that of tests/track_identity_cases.py: iou_min 0.5, max_missed 0 (a track that misses one frame
ends in it), both scores 0.5, min_hits 1, frames of grid boxes that never overlap.  So frame [0, 1, 2] of a fresh stream gives
serials 1, 2, 3 in slots 0, 1, 2, a track lives exactly as long as its grid index keeps appearing, and a birth takes the lowest
free slot, those freed in the same frame included."""
import numpy as np

import track_identity_cases as IC
import track_identity_ref as IR
import track_shots_ref as SR
import tracker_ref as TR

F = np.float32
FILL, FILL32, filled, up, down = IC.FILL, IC.FILL32, IC.filled, IC.up, IC.down
INF, NAN = float("inf"), float("nan")
I64_MIN, I64_MAX = -2 ** 63, 2 ** 63 - 1
NO_ID = (-1, -1, -INF, 0, 0, 0.0)


class Harness(IC.Harness):
    """builds the arrays of the calls; a subclass runs them (_start, _update, _fuse, _label, _keep, _collect, shots, shot_crop)"""
    max_det = 16

    def start(self, streams=1, max_tracks=64, crop=(5, 5), identities=None, tracker=None):
        """crop: (crop_w, crop_h); identities: None for a tracker without them, or the fields of their config; tracker: fields of
        the tracker's config other than the cases'"""
        self.n_streams, self.max_tracks, self.crop_w, self.crop_h = streams, max_tracks, crop[0], crop[1]
        self.dim = None if identities is None else identities.get("dim", 64)
        if identities is not None:
            identities = dict(dict(dim=64, accept=0.5, release=0.25, margin=0.125), **identities)
        self._start(dict(IC.TRACKER, streams=streams, max_tracks=max_tracks, **(tracker or {})), dict(crop_w=crop[0], crop_h=crop[1]), identities)

    def frames(self, items):
        """items: [(stream, [grid index of every row, or (grid index, score)])] -> the outputs of one update (track, stats, ended, ...)"""
        n, md = len(items), self.max_det
        boxes, lmk, count = np.zeros((n, md, 5), F), np.zeros((n, md, 5, 2), F), np.zeros(n, np.int32)
        for b, (_, ks) in enumerate(items):
            count[b] = len(ks)
            for i, k in enumerate(ks):
                boxes[b, i] = IC.grid_box(*k) if isinstance(k, tuple) else IC.grid_box(k)
        return self._update(np.asarray([s for s, _ in items], np.int32), boxes, lmk, count)

    def crop(self, tag):
        """the crop that names observation `tag`: no two tags below 251 share a first byte"""
        size = self.crop_h * self.crop_w * 3
        return ((int(tag) * 37 + np.arange(size)) % 251).astype(np.uint8).reshape(self.crop_h, self.crop_w, 3)

    def keep(self, streams, obs, tags, q=None, face_status=None, stamp=None, total=None):
        """obs: [(frame, row, serial)] in (frame, t) order, tags: the name of each observation's crop -> status [m]"""
        first, row, serial = self.obs(streams, obs)
        m = len(row)
        crops = np.stack([self.crop(t) for t in tags]).reshape(m, self.crop_h, self.crop_w, 3)
        status = filled((m,), np.int32)
        self._keep(np.asarray(streams, np.int32), None if stamp is None else np.asarray(stamp, np.int64), first, row, serial, crops,
                   None if face_status is None else np.asarray(face_status, np.int32), None if q is None else np.asarray(q, F), total, status)
        return status

    def collect(self, streams, stats, ended, cap, stamp=None, with_crops=True):
        """stats [n, 4], ended [n, max_tracks] as an update left them -> (total, first [n + 1], rec: RECORD [cap], crops [cap, h, w, 3]
        or None), everything the call did not write still holding the fill"""
        n = len(streams)
        total, first, rec = filled((1,), np.int32), filled((n + 1,), np.int32), filled((cap,), SR.RECORD)
        crops = filled((cap, self.crop_h, self.crop_w, 3), np.uint8) if with_crops else None
        self._collect(np.asarray(streams, np.int32), None if stamp is None else np.asarray(stamp, np.int64),
                      np.ascontiguousarray(stats, np.int32).reshape(n, 4), np.ascontiguousarray(ended, np.int32).reshape(n, self.max_tracks),
                      cap, total, first, rec, crops)
        return int(total[0]), first, rec, crops

    def ended_arrays(self, per_frame, counts=None):
        """stats / ended arrays written by hand: per_frame[b] = the serials of ended[b]; counts[b] overrides stats[b][2]"""
        n = len(per_frame)
        stats, ended = filled((n, 4), np.int32), filled((n, self.max_tracks), np.int32)
        for b, sers in enumerate(per_frame):
            ended[b, :len(sers)] = sers
            stats[b, 2] = len(sers) if counts is None else counts[b]
        return stats, ended

    def kept(self, stream):
        """{serial: (slot, shots, kept, q, first_stamp, best_stamp)} of the stream's live tracks with a kept shot"""
        return {int(e["serial"]): (int(e["slot"]), int(e["shots"]), int(e["kept"]), float(e["q"]), int(e["first_stamp"]), int(e["best_stamp"]))
                for e in self.shots(stream)}

    def stored(self, stream, serial, tag):
        c = self.shot_crop(stream, serial)
        return c is not None and c.tobytes() == self.crop(tag).tobytes()


class RefHarness(Harness, IC.RefHarness):
    """the restatement alone"""

    def _start(self, tracker_cfg, shot_cfg, identity_cfg):
        self.tracker = TR.TrackerRef(**tracker_cfg)
        self.ident = None if identity_cfg is None else IR.IdentityRef(self.tracker, self.max_det, **identity_cfg)
        self.ref = SR.ShotsRef(self.tracker, self.max_det, ident=self.ident, **shot_cfg)

    def _keep(self, streams, stamp, first, row, serial, crops, face_status, q, total, status):
        self.ref.keep(streams, stamp, first, row, serial, crops, face_status, q, total, status)

    def _collect(self, streams, stamp, stats, ended, cap, total, first, rec, crops):
        self.ref.collect(streams, stamp, stats, ended, cap, total, first, rec, crops)

    def shots(self, stream):
        return self.ref.entries(stream)

    def shot_crop(self, stream, serial):
        return self.ref.shot_crop(stream, serial)


def rec_tuple(r):
    return (int(r["stream"]), int(r["serial"]), int(r["frame"]), int(r["shots"]), int(r["kept"]), float(r["q"]), int(r["first_stamp"]),
            int(r["best_stamp"]), int(r["end_stamp"]))


def id_tuple(r):
    return (int(r["identity"]), int(r["row"]), float(r["id_score"]), int(r["named"]), int(r["id_shots"]), float(r["id_weight"]))


def untouched(a):
    return bool((np.ascontiguousarray(a).view(np.uint8) == FILL).all())


def case_q_on_and_beside_the_stored_q(h):
    """three tracks hold a shot of q 0.5; the next shots are one f32 step below, equal and one step above: passed, passed (an equal
    q keeps the earlier shot), kept"""
    h.start()
    out = h.frames([(0, [0, 1, 2])])
    assert out.track[0, :3].tolist() == [1, 2, 3]
    obs = [(0, r, r + 1) for r in range(3)]
    assert h.keep([0], obs, [10, 11, 12], q=[0.5] * 3, stamp=[100]).tolist() == [0, 0, 0]
    assert h.keep([0], obs, [20, 21, 22], q=[down(0.5), 0.5, up(0.5)], stamp=[200]).tolist() == [3, 3, 0]
    assert h.kept(0) == {1: (0, 2, 1, 0.5, 100, 100), 2: (1, 2, 1, 0.5, 100, 100), 3: (2, 2, 2, up(0.5), 100, 200)}
    assert h.stored(0, 1, 10) and h.stored(0, 2, 11) and h.stored(0, 3, 22)


def case_q_null_keeps_every_valid_shot(h):
    """q NULL: every valid shot is kept, the stored q reads 0; a q given later is compared with that 0"""
    h.start()
    h.frames([(0, [0])])
    assert h.keep([0], [(0, 0, 1)], [10], stamp=[7]).tolist() == [0]
    assert h.keep([0], [(0, 0, 1), (0, 3, 1)], [11, 12], stamp=[8]).tolist() == [0, 0]
    assert h.kept(0) == {1: (0, 3, 3, 0.0, 7, 8)} and h.stored(0, 1, 12)
    assert h.keep([0], [(0, 0, 1), (0, 1, 1)], [13, 14], q=[0.0, up(0.0)], stamp=[9]).tolist() == [3, 0]
    assert h.kept(0) == {1: (0, 5, 4, up(0.0), 7, 9)} and h.stored(0, 1, 14)


def case_q_nan_inf_and_negative(h):
    """a negative q on the first shot is kept (kept == 0 decides, not the comparison); NaN is bad input and counts for nothing;
    +inf is kept and nothing beats it; -inf on a first shot is kept, an equal -inf passes, any finite q beats it"""
    h.start()
    h.frames([(0, [0, 1])])
    assert h.keep([0], [(0, 0, 1), (0, 1, 1), (0, 2, 1), (0, 3, 1), (0, 4, 1)], [10, 11, 12, 13, 14], q=[-1.0, NAN, INF, INF, 3e38]).tolist() == [0, 2, 0, 3, 3]
    assert h.kept(0) == {1: (0, 4, 2, INF, 0, 0)} and h.stored(0, 1, 12)
    assert h.keep([0], [(0, 0, 2), (0, 1, 2), (0, 2, 2)], [20, 21, 22], q=[-INF, -INF, -3e38]).tolist() == [0, 3, 0]
    assert h.kept(0)[2] == (1, 3, 2, float(F(-3e38)), 0, 0) and h.stored(0, 2, 22)


def case_face_status(h):
    """a negative face_status (the alignment zero-filled the crop) is bad input whatever its q; 0 and 1 are valid"""
    h.start()
    h.frames([(0, [0])])
    st = h.keep([0], [(0, r, 1) for r in range(5)], [10, 11, 12, 13, 14], q=[9.0, 1.0, 2.0, 9.0, 1.5], face_status=[-1, 0, 1, -3, 0])
    assert st.tolist() == [2, 0, 0, 2, 3]
    assert h.kept(0) == {1: (0, 3, 2, 2.0, 0, 0)} and h.stored(0, 1, 12)
    assert h.keep([0], [(0, 0, 1)], [15], face_status=[-1]).tolist() == [2]      # q NULL: still bad input
    assert h.kept(0) == {1: (0, 3, 2, 2.0, 0, 0)}


def case_no_track(h):
    """serial 0, an unknown serial and rows outside the slab are "no track": status 1 and no state"""
    h.start()
    h.frames([(0, [0])])
    st = h.keep([0], [(0, 0, 0), (0, 1, 99), (0, -1, 1), (0, h.max_det, 1)], [10, 11, 12, 13], q=[1, 1, 1, 1])
    assert st.tolist() == [1, 1, 1, 1] and h.kept(0) == {} and h.shot_crop(0, 1) is None


def case_a_crop_two_updates_late_for_an_ended_track(h):
    """tracks 1 and 2 are due in update 1; their crops arrive after update 3, in which track 2 ended: track 1 keeps its shot, the
    crop of track 2 is "no track" """
    h.start()
    h.frames([(0, [0, 1])])
    h.frames([(0, [0, 1])])
    out = h.frames([(0, [0])])
    assert out.stats[0, 2] == 1 and out.ended[0, 0] == 2
    assert h.keep([0], [(0, 0, 1), (0, 1, 2)], [10, 11], q=[0.5, 0.5], stamp=[3]).tolist() == [0, 1]
    assert h.kept(0) == {1: (0, 1, 1, 0.5, 3, 3)}
    total, first, rec, crops = h.collect([0], out.stats, out.ended, 4, stamp=[3])
    assert total == 0 and first.tolist() == [0, 0] and untouched(rec) and untouched(crops)      # track 2 never had a kept shot


def case_a_slot_reborn_under_a_new_serial(h):
    """track 1 in slot 0 keeps two shots, misses a frame and ends; track 2 is born in slot 0.  The entry is stale: not listed, no
    crop for either serial; the first keep of track 2 clears it (shots and kept restart, first_stamp is the new one, and a q
    below the old track's is kept)"""
    h.start()
    h.frames([(0, [0])])
    assert h.keep([0], [(0, 0, 1), (0, 1, 1)], [10, 11], q=[0.5, 0.75], stamp=[5]).tolist() == [0, 0]
    out = h.frames([(0, [5])])
    assert out.track[0, 0] == 2 and out.ended[0, 0] == 1
    assert h.kept(0) == {} and h.shot_crop(0, 1) is None and h.shot_crop(0, 2) is None
    assert h.keep([0], [(0, 0, 1), (0, 1, 2)], [20, 21], q=[0.9, 0.25], stamp=[6]).tolist() == [1, 0]
    assert h.kept(0) == {2: (0, 1, 1, 0.25, 6, 6)} and h.stored(0, 2, 21)


def case_several_observations_of_one_track_in_one_call(h):
    """better then worse, worse then better, equal, and three in a row: the last KEPT observation is the stored one, and a kept
    one that was superseded still has status 0"""
    h.start()
    h.frames([(0, [0, 1, 2, 3])])
    obs = [(0, 0, 1), (0, 1, 1), (0, 2, 2), (0, 3, 2), (0, 4, 3), (0, 5, 3), (0, 6, 4), (0, 7, 4), (0, 8, 4)]
    st = h.keep([0], obs, range(30, 39), q=[0.75, 0.5, 0.5, 0.75, 0.5, 0.5, 0.25, 0.75, 0.5], stamp=[1])
    assert st.tolist() == [0, 3, 0, 0, 0, 3, 0, 0, 3]
    assert h.kept(0) == {1: (0, 2, 1, 0.75, 1, 1), 2: (1, 2, 2, 0.75, 1, 1), 3: (2, 2, 1, 0.5, 1, 1), 4: (3, 3, 2, 0.75, 1, 1)}
    assert h.stored(0, 1, 30) and h.stored(0, 2, 33) and h.stored(0, 3, 34) and h.stored(0, 4, 37)


def case_totals(h):
    """total 0 and negative skip every observation, a total of 1 stops after t = 0, a total above m is clamped to m; the
    observations of two frames of two streams are owned by their frames"""
    h.start(streams=2)
    h.frames([(1, [0, 1]), (0, [3])])
    obs = [(0, 0, 1), (0, 1, 2), (1, 0, 1)]
    for total in (0, -3):
        assert h.keep([1, 0], obs, [10, 11, 12], q=[1, 1, 1], total=total).tolist() == [FILL32] * 3
    assert h.kept(0) == {} and h.kept(1) == {}
    assert h.keep([1, 0], obs, [10, 11, 12], q=[1, 1, 1], total=1, stamp=[4, 5]).tolist() == [0, FILL32, FILL32]
    assert h.keep([1, 0], obs, [20, 21, 22], q=[1, 1, 1], total=8, stamp=[6, 7]).tolist() == [3, 0, 0]
    assert h.kept(1) == {1: (0, 2, 1, 1.0, 4, 4), 2: (1, 1, 1, 1.0, 6, 6)} and h.kept(0) == {1: (0, 1, 1, 1.0, 7, 7)}
    assert h.stored(1, 1, 10) and h.stored(1, 2, 21) and h.stored(0, 1, 22)


def _three_tracks_with_shots(h, **start):
    """stream 0: tracks 1, 2, 3 in slots 0, 1, 2; tracks 1 and 3 keep a shot (tags 10, 12), track 2 never does"""
    h.start(**start)
    h.frames([(0, [0, 1, 2])])
    assert h.keep([0], [(0, 0, 1), (0, 2, 3)], [10, 12], q=[0.5, 0.25], stamp=[100]).tolist() == [0, 0]


def case_ended_tracks_with_and_without_a_kept_shot(h):
    """three frames in one call: the first ends tracks 1 and 2 (only 1 has a shot), the second ends nothing, the third ends track
    3: two records, in (frame, ended) order, and first[] shows the empty frame"""
    _three_tracks_with_shots(h)
    out = h.frames([(0, [2]), (0, [2]), (0, [])])
    assert out.stats[:, 2].tolist() == [2, 0, 1] and out.ended[0, :2].tolist() == [1, 2] and out.ended[2, 0] == 3
    total, first, rec, crops = h.collect([0, 0, 0], out.stats, out.ended, 4, stamp=[201, 202, 203])
    assert total == 2 and first.tolist() == [0, 1, 1, 2]
    assert rec_tuple(rec[0]) == (0, 1, 0, 1, 1, 0.5, 100, 100, 201) and rec_tuple(rec[1]) == (0, 3, 2, 1, 1, 0.25, 100, 100, 203)
    assert id_tuple(rec[0]) == NO_ID and id_tuple(rec[1]) == NO_ID and rec["reserved"][:2].tolist() == [[0, 0], [0, 0]]
    assert crops[0].tobytes() == h.crop(10).tobytes() and crops[1].tobytes() == h.crop(12).tobytes()
    assert untouched(rec[2:]) and untouched(crops[2:])
    total, first, rec, crops = h.collect([0, 0, 0], out.stats, out.ended, 4, with_crops=False)        # crops NULL, stamp NULL
    assert total == 2 and [rec_tuple(r)[-1] for r in rec[:2]] == [0, 0]


def case_ended_counts_outside_their_range(h):
    """stats[b][2] negative lists nothing; above max_tracks it is clamped to max_tracks (entries of serial 0 and of unknown
    serials are skipped on the way)"""
    _three_tracks_with_shots(h)
    h.frames([(0, [])])                                                  # all three end; the arrays below are written by hand
    row = [3, 0, 77, 1] + [0] * (h.max_tracks - 5) + [1]                # serial 1 twice: looked up twice, listed twice
    stats, ended = h.ended_arrays([[1, 3], row, [3]], counts=[-1, h.max_tracks + 9, 1])
    total, first, rec, crops = h.collect([0, 0, 0], stats, ended, 8)
    assert total == 4 and first.tolist() == [0, 0, 3, 4]
    assert [rec_tuple(r)[1:3] for r in rec[:4]] == [(3, 1), (1, 1), (1, 1), (3, 2)]
    assert [c.tobytes() == h.crop(t).tobytes() for c, t in zip(crops[:4], (12, 10, 10, 12))] == [True] * 4
    assert untouched(rec[4:]) and untouched(crops[4:])


def case_cap_below_at_and_above_the_total(h):
    """total and first[] are untruncated; records at or past cap are dropped and every row at or past min(total, cap) keeps the
    fill"""
    _three_tracks_with_shots(h, streams=2)
    stats, ended = h.ended_arrays([[3], [], [1, 1]])
    for cap in (1, 2, 3, 5):
        total, first, rec, crops = h.collect([0, 1, 0], stats, ended, cap)
        assert total == 3 and first.tolist() == [0, 1, 1, 3]
        have = min(cap, 3)
        assert [rec_tuple(r)[1:3] for r in rec[:have]] == [(3, 0), (1, 2), (1, 2)][:have]
        assert [c.tobytes() == h.crop(t).tobytes() for c, t in zip(crops[:have], (12, 10, 10))] == [True] * have
        assert untouched(rec[have:]) and untouched(crops[have:])
    assert h.kept(0) == {1: (0, 1, 1, 0.5, 100, 100), 3: (2, 1, 1, 0.25, 100, 100)}     # collect changed nothing


def case_a_slot_reborn_in_the_frame_that_ended_its_track(h):
    """frame [5]: track 1 (slot 0) ends and track 2 is born in slot 0 in the same update.  Collect directly behind that update
    still yields track 1's record, because the new track's first keep comes later; a collect that comes too late, after that keep,
    finds the entry taken and lists nothing"""
    h.start()
    h.frames([(0, [0])])
    assert h.keep([0], [(0, 0, 1)], [10], q=[0.5], stamp=[1]).tolist() == [0]
    out = h.frames([(0, [5])])
    assert out.track[0, 0] == 2 and out.stats[0, 2] == 1 and out.ended[0, 0] == 1
    total, first, rec, crops = h.collect([0], out.stats, out.ended, 2, stamp=[2])
    assert total == 1 and rec_tuple(rec[0]) == (0, 1, 0, 1, 1, 0.5, 1, 1, 2) and crops[0].tobytes() == h.crop(10).tobytes()
    assert h.keep([0], [(0, 0, 2)], [20], q=[0.125], stamp=[2]).tolist() == [0]
    total, first, rec, crops = h.collect([0], out.stats, out.ended, 2, stamp=[2])        # too late
    assert total == 0 and first.tolist() == [0, 0] and untouched(rec) and untouched(crops)
    out = h.frames([(0, [])])
    total, first, rec, crops = h.collect([0], out.stats, out.ended, 2, stamp=[3])
    assert total == 1 and rec_tuple(rec[0]) == (0, 2, 0, 1, 1, 0.125, 2, 2, 3) and crops[0].tobytes() == h.crop(20).tobytes()


def case_the_identity_of_a_record(h):
    """identities on: track 1 is fused and named, track 2 is fused and stays unnamed, track 3 is never fused while slot 2's
    identity entry still belongs to an older track (stale: serial 3's lookup finds nothing).  All keep a shot and end."""
    h.start(identities=dict(dim=64))
    d = h.dim
    h.frames([(0, [0, 1, 7])])                                           # serials 1, 2, 3
    _, st = h.fuse([0], [(0, 2, 3)], [IC.vec(d, {2: 1})])              # slot 2's identity entry: serial 3 ...
    h.frames([(0, [0, 1])])                                              # ... which ends here
    out = h.frames([(0, [0, 1, 2])])                                     # serial 4 is born in slot 2
    assert out.track[0, :3].tolist() == [1, 2, 4]
    obs = [(0, 0, 1), (0, 1, 2), (0, 2, 4)]
    _, st = h.fuse([0], obs[:2], [IC.vec(d, {0: 3, 1: 4}), IC.vec(d, {1: 2})], weight=[2, 3])
    h.label([0], obs[:2], [[(0.75, 3, 7)], [(0.25, 4, 8)]], st)
    assert h.keep([0], obs, [10, 11, 12], q=[0.5, 0.5, 0.5], stamp=[I64_MIN]).tolist() == [0, 0, 0]
    out = h.frames([(0, [])])
    assert out.ended[0, :3].tolist() == [1, 2, 4]
    total, first, rec, crops = h.collect([0], out.stats, out.ended, 3, stamp=[I64_MAX])
    assert total == 3 and [rec_tuple(r) for r in rec] == [(0, s, 0, 1, 1, 0.5, I64_MIN, I64_MIN, I64_MAX) for s in (1, 2, 4)]
    assert id_tuple(rec[0]) == (7, 3, 0.75, 1, 1, 2.0) and id_tuple(rec[1]) == (-1, -1, -INF, 0, 1, 3.0) and id_tuple(rec[2]) == NO_ID


def case_stamps_at_their_ends_and_null(h):
    """stamps are stored and handed back, never interpreted: INT64_MIN, INT64_MAX, -1, and NULL for 0"""
    h.start()
    h.frames([(0, [0, 1])])
    assert h.keep([0], [(0, 0, 1)], [10], q=[0.25], stamp=[I64_MAX]).tolist() == [0]
    assert h.keep([0], [(0, 0, 1), (0, 1, 2)], [11, 12], q=[0.5, 0.5], stamp=[I64_MIN]).tolist() == [0, 0]
    assert h.keep([0], [(0, 1, 2)], [13], q=[0.75]).tolist() == [0]
    assert h.kept(0) == {1: (0, 2, 2, 0.5, I64_MAX, I64_MIN), 2: (1, 2, 2, 0.75, I64_MIN, 0)}
    out = h.frames([(0, [])])
    total, first, rec, crops = h.collect([0], out.stats, out.ended, 2, stamp=[-1])
    assert [rec_tuple(r)[6:] for r in rec] == [(I64_MAX, I64_MIN, -1), (I64_MIN, 0, -1)]


CASES = {f.__name__[5:]: f for f in (
    case_q_on_and_beside_the_stored_q, case_q_null_keeps_every_valid_shot, case_q_nan_inf_and_negative, case_face_status, case_no_track,
    case_a_crop_two_updates_late_for_an_ended_track, case_a_slot_reborn_under_a_new_serial, case_several_observations_of_one_track_in_one_call,
    case_totals, case_ended_tracks_with_and_without_a_kept_shot, case_ended_counts_outside_their_range, case_cap_below_at_and_above_the_total,
    case_a_slot_reborn_in_the_frame_that_ended_its_track, case_the_identity_of_a_record, case_stamps_at_their_ends_and_null)}
