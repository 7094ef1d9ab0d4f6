"""The track shots' two rules and two readers (include/rfd.h, "track shots") restated on the host, for the tests, on top of the
state of tests/tracker_ref.py and, for the identity fields of a record, of tests/track_identity_ref.py.  There is one f32
comparison in it and nothing else that rounds, so the library's results are compared with these byte for byte.  Nothing here is
shared with the code under test."""
import numpy as np

F = np.float32
KEPT, NO_TRACK, BAD_INPUT, PASSED = 0, 1, 2, 3
NEG_INF = F(-np.inf)

# rfd_track_shot (40 bytes) and rfd_track_record (80 bytes), field by field
SHOT = np.dtype([("slot", "<i4"), ("serial", "<i4"), ("shots", "<i4"), ("kept", "<i4"), ("q", "<f4"), ("reserved", "<i4"),
                 ("first_stamp", "<i8"), ("best_stamp", "<i8")])
RECORD = np.dtype([("stream", "<i4"), ("serial", "<i4"), ("frame", "<i4"), ("shots", "<i4"), ("kept", "<i4"), ("q", "<f4"),
                   ("first_stamp", "<i8"), ("best_stamp", "<i8"), ("end_stamp", "<i8"), ("identity", "<i4"), ("row", "<i4"),
                   ("id_score", "<f4"), ("named", "<i4"), ("id_shots", "<i4"), ("id_weight", "<f4"), ("reserved", "<i4", (2,))])
assert SHOT.itemsize == 40 and RECORD.itemsize == 80


class ShotsRef:
    """the heads and crops beside a tracker_ref.TrackerRef's slots; ident: a track_identity_ref.IdentityRef over the same tracker,
    or None when identities are not enabled"""

    def __init__(self, tracker, max_det, crop_w=112, crop_h=112, ident=None):
        self.t, self.max_det, self.ident = tracker, int(max_det), ident
        self.crop_w, self.crop_h = int(crop_w), int(crop_h)
        s, m = tracker.streams, tracker.max_tracks
        self.serial, self.shots, self.kept = np.zeros((s, m), np.int64), np.zeros((s, m), np.int64), np.zeros((s, m), np.int64)
        self.q = np.zeros((s, m), F)
        self.first_stamp, self.best_stamp = np.zeros((s, m), np.int64), np.zeros((s, m), np.int64)
        self.crop = np.zeros((s, m, self.crop_h, self.crop_w, 3), np.uint8)

    # ---- the readers ----
    def entries(self, stream):
        """rfd_tracker_get_shots as a SHOT array: the live slots whose entry is not stale, in ascending slot order"""
        out = []
        for j in range(self.t.max_tracks):
            live = int(self.t.serial[stream, j])
            if live != 0 and int(self.serial[stream, j]) == live:
                out.append((j, live, int(self.shots[stream, j]), int(self.kept[stream, j]), self.q[stream, j], 0,
                            int(self.first_stamp[stream, j]), int(self.best_stamp[stream, j])))
        return np.array(out, SHOT)

    def shot_crop(self, stream, serial):
        """rfd_tracker_get_shot_crop, None for "no such track" """
        j = self._find(stream, serial)
        return None if j < 0 or int(self.serial[stream, j]) != int(serial) else self.crop[stream, j].copy()

    def _find(self, s, serial):
        """the lowest slot of stream s that holds the serial now, or -1; 0 names no track"""
        if int(serial) == 0:
            return -1
        hit = np.flatnonzero(self.t.serial[s] == int(serial))
        return int(hit[0]) if len(hit) else -1

    # ---- 1 keep ----
    def keep(self, streams, stamp, first, row, serial, crops, face_status, q, total, status):
        """writes status [m] where the library writes it and nowhere else"""
        m = len(row)
        serial = np.asarray(serial).reshape(len(streams), self.max_det)
        crops = np.asarray(crops, np.uint8).reshape(m, self.crop_h, self.crop_w, 3)
        count = m if total is None else min(max(int(total), 0), m)
        for b, s in enumerate(streams):                 # the frames in call order: streams are independent
            s, at = int(s), (0 if stamp is None else int(stamp[b]))
            for t in range(max(int(first[b]), 0), min(int(first[b + 1]), count)):
                r = int(row[t])
                ser = int(serial[b, r]) if 0 <= r < self.max_det else 0
                if (face_status is not None and int(face_status[t]) < 0) or (q is not None and np.isnan(q[t])):
                    status[t] = BAD_INPUT
                    continue
                j = self._find(s, ser)
                if j < 0:
                    status[t] = NO_TRACK
                    continue
                if int(self.serial[s, j]) != ser:       # a stale entry is cleared first
                    self.serial[s, j], self.shots[s, j], self.kept[s, j], self.q[s, j] = ser, 0, 0, NEG_INF
                    self.first_stamp[s, j], self.best_stamp[s, j] = at, 0
                self.shots[s, j] += 1
                if self.kept[s, j] == 0 or q is None or F(q[t]) > self.q[s, j]:     # one f32 comparison
                    self.crop[s, j] = crops[t]
                    self.q[s, j] = F(0) if q is None else F(q[t])
                    self.best_stamp[s, j] = at
                    self.kept[s, j] += 1
                    status[t] = KEPT
                else:
                    status[t] = PASSED

    # ---- 2 collect ----
    def collect(self, streams, stamp, stats, ended, cap, total, first, rec, crops):
        """writes total [1], first [n + 1], rec (a RECORD array [cap]) and crops ([cap, h, w, 3] or None) where the library does"""
        n, mt = len(streams), self.t.max_tracks
        stats, ended = np.asarray(stats).reshape(n, 4), np.asarray(ended).reshape(n, mt)
        r = 0
        for b, s in enumerate(streams):
            s = int(s)
            first[b] = r
            for e in range(min(max(int(stats[b, 2]), 0), mt)):
                ser = int(ended[b, e])
                hit = np.flatnonzero(self.serial[s] == ser) if ser != 0 else []
                if len(hit) == 0:
                    continue
                j = int(hit[0])
                if r < cap:
                    o = rec[r]
                    o["stream"], o["serial"], o["frame"] = s, ser, b
                    o["shots"], o["kept"], o["q"] = self.shots[s, j], self.kept[s, j], self.q[s, j]
                    o["first_stamp"], o["best_stamp"] = self.first_stamp[s, j], self.best_stamp[s, j]
                    o["end_stamp"] = 0 if stamp is None else int(stamp[b])
                    o["identity"], o["row"], o["id_score"], o["named"], o["id_shots"], o["id_weight"] = -1, -1, NEG_INF, 0, 0, F(0)
                    o["reserved"] = 0
                    ihit = np.flatnonzero(self.ident.serial[s] == ser) if self.ident is not None else []
                    if len(ihit):
                        i, d = int(ihit[0]), self.ident
                        o["identity"], o["row"], o["id_score"] = d.identity[s, i], d.row[s, i], d.score[s, i]
                        o["named"], o["id_shots"], o["id_weight"] = d.named[s, i], d.shots[s, i], d.weight[s, i]
                    if crops is not None:
                        crops[r] = self.crop[s, j]
                r += 1
        first[n] = r
        total[0] = r
