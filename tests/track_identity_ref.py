"""The track identities' three rules (include/rfd.h, "track identities") restated on the host, for the tests, on top of the state
of tests/tracker_ref.py.  Every operation is one numpy float32 operation in the order the header writes it, the wave's butterfly
written out, so the library's results are compared with these bit for bit.  Nothing here is shared with the code under test."""
import numpy as np

F = np.float32
NAMED = 8
OK, NO_TRACK, BAD_INPUT, OVERFLOW = 0, 1, 2, 3
NEG_INF = F(-np.inf)


def wave_norm(x):
    """|x| as the 64 lanes compute it: lane l sums the squares of elements l, l + 64, ... in ascending order from 0, the partial
    sums meet in the xor butterfly 32, 16, ..., 1 (every lane ends with the same bits), one square root"""
    x = np.asarray(x, F)
    part = np.zeros(64, F)
    with np.errstate(all="ignore"):
        for i0 in range(0, len(x), 64):
            chunk = x[i0:i0 + 64]
            part[:len(chunk)] = part[:len(chunk)] + chunk * chunk      # one multiplication, one addition, each rounded
        lanes = np.arange(64)
        for off in (32, 16, 8, 4, 2, 1):
            part = part + part[lanes ^ off]
        assert len(set(part.view(np.uint32).tolist())) == 1 or np.isnan(part).any()
        return np.sqrt(part[0])


def normalise(x):
    """-> (x / |x| element by element, |x|)"""
    norm = wave_norm(x)
    with np.errstate(all="ignore"):
        return np.asarray(x, F) / norm, norm


class IdentityRef:
    """the entries and templates beside a tracker_ref.TrackerRef's slots"""

    def __init__(self, tracker, max_det, dim=512, accept=0.5, release=0.4, margin=0.05):
        self.t, self.max_det, self.dim = tracker, int(max_det), int(dim)
        self.accept, self.release, self.margin = F(accept), F(release), F(margin)
        s, m = tracker.streams, tracker.max_tracks
        self.serial = np.zeros((s, m), np.int64)
        self.identity, self.row = np.zeros((s, m), np.int64), np.zeros((s, m), np.int64)
        self.score, self.weight = np.zeros((s, m), F), np.zeros((s, m), F)
        self.named, self.shots = np.zeros((s, m), np.int64), np.zeros((s, m), np.int64)
        self.S = np.zeros((s, m, self.dim), F)

    # ---- reading the state ----
    def entries(self, stream):
        """[(slot, serial, identity, row, score bits, named, shots, weight bits)] of the live slots whose entry is not stale"""
        out = []
        for j in range(self.t.max_tracks):
            live = int(self.t.serial[stream, j])
            if live != 0 and int(self.serial[stream, j]) == live:
                out.append((j, live, int(self.identity[stream, j]), int(self.row[stream, j]), int(self.score[stream, j].view(np.uint32)),
                            int(self.named[stream, j]), int(self.shots[stream, j]), int(self.weight[stream, j].view(np.uint32))))
        return out

    def template(self, stream, serial):
        j = self._find(stream, serial)
        return None if j < 0 or int(self.serial[stream, j]) != int(serial) else self.S[stream, j].copy()

    # ---- the observations of a call ----
    def _find(self, s, serial):
        """the lowest slot of stream s that holds the serial now, or -1; 0 names no track"""
        if int(serial) == 0:
            return -1
        hit = np.flatnonzero(self.t.serial[s] == int(serial))
        return int(hit[0]) if len(hit) else -1

    def _observations(self, streams, first, row, serial, total, m):
        """(t, stream, serial) in the order of the rule: the frames in call order (streams are independent, so walking them
        stream by stream gives the same), each frame's t ascending within [max(first[b], 0), min(first[b + 1], count))"""
        count = m if total is None else min(max(int(total), 0), m)
        for b, s in enumerate(streams):
            for t in range(max(int(first[b]), 0), min(int(first[b + 1]), count)):
                r = int(row[t])
                yield t, int(s), (int(serial[b, r]) if 0 <= r < self.max_det else 0)

    # ---- 1 fuse ----
    def fuse(self, streams, first, row, serial, emb, weight, total, query, status):
        """writes query [m, dim] and status [m] where the library writes them and nowhere else"""
        m = len(row)
        serial = np.asarray(serial).reshape(len(streams), self.max_det)
        emb = np.asarray(emb, F).reshape(m, self.dim)
        for t, s, ser in self._observations(streams, first, row, serial, total, m):
            w = F(1.0) if weight is None else F(weight[t])
            e, norm = normalise(emb[t])                                             # a
            if not (norm > 0 and np.isfinite(norm)) or not (np.isfinite(w) and w > 0):  # b
                query[t], status[t] = e, BAD_INPUT
                continue
            j = self._find(s, ser)
            if j < 0:                                                               # c
                query[t], status[t] = e, NO_TRACK
                continue
            if int(self.serial[s, j]) != ser:                                       # d: a stale entry is cleared first
                self.serial[s, j], self.identity[s, j], self.row[s, j], self.score[s, j] = ser, -1, -1, NEG_INF
                self.named[s, j], self.shots[s, j], self.weight[s, j] = 0, 0, F(0)
                self.S[s, j] = 0
            with np.errstate(all="ignore"):
                self.S[s, j] = self.S[s, j] + w * e                                 # one multiplication, one addition
                self.shots[s, j] += 1
                self.weight[s, j] = self.weight[s, j] + w
            q, n2 = normalise(self.S[s, j])
            query[t], status[t] = q, (OK if np.isfinite(n2) else OVERFLOW)

    # ---- 2 label ----
    def label(self, streams, first, row, serial, scores, rows, ids, status_in, total):
        m = len(row)
        serial = np.asarray(serial).reshape(len(streams), self.max_det)
        scores = np.asarray(scores, F).reshape(m, -1)
        k = scores.shape[1]
        rows = np.asarray(rows).reshape(m, k)
        ids = np.full((m, k), -1) if ids is None else np.asarray(ids).reshape(m, k)
        for t, s, ser in self._observations(streams, first, row, serial, total, m):
            if int(status_in[t]) != 0:
                continue
            j = self._find(s, ser)
            if j < 0 or int(self.serial[s, j]) != ser:
                continue
            top, top_row, top_id = scores[t, 0], int(rows[t, 0]), int(ids[t, 0])
            top_ok = not (top_row == -1 or np.isnan(top))
            run_ok = k >= 2 and not (int(rows[t, 1]) == -1 or np.isnan(scores[t, 1]))
            keep = False
            if self.named[s, j]:
                x = int(self.identity[s, j])
                same = (top_id == x) if x >= 0 else (top_row == int(self.row[s, j]))
                keep = bool(top_ok and same and top >= self.release)
            with np.errstate(all="ignore"):
                take = keep or bool(top_ok and top >= self.accept and (not run_ok or top - scores[t, 1] >= self.margin))
            if take:
                if not keep:
                    self.identity[s, j] = top_id
                self.named[s, j], self.row[s, j], self.score[s, j] = 1, top_row, top
            else:
                self.named[s, j], self.identity[s, j], self.row[s, j], self.score[s, j] = 0, -1, -1, NEG_INF

    # ---- 3 who ----
    def who(self, streams, track, count, flags_in, who, identity, id_score):
        """writes rows below each frame's clamped count of who / identity / id_score (the last two may be None)"""
        for b, s in enumerate(streams):
            s = int(s)
            for i in range(min(max(int(count[b]), 0), self.max_det)):
                j = self._find(s, int(track[b, i]))
                named = j >= 0 and int(self.serial[s, j]) == int(track[b, i]) and bool(self.named[s, j])
                f = 0 if flags_in is None else int(flags_in[b, i])
                who[b, i] = f | (NAMED if named else 0)
                if identity is not None:
                    identity[b, i] = int(self.identity[s, j]) if named else -1
                if id_score is not None:
                    id_score[b, i] = self.score[s, j] if named else NEG_INF
