"""The tracker's rule (include/rfd.h, "tracker") restated on the host, for the tests: an IoU tracker with two score
thresholds.  Every operation is one numpy float32 operation in the order the header writes it, so the library's results are
compared with these bit for bit.  Nothing here is shared with the code under test."""
import numpy as np

NEW, CONFIRMED, DUE = 1, 2, 4
F = np.float32
INT32_MAX = 2 ** 31 - 1


def iou(rb, sb):
    """IoU of box rb [4] with every box of sb [m, 4]: nms.rs:39-54 (the +1 convention, one IEEE division), f32 throughout.
    fmax / fmin return the other operand for a NaN, as C's fmaxf / fminf do."""
    one, zero = F(1), F(0)
    with np.errstate(all="ignore"):
        area_i = (rb[2] - rb[0] + one) * (rb[3] - rb[1] + one)
        area_j = (sb[:, 2] - sb[:, 0] + one) * (sb[:, 3] - sb[:, 1] + one)
        xx1, yy1 = np.fmax(rb[0], sb[:, 0]), np.fmax(rb[1], sb[:, 1])
        xx2, yy2 = np.fmin(rb[2], sb[:, 2]), np.fmin(rb[3], sb[:, 3])
        w = np.fmax(zero, xx2 - xx1 + one)
        h = np.fmax(zero, yy2 - yy1 + one)
        inter = w * h
        return inter / (area_i + area_j - inter)


class Out:
    """host arrays with the names of rfd_hip.TrackOut, every byte `fill`"""

    def __init__(self, n, max_det, max_tracks, fill=0):
        new = lambda shape, dt: np.frombuffer(bytes([fill]) * (int(np.prod(shape)) * np.dtype(dt).itemsize), dt).reshape(shape).copy()
        self.track, self.flags = new((n, max_det), np.int32), new((n, max_det), np.uint32)
        self.stats, self.ended = new((n, 4), np.int32), new((n, max_tracks), np.int32)
        self.due_boxes, self.due_landmarks = new((n, max_det, 5), np.float32), new((n, max_det, 5, 2), np.float32)
        self.due_count, self.due_total = new((n,), np.int32), new((n,), np.int32)
        self.due_track = new((n, max_det), np.int32)


class TrackerRef:
    def __init__(self, streams=1, max_tracks=64, iou_min=0.3, max_missed=5, min_score=0.7, new_score=0.7, min_hits=2, improve=1.1):
        self.streams, self.max_tracks = int(streams), int(max_tracks)
        self.iou_min, self.min_score, self.new_score, self.improve = F(iou_min), F(min_score), F(new_score), F(improve)
        self.max_missed, self.min_hits = int(max_missed), int(min_hits)
        s, m = self.streams, self.max_tracks
        self.serial = np.zeros((s, m), np.int64)
        self.box = np.zeros((s, m, 4), F)
        self.missed, self.hits = np.zeros((s, m), np.int64), np.zeros((s, m), np.int64)
        self.shot = np.zeros((s, m), F)
        self.next = np.ones(s, np.int64)

    def reset(self, stream=-1):
        sel = slice(None) if stream < 0 else stream
        self.serial[sel] = 0

    def tracks(self, stream):
        """[(slot, serial, box bytes, missed, hits, shot_q bits)] of the live slots, ascending"""
        return [(int(k), int(self.serial[stream, k]), self.box[stream, k].tobytes(), int(self.missed[stream, k]), int(self.hits[stream, k]),
                 int(self.shot[stream, k].view(np.uint32))) for k in range(self.max_tracks) if self.serial[stream, k] != 0]

    def _shot(self, s, k, q, flags):
        """steps 6 and 7 for the row that has just taken slot k"""
        if self.hits[s, k] >= self.min_hits:
            flags |= CONFIRMED
            with np.errstate(all="ignore"):
                if q > self.shot[s, k] * self.improve:   # one multiplication, one comparison; false for a NaN
                    flags |= DUE
                    self.shot[s, k] = q
        return flags

    def frame(self, s, boxes, quality=None):
        """one frame of stream s: boxes [K, 5] f32 (x1, y1, x2, y2, score), quality [K] or None
        -> (track [K], flags [K], (matched, born, ended, dropped), ended serials)"""
        boxes = np.asarray(boxes, F).reshape(-1, 5)
        K = len(boxes)
        q = boxes[:, 4] if quality is None else np.asarray(quality, F).reshape(-1)[:K]
        track, flags = np.zeros(K, np.int64), np.zeros(K, np.int64)
        with np.errstate(all="ignore"):
            eligible = boxes[:, 4] >= self.min_score          # 1: false for a NaN
            fresh = boxes[:, 4] >= self.new_score
        matched = np.zeros(self.max_tracks, bool)
        unmatched_rows = []
        n_matched = n_born = n_dropped = 0
        for i in range(K):                                    # 2
            if not eligible[i]:
                continue
            open_ = (self.serial[s] != 0) & ~matched
            got = False
            if open_.any():
                v = iou(boxes[i, :4], self.box[s])
                with np.errstate(all="ignore"):
                    cand = open_ & (v >= self.iou_min)        # a NaN is no candidate
                if cand.any():
                    best = v[cand].max()
                    k = int(np.flatnonzero(cand & (v == best))[0])   # equal IoUs: the lowest slot
                    self.box[s, k] = boxes[i, :4]
                    self.missed[s, k] = 0
                    self.hits[s, k] += 1
                    matched[k] = True
                    track[i] = self.serial[s, k]
                    flags[i] = self._shot(s, k, q[i], 0)
                    n_matched += 1
                    got = True
            if not got:
                unmatched_rows.append(i)
        live = self.serial[s] != 0
        self.missed[s][live & ~matched] += 1                  # 3
        ending = live & (self.missed[s] > self.max_missed)    # 4
        ended = [int(x) for x in self.serial[s][ending]]
        for a in (self.serial, self.missed, self.hits):
            a[s][ending] = 0
        self.box[s][ending] = 0
        self.shot[s][ending] = 0
        for i in unmatched_rows:                              # 5
            if not fresh[i]:
                continue
            free = np.flatnonzero(self.serial[s] == 0)
            if len(free) == 0:
                n_dropped += 1
                continue
            k = int(free[0])
            self.serial[s, k] = self.next[s]
            self.next[s] = 1 if self.next[s] == INT32_MAX else self.next[s] + 1
            self.box[s, k] = boxes[i, :4]
            self.missed[s, k], self.hits[s, k] = 0, 1
            self.shot[s, k] = F(-np.inf)
            track[i] = self.serial[s, k]
            flags[i] = self._shot(s, k, q[i], NEW)
            n_born += 1
        return track, flags, (n_matched, n_born, len(ended), n_dropped), ended

    def update(self, streams, boxes, landmarks, count, quality, out):
        """a call: streams [n], boxes [n, max_det, 5], landmarks [n, max_det, 5, 2], count [n], quality [n, max_det] or None;
        writes into `out` (the arrays of an Out / rfd_hip.TrackOut) what the library writes and nothing else"""
        n, md = len(streams), boxes.shape[1]
        for b in range(n):
            c = min(max(int(count[b]), 0), md)
            t, f, stats, ended = self.frame(int(streams[b]), boxes[b, :c], None if quality is None else quality[b, :c])
            out.track[b, :c], out.flags[b, :c] = t, f
            if out.stats is not None:
                out.stats[b] = stats
            if out.ended is not None:
                out.ended[b, :len(ended)] = ended
            due = np.flatnonzero(f & DUE)
            if getattr(out, "due_boxes", None) is not None:
                out.due_boxes[b, :len(due)] = boxes[b, due]
                out.due_landmarks[b, :len(due)] = np.asarray(landmarks[b]).reshape(md, 5, 2)[due]
                out.due_count[b] = len(due)
                if out.due_total is not None:
                    out.due_total[b] = len(due)
            if out.due_track is not None:
                out.due_track[b, :len(due)] = t[due]
        return out
