"""Constructed cases of the track identities (include/rfd.h, "track identities"), each with its answer written down from the
construction: embeddings whose norms are exact ((3, 4), (0, 5, 12), multiples of axis vectors), thresholds that are exact in f32
and one f32 step either side of them.  A case is a function of a harness: the harness runs the calls (on the restatement alone
in tests/test_track_identity_cpu.py, on the library AND the restatement, compared bit for bit, in tests/test_track_identity_gpu.py)
and the case asserts the written answers on what comes back.

The tracker under every case: iou_min 0.5, max_missed 0 (a track that misses one frame ends in it), both scores 0.5, min_hits 1.
Its frames hold boxes of a grid that never overlap, named by their grid index, so frame [0, 1, 2] of a fresh stream gives serials
1, 2, 3 in slots 0, 1, 2, and a track lives exactly as long as its grid index keeps appearing."""
import numpy as np

import track_identity_ref as IR
import tracker_ref as TR

F = np.float32
FILL = 0xA5
FILL32 = int(np.frombuffer(bytes([FILL]) * 4, np.int32)[0])
FILLU = int(np.frombuffer(bytes([FILL]) * 4, np.uint32)[0])
INF = float("inf")
NAN = float("nan")
TRACKER = dict(iou_min=0.5, max_missed=0, min_score=0.5, new_score=0.5, min_hits=1, improve=1.1)


def filled(shape, dt):
    return np.frombuffer(bytes([FILL]) * (int(np.prod(shape)) * np.dtype(dt).itemsize), dt).reshape(shape).copy()


def grid_box(k, score=0.9):
    """box k of a 16-wide grid of 10 x 10 boxes, 20 apart: no two overlap"""
    x, y = 20 * (k % 16), 20 * (k // 16)
    return [x, y, x + 9, y + 9, score]


def vec(dim, at):
    """a [dim] f32 vector that is zero but for {index: value}"""
    v = np.zeros(dim, F)
    for i, x in at.items():
        v[i] = x
    return v


def up(x):
    return float(np.nextafter(F(x), F(np.inf)))


def down(x):
    return float(np.nextafter(F(x), F(-np.inf)))


class Harness:
    """builds the arrays of the calls; a subclass runs them (_update, _fuse, _label, _who, entries, template)"""
    max_det = 16

    def start(self, streams=1, max_tracks=64, dim=64, accept=0.5, release=0.25, margin=0.125):
        self.n_streams, self.max_tracks, self.dim = streams, max_tracks, dim
        self._start(dict(TRACKER, streams=streams, max_tracks=max_tracks), dict(dim=dim, accept=accept, release=release, margin=margin))

    def frames(self, items):
        """items: [(stream, [grid index of every row])] -> (track [n, max_det], flags [n, max_det], count [n]) of one update"""
        n, md = len(items), self.max_det
        boxes, lmk, count = np.zeros((n, md, 5), F), np.zeros((n, md, 5, 2), F), np.zeros(n, np.int32)
        for b, (_, ks) in enumerate(items):
            count[b] = len(ks)
            boxes[b, :len(ks)] = [grid_box(k) for k in ks]
        out = self._update(np.asarray([s for s, _ in items], np.int32), boxes, lmk, count)
        return out.track, out.flags, count

    def obs(self, streams, obs):
        """obs: [(frame, row, serial)] in (frame, t) order -> first [n + 1], row [m], serial [n, max_det]"""
        n = len(streams)
        first = np.zeros(n + 1, np.int32)
        row = np.asarray([r for _, r, _ in obs], np.int32).reshape(-1)
        serial = np.zeros((n, self.max_det), np.int32)
        for b, r, ser in obs:
            first[b + 1:] += 1
            if 0 <= r < self.max_det:
                serial[b, r] = ser
        assert [b for b, _, _ in obs] == sorted(b for b, _, _ in obs)
        return first, row, serial

    def fuse(self, streams, obs, emb, weight=None, total=None):
        first, row, serial = self.obs(streams, obs)
        m = len(row)
        query, status = filled((m, self.dim), F), filled((m,), np.int32)
        self._fuse(np.asarray(streams, np.int32), first, row, serial, np.asarray(emb, F).reshape(m, self.dim),
                   None if weight is None else np.asarray(weight, F), total, query, status)
        return query, status

    def label(self, streams, obs, results, status=None, total=None, with_ids=True):
        """results: per observation a list of k (score, row, identity)"""
        first, row, serial = self.obs(streams, obs)
        m = len(row)
        r = np.asarray(results, np.float64).reshape(m, -1, 3)
        scores, rows, ids = r[:, :, 0].astype(F), r[:, :, 1].astype(np.int32), r[:, :, 2].astype(np.int32)
        status = np.zeros(m, np.int32) if status is None else np.asarray(status, np.int32)
        self._label(np.asarray(streams, np.int32), first, row, serial, scores, rows, ids if with_ids else None, status, total)

    def who(self, streams, track, count, flags=None, in_place=False):
        """track: per frame the serial of every row (padded with the fill), count [n] -> (who, identity, id_score), [n, max_det]"""
        n, md = len(streams), self.max_det
        tr = filled((n, md), np.int32)
        for b, t in enumerate(track):
            tr[b, :len(t)] = t
        fl = None
        if flags is not None:
            fl = filled((n, md), np.uint32)
            for b, f in enumerate(flags):
                fl[b, :len(f)] = f
        who = fl if in_place else filled((n, md), np.uint32)
        identity, id_score = filled((n, md), np.int32), filled((n, md), F)
        self._who(np.asarray(streams, np.int32), tr, np.asarray(count, np.int32), fl, who, identity, id_score)
        return who, identity, id_score

    def named(self, stream):
        """{serial: (identity, row, score, named, shots, weight)} of the stream's fused live tracks"""
        u = lambda bits: float(np.asarray([bits], np.uint32).view(F)[0])
        return {e[1]: (e[2], e[3], u(e[4]), e[5], e[6], u(e[7])) for e in self.entries(stream)}


class RefHarness(Harness):
    """the restatement alone"""

    def _start(self, tracker_cfg, identity_cfg):
        self.tracker = TR.TrackerRef(**tracker_cfg)
        self.ident = IR.IdentityRef(self.tracker, self.max_det, **identity_cfg)

    def _update(self, streams, boxes, lmk, count):
        return self.tracker.update(streams, boxes, lmk, count, None, TR.Out(len(streams), self.max_det, self.max_tracks, fill=FILL))

    def _fuse(self, streams, first, row, serial, emb, weight, total, query, status):
        self.ident.fuse(streams, first, row, serial, emb, weight, total, query, status)

    def _label(self, streams, first, row, serial, scores, rows, ids, status, total):
        self.ident.label(streams, first, row, serial, scores, rows, ids, status, total)

    def _who(self, streams, track, count, flags, who, identity, id_score):
        self.ident.who(streams, track, count, flags, who, identity, id_score)

    def entries(self, stream):
        return self.ident.entries(stream)

    def template(self, stream, serial):
        return self.ident.template(stream, serial)


UNNAMED = (-1, -1, -INF, 0)


def bits(a):
    return np.asarray(a, F).view(np.uint32).tolist()


def case_exact_norms_and_no_track(h):
    """(3, 4) / 5, (0, 5, 12) / 13 and 2 e7 / 2 are exact divisions; serial 0, an unknown serial and rows outside the slab are
    "no track": status 1, the query is the shot alone, and nothing is fused"""
    h.start(dim=64)
    track, _, _ = h.frames([(0, [0])])
    assert track[0, 0] == 1
    d = h.dim
    emb = [vec(d, {0: 3, 1: 4}), vec(d, {1: 5, 2: 12}), vec(d, {7: 2}), vec(d, {0: 3, 1: 4})]
    q, st = h.fuse([0], [(0, 0, 0), (0, 1, 99), (0, -1, 1), (0, h.max_det, 1)], emb)
    assert st.tolist() == [1, 1, 1, 1]
    assert bits(q[0]) == bits(vec(d, {0: F(3) / F(5), 1: F(4) / F(5)}))
    assert bits(q[1]) == bits(vec(d, {1: F(5) / F(13), 2: F(12) / F(13)}))
    assert bits(q[2]) == bits(vec(d, {7: 1})) and bits(q[3]) == bits(q[0])
    assert h.entries(0) == [] and h.template(0, 1) is None


def case_two_shots_of_weight_1_and_3(h):
    """track 1: (3, 4) with weight 1, then (0, 5, 12) with weight 3 in a second call; track 2: 2 e0 with weight 3 and 7 e1 with
    weight 4 as two observations of ONE call: S = (3, 4), whose norm 5 is exact"""
    h.start(dim=96)
    track, _, _ = h.frames([(0, [0, 1])])
    assert track[0, :2].tolist() == [1, 2]
    d = h.dim
    q, st = h.fuse([0], [(0, 0, 1)], [vec(d, {0: 3, 1: 4})], weight=[1])
    assert st.tolist() == [0] and h.named(0) == {1: UNNAMED + (1, 1.0)}
    assert bits(h.template(0, 1)) == bits(vec(d, {0: F(3) / F(5), 1: F(4) / F(5)}))
    q, st = h.fuse([0], [(0, 0, 1)], [vec(d, {1: 5, 2: 12})], weight=[3])
    assert st.tolist() == [0] and h.named(0) == {1: UNNAMED + (2, 4.0)}
    want = vec(d, {0: F(3) / F(5), 1: F(4) / F(5) + F(3) * (F(5) / F(13)), 2: F(3) * (F(12) / F(13))})
    assert bits(h.template(0, 1)) == bits(want)
    q, st = h.fuse([0], [(0, 4, 2), (0, 9, 2)], [vec(d, {0: 2}), vec(d, {1: 7})], weight=[3, 4])
    assert st.tolist() == [0, 0]
    assert bits(q[0]) == bits(vec(d, {0: 1})) and bits(q[1]) == bits(vec(d, {0: F(3) / F(5), 1: F(4) / F(5)}))
    assert bits(h.template(0, 2)) == bits(vec(d, {0: 3, 1: 4}))
    assert h.named(0) == {1: UNNAMED + (2, 4.0), 2: UNNAMED + (2, 7.0)}


def case_bad_weights_and_embeddings(h):
    """weights 0, negative, inf and NaN, a zero and a NaN embedding: status 2, the query is the shot as computed, no state"""
    h.start(dim=64)
    h.frames([(0, [0])])
    d = h.dim
    emb = [vec(d, {3: 2})] * 4 + [np.zeros(d, F), vec(d, {5: NAN, 6: 1}), vec(d, {3: 2})]
    q, st = h.fuse([0], [(0, t, 1) for t in range(7)], emb, weight=[0, -1, INF, NAN, 1, 1, 2])
    assert st.tolist() == [2, 2, 2, 2, 2, 2, 0]
    for t in range(4):
        assert bits(q[t]) == bits(vec(d, {3: 1}))
    assert np.isnan(q[4]).all() and np.isnan(q[5]).all()              # 0 / 0, and x / NaN
    assert bits(q[6]) == bits(vec(d, {3: 1})) and bits(h.template(0, 1)) == bits(vec(d, {3: 2}))
    assert h.named(0) == {1: UNNAMED + (1, 2.0)}                       # the one good shot alone


def case_thresholds_on_and_beside_their_boundaries(h):
    """accept 0.5, release 0.25, margin 0.125, all exact in f32; nine tracks, one per probe"""
    h.start(dim=32, accept=0.5, release=0.25, margin=0.125)
    h.frames([(0, list(range(9)))])
    d = h.dim
    obs = [(0, r, r + 1) for r in range(9)]
    _, st = h.fuse([0], obs, [vec(d, {r: 1}) for r in range(9)])
    assert st.tolist() == [0] * 9
    # accept, k = 1: tracks 1..3 below, on, above
    h.label([0], obs[:3], [[(down(0.5), 3, 7)], [(0.5, 3, 7)], [(up(0.5), 3, 7)]], st[:3])
    n = h.named(0)
    assert n[1][:4] == UNNAMED and n[2][:4] == (7, 3, 0.5, 1) and n[3][:4] == (7, 3, up(0.5), 1)
    # release: tracks 4..6 are named at 0.75, then score below, on, above release with the same identity
    h.label([0], obs[3:6], [[(0.75, 3, 7)]] * 3, st[3:6])
    h.label([0], obs[3:6], [[(down(0.25), 3, 7)], [(0.25, 3, 7)], [(up(0.25), 3, 7)]], st[3:6])
    n = h.named(0)
    assert n[4][:4] == UNNAMED and n[5][:4] == (7, 3, 0.25, 1) and n[6][:4] == (7, 3, up(0.25), 1)
    # margin, k = 2: top 0.75, runner-up at 0.625 (difference exactly the margin) and one step either side
    h.label([0], obs[6:9], [[(0.75, 3, 7), (up(0.625), 4, 8)], [(0.75, 3, 7), (0.625, 4, 8)], [(0.75, 3, 7), (down(0.625), 4, 8)]], st[6:9])
    n = h.named(0)
    assert n[7][:4] == UNNAMED and n[8][:4] == (7, 3, 0.75, 1) and n[9][:4] == (7, 3, 0.75, 1)


def case_empty_entries_and_k_1(h):
    """top empty by its row and by a NaN score; an empty runner-up does not count against the margin; k = 1 has no runner-up;
    observations with a non-zero status are skipped"""
    h.start(dim=32)
    h.frames([(0, list(range(6)))])
    d = h.dim
    obs = [(0, r, r + 1) for r in range(6)]
    _, st = h.fuse([0], obs, [vec(d, {r: 1}) for r in range(6)])
    res = [[(-INF, -1, -1), (-INF, -1, -1)],          # 1: top empty by its row
           [(NAN, 2, 5), (0.1, 3, 6)],                # 2: top empty by its score
           [(0.75, 2, 5), (-INF, -1, -1)],            # 3: runner-up empty by its row
           [(0.75, 2, 5), (NAN, 3, 6)],               # 4: runner-up empty by its score
           [(0.75, 2, 5), (0.7, 3, 6)],               # 5: the margin fails
           [(0.75, 2, 5), (0.7, 3, 6)]]               # 6: skipped by its status
    status = st.copy()
    status[5] = 1
    h.label([0], obs, res, status)
    n = h.named(0)
    assert [n[s][:4] for s in range(1, 7)] == [UNNAMED, UNNAMED, (5, 2, 0.75, 1), (5, 2, 0.75, 1), UNNAMED, UNNAMED]
    h.label([0], obs[4:5], [[(0.75, 2, 5)]], st[4:5])                  # k = 1: the same top now names track 5
    assert h.named(0)[5][:4] == (5, 2, 0.75, 1)
    # a named track loses its name to an empty top
    h.label([0], obs[2:3], [[(-INF, -1, -1)]], st[2:3])
    assert h.named(0)[3][:4] == UNNAMED


def case_names_taken_over_kept_and_unlabelled(h):
    """a name taken over by another identity; a name kept on a refreshed score and row below accept; an unlabelled gallery row
    (identity -1) as the name, held by its row; two observations of one track in one call: the later one decides"""
    h.start(dim=32)
    h.frames([(0, [0, 1, 2, 3])])
    d = h.dim
    obs = [(0, r, r + 1) for r in range(4)]
    _, st = h.fuse([0], obs, [vec(d, {r: 1}) for r in range(4)])
    h.label([0], obs, [[(0.75, 3, 7), (0.2, 8, 9)]] * 3 + [[(0.75, 4, -1), (0.2, 8, 9)]], st)
    n = h.named(0)
    assert [n[s][:4] for s in (1, 2, 3, 4)] == [(7, 3, 0.75, 1)] * 3 + [(-1, 4, 0.75, 1)]
    h.label([0], obs, [[(0.875, 8, 9), (0.3, 3, 7)],       # 1: taken over by identity 9
                       [(0.3125, 5, 7), (0.3, 8, 9)],      # 2: kept (>= release), score and row refreshed, no margin asked
                       [(0.3125, 8, 9), (0.3, 3, 7)],      # 3: another identity below accept: the name is lost
                       [(0.3125, 4, -1), (0.3, 8, 9)]], st)  # 4: the same unlabelled row: kept
    n = h.named(0)
    assert [n[s][:4] for s in (1, 2, 3, 4)] == [(9, 8, 0.875, 1), (7, 5, 0.3125, 1), UNNAMED, (-1, 4, 0.3125, 1)]
    h.label([0], obs[3:4], [[(0.3125, 6, -1), (0.3, 8, 9)]], st[3:4])      # another unlabelled row below accept
    assert h.named(0)[4][:4] == UNNAMED
    # two observations of track 1 in one call, rows 0 and 5 of the frame: first named 7, then an empty top
    two = [(0, 0, 1), (0, 5, 1)]
    h.label([0], two, [[(0.75, 3, 7)], [(-INF, -1, -1)]], [0, 0])
    assert h.named(0)[1][:4] == UNNAMED
    h.label([0], two, [[(-INF, -1, -1)], [(0.75, 3, 7)]], [0, 0])
    assert h.named(0)[1][:4] == (7, 3, 0.75, 1)
    h.label([0], obs[:1], [[(0.75, 3, 7)]], st[:1], with_ids=False)        # a plain search: identities read -1, "the same" fails
    assert h.named(0)[1][:4] == (-1, 3, 0.75, 1)


def case_a_slot_reborn_under_a_new_serial(h):
    """track 1 in slot 0 is fused and named, misses a frame and ends; track 2 is born in slot 0.  The entry is stale: not listed,
    not named for who, and the first fuse of track 2 clears it.  An embedding of track 1 that arrives late is "no track"."""
    h.start(dim=64)
    d = h.dim
    h.frames([(0, [0])])
    _, st = h.fuse([0], [(0, 0, 1)], [vec(d, {0: 1})], weight=[2])
    h.label([0], [(0, 0, 1)], [[(0.75, 3, 7)]], st)
    assert h.named(0) == {1: (7, 3, 0.75, 1, 1, 2.0)}
    who, ident, score = h.who([0], [[1, 2]], [2], flags=[[2, 2]])
    assert who[0, :2].tolist() == [10, 2] and ident[0, :2].tolist() == [7, -1] and score[0, :2].tolist() == [0.75, -INF]
    track, _, _ = h.frames([(0, [5])])
    assert track[0, 0] == 2
    assert h.entries(0) == [] and h.template(0, 1) is None and h.template(0, 2) is None
    who, ident, score = h.who([0], [[1, 2]], [2], flags=[[2, 2]])
    assert who[0, :2].tolist() == [2, 2] and ident[0, :2].tolist() == [-1, -1]
    q, st = h.fuse([0], [(0, 0, 1), (0, 1, 2)], [vec(d, {0: 1}), vec(d, {1: 4})], weight=[1, 3])
    assert st.tolist() == [1, 0] and bits(q[1]) == bits(vec(d, {1: 1}))
    assert h.named(0) == {2: UNNAMED + (1, 3.0)} and bits(h.template(0, 2)) == bits(vec(d, {1: 3}))
    h.label([0], [(0, 0, 1)], [[(0.75, 3, 7)]], [0])                        # a late answer for track 1 names nobody
    assert h.named(0) == {2: UNNAMED + (1, 3.0)}


def case_totals_and_counts(h):
    """total 0 and negative skip every observation, a total above m is clamped to m, a total of 1 stops after t = 0; who's counts
    0, negative and above max_det; flags_in NULL; who in place; streams are independent"""
    h.start(streams=2, dim=64)
    h.frames([(1, [0, 1]), (0, [3])])
    d = h.dim
    obs = [(0, 0, 1), (0, 1, 2), (1, 0, 1)]
    emb = [vec(d, {0: 1}), vec(d, {1: 1}), vec(d, {2: 1})]
    for total in (0, -3):
        q, st = h.fuse([1, 0], obs, emb, total=total)
        assert st.tolist() == [FILL32] * 3 and (q.view(np.uint32) == FILLU).all()
    q, st = h.fuse([1, 0], obs, emb, total=1)
    assert st.tolist() == [0, FILL32, FILL32] and (q[1:].view(np.uint32) == FILLU).all()
    q, st = h.fuse([1, 0], obs, emb, total=8)
    assert st.tolist() == [0, 0, 0]
    assert h.named(1) == {1: UNNAMED + (2, 2.0), 2: UNNAMED + (1, 1.0)} and h.named(0) == {1: UNNAMED + (1, 1.0)}
    h.label([1, 0], obs, [[(0.75, 3, 7)], [(0.75, 4, 8)], [(0.75, 5, 9)]], st, total=2)     # the third is past the total
    assert h.named(1)[2][:4] == (8, 4, 0.75, 1) and h.named(0)[1][:4] == UNNAMED
    md = h.max_det
    rows = [1, 2, 0, 1] + [2] * (md - 4)
    who, ident, score = h.who([1, 0, 1, 1, 1], [rows] * 5, [4, 4, 0, -2, md + 1])
    assert who[0, :4].tolist() == [8, 8, 0, 8] and ident[0, :4].tolist() == [7, 8, -1, 7] and who[0, 4] == FILLU
    assert who[1, :4].tolist() == [0, 0, 0, 0] and ident[1, :4].tolist() == [-1] * 4        # stream 0's track 1 is unnamed
    assert (who[2:4] == FILLU).all() and (ident[2:4] == FILL32).all() and (score[2:4].view(np.uint32) == FILLU).all()
    assert who[4].tolist() == [8, 8, 0, 8] + [8] * (md - 4) and ident[4].tolist() == [7, 8, -1, 7] + [8] * (md - 4)
    who, ident, score = h.who([1], [rows], [3], flags=[[1, 2, 6]], in_place=True)
    assert who[0, :4].tolist() == [9, 10, 6, FILLU]


CASES = {f.__name__[5:]: f for f in (case_exact_norms_and_no_track, case_two_shots_of_weight_1_and_3, case_bad_weights_and_embeddings,
                                     case_thresholds_on_and_beside_their_boundaries, case_empty_entries_and_k_1,
                                     case_names_taken_over_kept_and_unlabelled, case_a_slot_reborn_under_a_new_serial, case_totals_and_counts)}
