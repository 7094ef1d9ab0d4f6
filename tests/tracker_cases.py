"""Constructed tracker cases (include/rfd.h, "tracker").  Every expected value is written down from the construction: boxes have
integer coordinates, so an IoU is a ratio of small integers worked out in the comments.  tests/test_tracker_ref_cpu.py holds
tests/tracker_ref.py to them; tests/test_tracker_gpu.py holds the library to the same numbers.

A case: cfg (fields of rfd_tracker_config besides streams) and frames.  A frame: s (stream), rows [[x1, y1, x2, y2, score]],
optionally q (a quality per row) and reset (a stream to reset BEFORE the frame); expected: track, flags, stats (matched, born,
ended, dropped) and ended (serials)."""
import numpy as np

F = np.float32
NAN = float("nan")
NEW, CONF, DUE = 1, 2, 4


def above(x):
    return float(np.nextafter(F(x), F(np.inf)))


def below(x):
    return float(np.nextafter(F(x), F(-np.inf)))


BASE = dict(max_tracks=64, iou_min=0.5, max_missed=5, min_score=0.5, new_score=0.5, min_hits=1, improve=1.1)
A, B, C_ = [0, 0, 9, 9], [100, 0, 109, 9], [200, 0, 209, 9]          # 10 x 10 boxes far from each other


def _iou_boundary(iou_min, second):
    # track [0,0,9,9] (area 100), row [0,0,9,4] (area 50): inter 50, 50 / (50 + 100 - 50) = 0.5 exactly
    return dict(cfg=dict(BASE, iou_min=iou_min), frames=[
        dict(s=0, rows=[A + [0.9]], track=[1], flags=[NEW | CONF | DUE], stats=(0, 1, 0, 0), ended=[]),
        dict(s=0, rows=[[0, 0, 9, 4, 0.9]], **second)])


CASES = {
    "iou_exactly_at_iou_min_matches": _iou_boundary(0.5, dict(track=[1], flags=[CONF], stats=(1, 0, 0, 0), ended=[])),
    "iou_one_step_below_iou_min_is_born": _iou_boundary(above(0.5), dict(track=[2], flags=[NEW | CONF | DUE], stats=(0, 1, 0, 0), ended=[])),
    "scores_at_and_below_the_two_thresholds": dict(cfg=dict(BASE, new_score=0.75), frames=[
        # at new_score: born; one step below: eligible, unmatched, no birth; at min_score: the same; below min_score: no part
        dict(s=0, rows=[A + [0.75], B + [below(0.75)], C_ + [0.5], [300, 0, 309, 9, below(0.5)]],
             track=[1, 0, 0, 0], flags=[NEW | CONF | DUE, 0, 0, 0], stats=(0, 1, 0, 0), ended=[]),
        # exactly min_score matches (q = 0.5 is not above 0.75 * 1.1: not due); the same box one step below takes no part
        dict(s=0, rows=[A + [0.5], A + [below(0.5)]], track=[1, 0], flags=[CONF, 0], stats=(1, 0, 0, 0), ended=[]),
        dict(s=0, rows=[A + [below(0.5)], A + [NAN]], track=[0, 0], flags=[0, 0], stats=(0, 0, 0, 0), ended=[]),
    ]),
    "ties_and_contention": dict(cfg=dict(BASE, iou_min=0.125), frames=[
        dict(s=0, rows=[A + [0.9], [20, 0, 29, 9, 0.9]], track=[1, 2], flags=[7, 7], stats=(0, 2, 0, 0), ended=[]),
        # row [5,0,24,9] (area 200): with slot 0 inter 5 x 10 = 50, 50 / (200 + 100 - 50) = 0.2; with slot 1 the same: slot 0 wins
        dict(s=0, rows=[[5, 0, 24, 9, 0.9]], track=[1], flags=[CONF], stats=(1, 0, 0, 0), ended=[]),
        # slot 0 is [5,0,24,9], slot 1 [20,0,29,9].  Row 0 = slot 0's box: IoU 1 beats 0.2.  Row 1 [6,0,25,9] prefers slot 0
        # (190 / 210) but it is taken: slot 1, 60 / (200 + 100 - 60) = 0.25
        dict(s=0, rows=[[5, 0, 24, 9, 0.9], [6, 0, 25, 9, 0.8]], track=[1, 2], flags=[CONF, CONF], stats=(2, 0, 0, 0), ended=[]),
        # slot 1 is [6,0,25,9] now: row 0 takes it at IoU 1 (slot 0: 190 / 210), row 1 is left slot 0
        dict(s=0, rows=[[6, 0, 25, 9, 0.9], [6, 0, 25, 9, 0.8]], track=[2, 1], flags=[CONF, CONF], stats=(2, 0, 0, 0), ended=[]),
        # both slots hold [6,0,25,9]: IoU 1 twice, the lower slot first; the third row finds no open slot and is born
        dict(s=0, rows=[[6, 0, 25, 9, 0.9], [6, 0, 25, 9, 0.8], [6, 0, 25, 9, 0.7]], track=[1, 2, 3], flags=[CONF, CONF, 7],
             stats=(2, 1, 0, 0), ended=[]),
    ]),
    "lifecycle_and_reset": dict(cfg=dict(BASE, max_missed=2), frames=[
        dict(s=0, rows=[A + [0.9], B + [0.9]], track=[1, 2], flags=[7, 7], stats=(0, 2, 0, 0), ended=[]),
        dict(s=0, rows=[B + [0.9]], track=[2], flags=[CONF], stats=(1, 0, 0, 0), ended=[]),          # slot 0 missed 1
        dict(s=0, rows=[], track=[], flags=[], stats=(0, 0, 0, 0), ended=[]),                          # an empty frame ages: 2, 1
        # slot 0's third unmatched frame: it ends, and the birth of this frame takes its slot
        dict(s=0, rows=[B + [0.9], C_ + [0.9]], track=[2, 3], flags=[CONF, 7], stats=(1, 1, 1, 0), ended=[1]),
        dict(s=0, rows=[], track=[], flags=[], stats=(0, 0, 0, 0), ended=[]),
        dict(s=0, rows=[], track=[], flags=[], stats=(0, 0, 0, 0), ended=[]),
        dict(s=0, rows=[], track=[], flags=[], stats=(0, 0, 2, 0), ended=[3, 2]),                      # ascending SLOT order: 3 sits in slot 0
        dict(s=0, rows=[A + [0.9]], track=[4], flags=[7], stats=(0, 1, 0, 0), ended=[]),
        # reset: track 4 vanishes without an ended entry, the same box is born again, serials go on
        dict(s=0, reset=0, rows=[A + [0.9]], track=[5], flags=[7], stats=(0, 1, 0, 0), ended=[]),
    ]),
    "confirmation_at_the_third_hit_and_due": dict(cfg=dict(BASE, min_hits=3, improve=1.25), frames=[
        dict(s=0, rows=[A + [0.9]], q=[0.5], track=[1], flags=[NEW], stats=(0, 1, 0, 0), ended=[]),
        dict(s=0, rows=[A + [0.9]], q=[0.5], track=[1], flags=[0], stats=(1, 0, 0, 0), ended=[]),
        dict(s=0, rows=[A + [0.9]], q=[0.5], track=[1], flags=[CONF | DUE], stats=(1, 0, 0, 0), ended=[]),       # the first confirmed shot
        dict(s=0, rows=[A + [0.9]], q=[0.625], track=[1], flags=[CONF], stats=(1, 0, 0, 0), ended=[]),           # 0.5 * 1.25 exactly: not above
        dict(s=0, rows=[A + [0.9]], q=[above(0.625)], track=[1], flags=[CONF | DUE], stats=(1, 0, 0, 0), ended=[]),
        dict(s=0, rows=[A + [0.9]], q=[NAN], track=[1], flags=[CONF], stats=(1, 0, 0, 0), ended=[]),             # never due, shot_q stays
        dict(s=0, rows=[A + [0.9]], q=[0.75], track=[1], flags=[CONF], stats=(1, 0, 0, 0), ended=[]),            # 0.75 < above(0.625) * 1.25
        dict(s=0, rows=[A + [0.9]], q=[1.0], track=[1], flags=[CONF | DUE], stats=(1, 0, 0, 0), ended=[]),
    ]),
    "confirmation_at_the_second_hit": dict(cfg=dict(BASE, min_hits=2), frames=[
        dict(s=0, rows=[A + [0.9]], track=[1], flags=[NEW], stats=(0, 1, 0, 0), ended=[]),
        dict(s=0, rows=[A + [0.9]], track=[1], flags=[CONF | DUE], stats=(1, 0, 0, 0), ended=[]),                 # q = the score 0.9
        dict(s=0, rows=[A + [0.9]], track=[1], flags=[CONF], stats=(1, 0, 0, 0), ended=[]),                       # 0.9 is not above 0.9 * 1.1
    ]),
    "non_finite_box": dict(cfg=dict(BASE, max_missed=1), frames=[
        dict(s=0, rows=[[NAN, 0, 9, 9, 0.9]], track=[1], flags=[7], stats=(0, 1, 0, 0), ended=[]),
        dict(s=0, rows=[[NAN, 0, 9, 9, 0.9]], track=[2], flags=[7], stats=(0, 1, 0, 0), ended=[]),               # a NaN IoU matches nothing
        # track 1's second unmatched frame ends it; the finite row matches neither NaN track and is born into the freed slot 0
        dict(s=0, rows=[A + [0.9]], track=[3], flags=[7], stats=(0, 1, 1, 0), ended=[1]),
        dict(s=0, rows=[A + [0.9]], track=[3], flags=[CONF], stats=(1, 0, 1, 0), ended=[2]),
    ]),
    "streams_are_independent": dict(cfg=dict(BASE, streams=2), frames=[
        dict(s=1, rows=[A + [0.9]], track=[1], flags=[7], stats=(0, 1, 0, 0), ended=[]),
        dict(s=0, rows=[A + [0.9]], track=[1], flags=[7], stats=(0, 1, 0, 0), ended=[]),                          # its own serials, no match over streams
        dict(s=1, rows=[A + [0.9], B + [0.9]], track=[1, 2], flags=[CONF, 7], stats=(1, 1, 0, 0), ended=[]),
    ]),
}


def crowd(max_tracks, rows=1024):
    """`rows` copies of one box over one track of that box: row 0 matches, the free slots fill, the rest are dropped"""
    born = max_tracks - 1
    first = dict(s=0, rows=[A + [0.9]], track=[1], flags=[7], stats=(0, 1, 0, 0), ended=[])
    many = dict(s=0, rows=[A + [0.9]] * rows, track=[1] + list(range(2, 2 + born)) + [0] * (rows - 1 - born),
                flags=[CONF] + [7] * born + [0] * (rows - 1 - born), stats=(1, born, 0, rows - 1 - born), ended=[])
    return dict(cfg=dict(BASE, max_tracks=max_tracks), frames=[first, many])


def slabs(frames, max_det, with_quality):
    """the frames of a case as the library takes them: streams [n], boxes [n, max_det, 5], landmarks [n, max_det, 5, 2] (a
    pattern of the row), count [n], quality [n, max_det] or None"""
    n = len(frames)
    boxes, lmk = np.zeros((n, max_det, 5), F), np.zeros((n, max_det, 5, 2), F)
    count, q = np.zeros(n, np.int32), (np.zeros((n, max_det), F) if with_quality else None)
    for b, f in enumerate(frames):
        k = len(f["rows"])
        count[b] = k
        if k:
            boxes[b, :k] = np.asarray(f["rows"], F)
            lmk[b, :k] = (np.arange(k * 10, dtype=F) + F(1000 * b)).reshape(k, 5, 2)
            if with_quality:
                q[b, :k] = np.asarray(f.get("q", boxes[b, :k, 4]), F)
    return np.asarray([f["s"] for f in frames], np.int32), boxes, lmk, count, q
