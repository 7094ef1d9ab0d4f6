"""tests/views_ref.py, the test-side statement of detection over views (include/rfd.h, "views"), pinned without a GPU: one
scale-1 view of the whole network image is the oracle's decode_nms itself, and the constructed cases of tests/views_cases.py
give the outcomes written down from their construction."""
import numpy as np
import pytest

import helpers
import views_cases as K
import views_ref as V

NET, NA = K.NET, K.NA


def _run(c, max_det=4096):
    return V.detect_views(c["heads"], c["views"], c["n_frames"], NET, NET, K.CONF, c["iou"], c["margin"], max_det)


def _holds(c, max_det=4096):
    got = _run(c, max_det)
    assert len(got) == c["n_frames"]
    for f, (det, lmk, gidx, total) in enumerate(got):
        assert len(det) == len(lmk) == len(gidx) == min(total, max_det)
        assert np.all(np.diff(det[:, 4]) <= 0)
        if c["want"] is not None:
            assert np.array_equal(gidx, K.want_gidx(c, f)), (f, gidx)
        if c["count"] is not None:
            assert total == c["count"][f]
        elif c["want"] is not None:
            assert total == len(c["want"][f])
    return got


def test_one_scale_1_view_is_the_oracles_decode_nms(oracle):
    """bit for bit: x / 1.0f + 0.0f changes no bit of a value that is not -0.0, and the decode makes none (a difference that
    cancels gives +0.0, and the clip's max with +0.0 has nothing negative to pass on)"""
    bits = lambda a: np.ascontiguousarray(a, np.float32).view(np.uint32)
    for seed, iou in ((3, 0.45), (4, 0.3)):
        heads = [h[0] for h in helpers.make_heads(seed, 1, NET, NET, cand_rate=0.1, n_faces=4)]
        det, lmk, gidx, _ = oracle.decode_nms(heads, NET, NET, np.float32(K.CONF), iou, 1.0)
        (d, l, g, total), = V.detect_views([heads], [(0, 0, 0, NET, NET, 0)], 1, NET, NET, K.CONF, iou, 4.0, NA)
        assert total == len(det) > 5
        assert np.array_equal(bits(d), bits(det)) and np.array_equal(bits(l), bits(lmk)) and np.array_equal(g, gidx)
        # every side inner and no margin drops nothing: the clip leaves every coordinate within [0, 127]
        (d15, _, _, _), = V.detect_views([heads], [(0, 0, 0, NET, NET, 15)], 1, NET, NET, K.CONF, 2.0, 0.0, NA)
        every = oracle.decode_nms(heads, NET, NET, np.float32(K.CONF), 2.0, 1.0)[0]
        assert np.array_equal(d15, every)


def test_slots_and_sort_bits():
    assert V.slots([(0,) * 6, (0,) * 6, (2,) + (0,) * 5, (3,) + (0,) * 5, (3,) + (0,) * 5]) == [0, 1, 0, 0, 1]
    s = np.array([0.9, -0.0, 0.0, 0.5, np.inf, -1.0, 0.9], np.float32)
    order = np.lexsort((np.arange(len(s)), V.sort_bits(s)))
    assert list(order) == [4, 0, 6, 3, 1, 2, 5]


def test_a_face_whole_in_two_tiles_gives_one_row():
    for sa, sb, winner in ((0.9, 0.95, 1), (0.95, 0.9, 0), (0.9, 0.9, 0)):   # the better score's; equal scores: the lower view's
        c = K.two_tiles(sa, sb)
        (det, _, gidx, _), = _holds(c)
        assert gidx[0] // NA == winner and det[0, 4] == np.float32(max(sa, sb))
        assert np.allclose(det[0, :4], [90, 40, 110, 70], atol=1e-3)


def test_a_face_cut_by_an_inner_edge_is_left_to_the_neighbour():
    (det, _, _, _), = _holds(K.cut_by_an_inner_edge())
    assert np.allclose(det[:, :4], [[20, 20, 50, 50], [100, 40, 140, 70]], atol=1e-3)     # B's whole box, in frame pixels
    # without the rule the half-box, the best score of the frame, is kept and suppresses the whole face (IoU 868 / 1271)
    c = dict(K.cut_by_an_inner_edge(), views=[(0, 0, 0, NET, NET, 0), (0, 72, 0, NET, NET, 0)])
    (det, _, _, total), = V.detect_views(c["heads"], c["views"], 1, NET, NET, K.CONF, c["iou"], c["margin"], 64)
    assert total == 2 and det[0, 2] == 127.0 and det[0, 4] == np.float32(0.99)


def test_the_full_view_and_a_tile_meet_in_frame_pixels():
    (det, _, _, _), = _holds(K.full_view_and_tile())
    assert np.allclose(det[0, :4], [160, 160, 220, 230], atol=1e-3) and det[0, 4] == np.float32(0.9)


def test_frames_with_three_views_none_and_one():
    got = _holds(K.frames_3_0_1())
    assert [g[3] for g in got] == [3, 0, 2]
    assert np.allclose(got[0][0][0, :4], np.float32([30, 50, 60, 90]) + np.float32([K.OFF[0] + 260, K.OFF[1]] * 2), atol=1e-3)


@pytest.mark.parametrize("side", K.SIDES)
def test_the_rule_at_the_bound_and_one_step_either_way(side):
    _, _, (at, inside, outside) = K.edge_margins(side)
    assert inside < at < outside
    for which in range(3):
        _holds(K.edge_case(side, which))


@pytest.mark.parametrize("n", K.COUNTS)
def test_counted_candidates_over_four_views(n):
    (det, _, gidx, total), = _holds(K.counted(n))
    assert total == n and len(np.unique(gidx)) == n and set(gidx // NA) == {0, 1, 2, 3}
    assert list(gidx[:8] // NA) == [0, 1, 2, 3, 0, 1, 2, 3]         # the order interleaves the views


def test_many_views_suppress_across_views():
    for vmax in (25, 26):
        c = K.many_views(vmax)
        (det, _, gidx, total), = _holds(c)
        assert 40 < total < 40 * vmax and len(set(gidx // NA)) > 3


def test_max_det_cuts_the_merged_list():
    (det, _, gidx, total), = _holds(K.truncated(), max_det=7)
    assert total == 30 and len(det) == 7
