"""Detection over overlapping views of a frame, merged on the device (include/rfd.h, "views": decode_views_kernel and the
unchanged sort and NMS behind it), against the restatement tests/views_ref.py BIT FOR BIT -- boxes, landmarks, scores, counts,
totals and gidx; there is no tolerance, both sides are the same f32 operations -- on the constructed inputs of
tests/views_cases.py, whose outcomes tests/test_views_ref_cpu.py writes down.  Contexts at 128x128 (672 anchors), 32 images.

Where each case lands in the kernels:
  counted          1023 / 1024 / 1025 / 2049 candidates of a frame over four views: one chunk of chunk_sort_kernel, exactly
                   full, the first key of a second chunk, three chunks merged by merge_rank_kernel -- across views
  many_views       Vmax = 25: 16 800 candidate slots a frame, nms_chunked_kernel; Vmax = 26: 17 472, nms_kernel<false>
  lds limit        462 views of a frame are the most launch_nms's LDS check lets through at 672 anchors, 463 are refused
  end to end       preprocess, network and merge on planned views of two 300x200 frames, host and device forms
"""
import ctypes as C

import numpy as np
import pytest

import helpers
import views_cases as K
import views_ref as V

pytestmark = pytest.mark.gpu

NET, NA, B = K.NET, K.NA, 32


@pytest.fixture(scope="module")
def det(rfd):
    d = rfd.RetinaFaceDetection(image_size=(NET, NET), max_batch_size=B, max_det=4096, confidence_threshold=K.CONF, iou_threshold=K.IOU)
    yield d
    d.close()


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _stack(heads):
    return [np.stack([h[k] for h in heads]) for k in range(9)]


def _same(got, totals, want, what=""):
    assert len(got) == len(want)
    for f, ((gd, gl, gg), (wd, wl, wg, total)) in enumerate(zip(got, want)):
        assert totals[f] == total and len(gd) == len(wd), (what, f, totals[f], total, len(gd), len(wd))
        assert np.array_equal(gg, wg), (what, f)
        assert np.array_equal(_bits(gd), _bits(wd)) and np.array_equal(_bits(gl), _bits(wl)), (what, f)


def _run(det, c, what=""):
    """the case through rfd_decode_nms_views, held against the restatement; -> the kernels' rows per frame"""
    det.set_thresholds(K.CONF, c["iou"])
    got = det.decode_nms_views(_stack(c["heads"]), c["views"], c["n_frames"], c["margin"], want_gidx=True)
    totals = det.last_total.copy()
    want = V.detect_views(c["heads"], c["views"], c["n_frames"], NET, NET, K.CONF, c["iou"], c["margin"], det.max_det)
    _same(got, totals, want, what)
    for f in range(c["n_frames"]):
        if c["want"] is not None:
            assert np.array_equal(got[f][2], K.want_gidx(c, f)), (what, f)
        if c["count"] is not None:
            assert totals[f] == c["count"][f], (what, f)
    return got, totals


def test_one_scale_1_full_view_is_rfd_decode_nms(det):
    c = K.P.decode_case("chain", 300, NET, NET)
    heads = [h[None] for h in c["heads"]]
    det.set_thresholds(K.CONF, c["iou_thr"])
    (d0, l0, g0), = det.decode_nms(heads, [1.0], want_gidx=True)
    t0 = det.last_total.copy()
    (d1, l1, g1), = det.decode_nms_views(heads, [(0, 0, 0, NET, NET, 0)], 1, 4.0, want_gidx=True)
    assert det.last_total[0] == t0[0] == len(c["kept_gidx"])
    # x / 1.0f + 0.0f changes no bit of a value that is not -0.0, and the decode makes none
    assert np.array_equal(_bits(d0), _bits(d1)) and np.array_equal(_bits(l0), _bits(l1))
    assert np.array_equal(g0, g1) and np.array_equal(g1, c["kept_gidx"])
    want = V.detect_views([c["heads"]], [(0, 0, 0, NET, NET, 0)], 1, NET, NET, K.CONF, c["iou_thr"], 4.0, det.max_det)
    _same([(d1, l1, g1)], det.last_total, want)


@pytest.mark.parametrize("sa,sb", [(0.9, 0.95), (0.95, 0.9), (0.9, 0.9)])
def test_a_face_whole_in_two_tiles_gives_one_row(det, sa, sb):
    got, totals = _run(det, K.two_tiles(sa, sb))
    assert totals[0] == 1 and got[0][2][0] // NA == (1 if sb > sa else 0)        # the better score's; equal scores: the lower view's


def test_inner_edge_full_view_and_uneven_frames(det):
    got, _ = _run(det, K.cut_by_an_inner_edge(), "cut")
    assert np.allclose(got[0][0][:, :4], [[20, 20, 50, 50], [100, 40, 140, 70]], atol=1e-3)
    got, _ = _run(det, K.full_view_and_tile(), "full view")                      # scale 1/2 against scale 1
    assert np.allclose(got[0][0][0, :4], [160, 160, 220, 230], atol=1e-3)
    got, totals = _run(det, K.frames_3_0_1(), "3, 0, 1 views")                   # Vmax = 3: unused slots, a frame with no view
    assert list(totals[:3]) == [3, 0, 2] and len(got[1][0]) == 0


@pytest.mark.parametrize("side", K.SIDES)
def test_the_rule_at_the_bound_and_one_step_either_way(det, side):
    for which in range(3):        # at the bound (kept), one f32 step inside (kept), one outside (dropped where the side is inner)
        got, totals = _run(det, K.edge_case(side, which), (side, which))
        assert list(totals[:2]) == [0 if which == 2 else 1, 1]
        x, y = K.OFF                                                             # offsets that are no multiple of a stride
        assert np.allclose(got[1][0][0, :4], np.float32(K.SIDE_BOXES[side]) + np.float32([x, y, x, y]), atol=1e-3)


@pytest.mark.parametrize("n", K.COUNTS)
def test_counted_candidates_over_four_views(det, n):
    got, totals = _run(det, K.counted(n))
    assert totals[0] == n == len(got[0][0])


@pytest.mark.parametrize("vmax", [25, 26])
def test_many_views_of_one_frame(det, vmax):
    got, totals = _run(det, K.many_views(vmax))
    assert 40 < totals[0] < 40 * vmax


def test_max_det_cuts_the_merged_list(rfd):
    small = rfd.RetinaFaceDetection(image_size=(NET, NET), max_batch_size=4, max_det=7, confidence_threshold=K.CONF, iou_threshold=K.IOU)
    got, totals = _run(small, K.truncated())
    assert totals[0] == 30 and len(got[0][0]) == 7
    small.close()


def test_the_lds_limit_of_the_nms(rfd):
    """462 views x 672 anchors = 310 464 candidate slots make an NMS bitmap of 4 852 words: with the 64 KiB box cache that is
    163 616 of the 163 840 bytes launch_nms allows; 463 views make 4 864 words and 16 bytes too many.  The accepted call runs:
    two boxes a view, the views 200 px apart, so every one of the 924 candidates is kept."""
    big = rfd.RetinaFaceDetection(image_size=(NET, NET), max_batch_size=512, max_det=1024, confidence_threshold=K.CONF, iou_threshold=K.IOU)
    heads, _ = K.view_heads([[10, 10, 40, 50], [60, 60, 100, 110]], [0.9, 0.8], 90)
    stacked = [np.broadcast_to(h[None], (462,) + h.shape) for h in heads]
    views = [(0, 200 * v, 0, NET, NET, 0) for v in range(463)]
    got = big.decode_nms_views(stacked, views[:462], 1, 4.0, want_gidx=True)
    totals = big.last_total.copy()
    want = V.detect_views([heads] * 462, views[:462], 1, NET, NET, K.CONF, K.IOU, 4.0, 1024)
    _same(got, totals, want)
    assert totals[0] == 924
    with pytest.raises(rfd.RfdError) as e:
        big.decode_nms_views([np.broadcast_to(h[None], (463,) + h.shape) for h in heads], views, 1, 4.0)
    assert e.value.status == rfd.RFD_ERR_CAPACITY and "463 views" in str(e.value) and "LDS" in str(e.value)
    big.close()


def _refused(rfd, det, status, views, n_frames=1, margin=4.0, frames=None, needle=None):
    """the call refuses with `status` and writes nothing: the host slabs keep their fill"""
    L = rfd.load_library()
    n = len(views)
    arr = (rfd.rfd_view * max(n, 1))(*[rfd.rfd_view(*v) for v in views])
    heads = [np.zeros(s, np.float32) for s in helpers.head_shapes(max(n, 1), NET, NET)]
    ptrs = (C.c_void_p * 9)(*[h.ctypes.data for h in heads])
    nf = max(n_frames, 1)
    boxes, lmk = np.full((nf, det.max_det, 5), 7, np.float32), np.full((nf, det.max_det, 10), 7, np.float32)
    count, total = np.full(nf, 7, np.int32), np.full(nf, 7, np.int32)
    d = rfd.rfd_dets(boxes.ctypes.data, lmk.ctypes.data, count.ctypes.data, total.ctypes.data)
    if frames is None:
        got = L.rfd_decode_nms_views(det._ctx, ptrs, arr, n, n_frames, margin, C.byref(d), None)
    else:
        imgs, keep = det._images(frames)
        got = L.rfd_detect_views_batch(det._ctx, imgs, len(frames), arr, n, margin, C.byref(d))
    msg = L.rfd_last_error().decode()
    assert got == status, (got, msg)
    assert needle is None or needle in msg, msg
    assert np.all(boxes == 7) and np.all(lmk == 7) and np.all(count == 7) and np.all(total == 7)


def test_refusals_enqueue_nothing(rfd, det):
    INV, CAP = rfd.RFD_ERR_INVALID_ARG, rfd.RFD_ERR_CAPACITY
    v = (0, 0, 0, NET, NET, 0)
    # the two capacity limits: frames x Vmax image slots (both numbers are named), and -- test_the_lds_limit_of_the_nms -- the LDS
    _refused(rfd, det, CAP, [v] * 17 + [(1,) + v[1:]], n_frames=2, needle="2 frames of up to 17 views")
    _refused(rfd, det, CAP, [v], n_frames=33, needle="33 frames of up to 1 views")
    _refused(rfd, det, CAP, [v] * 33, needle="33")                            # more views than max_batch_size
    _refused(rfd, det, CAP, [])                                                # n_views = 0
    # the argument rules
    _refused(rfd, det, INV, [(1,) + v[1:], v], n_frames=2, needle="sorted by frame")
    _refused(rfd, det, INV, [(1,) + v[1:]], n_frames=1, needle="names frame 1 of 1")
    _refused(rfd, det, INV, [(-1,) + v[1:]], needle="names frame -1")
    _refused(rfd, det, INV, [(0, 0, 0, 0, NET, 0)], needle="empty")
    _refused(rfd, det, INV, [(0, -1, 0, NET, NET, 0)], needle="outside")
    _refused(rfd, det, INV, [(0, 0, 0, NET, NET, 16)], needle="inner")
    _refused(rfd, det, INV, [(0, 0, 0, 1, 1000, 0)], needle="letterboxes to an empty")
    _refused(rfd, det, INV, [v], n_frames=0)
    for margin in (-1.0, float("nan"), float("inf")):
        _refused(rfd, det, INV, [v], margin=margin, needle="edge_margin")
    # with frames: a view must lie inside its frame
    frame = helpers.make_image(1, 150, 200)
    _refused(rfd, det, INV, [(0, 73, 0, NET, NET, 0)], frames=[frame], needle="does not lie inside")
    _refused(rfd, det, INV, [(0, 0, 23, NET, NET, 0)], frames=[frame], needle="does not lie inside")
    L = rfd.load_library()
    assert L.rfd_decode_nms_views(det._ctx, None, None, 1, 1, 4.0, None, None) == INV
    # the context still works
    _run(det, K.two_tiles(0.9, 0.95))


@pytest.fixture(scope="module")
def e2e(rfd):
    d = rfd.RetinaFaceDetection(image_size=(NET, NET), max_batch_size=B, max_det=256)
    d.init_synthetic_weights(1234)
    frames = [helpers.make_image(s, 200, 300) for s in (5, 6)]
    cfg = rfd.view_config((NET, NET))
    views = [v for f in range(2) for v in rfd.view_plan(300, 200, cfg, frame=f)]
    assert len(views) == 14                                                      # 3 x 2 tiles and the full view, per frame
    rois = [frames[v.frame][v.y:v.y + v.h, v.x:v.x + v.w] for v in views]        # the views as images of their own
    _, tensor, scales = d.preprocess(rois)
    heads = d.forward(tensor)                                                    # one pass of 14 images, as the views call runs it
    fg = np.concatenate([heads[3 * l][:, 2:4].reshape(len(views), -1) for l in range(3)], 1)
    d.set_thresholds(float(np.quantile(fg, 0.97)), 0.45)
    want = d.decode_nms_views(heads, views, 2, cfg.edge_margin)
    totals = d.last_total.copy()
    assert all(t > 0 for t in totals[:2]) and all(np.float32(s) == V.O.geometry(v.h, v.w, NET, NET)[2] for s, v in zip(scales, views))
    yield d, frames, views, cfg, want, totals
    d.close()


def _same_rows(got, want):
    return len(got) == len(want) and all(np.array_equal(_bits(a), _bits(c)) and np.array_equal(_bits(b), _bits(d)) for (a, b), (c, d) in zip(got, want))


def test_end_to_end_host_form(e2e):
    d, frames, views, cfg, want, totals = e2e
    got = d.detect_views(frames, views, cfg.edge_margin)
    assert np.array_equal(d.last_total, totals[:2]) and _same_rows(got, want)


def test_end_to_end_device_form_and_alignment(e2e):
    import torch
    d, frames, views, cfg, want, totals = e2e
    dev = torch.device("cuda", 0)
    bufs = [torch.from_numpy(f).to(dev) for f in frames]
    boxes = torch.full((2, d.max_det, 5), 7.0, dtype=torch.float32, device=dev)
    lmk = torch.full((2, d.max_det, 10), 7.0, dtype=torch.float32, device=dev)
    count, total = torch.full((2,), 7, dtype=torch.int32, device=dev), torch.full((2,), 7, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    for async_ in (True, False):
        d.detect_views_device([b.data_ptr() for b in bufs], [f.shape[:2] for f in frames], views, boxes.data_ptr(), lmk.data_ptr(),
                              count.data_ptr(), total.data_ptr(), cfg.edge_margin, async_=async_)
        d.sync()
        cnt = count.cpu().numpy()
        got = d._split(boxes.cpu().numpy(), lmk.cpu().numpy().reshape(2, -1, 5, 2), cnt)
        assert np.array_equal(total.cpu().numpy(), totals[:2]) and _same_rows(got, want), async_
    # the merged slab is an ordinary one: the face list and the alignment take its rows as they take the host call's
    a, b = d.align_detections(frames, got, cap=64), d.align_detections(frames, want, cap=64)
    assert a.total[0] == b.total[0] > 0 and a.valid == b.valid
    n = a.valid
    for x, y in ((a.first, b.first), (a.frame[:n], b.frame[:n]), (a.row[:n], b.row[:n]), (a.status[:n], b.status[:n]), (a.crops[:n], b.crops[:n])):
        assert np.array_equal(x, y)
    assert np.array_equal(_bits(a.box[:n]), _bits(b.box[:n])) and np.array_equal(_bits(a.kps[:n]), _bits(b.kps[:n]))
