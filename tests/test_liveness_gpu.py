"""The liveness stage on the device (include/rfd.h: rfd_liveness_tensors, rfd_liveness_tensors_device, rfd_liveness_decide,
rfd_liveness_decide_device) against tests/liveness_ref.py, the numpy restatement of face_antispoofing.rs.

Every tensor value is an integer of the restated cv::resize converted exactly to f32, every weight and score a pinned sequence
of single IEEE f32 operations, every ROI an integer: the bar is np.array_equal throughout.  Each case first asserts ON THE
REFERENCE ALONE that the branch it is there for is reached, so that a case cannot silently stop covering it.
Parity status: byte-exact against the oracle's restatement of cv::resize; unpinned against a running OpenCV, like alignment."""
import ctypes as C

import numpy as np
import pytest

import helpers
import liveness_ref as R

pytestmark = pytest.mark.gpu

f32 = np.float32


@pytest.fixture(scope="module")
def det(rfd):
    d = rfd.RetinaFaceDetection(max_batch_size=6, max_det=64)   # the liveness stage needs no network weights
    yield d
    d.close()


@pytest.fixture(scope="module")
def frames():
    wide = helpers.make_image(503, 300, 480, n_blobs=5)
    view = wide[:, 40:440]                                      # 300 x 400, a strided view of a wider array
    assert view.strides[0] == 1440 and view.shape == (300, 400, 3)
    return dict(small=helpers.make_image(501, 96, 128, n_blobs=5), mid=helpers.make_image(502, 240, 320, n_blobs=5), view=view,
                wide=wide)


def _check(got, want, what):
    tensors, weights, rois, status = got
    wt, ww, wr, ws, _ = want
    assert np.array_equal(status, ws), (what, status.tolist(), ws.tolist())
    assert np.array_equal(rois, wr), (what, rois.tolist(), wr.tolist())
    assert np.array_equal(weights.view(np.uint32), ww.view(np.uint32)), (what, weights.tolist(), ww.tolist())
    for j, (g, w) in enumerate(zip(tensors, wt)):
        assert g.shape == w.shape and np.array_equal(g, w), (what, j)


# name, frame, box, found, what the reference must show for the case to be the case
CASES = [
    ("centred", "mid", (100, 60, 180, 160), 1,
     lambda r: r["status"] == 0 and r["shifts"][2] == [] and r["shifts"][3] == [] and r["weights"][3] == 1.0),
    ("left", "mid", (2, 80, 42, 140), 1, lambda r: r["status"] == 0 and r["shifts"][3] == ["left"] and r["rois"][3][0] == 0),
    ("top", "mid", (140, 2, 180, 62), 1, lambda r: r["status"] == 0 and r["shifts"][2] == ["top"] and r["rois"][2][1] == 0),
    ("right", "mid", (278, 80, 318, 140), 1, lambda r: r["status"] == 0 and r["shifts"][3] == ["right"] and r["rois"][3][2] == 319),
    ("bottom", "mid", (140, 178, 180, 238), 1, lambda r: r["status"] == 0 and r["shifts"][2] == ["bottom"] and r["rois"][2][3] == 239),
    ("larger than the frame", "mid", (0, -200, 320, 600), 1, lambda r: r["status"] == 0 and (r["weights"] < 1.0).all()),
    ("every model up-samples", "small", (60, 40, 66, 48), 1,
     lambda r: r["status"] == 0 and all(r["rois"][j][2] - r["rois"][j][0] + 1 < R.DEFAULT_SIZES[j][0] and
                                        r["rois"][j][3] - r["rois"][j][1] + 1 < R.DEFAULT_SIZES[j][1] for j in range(4))),
    ("strided frame", "view", (150, 80, 260, 220), 1, lambda r: r["status"] == 0 and (r["weights"] < 1.0).any()),
    ("no face", "mid", (100, 60, 180, 160), 0, lambda r: r["status"] == -2),
    ("degenerate", "mid", (100, 100, 180, 90), 1, lambda r: r["status"] == -3),
]


@pytest.mark.parametrize("part", [0, 1])
def test_default_config_every_branch(det, oracle, frames, part):
    cases = CASES[5 * part:5 * part + 5]
    fr = [frames[c[1]] for c in cases]
    boxes = np.array([c[2] for c in cases], np.float32)
    found = np.array([c[3] for c in cases], np.int32)
    want = R.batch(fr, boxes, found, oracle=oracle)
    for c, r in zip(cases, want[4]):
        assert c[4](r), "the reference does not reach the branch of case '%s': %s" % (c[0], {k: v for k, v in r.items() if k != "tensors"})
    got = det.liveness_tensors(fr, boxes, found)
    _check(got, want, [c[0] for c in cases])
    for i, st in enumerate(want[3]):
        for t, w in zip(got[0], got[1].T):
            assert (t[i].any() and w[i] > 0) if st == 0 else (not t[i].any() and w[i] == 0)


def _search_roi(frame_hw, out_wh, want_wh):
    """a box whose scale-1.0 ROI is exactly want_wh (w, h): a search over the box centre and height, on the reference alone"""
    for ymin in range(10, 40):
        for h in range(want_wh[1] - 4, want_wh[1] + 2):
            for cx4 in range(4 * 130, 4 * 260):
                box = (cx4 / 4.0 - 50, ymin, cx4 / 4.0 + 50, ymin + h)
                l, t, r, b, w, _ = R.new_box(frame_hw[1], frame_hw[0], R.scale_image_box(box), 1.0)
                if (r - l + 1, b - t + 1) == want_wh and w == 1.0 and R.roi_ok(R.roi_rect(l, t, r, b), frame_hw[1], frame_hw[0]):
                    return box
    return None


def test_the_two_by_two_mean_branch(rfd, det, oracle, frames):
    """cv::resize switches to the 2x2 mean when both scale factors are exactly 2.  The crop box is 0.94 x its height wide, so
    with the default config's SQUARE model inputs no ordinary box gives a ROI of exactly twice the input (256 x 256 for the
    128 model would need a square ROI); a model input of 120 x 128 does: the search finds a box whose ROI is 240 x 256."""
    view = frames["view"]
    box = _search_roi(view.shape[:2], (120, 128), (240, 256))
    assert box is not None
    cfg = rfd.liveness_config([1.0, 1.0], [(120, 128), (128, 128)])      # the second model resizes the same ROI generically
    want = R.batch([view], [box], [1], [1.0, 1.0], [(120, 128), (128, 128)], oracle=oracle)
    l, t, r, b = want[2][0, 0]
    assert (r - l + 1, b - t + 1) == (240, 256) and want[3][0] == 0
    roi = view[t:b + 1, l:r + 1].astype(np.int32)
    mean = (roi[0::2, 0::2] + roi[0::2, 1::2] + roi[1::2, 0::2] + roi[1::2, 1::2] + 2) >> 2
    assert np.array_equal(want[0][0][0], mean.transpose(2, 0, 1).astype(np.float32))   # the reference took the 2x2 mean
    _check(det.liveness_tensors([view], np.array([box], np.float32), cfg=cfg), want, "2x2 mean")


@pytest.mark.parametrize("scales,sizes", [([2.0], [(3, 2)]), ([1.5, 3.0, 1.0], [(96, 80), (3, 2), (64, 64)])])
def test_custom_configs(rfd, det, oracle, frames, scales, sizes):
    fr = [frames["mid"], frames["small"], frames["view"], frames["mid"]]
    boxes = np.array([(100, 60, 180, 160), (30, 20, 70, 80), (150, 80, 260, 220), (100, 100, 180, 90)], np.float32)
    found = np.array([1, 3, 1, 1], np.int32)
    want = R.batch(fr, boxes, found, scales, sizes, oracle=oracle)
    assert want[3].tolist() == [0, 0, 0, -3]
    got = det.liveness_tensors(fr, boxes, found, cfg=rfd.liveness_config(scales, sizes))
    assert [t.shape for t in got[0]] == [(4, 3, h, w) for w, h in sizes]
    _check(got, want, (scales, sizes))


def test_argument_errors(rfd, det, frames):
    fr = [frames["mid"]]
    box = np.array([(100, 60, 180, 160, 0.9)], np.float32)

    def refuse(cfg, status, word, n=1):
        with pytest.raises(rfd.RfdError) as e:
            det.liveness_tensors(fr * n, np.repeat(box, n, 0), cfg=cfg)
        assert e.value.status == status and word in str(e.value), str(e.value)

    refuse(rfd.liveness_config([1.0] * 5, [(8, 8)] * 5), rfd.RFD_ERR_CAPACITY, "RFD_MAX_FACE_TENSORS")
    refuse(rfd.liveness_config([], []), rfd.RFD_ERR_INVALID_ARG, "k = 0")
    refuse(rfd.liveness_config([1.0, 1.0], [(8, 8), (0, 8)]), rfd.RFD_ERR_INVALID_ARG, "out_w[1]")
    refuse(rfd.liveness_config([1.0], [(8, -1)]), rfd.RFD_ERR_INVALID_ARG, "out_h[0]")
    for bad in (0.0, -1.0, np.inf, np.nan):
        refuse(rfd.liveness_config([1.0, 2.0, bad], [(8, 8)] * 3), rfd.RFD_ERR_INVALID_ARG, "scale[2]")
    refuse(None, rfd.RFD_ERR_CAPACITY, "max_batch_size", n=7)
    L = rfd.load_library()
    arr, keep = det._images(fr)
    cfg = rfd.liveness_config()
    outs = [np.zeros((1, 3, h, w), np.float32) for w, h in R.DEFAULT_SIZES]
    ptrs = (C.c_void_p * 4)(outs[0].ctypes.data, outs[1].ctypes.data, None, outs[3].ctypes.data)
    found, weights, status = np.ones(1, np.int32), np.zeros((1, 4), np.float32), np.zeros(1, np.int32)
    args = [det._ctx, arr, 1, box.ctypes.data, found.ctypes.data, C.addressof(cfg), ptrs, weights.ctypes.data, None, status.ctypes.data]
    assert L.rfd_liveness_tensors(*args) == rfd.RFD_ERR_INVALID_ARG and b"tensor pointer 2 is null" in L.rfd_last_error()
    ptrs[2] = outs[2].ctypes.data
    assert L.rfd_liveness_tensors(*args) == rfd.RFD_OK and status[0] == 0          # rois = NULL is allowed
    args[7] = None
    assert L.rfd_liveness_tensors(*args) == rfd.RFD_ERR_INVALID_ARG and b"null" in L.rfd_last_error()
    one = np.zeros((2, 2), np.float32)
    lp = (C.c_void_p * 1)(one.ctypes.data)
    assert L.rfd_liveness_decide(det._ctx, lp, 1, 2, 1, one.ctypes.data, 0.55, one.ctypes.data, status.ctypes.data) == rfd.RFD_ERR_INVALID_ARG
    assert b"classes < 2" in L.rfd_last_error()


# ---- device-resident ---------------------------------------------------------------------------------------------------
def test_device_form_on_a_strided_frame(det, oracle, frames):
    """rfd_liveness_tensors_device on a frame whose rows are 1440 bytes apart in HBM (a view of a wider array): the kernel
    walks the frame's stride, and its 8-byte loads stay inside the ROI's rows"""
    import torch
    dev = torch.device("cuda", 0)
    wide = torch.from_numpy(frames["wide"]).to(dev)
    view = frames["view"]
    boxes = np.array([(150, 80, 260, 220, 0.9), (330, 10, 399, 120, 0.9), (1, 200, 60, 299, 0.9)], np.float32)
    found = np.array([1, 1, 3], np.int32)
    want = R.batch([view] * 3, boxes, found, oracle=oracle)
    assert want[3].tolist() == [0, 0, 0] and want[2][1, 3, 2] == 399 and want[2][2, 3, 3] == 299   # ROIs that end at the frame's last column / row
    d_box, d_found = torch.from_numpy(boxes).to(dev), torch.from_numpy(found).to(dev)
    t = [torch.full((3, 3, h, w), -1.0, device=dev) for w, h in R.DEFAULT_SIZES]
    d_w, d_r, d_s = torch.zeros(3, 4, device=dev), torch.zeros(3, 4, 4, dtype=torch.int32, device=dev), torch.zeros(3, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    det.liveness_tensors_device([wide.data_ptr() + 40 * 3] * 3, [view.shape[:2]] * 3, d_box.data_ptr(), d_found.data_ptr(),
                                [x.data_ptr() for x in t], d_w.data_ptr(), d_r.data_ptr(), d_s.data_ptr(), strides=[1440] * 3)   # async = 0
    _check(([x.cpu().numpy() for x in t], d_w.cpu().numpy(), d_r.cpu().numpy(), d_s.cpu().numpy()), want, "strided device frame")


@pytest.fixture(scope="module")
def chain(rfd):
    """A context of its own, with weights, that has never made a liveness call; two frames whose detections come from the
    network and one without any, by the calibration idiom of test_face_tensors_gpu.py: the threshold is read off the head
    tensors, between the best foreground score of the quietest flat frame and that of the busy frames."""
    d = rfd.RetinaFaceDetection(max_batch_size=9, max_det=512)
    d.init_synthetic_weights(1234)
    busy = [helpers.make_image(400 + i, 240, 320, n_blobs=5) for i in range(3)]
    rng = np.random.default_rng(7)
    quiet = [np.zeros((240, 320, 3), np.uint8), np.full((240, 320, 3), 128, np.uint8), np.full((300, 200, 3), 255, np.uint8),
             np.full((240, 320, 3), 64, np.uint8), np.full((240, 320, 3), 192, np.uint8),
             rng.integers(100, 104, size=(240, 320, 3), dtype=np.uint8)]
    allf = busy + quiet
    _, tn, _ = d.preprocess(allf)
    heads = d.forward(tn)
    best = np.concatenate([heads[3 * l][:, 2:4].reshape(len(allf), -1) for l in range(3)], 1).max(1)
    print("best foreground score per frame:", best.tolist())
    order = np.argsort(best[0:3])[::-1]
    a, b, c = int(order[0]), int(order[1]), 3 + int(np.argmin(best[3:]))
    lo, hi = float(best[c]), float(best[b])
    assert lo < hi, "no calibration separates the empty frame: %s" % best.tolist()
    d.set_thresholds(lo + 0.25 * (hi - lo), 0.45)
    fr = [np.ascontiguousarray(allf[a]), np.ascontiguousarray(allf[b]), np.ascontiguousarray(allf[c])]
    before = d.call_batch(fr)                    # before the context's first liveness call
    yield d, fr, before
    d.close()


def test_device_resident_chain(rfd, oracle, chain):
    """rfd_detect_faces_device, then rfd_liveness_tensors_device on the box / found buffers it is filling, both async, one
    rfd_sync: equal to the host form fed with the boxes read back afterwards (and to the reference); then rfd_detect_batch
    on this context still returns the bits it returned before the context's first liveness call."""
    import torch
    det, fr, before = chain
    dev = torch.device("cuda", 0)
    bufs = [torch.from_numpy(f).to(dev) for f in fr]
    q = rfd.face_tensor_config_quality()
    z = dict(box=torch.zeros(3, 5, device=dev), kps=torch.zeros(3, 10, device=dev), found=torch.zeros(3, dtype=torch.int32, device=dev),
             status=torch.zeros(3, dtype=torch.int32, device=dev), tensor=torch.zeros(3, 3, 112, 112, device=dev))
    t = [torch.full((3, 3, h, w), -1.0, device=dev) for w, h in R.DEFAULT_SIZES]
    d_w, d_r, d_s = torch.full((3, 4), -1.0, device=dev), torch.zeros(3, 4, 4, dtype=torch.int32, device=dev), torch.full((3,), 7, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    ptrs, shapes = [b.data_ptr() for b in bufs], [f.shape[:2] for f in fr]
    det.detect_faces_device(ptrs, shapes, [q], z["box"].data_ptr(), z["kps"].data_ptr(), z["found"].data_ptr(), None,
                            z["status"].data_ptr(), [z["tensor"].data_ptr()], is_enroll=True, async_=True)
    det.liveness_tensors_device(ptrs, shapes, z["box"].data_ptr(), z["found"].data_ptr(), [x.data_ptr() for x in t], d_w.data_ptr(),
                                d_r.data_ptr(), d_s.data_ptr(), async_=True)
    det.sync()
    torch.cuda.synchronize()
    box, found = z["box"].cpu().numpy(), z["found"].cpu().numpy()
    got = ([x.cpu().numpy() for x in t], d_w.cpu().numpy(), d_r.cpu().numpy(), d_s.cpu().numpy())
    print("found:", found.tolist(), "liveness status:", got[3].tolist(), "boxes:", box.tolist())
    assert (found[:2] & 1).all() and found[2] == 0 and got[3][2] == -2 and not any(x[2].any() for x in got[0])
    host = det.liveness_tensors(fr, box, found)
    _check(got, host + (None,), "device chain against the host form")
    _check(got, R.batch(fr, box, found, oracle=oracle), "device chain against the reference")
    after = det.call_batch(fr)
    assert len(after[0][0]) > 0 and len(after[2][0]) == 0
    for (b0, k0), (b1, k1) in zip(before, after):
        assert np.array_equal(b0, b1) and np.array_equal(k0, k1)


# ---- the decision rule ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 4, 8, 9, 17])   # 8 / 9: one launch takes eight models, more go through the running sums
def test_decide_host(det, k):
    rng = np.random.default_rng(60 + k)
    n = 6
    logits = [rng.uniform(-0.5, 1.5, size=(n, 3)).astype(np.float32) for _ in range(k)]
    w = rng.uniform(0.05, 1.0, size=(n, k)).astype(np.float32)
    w[1] = 0.0                                    # a face with a negative status: NaN, not live
    w[2] = 1.0
    for x in logits:
        x[2, 1] = f32(0.55)                       # every model says exactly the threshold: the mean of equal values ...
    want = R.decide(logits, w)
    if k == 1:
        assert want[0][2] == f32(0.55)            # ... is that value for one model: equality is not live
    assert np.isnan(want[0][1]) and want[1][1] == 0 and want[1].any() and not want[1].all()
    score, live = det.liveness_decide(logits, w)
    assert np.array_equal(score.view(np.uint32)[[0, 2, 3, 4, 5]], want[0].view(np.uint32)[[0, 2, 3, 4, 5]]) and np.isnan(score[1])
    assert np.array_equal(live, want[1])
    if k == 1:
        assert live[2] == 0
    score2, live2 = det.liveness_decide(logits, w, threshold=0.2)
    assert np.array_equal(score2, score, equal_nan=True) and np.array_equal(live2, R.decide(logits, w, 0.2)[1])


def test_decide_on_the_tensor_calls_weights_and_as_written(det, frames):
    cases = CASES[:3] + CASES[5:6] + CASES[8:]
    fr = [frames[c[1]] for c in cases]
    boxes, found = np.array([c[2] for c in cases], np.float32), np.array([c[3] for c in cases], np.int32)
    _, weights, _, status = det.liveness_tensors(fr, boxes, found)
    assert status.tolist() == [0, 0, 0, 0, -2, -3] and (weights[3] < 1.0).all()
    rng = np.random.default_rng(70)
    logits = [rng.uniform(0.0, 1.0, size=(6, 2)).astype(np.float32) for _ in range(4)]
    want = R.decide(logits, weights)
    score, live = det.liveness_decide(logits, weights)
    assert np.array_equal(score, want[0], equal_nan=True) and np.array_equal(live, want[1])
    assert np.isnan(score[4:]).all() and not live[4:].any() and not np.isnan(score[:4]).any()
    # the reference as written: only the first model's output and weight are used -- the k = 1 call
    for i in range(4):
        aw = R.decide_as_written([x[i:i + 1] for x in logits], [weights[i, 0]])
        s1, l1 = det.liveness_decide([logits[0][i:i + 1]], weights[i:i + 1, :1])
        assert s1[0] == aw[0][0] and l1[0] == aw[1][0]


def test_decide_device(det):
    import torch
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(80)
    n = 70                                        # more than one 64-thread workgroup
    for k in (1, 4, 9):
        logits = [rng.uniform(-0.5, 1.5, size=(n, 2)).astype(np.float32) for _ in range(k)]
        w = rng.uniform(0.05, 1.0, size=(n, k)).astype(np.float32)
        want = R.decide(logits, w)
        dl = [torch.from_numpy(x).to(dev) for x in logits]
        dw = torch.from_numpy(w).to(dev)
        score, live = torch.zeros(n, device=dev), torch.full((n,), 5, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        out = dw if k == 1 else score             # k = 1: score may be the weights array itself
        det.liveness_decide_device([x.data_ptr() for x in dl], n, 2, dw.data_ptr(), out.data_ptr(), live.data_ptr())
        det.sync()
        torch.cuda.synchronize()
        assert np.array_equal(out.cpu().numpy().reshape(-1), want[0]) and np.array_equal(live.cpu().numpy(), want[1]), k
