"""The glue around the quality and the ID model on the device (include/rfd.h: rfd_face_tensors, rfd_align_faces_tensors,
rfd_detect_select_align_tensors_batch, rfd_detect_faces_device, rfd_quality_decide, rfd_normalize_embeddings) against numpy.

Model inputs (face_quality.rs:43-44,56-101, face_extraction.rs:38-77): oracle.resize_linear of the crop, [..., ::-1],
(x.astype(f32) - mean32) * scale32, transpose -- every step one IEEE f32 operation, so the bar is np.array_equal.
Parity status: byte-exact against the oracle's restatement of cv::resize; unpinned against a running OpenCV, like alignment."""
import ctypes as C
import math

import numpy as np
import pytest

import helpers

pytestmark = pytest.mark.gpu

SIZES = [(112, 112), (56, 56), (96, 80), (224, 224)]   # (w, h): copy, the exact-2x mean, generic down, generic up


def _expect(oracle, crops, cfg):
    mean, scale = np.array(list(cfg.mean), np.float32), np.array(list(cfg.scale), np.float32)
    out = [((oracle.resize_linear(c, cfg.out_h, cfg.out_w)[..., ::-1].astype(np.float32) - mean) * scale).transpose(2, 0, 1) for c in crops]
    return np.stack(out)


def _presets(rfd):
    return [rfd.face_tensor_config_quality(), rfd.face_tensor_config_extraction()]


def _sized(rfd, preset, size):
    return rfd.face_tensor_config(size, list(preset.mean), list(preset.scale))


@pytest.fixture(scope="module")
def det(rfd):
    d = rfd.RetinaFaceDetection(max_batch_size=12, max_det=512)
    d.init_synthetic_weights(1234)
    yield d
    d.close()


# ---- stage level -------------------------------------------------------------------------------------------------------
def test_stage_level_every_size_and_both_presets(rfd, oracle, det):
    crops = np.random.default_rng(21).integers(0, 256, size=(3, 112, 112, 3), dtype=np.uint8)
    for pi, preset in enumerate(_presets(rfd)):
        cfgs = [_sized(rfd, preset, s) for s in SIZES]
        want = [_expect(oracle, crops, c) for c in cfgs]
        got = det.face_tensors(crops, cfgs)                       # k = 4 in one call
        for s, g, w in zip(SIZES, got, want):
            assert g.shape == (3, 3, s[1], s[0]) and np.array_equal(g, w), (pi, s)
        for c, w, s in zip(cfgs, want, SIZES):                    # k = 1
            assert np.array_equal(det.face_tensors(crops, [c])[0], w), (pi, s)
    mixed = [_sized(rfd, _presets(rfd)[j % 2], s) for j, s in enumerate(SIZES)]   # both presets' constants in one call
    for g, c in zip(det.face_tensors(crops, mixed), mixed):
        assert np.array_equal(g, _expect(oracle, crops, c))


def test_stage_level_edge_clamps(rfd, oracle, det):
    crops = np.random.default_rng(22).integers(0, 256, size=(2, 5, 7, 3), dtype=np.uint8)    # 7 wide, 5 high
    for preset in _presets(rfd):
        cfg = _sized(rfd, preset, (3, 2))
        assert np.array_equal(det.face_tensors(crops, [cfg])[0], _expect(oracle, crops, cfg))


def test_capacity_and_arguments(rfd, det):
    crops = np.zeros((2, 112, 112, 3), np.uint8)
    q = rfd.face_tensor_config_quality()
    with pytest.raises(rfd.RfdError) as e:
        det.face_tensors(crops, [q] * (rfd.MAX_FACE_TENSORS + 1))
    assert e.value.status == rfd.RFD_ERR_CAPACITY and "RFD_MAX_FACE_TENSORS" in str(e.value)
    with pytest.raises(rfd.RfdError) as e:
        det.face_tensors(crops, [rfd.face_tensor_config((0, 112), list(q.mean), list(q.scale))])
    assert e.value.status == rfd.RFD_ERR_INVALID_ARG and "size" in str(e.value)
    with pytest.raises(rfd.RfdError) as e:
        det.face_tensors(np.zeros((13, 8, 8, 3), np.uint8), [q])
    assert e.value.status == rfd.RFD_ERR_CAPACITY and "max_batch_size" in str(e.value)
    L = rfd.load_library()
    arr = (rfd.rfd_face_tensor_config * 2)(q, q)
    good = np.zeros((2, 3, 112, 112), np.float32)
    ptrs = (C.c_void_p * 2)(good.ctypes.data, None)
    assert L.rfd_face_tensors(det._ctx, crops.ctypes.data, 2, 112, 112, C.addressof(arr), 2, ptrs) == rfd.RFD_ERR_INVALID_ARG
    assert b"null" in L.rfd_last_error()
    frames = [helpers.make_image(5, 240, 320)]
    with pytest.raises(rfd.RfdError) as e:
        det.detect_select_align_tensors(frames, [q] * 5)
    assert e.value.status == rfd.RFD_ERR_CAPACITY


# ---- alignment + tensors -----------------------------------------------------------------------------------------------
def test_stage_level_alignment_with_tensors_every_branch(rfd, oracle, det):
    """Every alignment status through rfd_align_faces_tensors: the crop + resize fallback (status 1) does not occur with
    detections fed in by the network (its key points are never coincident), so that branch -- and the -1 / -3 error branches --
    are covered here, on caller-supplied selections, through the same kernels the fused entries launch."""
    f = helpers.make_image(9, 400, 480, n_blobs=5)
    same = np.tile(np.array([[100.0, 100.0]], np.float32), (5, 1))
    kps, box = helpers.make_face_kps(4, 400, 480)
    cases = [(np.array([60, 50, 200, 150, 0.9], np.float32), same), (np.array([60, 50, 470, 150, 0.9], np.float32), same),
             (box, None), (None, None), (box, kps), (np.array([206, 100, 310, 190, 0.9], np.float32), same)]
    frames = [f] * len(cases)
    want_crops, want_status = det.align_faces(frames, cases)
    assert want_status.tolist() == [1, -3, -1, -2, 0, 1]
    q, e = _presets(rfd)
    for cfgs in ([q, e], [q, _sized(rfd, e, (56, 56)), _sized(rfd, q, (96, 80)), e]):
        for want_c in (True, False):
            crops, status, tensors = det.align_faces_tensors(frames, cases, cfgs, want_crops=want_c)
            assert status.tolist() == want_status.tolist()
            assert crops is None or np.array_equal(crops, want_crops)
            for c, t in zip(cfgs, tensors):
                w = _expect(oracle, want_crops, c)
                w[want_status < 0] = 0.0
                assert np.array_equal(t, w), (c.out_w, c.out_h, want_c)
                assert not t[want_status < 0].any() and t[want_status >= 0].any()


@pytest.fixture(scope="module")
def calibrated(rfd, det):
    """Frames whose detections come from the network: a 240x320 one, a strided 1080x1920 one (a view of a wider array) and one
    without any detection, hence without a selected face.  Random weights score arbitrarily, so -- the calibration idiom of
    smoke() -- the threshold is read off the head tensors: just above the best foreground score of the quietest candidate
    for the empty frame, which must lie below the best score of a small and of a large frame."""
    small = [helpers.make_image(400 + i, 240, 320, n_blobs=5) for i in range(3)]
    large = [helpers.make_image(410 + i, 1080, 2000, n_blobs=5)[:, 40:1960] for i in range(3)]
    rng = np.random.default_rng(7)
    quiet = [np.zeros((240, 320, 3), np.uint8), np.full((240, 320, 3), 128, np.uint8), np.full((300, 200, 3), 255, np.uint8),
             np.full((240, 320, 3), 64, np.uint8), np.full((240, 320, 3), 192, np.uint8),
             rng.integers(100, 104, size=(240, 320, 3), dtype=np.uint8)]
    allf = small + large + quiet
    assert large[0].strides[0] == 6000 and large[0].shape == (1080, 1920, 3)
    _, tn, _ = det.preprocess(allf)
    heads = det.forward(tn)
    best = np.concatenate([heads[3 * l][:, 2:4].reshape(len(allf), -1) for l in range(3)], 1).max(1)
    print("best foreground score per frame:", best.tolist())
    a, b, c = int(np.argmax(best[0:3])), 3 + int(np.argmax(best[3:6])), 6 + int(np.argmin(best[6:]))
    lo, hi = float(best[c]), float(min(best[a], best[b]))
    assert lo < hi, "no calibration separates the empty frame: %s" % best.tolist()
    thr = lo + 0.25 * (hi - lo)   # well clear of both: a pass of another batch size may round a score differently
    det.set_thresholds(thr, 0.45)
    frames = [allf[a], allf[b], allf[c]]
    sel, crops, status = det.detect_select_align(frames, is_enroll=True)
    print("status of the calibrated frames:", status.tolist())
    assert status[0] >= 0 and status[1] >= 0 and status[2] == -2 and sel[2] == (None, None)
    yield frames, sel, crops, status
    det.set_thresholds(0.7, 0.45)


def _same_sel(a, b):
    return all((x is None and y is None) or (x is not None and y is not None and np.array_equal(x, y))
               for p, q in zip(a, b) for x, y in zip(p, q))


def test_fused_alignment_with_tensors(rfd, oracle, det, calibrated):
    frames, sel, crops, status = calibrated
    q, e = _presets(rfd)
    for cfgs in ([q, e], [q, _sized(rfd, e, (56, 56)), _sized(rfd, q, (96, 80))], []):
        ref = None
        for want_c in (True, False):
            s2, c2, st2, tensors = det.detect_select_align_tensors(frames, cfgs, is_enroll=True, want_crops=want_c)
            assert _same_sel(s2, sel) and st2.tolist() == status.tolist()
            assert c2 is None or np.array_equal(c2, crops)
            for c, t in zip(cfgs, tensors):
                w = _expect(oracle, crops, c)
                w[status < 0] = 0.0
                assert np.array_equal(t, w), (c.out_w, c.out_h, want_c)
                assert not t[2].any() and t[0].any() and t[1].any()
            if ref is not None:    # out_crops = NULL gives the same tensors
                assert all(np.array_equal(x, y) for x, y in zip(ref, tensors))
            ref = tensors
    assert not crops[2].any()


@pytest.mark.parametrize("enroll", [True, False])
def test_device_resident(rfd, oracle, det, calibrated, enroll):
    """rfd_detect_faces_device, async = 1 then rfd_sync, on the two frames held in device memory: every output equals the host
    entry's.  Two calls are enqueued back to back with the frames in opposite order (different frame sizes per slot), so the
    second call's frame-size array is written while the first call's copy of its own may still be pending."""
    import torch
    frames = [np.ascontiguousarray(f) for f in calibrated[0][:2]]
    q, e = _presets(rfd)
    cfgs = [q, e, _sized(rfd, e, (56, 56))]
    dev = torch.device("cuda", 0)
    bufs = [torch.from_numpy(f).to(dev) for f in frames]
    orders = [[0, 1], [1, 0]]
    want = [det.detect_select_align_tensors([frames[i] for i in o], cfgs, is_enroll=enroll) for o in orders]
    outs = []
    for o in orders:
        z = dict(box=torch.zeros(2, 5, device=dev), kps=torch.zeros(2, 10, device=dev), found=torch.zeros(2, dtype=torch.int32, device=dev),
                 crops=torch.zeros(2, 112, 112, 3, dtype=torch.uint8, device=dev), status=torch.zeros(2, dtype=torch.int32, device=dev),
                 tensors=[torch.zeros(2, 3, c.out_h, c.out_w, device=dev) for c in cfgs])
        outs.append(z)
    torch.cuda.synchronize()
    for o, z in zip(orders, outs):
        det.detect_faces_device([bufs[i].data_ptr() for i in o], [frames[i].shape[:2] for i in o], cfgs, z["box"].data_ptr(),
                                z["kps"].data_ptr(), z["found"].data_ptr(), z["crops"].data_ptr(), z["status"].data_ptr(),
                                [t.data_ptr() for t in z["tensors"]], is_enroll=enroll, async_=True)
    det.sync()
    torch.cuda.synchronize()
    for o, z, (sel, crops, status, tensors) in zip(orders, outs, want):
        found = z["found"].cpu().numpy()
        got_sel = rfd.RetinaFaceDetection._sel_out(z["box"].cpu().numpy(), z["kps"].cpu().numpy(), found)
        assert _same_sel(got_sel, sel), o
        assert np.array_equal(z["status"].cpu().numpy(), status) and np.array_equal(z["crops"].cpu().numpy(), crops), o
        for t, w in zip(z["tensors"], tensors):
            assert np.array_equal(t.cpu().numpy(), w), o
    if enroll:
        assert (want[0][2] >= 0).all()
    # crops = NULL, synchronous form
    z = outs[0]
    for t in z["tensors"]:
        t.zero_()
    torch.cuda.synchronize()
    det.detect_faces_device([bufs[i].data_ptr() for i in orders[0]], [frames[i].shape[:2] for i in orders[0]], cfgs, z["box"].data_ptr(),
                            z["kps"].data_ptr(), z["found"].data_ptr(), None, z["status"].data_ptr(),
                            [t.data_ptr() for t in z["tensors"]], is_enroll=enroll, async_=False)
    for t, w in zip(z["tensors"], want[0][3]):
        assert np.array_equal(t.cpu().numpy(), w)


# ---- after the models --------------------------------------------------------------------------------------------------
def _decide(row, threshold):
    """face_quality.rs:159-168: max_by keeps the last of equal maxima; class 1 below the threshold falls back to class 0"""
    predict = 0
    for i in range(1, len(row)):
        if not row[predict] > row[i]:
            predict = i
    score = row[predict]
    if predict == 1 and score < threshold:
        predict = 0
        score = row[predict]
    return score, predict


def test_quality_decision_rule(rfd, det):
    thr = np.float32(0.5)
    rows = np.array([[0.1, 0.2, 0.9],      # plain argmax
                     [0.9, 0.2, 0.1],
                     [0.1, 0.4, 0.2],      # class 1 below the threshold -> class 0
                     [0.1, 0.5, 0.2],      # class 1 AT the threshold stays (`<` is strict)
                     [0.7, 0.7, 0.1],      # two-way tie: the last index wins
                     [0.2, 0.9, 0.9],
                     [0.3, 0.3, 0.1],      # tie won by class 1, then below the threshold
                     [-1.0, -1.0, -1.0]], np.float32)
    score, klass = det.quality_decide(rows, thr)
    want = [_decide(r, thr) for r in rows]
    assert klass.tolist() == [w[1] for w in want] == [2, 0, 0, 1, 1, 2, 0, 2]
    assert np.array_equal(score, np.array([w[0] for w in want], np.float32))
    one = np.array([[0.3], [-2.0], [0.9]], np.float32)                        # classes = 1
    score, klass = det.quality_decide(one, thr)
    assert klass.tolist() == [0, 0, 0] and np.array_equal(score, one[:, 0])
    bad = rows.copy()
    bad[5, 1] = np.nan
    with pytest.raises(rfd.RfdError) as e:
        det.quality_decide(bad, thr)
    assert e.value.status == rfd.RFD_ERR_INVALID_ARG and "frame 5" in str(e.value)


@pytest.mark.parametrize("dim", [1, 63, 64, 65, 512])
def test_embedding_normalisation(rfd, det, dim):
    """|got - exact| <= (ceil(log2 dim) + 4) * 2^-24 * |exact|: a wave-tree f32 sum of dim squares carries at most
    (ceil(log2 dim) + 2) * 2^-24 relative error, sqrtf and the division add half an ulp each (derived, not measured)."""
    emb = np.random.default_rng(30 + dim).normal(0, 1, size=(5, dim)).astype(np.float32)
    got = det.normalize_embeddings(emb)
    x = emb.astype(np.float64)
    exact = x / np.sqrt((x * x).sum(1, keepdims=True))
    bound = (math.ceil(math.log2(dim)) + 4) * 2.0 ** -24
    err = np.abs(got.astype(np.float64) - exact)
    print("dim %d: worst relative error %.3g (bound %.3g)" % (dim, float((err / np.abs(exact)).max()), bound))
    assert (err <= bound * np.abs(exact)).all()
    assert np.array_equal(det.normalize_embeddings(emb), got)       # deterministic
    emb[2] = 0.0
    z = det.normalize_embeddings(emb)
    assert np.isnan(z[2]).all() and np.array_equal(z[[0, 1, 3, 4]], got[[0, 1, 3, 4]])
