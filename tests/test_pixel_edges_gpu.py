"""The pixel path on the device (csrc/kernels_pre.hip: preprocess_kernel, align_setup_kernel, align_warp_kernel,
align_warp_tensor_kernel, face_tensor_kernel, liveness_tensor_kernel and the shared resize_linear_px / align_warp_px) at every
branch of the resize and of the warp, on constructed inputs.  Every comparison is of bytes.

Expected values are the closed forms of tests/pixel_cases.py where one exists and the CPU oracle elsewhere;
tests/test_pixel_cases_cpu.py holds the two against each other without a GPU, and asserts what this sweep relies on: the tie
counts of the two rounding families and at least 8 letterbox geometries of every class per network input."""
import collections
import functools

import numpy as np
import pytest

import helpers
import liveness_ref as R
import pixel_cases as pc

pytestmark = pytest.mark.gpu

BATCH = 16
BOX = np.array([0, 0, 10, 10, 0.9], np.float32)
ALIGN = dict(image_size=(pc.CROP_W, pc.CROP_H), standard_landmarks=pc.TEMPLATE)


@pytest.fixture(scope="module")
def det(rfd):
    d = rfd.RetinaFaceDetection(max_batch_size=BATCH, max_det=64)   # no call here runs the network
    yield d
    d.close()


def _raw(rfd, w, h):
    """mean 0, scale 1: the planes are the resized bytes"""
    return rfd.face_tensor_config((w, h), [0.0, 0.0, 0.0], [1.0, 1.0, 1.0])


def _planes(px):
    """[n, h, w, 3] u8 B, G, R -> [n, 3, h, w] f32 R, G, B"""
    return np.ascontiguousarray(px[..., ::-1].transpose(0, 3, 1, 2)).astype(np.float32)


def _resized(oracle, crop, dh, dw):
    h, w = crop.shape[:2]
    if pc.is_dyadic(h, dh) and pc.is_dyadic(w, dw):
        return pc.resize_exact(crop, dh, dw)
    return oracle.resize_linear(crop, dh, dw)


# ---- resize, through rfd_face_tensors ------------------------------------------------------------------------------------
@pytest.mark.parametrize("along_y", [False, True], ids=["x", "y"])
@pytest.mark.parametrize("ch", [3, 6])
def test_resize_sweep(rfd, oracle, det, ch, along_y):
    """crops 1 .. 17 wide and ch high to 1 .. 34 x 3 (and all of it transposed), 14 noise crops and the two 0 / 255 checkerboards
    per call, RFD_MAX_FACE_TENSORS sizes per call: every first-tap byte offset mod 8, both clamps, widths where the 8-byte load
    is never legal, the copy (ch = 3, equal widths), the 2x2 mean (ch = 6, half the width) and exactly one factor 2"""
    K = rfd.MAX_FACE_TENSORS
    outs = list(range(1, 35))
    outs += outs[:-len(outs) % K]
    seen = collections.Counter()
    for cw in range(1, 18):
        crops = np.stack([pc.noise(1000 * ch + 10 * cw + i, ch, cw) for i in range(BATCH - 2)] + [pc.checker(ch, cw), 255 - pc.checker(ch, cw)])
        if along_y:
            crops = np.ascontiguousarray(crops.transpose(0, 2, 1, 3))
        for k0 in range(0, len(outs), K):
            sizes = [(ow, 3)[::-1 if along_y else 1] for ow in outs[k0:k0 + K]]          # (w, h)
            got = det.face_tensors(crops, [_raw(rfd, w, h) for w, h in sizes])
            for (w, h), g in zip(sizes, got):
                want = np.stack([_resized(oracle, c, h, w) for c in crops])
                assert np.array_equal(g, _planes(want)), (crops.shape[1:3], (h, w))
                x2, y2 = crops.shape[2] == 2 * w, crops.shape[1] == 2 * h
                seen["copy" if crops.shape[1:3] == (h, w) else "both-2" if x2 and y2 else "mixed" if x2 or y2 else "other"] += 1
    print(dict(seen))
    assert seen["mixed"] >= 8 and seen["copy" if ch == 3 else "both-2"] >= 8


RESIZE = pc.resize_cases()


@pytest.mark.parametrize("case", RESIZE, ids=[c[0] for c in RESIZE])
def test_resize_closed_forms(rfd, det, case):
    """identity, 2x2 mean, constants, integer upscales of a step, one factor 2, the two tie families (round half to even in
    2048 and 1366 columns or rows) and 4096 <-> 1, against bytes written down from the geometry alone"""
    name, src, (dh, dw), want = case
    got = det.face_tensors(np.stack([src, src]), [_raw(rfd, dw, dh)])[0]
    assert np.array_equal(got, _planes(np.stack([want, want]))), name


@pytest.mark.parametrize("along_y", [False, True], ids=["x", "y"])
def test_resize_size_limits(rfd, oracle, det, along_y):
    """one row of 4096 and of 4095 pixels to 4095, 4096, 2048 and 1 and back: the largest sizes the entry accepts"""
    for n in (4096, 4095, 1):
        crops = np.stack([pc.noise(1200 + n + i, 1, n) for i in range(4)])
        sizes = [(4096, 1), (4095, 1), (2048, 1), (1, 1)]
        if along_y:
            crops, sizes = np.ascontiguousarray(crops.transpose(0, 2, 1, 3)), [s[::-1] for s in sizes]
        got = det.face_tensors(crops, [_raw(rfd, w, h) for w, h in sizes])
        for (w, h), g in zip(sizes, got):
            assert np.array_equal(g, _planes(np.stack([_resized(oracle, c, h, w) for c in crops]))), (n, w, h)


# ---- preprocess ----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _source(h, w):
    return pc.noise(7000 + 200 * h + w, h, w)


def _view(seed, h, w, offset, pad):
    """an h x w frame `offset` bytes into a buffer of its own, rows w * 3 + pad bytes apart; every byte of the buffer that is
    not a pixel of the frame is 0xA5, and the buffer ends with the frame's last pixel"""
    stride = w * 3 + pad
    buf = np.full(offset + (h - 1) * stride + w * 3, 0xA5, np.uint8)
    v = np.ndarray((h, w, 3), np.uint8, buf, offset=offset, strides=(stride, 3, 1))
    v[...] = pc.noise(seed, h, w)
    return v


def _check_preprocess(oracle, d, frames, net, seen=None):
    di, tn, sc = d.preprocess(frames)
    for i, f in enumerate(frames):
        odi, otn, osc = oracle.preprocess(np.ascontiguousarray(f), *net)
        tag = (net, f.shape[:2], i)
        assert sc[i] == osc, tag
        assert np.array_equal(di[i], odi), tag
        assert np.array_equal(tn[i], otn), tag
        if seen is not None:
            nw, nh, _ = oracle.geometry(f.shape[0], f.shape[1], *net)
            seen[pc.letterbox_class(f.shape[0], f.shape[1], nh, nw)] += 1


@pytest.mark.parametrize("net", pc.LETTERBOX_NETS, ids=["%dx%d" % n for n in pc.LETTERBOX_NETS])
def test_preprocess_sweep(rfd, oracle, net):
    """every source h x w of LETTERBOX_SIDES in full batches of mixed sizes (host frames are packed back to back on the device:
    every frame starts at another alignment): det_img, tensor and det_scale of the oracle; the network inputs 96 and 32 wide end
    inside a 64-wide tile of the kernel.  Every geometry that letterboxes to an empty image refuses the whole call and leaves
    the next call as it was.  Then one batch of views with padded rows, 0 .. 7 bytes into their poisoned buffers."""
    d = rfd.RetinaFaceDetection(image_size=net, max_batch_size=BATCH, max_det=16)
    try:
        good, empty = [], []
        for h in pc.LETTERBOX_SIDES:
            for w in pc.LETTERBOX_SIDES:
                nw, nh, _ = oracle.geometry(h, w, *net)
                (empty if nw <= 0 or nh <= 0 else good).append((h, w))
        order = np.random.default_rng(net[0] * 100 + net[1]).permutation(len(good))
        good = [good[i] for i in order]
        good += good[:-len(good) % BATCH]
        seen = collections.Counter()
        for k in range(0, len(good), BATCH):
            _check_preprocess(oracle, d, [_source(h, w) for h, w in good[k:k + BATCH]], net, seen)
        print(net, dict(seen), "empty:", len(empty))
        assert len(empty) >= 8 and all(seen[k] >= 8 for k in pc.LETTERBOX_CLASSES if k != "empty")
        probe = [_source(33, 64), _source(9, 7)]
        for h, w in empty:
            with pytest.raises(rfd.RfdError) as e:
                d.preprocess([probe[0], _source(h, w), probe[1]])
            assert e.value.status == rfd.RFD_ERR_INVALID_ARG, (h, w)
            _check_preprocess(oracle, d, probe, net)
        sizes = [(33, 64), (5, 7), (64, 33), (2, 33), (97, 129), (1, 1), (31, 63), (128, 192)]
        views = [_view(7700 + i, h, w, i, (1, 5, 2, 13, 7, 3, 8, 11)[i]) for i, (h, w) in enumerate(sizes)]
        assert all(v.ctypes.data - v.base.ctypes.data == i and v.strides[0] > v.shape[1] * 3 for i, v in enumerate(views))
        _check_preprocess(oracle, d, views + views[::-1], net)
        assert all((np.delete(v.base, _pixel_bytes(v)) == 0xA5).all() for v in views)
    finally:
        d.close()


def _pixel_bytes(v):
    off, stride = v.ctypes.data - v.base.ctypes.data, v.strides[0]
    return (off + np.arange(v.shape[0])[:, None] * stride + np.arange(v.shape[1] * 3)[None, :]).reshape(-1)


def test_network_input_is_the_canvas(rfd, oracle):
    """The NHWC4 bf16 tensor the network reads, after rfd_detect_batch: R, G, B, 0 of the oracle's canvas for every frame of the
    batch, zeros beside and below the paste.  Three frames per call, geometries of every class of the 96 x 64 letterbox."""
    net = (96, 64)
    d = rfd.RetinaFaceDetection(image_size=net, max_batch_size=BATCH, max_det=16)
    try:
        d.init_synthetic_weights(1234)
        g = rfd.Graph(rfd.BACKBONE_R50, *net)
        tid = next(i for i, t in enumerate(g.tensors) if t.is_input)
        desc = g.tensors[tid]
        assert (desc.channels, desc.height, desc.width, desc.is_f32) == (4, 64, 96, 0)
        by_class = collections.defaultdict(list)
        for h in pc.LETTERBOX_SIDES:
            for w in pc.LETTERBOX_SIDES:
                nw, nh, _ = oracle.geometry(h, w, *net)
                by_class[pc.letterbox_class(h, w, nh, nw)].append((h, w, nh, nw))
        rng = np.random.default_rng(96)
        picks = [[by_class[k][i] for i in rng.permutation(len(by_class[k]))[:3]] for k in pc.LETTERBOX_CLASSES if k != "empty"]
        flat = [p[j] for j in range(3) for p in picks]                  # 15 geometries, the classes interleaved
        for call in range(5):
            geo = flat[3 * call:3 * call + 3]
            frames = [_source(h, w) for h, w, _, _ in geo]
            d.call_batch(frames)
            got = d.debug_read(tid, len(frames), desc)
            assert got.shape == (len(frames), 64, 96, 4) and got.dtype == np.uint16
            for i, (f, (h, w, nh, nw)) in enumerate(zip(frames, geo)):
                canvas = oracle.preprocess(f, *net)[0]
                want = np.zeros((64, 96, 4), np.float32)
                want[..., :3] = canvas[..., ::-1]
                assert np.array_equal(got[i], helpers.f32_to_bf16_bits(want)), (call, h, w)
                assert got[i, :nh, :nw, :3].any() and not got[i, nh:].any() and not got[i, :, nw:].any() and not got[i, ..., 3].any()
    finally:
        d.close()


# ---- warp ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def warp_sets():
    frames = [pc.noise(950, 97, 131), pc.noise(951, 2160, 3840), pc.wide_frame()]
    return [(frames[0], pc.warp_cases(frames[0])), (frames[1], pc.warp_cases(frames[1])), (frames[2], pc.wide_cases(frames[2]))]


FRAMES = pytest.mark.parametrize("which", [0, 1, 2], ids=["97x131", "2160x3840", "64x33000"])
TENSOR_SIZES = [(pc.CROP_W, pc.CROP_H), (pc.CROP_W // 2, pc.CROP_H // 2), (7, 9), (2 * pc.CROP_W, pc.CROP_H)]   # fused; 2x2 mean; generic; dyadic


def _check_tensors(oracle, tensors, crops):
    for (w, h), t in zip(TENSOR_SIZES, tensors):
        want = np.stack([_resized(oracle, c, h, w) for c in crops])
        assert np.array_equal(t, _planes(want)), (w, h)


@FRAMES
def test_warp_align_faces(det, warp_sets, which):
    frame, cases = warp_sets[which]
    for k in range(0, len(cases), BATCH):
        part = cases[k:k + BATCH]
        crops, status = det.align_faces([frame] * len(part), [(BOX, c["kps"]) for c in part], **ALIGN)
        for c, crop, st in zip(part, crops, status):
            assert st == 0 and np.array_equal(crop, c["want"]), c["name"]


@FRAMES
def test_warp_align_faces_tensors(rfd, oracle, det, warp_sets, which):
    """the config of the crop's own size is written by the warp kernel itself, the others are resized from the crop"""
    frame, cases = warp_sets[which]
    cfgs = [_raw(rfd, w, h) for w, h in TENSOR_SIZES]
    for k in range(0, len(cases), BATCH):
        part = cases[k:k + BATCH]
        want = np.stack([c["want"] for c in part])
        for want_crops in ((True, False) if which != 1 else (k == 0,)):        # the large frame is staged once per face: one form per part
            crops, status, tensors = det.align_faces_tensors([frame] * len(part), [(BOX, c["kps"]) for c in part], cfgs, want_crops=want_crops, **ALIGN)
            assert not status.any() and (crops is None or np.array_equal(crops, want)), [c["name"] for c in part]
            _check_tensors(oracle, tensors, want)


@FRAMES
def test_warp_packed_list(rfd, oracle, det, warp_sets, which):
    """rfd_align_detections: the cases as the detections of two frames, several faces per frame"""
    frame, cases = warp_sets[which]
    half = (len(cases) + 1) // 2
    split = [cases[:half], cases[half:]]
    dets = [(np.tile(BOX, (len(s), 1)), np.stack([c["kps"] for c in s])) for s in split]
    cfgs = [_raw(rfd, w, h) for w, h in TENSOR_SIZES]
    lst = det.align_detections([frame, frame], dets, cfgs=cfgs, cap=len(cases) + 3, **ALIGN)
    assert int(lst.total[0]) == lst.valid == len(cases) and lst.first.tolist() == [0, half, len(cases)]
    assert lst.frame[:lst.valid].tolist() == [0] * half + [1] * (len(cases) - half)
    assert lst.row[:lst.valid].tolist() == list(range(half)) + list(range(len(cases) - half))
    want = np.stack([c["want"] for c in cases])
    assert not lst.status[:lst.valid].any()
    for c, crop in zip(cases, lst.crops):
        assert np.array_equal(crop, c["want"]), c["name"]
    _check_tensors(oracle, [t[:lst.valid] for t in lst.tensors], want)


# ---- exactly one scale factor 2 in the two ROI set-ups ------------------------------------------------------------------------
def test_alignment_fallback_with_one_factor_two(det, oracle):
    """coincident key points take the crop + resize branch on the ROI [x0, W) x [y0, H).  224 x 112 -> 112 x 112 has scale_x
    exactly 2 and scale_y 1: not the 2x2 mean, but the rounded mean of two neighbours in a row; 224 x 150 and 100 x 224 have one
    factor 2 and a generic one; 224 x 224 next to them is the 2x2 mean."""
    same = np.tile(np.array([[100.0, 100.0]], np.float32), (5, 1))
    b = np.array([62, 52, 100, 100, 0.9], np.float32)                  # x0 = 40, y0 = 30
    frames = [helpers.make_image(20 + i, rh + 30, rw + 40, n_blobs=3) for i, (rw, rh) in enumerate([(224, 112), (224, 150), (100, 224), (224, 224)])]
    crops, status = det.align_faces(frames, [(b, same)] * 4)
    assert status.tolist() == [1, 1, 1, 1]
    for i, f in enumerate(frames):
        want, st = oracle.face_alignment(f, b, same)
        assert st == 1 and np.array_equal(crops[i], want), i
    roi = frames[0][30:, 40:].astype(np.int32)
    assert np.array_equal(crops[0], (roi[:, 0::2] + roi[:, 1::2] + 1) >> 1)
    assert np.array_equal(crops[3], pc.mean_2x2(frames[3][30:, 40:]))
    assert not np.array_equal(crops[1], pc.mean_2x2(frames[1][30:, 40:])[:112])


def _box_with_roi(rw, rh, frame_w=400, frame_h=300):
    """a box whose scale-1.0 ROI is exactly rw x rh: a search over the box centre and height, on the reference alone"""
    for ymin in range(10, 40):
        for h in range(rh - 4, rh + 2):
            for cx4 in range(4 * 130, 4 * 260):
                box = (cx4 / 4.0 - 50, ymin, cx4 / 4.0 + 50, ymin + h)
                l, t, r, b, w, _ = R.new_box(frame_w, frame_h, R.scale_image_box(box), 1.0)
                if (r - l + 1, b - t + 1) == (rw, rh) and w == 1.0 and R.roi_ok(R.roi_rect(l, t, r, b), frame_w, frame_h):
                    return box
    return None


def test_liveness_with_one_factor_two(rfd, det, oracle):
    """a ROI of 240 x 256 into models of 120 x 100 (scale_x 2, scale_y 2.56), 100 x 128 (2.4, 2) and 120 x 128 (the 2x2 mean)"""
    wide = helpers.make_image(503, 300, 480, n_blobs=5)
    view = wide[:, 40:440]
    box = _box_with_roi(240, 256)
    assert box is not None
    sizes = [(120, 100), (100, 128), (120, 128)]
    want = R.batch([view], [box], [1], [1.0] * 3, sizes, oracle=oracle)
    l, t, r, b = want[2][0, 0]
    assert (r - l + 1, b - t + 1) == (240, 256) and want[3][0] == 0
    roi = view[t:b + 1, l:r + 1]
    assert np.array_equal(want[0][2][0], pc.mean_2x2(roi).transpose(2, 0, 1).astype(np.float32))
    tensors, weights, rois, status = det.liveness_tensors([view], np.array([box], np.float32), cfg=rfd.liveness_config([1.0] * 3, sizes))
    assert status.tolist() == [0] and np.array_equal(rois, want[2]) and np.array_equal(weights, want[1])
    for j, (g, w) in enumerate(zip(tensors, want[0])):
        assert np.array_equal(g, w), sizes[j]
