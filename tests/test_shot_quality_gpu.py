"""The shot quality on the device (include/rfd.h, "shot quality") against tests/shot_quality_ref.py, bit for bit: quality, parts
and status of every row below a frame's count, and the fill (0xA5) in every byte at or past it.  There is no tolerance: both sides
are the same integer and f32 / f64 operations.  The constructed cases of tests/shot_quality_cases.py are held to their written
values as well."""
import ctypes as C

import numpy as np
import pytest

import helpers
import shot_quality_cases as SC
import shot_quality_ref as SR
import tracker_ref as TR

pytestmark = pytest.mark.gpu

MAX_DET, MAX_BATCH = 1024, 32
FILL = 0xA5
F = np.float32


@pytest.fixture(scope="module")
def det(rfd):
    d = rfd.RetinaFaceDetection(image_size=(128, 128), max_batch_size=MAX_BATCH, max_det=MAX_DET)
    yield d
    d.close()


def _filled(shape, dt):
    return np.frombuffer(bytes([FILL]) * (int(np.prod(shape)) * np.dtype(dt).itemsize), dt).reshape(shape).copy()


def _outs(n):
    return _filled((n, MAX_DET), F), _filled((n, MAX_DET, 8), F), _filled((n, MAX_DET), np.int32)


def _slabs(rows):
    """rows: per frame a list of (box [5], lmk [10]) -> boxes, lmk, count"""
    n = len(rows)
    boxes, lmk, count = np.zeros((n, MAX_DET, 5), F), np.zeros((n, MAX_DET, 10), F), np.zeros(n, np.int32)
    for b, rr in enumerate(rows):
        count[b] = len(rr)
        for i, (bx, l) in enumerate(rr):
            boxes[b, i], lmk[b, i] = bx, l
    return boxes, lmk, count


def _same(got, want, what):
    for name, g, w in zip(("quality", "parts", "status"), got, want):
        assert g.tobytes() == w.tobytes(), "%s: %s differs at %s" % (what, name, np.argwhere(g.view(np.uint32) != w.view(np.uint32))[:4].tolist())


def _want(frames, boxes, lmk, count, cfg):
    return SR.run(frames, boxes, lmk, count, cfg, *_outs(len(frames)))


def _cfg(rfd, fields):
    return rfd.shot_quality_config(**fields) if fields else None


class Device:
    """frames and slabs in HBM, the frames at any stride and at any byte offset in exactly sized buffers"""

    def __init__(self, frames, boxes, lmk, count, strides=None, offsets=None):
        import torch
        self.torch, self.dev = torch, torch.device("cuda", 0)
        self.keep, self.desc = [], []
        for i, f in enumerate(frames):
            h, w = f.shape[:2]
            stride = w * 3 if strides is None else strides[i]
            off = 0 if offsets is None else offsets[i]
            host = np.full(off + (h - 1) * stride + w * 3, 0xEE, np.uint8)
            np.lib.stride_tricks.as_strided(host[off:], (h, w * 3), (stride, 1))[:] = f.reshape(h, w * 3)
            t = torch.from_numpy(host).to(self.dev)
            self.keep.append(t)
            self.desc.append((t.data_ptr() + off, h, w, stride))
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(self.dev)
        self.boxes, self.lmk, self.count = up(boxes), up(lmk), up(count)
        q, p, s = _outs(len(frames))
        self.q, self.p, self.s = up(q), up(p), up(s)

    def dets(self):
        return self.boxes.data_ptr(), self.lmk.data_ptr(), self.count.data_ptr()

    def outs(self):
        return self.q.data_ptr(), self.p.data_ptr(), self.s.data_ptr()

    def run(self, det, cfg, async_=False):
        det.shot_quality(self.desc, self.dets(), cfg=cfg, device=True, out=self.outs(), async_=async_)
        if async_:
            det.sync()
        self.torch.cuda.synchronize()
        return self.q.cpu().numpy(), self.p.cpu().numpy(), self.s.cpu().numpy()


def test_constructed_cases_on_the_host_and_the_device_form(rfd, det):
    """every case of tests/shot_quality_cases.py, grouped by config into calls of up to 32 frames of different sizes, one row
    each: both forms equal the restatement bit for bit and give every written value"""
    groups = {}
    for name in sorted(SC.CASES):
        groups.setdefault(tuple(sorted(SC.CASES[name]["cfg"].items())), []).append(name)
    seen = 0
    for fields, names in sorted(groups.items()):
        for at in range(0, len(names), MAX_BATCH):
            part = names[at:at + MAX_BATCH]
            frames = [SC.CASES[n]["frame"] for n in part]
            boxes, lmk, count = _slabs([[(SC.CASES[n]["box"], SC.CASES[n]["lmk"])] for n in part])
            want = _want(frames, boxes, lmk, count, SR.config(**dict(fields)))
            host = det.shot_quality(frames, (boxes, lmk, count), cfg=_cfg(rfd, dict(fields)), out=_outs(len(part)))
            _same(host, want, "host form %s" % (part,))
            _same(Device(frames, boxes, lmk, count).run(det, _cfg(rfd, dict(fields))), want, "device form %s" % (part,))
            for b, n in enumerate(part):
                SC.check(n, dict(q=host[0][b, 0], parts=host[1][b, 0], status=int(host[2][b, 0])))
                seen += 1
    assert seen == len(SC.CASES)


def _random_rows(rng, h, w, k):
    """k boxes of a frame: sides from below 32 up to the frame and beyond it, corners at fractions, some outside; landmarks
    around the box, now and then a NaN, an infinity or coinciding eyes"""
    rows = []
    for _ in range(k):
        bw, bh = rng.uniform(25, w * 1.2), rng.uniform(25, h * 1.2)
        x1, y1 = rng.uniform(-20, max(w - 30, 1)), rng.uniform(-20, max(h - 30, 1))
        box = [x1, y1, x1 + bw, y1 + bh, rng.choice([0.5, 0.75, 0.96875])]
        l = (np.asarray(SC.STANDARD).reshape(5, 2) / 112.0 * [bw, bh] + [x1, y1] + rng.normal(0, bw * 0.05, size=(5, 2))).reshape(10)
        kind = rng.integers(0, 12)
        if kind == 0:
            l[rng.integers(0, 10)] = np.nan
        elif kind == 1:
            l[rng.integers(0, 10)] = np.inf * rng.choice([-1, 1])
        elif kind == 2:
            l[2] = l[0]
        rows.append((box, l))
    return rows


SIZES = [(40, 40), (41, 47), (64, 33), (33, 64), (150, 200), (97, 131), (128, 128), (45, 199)]      # (h, w), up to 200 x 150


@pytest.mark.parametrize("n", [1, 32])
def test_seeded_frames_strides_and_offsets(rfd, det, n):
    """n frames of different sizes in one call, rows at odd strides (w * 3 + 0 .. 7) and data pointers at byte offsets 0 .. 3,
    seeded noise with blobs, up to 12 seeded boxes per frame (one frame empty); default config and one with every field moved"""
    rng = np.random.default_rng(1000 + n)
    frames, rows, strides, offsets = [], [], [], []
    for b in range(n):
        h, w = SIZES[(b + n) % len(SIZES)]
        frames.append(helpers.make_image(200 + b, h, w))
        rows.append(_random_rows(rng, h, w, 0 if b == 5 else int(rng.integers(1, 13))))
        strides.append(w * 3 + (b + n) % 8)
        offsets.append((b + n // 32) % 4)
    boxes, lmk, count = _slabs(rows)
    moved = dict(dark=60, bright=200, pitch0=0.4, w_yaw=0.5, w_roll=1.5, w_pitch=1.0, sharp_ref=2000.0, size_ref=90.0, times_score=1)
    measured = 0
    for fields in ({}, moved):
        want = _want(frames, boxes, lmk, count, SR.config(**fields))
        dev = Device(frames, boxes, lmk, count, strides, offsets)
        _same(dev.run(det, _cfg(rfd, fields), async_=bool(fields)), want, "device form, %d frames" % n)
        # the host form of the same call, frames as strided views
        views = []
        for f, st in zip(frames, strides):
            h, w = f.shape[:2]
            buf = np.zeros(h * st, np.uint8)
            v = np.lib.stride_tricks.as_strided(buf, (h, w, 3), (st, 3, 1))
            v[:] = f
            views.append(v)
        _same(det.shot_quality(views, (boxes, lmk, count), cfg=_cfg(rfd, fields), out=_outs(n)), want, "host form, %d frames" % n)
        measured += int((want[2][:, :12] == 0).sum())
        q = want[0][want[2] == 0]
        assert n == 1 or ((q > 0) & (q < 1)).sum() > 20                 # the product is alive, not all zeros
    assert measured >= (2 if n == 1 else 100)


def test_whole_frame_box_of_640_x_480(rfd, det):
    """one workgroup reads 900 KB: 64 lanes per source row, 160 groups of four pixels per row, cells of 20 x 15 pixels"""
    frame = helpers.make_image(77, 480, 640)
    l = (np.asarray(SC.STANDARD) * (640 / 112.0)).tolist()
    boxes, lmk, count = _slabs([[([0, 0, 639, 479, 0.9], l), ([-5, -5, 700, 500, 0.9], l), ([1, 1, 638, 478, 0.9], l), ([100.5, 50, 611, 300, 0.9], l)]])
    want = _want([frame], boxes, lmk, count, SR.config())
    assert want[1][0, 0, 7] == 480 and want[1][0, 0].tobytes() == want[1][0, 1].tobytes() and want[1][0, 0, 0] != want[1][0, 2, 0]
    _same(Device([frame], boxes, lmk, count, [640 * 3 + 5], [3]).run(det, None), want, "640 x 480")


def test_counts_and_the_row_walk(rfd, det):
    """counts 0, negative and above max_det (clamped), and 1024 rows of 32 .. 40 pixel boxes in one frame, which the eight
    workgroups of a frame walk 128 rows each; every row past a count keeps the fill"""
    rng = np.random.default_rng(9)
    frames = [helpers.make_image(300 + b, 150, 200) for b in range(4)]
    rows = []
    for b in range(4):
        rr = []
        for i in range(MAX_DET):
            w, h = 32 + (i % 9), 32 + ((i // 9) % 9)
            x, y = (i * 7) % (200 - w), (i * 13) % (150 - h)
            bx = [x + 0.25, y + 0.5, x + w - 1 + 0.5, y + h - 1 + 0.25, 0.75]
            l = (np.asarray(SC.STANDARD).reshape(5, 2) / 112.0 * [w, h] + [x, y] + rng.normal(0, 1.0, size=(5, 2))).reshape(10)
            rr.append((bx, l))
        rows.append(rr)
    boxes, lmk, count = _slabs(rows)
    count[:] = [0, -7, MAX_DET + 1, MAX_DET]
    want = _want(frames, boxes, lmk, count, SR.config())
    fill32 = _filled((1,), np.int32)[0]
    assert (want[2][:2] == fill32).all() and (want[2][2:] == 0).all()                   # two frames untouched, two full and measured
    assert {int(s) for s in want[1][2, :, 7]} == set(range(32, 41))
    _same(Device(frames, boxes, lmk, count).run(det, None, async_=True), want, "device form")
    _same(det.shot_quality(frames, (boxes, lmk, count), out=_outs(4)), want, "host form")
    # a count between: rows 0 .. 136 of frame 3 alone, so the workgroups stop at different rows
    count[:] = [0, 0, 0, 137]
    want = _want(frames, boxes, lmk, count, SR.config())
    _same(Device(frames, boxes, lmk, count).run(det, None), want, "137 rows")


def test_parts_and_status_are_optional(rfd, det):
    frame = SC.BOARD
    boxes, lmk, count = _slabs([[(SC.whole(frame), SC.QUARTER_ROLL)]])
    want = _want([frame], boxes, lmk, count, SR.config(pitch0=0.5))
    d = Device([frame], boxes, lmk, count)
    det.shot_quality(d.desc, d.dets(), cfg=rfd.shot_quality_config(pitch0=0.5), device=True, out=(d.q.data_ptr(), None, None))
    assert d.q.cpu().numpy().tobytes() == want[0].tobytes() and want[0][0, 0] == F(0.75)
    assert (d.p.cpu().numpy().view(np.uint8) == FILL).all() and (d.s.cpu().numpy().view(np.uint8) == FILL).all()
    q, _, _ = det.shot_quality([frame], (boxes, lmk, count), cfg=rfd.shot_quality_config(pitch0=0.5), out=(_outs(1)[0], None, None))
    assert q.tobytes() == want[0].tobytes()


def test_argument_errors_on_the_device(rfd, det):
    L = rfd.load_library()
    frame = SC.BOARD
    boxes, lmk, count = _slabs([[(SC.whole(frame), SC.QUARTER_ROLL)]])
    d = Device([frame] * 2, np.repeat(boxes, 2, 0), np.repeat(lmk, 2, 0), np.repeat(count, 2, 0))
    dets = rfd.rfd_dets(*d.dets(), None)
    q, p, s = d.outs()

    def refused(status, text, n=2, imgs=None):
        arr = (rfd.rfd_image * max(n, 2))()
        for i in range(2):
            arr[i].data, arr[i].height, arr[i].width, arr[i].stride = d.desc[i]
        for i, im in (imgs or {}).items():
            arr[i].data, arr[i].height, arr[i].width, arr[i].stride = im
        host = np.zeros(16, F)
        hd = rfd.rfd_dets(host.ctypes.data, host.ctypes.data, host.ctypes.data, None)
        for call in (lambda: L.rfd_shot_quality_device(det._ctx, arr, n, C.byref(dets), None, q, p, s, 1),
                     lambda: L.rfd_shot_quality(det._ctx, arr, n, C.byref(hd), None, host.ctypes.data, None, None)):
            assert call() == status
            assert text in L.rfd_last_error().decode(), L.rfd_last_error()
    ptr, h, w, st = d.desc[1]
    refused(rfd.RFD_ERR_CAPACITY, "max_batch_size", n=MAX_BATCH + 1)
    refused(rfd.RFD_ERR_INVALID_ARG, "frame 1: data", imgs={1: (None, h, w, st)})
    refused(rfd.RFD_ERR_INVALID_ARG, "frame 1: non-positive size", imgs={1: (ptr, 0, w, st)})
    refused(rfd.RFD_ERR_INVALID_ARG, "frame 0: non-positive size", imgs={0: (ptr, h, -1, st)})
    refused(rfd.RFD_ERR_INVALID_ARG, "frame 1: stride", imgs={1: (ptr, h, w, w * 3 - 1)})
    refused(rfd.RFD_ERR_INVALID_ARG, "frame 1: a side exceeds 32768", imgs={1: (ptr, 32769, w, st)})
    assert L.rfd_shot_quality_device(det._ctx, None, 0, None, None, None, None, None, 1) == rfd.RFD_OK       # n = 0 is a no-op
    assert L.rfd_shot_quality(det._ctx, None, 0, None, None, None, None, None) == rfd.RFD_OK
    det.sync()
    for t in (d.q, d.p, d.s):
        assert (t.cpu().numpy().view(np.uint8) == FILL).all()                                                  # nothing was enqueued


def test_detect_quality_track_in_one_stream_order(rfd, det):
    """Two 300 x 200 frames, synthetic weights, async = 1 throughout: rfd_detect_batch_device -> rfd_shot_quality_device ->
    rfd_tracker_update_device(quality = that array), one rfd_sync.  The qualities equal the restatement on the slabs the
    detection left, and the tracker's outputs equal the tracker restatement fed those restated qualities."""
    import torch
    dev = torch.device("cuda", 0)
    det.init_synthetic_weights(1234)
    det.set_thresholds(0.0, 1.0)              # every anchor is a candidate and none is suppressed: the synthetic network has no say
    frames = [helpers.make_image(31, 200, 300), helpers.make_image(32, 200, 300)]
    bufs = [torch.from_numpy(np.ascontiguousarray(f)).to(dev) for f in frames]
    fill32 = int(_filled((1,), np.int32)[0])
    t32 = lambda *shape: torch.full(shape, fill32, dtype=torch.int32, device=dev)
    n = 2
    d_boxes, d_lmk, d_count, d_total = t32(n, MAX_DET, 5), t32(n, MAX_DET, 10), t32(n), t32(n)
    d_q, d_parts, d_status = t32(n, MAX_DET), t32(n, MAX_DET, 8), t32(n, MAX_DET)
    z = dict(track=t32(n, MAX_DET), flags=t32(n, MAX_DET), stats=t32(n, 4), ended=t32(n, 64), due_boxes=t32(n, MAX_DET, 5),
             due_landmarks=t32(n, MAX_DET, 10), due_count=t32(n), due_total=t32(n), due_track=t32(n, MAX_DET))
    cfg = dict(streams=2, max_tracks=64, iou_min=0.3, max_missed=5, min_score=0.0, new_score=0.0, min_hits=1, improve=1.1)
    tracker = det.tracker(**cfg)
    out = rfd.rfd_track_out(z["track"].data_ptr(), z["flags"].data_ptr(), z["stats"].data_ptr(), z["ended"].data_ptr(),
                            rfd.rfd_dets(z["due_boxes"].data_ptr(), z["due_landmarks"].data_ptr(), z["due_count"].data_ptr(), z["due_total"].data_ptr()),
                            z["due_track"].data_ptr())
    ptrs, shapes = [b.data_ptr() for b in bufs], [f.shape[:2] for f in frames]
    torch.cuda.synchronize()
    calls = ([1, 0], [0, 1])                  # the second call shows each camera the other frame: its rows meet the first call's tracks
    for streams in calls:
        det.detect_device(ptrs, shapes, d_boxes.data_ptr(), d_lmk.data_ptr(), d_count.data_ptr(), d_total.data_ptr(), async_=True)
        det.shot_quality([(p, h, w) for p, (h, w) in zip(ptrs, shapes)], (d_boxes.data_ptr(), d_lmk.data_ptr(), d_count.data_ptr()), device=True,
                         out=(d_q.data_ptr(), d_parts.data_ptr(), d_status.data_ptr()), async_=True)
        tracker.update_device(streams, d_boxes.data_ptr(), d_lmk.data_ptr(), d_count.data_ptr(), out, quality_ptr=d_q.data_ptr(), async_=True)
    det.sync()
    torch.cuda.synchronize()
    host = lambda t, dt=np.int32: t.cpu().numpy().view(dt)
    boxes, lmk, count = host(d_boxes, F), host(d_lmk, F), host(d_count)
    assert count.min() > 64, count
    want = _want(frames, boxes, lmk, count, SR.config())
    _same((host(d_q, F), host(d_parts, F), host(d_status)), want, "quality behind the detection")
    measured = want[2] == 0
    assert measured.sum() > 10, measured.sum()
    ref = TR.TrackerRef(**cfg)
    w = TR.Out(n, MAX_DET, 64, fill=FILL)     # one set of arrays for both calls, as on the device: what a call leaves past its counts stays
    for streams in calls:
        ref.update(np.asarray(streams, np.int32), boxes, lmk.reshape(n, MAX_DET, 5, 2), count, want[0], w)
    for name in z:
        assert host(z[name], getattr(w, name).dtype).reshape(getattr(w, name).shape).tobytes() == getattr(w, name).tobytes(), name
    det.set_thresholds(0.7, 0.45)
    tracker.close()
