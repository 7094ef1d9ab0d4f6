"""The redaction on the device (include/rfd.h, "redaction") against tests/redact_ref.py, byte for byte over WHOLE ALLOCATIONS: the
frames lie in exactly sized buffers filled with a pattern, at odd strides and byte offsets, and every byte of every buffer is
compared -- the painted pixels, the pixels left alone, the stride padding and the bytes in front of the data pointer; in place
the source buffer is the output, out of place the source buffer must come back as it went in.  There is no tolerance: both
sides are the same integer and f32 operations.  The constructed cases of tests/redact_cases.py are held to their written frames."""
import ctypes as C

import numpy as np
import pytest

import helpers
import jpeg_encode_ref as JR
import redact_cases as RC
import redact_ref as RR

pytestmark = pytest.mark.gpu

MAX_DET, MAX_BATCH = 1024, 32
PAD_SRC, PAD_DST, FILL = 0xEE, 0xD7, 0xA5
F = np.float32


@pytest.fixture(scope="module")
def det(rfd):
    d = rfd.RetinaFaceDetection(image_size=(128, 128), max_batch_size=MAX_BATCH, max_det=MAX_DET)
    yield d
    d.close()


def _slabs(rows):
    """rows: per frame a list of box rows -> boxes [n, MAX_DET, 5], count [n]"""
    boxes, count = np.zeros((len(rows), MAX_DET, 5), F), np.zeros(len(rows), np.int32)
    for b, rr in enumerate(rows):
        count[b] = len(rr)
        for i, bx in enumerate(rr):
            boxes[b, i, :len(bx)] = bx
    return boxes, count


def _embed(frame, stride, off, pad):
    """the exactly sized buffer of a frame at a byte offset and a stride, everything else the pattern"""
    h, w = frame.shape[:2]
    host = np.full(off + (h - 1) * stride + w * 3, pad, np.uint8)
    np.lib.stride_tricks.as_strided(host[off:], (h, w * 3), (stride, 1))[:] = frame.reshape(h, w * 3)
    return host


def _cfg(rfd, fields):
    return rfd.redact_config(**fields)


class Device:
    """frames, dst frames and slabs in HBM; run() gives back every buffer whole"""

    def __init__(self, frames, boxes, count, sel=None, strides=None, offsets=None, dst_strides=None, dst_offsets=None):
        import torch
        self.torch, self.dev, self.frames, self.n = torch, torch.device("cuda", 0), frames, len(frames)
        pick = lambda a, i, d: d if a is None else a[i]
        self.place = [(pick(strides, i, f.shape[1] * 3), pick(offsets, i, 0)) for i, f in enumerate(frames)]
        self.dplace = [(pick(dst_strides, i, f.shape[1] * 3), pick(dst_offsets, i, 0)) for i, f in enumerate(frames)]
        self.src_host = [_embed(f, st, off, PAD_SRC) for f, (st, off) in zip(frames, self.place)]
        self.dst_host = [_embed(np.full_like(f, PAD_DST), st, off, PAD_DST) for f, (st, off) in zip(frames, self.dplace)]
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(self.dev)
        self.boxes, self.count = up(boxes), up(count)
        self.sel = None if sel is None else up(sel.astype(np.uint32).view(np.int32))
        self.reset()

    def reset(self):
        up = lambda a: self.torch.from_numpy(a).to(self.dev)
        self.src, self.dst = [up(h) for h in self.src_host], [up(h) for h in self.dst_host]
        self.applied = up(np.full(MAX_BATCH + 1, FILL * 0x01010101, np.uint32).view(np.int32))
        self.torch.cuda.synchronize()                              # the context's stream is not ordered with torch's

    def desc(self, bufs, place):
        return [(t.data_ptr() + off, f.shape[0], f.shape[1], st) for t, f, (st, off) in zip(bufs, self.frames, place)]

    def run(self, det, cfg, in_place, async_=False, with_applied=True):
        self.reset()
        det.redact_faces(self.desc(self.src, self.place), (self.boxes.data_ptr(), self.count.data_ptr()),
                         sel=None if self.sel is None else self.sel.data_ptr(), cfg=cfg, device=True,
                         dst=None if in_place else self.desc(self.dst, self.dplace), applied=self.applied.data_ptr() if with_applied else None,
                         async_=async_)
        if async_:
            det.sync()
        return [t.cpu().numpy() for t in self.src], [t.cpu().numpy() for t in self.dst], self.applied.cpu().numpy()

    def check(self, got, want, want_applied, in_place, what):
        src, dst, applied = got
        for b in range(self.n):
            (st, off), (dst_st, dst_off) = self.place[b], self.dplace[b]
            exp_src = _embed(want[b], st, off, PAD_SRC) if in_place else self.src_host[b]
            exp_dst = self.dst_host[b] if in_place else _embed(want[b], dst_st, dst_off, PAD_DST)
            for name, g, e in (("source", src[b], exp_src), ("dst", dst[b], exp_dst)):
                assert g.tobytes() == e.tobytes(), "%s, %s: the %s buffer of frame %d (%s) differs at bytes %s" % (
                    what, "in place" if in_place else "out of place", name, b, self.frames[b].shape, np.flatnonzero(g != e)[:8].tolist())
        assert applied[:self.n].tolist() == list(want_applied), (what, applied[:self.n], want_applied)
        assert (applied[self.n:].view(np.uint8) == FILL).all(), what

    def both(self, det, cfg, want, want_applied, what, async_=False):
        for in_place in (True, False):
            self.check(self.run(det, cfg, in_place, async_=async_), want, want_applied, in_place, what)


def _host_forms(det, frames, boxes, count, sel, cfg, want, want_applied, what):
    """the host form, in place on strided views and out of place into strided views: the rows come back, the padding stays"""
    def views(fill=None):
        out, bufs = [], []
        for i, f in enumerate(frames):
            h, w = f.shape[:2]
            buf = np.full(h * (w * 3 + i % 5), 0x5C, np.uint8)
            v = np.lib.stride_tricks.as_strided(buf, (h, w, 3), (w * 3 + i % 5, 3, 1))
            v[:] = f if fill is None else fill
            out.append(v)
            bufs.append(buf)
        return out, bufs
    src, src_bufs = views()
    got, applied = det.redact_faces(src, (boxes, count), sel=sel, cfg=cfg)
    assert applied.tolist() == list(want_applied), what
    for b, (g, buf) in enumerate(zip(got, src_bufs)):
        h, w = frames[b].shape[:2]
        exp = np.full_like(buf, 0x5C)
        np.lib.stride_tricks.as_strided(exp, (h, w, 3), (w * 3 + b % 5, 3, 1))[:] = want[b]
        assert buf.tobytes() == exp.tobytes(), "%s: host form in place, frame %d" % (what, b)
    src, src_bufs = views()
    before = [b.copy() for b in src_bufs]
    dst, dst_bufs = views(fill=0x33)
    got, applied = det.redact_faces(src, (boxes, count), sel=sel, cfg=cfg, dst=dst)
    assert applied.tolist() == list(want_applied), what
    for b in range(len(frames)):
        assert src_bufs[b].tobytes() == before[b].tobytes() and got[b].tobytes() == want[b].tobytes(), "%s: host form out of place, frame %d" % (what, b)
        h, w = frames[b].shape[:2]
        exp = np.full_like(dst_bufs[b], 0x5C)
        np.lib.stride_tricks.as_strided(exp, (h, w, 3), (w * 3 + b % 5, 3, 1))[:] = want[b]
        assert dst_bufs[b].tobytes() == exp.tobytes(), "%s: host form out of place, dst padding of frame %d" % (what, b)


def test_constructed_cases_on_the_host_and_the_device_form(rfd, det):
    """every case of tests/redact_cases.py, grouped by config into calls of up to 32 frames of different sizes: both device forms
    and both host forms equal the restatement byte for byte and give every written frame"""
    groups = {}
    for name in sorted(RC.CASES):
        groups.setdefault(tuple(sorted(RC.CASES[name]["cfg"].items())), []).append(name)
    seen = 0
    for fields, names in sorted(groups.items()):
        for at in range(0, len(names), MAX_BATCH):
            part = names[at:at + MAX_BATCH]
            frames = [RC.CASES[n]["frame"] for n in part]
            boxes, count = _slabs([RC.CASES[n]["rows"] for n in part])
            want, applied = RR.run(frames, boxes, count, None, RR.config(**dict(fields)))
            for n, w, a in zip(part, want, applied):
                RC.check(n, w, a)
                seen += 1
            cfg = _cfg(rfd, dict(fields))
            d = Device(frames, boxes, count, strides=[f.shape[1] * 3 + 1 + i % 3 for i, f in enumerate(frames)], offsets=[i % 4 for i in range(len(frames))])
            d.both(det, cfg, want, applied, "%s" % (part,))
            _host_forms(det, frames, boxes, count, None, cfg, want, applied, "%s" % (part,))
    assert seen == len(RC.CASES)


def _random_rows(rng, h, w, k):
    """k boxes of a frame: sides from one pixel up to beyond the frame, corners at fractions, some outside, now and then a NaN"""
    rows = []
    for _ in range(k):
        bw, bh = rng.uniform(0, w * 0.8), rng.uniform(0, h * 0.8)
        x1, y1 = rng.uniform(-0.3 * w - 2, w), rng.uniform(-0.3 * h - 2, h)
        box = [x1, y1, x1 + bw, y1 + bh, 0.75]
        if rng.integers(0, 10) == 0:
            box[rng.integers(0, 4)] = rng.choice([np.nan, np.inf, -np.inf])
        rows.append(box)
    return rows


SIZES = [(1, 1), (7, 5), (5, 7), (64, 64), (65, 67), (67, 65), (130, 70), (70, 130)]          # (h, w)


@pytest.mark.parametrize("cell", [2, 3, 8, 16, 64])
def test_seeded_frames_cells_modes_and_shapes(rfd, det, cell):
    """frames of 1 x 1 up to 130 x 70, both ways round, in one call: tiles of 64 (63 at cell 3) cut by the frame, regions that cross
    tile edges and end inside a cell; both modes, both shapes, in place and out of place, odd strides and data offsets 0 .. 3"""
    rng = np.random.default_rng(100 + cell)
    frames = [helpers.make_image(500 + i, h, w) for i, (h, w) in enumerate(SIZES)]
    rows = [_random_rows(rng, f.shape[0], f.shape[1], 1 + i % 6) for i, f in enumerate(frames)]
    rows[3].append([0, 0, 63, 63, 0.5])                          # a whole tile and one pixel more each way
    rows[4].append([-5, -5, 64.5, 64.5, 0.5])
    boxes, count = _slabs(rows)
    strides = [f.shape[1] * 3 + (i * 3 + cell) % 8 for i, f in enumerate(frames)]
    d = Device(frames, boxes, count, strides=strides, offsets=[(i + cell) % 4 for i in range(len(frames))],
               dst_strides=[f.shape[1] * 3 + (i * 5 + 1) % 7 for i, f in enumerate(frames)], dst_offsets=[(3 * i + 1) % 4 for i in range(len(frames))])
    painted = 0
    for mode in (RR.FILL, RR.PIXELATE):
        for shape in (RR.RECT, RR.ELLIPSE):
            fields = dict(mode=mode, shape=shape, cell=cell, fill=(3, 250, 77), margin_x=0.1 * shape, margin_top=0.25, margin_bottom=0.0)
            want, applied = RR.run(frames, boxes, count, None, RR.config(**fields))
            d.both(det, _cfg(rfd, fields), want, applied, "cell %d mode %d shape %d" % (cell, mode, shape), async_=bool(mode))
            painted += sum(int((w != f).any()) for w, f in zip(want, frames))
    assert painted >= 20                                          # the calls did paint


@pytest.mark.parametrize("n", [1, 32])
def test_one_and_32_frames_of_mixed_sizes(rfd, det, n):
    """n frames of different sizes in one call, up to 12 seeded boxes each (one frame empty), a caller-written sel array; the
    default config and one with every field moved; the host forms of the same calls"""
    rng = np.random.default_rng(2000 + n)
    sizes = [(40, 40), (41, 47), (64, 33), (33, 64), (150, 200), (97, 131), (128, 128), (45, 199)]
    frames, rows, strides, offsets = [], [], [], []
    for b in range(n):
        h, w = sizes[(b + n) % len(sizes)]
        frames.append(helpers.make_image(700 + b, h, w))
        rows.append(_random_rows(rng, h, w, 0 if b == 5 else int(rng.integers(1, 13))))
        strides.append(w * 3 + (b + n) % 8)
        offsets.append((b + n // 32) % 4)
    boxes, count = _slabs(rows)
    sel = rng.integers(0, 8, (n, MAX_DET)).astype(np.uint32)
    moved = dict(mode=RR.FILL, shape=RR.RECT, cell=5, fill=(255, 1, 128), margin_x=0.0, margin_top=1.5, margin_bottom=4.0, sel_mask=5, sel_value=4)
    for fields, s in (({}, None), (moved, sel)):
        want, applied = RR.run(frames, boxes, count, s, RR.config(**fields))
        d = Device(frames, boxes, count, sel=s, strides=strides, offsets=offsets)
        d.both(det, _cfg(rfd, fields), want, applied, "%d frames" % n, async_=bool(fields))
        _host_forms(det, frames, boxes, count, s, _cfg(rfd, fields), want, applied, "%d frames" % n)
        assert n == 1 or (applied > 0).sum() > 10


def test_counts_and_max_det_rows_in_one_frame(rfd, det):
    """counts 0, negative and above max_det (clamped), and 1024 rows in one 200 x 150 frame, which a workgroup takes in four chunks
    of 256; then a count between, so the last chunk is cut"""
    frames = [helpers.make_image(300 + b, 150, 200) for b in range(4)]
    rows = []
    for b in range(4):
        rr = []
        for i in range(MAX_DET):
            w, h = 3 + (i % 9), 2 + ((i // 9) % 7)
            x, y = (i * 7) % (200 - w), (i * 13) % (150 - h)
            rr.append([x + 0.25, y + 0.5, x + w - 1 + 0.5, y + h - 1 + 0.25, 0.75])
        rows.append(rr)
    boxes, count = _slabs(rows)
    cfg = dict(cell=8, margin_x=0.0, margin_top=0.0, margin_bottom=0.0)
    for counts in ([0, -7, MAX_DET + 1, MAX_DET], [0, 0, 600, 137]):
        count[:] = counts
        want, applied = RR.run(frames, boxes, count, None, RR.config(**cfg))
        assert applied.tolist() == [0, 0, min(counts[2], MAX_DET), counts[3]]
        assert want[0].tobytes() == frames[0].tobytes() and want[1].tobytes() == frames[1].tobytes() and (want[3] != frames[3]).any()
        Device(frames, boxes, count).both(det, _cfg(rfd, cfg), want, applied, "counts %s" % counts, async_=True)
    # the rows of the fourth chunk alone reach the frame: rows 0 .. 767 are skipped
    boxes[2, :768, 0] = np.nan
    count[:] = [0, 0, MAX_DET, 0]
    want, applied = RR.run(frames, boxes, count, None, RR.config(**cfg))
    assert applied.tolist() == [0, 0, 256, 0]
    Device(frames, boxes, count).both(det, _cfg(rfd, cfg), want, applied, "the fourth chunk")


def test_sel_null_all_none_and_the_tracker_flags(rfd, det):
    rng = np.random.default_rng(7)
    frames = [helpers.make_image(900 + b, 90, 120) for b in range(3)]
    rows = [[[10 + 9 * i, 5 + 6 * i, 22 + 9 * i, 20 + 6 * i, 0.9] for i in range(10)] for _ in frames]
    boxes, count = _slabs(rows)
    flags = rng.integers(0, 8, (3, MAX_DET)).astype(np.uint32)              # NEW 1, CONFIRMED 2, DUE 4 in every combination
    confirmed = [int(((flags[b, :10] & rfd.TRACK_CONFIRMED) != 0).sum()) for b in range(3)]
    plain = dict(mode=RR.FILL, shape=RR.ELLIPSE, fill=(0, 0, 255))
    for what, sel, fields, expect in (("NULL", None, dict(plain, sel_mask=6, sel_value=2), [10] * 3),
                                      ("all pass", flags, dict(plain, sel_mask=0, sel_value=0), [10] * 3),
                                      ("none pass", flags, dict(plain, sel_mask=0, sel_value=1), [0] * 3),
                                      ("confirmed", flags, dict(plain, sel_mask=rfd.TRACK_CONFIRMED, sel_value=rfd.TRACK_CONFIRMED), confirmed),
                                      ("high bit", flags | np.uint32(0x80000000), dict(plain, sel_mask=0x80000002, sel_value=0x80000002), confirmed)):
        want, applied = RR.run(frames, boxes, count, sel, RR.config(**fields))
        assert applied.tolist() == expect and 0 < min(confirmed) and max(confirmed) < 10, what
        d = Device(frames, boxes, count, sel=sel)
        d.both(det, _cfg(rfd, fields), want, applied, what)
        if what == "none pass":
            assert all(w.tobytes() == f.tobytes() for w, f in zip(want, frames))
    # applied is optional
    got = d.run(det, _cfg(rfd, fields), True, with_applied=False)
    assert (got[2].view(np.uint8) == FILL).all() and got[0][0].tobytes() == _embed(want[0], 360, 0, PAD_SRC).tobytes()


def test_argument_errors_on_the_device(rfd, det):
    L = rfd.load_library()
    frames = [helpers.make_image(40, 30, 50), helpers.make_image(41, 30, 50)]
    boxes, count = _slabs([[[5, 5, 30, 20, 0.9]], [[5, 5, 30, 20, 0.9]]])
    d = Device(frames, boxes, count)
    dets = rfd.rfd_dets(d.boxes.data_ptr(), None, d.count.data_ptr(), None)

    def refused(status, text, n=2, imgs=None, dsts=None, use_dst=True):
        arr, darr = (rfd.rfd_image * max(n, 2))(), (rfd.rfd_image * max(n, 2))()
        for a, bufs, place in ((arr, d.src, d.place), (darr, d.dst, d.dplace)):
            for i, im in enumerate(d.desc(bufs, place)):
                a[i].data, a[i].height, a[i].width, a[i].stride = im
        for a, changes in ((arr, imgs), (darr, dsts)):
            for i, im in (changes or {}).items():
                a[i].data, a[i].height, a[i].width, a[i].stride = im
        host = np.zeros(16, F)
        hd = rfd.rfd_dets(host.ctypes.data, None, host.ctypes.data, None)
        for call in (lambda: L.rfd_redact_faces_device(det._ctx, arr, darr if use_dst else None, n, C.byref(dets), None, None, d.applied.data_ptr(), 1),
                     lambda: L.rfd_redact_faces(det._ctx, arr, darr if use_dst else None, n, C.byref(hd), None, None, None)):
            assert call() == status
            assert text in L.rfd_last_error().decode(), L.rfd_last_error()
    ptr, h, w, st = d.desc(d.src, d.place)[1]
    dptr = d.desc(d.dst, d.dplace)[1][0]
    refused(rfd.RFD_ERR_CAPACITY, "max_batch_size", n=MAX_BATCH + 1)
    for use_dst in (True, False):
        refused(rfd.RFD_ERR_INVALID_ARG, "frame 1: data", imgs={1: (None, h, w, st)}, use_dst=use_dst)
        refused(rfd.RFD_ERR_INVALID_ARG, "frame 1: non-positive size", imgs={1: (ptr, 0, w, st)}, use_dst=use_dst)
        refused(rfd.RFD_ERR_INVALID_ARG, "frame 0: non-positive size", imgs={0: (ptr, h, -1, st)}, use_dst=use_dst)
        refused(rfd.RFD_ERR_INVALID_ARG, "frame 1: stride", imgs={1: (ptr, h, w, w * 3 - 1)}, use_dst=use_dst)
        refused(rfd.RFD_ERR_INVALID_ARG, "frame 1: a side exceeds 32768", imgs={1: (ptr, 32769, w, st)}, use_dst=use_dst)
    refused(rfd.RFD_ERR_INVALID_ARG, "dst 1: data", dsts={1: (None, h, w, st)})
    refused(rfd.RFD_ERR_INVALID_ARG, "dst 1: stride", dsts={1: (dptr, h, w, w * 3 - 1)})
    refused(rfd.RFD_ERR_INVALID_ARG, "dst 1: size", dsts={1: (dptr, h, w - 1, st)})
    refused(rfd.RFD_ERR_INVALID_ARG, "dst 0: size", dsts={0: (dptr, h + 1, w, st)})
    assert L.rfd_redact_faces_device(det._ctx, None, None, 0, None, None, None, None, 1) == rfd.RFD_OK        # n = 0 is a no-op
    assert L.rfd_redact_faces(det._ctx, None, None, 0, None, None, None, None) == rfd.RFD_OK
    det.sync()
    for t, hst in zip(d.src + d.dst, d.src_host + d.dst_host):
        assert t.cpu().numpy().tobytes() == hst.tobytes()                                                       # nothing was enqueued
    assert (d.applied.cpu().numpy().view(np.uint8) == FILL).all()


def test_detect_redact_encode_in_one_stream_order(rfd, det):
    """Two 300 x 200 frames, synthetic weights, async = 1 throughout: rfd_detect_batch_device -> rfd_redact_faces_device out of place
    -> rfd_encode_jpeg_batch_device on dst, one rfd_sync.  Each file equals the JPEG restatement of the redaction restatement
    applied to the detections the same call left, and the source frames are untouched."""
    import torch
    dev = torch.device("cuda", 0)
    det.init_synthetic_weights(1234)
    det.set_thresholds(0.0, 1.0)              # every anchor is a candidate and none is suppressed: the synthetic network has no say
    frames = [helpers.make_image(31, 200, 300), helpers.make_image(32, 200, 300)]
    n = 2
    bufs = [torch.from_numpy(np.ascontiguousarray(f)).to(dev) for f in frames]
    dsts = [torch.full((200 * 300 * 3,), PAD_DST, dtype=torch.uint8, device=dev) for _ in frames]
    fill32 = int(np.full(1, FILL * 0x01010101, np.uint32).view(np.int32)[0])
    t32 = lambda *shape: torch.full(shape, fill32, dtype=torch.int32, device=dev)
    d_boxes, d_lmk, d_count, d_total, d_applied = t32(n, MAX_DET, 5), t32(n, MAX_DET, 10), t32(n), t32(n), t32(n)
    slot = 1 << 17
    files, sizes = torch.zeros(n * slot, dtype=torch.uint8, device=dev), t32(n)
    # the first 200 rows of a frame are redacted: a cap by the count is not part of the call, so sel carries it
    sel = torch.from_numpy((np.arange(MAX_DET)[None, :].repeat(n, 0) < 200).astype(np.int32)).to(dev)
    fields = dict(cell=8, sel_mask=1, sel_value=1)
    ptrs, shapes = [b.data_ptr() for b in bufs], [f.shape[:2] for f in frames]
    torch.cuda.synchronize()
    det.detect_device(ptrs, shapes, d_boxes.data_ptr(), d_lmk.data_ptr(), d_count.data_ptr(), d_total.data_ptr(), async_=True)
    det.redact_faces([(p, h, w) for p, (h, w) in zip(ptrs, shapes)], (d_boxes.data_ptr(), d_count.data_ptr()), sel=sel.data_ptr(),
                     cfg=_cfg(rfd, fields), device=True, dst=[(t.data_ptr(), h, w) for t, (h, w) in zip(dsts, shapes)],
                     applied=d_applied.data_ptr(), async_=True)
    jcfg = rfd.jpeg_encode_config(90, JR.S420, 1)
    det.encode_jpeg_device([t.data_ptr() for t in dsts], shapes, files.data_ptr(), slot, sizes.data_ptr(), cfg=jcfg, async_=True)
    det.sync()
    torch.cuda.synchronize()
    boxes, count = d_boxes.cpu().numpy().view(F), d_count.cpu().numpy()
    assert count.min() > 64, count
    want, applied = RR.run(frames, boxes, count, sel.cpu().numpy().view(np.uint32), RR.config(**fields))
    assert d_applied.cpu().numpy().tolist() == applied.tolist() and applied.min() > 0
    size, data = sizes.cpu().numpy(), files.cpu().numpy()
    for b in range(n):
        assert (want[b] != frames[b]).any()
        assert dsts[b].cpu().numpy().tobytes() == want[b].tobytes(), "dst %d" % b
        assert bufs[b].cpu().numpy().tobytes() == frames[b].tobytes(), "source %d" % b
        file = JR.encode(want[b], 90, JR.S420, 1)
        assert size[b] == len(file) and data[b * slot:b * slot + size[b]].tobytes() == file, "file %d" % b
    det.set_thresholds(0.7, 0.45)
