"""The annotation on the device (include/rfd.h, "annotation") against tests/annotate_ref.py, byte for byte over WHOLE ALLOCATIONS:
the frames lie in exactly sized buffers filled with 0xA5, at odd strides and byte offsets, and every byte of every buffer is
compared -- the painted pixels, the pixels left alone, the stride padding and the bytes in front of the data pointer; in place
the source buffer is the output, out of place the source buffer must come back as it went in; `applied` is a filled allocation
too.  There is no tolerance: both sides are the same integer and f32 operations.  The constructed cases of
tests/annotate_cases.py are held to their written frames."""
import ctypes as C

import numpy as np
import pytest

import annotate_cases as AC
import annotate_ref as AR
import helpers
import jpeg_encode_ref as JR
import redact_ref as RR

pytestmark = pytest.mark.gpu

MAX_DET, MAX_BATCH = 1024, 32
FILL = 0xA5
F = np.float32


@pytest.fixture(scope="module")
def det(rfd):
    d = rfd.RetinaFaceDetection(image_size=(128, 128), max_batch_size=MAX_BATCH, max_det=MAX_DET)
    yield d
    d.close()


@pytest.fixture(scope="module")
def font(rfd):
    return [rfd.annotate_glyph(g) for g in range(14)]


def _slabs(rows, lmk=None, unused=0.0):
    """rows: per frame a list of box rows; lmk: per frame a list of ten floats per row -> boxes [n, MAX_DET, 5], landmarks
    [n, MAX_DET, 10], count [n]"""
    boxes, marks, count = np.full((len(rows), MAX_DET, 5), unused, F), np.full((len(rows), MAX_DET, 10), np.nan, F), np.zeros(len(rows), np.int32)
    for b, rr in enumerate(rows):
        count[b] = len(rr)
        for i, bx in enumerate(rr):
            boxes[b, i, :len(bx)] = bx
            if lmk is not None:
                marks[b, i] = np.asarray(lmk[b][i], F).reshape(10)
    return boxes, marks, count


def _per_row(lists, dtype):
    """per frame a list of per-row entries, or None -> [n, MAX_DET]; None when no frame has one"""
    if all(l is None for l in lists):
        return None
    out = np.zeros((len(lists), MAX_DET), dtype)
    for b, l in enumerate(lists):
        if l is not None:
            out[b, :len(l)] = np.asarray(l, dtype)
    return out


def _embed(frame, stride, off):
    """the exactly sized buffer of a frame at a byte offset and a stride, everything else the pattern"""
    h, w = frame.shape[:2]
    host = np.full(off + (h - 1) * stride + w * 3, FILL, np.uint8)
    np.lib.stride_tricks.as_strided(host[off:], (h, w * 3), (stride, 1))[:] = frame.reshape(h, w * 3)
    return host


def _cfg(rfd, fields):
    return rfd.annotate_config(**{k: (list(v) if k == "styles" else v) for k, v in fields.items()})


class Device:
    """frames, dst frames, slabs and per-row arrays in HBM; run() gives back every buffer whole"""

    def __init__(self, frames, boxes, lmk, count, sel=None, label=None, value=None, strides=None, offsets=None, dst_strides=None, dst_offsets=None):
        import torch
        self.torch, self.dev, self.frames, self.n = torch, torch.device("cuda", 0), frames, len(frames)
        pick = lambda a, i, d: d if a is None else a[i]
        self.place = [(pick(strides, i, f.shape[1] * 3), pick(offsets, i, 0)) for i, f in enumerate(frames)]
        self.dplace = [(pick(dst_strides, i, f.shape[1] * 3), pick(dst_offsets, i, 0)) for i, f in enumerate(frames)]
        self.src_host = [_embed(f, st, off) for f, (st, off) in zip(frames, self.place)]
        self.dst_host = [_embed(np.full_like(f, FILL), st, off) for f, (st, off) in zip(frames, self.dplace)]
        up = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(self.dev)
        self.boxes, self.lmk, self.count = up(boxes), up(lmk), up(count)
        self.sel = up(None if sel is None else sel.astype(np.uint32).view(np.int32))
        self.label, self.value = up(None if label is None else label.astype(np.int32)), up(None if value is None else value.astype(F))
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
        ptr = lambda t: None if t is None else t.data_ptr()
        det.annotate_faces(self.desc(self.src, self.place), (self.boxes.data_ptr(), ptr(self.lmk), self.count.data_ptr()), sel=ptr(self.sel),
                           label=ptr(self.label), value=ptr(self.value), cfg=cfg, device=True,
                           dst=None if in_place else self.desc(self.dst, self.dplace), applied=self.applied.data_ptr() if with_applied else None,
                           async_=async_)
        if async_:
            det.sync()
        return [t.cpu().numpy() for t in self.src], [t.cpu().numpy() for t in self.dst], self.applied.cpu().numpy()

    def check(self, got, want, want_applied, in_place, what):
        src, dst, applied = got
        for b in range(self.n):
            (st, off), (dst_st, dst_off) = self.place[b], self.dplace[b]
            exp_src = _embed(want[b], st, off) if in_place else self.src_host[b]
            exp_dst = self.dst_host[b] if in_place else _embed(want[b], dst_st, dst_off)
            for name, g, e in (("source", src[b], exp_src), ("dst", dst[b], exp_dst)):
                assert g.tobytes() == e.tobytes(), "%s, %s: the %s buffer of frame %d (%s) differs at bytes %s" % (
                    what, "in place" if in_place else "out of place", name, b, self.frames[b].shape, np.flatnonzero(g != e)[:8].tolist())
        assert applied[:self.n].tolist() == list(want_applied), (what, applied[:self.n], want_applied)
        assert (applied[self.n:].view(np.uint8) == FILL).all(), what

    def both(self, det, cfg, want, want_applied, what, async_=False):
        for in_place in (True, False):
            self.check(self.run(det, cfg, in_place, async_=async_), want, want_applied, in_place, what)


def _host_forms(det, frames, boxes, lmk, count, sel, label, value, cfg, want, want_applied, what):
    """the host form, in place on strided views and out of place into strided views: the rows come back, the padding stays"""
    def views(fill=None):
        out, bufs = [], []
        for i, f in enumerate(frames):
            h, w = f.shape[:2]
            buf = np.full(h * (w * 3 + i % 5), FILL, np.uint8)
            v = np.lib.stride_tricks.as_strided(buf, (h, w, 3), (w * 3 + i % 5, 3, 1))
            v[:] = f if fill is None else fill
            out.append(v)
            bufs.append(buf)
        return out, bufs

    def expect(b, buf):
        h, w = frames[b].shape[:2]
        exp = np.full_like(buf, FILL)
        np.lib.stride_tricks.as_strided(exp, (h, w, 3), (w * 3 + b % 5, 3, 1))[:] = want[b]
        return exp
    src, src_bufs = views()
    applied = np.full(len(frames) + 1, FILL * 0x01010101, np.uint32).view(np.int32)
    det.annotate_faces(src, (boxes, lmk, count), sel=sel, label=label, value=value, cfg=cfg, applied=applied)
    assert applied[:-1].tolist() == list(want_applied) and (applied[-1:].view(np.uint8) == FILL).all(), what
    for b, buf in enumerate(src_bufs):
        assert buf.tobytes() == expect(b, buf).tobytes(), "%s: host form in place, frame %d" % (what, b)
    src, src_bufs = views()
    before = [b.copy() for b in src_bufs]
    dst, dst_bufs = views(fill=0x33)
    got, applied = det.annotate_faces(src, (boxes, lmk, count), sel=sel, label=label, value=value, cfg=cfg, dst=dst)
    assert applied.tolist() == list(want_applied), what
    for b in range(len(frames)):
        assert src_bufs[b].tobytes() == before[b].tobytes(), "%s: host form out of place, source %d" % (what, b)
        assert dst_bufs[b].tobytes() == expect(b, dst_bufs[b]).tobytes(), "%s: host form out of place, dst %d" % (what, b)


def test_constructed_cases_on_the_host_and_the_device_form(rfd, det, font):
    """every case of tests/annotate_cases.py, grouped by config and by which arrays it passes into calls of up to 32 frames of
    different sizes: both device forms and both host forms equal the restatement byte for byte and give every written frame"""
    cases = AC.cases(font)
    groups = {}
    for name in sorted(cases):
        c = cases[name]
        key = (tuple(sorted(c["cfg"].items())), c["sel"] is None, c["label"] is None, c["value"] is None, c["count"] == "above")
        groups.setdefault(key, []).append(name)
    seen = 0
    for key, names in sorted(groups.items(), key=lambda kv: kv[1]):
        fields = dict(key[0])
        for at in range(0, len(names), MAX_BATCH):
            part = [cases[n] for n in names[at:at + MAX_BATCH]]
            frames = [c["frame"] for c in part]
            boxes, lmk, count = _slabs([c["rows"] for c in part], [c["lmk"] for c in part], unused=np.nan if key[4] else 0.0)
            for b, c in enumerate(part):
                if c["count"] is not None:
                    count[b] = MAX_DET + 1 if c["count"] == "above" else c["count"]
            sel, label, value = (_per_row([c[k] for c in part], t) for k, t in (("sel", np.uint32), ("label", np.int32), ("value", F)))
            want, applied = AR.run(frames, boxes, lmk, count, sel, label, value, AR.config(**fields), font)
            for n, w, a in zip(names[at:at + MAX_BATCH], want, applied):
                AC.check(cases, n, w, a)
                seen += 1
            cfg = _cfg(rfd, fields)
            d = Device(frames, boxes, lmk, count, sel, label, value, strides=[f.shape[1] * 3 + 1 + i % 3 for i, f in enumerate(frames)],
                       offsets=[i % 4 for i in range(len(frames))])
            d.both(det, cfg, want, applied, "%s" % (names,))
            _host_forms(det, frames, boxes, lmk, count, sel, label, value, cfg, want, applied, "%s" % (names,))
    assert seen == len(cases)


def _random_rows(rng, h, w, k):
    """k boxes of a frame with landmarks, labels and values: sides from one pixel up to beyond the frame, corners at fractions, some
    outside, now and then a NaN or an infinity; landmarks inside and around the box; labels of every length; values around 0 .. 1"""
    rows, marks, labels, values = [], [], [], []
    for _ in range(k):
        bw, bh = rng.uniform(0, w * 0.8), rng.uniform(0, h * 0.8)
        x1, y1 = rng.uniform(-0.3 * w - 2, w), rng.uniform(-0.3 * h - 2, h)
        box = [x1, y1, x1 + bw, y1 + bh, rng.choice([0.0, 0.5, 0.995, 0.9951, 1.0, rng.uniform(0, 1)])]
        if rng.integers(0, 10) == 0:
            box[rng.integers(0, 4)] = rng.choice([np.nan, np.inf, -np.inf])
        m = np.stack([rng.uniform(x1 - 5, x1 + bw + 5, 5), rng.uniform(y1 - 5, y1 + bh + 5, 5)], axis=1)
        if rng.integers(0, 4) == 0:
            m[rng.integers(0, 5), rng.integers(0, 2)] = rng.choice([np.nan, np.inf, -3e9])
        rows.append(box)
        marks.append(m.reshape(10))
        labels.append(int(rng.choice([-1, 0, 7, 42, 999, 123456, 2**31 - 1, -2**31])))
        values.append(float(rng.choice([np.nan, -0.5, 0.0, 0.004999, 0.83, 1.0, 12.0, rng.uniform(0, 1)])))
    return rows, marks, labels, values


def _seeded(rng, frames, counts):
    parts = [_random_rows(rng, f.shape[0], f.shape[1], k) for f, k in zip(frames, counts)]
    boxes, lmk, count = _slabs([p[0] for p in parts], [p[1] for p in parts])
    return boxes, lmk, count, _per_row([p[2] for p in parts], np.int32), _per_row([p[3] for p in parts], F)


SIZES = [(1, 1), (7, 5), (5, 7), (64, 64), (65, 67), (67, 65), (130, 70), (70, 130)]          # (h, w)
SOURCES = [(l, v) for l in (AR.NONE, AR.ARRAY) for v in (AR.NONE, AR.ARRAY, AR.SCORE)]


@pytest.mark.parametrize("label_source,value_source", SOURCES)
def test_seeded_frames_and_every_source_combination(rfd, det, font, label_source, value_source):
    """frames of 1 x 1 up to 130 x 70, both ways round, in one call: tiles of 64 cut by the frame, outlines, plates and marks that
    cross tile edges; every combination of label and value source (an array its source does not name is passed as NULL), two
    thicknesses, radii, scales and alphas, in place and out of place, odd strides and data offsets 0 .. 3"""
    rng = np.random.default_rng(100 + 3 * label_source + value_source)
    frames = [helpers.make_image(500 + i, h, w) for i, (h, w) in enumerate(SIZES)]
    boxes, lmk, count, label, value = _seeded(rng, frames, [1 + i % 6 for i in range(len(frames))])
    sel = rng.integers(0, 4, (len(frames), MAX_DET)).astype(np.uint32)
    if label_source != AR.ARRAY:
        label = None
    if value_source != AR.ARRAY:
        value = None
    strides = [f.shape[1] * 3 + (i * 3 + value_source) % 8 for i, f in enumerate(frames)]
    d = Device(frames, boxes, lmk, count, sel, label, value, strides=strides, offsets=[(i + label_source) % 4 for i in range(len(frames))],
               dst_strides=[f.shape[1] * 3 + (i * 5 + 1) % 7 for i, f in enumerate(frames)], dst_offsets=[(3 * i + 1) % 4 for i in range(len(frames))])
    painted = 0
    for t, r, s, alpha in ((1, 2, 1, 256), (5, 0, 3, 77)):
        fields = dict(styles=((3, 3, (1, 2, 3)), (1, 0, (250, 128, 7))), thickness=t, mark_radius=r, label_source=label_source, value_source=value_source,
                      text_scale=s, text_colour=(255, 254, 0), alpha=alpha, margin_x=0.1, margin_top=0.25, margin_bottom=0.0)
        want, applied = AR.run(frames, boxes, lmk, count, sel, label, value, AR.config(**fields), font)
        d.both(det, _cfg(rfd, fields), want, applied, "sources %d %d, thickness %d" % (label_source, value_source, t), async_=alpha != 256)
        painted += sum(int((w != f).any()) for w, f in zip(want, frames))
    assert painted >= 8                                           # the calls did paint


@pytest.mark.parametrize("n", [1, 32])
def test_one_and_32_frames_of_mixed_sizes(rfd, det, font, n):
    """n frames of different sizes in one call, up to 12 seeded rows each (one frame empty); the default config (landmarks and
    the score) and one with every field moved; the host forms of the same calls"""
    rng = np.random.default_rng(2000 + n)
    sizes = [(40, 40), (41, 47), (64, 33), (33, 64), (150, 200), (97, 131), (128, 128), (45, 199)]
    frames = [helpers.make_image(700 + b, *sizes[(b + n) % len(sizes)]) for b in range(n)]
    boxes, lmk, count, label, value = _seeded(rng, frames, [0 if b == 5 else int(rng.integers(1, 13)) for b in range(n)])
    sel = rng.integers(0, 8, (n, MAX_DET)).astype(np.uint32)
    strides, offsets = [f.shape[1] * 3 + (b + n) % 8 for b, f in enumerate(frames)], [(b + n // 32) % 4 for b in range(n)]
    moved = dict(styles=((5, 4, (255, 1, 128)), (5, 1, (0, 0, 0)), (2, 2, (9, 9, 9)), (0, 0, (77, 88, 99))), thickness=16, mark_radius=8,
                 label_source=AR.ARRAY, value_source=AR.ARRAY, text_scale=4, text_colour=(1, 2, 3), alpha=255, margin_x=0.5, margin_top=1.5, margin_bottom=4.0)
    for fields, s, lb, va in (({}, None, None, None), (moved, sel, label, value)):
        want, applied = AR.run(frames, boxes, lmk, count, s, lb, va, AR.config(**fields), font)
        d = Device(frames, boxes, lmk, count, s, lb, va, strides=strides, offsets=offsets)
        d.both(det, _cfg(rfd, fields), want, applied, "%d frames" % n, async_=bool(fields))
        _host_forms(det, frames, boxes, lmk, count, s, lb, va, _cfg(rfd, fields), want, applied, "%d frames" % n)
        assert n == 1 or (applied > 0).sum() > 10


def test_counts_and_max_det_rows_in_one_frame(rfd, det, font):
    """counts 0, negative and above max_det (clamped), and 1024 rows in one 200 x 150 frame, which a workgroup takes in four chunks
    of 256 with the lowest row on top; then a count between, so the last chunk is cut, and rows of the fourth chunk alone"""
    frames = [helpers.make_image(300 + b, 150, 200) for b in range(4)]
    rows, marks = [], []
    for b in range(4):
        rr, mm = [], []
        for i in range(MAX_DET):
            w, h = 8 + (i % 9), 6 + ((i // 9) % 7)
            x, y = (i * 7) % (200 - w), (i * 13) % (150 - h)
            rr.append([x + 0.25, y + 0.5, x + w - 1 + 0.5, y + h - 1 + 0.25, (i % 101) / 100.0])
            mm.append([x + 2, y + 2, x + w - 3, y + 2, x + w // 2, y + h // 2, x + 2, y + h - 2, x + w - 3, y + h - 2])
        rows.append(rr)
        marks.append(mm)
    boxes, lmk, count = _slabs(rows, marks)
    label = (np.arange(4 * MAX_DET, dtype=np.int32).reshape(4, MAX_DET) * 37) % 1000
    sel = (np.arange(4 * MAX_DET, dtype=np.uint32).reshape(4, MAX_DET) % 3)
    fields = dict(styles=((3, 0, (0, 0, 255)), (3, 1, (0, 255, 0)), (3, 2, (255, 0, 0))), thickness=1, mark_radius=1, label_source=AR.ARRAY,
                  value_source=AR.SCORE, text_scale=1, text_colour=(255, 255, 255), alpha=256)
    for counts in ([0, -7, MAX_DET + 1, MAX_DET], [0, 0, 600, 137]):
        count[:] = counts
        want, applied = AR.run(frames, boxes, lmk, count, sel, label, None, AR.config(**fields), font)
        assert applied.tolist() == [0, 0, min(counts[2], MAX_DET), counts[3]]
        assert want[0].tobytes() == frames[0].tobytes() and want[1].tobytes() == frames[1].tobytes() and (want[3] != frames[3]).any()
        Device(frames, boxes, lmk, count, sel, label).both(det, _cfg(rfd, fields), want, applied, "counts %s" % counts, async_=True)
    boxes[2, :768, 0] = np.nan                                    # the rows of the fourth chunk alone reach the frame
    count[:] = [0, 0, MAX_DET, 0]
    want, applied = AR.run(frames, boxes, lmk, count, sel, label, None, AR.config(**fields), font)
    assert applied.tolist() == [0, 0, 256, 0]
    Device(frames, boxes, lmk, count, sel, label).both(det, _cfg(rfd, fields), want, applied, "the fourth chunk")


def test_sel_as_the_tracker_flags_with_two_styles(rfd, det, font):
    rng = np.random.default_rng(7)
    frames = [helpers.make_image(900 + b, 90, 120) for b in range(3)]
    rows = [[[10 + 9 * i, 25 + 6 * i, 22 + 9 * i, 40 + 6 * i, 0.9 - 0.05 * i] for i in range(10)] for _ in frames]
    boxes, lmk, count = _slabs(rows)
    flags = rng.integers(0, 8, (3, MAX_DET)).astype(np.uint32)              # NEW 1, CONFIRMED 2, DUE 4 in every combination
    confirmed = [int(((flags[b, :10] & rfd.TRACK_CONFIRMED) != 0).sum()) for b in range(3)]
    new = [int(((flags[b, :10] & (rfd.TRACK_CONFIRMED | rfd.TRACK_NEW)) == rfd.TRACK_NEW).sum()) for b in range(3)]
    two = ((rfd.TRACK_CONFIRMED, rfd.TRACK_CONFIRMED, (0, 255, 0)), (rfd.TRACK_NEW, rfd.TRACK_NEW, (0, 255, 255)))
    plain = dict(thickness=2, mark_radius=0, value_source=AR.SCORE, text_scale=1)
    for what, sel, styles, expect in (("NULL", None, ((6, 2, (1, 1, 1)),), [0] * 3), ("NULL, a style for the word 0", None, ((6, 0, (1, 1, 1)),), [10] * 3),
                                      ("confirmed green, new yellow", flags, two, [c + k for c, k in zip(confirmed, new)]),
                                      ("high bit", flags | np.uint32(0x80000000), ((0x80000002, 0x80000002, (5, 5, 5)),), confirmed)):
        fields = dict(plain, styles=styles)
        want, applied = AR.run(frames, boxes, lmk, count, sel, None, None, AR.config(**fields), font)
        assert applied.tolist() == expect and 0 < min(confirmed) and max(confirmed) < 10 and max(new) > 0, what
        d = Device(frames, boxes, None, count, sel)
        d.both(det, _cfg(rfd, fields), want, applied, what)
    # applied is optional
    got = d.run(det, _cfg(rfd, fields), True, with_applied=False)
    assert (got[2].view(np.uint8) == FILL).all() and got[0][0].tobytes() == _embed(want[0], 360, 0).tobytes()


def test_argument_errors_on_the_device(rfd, det):
    L = rfd.load_library()
    frames = [helpers.make_image(40, 30, 50), helpers.make_image(41, 30, 50)]
    boxes, lmk, count = _slabs([[[5, 5, 30, 20, 0.9]], [[5, 5, 30, 20, 0.9]]])
    d = Device(frames, boxes, lmk, count)
    dets = rfd.rfd_dets(d.boxes.data_ptr(), d.lmk.data_ptr(), d.count.data_ptr(), None)

    def refused(status, text, n=2, imgs=None, dsts=None, use_dst=True):
        arr, darr = (rfd.rfd_image * max(n, 2))(), (rfd.rfd_image * max(n, 2))()
        for a, bufs, place in ((arr, d.src, d.place), (darr, d.dst, d.dplace)):
            for i, im in enumerate(d.desc(bufs, place)):
                a[i].data, a[i].height, a[i].width, a[i].stride = im
        for a, changes in ((arr, imgs), (darr, dsts)):
            for i, im in (changes or {}).items():
                a[i].data, a[i].height, a[i].width, a[i].stride = im
        hd = rfd.rfd_dets(boxes.ctypes.data, lmk.ctypes.data, count.ctypes.data, None)
        for call in (lambda: L.rfd_annotate_faces_device(det._ctx, arr, darr if use_dst else None, n, C.byref(dets), None, None, None, None, d.applied.data_ptr(), 1),
                     lambda: L.rfd_annotate_faces(det._ctx, arr, darr if use_dst else None, n, C.byref(hd), None, None, None, None, None)):
            assert call() == status
            assert text in L.rfd_last_error().decode(), L.rfd_last_error()
    ptr, h, w, st = d.desc(d.src, d.place)[1]
    dptr = d.desc(d.dst, d.dplace)[1][0]
    refused(rfd.RFD_ERR_CAPACITY, "max_batch_size", n=MAX_BATCH + 1)
    for use_dst in (True, False):
        refused(rfd.RFD_ERR_INVALID_ARG, "frame 1: data", imgs={1: (None, h, w, st)}, use_dst=use_dst)
        refused(rfd.RFD_ERR_INVALID_ARG, "frame 1: non-positive size", imgs={1: (ptr, 0, w, st)}, use_dst=use_dst)
        refused(rfd.RFD_ERR_INVALID_ARG, "frame 1: stride", imgs={1: (ptr, h, w, w * 3 - 1)}, use_dst=use_dst)
        refused(rfd.RFD_ERR_INVALID_ARG, "frame 1: a side exceeds 32768", imgs={1: (ptr, 32769, w, st)}, use_dst=use_dst)
    refused(rfd.RFD_ERR_INVALID_ARG, "dst 1: data", dsts={1: (None, h, w, st)})
    refused(rfd.RFD_ERR_INVALID_ARG, "dst 1: stride", dsts={1: (dptr, h, w, w * 3 - 1)})
    refused(rfd.RFD_ERR_INVALID_ARG, "dst 1: size", dsts={1: (dptr, h, w - 1, st)})
    assert L.rfd_annotate_faces_device(det._ctx, None, None, 0, None, None, None, None, None, None, 1) == rfd.RFD_OK        # n = 0 is a no-op
    assert L.rfd_annotate_faces(det._ctx, None, None, 0, None, None, None, None, None, None) == rfd.RFD_OK
    det.sync()
    for t, hst in zip(d.src + d.dst, d.src_host + d.dst_host):
        assert t.cpu().numpy().tobytes() == hst.tobytes()                                                       # nothing was enqueued
    assert (d.applied.cpu().numpy().view(np.uint8) == FILL).all()


def test_detect_track_who_redact_annotate_encode_in_one_stream_order(rfd, det, font):
    """Two 300 x 200 frames of two cameras, synthetic weights, async = 1 throughout and a single wait: rfd_detect_batch_device ->
    rfd_tracker_update_device -> rfd_tracker_who_device -> rfd_redact_faces_device out of place into dst (the confirmed rows, filled)
    -> rfd_annotate_faces_device IN PLACE on that dst (sel = who with a style for named and one for every other row, label =
    identity, value = id_score) -> rfd_encode_jpeg_batch_device on dst.  The restatements are fed what detection, the tracker and
    who left; dst equals the annotation restatement of the redaction restatement, each file is the JPEG restatement's file of that
    frame -- so it decodes to what the restated frame encodes to -- and the source frames are untouched."""
    import torch
    dev = torch.device("cuda", 0)
    det.init_synthetic_weights(1234)
    det.set_thresholds(0.0, 1.0)              # every anchor is a candidate and none is suppressed: the synthetic network has no say
    frames = [helpers.make_image(31, 200, 300), helpers.make_image(32, 200, 300)]
    n, streams = 2, [1, 0]
    bufs = [torch.from_numpy(np.ascontiguousarray(f)).to(dev) for f in frames]
    dsts = [torch.full((200 * 300 * 3,), FILL, dtype=torch.uint8, device=dev) for _ in frames]
    fill32 = int(np.full(1, FILL * 0x01010101, np.uint32).view(np.int32)[0])
    t32 = lambda *shape: torch.full(shape, fill32, dtype=torch.int32, device=dev)
    d_boxes, d_lmk, d_count, d_total = t32(n, MAX_DET, 5), t32(n, MAX_DET, 10), t32(n), t32(n)
    z = dict(track=t32(n, MAX_DET), flags=t32(n, MAX_DET), stats=t32(n, 4), ended=t32(n, 64), due_boxes=t32(n, MAX_DET, 5),
             due_landmarks=t32(n, MAX_DET, 10), due_count=t32(n), due_total=t32(n), due_track=t32(n, MAX_DET))
    d_who, d_identity, d_id_score, d_redacted, d_applied = t32(n, MAX_DET), t32(n, MAX_DET), t32(n, MAX_DET), t32(n), t32(n)
    slot = 1 << 17
    files, sizes = torch.zeros(n * slot, dtype=torch.uint8, device=dev), t32(n)
    out = rfd.rfd_track_out(z["track"].data_ptr(), z["flags"].data_ptr(), z["stats"].data_ptr(), z["ended"].data_ptr(),
                            rfd.rfd_dets(z["due_boxes"].data_ptr(), z["due_landmarks"].data_ptr(), z["due_count"].data_ptr(), z["due_total"].data_ptr()),
                            z["due_track"].data_ptr())
    tracker = det.tracker(streams=2, max_tracks=64, iou_min=0.3, max_missed=5, min_score=0.0, new_score=0.0, min_hits=1, improve=1.1)
    tracker.enable_identities(dim=512)
    ptrs, shapes = [b.data_ptr() for b in bufs], [f.shape[:2] for f in frames]
    images = [(p, h, w) for p, (h, w) in zip(ptrs, shapes)]
    painted = [(t.data_ptr(), h, w) for t, (h, w) in zip(dsts, shapes)]
    rfields = dict(mode=RR.FILL, shape=RR.RECT, fill=(40, 40, 40), sel_mask=rfd.TRACK_CONFIRMED, sel_value=rfd.TRACK_CONFIRMED)
    afields = dict(styles=((rfd.TRACK_NAMED, rfd.TRACK_NAMED, (0, 255, 0)), (0, 0, (0, 0, 255))), thickness=1, mark_radius=1, label_source=AR.ARRAY,
                   value_source=AR.ARRAY, text_scale=1, text_colour=(255, 255, 255), alpha=192, margin_x=0.1, margin_top=0.2, margin_bottom=0.1)
    jcfg = rfd.jpeg_encode_config(90, JR.S420, 1)
    torch.cuda.synchronize()
    try:
        det.detect_device(ptrs, shapes, d_boxes.data_ptr(), d_lmk.data_ptr(), d_count.data_ptr(), d_total.data_ptr(), async_=True)
        tracker.update_device(streams, d_boxes.data_ptr(), d_lmk.data_ptr(), d_count.data_ptr(), out, async_=True)
        tracker.who_device(streams, z["track"].data_ptr(), d_count.data_ptr(), d_who.data_ptr(), flags_ptr=z["flags"].data_ptr(),
                           identity_ptr=d_identity.data_ptr(), id_score_ptr=d_id_score.data_ptr(), async_=True)
        det.redact_faces(images, (d_boxes.data_ptr(), d_count.data_ptr()), sel=d_who.data_ptr(), cfg=rfd.redact_config(**rfields), device=True, dst=painted,
                         applied=d_redacted.data_ptr(), async_=True)
        det.annotate_faces(painted, (d_boxes.data_ptr(), d_lmk.data_ptr(), d_count.data_ptr()), sel=d_who.data_ptr(), label=d_identity.data_ptr(),
                           value=d_id_score.data_ptr(), cfg=_cfg(rfd, afields), device=True, applied=d_applied.data_ptr(), async_=True)
        det.encode_jpeg_device([t.data_ptr() for t in dsts], shapes, files.data_ptr(), slot, sizes.data_ptr(), cfg=jcfg, async_=True)
        det.sync()                                                                       # the single wait
        torch.cuda.synchronize()
        host = lambda t, dt=np.int32: t.cpu().numpy().view(dt)
        boxes, lmk, count = host(d_boxes, F), host(d_lmk, F), host(d_count)
        who, identity, id_score = host(d_who, np.uint32), host(d_identity), host(d_id_score, F)
        assert count.min() > 64, count
        live = np.arange(MAX_DET)[None, :] < count[:, None]
        assert ((who[live] & rfd.TRACK_CONFIRMED) != 0).any()
        redacted, r_applied = RR.run(frames, boxes, count, who, RR.config(**rfields))
        want, applied = AR.run(redacted, boxes, lmk, count, who, identity, id_score, AR.config(**afields), font)
        assert host(d_redacted).tolist() == r_applied.tolist() and host(d_applied).tolist() == applied.tolist() and applied.min() > 64
        size, data = host(sizes), files.cpu().numpy()
        for b in range(n):
            assert (redacted[b] != frames[b]).any() and (want[b] != redacted[b]).any()
            assert dsts[b].cpu().numpy().tobytes() == want[b].tobytes(), "dst %d" % b
            assert bufs[b].cpu().numpy().tobytes() == frames[b].tobytes(), "source %d" % b
            file = JR.encode(want[b], 90, JR.S420, 1)
            assert size[b] == len(file) and data[b * slot:b * slot + size[b]].tobytes() == file, "file %d" % b
    finally:
        tracker.close()
        det.set_thresholds(0.7, 0.45)
