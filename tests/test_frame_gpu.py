"""The frame conversion on the device (include/rfd.h, "frames in camera and decoder formats") against tests/frame_ref.py, bit for
bit, through all three forms: rfd_convert_frames_device (planes and frames in HBM), rfd_upload_frames_device (planes on the
host) and rfd_convert_frames (everything on the host).  There is no tolerance: both sides are the same int32 operations.  Every
output lies in one buffer pre-filled with a sentinel, and the whole buffer is compared, so a byte written past 3 * width of a
row, between two frames or behind the last one fails the test."""
import ctypes as C
import functools

import numpy as np
import pytest

import frame_cases as FC
import frame_ref as FR

pytestmark = pytest.mark.gpu

MAX_BATCH = 32
FILL, SRC_FILL = 0xA5, 0xEE
FORMS = ("device", "upload", "host")


@pytest.fixture(scope="module")
def det(rfd):
    d = rfd.RetinaFaceDetection(image_size=(128, 128), max_batch_size=MAX_BATCH, max_det=256)
    yield d
    d.close()


def _rows(buf, start, rows, row_bytes, stride):
    return np.lib.stride_tricks.as_strided(buf[start:], (rows, row_bytes), (stride, 1))


class Batch:
    """Frames (format, width, height, planes, color) laid out for one call of one form.  The planes lie in one source buffer,
    plane k of frame i at 16-aligned + src_geo[i][k][0] bytes with src_geo[i][k][1] bytes between its rows; the output frames lie
    in one buffer filled with FILL, frame i at 16-aligned + out_geo[i][0] with out_geo[i][1] bytes between its rows.  `want` is
    that buffer as it must be after the call."""

    def __init__(self, rfd, det, frames, wants, form, src_geo=None, out_geo=None, pinned=False):
        import torch
        self.rfd, self.det, self.form, self.n = rfd, det, form, len(frames)
        src_geo = src_geo or [[(0, 0)] * 3] * self.n
        out_geo = out_geo or [(0, 0)] * self.n
        spans, size = [], 0
        for f, geo in zip(frames, src_geo):
            for plane, (off, extra) in zip(f[3], geo):
                rows, rb = plane.shape
                start = (size + 15) // 16 * 16 + 16 + off
                spans.append((start, rb + extra, plane))
                size = start + (rows - 1) * (rb + extra) + rb
        src = np.full(size + 16, SRC_FILL, np.uint8)
        for start, stride, plane in spans:
            _rows(src, start, plane.shape[0], plane.shape[1], stride)[:] = plane
        outs, size = [], 0
        for f, (off, extra) in zip(frames, out_geo):
            start = (size + 15) // 16 * 16 + 16 + off
            outs.append((start, 3 * f[1] + extra))
            size = start + (f[2] - 1) * (3 * f[1] + extra) + 3 * f[1]
        self.want = np.full(size + 16, FILL, np.uint8)
        for f, w, (start, stride) in zip(frames, wants, outs):
            _rows(self.want, start, f[2], 3 * f[1], stride)[:] = w.reshape(f[2], 3 * f[1])
        dev = torch.device("cuda", 0)
        self.pinned = None
        if form == "device":
            self.src_buf = torch.from_numpy(src).to(dev)
            src_base = self.src_buf.data_ptr()
        elif pinned:                                                          # rfd_host_alloc memory
            self.pinned = C.c_void_p()
            assert det._L.rfd_host_alloc(src.size, C.byref(self.pinned)) == 0
            C.memmove(self.pinned, src.ctypes.data, src.size)
            src_base = self.pinned.value
        else:
            self.src_buf = src
            src_base = src.ctypes.data
        if form == "host":
            self.out_buf = np.full(self.want.size, FILL, np.uint8)
            out_base = self.out_buf.ctypes.data
        else:
            self.out_buf = torch.full((self.want.size,), FILL, dtype=torch.uint8, device=dev)
            out_base = self.out_buf.data_ptr()
        torch.cuda.synchronize()                                              # the context's stream is not ordered with torch's
        self.src = (rfd.rfd_frame * max(self.n, 1))()
        self.out = (rfd.rfd_image * max(self.n, 1))()
        self.plane_addr, self.out_addr, k = [], [], 0
        for i, f in enumerate(frames):
            addrs = []
            for _ in f[3]:
                addrs.append((src_base + spans[k][0], spans[k][1]))
                k += 1
            self.plane_addr.append(addrs)
            self.src[i] = rfd.frame(f[0], f[1], f[2], [a for a, _ in addrs], [s for _, s in addrs], f[4] if len(f) > 4 else 0)
            self.out[i].data, self.out[i].height, self.out[i].width, self.out[i].stride = out_base + outs[i][0], f[2], f[1], outs[i][1]
            self.out_addr.append((out_base + outs[i][0], outs[i][1]))

    def call(self, async_=False, n=None):
        L, c = self.det._L, self.det._ctx
        n = self.n if n is None else n
        if self.form == "device":
            return L.rfd_convert_frames_device(c, self.src, n, self.out, int(async_))
        if self.form == "upload":
            return L.rfd_upload_frames_device(c, self.src, n, self.out, int(async_))
        return L.rfd_convert_frames(c, self.src, n, self.out)

    def got(self):
        return self.out_buf if self.form == "host" else self.out_buf.cpu().numpy()

    def check(self, what):
        got = self.got()
        if got.tobytes() != self.want.tobytes():
            bad = np.flatnonzero(got != self.want)
            raise AssertionError("%s (%s form): %d bytes differ, first at %s: got %s, want %s" % (
                what, self.form, bad.size, bad[:6].tolist(), got[bad[:6]].tolist(), self.want[bad[:6]].tolist()))

    def close(self):
        if self.pinned is not None:
            self.det.sync()
            assert self.det._L.rfd_host_free(self.pinned) == 0
            self.pinned = None


def _run(rfd, det, frames, wants, form, what, **kw):
    b = Batch(rfd, det, frames, wants, form, **kw)
    status = b.call()
    assert status == 0, (what, form, det._L.rfd_last_error())
    b.check(what)
    b.close()
    return b


# ---- the constructed cases: every one through all three forms, held to its written pixels ----
@pytest.mark.parametrize("form", FORMS)
def test_constructed_cases(rfd, det, form):
    cases = FC.frames()
    assert len(cases) >= 29
    for at in range(0, len(cases), MAX_BATCH):
        part = cases[at:at + MAX_BATCH]
        _run(rfd, det, [c[1] for c in part], [c[2] for c in part], form, "constructed cases %d.." % at)
    if form == "host":                                                      # and through the array interface of the binding
        got = det.convert_frames([c[1] for c in cases[:MAX_BATCH]])
        for c, g in zip(cases, got):
            assert g.tobytes() == c[2].tobytes(), c[0]


# ---- the value cube ----
Y16 = (0, 1, 15, 16, 17, 64, 127, 128, 129, 200, 234, 235, 236, 253, 254, 255)


def _cube_frame(ys):
    """one 1024 x 1024 4:2:0 image: chroma sample j = row * 512 + column holds U = j & 255, V = (j >> 8) & 255, and the four luma
    samples over it hold ys[4 * (j >> 16) + 0 .. 3]: every (U, V) under 16 values of Y"""
    j = np.arange(512 * 512, dtype=np.int64).reshape(512, 512)
    u, v, g = (j & 255).astype(np.uint8), ((j >> 8) & 255).astype(np.uint8), j >> 16
    ys = np.asarray(ys, np.uint8)
    y = np.zeros((1024, 1024), np.uint8)
    for dy in range(2):
        for dx in range(2):
            y[dy::2, dx::2] = ys[4 * g + 2 * dy + dx]
    return y, u, v


def test_the_whole_value_cube_of_bt601_limited_as_nv12(rfd, det):
    """all 2^24 (Y, U, V): 16 frames of 1024 x 1024, frame k holding Y = 16 k .. 16 k + 15, in one call"""
    frames, wants = [], []
    seen = np.zeros(1 << 24, np.uint8)
    for k in range(16):
        y, u, v = _cube_frame(range(16 * k, 16 * k + 16))
        frames.append((FR.NV12, 1024, 1024, FR.planes_420(FR.NV12, y, u, v), FR.BT601_LIMITED))
        wants.append(FR.convert_frame(frames[-1]))
        seen[(y.astype(np.int64) << 16) | (np.repeat(np.repeat(u, 2, 0), 2, 1).astype(np.int64) << 8) | np.repeat(np.repeat(v, 2, 0), 2, 1)] = 1
    assert seen.all()                                                        # the frames do hold the whole cube
    _run(rfd, det, frames, wants, "device", "the BT.601 limited cube")


def test_every_chroma_pair_of_the_other_colours(rfd, det):
    """every (U, V) under the 16 values of Y16, one 1024 x 1024 frame per colour, in one call of three formats"""
    y, u, v = _cube_frame(Y16)
    frames = [(fmt, 1024, 1024, FR.planes_420(fmt, y, u, v), color)
              for fmt, color in ((FR.NV12, FR.BT601_FULL), (FR.I420, FR.BT709_LIMITED), (FR.NV21, FR.BT709_FULL))]
    wants = [FR.convert_frame(f) for f in frames]
    assert len({w.tobytes() for w in wants}) == 3
    _run(rfd, det, frames, wants, "device", "the three other colours")


# ---- the geometry sweep ----
WIDTHS, HEIGHTS = (1, 2, 3, 4, 5, 7, 8, 9, 63, 64, 65, 66), (1, 2, 3, 5)
SRC_EXTRA, OUT_EXTRA = (0, 1, 3), (0, 1, 5)


@functools.lru_cache(maxsize=None)
def _sweep():
    """every format x width x height three times over, each plane of a frame with its own drawn base offset 0 .. 3 and stride
    (tight, + 1, + 3), each output with its own offset 0 .. 3 and stride (tight, + 1, + 5), seeded contents and colours; shuffled,
    then cut into batches of 1, 2, 31 and 32 -> [(frames, wants, src_geo, out_geo)]"""
    rng = np.random.default_rng(20261020)
    items = []
    for rep in range(3):
        for fmt in range(10):
            for w in WIDTHS:
                for h in HEIGHTS:
                    f = (fmt, w, h, FR.random_planes(rng, fmt, w, h), int(rng.integers(0, 4)))
                    src = [(int(rng.integers(0, 4)), int(rng.choice(SRC_EXTRA))) for _ in range(3)]
                    out = (int(rng.integers(0, 4)), int(rng.choice(OUT_EXTRA)))
                    items.append((f, FR.convert_frame(f), src, out))
    order = rng.permutation(len(items))
    batches, at, k = [], 0, 0
    while at < len(items):
        size = (1, 2, 31, 32)[k % 4]
        part = [items[i] for i in order[at:at + size]]
        batches.append(tuple(list(x) for x in zip(*part)))
        at, k = at + size, k + 1
    return batches


def test_the_sweep_draws_what_it_claims():
    batches = _sweep()
    assert {len(b[0]) for b in batches} >= {1, 2, 31, 32}
    assert sum(len({f[0] for f in b[0]}) >= 5 for b in batches) >= len(batches) // 3          # mixed-format batches
    src, out, sizes = {}, {}, set()
    for frames, _, sgeo, ogeo in batches:
        for f, sg, og in zip(frames, sgeo, ogeo):
            sizes.add((f[0], f[1], f[2]))
            for k in range(len(f[3])):
                src.setdefault((f[0], k), set()).add(sg[k])
            out.setdefault(f[0], set()).add(og)
    assert len(sizes) == 10 * len(WIDTHS) * len(HEIGHTS)
    assert all(len(v) == 12 for v in src.values()) and len(src) == 5 + 2 * 2 + 3 + 2          # every plane of every format: 4 offsets x 3 strides
    assert all(len(v) == 12 for v in out.values()) and len(out) == 10


def _paths(batch, frames):
    """which read and store paths the addresses of a batch select, counted per row.  The unit of a wide read is 16 bytes (four
    pixels) in a BGRA / RGBA row, 2 bytes in a chroma row of I420, 4 bytes in every other row: a row is read wide where it holds a
    unit and starts aligned to it (read_16, read_2, read_4), and every row whose length is no multiple of its unit, or that
    starts unaligned, takes the byte path (bytes_16, bytes_2, bytes_4).  A row is stored wide where it holds 4 pixels and starts
    4-aligned."""
    n = dict(read_16=0, bytes_16=0, read_2=0, bytes_2=0, read_4=0, bytes_4=0, store_wide=0, store_bytes=0)
    for f, planes, (out, ostride) in zip(frames, batch.plane_addr, batch.out_addr):
        for k, ((addr, stride), plane) in enumerate(zip(planes, f[3])):
            unit = 16 if f[0] in (FR.BGRA, FR.RGBA) else 2 if f[0] == FR.I420 and k > 0 else 4
            for r in range(plane.shape[0]):
                wide = (addr + r * stride) % unit == 0 and plane.shape[1] >= unit
                n["read_%d" % unit] += wide
                n["bytes_%d" % unit] += (not wide) or plane.shape[1] % unit != 0
        for r in range(f[2]):
            wide = (out + r * ostride) % 4 == 0 and f[1] >= 4
            n["store_wide"] += wide
            n["store_bytes"] += (not wide) or f[1] % 4 != 0
    return n


def test_geometry_sweep_on_the_device(rfd, det):
    total = {}
    for i, (frames, wants, sgeo, ogeo) in enumerate(_sweep()):
        b = _run(rfd, det, frames, wants, "device", "sweep batch %d of %d frames" % (i, len(frames)), src_geo=sgeo, out_geo=ogeo)
        for k, v in _paths(b, frames).items():
            total[k] = total.get(k, 0) + v
    assert len(total) == 8 and all(v > 0 for v in total.values()), total      # both paths of every read width and of the store occurred


@pytest.mark.parametrize("form", ("upload", "host"))
def test_geometry_sweep_from_the_host(rfd, det, form):
    """the first two rounds of batch sizes (1, 2, 31, 32 twice) with the planes at their drawn offsets and strides in host memory"""
    for i, (frames, wants, sgeo, ogeo) in enumerate(_sweep()[:8]):
        _run(rfd, det, frames, wants, form, "sweep batch %d of %d frames" % (i, len(frames)), src_geo=sgeo, out_geo=ogeo)


# ---- the largest sizes ----
@pytest.mark.parametrize("fmt,w,h", [(FR.NV12, 1920, 1080), (FR.I420, 3840, 2160)])
def test_a_whole_large_frame(rfd, det, fmt, w, h):
    rng = np.random.default_rng(w)
    f = (fmt, w, h, FR.random_planes(rng, fmt, w, h), FR.BT709_LIMITED)
    _run(rfd, det, [f], [FR.convert_frame(f)], "device", "%s %d x %d" % (FR.NAMES[fmt], w, h))


def test_a_frame_whose_rows_lie_past_2_31_bytes(rfd, det):
    """NV12, 16 x 2160, with 1100000 bytes between the rows of the luma plane and of the output frame: from row 1953 on the
    offsets of both exceed 2^31"""
    import torch
    w, h, stride = 16, 2160, 1100000
    size = (h - 1) * stride + 3 * w
    assert size > 2 ** 31
    free = torch.cuda.mem_get_info()[0]
    if free < 4 * size:
        pytest.skip("the device has %.1f GB free, the test needs three buffers of %.1f GB" % (free / 1e9, size / 1e9))
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(7)
    planes = FR.random_planes(rng, FR.NV12, w, h)
    want = FR.convert(FR.NV12, w, h, planes, FR.BT601_FULL)
    luma = torch.full((size,), SRC_FILL, dtype=torch.uint8, device=dev)
    luma.as_strided((h, w), (stride, 1)).copy_(torch.from_numpy(planes[0]).to(dev))
    chroma = torch.from_numpy(planes[1]).to(dev)
    out = torch.full((size,), FILL, dtype=torch.uint8, device=dev)
    expect = torch.full((size,), FILL, dtype=torch.uint8, device=dev)
    expect.as_strided((h, 3 * w), (stride, 1)).copy_(torch.from_numpy(want.reshape(h, 3 * w)).to(dev))
    torch.cuda.synchronize()
    f = rfd.frame(FR.NV12, w, h, [luma.data_ptr(), chroma.data_ptr()], [stride, w], FR.BT601_FULL)
    det.convert_frames_device([f], [out.data_ptr()], [stride])
    assert torch.equal(out.as_strided((h, 3 * w), (stride, 1)), expect.as_strided((h, 3 * w), (stride, 1)))   # the rows, for the message
    assert torch.equal(out, expect)                                                                        # and every byte between them


# ---- the three forms agree; staging reuse ----
def _small_batch(seed, n=6):
    rng = np.random.default_rng(seed)
    frames = []
    for i in range(n):
        fmt, w, h = int(rng.integers(0, 10)), int(rng.integers(1, 200)), int(rng.integers(1, 120))
        frames.append((fmt, w, h, FR.random_planes(rng, fmt, w, h), int(rng.integers(0, 4))))
    return frames, [FR.convert_frame(f) for f in frames]


@pytest.mark.parametrize("pinned", (False, True))
def test_upload_from_pageable_and_from_page_locked_memory(rfd, det, pinned):
    frames, wants = _small_batch(11)
    geo = [[(1, 3)] * 3] * len(frames)
    up = _run(rfd, det, frames, wants, "upload", "upload", src_geo=geo, pinned=pinned)
    for form in ("device", "host"):
        assert _run(rfd, det, frames, wants, form, form, src_geo=geo).got().tobytes() == up.got().tobytes()


def test_two_asynchronous_uploads_back_to_back(rfd, det):
    """the second call's copies into the staging follow the first call's kernel in stream order: no wait between them"""
    a = Batch(rfd, det, *_small_batch(21, 9), "upload", pinned=True)
    b = Batch(rfd, det, *_small_batch(22, 5), "upload", pinned=True)
    assert a.call(async_=True) == 0 and b.call(async_=True) == 0, det._L.rfd_last_error()
    det.sync()
    a.check("the first upload")
    b.check("the second upload")
    a.close()
    b.close()


# ---- one stream order with the detector ----
def _detect_device(rfd, det, arr, n):
    import torch
    dev = torch.device("cuda", 0)
    md = det.max_det
    boxes, lmk = torch.zeros((n, md, 5), device=dev), torch.zeros((n, md, 10), device=dev)
    count, total = torch.zeros(n, dtype=torch.int32, device=dev), torch.zeros(n, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    out = rfd.rfd_dets(boxes.data_ptr(), lmk.data_ptr(), count.data_ptr(), total.data_ptr())
    return out, (boxes, lmk, count, total)


def _calibrate(det, frames):
    """synthetic weights and, as smoke() does, a threshold at a quantile of the scores, so that the slabs are not empty: the
    lowest of the frames' own 0.99 quantiles, so that about 1 % of the anchors pass in the frame that scores lowest"""
    det.init_synthetic_weights(1234)
    _, tn, _ = det.preprocess(frames)
    heads = det.forward(tn)
    fg = np.concatenate([heads[3 * l][:, 2:4].reshape(len(frames), -1) for l in range(3)], 1)
    det.set_thresholds(float(np.quantile(fg, 0.99, axis=1).min()), 0.45)


def _same_slabs(det, host, slabs):
    boxes, lmk, count, total = (t.cpu().numpy() for t in slabs)
    for b, (hb, hl) in enumerate(host):
        k = int(count[b])
        assert k == len(hb) > 0 and int(total[b]) == int(det.last_total[b])
        assert boxes[b, :k].tobytes() == hb.tobytes() and lmk[b, :k].tobytes() == hl.reshape(k, 10).tobytes(), b


def test_upload_then_detect_in_one_stream_order(rfd, det):
    """rfd_upload_frames_device (NV12, asynchronous) then rfd_detect_batch_device with no wait in between: the slabs of
    rfd_detect_batch on the BGR frames the restatement makes from the same planes, bit for bit"""
    import torch
    rng = np.random.default_rng(3)
    frames = [(FR.NV12, w, h, FR.random_planes(rng, FR.NV12, w, h), FR.BT601_LIMITED) for w, h in ((160, 120), (97, 131))]
    bgr = [FR.convert_frame(f) for f in frames]
    _calibrate(det, bgr)
    host = det.call_batch(bgr)
    b = Batch(rfd, det, frames, bgr, "upload", pinned=True)
    out, slabs = _detect_device(rfd, det, b.out, 2)
    assert b.call(async_=True) == 0, det._L.rfd_last_error()
    assert det._L.rfd_detect_batch_device(det._ctx, b.out, 2, C.byref(out), 0) == 0, det._L.rfd_last_error()
    _same_slabs(det, host, slabs)
    b.check("the uploaded frames")
    b.close()


def test_decoded_and_converted_frames_in_one_detect_call(rfd, det):
    """frame 0 decoded from a JPEG file on the device, frame 1 converted from I420 planes, both asynchronous, then one detect call"""
    import torch
    import jpeg_ref
    from test_jpeg_cpu import golden, load
    name = "64x48_420"
    jpeg_bgr = np.ascontiguousarray(jpeg_ref.to_bgr(golden(name)))
    rng = np.random.default_rng(4)
    f = (FR.I420, 75, 51, FR.random_planes(rng, FR.I420, 75, 51), FR.BT709_FULL)
    bgr = [jpeg_bgr, FR.convert_frame(f)]
    _calibrate(det, bgr)
    host = det.call_batch(bgr)
    b = Batch(rfd, det, [f], [bgr[1]], "device")
    decoded = torch.zeros((48, 64 * 3), dtype=torch.uint8, device=torch.device("cuda", 0))
    out, slabs = _detect_device(rfd, det, None, 2)
    arr = (rfd.rfd_image * 2)()
    arr[0] = det.decode_jpeg_device([load(name)], [decoded.data_ptr()], [(48, 64)], async_=True)[0]
    assert b.call(async_=True) == 0, det._L.rfd_last_error()
    arr[1] = b.out[0]
    assert det._L.rfd_detect_batch_device(det._ctx, arr, 2, C.byref(out), 0) == 0, det._L.rfd_last_error()
    _same_slabs(det, host, slabs)
    assert decoded.cpu().numpy().tobytes() == jpeg_bgr.tobytes()
    b.check("the converted frame")


# ---- refusals ----
def _mutations(rfd):
    """(name, frame it names, status, a word of the message, what to do to the batch)"""
    bad, cap = rfd.RFD_ERR_INVALID_ARG, rfd.RFD_ERR_CAPACITY

    def field(arr, name, value):
        return lambda b, i: setattr(getattr(b, arr)[i], name, value(getattr(getattr(b, arr)[i], name)))

    def element(name, k, value):
        def go(b, i):
            getattr(b.src[i], name)[k] = value(getattr(b.src[i], name)[k])
        return go

    def both(name, value):
        def go(b, i):
            setattr(b.src[i], name, value)
            setattr(b.out[i], name, value)
        return go

    return [
        ("output width differs", bad, b"the output frame is", field("out", "width", lambda v: v + 1)),
        ("output height differs", bad, b"the output frame is", field("out", "height", lambda v: v - 1)),
        ("output stride below 3 * width", bad, b"stride < 3 * width", field("out", "stride", lambda v: 3 * 24 - 1)),
        ("output data null", bad, b"data is null", field("out", "data", lambda v: None)),
        ("stride of plane 0 below its row", bad, b"stride", element("stride", 0, lambda v: 23)),
        ("stride of plane 1 below its row", bad, b"of plane 1", element("stride", 1, lambda v: 23)),
        ("plane 0 null", bad, b"plane 0", element("plane", 0, lambda v: None)),
        ("plane 1 null", bad, b"plane 1", element("plane", 1, lambda v: None)),
        ("unknown format", bad, b"unknown pixel format 10", field("src", "format", lambda v: 10)),
        ("negative format", bad, b"unknown pixel format -1", field("src", "format", lambda v: -1)),
        ("unknown colour", bad, b"unknown colour 4", field("src", "color", lambda v: 4)),
        ("reserved not zero", bad, b"reserved", element("reserved", 3, lambda v: 1)),
        ("zero width", bad, b"non-positive", both("width", 0)),
        ("wider than max_src_w", cap, b"exceeds max_src", both("width", 3841)),
        ("higher than max_src_h", cap, b"exceeds max_src", both("height", 2161)),
    ]


@pytest.mark.parametrize("form", FORMS)
def test_every_refusal_names_its_frame_and_writes_nothing(rfd, det, form):
    """three NV12 frames of 24 x 10; each refusal applied to each of them in turn: the status, "frame i" and the cause in
    rfd_last_error(), and every byte of the output buffer still the sentinel"""
    rng = np.random.default_rng(9)
    frames = [(FR.NV12, 24, 10, FR.random_planes(rng, FR.NV12, 24, 10), i) for i in range(3)]
    wants = [FR.convert_frame(f) for f in frames]
    L = det._L
    assert det.cfg.max_src_w == 3840 and det.cfg.max_src_h == 2160 and det.cfg.max_batch_size == MAX_BATCH
    for name, status, word, mutate in _mutations(rfd):
        for i in range(3):
            b = Batch(rfd, det, frames, wants, form)
            mutate(b, i)
            assert b.call(async_=True) == status, (name, i, L.rfd_last_error())
            msg = L.rfd_last_error()
            assert b"frame %d:" % i in msg and word in msg, (name, i, msg)
            det.sync()
            assert (b.got() == FILL).all(), (name, i)
    # n > max_batch_size: 33 times the same good frame
    b = Batch(rfd, det, frames[:1] * 33, wants[:1] * 33, form)
    assert b.call(async_=True) == rfd.RFD_ERR_CAPACITY and b"33" in L.rfd_last_error() and b"max_batch_size" in L.rfd_last_error()
    det.sync()
    assert (b.got() == FILL).all()
    # n = 0 is a no-op, whatever the pointers; n < 0 is not
    assert b.call(n=0) == 0 and (b.got() == FILL).all()
    for fn in (L.rfd_convert_frames_device, L.rfd_upload_frames_device):
        assert fn(det._ctx, None, 0, None, 0) == 0
    assert L.rfd_convert_frames(det._ctx, None, 0, None) == 0
    assert b.call(n=-1) == rfd.RFD_ERR_INVALID_ARG and L.rfd_convert_frames_device(det._ctx, None, 1, None, 0) == rfd.RFD_ERR_INVALID_ARG
    # and the untouched batch converts
    good = Batch(rfd, det, frames, wants, form)
    assert good.call() == 0
    good.check("the untouched batch")
