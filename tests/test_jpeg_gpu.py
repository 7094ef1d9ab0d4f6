"""JPEG decode on the device (include/rfd.h, "JPEG decode": rfd_decode_jpeg_batch, rfd_decode_jpeg_batch_device) against the
pixels libjpeg-turbo (Pillow) decoded from the same files, stored under tests/golden/jpeg/.  The bar is byte equality
throughout: the contract is libjpeg's integer arithmetic, bit for bit.  tests/test_jpeg_cpu.py pins the host half and the
arithmetic without a GPU; here the two kernels, the batching, the staging and the hand-over to the detector are under test.
tests/test_jpeg_sweep_gpu.py sweeps the kernels over the geometries, tables and coefficients these 24 fixtures do not reach."""
import ctypes as C
import struct

import numpy as np
import pytest

import jpeg_ref
from test_jpeg_cpu import AC_EOB, DC0, DQT, EOI, SOI, SUPPORTED, dht, golden, load, seg, sof, sos

pytestmark = pytest.mark.gpu

MIXED = ["37x53_420", "1x1_444", "64x48_422", "17x9_GRAY", "8x8_420", "64x48_444", "37x53_420_rst2", "17x9_422"]   # 8 files, every sampling
FILL = 0xA5


@pytest.fixture(scope="module")
def det(rfd):
    d = rfd.RetinaFaceDetection(max_batch_size=8, max_det=256, max_src=(64, 64))   # the staging is sized by max_src and the batch
    yield d
    d.close()


@pytest.fixture(scope="module")
def want():
    """the golden pixels of every supported fixture as BGR frames, loaded once"""
    return {name: jpeg_ref.to_bgr(golden(name)) for name in SUPPORTED}


def device_frames(names, want, pad):
    """(torch buffers [h, stride] filled with FILL, pointers, shapes, strides) for the frames of `names`; pad(i, w) = extra bytes"""
    import torch
    dev = torch.device("cuda", 0)
    shapes = [want[n].shape[:2] for n in names]
    strides = [3 * w + pad(i, w) for i, (h, w) in enumerate(shapes)]
    bufs = [torch.full((h, s), FILL, dtype=torch.uint8, device=dev) for (h, w), s in zip(shapes, strides)]
    torch.cuda.synchronize()
    return bufs, [b.data_ptr() for b in bufs], shapes, strides


def check_frames(names, want, bufs, shapes):
    for n, b, (h, w) in zip(names, bufs, shapes):
        got = b.cpu().numpy()
        assert np.array_equal(got[:, :3 * w].reshape(h, w, 3), want[n]), n
        assert (got[:, 3 * w:] == FILL).all(), "%s: the stride padding was written" % n


@pytest.mark.parametrize("name", SUPPORTED)
def test_every_fixture_decodes_to_the_golden_pixels(det, want, name):
    got = det.decode_jpeg([load(name)])
    assert len(got) == 1 and got[0].dtype == np.uint8 and got[0].shape == want[name].shape
    diff = got[0] != want[name]
    assert not diff.any(), "%s: %d of %d pixels differ, first at %s" % (name, int(diff.any(-1).sum()), diff.shape[0] * diff.shape[1], np.argwhere(diff.any(-1))[:1].tolist())


def test_a_mixed_batch_on_the_device_leaves_the_stride_padding_alone(det, want):
    # odd paddings take the byte stores (rows are not 4-byte aligned), paddings that round the row to a multiple of 4 the word stores
    bufs, ptrs, shapes, strides = device_frames(MIXED, want, lambda i, w: 5 if i % 2 else (-3 * w) % 4 + 8)
    assert all(s > 3 * w for s, (h, w) in zip(strides, shapes))
    assert {s % 4 for s in strides} >= {0} and any(s % 4 for s in strides)
    det.decode_jpeg_device([load(n) for n in MIXED], ptrs, shapes, strides)
    check_frames(MIXED, want, bufs, shapes)


def test_results_do_not_depend_on_the_thread_count_or_the_position_in_the_batch(det, want):
    files = [load(n) for n in MIXED]
    det.set_decode_threads(1)
    one = det.decode_jpeg(files)
    det.set_decode_threads(4)
    four = det.decode_jpeg(files[::-1])[::-1]
    alone = det.decode_jpeg(files[2:3])[0]
    for n, a, b in zip(MIXED, one, four):
        assert np.array_equal(a, want[n]) and np.array_equal(b, want[n]), n
    assert np.array_equal(alone, want[MIXED[2]])
    for t in (0, 17, -1):
        assert det._L.rfd_set_decode_threads(det._ctx, t) == -1        # RFD_ERR_INVALID_ARG; the count stays 4


def test_two_async_calls_back_to_back_reuse_the_staging_safely(det, want):
    """Two asynchronous calls, then one rfd_sync: both outputs are exact.  This pins the RESULT of the staging-reuse rule, it is no
    race detector: the first call's copies are a few KB and have long run when the second call's threads write the staging, so
    the test would most likely pass without the wait too.  The rule itself is in the code: rfd_decode_jpeg_batch* waits on the
    event recorded behind the previous call's last copy before any worker thread starts."""
    first, second = MIXED[:5], ["64x48_420", "37x53_420_q100", "37x53_444", "64x48_GRAY", "37x53_420_q5", "8x8_GRAY"]
    b1, p1, s1, st1 = device_frames(first, want, lambda i, w: 4 + (-3 * w) % 4)
    b2, p2, s2, st2 = device_frames(second, want, lambda i, w: 7)
    det.decode_jpeg_device([load(n) for n in first], p1, s1, st1, async_=True)
    det.decode_jpeg_device([load(n) for n in second], p2, s2, st2, async_=True)
    det.sync()
    check_frames(first, want, b1, s1)
    check_frames(second, want, b2, s2)


def test_a_truncated_file_refuses_the_whole_batch_and_enqueues_nothing(det, rfd, want):
    names = ["8x8_444", "17x9_420", "37x53_420", "64x48_GRAY"]
    files = [load(n) for n in names]
    scan = files[2].index(b"\xff\xda")
    broken = files[:2] + [files[2][:scan + 60]] + files[3:]
    bufs, ptrs, shapes, strides = device_frames(names, want, lambda i, w: 6)
    with pytest.raises(rfd.RfdError) as e:
        det.decode_jpeg_device(broken, ptrs, shapes, strides)
    assert e.value.status == rfd.RFD_ERR_INVALID_ARG and "file 2" in str(e.value) and "truncated" in str(e.value)
    det.sync()
    for b in bufs:
        assert (b.cpu().numpy() == FILL).all()                         # no frame of the call was touched
    det.decode_jpeg_device(files, ptrs, shapes, strides)               # and the context is as good as before
    check_frames(names, want, bufs, shapes)


def test_argument_and_capacity_errors(det, rfd, want):
    L, data = det._L, load("8x8_444")
    assert L.rfd_decode_jpeg_batch(det._ctx, None, None, 0, None) == 0                    # n = 0 is a no-op
    assert L.rfd_decode_jpeg_batch_device(det._ctx, None, None, 0, None, 1) == 0
    with pytest.raises(rfd.RfdError) as e:
        det.decode_jpeg([data] * 9)
    assert e.value.status == rfd.RFD_ERR_CAPACITY and "max_batch_size" in str(e.value)
    wide = SOI + DQT + sof(w=72) + DC0 + AC_EOB + sos() + b"\x00" * 2 + EOI               # wider than max_src_w = 64
    with pytest.raises(rfd.RfdError) as e:
        det.decode_jpeg([wide])
    assert e.value.status == rfd.RFD_ERR_CAPACITY and "max_src" in str(e.value)
    bufs, ptrs, shapes, strides = device_frames(["8x8_444"], want, lambda i, w: 0)
    for shp, st in (((8, 9), [27]), ((9, 8), [24]), ((8, 8), [23])):                         # wrong width, wrong height, short stride
        with pytest.raises(rfd.RfdError) as e:
            det.decode_jpeg_device([data], ptrs, [shp], st)
        assert e.value.status == rfd.RFD_ERR_INVALID_ARG
    with pytest.raises(rfd.RfdError) as e:
        det.decode_jpeg([load("37x53_420_progressive")])
    assert e.value.status == rfd.RFD_ERR_UNSUPPORTED and "file 0" in str(e.value)
    with pytest.raises(rfd.RfdError) as e:                             # the library's own batch call names the file too
        det.decode_jpeg_device([data, load("37x53_420_progressive")], ptrs * 2, [(8, 8), (53, 37)], [24, 111])
    assert e.value.status == rfd.RFD_ERR_UNSUPPORTED and "file 1" in str(e.value) and "progressive" in str(e.value)


def test_hostile_coefficients_decode_without_a_fault(det):
    """Well-formed, but no 8-bit image produces it: a 16-bit quantisation table of 65535s and 64 coefficients of 15 magnitude
    bits each, +32767 and -32767 in turn.  The IDCT's sums leave 32 bits; the pixels are not pinned (rfd.h), the call succeeds
    and the next one is exact."""
    unit = [b"\x7f\xff\x00", b"\x00\x00"]                                                 # code 0 + 0x7fff (stuffed) / code 0 + fifteen 0 bits
    data = SOI + seg(0xdb, bytes([0x10]) + struct.pack(">64H", *([65535] * 64))) + sof() + dht(0, 0, 15) + dht(1, 0, 0x0f) + sos() + \
        b"".join(unit[k % 2] for k in range(64)) + EOI
    got = det.decode_jpeg([data])[0]
    assert got.shape == (8, 8, 3) and (got[..., 0] == got[..., 1]).all()
    assert np.array_equal(det.decode_jpeg([load("8x8_420")])[0], jpeg_ref.to_bgr(golden("8x8_420")))


def test_decoded_device_frames_feed_the_detector(rfd, want):
    """Hand-over: a file decoded on the device, the same rfd_image array passed to rfd_detect_batch_device, against
    rfd_detect_batch on the golden pixels from the host: identical detections."""
    import torch
    name = "64x48_420"
    d = rfd.RetinaFaceDetection(max_batch_size=1, max_det=256, max_src=(64, 48))
    try:
        d.init_synthetic_weights(1234)
        frame = np.ascontiguousarray(want[name])
        _, tn, _ = d.preprocess([frame])
        heads = d.forward(tn)
        fg = np.concatenate([heads[3 * l][:, 2:4].reshape(1, -1) for l in range(3)], 1)
        d.set_thresholds(float(np.quantile(fg, 0.99)), 0.45)                              # the smoke test's calibration: about 1 % of the anchors pass
        host = d.call_batch([frame])[0]
        assert len(host[0]) > 0
        dev = torch.device("cuda", 0)
        buf = torch.zeros((48, 64 * 3), dtype=torch.uint8, device=dev)
        boxes, lmk = torch.zeros((1, 256, 5), device=dev), torch.zeros((1, 256, 10), device=dev)
        count, total = torch.zeros(1, dtype=torch.int32, device=dev), torch.zeros(1, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        arr = d.decode_jpeg_device([load(name)], [buf.data_ptr()], [(48, 64)], async_=True)
        out = rfd.rfd_dets(boxes.data_ptr(), lmk.data_ptr(), count.data_ptr(), total.data_ptr())
        assert d._L.rfd_detect_batch_device(d._ctx, arr, 1, C.byref(out), 0) == 0, d._L.rfd_last_error()
        k = int(count.cpu()[0])
        assert k == len(host[0]) and int(total.cpu()[0]) == int(d.last_total[0])
        assert np.array_equal(boxes.cpu().numpy()[0, :k], host[0])
        assert np.array_equal(lmk.cpu().numpy()[0, :k].reshape(k, 5, 2), host[1])
    finally:
        d.close()
