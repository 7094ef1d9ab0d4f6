"""The JPEG encode on the device (include/rfd.h, "JPEG encode": rfd_encode_jpeg_batch_device, rfd_encode_jpeg_batch and the two
test hooks) against the numpy restatement tests/jpeg_encode_ref.py, which tests/test_jpeg_encode_cpu.py holds to Pillow.  Every
comparison is of bytes.

The entropy workgroup packs kEncChunk = 256 blocks at a time.  1920 x 16 at 4:2:0 with one restart row is one interval of 120
MCUs = 720 blocks: two chunk boundaries inside the interval, both inside an MCU (256 and 512 are no multiples of 6), so the DC
prediction, the bit offset and a partial byte all cross a chunk.  200 x 150 without restart rows is one interval of 780 blocks."""
import io

import numpy as np
import pytest

import jpeg_encode_cases as EC
import jpeg_encode_ref as R

pytestmark = pytest.mark.gpu

MAX_BATCH = 40
FILL = 0xA5
SIZE_FILL = -7


@pytest.fixture(scope="module")
def det(rfd):
    d = rfd.RetinaFaceDetection(image_size=(128, 128), max_batch_size=MAX_BATCH, max_det=256)
    d.init_synthetic_weights(1234)
    yield d
    d.close()


def _device_encode(rfd, det, frames, cfg, slot_bytes, place=None, count=None, guard=64):
    """frames: [H, W, 3] u8 arrays.  place[i] = (offset, stride) of frame i in one device buffer of FILL bytes (default: tight,
    16-aligned).  -> (size [n] i32, slots [n, slot_bytes] u8, the guard bytes behind the last slot)"""
    import torch
    dev = torch.device("cuda", 0)
    n = len(frames)
    if place is None:
        place, at = [], 0
        for f in frames:
            place.append((at, f.shape[1] * 3))
            at = (at + f.shape[0] * f.shape[1] * 3 + 15) & ~15
    total = max(o + s * (f.shape[0] - 1) + f.shape[1] * 3 for (o, s), f in zip(place, frames))
    host = np.full(total, FILL, np.uint8)
    for (o, s), f in zip(place, frames):
        h, w = f.shape[:2]
        np.lib.stride_tricks.as_strided(host[o:], (h, w * 3), (s, 1))[...] = f.reshape(h, w * 3)
    src = torch.from_numpy(host).to(dev)
    out = torch.full((n * slot_bytes + guard,), FILL, dtype=torch.uint8, device=dev)
    size = torch.full((n,), SIZE_FILL, dtype=torch.int32, device=dev)
    cnt = None if count is None else torch.tensor([count], dtype=torch.int32, device=dev)
    torch.cuda.synchronize()                                   # the context's stream is not ordered with torch's
    det.encode_jpeg_device([src.data_ptr() + o for o, _ in place], [f.shape[:2] for f in frames], out.data_ptr(), slot_bytes, size.data_ptr(),
                           cfg=cfg, strides=[s for _, s in place], count_ptr=None if cnt is None else cnt.data_ptr(), async_=True)
    det.sync()
    o = out.cpu().numpy()
    return size.cpu().numpy(), o[:n * slot_bytes].reshape(n, slot_bytes), o[n * slot_bytes:]


def _check_slots(size, slots, guard, want):
    """want[i]: the expected file, or None for a slot that must be untouched (its size is then not looked at here)"""
    assert (guard == FILL).all()
    for i, w in enumerate(want):
        if w is None:
            assert (slots[i] == FILL).all(), i
            continue
        assert size[i] == len(w), (i, size[i], len(w))
        assert slots[i, :len(w)].tobytes() == w, i
        assert (slots[i, len(w):] == FILL).all(), i


# ---- 1. the sweep, both forms ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("restart", EC.RESTARTS)
@pytest.mark.parametrize("sampling", EC.SAMPLINGS, ids=lambda s: EC.SAMPLING_NAMES[s])
@pytest.mark.parametrize("form", ["device", "host"])
def test_the_sweep_equals_the_restatement(rfd, det, form, sampling, restart):
    cases = EC.sweep(sampling, restart)
    for q in EC.QUALITIES:
        cfg = rfd.jpeg_encode_config(q, sampling, restart)
        batch = [(h, w, c) for (h, w, c, qq) in cases if qq == q]
        assert len(batch) <= MAX_BATCH
        frames = [np.ascontiguousarray(EC.image(h, w, c)) for h, w, c in batch]
        want = [EC.expected(h, w, c, q, sampling, restart) for h, w, c in batch]
        slot = max(len(x) for x in want) + 5
        if form == "device":
            _check_slots(*_device_encode(rfd, det, frames, cfg, slot), want)
        else:
            got = det.encode_jpeg(frames, cfg, slot_bytes=slot)
            assert [len(g) for g in got] == [len(x) for x in want] and got == want, q


# ---- 2. the entry forms ------------------------------------------------------------------------------------------------------
def test_sixteen_images_of_mixed_sizes_offsets_and_strides(rfd, det):
    """one call: every data offset 0 .. 3 modulo 4, odd strides, and a rectangle inside a larger frame"""
    cfg = rfd.jpeg_encode_config(90, R.S420, 1)
    sizes = EC.GEOMETRIES + [(150, 200), (33, 64), (64, 31), (5, 100)]
    frames = [np.ascontiguousarray(EC.image(h, w, EC.CONTENTS[i % 3], seed=1)) for i, (h, w) in enumerate(sizes)]
    big = np.ascontiguousarray(EC.image(120, 160, "noise", seed=2))
    frames.append(np.ascontiguousarray(big[17:17 + 50, 23:23 + 77]))     # the rectangle, as pixels
    assert len(frames) == 16
    place, at = [], 0
    for i, f in enumerate(frames[:-1]):
        h, w = f.shape[:2]
        stride = 3 * w + [0, 1, 5, 7][(i // 4) % 4]
        at = ((at + 3) & ~3) + i % 4
        place.append((at, stride))
        at += stride * h
    at = (at + 3) & ~3
    base = at
    place.append((base + 17 * 480 + 23 * 3, 480))                        # ... and as a pointer into the frame with its stride
    want = [R.encode(f, 90, R.S420, 1) for f in frames]
    # the helper writes only the rectangle's own bytes; the frame around it stays FILL, which the encoder must not care about
    assert {p[0] % 4 for p in place} == {0, 1, 2, 3} and any(p[1] % 2 for p in place)
    _check_slots(*_device_encode(rfd, det, frames, cfg, max(len(w) for w in want) + 9, place=place), want)


@pytest.mark.parametrize("count", [0, 3, 11])
def test_count_on_the_device(rfd, det, count):
    """images at and past *count_dev: slots untouched, size 0; a count above n takes all"""
    cfg = rfd.jpeg_encode_config(75, R.S422, 1)
    frames = [np.ascontiguousarray(EC.image(h, w, "noise", seed=3)) for h, w in EC.GEOMETRIES[3:11]]
    want = [R.encode(f, 75, R.S422, 1) if i < count else None for i, f in enumerate(frames)]
    size, slots, guard = _device_encode(rfd, det, frames, cfg, 12288, count=count)
    _check_slots(size, slots, guard, want)
    assert (size[min(count, 8):] == 0).all()


def test_capacity_one_byte_short_and_exact(rfd, det):
    cfg = rfd.jpeg_encode_config(90, R.S444, 1)
    frames = [np.ascontiguousarray(EC.image(37, 53, "noise")), np.ascontiguousarray(EC.image(37, 53, "ramp"))]
    want = [R.encode(f, 90, R.S444, 1) for f in frames]
    long, short = (0, 1) if len(want[0]) > len(want[1]) else (1, 0)
    assert len(want[long]) > len(want[short])
    size, slots, guard = _device_encode(rfd, det, frames, cfg, len(want[long]))          # exact: both fit
    _check_slots(size, slots, guard, want)
    size, slots, guard = _device_encode(rfd, det, frames, cfg, len(want[long]) - 1)      # one byte short: the longer one does not
    assert size[long] == -1
    _check_slots(size, slots, guard, [None if i == long else w for i, w in enumerate(want)])
    got = det.encode_jpeg(frames, cfg, slot_bytes=len(want[long]) - 1)
    assert got[long] is None and got[short] == want[short]


@pytest.mark.parametrize("h,w,sampling,restart", [(150, 200, R.S420, 0), (150, 200, R.S420, 1), (16, 1920, R.S420, 1), (16, 1920, R.S444, 0), (16, 1920, R.GRAY, 1)])
def test_intervals_longer_than_a_chunk(rfd, det, h, w, sampling, restart):
    frames = [np.ascontiguousarray(EC.image(h, w, "noise")), np.ascontiguousarray(EC.image(h, w, "ramp"))]
    want = [R.encode(f, 90, sampling, restart) for f in frames]
    cfg = rfd.jpeg_encode_config(90, sampling, restart)
    _check_slots(*_device_encode(rfd, det, frames, cfg, max(len(x) for x in want) + 3), want)


# ---- 3. the entropy stage alone, on constructed coefficients -------------------------------------------------------------------
def _entropy_case(rfd, det, zz, width, height, sampling, restart, quality=75):
    coef = EC.natural(zz)
    cfg = rfd.jpeg_encode_config(quality, sampling, restart)
    want = R.file_from_blocks(coef, width, height, quality, sampling, restart)
    got = det.jpeg_encode_coefficients(coef, width, height, cfg)
    assert got == want, (len(got), len(want))
    assert det.jpeg_encode_coefficients(coef, width, height, cfg, cap=len(want)) == want
    assert det.jpeg_encode_coefficients(coef, width, height, cfg, cap=len(want) - 1) is None
    return want


@pytest.mark.parametrize("restart", [0, 1])
def test_a_lone_coefficient_at_every_zigzag_position(rfd, det, restart):
    _entropy_case(rfd, det, *EC.lone_coefficients(), restart)


@pytest.mark.parametrize("restart", [0, 1])
def test_zero_runs_and_the_largest_symbols(rfd, det, restart):
    zz, w, h, s = EC.zero_runs()
    assert [int(np.flatnonzero(zz[b, 1:])[0]) for b in range(5)] == [15, 16, 17, 32, 62] and zz[4, 63] != 0
    assert list(np.diff(zz[4:7, 0].astype(int))) == [-2047, 2047] and zz[5, 1] == -1023 and zz[5, 2] == 1023
    _entropy_case(rfd, det, zz, w, h, s, restart)


def test_ff_bytes_in_single_mcu_intervals_and_the_rst_wrap(rfd, det):
    f = EC.ff_blocks()
    data, n = EC.interval_bytes(f["middle"])
    assert 0xff in data[:-1]
    data, n = EC.interval_bytes(f["last_data"])
    assert n % 8 == 0 and data[-1] == 0xff
    data, n = EC.interval_bytes(f["pad"])
    assert n % 8 != 0 and data[-1] == 0xff
    data, n = EC.interval_bytes(f["exact"])
    assert n % 8 == 0 and data[-1] != 0xff
    zz, w, h, s = EC.single_mcu_intervals()
    want = _entropy_case(rfd, det, zz, w, h, s, 1)
    scan = R.scan_of(want)
    assert [scan[i + 1] for i in range(len(scan) - 1) if scan[i] == 0xff and 0xd0 <= scan[i + 1] <= 0xd7] == [0xd0 + i % 8 for i in range(11)]
    assert b"\xff\x00\xff\xd0" in scan or any(bytes([0xff, 0, 0xff, 0xd0 + k]) in scan for k in range(8))   # a stuffed FF right in front of a marker


@pytest.mark.parametrize("sampling,restart", [(R.S444, 1), (R.S422, 2), (R.S420, 1), (R.S420, 0)])
def test_random_coefficients_of_colour_files(rfd, det, sampling, restart):
    """53 x 37: dummy blocks' positions in the MCU order, three components, two tables; 300 x 40 at 4:2:0 is 342 blocks"""
    for (w, h) in [(53, 37), (300, 40)]:
        coef = EC.colour_blocks(w, h, sampling, seed=w + sampling)
        cfg = rfd.jpeg_encode_config(50, sampling, restart)
        assert det.jpeg_encode_coefficients(coef, w, h, cfg) == R.file_from_blocks(coef, w, h, 50, sampling, restart)


def test_coefficients_the_tables_cannot_code_are_refused(rfd, det):
    cfg = rfd.jpeg_encode_config(50, R.GRAY, 0)
    for pos, v in [(1, 1024), (63, -1024), (0, 1024), (0, -1025)]:
        coef = np.zeros((1, 64), np.int16)
        coef[0, pos] = v
        with pytest.raises(rfd.RfdError) as e:
            det.jpeg_encode_coefficients(coef, 8, 8, cfg)
        assert e.value.status == rfd.RFD_ERR_INVALID_ARG
    with pytest.raises(rfd.RfdError) as e:
        det.jpeg_encode_coefficients(np.zeros((2, 64), np.int16), 8, 8, cfg)
    assert e.value.status == rfd.RFD_ERR_INVALID_ARG and "blocks" in e.value.message


# ---- 4. the front half alone -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sampling", EC.SAMPLINGS, ids=lambda s: EC.SAMPLING_NAMES[s])
def test_the_blocks_equal_the_restatement(rfd, det, sampling):
    for (h, w) in EC.GEOMETRIES:
        for c in EC.CONTENTS:
            for q in (1, 90, 100):
                img = np.ascontiguousarray(EC.image(h, w, c))
                got = det.jpeg_encode_blocks(img, rfd.jpeg_encode_config(q, sampling, 0))
                want = R.blocks(img, q, sampling)
                assert got.shape == want.shape and np.array_equal(got, want), (h, w, c, q)


# ---- 5. with the rest of the pipeline ----------------------------------------------------------------------------------------------
def test_round_trip_through_the_device_entropy_decoder(rfd, det):
    """encode on the device, then the device entropy decoder on the files it wrote (they have restart intervals, so they are
    eligible): the frames equal Pillow's decode of the same bytes"""
    import torch
    from PIL import Image
    shapes = [(37, 53), (112, 112), (150, 200)]
    frames = [np.ascontiguousarray(EC.image(h, w, "ramp" if i else "noise", seed=5)) for i, (h, w) in enumerate(shapes)]
    cfg = rfd.jpeg_encode_config(90, R.S420, 1)
    size, slots, guard = _device_encode(rfd, det, frames, cfg, 1 << 16)
    files = [slots[i, :size[i]].tobytes() for i in range(3)]
    assert all(s > 0 for s in size) and files == [R.encode(f, 90, R.S420, 1) for f in frames]
    dev = torch.device("cuda", 0)
    outs = [torch.full((h, w * 3), FILL, dtype=torch.uint8, device=dev) for h, w in shapes]
    torch.cuda.synchronize()
    det.set_jpeg_entropy("device")
    try:
        det.decode_jpeg_device(files, [o.data_ptr() for o in outs], shapes)
        assert list(det.jpeg_last_paths()) == [rfd.JPEG_PATH_DEVICE] * 3
    finally:
        det.set_jpeg_entropy("host")
    for f, o, (h, w) in zip(files, outs, shapes):
        want = np.asarray(Image.open(io.BytesIO(f)).convert("RGB"))[..., ::-1]
        assert np.array_equal(o.cpu().numpy().reshape(h, w, 3), want)


def test_detect_all_faces_then_encode_their_crops_in_one_stream_order(rfd, det):
    """rfd_detect_all_faces_device, then the encode of `crops` with `total` as count_dev, both enqueued before one sync"""
    import torch
    import helpers
    frames = [helpers.make_image(500 + i, 240, 320, n_blobs=6) for i in range(2)]
    _, tn, _ = det.preprocess(frames)
    heads = det.forward(tn)
    fg = np.concatenate([heads[3 * l][:, 2:4].reshape(2, -1) for l in range(3)], 1)
    det.set_thresholds(float(np.quantile(fg, 0.98)), 0.45)
    cap = 12
    lc = rfd.face_list_config(max_faces=4)
    dev = torch.device("cuda", 0)
    bufs = [torch.from_numpy(np.ascontiguousarray(f)).to(dev) for f in frames]
    i32 = lambda *shape: torch.zeros(shape, dtype=torch.int32, device=dev)
    total, first, frame, row, status = i32(1), i32(3), i32(cap), i32(cap), i32(cap)
    box, kps = torch.zeros((cap, 5), device=dev), torch.zeros((cap, 5, 2), device=dev)
    crops = torch.full((cap, 112, 112, 3), FILL, dtype=torch.uint8, device=dev)
    slot = 16384
    out = torch.full((cap * slot,), FILL, dtype=torch.uint8, device=dev)
    size = torch.full((cap,), SIZE_FILL, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    det.detect_all_faces_device([b.data_ptr() for b in bufs], [f.shape[:2] for f in frames], [], cap, total.data_ptr(), first.data_ptr(), frame.data_ptr(),
                                row.data_ptr(), box.data_ptr(), kps.data_ptr(), status.data_ptr(), crops.data_ptr(), [], list_cfg=lc, async_=True)
    cfg = rfd.jpeg_encode_config(90, R.S420, 0)
    det.encode_jpeg_device([crops.data_ptr() + t * 112 * 112 * 3 for t in range(cap)], [(112, 112)] * cap, out.data_ptr(), slot, size.data_ptr(), cfg=cfg,
                           count_ptr=total.data_ptr(), async_=True)
    det.sync()
    T = int(total.cpu().numpy()[0])
    assert 1 <= T < cap, T
    px, got, sz = crops.cpu().numpy(), out.cpu().numpy().reshape(cap, slot), size.cpu().numpy()
    want = [R.encode(px[t], 90, R.S420, 0) if t < T else None for t in range(cap)]
    _check_slots(sz, got, np.full(1, FILL, np.uint8), want)
    assert (sz[T:] == 0).all()


# ---- 6. argument errors that need a context -------------------------------------------------------------------------------------
def test_argument_errors_enqueue_nothing(rfd, det):
    import torch
    dev = torch.device("cuda", 0)
    src = torch.zeros(64 * 64 * 3, dtype=torch.uint8, device=dev)
    out = torch.full((4096,), FILL, dtype=torch.uint8, device=dev)
    size = torch.full((MAX_BATCH + 1,), SIZE_FILL, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    call = lambda shapes, strides=None, cfg=None: det.encode_jpeg_device([src.data_ptr()] * len(shapes), shapes, out.data_ptr(), 64, size.data_ptr(), cfg=cfg, strides=strides)
    for shapes, strides, word in [([(0, 8)], None, "height"), ([(8, 0)], None, "width"), ([(65536, 8)], None, "height"), ([(8, 65536)], None, "width"),
                                  ([(8, 8)], [23], "stride"), ([(8, 8), (8, 8)], [24, 23], "image 1")]:
        with pytest.raises(rfd.RfdError) as e:
            call(shapes, strides)
        assert e.value.status == rfd.RFD_ERR_INVALID_ARG and word in e.value.message, e.value.message
    with pytest.raises(rfd.RfdError) as e:
        call([(8, 8)] * (MAX_BATCH + 1))
    assert e.value.status == rfd.RFD_ERR_CAPACITY and "max_batch_size" in e.value.message
    with pytest.raises(rfd.RfdError) as e:                     # 65535 MCU rows of 1 MCU... one restart row of 8192 MCUs fits; 8 rows do not
        call([(64, 65535)], [65535 * 3], rfd.jpeg_encode_config(90, R.S444, 8))
    assert e.value.status == rfd.RFD_ERR_INVALID_ARG and "restart_rows" in e.value.message
    det.sync()
    assert (out.cpu().numpy() == FILL).all() and (size.cpu().numpy() == SIZE_FILL).all()
    call([])                                                   # n = 0 is a no-op
