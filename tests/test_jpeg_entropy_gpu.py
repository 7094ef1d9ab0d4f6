"""Entropy decoding on the device (include/rfd.h, "entropy decoding on the device"; csrc/kernels_jpeg_entropy.hip): the kernel's
coefficients element for element, the pixels of DEVICE-mode calls byte for byte, the per-frame paths (so that no fallback can
stand in for the kernel), files libjpeg wrote, both modes on one context, and refusal: status and message string for string
as in HOST mode.  The files are those of tests/jpeg_entropy_cases.py, all of which tests/test_jpeg_entropy_cpu.py has run
through the same decoder on the host under the sanitizers."""
import io
import os

import numpy as np
import pytest

import jpeg_cases
import jpeg_entropy_cases
import jpeg_ref
from jpeg_entropy_cases import damaged, entries, entry, without_restarts
from test_jpeg_sweep_gpu import FILL, GUARD, decode_on_device, describe, detector

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "jpeg")
HOST, DEVICE, REFUSED = 0, 1, 2


def eligible():
    return [e for e in entries() if e.restart_interval <= jpeg_entropy_cases.MAX_INTERVAL]


@pytest.fixture(scope="module")
def mixed():
    """every eligible file, and behind every third one the same case without a restart interval"""
    out = []
    for k, e in enumerate(eligible()):
        out.append(e)
        if k % 3 == 0:
            out.append(without_restarts(e))
    return out


@pytest.fixture(scope="module")
def want(mixed):
    w = {}
    for e in mixed:
        if e.case not in w:
            w[e.case] = jpeg_cases.expected_bgr(e)
    return {e.name: w[e.case] for e in list(mixed) + list(entries())}


def paths_of(batch):
    return [DEVICE if e.restart_interval else HOST for e in batch]


def test_the_mode_switch(rfd):
    e = entry("restart_3@R3")
    with detector(rfd, 1, [e]) as det:
        assert det._L.rfd_set_jpeg_entropy(det._ctx, 2) == rfd.RFD_ERR_INVALID_ARG and det._L.rfd_set_jpeg_entropy(det._ctx, -1) == rfd.RFD_ERR_INVALID_ARG
        assert det.jpeg_last_paths() == []
        got = det.decode_jpeg([e.data])                                # HOST is the default: an eligible file stays on the host
        assert det.jpeg_last_paths() == [HOST] and np.array_equal(got[0], jpeg_cases.expected_bgr(e))
        det.set_jpeg_entropy("device")
        got = det.decode_jpeg([e.data])
        assert det.jpeg_last_paths() == [DEVICE] and np.array_equal(got[0], jpeg_cases.expected_bgr(e))
        det.set_jpeg_entropy("host")
        det.decode_jpeg([e.data])
        assert det.jpeg_last_paths() == [HOST]


def test_the_kernel_s_coefficients_equal_the_writer_s_and_the_host_decoder_s(rfd):
    files = eligible()
    with detector(rfd, 1, files) as det:
        for e in files:
            got = det.jpeg_coefficients_device(e.data)
            assert got.shape == e.coef.shape and np.array_equal(got, e.coef), "%s: %d coefficients differ" % (e.name, int((got != e.coef).sum()))
            assert np.array_equal(got, rfd.jpeg_coefficients(e.data)), e.name
        for data in (entry("geo_17x9_420@R65535").data, without_restarts(files[0]).data, {d.name: d for d in damaged()}["garbage"].data):
            with pytest.raises(rfd.RfdError) as err:                  # never a fallback: not eligible, or refused by the device
                det.jpeg_coefficients_device(data)
            assert err.value.status == rfd.RFD_ERR_UNSUPPORTED


def test_device_mode_pixels_and_paths_in_batches_of_1_2_5_and_16(rfd, mixed, want):
    sizes, k, step = [1, 2, 5, 16], 0, 0
    assert len({(e.width, e.height, e.sampling) for e in mixed[:16]}) > 4
    with detector(rfd, 16, mixed) as det:
        det.set_jpeg_entropy("device")
        while k < len(mixed):
            batch = mixed[k:k + sizes[step % 4]]
            decode_on_device(det, batch, want, k)
            assert det.jpeg_last_paths() == paths_of(batch), [e.name for e in batch]
            k, step = k + len(batch), step + 1
        assert step > 8
        for k in range(0, len(mixed), 16):                             # the host-output form
            batch = mixed[k:k + 16]
            got = det.decode_jpeg([e.data for e in batch])
            assert det.jpeg_last_paths() == paths_of(batch)
            for e, g in zip(batch, got):
                assert g.shape == want[e.name].shape and np.array_equal(g, want[e.name]), describe(e.name, g, want[e.name])


def test_the_libjpeg_fixture_with_a_restart_interval(rfd):
    with open(os.path.join(GOLDEN, "37x53_420_rst2.jpg"), "rb") as f:
        data = f.read()
    pixels = jpeg_ref.to_bgr(np.load(os.path.join(GOLDEN, "37x53_420_rst2.npz"))["pixels"])
    with detector(rfd, 1, [entry("restart_3@R3")]) as det:             # 77 x 61 holds 37 x 53
        det.set_jpeg_entropy("device")
        got = det.decode_jpeg([data])
        assert det.jpeg_last_paths() == [DEVICE] and np.array_equal(got[0], pixels)


def test_files_libjpeg_wrote(rfd):
    Image = pytest.importorskip("PIL.Image")
    rng = np.random.default_rng(7)
    files, pixels = [], []
    for w, h in ((37, 53), (64, 48), (203, 77)):
        img = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        img[:, :w // 2] = ((np.arange(h)[:, None, None] * 5 + np.arange(w // 2)[None, :, None] * 3) % 256).astype(np.uint8)
        for kw in (dict(restart_marker_blocks=1), dict(restart_marker_rows=1), dict(restart_marker_blocks=5)):
            for sampling in ("444", "422", "420", "GRAY"):
                for quality in (50, 95):
                    buf = io.BytesIO()
                    if sampling == "GRAY":
                        Image.fromarray(img).convert("L").save(buf, "JPEG", quality=quality, **kw)
                    else:
                        Image.fromarray(img).save(buf, "JPEG", quality=quality, subsampling={"444": 0, "422": 1, "420": 2}[sampling], **kw)
                    files.append(buf.getvalue())
                    pixels.append(jpeg_ref.to_bgr(np.asarray(Image.open(io.BytesIO(files[-1])))))
    assert len(files) == 72 and all(rfd.jpeg_info(f)["restart_interval"] > 0 for f in files)
    det = rfd.RetinaFaceDetection(max_batch_size=16, max_det=256, max_src=(203, 77))
    try:
        det.set_jpeg_entropy("device")
        for k in range(0, len(files), 16):
            got = det.decode_jpeg(files[k:k + 16])
            assert det.jpeg_last_paths() == [DEVICE] * len(got)
            for i, g in enumerate(got):
                assert g.shape == pixels[k + i].shape and np.array_equal(g, pixels[k + i]), describe("file %d" % (k + i), g, pixels[k + i])
    finally:
        det.close()


def arena_for(batch, fill=FILL):
    """one FILL-filled device buffer with a frame per file, GUARD bytes around each -> (tensor, offsets, strides)"""
    import torch
    at, place = GUARD, []
    for i, e in enumerate(batch):
        at += (i - at) % 4
        place.append((at, 3 * e.width + i % 3))
        at += e.height * place[-1][1] + GUARD
    t = torch.full((at,), fill, dtype=torch.uint8, device=torch.device("cuda", 0))
    torch.cuda.synchronize()
    return t, place


def frames_of(t, batch, place):
    got = t.cpu().numpy()
    return [np.lib.stride_tricks.as_strided(got[o:], (e.height, 3 * e.width), (s, 1)).reshape(e.height, e.width, 3).copy() for e, (o, s) in zip(batch, place)]


def enqueue(det, t, batch, place, async_):
    det.decode_jpeg_device([e.data for e in batch], [t.data_ptr() + o for o, s in place], [(e.height, e.width) for e in batch], [s for o, s in place], async_=async_)


def test_host_device_host_calls_back_to_back_without_a_sync(rfd, mixed, want):
    a, b, c = mixed[0:6], mixed[6:12], mixed[12:18]
    with detector(rfd, 6, a + b + c) as det:
        runs = []
        for mode, batch in (("host", a), ("device", b), ("host", c), ("device", a), ("device", c)):
            det.set_jpeg_entropy(mode)
            t, place = arena_for(batch)
            enqueue(det, t, batch, place, True)
            assert det.jpeg_last_paths() == (paths_of(batch) if mode == "device" else [HOST] * len(batch))
            runs.append((t, batch, place))
        det.sync()
        for t, batch, place in runs:
            for e, g in zip(batch, frames_of(t, batch, place)):
                assert np.array_equal(g, want[e.name]), describe(e.name, g, want[e.name])


def outcome(rfd, det, mode, batch):
    """(status, message, frames, paths) of one call in `mode`"""
    det.set_jpeg_entropy(mode)
    t, place = arena_for(batch)
    status, message = rfd.RFD_OK, ""
    try:
        enqueue(det, t, batch, place, False)
    except rfd.RfdError as e:
        status, message = e.status, e.message
    det.sync()
    return status, message, t.cpu().numpy(), frames_of(t, batch, place), det.jpeg_last_paths()


@pytest.mark.parametrize("k", range(5))
def test_a_damaged_file_gets_the_host_decoder_s_verdict_in_both_modes(rfd, want, k):
    d = damaged()[k]
    bad = d.base._replace(name=d.name, data=d.data)
    good = [entry("restart_1@R1"), entry("geo_33x17_422@R1")]
    with detector(rfd, 3, [d.base] + good) as det:
        for batch in ([bad], [good[0], bad, good[1]]):
            hs, hm, hraw, hframes, _ = outcome(rfd, det, "host", batch)
            ds, dm, draw, dframes, paths = outcome(rfd, det, "device", batch)
            assert (ds, dm) == (hs, hm), d.name
            assert (hs == rfd.RFD_OK) == d.host_accepts, (d.name, hs, hm)
            at = batch.index(bad)
            if d.host_accepts:
                assert paths[at] == REFUSED and all(p == DEVICE for i, p in enumerate(paths) if i != at)
                assert np.array_equal(draw, hraw)
                assert np.array_equal(dframes[at], want[d.base.name]), describe(d.name, dframes[at], want[d.base.name])
            else:
                assert ("file %d" % at) in dm
                assert (hraw == FILL).all() and (draw == FILL).all()   # a refused file refuses the whole call: no frame is written
        ok = outcome(rfd, det, "device", good)                         # and the context is as good as before
        assert ok[0] == rfd.RFD_OK and ok[4] == [DEVICE, DEVICE] and all(np.array_equal(g, want[e.name]) for e, g in zip(good, ok[3]))


def test_an_interval_above_the_cap_stays_on_the_host(rfd, want):
    e = jpeg_entropy_cases.over_the_cap()
    assert e.restart_interval == jpeg_entropy_cases.MAX_INTERVAL + 1 and rfd.jpeg_info(e.data)["restart_interval"] == e.restart_interval
    under = entry("restart_1@R1")
    with detector(rfd, 2, [e]) as det:
        det.set_jpeg_entropy("device")
        got = det.decode_jpeg([e.data, under.data])
        assert det.jpeg_last_paths() == [HOST, DEVICE]
        assert np.array_equal(got[0], want[under.name]) and np.array_equal(got[1], want[under.name])
