"""The reduced-size JPEG decode on the device (include/rfd.h, "JPEG decode, reduced size"): jpeg_idct_reduced_kernel and the two
colour kernels of scaled frames (csrc/kernels_jpeg.hip), and the host layer that sizes, places and launches them.  Every file is
written at test time (tests/jpeg_scaled_cases.py).

Expected pixels everywhere: jpeg_scaled_ref.decode_scaled, which tests/test_jpeg_scaled_cpu.py pins to libjpeg-turbo through
Pillow's draft mode on these very files, followed where a file is tagged by jpeg_exif.orient.  The bar is byte equality, and that
every byte of the output buffer outside the pixels still holds its sentinel (decode_on_device of the orientation tests)."""
import ctypes as C
import io
import os

import numpy as np
import pytest

import jpeg_cases
import jpeg_scaled_cases
from jpeg_cases import SAMPLING_NAME, SAMPLINGS
from jpeg_exif import app1, orient, tagged
from jpeg_ref import GRAY, S420, S422, S444, to_bgr
from jpeg_scaled_cases import DENOMS, expected_bgr, sparse
from jpeg_scaled_ref import scaled_size
from test_jpeg_orientation_gpu import FILL, T, decode_on_device

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "jpeg")
ODD_SCALED = (37, 23)                                  # the output-contract test's SCALED size
TILE_SCALED = [(T - 1, 5), (T, 3), (T + 1, 9), (2 * T + 3, 2)]   # scaled sizes around the oriented kernel's tile, thin in the other direction


def stored_of(scaled, s):
    """a stored size whose scaled size is `scaled` and no multiple of s"""
    return tuple(v * s - s // 2 for v in scaled)


@pytest.fixture(scope="module")
def stock():
    """{key: Case} of everything beyond the geometry list, built once"""
    rng = np.random.default_rng(20250925)
    out = {}
    for s in DENOMS:
        for sampling in SAMPLINGS:
            for scaled in [ODD_SCALED] + TILE_SCALED:
                w, h = stored_of(scaled, s)
                assert scaled_size(w, h, s) == scaled
                out[w, h, sampling] = sparse(rng, "edge_%dx%d_%s" % (w, h, SAMPLING_NAME[sampling]), w, h, sampling)
    for w, h, sampling, ri in ((80, 64, S420, 1), (77, 61, S420, 3), (45, 60, S422, 2), (33, 31, GRAY, 1), (40, 24, S444, 2)):
        out["restart", w, h] = sparse(rng, "restart_%dx%d" % (w, h), w, h, sampling, restart_interval=ri)
    out["hand_over"] = sparse(rng, "hand_over", 191, 127, S420)
    out["plain", S420], out["plain", S422] = sparse(rng, "plain_420", 17, 9, S420), sparse(rng, "plain_422", 17, 9, S422)
    return out


def tag(case, o):
    return case.data if o in (None, 1) else tagged(case.data, app1(value=o, entries=3, position=1))


def detector(rfd, batch, max_src, s, orientation="ignore"):
    d = rfd.RetinaFaceDetection(max_batch_size=batch, max_det=256, max_src=max_src)
    d.set_jpeg_scale(s)
    d.set_jpeg_orientation(orientation)
    return d


@pytest.mark.parametrize("s", DENOMS)
def test_every_sampling_and_geometry_in_mixed_batches_of_16(rfd, s):
    """4 samplings x the sizes of jpeg_scaled_cases.sizes_of(s) (30 at 1/2, 45 at 1/4 and 1/8), shuffled, 16 per call: inverse-DCT
    sizes n and 2 n, all four samplings, plane pitches that are no multiple of 4 and scaled sizes of 1 and 2 pixels in one launch,
    at every base alignment and stride class"""
    cases = jpeg_scaled_cases.geometry()
    keys = [(w, h, sampling) for sampling in SAMPLINGS for w, h in jpeg_scaled_cases.sizes_of(s)]
    assert len(set(keys)) == len(keys) >= 120 and {1, 2 if s > 2 else 1} <= {scaled_size(w, h, s)[0] for w, h, _ in keys}   # no width scales to 2 at 1/2
    order = np.random.default_rng(s).permutation(len(keys))
    d = detector(rfd, 16, (16 * s + 1, 16 * s + 1), s)
    try:
        for k in range(0, len(keys), 16):
            batch = [cases[keys[i]] for i in order[k:k + 16]]
            decode_on_device(d, [c.data for c in batch], [expected_bgr(c, s) for c in batch], k0=k)
            assert d.jpeg_last_paths() == [0] * len(batch) and d.jpeg_last_orientations() == [1] * len(batch)
    finally:
        d.close()


@pytest.mark.parametrize("s", DENOMS)
def test_the_output_contract_at_every_base_alignment_and_stride(rfd, stock, s):
    """an odd scaled size per sampling x base address offset 0 .. 3 x stride 3 * w + {0, 1, 5}: the pixels, and the sentinel in
    every pad byte of every row and in the guard in front of and behind every frame"""
    combos = [(sampling, base, pad) for sampling in SAMPLINGS for base in range(4) for pad in (0, 1, 5)]
    size = stored_of(ODD_SCALED, s)
    d = detector(rfd, 16, size, s)
    try:
        for k in range(0, len(combos), 16):
            part = combos[k:k + 16]
            batch = [stock[size + (sampling,)] for sampling, _, _ in part]
            expect = [expected_bgr(c, s) for c in batch]
            assert all(e.shape == ODD_SCALED[::-1] + (3,) for e in expect)
            decode_on_device(d, [c.data for c in batch], expect, place=lambda i, w: part[i - k][1:], k0=k)
    finally:
        d.close()


@pytest.mark.parametrize("o", range(1, 9))
def test_orientation_composes_with_scale(rfd, stock, o):
    """one orientation x 3 denominators x 4 samplings x scaled sizes of 63, 64, 65 and 2 * 64 + 3 pixels along the tile, 16 files
    per call: the stored image is scaled, then the index map is applied to the scaled image.  One file of each sampling is left
    untagged, a different size for each, so that both colour kernels run in every call and every size -- the three-tile one
    included -- goes through the oriented kernel in three samplings.  Every file is also judged by Pillow: draft, then
    ImageOps.exif_transpose."""
    Image = pytest.importorskip("PIL.Image")
    ImageOps = pytest.importorskip("PIL.ImageOps")
    for s in DENOMS:
        keys = [stored_of(scaled, s) + (sampling,) for sampling in SAMPLINGS for scaled in TILE_SCALED]
        d = detector(rfd, 16, stored_of((2 * T + 3, 9), s), s, "apply")
        try:
            tags = [None if i % 4 == i // 4 and o != 1 else o for i in range(16)]   # keys[i]: sampling i // 4, size i % 4
            for k in range(4):                                            # each size is tagged in three samplings, untagged in one
                assert [t for t in tags[k::4]].count(o) == (3 if o != 1 else 4)
            files = [tag(stock[key], t) for key, t in zip(keys, tags)]
            expect = [orient(expected_bgr(stock[key], s), t or 1) for key, t in zip(keys, tags)]
            for (w, h, _), data, e in zip(keys, files, expect):
                assert rfd.jpeg_scaled_size(data, s, "apply")["width"] == e.shape[1]
                im = Image.open(io.BytesIO(data))
                im.draft(im.mode, (w // s, h // s))
                assert im.size == scaled_size(w, h, s) and min(w, h) >= s
                assert np.array_equal(to_bgr(np.asarray(ImageOps.exif_transpose(im))), e), (w, h, s, o)
            decode_on_device(d, files, expect, k0=o)
            assert d.jpeg_last_orientations() == [t or 1 for t in tags]
        finally:
            d.close()


@pytest.mark.parametrize("s", DENOMS)
def test_restart_interval_files_on_both_entropy_paths(rfd, stock, s):
    cases = [stock[k] for k in stock if k[0] == "restart"] + [stock["plain", S420]]
    expect = [expected_bgr(c, s) for c in cases]
    d = detector(rfd, 8, (80, 64), s)
    try:
        on_host = decode_on_device(d, [c.data for c in cases], expect)
        assert d.jpeg_last_paths() == [0] * 6
        d.set_jpeg_entropy("device")
        on_device = decode_on_device(d, [c.data for c in cases], expect, k0=1)
        assert d.jpeg_last_paths() == [1] * 5 + [0]                       # the device took the five files with a restart interval
        assert all(np.array_equal(a, b) for a, b in zip(on_host, on_device))
    finally:
        d.close()


@pytest.mark.parametrize("s", (1,) + DENOMS)
def test_one_coefficient_at_each_position_through_the_kernels(rfd, s):
    grey, colour = jpeg_scaled_cases.single_coefficient()
    d = detector(rfd, 2, (128, 128), s)
    try:
        decode_on_device(d, [grey.data, colour.data], [expected_bgr(grey, s), expected_bgr(colour, s)])
    finally:
        d.close()


def test_the_stored_size_is_the_wrong_one_in_scaled_mode(rfd, stock):
    import torch
    s = 4
    size = stored_of(ODD_SCALED, s)
    case, other = stock[size + (S420,)], stock["plain", S422]
    d = detector(rfd, 4, size, s)
    try:
        for bad in (0, 3, 16, -1):
            assert d._L.rfd_set_jpeg_scale(d._ctx, bad) == rfd.RFD_ERR_INVALID_ARG
            with pytest.raises(rfd.RfdError):
                d.set_jpeg_scale(bad)
        shapes = [(3, 5), size[::-1], (3, 5)]                              # frame 1 in the stored size
        bufs = [torch.full(((h + 2) * 3 * w,), FILL, dtype=torch.uint8, device=torch.device("cuda", 0)) for h, w in shapes]
        torch.cuda.synchronize()
        with pytest.raises(rfd.RfdError) as e:
            d.decode_jpeg_device([other.data, case.data, other.data], [b.data_ptr() for b in bufs], shapes)
        assert e.value.status == rfd.RFD_ERR_INVALID_ARG and "frame 1" in str(e.value) and "1/4" in str(e.value)
        d.sync()
        for b in bufs:
            assert (b.cpu().numpy() == FILL).all()                         # no frame of the call was written
        with pytest.raises(rfd.RfdError) as e:                             # the scaled size, a stride one byte short of the scaled row
            d.decode_jpeg_device([case.data], [bufs[1].data_ptr()], [ODD_SCALED[::-1]], [3 * ODD_SCALED[0] - 1])
        assert e.value.status == rfd.RFD_ERR_INVALID_ARG and "stride" in str(e.value)
        assert (bufs[1].cpu().numpy() == FILL).all()
        decode_on_device(d, [other.data, case.data, other.data], [expected_bgr(c, s) for c in (other, case, other)])   # the context is as good as before
        # a file larger than max_src is refused by its STORED size, although its scaled frame would fit
        big = stock[stored_of(TILE_SCALED[3], s) + (GRAY,)]
        with pytest.raises(rfd.RfdError) as e:
            decode_on_device(d, [big.data], [expected_bgr(big, s)])
        assert e.value.status == rfd.RFD_ERR_CAPACITY
    finally:
        d.close()


def test_the_host_form_and_two_async_calls_with_different_denominators(rfd, stock):
    golden = ["64x48_420", "37x53_422", "17x9_444", "37x53_GRAY", "1x1_420"]
    files = [open(os.path.join(GOLDEN, n + ".jpg"), "rb").read() for n in golden]
    full = [to_bgr(np.load(os.path.join(GOLDEN, n + ".npz"))["pixels"]) for n in golden]
    cases = [stock[stored_of(ODD_SCALED, 4) + (sampling,)] for sampling in SAMPLINGS]
    d = detector(rfd, 8, stored_of(ODD_SCALED, 4), 4, "apply")
    try:
        tagged_files = [tag(c, o) for c, o in zip(cases, (6, None, 3, 8))]
        expect = [orient(expected_bgr(c, 4), o or 1) for c, o in zip(cases, (6, None, 3, 8))]
        on_host = d.decode_jpeg(tagged_files)                             # allocates by the scaled and oriented size
        for i, (a, b) in enumerate(zip(on_host, expect)):
            assert a.shape == b.shape and np.array_equal(a, b), i
        d.set_jpeg_orientation("ignore")
        for s in (4, 8, 2):                                               # the golden files, by the restatement over the library's coefficients
            d.set_jpeg_scale(s)
            got = d.decode_jpeg(files)
            for f, g in zip(files, got):
                i = rfd.jpeg_info(f)
                c = jpeg_cases.Case("golden", f, rfd.jpeg_coefficients(f), i["width"], i["height"], i["sampling"], 0, ())
                assert np.array_equal(g, expected_bgr(c, s)), (i, s)
        d.set_jpeg_scale(2)
        first = decode_on_device(d, [c.data for c in cases], [expected_bgr(c, 2) for c in cases], async_=True)
        d.set_jpeg_scale(4)
        second = decode_on_device(d, [c.data for c in cases[::-1]], [expected_bgr(c, 4) for c in cases[::-1]], k0=1, async_=True)
        d.set_jpeg_scale(1)
        third = decode_on_device(d, files, full, k0=2, async_=True)       # 1 after 4: the full-size golden pixels again
        d.sync()
        first()
        second()
        third()
        assert all(np.array_equal(a, b) for a, b in zip(d.decode_jpeg(files), full))
    finally:
        d.close()


def test_a_scaled_frame_feeds_the_detector(rfd, stock):
    """Hand-over: a 191 x 127 file decoded at 1/2 into a 96 x 64 frame that goes to rfd_detect_batch_device on the same stream,
    against the same pixels uploaded as an ordinary frame: identical detections, in the scaled frame's coordinates."""
    import torch
    case = stock["hand_over"]
    frame = expected_bgr(case, 2)
    assert frame.shape == (64, 96, 3)
    d = detector(rfd, 1, (191, 127), 2)
    try:
        d.init_synthetic_weights(1234)
        _, tn, _ = d.preprocess([frame])
        heads = d.forward(tn)
        fg = np.concatenate([heads[3 * l][:, 2:4].reshape(1, -1) for l in range(3)], 1)
        d.set_thresholds(float(np.quantile(fg, 0.99)), 0.45)              # the smoke test's calibration: about 1 % of the anchors pass
        dev = torch.device("cuda", 0)

        def outputs():
            return (torch.zeros((1, 256, 5), device=dev), torch.zeros((1, 256, 10), device=dev), torch.zeros(1, dtype=torch.int32, device=dev),
                    torch.zeros(1, dtype=torch.int32, device=dev))
        uploaded, decoded = torch.from_numpy(frame.reshape(64, 96 * 3)).to(dev), torch.zeros((64, 96 * 3), dtype=torch.uint8, device=dev)
        want, got = outputs(), outputs()
        torch.cuda.synchronize()
        img = (rfd.rfd_image * 1)()
        img[0].data, img[0].height, img[0].width, img[0].stride = uploaded.data_ptr(), 64, 96, 96 * 3
        out = rfd.rfd_dets(*(t.data_ptr() for t in want))
        assert d._L.rfd_detect_batch_device(d._ctx, img, 1, C.byref(out), 0) == 0, d._L.rfd_last_error()
        arr = d.decode_jpeg_device([case.data], [decoded.data_ptr()], [(64, 96)], async_=True)
        out = rfd.rfd_dets(*(t.data_ptr() for t in got))
        assert d._L.rfd_detect_batch_device(d._ctx, arr, 1, C.byref(out), 0) == 0, d._L.rfd_last_error()
        d.sync()
        assert np.array_equal(decoded.cpu().numpy().reshape(64, 96, 3), frame)
        k = int(want[2].cpu()[0])
        assert k > 0 and int(got[2].cpu()[0]) == k and int(got[3].cpu()[0]) == int(want[3].cpu()[0])
        assert np.array_equal(got[0].cpu().numpy()[0, :k], want[0].cpu().numpy()[0, :k])
        assert np.array_equal(got[1].cpu().numpy()[0, :k], want[1].cpu().numpy()[0, :k])
    finally:
        d.close()
