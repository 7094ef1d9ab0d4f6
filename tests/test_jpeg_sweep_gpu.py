"""The two JPEG kernels (csrc/kernels_jpeg.hip) and their host staging swept over the case list of tests/jpeg_cases.py: every
chroma width and height at which the upsampling takes another branch, three distinct quantisation tables, one non-zero
coefficient at each zigzag position and every run length 0 .. 64, planes more than 32 blocks wide, both clamps over the whole
pinned range, every Cb and Cr level, restart intervals that wrap RST7 -> RST0, batches of 1 .. 16 frames, and output frames
at every base alignment and stride.  The files are written in the test process (tests/jpeg_write.py); no Pillow is needed here.

Expected pixels everywhere: jpeg_ref.to_bgr(jpeg_ref.decode(dequantised coefficients)), which tests/test_jpeg_write_cpu.py has
libjpeg-turbo confirm byte for byte on the very same files.  The bar is byte equality."""
import contextlib

import numpy as np
import pytest

import jpeg_cases
import jpeg_ref
from jpeg_cases import cases, select

pytestmark = pytest.mark.gpu

FILL = 0xA5
GUARD = 8                          # bytes in front of, between and behind the frames of an arena: they must still hold FILL


@pytest.fixture(scope="module")
def want():
    """the expected BGR frame of every case, computed once"""
    return {c.name: jpeg_cases.expected_bgr(c) for c in cases()}


@contextlib.contextmanager
def detector(rfd, batch, frames):
    """a detector whose staging (max_src, max_batch_size) is the smallest that holds `frames` in batches of `batch`"""
    d = rfd.RetinaFaceDetection(max_batch_size=batch, max_det=256, max_src=(max(c.width for c in frames), max(c.height for c in frames)))
    try:
        yield d
    finally:
        d.close()


def describe(name, got, expect):
    diff = (got != expect).any(-1)
    return "%s: %d of %d pixels differ, first at (y, x) = %s: got %s, want %s" % (
        name, int(diff.sum()), diff.size, np.argwhere(diff)[0].tolist(), got[tuple(np.argwhere(diff)[0])].tolist(), expect[tuple(np.argwhere(diff)[0])].tolist())


def decode_on_device(det, batch, want, k0=0):
    """rfd_decode_jpeg_batch_device into one FILL-filled torch buffer.  Frame k = k0 + i starts k % 4 bytes past a 4-byte boundary
    and has (k // 4) % 8 bytes of stride padding.  Asserts the pixels and that every other byte of the buffer still holds FILL.
    -> (the frames, the set of (base % 4, stride % 4) used)"""
    import torch
    at, place = GUARD, []
    for i, c in enumerate(batch):
        k = k0 + i
        at += (k - at) % 4
        stride = 3 * c.width + (k // 4) % 8
        place.append((at, stride))
        at += c.height * stride + GUARD
    arena = torch.full((at,), FILL, dtype=torch.uint8, device=torch.device("cuda", 0))
    torch.cuda.synchronize()
    assert arena.data_ptr() % 4 == 0
    expect = np.full(at, FILL, np.uint8)
    rows = lambda a, c, o, s: np.lib.stride_tricks.as_strided(a[o:], (c.height, 3 * c.width), (s, 1))
    for c, (o, s) in zip(batch, place):
        rows(expect, c, o, s)[:] = want[c.name].reshape(c.height, 3 * c.width)
    det.decode_jpeg_device([c.data for c in batch], [arena.data_ptr() + o for o, s in place], [(c.height, c.width) for c in batch], [s for o, s in place])
    got = arena.cpu().numpy()
    frames = [rows(got, c, o, s).reshape(c.height, c.width, 3).copy() for c, (o, s) in zip(batch, place)]
    if not np.array_equal(got, expect):
        for c, f in zip(batch, frames):
            assert np.array_equal(f, want[c.name]), describe(c.name, f, want[c.name])
        bad = int(np.flatnonzero(got != expect)[0])
        owner = max(i for i, (o, s) in enumerate(place) if o - GUARD <= bad)
        raise AssertionError("a byte outside the pixels was written: byte %d of the buffer, %d past the start of frame %d (%s, stride %d)" %
                             (bad, bad - place[owner][0], owner, batch[owner].name, place[owner][1]))
    return frames, {((arena.data_ptr() + o) % 4, s % 4) for o, s in place}


def test_geometry_sweep_in_batches_of_1_to_16_at_every_alignment_and_stride(rfd, want):
    geo = select("geo_")                                               # 1080 frames of at most 66 x 17
    seen, sizes, k, n = set(), set(), 0, 1
    with detector(rfd, 16, geo) as det:
        while k < len(geo):
            batch = geo[k:k + n]
            seen |= decode_on_device(det, batch, want, k)[1]
            sizes.add(len(batch))
            k, n = k + len(batch), n % 16 + 1
    assert sizes == set(range(1, 17))
    assert seen == {(a, s) for a in range(4) for s in range(4)}        # all four base alignments with all four stride classes


def test_geometry_sweep_through_the_host_form_at_1_and_16_threads(rfd, want):
    geo = select("geo_")
    with detector(rfd, 16, geo) as det:
        for threads in (1, 16):
            det.set_decode_threads(threads)
            for k in range(0, len(geo), 16):
                batch = geo[k:k + 16]
                got = det.decode_jpeg([c.data for c in batch])
                for c, g in zip(batch, got):
                    assert g.shape == want[c.name].shape and np.array_equal(g, want[c.name]), "%d threads, %s" % (threads, describe(c.name, g, want[c.name]))


def test_sixteen_frames_of_one_workgroup_each(rfd, want):
    """1 x 1 .. 4 x 4 in mixed samplings: every frame is one workgroup of either kernel, so the first-workgroup indices the
    kernels search are 0, 1, 2, .. 15"""
    geo = {c.name: c for c in select("geo_")}
    batch = [geo["geo_%dx%d_%s" % (i % 4 + 1, i // 4 + 1, jpeg_cases.SAMPLING_NAME[jpeg_cases.SAMPLINGS[(i + i // 4) % 4]])] for i in range(16)]
    assert len({c.sampling for c in batch[:4]}) == 4 and all(jpeg_ref.num_blocks(c.width, c.height, c.sampling) <= 32 for c in batch)
    with detector(rfd, 16, batch) as det:
        decode_on_device(det, batch, want)
        decode_on_device(det, batch[::-1], want, 1)


def decode_group(rfd, want, prefix, frames):
    batch = select(prefix)
    assert len(batch) == frames
    with detector(rfd, frames, batch) as det:
        decode_on_device(det, batch, want)                             # 0 .. 3 bytes of base offset, no padding
        decode_on_device(det, batch[::-1], want, 5)                    # 1 byte of padding: rows at every alignment, byte stores


def test_planes_more_than_32_blocks_wide(rfd, want):
    decode_group(rfd, want, "wide_", 4)                                # 4 frames, the largest 520 x 16: luma 66 blocks per row, chroma 33


def test_one_coefficient_at_each_zigzag_position_and_every_run_length(rfd, want):
    decode_group(rfd, want, "zigzag_", 6)                              # 6 frames of 100 x 37 (65 blocks) and 203 x 77 (390 blocks)


def test_both_clamps_over_the_whole_pinned_range(rfd, want):
    decode_group(rfd, want, "saturation_", 2)                          # 2 frames of 253 x 205: 832 and 2496 blocks


def test_every_cb_and_cr_level_at_three_luma_levels(rfd, want):
    decode_group(rfd, want, "colour_grid", 1)                          # 1 frame of 1024 x 672: 3 x 10752 flat blocks


def test_restart_intervals_of_one_and_three(rfd, want):
    decode_group(rfd, want, "restart_", 2)                             # 2 frames of 80 x 64 and 77 x 61, 20 MCUs each


def test_a_frame_decodes_the_same_alone_and_as_frame_7_of_16_between_two_wide_frames(rfd, want):
    zigzag, wide = select("zigzag_single_420")[0], select("wide_520x16_420")[0]
    batch = select("geo_")[500:506] + [wide, zigzag, wide] + select("geo_")[900:907]
    assert len(batch) == 16 and batch[7] is zigzag
    with detector(rfd, 16, batch) as det:                              # 16 frames of at most 520 x 77
        alone = decode_on_device(det, [zigzag], want)[0][0]
        seventh = decode_on_device(det, batch, want)[0][7]
    assert np.array_equal(alone, seventh)
