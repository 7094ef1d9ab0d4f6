"""The case list of tests/jpeg_cases.py without a GPU.  tests/jpeg_write.py and the library's host entropy decoder pin each other:
every file's coefficients come back exactly.  libjpeg-turbo (through Pillow) then judges tests/jpeg_ref.py on exactly the
files tests/test_jpeg_sweep_gpu.py decodes on the device, byte for byte, which is what lets that test use jpeg_ref as its
reference.  Three of the files also go through the stand-alone parser program under AddressSanitizer and UBSan."""
import io
import os
import subprocess

import numpy as np
import pytest

import jpeg_cases
import jpeg_ref
import jpeg_write
from jpeg_cases import GEOMETRY_HEIGHTS, GEOMETRY_WIDTHS, SAMPLINGS, cases, select

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GROUPS = ["geo_", "wide_", "zigzag_", "saturation_", "colour_grid", "restart_"]


def test_the_groups_cover_the_list():
    assert sum(len(select(g)) for g in GROUPS) == len(cases())


@pytest.mark.parametrize("group", GROUPS)
def test_the_host_decoder_returns_the_written_coefficients_exactly(rfd, group):
    for c in select(group):
        got = rfd.jpeg_coefficients(c.data)
        assert got.dtype == np.int16 and got.shape == c.coef.shape and np.array_equal(got, c.coef), c.name
        assert rfd.jpeg_info(c.data) == dict(width=c.width, height=c.height, components=len(c.quant), sampling=c.sampling,
                                             restart_interval=c.restart_interval), c.name


@pytest.mark.parametrize("group", GROUPS)
def test_libjpeg_turbo_decodes_every_case_to_the_pixels_of_jpeg_ref(group):
    Image = pytest.importorskip("PIL.Image")
    for c in select(group):
        want = jpeg_ref.decode(c.coef, c.width, c.height, c.sampling)
        got = np.asarray(Image.open(io.BytesIO(c.data)))
        assert got.shape == want.shape and got.dtype == np.uint8, c.name
        diff = got != want
        assert not diff.any(), "%s: %d values differ, first at %s" % (c.name, int(diff.sum()), np.argwhere(diff)[:1].tolist())


def test_the_list_contains_what_it_promises():
    geo = {(c.width, c.height, c.sampling): c for c in select("geo_")}
    assert len(geo) == len(select("geo_")) == len(GEOMETRY_WIDTHS) * len(GEOMETRY_HEIGHTS) * 4 == 1080
    assert set(geo) == {(w, h, s) for w in GEOMETRY_WIDTHS for h in GEOMETRY_HEIGHTS for s in SAMPLINGS}
    for w in (3, 4, 5, 6):                                             # chroma rows of two and of three samples
        for s in (jpeg_ref.S422, jpeg_ref.S420):
            assert all((w, h, s) in geo for h in GEOMETRY_HEIGHTS)
    for c in geo.values():                                             # three distinct tables under three distinct ids
        if c.sampling != jpeg_ref.GRAY:
            assert len({q.tobytes() for q in c.quant}) == 3, c.name
            sof = c.data.index(b"\xff\xc1" if c.quant[0].max() > 255 else b"\xff\xc0")
            assert [c.data[sof + 12 + 3 * k] for k in range(3)] == [0, 1, 2], c.name
    luma = [bool(c.quant[0].max() > 255) for c in select("geo_")]
    assert luma[0::2] == [False] * 540 and luma[1::2] == [True] * 540
    assert {(c.width, c.height, c.sampling) for c in select("wide_")} == set(jpeg_cases.WIDE)
    for kind in ("single", "prefix"):
        for c in select("zigzag_" + kind):
            assert all(len(set(q.tolist())) == 64 for q in c.quant) and any(q.max() > 255 for q in c.quant), c.name
            zz = c.coef[:, jpeg_write.NATURAL] != 0
            at = 0
            for bw, bh in jpeg_ref.geometry(c.width, c.height, c.sampling)[1]:     # every component holds the whole set
                for k in range(64):
                    assert zz[at + k].tolist() == [(z == k if kind == "single" else z <= k) for z in range(64)], (c.name, at, k)
                assert not zz[at + 64].any()
                at += bw * bh
    assert all(not c.coef.any() for c in select("zigzag_zero")) and len(select("zigzag_zero")) == 2
    counts = {int(np.flatnonzero(np.r_[True, row]).max()) for c in select("zigzag_prefix") for row in c.coef[:, jpeg_write.NATURAL] != 0}
    assert counts == set(range(65))                                    # the run the decoder records: every length 0 .. 64
    assert [c.restart_interval for c in select("restart_")] == [1, 3]
    for c in select("restart_"):
        mcus = -(-c.width // 16) * -(-c.height // 16)
        scan = c.data[c.data.index(b"\xff\xda"):]
        assert c.sampling == jpeg_ref.S420 and mcus >= 20
        assert sum(scan.count(bytes([0xff, 0xd0 + k])) for k in range(8)) == (mcus - 1) // c.restart_interval
    grid = select("colour_grid")[0]
    assert grid.width <= 1024 and grid.coef.shape[0] == 3 * 3 * 2 * 256 * 7 and not grid.coef[:, 1:].any()
    sat = jpeg_ref.idct_unclamped(select("saturation_GRAY")[0].coef)
    assert sat.min() == -384 and sat.max() == 383                      # the whole pinned range, both clamps


def test_the_unclamped_idct_is_the_idct_before_the_level_shift_and_the_clamp():
    c = select("saturation_444")[0]
    s = jpeg_ref.idct_unclamped(c.coef)
    assert s.dtype == np.int64 and (s + 128 < 0).any() and (s + 128 > 255).any()
    assert np.array_equal(np.clip(s + 128, 0, 255), jpeg_ref.idct(c.coef))


def test_the_writer_places_extra_segments_and_honours_table_ids(rfd):
    c = select("geo_17x9_420")[0]
    dims = jpeg_ref.geometry(17, 9, c.sampling)[1]
    coef_q = c.coef.astype(np.int64) // np.concatenate([np.broadcast_to(q, (bw * bh, 64)) for q, (bw, bh) in zip(c.quant, dims)])
    com = jpeg_write.seg(0xfe, b"a comment") + jpeg_write.seg(0xe1, b"Exif\0\0")
    data = jpeg_write.write(coef_q, 17, 9, c.sampling, c.quant, table_ids=[3, 0, 2], extra_segments=com)
    assert data[:2] == b"\xff\xd8" and data[2:2 + len(com)] == com and data.endswith(b"\xff\xd9")
    assert np.array_equal(rfd.jpeg_coefficients(data), c.coef)


def test_written_files_through_the_front_end_under_address_and_ub_sanitizers(tmp_path):
    """tests/cpp/jpeg_parse_check.cpp, built as tests/test_jpeg_cpu.py builds it, on three written files: the restart interval of
    one (RST7 -> RST0), the zigzag set under a 16-bit table, one 4:2:0 geometry case with its three table ids."""
    exe = str(tmp_path / "jpeg_parse_check")
    src = os.path.join(ROOT, "tests", "cpp", "jpeg_parse_check.cpp")
    base = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", src, "-o", exe]
    san = subprocess.run(base + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan"], capture_output=True, text=True)
    if san.returncode != 0:
        plain = subprocess.run(base, capture_output=True, text=True)
        assert plain.returncode == 0, "the build failed:\n" + san.stderr + plain.stderr
    files = []
    for name in ("restart_1", "zigzag_prefix_GRAY", "geo_17x17_420"):
        c = select(name)[0]
        assert c.name == name
        files.append(str(tmp_path / (name + ".jpg")))
        with open(files[-1], "wb") as f:
            f.write(c.data)
    run = subprocess.run([exe] + files, capture_output=True, text=True)
    assert run.returncode == 0 and " 0 failures" in run.stdout, run.stdout + run.stderr
