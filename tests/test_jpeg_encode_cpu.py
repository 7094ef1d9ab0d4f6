"""The JPEG encode without a GPU (include/rfd.h, "JPEG encode"): the numpy restatement tests/jpeg_encode_ref.py against Pillow
(libjpeg-turbo's default compressor) byte for byte, SOI to EOI; rfd_jpeg_encode_header and rfd_jpeg_encode_bound through ctypes;
the exports, the struct layout, the argument errors that need no device; and csrc/jpeg_encode_plan.h alone in a stand-alone
program, plain and under the sanitizers."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import jpeg_encode_cases as EC
import jpeg_encode_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["rfd_jpeg_encode_config_default", "rfd_jpeg_encode_bound", "rfd_jpeg_encode_header", "rfd_encode_jpeg_batch_device", "rfd_encode_jpeg_batch",
           "rfd_debug_jpeg_encode_blocks", "rfd_debug_jpeg_encode_coefficients"]


def _judge(h, w, content, q, sampling, restart):
    pytest.importorskip("PIL.Image")
    img = EC.image(h, w, content)
    y = R.ycc(img)[0].astype(np.uint8) if sampling == R.GRAY else None      # grey: an `L` image equal to the restated Y plane
    return R.pillow(img, q, sampling, restart, y_plane=y)


@pytest.mark.parametrize("restart", EC.RESTARTS)
@pytest.mark.parametrize("sampling", EC.SAMPLINGS, ids=lambda s: EC.SAMPLING_NAMES[s])
def test_the_restatement_equals_pillow_byte_for_byte(sampling, restart):
    for h, w, content, q in EC.sweep(sampling, restart):
        want = _judge(h, w, content, q, sampling, restart)
        got = EC.expected(h, w, content, q, sampling, restart)
        assert got == want, (h, w, content, q, len(got), len(want))


def test_the_sizes_that_separate_the_two_bottom_edge_rules_do():
    """padding the INPUT of a 4:2:0 file to whole MCUs instead of repeating the downsampled rows gives another file at 8x8,
    8x16, 24x24 and 40x8, and the same one at 16x8: the sweep can tell the rules apart"""
    def wrong(img, q):
        h, w = img.shape[:2]
        padded = R._extend(img.reshape(h, w * 3), -(-h // 16) * 16, w * 3).reshape(-1, w, 3)
        coef = R.blocks(padded, q, R.S420)
        return R.file_from_blocks(coef, w, h, q, R.S420, 0)
    differs = {(h, w): wrong(EC.image(h, w, "noise"), 90) != EC.expected(h, w, "noise", 90, R.S420, 0) for (h, w) in EC.GEOMETRIES}
    assert all(differs[g] for g in [(8, 8), (8, 16), (24, 24), (40, 8)]) and not differs[(16, 8)] and not differs[(112, 112)]


def test_the_restated_colour_conversion_over_the_cube_corners_and_noise():
    """Y, Cb, Cr stay in 0 .. 255 and the corners give the known values"""
    px = np.array([[[0, 0, 0], [255, 255, 255], [255, 0, 0], [0, 255, 0], [0, 0, 255]]], np.uint8)   # BGR
    y, cb, cr = R.ycc(px)
    assert y.tolist() == [[0, 255, 29, 150, 76]] and cb.tolist() == [[128, 128, 255, 44, 85]] and cr.tolist() == [[128, 128, 107, 21, 255]]
    y, cb, cr = R.ycc(np.random.default_rng(3).integers(0, 256, (64, 64, 3), dtype=np.uint8))
    assert min(y.min(), cb.min(), cr.min()) >= 0 and max(y.max(), cb.max(), cr.max()) <= 255


# ---- the library's host-only calls ----
def test_exports_header_and_binding_agree(rfd):
    header = open(os.path.join(ROOT, "include", "rfd.h")).read()
    L = rfd.load_library()
    for name in SYMBOLS:
        assert re.search(r"RFD_API\s+int\s+%s\s*\(" % name, header), name
        assert hasattr(L, name) and name in rfd.API_SYMBOLS, name
    assert header.count("encode") > 20
    for text in ("baseline", "8 bits", "no progressive", "no optimised Huffman", "no EXIF", "restart_rows = 0 is ONE interval", "22 + 63 * 26"):
        assert text in header, text


def test_struct_layout_and_default(rfd):
    c = rfd.rfd_jpeg_encode_config
    assert C.sizeof(c) == 32 and [getattr(c, f).offset for f in ("quality", "sampling", "restart_rows", "reserved")] == [0, 4, 8, 12]
    L = rfd.load_library()
    v = c()
    C.memset(C.byref(v), 0xFF, C.sizeof(v))
    assert L.rfd_jpeg_encode_config_default(C.byref(v)) == rfd.RFD_OK
    assert (v.quality, v.sampling, v.restart_rows, list(v.reserved)) == (90, rfd.JPEG_420, 1, [0] * 5)
    assert L.rfd_jpeg_encode_config_default(None) == rfd.RFD_ERR_INVALID_ARG


def test_the_header_equals_pillows_first_bytes(rfd):
    for (h, w) in EC.GEOMETRIES + [(1080, 1920), (65535, 1)]:
        for sampling in EC.SAMPLINGS:
            for q in EC.QUALITIES:
                for restart in EC.RESTARTS:
                    got = rfd.jpeg_encode_header(w, h, rfd.jpeg_encode_config(q, sampling, restart))
                    assert got == R.header(w, h, q, sampling, restart), (h, w, sampling, q, restart)
                    if h * w <= 112 * 112:
                        assert _judge(h, w, "ramp", q, sampling, restart).startswith(got), (h, w, sampling, q, restart)
    L = rfd.load_library()
    cfg, n, buf = rfd.jpeg_encode_config(), C.c_size_t(0), (C.c_uint8 * 700)()
    assert L.rfd_jpeg_encode_header(8, 8, C.byref(cfg), buf, 628, C.byref(n)) == rfd.RFD_ERR_CAPACITY and n.value == 629
    assert L.rfd_jpeg_encode_header(8, 8, C.byref(cfg), None, 0, C.byref(n)) == rfd.RFD_ERR_CAPACITY and n.value == 629
    assert L.rfd_jpeg_encode_header(8, 8, C.byref(cfg), buf, 629, C.byref(n)) == rfd.RFD_OK


def test_every_file_of_the_sweep_is_within_its_bound(rfd):
    for sampling in EC.SAMPLINGS:
        for restart in EC.RESTARTS:
            for h, w, content, q in EC.sweep(sampling, restart):
                bound = rfd.jpeg_encode_bound(w, h, rfd.jpeg_encode_config(q, sampling, restart))
                assert len(EC.expected(h, w, content, q, sampling, restart)) <= bound
    # the bound's own arithmetic: one MCU of 6 blocks, and 1080p in rows
    assert rfd.jpeg_encode_bound(1, 1, rfd.jpeg_encode_config(90, R.S420, 1)) == 629 + 2 * ((6 * 1660 + 7) // 8) + 2
    assert rfd.jpeg_encode_bound(1920, 1080, rfd.jpeg_encode_config(90, R.S420, 1)) == 629 + 68 * (2 * ((120 * 6 * 1660 + 7) // 8) + 2)
    assert rfd.jpeg_encode_bound(1920, 1080, rfd.jpeg_encode_config(90, R.S420, 0)) == 623 + 2 * ((68 * 120 * 6 * 1660 + 7) // 8) + 2


def test_the_densest_block_the_tables_can_code_meets_the_bounds_unit():
    """a chrominance block of DC category 11 and 63 AC symbols of size 10 is what the bound assumes for every block, less the
    few bits by which the 0/10 code is shorter than 16"""
    zz = np.full(64, -1023, np.int16)
    zz[0] = -1024                      # against a predictor of 1023 it would be category 11; alone it is -1024: category 11 too
    acc, n = EC.block_bits(zz, table=1)
    assert 22 + 63 * 20 <= n <= 22 + 63 * 26


BAD = [("quality", 0), ("quality", 101), ("quality", -5), ("sampling", -1), ("sampling", 4), ("restart_rows", -1), ("reserved", 1)]


@pytest.mark.parametrize("field,value", BAD)
def test_every_config_bound_is_refused_by_name_before_the_context(rfd, field, value):
    L = rfd.load_library()
    cfg = rfd.jpeg_encode_config()
    if field == "reserved":
        cfg.reserved[2] = value
    else:
        setattr(cfg, field, value)
    n, size = C.c_size_t(0), C.c_int32(0)
    img = (rfd.rfd_image * 1)()
    calls = [lambda: L.rfd_jpeg_encode_bound(8, 8, C.byref(cfg), C.byref(n)),
             lambda: L.rfd_jpeg_encode_header(8, 8, C.byref(cfg), None, 0, C.byref(n)),
             lambda: L.rfd_encode_jpeg_batch_device(None, img, 1, None, C.byref(cfg), None, 0, None, 1),
             lambda: L.rfd_encode_jpeg_batch(None, img, 1, C.byref(cfg), None, 0, None),
             lambda: L.rfd_debug_jpeg_encode_blocks(None, img, C.byref(cfg), None, 0, C.byref(n)),
             lambda: L.rfd_debug_jpeg_encode_coefficients(None, None, 0, 8, 8, C.byref(cfg), None, 0, C.byref(size))]
    for call in calls:
        assert call() == rfd.RFD_ERR_INVALID_ARG
        assert field in L.rfd_last_error().decode(), L.rfd_last_error()


def test_sizes_and_null_arguments_are_refused_before_a_device_is_needed(rfd):
    L = rfd.load_library()
    cfg, n = rfd.jpeg_encode_config(), C.c_size_t(0)
    for w, h, word in [(0, 8, "width"), (8, 0, "height"), (65536, 8, "width"), (8, 65536, "height"), (-1, 8, "width")]:
        assert L.rfd_jpeg_encode_bound(w, h, C.byref(cfg), C.byref(n)) == rfd.RFD_ERR_INVALID_ARG and word in L.rfd_last_error().decode()
        assert L.rfd_jpeg_encode_header(w, h, C.byref(cfg), None, 0, C.byref(n)) == rfd.RFD_ERR_INVALID_ARG and word in L.rfd_last_error().decode()
    wide = rfd.jpeg_encode_config(90, R.S444, 8)                      # 8 MCU rows of 8192 MCUs: above what DRI can say
    assert L.rfd_jpeg_encode_bound(65535, 64, C.byref(wide), C.byref(n)) == rfd.RFD_ERR_INVALID_ARG and "restart_rows" in L.rfd_last_error().decode()
    assert L.rfd_jpeg_encode_bound(8, 8, None, C.byref(n)) == rfd.RFD_ERR_INVALID_ARG
    assert L.rfd_jpeg_encode_bound(8, 8, C.byref(cfg), None) == rfd.RFD_ERR_INVALID_ARG
    assert L.rfd_jpeg_encode_header(8, 8, C.byref(cfg), None, 0, None) == rfd.RFD_ERR_INVALID_ARG
    img = (rfd.rfd_image * 1)()
    assert L.rfd_encode_jpeg_batch_device(None, img, 1, None, C.byref(cfg), None, 0, None, 1) == rfd.RFD_ERR_INVALID_ARG and b"ctx" in L.rfd_last_error()
    assert L.rfd_encode_jpeg_batch(None, img, 1, C.byref(cfg), None, 0, None) == rfd.RFD_ERR_INVALID_ARG and b"ctx" in L.rfd_last_error()


# ---- the plan header alone ----
def _build_and_run(tmp_path, name, extra):
    exe = str(tmp_path / name)
    src = os.path.join(ROOT, "tests", "cpp", "jpeg_encode_plan_check.cpp")
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", src, "-o", exe] + extra, capture_output=True, text=True)
    if build.returncode != 0:
        return build
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0 and " 0 failures" in run.stdout, run.stdout + run.stderr
    m = re.search(r"(\d+) checks, 0 failures", run.stdout)
    assert m and int(m.group(1)) > 2033 * 32768, run.stdout   # the program did try every divisor against every magnitude
    return build


def test_the_plan_alone_in_a_plain_build(tmp_path):
    """tests/cpp/jpeg_encode_plan_check.cpp: geometry and bounds at 1 x 1 and 65535 x 65535, every quality's tables, the code
    tables, the refusals, and the exhaustive proof that the reciprocal multiplication is the division"""
    build = _build_and_run(tmp_path, "jpeg_encode_plan_check", [])
    assert build.returncode == 0, build.stderr


def test_the_plan_alone_under_address_and_ub_sanitizers(tmp_path):
    """the same program under AddressSanitizer and UBSan, as tests/test_shot_quality_cpu.py builds its own; where the sanitizer
    runtimes cannot be linked the plain build above is what ran"""
    build = _build_and_run(tmp_path, "jpeg_encode_plan_check_san",
                           ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan"])
    if build.returncode != 0:
        assert "sanitize" in build.stderr or "asan" in build.stderr or "ubsan" in build.stderr, build.stderr


def test_the_plan_is_plain_host_code():
    txt = open(os.path.join(ROOT, "rs-face-detection_amd", "csrc", "jpeg_encode_plan.h")).read()
    code = re.sub(r"//.*", "", txt)
    assert "#include <hip" not in code and "hipStream" not in code and "rfd_common" not in code and "__device__" not in code
