"""The frame conversion without a GPU (include/rfd.h, "frames in camera and decoder formats"): the numpy restatement against every
written value of the constructed cases and against the real coefficients over the whole (Y, U, V) cube, the layouts, the
exports, the struct layout, the argument errors that need no device, and the plan header alone in a stand-alone program, plain
and under the sanitizers."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import frame_cases as FC
import frame_ref as FR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["rfd_frame_layout_of", "rfd_convert_frames_device", "rfd_upload_frames_device", "rfd_convert_frames"]
CASES = FC.frames()


@pytest.mark.parametrize("color", sorted(FC.YUV))
def test_the_restatement_gives_every_written_pixel(color):
    for name, (Y, U, V), bgr in FC.YUV[color]:
        got = FR.yuv_to_bgr(np.array([Y]), np.array([U]), np.array([V]), color)[0]
        assert tuple(int(x) for x in got) == bgr, (color, name, got)


def test_the_cases_cover_what_they_claim():
    for color, cases in FC.YUV.items():
        limited = FR.TABLE[color][5]
        names = {n for n, _, _ in cases}
        assert {"black", "white", "r_high", "r_low", "b_high", "b_low", "g_high", "g_low"} <= names
        assert ("below_16" in names) == limited and ("y_unchanged" in names) == (not limited)
        by = {n: (yuv, bgr) for n, yuv, bgr in cases}
        assert by["black"][0][0] == (16 if limited else 0) and by["white"][0][0] == (235 if limited else 255)
        for ch, k in (("b", 0), ("g", 1), ("r", 2)):                      # each channel at both ends of the clamp
            assert by[ch + "_high"][1][k] == 255 and by[ch + "_low"][1][k] == 0
            s_hi = FR.shifted(*[np.array([x]) for x in by[ch + "_high"][0]], color)[0, k]
            s_lo = FR.shifted(*[np.array([x]) for x in by[ch + "_low"][0]], color)[0, k]
            assert s_hi > 255 and s_lo < 0, (color, ch, s_hi, s_lo)       # saturating, not merely reaching the end
    assert {c for c, _, _, _ in FC.FLOOR} == set(FR.TABLE)


@pytest.mark.parametrize("color,yuv,total,want", FC.FLOOR)
def test_the_shift_of_a_negative_sum_is_a_floor(color, yuv, total, want):
    Y, U, V = yuv
    cy, cvr, cug, cvg, cub, limited = FR.TABLE[color]
    assert cy * max(Y - 16, 0) * limited + cy * Y * (not limited) + cub * (U - 128) + 524288 == total < 0   # the written sum, in Python integers
    assert total // (1 << 20) == want and int(total / (1 << 20)) == want + 1                               # floor, where truncation differs
    assert int(FR.shifted(np.array([Y]), np.array([U]), np.array([V]), color)[0, 0]) == want
    assert tuple(FR.yuv_to_bgr(np.array([Y]), np.array([U]), np.array([V]), color)[0]) == (0, 0, 0)


@pytest.mark.parametrize("name", [c[0] for c in CASES])
def test_the_restatement_converts_every_constructed_frame(name):
    _, frame, want = next(c for c in CASES if c[0] == name)
    got = FR.convert_frame(frame)
    assert got.dtype == np.uint8 and got.shape == want.shape and got.tobytes() == want.tobytes(), (name, got, want)


def test_the_layouts_of_one_image_agree():
    """NV12, NV21 and I420 of one image give the same bytes; so do YUYV and UYVY of one 4:2:2 image; alpha changes nothing"""
    by = {c[0]: FR.convert_frame(c[1]) for c in CASES}
    for color in sorted(FC.YUV):
        a = by["nv12_colour%d" % color]
        assert a.tobytes() == by["nv21_colour%d" % color].tobytes() == by["i420_colour%d" % color].tobytes()
        assert by["yuyv_colour%d" % color].tobytes() == by["uyvy_colour%d" % color].tobytes() == a.tobytes()
    assert len({by[n].tobytes() for n in by if n.startswith(("bgra_", "rgba_", "bgr", "rgb"))}) == 1
    rng = np.random.default_rng(5)
    for w, h in ((1, 1), (2, 2), (5, 3), (8, 4), (9, 7)):
        cw, ch = (w + 1) // 2, (h + 1) // 2
        y, u, v = (rng.integers(0, 256, s, dtype=np.uint8) for s in ((h, w), (ch, cw), (ch, cw)))
        got = [FR.convert(f, w, h, FR.planes_420(f, y, u, v), 2) for f in (FR.NV12, FR.NV21, FR.I420)]
        assert got[0].tobytes() == got[1].tobytes() == got[2].tobytes()
        # replication: pixel (x, y) takes the chroma of (x >> 1, y >> 1)
        yy, xx = np.mgrid[0:h, 0:w]
        assert got[0].tobytes() == FR.yuv_to_bgr(y, u[yy >> 1, xx >> 1], v[yy >> 1, xx >> 1], 2).tobytes()
        u2, v2 = (rng.integers(0, 256, (h, cw), dtype=np.uint8) for _ in range(2))
        got = [FR.convert(f, w, h, FR.planes_422(f, y, u2, v2), 3) for f in (FR.YUYV, FR.UYVY)]
        assert got[0].tobytes() == got[1].tobytes() == FR.yuv_to_bgr(y, u2[yy, xx >> 1], v2[yy, xx >> 1], 3).tobytes()


@pytest.mark.parametrize("color", sorted(FR.TABLE))
def test_the_tables_against_the_real_coefficients_over_the_whole_cube(color):
    """A guard against typing errors in the constants: over all 2^24 (Y, U, V) the fixed-point result differs from the f64
    evaluation of the real coefficients, rounded to nearest and clamped, by at most 1.  The bound is derived: each table entry is
    its coefficient x 2^20 rounded, so off by under 2^-21 of a unit; |y| <= 255 and |u|, |v| <= 128 make the sums differ by
    under (255 + 128 + 128) * 2^-21 < 10^-3 units, so only the rounding of a sum that lies within 10^-3 of a half can move."""
    ky, kvr, kug, kvg, kub = FR.REAL[color]
    table = FR.TABLE[color]
    for got, real in zip(table[:5], FR.REAL[color]):
        assert abs(got - real * 2 ** 20) <= 0.5, (color, got, real)      # "x 2^20, rounded"
    U, V = np.meshgrid(np.arange(256), np.arange(256), indexing="ij")
    u, v = U.astype(np.float64) - 128, V.astype(np.float64) - 128
    worst = 0
    for Y in range(256):
        y = float(max(Y - 16, 0) if table[5] else Y)
        want = np.stack([ky * y + kub * u, ky * y + kug * u + kvg * v, ky * y + kvr * v], -1)
        want = np.clip(np.floor(want + 0.5), 0, 255).astype(np.int32)
        got = FR.yuv_to_bgr(np.full(U.shape, Y), U, V, color).astype(np.int32)
        worst = max(worst, int(np.abs(got - want).max()))
    assert worst <= 1, worst


def test_layouts_of_the_library_equal_the_restatement(rfd):
    for fmt in range(10):
        for w in (1, 2, 3, 4, 5, 9, 640, 1921):
            for h in (1, 2, 3, 1081):
                l = rfd.frame_layout(fmt, w, h)
                want = FR.layout(fmt, w, h)
                assert l["planes"] == len(want) and list(zip(l["row_bytes"], l["rows"])) == want, (fmt, w, h, l)
                assert rfd.frame_layout(FR.NAMES[fmt], w, h) == l
    L = rfd.load_library()
    l = rfd.rfd_frame_layout()
    C.memset(C.byref(l), 0x5A, C.sizeof(l))
    for fmt, w, h, word in ((10, 4, 4, b"pixel format 10"), (-1, 4, 4, b"pixel format -1"), (5, 0, 4, b"nv12"), (5, 4, -1, b"nv12"), (2, 2 ** 28 + 1, 1, b"bgra")):
        assert L.rfd_frame_layout_of(fmt, w, h, C.byref(l)) == rfd.RFD_ERR_INVALID_ARG and word in L.rfd_last_error(), L.rfd_last_error()
        assert bytes(l) == b"\x5A" * C.sizeof(l)
    assert L.rfd_frame_layout_of(0, 4, 4, None) == rfd.RFD_ERR_INVALID_ARG
    assert rfd.PIXEL_FORMAT_NAMES == FR.NAMES


def test_exports_header_and_binding_agree(rfd):
    header = open(os.path.join(ROOT, "include", "rfd.h")).read()
    L = rfd.load_library()
    for name in SYMBOLS:
        assert re.search(r"RFD_API\s+int\s+%s\s*\(" % name, header), name
        assert name in rfd.API_SYMBOLS and hasattr(L, name), name
    vp, ci = C.c_void_p, C.c_int
    frames, images = C.POINTER(rfd.rfd_frame), C.POINTER(rfd.rfd_image)
    want = {"rfd_frame_layout_of": [ci, ci, ci, C.POINTER(rfd.rfd_frame_layout)], "rfd_convert_frames_device": [vp, frames, ci, images, ci],
            "rfd_upload_frames_device": [vp, frames, ci, images, ci], "rfd_convert_frames": [vp, frames, ci, images]}
    for name, types in want.items():                                     # arity and types, as the header declares them
        assert list(getattr(L, name).argtypes) == types, name
        decl = re.search(r"RFD_API\s+int\s+%s\s*\(([^)]*)\)" % name, header).group(1)
        assert len(decl.split(",")) == len(types), (name, decl)
    for name in ("convert_frames", "convert_frames_device", "upload_frames_device"):
        assert callable(getattr(rfd.RetinaFaceDetection, name)), name
    assert callable(rfd.frame_layout) and callable(rfd.frame)
    # the enumerations: every name with its value, in the header and in the binding
    for i, name in enumerate(FR.NAMES):
        assert re.search(r"\bRFD_PIXEL_%s = %d\b" % (name.upper(), i), header), name
        assert getattr(rfd, "PIXEL_" + name.upper()) == i == getattr(FR, name.upper())
    for i, name in enumerate(("BT601_LIMITED", "BT601_FULL", "BT709_LIMITED", "BT709_FULL")):
        assert re.search(r"\bRFD_COLOR_%s = %d\b" % (name, i), header), name
        assert getattr(rfd, "COLOR_" + name) == i == getattr(FR, name)
    # the header states the arithmetic: every constant of the four tables, the rounding term and the shift
    for color, row in FR.TABLE.items():
        for k in row[:5]:
            assert str(k) in header, k
    for text in ("524288", ">> 20", "max(Y - 16, 0)", "unpinned against a running OpenCV", "utils.rs:29", "RFD_ERR_CAPACITY"):
        assert text in header, text
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "unpinned against a running OpenCV" in design and "frame_convert_kernel" in design


def test_struct_layout(rfd):
    f = rfd.rfd_frame
    assert C.sizeof(f) == 80
    assert [getattr(f, n).offset for n in ("plane", "stride", "width", "height", "format", "color", "reserved")] == [0, 24, 48, 52, 56, 60, 64]
    l = rfd.rfd_frame_layout
    assert C.sizeof(l) == 32 and [getattr(l, n).offset for n in ("planes", "row_bytes", "rows", "reserved")] == [0, 4, 16, 28]


def test_arguments_refused_before_a_device_is_needed(rfd):
    L = rfd.load_library()
    src, out = (rfd.rfd_frame * 1)(), (rfd.rfd_image * 1)()
    calls = (lambda c, s, n, o: L.rfd_convert_frames(c, s, n, o), lambda c, s, n, o: L.rfd_convert_frames_device(c, s, n, o, 1),
             lambda c, s, n, o: L.rfd_upload_frames_device(c, s, n, o, 1))
    for call in calls:
        for n in (0, 1):
            assert call(None, src, n, out) == rfd.RFD_ERR_INVALID_ARG and b"ctx" in L.rfd_last_error()
        assert call(None, src, -1, out) == rfd.RFD_ERR_INVALID_ARG and b"ctx" in L.rfd_last_error()


def _build_and_run(tmp_path, name, extra):
    exe = str(tmp_path / name)
    src = os.path.join(ROOT, "tests", "cpp", "frame_plan_check.cpp")
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", src, "-o", exe] + extra, capture_output=True, text=True)
    if build.returncode != 0:
        return build
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0 and " 0 failures" in run.stdout, run.stdout + run.stderr
    m = re.search(r"(\d+) steps, (\d+) checks, 0 failures", run.stdout)
    assert m and int(m.group(1)) > 1520 and int(m.group(2)) > 14000, run.stdout   # the program did run its cases
    return build


def test_the_plan_alone_in_a_plain_build(tmp_path):
    """tests/cpp/frame_plan_check.cpp: every format at widths and heights 1 .. 9 and 4095 .. 4097, every refusal, the work items
    and first workgroups of mixed batches, a 32768-wide frame"""
    build = _build_and_run(tmp_path, "frame_plan_check", [])
    assert build.returncode == 0, build.stderr


def test_the_plan_alone_under_address_and_ub_sanitizers(tmp_path):
    """the same program under AddressSanitizer and UBSan, as tests/test_shot_quality_cpu.py builds its own.  Where the linker
    cannot find the sanitizer runtimes the test is skipped with the linker's message; any other failure of the build fails it"""
    build = _build_and_run(tmp_path, "frame_plan_check_san",
                           ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan"])
    if build.returncode != 0:
        missing = re.search(r"cannot find -l?(lib)?(asan|ubsan)\S*|cannot find \S*(asan|ubsan)\S*", build.stderr)
        assert missing and " error: " not in build.stderr.replace("ld: error: ", ""), build.stderr   # a compiler diagnostic is a failure
        pytest.skip("the sanitizer runtimes cannot be linked here: " + missing.group(0))


def test_the_plan_is_plain_host_code():
    txt = open(os.path.join(ROOT, "rs-face-detection_amd", "csrc", "frame_plan.h")).read()
    code = re.sub(r"//.*", "", txt)
    assert "#include <hip" not in code and "hipStream" not in code and "rfd_common" not in code
    assert not [l for l in code.splitlines() if "hip" in l.lower()]
