"""The shot quality without a GPU (include/rfd.h, "shot quality"): the numpy restatement against every written value of the
constructed cases, the exports, the struct layout, the default config, the argument errors that need no device, and the plan
header alone in a stand-alone program, plain and under the sanitizers."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import shot_quality_cases as SC
import shot_quality_ref as SR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["rfd_shot_quality_config_default", "rfd_shot_quality_device", "rfd_shot_quality"]
F = np.float32


@pytest.mark.parametrize("name", sorted(SC.CASES))
def test_the_restatement_gives_every_written_value(name):
    c = SC.CASES[name]
    SC.check(name, SR.measure(c["frame"], c["box"], c["lmk"], SR.config(**c["cfg"])))


def test_the_cases_cover_what_they_claim():
    """both statuses, every box side of the list, NaNs in all ten landmark coordinates, and values on both sides of each cap"""
    got = {n: SR.measure(c["frame"], c["box"], c["lmk"], SR.config(**c["cfg"])) for n, c in SC.CASES.items()}
    assert {g["status"] for g in got.values()} == {0, 1}
    sides = {g["region"][4] for n, g in got.items() if n.startswith("box_")} | {g["region"][5] for n, g in got.items() if n.startswith("box_")}
    assert {31, 32, 33, 63, 64, 65, 95} <= sides and min(sides) < -2**31
    assert sum(n.startswith("pose_nan_") for n in got) == 10
    sharp = [float(g["parts"][0]) for g in got.values()]
    assert min(sharp) == 0.0 and max(sharp) == 1040400.0
    assert any(np.isnan(g["q"]) for g in got.values()) and any(0 < float(g["q"]) < 1 for g in got.values() if not np.isnan(g["q"]))


def test_the_inverse_cell_map_equals_the_edges():
    """the cell of column x is (32 (x + 1) - 1) // w: what the kernel uses, against the edges the restatement uses"""
    for w in list(range(32, 400)) + [1080, 1920, 3840]:
        e = SR.edges(0, w)
        x = np.arange(w, dtype=np.int64)
        c = (32 * (x + 1) - 1) // w
        assert e[0] == 0 and e[32] == w and (np.diff(e) > 0).all()
        assert ((e[c] <= x) & (x < e[c + 1])).all(), w


def test_as_i32_and_the_region_at_the_extremes():
    assert [SR.as_i32(v) for v in (1.75, -1.75, np.nan, np.inf, -np.inf, 2147483648.0, -2147483648.0, 2147483520.0)] == \
        [1, -1, 0, 2**31 - 1, -2**31, 2**31 - 1, -2**31, 2147483520]
    assert SR.region([np.inf, np.inf, -np.inf, -np.inf], 100, 80) == (2**31 - 1, 2**31 - 1, -2**31, -2**31, -2**32 + 2, -2**32 + 2)
    assert SR.region([-1e30, np.nan, 1e30, 1e30], 100, 80) == (0, 0, 99, 79, 100, 80)


def test_run_leaves_the_rows_past_the_count():
    frame = SC.NOISE
    boxes = np.zeros((1, 4, 5), F)
    boxes[0, :] = [10, 10, 60, 60, 0.5]
    lmk = np.tile(np.asarray(SC.STANDARD, F), (1, 4, 1))
    for count, rows in ((2, 2), (-3, 0), (9, 4)):
        q, parts, status = np.full((1, 4), -7, F), np.full((1, 4, 8), -7, F), np.full((1, 4), -7, np.int32)
        SR.run([frame], boxes, lmk, [count], SR.config(), q, parts, status)
        assert (q[0, rows:] == -7).all() and (parts[0, rows:] == -7).all() and (status[0, rows:] == -7).all()
        assert (status[0, :rows] == 0).all() and (q[0, :rows] > 0).all()


def test_exports_header_and_binding_agree(rfd):
    header = open(os.path.join(ROOT, "include", "rfd.h")).read()
    L = rfd.load_library()
    for name in SYMBOLS:
        assert re.search(r"RFD_API\s+int\s+%s\s*\(" % name, header), name
        assert name in rfd.API_SYMBOLS and hasattr(L, name), name
        assert getattr(L, name).argtypes is not None, name
    assert callable(rfd.RetinaFaceDetection.shot_quality) and callable(rfd.shot_quality_config)
    assert (rfd.SHOT_QUALITY_PARTS, rfd.SHOT_QUALITY_MAX_SIDE) == (8, 32768)
    for name, value in (("RFD_SHOT_QUALITY_PARTS", "8"), ("RFD_SHOT_QUALITY_MAX_SIDE", "32768")):
        assert re.search(r"#define %s %s\b" % (name, value), header), name
    assert header.count("CHOSEN values, not tuned on data") >= 2        # the tracker's defaults and these
    hpp = open(os.path.join(ROOT, "include", "rfd.hpp")).read()
    assert "rfd_shot_quality(" in hpp and "rfd_shot_quality_device(" in hpp and "rfd_shot_quality_config_default(" in hpp
    # the header states the measure: every constant of it is there
    for text in ("1868", "9617", "4899", "8192", ">> 14", "207360000.0", "16384.0", "/ 1024", "0x7FC00000", "as_i32"):
        assert text in header, text


def test_struct_layout(rfd):
    c = rfd.rfd_shot_quality_config
    assert C.sizeof(c) == 52
    assert [getattr(c, f).offset for f in ("dark", "bright", "pitch0", "w_yaw", "w_roll", "w_pitch", "sharp_ref", "size_ref", "times_score", "reserved")] == \
        [0, 4, 8, 12, 16, 20, 24, 28, 32, 36]


def test_default_config(rfd):
    L = rfd.load_library()
    c = rfd.rfd_shot_quality_config()
    C.memset(C.byref(c), 0xFF, C.sizeof(c))
    assert L.rfd_shot_quality_config_default(C.byref(c)) == rfd.RFD_OK
    f32 = lambda x: float(F(x))
    assert (c.dark, c.bright, c.pitch0, c.w_yaw, c.w_roll, c.w_pitch, c.sharp_ref, c.size_ref, c.times_score) == \
        (30, 225, f32(0.495), 1.0, 1.0, 2.0, 64.0, 112.0, 0)
    assert list(c.reserved) == [0, 0, 0, 0]
    assert L.rfd_shot_quality_config_default(None) == rfd.RFD_ERR_INVALID_ARG
    d = SR.config()
    assert all(f32(getattr(c, k)) == f32(v) for k, v in d.items())           # the restatement's defaults are the library's
    assert rfd.shot_quality_config(dark=10).dark == 10
    with pytest.raises(TypeError):
        rfd.shot_quality_config(reserved=1)


BAD = [("dark", -1), ("dark", 256), ("bright", 256), ("bright", -1), ("dark", 225), ("dark", 226), ("pitch0", float("nan")), ("pitch0", float("inf")),
       ("w_yaw", -1.0), ("w_yaw", float("nan")), ("w_roll", -0.5), ("w_roll", float("inf")), ("w_pitch", -2.0), ("w_pitch", float("nan")),
       ("sharp_ref", 0.0), ("sharp_ref", -1.0), ("sharp_ref", float("nan")), ("sharp_ref", float("inf")), ("size_ref", 0.0), ("size_ref", float("nan")),
       ("size_ref", float("inf")), ("times_score", 2), ("times_score", -1)]


def _call_both(L, rfd, ctx, imgs, n, dets, cfg, q):
    yield L.rfd_shot_quality(ctx, imgs, n, dets, cfg, q, None, None)
    yield L.rfd_shot_quality_device(ctx, imgs, n, dets, cfg, q, None, None, 1)


@pytest.mark.parametrize("field,value", BAD)
def test_every_config_bound_is_refused_by_name_before_the_context(rfd, field, value):
    L = rfd.load_library()
    c = rfd.shot_quality_config()
    setattr(c, field, value)
    for status in _call_both(L, rfd, None, None, 1, None, C.byref(c), None):
        assert status == rfd.RFD_ERR_INVALID_ARG
        assert field in L.rfd_last_error().decode(), L.rfd_last_error()


def test_null_arguments_are_refused_before_a_device_is_needed(rfd):
    L = rfd.load_library()
    img = (rfd.rfd_image * 1)()
    one = np.zeros(16, F)
    full = rfd.rfd_dets(one.ctypes.data, one.ctypes.data, one.ctypes.data, None)
    for status in _call_both(L, rfd, None, None, 1, C.byref(full), None, one.ctypes.data):
        assert status == rfd.RFD_ERR_INVALID_ARG and b"imgs" in L.rfd_last_error()
    for dets in (None, C.byref(rfd.rfd_dets()), C.byref(rfd.rfd_dets(one.ctypes.data, None, one.ctypes.data, None))):
        for status in _call_both(L, rfd, None, img, 1, dets, None, one.ctypes.data):
            assert status == rfd.RFD_ERR_INVALID_ARG and b"dets" in L.rfd_last_error()
    for status in _call_both(L, rfd, None, img, 1, C.byref(full), None, None):
        assert status == rfd.RFD_ERR_INVALID_ARG and b"quality" in L.rfd_last_error()
    for status in _call_both(L, rfd, None, img, -1, C.byref(full), None, one.ctypes.data):
        assert status == rfd.RFD_ERR_INVALID_ARG and b"n < 0" in L.rfd_last_error()
    for n in (0, 1):
        for status in _call_both(L, rfd, None, img, n, C.byref(full), None, one.ctypes.data):
            assert status == rfd.RFD_ERR_INVALID_ARG and b"ctx" in L.rfd_last_error()


def _build_and_run(tmp_path, name, extra):
    exe = str(tmp_path / name)
    src = os.path.join(ROOT, "tests", "cpp", "shot_quality_plan_check.cpp")
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", src, "-o", exe] + extra, capture_output=True, text=True)
    if build.returncode != 0:
        return build
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0 and " 0 failures" in run.stdout, run.stdout + run.stderr
    m = re.search(r"(\d+) steps, (\d+) checks, 0 failures", run.stdout)
    assert m and int(m.group(1)) > 4000 and int(m.group(2)) > 16000000, run.stdout   # the program did run its cases
    return build


def test_the_plan_alone_in_a_plain_build(tmp_path):
    """tests/cpp/shot_quality_plan_check.cpp: the inverse cell map against the edges for every side of 32 .. 4096 pixels, the
    regions at the int32 extremes, the config and frame bounds"""
    build = _build_and_run(tmp_path, "shot_quality_plan_check", [])
    assert build.returncode == 0, build.stderr


def test_the_plan_alone_under_address_and_ub_sanitizers(tmp_path):
    """the same program under AddressSanitizer and UBSan, as tests/test_tracker_ref_cpu.py builds its own; where the sanitizer
    runtimes cannot be linked the plain build above is what ran"""
    build = _build_and_run(tmp_path, "shot_quality_plan_check_san",
                           ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan"])
    if build.returncode != 0:
        assert "sanitize" in build.stderr or "asan" in build.stderr or "ubsan" in build.stderr, build.stderr


def test_the_plan_is_plain_host_code():
    txt = open(os.path.join(ROOT, "rs-face-detection_amd", "csrc", "shot_quality_plan.h")).read()
    code = re.sub(r"//.*", "", txt)
    assert "#include <hip" not in code and "hipStream" not in code and "rfd_common" not in code
    # the only word of HIP is the macro that lets the kernel compile the same functions for the device
    assert [l.strip() for l in code.splitlines() if "hip" in l.lower()] == ["#if defined(__HIPCC__)"]
