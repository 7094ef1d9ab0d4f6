"""The redaction without a GPU (include/rfd.h, "redaction"): the numpy restatement against every written frame of the constructed
cases, the exports, the struct layout, the default config, the argument errors that need no device, and the plan header alone in
a stand-alone program, plain and under the sanitizers."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import redact_cases as RC
import redact_ref as RR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["rfd_redact_config_default", "rfd_redact_faces_device", "rfd_redact_faces"]
F = np.float32


def _run(c):
    boxes = np.asarray(c["rows"], F)
    return RR.redact(c["frame"], boxes, len(boxes), None, RR.config(**c["cfg"]))


@pytest.mark.parametrize("name", sorted(RC.CASES))
def test_the_restatement_gives_every_written_frame(name):
    c = RC.CASES[name]
    before = c["frame"].copy()
    out, applied = _run(c)
    RC.check(name, out, applied)
    assert c["frame"].tobytes() == before.tobytes()                     # the source is untouched


def test_the_cases_cover_what_they_claim():
    """the constant frames stay, the checkerboard has cells cut by both edges and the corner, the cut cell is cut, the two boxes
    share a cell and overlap, the ellipses have every side 1 .. 4, every skipped row is skipped for its own reason, the margins
    reach every side, and the truncations are the three written ones"""
    C_ = RC.CASES
    reg = lambda name, i=0: RR.region(C_[name]["rows"][i], RR.config(**C_[name]["cfg"]), C_[name]["frame"].shape[1], C_[name]["frame"].shape[0])
    assert sum(n.startswith("constant_") for n in C_) == 6
    c = C_["checkerboard_cell2"]
    assert c["frame"].shape[:2] == (9, 11) and c["cfg"]["cell"] == 2 and reg("checkerboard_cell2") == (0, 0, 10, 8)
    assert (c["want"][:8, :10] == 128).all() and (c["want"][8, :10] == 128).all() and (c["want"][:8, 10] == 128).all() and (c["want"][8, 10] == 255).all()
    c = C_["cell_cut_by_the_frame"]
    assert c["frame"].shape[0] % c["cfg"]["cell"] and c["frame"].shape[1] % c["cfg"]["cell"] and reg("cell_cut_by_the_frame") == (5, 4, 5, 4)
    a, b = reg("overlap_a_b", 0), reg("overlap_a_b", 1)
    assert a == (0, 0, 1, 1) and b == (1, 1, 2, 2) and max(a[2], b[2]) < 4 and C_["overlap_a_b"]["cfg"]["cell"] == 4
    assert C_["overlap_a_b"]["rows"] == C_["overlap_b_a"]["rows"][::-1] and C_["overlap_a_b"]["want"].tobytes() == C_["overlap_b_a"]["want"].tobytes()
    sides = {s for (w, h) in RC.ELLIPSES for s in (w, h)}
    assert {1, 2, 3, 4} <= sides and all((w, 1) in RC.ELLIPSES and (1, w) in RC.ELLIPSES for w in (1, 2, 3, 4))
    for (w, h), art in RC.ELLIPSES.items():
        assert len(art) == h and all(len(r) == w for r in art)
        assert reg("ellipse_%dx%d" % (w, h)) == (3, 2, 3 + w - 1, 2 + h - 1)
    assert any("." in "".join(a) for a in RC.ELLIPSES.values())
    skipped = C_["skipped_rows_alone"]
    assert len(skipped["rows"]) == 6 + 12 and all(reg("skipped_rows_alone", i) is None for i in range(18))
    for k in range(4):                                                   # a NaN, +inf and -inf in each coordinate
        col = [r[k] for r in skipped["rows"]]
        assert sum(np.isnan(v) for v in col) == 1 and sum(v == np.inf for v in col) == 1 and sum(v == -np.inf for v in col) == 1
    assert sum(reg("skipped_rows", i) is not None for i in range(19)) == 1 == C_["skipped_rows"]["applied"]
    h, w = C_["margins_past_every_side"]["frame"].shape[:2]
    box, m = C_["margins_past_every_side"]["rows"][0], 4.0
    assert box[0] - (box[2] - box[0]) * m < 0 and box[2] + (box[2] - box[0]) * m > w and box[1] - (box[3] - box[1]) * m < 0 and box[3] + (box[3] - box[1]) * m > h
    assert reg("margins_past_every_side") == (0, 0, w - 1, h - 1) and reg("margins_exact") == (7, 6, 13, 15)
    assert [C_[n]["rows"][0][0] for n in ("trunc_minus_half", "trunc_10_7", "trunc_w_minus_tenth")] == [-0.5, 10.7, 20 - 0.1]
    assert [reg(n)[0] for n in ("trunc_minus_half", "trunc_left_of_zero", "trunc_10_7", "trunc_w_minus_tenth")] == [0, 0, 10, 19]


def test_as_i32_and_the_region_at_the_extremes():
    assert [RR.as_i32(v) for v in (1.75, -1.75, np.nan, np.inf, -np.inf, 2147483648.0, -2147483648.0, 2147483520.0, -0.5)] == \
        [1, -1, 0, 2**31 - 1, -2**31, 2**31 - 1, -2**31, 2147483520, 0]
    big = float(np.finfo(F).max)
    plain = RR.config(margin_x=0.0, margin_top=0.0, margin_bottom=0.0)
    assert RR.region([-big, -big, big, big], plain, 1920, 1080) is None                 # bw = +inf, inf * 0 = NaN
    assert RR.region([-big, -big, big, big], RR.config(), 1920, 1080) == (0, 0, 1919, 1079)
    assert RR.region([-2.0**32, -2.0**32, 2.0**32, 2.0**32], plain, 32768, 32768) == (0, 0, 32767, 32767)
    assert RR.region([2.0**31, 0, 2.0**32, 5], plain, 32768, 32768) is None
    assert RR.region([5, 5, 5, 5], RR.config(margin_x=4.0), 100, 80) == (5, 5, 5, 5)


def test_the_ellipse_sum_does_not_overflow_at_the_limit():
    cov = RR.region_cover((0, 0, 32767, 0), RR.ELLIPSE)
    assert cov.all() and cov.shape == (1, 32768)
    w = h = 32768
    dx, dy = np.int64(-32767), np.int64(257)
    assert int(dx * dx * (h * h) + dy * dy * (w * w)) == 32767**2 * 2**30 + 257**2 * 2**30 > 2**60


def test_selection_counts_and_order():
    """sel with mask and value, counts below zero and above the rows, and the independence of the row order"""
    rng = np.random.default_rng(5)
    frame = rng.integers(0, 256, (40, 50, 3), dtype=np.uint8)
    boxes = np.zeros((6, 5), F)
    boxes[:, :4] = [[2, 2, 20, 18], [15, 10, 40, 30], [30, 5, 48, 20], [0, 25, 12, 39], [22, 22, 26, 26], [np.nan, 0, 5, 5]]
    cfg = RR.config(cell=5)
    full, applied = RR.redact(frame, boxes, 6, None, cfg)
    assert applied == 5 and (full != frame).any()
    assert RR.redact(frame, boxes, -3, None, cfg)[1] == 0 and RR.redact(frame, boxes, 99, None, cfg)[1] == 5
    perm = [4, 2, 5, 0, 3, 1]
    assert RR.redact(frame, boxes[perm], 6, None, cfg)[0].tobytes() == full.tobytes()
    sel = np.array([2, 3, 0, 6, 1, 2], np.uint32)
    out, applied = RR.redact(frame, boxes, 6, sel, RR.config(cell=5, sel_mask=2, sel_value=2))
    assert applied == 3 and out.tobytes() == RR.redact(frame, boxes[[0, 1, 3]], 3, None, cfg)[0].tobytes()
    assert RR.redact(frame, boxes, 6, sel, RR.config(sel_mask=0, sel_value=1))[1] == 0          # a value outside the mask: no row
    assert RR.redact(frame, boxes, 6, sel, RR.config(sel_mask=0, sel_value=0))[1] == 5


def test_exports_header_and_binding_agree(rfd):
    header = open(os.path.join(ROOT, "include", "rfd.h")).read()
    L = rfd.load_library()
    for name in SYMBOLS:
        assert re.search(r"RFD_API\s+int\s+%s\s*\(" % name, header), name
        assert name in rfd.API_SYMBOLS and hasattr(L, name), name
        assert getattr(L, name).argtypes is not None, name
    assert callable(rfd.RetinaFaceDetection.redact_faces) and callable(rfd.redact_config)
    consts = dict(RFD_REDACT_FILL=rfd.REDACT_FILL, RFD_REDACT_PIXELATE=rfd.REDACT_PIXELATE, RFD_REDACT_RECT=rfd.REDACT_RECT,
                  RFD_REDACT_ELLIPSE=rfd.REDACT_ELLIPSE, RFD_REDACT_MAX_SIDE=rfd.REDACT_MAX_SIDE)
    assert consts == dict(RFD_REDACT_FILL=0, RFD_REDACT_PIXELATE=1, RFD_REDACT_RECT=0, RFD_REDACT_ELLIPSE=1, RFD_REDACT_MAX_SIDE=32768)
    for name, value in consts.items():
        assert re.search(r"#define %s\s+%d\b" % (name, value), header), name
    assert (RR.FILL, RR.PIXELATE, RR.RECT, RR.ELLIPSE) == (rfd.REDACT_FILL, rfd.REDACT_PIXELATE, rfd.REDACT_RECT, rfd.REDACT_ELLIPSE)
    assert header.count("CHOSEN values, not tuned on data") >= 3        # the tracker's defaults, the shot quality's and these
    hpp = open(os.path.join(ROOT, "include", "rfd.hpp")).read()
    assert "rfd_redact_faces(" in hpp and "rfd_redact_faces_device(" in hpp and "rfd_redact_config_default(" in hpp
    # the header states the rule and the limits
    for text in ("(sel[b][i] & sel_mask) == sel_value", "bw * margin_x", "as_i32(xa)", "dx^2 h^2 + dy^2 w^2 <= w^2 h^2", "(S + cnt / 2) / cnt",
                 "FRAME-ANCHORED", "no stride padding is ever written", "WEAK ON VERY LARGE FACES", "FILL is the mode", "Gaussian"):
        assert text in re.sub(r"\s*\n \*\s*", " ", header), text


def test_struct_layout(rfd):
    c = rfd.rfd_redact_config
    assert C.sizeof(c) == 60
    assert [getattr(c, f).offset for f in ("mode", "shape", "cell", "fill", "margin_x", "margin_top", "margin_bottom", "sel_mask", "sel_value", "reserved")] == \
        [0, 4, 8, 12, 16, 20, 24, 28, 32, 36]


def test_default_config(rfd):
    L = rfd.load_library()
    c = rfd.rfd_redact_config()
    C.memset(C.byref(c), 0xFF, C.sizeof(c))
    assert L.rfd_redact_config_default(C.byref(c)) == rfd.RFD_OK
    f32 = lambda x: float(F(x))
    assert (c.mode, c.shape, c.cell, list(c.fill), c.margin_x, c.margin_top, c.margin_bottom, c.sel_mask, c.sel_value) == \
        (rfd.REDACT_PIXELATE, rfd.REDACT_ELLIPSE, 16, [0, 0, 0, 0], f32(0.1), f32(0.2), f32(0.1), 0, 0)
    assert list(c.reserved) == [0] * 6
    assert L.rfd_redact_config_default(None) == rfd.RFD_ERR_INVALID_ARG
    d = RR.config()                                                       # the restatement's defaults are the library's
    assert all(f32(getattr(c, k)) == f32(v) for k, v in d.items() if k != "fill") and tuple(c.fill[:3]) == tuple(d["fill"])
    assert rfd.redact_config(cell=3).cell == 3 and list(rfd.redact_config(fill=(1, 2, 3)).fill) == [1, 2, 3, 0]
    with pytest.raises(TypeError):
        rfd.redact_config(reserved=1)


BAD = [("mode", 2), ("mode", -1), ("shape", 2), ("shape", -1), ("cell", 1), ("cell", 0), ("cell", 65), ("cell", -16), ("fill", (0, 0, 0, 1)),
       ("margin_x", -0.5), ("margin_x", 4.5), ("margin_x", float("nan")), ("margin_x", float("inf")),
       ("margin_top", -0.5), ("margin_top", 4.5), ("margin_top", float("nan")), ("margin_top", float("-inf")),
       ("margin_bottom", -0.5), ("margin_bottom", 4.5), ("margin_bottom", float("nan")), ("margin_bottom", float("inf"))]


def _call_both(L, ctx, imgs, dst, n, dets, cfg):
    yield L.rfd_redact_faces(ctx, imgs, dst, n, dets, None, cfg, None)
    yield L.rfd_redact_faces_device(ctx, imgs, dst, n, dets, None, cfg, None, 1)


@pytest.mark.parametrize("field,value", BAD)
def test_every_config_bound_is_refused_by_name_before_the_context(rfd, field, value):
    L = rfd.load_library()
    c = rfd.redact_config(**{field: value})
    for status in _call_both(L, None, None, None, 1, None, C.byref(c)):
        assert status == rfd.RFD_ERR_INVALID_ARG
        assert field in L.rfd_last_error().decode(), L.rfd_last_error()


def test_a_reserved_word_is_refused(rfd):
    L = rfd.load_library()
    for i in range(6):
        c = rfd.redact_config()
        c.reserved[i] = 1
        for status in _call_both(L, None, None, None, 1, None, C.byref(c)):
            assert status == rfd.RFD_ERR_INVALID_ARG and b"reserved" in L.rfd_last_error()


def test_null_arguments_are_refused_before_a_device_is_needed(rfd):
    L = rfd.load_library()
    img = (rfd.rfd_image * 1)()
    one = np.zeros(16, F)
    full = rfd.rfd_dets(one.ctypes.data, None, one.ctypes.data, None)              # landmarks and total are not needed
    for status in _call_both(L, None, None, None, 1, C.byref(full), None):
        assert status == rfd.RFD_ERR_INVALID_ARG and b"imgs" in L.rfd_last_error()
    for dets in (None, C.byref(rfd.rfd_dets()), C.byref(rfd.rfd_dets(one.ctypes.data, one.ctypes.data, None, None)),
                 C.byref(rfd.rfd_dets(None, one.ctypes.data, one.ctypes.data, None))):
        for status in _call_both(L, None, img, None, 1, dets, None):
            assert status == rfd.RFD_ERR_INVALID_ARG and b"dets" in L.rfd_last_error()
    for status in _call_both(L, None, img, None, -1, C.byref(full), None):
        assert status == rfd.RFD_ERR_INVALID_ARG and b"n < 0" in L.rfd_last_error()
    for n in (0, 1):
        for status in _call_both(L, None, img, img, n, C.byref(full), None):
            assert status == rfd.RFD_ERR_INVALID_ARG and b"ctx" in L.rfd_last_error()


def _build_and_run(tmp_path, name, extra):
    exe = str(tmp_path / name)
    src = os.path.join(ROOT, "tests", "cpp", "redact_plan_check.cpp")
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", src, "-o", exe] + extra, capture_output=True, text=True)
    if build.returncode != 0:
        return build
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0 and " 0 failures" in run.stdout, run.stdout + run.stderr
    m = re.search(r"(\d+) steps, (\d+) checks, 0 failures", run.stdout)
    assert m and int(m.group(1)) > 2400 and int(m.group(2)) > 6000000, run.stdout   # the program did run its cases
    return build


def test_the_plan_alone_in_a_plain_build(tmp_path):
    """tests/cpp/redact_plan_check.cpp: the regions at the int32 and f32 extremes, the ellipse sum against 128-bit arithmetic up to
    32768 x 32768, the tiles of every cell 2 .. 64 over every frame side 1 .. 200, the config and frame bounds"""
    build = _build_and_run(tmp_path, "redact_plan_check", [])
    assert build.returncode == 0, build.stderr


def test_the_plan_alone_under_address_and_ub_sanitizers(tmp_path):
    """the same program under AddressSanitizer and UBSan, as tests/test_shot_quality_cpu.py builds its own; where the sanitizer
    runtimes cannot be linked the plain build above is what ran"""
    build = _build_and_run(tmp_path, "redact_plan_check_san",
                           ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan"])
    if build.returncode != 0:
        assert "sanitize" in build.stderr or "asan" in build.stderr or "ubsan" in build.stderr, build.stderr


def test_the_plan_is_plain_host_code():
    txt = open(os.path.join(ROOT, "rs-face-detection_amd", "csrc", "redact_plan.h")).read()
    code = re.sub(r"//.*", "", txt)
    assert "#include <hip" not in code and "hipStream" not in code and "rfd_common" not in code
    # the only word of HIP is the macro that lets the kernel compile the same functions for the device
    assert [l.strip() for l in code.splitlines() if "hip" in l.lower()] == ["#if defined(__HIPCC__)"]
