"""The annotation without a GPU (include/rfd.h, "annotation"): the numpy restatement against every written frame of the
constructed cases, what the cases cover, the exports, the struct layout, the default config, the font through the debug hook, the
argument errors that need no device, and the plan header alone in a stand-alone program, plain and under the sanitizers."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import annotate_cases as AC
import annotate_ref as AR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["rfd_annotate_config_default", "rfd_annotate_faces_device", "rfd_annotate_faces", "rfd_debug_annotate_glyph"]
F = np.float32


@pytest.fixture(scope="module")
def font(rfd):
    return [rfd.annotate_glyph(g) for g in range(14)]


@pytest.fixture(scope="module")
def cases(font):
    return AC.cases(font)


def _inputs(c):
    boxes = np.asarray(c["rows"], F).reshape(-1, 5)
    lmk = np.asarray(c["lmk"], F).reshape(len(boxes), 10)
    count = len(boxes) if c["count"] in (None, "above") else c["count"]
    return boxes, lmk, count


def _run(c, font):
    boxes, lmk, count = _inputs(c)
    return AR.annotate(c["frame"], boxes, lmk, count, c["sel"], c["label"], c["value"], AR.config(**c["cfg"]), font)


NAMES = AC.NAMES


def test_the_list_of_the_cases_is_the_cases(cases):
    assert sorted(NAMES) == sorted(cases), set(NAMES) ^ set(cases)


@pytest.mark.parametrize("name", NAMES)
def test_the_restatement_gives_every_written_frame(cases, font, name):
    c = cases[name]
    before = c["frame"].copy()
    out, applied = _run(c, font)
    AC.check(cases, name, out, applied)
    assert c["frame"].tobytes() == before.tobytes()                     # the source is untouched


def _winning_layers(c, font):
    boxes, lmk, count = _inputs(c)
    return AR.layers(c["frame"].shape, boxes, lmk, count, c["sel"], c["label"], c["value"], AR.config(**c["cfg"]), font)[1]


def _row_alone(c, font, i):
    """the layer map of row i of a case with no other row"""
    boxes, lmk, _ = _inputs(c)
    pick = lambda a: None if a is None else [a[i]]
    return AR.layers(c["frame"].shape, boxes[i:i + 1], lmk[i:i + 1], 1, pick(c["sel"]), pick(c["label"]), pick(c["value"]), AR.config(**c["cfg"]), font)[1]


def test_the_cases_cover_what_they_claim(cases, font):
    """every layer is the winner somewhere and every skip reason occurs; the written frames differ from their sources where the
    case says something is drawn; in the winner cases each layer of a lower row lies over every layer of a higher one"""
    won = set()
    for name, c in cases.items():
        won |= set(np.unique(_winning_layers(c, font)).tolist())
        drawn = (c["want"] != c["frame"]).any()
        assert drawn == (name not in ("wholly_outside", "box_3e9_all", "count_zero", "count_negative")), name
    assert won == {0, 1, 2, 3, 4}
    # the skip reasons, each by its own row
    rows = cases["skipped_rows"]["rows"]
    cfg = AR.config(**cases["skipped_rows"]["cfg"])
    good = [i for i, r in enumerate(rows) if AR.box(r, cfg) is not None]
    assert len(rows) == 17 and good == [7] and cases["skipped_rows"]["applied"] == 1
    finite = [r for r in rows if np.isfinite(r[:4]).all()]
    assert sum(r[2] < r[0] for r in finite) == 1 and sum(r[3] < r[1] for r in finite) == 1           # !(bw >= 0), !(bh >= 0)
    with np.errstate(all="ignore"):
        assert sum(np.isinf(F(r[2]) - F(r[0])) or np.isinf(F(r[3]) - F(r[1])) for r in finite) == 2   # inf * 0: a NaN among the four
    for k in range(4):                                                   # a NaN, +inf and -inf in each coordinate
        col = [r[k] for r in rows]
        assert sum(np.isnan(v) for v in col) == 1 and sum(v == np.inf for v in col) == 1 and sum(v == -np.inf for v in col) == 1
    # a row that matches no style; counts
    c = cases["style_no_match"]
    assert [AR.style_of(w, AR.config(**c["cfg"])) for w in c["sel"]] == [0, None, 1] and c["applied"] == 2
    assert [AR.style_of(w, AR.config(**cases["style_first_match"]["cfg"])) for w in cases["style_first_match"]["sel"]] == [0, 1, 0]
    assert cases["sel_null"]["sel"] is None and {cases[n]["count"] for n in ("count_zero", "count_negative", "count_above")} == {0, -3, "above"}
    # geometry the names promise
    box = lambda n, i=0: AR.box(cases[n]["rows"][i], AR.config(**cases[n]["cfg"]))
    assert box("box_1x1") == (5, 4, 5, 4) and box("seam_63_64") == (63, 63, 64, 64) and box("trunc_minus_half")[0] == 0
    assert box("trunc_w_minus_tenth")[2] == 19 and cases["trunc_w_minus_tenth"]["frame"].shape[1] == 20
    assert box("box_3e9_left")[0] == -2**31 and box("box_3e9_all") == (-2**31, -2**31, 2**31 - 1, 2**31 - 1)
    b = box("box_thinner_than_2t")
    assert b[2] - b[0] + 1 < 2 * cases["box_thinner_than_2t"]["cfg"]["thickness"]
    assert [cases[n]["cfg"]["thickness"] for n in ("outline_t1", "outline_t2", "outline_t16")] == [1, 2, 16]
    assert [cases[n]["cfg"]["mark_radius"] for n in ("mark_r1", "mark_r2", "mark_r8")] == [1, 2, 8]
    assert [cases[n]["cfg"]["alpha"] for n in ("alpha_1", "alpha_128", "alpha_255", "alpha_256")] == [1, 128, 255, 256]
    assert cases["text_scale1_0"]["cfg"]["text_scale"] == 1 and cases["text_scale4_0"]["cfg"]["text_scale"] == 4
    for n, ya_minus_ph in (("plate_ya_minus_ph_0", 0), ("plate_ya_minus_ph_minus_1", -1)):
        assert box(n)[1] - 9 * cases[n]["cfg"]["text_scale"] == ya_minus_ph
    assert box("plate_px_negative")[0] < 0 and box("plate_past_right")[0] + 7 > cases["plate_past_right"]["frame"].shape[1]
    for side, n in enumerate(("leaves_left", "leaves_top", "leaves_right", "leaves_bottom")):
        h, w = cases[n]["frame"].shape[:2]
        b = box(n)
        assert [b[0] < 0, b[1] < 0, b[2] > w - 1, b[3] > h - 1] == [side == k for k in range(4)], n
        edge = [np.s_[:, 0], np.s_[0, :], np.s_[:, w - 1], np.s_[h - 1, :]][side]
        painted = (cases[n]["want"][edge] != cases[n]["frame"][edge]).any(axis=-1)
        assert 0 < painted.sum() <= 2, n                                 # the two crossing lines, no line along the edge
    # the strings
    strings = dict(text_scale1_0="0", text_2147483647="2147483647", text_question="?", text_dashes="--%", text_100="100%", text_999="999%",
                   text_7_50="7 50%", round_below="0%", round_at="1%", round_above="1%")
    for n, s in strings.items():
        c = cases[n]
        cfg = AR.config(**c["cfg"])
        got = AR.string(AR.text(cfg, 0 if c["label"] is None else c["label"][0], 0 if c["value"] is None else c["value"][0], c["rows"][0][4]))
        assert got == s, (n, got)
    v = [F(cases[n]["value"][0]) for n in ("round_below", "round_at", "round_above")]
    assert v[1] == F(0.005) and np.nextafter(v[0], F(1)) == v[1] and np.nextafter(v[1], F(1)) == v[2]
    # winner: for each pair lower < higher, all 16 pairs (layer of the lower, layer of the higher) occur at some pixel
    c = cases["winner_three_rows"]
    alone = [_row_alone(c, font, i) for i in range(3)]
    pairs = set()
    for lo, hi in ((0, 1), (0, 2)):
        both = (alone[lo] > 0) & (alone[hi] > 0)
        pairs |= set(zip(alone[lo][both].tolist(), alone[hi][both].tolist()))
    missing = {(a, b) for a in range(1, 5) for b in range(1, 5)} - pairs
    assert not missing, sorted(missing)
    final = _winning_layers(c, font)
    assert (final[alone[0] > 0] == alone[0][alone[0] > 0]).all()         # row 0 shows wherever it covers
    mid = (alone[0] == 0) & (alone[1] > 0)
    assert (final[mid] == alone[1][mid]).all() and (mid & (alone[2] > 0)).any()
    two = cases["winner_two_rows"]
    a2 = [_row_alone(two, font, i) for i in range(2)]
    assert {(a, b) for a, b in zip(a2[0][(a2[0] > 0) & (a2[1] > 0)].tolist(), a2[1][(a2[0] > 0) & (a2[1] > 0)].tolist())} >= {(1, 1), (2, 2), (3, 3), (4, 4)}
    # tiles: the seam cases and the tile-corner mark touch four tiles, the long string crosses x = 64
    for n in ("seam_63_64", "seam_box_across", "mark_tile_corner"):
        ys, xs = np.nonzero((cases[n]["want"] != cases[n]["frame"]).any(axis=-1))
        assert {(y // 64, x // 64) for y, x in zip(ys, xs)} >= {(0, 0), (0, 1), (1, 0), (1, 1)}, n
    xs = np.nonzero((cases["text_2147483647"]["want"] != cases["text_2147483647"]["frame"]).any(axis=-1))[1]
    assert xs.min() < 64 <= xs.max()


def test_the_painter_does_not_depend_on_how_rows_are_listed_twice(font):
    """a row listed twice changes nothing, and a row under a later copy of itself neither: the winner is by index alone"""
    rng = np.random.default_rng(3)
    frame = rng.integers(0, 256, (40, 60, 3), dtype=np.uint8)
    boxes = np.array([[5, 12, 30, 30, 0.5], [10, 15, 50, 35, 0.25], [5, 12, 30, 30, 0.5]], F)
    lmk = rng.uniform(0, 40, (3, 10)).astype(F)
    lmk[2] = lmk[0]
    cfg = AR.config(label_source=AR.ARRAY, alpha=200)
    lab = np.array([3, 4, 3], np.int32)
    a, na = AR.annotate(frame, boxes, lmk, 3, None, lab, None, cfg, font)
    b, nb = AR.annotate(frame, boxes, lmk, 2, None, lab, None, cfg, font)
    assert (na, nb) == (3, 2) and a.tobytes() == b.tobytes() and (a != frame).any()


def test_exports_header_and_binding_agree(rfd):
    header = open(os.path.join(ROOT, "include", "rfd.h")).read()
    L = rfd.load_library()
    for name in SYMBOLS:
        assert re.search(r"RFD_API\s+int\s+%s\s*\(" % name, header), name
        assert name in rfd.API_SYMBOLS and hasattr(L, name), name
        assert getattr(L, name).argtypes is not None, name
    assert callable(rfd.RetinaFaceDetection.annotate_faces) and callable(rfd.annotate_config) and callable(rfd.annotate_glyph)
    consts = dict(RFD_ANNOTATE_NONE=rfd.ANNOTATE_NONE, RFD_ANNOTATE_ARRAY=rfd.ANNOTATE_ARRAY, RFD_ANNOTATE_SCORE=rfd.ANNOTATE_SCORE,
                  RFD_ANNOTATE_MAX_STYLES=rfd.ANNOTATE_MAX_STYLES)
    assert consts == dict(RFD_ANNOTATE_NONE=0, RFD_ANNOTATE_ARRAY=1, RFD_ANNOTATE_SCORE=2, RFD_ANNOTATE_MAX_STYLES=4)
    for name, value in consts.items():
        assert re.search(r"#define %s\s+%d\b" % (name, value), header), name
    assert (AR.NONE, AR.ARRAY, AR.SCORE) == (rfd.ANNOTATE_NONE, rfd.ANNOTATE_ARRAY, rfd.ANNOTATE_SCORE)
    hpp = open(os.path.join(ROOT, "include", "rfd.hpp")).read()
    assert "rfd_annotate_faces(" in hpp and "rfd_annotate_faces_device(" in hpp and "rfd_annotate_config_default(" in hpp
    # the header states the rule
    flat = re.sub(r"\s*\n \*\s*", " ", header)
    for text in ("(s & mask_k) == value_k", "NOT clipped to the frame", "x < XA + t or x > XB - t or y < YA + t or y > YB - t",
                 "(x - cx)^2 + (y - cy)^2 <= r^2", "min(as_i32(v * 100.0f + 0.5f), 999)", "PW = s * (6 * len + 1), PH = 9 * s",
                 "PY = YA - PH if YA - PH >= 0, else YA", "k = (fx - 1) div 6 < len, u = (fx - 1) mod 6 < 5, v = fy - 1 < 7",
                 "the LOWEST row index wins", "(alpha * C + (256 - alpha) * P + 128) >> 8", "no stride padding is ever written",
                 "a row wholly outside the frame counts", "The context is checked last"):
        assert text in flat, text
    assert 'no outlines or landmarks drawn (that is "annotation" below)' in flat


def test_struct_layout(rfd):
    c, s = rfd.rfd_annotate_config, rfd.rfd_annotate_style
    assert C.sizeof(s) == 12 and [getattr(s, f).offset for f in ("sel_mask", "sel_value", "colour")] == [0, 4, 8]
    assert C.sizeof(c) == 108
    fields = ("n_styles", "style", "thickness", "mark_radius", "label_source", "value_source", "text_scale", "text_colour", "alpha", "margin_x",
              "margin_top", "margin_bottom", "reserved")
    assert [getattr(c, f).offset for f in fields] == [0, 4, 52, 56, 60, 64, 68, 72, 76, 80, 84, 88, 92]


def test_default_config(rfd):
    L = rfd.load_library()
    c = rfd.rfd_annotate_config()
    C.memset(C.byref(c), 0xFF, C.sizeof(c))
    assert L.rfd_annotate_config_default(C.byref(c)) == rfd.RFD_OK
    assert (c.n_styles, c.thickness, c.mark_radius, c.label_source, c.value_source, c.text_scale, list(c.text_colour), c.alpha, c.margin_x,
            c.margin_top, c.margin_bottom) == (1, 2, 2, rfd.ANNOTATE_NONE, rfd.ANNOTATE_SCORE, 2, [0, 0, 0, 0], 256, 0.0, 0.0, 0.0)
    assert [(s.sel_mask, s.sel_value, list(s.colour)) for s in c.style] == [(0, 0, [0, 255, 0, 0])] + [(0, 0, [0, 0, 0, 0])] * 3
    assert list(c.reserved) == [0] * 4
    assert L.rfd_annotate_config_default(None) == rfd.RFD_ERR_INVALID_ARG
    d = AR.config()                                                       # the restatement's defaults are the library's
    assert [tuple(s) for s in d["styles"]] == [(0, 0, (0, 255, 0))] and tuple(d["text_colour"]) == (0, 0, 0)
    assert all(getattr(c, k) == v for k, v in d.items() if k not in ("styles", "text_colour"))
    two = rfd.annotate_config(styles=[(1, 1, (1, 2, 3)), (0, 0, (4, 5, 6))], thickness=5, text_colour=(7, 8, 9))
    assert two.n_styles == 2 and list(two.style[1].colour) == [4, 5, 6, 0] and two.style[0].sel_mask == 1 and two.thickness == 5
    assert list(two.text_colour) == [7, 8, 9, 0] and list(two.style[2].colour) == [0] * 4
    with pytest.raises(TypeError):
        rfd.annotate_config(reserved=1)


def test_the_font_through_the_debug_hook(rfd, font):
    """14 distinct glyphs within 5 x 7; the space is empty and every other glyph is not; no digit is another's shifted copy"""
    L = rfd.load_library()
    assert len({tuple(g) for g in font}) == 14
    for g in font:
        assert len(g) == 7 and all(0 <= row < 32 for row in g)
    assert font[AR.SPACE] == [0] * 7 and all(any(g) for i, g in enumerate(font) if i != AR.SPACE)
    assert font[AR.MINUS].count(0) == 6
    for g in font[:10]:
        assert sum(bin(row).count("1") for row in g) >= 9 and g[0] and g[6]          # a digit fills its cell top to bottom
    rows = (C.c_uint8 * 7)()
    for bad in (-1, 14):
        assert L.rfd_debug_annotate_glyph(bad, C.byref(rows)) == rfd.RFD_ERR_INVALID_ARG and b"glyph" in L.rfd_last_error()
    assert L.rfd_debug_annotate_glyph(0, None) == rfd.RFD_ERR_INVALID_ARG


def _style(mask, value, colour):
    return dict(styles=[(mask, value, colour)])


BAD = [("n_styles", dict(n_styles=0)), ("n_styles", dict(n_styles=5)), ("n_styles", dict(n_styles=-1)),
       ("style", dict(styles=[(0, 0, (1, 1, 1)), (0, 0, (2, 2, 2))], n_styles=1)),
       ("colour", dict(styles=[(0, 0, (1, 1, 1, 1))])),
       ("thickness", dict(thickness=-1)), ("thickness", dict(thickness=17)), ("mark_radius", dict(mark_radius=-1)), ("mark_radius", dict(mark_radius=9)),
       ("label_source", dict(label_source=2)), ("label_source", dict(label_source=-1)), ("value_source", dict(value_source=3)),
       ("value_source", dict(value_source=-1)), ("text_scale", dict(text_scale=0)), ("text_scale", dict(text_scale=5)),
       ("text_colour", dict(text_colour=(0, 0, 0, 1))), ("alpha", dict(alpha=0)), ("alpha", dict(alpha=257)), ("alpha", dict(alpha=-256)),
       ("margin_x", dict(margin_x=-0.5)), ("margin_x", dict(margin_x=4.5)), ("margin_x", dict(margin_x=float("nan"))), ("margin_x", dict(margin_x=float("inf"))),
       ("margin_top", dict(margin_top=-0.5)), ("margin_top", dict(margin_top=4.5)), ("margin_top", dict(margin_top=float("nan"))),
       ("margin_bottom", dict(margin_bottom=-0.5)), ("margin_bottom", dict(margin_bottom=4.5)), ("margin_bottom", dict(margin_bottom=float("-inf")))]


def _call_both(L, ctx, imgs, dst, n, dets, label, value, cfg):
    yield L.rfd_annotate_faces(ctx, imgs, dst, n, dets, None, label, value, cfg, None)
    yield L.rfd_annotate_faces_device(ctx, imgs, dst, n, dets, None, label, value, cfg, None, 1)


@pytest.mark.parametrize("field,change", BAD, ids=["%s-%d" % (f, i) for i, (f, _) in enumerate(BAD)])
def test_every_config_bound_is_refused_by_name_before_the_context(rfd, field, change):
    L = rfd.load_library()
    c = rfd.annotate_config(**change)
    for status in _call_both(L, None, None, None, 1, None, None, None, C.byref(c)):
        assert status == rfd.RFD_ERR_INVALID_ARG
        assert field in L.rfd_last_error().decode(), L.rfd_last_error()


def test_a_reserved_word_is_refused(rfd):
    L = rfd.load_library()
    for i in range(4):
        c = rfd.annotate_config()
        c.reserved[i] = 1
        for status in _call_both(L, None, None, None, 1, None, None, None, C.byref(c)):
            assert status == rfd.RFD_ERR_INVALID_ARG and b"reserved" in L.rfd_last_error()


def test_null_arguments_are_refused_before_a_device_is_needed(rfd):
    L = rfd.load_library()
    img = (rfd.rfd_image * 1)()
    one = np.zeros(16, F)
    p = one.ctypes.data
    full = rfd.rfd_dets(p, p, p, None)
    for status in _call_both(L, None, None, None, 1, C.byref(full), None, None, None):
        assert status == rfd.RFD_ERR_INVALID_ARG and b"imgs" in L.rfd_last_error()
    for dets in (None, C.byref(rfd.rfd_dets()), C.byref(rfd.rfd_dets(p, p, None, None)), C.byref(rfd.rfd_dets(None, p, p, None))):
        for status in _call_both(L, None, img, None, 1, dets, None, None, None):
            assert status == rfd.RFD_ERR_INVALID_ARG and b"dets" in L.rfd_last_error()
    # the default draws marks: the landmarks are needed; with radius 0 they are not, and the context is what is missing
    for status in _call_both(L, None, img, None, 1, C.byref(rfd.rfd_dets(p, None, p, None)), None, None, None):
        assert status == rfd.RFD_ERR_INVALID_ARG and b"landmarks" in L.rfd_last_error()
    flat = rfd.annotate_config(mark_radius=0)
    for status in _call_both(L, None, img, None, 1, C.byref(rfd.rfd_dets(p, None, p, None)), None, None, C.byref(flat)):
        assert status == rfd.RFD_ERR_INVALID_ARG and b"ctx" in L.rfd_last_error()
    lab = rfd.annotate_config(label_source=rfd.ANNOTATE_ARRAY)
    for status in _call_both(L, None, img, None, 1, C.byref(full), None, p, C.byref(lab)):
        assert status == rfd.RFD_ERR_INVALID_ARG and b"label" in L.rfd_last_error()
    val = rfd.annotate_config(value_source=rfd.ANNOTATE_ARRAY)
    for status in _call_both(L, None, img, None, 1, C.byref(full), p, None, C.byref(val)):
        assert status == rfd.RFD_ERR_INVALID_ARG and b"value" in L.rfd_last_error()
    for cfg in (lab, val):
        for status in _call_both(L, None, img, None, 1, C.byref(full), p, p, C.byref(cfg)):
            assert status == rfd.RFD_ERR_INVALID_ARG and b"ctx" in L.rfd_last_error()
    for status in _call_both(L, None, img, None, -1, C.byref(full), None, None, None):
        assert status == rfd.RFD_ERR_INVALID_ARG and b"n < 0" in L.rfd_last_error()
    for n in (0, 1):
        for status in _call_both(L, None, img, img, n, C.byref(full), None, None, None):
            assert status == rfd.RFD_ERR_INVALID_ARG and b"ctx" in L.rfd_last_error()


def _build_and_run(tmp_path, name, extra):
    exe = str(tmp_path / name)
    src = os.path.join(ROOT, "tests", "cpp", "annotate_plan_check.cpp")
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", src, "-o", exe] + extra, capture_output=True, text=True)
    if build.returncode != 0:
        return build
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0 and " 0 failures" in run.stdout, run.stdout + run.stderr
    m = re.search(r"(\d+) steps, (\d+) checks, 0 failures", run.stdout)
    assert m and int(m.group(1)) > 250000 and int(m.group(2)) > 40000000, run.stdout   # the program did run its cases
    return build


def test_the_plan_alone_in_a_plain_build(tmp_path):
    """tests/cpp/annotate_plan_check.cpp: the box at the int32 and f32 ends, an_layer on clamped rows against the rule in int64 over
    a small exhaustive sweep and around +-2^20 for every thickness, radius and scale, the extent, the formatting of 0 .. 999 and of
    labels at the int32 ends, the font, the config bounds"""
    build = _build_and_run(tmp_path, "annotate_plan_check", [])
    assert build.returncode == 0, build.stderr


def test_the_plan_alone_under_address_and_ub_sanitizers(tmp_path):
    """the same program under AddressSanitizer and UBSan, as tests/test_redact_cpu.py builds its own; where the sanitizer runtimes
    cannot be linked the plain build above is what ran"""
    build = _build_and_run(tmp_path, "annotate_plan_check_san",
                           ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan"])
    if build.returncode != 0:
        assert "sanitize" in build.stderr or "asan" in build.stderr or "ubsan" in build.stderr, build.stderr


def test_the_plan_is_plain_host_code():
    txt = open(os.path.join(ROOT, "rs-face-detection_amd", "csrc", "annotate_plan.h")).read()
    code = re.sub(r"//.*", "", txt)
    assert "#include <hip" not in code and "hipStream" not in code and "rfd_common" not in code
    # the only words of HIP: the unroll hint of the device build in an_layer (the RD_HD macro comes from redact_plan.h)
    assert [l.strip() for l in code.splitlines() if "hip" in l.lower()] == ["#if defined(__HIP_DEVICE_COMPILE__)"]
