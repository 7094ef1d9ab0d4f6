"""CPU side of the packed face list (include/rfd.h, "every detected face of a frame"): the numpy restatement of the list rule
(tests/face_list_ref.py, what the GPU tests hold face_list_kernel to) on hand-written cases with written-out answers; the new
symbols, the struct layouts and the default config.  No GPU needed."""
import ctypes as C
import os
import re

import numpy as np

import face_list_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NEW_SYMBOLS = ["rfd_face_list_config_default", "rfd_align_detections", "rfd_detect_align_all_batch", "rfd_detect_all_faces_device"]


def _box(x1, y1, x2, y2, s):
    return [x1, y1, x2, y2, s]


def _kps(boxes):
    """distinct key points per row: row i of a frame holds 100 i + 0 .. 9"""
    return (np.arange(len(boxes), dtype=np.float32)[:, None] * 100 + np.arange(10, dtype=np.float32)[None, :]).reshape(-1, 5, 2)


def test_predicate_on_written_out_rows():
    rows = np.array([_box(0, 0, 32, 40, 0.9),            # 32 wide, 40 high against 32: exactly the limit passes
                     _box(0, 0, 31.5, 40, 0.9),          # 31.5 < 32 fails
                     _box(0, 0, 40, 31.5, 0.9),          # the narrower side decides, whichever it is
                     _box(10, 10, 50, 50, 0.5),          # score exactly at min_score passes
                     _box(10, 10, 50, 50, 0.25),         # below it fails
                     _box(np.nan, 0, 50, 50, 0.9),       # a NaN coordinate fails ...
                     _box(0, 0, 50, np.nan, 0.9),
                     _box(0, 0, 50, 50, np.nan),         # ... and a NaN score
                     _box(50, 50, 10, 10, 0.9)], np.float32)   # an inverted box has a negative size
    assert R.row_passes(rows, 32.0, 0.5).tolist() == [True, False, False, True, False, False, False, False, False]
    assert R.row_passes(rows, 0.0, 0.0).tolist() == [True, True, True, True, True, False, False, False, False]


def test_list_rule_on_written_out_frames():
    big, small = _box(0, 0, 64, 64, 0.75), _box(0, 0, 8, 8, 0.75)
    f0 = np.array([big, small, big, big, small, big], np.float32)     # passing rows 0, 2, 3, 5
    f1 = np.zeros((0, 5), np.float32)                                 # an empty frame
    f2 = np.array([small, small], np.float32)                         # every row fails
    f3 = np.array([small, big, big], np.float32)                      # passing rows 1, 2
    dets = [(f, _kps(f)) for f in (f0, f1, f2, f3)]
    got = R.face_list(dets, max_faces=3, min_face_px=16.0, min_score=0.0, cap=100)
    assert got["total"] == 5 and got["first"].tolist() == [0, 3, 3, 3, 5]
    assert got["frame"].tolist() == [0, 0, 0, 3, 3] and got["row"].tolist() == [0, 2, 3, 1, 2]
    assert got["box"].tolist() == [big, big, big, big, big]
    assert got["kps"][:, 0].tolist() == [0.0, 200.0, 300.0, 100.0, 200.0]
    # cap drops from the end -- later frames lose first -- and truncates neither total nor first
    cut = R.face_list(dets, max_faces=3, min_face_px=16.0, min_score=0.0, cap=4)
    assert cut["total"] == 5 and cut["first"].tolist() == [0, 3, 3, 3, 5]
    assert cut["frame"].tolist() == [0, 0, 0, 3] and cut["row"].tolist() == [0, 2, 3, 1] and cut["box"].shape == (4, 5)
    # max_faces beyond what passes takes them all; 1 takes the first passing row of every frame
    assert R.face_list(dets, 10, 16.0, 0.0, 100)["row"].tolist() == [0, 2, 3, 5, 1, 2]
    assert R.face_list(dets, 1, 16.0, 0.0, 100)["row"].tolist() == [0, 1]
    # min_score cuts a prefix of a slab in descending score
    f = np.array([_box(0, 0, 64, 64, s) for s in (0.9, 0.8, 0.5, 0.4)], np.float32)
    assert R.face_list([(f, _kps(f))], 32, 0.0, 0.5, 100)["row"].tolist() == [0, 1, 2]
    none = R.face_list([(f2, _kps(f2))], 32, 16.0, 0.0, 4)
    assert none["total"] == 0 and none["first"].tolist() == [0, 0] and none["frame"].shape == (0,) and none["kps"].shape == (0, 10)


def test_new_entry_points_are_declared_and_exported(rfd):
    txt = open(os.path.join(ROOT, "include", "rfd.h")).read()
    declared = set(re.findall(r"RFD_API\s+[\w \*]+?\b(rfd_\w+)\s*\(", txt))
    L = rfd.load_library()
    for name in NEW_SYMBOLS:
        assert name in declared, "include/rfd.h does not declare %s" % name
        assert hasattr(L, name), "librfd_hip.so does not export %s" % name
        assert name in rfd.API_SYMBOLS
    for method in ("align_detections", "detect_align_all", "detect_all_faces_device"):
        assert callable(getattr(rfd.RetinaFaceDetection, method))


def test_struct_layouts_match_the_header(rfd):
    """sizeof as the header's declarations give it: i32, f32, f32, i32 [4]; eight pointers and RFD_MAX_FACE_TENSORS more"""
    txt = open(os.path.join(ROOT, "include", "rfd.h")).read()
    cfg = re.search(r"typedef struct rfd_face_list_config \{(.*?)\} rfd_face_list_config;", txt, re.S).group(1)
    fields = re.findall(r"^\s*(int32_t|float)\s+(\w+)(?:\[(\d+)\])?;", cfg, re.M)
    assert [(t, n) for t, n, _ in fields] == [("int32_t", "max_faces"), ("float", "min_face_px"), ("float", "min_score"), ("int32_t", "reserved")]
    assert C.sizeof(rfd.rfd_face_list_config) == sum(4 * int(d or 1) for _, _, d in fields) == 28
    assert [f[0] for f in rfd.rfd_face_list_config._fields_] == [n for _, n, _ in fields]
    assert rfd.rfd_face_list_config.min_face_px.offset == 4 and rfd.rfd_face_list_config.min_score.offset == 8
    lst = re.search(r"typedef struct rfd_face_list \{(.*?)\} rfd_face_list;", txt, re.S).group(1)
    ptrs = re.findall(r"^\s*(?:int32_t|float|uint8_t)\s*\*\s*(\w+)(\[RFD_MAX_FACE_TENSORS\])?;", lst, re.M)
    assert [n for n, _ in ptrs] == ["total", "first", "frame", "row", "box", "kps", "status", "crops", "tensors"]
    assert [f[0] for f in rfd.rfd_face_list._fields_] == [n for n, _ in ptrs]
    assert C.sizeof(rfd.rfd_face_list) == (8 + rfd.MAX_FACE_TENSORS) * C.sizeof(C.c_void_p)
    assert rfd.rfd_face_list.tensors.offset == 8 * C.sizeof(C.c_void_p)


def test_default_list_config(rfd):
    c = rfd.rfd_face_list_config(7, 3.0, 4.0, (C.c_int32 * 4)(1, 2, 3, 4))
    rfd.load_library().rfd_face_list_config_default(C.byref(c))
    assert c.max_faces == 32 == rfd.GALLERY_MAX_K       # one gallery search pass per frame
    assert c.min_face_px == 0.0 and c.min_score == 0.0 and list(c.reserved) == [0] * 4
    d = rfd.face_list_config(max_faces=5, min_face_px=24.0, min_score=0.5)
    assert (d.max_faces, d.min_face_px, d.min_score) == (5, 24.0, 0.5)
