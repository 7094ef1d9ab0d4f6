"""The tracker's boundary without a GPU (include/rfd.h, "tracker"): the exports, the struct layouts, the default config and
every argument error that needs no device."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["rfd_tracker_config_default", "rfd_tracker_create", "rfd_tracker_destroy", "rfd_tracker_update_device", "rfd_tracker_update",
           "rfd_tracker_reset", "rfd_tracker_get_tracks", "rfd_align_detections_device"]


def test_exports_header_and_binding_agree(rfd):
    header = open(os.path.join(ROOT, "include", "rfd.h")).read()
    L = rfd.load_library()
    for name in SYMBOLS:
        assert re.search(r"RFD_API\s+(int|void)\s+%s\s*\(" % name, header), name
        assert name in rfd.API_SYMBOLS and hasattr(L, name), name
        assert getattr(L, name).argtypes is not None, name
    for method in ("update", "update_device", "reset", "tracks", "close"):
        assert callable(getattr(rfd.Tracker, method)), method
    assert callable(rfd.RetinaFaceDetection.tracker) and callable(rfd.RetinaFaceDetection.align_detections_device) and callable(rfd.tracker_config)
    assert (rfd.TRACK_NEW, rfd.TRACK_CONFIRMED, rfd.TRACK_DUE) == (1, 2, 4)
    for name, value in (("RFD_TRACK_NEW", "1u"), ("RFD_TRACK_CONFIRMED", "2u"), ("RFD_TRACK_DUE", "4u"), ("RFD_TRACKER_MAX_DET", "8192")):
        assert re.search(r"#define %s %s\b" % (name, value), header), name
    assert "CHOSEN values, not tuned on data" in header      # what the defaults are, said plainly
    assert "restarts at 1" in header                           # the serial's wrap is documented


def test_struct_layouts(rfd):
    c, o, t = rfd.rfd_tracker_config, rfd.rfd_track_out, rfd.rfd_track
    assert C.sizeof(c) == 48
    assert [getattr(c, f).offset for f in ("streams", "max_tracks", "iou_min", "max_missed", "min_score", "new_score", "min_hits", "improve", "reserved")] == [0, 4, 8, 12, 16, 20, 24, 28, 32]
    assert C.sizeof(o) == 4 * 8 + 4 * 8 + 8
    assert [getattr(o, f).offset for f in ("track", "flags", "stats", "ended", "due", "due_track")] == [0, 8, 16, 24, 32, 64]
    assert C.sizeof(t) == 36
    assert [getattr(t, f).offset for f in ("slot", "serial", "box", "missed", "hits", "shot_q")] == [0, 4, 8, 24, 28, 32]


def test_default_config_without_a_context(rfd):
    L = rfd.load_library()
    c = rfd.rfd_tracker_config()
    C.memset(C.byref(c), 0xFF, C.sizeof(c))
    assert L.rfd_tracker_config_default(None, C.byref(c)) == rfd.RFD_OK
    f32 = lambda x: float(np.float32(x))
    assert (c.streams, c.max_tracks, c.iou_min, c.max_missed, c.min_score, c.new_score, c.min_hits, c.improve) == \
        (1, 64, f32(0.3), 5, f32(0.7), f32(0.7), 2, f32(1.1))
    assert list(c.reserved) == [0, 0, 0, 0]
    assert L.rfd_tracker_config_default(None, None) == rfd.RFD_ERR_INVALID_ARG


BAD = [("streams", 0), ("streams", 4097), ("max_tracks", 0), ("max_tracks", 96), ("max_tracks", 512), ("iou_min", 0.0), ("iou_min", -1.0),
       ("iou_min", float("nan")), ("iou_min", float("inf")), ("max_missed", -1), ("min_score", float("nan")), ("new_score", 0.5),
       ("new_score", float("nan")), ("min_hits", 0), ("improve", 0.5), ("improve", float("nan")), ("improve", float("inf"))]


@pytest.mark.parametrize("field,value", BAD)
def test_create_refuses_every_config_bound_and_names_the_field(rfd, field, value):
    L = rfd.load_library()
    c = rfd.rfd_tracker_config()
    L.rfd_tracker_config_default(None, C.byref(c))
    setattr(c, field, value)
    t = C.c_void_p(0x1234)
    assert L.rfd_tracker_create(None, C.byref(c), C.byref(t)) == rfd.RFD_ERR_INVALID_ARG
    assert field in L.rfd_last_error().decode() and not t.value      # judged before the context; *out is cleared


def test_null_arguments(rfd):
    L = rfd.load_library()
    c = rfd.rfd_tracker_config()
    L.rfd_tracker_config_default(None, C.byref(c))
    t = C.c_void_p()
    assert L.rfd_tracker_create(None, C.byref(c), C.byref(t)) == rfd.RFD_ERR_INVALID_ARG and b"ctx" in L.rfd_last_error()
    assert L.rfd_tracker_create(None, C.byref(c), None) == rfd.RFD_ERR_INVALID_ARG
    L.rfd_tracker_destroy(None)                                       # a no-op
    s = np.zeros(1, np.int32)
    d, o = rfd.rfd_dets(), rfd.rfd_track_out()
    assert L.rfd_tracker_update(None, s.ctypes.data, C.byref(d), None, 1, C.byref(o)) == rfd.RFD_ERR_INVALID_ARG
    assert L.rfd_tracker_update_device(None, s.ctypes.data, C.byref(d), None, 1, C.byref(o), 1) == rfd.RFD_ERR_INVALID_ARG
    assert L.rfd_tracker_reset(None, -1) == rfd.RFD_ERR_INVALID_ARG
    n = C.c_int(7)
    assert L.rfd_tracker_get_tracks(None, 0, None, 0, C.byref(n)) == rfd.RFD_ERR_INVALID_ARG and b"tracker" in L.rfd_last_error()
    fl = rfd.rfd_face_list()
    assert L.rfd_align_detections_device(None, None, 1, C.byref(d), None, None, None, 0, 1, C.byref(fl), 1) == rfd.RFD_ERR_INVALID_ARG
