"""CPU side of the quality / ID stage glue (include/rfd.h: rfd_face_tensors and friends): the presets hold exactly the
constants of the reference (face_quality.rs:43-44, face_extraction.rs:38-39), the new entry points are declared and
exported, and the structs have the layout the header states.  No GPU needed."""
import ctypes as C
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NEW_SYMBOLS = ["rfd_face_tensor_config_quality", "rfd_face_tensor_config_extraction", "rfd_face_tensors",
               "rfd_detect_select_align_tensors_batch", "rfd_detect_faces_device", "rfd_quality_decide",
               "rfd_normalize_embeddings", "rfd_quality_decide_device", "rfd_normalize_embeddings_device"]


def _bits(values):
    return np.asarray(values, np.float32).view(np.uint32).tolist()


def test_presets_hold_the_reference_constants_to_the_bit(rfd):
    q = rfd.face_tensor_config_quality()
    assert (q.out_w, q.out_h) == (112, 112)
    assert _bits(list(q.mean)) == _bits([np.float32(123.675), np.float32(116.28), np.float32(103.53)])
    assert _bits(list(q.scale)) == _bits([np.float32(0.01712475), np.float32(0.017507), np.float32(0.01742919)])
    e = rfd.face_tensor_config_extraction()
    assert (e.out_w, e.out_h) == (112, 112)
    assert _bits(list(e.mean)) == _bits([np.float32(127.5)] * 3)
    assert _bits(list(e.scale)) == _bits([np.float32(0.0078125)] * 3)
    assert list(q.reserved) == [0] * 4 and list(e.reserved) == [0] * 4


def test_new_entry_points_are_declared_and_exported(rfd):
    txt = open(os.path.join(ROOT, "include", "rfd.h")).read()
    declared = set(re.findall(r"RFD_API\s+[\w \*]+?\b(rfd_\w+)\s*\(", txt))
    L = rfd.load_library()
    for name in NEW_SYMBOLS:
        assert name in declared, "include/rfd.h does not declare %s" % name
        assert hasattr(L, name), "librfd_hip.so does not export %s" % name
        assert name in rfd.API_SYMBOLS
    assert re.search(r"#define\s+RFD_MAX_FACE_TENSORS\s+4\b", txt) and rfd.MAX_FACE_TENSORS == 4


def test_struct_layouts(rfd):
    assert C.sizeof(rfd.rfd_face_tensor_config) == (2 + 3 + 3 + 4) * 4
    assert rfd.rfd_face_tensor_config.mean.offset == 8 and rfd.rfd_face_tensor_config.scale.offset == 20
    assert C.sizeof(rfd.rfd_faces) == (5 + rfd.MAX_FACE_TENSORS) * C.sizeof(C.c_void_p)


def test_resize_to_the_same_size_is_the_identity(oracle):
    """the copy path and the resize path of a config of the crop's own size share one expectation"""
    a = np.random.default_rng(3).integers(0, 256, size=(112, 112, 3), dtype=np.uint8)
    assert np.array_equal(oracle.resize_linear(a, 112, 112), a)
