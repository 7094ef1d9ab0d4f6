"""The face stage on the device -- face_select_kernel (csrc/kernels_post.hip) and align_setup_kernel with its LMedS estimate
(csrc/kernels_pre.hip) -- on the constructed cases of tests/face_cases.py: every comparison on its boundary and one f32 step
outside, gross outliers at every landmark, the sigma floor, coincident and non-finite landmarks, every branch of the fallback.

Selection: box and key points are, to the bit, the rows the case states.  Set-up: rfd_debug_align_setup returns the records the
crops hide behind their 1/32-pixel rounding; status, ROI, scales and area_fast equal the closed form, and the inverted f64 matrix
is BIT-IDENTICAL both to the written least squares over the case's stated inlier mask (plain Python floats) and to the oracle's
matrix inverted the same way -- that is how an inlier decision shows on the device.  Crops are the oracle's bytes.  One call of
136 frames or faces each puts work past thread 63 of both kernels, the outcome changing from one to the next.
tests/test_face_cases_cpu.py holds the cases against the oracle without a GPU."""
import functools

import numpy as np
import pytest

import face_cases as fc

pytestmark = pytest.mark.gpu

N_BIG = 136          # two full workgroups of 64 and a partly filled third
SEL = fc.selection_cases()
ALIGN = fc.alignment_cases()


@pytest.fixture(scope="module")
def det(rfd):
    d = rfd.RetinaFaceDetection(image_size=(32, 32), max_batch_size=N_BIG, max_det=fc.MAX_DET)   # no call here runs the network
    yield d
    d.close()


frame_of = functools.lru_cache(maxsize=None)(fc.coded_frame)


def _bits(a):
    return np.ascontiguousarray(a, np.float64).tobytes()


# ---- selection -----------------------------------------------------------------------------------------------------------
def _check_selection(det, cases):
    got = det.select_faces([(c["boxes"], c["kps"].reshape(-1, 5, 2)) for c in cases], [c["size"] for c in cases],
                           is_enroll=cases[0]["enroll"], cfg=cases[0]["cfg"])
    assert len(got) == len(cases)
    for i, (c, (box, kps)) in enumerate(zip(cases, got)):
        tag = (i, c["name"])
        if c["want"] is None:
            assert box is None and kps is None, tag
            continue
        assert box is not None and box.tobytes() == c["boxes"][c["want"]].tobytes(), tag
        if c["kp"] is None:
            assert kps is None, tag
        else:
            assert kps is not None and kps.tobytes() == c["kps"][c["kp"]].tobytes(), tag


GROUPS = sorted({(c["cfg"], c["enroll"]) for c in SEL})


@pytest.mark.parametrize("group", GROUPS, ids=["%s-%s" % ("default" if g[0] == fc.DEFAULT else "dyadic", "enrol" if g[1] else "select") for g in GROUPS])
def test_selection_cases(det, group):
    """all cases of a config and mode in one call, in order and reversed: a frame's result must not depend on its place"""
    cases = [c for c in SEL if (c["cfg"], c["enroll"]) == group]
    _check_selection(det, cases)
    _check_selection(det, cases[::-1])


def test_selection_past_thread_63(det):
    """136 frames in one call, the winning row and the frame size changing from frame to frame"""
    cases = fc.selection_batch([c for c in SEL if (c["cfg"], c["enroll"]) == (fc.DYADIC, False)], N_BIG)
    assert len({c["size"] for c in cases[64:]}) >= 2
    _check_selection(det, cases)
    enrol = fc.selection_batch([c for c in SEL if c["enroll"]], N_BIG)
    _check_selection(det, enrol)


# ---- set-up records ------------------------------------------------------------------------------------------------------
def _selected(c):
    return (c["box"], c["kps"])


def _check_setup(det, oracle, cases):
    (ow, oh), tmpl = fc.CONFIGS[cases[0]["cfg"]]
    got = det.debug_align_setup([c["size"] for c in cases], [_selected(c) for c in cases], image_size=(ow, oh), standard_landmarks=tmpl)
    for i, c in enumerate(cases):
        tag = (i, c["name"])
        assert got["mode"][i] == c["mode"], tag
        assert tuple(got["roi"][i]) == c["roi"] and got["area_fast"][i] == c["area_fast"], tag
        assert _bits(got["scale"][i]) == _bits(c["scale"]), tag
        if c["mode"] != 0:
            assert not got["M"][i].any(), tag
            continue
        assert _bits(got["M"][i]) == _bits(c["M"]), (tag, got["M"][i].tolist(), c["M"])
        M = oracle.estimate_similarity(c["kps"], tmpl)
        assert M is not None and _bits(got["M"][i]) == _bits(fc.invert(M.reshape(-1))), tag


@pytest.mark.parametrize("cfg", sorted(fc.CONFIGS))
def test_setup_records(det, oracle, cfg):
    _check_setup(det, oracle, [c for c in ALIGN if c["cfg"] == cfg])


def test_setup_records_past_thread_63(det, oracle):
    _check_setup(det, oracle, fc.alignment_batch([c for c in ALIGN if c["cfg"] == "small"], N_BIG))


# ---- crops ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _oracle_crop(oracle, index):
    c = ALIGN[index]
    (ow, oh), tmpl = fc.CONFIGS[c["cfg"]]
    return oracle.face_alignment(frame_of(*c["size"]), c["box"], c["kps"], (ow, oh), tmpl)


def _check_crops(det, oracle, cases):
    (ow, oh), tmpl = fc.CONFIGS[cases[0]["cfg"]]
    crops, status = det.align_faces([frame_of(*c["size"]) for c in cases], [_selected(c) for c in cases], image_size=(ow, oh), standard_landmarks=tmpl)
    for i, c in enumerate(cases):
        tag = (i, c["name"])
        assert status[i] == c["mode"], tag
        if c["mode"] < 0:
            assert not crops[i].any(), tag
            continue
        want, st = _oracle_crop(oracle, next(k for k, a in enumerate(ALIGN) if a is c))
        assert st == c["mode"] and np.array_equal(crops[i], want), tag
        assert c["crop"] is None or np.array_equal(crops[i], c["crop"]), tag


@pytest.mark.parametrize("cfg", sorted(fc.CONFIGS))
def test_crops(det, oracle, cfg):
    _check_crops(det, oracle, [c for c in ALIGN if c["cfg"] == cfg])


def test_crops_past_thread_63(det, oracle):
    _check_crops(det, oracle, fc.alignment_batch([c for c in ALIGN if c["cfg"] == "small"], N_BIG))
