"""tests/face_cases.py against the CPU oracle, without a GPU: every decision a case states -- selected row, key-point row, found,
inlier mask, status, crop -- is what oracle.face_selection, oracle.estimate_similarity and oracle.face_alignment give, and the
oracle's matrix is, to the bit, the written least squares over the stated mask (for four or five exact points: the closed form).
tests/test_face_edges_gpu.py runs the same cases on the device."""
import numpy as np
import pytest

import face_cases as fc

SEL = fc.selection_cases()
ALIGN = fc.alignment_cases()
ESTIMATED = [c for c in ALIGN if c["found"] == 3]


def _bits(a):
    return np.ascontiguousarray(a, np.float64).tobytes()


def test_lmeds_sample_pairs(oracle):
    assert oracle.lmeds_samples(5).tolist() == [list(p) for p in fc.LMEDS_PAIRS]
    assert oracle.cv_ransac_num_iters(0.99, 0.45, 2, 2000) == len(fc.LMEDS_PAIRS)


def test_what_the_case_list_says_it_cannot_build():
    inside, uncovered = fc.exact_subsets_covered()
    assert len(uncovered) == 1 and "two-outliers-exact-%d-%d-%d" % uncovered[0] in fc.NOT_CONSTRUCTIBLE
    names = {c["name"] for c in ALIGN}
    assert all("two-outliers-exact-%d-%d-%d" % t in names for t in inside) and len(fc.NOT_CONSTRUCTIBLE) == 2


def test_the_cases_cover_what_the_sweep_relies_on():
    groups = {}
    for c in SEL:
        groups.setdefault((c["cfg"], c["enroll"]), []).append(c)
    assert set(groups) == {(fc.DYADIC, False), (fc.DEFAULT, False), (fc.DEFAULT, True)}
    assert {c["found"] for c in SEL} == {0, 1, 3}
    assert len({c["size"] for c in groups[(fc.DYADIC, False)]}) >= 2                    # frame sizes differ within one call
    assert any(len(c["boxes"]) == fc.MAX_DET and c["want"] == fc.MAX_DET - 1 for c in SEL)
    assert len(fc.selection_batch(groups[(fc.DYADIC, False)], 136)) == 136
    small = [c for c in ALIGN if c["cfg"] == "small"]
    assert {c["mode"] for c in small} == {0, 1, -1, -2, -3} and len(fc.alignment_batch(small, 136)) == 136
    assert sum(c["noisy"] for c in ALIGN) == 5 and all(c["cfg"] == "default" for c in ALIGN if c["noisy"])


@pytest.mark.parametrize("case", SEL, ids=[c["name"] for c in SEL])
def test_selection(oracle, case):
    H, W = case["size"]
    box, kps = oracle.face_selection(case["boxes"], case["kps"], H, W, case["enroll"], *case["cfg"])
    if case["want"] is None:
        assert box is None and kps is None
        return
    assert box.tobytes() == case["boxes"][case["want"]].tobytes()
    if case["kp"] is None:
        assert kps is None
    else:
        assert kps.tobytes() == case["kps"][case["kp"]].tobytes()


@pytest.mark.parametrize("case", ESTIMATED, ids=[c["name"] for c in ESTIMATED])
def test_estimate_and_alignment(oracle, case):
    (ow, oh), tmpl = fc.CONFIGS[case["cfg"]]
    M, inl = oracle.estimate_similarity(case["kps"], tmpl, return_inliers=True)
    if case["mask"] is None:
        assert M is None and case["mode"] in (1, -3)
    else:
        assert M is not None and case["mode"] == 0 and inl.tolist() == case["mask"]
        assert _bits(M) == _bits(fc.ls_from_mask(case["kps"], tmpl, case["mask"]))
        assert _bits(fc.invert(M.reshape(-1))) == _bits(case["M"])
    frame = fc.coded_frame(*case["size"])
    crop, st = oracle.face_alignment(frame, case["box"], case["kps"], (ow, oh), tmpl)
    assert st == {0: 0, 1: 1, -3: -1}[case["mode"]]
    assert crop.shape == (oh, ow, 3) and (case["mode"] >= 0 or not crop.any())
    if case["crop"] is not None:
        assert np.array_equal(crop, case["crop"])
