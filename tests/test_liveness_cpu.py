"""CPU side of the liveness stage (include/rfd.h: rfd_liveness_tensors, rfd_liveness_decide and friends): known answers of the
crop geometry and of the decision rule worked by hand from the reference's formulas (face_antispoofing.rs:219-385) and checked
on tests/liveness_ref.py, the restatement the GPU tests compare the kernels with; and the new symbols, the struct layout and
the preset constants of the built library.  No GPU needed."""
import ctypes as C
import os
import re

import numpy as np

import liveness_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32

NEW_SYMBOLS = ["rfd_liveness_config_default", "rfd_liveness_tensors", "rfd_liveness_tensors_device", "rfd_liveness_decide",
               "rfd_liveness_decide_device", "rfd_face_tensor_config_quality_assessment"]

FRAME = np.zeros((240, 320, 3), np.uint8)   # 320 x 240 (w x h)


def _one(box, scale):
    r = R.face(FRAME, box, 1, [scale], [(80, 80)])
    return r["rois"][0].tolist(), r["weights"][0], r["status"], r["shifts"][0]


# ---- geometry ----------------------------------------------------------------------------------------------------------
def test_rust_casts():
    assert [R.as_i32(v) for v in (1.9, -1.9, -0.5, np.nan, np.inf, -np.inf, 3e9, -3e9, 2147483520.0)] == \
           [1, -1, 0, 0, 2147483647, -2147483648, 2147483647, -2147483648, 2147483520]
    assert R.wrap_i32(2147483647 - (-2147483648) + 1) == 0 and R.wrap_i32(-5) == -5
    assert R.f32_min(f32(np.nan), f32(2.0)) == 2.0 and R.f32_min(f32(2.0), f32(np.nan)) == 2.0
    assert R.f32_min(f32(np.inf), f32(3.0)) == 3.0 and np.isnan(R.f32_min(f32(np.nan), f32(np.nan)))


def test_crop_box_of_the_known_face():
    # det_height = 100, c_x = 140; 0.47f * 100 = 46.99999988... rounds to 47.0f: left = 93, right = 187;
    # Rect(93, 60, 187 - 93 + 1, (160 - 60 + 1.0) as i32)
    assert R.scale_image_box((100, 60, 180, 160)) == (93, 60, 95, 101)


def test_known_rois_of_the_four_models():
    r = R.face(FRAME, (100, 60, 180, 160), 1)
    # scale 1.0: min(239/101, 319/95, 1) = 1; centre (47.5 + 93, 50.5 + 60) = (140.5, 110.5); half sizes 47.5, 50.5
    assert r["rois"][3].tolist() == [93, 60, 188, 161] and r["weights"][3] == 1.0 and r["shifts"][3] == []
    # scale 2.0: half sizes 95, 101: 45.5 .. 235.5, 9.5 .. 211.5, inside the frame, truncated
    assert r["rois"][2].tolist() == [45, 9, 235, 211] and r["weights"][2] == 1.0 and r["shifts"][2] == []
    # scale 4.0 is capped by (240 - 1) / 101.  In f32 239/101 = 9925135 * 2^-22 (the exact quotient * 2^22 = 9925135.21,
    # rounded down).  new_height = 101 * that = 239 - 21 * 2^-22 exactly, which is nearer to 239.0 than to the f32 below it
    # (239 - 2^-16 = 239 - 64 * 2^-22): new_height = 239.0.  left_top_y = 110.5 - 119.5 = -9 < 0, so right_bottom_y =
    # 230 + 9 = 239 and left_top_y = 0; 239 > 239 is false: rows 0 .. 239, the whole frame height.
    # new_width = 95 * 9925135 * 2^-22 = 224.80197..., half 112.40098...: 140.5 -/+ that = 28.09.. and 252.90..
    s = f32(239.0) / f32(101.0)
    assert float(s) == 9925135 * 2.0 ** -22 and f32(101.0) * s == f32(239.0)
    assert r["rois"][0].tolist() == [28, 0, 252, 239] and r["shifts"][0] == ["top"]
    assert r["weights"][0] == s / f32(4.0) and r["weights"][0] < 1.0
    # scale 2.7 is capped the same way: the same ROI, another weight
    assert r["rois"][1].tolist() == [28, 0, 252, 239] and r["weights"][1] == s / f32(2.7) and r["weights"][1] < 1.0
    assert r["status"] == 0


def test_each_shift_branch():
    # 0.47f * 60 = 28.2000007...: a box 60 high gives left = c_x - 28.2.., right = c_x + 28.2.., truncated toward zero
    # left: Rect(-6, 80, 57, 61), centre x 22.5, 22.5 - 28.5 = -6 < 0: right_bottom_x = 51 + 6, left_top_x = 0
    assert _one((2, 80, 42, 140), 1.0) == ([0, 80, 57, 141], 1.0, 0, ["left"])
    # top: Rect(131, 2, 58, 61) at scale 2: centre y 32.5, 32.5 - 61 = -28.5 < 0: right_bottom_y = 93.5 + 28.5, left_top_y = 0
    assert _one((140, 2, 180, 62), 2.0) == ([102, 0, 218, 122], 1.0, 0, ["top"])
    # right: Rect(269, 80, 58, 61): 298 + 29 = 327 > 319: left_top_x = 269 - (327 - 320 + 1), right_bottom_x = 319
    assert _one((278, 80, 318, 140), 1.0) == ([261, 80, 319, 141], 1.0, 0, ["right"])
    # bottom: Rect(131, 178, 58, 61) at scale 2: 208.5 + 61 = 269.5 > 239: left_top_y = 147.5 - (269.5 - 240 + 1), 239
    assert _one((140, 178, 180, 238), 2.0) == ([102, 117, 218, 239], 1.0, 0, ["bottom"])


def test_degenerate_boxes():
    # ymax < ymin: Rect(144, 100, -8, -9); both ratios are negative and f32::min takes the smaller, 319 / -8 = -39.875:
    # new_width = 319, new_height = 358.875.  x: 140 - 159.5 < 0 -> 0 .. 319.  y: 95.5 - 179.4375 < 0 -> 0 .. 358.875, which
    # is > 239 -> left_top_y = 0 - (358.875 - 240 + 1) = -119.875 -> -119: Mat::roi rejects it
    assert _one((100, 100, 180, 90), 1.0) == ([0, -119, 319, 239], 0.0, -3, ["left", "top", "bottom"])
    # ymax = ymin - 1: Rect(140, 100, 0, 0); both ratios are +inf, the scale stays 1, the new box is the point (140, 100):
    # a 1 x 1 ROI, which Mat::roi and cv::resize accept
    assert _one((100, 100, 180, 99), 1.0) == ([140, 100, 140, 100], 1.0, 0, [])
    # a NaN x: c_x is NaN, left = right = 0 (`as i32`): Rect(0, 60, 1, 101), a valid two-pixel-wide ROI
    assert _one((np.nan, 60, 180, 160), 1.0) == ([0, 60, 1, 161], 1.0, 0, [])
    # a NaN y: det_height NaN -> Rect(0, 0, 1, 0); 239 / 0 = +inf leaves the scale at 1; rows 0 .. 0
    assert _one((100, np.nan, 180, 160), 1.0) == ([0, 0, 1, 0], 1.0, 0, [])
    # a box taller than the frame makes the crop box wider than the frame too (its width is 0.94 x the height):
    # Rect(-216, -200, 753, 801); every model is capped by 239 / 801, so all four take the same ROI with weights < 1
    r = R.face(FRAME, (0, -200, 320, 600), 1)
    assert r["status"] == 0 and (r["rois"] == [48, 0, 272, 239]).all() and (r["weights"] < 1.0).all()
    assert np.array_equal(r["weights"], (f32(239.0) / f32(801.0)) / np.array(R.DEFAULT_SCALES, np.float32))
    # saturating casts and the wrapping width: left = i32::MIN, right = i32::MAX, width = 2^32 wraps to 0, height saturates
    assert R.scale_image_box((0, 0, 0, 1e10)) == (-2147483648, 0, 0, 2147483647)
    assert _one((0, 0, 0, 1e10), 1.0)[2] == 0
    # no face
    r = R.face(FRAME, (100, 60, 180, 160), 0)
    assert r["status"] == -2 and not r["rois"].any() and not r["weights"].any()


def test_one_bad_model_fails_the_whole_face():
    """Rect(144, 100, -8, -9) again with two models: the reference returns Err at the first rejected ROI, so the face has no
    tensors at all"""
    r = R.face(FRAME, (100, 100, 180, 90), 1, [1.0, 2.0], [(80, 80), (80, 80)])
    assert r["status"] == -3 and not r["weights"].any()


# ---- the decision rule -------------------------------------------------------------------------------------------------
def test_decide_weighted_mean_of_four_models():
    logits = [np.array([[0.0, v, 0.0]], np.float32) for v in (0.9, 0.8, 0.25, 0.5)]
    w = np.array([[0.5, 0.75, 1.0, 1.0]], np.float32)
    score, live = R.decide(logits, w)
    # ((((0 + 0.9f*0.5) + 0.8f*0.75) + 0.25*1) + 0.5*1) / (((0.5 + 0.75) + 1) + 1), each step rounded to f32
    want = (((f32(0.9) * f32(0.5) + f32(0.8) * f32(0.75)) + f32(0.25)) + f32(0.5)) / f32(3.25)
    assert score[0] == want and abs(float(want) - 1.8 / 3.25) < 1e-6 and live[0] == 1
    assert R.decide(logits, w, threshold=0.56)[1][0] == 0


def test_decide_as_written_is_the_k_1_call():
    """_postprocess zips the four outputs with a list of one weight: only the first model counts, o0 * w0 / w0"""
    rng = np.random.default_rng(5)
    logits = [rng.uniform(0, 1, size=(1, 3)).astype(np.float32) for _ in range(4)]
    w0 = f32(239.0) / f32(101.0) / f32(4.0)
    score, live = R.decide_as_written(logits, [w0])
    want = (f32(0.0) + logits[0][0, 1] * w0) / (f32(0.0) + w0)
    assert score[0] == want and live[0] == (1 if want > f32(0.55) else 0)
    assert np.array_equal(score, R.decide(logits[:1], np.array([[w0]], np.float32))[0])
    full = R.decide(logits, np.array([[w0, 1, 1, 1]], np.float32))[0]
    assert full[0] != score[0]      # the weighted mean over all four models is another number


def test_decide_zero_weights_and_equality():
    logits = [np.array([[0.1, 0.9]], np.float32)] * 2
    score, live = R.decide(logits, np.zeros((1, 2), np.float32))
    assert np.isnan(score[0]) and live[0] == 0                      # 0 / 0, as the reference's division
    # score == threshold is not live: 0.55f * 1 / 1 = 0.55f, and `>` is strict
    eq = [np.array([[0.0, 0.55]], np.float32)]
    score, live = R.decide(eq, np.ones((1, 1), np.float32))
    assert score[0] == f32(0.55) and live[0] == 0
    above = [np.array([[0.0, np.nextafter(f32(0.55), f32(1.0))]], np.float32)]
    assert R.decide(above, np.ones((1, 1), np.float32))[1][0] == 1


# ---- the built library ---------------------------------------------------------------------------------------------------
def test_new_entry_points_are_declared_and_exported(rfd):
    txt = open(os.path.join(ROOT, "include", "rfd.h")).read()
    declared = set(re.findall(r"RFD_API\s+[\w \*]+?\b(rfd_\w+)\s*\(", txt))
    L = rfd.load_library()
    for name in NEW_SYMBOLS:
        assert name in declared, "include/rfd.h does not declare %s" % name
        assert hasattr(L, name), "librfd_hip.so does not export %s" % name
        assert name in rfd.API_SYMBOLS


def test_default_config_and_layout(rfd):
    c = rfd.liveness_config()
    assert c.k == 4 and list(c.reserved) == [0] * 4
    assert np.asarray(list(c.scale), np.float32).view(np.uint32).tolist() == np.array(R.DEFAULT_SCALES, np.float32).view(np.uint32).tolist()
    assert list(zip(c.out_w, c.out_h)) == R.DEFAULT_SIZES
    assert C.sizeof(rfd.rfd_liveness_config) == (1 + 3 * rfd.MAX_FACE_TENSORS + 4) * 4
    assert rfd.rfd_liveness_config.scale.offset == 4 and rfd.rfd_liveness_config.out_w.offset == 20 and rfd.rfd_liveness_config.out_h.offset == 36
    one = rfd.liveness_config([2.0], [(96, 80)])
    assert one.k == 1 and one.scale[0] == 2.0 and (one.out_w[0], one.out_h[0]) == (96, 80)


def test_quality_assessment_preset(rfd):
    q = rfd.face_tensor_config_quality_assessment((64, 48))
    assert (q.out_w, q.out_h) == (64, 48) and list(q.reserved) == [0] * 4
    bits = lambda v: np.asarray(v, np.float32).view(np.uint32).tolist()
    assert bits(list(q.mean)) == bits([127.5] * 3)
    assert bits(list(q.scale)) == bits([np.float32(0.00784313725)] * 3)
    assert q.scale[0] != rfd.face_tensor_config_extraction().scale[0]    # 1/127.5, not the ID model's 1/128
