"""The builders of tests/pixel_cases.py against the CPU oracle alone, so that a failure of tests/test_pixel_edges_gpu.py points
at a kernel and not at a fixture.  The closed forms pin the oracle's resize, warp, similarity estimate and letterbox; the oracle
then judges the general geometries of the GPU sweep.  Also here: the conditions the sweep relies on -- the tie counts of the
two rounding families and the number of letterbox geometries of every class per network input."""
import collections

import numpy as np
import pytest

import pixel_cases as pc

RESIZE = pc.resize_cases()


@pytest.mark.parametrize("case", RESIZE, ids=[c[0] for c in RESIZE])
def test_resize_builders(oracle, case):
    name, src, (dh, dw), want = case
    assert want.shape == (dh, dw, 3) and want.dtype == np.uint8
    assert np.array_equal(oracle.resize_linear(src, dh, dw), want)


@pytest.mark.parametrize("along_y", [False, True])
@pytest.mark.parametrize("sn,dn", list(pc.TIE_FAMILIES))
def test_tie_families(oracle, sn, dn, along_y):
    """every unclamped column sits on a rounding tie of both coefficients (2048 and 1366 columns), and rounding half away from
    zero instead of half to even would change output pixels of the case: the case can tell the two apart"""
    src, want, tied, changed = pc.tie_case(sn, dn, along_y)
    print("%d -> %d along %s: %d tied columns, a round-half-away changes %d of %d pixels" % (sn, dn, "xy"[along_y], tied, changed, want.shape[0] * want.shape[1]))
    assert tied == pc.TIE_FAMILIES[(sn, dn)] == {(2, 4096): 2048, (3, 2048): 1366}[(sn, dn)]
    s, a0, a1, tie = pc.exact_axis(sn, dn, not along_y)
    assert np.all(a0 + a1 == 2048) and np.all((a1[tie] % 2 == 0) & (a0[tie] % 2 == 0))      # ties went to the even neighbour
    away = pc.exact_axis(sn, dn, not along_y, half_even=False)
    assert np.all((away[1] + away[2])[tie] == 2049)
    assert changed > 0 and np.array_equal(oracle.resize_linear(src, *want.shape[:2]), want)


def _frames():
    return [pc.noise(950, 97, 131), pc.noise(951, 2160, 3840)]


@pytest.fixture(scope="module")
def warp_sets():
    sets = [(f, pc.warp_cases(f)) for f in _frames()]
    wide = pc.wide_frame()
    return sets + [(wide, pc.wide_cases(wide))]


def test_warp_builders(oracle, warp_sets):
    """oracle.warp_affine with the closed-form matrix, oracle.estimate_similarity of the key points, and the two together
    (oracle.face_alignment) give the closed-form crop; the estimate is the closed-form matrix to the last bit"""
    box = np.array([0, 0, 10, 10, 0.9], np.float32)
    names = set()
    for frame, cases in warp_sets:
        for c in cases:
            tag = (frame.shape, c["name"])
            names.add(c["name"])
            assert np.array_equal(oracle.warp_affine(frame, c["M"], pc.CROP_H, pc.CROP_W), c["want"]), tag
            M, inl = oracle.estimate_similarity(c["kps"], pc.TEMPLATE, return_inliers=True)
            assert M is not None and np.array_equal(M, c["M"]), (tag, M, c["M"])
            if c["name"].startswith("displaced-"):
                k = int(c["name"][-1])
                assert not inl[k] and inl.sum() == 4, tag
            else:
                assert inl.all(), tag
            crop, st = oracle.face_alignment(frame, box, c["kps"], image_size=(pc.CROP_W, pc.CROP_H), standard_landmarks=pc.TEMPLATE)
            assert st == 0 and np.array_equal(crop, c["want"]), tag
    assert len(names) == len(warp_sets[0][1]) + len(warp_sets[2][1])


def test_warp_cases_reach_what_they_name(warp_sets):
    (small, cs), (big, cb), (wide, cw) = warp_sets
    by = {c["name"]: c for c in cs}
    assert by["shift-int"]["want"].any() and by["rot-90"]["want"].any() and by["scale-half"]["want"].any()
    for n in ("left-partly", "above-partly", "right-partly", "below-partly", "shift-frac-origin", "scale-2-over-the-corner"):
        w = by[n]["want"]
        assert w.any() and not w.reshape(-1, 3).any(1).all(), n          # some pixels from the frame, some from the border
    yy, xx = np.mgrid[0:pc.CROP_H, 0:pc.CROP_W]
    assert np.array_equal(by["rot-90"]["want"], small[xx + 97 - 30, 131 - 5 - yy])
    assert np.array_equal(by["rot-270"]["want"], small[97 - 4 - xx, yy + 131 - 25])
    far = {c["name"]: c for c in cb}["shift-frac-far"]
    assert far["kps"][:, 0].max() > 3820 and far["kps"][:, 1].max() > 2140      # coordinates near 3840 * 1024 in the fixed point
    assert cw[0]["kps"][:, 0].max() > 32767


def test_letterbox_classes(oracle):
    """The preprocess sweep of the GPU file runs every (h, w) of LETTERBOX_SIDES on three network inputs.  Every class of
    geometry -- identity, both factors 2, exactly one factor 2, upscale, generic, empty -- has at least 8 members per input."""
    for net_w, net_h in pc.LETTERBOX_NETS:
        count = collections.Counter()
        for h in pc.LETTERBOX_SIDES:
            for w in pc.LETTERBOX_SIDES:
                nw, nh, sc = oracle.geometry(h, w, net_w, net_h)
                assert nw <= net_w and nh <= net_h
                k = pc.letterbox_class(h, w, nh, nw)
                count[k] += 1
                if k == "identity":
                    assert sc == 1.0
        print("network input %dx%d:" % (net_w, net_h), dict(count))
        assert sum(count.values()) == len(pc.LETTERBOX_SIDES) ** 2
        for k in pc.LETTERBOX_CLASSES:
            assert count[k] >= 8, (net_w, net_h, k, dict(count))


def test_integer_restatement_on_the_sweeps_dyadic_geometries(oracle):
    """The GPU sweep takes resize_exact wherever both scale factors are dyadic.  Over the sweep's own sizes (crops 1 .. 17 x 3 or 6
    to 1 .. 34 x 3, transposed too, and the 4096-pixel rows) the oracle gives the same bytes on noise and on the checkerboard."""
    n = 0
    for ch in (3, 6):
        for cw in range(1, 18):
            srcs = [pc.noise(300 + cw, ch, cw), pc.checker(ch, cw)]
            for ow in range(1, 35):
                if pc.is_dyadic(cw, ow) and pc.is_dyadic(ch, 3):
                    for s in srcs:
                        assert np.array_equal(oracle.resize_linear(s, 3, ow), pc.resize_exact(s, 3, ow)), (ch, cw, ow)
                        t = np.ascontiguousarray(s.transpose(1, 0, 2))
                        assert np.array_equal(oracle.resize_linear(t, ow, 3), pc.resize_exact(t, ow, 3)), (ch, cw, ow, "y")
                    n += 1
    row = pc.noise(301, 1, 4096)
    for ow in (4096, 2048, 1):
        assert np.array_equal(oracle.resize_linear(row, 1, ow), pc.resize_exact(row, 1, ow))
    assert n >= 100 and not pc.is_dyadic(4096, 4095) and not pc.is_dyadic(5, 3)
