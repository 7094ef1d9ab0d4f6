"""What carries over between the entries of the face stage (csrc/face_host.h: FaceStage).  Its device buffers -- the selection,
crops and status, the set-up records, the model-input planes, the packed list, the liveness staging -- are shared by every entry
of one context, grow on demand and are reused by the next call whatever it is.  One context makes six calls whose sizes make
every shared buffer both grow and be reused at a smaller size:

  1. rfd_align_faces_tensors               n = 3, crops wanted, k = 2: one config of the crop's size (the warp writes it), one of 56 x 56
  2. rfd_detect_align_all_batch            n = 2, cap = 5, k = 1 (64 x 64, resized from crops the context keeps itself), no crops
  3. rfd_liveness_tensors                  n = 1, k = 4 (80, 80, 256, 128)
  4. rfd_face_tensors                      n = 3 crops of 112 x 112, k = 2 (128 x 128 and 40 x 24)
  5. rfd_detect_select_align_tensors_batch n = 1, k = 0
  6. the first call again

and every output of every call is the bytes of the same call on a context that has made no other.  Call 2 writes into arrays
filled with a pattern: the rows past min(total, cap) keep it.  The test does not depend on how the host layer is arranged: it
passes unchanged on the commit before FaceStage existed."""
import numpy as np
import pytest

import helpers

pytestmark = pytest.mark.gpu

SIZE = (160, 160)        # the network's input: frames of 160 x 120 are letterboxed at scale 1
FILL = 0xA5
NAN_BITS = 0x7FA5A5A5


def _context(rfd, thr=None):
    d = rfd.RetinaFaceDetection(image_size=SIZE, max_batch_size=3, max_det=32)
    d.init_synthetic_weights(1234)
    if thr is not None:
        d.set_thresholds(thr, 0.45)
    return d


@pytest.fixture(scope="module")
def frames():
    return [np.ascontiguousarray(helpers.make_image(900 + i, 120, 160, n_blobs=5)) for i in range(3)]


@pytest.fixture(scope="module")
def threshold(rfd, frames):
    """Random weights score arbitrarily, so -- the idiom of test_multi_face_gpu.py -- the threshold is read off the head tensors:
    between the 4th and the 5th best foreground score of the two frames of call 2, so that at most 4 candidates exist before the
    NMS and the list of call 2 ends below its cap of 5."""
    d = _context(rfd)
    _, tn, _ = d.preprocess(frames[:2])
    heads = d.forward(tn)
    d.close()
    fg = np.sort(np.concatenate([heads[3 * l][:, 2:4].reshape(-1) for l in range(3)]))[::-1]
    assert fg[3] > fg[4], "the 4th and 5th best scores are equal"
    return float(fg[4]) + 0.5 * (float(fg[3]) - float(fg[4]))


def _prefilled_list(rfd, cfgs):
    lst = rfd.FaceList(2, 5, cfgs, want_crops=False, fill=FILL)
    for a in [lst.box, lst.kps] + lst.tensors:
        a.view(np.uint32)[...] = NAN_BITS
    return lst


def _calls(rfd, frames):
    """name -> a function of a context that makes the call and returns its outputs as a flat list of arrays"""
    q, e = rfd.face_tensor_config_quality(), rfd.face_tensor_config_extraction()
    sized = lambda c, wh: rfd.face_tensor_config(wh, list(c.mean), list(c.scale))
    sel = [tuple(reversed(helpers.make_face_kps(40 + i, 120, 160, scale_range=(0.4, 0.9)))) for i in range(3)]   # (box, kps)
    crops = np.stack([helpers.make_image(950 + i, 112, 112, n_blobs=4) for i in range(3)])
    boxes = np.array([[30.0, 20.0, 90.0, 100.0, 0.9]], np.float32)

    def align_tensors(d):
        c, status, tensors = d.align_faces_tensors(frames, sel, [q, sized(e, (56, 56))])
        return [c, status] + tensors

    def align_all(d):
        cfgs = [sized(q, (64, 64))]
        lst = d.detect_align_all(frames[:2], cfgs=cfgs, cap=5, want_crops=False, out=_prefilled_list(rfd, cfgs))
        return [lst.total, lst.first, lst.frame, lst.row, lst.status, lst.box, lst.kps] + lst.tensors

    def liveness(d):
        tensors, weights, rois, status = d.liveness_tensors(frames[2:], boxes)
        return tensors + [weights, rois, status]

    def face_tensors(d):
        return d.face_tensors(crops, [sized(q, (128, 128)), sized(e, (40, 24))])

    def select_align(d):
        selected, c, status, tensors = d.detect_select_align_tensors(frames[1:2], [])
        flat = [np.asarray(x, np.float32) for s in selected for x in s if x is not None]
        return flat + [np.array([[x is not None for x in s] for s in selected]), c, status] + tensors

    return [("align_faces_tensors", align_tensors), ("detect_align_all", align_all), ("liveness_tensors", liveness),
            ("face_tensors", face_tensors), ("detect_select_align_tensors", select_align), ("align_faces_tensors again", align_tensors)]


def _same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def test_a_sequence_of_entries_equals_each_on_a_fresh_context(rfd, frames, threshold):
    calls = _calls(rfd, frames)
    seq = _context(rfd, threshold)
    got = [(name, call(seq)) for name, call in calls]
    seq.close()
    fresh = {}
    for name, call in calls[:5]:
        d = _context(rfd, threshold)
        fresh[name] = call(d)
        d.close()
    for name, outs in got:
        want = fresh[name.replace(" again", "")]
        assert len(outs) == len(want), name
        for i, (a, w) in enumerate(zip(outs, want)):
            assert _same(a, w), (name, i)
    # the calls did something: faces were aligned, the list holds faces and ends below its cap, the tail kept the pattern
    assert (got[0][1][1] == 0).all() and got[0][1][0].any() and all(np.isfinite(t).all() and t.any() for t in got[0][1][2:])
    total, first, frame, row, status, box, kps, tensor = got[1][1]
    T = int(total[0])
    print("faces listed by call 2:", T, "first:", first.tolist())
    assert 1 <= T < 5 and first[0] == 0 and first[2] == T
    fill32 = np.frombuffer(bytes([FILL]) * 4, np.int32)[0]
    for a in (frame, row, status):
        assert (a[T:] == fill32).all() and (a[:T] != fill32).all()
    for a in (box, kps, tensor):
        assert (a[T:].view(np.uint32) == NAN_BITS).all() and np.isfinite(a[:T]).all()
    assert (got[2][1][-1] == 0).all() and all(t.any() for t in got[2][1][:4])       # liveness: status 0, four inputs written
    assert all(t.any() for t in got[3][1])
