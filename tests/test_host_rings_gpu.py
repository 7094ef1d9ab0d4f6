"""The rings of page-locked slots that per-call descriptors travel through (csrc/host_resources.h: PinnedRing): more calls in
flight than a ring has slots (4).  Every round below differs from every other in what it puts into its slot, so a ring that
hands out the wrong slot, a slot of the wrong size, or one ring's event for another ring's slot changes a result.  A missing
wait is a race and cannot be caught here deterministically.  The bar is bit equality throughout: the same kernels run on the
same inputs."""
import numpy as np
import pytest

import helpers
import liveness_ref as R

pytestmark = pytest.mark.gpu

ROUNDS = 6   # through rings of 4 slots


@pytest.fixture(scope="module")
def det(rfd):
    d = rfd.RetinaFaceDetection(image_size=(640, 640), max_batch_size=2, max_det=64, backbone=rfd.BACKBONE_MNET025)
    d.init_synthetic_weights(1234)
    yield d
    d.close()


def _bits(t):
    a = t.cpu().numpy()
    return a.view(np.uint32) if a.dtype.itemsize == 4 else a


def _best_foreground(det, pair):
    _, tn, _ = det.preprocess(pair)
    heads = det.forward(tn)
    return np.concatenate([heads[3 * l][:, 2:4].reshape(len(pair), -1) for l in range(3)], 1).max(1)


def _calibrated_rounds(det):
    """Two frames per round, of sizes no other round has; the threshold by the idiom of test_liveness_gpu.py's `chain`: read
    off the head tensors, between the best foreground score of the quietest flat frame and that of the rounds' frames."""
    rounds = [[helpers.make_image(700 + 2 * r, 240 + 24 * r, 320 + 40 * r, n_blobs=5),
               helpers.make_image(701 + 2 * r, 300 + 8 * r, 200 + 16 * r, n_blobs=5)] for r in range(ROUNDS)]
    quiet = [np.zeros((240, 320, 3), np.uint8), np.full((240, 320, 3), 128, np.uint8), np.full((300, 200, 3), 255, np.uint8),
             np.full((240, 320, 3), 64, np.uint8)]
    busy = np.stack([_best_foreground(det, pair) for pair in rounds])          # [ROUNDS, 2]
    flat = np.concatenate([_best_foreground(det, quiet[0:2]), _best_foreground(det, quiet[2:4])])
    print("best foreground score per round:", busy.tolist(), "of the flat frames:", flat.tolist())
    lo, hi = float(flat.min()), float(busy.max(1).min())
    assert lo < hi, "no calibration separates the flat frame from every round"
    det.set_thresholds(lo + 0.25 * (hi - lo), 0.45)
    return rounds


def _outputs(torch, dev, n):
    z = dict(box=torch.full((n, 5), -1.0, device=dev), kps=torch.full((n, 10), -1.0, device=dev),
             found=torch.full((n,), 7, dtype=torch.int32, device=dev), status=torch.full((n,), 7, dtype=torch.int32, device=dev),
             tensor=torch.full((n, 3, 112, 112), -1.0, device=dev), weights=torch.full((n, 4), -1.0, device=dev),
             rois=torch.full((n, 4, 4), -1, dtype=torch.int32, device=dev), live_status=torch.full((n,), 7, dtype=torch.int32, device=dev))
    for j, (w, h) in enumerate(R.DEFAULT_SIZES):
        z["live%d" % j] = torch.full((n, 3, h, w), -1.0, device=dev)
    return z


def _round(rfd, det, bufs, shapes, z, async_):
    ptrs = [b.data_ptr() for b in bufs]
    det.detect_faces_device(ptrs, shapes, [rfd.face_tensor_config_quality()], z["box"].data_ptr(), z["kps"].data_ptr(), z["found"].data_ptr(),
                            None, z["status"].data_ptr(), [z["tensor"].data_ptr()], is_enroll=True, async_=async_)
    det.liveness_tensors_device(ptrs, shapes, z["box"].data_ptr(), z["found"].data_ptr(), [z["live%d" % j].data_ptr() for j in range(4)],
                                z["weights"].data_ptr(), z["rois"].data_ptr(), z["live_status"].data_ptr(), async_=async_)


def test_more_calls_in_flight_than_a_ring_has_slots(rfd, det):
    """Six rounds of rfd_detect_faces_device + rfd_liveness_tensors_device, all async, each with frames of its own size and
    outputs of its own, one rfd_sync: every round equals the same round run alone with async = 0 afterwards."""
    import torch
    dev = torch.device("cuda", 0)
    rounds = _calibrated_rounds(det)
    bufs = [[torch.from_numpy(f).to(dev) for f in pair] for pair in rounds]
    shapes = [[f.shape[:2] for f in pair] for pair in rounds]
    got = [_outputs(torch, dev, 2) for _ in rounds]
    torch.cuda.synchronize()
    for r in range(ROUNDS):
        _round(rfd, det, bufs[r], shapes[r], got[r], True)
    det.sync()
    torch.cuda.synchronize()
    for r in range(ROUNDS):
        found = got[r]["found"].cpu().numpy()
        print("round", r, "found:", found.tolist(), "liveness status:", got[r]["live_status"].cpu().tolist())
        assert (found & 1).any(), "round %d found no face: equality of empty results would prove nothing" % r
        alone = _outputs(torch, dev, 2)
        torch.cuda.synchronize()
        _round(rfd, det, bufs[r], shapes[r], alone, False)
        torch.cuda.synchronize()
        for name in alone:
            assert np.array_equal(_bits(got[r][name]), _bits(alone[name])), (r, name)


def test_a_gallery_edit_longer_than_its_ring(rfd, det):
    """dim 32, 6 000 rows, device forms only: one rfd_gallery_remove of 5 * 1024 + 7 distinct rows, then one
    rfd_gallery_replace_device of as many other rows -- six chunks each through four slots, no host wait in between.  Rows, live
    count, removed list and a masked search equal a second gallery built through the host forms."""
    import torch
    dev = torch.device("cuda", 0)
    dim, rows, n_edit = 32, 6000, 5 * 1024 + 7
    rng = np.random.default_rng(91)

    def units(n):
        x = rng.normal(size=(n, dim)).astype(np.float32)
        return x / np.linalg.norm(x, axis=1, keepdims=True).astype(np.float32)
    emb, new, q = units(rows), units(n_edit), units(33)
    gone, back = rng.permutation(rows)[:n_edit], rng.permutation(rows)[:n_edit]
    assert len(set(gone.tolist())) == n_edit and set(gone.tolist()) != set(back.tolist())
    want_removed = sorted(set(gone.tolist()) - set(back.tolist()))
    assert 0 < len(want_removed) < n_edit          # some removed rows come back, some stay removed: the search is masked

    a, b = det.gallery(dim, rows), det.gallery(dim, rows)
    d_emb, d_new, d_q = (torch.from_numpy(x).to(dev) for x in (emb, new, q))
    k = 5
    d_s, d_r = torch.zeros(33, k, device=dev), torch.zeros(33, k, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    assert a.add_device(d_emb.data_ptr(), rows) == 0
    a.remove(gone)
    a.replace_device(back, d_new.data_ptr())
    a.search_device(d_q.data_ptr(), 33, k, d_s.data_ptr(), d_r.data_ptr(), async_=True)
    det.sync()
    torch.cuda.synchronize()

    assert b.add(emb) == 0
    b.remove(gone)
    b.replace(back, new)
    want_s, want_r = b.search(q, k)
    assert a.live() == b.live() == rows - len(want_removed)
    assert a.removed().tolist() == b.removed().tolist() == want_removed
    got_rows, want_rows = a.rows(0, rows), b.rows(0, rows)
    assert np.array_equal(got_rows.view(np.uint32), want_rows.view(np.uint32))
    assert not got_rows[want_removed].any() and got_rows[back].any(1).all()
    assert np.array_equal(d_r.cpu().numpy(), want_r) and np.array_equal(_bits(d_s), want_s.view(np.uint32))
    assert not np.isin(want_r, want_removed).any() and (want_r >= 0).all()
    a.close()
    b.close()
