"""bench.py --dump-outputs without a GPU: the detection slab of the timed step (filled here from CPU arrays) is written
as float32 / float64 .npy files, padded per image, identical from call to call, and sampled by a fixed seed above the
size limit."""
import os

import numpy as np
import torch

import bench
from rfd_hip import parallel

NAMES = ("boxes", "landmarks", "count", "total", "image_index")


def _dets(n, seed):
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        k = int(rng.integers(0, 6))
        out.append((rng.random((k, 5), dtype=np.float32), rng.random((k, 5, 2), dtype=np.float32)))
    return out


def _load(d):
    return {n: np.load(os.path.join(d, n + ".npy")) for n in NAMES}


def test_dump_outputs_of_the_local_slab(tmp_path):
    dets = _dets(6, 1)
    slab = parallel.DetectionSlab(6, bench.MAX_DET)
    slab.fill_from(dets)
    slab.boxes()[0, len(dets[0]):] = 7.0  # rows past the count are unspecified in the slab: never dumped
    bench.dump_outputs(str(tmp_path / "a"), *bench.timed_outputs(slab, None, None, 1))
    bench.dump_outputs(str(tmp_path / "b"), *bench.timed_outputs(slab, None, None, 1))
    a, b = _load(str(tmp_path / "a")), _load(str(tmp_path / "b"))
    for n in NAMES:
        assert a[n].dtype in (np.float32, np.float64), n
        np.testing.assert_array_equal(a[n], b[n])
    assert a["boxes"].shape == (6, bench.MAX_DET, 5) and a["landmarks"].shape == (6, bench.MAX_DET, 5, 2)
    np.testing.assert_array_equal(a["image_index"], np.arange(6))
    for i, (d, k) in enumerate(dets):
        assert a["count"][i] == a["total"][i] == len(d)
        np.testing.assert_array_equal(a["boxes"][i, :len(d)], d)
        np.testing.assert_array_equal(a["landmarks"][i, :len(d)], k)
        assert not a["boxes"][i, len(d):].any() and not a["landmarks"][i, len(d):].any()


def test_dump_outputs_samples_a_fixed_subset_above_the_limit(tmp_path):
    dets = _dets(10, 2)
    totals = np.arange(10) + 100
    per_image = bench.MAX_DET * 15 * 4 + 3 * 8
    for sub in ("a", "b"):
        bench.dump_outputs(str(tmp_path / sub), dets, totals, limit=4 * per_image)
    a, b = _load(str(tmp_path / "a")), _load(str(tmp_path / "b"))
    idx = a["image_index"].astype(int)
    assert len(idx) == 4 and (np.diff(idx) > 0).all()
    np.testing.assert_array_equal(a["image_index"], b["image_index"])
    assert sum(os.path.getsize(os.path.join(str(tmp_path / "a"), n + ".npy")) for n in NAMES) <= 4 * per_image + 5 * 128
    np.testing.assert_array_equal(a["total"], totals[idx])
    for j, i in enumerate(idx):
        np.testing.assert_array_equal(a["boxes"][j, :len(dets[i][0])], dets[i][0])


def test_timed_outputs_after_a_gather_are_rank_major():
    world, n = 2, 3
    slabs = []
    for r in range(world):
        s = parallel.DetectionSlab(n, bench.MAX_DET)
        s.fill_from(_dets(n, 10 + r))
        slabs.append(s)
    gathered = torch.cat([s.buf for s in slabs])
    dets, totals = bench.timed_outputs(slabs[0], None, gathered, world)
    want = slabs[0].unpack() + slabs[1].unpack()
    assert len(dets) == world * n
    for (gd, gk), (wd, wk) in zip(dets, want):
        np.testing.assert_array_equal(gd, wd)
        np.testing.assert_array_equal(gk, wk)
    np.testing.assert_array_equal(totals, np.concatenate([s.total().numpy() for s in slabs]))
