"""The latency schedule (rfd_config.schedule = RFD_SCHEDULE_LATENCY; csrc/kernels_splitk.hip) on the GPU.

1. every op a latency pass runs with a split-K kernel, against the exact f64 per-op reference of tests/exact_ref.py -- the sweep,
   inputs, seeds and verdicts of tests/test_conv_exact_gpu.py (imported, not copied);
2. coverage: kernels_splitk.o holds exactly the kernels (1) reaches; the layers the batch-1 profile names are split; a larger
   pass and a throughput context name no split-K kernel;
3. a frame's nine head tensors are the same bits alone, in every batch size of a latency pass and at every position;
4. replays of the captured graph, eager passes and passes without side streams all give identical outputs (the arrival counters
   are left clean by every launch, and no two concurrent ops share one);
5. rfd_detect_batch equals the oracle's decode + NMS on the context's own rfd_forward heads, row for row;
6. creating a latency context does not move a throughput context's bits."""
import os
import re
import subprocess

import numpy as np
import pytest

import exact_ref  # noqa: F401  (the reference the imported sweep checks against)
import helpers
import torch_ref  # noqa: F401
from test_conv_exact_gpu import BUILD, LLVM, Sweep, _bb, _dyadic_weights, plan

pytestmark = pytest.mark.gpu

SPLITK = "conv_splitk_kernel"


def _geometries(rfd):
    nmax = rfd.LATENCY_MAX_BATCH
    geos = [("r50", 640, 640, 1), ("r50", 640, 640, 2)]
    if nmax > 2:
        geos.append(("r50", 640, 640, nmax))
    return geos + [("r50", 768, 480, 1), ("r50", 96, 64, 2), ("r50", 32, 32, 1), ("mnet025", 640, 640, 1)]


def _latency_det(rfd, bb, w, h, n, **kw):
    return rfd.RetinaFaceDetection(image_size=(w, h), max_batch_size=n, max_det=kw.pop("max_det", 16), backbone=_bb(rfd, bb),
                                   schedule=rfd.SCHEDULE_LATENCY, **kw)


def _split_cases(det, g, n):
    """the cases of the imported plan() that the schedule itself picks (tile 0) and that run a split-K kernel"""
    return [c for c in plan(det, g, n) if c[2] == 0 and any(k.startswith(SPLITK) for k in c[1])]


_reached = {}   # geometry -> kernel names, filled by the sweep and read by the coverage test


def _sweep(rfd, bb, w, h, n):
    det = _latency_det(rfd, bb, w, h, n)
    try:
        det.init_synthetic_weights(1234)
        g = rfd.Graph(_bb(rfd, bb), w, h)
        cases = _split_cases(det, g, n)
        sw = Sweep(det, g, "latency %s %dx%d" % (bb, w, h), n)
        if cases:
            sw.run_set(cases, dyadic=False, seed=11)
            _dyadic_weights(det, g, np.random.default_rng(12))
            sw.run_set(cases, dyadic=True, seed=13)
        print("\nlatency sweep %s %dx%d n=%d: %d split ops, kernels %s, %d failures, ties %d down / %d up, max undecided %.2f %%" % (
            bb, w, h, n, len(cases), sorted(k for k in sw.names if k.startswith(SPLITK)), len(sw.fail), sw.ties[0], sw.ties[1],
            100 * sw.undecided))
        return sw, cases, g
    finally:
        det.close()


def test_every_split_op_matches_the_f64_reference(rfd):
    total = 0
    for bb, w, h, n in _geometries(rfd):
        sw, cases, g = _sweep(rfd, bb, w, h, n)
        _reached[(bb, w, h, n)] = ({k for k in sw.names if k.startswith(SPLITK)}, {g.layers[g.ops[c[0]].layer].name.decode() for c in cases})
        assert not sw.fail, "\n".join(sw.fail[:12]) + ("\n... %d more" % (len(sw.fail) - 12) if len(sw.fail) > 12 else "")
        total += len(cases)
        if (bb, w, h) == ("r50", 640, 640):
            assert len(cases) >= 10 and min(sw.ties) >= 1, (len(cases), sw.ties)   # the dyadic set exercises ties-to-even here too
    assert total >= 30


def _splitk_object_kernels(tmp):
    """the name extraction of test_conv_exact_gpu._shipped_kernels, on kernels_splitk.o"""
    obj = os.path.join(BUILD, "kernels_splitk.o")
    fat, co = os.path.join(tmp, "sk.fat"), os.path.join(tmp, "sk.co")
    subprocess.run([os.path.join(LLVM, "llvm-objcopy"), "-O", "binary", "--only-section=.hip_fatbin", obj, fat], check=True)
    subprocess.run([os.path.join(LLVM, "clang-offload-bundler"), "--unbundle", "--type=o", "--input=" + fat,
                    "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", "--output=" + co], check=True)
    txt = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", co], check=True, capture_output=True, text=True).stdout
    mangled = re.findall(r"^\s+\.name:\s+(_Z\S+)", txt, re.M)
    filt = os.path.join(LLVM, "llvm-cxxfilt")
    filt = filt if os.path.exists(filt) else "c++filt"
    out = subprocess.run([filt], input="\n".join(mangled), check=True, capture_output=True, text=True).stdout
    names = set()
    for line in out.splitlines():
        s = re.sub(r"^void ", "", line.strip()).replace("rfd::", "")
        names.add(s[:s.rindex("(")] if s.endswith(")") else s)
    return names


def test_the_split_set_and_the_shipped_kernels(rfd, tmp_path):
    shipped = _splitk_object_kernels(str(tmp_path))
    assert shipped and all(k.startswith(SPLITK) for k in shipped), shipped
    reached = set()
    for bb, w, h, n in _geometries(rfd):
        if (bb, w, h, n) not in _reached:   # run alone: ask the library (nothing is launched)
            det = _latency_det(rfd, bb, w, h, n)
            try:
                det.init_synthetic_weights(1234)
                g = rfd.Graph(_bb(rfd, bb), w, h)
                cases = _split_cases(det, g, n)
                _reached[(bb, w, h, n)] = ({k for c in cases for k in c[1] if k.startswith(SPLITK)},
                                           {g.layers[g.ops[c[0]].layer].name.decode() for c in cases})
            finally:
                det.close()
        reached |= _reached[(bb, w, h, n)][0]
    assert shipped == reached, "reached but not shipped: %s; shipped without an exact-reference check: %s" % (
        sorted(reached - shipped), sorted(shipped - reached))
    # the layers the batch-1 profile names
    layers = _reached[("r50", 640, 640, 1)][1]
    print("\nsplit at R50 640x640 n = 1: %s" % sorted(layers))
    g = rfd.Graph(rfd.BACKBONE_R50, 640, 640)
    s4c2 = [L.name.decode() for L in g.layers if re.search(r"stage4.*conv2", L.name.decode())]
    assert len(s4c2) == 3, s4c2
    for name in s4c2 + ["fpn_lat3", "ssh32_conv1"]:
        assert name in layers, "%s is not split (split: %s)" % (name, sorted(layers))
    # beyond the latency batch, and in a throughput context, nothing is split
    nmax = rfd.LATENCY_MAX_BATCH
    det = _latency_det(rfd, "r50", 640, 640, nmax + 1)
    thr = rfd.RetinaFaceDetection(image_size=(640, 640), max_batch_size=1, max_det=16)
    try:
        det.init_synthetic_weights(1234)
        thr.init_synthetic_weights(1234)
        some = 0
        for i in range(g.num_ops):
            big = det.debug_op_kernels(nmax + 1, i, co_running=False)
            assert not any(SPLITK in k for k in big), (i, big)
            one = thr.debug_op_kernels(1, i, co_running=False)
            assert not any(SPLITK in k for k in one), (i, one)
            some += any(SPLITK in k for k in det.debug_op_kernels(nmax, i, co_running=False))
            assert any(SPLITK in k for k in det.debug_op_kernels(1, i, co_running=False)) == any(
                SPLITK in k for k in det.debug_op_kernels(nmax, i, co_running=False)), i   # the decision does not depend on n
            # a forced tile wins over the schedule
            det.debug_set_conv_tile(1)
            assert not any(SPLITK in k for k in det.debug_op_kernels(1, i, co_running=False)), i
            det.debug_set_conv_tile(0)
        assert some >= 10
    finally:
        det.debug_set_conv_tile(0)
        det.close()
        thr.close()


@pytest.mark.parametrize("bb,w,h", [("r50", 640, 640), ("r50", 768, 480), ("mnet025", 640, 640)])
def test_heads_do_not_depend_on_the_size_of_a_latency_pass(rfd, bb, w, h):
    nmax = rfd.LATENCY_MAX_BATCH
    det = _latency_det(rfd, bb, w, h, nmax)
    try:
        det.init_synthetic_weights(1234)
        g = rfd.Graph(_bb(rfd, bb), w, h)
        if bb == "r50":
            assert any(SPLITK in k for i in range(g.num_ops) for k in det.debug_op_kernels(1, i, co_running=False))
        rng = np.random.default_rng(21)
        frames = rng.uniform(-1.0, 1.0, size=(6 + nmax, 3, h, w)).astype(np.float32)
        alone = [det.forward(frames[k:k + 1]) for k in range(6)]
        runs = []
        for bs in range(2, nmax + 1):
            for shift in range(bs):   # every frame at every position of the batch
                for s0 in range(-shift, 6, bs):
                    idx = [s0 + j if 0 <= s0 + j < 6 else 6 + j for j in range(bs)]
                    heads = det.forward(frames[idx])
                    runs += [("B=%d pos %d" % (bs, j), idx[j], [x[j:j + 1] for x in heads]) for j in range(bs) if idx[j] < 6]
        assert len(runs) >= 12
        for tag, k, hs in runs:
            assert len(hs) == 9
            for lvl, (a, b) in enumerate(zip(hs, alone[k])):
                assert np.array_equal(a, b), "%s %dx%d frame %d, %s: head tensor %d differs from the B = 1 run (%d elements)" % (
                    bb, w, h, k, tag, lvl, int((a != b).sum()))
    finally:
        det.close()


def _head_tensors(g):
    return [t for t in range(g.num_tensors) if g.tensors[t].is_f32]


def _detect(det, g, frames):
    got = det.call_batch(frames)
    heads = [det.debug_read(t, len(frames), g.tensors[t]).copy() for t in _head_tensors(g)]
    return got, heads


def _calibrate(det, oracle, frames, w, h):
    pre = [oracle.preprocess(f, w, h) for f in frames]
    tensor = np.stack([p[1] for p in pre])
    heads = det.forward(tensor)
    fg = np.concatenate([heads[3 * l][:, 2:4].reshape(len(frames), -1) for l in range(3)], 1)
    thr = float(np.quantile(fg, 0.99))
    det.set_thresholds(thr, 0.45)
    return pre, heads, thr


@pytest.mark.parametrize("n", [1, 2])
def test_graph_replay_eager_and_single_stream_agree(rfd, oracle, n):
    det = _latency_det(rfd, "r50", 640, 640, n, max_det=1024)
    try:
        det.init_synthetic_weights(1234)
        g = rfd.Graph(rfd.BACKBONE_R50, 640, 640)
        assert len(_head_tensors(g)) == 3
        frames = [helpers.make_image(101, 720, 1000), helpers.make_image(102, 1080, 1920)][:n]
        _calibrate(det, oracle, frames, 640, 640)
        runs = [("graph call %d" % k, _detect(det, g, frames)) for k in range(5)]   # eager warm-up, capture, three replays
        det.debug_set_concurrency(multi_stream=True, split_min_part=4, split_max_parts=2, use_graph=False)
        runs += [("eager %d" % k, _detect(det, g, frames)) for k in range(2)]
        det.debug_set_concurrency(multi_stream=False, split_min_part=4, split_max_parts=2, use_graph=False)
        runs += [("one stream %d" % k, _detect(det, g, frames)) for k in range(2)]
        det.debug_set_concurrency(multi_stream=False, split_min_part=4, split_max_parts=2, use_graph=True)
        runs += [("one stream graph %d" % k, _detect(det, g, frames)) for k in range(3)]
        got0, heads0 = runs[0][1]
        assert sum(len(d) for d, _ in got0) >= 1
        for tag, (got, heads) in runs[1:]:
            for a, b in zip(heads, heads0):
                assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), "%s: head tensor differs from the first call (%d elements)" % (tag, int((a != b).sum()))
            for (d, k), (d0, k0) in zip(got, got0):
                assert np.array_equal(d, d0) and np.array_equal(k, k0), tag
    finally:
        det.close()


def test_detect_batch_matches_the_oracle_on_the_contexts_own_heads(rfd, oracle):
    det = _latency_det(rfd, "r50", 640, 640, 2, max_det=1024)
    try:
        det.init_synthetic_weights(1234)
        frames = [helpers.make_image(101, 720, 1000), helpers.make_image(102, 1080, 1920)]
        pre, heads, thr = _calibrate(det, oracle, frames, 640, 640)
        got = det.call_batch(frames)
        assert det.stats()["candidates"] >= 200
        for b in range(2):
            odet, olmk, ogidx, ncand = oracle.decode_nms([x[b] for x in heads], 640, 640, np.float32(thr), 0.45, det_scale=float(pre[b][2]))
            gdet, glmk = got[b]
            assert len(gdet) == len(odet) == det.last_total[b] and len(odet) >= 1
            assert np.array_equal(gdet, odet[:, :5]) and np.array_equal(glmk, olmk)
        # a single frame through `call` (a latency pass of 1) returns the rows it has inside the batch of 2
        d0, k0 = det.call(frames[0])
        assert np.array_equal(d0, got[0][0]) and np.array_equal(k0, got[0][1])
    finally:
        det.close()


def test_a_latency_context_does_not_move_the_throughput_bits(rfd):
    rng = np.random.default_rng(5)
    frames = rng.uniform(-1.0, 1.0, size=(2, 3, 640, 640)).astype(np.float32)

    def throughput_heads():
        det = rfd.RetinaFaceDetection(image_size=(640, 640), max_batch_size=2, max_det=16)
        try:
            det.init_synthetic_weights(1234)
            return det.forward(frames)
        finally:
            det.close()

    before = throughput_heads()
    lat = _latency_det(rfd, "r50", 640, 640, 2)
    try:
        lat.init_synthetic_weights(1234)
        lheads = lat.forward(frames)
        during = throughput_heads()   # created and run while the latency context is alive
    finally:
        lat.close()
    after = throughput_heads()
    for a, b, c in zip(before, during, after):
        assert np.array_equal(a, b) and np.array_equal(a, c)
    # the two schedules agree to bf16 rounding noise (not bit for bit: see rfd.h); the bound test_network_gpu.py holds two
    # implementations of the network to, whose bf16 activations differ by 1-ulp flips through ~55 layers
    for a, l in zip(before, lheads):
        rms = float(np.sqrt(np.mean(a.astype(np.float64) ** 2)))
        assert float(np.abs(a - l).max()) < 0.15 * rms + 2e-2
