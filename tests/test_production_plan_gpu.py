"""Every kernel a PRODUCTION pass picks, on the layer it picks it for, against the f64 reference of tests/exact_ref.py -- run the
way the pass runs it.

A pass of 8 or more images runs as two chains (Network::split_body): each chain picks its kernels with co_running set and by its
own size, and the second chain works on the images behind the first (batch_off != 0).  tests/test_conv_exact_gpu.py reaches every
shipped kernel, but through one chain at image 0 with co_running off, and mostly at 1-5 images.  This file closes that gap:

- production_pairs(): for every pass size B = 1 .. 32 the library itself says how the pass splits (debug_pass_chains: the code the
  pass runs, no rule restated here) and which kernel(s) every op then takes (debug_op_kernels; nothing is launched).  A "pair" is
  (op, kernel list);
- the chain sweep runs ops as the second chain of a pass: on images [batch_off, batch_off + n) of a 32-image workspace, with
  co_running as in the pass, every tensor sent as its whole workspace buffer with NaN bits outside the chain's images.  The
  chain's images get the verdicts of the exact sweep (dyadic set bit-exact, random set inside the interval, NaN overwritten on
  the written channels, other channels kept); every other byte of every buffer must come back unchanged.
  R50 and MobileNet-0.25 at 640 x 640: all ops as the chain of 16 at image 16 (the second chain of the benchmark's pass).  Every
  other production pair the exact sweep does not plan: at the smallest chain that picks it, as the second chain of the smallest
  such pass.  Both input sets on every case;
- test_every_production_choice_is_checked: every production pair is planned by the exact sweep for the same (backbone, w, h) or
  run by the chain sweep.  The chain sweep derives its cases from production_pairs(), so a change of launch_conv's heuristics that
  picks a kernel nobody checked on that layer is run against the reference from then on (and shows in the printed count of pairs
  new to the sweep); the audit is what fails should a pair ever be left out of both;
- test_context_and_device_free_choices_agree: over the enumeration tests/golden/kernel_choice.json pins (the exact sweep's geometries
  x every forced tile, these geometries x 1 .. 32 images, the latency schedule at 1 and 2 images; co_running off and on) the
  context's answer (debug_op_kernels) and the device-free entry's (op_kernels_static, asked with this device's CU count) are the
  same strings -- so what tests/test_kernel_choice_cpu.py replays without a GPU is what a context on the GPU picks."""
import time

import numpy as np
import pytest

import torch

from test_conv_exact_gpu import GEOMETRIES, TILES, Sweep, _bb, _dyadic_weights, plan

pytestmark = pytest.mark.gpu

MAX_BATCH = 32
GEOS = [("r50", 640, 640), ("r50", 768, 480), ("mnet025", 640, 640)]
CHAIN16 = {("r50", 640, 640), ("mnet025", 640, 640)}   # all ops as the second chain of the pass of 32
CHUNK = 4   # images per evaluation of the f64 reference: four f64 tensors of 4 x 256 x 160 x 160 are 0.8 GB, of 16 images 3.4 GB

_EXECUTED = {}   # (bb, w, h) -> pairs the chain sweep ran in this session


def _ctx(rfd, bb, w, h):
    det = rfd.RetinaFaceDetection(image_size=(w, h), max_batch_size=MAX_BATCH, max_det=16, backbone=_bb(rfd, bb))
    det.init_synthetic_weights(1234)
    return det, rfd.Graph(_bb(rfd, bb), w, h)


def cases_at(det, g, n, co):
    """plan()'s cases for the production heuristic (tile 0) of a chain of n images: [(op, kernel names, 0, last op of the run)];
    the conv fused into the stem's launch runs, and is checked, with the stem"""
    names = [tuple(det.debug_op_kernels(n, i, co_running=co)) for i in range(len(g.ops))]
    fused = [x[0].startswith("(fused into") for x in names]
    return [(i, names[i], 0, i + 1 if g.ops[i].kind == 3 and i + 1 < len(g.ops) and fused[i + 1] else i)
            for i in range(len(g.ops)) if not fused[i]]


def production_pairs(det, g):
    """{(op, kernel names): (chain size, co_running, first image of the chain, B)}: every pair some pass of 1 .. MAX_BATCH images
    runs, with the smallest chain that picks it -- as a chain behind another one (first image > 0) where the pass has one"""
    pairs, memo = {}, {}
    for B in range(1, MAX_BATCH + 1):
        chains = det.debug_pass_chains(B)
        assert sum(chains) == B and min(chains) >= 1, (B, chains)
        co = len(chains) > 1
        for p, c in enumerate(chains):
            if (c, co) not in memo:
                memo[(c, co)] = cases_at(det, g, c, co)
            off = sum(chains[:p])
            for i, names, _, _ in memo[(c, co)]:
                if (i, names) not in pairs or (c, off == 0) < (pairs[(i, names)][0], pairs[(i, names)][2] == 0):
                    pairs[(i, names)] = (c, co, off, B)
    return pairs


def old_pairs(det, g, bb, w, h):
    """the pairs the exact sweep plans for this (backbone, w, h), over all its chain sizes and forced tiles"""
    return {(i, names) for b, gw, gh, n, ops in GEOMETRIES if (b, gw, gh) == (bb, w, h) for i, names, _, _ in plan(det, g, n, ops)}


def chain_runs(det, g, key, prod, old):
    """[(n, batch_off, co_running, cases of the random set, cases of the dyadic set)]"""
    runs, done = [], set()
    if key in CHAIN16:
        chains = det.debug_pass_chains(MAX_BATCH)
        assert chains == [16, 16], chains
        cases = cases_at(det, g, chains[1], True)
        runs.append((chains[1], chains[0], True, cases, cases))
        done = {(c[0], c[1]) for c in cases}
    rest = {}
    for pair, (c, co, off, _) in prod.items():
        if pair not in old and pair not in done:
            rest.setdefault((c, off, co), set()).add(pair)
    for (c, off, co), ps in sorted(rest.items()):
        cases = [x for x in cases_at(det, g, c, co) if (x[0], x[1]) in ps]
        assert len(cases) == len(ps)
        runs.append((c, off, co, cases, cases))
    return runs


def _planned(runs):
    return {(c[0], c[1]) for _, _, _, rnd, _ in runs for c in rnd}


@pytest.mark.parametrize("bb,w,h", GEOS, ids=["%s-%dx%d" % k for k in GEOS])
def test_production_chains_match_the_f64_reference(rfd, bb, w, h):
    t0 = time.time()
    det, g = _ctx(rfd, bb, w, h)
    try:
        prod, old = production_pairs(det, g), old_pairs(det, g, bb, w, h)
        runs = chain_runs(det, g, (bb, w, h), prod, old)
        sweeps = [Sweep(det, g, "%s %dx%d" % (bb, w, h), n, batch_off=off, co_running=co, max_batch=MAX_BATCH, chunk=CHUNK)
                  for n, off, co, _, _ in runs]
        for sw, (_, _, _, rnd, _) in zip(sweeps, runs):
            sw.run_set(rnd, dyadic=False, seed=11)
        _dyadic_weights(det, g, np.random.default_rng(12))
        for sw, (_, _, _, _, dya) in zip(sweeps, runs):
            sw.run_set(dya, dyadic=True, seed=13)
        fail = [f for sw in sweeps for f in sw.fail]
        for sw, (n, off, co, rnd, dya) in zip(sweeps, runs):
            print("\nchain sweep %s %dx%d chain of %d at image %d%s: %d + %d cases (random + dyadic), %d kernel names, %d failures, "
                  "ties %d down / %d up, max undecided %.2f %%, head |got - v64| / r max %.3f" % (
                      bb, w, h, n, off, ", co-running" if co else "", len(rnd), len(dya), len(sw.names), len(sw.fail), sw.ties[0],
                      sw.ties[1], 100 * sw.undecided, sw.ratio))
            assert sw.cases == len(rnd) + len(dya)
        print("chain sweep %s %dx%d: %d runs, %.0f s" % (bb, w, h, len(runs), time.time() - t0))
        assert not fail, "\n".join(fail[:12]) + ("\n... %d more" % (len(fail) - 12) if len(fail) > 12 else "")
        executed = set().union(*[sw.pairs for sw in sweeps]) if sweeps else set()
        assert executed == _planned(runs)
        _EXECUTED[(bb, w, h)] = executed
        if (bb, w, h) in CHAIN16:
            assert {c[0] for c in runs[0][3]} | {c[3] for c in runs[0][3]} == set(range(len(g.ops))), "the chain of 16 skips an op"
            assert min(sweeps[0].ties) >= 200 and sum(sweeps[0].ties) >= 2000, sweeps[0].ties   # as the exact sweep: ties-to-even are met
            if bb == "r50":
                assert 0 < sweeps[0].ratio <= 1.0, sweeps[0].ratio
    finally:
        det.close()


@pytest.mark.parametrize("bb,w,h", GEOS, ids=["%s-%dx%d" % k for k in GEOS])
def test_every_production_choice_is_checked(rfd, bb, w, h):
    det, g = _ctx(rfd, bb, w, h)
    try:
        prod, old = production_pairs(det, g), old_pairs(det, g, bb, w, h)
        chain = _planned(chain_runs(det, g, (bb, w, h), prod, old))
        if (bb, w, h) in _EXECUTED:   # the sweep above ran in this session: what it executed, not what it meant to
            assert _EXECUTED[(bb, w, h)] == chain
        missed = sorted(p for p in prod if p not in old)
        print("\nproduction plan %s %dx%d: %d (op, kernels) pairs over passes of 1 .. %d images; the exact sweep plans %d pairs for this "
              "geometry and misses %d of production's; the chain sweep runs %d pairs" % (bb, w, h, len(prod), MAX_BATCH, len(old),
                                                                                          len(missed), len(chain)))
        for i, names in missed:
            c, co, off, B = prod[(i, names)]
            print("  new to the sweep: op %d (%s) %s, chain of %d at image %d of a pass of %d" % (
                i, g.layers[g.ops[i].layer].name.decode(), " + ".join(names), c, off, B))
        assert len(prod) >= len(g.ops) - 1 > 0, len(prod)   # every op but the conv fused into the stem has at least one choice
        unchecked = ["op %d (%s, kind %d): %s, picked by a pass of B = %d for its chain of %d images" % (
            i, g.layers[g.ops[i].layer].name.decode(), g.ops[i].kind, " + ".join(names), prod[(i, names)][3], prod[(i, names)][0])
            for i, names in sorted(prod) if (i, names) not in old and (i, names) not in chain]
        assert not unchecked, "production picks kernels no test checks on that layer:\n" + "\n".join(unchecked)
    finally:
        det.close()


def test_context_and_device_free_choices_agree(rfd):
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    sweeps = [(bb, w, h, 0, [(n, t) for t in TILES], ops) for bb, w, h, n, ops in GEOMETRIES]
    sweeps += [(bb, w, h, 0, [(n, 0) for n in range(1, MAX_BATCH + 1)], None) for bb, w, h in GEOS]
    sweeps += [(bb, 640, 640, rfd.SCHEDULE_LATENCY, [(1, 0), (2, 0)], None) for bb in ("r50", "mnet025")]
    count, bad = 0, []
    for bb, w, h, schedule, points, ops in sweeps:
        det = rfd.RetinaFaceDetection(image_size=(w, h), max_batch_size=max(n for n, _ in points), max_det=16, backbone=_bb(rfd, bb), schedule=schedule)
        try:
            det.init_synthetic_weights(1234)
            g = rfd.Graph(_bb(rfd, bb), w, h)
            idx = range(len(g.ops)) if ops is None else [i for i, o in enumerate(g.ops) if o.kind == 3 or (
                o.kind in (2, 6) and g.layers[o.layer].kh == 1 and g.tensors[o.in_].height <= 40)]
            for n, tile in points:
                det.debug_set_conv_tile(tile)
                for co in (False, True):
                    for i in idx:
                        ctx = det.debug_op_kernels(n, i, co_running=co)
                        free = rfd.op_kernels_static(_bb(rfd, bb), w, h, n, i, co_running=co, tile=tile, schedule=schedule, cus=cus)
                        count += 1
                        if ctx != free:
                            bad.append("%s %dx%d schedule %d n=%d op %d co_running %d tile %d: context %s, device-free %s" % (
                                bb, w, h, schedule, n, i, co, tile, ctx, free))
        finally:
            det.debug_set_conv_tile(0)
            det.close()
    print("\nkernel choice: %d (geometry, n, op, co_running, tile) points, context vs device-free entry at %d CUs: %d differ" % (count, cus, len(bad)))
    assert count >= 29600
    assert not bad, "\n".join(bad[:20]) + ("\n... %d more" % (len(bad) - 20) if len(bad) > 20 else "")
