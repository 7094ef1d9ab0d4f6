#!/usr/bin/env python3
"""Asks the LIBRARY which kernel(s) run every op of the network (the chooser of csrc/conv_select.hip; nothing is launched).

Default mode: {op index: {"layer": name, "kernels": [...]}} as JSON for one chain size -- the op -> kernel map that
tools/traffic_model.py and tools/roof_gap.py attribute bytes and time with.  Needs the GPU (rfd_debug_op_kernels of a context).
    python tools/op_kernels.py [--batch 16] [--solo] > op_kernels.json

--choice-table OUT: the choice table tests/golden/kernel_choice.json pins (tests/test_kernel_choice_cpu.py replays it on any
machine).  Three sets, run-length encoded per op over the axis that varies:
  - every (backbone, w, h, n, ops) of test_conv_exact_gpu.GEOMETRIES x force_tile 0 .. 19 x co_running 0 / 1 (axis: tile);
  - every (backbone, w, h) of test_production_plan_gpu.GEOS x n = 1 .. 32 x co_running 0 / 1 at tile 0 (axis: n);
  - the latency schedule at n = 1, 2 for the R50 and MobileNet 640 x 640 contexts (axis: n).
From a context on the GPU by default; --static CUS asks the device-free entry (rfd_debug_op_kernels_static) instead, for a GPU of
CUS compute units, and needs no GPU.  A pull request that changes a heuristic on purpose regenerates the file and shows its diff
("kernel choice").
    python tools/op_kernels.py --choice-table tests/golden/kernel_choice.json [--static 256]"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "rs-face-detection_amd", "python"))
import rfd_hip  # noqa: E402

TILES = 20       # force_tile 0 .. 19
MAX_BATCH = 32


def _bb(name):
    return rfd_hip.BACKBONE_R50 if name == "r50" else rfd_hip.BACKBONE_MNET025


def _ops(g, ops):
    """test_conv_exact_gpu.plan()'s op subset: None = all, "large" = the stem and the 1x1 convs on maps of <= 40 rows"""
    if ops is None:
        return list(range(len(g.ops)))
    return [i for i, o in enumerate(g.ops) if o.kind == 3 or (o.kind in (2, 6) and g.layers[o.layer].kh == 1 and g.tensors[o.in_].height <= 40)]


def choice_sweeps():
    """[(backbone, w, h, schedule, axis, fixed value of the other axis, axis values, ops subset)]"""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from test_conv_exact_gpu import GEOMETRIES
    from test_production_plan_gpu import GEOS
    out = [(bb, w, h, 0, "tile", n, list(range(TILES)), ops) for bb, w, h, n, ops in GEOMETRIES]
    out += [(bb, w, h, 0, "n", 0, list(range(1, MAX_BATCH + 1)), None) for bb, w, h in GEOS]
    out += [(bb, 640, 640, 1, "n", 0, [1, 2], None) for bb in ("r50", "mnet025")]
    return out


class _Context:
    """the kernel names of (n, op, co_running, tile): from a context on the GPU, or from the device-free entry"""

    def __init__(self, bb, w, h, schedule, static_cus):
        self.key, self.cus, self.det = (_bb(bb), w, h, schedule), static_cus, None
        if not static_cus:
            self.det = rfd_hip.RetinaFaceDetection(image_size=(w, h), max_batch_size=2 if schedule else MAX_BATCH, max_det=16,
                                                   backbone=_bb(bb), schedule=schedule)
            self.det.init_synthetic_weights(1234)

    def names(self, n, op, co, tile):
        if self.det is None:
            b, w, h, schedule = self.key
            return " + ".join(rfd_hip.op_kernels_static(b, w, h, n, op, co_running=co, tile=tile, schedule=schedule, cus=self.cus))
        self.det.debug_set_conv_tile(tile)
        return " + ".join(self.det.debug_op_kernels(n, op, co_running=co))

    def close(self):
        if self.det is not None:
            self.det.debug_set_conv_tile(0)
            self.det.close()


def choice_table(static_cus=0):
    if static_cus:
        cus = static_cus
    else:
        import torch
        cus = torch.cuda.get_device_properties(0).multi_processor_count
    strings, index, entries, count = [], {}, [], 0
    ctxs = {}
    for bb, w, h, schedule, axis, fixed, values, ops in choice_sweeps():
        if (bb, w, h, schedule) not in ctxs:
            ctxs[(bb, w, h, schedule)] = _Context(bb, w, h, schedule, static_cus)
        ctx = ctxs[(bb, w, h, schedule)]
        g = rfd_hip.Graph(_bb(bb), w, h)
        for co in (0, 1):
            per_op = {}
            entries.append({"backbone": bb, "w": w, "h": h, "schedule": schedule, "co_running": co, "axis": axis,
                            "n" if axis == "tile" else "tile": fixed, "ops": per_op})
            for op in _ops(g, ops):
                runs = []
                for v in values:
                    s = ctx.names(fixed if axis == "tile" else v, op, bool(co), v if axis == "tile" else fixed)
                    sid = index.setdefault(s, len(strings))
                    if sid == len(strings):
                        strings.append(s)
                    if runs and runs[-1][2] == sid and runs[-1][1] == v - 1:
                        runs[-1][1] = v
                    else:
                        runs.append([v, v, sid])
                    count += 1
                per_op[str(op)] = runs
    for ctx in ctxs.values():
        ctx.close()
    commit = subprocess.run(["git", "-C", ROOT, "rev-parse", "HEAD"], capture_output=True, text=True).stdout.strip()
    return {"doc": "kernel choice table: tools/op_kernels.py --choice-table; runs are [first, last, index into strings] over the axis",
            "cus": cus, "source": "rfd_debug_op_kernels_static" if static_cus else "rfd_debug_op_kernels", "commit": commit or None,
            "entries_expanded": count, "strings": strings, "entries": entries}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16, help="images per chain (the timed mode runs two chains of 16)")
    ap.add_argument("--solo", action="store_true", help="a chain that has the GPU to itself (unsplit pass) instead of one of two")
    ap.add_argument("--choice-table", metavar="OUT", help="write the choice table (tests/golden/kernel_choice.json) instead")
    ap.add_argument("--static", type=int, default=0, metavar="CUS", help="with --choice-table: ask the device-free entry, for CUS compute units")
    a = ap.parse_args()
    if a.choice_table:
        t = choice_table(a.static)
        with open(a.choice_table, "w") as f:
            f.write("{\n" + ",\n".join(' %s: %s' % (json.dumps(k), json.dumps(v)) for k, v in t.items() if k != "entries"))
            f.write(',\n "entries": [\n' + ",\n".join("  " + json.dumps(e, separators=(",", ":")) for e in t["entries"]) + "\n ]\n}\n")
        print("%s: %d entries in %d runs over %d distinct strings, %d CUs" % (
            a.choice_table, t["entries_expanded"], sum(len(r) for e in t["entries"] for r in e["ops"].values()), len(t["strings"]), t["cus"]))
        return
    det = rfd_hip.RetinaFaceDetection(max_batch_size=a.batch, max_det=16)
    det.init_synthetic_weights(1234)
    g = rfd_hip.Graph()
    out = {"batch_per_chain": a.batch, "co_running": not a.solo, "ops": {}}
    for i, o in enumerate(g.ops):
        out["ops"][str(i)] = {"layer": g.layers[o.layer].name.decode(), "kind": o.kind, "kernels": det.debug_op_kernels(a.batch, i, not a.solo)}
    json.dump(out, sys.stdout, indent=1)
    print()


if __name__ == "__main__":
    main()
