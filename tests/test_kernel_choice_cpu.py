"""The kernel choice of every op, replayed without a GPU against the pinned table tests/golden/kernel_choice.json.

The table is what rfd_debug_op_kernels answered on an MI355X over three sets (tools/op_kernels.py --choice-table: the exact
sweep's geometries under every forced tile, the production plan's geometries at 1 .. 32 images, the latency schedule at 1 and 2
images; both co_running values each).  The device-free entry rfd_debug_op_kernels_static -- the same chooser
(csrc/conv_select.hip), parameters derived from the graph alone -- must reproduce every entry for the table's CU count.  A
change of a selection rule shows here, on any machine, as the entries it moves; one made on purpose regenerates the table
("kernel choice")."""
import json
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TABLE = os.path.join(ROOT, "tests", "golden", "kernel_choice.json")


def test_static_entry_reproduces_the_pinned_choice_table(rfd):
    t = json.load(open(TABLE))
    strings, cus = t["strings"], t["cus"]
    assert cus >= 1 and len(strings) >= 49   # at least the 49 conv-path kernels of the exact sweep appear
    bad, count, seen = [], 0, set()
    for e in t["entries"]:
        bb = rfd.BACKBONE_R50 if e["backbone"] == "r50" else rfd.BACKBONE_MNET025
        for op, runs in e["ops"].items():
            for first, last, sid in runs:
                for v in range(first, last + 1):
                    n, tile = (e["n"], v) if e["axis"] == "tile" else (v, e["tile"])
                    got = " + ".join(rfd.op_kernels_static(bb, e["w"], e["h"], n, int(op), co_running=bool(e["co_running"]), tile=tile,
                                                           schedule=e["schedule"], cus=cus))
                    count += 1
                    seen.add(sid)
                    if got != strings[sid]:
                        bad.append("%s %dx%d schedule %d n=%d op %s co_running %d tile %d: pinned %r, chooser %r" % (
                            e["backbone"], e["w"], e["h"], e["schedule"], n, op, e["co_running"], tile, strings[sid], got))
    print("\nkernel choice table: %d entries over %d distinct strings replayed for %d CUs, %d differ" % (count, len(strings), cus, len(bad)))
    assert count == t["entries_expanded"] >= 29600, (count, t["entries_expanded"])   # the whole table, and no smaller than the sets it is defined over
    assert seen == set(range(len(strings)))
    assert not bad, "\n".join(bad[:20]) + ("\n... %d more" % (len(bad) - 20) if len(bad) > 20 else "")


def test_static_entry_rejects_bad_arguments(rfd):
    import pytest
    for args in [(9, 640, 640, 1, 0), (rfd.BACKBONE_R50, 640, 641, 1, 0), (rfd.BACKBONE_R50, 640, 640, 0, 0), (rfd.BACKBONE_R50, 640, 640, 1, 10 ** 6)]:
        with pytest.raises(rfd.RfdError):
            rfd.op_kernels_static(*args)
    with pytest.raises(rfd.RfdError):
        rfd.op_kernels_static(rfd.BACKBONE_R50, 640, 640, 1, 0, cus=0)
