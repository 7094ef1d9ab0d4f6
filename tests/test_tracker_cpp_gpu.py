"""A compiled C++ program using rfd::Tracker of include/rfd.hpp (tests/cpp/tracker_demo.cpp) must print the ids, flags, ended
and due lists and the state that tests/tracker_ref.py computes."""
import os
import subprocess

import numpy as np
import pytest

import tracker_ref as TR
from test_tracker_gpu import _sequence

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEMO = os.path.join(ROOT, "rs-face-detection_amd", "build", "tracker_demo")


def test_cpp_program_matches_the_restatement(rfd, tmp_path):
    if not os.path.exists(DEMO):
        subprocess.check_call(["bash", os.path.join(ROOT, "rs-face-detection_amd", "build.sh")])
    rows, n_streams, per = 8, 2, 9
    seq = _sequence(55, n_streams, per, max_rows=rows)
    items = [(s, seq[s][t][0]) for t in range(per) for s in range(n_streams)]
    n = len(items)
    boxes, counts = np.zeros((n, rows, 5), np.float32), np.zeros(n, np.int32)
    for b, (_, r) in enumerate(items):
        boxes[b, :len(r)], counts[b] = r, len(r)
    streams = np.asarray([s for s, _ in items], np.int32)
    for name, a in (("b.f32", boxes), ("c.i32", counts), ("s.i32", streams)):
        a.tofile(tmp_path / name)
    cfg = dict(streams=n_streams, max_tracks=128, iou_min=0.5, max_missed=1, min_score=0.5, new_score=0.625, min_hits=2, improve=1.25)
    r = subprocess.run([DEMO, str(tmp_path / "b.f32"), str(tmp_path / "c.i32"), str(tmp_path / "s.i32"), str(rows), str(n_streams), "128", "0.5", "1", "0.5",
                        "0.625", "2", "1.25"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    lines = r.stdout.strip().splitlines()
    ref = TR.TrackerRef(**cfg)
    at = 0

    def round_():
        nonlocal at
        for b, (s, rws) in enumerate(items):
            track, flags, (matched, born, _, dropped), ended = ref.frame(s, rws)
            want = "frame %d stream %d matched %d born %d dropped %d track%s flags%s ended%s due%s" % (
                b, s, matched, born, dropped, "".join(" %d" % t for t in track), "".join(" %d" % f for f in flags),
                "".join(" %d" % e for e in ended), "".join(" %d" % i for i in np.flatnonzero(flags & TR.DUE)))
            assert lines[at] == want, at
            at += 1
        for s in range(n_streams):
            for slot, serial, box, missed, hits, shot in ref.tracks(s):
                t = lines[at].split()
                assert t[0::2][:3] == ["state", "slot", "serial"] and [int(t[1]), int(t[3]), int(t[5])] == [s, slot, serial], lines[at]
                got_box = np.asarray([float.fromhex(x) for x in t[7:11]], np.float32)
                assert got_box.tobytes() == box and [int(t[12]), int(t[14])] == [missed, hits], lines[at]
                assert int(np.asarray([float.fromhex(t[16])], np.float32).view(np.uint32)[0]) == shot, lines[at]
                at += 1

    round_()
    assert lines[at] == "reset 0"
    at += 1
    ref.reset(0)
    round_()
    assert lines[at] == "bad stream rejected %d" % rfd.RFD_ERR_INVALID_ARG and at + 1 == len(lines)
    assert any(" due " in l and not l.endswith(" due") for l in lines) and any("born 0" not in l for l in lines if l.startswith("frame"))
