"""A compiled C++ program using the track shots of rfd::Tracker (include/rfd.hpp, tests/cpp/track_shots_demo.cpp) must print the
statuses, entries, records and crop bytes that tests/track_shots_ref.py computes for its fixed scenario."""
import os
import subprocess

import numpy as np
import pytest

import track_shots_cases as SC

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEMO = os.path.join(ROOT, "rs-face-detection_amd", "build", "track_shots_demo")
F = np.float32


def _bits(word):
    return int(np.asarray([float.fromhex(word)], F).view(np.uint32)[0])


def test_cpp_program_matches_the_restatement(rfd):
    if not os.path.exists(DEMO):
        subprocess.check_call(["bash", os.path.join(ROOT, "rs-face-detection_amd", "build.sh")])
    r = subprocess.run([DEMO], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    lines = r.stdout.strip().splitlines()
    # the same scenario on the restatement (max_det 16, crops 4 x 3)
    h = SC.RefHarness()
    h.start(crop=(4, 3))
    out = h.frames([(0, [0, 1])])
    st = h.keep([0], [(0, 0, 1), (0, 1, 2), (0, 5, 1)], [10, 11, 12], q=[0.5, 0.25, 0.75], stamp=[1000])
    entries, one = h.shots(0), h.shot_crop(0, 1)
    gone = h.frames([(0, [])])
    total, first, rec, crops = h.collect([0], gone.stats, gone.ended, 4, stamp=[2000])
    assert lines[0] == "not enabled rejected %d" % rfd.RFD_ERR_INVALID_ARG and lines[1] == "default 112 112"
    assert lines[2] == "second enable rejected %d" % rfd.RFD_ERR_INVALID_ARG
    assert lines[3] == "track 1 2" and out.track[0, :2].tolist() == [1, 2]
    assert lines[4] == "status " + " ".join(str(int(s)) for s in st) and st.tolist() == [0, 0, 0]
    for i, e in enumerate(entries):
        w = lines[5 + i].split()
        assert w[0] == "entry" and [int(w[2]), int(w[4]), int(w[6]), int(w[8])] == [int(e["slot"]), int(e["serial"]), int(e["shots"]), int(e["kept"])], lines[5 + i]
        assert _bits(w[10]) == int(e["q"].view(np.uint32)) and [int(w[12]), int(w[14])] == [int(e["first_stamp"]), int(e["best_stamp"])], lines[5 + i]
    assert len(entries) == 2 and [int(e["kept"]) for e in entries] == [2, 1]
    assert lines[7].split() == ["crop", "1"] + [str(int(b)) for b in one.reshape(-1)] and one.tobytes() == h.crop(12).tobytes()
    assert lines[8] == "unknown serial rejected %d" % rfd.RFD_ERR_INVALID_ARG
    assert lines[9] == "ended 1 2" and gone.ended[0, :2].tolist() == [1, 2]
    assert lines[10] == "total %d first %d %d" % (total, first[0], first[1]) and total == 2
    for i in range(2):
        w, x = lines[11 + 2 * i].split(), rec[i]
        got = [int(w[k]) for k in (1, 3, 5, 7, 9, 11)] + [_bits(w[13])] + [int(w[k]) for k in (15, 17, 19, 21, 23)] + [_bits(w[25]), int(w[27])]
        want = [i, int(x["stream"]), int(x["serial"]), int(x["frame"]), int(x["shots"]), int(x["kept"]), int(x["q"].view(np.uint32)), int(x["first_stamp"]),
                int(x["best_stamp"]), int(x["end_stamp"]), int(x["identity"]), int(x["row"]), int(x["id_score"].view(np.uint32)), int(x["named"])]
        assert got == want, lines[11 + 2 * i]
        assert lines[12 + 2 * i].split() == ["picture", str(i)] + [str(int(b)) for b in crops[i].reshape(-1)]
    assert SC.rec_tuple(rec[0]) == (0, 1, 0, 2, 2, 0.75, 1000, 1000, 2000) and SC.rec_tuple(rec[1]) == (0, 2, 0, 1, 1, 0.25, 1000, 1000, 2000)
    assert crops[0].tobytes() == h.crop(12).tobytes() and crops[1].tobytes() == h.crop(11).tobytes() and len(lines) == 15
