"""A compiled C++ program using the track identities of rfd::Tracker (include/rfd.hpp, tests/cpp/track_identity_demo.cpp) must
print the statuses, queries, answers, entries and template that tests/track_identity_ref.py computes for its fixed scenario."""
import os
import subprocess

import numpy as np
import pytest

import track_identity_cases as IC

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEMO = os.path.join(ROOT, "rs-face-detection_amd", "build", "track_identity_demo")
F = np.float32
INF = float("inf")


def _bits(words):
    return np.asarray([float.fromhex(w) for w in words], F).view(np.uint32).tolist()


def test_cpp_program_matches_the_restatement(rfd):
    if not os.path.exists(DEMO):
        subprocess.check_call(["bash", os.path.join(ROOT, "rs-face-detection_amd", "build.sh")])
    r = subprocess.run([DEMO], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    lines = r.stdout.strip().splitlines()
    # the same scenario on the restatement (max_det 16, dim 96)
    h = IC.RefHarness()
    h.start(dim=96, accept=0.5, release=0.25, margin=0.125)
    track, _, _ = h.frames([(0, [0, 1, 2])])
    d = h.dim
    obs = [(0, 0, 1), (0, 1, 2), (0, 2, 3), (0, 5, 2)]
    q, st = h.fuse([0], obs, [IC.vec(d, {0: 3, 1: 4}), IC.vec(d, {0: 2}), IC.vec(d, {1: 5, 2: 12}), IC.vec(d, {1: 7})], weight=[1, 3, 2, 4])
    h.label([0], obs, [[(0.75, 3, 7), (0.2, 8, 9)], [(0.3, 3, 7), (0.1, 8, 9)], [(0.875, 4, -1), (-INF, -1, -1)], [(0.75, 5, 8), (0.6875, 3, 7)]], st)
    who, ident, score = h.who([0], [[1, 2, 3]], [3], flags=[[3, 3, 3]])       # min_hits 1: NEW | CONFIRMED... DUE is added below
    assert lines[0] == "not enabled rejected %d" % rfd.RFD_ERR_INVALID_ARG and lines[1] == "second enable rejected %d" % rfd.RFD_ERR_INVALID_ARG
    assert lines[2] == "track 1 2 3" and track[0, :3].tolist() == [1, 2, 3]
    for t in range(4):
        w = lines[3 + t].split()
        assert w[:4] == ["fuse", str(t), "status", str(int(st[t]))] and w[4] == "query", lines[3 + t]
        assert _bits(w[5:]) == q[t].view(np.uint32).tolist(), t
    assert st.tolist() == [0, 0, 0, 0]
    for i in range(3):
        w = lines[7 + i].split()
        # the demo passes update's flags on: NEW | CONFIRMED | DUE = 7 for a born row of a min_hits 1 tracker
        assert [w[0], int(w[1]), int(w[2]) & 8, int(w[2]) & 7, int(w[3])] == ["who", i, int(who[0, i]) & 8, 7, int(ident[0, i])], lines[7 + i]
        assert _bits(w[4:5]) == score[0, i:i + 1].view(np.uint32).tolist()
    assert [int(x) & 8 for x in who[0, :3]] == [8, 0, 8] and ident[0, :3].tolist() == [7, -1, -1]
    at = 10
    for e in h.entries(0):
        w = lines[at].split()
        assert w[0::2][:1] == ["entry"] and [int(w[2]), int(w[4]), int(w[6]), int(w[8])] == list(e[:4]), lines[at]
        assert _bits([w[10]])[0] == e[4] and [int(w[12]), int(w[14])] == [e[5], e[6]] and _bits([w[16]])[0] == e[7], lines[at]
        at += 1
    assert at == 13
    w = lines[at].split()
    assert w[:2] == ["template", "2"] and _bits(w[2:]) == h.template(0, 2).view(np.uint32).tolist()
    assert _bits(w[2:4]) == np.asarray([3, 4], F).view(np.uint32).tolist()          # 3 e0 + 4 e1, written down
    assert lines[at + 1] == "unknown serial rejected %d" % rfd.RFD_ERR_INVALID_ARG and at + 2 == len(lines)
