"""The tracker's rule on the host: tests/tracker_ref.py held to the constructed cases of tests/tracker_cases.py, whose expected
values are written down from the construction, and csrc/track_plan.h alone under the sanitizers.  tests/test_tracker_gpu.py holds
the library to the same cases and, beyond them, to the restatement."""
import os
import re
import subprocess

import numpy as np
import pytest

import tracker_cases as TC
import tracker_ref as TR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run_case(case):
    cfg = dict(case["cfg"])
    ref = TR.TrackerRef(**cfg)
    got = []
    for f in case["frames"]:
        if "reset" in f:
            ref.reset(f["reset"])
        rows = np.asarray(f["rows"], np.float32).reshape(-1, 5)
        got.append(ref.frame(f["s"], rows, f.get("q")))
    return ref, got


@pytest.mark.parametrize("name", sorted(TC.CASES))
def test_the_restatement_decides_every_constructed_case_as_written(name):
    case = TC.CASES[name]
    _, got = run_case(case)
    for i, (f, (track, flags, stats, ended)) in enumerate(zip(case["frames"], got)):
        assert list(track) == f["track"], "frame %d track" % i
        assert list(flags) == f["flags"], "frame %d flags" % i
        assert tuple(stats) == f["stats"], "frame %d stats" % i
        assert ended == f["ended"], "frame %d ended" % i


@pytest.mark.parametrize("max_tracks", [64, 128, 256])
def test_1024_rows_over_one_track_fill_the_slots_then_drop(max_tracks):
    case = TC.crowd(max_tracks)
    ref, got = run_case(case)
    track, flags, stats, ended = got[1]
    f = case["frames"][1]
    assert list(track) == f["track"] and list(flags) == f["flags"] and tuple(stats) == f["stats"] == (1, max_tracks - 1, 0, 1024 - max_tracks)
    assert [t[:2] for t in ref.tracks(0)] == [(k, k + 1) for k in range(max_tracks)]


def test_the_iou_is_the_written_arithmetic():
    one = np.asarray([[0, 0, 9, 9]], np.float32)
    assert TR.iou(np.asarray([0, 0, 9, 4], np.float32), one)[0] == np.float32(0.5)
    assert TR.iou(np.asarray([10, 0, 19, 9], np.float32), one)[0] == 0          # touching boxes: w = 9 - 10 + 1 = 0
    assert TR.iou(np.asarray([9, 9, 18, 18], np.float32), one)[0] == np.float32(1) / np.float32(199)   # the +1 convention: one shared pixel
    assert np.isnan(TR.iou(np.asarray([np.nan, 0, 9, 9], np.float32), one)[0])


def test_update_leaves_everything_past_the_counts_alone_and_splits_do_not_matter():
    frames = TC.CASES["lifecycle_and_reset"]["frames"][:8]
    streams, boxes, lmk, count, _ = TC.slabs(frames, 4, False)
    cfg = TC.CASES["lifecycle_and_reset"]["cfg"]
    whole = TR.TrackerRef(**cfg).update(streams, boxes, lmk, count, None, TR.Out(8, 4, 64, fill=0xA5))
    parts, ref = TR.Out(8, 4, 64, fill=0xA5), TR.TrackerRef(**cfg)
    for a, b in ((0, 3), (3, 4), (4, 8)):
        sub = TR.Out(b - a, 4, 64, fill=0xA5)
        ref.update(streams[a:b], boxes[a:b], lmk[a:b], count[a:b], None, sub)
        for k, v in vars(sub).items():
            getattr(parts, k)[a:b] = v
    for k, v in vars(whole).items():
        assert v.tobytes() == getattr(parts, k).tobytes(), k
    assert whole.track[3].tolist() == [2, 3, -1515870811, -1515870811] and whole.ended[3].tolist()[:2] == [1, -1515870811]
    assert whole.due_count.tolist() == [2, 0, 0, 1, 0, 0, 0, 1] and whole.due_track[3, 0] == 3
    assert whole.due_boxes[3, 0].tolist() == boxes[3, 1].tolist() and whole.due_landmarks[3, 0].tobytes() == lmk[3, 1].tobytes()


def test_the_plan_alone_under_address_and_ub_sanitizers(tmp_path):
    """tests/cpp/track_plan_check.cpp, built as tests/test_view_plan_cpu.py builds its program; a plain build where the sanitizer
    runtimes cannot be linked."""
    exe = str(tmp_path / "track_plan_check")
    src = os.path.join(ROOT, "tests", "cpp", "track_plan_check.cpp")
    base = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", src, "-o", exe]
    san = subprocess.run(base + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan"], capture_output=True, text=True)
    if san.returncode != 0:
        plain = subprocess.run(base, capture_output=True, text=True)
        assert plain.returncode == 0, "the build failed:\n" + san.stderr + plain.stderr
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0 and " 0 failures" in run.stdout, run.stdout + run.stderr
    m = re.search(r"(\d+) steps, (\d+) checks, 0 failures", run.stdout)
    assert m and int(m.group(1)) > 100000 and int(m.group(2)) > 1000000, run.stdout   # the program did run its cases


def test_the_plan_is_plain_host_code():
    txt = open(os.path.join(ROOT, "rs-face-detection_amd", "csrc", "track_plan.h")).read()
    assert "hip" not in re.sub(r"//.*", "", txt).lower()
