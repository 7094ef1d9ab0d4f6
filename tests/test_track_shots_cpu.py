"""The track shots' boundary without a GPU (include/rfd.h, "track shots"): the exports, the struct layouts, the default config,
every config bound and every argument error that needs no device; the restatement (tests/track_shots_ref.py) held to the
constructed cases (tests/track_shots_cases.py); csrc/track_shots_plan.h alone under the sanitizers; and the build-time ISA rules
on kernels_track_shots.o.  "Shots not enabled" needs a tracker and therefore a device: tests/test_track_shots_gpu.py holds it."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import track_shots_cases as SC
import track_shots_ref as SR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["rfd_track_shot_config_default", "rfd_tracker_shots_enable", "rfd_tracker_keep_shots_device", "rfd_tracker_collect_ended_device",
           "rfd_tracker_keep_shots", "rfd_tracker_collect_ended", "rfd_tracker_get_shots", "rfd_tracker_get_shot_crop"]


def test_exports_header_and_binding_agree(rfd):
    header = open(os.path.join(ROOT, "include", "rfd.h")).read()
    L = rfd.load_library()
    for name in SYMBOLS:
        assert re.search(r"RFD_API\s+(int|void)\s+%s\s*\(" % name, header), name
        assert name in rfd.API_SYMBOLS and hasattr(L, name), name
        assert getattr(L, name).argtypes is not None, name
    for method in ("enable_shots", "keep_shots", "keep_shots_device", "collect_ended", "collect_ended_device", "shots", "shot_crop"):
        assert callable(getattr(rfd.Tracker, method)), method
    assert callable(rfd.track_shot_config)
    assert (rfd.TRACK_SHOT_KEPT, rfd.TRACK_SHOT_NO_TRACK, rfd.TRACK_SHOT_BAD_INPUT, rfd.TRACK_SHOT_PASSED) == (0, 1, 2, 3)
    for name, value in (("RFD_TRACK_SHOT_KEPT", "0"), ("RFD_TRACK_SHOT_NO_TRACK", "1"), ("RFD_TRACK_SHOT_BAD_INPUT", "2"), ("RFD_TRACK_SHOT_PASSED", "3")):
        assert re.search(r"#define %s %s\b" % (name, value), header), name
    section = header[header.index("---- track shots:"):header.index("#define RFD_TRACK_SHOT_KEPT")]
    section = re.sub(r"\s+", " ", re.sub(r"\n \*", " ", section))       # the comment as running text
    for said in ("rfd_tracker_reset needs no change", "STALE", "Out of scope", "stays as passed", "IS LEFT EXACTLY AS PASSED",
                 "directly behind the rfd_tracker_update_device", "a slot reborn in the same frame still yields its old track's record",
                 "a track whose only due shot arrives after it ended has none", "rfd_quality_decide_device", "an equal q keeps the earlier shot",
                 "changes nothing in it", "among the HEADS"):
        assert said in section, said
    ident = header[header.index("---- track identities:"):header.index("#define RFD_TRACK_NAMED")]
    assert "Out of scope" in ident and "the identity of tracks at the moment they end" not in ident and "track shots" in ident
    hpp = open(os.path.join(ROOT, "include", "rfd.hpp")).read()
    for name in SYMBOLS:
        assert name + "(" in hpp, name                              # the C++ wrapper calls every entry


def test_struct_layouts(rfd):
    offsets = lambda t, fields: [getattr(t, f).offset for f in fields]
    c, s, r, l = rfd.rfd_track_shot_config, rfd.rfd_track_shot, rfd.rfd_track_record, rfd.rfd_track_records
    assert C.sizeof(c) == 32 and offsets(c, ("crop_w", "crop_h", "reserved")) == [0, 4, 8]
    assert C.sizeof(s) == 40 and offsets(s, ("slot", "serial", "shots", "kept", "q", "reserved", "first_stamp", "best_stamp")) == [0, 4, 8, 12, 16, 20, 24, 32]
    assert C.sizeof(r) == 80
    assert offsets(r, ("stream", "serial", "frame", "shots", "kept", "q", "first_stamp", "best_stamp", "end_stamp", "identity", "row", "id_score", "named",
                       "id_shots", "id_weight", "reserved")) == [0, 4, 8, 12, 16, 20, 24, 32, 40, 48, 52, 56, 60, 64, 68, 72]
    assert C.sizeof(l) == 32 and offsets(l, ("total", "first", "rec", "crops")) == [0, 8, 16, 24]
    # the restatement's dtypes are those structs
    assert SR.SHOT.itemsize == 40 and [SR.SHOT.fields[f][1] for f in SR.SHOT.names] == offsets(s, SR.SHOT.names)
    assert SR.RECORD.itemsize == 80 and [SR.RECORD.fields[f][1] for f in SR.RECORD.names] == offsets(r, SR.RECORD.names)
    # the tracker's and the identities' structs keep their layouts
    assert C.sizeof(rfd.rfd_tracker_config) == 48 and C.sizeof(rfd.rfd_track_out) == 72 and C.sizeof(rfd.rfd_track) == 36
    assert C.sizeof(rfd.rfd_track_identity_config) == 32 and C.sizeof(rfd.rfd_track_obs) == 32 and C.sizeof(rfd.rfd_track_identity) == 32


def test_default_config(rfd):
    L = rfd.load_library()
    c = rfd.rfd_track_shot_config()
    C.memset(C.byref(c), 0xFF, C.sizeof(c))
    assert L.rfd_track_shot_config_default(C.byref(c)) == rfd.RFD_OK
    assert (c.crop_w, c.crop_h) == (112, 112) and list(c.reserved) == [0] * 6
    assert L.rfd_track_shot_config_default(None) == rfd.RFD_ERR_INVALID_ARG
    assert rfd.track_shot_config(crop_w=5).crop_w == 5 and rfd.track_shot_config(crop_w=5).crop_h == 112
    with pytest.raises(TypeError):
        rfd.track_shot_config(reserved=1)


BAD = [("crop_w", 0), ("crop_w", -1), ("crop_w", 1025), ("crop_w", -2 ** 31), ("crop_h", 0), ("crop_h", -112), ("crop_h", 1025), ("crop_h", 2 ** 31 - 1)]


@pytest.mark.parametrize("field,value", BAD)
def test_enable_refuses_every_config_bound_and_names_the_field(rfd, field, value):
    L = rfd.load_library()
    c = rfd.track_shot_config()
    setattr(c, field, value)
    assert L.rfd_tracker_shots_enable(None, C.byref(c)) == rfd.RFD_ERR_INVALID_ARG       # judged before the tracker
    assert field in L.rfd_last_error().decode() and "tracker is null" not in L.rfd_last_error().decode()


@pytest.mark.parametrize("at", range(6))
def test_enable_refuses_a_non_zero_reserved(rfd, at):
    L = rfd.load_library()
    c = rfd.track_shot_config()
    c.reserved[at] = 1
    assert L.rfd_tracker_shots_enable(None, C.byref(c)) == rfd.RFD_ERR_INVALID_ARG and b"reserved" in L.rfd_last_error()


def test_null_arguments(rfd):
    L = rfd.load_library()
    c = rfd.track_shot_config()
    assert L.rfd_tracker_shots_enable(None, C.byref(c)) == rfd.RFD_ERR_INVALID_ARG and b"tracker is null" in L.rfd_last_error()
    assert L.rfd_tracker_shots_enable(None, None) == rfd.RFD_ERR_INVALID_ARG and b"tracker is null" in L.rfd_last_error()
    s, a = np.zeros(1, np.int32), np.zeros(64, np.int64)
    p = a.ctypes.data
    o = rfd.rfd_track_obs(None, p, p, p)
    r = rfd.rfd_track_records(p, p, p, None)
    calls = [lambda: L.rfd_tracker_keep_shots(None, s.ctypes.data, None, 1, C.byref(o), 1, p, None, None, p),
             lambda: L.rfd_tracker_keep_shots_device(None, s.ctypes.data, None, 1, C.byref(o), 1, p, None, None, p, 1),
             lambda: L.rfd_tracker_collect_ended(None, s.ctypes.data, None, 1, p, p, 1, C.byref(r)),
             lambda: L.rfd_tracker_collect_ended_device(None, s.ctypes.data, None, 1, p, p, 1, C.byref(r), 1),
             lambda: L.rfd_tracker_get_shot_crop(None, 0, 1, p)]
    for call in calls:
        assert call() == rfd.RFD_ERR_INVALID_ARG and b"tracker is null" in L.rfd_last_error()
    n = C.c_int(7)
    assert L.rfd_tracker_get_shots(None, 0, None, 0, C.byref(n)) == rfd.RFD_ERR_INVALID_ARG and b"tracker" in L.rfd_last_error()


def test_no_message_of_the_new_code_is_a_bare_constant_name():
    """tests/test_build_cpu.py reads whole strings of the library that look like RFD_... as environment variables"""
    for name in ("track_shots_host.hip", "kernels_track_shots.hip", "track_shots_plan.h", "track_shots_host.h"):
        txt = open(os.path.join(ROOT, "rs-face-detection_amd", "csrc", name)).read()
        assert not re.search(r'"(RFD_|GPU_MAX)[A-Z0-9_]+"', txt), name


@pytest.mark.parametrize("name", sorted(SC.CASES))
def test_the_restatement_is_held_to_the_constructed_cases(name):
    SC.CASES[name](SC.RefHarness())


def test_splitting_the_observations_of_a_stream_over_calls_gives_the_same_state():
    def run(split):
        rng = np.random.default_rng(77)                                # the same draws for every split
        h = SC.RefHarness()
        h.start(crop=(3, 2))
        h.frames([(0, [0, 1, 2])])
        obs = [(0, r, int(rng.integers(1, 4))) for r in range(10)]
        q = rng.choice([0.25, 0.5, 0.75, np.nan], size=10).astype(np.float32)
        sts, at = [], 0
        for k in split:
            sts += h.keep([0], obs[at:at + k], range(at, at + k), q=q[at:at + k], stamp=[5]).tolist()
            at += k
        return sts, h.shots(0).tobytes(), [h.shot_crop(0, s).tobytes() for s in (1, 2, 3)]

    outs = [run(split) for split in ([10], [1] * 10, [3, 1, 6])]
    assert outs[0] == outs[1] == outs[2] and len(outs[0][1]) == 3 * 40


def test_the_plan_alone_under_address_and_ub_sanitizers(tmp_path):
    """tests/cpp/track_shots_plan_check.cpp, built plain and under the sanitizers as tests/test_track_identity_cpu.py builds its
    program; where the sanitizer runtimes cannot be linked the plain build stands alone."""
    src = os.path.join(ROOT, "tests", "cpp", "track_shots_plan_check.cpp")
    ran = 0
    for name, extra in (("plain", []), ("san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan"])):
        exe = str(tmp_path / ("track_shots_plan_check_" + name))
        build = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", src, "-o", exe] + extra, capture_output=True, text=True)
        if build.returncode != 0:
            assert name == "san", "the plain build failed:\n" + build.stderr
            continue
        run = subprocess.run([exe], capture_output=True, text=True)
        assert run.returncode == 0 and " 0 failures" in run.stdout, run.stdout + run.stderr
        m = re.search(r"(\d+) steps, (\d+) checks, 0 failures", run.stdout)
        assert m and int(m.group(1)) > 25000 and int(m.group(2)) > 3000000, run.stdout     # the program did run its cases
        ran += 1
    assert ran >= 1


def test_the_plan_is_plain_host_code():
    txt = open(os.path.join(ROOT, "rs-face-detection_amd", "csrc", "track_shots_plan.h")).read()
    assert "hip" not in re.sub(r"//.*", "", txt).lower()


@pytest.mark.skipif(not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-objdump"), reason="LLVM tools not installed")
def test_the_three_kernels_are_built_without_scratch_and_the_copy_has_its_wide_path(tmp_path):
    """the build-time ISA rules of tests/test_build_cpu.py (no scratch, no VGPR spills, no ds_read_b128 under a partial EXEC) run
    over every kernels_*.o; this names the three kernels, holds them to no scratch instruction and no 128-bit LDS read at all,
    and finds the 16-byte global loads and stores of the copy kernel's aligned path"""
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import isa_check
    obj = os.path.join(ROOT, "rs-face-detection_amd", "build", "kernels_track_shots.o")
    assert os.path.exists(obj), "run rs-face-detection_amd/build.sh (or __graft_entry__.build()) first"
    kernels = isa_check.disassemble(obj, str(tmp_path))
    for name, ins in kernels.items():
        assert not isa_check.has_instr(ins, "scratch_"), "%s uses scratch" % name
        assert not isa_check.has_instr(ins, "ds_read_b128"), "%s uses ds_read_b128" % name
        assert not isa_check.ds_read_b128_under_partial_exec(ins), name
    names = " ".join(kernels)
    assert "track_shot_decide_kernel" in names and "track_record_list_kernel" in names and "shot_copy_kernel" in names and len(kernels) == 3
    copy = [ins for name, ins in kernels.items() if "shot_copy_kernel" in name][0]
    assert isa_check.has_instr(copy, "global_load_dwordx4") and isa_check.has_instr(copy, "global_store_dwordx4")
    assert not isa_check.has_instr(copy, "ds_"), "the copy kernel needs no LDS"
