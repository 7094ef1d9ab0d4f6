"""The track identities' boundary without a GPU (include/rfd.h, "track identities"): the exports, the struct layouts, the default
config, every config bound and every argument error that needs no device; the restatement (tests/track_identity_ref.py) held to
the constructed cases (tests/track_identity_cases.py); and csrc/track_identity_plan.h alone under the sanitizers.  "Identities
not enabled" needs a tracker and therefore a device: tests/test_track_identity_gpu.py holds it."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import track_identity_cases as IC
import track_identity_ref as IR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["rfd_track_identity_config_default", "rfd_tracker_identity_enable", "rfd_tracker_fuse_device", "rfd_tracker_label_device",
           "rfd_tracker_who_device", "rfd_tracker_fuse", "rfd_tracker_label", "rfd_tracker_who", "rfd_tracker_get_identities",
           "rfd_tracker_get_template"]
F = np.float32


def test_exports_header_and_binding_agree(rfd):
    header = open(os.path.join(ROOT, "include", "rfd.h")).read()
    L = rfd.load_library()
    for name in SYMBOLS:
        assert re.search(r"RFD_API\s+(int|void)\s+%s\s*\(" % name, header), name
        assert name in rfd.API_SYMBOLS and hasattr(L, name), name
        assert getattr(L, name).argtypes is not None, name
    for method in ("enable_identities", "fuse", "fuse_device", "label", "label_device", "who", "who_device", "identities", "template"):
        assert callable(getattr(rfd.Tracker, method)), method
    assert callable(rfd.track_identity_config)
    assert rfd.TRACK_NAMED == 8 and rfd.TRACK_NAMED & (rfd.TRACK_NEW | rfd.TRACK_CONFIRMED | rfd.TRACK_DUE) == 0
    assert (rfd.TRACK_FUSE_OK, rfd.TRACK_FUSE_NO_TRACK, rfd.TRACK_FUSE_BAD_INPUT, rfd.TRACK_FUSE_OVERFLOW) == (0, 1, 2, 3)
    for name, value in (("RFD_TRACK_NAMED", "8u"), ("RFD_TRACK_FUSE_OK", "0"), ("RFD_TRACK_FUSE_NO_TRACK", "1"),
                        ("RFD_TRACK_FUSE_BAD_INPUT", "2"), ("RFD_TRACK_FUSE_OVERFLOW", "3")):
        assert re.search(r"#define %s %s\b" % (name, value), header), name
    section = header[header.index("---- track identities:"):header.index("#define RFD_TRACK_NAMED")]
    section = re.sub(r"\s+", " ", re.sub(r"\n \*", " ", section))       # the comment as running text
    for said in ("CHOSEN values, not tuned on data", "rfd_tracker_reset needs no change", "STALE", "means \"on the list\"", "Out of scope",
                 "stay as passed"):
        assert said in section, said
    hpp = open(os.path.join(ROOT, "include", "rfd.hpp")).read()
    for name in SYMBOLS[1:]:
        assert name + "(" in hpp, name                              # the C++ wrapper calls every entry


def test_struct_layouts(rfd):
    c, o, t = rfd.rfd_track_identity_config, rfd.rfd_track_obs, rfd.rfd_track_identity
    assert C.sizeof(c) == 32 and [getattr(c, f).offset for f in ("dim", "accept", "release", "margin", "reserved")] == [0, 4, 8, 12, 16]
    assert C.sizeof(o) == 32 and [getattr(o, f).offset for f in ("total", "first", "row", "serial")] == [0, 8, 16, 24]
    assert C.sizeof(t) == 32
    assert [getattr(t, f).offset for f in ("slot", "serial", "identity", "row", "score", "named", "shots", "weight")] == [0, 4, 8, 12, 16, 20, 24, 28]
    # the tracker's own structs keep their layouts
    assert C.sizeof(rfd.rfd_tracker_config) == 48 and C.sizeof(rfd.rfd_track_out) == 72 and C.sizeof(rfd.rfd_track) == 36


def test_default_config(rfd):
    L = rfd.load_library()
    c = rfd.rfd_track_identity_config()
    C.memset(C.byref(c), 0xFF, C.sizeof(c))
    assert L.rfd_track_identity_config_default(C.byref(c)) == rfd.RFD_OK
    f32 = lambda x: float(F(x))
    assert (c.dim, c.accept, c.release, c.margin) == (512, f32(0.5), f32(0.4), f32(0.05)) and list(c.reserved) == [0, 0, 0, 0]
    assert L.rfd_track_identity_config_default(None) == rfd.RFD_ERR_INVALID_ARG
    assert rfd.track_identity_config(dim=64, margin=0.0).dim == 64
    with pytest.raises(TypeError):
        rfd.track_identity_config(reserved=1)


BAD = [("dim", 0), ("dim", 16), ("dim", 48), ("dim", 1000), ("dim", 1056), ("dim", -32), ("accept", float("nan")), ("accept", float("inf")),
       ("release", float("nan")), ("release", float("-inf")), ("release", 0.6), ("margin", -0.01), ("margin", float("nan")), ("margin", float("inf"))]


@pytest.mark.parametrize("field,value", BAD)
def test_enable_refuses_every_config_bound_and_names_the_field(rfd, field, value):
    L = rfd.load_library()
    c = rfd.track_identity_config()
    setattr(c, field, value)
    assert L.rfd_tracker_identity_enable(None, C.byref(c)) == rfd.RFD_ERR_INVALID_ARG       # judged before the tracker
    assert field in L.rfd_last_error().decode() and "tracker is null" not in L.rfd_last_error().decode()


def test_null_arguments(rfd):
    L = rfd.load_library()
    c = rfd.track_identity_config()
    assert L.rfd_tracker_identity_enable(None, C.byref(c)) == rfd.RFD_ERR_INVALID_ARG and b"tracker" in L.rfd_last_error()
    assert L.rfd_tracker_identity_enable(None, None) == rfd.RFD_ERR_INVALID_ARG and b"tracker" in L.rfd_last_error()
    s, a = np.zeros(1, np.int32), np.zeros(64, np.float32)
    o = rfd.rfd_track_obs(None, a.ctypes.data, a.ctypes.data, a.ctypes.data)
    p = a.ctypes.data
    calls = [lambda: L.rfd_tracker_fuse(None, s.ctypes.data, 1, C.byref(o), 1, p, None, p, p),
             lambda: L.rfd_tracker_fuse_device(None, s.ctypes.data, 1, C.byref(o), 1, p, None, p, p, 1),
             lambda: L.rfd_tracker_label(None, s.ctypes.data, 1, C.byref(o), 1, 1, p, p, p, p),
             lambda: L.rfd_tracker_label_device(None, s.ctypes.data, 1, C.byref(o), 1, 1, p, p, p, p, 1),
             lambda: L.rfd_tracker_who(None, s.ctypes.data, 1, p, p, None, p, None, None),
             lambda: L.rfd_tracker_who_device(None, s.ctypes.data, 1, p, p, None, p, None, None, 1),
             lambda: L.rfd_tracker_get_template(None, 0, 1, p)]
    for call in calls:
        assert call() == rfd.RFD_ERR_INVALID_ARG and b"tracker is null" in L.rfd_last_error()
    n = C.c_int(7)
    assert L.rfd_tracker_get_identities(None, 0, None, 0, C.byref(n)) == rfd.RFD_ERR_INVALID_ARG and b"tracker" in L.rfd_last_error()


@pytest.mark.parametrize("name", sorted(IC.CASES))
def test_the_restatement_is_held_to_the_constructed_cases(name):
    IC.CASES[name](IC.RefHarness())


def test_the_restatements_norm_is_the_lane_sum_and_butterfly():
    """against a second, scalar spelling: 64 running sums in np.float32 scalars, the butterfly lane by lane"""
    rng = np.random.default_rng(5)
    for dim in (32, 64, 96, 512, 1024):
        x = rng.standard_normal(dim).astype(F)
        part = [F(0)] * 64
        for i in range(dim):
            part[i % 64] = F(part[i % 64] + F(x[i] * x[i]))
        for off in (32, 16, 8, 4, 2, 1):
            part = [F(part[l] + part[l ^ off]) for l in range(64)]
        assert len({int(p.view(np.uint32)) for p in part}) == 1
        want = np.sqrt(part[0])
        assert int(IR.wave_norm(x).view(np.uint32)) == int(want.view(np.uint32)), dim
        e, _ = IR.normalise(x)
        assert e.tobytes() == (x / want).tobytes()


def test_splitting_the_observations_of_a_stream_over_calls_gives_the_same_bits():
    def run(split):
        h = IC.RefHarness()
        h.start(dim=96)
        h.frames([(0, [0, 1, 2])])
        obs = [(0, r, int(rng2.integers(1, 4))) for r in range(8)]
        emb = rng2.standard_normal((8, 96)).astype(F)
        w = rng2.choice([0.25, 0.5, 1.0, 3.0], size=8).astype(F)
        qs, at = [], 0
        for k in split:
            part = [(0, r, s) for (_, r, s) in obs[at:at + k]]
            q, st = h.fuse([0], part, emb[at:at + k], weight=w[at:at + k])
            qs.append(q)
            at += k
        return np.concatenate(qs).tobytes(), h.entries(0), [h.template(0, s).tobytes() for s in (1, 2, 3)]

    outs = []
    for split in ([8], [1] * 8, [3, 1, 4]):
        rng2 = np.random.default_rng(77)                               # the same draws for every split
        outs.append(run(split))
    assert outs[0] == outs[1] == outs[2] and len(outs[0][1]) == 3


def test_the_plan_alone_under_address_and_ub_sanitizers(tmp_path):
    """tests/cpp/track_identity_plan_check.cpp, built plain and under the sanitizers as tests/test_tracker_ref_cpu.py builds its
    program; where the sanitizer runtimes cannot be linked the plain build stands alone."""
    src = os.path.join(ROOT, "tests", "cpp", "track_identity_plan_check.cpp")
    ran = 0
    for name, extra in (("plain", []), ("san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan"])):
        exe = str(tmp_path / ("track_identity_plan_check_" + name))
        build = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", src, "-o", exe] + extra, capture_output=True, text=True)
        if build.returncode != 0:
            assert name == "san", "the plain build failed:\n" + build.stderr
            continue
        run = subprocess.run([exe], capture_output=True, text=True)
        assert run.returncode == 0 and " 0 failures" in run.stdout, run.stdout + run.stderr
        m = re.search(r"(\d+) steps, (\d+) checks, 0 failures", run.stdout)
        assert m and int(m.group(1)) > 2000 and int(m.group(2)) > 50000, run.stdout     # the program did run its cases
        ran += 1
    assert ran >= 1


def test_the_plan_is_plain_host_code():
    txt = open(os.path.join(ROOT, "rs-face-detection_amd", "csrc", "track_identity_plan.h")).read()
    assert "hip" not in re.sub(r"//.*", "", txt).lower()


@pytest.mark.skipif(not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-objdump"), reason="LLVM tools not installed")
def test_the_kernels_keep_to_narrow_lds_reads_and_every_instantiation_is_built(tmp_path):
    """the build-time ISA rules of tests/test_build_cpu.py (no scratch, no ds_read_b128 under a partial EXEC) run over every
    kernels_*.o; this adds what the identities promise beyond them: no 128-bit LDS read at all, and one fuse kernel per lane
    element count 1, 2, 4, 8, 16 beside the label and who kernels"""
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import isa_check
    obj = os.path.join(ROOT, "rs-face-detection_amd", "build", "kernels_track_identity.o")
    assert os.path.exists(obj), "run rs-face-detection_amd/build.sh (or __graft_entry__.build()) first"
    kernels = isa_check.disassemble(obj, str(tmp_path))
    for name, ins in kernels.items():
        assert not isa_check.has_instr(ins, "ds_read_b128"), "%s uses ds_read_b128" % name
    names = " ".join(kernels)
    for j in (1, 2, 4, 8, 16):
        assert "track_fuse_kernelILi%dE" % j in names, j
    assert "track_label_kernel" in names and "track_who_kernel" in names and len(kernels) == 7
