"""The gallery file "RFDG" (include/rfd.h, "gallery file") without a GPU: rfd_gallery_file_info, which performs the whole
validation on the host, against files that the numpy writer of rfd_hip produces and against bytes written out by hand; every
malformed case with its status and a message that names the cause; and the parser alone (csrc/gallery_file.h), built with the
host compiler under AddressSanitizer and UBSan and run as a program of its own."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

HEADER = b"RFDG" + bytes([1, 0, 0, 0, 32, 0, 0, 0, 3, 0, 0, 0, 0, 0, 0, 0])   # version 1, dim 32, 3 rows, reserved 0
# rows 0 and 2 live (bits 0 and 2); row 0 = 1.0 (bf16 0x3f80), row 1 removed = zeros, row 2 = -0.5 (bf16 0xbf00)
TINY = HEADER + b"\x05" + b"\x80\x3f" * 32 + b"\x00\x00" * 32 + b"\x00\xbf" * 32


def _info(rfd, path):
    dim, rows, live = C.c_int(-7), C.c_int(-7), C.c_int(-7)
    L = rfd.load_library()
    st = L.rfd_gallery_file_info(os.fsencode(str(path)), C.byref(dim), C.byref(rows), C.byref(live))
    return st, (dim.value, rows.value, live.value), L.rfd_last_error().decode()


def test_the_bytes_of_a_tiny_file_are_pinned(rfd, tmp_path):
    assert len(TINY) == 20 + 1 + 3 * 32 * 2
    p = tmp_path / "tiny.rfdg"
    values = np.zeros((3, 32), np.float32)
    values[0], values[2] = 1.0, -0.5
    rfd.gallery_file_write(p, values, [True, False, True])
    assert p.read_bytes() == TINY
    assert _info(rfd, p)[:2] == (0, (32, 3, 2))
    assert rfd.gallery_file_info(p) == (32, 3, 2)
    v, live = rfd.gallery_file_read(p)
    assert np.array_equal(v.view(np.uint32), values.view(np.uint32)) and live.tolist() == [True, False, True]


@pytest.mark.parametrize("dim,rows", [(32, 0), (32, 1), (64, 8), (512, 9), (1024, 16), (128, 1001)])
def test_info_reports_what_the_numpy_writer_wrote(rfd, tmp_path, dim, rows):
    rng = np.random.default_rng(dim + rows)
    bits = rng.integers(0, 1 << 16, (rows, dim), dtype=np.uint32)
    bits[(bits & 0x7f80) == 0x7f80] = 0x3f80                      # finite values only; subnormals and both zeros stay
    values = (bits << 16).view(np.float32)
    live = rng.random(rows) < 0.7
    values[~live] = 0.0
    p = tmp_path / "g.rfdg"
    rfd.gallery_file_write(p, values, live)
    assert os.path.getsize(p) == 20 + (rows + 7) // 8 + rows * dim * 2
    assert _info(rfd, p)[:2] == (0, (dim, rows, int(live.sum())))
    v, l2 = rfd.gallery_file_read(p)
    assert np.array_equal(v.view(np.uint32), values.view(np.uint32)) and np.array_equal(l2, live)
    # any pointer may be null
    assert rfd.load_library().rfd_gallery_file_info(os.fsencode(str(p)), None, None, None) == 0


def _patched(at, value):
    b = bytearray(TINY)
    b[at] = value
    return bytes(b)


VALUES = 21   # offset of the first value in TINY
MALFORMED = [
    ("wrong magic", _patched(3, ord("W")), "magic"),
    ("version 2", _patched(4, 2), "version"),
    ("dim 48", _patched(8, 48), "dim 48"),
    ("dim 0", _patched(8, 0), "dim 0"),
    ("dim 2080", _patched(9, 8), "dim 2080"),
    ("reserved field", _patched(16, 9), "reserved"),
    ("one byte short", TINY[:-1], "length"),
    ("one byte long", TINY + b"\x00", "length"),
    ("header only", TINY[:20], "length"),
    ("shorter than the header", TINY[:7], "length"),
    ("empty", b"", "length"),
    ("rows 4 in the header", _patched(12, 4), "length"),
    ("liveness bit of row 3", _patched(20, 0x0d), "beyond row 2"),
    ("liveness bit 7", _patched(20, 0x85), "beyond row 2"),
]
# 0x7f80 = +inf in row 2, element 5; 0xffc0 = a NaN in row 0, element 31; 0xff80 = -inf in the removed row 1, element 0
_inf = bytearray(TINY)
_inf[VALUES + 2 * (2 * 32 + 5):VALUES + 2 * (2 * 32 + 5) + 2] = b"\x80\x7f"
_nan = bytearray(TINY)
_nan[VALUES + 2 * 31:VALUES + 2 * 31 + 2] = b"\xc0\xff"
_ninf = bytearray(TINY)
_ninf[VALUES + 2 * 32:VALUES + 2 * 32 + 2] = b"\x80\xff"
MALFORMED += [("+inf", bytes(_inf), "row 2"), ("+inf element", bytes(_inf), "element 5"), ("NaN", bytes(_nan), "row 0"),
              ("NaN element", bytes(_nan), "element 31"), ("-inf in a removed row", bytes(_ninf), "row 1")]


@pytest.mark.parametrize("name,data,needle", MALFORMED, ids=[m[0] for m in MALFORMED])
def test_a_malformed_file_is_refused_and_the_message_names_the_cause(rfd, tmp_path, name, data, needle):
    p = tmp_path / "bad.rfdg"
    p.write_bytes(data)
    st, out, msg = _info(rfd, p)
    assert st == rfd.RFD_ERR_INVALID_ARG, (name, st, msg)
    assert needle in msg, (name, msg)
    assert out == (-7, -7, -7)                                     # nothing is reported about a refused file
    with pytest.raises(rfd.RfdError) as e:
        rfd.gallery_file_info(p)
    assert e.value.status == rfd.RFD_ERR_INVALID_ARG and needle in str(e.value)


def test_a_missing_path_fails_with_the_io_status(rfd, tmp_path):
    st, out, msg = _info(rfd, tmp_path / "nothing" / "here.rfdg")
    assert st == rfd.RFD_ERR_IO and "cannot open" in msg and out == (-7, -7, -7)
    st, _, msg = _info(rfd, tmp_path)                              # a directory
    assert st in (rfd.RFD_ERR_IO, rfd.RFD_ERR_INVALID_ARG) and msg
    assert rfd.load_library().rfd_gallery_file_info(None, None, None, None) == rfd.RFD_ERR_INVALID_ARG


def test_the_parser_alone_under_address_and_ub_sanitizers(tmp_path):
    """tests/cpp/gallery_file_check.cpp: the malformed files again and the valid file cut at every byte, in a program of its own
    whose every out-of-bounds access or undefined operation aborts it.  The sanitizer runtimes are linked into the program
    (-static-libasan), so it runs whatever else the environment preloads."""
    exe = str(tmp_path / "gallery_file_check")
    src = os.path.join(ROOT, "tests", "cpp", "gallery_file_check.cpp")
    base = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", src, "-o", exe]
    san = subprocess.run(base + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan"], capture_output=True, text=True)
    assert san.returncode == 0, "the sanitizer build failed:\n" + san.stderr
    work = tmp_path / "work"
    work.mkdir()
    run = subprocess.run([exe, str(work)], capture_output=True, text=True)
    assert run.returncode == 0 and "0 failures" in run.stdout, run.stdout + run.stderr
