"""The host side of device entropy decoding (include/rfd.h, "entropy decoding on the device") without a GPU: the marker pre-scan
against the boundaries the test-side writer laid out, the eligibility rule with its messages, the interval decoder the kernel
runs (csrc/jpeg_entropy.h, one function for host and device) as a program of its own under AddressSanitizer and UBSan, and
the new symbols of the interface."""
import os
import subprocess

import pytest

import jpeg_entropy_cases
from jpeg_entropy_cases import damaged, entries, entry

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "jpeg")


def load(name):
    with open(os.path.join(GOLDEN, name + ".jpg"), "rb") as f:
        return f.read()


def refusal(rfd, data):
    with pytest.raises(rfd.RfdError) as e:
        rfd.jpeg_intervals(data)
    return e.value.status, e.value.message


def test_the_pre_scan_finds_the_boundaries_the_writer_produced(rfd):
    for e in entries():
        if e.restart_interval <= jpeg_entropy_cases.MAX_INTERVAL:
            assert rfd.jpeg_intervals(e.data) == list(e.intervals), e.name
    big = entry("geo_17x9_420@R65535")
    st, msg = refusal(rfd, big.data)
    assert st == rfd.RFD_ERR_UNSUPPORTED and "65535" in msg and str(jpeg_entropy_cases.MAX_INTERVAL) in msg


def test_the_pre_scan_of_the_libjpeg_fixture(rfd):
    data = load("37x53_420_rst2")                                      # 3 x 4 MCUs at 2 per interval
    got = rfd.jpeg_intervals(data)
    assert got == list(jpeg_entropy_cases.marker_intervals(data)) and len(got) == 6


def test_fill_bytes_in_front_of_a_marker_are_not_part_of_the_interval(rfd):
    e = entry("restart_3@R3")
    at = e.intervals[1][1]                                             # the first 0xFF of RST1
    assert e.data[at:at + 2] == b"\xff\xd1"
    data = e.data[:at] + b"\xff\xff" + e.data[at:]                      # FF FF FF D1
    want = [(b + 2 * (b > at), x + 2 * (x > at)) for b, x in e.intervals]
    assert rfd.jpeg_intervals(data) == want and want[1][1] == at and want[2][0] == at + 4
    first = e.intervals[0][1]
    spliced = e.data[:first] + b"\xff" + e.data[first:]                 # FF FF D0, as the issue spells it
    assert rfd.jpeg_intervals(spliced)[0] == e.intervals[0] and rfd.jpeg_intervals(spliced)[1][0] == e.intervals[1][0] + 1


def test_files_that_are_not_eligible_say_why(rfd):
    e = entry("restart_3@R3")
    st, msg = refusal(rfd, jpeg_entropy_cases.without_restarts(e).data)
    assert st == rfd.RFD_ERR_UNSUPPORTED and "no restart interval" in msg
    st, msg = refusal(rfd, load("37x53_420_progressive"))
    assert st == rfd.RFD_ERR_UNSUPPORTED and "progressive" in msg
    by = {d.name: d for d in damaged()}
    st, msg = refusal(rfd, by["rst_out_of_sequence"].data)
    assert st == rfd.RFD_ERR_UNSUPPORTED and "out of sequence" in msg
    st, msg = refusal(rfd, by["data_ends_early"].data)
    assert st == rfd.RFD_ERR_UNSUPPORTED and "6 intervals" in msg and "need 7" in msg
    st, msg = refusal(rfd, jpeg_entropy_cases.over_the_cap().data)
    assert st == rfd.RFD_ERR_UNSUPPORTED and "exceeds the limit" in msg
    assert len(rfd.jpeg_intervals(by["garbage"].data)) == 7             # structurally fine: the device decoder is the one to refuse it
    st, msg = refusal(rfd, b"")
    assert st == rfd.RFD_ERR_INVALID_ARG


def test_the_interval_decoder_alone_under_address_and_ub_sanitizers(tmp_path):
    """tests/cpp/jpeg_entropy_check.cpp over every file of the builder and the five damaged ones: each file, the file cut at every
    byte of its scan and with each of its first 700 scan bytes replaced by 0x00, 0xFF and 0xD0.  Every interval is refused or
    equals the host decoder's; the sanitizers stay silent.  Built as tests/test_jpeg_cpu.py builds its program."""
    exe = str(tmp_path / "jpeg_entropy_check")
    src = os.path.join(ROOT, "tests", "cpp", "jpeg_entropy_check.cpp")
    base = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", src, "-o", exe]
    san = subprocess.run(base + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan"], capture_output=True, text=True)
    if san.returncode != 0:
        plain = subprocess.run(base, capture_output=True, text=True)
        assert plain.returncode == 0, "the build failed:\n" + san.stderr + plain.stderr
    good, bad = [], []
    for group, items in ((good, [e for e in entries() if e.restart_interval <= jpeg_entropy_cases.MAX_INTERVAL]), (bad, damaged())):
        for x in items:
            path = str(tmp_path / (x.name.replace("@", "_") + ".jpg"))
            with open(path, "wb") as f:
                f.write(x.data)
            group.append(path)
    good.sort(key=os.path.getsize, reverse=True)
    jobs = [[exe] + good[k::4] + (["--damaged"] + bad if k == 3 else []) for k in range(4)]   # four processes: the largest files apart
    procs = [subprocess.Popen(j, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True) for j in jobs]
    for p in procs:
        out, err = p.communicate()
        assert p.returncode == 0 and err == "" and " 0 failures" in out, out + err


def test_the_new_symbols_are_part_of_the_interface_and_host_is_the_default(rfd):
    names = ("rfd_set_jpeg_entropy", "rfd_jpeg_last_paths", "rfd_debug_jpeg_intervals", "rfd_debug_jpeg_coefficients_device")
    for name in names:
        assert name in rfd.API_SYMBOLS and hasattr(rfd.load_library(), name)
    txt = open(os.path.join(ROOT, "include", "rfd.h")).read()
    assert "RFD_JPEG_ENTROPY_HOST = 0" in txt and "RFD_JPEG_ENTROPY_DEVICE = 1" in txt
    assert (rfd.JPEG_ENTROPY_HOST, rfd.JPEG_ENTROPY_DEVICE) == (0, 1)
    for name in ("set_jpeg_entropy", "jpeg_last_paths", "jpeg_coefficients_device"):
        assert callable(getattr(rfd.RetinaFaceDetection, name))
    assert callable(rfd.jpeg_intervals)
    L = rfd.load_library()
    assert L.rfd_set_jpeg_entropy(None, 1) == rfd.RFD_ERR_INVALID_ARG   # no context: refused before anything else
    hdr = open(os.path.join(ROOT, "rs-face-detection_amd", "csrc", "jpeg_entropy.h")).read()
    assert "kJpegDeviceMaxInterval = %d;" % jpeg_entropy_cases.MAX_INTERVAL in hdr
