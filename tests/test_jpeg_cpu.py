"""The host half of the JPEG decoder (include/rfd.h, "JPEG decode") without a GPU: rfd_jpeg_info on every fixture of
tests/golden/jpeg/, every unsupported and malformed case with its status and a message that names the cause, and
rfd_debug_jpeg_coefficients -> tests/jpeg_ref.py against libjpeg-turbo's pixels byte for byte -- which pins the marker parser,
the Huffman decoder and the restated IDCT / upsampling / colour arithmetic before any kernel is involved.  The parser alone
(csrc/jpeg_parse.h) is also built with the host compiler under AddressSanitizer and UBSan and run as a program of its own."""
import glob
import io
import os
import struct
import subprocess

import numpy as np
import pytest

import jpeg_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "jpeg")
SAMPLING = {"GRAY": jpeg_ref.GRAY, "444": jpeg_ref.S444, "422": jpeg_ref.S422, "420": jpeg_ref.S420}
SUPPORTED = sorted(os.path.basename(f)[:-4] for f in glob.glob(os.path.join(GOLDEN, "*.npz")))


def load(name):
    with open(os.path.join(GOLDEN, name + ".jpg"), "rb") as f:
        return f.read()


def golden(name):
    return np.load(os.path.join(GOLDEN, name + ".npz"))["pixels"]


def decode_on_host(rfd, data):
    i = rfd.jpeg_info(data)
    coef = rfd.jpeg_coefficients(data)
    assert coef.shape == (jpeg_ref.num_blocks(i["width"], i["height"], i["sampling"]), 64)
    return jpeg_ref.decode(coef, i["width"], i["height"], i["sampling"])


def test_the_fixture_set_is_complete():
    want = ["%dx%d_%s" % (w, h, s) for w, h in ((1, 1), (8, 8), (17, 9), (37, 53), (64, 48)) for s in ("GRAY", "444", "422", "420")]
    want += ["37x53_420_q5", "37x53_420_q100", "37x53_420_rst2", "37x53_420_com_app1"]
    assert SUPPORTED == sorted(want)
    assert os.path.exists(os.path.join(GOLDEN, "37x53_420_progressive.jpg"))
    assert sum(os.path.getsize(f) for f in glob.glob(os.path.join(GOLDEN, "*"))) < 128 * 1024


@pytest.mark.parametrize("name", SUPPORTED)
def test_info_reports_the_fields_of_every_fixture(rfd, name):
    size, sampling = name.split("_")[:2]
    w, h = (int(v) for v in size.split("x"))
    i = rfd.jpeg_info(load(name))
    assert i == dict(width=w, height=h, components=1 if sampling == "GRAY" else 3, sampling=SAMPLING[sampling],
                     restart_interval=2 if name.endswith("rst2") else 0)
    assert golden(name).shape == ((h, w) if sampling == "GRAY" else (h, w, 3))


def test_info_skips_com_and_app1_and_the_struct_is_zero_padded(rfd):
    import ctypes as C
    data = load("37x53_420_com_app1")
    assert b"rfd golden file" in data and b"\xff\xe1" in data[:40] and data.index(b"\xff\xfe") < data.index(b"\xff\xc0")
    info = rfd.rfd_jpeg_info()
    C.memset(C.byref(info), 0x5a, C.sizeof(info))
    assert C.sizeof(info) == 32
    assert rfd.load_library().rfd_jpeg_info(data, len(data), C.byref(info)) == 0
    assert (info.width, info.height, list(info.reserved)) == (37, 53, [0, 0, 0])


@pytest.mark.parametrize("name", SUPPORTED)
def test_host_decoder_and_numpy_arithmetic_equal_libjpeg_turbo(rfd, name):
    got, want = decode_on_host(rfd, load(name)), golden(name)
    assert got.shape == want.shape and got.dtype == np.uint8
    assert np.array_equal(got, want), "%d pixels differ" % int((got != want).any(-1).sum() if got.ndim == 3 else (got != want).sum())


@pytest.mark.parametrize("sampling", ["GRAY", "444", "422", "420"])
def test_freshly_encoded_random_sizes_equal_pillow(rfd, sampling):
    Image = pytest.importorskip("PIL.Image")
    rng = np.random.default_rng(SAMPLING[sampling] + 11)
    for k in range(20):
        w, h = int(rng.integers(1, 81)), int(rng.integers(1, 81))
        img = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        img[:, :w // 2] = ((np.arange(h)[:, None, None] * 5 + np.arange(w // 2)[None, :, None] * 3) % 256).astype(np.uint8)   # half smooth, half noise
        kw = dict(quality=int(rng.integers(5, 101)))
        if k % 4 == 0:
            kw["restart_marker_blocks"] = int(rng.integers(1, 5))
        buf = io.BytesIO()
        if sampling == "GRAY":
            Image.fromarray(img).convert("L").save(buf, "JPEG", **kw)
        else:
            Image.fromarray(img).save(buf, "JPEG", subsampling={"444": 0, "422": 1, "420": 2}[sampling], **kw)
        data = buf.getvalue()
        want = np.asarray(Image.open(io.BytesIO(data)))
        got = decode_on_host(rfd, data)
        assert got.shape == want.shape and np.array_equal(got, want), (sampling, w, h, kw)


# ---- files written out by hand: one 8x8 (or 16x16) image, one-code Huffman tables ----
def seg(marker, payload):
    return bytes([0xff, marker]) + struct.pack(">H", len(payload) + 2) + payload


def dht(klass, table, symbol):
    """one code of length 1 ("0") for `symbol`"""
    return seg(0xc4, bytes([klass << 4 | table, 1] + [0] * 15 + [symbol]))


def sof(marker=0xc0, precision=8, h=8, w=8, comps=((1, 0x11, 0),)):
    return seg(marker, bytes([precision]) + struct.pack(">HH", h, w) + bytes([len(comps)]) + b"".join(bytes(c) for c in comps))


def sos(comps=((1, 0x00),)):
    return seg(0xda, bytes([len(comps)]) + b"".join(bytes(c) for c in comps) + bytes([0, 63, 0]))


SOI, EOI = b"\xff\xd8", b"\xff\xd9"
DQT = seg(0xdb, bytes([0]) + bytes([1] * 64))
DC0, AC_EOB, AC_RUN = dht(0, 0, 0), dht(1, 0, 0x00), dht(1, 0, 0xf1)   # DC: always 0; AC: end of block / 15 zeros then a 1-bit value
TINY = SOI + DQT + sof() + DC0 + AC_EOB + sos() + b"\x00" + EOI          # bits 0 (DC), 0 (EOB): one grey block of 128
YCC = ((1, 0x11, 0), (2, 0x11, 0), (3, 0x11, 0))


def test_the_hand_written_file_decodes(rfd):
    assert rfd.jpeg_info(TINY) == dict(width=8, height=8, components=1, sampling=rfd.JPEG_GRAY, restart_interval=0)
    assert np.array_equal(rfd.jpeg_coefficients(TINY), np.zeros((1, 64), np.int16))
    assert np.array_equal(decode_on_host(rfd, TINY), np.full((8, 8), 128, np.uint8))
    # a 16-bit quantisation table of 300s, a DC difference of one magnitude bit: code 0, bit 1 (+1), EOB
    sixteen = SOI + seg(0xdb, bytes([0x10]) + struct.pack(">64H", *([300] * 64))) + sof() + dht(0, 0, 1) + AC_EOB + sos() + b"\x40" + EOI
    c = rfd.jpeg_coefficients(sixteen)
    assert c.shape == (1, 64) and c[0, 0] == 300 and not c[0, 1:].any()
    # all-zero data under the run table: DC 0, then "15 zeros and a -1" (code 0, magnitude bit 0) at zigzag 16, 32 and 48
    runs = SOI + DQT + sof() + DC0 + AC_RUN + sos() + b"\x00" + EOI
    st, msg = _run(rfd, runs)
    assert st == rfd.RFD_ERR_INVALID_ARG and "index above 63" in msg       # the fourth run would land on 64


def _patched(data, at, value):
    b = bytearray(data)
    b[at:at + len(value)] = value
    return bytes(b)


def _sof_at(data):
    return data.index(b"\xff\xc0")


F444, F420, RST2 = "37x53_444", "37x53_420", "37x53_420_rst2"


def unsupported_cases():
    d444 = load(F444)
    s = _sof_at(d444)
    return [
        ("progressive", load("37x53_420_progressive"), "progressive"),
        ("12-bit precision", _patched(d444, s + 4, b"\x0c"), "12-bit"),
        ("four components", SOI + DQT + sof(comps=YCC + ((4, 0x11, 0),)) + DC0 + AC_EOB + sos() + b"\x00" + EOI, "four components"),
        ("luma 1x2", _patched(d444, s + 11, b"\x12"), "sampling factors 1x2"),
        ("luma 4x1", _patched(d444, s + 11, b"\x41"), "sampling factors 4x1"),
        ("chroma 2x1", _patched(d444, s + 14, b"\x21"), "sampling factors"),
        ("arithmetic", _patched(d444, s + 1, b"\xc9"), "arithmetic"),
        ("lossless", _patched(d444, s + 1, b"\xc3"), "lossless"),
        ("multi-scan", SOI + DQT + sof(comps=YCC) + DC0 + AC_EOB + sos() + b"\x00" + EOI, "multi-scan"),
    ]


def malformed_cases():
    d420, rst = load(F420), load(RST2)
    dqt, scan = d420.index(b"\xff\xdb"), d420.index(b"\xff\xda")
    first_rst = rst.index(b"\xff\xd0", rst.index(b"\xff\xda"))
    return [
        ("length past the end", _patched(d420, dqt + 2, b"\xff\xff"), "points past the end"),
        ("length below 2", _patched(d420, dqt + 2, b"\x00\x01"), "less than 2"),
        ("code not in the table", SOI + DQT + sof() + DC0 + AC_EOB + sos() + b"\x80" + EOI, "not in DC table"),
        ("AC code not in the table", SOI + DQT + sof() + DC0 + AC_EOB + sos() + b"\x40" + EOI, "not in AC table"),
        ("coefficient index above 63", SOI + DQT + sof() + DC0 + AC_RUN + sos() + b"\x2a\xa0" + EOI, "index above 63"),
        ("missing AC table", SOI + DQT + sof() + DC0 + sos() + b"\x00" + EOI, "missing table"),
        ("missing DC table", SOI + DQT + sof() + AC_EOB + sos() + b"\x00" + EOI, "missing table"),
        ("missing quantisation table", SOI + sof() + DC0 + AC_EOB + sos() + b"\x00" + EOI, "missing table"),
        ("zero height", SOI + DQT + sof(h=0) + DC0 + AC_EOB + sos() + b"\x00" + EOI, "zero dimensions"),
        ("zero width", SOI + DQT + sof(w=0) + DC0 + AC_EOB + sos() + b"\x00" + EOI, "zero dimensions"),
        ("RST out of sequence", _patched(rst, first_rst + 1, b"\xd1"), "RST out of sequence"),
        ("RST missing", rst[:first_rst] + rst[first_rst + 2:], "RST"),
        ("data ends before the last MCU", d420[:scan + 40], "truncated"),
        ("EOI before the last MCU", d420[:scan + 40] + EOI, "before MCU"),
        ("cut in front of SOS", d420[:scan], "truncated"),
        ("no SOI", d420[2:], "SOI"),
        ("empty", b"", "null"),
        ("SOS before SOF", SOI + DQT + DC0 + AC_EOB + sos() + b"\x00" + EOI, "before any SOF"),
        ("not a prefix code", SOI + DQT + sof() + seg(0xc4, bytes([0, 3] + [0] * 15 + [0, 1, 2])) + AC_EOB + sos() + b"\x00" + EOI, "prefix code"),
    ]


def _run(rfd, data):
    """(status, message) of rfd_jpeg_info, then of rfd_debug_jpeg_coefficients where the header passes"""
    L = rfd.load_library()
    buf = np.frombuffer(data, np.uint8)
    addr = buf.ctypes.data if buf.size else None
    import ctypes as C
    info = rfd.rfd_jpeg_info()
    C.memset(C.byref(info), 0x5a, C.sizeof(info))
    st = L.rfd_jpeg_info(addr, buf.size, C.byref(info))
    if st != 0:
        assert info.width == 0x5a5a5a5a                                # nothing is reported about a refused file
        return st, L.rfd_last_error().decode()
    blocks = C.c_size_t()
    out = np.zeros((4096, 64), np.int16)
    st = L.rfd_debug_jpeg_coefficients(addr, buf.size, out.ctypes.data, 4096, C.byref(blocks))
    return st, L.rfd_last_error().decode() if st else ""


@pytest.mark.parametrize("case", range(9))
def test_an_unsupported_file_is_refused_and_the_message_names_the_kind(rfd, case):
    name, data, needle = unsupported_cases()[case]
    st, msg = _run(rfd, data)
    assert st == rfd.RFD_ERR_UNSUPPORTED == -8, (name, st, msg)
    assert needle in msg and "byte" in msg, (name, msg)
    with pytest.raises(rfd.RfdError) as e:
        rfd.jpeg_info(data)
    assert e.value.status == rfd.RFD_ERR_UNSUPPORTED


@pytest.mark.parametrize("case", range(19))
def test_a_malformed_file_is_refused_and_the_message_names_the_cause(rfd, case):
    name, data, needle = malformed_cases()[case]
    st, msg = _run(rfd, data)
    assert st == rfd.RFD_ERR_INVALID_ARG, (name, st, msg)
    assert needle in msg, (name, msg)
    if name != "empty":
        assert "byte" in msg, (name, msg)                              # the offset is part of the message


def test_the_case_lists_have_the_lengths_the_parametrisation_assumes():
    assert len(unsupported_cases()) == 9 and len(malformed_cases()) == 19


def test_the_coefficient_hook_reports_the_block_count_and_refuses_a_small_buffer(rfd):
    import ctypes as C
    L, data = rfd.load_library(), load(F420)
    blocks = C.c_size_t()
    assert L.rfd_debug_jpeg_coefficients(data, len(data), None, 0, C.byref(blocks)) == rfd.RFD_ERR_CAPACITY
    assert blocks.value == jpeg_ref.num_blocks(37, 53, jpeg_ref.S420) == 3 * 4 * 6
    assert L.rfd_debug_jpeg_coefficients(data, len(data), None, 5, C.byref(blocks)) == rfd.RFD_ERR_INVALID_ARG


def test_the_symbols_and_the_status_are_part_of_the_interface(rfd):
    for name in ("rfd_jpeg_info", "rfd_decode_jpeg_batch_device", "rfd_decode_jpeg_batch", "rfd_set_decode_threads", "rfd_debug_jpeg_coefficients"):
        assert name in rfd.API_SYMBOLS and hasattr(rfd.load_library(), name)
    txt = open(os.path.join(ROOT, "include", "rfd.h")).read()
    assert "RFD_ERR_UNSUPPORTED = -8" in txt


def test_the_front_end_alone_under_address_and_ub_sanitizers(tmp_path):
    """tests/cpp/jpeg_parse_check.cpp: a valid file cut at every byte and with every one of its first 700 bytes replaced by 0x00
    and 0xFF, through the parser and the entropy decoder, in a program of its own whose every out-of-bounds access or undefined
    operation aborts it.  Built as tests/test_gallery_file_cpu.py builds its program; a plain build where the sanitizer
    runtimes cannot be linked."""
    exe = str(tmp_path / "jpeg_parse_check")
    src = os.path.join(ROOT, "tests", "cpp", "jpeg_parse_check.cpp")
    base = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", src, "-o", exe]
    san = subprocess.run(base + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan"], capture_output=True, text=True)
    if san.returncode != 0:
        plain = subprocess.run(base, capture_output=True, text=True)
        assert plain.returncode == 0, "the build failed:\n" + san.stderr + plain.stderr
    files = [os.path.join(GOLDEN, n + ".jpg") for n in (F420, RST2, "37x53_GRAY")]
    run = subprocess.run([exe] + files, capture_output=True, text=True)
    assert run.returncode == 0 and " 0 failures" in run.stdout, run.stdout + run.stderr
