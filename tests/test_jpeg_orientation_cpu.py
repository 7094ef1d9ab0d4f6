"""The EXIF reader of the JPEG front end (include/rfd.h, "EXIF orientation"; csrc/jpeg_parse.h) without a GPU: the eight index
maps of tests/jpeg_exif.py against Pillow's ImageOps.exif_transpose, rfd_jpeg_orientation against Pillow's getexif() on
well-formed segments, orientation 1 and RFD_OK on every kind of damage, the refusal of a file the decoder does not do, and the
reader alone under AddressSanitizer and UBSan in a program of its own (tests/cpp/jpeg_exif_check.cpp)."""
import ctypes as C
import glob
import io
import os
import subprocess

import numpy as np
import pytest

import jpeg_exif
from jpeg_exif import BYTE, LONG, RATIONAL, SHORT, app1, before_sos, orient, tagged

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "jpeg")
FILE = "37x53_444"                  # not square, so a swapped size shows
JFIF = jpeg_exif.segment(0xe0, b"JFIF\0\1\1\0\0\1\0\1\0\0")


def load(name):
    with open(os.path.join(GOLDEN, name + ".jpg"), "rb") as f:
        return f.read()


def orientation(rfd, data):
    """(status, dict or None) of rfd_jpeg_orientation through the Python wrapper's struct, which starts out as 0x5a bytes"""
    o = rfd.rfd_jpeg_orientation()
    C.memset(C.byref(o), 0x5a, C.sizeof(o))
    st = rfd.load_library().rfd_jpeg_orientation(data, len(data), C.byref(o))
    if st != 0:
        assert bytes(o) == b"\x5a" * C.sizeof(o)                       # a refused file leaves *out untouched
        return st, None
    assert list(o.reserved) == [0, 0, 0]
    return st, dict(orientation=o.orientation, width=o.width, height=o.height, stored_width=o.stored_width, stored_height=o.stored_height)


def upright(rfd, data):
    i = rfd.jpeg_info(data)
    return 0, dict(orientation=1, width=i["width"], height=i["height"], stored_width=i["width"], stored_height=i["height"])


def test_the_numpy_maps_follow_the_table_index_by_index():
    a = np.arange(5 * 7 * 3).reshape(5, 7, 3)
    for o in range(1, 9):
        assert np.array_equal(orient(a, o), jpeg_exif.orient_by_index(a, o)), o
        assert orient(a, o).shape == ((7, 5, 3) if o >= 5 else (5, 7, 3))


@pytest.mark.parametrize("order", "<>")
def test_the_numpy_maps_equal_pillows_exif_transpose(order):
    Image = pytest.importorskip("PIL.Image")
    ImageOps = pytest.importorskip("PIL.ImageOps")
    data = load(FILE)
    stored = np.asarray(Image.open(io.BytesIO(data)))
    assert stored.shape == (53, 37, 3)
    for o in range(1, 9):
        want = np.asarray(ImageOps.exif_transpose(Image.open(io.BytesIO(tagged(data, app1(value=o, order=order))))))
        assert np.array_equal(orient(stored, o), want), (o, order)
    for o in (0, 9):                                                   # Pillow ignores them as well
        want = np.asarray(ImageOps.exif_transpose(Image.open(io.BytesIO(tagged(data, app1(value=o, order=order))))))
        assert np.array_equal(stored, want), (o, order)


def well_formed():
    """(name, segment, where) -- where: "soi" behind SOI, "jfif" behind SOI and a JFIF APP0, "sos" in front of SOS"""
    out = [("value_%d_%s" % (o, "II" if order == "<" else "MM"), dict(value=o, order=order), "soi") for o in range(1, 9) for order in "<>"]
    for order in "<>":
        e = "II" if order == "<" else "MM"
        out += [("first_of_5_" + e, dict(value=6, order=order, entries=5, position=0), "soi"),
                ("middle_of_5_" + e, dict(value=8, order=order, entries=5, position=2), "soi"),
                ("last_of_5_" + e, dict(value=3, order=order, entries=5, position=4), "soi"),
                ("ifd_at_100_" + e, dict(value=5, order=order, ifd_offset=100, entries=3, position=1), "soi"),
                ("long_" + e, dict(value=7, order=order, type_=LONG), "soi"),
                ("jfif_in_front_" + e, dict(value=6, order=order), "jfif"),
                ("behind_sof_" + e, dict(value=8, order=order), "sos")]
    return out


def place(data, seg, where):
    return {"soi": tagged(data, seg), "jfif": tagged(data, JFIF + seg), "sos": before_sos(data, seg)}[where]


@pytest.mark.parametrize("name,kw,where", well_formed(), ids=[c[0] for c in well_formed()])
def test_a_well_formed_tag_is_read_as_pillow_reads_it(rfd, name, kw, where):
    Image = pytest.importorskip("PIL.Image")
    data = place(load(FILE), app1(**kw), where)
    if where == "sos":
        assert data.index(b"\xff\xc0") < data.index(b"\xff\xe1") < data.index(b"\xff\xda")
    want = Image.open(io.BytesIO(data)).getexif().get(0x0112)
    assert want == kw["value"]
    st, got = orientation(rfd, data)
    w, h = (53, 37) if want >= 5 else (37, 53)
    assert st == 0 and got == dict(orientation=want, width=w, height=h, stored_width=37, stored_height=53), (name, got)
    assert rfd.jpeg_orientation(data) == got
    assert rfd.jpeg_info(data) == rfd.jpeg_info(load(FILE))            # rfd_jpeg_info reports what it did


def damaged():
    """(name, the bytes between SOI and the rest of the file): every one leaves orientation 1 and the file accepted"""
    tag = jpeg_exif.entry_offset(position=1)                           # payload offset of the tag's entry in the cut cases
    return [("value_0", app1(value=0)), ("value_9", app1(value=9)), ("value_65535", app1(value=65535)),
            ("value_9_long_MM", app1(value=9, type_=LONG, order=">")), ("value_65542_long", app1(value=65536 + 6, type_=LONG)),
            ("type_byte", app1(value=6, type_=BYTE)), ("type_rational", app1(value=6, type_=RATIONAL)),
            ("count_0", app1(value=6, count=0)), ("count_2", app1(value=6, count=2)), ("count_2_long", app1(value=6, type_=LONG, count=2)),
            ("bad_byte_order_mark", app1(value=6, byte_order_mark=b"IM")), ("bad_byte_order_mark_lower", app1(value=6, byte_order_mark=b"ii")),
            ("bad_42", app1(value=6, magic=43)), ("bad_42_swapped", app1(value=6, magic=42 << 8)),
            ("ifd_past_the_payload", app1(value=6, ifd_offset=0x7fffffff, gap=0)),
            ("ifd_at_0xffffffff", app1(value=6, ifd_offset=0xffffffff, gap=0)),
            ("ifd_one_past_the_end", app1(value=6, ifd_offset=8 + 18 + 1, gap=0)),
            ("ifd_exactly_at_the_end", app1(value=6, ifd_offset=8, cut=6 + 8)),
            ("ifd_one_byte_before_the_end", app1(value=6, ifd_offset=8, cut=6 + 8 + 1)),
            ("entry_count_past_the_payload", app1(value=6, entries=2, position=1, entry_count=3, with_tag=False)),
            ("entry_count_65535", app1(value=6, entries=2, position=1, entry_count=65535, with_tag=False)),
            ("cut_inside_the_tags_entry", app1(value=6, entries=3, position=1, cut=tag + 9)),
            ("cut_at_the_tags_entry", app1(value=6, entries=3, position=1, cut=tag)),
            ("cut_one_byte_short_of_the_entry", app1(value=6, entries=3, position=1, cut=tag + 11)),
            ("no_tag", app1(entries=4, position=0, with_tag=False)), ("no_entries", app1(entries=1, entry_count=0)),
            ("header_only", app1(cut=6)), ("cut_in_the_header", app1(cut=6 + 5)),
            ("xmp_app1", app1(value=6, ident=jpeg_exif.XMP_ID)),
            ("exif_in_app2", app1(value=6, marker=0xe2)),
            ("two_exif_the_first_wins_with_1", app1(value=1) + app1(value=6)),
            ("two_exif_the_first_is_broken", app1(value=6, magic=0) + app1(value=6)),
            ("two_exif_the_first_has_no_tag", app1(with_tag=False) + app1(value=8))]


@pytest.mark.parametrize("name,segs", damaged(), ids=[c[0] for c in damaged()])
def test_anything_else_is_orientation_1_and_never_a_refusal(rfd, name, segs):
    data = tagged(load(FILE), segs)
    assert orientation(rfd, data) == upright(rfd, data), name
    assert rfd.jpeg_info(data) == rfd.jpeg_info(load(FILE))
    assert np.array_equal(rfd.jpeg_coefficients(data), rfd.jpeg_coefficients(load(FILE)))


def test_of_two_exif_segments_the_first_wins(rfd):
    data = tagged(load(FILE), app1(value=3) + app1(value=6))
    assert orientation(rfd, data)[1]["orientation"] == 3
    data = tagged(load(FILE), app1(value=6, ident=jpeg_exif.XMP_ID) + app1(value=6, marker=0xe2) + app1(value=5, order=">") + app1(value=2))
    assert orientation(rfd, data)[1] == dict(orientation=5, width=53, height=37, stored_width=37, stored_height=53)


def test_every_golden_file_is_upright(rfd):
    names = sorted(os.path.basename(f)[:-4] for f in glob.glob(os.path.join(GOLDEN, "*.npz")))
    assert len(names) == 24 and "37x53_420_com_app1" in names
    for name in names:
        data = load(name)
        assert orientation(rfd, data) == upright(rfd, data), name
    data = load("37x53_420_com_app1")                                  # Exif with no orientation
    at = data.index(b"\xff\xe1")
    assert data[at + 4:at + 10] == jpeg_exif.EXIF_ID


def test_a_refused_file_is_refused_alike_and_the_output_stays_untouched(rfd):
    L = rfd.load_library()
    for data in (load("37x53_420_progressive"), tagged(load("37x53_420_progressive"), app1(value=6)), load(FILE)[:100], load(FILE)[2:]):
        st_info = L.rfd_jpeg_info(data, len(data), C.byref(rfd.rfd_jpeg_info()))
        msg_info = L.rfd_last_error().decode()
        st, got = orientation(rfd, data)
        assert st == st_info != 0 and got is None
        assert L.rfd_last_error().decode() == msg_info and msg_info
    assert L.rfd_jpeg_orientation(None, 0, None) == L.rfd_jpeg_info(None, 0, None) == rfd.RFD_ERR_INVALID_ARG
    with pytest.raises(rfd.RfdError) as e:
        rfd.jpeg_orientation(load("37x53_420_progressive"))
    assert e.value.status == rfd.RFD_ERR_UNSUPPORTED and "progressive" in str(e.value)


def test_the_structs_keep_their_layout(rfd):
    assert C.sizeof(rfd.rfd_jpeg_orientation) == 32 and rfd.rfd_jpeg_orientation.reserved.offset == 20
    assert C.sizeof(rfd.rfd_jpeg_info) == 32 and rfd.rfd_jpeg_info.reserved.offset == 20
    info = rfd.rfd_jpeg_info()
    C.memset(C.byref(info), 0x5a, C.sizeof(info))
    data = tagged(load(FILE), app1(value=6))
    assert rfd.load_library().rfd_jpeg_info(data, len(data), C.byref(info)) == 0
    assert (info.width, info.height, list(info.reserved)) == (37, 53, [0, 0, 0])
    for name in ("rfd_jpeg_orientation", "rfd_set_jpeg_orientation", "rfd_jpeg_last_orientations"):
        assert name in rfd.API_SYMBOLS and hasattr(rfd.load_library(), name)
    assert (rfd.JPEG_ORIENTATION_IGNORE, rfd.JPEG_ORIENTATION_APPLY) == (0, 1)
    L = rfd.load_library()
    assert L.rfd_set_jpeg_orientation(None, 1) == rfd.RFD_ERR_INVALID_ARG          # no context
    assert L.rfd_jpeg_last_orientations(None, None, 0, None) == rfd.RFD_ERR_INVALID_ARG


def test_the_exif_reader_alone_under_address_and_ub_sanitizers(tmp_path):
    """tests/cpp/jpeg_exif_check.cpp over a file whose Exif segment holds five entries behind a gap, the tag in the middle: every
    payload byte replaced by 0x00, 0x7F, 0x80 and 0xFF and the payload cut at every length, each run RFD_OK, the stored size
    unchanged, the orientation in 1 .. 8.  Built as tests/test_jpeg_cpu.py builds jpeg_parse_check; a plain build where the
    sanitizer runtimes cannot be linked."""
    exe = str(tmp_path / "jpeg_exif_check")
    src = os.path.join(ROOT, "tests", "cpp", "jpeg_exif_check.cpp")
    base = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", src, "-o", exe]
    san = subprocess.run(base + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan"], capture_output=True, text=True)
    if san.returncode != 0:
        plain = subprocess.run(base, capture_output=True, text=True)
        assert plain.returncode == 0, "the build failed:\n" + san.stderr + plain.stderr
    for k, kw in enumerate((dict(value=6, order="<", entries=5, position=2, ifd_offset=20), dict(value=8, order=">", type_=LONG, entries=2, position=1))):
        seg = app1(**kw)
        path = str(tmp_path / ("exif_%d.jpg" % k))
        with open(path, "wb") as f:
            f.write(tagged(load(FILE), JFIF + seg))
        run = subprocess.run([exe, path, str(2 + len(JFIF) + 4), str(len(seg) - 4)], capture_output=True, text=True)
        assert run.returncode == 0 and " 0 failures" in run.stdout, run.stdout + run.stderr
        calls, uprights = (int(v) for v in run.stdout.split(":")[1].replace(",", "").split()[0:3:2])
        assert calls > 4 * (len(seg) - 4) * 0.9 and 0 < uprights < calls   # some damage leaves the tag readable, some does not
