"""Exif APP1 segments built by hand, and the eight EXIF orientations in numpy: what tests/test_jpeg_orientation_cpu.py and
tests/test_jpeg_orientation_gpu.py put into their files and compare the decoded frames with.

app1() writes the segment (include/rfd.h, "EXIF orientation"): "Exif\\0\\0", a TIFF header (byte order, 42, the offset of IFD0)
and IFD0 with the orientation entry at a chosen place among filler entries; every field can be set to something a reader must
not trust, and the payload can be cut.  The segment goes through jpeg_write.write(..., extra_segments=...) or behind the SOI of
a finished file (tagged()).  orient() is judged by Pillow in test_jpeg_orientation_cpu.py, not by the code under test."""
import struct

import numpy as np

TAG_ORIENTATION = 0x0112
BYTE, ASCII, SHORT, LONG, RATIONAL = 1, 2, 3, 4, 5
EXIF_ID = b"Exif\0\0"
XMP_ID = b"http://ns.adobe.com/xap/1.0/\0"
_FILLER_TAGS = (0x010f, 0x0110, 0x011a, 0x011b, 0x0128, 0x0131, 0x0132, 0x0213)   # make, model, resolutions, ...: all below or above 0x0112


def segment(marker, payload):
    return bytes([0xff, marker]) + struct.pack(">H", len(payload) + 2) + payload


def tiff(value=6, order="<", type_=SHORT, count=1, entries=1, position=0, ifd_offset=8, byte_order_mark=None, magic=42,
         entry_count=None, with_tag=True, gap=None):
    """the TIFF block: `entries` IFD0 entries at `ifd_offset` (the gap is filled with 0xEE), the orientation entry at index
    `position` unless with_tag is false; entry_count overrides the count the directory announces, gap the bytes really placed
    between the header and IFD0 (for an offset that points far away)"""
    assert order in "<>" and 0 <= position < entries and ifd_offset >= 8
    e = []
    for k in range(entries):
        if k == position and with_tag:
            field = struct.pack(order + "H", value & 0xffff) + b"\0\0" if type_ == SHORT else struct.pack(order + "I", value & 0xffffffff)
            e.append(struct.pack(order + "HHI", TAG_ORIENTATION, type_, count) + field)
        else:   # a SHORT that is not the orientation, with a value that would be a valid one
            e.append(struct.pack(order + "HHIHH", _FILLER_TAGS[k % len(_FILLER_TAGS)], SHORT, 1, 3, 0))
    mark = byte_order_mark if byte_order_mark is not None else (b"II" if order == "<" else b"MM")
    head = mark + struct.pack(order + "HI", magic, ifd_offset)
    n = len(e) if entry_count is None else entry_count
    return head + b"\xee" * (ifd_offset - 8 if gap is None else gap) + struct.pack(order + "H", n) + b"".join(e) + struct.pack(order + "I", 0)


def app1(cut=None, marker=0xe1, ident=EXIF_ID, **kw):
    """the APP1 segment around tiff(**kw); cut: keep only the first `cut` bytes of the payload"""
    payload = ident + tiff(**kw)
    return segment(marker, payload if cut is None else payload[:cut])


def entry_offset(position=0, ifd_offset=8):
    """payload offset of IFD0 entry `position`"""
    return len(EXIF_ID) + ifd_offset + 2 + 12 * position


def tagged(data, seg):
    """a finished file with `seg` spliced in right behind its SOI"""
    assert data[:2] == b"\xff\xd8"
    return data[:2] + seg + data[2:]


def before_sos(data, seg):
    """a finished file with `seg` spliced in right in front of its SOS (behind SOF, DHT, ...)"""
    at = data.index(b"\xff\xda")
    return data[:at] + seg + data[at:]


def orient(a, o):
    """[H, W, ...] stored pixels -> the frame of orientation o, as the table of include/rfd.h states it"""
    a = np.asarray(a)
    assert 1 <= o <= 8
    if o in (2, 3):
        a = a[:, ::-1]
    if o in (3, 4):
        a = a[::-1]
    if o >= 5:                       # out[yo][xo] = S[f(xo)][g(yo)]: transpose, then mirror what the table mirrors
        a = np.swapaxes(a, 0, 1)     # 5: out[yo][xo] = S[xo][yo]
        if o in (6, 7):
            a = a[:, ::-1]           # S[H-1-xo][..]
        if o in (7, 8):
            a = a[::-1]              # S[..][W-1-yo]
    return np.ascontiguousarray(a)


def orient_by_index(a, o):
    """the same, written out index by index from the table: slow, for small arrays, a check on orient() itself"""
    a = np.asarray(a)
    H, W = a.shape[:2]
    Ho, Wo = (W, H) if o >= 5 else (H, W)
    out = np.zeros((Ho, Wo) + a.shape[2:], a.dtype)
    for yo in range(Ho):
        for xo in range(Wo):
            sy, sx = {1: (yo, xo), 2: (yo, W - 1 - xo), 3: (H - 1 - yo, W - 1 - xo), 4: (H - 1 - yo, xo),
                      5: (xo, yo), 6: (H - 1 - xo, yo), 7: (H - 1 - xo, W - 1 - yo), 8: (xo, W - 1 - yo)}[o]
            out[yo, xo] = a[sy, sx]
    return out
