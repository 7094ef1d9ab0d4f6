"""Cases of tests/jpeg_cases.py written again with a chosen restart interval, for the device entropy decoder (include/rfd.h,
"entropy decoding on the device"): tests/test_jpeg_entropy_cpu.py (pre-scan, the shared interval decoder under the host
sanitizers) and tests/test_jpeg_entropy_gpu.py (the kernel).  The quantised coefficients of a case are recovered from its
dequantised ones (the division is exact, asserted) and handed to tests/jpeg_write.py with restart_interval = R; coefficients
and pixels expected of the new file are therefore the case's own.

The list asserts, while it is built, every property a test relies on: the number and the order of the restart markers, more
than 64 intervals in one frame, codes longer than the 9 bits of the fast table, intervals that end in a stuffed 0xFF00, DC
levels that differ between intervals."""
import functools
import re
from typing import NamedTuple

import numpy as np

import jpeg_cases
import jpeg_ref
import jpeg_write

MAX_INTERVAL = 128                 # kJpegDeviceMaxInterval (csrc/jpeg_entropy.h)
GEOMETRY = ("geo_20x16_GRAY", "geo_66x17_444", "geo_33x17_422", "geo_17x9_420")          # all four samplings
EXTRA = (("restart_3", 7), ("geo_17x9_420", 65535))                                      # a short last interval; R far above the MCU count


class Entry(NamedTuple):
    name: str                      # "<case>@R<restart interval>"
    data: bytes
    coef: np.ndarray               # [blocks, 64] i16 dequantised, natural order
    width: int
    height: int
    sampling: int
    restart_interval: int
    quant: tuple
    intervals: tuple               # ((begin, end), ...) byte positions in data, as the writer laid them out
    mcus: int
    long_codes: int                # AC Huffman codes of more than 9 bits in the file
    case: str


def _quantised(case):
    dims = jpeg_ref.geometry(case.width, case.height, case.sampling)[1]
    q = np.concatenate([np.broadcast_to(t, (bw * bh, 64)) for t, (bw, bh) in zip(case.quant, dims)])
    coef_q, rem = np.divmod(case.coef.astype(np.int64), q)
    assert not rem.any(), case.name
    return coef_q


def _ac_symbols(zz):
    run = 0
    last = max([k for k in range(1, 64) if zz[k]], default=0)
    for k in range(1, last + 1):
        if zz[k] == 0:
            run += 1
            continue
        for _ in range(run >> 4):
            yield 0xf0
        yield (run & 15) << 4 | abs(zz[k]).bit_length()
        run = 0
    if last < 63:
        yield 0x00


def _count_long_codes(coef_q, width, height, sampling):
    dims = jpeg_ref.geometry(width, height, sampling)[1]
    first_chroma = dims[0][0] * dims[0][1]
    zz = coef_q[:, jpeg_write.NATURAL].tolist()
    return sum(jpeg_write._CODE[1, int(b >= first_chroma)][s][1] > 9 for b, row in enumerate(zz) for s in _ac_symbols(row))


def scan_start(data):
    at = data.index(b"\xff\xda")
    return at + 2 + int.from_bytes(data[at + 2:at + 4], "big")


def marker_intervals(data):
    """the intervals of a file this writer made, by its markers: entropy-coded data holds 0xFF only in front of 0x00, so every
    0xFF 0xD0..0xD7 behind the SOS header is a restart marker and the 0xFF 0xD9 at the very end is EOI"""
    scan = scan_start(data)
    assert data.endswith(b"\xff\xd9")
    marks = [m.start() for m in re.finditer(rb"\xff[\xd0-\xd7]", data) if m.start() >= scan]
    for k, at in enumerate(marks):
        assert data[at + 1] == 0xd0 + k % 8, "restart marker %d is 0x%02x" % (k, data[at + 1])
    return tuple(zip([scan] + [at + 2 for at in marks], marks + [len(data) - 2]))


def rewrite(case, restart_interval):
    coef_q = _quantised(case)
    data = jpeg_write.write(coef_q, case.width, case.height, case.sampling, case.quant, restart_interval)
    mcux, mcuy = jpeg_ref.geometry(case.width, case.height, case.sampling)[1][-1]
    intervals = marker_intervals(data)
    assert len(intervals) == -(-mcux * mcuy // restart_interval), (case.name, restart_interval, len(intervals))
    assert all(b < e for b, e in intervals)
    return Entry("%s@R%d" % (case.name, restart_interval), data, case.coef, case.width, case.height, case.sampling, restart_interval, case.quant, intervals,
                 mcux * mcuy, _count_long_codes(coef_q, case.width, case.height, case.sampling), case.name)


def ends_stuffed(entry):
    """the intervals whose last two bytes are a stuffed 0xFF 0x00"""
    return [k for k, (b, e) in enumerate(entry.intervals) if e - b >= 2 and entry.data[e - 2:e] == b"\xff\x00"]


def first_dc(entry):
    """the quantised DC coefficient of the first block of every interval (luma block of the interval's first MCU)"""
    dims, (hmax, vmax) = jpeg_ref.geometry(entry.width, entry.height, entry.sampling)[1:]
    mcux = dims[-1][0]
    out = []
    for k in range(len(entry.intervals)):
        my, mx = divmod(k * entry.restart_interval, mcux)
        out.append(int(entry.coef[my * vmax * dims[0][0] + mx * hmax, 0]) // int(entry.quant[0][0]))
    return out


@functools.lru_cache(maxsize=None)
def entries():
    base = {c.name: c for c in jpeg_cases.cases()}
    names = [c.name for c in jpeg_cases.cases() if not c.name.startswith(("geo_", "colour_grid"))] + list(GEOMETRY)
    out = [rewrite(base[n], r) for n in names for r in (1, 3)] + [rewrite(base[n], r) for n, r in EXTRA]
    by = {e.name: e for e in out}
    assert len(by) == len(out)
    assert sum(len(e.intervals) for e in out if e.restart_interval in (1, 3)) == 3010
    assert len(by["restart_1@R1"].intervals) == 20                                      # RST7 -> RST0 twice
    assert len(by["restart_3@R3"].intervals) == 7 and len(by["restart_3@R7"].intervals) == 3 and by["restart_3@R7"].mcus == 20   # 5 x 4 MCUs: rows are crossed, the last interval is short
    assert len(by["geo_17x9_420@R3"].intervals) == 1 == len(by["geo_17x9_420@R65535"].intervals)    # R >= MCUs: no marker in the file
    assert {by[n + "@R1"].sampling for n in GEOMETRY} == set(jpeg_cases.SAMPLINGS)
    assert len(ends_stuffed(by["geo_33x17_422@R1"])) >= 1
    assert sum(len(ends_stuffed(e)) for e in out) >= 10
    assert len(by["saturation_GRAY@R1"].intervals) == 832 and len(by["zigzag_single_420@R1"].intervals) == 65       # more than one workgroup per frame
    assert by["zigzag_single_420@R1"].long_codes > 0 and sum(e.long_codes for e in out) > 1000
    assert all(not by["zigzag_zero_%s@R%d" % (s, r)].coef.any() for s in ("GRAY", "420") for r in (1, 3))
    assert any(np.asarray(q).max() > 255 for q in by["zigzag_single_GRAY@R1"].quant) and any(np.asarray(q).max() > 255 for q in by["restart_3@R3"].quant)
    for n in ("restart_1@R1", "restart_3@R3"):                                          # a decoder that keeps the predictor gets these wrong
        dc = first_dc(by[n])
        assert len({v for v in dc if v}) >= 2, (n, dc)
    return tuple(out)


def entry(name):
    return {e.name: e for e in entries()}[name]


def over_the_cap():
    """restart_1 with R = MAX_INTERVAL + 1: R only has to exceed the constant, not the MCU count"""
    return rewrite({c.name: c for c in jpeg_cases.cases()}["restart_1"], MAX_INTERVAL + 1)


def without_restarts(e):
    """the same case with no DRI at all: never eligible"""
    case = {c.name: c for c in jpeg_cases.cases()}[e.case]
    data = jpeg_write.write(_quantised(case), case.width, case.height, case.sampling, case.quant, 0)
    return e._replace(name=e.case + "@R0", data=data, restart_interval=0, intervals=())


class Damaged(NamedTuple):
    name: str
    data: bytes
    base: Entry
    host_accepts: bool


@functools.lru_cache(maxsize=None)
def damaged():
    """restart_3@R3 (7 intervals) damaged in five ways.  Only "garbage" is a file the lenient host decoder accepts."""
    e = entry("restart_3@R3")
    d, iv = e.data, e.intervals
    b2, e2 = iv[2]
    assert e2 - b2 >= 8 and d[e2 - 1] != 0 and d[e2 - 2] != 0xff and d[e2:e2 + 2] == b"\xff\xd2"
    out = [
        Damaged("invalid_code", d[:b2] + b"\xff\x00\xff\x00" + d[b2 + 4:], e, False),   # sixteen 1 bits where a DC code is due: a code of no table
        Damaged("truncated_interval", d[:e2 - 1] + d[e2:], e, False),                   # the interval's last byte is gone, its marker moved up
        Damaged("rst_out_of_sequence", d[:e2 + 1] + b"\xd3" + d[e2 + 2:], e, False),
        Damaged("data_ends_early", d[:iv[5][0] + 3], e, False),
        Damaged("garbage", d[:e2] + b"\x12\x34\x56" + d[e2:], e, True),                 # three bytes in front of RST2
    ]
    assert all(len(x.data) > 0 and x.data != d for x in out)
    return tuple(out)
