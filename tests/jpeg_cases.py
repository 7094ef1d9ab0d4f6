"""One seeded list of JPEG files written by tests/jpeg_write.py from chosen coefficients, shared by tests/test_jpeg_write_cpu.py
(libjpeg-turbo judges tests/jpeg_ref.py on exactly these files) and tests/test_jpeg_sweep_gpu.py (the kernels against jpeg_ref).

Every case is inside the contract include/rfd.h pins, and the list asserts it while it is built: every dequantised coefficient
lies in i16 and every sample of jpeg_ref.idct_unclamped in [-384, 383], so the level-shifted sample lies in [-256, 511]: enough
overshoot to take both clamps, and inside the range where libjpeg's range-limit table and its SIMD paths agree with a clamp.

The forward DCT of the natural-content cases runs in fixed point (a basis rounded to 2^-14, integer products, integer rounding),
so that no tie in a float division can round one way on one machine and the other way on the next: the files are the same bytes
wherever the list is built."""
import functools
from typing import NamedTuple

import numpy as np

import jpeg_ref
import jpeg_write
from jpeg_ref import GRAY, S420, S422, S444

SAMPLINGS = (GRAY, S444, S422, S420)
SAMPLING_NAME = {GRAY: "GRAY", S444: "444", S422: "422", S420: "420"}
GEOMETRY_WIDTHS = list(range(1, 21)) + [31, 32, 33, 63, 64, 65, 66]
GEOMETRY_HEIGHTS = [1, 2, 3, 4, 7, 8, 9, 15, 16, 17]
WIDE = [(520, 16, S420), (264, 8, S444), (264, 8, GRAY), (272, 8, S422)]
GRID_CR = [0, 1, 127, 128, 129, 254, 255]
GRID_Y = [0, 128, 255]
GRID_BLOCKS_PER_ROW = 128          # 1024 pixels
SAMPLE_MIN, SAMPLE_MAX = -384, 383


class Case(NamedTuple):
    name: str
    data: bytes
    coef: np.ndarray               # [blocks, 64] i16 dequantised, natural order: what rfd.jpeg_coefficients must return
    width: int
    height: int
    sampling: int
    restart_interval: int
    quant: tuple                   # one [64] table per component, natural order


_V, _U = np.mgrid[:8, :8]          # vertical and horizontal frequency of natural index v * 8 + u


def _table(base, du, dv):
    return (base + du * _U + dv * _V).reshape(64)


LUMA8, CB, CR = _table(3, 2, 3), _table(5, 4, 3), _table(6, 3, 5)
LUMA16 = np.where(_U + _V >= 12, 250 + 10 * (_U + _V), 4 + 3 * _U + 2 * _V).reshape(64)    # six entries of 370 .. 390: a 16-bit DQT entry
SATURATION = [_table(8, 4, 4), _table(4, 5, 3), _table(2, 3, 6)]                           # DC steps of 8, 4 and 2: flat levels are exact

_K = np.arange(8)
_BASIS = np.rint(np.cos((2 * _K[None, :] + 1) * _K[:, None] * np.pi / 16) * np.where(_K[:, None] == 0, np.sqrt(0.125), 0.5) * (1 << 14)).astype(np.int64)


def _quantise(plane, q):
    """[rows, cols] u8 plane of whole blocks -> [blocks, 64] quantised coefficients: the 8x8 DCT of the level-shifted samples,
    divided by q and rounded half away from zero"""
    bh, bw = plane.shape[0] // 8, plane.shape[1] // 8
    b = plane.astype(np.int64).reshape(bh, 8, bw, 8).transpose(0, 2, 1, 3).reshape(-1, 8, 8) - 128
    x = (_BASIS @ b @ _BASIS.T).reshape(-1, 64)                        # scaled by 2^28
    d = np.asarray(q, np.int64).reshape(64) << 28
    return np.sign(x) * ((2 * np.abs(x) + d) // (2 * d))


def _plane(rng, rows, cols):
    """part smooth, part noise, one saturated patch"""
    p = rng.integers(0, 256, (rows, cols))
    yy, xx = np.mgrid[:rows, :cols // 2]
    p[:, :cols // 2] = (yy * 5 + xx * 3 + int(rng.integers(0, 256))) % 256
    r, c = int(rng.integers(0, rows)), int(rng.integers(0, cols))
    p[r:r + 5, c:c + 6] = 255 * int(rng.integers(0, 2))
    return p


def _case(name, coef_q, width, height, sampling, quant, restart_interval=0):
    ncomp, dims, _ = jpeg_ref.geometry(width, height, sampling)
    quant = tuple(np.asarray(q, np.int64).reshape(64) for q in quant[:ncomp])
    coef_q = np.asarray(coef_q, np.int64)
    deq = coef_q * np.concatenate([np.broadcast_to(q, (bw * bh, 64)) for q, (bw, bh) in zip(quant, dims)])
    assert np.abs(deq).max() <= 32767, (name, int(np.abs(deq).max()))
    s = jpeg_ref.idct_unclamped(deq)
    assert SAMPLE_MIN <= s.min() and s.max() <= SAMPLE_MAX, (name, int(s.min()), int(s.max()))
    data = jpeg_write.write(coef_q, width, height, sampling, quant, restart_interval)
    return Case(name, data, deq.astype(np.int16), width, height, sampling, restart_interval, quant)


def _natural(rng, name, width, height, sampling, quant, restart_interval=0):
    dims = jpeg_ref.geometry(width, height, sampling)[1]
    coef_q = np.concatenate([_quantise(_plane(rng, bh * 8, bw * 8), q) for (bw, bh), q in zip(dims, quant)])
    return _case(name, coef_q, width, height, sampling, quant, restart_interval)


def _from_zigzag(zz):
    out = np.zeros_like(zz)
    out[:, jpeg_write.NATURAL] = zz
    return out


def _zigzag_set(rng, kind, blocks):
    """[blocks, 64] quantised, natural order.  Block i carries pattern k = i % 65: "single" one non-zero value at zigzag position
    k, "prefix" every position <= k non-zero (a run of k + 1 values); k = 64 is the all-zero block."""
    zz = np.zeros((blocks, 64), np.int64)
    for i in range(blocks):
        k = i % 65
        if k == 64:
            continue
        if kind == "single":
            zz[i, k] = int(rng.choice([-3, -2, -1, 1, 2, 3]))
        else:
            zz[i, :k + 1] = rng.choice([-1, 1], k + 1)
    return _from_zigzag(zz)


def _saturation_blocks(quant):
    """dequantised targets -> quantised (towards zero) by `quant`: flat levels -256 .. 511, the highest frequency at both signs
    around three levels, each row-only and column-only coefficient at both signs, whole first rows and columns"""
    d = []
    for level in range(-256, 512):
        d.append({0: (level - 128) * 8})
    for f in (1500, -1500):
        d.append({63: f})
    for level in (0, 255):
        for f in (900, -900):
            d.append({0: (level - 128) * 8, 63: f})
    for n in range(1, 8):
        for f in (1900, -1900):
            d.append({n: f})
            d.append({8 * n: f})
    for sign in (1, -1):
        d.append({n: sign * 250 * (-1) ** n for n in range(1, 8)})
        d.append({8 * n: sign * 250 * (-1) ** n for n in range(1, 8)})
    want = np.zeros((len(d), 64), np.int64)
    for b, e in enumerate(d):
        for n, v in e.items():
            want[b, n] = v
    return np.sign(want) * (np.abs(want) // np.asarray(quant, np.int64).reshape(64))


def _in_frame(blocks, bw, bh):
    out = np.zeros((bw * bh, 64), np.int64)
    out[:len(blocks)] = blocks
    return out


def colour_grid_levels():
    """[blocks, 3] flat (Y, Cb, Cr) levels: every Cb against the seven Cr of GRID_CR, then the transpose, each at three Y"""
    pairs = [(cb, cr) for cb in range(256) for cr in GRID_CR] + [(cb, cr) for cr in range(256) for cb in GRID_CR]
    return np.array([(y, cb, cr) for y in GRID_Y for cb, cr in pairs], np.int64)


@functools.lru_cache(maxsize=None)
def cases():
    rng = np.random.default_rng(20250117)
    out = []
    # geometry sweep: three distinct tables, luma 8- and 16-bit in turn
    for sampling in SAMPLINGS:
        for w in GEOMETRY_WIDTHS:
            for h in GEOMETRY_HEIGHTS:
                luma = LUMA16 if len(out) % 2 else LUMA8
                out.append(_natural(rng, "geo_%dx%d_%s" % (w, h, SAMPLING_NAME[sampling]), w, h, sampling, [luma, CB, CR]))
    for k, (w, h, sampling) in enumerate(WIDE):
        out.append(_natural(rng, "wide_%dx%d_%s" % (w, h, SAMPLING_NAME[sampling]), w, h, sampling, [LUMA16 if k % 2 else LUMA8, CB, CR]))
    # zigzag sets: tables of 64 distinct values, the 16-bit one with three entries above 255
    perm = [rng.permutation(64) + 1 for _ in range(3)]
    wide16 = np.where(perm[1] > 61, perm[1] + 200, perm[1])
    assert all(len(set(t.tolist())) == 64 for t in perm + [wide16]) and wide16.max() > 255
    for kind in ("single", "prefix"):
        out.append(_case("zigzag_%s_GRAY" % kind, _zigzag_set(rng, kind, 13 * 5), 100, 37, GRAY, [wide16]))
        coef_q = np.concatenate([_zigzag_set(rng, kind, n) for n in (26 * 10, 13 * 5, 13 * 5)])
        out.append(_case("zigzag_%s_420" % kind, coef_q, 203, 77, S420, [perm[0], wide16, perm[2]]))
    out.append(_case("zigzag_zero_GRAY", np.zeros((13 * 5, 64), np.int64), 100, 37, GRAY, [wide16]))
    out.append(_case("zigzag_zero_420", np.zeros((26 * 10 + 2 * 13 * 5, 64), np.int64), 203, 77, S420, [perm[0], wide16, perm[2]]))
    # saturation: 806 blocks in a plane of 32 x 26
    out.append(_case("saturation_GRAY", _in_frame(_saturation_blocks(SATURATION[0]), 32, 26), 253, 205, GRAY, SATURATION[:1]))
    out.append(_case("saturation_444", np.concatenate([_in_frame(_saturation_blocks(q), 32, 26) for q in SATURATION]), 253, 205, S444, SATURATION))
    # colour grid: flat DC-only blocks, 128 per row
    levels = colour_grid_levels()
    rows = len(levels) // GRID_BLOCKS_PER_ROW
    assert rows * GRID_BLOCKS_PER_ROW == len(levels)
    coef_q = np.zeros((3 * len(levels), 64), np.int64)
    coef_q[:, 0] = np.concatenate([(levels[:, c] - 128) * (8 // int(SATURATION[c][0])) for c in range(3)])
    grid = _case("colour_grid", coef_q, GRID_BLOCKS_PER_ROW * 8, rows * 8, S444, SATURATION)
    for c, p in enumerate(jpeg_ref.planes(grid.coef, grid.width, grid.height, S444)):       # the flat levels come out as intended
        assert np.array_equal(p, np.repeat(np.repeat(levels[:, c].reshape(rows, GRID_BLOCKS_PER_ROW), 8, 0), 8, 1)), c
    out.append(grid)
    # restarts: 20 MCUs; an interval of one wraps RST7 -> RST0 twice
    out.append(_natural(rng, "restart_1", 80, 64, S420, [LUMA8, CB, CR], restart_interval=1))
    out.append(_natural(rng, "restart_3", 77, 61, S420, [LUMA16, CB, CR], restart_interval=3))
    scan = out[-2].data[out[-2].data.index(b"\xff\xda"):]
    assert b"\xff\x00" in scan and scan.count(b"\xff\xd0") == 3 and scan.count(b"\xff\xd7") == 2, "restart_1: no stuffed byte, or not 19 restarts"
    assert len({c.name for c in out}) == len(out)
    return tuple(out)


def select(prefix):
    return [c for c in cases() if c.name.startswith(prefix)]


def expected_bgr(case):
    """the frame the library must produce: [H, W, 3] u8 BGR"""
    return jpeg_ref.to_bgr(jpeg_ref.decode(case.coef, case.width, case.height, case.sampling))
