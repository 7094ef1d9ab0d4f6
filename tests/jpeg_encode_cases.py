"""The cases the JPEG encode tests share (tests/test_jpeg_encode_cpu.py, tests/test_jpeg_encode_gpu.py): the geometries, settings
and contents of the sweep, with the restatement's file of each computed once, and the constructed coefficients of the entropy
stage's tests."""
import functools

import numpy as np

import jpeg_encode_ref as R
import jpeg_ref
import jpeg_write

# H x W.  8x8, 8x16, 24x24 and 40x8 at 4:2:0 separate the two bottom-edge rules: H is a multiple of 8 with an odd number of luma
# block rows, so the chroma rows 4 .. 7 of the last block row repeat row 3 and are not the mean of a repeated input row.
GEOMETRIES = [(1, 1), (7, 7), (8, 8), (8, 16), (16, 8), (9, 17), (24, 24), (17, 33), (37, 53), (40, 8), (112, 112)]
SAMPLINGS = [R.GRAY, R.S444, R.S422, R.S420]
QUALITIES = [1, 50, 75, 90, 100]
RESTARTS = [0, 1, 2]
CONTENTS = ["noise", "ramp", "saturated"]
SAMPLING_NAMES = {R.GRAY: "gray", R.S444: "444", R.S422: "422", R.S420: "420"}


@functools.lru_cache(maxsize=None)
def image(h, w, content, seed=0):
    """[h, w, 3] u8 BGR"""
    rng = np.random.default_rng(1000 * h + w + 7919 * seed + CONTENTS.index(content))
    if content == "noise":
        img = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    elif content == "ramp":
        yy, xx = np.mgrid[0:h, 0:w]
        img = np.stack([(xx * 3 + yy) % 256, (yy * 5 + 17) % 256, (xx + yy * 2 + 90) % 256], -1).astype(np.uint8)
    else:
        img = (rng.integers(0, 2, (h, w, 3)) * 255).astype(np.uint8)
    img.setflags(write=False)
    return img


@functools.lru_cache(maxsize=None)
def expected(h, w, content, quality, sampling, restart_rows, seed=0):
    """the restatement's file of image(h, w, content, seed)"""
    return R.encode(image(h, w, content, seed), quality, sampling, restart_rows)


def sweep(sampling, restart_rows):
    """the (h, w, content, quality) of one sampling and restart setting"""
    return [(h, w, c, q) for (h, w) in GEOMETRIES for c in CONTENTS for q in QUALITIES]


# ---- constructed coefficients for the entropy stage (zigzag order here; natural() turns them round) ----
def natural(zz):
    """[blocks, 64] zigzag order -> natural order, what the library's hooks and jpeg_write.write take"""
    out = np.zeros_like(zz)
    out[:, jpeg_write.NATURAL] = zz
    return out


def block_bits(zz, table=0):
    """one block alone in an interval -> (its bits as an int, their number): the test-side writer's own coder"""
    b = jpeg_write._Bits()
    jpeg_write._block(b, [int(v) for v in zz], 0, jpeg_write._CODE[0, table], jpeg_write._CODE[1, table])
    return b.acc, b.n


def interval_bytes(zz, table=0):
    """-> (the unstuffed bytes of the block's interval, padded; the number of bits before the padding)"""
    acc, n = block_bits(zz, table)
    pad = -n % 8
    acc, m = (acc << pad) | ((1 << pad) - 1), n + pad
    return acc.to_bytes(m // 8, "big"), n


def lone_coefficients():
    """GRAY 512 x 8: 64 blocks in one MCU row, block k with a coefficient at zigzag position k alone"""
    zz = np.zeros((64, 64), np.int16)
    for k in range(64):
        zz[k, k] = [5, -3, 1, -1, 255, -256, 1023, -1023][k % 8]
    return zz, 512, 8, R.GRAY


def zero_runs():
    """GRAY 48 x 8: a DC, then zero runs of 15, 16, 17, 32 and 62 in front of one coefficient (62: position 63, no EOB), then
    DC differences of -2047 and +2047 with AC of -1023 and +1023"""
    zz = np.zeros((6, 64), np.int16)
    for b, run in enumerate([15, 16, 17, 32, 62]):
        zz[b, 0] = 10 * b
        zz[b, run + 1] = [-1, 2, -7, 100, 1023][b]
    zz[4, 0] = 1023
    zz[5, 0], zz[5, 1], zz[5, 2] = -1024, -1023, 1023
    zz = np.concatenate([zz, zz[4:5]])                   # -1024 -> 1023: +2047
    return zz, 56, 8, R.GRAY


@functools.lru_cache(maxsize=None)
def ff_blocks():
    """Blocks found by a seeded search, each alone in its interval, by what their bits do: `middle`: an FF byte that is not the
    interval's last; `last_data`: the bits are a multiple of 8 and the last byte is FF; `pad`: the bits are no multiple of 8 and
    the padded last byte is FF; `exact`: the bits are a multiple of 8 and the last byte is not FF."""
    rng = np.random.default_rng(424242)
    want, found = ["middle", "last_data", "pad", "exact"], {}
    for _ in range(200000):
        zz = np.zeros(64, np.int16)
        zz[0] = rng.integers(-1024, 1024)
        for pos in rng.choice(np.arange(1, 64), size=rng.integers(0, 6), replace=False):
            s = int(rng.integers(1, 11))
            zz[pos] = ((1 << s) - 1) * (1 if rng.integers(0, 2) else -1) if rng.integers(0, 2) else rng.integers(-1023, 1024)
        if rng.integers(0, 2):
            zz[63] = (1 << int(rng.integers(1, 11))) - 1
        data, n = interval_bytes(zz)
        kinds = []
        if 0xff in data[:-1]:
            kinds.append("middle")
        if n % 8 == 0:
            kinds.append("last_data" if data[-1] == 0xff else "exact")
        elif data[-1] == 0xff:
            kinds.append("pad")
        for k in kinds:
            found.setdefault(k, zz.copy())
        if len(found) == len(want):
            break
    assert sorted(found) == sorted(want), sorted(found)
    return found


def single_mcu_intervals():
    """GRAY 8 x 96 with one restart row: 12 intervals of a single MCU (the RST index wraps), the ff_blocks among them"""
    f = ff_blocks()
    zz = np.zeros((12, 64), np.int16)
    for i, k in enumerate(["middle", "last_data", "pad", "exact"]):
        zz[2 * i + 1] = f[k]
        zz[2 * i + 8 if 2 * i + 8 < 12 else 2 * i] = f[k]
    zz[0, 0], zz[11, 0] = -5, 77
    return zz, 8, 96, R.GRAY


def colour_blocks(width, height, sampling, seed):
    """random coefficients of a colour file in the library's block order, sparse like real ones, natural order"""
    rng = np.random.default_rng(seed)
    n = jpeg_ref.num_blocks(width, height, sampling)
    zz = np.zeros((n, 64), np.int16)
    zz[:, 0] = rng.integers(-1024, 1024, n)
    for b in range(n):
        for pos in rng.choice(np.arange(1, 64), size=rng.integers(0, 9), replace=False):
            zz[b, pos] = rng.integers(-1023, 1024)
    return natural(zz)
