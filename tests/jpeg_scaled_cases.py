"""Files for the reduced-size JPEG decode (rfd.h, "JPEG decode, reduced size"), written by tests/jpeg_write.py from chosen
coefficients and shared by tests/test_jpeg_scaled_cpu.py (Pillow's draft mode judges tests/jpeg_scaled_ref.py on them) and
tests/test_jpeg_scaled_gpu.py (the kernels against jpeg_scaled_ref).

The coefficients are sparse: a DC level and up to five AC values anywhere in the block, high frequencies included, so that
blocks differ in which of their values a reduced inverse DCT reads and where their runs end, and the pure-Python writer stays
quick.  jpeg_cases._case asserts the contract's range on every file: samples in [-384, 383] before the level shift, which takes
both clamps."""
import functools

import numpy as np

import jpeg_cases
import jpeg_ref
import jpeg_scaled_ref
from jpeg_cases import CB, CR, LUMA16, LUMA8, SAMPLING_NAME, SAMPLINGS
from jpeg_ref import GRAY, S420

DENOMS = (2, 4, 8)
BASE_DIMS = [1, 2, 7, 8, 9, 15, 16, 17, 31, 33]


def dims_of(s):
    """the widths and heights of the geometry sweep at denominator s: partial MCUs, odd block counts per row (plane pitches at
    n = 1 and 2 that are no multiple of 4), scaled sizes of 1 and 2 pixels, and the sizes around one and two scaled blocks"""
    return sorted(set(BASE_DIMS + [8 * s - 1, 8 * s, 8 * s + 1, 16 * s - 1, 16 * s + 1]))


def sizes_of(s):
    """every width of dims_of(s) with three of its heights, so that every height meets every third width"""
    d = dims_of(s)
    return [(w, d[(i + (len(d) // 3) * k) % len(d)]) for i, w in enumerate(d) for k in range(3)]


def sparse(rng, name, width, height, sampling, quant=(LUMA8, CB, CR), restart_interval=0):
    ncomp, dims, _ = jpeg_ref.geometry(width, height, sampling)
    parts = []
    for q, (bw, bh) in zip(quant, dims):
        q = np.asarray(q, np.int64).reshape(64)
        c = np.zeros((bw * bh, 64), np.int64)
        c[:, 0] = rng.integers(-1100, 1101, bw * bh) // q[0]
        for b in range(bw * bh):
            for pos in rng.integers(1, 64, int(rng.integers(0, 6))):
                c[b, pos] = int(rng.choice([-1, 1])) * int(rng.integers(1, max(1, min(3, 100 // q[pos])) + 1))
        parts.append(c)
    return jpeg_cases._case(name, np.concatenate(parts), width, height, sampling, list(quant), restart_interval)


@functools.lru_cache(maxsize=None)
def geometry():
    """{(width, height, sampling): Case} over the sizes of all three denominators"""
    rng = np.random.default_rng(20250923)
    out = {}
    for s in DENOMS:
        for w, h in sizes_of(s):
            for k, sampling in enumerate(SAMPLINGS):
                if (w, h, sampling) not in out:
                    out[w, h, sampling] = sparse(rng, "scaled_%dx%d_%s" % (w, h, SAMPLING_NAME[sampling]), w, h, sampling,
                                                 (LUMA16 if (w + k) % 2 else LUMA8, CB, CR))
    return out


@functools.lru_cache(maxsize=None)
def single_coefficient():
    """(grey Case of 8 x 8 blocks, 4:2:0 Case of 16 x 16 luma and 8 x 8 chroma blocks): block i of a plane carries a DC level and
    one more non-zero coefficient at natural position i % 64 (block 0: the DC alone)"""
    rng = np.random.default_rng(20250924)
    perm = np.asarray(rng.permutation(64) + 1, np.int64)              # 64 distinct quantisers: a value at the wrong position shows

    def plane(blocks):
        c = np.zeros((blocks, 64), np.int64)
        c[:, 0] = rng.integers(-12, 13, blocks)
        for b in range(blocks):
            if b % 64:
                c[b, b % 64] = int(rng.choice([-1, 1])) * max(1, 60 // int(perm[b % 64]))
        return c
    q = perm.copy()
    q[0] = 16
    grey = jpeg_cases._case("single_GRAY", plane(64), 64, 64, GRAY, [q])
    colour = jpeg_cases._case("single_420", np.concatenate([plane(256), plane(64), plane(64)]), 128, 128, S420, [q, q, q])
    return grey, colour


def expected_bgr(case, s):
    """the frame the library must produce at 1 / s: [ceil(H / s), ceil(W / s), 3] u8 BGR"""
    return jpeg_ref.to_bgr(jpeg_scaled_ref.decode_scaled(case.coef, case.width, case.height, case.sampling, s))
