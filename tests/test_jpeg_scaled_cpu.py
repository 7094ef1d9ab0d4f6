"""The reduced-size JPEG decode (include/rfd.h, "JPEG decode, reduced size") without a GPU: tests/jpeg_scaled_ref.py -- the numpy
restatement the GPU tests judge the kernels by -- against libjpeg-turbo through Pillow's draft mode byte for byte, the counts the
host entropy decoder writes at every denominator, rfd_jpeg_scaled_size, and the host half alone under AddressSanitizer and
UBSan as a program of its own."""
import ctypes as C
import glob
import io
import os
import subprocess

import numpy as np
import pytest

import jpeg_cases
import jpeg_ref
import jpeg_scaled_cases
import jpeg_scaled_ref
import jpeg_write
from jpeg_exif import app1, orient, tagged
from jpeg_ref import GRAY, S420, S422, S444
from jpeg_scaled_ref import decode_scaled, scaled_size

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "jpeg")
SUPPORTED = sorted(os.path.basename(f)[:-4] for f in glob.glob(os.path.join(GOLDEN, "*.npz")))


def load(name):
    with open(os.path.join(GOLDEN, name + ".jpg"), "rb") as f:
        return f.read()


def pillow(data, w, h, s):
    """what Pillow returns in draft mode at 1 / s; asserts that it took the scale"""
    Image = pytest.importorskip("PIL.Image")
    im = Image.open(io.BytesIO(data))
    if s != 1:
        im.draft(im.mode, (w // s, h // s))
    assert im.size == scaled_size(w, h, s), (im.size, w, h, s)
    return np.asarray(im)


def judge(rfd, data, s):
    """decode_scaled over the library's own coefficients against Pillow where Pillow can be steered to 1 / s (min(w, h) >= s);
    by the restatement alone elsewhere: its shape and that it runs"""
    i = rfd.jpeg_info(data)
    w, h = i["width"], i["height"]
    got = decode_scaled(rfd.jpeg_coefficients(data), w, h, i["sampling"], s)
    assert got.dtype == np.uint8 and got.shape[:2] == scaled_size(w, h, s)[::-1]
    if min(w, h) >= s:
        want = pillow(data, w, h, s)
        assert got.shape == want.shape and np.array_equal(got, want), (w, h, i["sampling"], s, int((got != want).sum()))
        return True
    return False


def test_the_component_sizes_are_the_table_of_the_header():
    table = {GRAY: ([4], [2], [1]), S444: ([4, 4, 4], [2, 2, 2], [1, 1, 1]), S422: ([4, 4, 4], [2, 2, 2], [1, 1, 1]),
             S420: ([4, 8, 8], [2, 4, 4], [1, 2, 2])}
    for sampling, rows in table.items():
        for s, ns in zip((2, 4, 8), rows):
            got, ups = jpeg_scaled_ref.idct_sizes(sampling, s)
            assert got == ns
            assert ups[1:] == ([(2, 1)] * 2 if sampling == S422 else [(1, 1)] * (len(ns) - 1)), (sampling, s, ups)
        assert jpeg_scaled_ref.idct_sizes(sampling, 1)[0] == [8] * len(rows[0])


@pytest.mark.parametrize("name", SUPPORTED)
def test_every_fixture_at_every_denominator_equals_pillow(rfd, name):
    data = load(name)
    w, h = (int(v) for v in name.split("_")[0].split("x"))
    judged = [s for s in (1, 2, 4, 8) if judge(rfd, data, s)]
    assert judged == [s for s in (1, 2, 4, 8) if min(w, h) >= s]          # no case Pillow can judge was left to the restatement


@pytest.mark.parametrize("s", [2, 4, 8])
def test_the_written_geometry_files_equal_pillow(rfd, s):
    """the files the GPU sweep decodes at this denominator: every sampling x the sizes of jpeg_scaled_cases.sizes_of"""
    cases = jpeg_scaled_cases.geometry()
    judged = 0
    for w, h in jpeg_scaled_cases.sizes_of(s):
        for sampling in jpeg_cases.SAMPLINGS:
            c = cases[w, h, sampling]
            assert np.array_equal(rfd.jpeg_coefficients(c.data), c.coef)
            judged += judge(rfd, c.data, s)
    assert judged == 4 * sum(min(w, h) >= s for w, h in jpeg_scaled_cases.sizes_of(s)) > 0


@pytest.mark.parametrize("sampling", [GRAY, S444, S422, S420])
def test_two_sweeps_of_sparse_coefficients_equal_pillow(rfd, sampling):
    """eight sizes from 8 x 8 to 64 x 48 x three quantiser sets x small values and values that take both clamps, at 1, 2, 4, 8"""
    rng = np.random.default_rng(100 + sampling)
    sizes = [(8, 8), (9, 15), (16, 16), (17, 33), (31, 24), (40, 47), (63, 9), (64, 48)]
    quants = [(jpeg_cases.LUMA8, jpeg_cases.CB, jpeg_cases.CR), (jpeg_cases.LUMA16, jpeg_cases.CR, jpeg_cases.CB), tuple(jpeg_cases.SATURATION)]
    for w, h in sizes:
        ncomp, dims, _ = jpeg_ref.geometry(w, h, sampling)
        for quant in quants:
            for big in (False, True):
                parts = []
                for q, (bw, bh) in zip(quant, dims):
                    q = np.asarray(q, np.int64).reshape(64)
                    c = np.zeros((bw * bh, 64), np.int64)
                    c[:, 0] = rng.integers(-1000, 1001, bw * bh) * (2 if big else 1) // q[0]
                    for b in range(bw * bh):
                        for pos in rng.integers(1, 64, int(rng.integers(0, 7))):
                            c[b, pos] = int(rng.integers(-3, 4)) * (max(1, 300 // int(q[pos])) if big else 1)
                    parts.append(c)
                data = jpeg_write.write(np.concatenate(parts), w, h, sampling, list(quant[:ncomp]))
                for s in (1, 2, 4, 8):
                    assert judge(rfd, data, s)


def _planes_by_block(case, s):
    """per component [blocks, n, n]: the scaled planes cut back into blocks"""
    _, dims, _ = jpeg_ref.geometry(case.width, case.height, case.sampling)
    ns, _ = jpeg_scaled_ref.idct_sizes(case.sampling, s)
    out = []
    for p, (bw, bh), n in zip(jpeg_scaled_ref.planes(case.coef, case.width, case.height, case.sampling, s), dims, ns):
        out.append(p.reshape(bh, n, bw, n).transpose(0, 2, 1, 3).reshape(bw * bh, n, n))
    return out, ns


@pytest.mark.parametrize("s", [1, 2, 4, 8])
def test_one_coefficient_at_each_of_the_64_positions(rfd, s):
    """grey gives n = 8, 4, 2, 1 over the four denominators, 4:2:0 adds the doubled chroma sizes.  Judge: Pillow; and a position
    outside the read set yields the pixels of the block's DC alone."""
    for case in jpeg_scaled_cases.single_coefficient():
        assert np.array_equal(rfd.jpeg_coefficients(case.data), case.coef)
        assert judge(rfd, case.data, s)
        dc_only = case._replace(coef=np.concatenate([case.coef[:, :1], np.zeros_like(case.coef[:, 1:])], 1))
        (with_ac, ns), (without, _) = _planes_by_block(case, s), _planes_by_block(dc_only, s)
        changed = 0
        for a, b, n in zip(with_ac, without, ns):
            for blk in range(a.shape[0]):
                if not jpeg_scaled_ref.reads(n, blk % 64):
                    assert np.array_equal(a[blk], b[blk]), (case.name, s, n, blk)
                else:
                    changed += int(not np.array_equal(a[blk], b[blk]))
        assert changed > 0 or all(n == 1 for n in ns)


def expected_counts(coef, sampling, width, height, s):
    """the count of every record from the dequantised coefficients: 1 + the zigzag position of the last non-zero coefficient the
    component's inverse DCT reads, 0 for a block without one (a dequantised value is zero exactly where the quantised one is)"""
    _, dims, _ = jpeg_ref.geometry(width, height, sampling)
    ns, _ = jpeg_scaled_ref.idct_sizes(sampling, s)
    out, at = [], 0
    for (bw, bh), n in zip(dims, ns):
        read = np.array([jpeg_scaled_ref.reads(n, nat) for nat in jpeg_write.NATURAL])       # by zigzag position
        zz = np.asarray(coef[at:at + bw * bh])[:, jpeg_write.NATURAL] != 0
        pos = np.where(zz & read[None, :], np.arange(1, 65)[None, :], 0)
        out.append(pos.max(1))
        at += bw * bh
    return np.concatenate(out).astype(np.uint8)


def test_the_block_counts_follow_the_read_set_rule(rfd):
    files = [(load(n), None) for n in SUPPORTED if n.startswith(("37x53", "64x48", "17x9"))]
    files += [(c.data, c) for c in jpeg_scaled_cases.single_coefficient()]
    files += [(c.data, c) for c in jpeg_cases.select("zigzag_")]
    shorter = 0
    for data, _ in files:
        i = rfd.jpeg_info(data)
        coef = rfd.jpeg_coefficients(data)
        full = rfd.jpeg_block_counts(data, 1)
        for s in (1, 2, 4, 8):
            got = rfd.jpeg_block_counts(data, s)
            assert got.dtype == np.uint8 and np.array_equal(got, expected_counts(coef, i["sampling"], i["width"], i["height"], s)), (i, s)
            shorter += int((got < full).sum())
        if i["sampling"] == S420:                                           # the chroma of 4:2:0 at 1/2 keeps the full-size rule
            luma = 4 * (len(full) // 6)
            assert np.array_equal(rfd.jpeg_block_counts(data, 2)[luma:], full[luma:])
    assert shorter > 1000
    # the capacity convention of rfd_debug_jpeg_coefficients, and the denominators
    L, data = rfd.load_library(), load("37x53_420")
    blocks = C.c_size_t()
    assert L.rfd_debug_jpeg_block_counts(data, len(data), 2, None, 0, C.byref(blocks)) == rfd.RFD_ERR_CAPACITY and blocks.value == 72
    assert L.rfd_debug_jpeg_block_counts(data, len(data), 2, None, 5, C.byref(blocks)) == rfd.RFD_ERR_INVALID_ARG
    for bad in (0, 3, 16, -1):
        buf = np.zeros(72, np.uint8)
        assert L.rfd_debug_jpeg_block_counts(data, len(data), bad, buf.ctypes.data, 72, C.byref(blocks)) == rfd.RFD_ERR_INVALID_ARG


def test_scaled_size_for_every_orientation_and_denominator(rfd):
    rng = np.random.default_rng(5)
    for w, h, sampling in ((37, 23, S420), (1, 9, GRAY), (65, 127, S422), (15, 15, S444)):
        plain = jpeg_scaled_cases.sparse(rng, "size_%dx%d" % (w, h), w, h, sampling).data
        for o in range(1, 9):
            data = tagged(plain, app1(value=o, entries=3, position=1))
            for s in (1, 2, 4, 8):
                sw, sh = scaled_size(w, h, s)
                want = dict(denom=s, stored_width=w, stored_height=h)
                assert rfd.jpeg_scaled_size(data, s, "ignore") == dict(want, width=sw, height=sh, orientation=1)
                ow, oh = (sh, sw) if o >= 5 else (sw, sh)
                assert rfd.jpeg_scaled_size(data, s, "apply") == dict(want, width=ow, height=oh, orientation=o)
                assert orient(np.zeros((sh, sw, 3), np.uint8), o).shape == (oh, ow, 3)
        assert rfd.jpeg_scaled_size(plain, 4, "apply")["orientation"] == 1


def test_scaled_size_refuses_what_info_refuses_and_leaves_the_struct_alone(rfd):
    import test_jpeg_cpu as base
    L = rfd.load_library()
    z = rfd.rfd_jpeg_scaled_size()
    assert C.sizeof(z) == 32
    for name, data, _ in base.unsupported_cases() + base.malformed_cases():
        buf = np.frombuffer(data, np.uint8)
        addr = buf.ctypes.data if buf.size else None
        info = rfd.rfd_jpeg_info()
        st = L.rfd_jpeg_info(addr, buf.size, C.byref(info))
        msg = L.rfd_last_error().decode() if st else ""
        for s in (1, 2, 4, 8):
            C.memset(C.byref(z), 0x5a, C.sizeof(z))
            assert L.rfd_jpeg_scaled_size(addr, buf.size, s, rfd.JPEG_ORIENTATION_APPLY, C.byref(z)) == st, (name, s)
            if st:
                assert L.rfd_last_error().decode() == msg and bytes(z) == b"\x5a" * 32, name
            else:                                                           # the entropy data is the decode's business
                assert z.denom == s and list(z.reserved) == [0, 0]
    data = load("37x53_420")
    for bad in (0, 3, 16, -1):
        C.memset(C.byref(z), 0x5a, C.sizeof(z))
        assert L.rfd_jpeg_scaled_size(data, len(data), bad, 0, C.byref(z)) == rfd.RFD_ERR_INVALID_ARG and bytes(z) == b"\x5a" * 32
        with pytest.raises(rfd.RfdError):
            rfd.jpeg_scaled_size(data, bad)
    assert L.rfd_jpeg_scaled_size(data, len(data), 2, 2, C.byref(z)) == rfd.RFD_ERR_INVALID_ARG
    C.memset(C.byref(z), 0x5a, C.sizeof(z))
    assert L.rfd_jpeg_scaled_size(data, len(data), 8, 0, C.byref(z)) == 0
    assert (z.denom, z.width, z.height, z.stored_width, z.stored_height, z.orientation, list(z.reserved)) == (8, 5, 7, 37, 53, 1, [0, 0])


def test_the_symbols_are_part_of_the_interface(rfd):
    txt = open(os.path.join(ROOT, "include", "rfd.h")).read()
    for name in ("rfd_set_jpeg_scale", "rfd_jpeg_scaled_size", "rfd_debug_jpeg_block_counts"):
        assert name in rfd.API_SYMBOLS and hasattr(rfd.load_library(), name) and ("RFD_API int %s(" % name) in txt
    assert "JPEG decode, reduced size" in txt


def test_the_scaled_host_decoder_alone_under_address_and_ub_sanitizers(tmp_path):
    """tests/cpp/jpeg_scaled_check.cpp: at every denominator, valid files cut at every byte and with every one of their first 700
    bytes replaced by 0x00 and 0xFF, through the parser and the entropy decoder told each component's inverse-DCT size, in a
    program of its own whose every out-of-bounds access or undefined operation aborts it.  Built as tests/test_jpeg_cpu.py
    builds its program; a plain build where the sanitizer runtimes cannot be linked."""
    exe = str(tmp_path / "jpeg_scaled_check")
    src = os.path.join(ROOT, "tests", "cpp", "jpeg_scaled_check.cpp")
    base = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", src, "-o", exe]
    san = subprocess.run(base + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan"], capture_output=True, text=True)
    if san.returncode != 0:
        plain = subprocess.run(base, capture_output=True, text=True)
        assert plain.returncode == 0, "the build failed:\n" + san.stderr + plain.stderr
    files = [os.path.join(GOLDEN, n + ".jpg") for n in ("37x53_420", "37x53_420_rst2", "37x53_GRAY", "37x53_422")]
    run = subprocess.run([exe] + files, capture_output=True, text=True)
    assert run.returncode == 0 and " 0 failures" in run.stdout, run.stdout + run.stderr


def test_the_planning_of_a_decode_call_alone_under_address_and_ub_sanitizers(tmp_path):
    """tests/cpp/jpeg_plan_check.cpp: the layout of the staging, the per-file argument check and the descriptor tables of the
    launches (csrc/jpeg_plan.h) on files of 1 x 1 to 130 x 70 in every sampling and with the orientation tags 1, 3, 6 and 8,
    planned alone, in pairs and all together, in a program of its own whose every out-of-bounds access or undefined operation
    aborts it.  Built as the program above; a plain build where the sanitizer runtimes cannot be linked."""
    exe = str(tmp_path / "jpeg_plan_check")
    src = os.path.join(ROOT, "tests", "cpp", "jpeg_plan_check.cpp")
    base = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", src, "-o", exe]
    san = subprocess.run(base + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan"], capture_output=True, text=True)
    if san.returncode != 0:
        plain = subprocess.run(base, capture_output=True, text=True)
        assert plain.returncode == 0, "the build failed:\n" + san.stderr + plain.stderr
    rng = np.random.default_rng(7)
    files = []
    for w, h in ((1, 1), (8, 8), (9, 17), (64, 64), (65, 63), (130, 70)):
        for sampling in (GRAY, S444, S422, S420):
            plain = jpeg_scaled_cases.sparse(rng, "plan_%dx%d" % (w, h), w, h, sampling).data
            for o in (1, 3, 6, 8):
                files.append(str(tmp_path / ("%dx%d_%d_%d.jpg" % (w, h, sampling, o))))
                with open(files[-1], "wb") as f:
                    f.write(tagged(plain, app1(value=o)))
    run = subprocess.run([exe] + files, capture_output=True, text=True)
    assert run.returncode == 0 and "96 files" in run.stdout and " 0 failures" in run.stdout, run.stdout[-3000:] + run.stderr[-3000:]
