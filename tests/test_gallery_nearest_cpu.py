"""The gallery's self-join (include/rfd.h, "nearest") without a GPU: the three entries and the plan entry are declared, exported
and bound; the configuration's layout and defaults; tests/gallery_nearest_ref.py agrees with itself (its two forms, written
differently) on seeded cases with ties, removed rows, both modes and masks; the plan (csrc/gallery_nearest_plan.h) alone in a
program of its own under AddressSanitizer and UBSan, and through the exported entry; the methods of include/rfd.hpp compile."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import gallery_nearest_ref as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("rfd_gallery_nearest_config_default", "rfd_gallery_nearest", "rfd_gallery_nearest_device", "rfd_debug_gallery_nearest_plan")


def test_the_entries_are_declared_exported_and_bound(rfd):
    header = open(os.path.join(ROOT, "include", "rfd.h")).read()
    L = rfd.load_library()
    for name in SYMBOLS:
        assert re.search(r"RFD_API\s+(int|void)\s+%s\s*\(" % name, header), name
        assert name in rfd.API_SYMBOLS and hasattr(L, name), name
        assert getattr(L, name).argtypes is not None, name
    for method in ("nearest", "nearest_device"):
        assert callable(getattr(rfd.Gallery, method)), method
    assert "do NOT ENUMERATE all pairs" in header        # what k = 1 gives is said plainly
    assert re.search(r"#define\s+RFD_GALLERY_NEAREST_OTHER_ROW\s+0\b", header) and re.search(r"#define\s+RFD_GALLERY_NEAREST_OTHER_IDENTITY\s+1\b", header)
    assert (rfd.NEAREST_OTHER_ROW, rfd.NEAREST_OTHER_IDENTITY) == (0, 1) == (N.OTHER_ROW, N.OTHER_IDENTITY)


def test_the_configuration_is_32_bytes_with_the_documented_defaults(rfd):
    cfg = rfd.rfd_gallery_nearest_config
    assert C.sizeof(cfg) == 32
    assert (cfg.mode.offset, cfg.min_score.offset, cfg.tag_mask.offset, cfg.reserved.offset) == (0, 4, 8, 12)
    c = cfg(7, 1.0, 9, (C.c_int32 * 5)(1, 2, 3, 4, 5))
    rfd.load_library().rfd_gallery_nearest_config_default(C.byref(c))
    assert c.mode == rfd.NEAREST_OTHER_ROW and c.min_score == float("-inf") and c.tag_mask == 0 and list(c.reserved) == [0] * 5
    rfd.load_library().rfd_gallery_nearest_config_default(None)   # a null pointer is ignored
    # without a gallery both calls refuse before they look at anything else
    out = np.full(4, 7, np.int32)
    L = rfd.load_library()
    assert L.rfd_gallery_nearest(None, 0, 1, None, out.ctypes.data, out.ctypes.data, None) == rfd.RFD_ERR_INVALID_ARG
    assert L.rfd_gallery_nearest_device(None, 0, 1, None, out.ctypes.data, out.ctypes.data, None, 0) == rfd.RFD_ERR_INVALID_ARG
    assert np.all(out == 7)


def _same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


def _cases():
    rng = np.random.default_rng(41)
    out = []
    for rows, m in ((1, 1), (2, 1), (5, 2), (40, 3), (97, 8), (97, 200)):
        half = rng.integers(-6, 7, (rows, rows)).astype(np.float64) / 8          # few levels: many ties
        s = np.triu(half) + np.triu(half, 1).T                                   # score(a, b) == score(b, a)
        ids = rng.integers(-1, m, rows)
        tags = rng.integers(0, 4, rows) << 30 | rng.integers(0, 4, rows)
        out.append(("ties", s, ids, tags))
        out.append(("all equal", np.full((rows, rows), 0.375), np.arange(rows) % m, tags))
        out.append(("one identity", s, np.zeros(rows, np.int64), tags))
        t = s.copy()
        t[rng.random((rows, rows)) < 0.2] = np.nan
        t[rng.random((rows, rows)) < 0.2] = -np.inf
        out.append(("nan and -inf", t, ids, tags))
    return out


@pytest.mark.parametrize("mode", [N.OTHER_ROW, N.OTHER_IDENTITY])
def test_the_two_forms_agree(mode):
    rng = np.random.default_rng(43)
    empty = found = 0
    for name, s, ids, tags in _cases():
        rows = s.shape[0]
        for live in (None, rng.random(rows) < 0.6, np.zeros(rows, bool)):
            for tag_mask in (0, N.ALL, 0xC0000000, 1):
                for min_score in (-np.inf, 0.25, 0.375, np.nextafter(0.375, 1), np.inf):
                    kw = dict(mode=mode, min_score=min_score, tag_mask=tag_mask, ids=ids, tags=tags, live=live)
                    a, b = N.nearest_of_scores(s, **kw), N.naive_nearest_of_scores(s, **kw)
                    assert _same(a, b), (name, rows, tag_mask, min_score)
                    sc, r, i = a
                    got = r >= 0
                    found += int(got.sum())
                    empty += int((~got).sum())
                    assert np.all(np.isneginf(sc[~got])) and np.all(i[~got] == -1)
                    assert np.all(r[got] != np.flatnonzero(got)) and np.all(sc[got] >= min_score)        # never the row itself
                    if live is not None:
                        assert np.all(live[r[got]]) and not got[~live].any()                             # only live rows, on both sides
                    if mode == N.OTHER_IDENTITY:
                        assert not np.any((ids[got] >= 0) & (ids[r[got]] == ids[got]))
                    assert np.all(((tags[got] ^ tags[r[got]]) & tag_mask) == 0)
                    if rows == 1 or min_score == np.inf or (name == "one identity" and mode == N.OTHER_IDENTITY):
                        assert not got.any(), name
                    # a range is a slice of the whole
                    if rows >= 5:
                        part = N.nearest_of_scores(s, row0=2, n=rows - 3, **kw)
                        assert _same(part, [x[2:rows - 1] for x in a])
    assert empty > 0 and found > 0


def test_equal_scores_resolve_to_the_lower_row_and_links_are_symmetric_in_bits():
    s = np.full((6, 6), 0.5)
    sc, r, _ = N.nearest_of_scores(s)
    assert list(r) == [1, 0, 0, 0, 0, 0] and np.all(sc == 0.5)
    sc, r, _ = N.nearest_of_scores(s, live=np.array([0, 1, 1, 0, 1, 1], bool))
    assert list(r) == [-1, 2, 1, -1, 1, 1]


def test_the_plan_alone_under_address_and_ub_sanitizers(tmp_path):
    """tests/cpp/gallery_nearest_plan_check.cpp: rows and n of 0, 1, 15 .. 17 and the tile +- 1 and more, every start, dims 32,
    512 and 1024, 1, 8 and 256 CUs; tiles and splits counted into arrays.  Built as tests/test_gallery_book_cpu.py builds its
    program; a plain build where the sanitizer runtimes cannot be linked."""
    exe = str(tmp_path / "gallery_nearest_plan_check")
    src = os.path.join(ROOT, "tests", "cpp", "gallery_nearest_plan_check.cpp")
    base = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", src, "-o", exe]
    san = subprocess.run(base + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan"], capture_output=True, text=True)
    if san.returncode != 0:
        plain = subprocess.run(base, capture_output=True, text=True)
        assert plain.returncode == 0, "the build failed:\n" + san.stderr + plain.stderr
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0 and " 0 failures" in run.stdout, run.stdout + run.stderr
    m = re.search(r"(\d+) steps, (\d+) checks, 0 failures", run.stdout)
    assert m and int(m.group(1)) > 1000 and int(m.group(2)) > 10000, run.stdout   # the program did run its cases


def test_the_plan_is_plain_host_code():
    text = open(os.path.join(ROOT, "rs-face-detection_amd", "csrc", "gallery_nearest_plan.h")).read()
    includes = re.findall(r'#include\s+[<"]([^>"]+)[>"]', text)
    assert includes and not [i for i in includes if "hip" in i.lower() or i in ("rfd_common.h", "kernels.h", "host_resources.h")], includes


def test_the_exported_plan_entry(rfd):
    """the entry needs no context and no device; it states the two regimes and refuses what the gallery refuses"""
    few = rfd.gallery_nearest_plan(1 << 20, 0, 32, 512, 256)
    assert few["tile_rows"] % 16 == 0 and few["tiles"] == 1 and few["grid"] >= 256                                 # 32 new rows fill the chip
    assert few["ws_bytes"] == few["splits"] * 32 * 8 and few["splits"] * few["blocks_per_split"] >= few["blocks"] == 1 << 16
    many = rfd.gallery_nearest_plan(1 << 20, 0, 1 << 20, 512, 256)
    assert many["splits"] == 1 and many["tiles"] * many["tile_rows"] == 1 << 20                                    # a sweep reads the gallery once per tile
    assert many["form"] == 1 and many["tile_rows"] > few["tile_rows"]                                              # dim 512: the register form, once a call has rows for it
    other = rfd.gallery_nearest_plan(3000, 5, 2900, 64, 256)
    assert other["form"] == 0 and other["grid"] == other["tiles"] * other["splits"] <= -(-2900 // other["tile_rows"]) + 4 * 256
    assert rfd.gallery_nearest_plan(10, 3, 0, 512, 8)["grid"] == 0                                                 # n = 0: nothing to launch
    L, p = rfd.load_library(), rfd.rfd_gallery_nearest_plan()
    for bad in ((10, 0, 11, 512, 8), (10, -1, 2, 512, 8), (10, 9, 2, 512, 8), (10, 0, -1, 512, 8), (10, 0, 5, 48, 8), (10, 0, 5, 2048, 8), (10, 0, 5, 512, 0)):
        p.grid = 7
        assert L.rfd_debug_gallery_nearest_plan(*bad, C.byref(p)) == rfd.RFD_ERR_INVALID_ARG and p.grid == 0, bad
    assert L.rfd_debug_gallery_nearest_plan(10, 0, 5, 512, 8, None) == rfd.RFD_ERR_INVALID_ARG


def test_the_cpp_methods_compile(tmp_path):
    src = tmp_path / "t.cpp"
    src.write_text('#include "rfd.hpp"\n'
                   "void use(rfd::Gallery &g, float *ds, int32_t *dr, int32_t *di)\n"
                   "{\n"
                   "    rfd::Gallery::Nearest all = g.nearest(0, g.size());\n"
                   "    rfd_gallery_nearest_config cfg = rfd::Gallery::nearest_config(RFD_GALLERY_NEAREST_OTHER_IDENTITY, 0.5f, 0xC0000000u);\n"
                   "    rfd::Gallery::Nearest some = g.nearest(3, 2, cfg);\n"
                   "    g.nearest_device(0, (int)all.rows.size() + (int)some.ids.size(), cfg, ds, dr, di, true);\n"
                   "    static_assert(sizeof(rfd_gallery_nearest_config) == 32, \"\");\n"
                   "}\n"
                   "int main() { return 0; }\n")
    subprocess.check_call(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src)])
