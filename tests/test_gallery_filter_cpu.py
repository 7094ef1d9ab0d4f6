"""The gallery's tags and filtered search (include/rfd.h, "tags") without a GPU: the four entries are declared, exported and
bound; tests/gallery_filter_ref.py agrees with itself (its two forms, written differently) on seeded cases; the tags of the host
bookkeeping (csrc/gallery_book.h) against a one-word-per-row model, in a program of its own under AddressSanitizer and UBSan;
the four methods of include/rfd.hpp compile."""
import os
import re
import subprocess

import numpy as np
import pytest

import gallery_filter_ref as F
import gallery_identity_ref as I

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("rfd_gallery_set_tags", "rfd_gallery_get_tags", "rfd_gallery_search_filtered", "rfd_gallery_search_filtered_device")


def test_the_four_entries_are_declared_exported_and_bound(rfd):
    header = open(os.path.join(ROOT, "include", "rfd.h")).read()
    L = rfd.load_library()
    for name in SYMBOLS:
        assert re.search(r"RFD_API\s+int\s+%s\s*\(" % name, header), name
        assert name in rfd.API_SYMBOLS and hasattr(L, name), name
        assert getattr(L, name).argtypes is not None, name
    for method in ("set_tags", "tags", "search_filtered", "search_filtered_device"):
        assert callable(getattr(rfd.Gallery, method)), method


def _same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


def _cases():
    rng = np.random.default_rng(23)
    out = []
    for rows, m in ((1, 1), (5, 2), (40, 3), (97, 8), (97, 200)):
        s = rng.integers(-6, 7, (6, rows)).astype(np.float64) / 8                      # few levels: many ties
        ids = rng.integers(-1, m, rows)
        small = rng.integers(0, 4, rows)                                                # partitions 0..3
        wide = rng.integers(0, 4, rows) << 30 | rng.integers(0, 8, rows)                # a tenant in bits 31..30, lists in the low bits
        wide[::7] = 0xFFFFFFFF
        wide[3 % rows] = 0x80000000
        # per query: everything; partition 2; the tenant with bit 31; list bit 1 of tenant 3; value outside mask; no eligible row
        mask = np.array([0, F.ALL, 0xC0000000, 0xC0000002, 0x0000000F, F.ALL])
        value = np.array([0, 2, 0x80000000, 0xC0000002, 0x00000010, 0x12345678])
        out.append(("partitions", s, ids, small, mask, value))
        out.append(("tenant and lists", s, ids, wide, mask, value))
        out.append(("all one tag", s, ids, np.full(rows, 0xFFFFFFFF), np.array([F.ALL, 0x80000000, 1, 0, F.ALL, 2]),
                    np.array([F.ALL, 0x80000000, 1, 0, 0x7FFFFFFF, 3])))
        out.append(("all scores equal", np.full((6, rows), 0.375), np.arange(rows) % m, small, mask, value))
    return out


@pytest.mark.parametrize("k", [1, 5, 32])
def test_the_two_forms_agree(k):
    rng = np.random.default_rng(29)
    nothing = 0
    for name, s, ids, tags, mask, value in _cases():
        rows = s.shape[1]
        el = F.eligible(tags, mask, value)
        assert el.shape == (6, rows)
        assert all(el[q].all() for q in range(6) if mask[q] == 0 and value[q] == 0)    # mask = value = 0 matches every row
        for live in (None, rng.random(rows) < 0.6, np.zeros(rows, bool)):
            for min_score in (-np.inf, 0.25, 10.0):
                a = F.topk_of_scores(s, ids, tags, mask, value, k, min_score, live)
                b = F.brute_topk_of_scores(s, ids, tags, mask, value, k, min_score, live)
                assert _same(a, b), (name, rows, k, min_score)
                sc, r, i = a
                for q in range(len(s)):
                    got = r[q][r[q] >= 0]
                    assert np.all(el[q, got]) and (live is None or np.all(live[got])), (name, q)   # only live, eligible rows
                    assert np.all(r[q][len(got):] == -1) and np.all(np.isneginf(sc[q][len(got):])) and np.all(i[q][len(got):] == -1)
                    if not el[q].any():
                        nothing += 1
                        assert len(got) == 0
                # a value with bits outside its mask matches nothing
                outside = [q for q in range(len(s)) if int(value[q]) & ~int(mask[q]) & F.ALL]
                assert outside and all(np.all(r[q] == -1) for q in outside), name
    assert nothing > 0


def test_no_filter_is_the_identity_search_and_one_tag_is_a_sub_gallery():
    rng = np.random.default_rng(31)
    s = rng.integers(-6, 7, (4, 60)).astype(np.float64) / 8
    ids = rng.integers(-1, 9, 60)
    tags = rng.integers(0, 3, 60) | 0x80000000
    live = rng.random(60) < 0.8
    zero = np.zeros(4, np.int64)
    assert _same(F.topk_of_scores(s, ids, tags, zero, zero, 7, 0.1, live), I.topk_of_scores(s, ids, 7, 0.1, live))
    for t in (0x80000000, 0x80000001, 0x80000002):
        sub = np.flatnonzero(tags == t)
        a = F.topk_of_scores(s, ids, tags, zero + F.ALL, zero + t, 7, -np.inf, live)
        b = I.topk_of_scores(s[:, sub], ids[sub], 7, -np.inf, live[sub])
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[2], b[2])
        assert np.array_equal(a[1], np.where(b[1] >= 0, sub[np.maximum(b[1], 0)], -1))             # under the map between the row numbers


def test_the_tags_of_the_book_under_address_and_ub_sanitizers(tmp_path):
    """tests/cpp/gallery_tags_check.cpp: set, get, remove zeroing, replace keeping, clear and from_file; chunks of 1, 1 023, 1 024
    and 1 025 rows; refused lists (a removed row, a row twice, rows out of range) leaving the book unchanged; the slot contents;
    then seeded random sequences.  Built as tests/test_gallery_book_cpu.py builds its program; a plain build where the sanitizer
    runtimes cannot be linked."""
    exe = str(tmp_path / "gallery_tags_check")
    src = os.path.join(ROOT, "tests", "cpp", "gallery_tags_check.cpp")
    base = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", src, "-o", exe]
    san = subprocess.run(base + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan"], capture_output=True, text=True)
    if san.returncode != 0:
        plain = subprocess.run(base, capture_output=True, text=True)
        assert plain.returncode == 0, "the build failed:\n" + san.stderr + plain.stderr
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0 and " 0 failures" in run.stdout, run.stdout + run.stderr
    m = re.search(r"(\d+) steps, (\d+) checks, 0 failures", run.stdout)
    assert m and int(m.group(1)) > 1000 and int(m.group(2)) > 100000, run.stdout   # the program did run its cases


def test_the_cpp_methods_compile(tmp_path):
    src = tmp_path / "t.cpp"
    src.write_text('#include "rfd.hpp"\n'
                   "void use(rfd::Gallery &g, const float *dq, const uint32_t *dm, const uint32_t *dv, float *ds, int32_t *dr, int32_t *di)\n"
                   "{\n"
                   "    g.set_tags({0, 1}, {0x80000000u, 7u});\n"
                   "    std::vector<uint32_t> t = g.tags(0, 2);\n"
                   "    rfd::Gallery::IdentityMatches m = g.search_filtered(std::vector<float>(64), 5, {0xFFFFFFFFu, 0u}, {t[0], 0u}, 0.25f);\n"
                   "    g.search_filtered_device(dq, 2, m.k, 0.25f, dm, dv, ds, dr, di, true);\n"
                   "}\n"
                   "int main() { return 0; }\n")
    subprocess.check_call(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src)])
