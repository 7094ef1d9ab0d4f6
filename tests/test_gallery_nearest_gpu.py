"""The gallery's self-join (include/rfd.h, "nearest"; csrc/kernels_gallery_nearest.hip) through the C ABI, against
tests/gallery_nearest_ref.py.  The data are dyadic (values m / 64, |m| <= 8), so every score is exact in f32 in any summation
order (asserted on the CPU first) and every comparison is bit for bit.  Tile sizes come from rfd_debug_gallery_nearest_plan,
never from a number written here.  A case computes its score matrix once and shares it among its checks."""
import ctypes as C

import numpy as np
import pytest

import gallery_nearest_ref as N
import gallery_ref as R
from test_gallery_gpu import _bits, _dyadic_case, _units, det  # noqa: F401  (det: the module's detector fixture)
from test_gallery_edit_gpu import EditGal, gal  # noqa: F401  (gal: makes EditGal galleries)
from test_gallery_identity_gpu import _cus, _exact, _search_ids, _set_ids
from test_gallery_filter_gpu import _search as _search_filtered, _set_tags

pytestmark = pytest.mark.gpu

NEG_INF = float("-inf")
ALL = N.ALL


def _plan(rfd, rows, row0, n, dim):
    return rfd.gallery_nearest_plan(rows, row0, n, dim, _cus())


def _tiles(rfd, dim):
    """the tile sizes of the forms that run this dim: of a call of one row, and of a large one"""
    return sorted({_plan(rfd, 1, 0, 1, dim)["tile_rows"], _plan(rfd, 4096, 0, 4096, dim)["tile_rows"]})


def _nearest(ga, row0, n, mode=N.OTHER_ROW, min_score=NEG_INF, tag_mask=0, with_ids=True):
    """the host form; outputs pre-filled so that an unwritten word shows"""
    s, r, i = np.full(max(n, 1), 7.0, np.float32), np.full(max(n, 1), -7, np.int32), np.full(max(n, 1), -7, np.int32)
    cfg = ga.rfd.rfd_gallery_nearest_config(mode, min_score, tag_mask & ALL)
    st = ga.L.rfd_gallery_nearest(ga.g, row0, n, C.byref(cfg), s.ctypes.data, r.ctypes.data, i.ctypes.data if with_ids else None)
    return st, s[:n], r[:n], i[:n]


def _self_scores(g):
    full = R.scores(g, g)
    _exact(full)
    full.setflags(write=False)
    return full


def _check(ga, full, row0, n, tag, **kw):
    """nearest of rows [row0, row0 + n) equals the reference on the score matrix `full`, bit for bit"""
    ref = N.nearest_of_scores(full, row0, n, **kw)
    st, s, r, i = _nearest(ga, row0, n, kw.get("mode", N.OTHER_ROW), kw.get("min_score", NEG_INF), kw.get("tag_mask", 0))
    assert st == 0, (tag, ga.err())
    assert np.array_equal(r, ref[1]), tag
    assert np.array_equal(i, ref[2]), tag
    assert np.array_equal(_bits(s), _bits(ref[0])), tag
    return s, r, i


def _filled(gal, g, extra=3):
    ga = gal(g.shape[1], len(g) + extra)
    assert ga.status == 0 and ga.add(g) == (0, 0)
    return ga


# ---- 1. geometry ----
@pytest.mark.parametrize("dim", [32, 64, 512, 1024])
def test_geometry_sweep(rfd, gal, dim):
    """K-step counts 1, 2, 16 and 32; galleries of one row, one partial block, one block and a row, a tile less a row, a tile, a
    tile and a row; the whole gallery, single rows, and ranges that start at no block and no tile"""
    tiles = _tiles(rfd, dim)
    T = tiles[-1]
    assert all(t % 16 == 0 for t in tiles) and (_plan(rfd, 4096, 0, 4096, dim)["form"] == 1) == (dim == 512)
    # where the plan changes the form with the rows of a call (dim 512), the sizes on both sides of that step
    step = [n for n in range(1, 130) if _plan(rfd, 4096, 0, n, dim)["form"] != _plan(rfd, 4096, 0, n + 1, dim)["form"]]
    sizes = {1, 2, 15, 16, 17, 33, 2 * T + 5}
    for t in tiles + step:
        sizes |= {t - 1, t, t + 1, t + 2}
    for rows in sorted(sizes - {0}):
        _, g, _ = _dyadic_case(dim, rows, 2, 8000 + dim + rows)
        full = _self_scores(g)
        ga = _filled(gal, g)
        s, r, i = _check(ga, full, 0, rows, (dim, rows, "all"))
        assert np.all(i == -1)
        if rows == 1:
            assert r[0] == -1 and np.isneginf(s[0])                      # a gallery of one row: the empty entry
        else:
            assert np.all(r >= 0) and np.all(r != np.arange(rows))
        for a in sorted({0, rows // 2, rows - 1}):
            _check(ga, full, a, 1, (dim, rows, a, 1))
        for row0, n in ((1, rows - 1), (3, rows - 5), (17, rows - 18), (T + 1, rows - T - 2), (T - 3, 7)):
            if row0 >= 0 and n >= 1 and row0 + n <= rows:
                assert row0 % 16 != 0 and all(row0 % t != 0 for t in tiles)
                _check(ga, full, row0, n, (dim, rows, row0, n))
        ga.close()


@pytest.mark.parametrize("dim", [32, 64, 512, 1024])
def test_several_tiles_and_several_splits_at_once(rfd, gal, dim):
    rows = 3001
    p = _plan(rfd, rows, 0, rows, dim)
    assert p["tiles"] > 1 and p["splits"] > 1
    _, g, planted = _dyadic_case(dim, rows, 2, 8100 + dim)
    full = _self_scores(g)
    ga = _filled(gal, g)
    s, r, _ = _check(ga, full, 0, rows, (dim, "all"))
    assert len(planted) >= 5 and r[planted[0]] == planted[1] and all(r[q] == planted[0] for q in planted[1:])   # duplicates: the lower row wins
    few = _plan(rfd, rows, 1234, 5, dim)
    assert few["tiles"] == 1 and few["splits"] > 1                        # few rows: split over the gallery and merged
    _check(ga, full, 1234, 5, (dim, "few"))
    _check(ga, full, rows - 1, 1, (dim, "last"))


# ---- 2. order ----
@pytest.mark.parametrize("dim", [64, 512])
def test_equal_rows_and_twins_in_other_tiles_and_splits(rfd, gal, dim):
    rows = 3000
    p = _plan(rfd, rows, 0, rows, dim)
    T, splits = p["tile_rows"], p["splits"]
    assert splits >= 3
    rng = np.random.default_rng(8200 + dim)
    g = rng.integers(-4, 5, (rows, dim)).astype(np.float64) / 64
    twin = np.where(rng.random(dim) < 0.5, -8, 8) / 64                     # no other row reaches its self-score
    split_of = lambda row: row // 64 % splits                              # groups of four blocks, dealt round-robin
    a, b = 5, 64 + T + 7
    c = next(row for row in range(rows - 9, 0, -1) if len({split_of(a), split_of(b), split_of(row)}) == 3)
    assert len({a // T, b // T, c // T}) == 3 and c > rows - 64 * splits    # three tiles, three splits
    g[a] = g[b] = g[c] = twin
    full = _self_scores(g)
    ga = _filled(gal, g)
    s, r, _ = _check(ga, full, 0, rows, (dim, "twins"))
    assert (r[a], r[b], r[c]) == (b, a, a) and _bits(s[a]) == _bits(s[b]) == _bits(s[c])
    ga.close()
    same = np.tile(twin, (2 * T + 3, 1))                                    # rows that are all equal
    ga = _filled(gal, same)
    s, r, _ = _check(ga, _self_scores(same), 0, len(same), (dim, "equal"))
    assert r[0] == 1 and np.all(r[1:] == 0) and len(set(_bits(s).tolist())) == 1


# ---- 3. eligibility ----
def _case(dim, rows, seed):
    _, g, planted = _dyadic_case(dim, rows, 2, seed)
    return g, planted, _self_scores(g)


@pytest.mark.parametrize("dim", [64, 512])
def test_removed_rows_on_both_sides(rfd, gal, dim):
    rows = 300
    g, planted, full = _case(dim, rows, 8300 + dim)
    ga = _filled(gal, g)
    before = _check(ga, full, 0, rows, (dim, "whole"))
    gone = sorted(set([planted[0], planted[2], 1, 17, 298] + list(range(32, 48)) + list(range(100, 300, 7))))   # a best match, a whole block
    assert before[1][planted[1]] == planted[0]
    assert ga.remove(gone) == 0
    live = np.ones(rows, bool)
    live[gone] = False
    s, r, i = _check(ga, full, 0, rows, (dim, "removed"), live=live)
    assert np.all(r[gone] == -1) and np.all(np.isneginf(s[gone])) and not np.isin(r, gone).any()
    assert r[planted[1]] == planted[3]                                      # its best match is gone: the next duplicate
    _check(ga, full, 30, 20, (dim, "a range over the dead block"), live=live)
    assert ga.remove(np.flatnonzero(live)[2:]) == 0                         # two live rows stay
    live[np.flatnonzero(live)[2:]] = False
    s, r, _ = _check(ga, full, 0, rows, (dim, "two left"), live=live)
    a, b = np.flatnonzero(live)
    assert r[a] == b and r[b] == a and (r >= 0).sum() == 2


@pytest.mark.parametrize("dim", [32, 512])
def test_both_modes_over_identity_patterns(rfd, gal, dim):
    rows = 330
    g, planted, full = _case(dim, rows, 8400 + dim)
    rng = np.random.default_rng(dim)
    every = np.arange(rows)
    mixed = np.where(rng.random(rows) < 0.3, -1, every % 5)
    for name, ids in (("row % 7", every % 7), ("runs", every // 40), ("one identity", np.zeros(rows, int)), ("with unlabelled rows", mixed)):
        ga = _filled(gal, g)
        assert _set_ids(ga, every[ids >= 0], ids[ids >= 0]) == 0
        for mode in (N.OTHER_ROW, N.OTHER_IDENTITY):
            s, r, i = _check(ga, full, 0, rows, (dim, name, mode), mode=mode, ids=ids)
            if mode == N.OTHER_IDENTITY and name == "one identity":
                assert np.all(r == -1) and np.all(i == -1) and np.all(np.isneginf(s))      # every entry is empty
            elif mode == N.OTHER_IDENTITY:
                assert np.all(r >= 0) and not np.any((ids >= 0) & (ids[r] == ids))
            else:
                assert np.array_equal(i, ids[r])
        _check(ga, full, 41, 77, (dim, name, "range"), mode=N.OTHER_IDENTITY, ids=ids)
        assert ga.remove([planted[0], 40, 41]) == 0                                         # remove unlabels, too
        live = np.ones(rows, bool)
        live[[planted[0], 40, 41]] = False
        _check(ga, full, 0, rows, (dim, name, "removed"), mode=N.OTHER_IDENTITY, ids=np.where(live, ids, -1), live=live)
        ga.close()


@pytest.mark.parametrize("dim", [64, 512])
def test_tag_masks(rfd, gal, dim):
    rows = 330
    g, planted, full = _case(dim, rows, 8500 + dim)
    rng = np.random.default_rng(dim + 1)
    tags = np.array([0, 1, 2, 0x80000001, 0x80000002, 0xFFFFFFFF], np.int64)[rng.integers(0, 6, rows)]
    tags[7] = 0x40000000                                                                    # a tenant of one row
    ids = np.arange(rows) % 9
    ga = _filled(gal, g)
    _check(ga, full, 0, rows, (dim, "a mask without any tag set"), tag_mask=ALL)
    assert _set_tags(ga, np.arange(rows), tags) == 0 and _set_ids(ga, np.arange(rows), ids) == 0
    for mask in (0, ALL, 0xC0000000, 3):
        for mode in (N.OTHER_ROW, N.OTHER_IDENTITY):
            s, r, i = _check(ga, full, 0, rows, (dim, mask, mode), mode=mode, tag_mask=mask, ids=ids, tags=tags)
            ok = r >= 0
            assert np.all(((tags[ok] ^ tags[r[ok]]) & mask) == 0)
            if mask in (ALL, 0xC0000000):
                assert r[7] == -1                                                           # nobody shares its tenant
    _check(ga, full, 5, 100, (dim, "range"), tag_mask=0x80000000, ids=ids, tags=tags)


def test_min_score_at_a_score_one_ulp_above_and_infinite(rfd, gal):
    dim, rows = 512, 200
    g, planted, full = _case(dim, rows, 8600)
    ga = _filled(gal, g)
    s0, r0, _ = _check(ga, full, 0, rows, "no threshold")
    at = float(np.sort(s0)[rows // 2])
    above = float(np.nextafter(np.float32(at), np.float32(np.inf)))
    assert (s0 == np.float32(at)).any() and above > at
    for ms in (at, above, float("inf"), float(s0.max()), NEG_INF):
        s, r, i = _check(ga, full, 0, rows, ("min_score", ms), min_score=ms)
        keep = s0 >= np.float32(ms)
        assert np.array_equal(r, np.where(keep, r0, -1)) and np.array_equal(_bits(s), _bits(np.where(keep, s0, NEG_INF)))
    assert not (_nearest(ga, 0, rows, min_score=float("inf"))[2] >= 0).any()
    assert (_nearest(ga, 0, rows, min_score=at)[2] >= 0).sum() > (_nearest(ga, 0, rows, min_score=above)[2] >= 0).sum() > 0


def test_a_nan_row_and_a_minus_infinite_score_are_never_selected(rfd, det, gal):
    import torch
    dim, rows = 32, 50
    rng = np.random.default_rng(8700)
    g = rng.integers(-8, 9, (rows, dim)).astype(np.float64) / 64
    g[:, 0] = rng.integers(1, 9, rows) / 64                                # element 0 > 0 everywhere ...
    g[9, 0] = NEG_INF                                                      # ... so every score against row 9 is -inf
    g[7, 3] = np.nan                                                       # every score of and against row 7 is NaN
    with np.errstate(invalid="ignore"):
        full = R.scores(g, g)
    others = np.setdiff1d(np.arange(rows), [7, 9])
    assert np.all(np.isneginf(full[others, 9])) and np.all(np.isnan(full[:, 7])) and np.all(np.isfinite(full[np.ix_(others, others)]))
    ga = gal(dim, rows)
    d = torch.tensor(g.astype(np.float32), device="cuda")                  # only the device form stores what it cannot look at
    first = C.c_int(-1)
    assert ga.L.rfd_gallery_add_device(ga.g, d.data_ptr(), rows, C.byref(first)) == 0 and ga.L.rfd_sync(det._ctx) == 0
    with np.errstate(invalid="ignore"):
        s, r, _ = _check(ga, full, 0, rows, "nan and -inf")
    assert r[7] == -1 and r[9] == -1 and not np.isin(r, [7, 9]).any() and np.all(r[others] >= 0)


# ---- 4. consistency with the shipped searches, any data ----
@pytest.mark.parametrize("dim", [64, 512])
def test_every_entry_is_the_rows_own_search_without_the_self_match(rfd, gal, dim):
    rows = 700
    x = _units(np.random.default_rng(8800 + dim), rows, dim)
    x[300] = x[20]                                                          # an exact duplicate
    rng = np.random.default_rng(dim)
    tags = rng.integers(0, 3, rows) | 0x80000000
    ids = np.where(rng.random(rows) < 0.2, -1, np.arange(rows) % 40)
    ga = _filled(gal, x)
    stored = ga.get(0, rows)[1]
    every = np.arange(rows)

    def first_other(s, r, i, drop):
        out = []
        for a in range(rows):
            left = [j for j in range(s.shape[1]) if r[a, j] >= 0 and not drop(a, r[a, j], i[a, j])]
            out.append((s[a, left[0]], r[a, left[0]], i[a, left[0]]) if left else (np.float32(NEG_INF), -1, -1))
        return [np.array(c) for c in zip(*out)]

    # rows alone: the filtered search on a gallery without identities is the filtered row search
    assert _set_tags(ga, every, tags) == 0
    for mask in (0, ALL):
        st, s, r, i = _search_filtered(ga, stored, 2, np.full(rows, mask), tags & mask)
        assert st == 0
        want = first_other(s, r, i, lambda a, b, ident: b == a)
        st, ns, nr, ni = _nearest(ga, 0, rows, tag_mask=mask)
        assert st == 0 and np.array_equal(nr, want[1]) and np.array_equal(_bits(ns), _bits(want[0])) and np.all(ni == -1), mask
    assert nr[20] == 300 or tags[20] != tags[300]
    # identities: the identity search with the row's own identity dropped
    assert _set_ids(ga, every[ids >= 0], ids[ids >= 0]) == 0
    st, s, r, i = _search_ids(ga, stored, 2)
    assert st == 0
    want = first_other(s, r, i, lambda a, b, ident: b == a or (ids[a] >= 0 and ident == ids[a]))
    st, ns, nr, ni = _nearest(ga, 0, rows, mode=N.OTHER_IDENTITY)
    assert st == 0 and np.array_equal(nr, want[1]) and np.array_equal(ni, want[2]) and np.array_equal(_bits(ns), _bits(want[0]))
    # score(a, b) and score(b, a): where a is the nearest of its nearest, the bits agree
    st, ns, nr, _ = _nearest(ga, 0, rows)
    mutual = 0
    for a in range(0, rows, 9):
        b = int(nr[a])
        st, bs, br, _ = _nearest(ga, b, 1)
        if st == 0 and br[0] == a:
            mutual += 1
            assert _bits(bs)[0] == _bits(ns)[a]
    assert mutual >= 10


# ---- 5. independence ----
@pytest.mark.parametrize("dim", [64, 512])
def test_one_call_and_many_calls_give_the_same_and_the_device_form_too(rfd, det, gal, dim):
    import torch
    rows = 900
    g, planted, full = _case(dim, rows, 8900 + dim)
    ids, tags = np.arange(rows) % 11, np.arange(rows) % 3
    ga = _filled(gal, g)
    assert _set_ids(ga, np.arange(rows), ids) == 0 and _set_tags(ga, np.arange(rows), tags) == 0 and ga.remove([3, 500]) == 0
    live = np.ones(rows, bool)
    live[[3, 500]] = False
    kw = dict(mode=N.OTHER_IDENTITY, tag_mask=1, ids=np.where(live, ids, -1), tags=np.where(live, tags, 0), live=live)
    row0, n = 13, 870
    one = _check(ga, full, row0, n, (dim, "one call"), **kw)
    for step in (1, 7, 64):
        parts = [_nearest(ga, a, min(step, row0 + n - a), kw["mode"], NEG_INF, kw["tag_mask"]) for a in range(row0, row0 + n, step)]
        assert all(p[0] == 0 for p in parts)
        for j in range(3):
            assert np.array_equal(np.concatenate([p[j + 1] for p in parts]).view(np.uint32), one[j].view(np.uint32)), (dim, step, j)
    assert np.array_equal(_nearest(ga, row0, n, kw["mode"], NEG_INF, kw["tag_mask"], with_ids=False)[2], one[1])     # ids may be NULL
    # the device form, outputs at 4-byte-aligned offsets, guard words around them
    buf = torch.full((3, n + 8), -7, dtype=torch.int32, device="cuda")
    cfg = rfd.rfd_gallery_nearest_config(kw["mode"], NEG_INF, kw["tag_mask"])
    ptr = [buf[j].data_ptr() + 4 * (1 + 2 * j) for j in range(3)]
    assert all(p % 16 != 0 for p in ptr)
    assert ga.L.rfd_gallery_nearest_device(ga.g, row0, n, C.byref(cfg), ptr[0], ptr[1], ptr[2], 0) == 0
    out = buf.cpu().numpy()
    for j in range(3):
        at = 1 + 2 * j
        assert np.array_equal(out[j, at:at + n].view(np.uint32), one[j].view(np.uint32)), (dim, j)
        assert np.all(out[j, :at] == -7) and np.all(out[j, at + n:] == -7)


# ---- 6. stream order, refusals, and the searches around a call ----
def test_device_calls_run_in_stream_order_without_host_waits(rfd, det, gal):
    import torch
    L, dim, rows = rfd.load_library(), 512, 700
    g, planted, full = _case(dim, rows, 9000)
    emb = torch.tensor(g.astype(np.float32), device="cuda")
    out1 = [torch.full((rows,), -7, dtype=t, device="cuda") for t in (torch.float32, torch.int32, torch.int32)]
    out2 = [torch.full((rows,), -7, dtype=t, device="cuda") for t in (torch.float32, torch.int32, torch.int32)]
    torch.cuda.synchronize()
    gone = np.array([planted[0], 16, 17, 350, 699], np.int32)
    ga = gal(dim, rows)
    first = C.c_int(-1)
    assert L.rfd_gallery_add_device(ga.g, emb.data_ptr(), rows, C.byref(first)) == 0 and first.value == 0
    assert L.rfd_gallery_nearest_device(ga.g, 0, rows, None, out1[0].data_ptr(), out1[1].data_ptr(), out1[2].data_ptr(), 1) == 0
    assert L.rfd_gallery_remove(ga.g, gone.ctypes.data, len(gone)) == 0
    assert L.rfd_gallery_nearest_device(ga.g, 0, rows, None, out2[0].data_ptr(), out2[1].data_ptr(), out2[2].data_ptr(), 1) == 0
    assert L.rfd_sync(det._ctx) == 0
    live = np.ones(rows, bool)
    live[gone] = False
    for out, ref in ((out1, N.nearest_of_scores(full)), (out2, N.nearest_of_scores(full, live=live))):
        s, r, i = (o.cpu().numpy() for o in out)
        assert np.array_equal(r, ref[1]) and np.array_equal(i, ref[2]) and np.array_equal(_bits(s), _bits(ref[0]))


def test_refusals_write_nothing_and_searches_around_a_call_are_unchanged(rfd, gal):
    dim, rows = 64, 100
    q, g, planted = _dyadic_case(dim, rows, 5, 9100)
    ga = _filled(gal, g, extra=20)
    L, INV = ga.L, rfd.RFD_ERR_INVALID_ARG
    before = ga.search(q, 7)
    s, r, i = np.full(8, 7.0, np.float32), np.full(8, -7, np.int32), np.full(8, -7, np.int32)
    sp, rp, ip = s.ctypes.data, r.ctypes.data, i.ctypes.data
    cfg = rfd.rfd_gallery_nearest_config

    def call(row0, n, c=None, scores=sp, out_rows=rp, out_ids=ip):
        return L.rfd_gallery_nearest(ga.g, row0, n, None if c is None else C.byref(c), scores, out_rows, out_ids)

    assert call(-1, 2) == INV and call(0, -1) == INV and call(rows - 1, 2) == INV and call(rows, 1) == INV and call(0, rows + 1) == INV
    assert call(100, 4) == INV                                                           # within the capacity, beyond the rows handed out
    assert call(0, 4, cfg(2, NEG_INF, 0)) == INV and call(0, 4, cfg(-1, NEG_INF, 0)) == INV and "mode" in ga.err()
    for word in range(5):
        c = cfg(0, NEG_INF, 0)
        c.reserved[word] = 1
        assert call(0, 4, c) == INV and "reserved" in ga.err()
    assert call(0, 4, scores=None) == INV and call(0, 4, out_rows=None) == INV
    assert call(0, 4, scores=sp + 2) == INV and call(0, 4, out_rows=rp + 1) == INV and call(0, 4, out_ids=ip + 3) == INV
    assert L.rfd_gallery_nearest_device(ga.g, 0, 4, None, sp + 2, rp, ip, 0) == INV and L.rfd_gallery_nearest_device(ga.g, 0, 4, None, None, rp, ip, 0) == INV
    assert L.rfd_gallery_nearest(None, 0, 4, None, sp, rp, ip) == INV
    assert np.all(s == 7.0) and np.all(r == -7) and np.all(i == -7)                      # a refused call writes nothing
    assert call(0, 0) == 0 and call(rows, 0) == 0 and call(0, 0, scores=None, out_rows=None, out_ids=None) == 0   # n = 0: a no-op
    assert np.all(s == 7.0) and np.all(r == -7) and np.all(i == -7)
    assert call(0, 4, out_ids=None) == 0 and np.all(r[:4] >= 0) and np.all(r[4:] == -7) and np.all(i == -7) and np.all(s[4:] == 7.0)
    assert call(96, 4, cfg(1, 0.0, ALL)) == 0                                            # the last rows, every field set
    after = ga.search(q, 7)
    assert after[0] == before[0] == 0 and np.array_equal(after[2], before[2]) and np.array_equal(_bits(after[1]), _bits(before[1]))
