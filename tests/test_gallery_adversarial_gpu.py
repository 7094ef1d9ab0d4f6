"""The gallery search (csrc/kernels_gallery.hip) where the two other gallery files do not go, through the C ABI and against
tests/gallery_ref.py, bit for bit on data whose scores are exact in f32 in any summation order (asserted on the CPU first):

a. dims whose K-step count (3, 5, 11, 32) is no divisor and no multiple of the scan's prefetch depth of 8, so a block's last K
   step, the selection, the accumulator reset and (masked) the live word's slot rotate through all eight unroll slots; dim 1024
   also launches the scan with more than 64 KiB of dynamic LDS;
b. hostile orders of arrival inside one batch: scores that rise with the row (every row of every block is inserted at the head
   of its list), that fall with it, that are all equal (the tie rule alone decides, across waves, workgroups and the merge), and
   that lie in long runs of equal values;
c. a gallery large enough for the cap on the scan's workgroups to bind: waves walk three and four blocks at a stride;
d. NaN, +inf and -inf in rows and in a query of the device forms;
e. a host search of more than two passes.

Every case asserts on the CPU that it is in the regime it names, so a change of the launch rules makes it fail instead of pass
emptily."""
import ctypes as C
import functools

import numpy as np
import pytest

import gallery_ref as R
from test_gallery_gpu import _bits, _dyadic_case, det  # noqa: F401  (det: the module's detector fixture)
from test_gallery_edit_gpu import _check_search, _masked_topk, _patterns, gal  # noqa: F401  (gal: makes EditGal galleries)

pytestmark = pytest.mark.gpu

WAVES, PREFETCH, MAX_QUERIES = 4, 8, 32   # kGalleryWaves, kGalleryPrefetch, kGalleryMaxQueries


def _scan_lds_bytes(dim, n, k):
    """dynamic LDS of one scan of n <= 32 queries: the queries' A fragments, then one list of k keys per wave and query"""
    nmt = 2 if n > 16 else 1
    return nmt * 16 * dim * 2 + WAVES * nmt * 16 * k * 8


def _add_in_pieces(ga, g):
    """adds that start and end inside 16-row blocks"""
    cuts = [0] + [c for c in (7, 37, 1037) if c < len(g)] + [len(g)]
    for a, b in zip(cuts[:-1], cuts[1:]):
        assert ga.add(g[a:b]) == (0, a)
    assert ga.size()[0] == len(g)


# ---- a. K-step counts that rotate a block's end through the unroll slots; more than 64 KiB of LDS ----
NK = ((1, 1), (16, 32), (17, 5), (33, 32))   # NMT = 1, NMT = 1 full, NMT = 2, and a second pass of one query


@pytest.mark.parametrize("rows", [1, 40, 4097])
@pytest.mark.parametrize("dim", [96, 160, 352, 1024])
def test_exact_at_k_step_counts_off_the_prefetch_depth(rfd, gal, dim, rows):
    ksteps = dim // 32
    if dim != 1024:
        assert ksteps % PREFETCH != 0 and PREFETCH % ksteps != 0              # 3, 5, 11: a block's end visits every unroll slot
    if dim == 1024:
        # the first pass of (33, 32), 32 queries and k = 32, is the launch that needs the raised limit, masked and not
        assert _scan_lds_bytes(dim, 32, 32) == 98304 > 65536 and _scan_lds_bytes(dim, 17, 5) > 65536
    q, g, planted = _dyadic_case(dim, rows, 33, 1000 + dim + rows)
    full = R.scores(q, g)
    assert np.array_equal(full.astype(np.float32).astype(np.float64), full)
    ga = gal(dim, rows + 3)
    _add_in_pieces(ga, g)
    for n, k in NK:
        ref_s, ref_r = R.topk_of_scores(full[:n], k)
        st, s, r = ga.search(q[:n], k)
        assert st == 0
        assert np.array_equal(r, ref_r), (dim, rows, n, k)
        assert np.array_equal(_bits(s), _bits(ref_s)), (dim, rows, n, k)
        assert list(r[0, :min(k, len(planted))]) == planted[:k]              # equal scores: the lower row first
    ga.close()
    for name, gone in _patterns(rows):
        ga = gal(dim, rows + 3)
        _add_in_pieces(ga, g)
        assert ga.remove(gone) == 0
        live_rows = np.setdiff1d(np.arange(rows), gone)
        assert ga.live() == len(live_rows)
        for n, k in NK:
            s, r = _check_search(ga, q, full, live_rows, n, k, (dim, rows, name, n, k))
            assert not np.isin(r, gone).any(), (dim, rows, name, n, k)
        ga.close()


# ---- b. hostile orders of arrival ----
H_DIM, H_ROWS = 96, 4097
H_PLACES = (0, 15, 16, 31, 32)   # both ends of both M-tiles, and the second pass


def _query_unit(v):
    """the largest power of two that divides every element of the dyadic vector v"""
    u = 1.0
    while not np.array_equal(np.rint(v / u), v / u):
        u /= 2
        assert u >= 2.0 ** -40
    return u


def _assert_exact_per_query(q, g):
    """g in units of 2^-6, query i in units of its own u_i: every product is an integer in units of u_i 2^-6, and so is every
    partial sum in any order, below 2^24 in magnitude -- exact in f32"""
    assert np.array_equal(R.rne_bf16(g), g) and np.array_equal(R.rne_bf16(q), q)
    assert np.array_equal(np.rint(g * 64), g * 64)
    mag = np.abs(q) @ np.abs(g).T
    for i in range(len(q)):
        assert float(mag[i].max()) / (_query_unit(q[i]) / 64) < 2.0 ** 24, i


@functools.lru_cache(maxsize=None)
def _hostile_gallery():
    rng = np.random.default_rng(41)
    j = np.arange(H_ROWS)
    g = rng.integers(-8, 9, (H_ROWS, H_DIM)).astype(np.float64) / 64
    for e in range(4):
        g[:, e] = ((j >> (4 * (3 - e))) & 15) / 64   # the base-16 digits of the row number, most significant first
    g[:, 4] = 5 / 64
    g.setflags(write=False)
    return g


def _hostile_batch(rot):
    """33 queries: random dyadic ones over the random elements, and at H_PLACES the five special ones, rotated by `rot`.
    Returns the batch and {name: place}."""
    rng = np.random.default_rng(43)
    q = rng.integers(-8, 9, (33, H_DIM)).astype(np.float64) / 64
    q[:, :5] = 0
    z = np.zeros(H_DIM)
    a, c, d, e = z.copy(), z.copy(), z.copy(), z.copy()
    a[:4] = [1.0, 2.0 ** -4, 2.0 ** -8, 2.0 ** -12]   # A: score j * 2^-18, strictly rising with the row
    c[4] = 0.5                                          # C: every score equal
    d[0] = 0.25                                         # D: element 0 alone
    e[1] = 0.25                                         # E: element 1 alone
    special = [("A", a), ("B", -a), ("C", c), ("D", d), ("E", e)]
    where = {}
    for i, place in enumerate(H_PLACES):
        name, v = special[(i + rot) % 5]
        q[place], where[name] = v, place
    return q, where


H_PATTERNS = [("none", []), ("the top 40 of A", list(range(H_ROWS - 40, H_ROWS))), ("rows 0..39", list(range(40))),
              ("every even row", list(range(0, H_ROWS, 2)))]


@pytest.mark.parametrize("pattern", H_PATTERNS, ids=[p[0].replace(" ", "_") for p in H_PATTERNS])
def test_hostile_orders_of_arrival_in_one_batch(rfd, gal, pattern):
    """Query D is as the construction states it, nonzero in element 0 alone; with 4097 rows that digit is 0 for every row but
    the last, so D has one row above a single run of 4096 equal scores.  Query E, nonzero in element 1 alone, is the one with 16
    score levels in runs of 256 rows.  The five special queries take every one of the five places in turn."""
    name, gone = pattern
    g = _hostile_gallery()
    live_rows = np.setdiff1d(np.arange(H_ROWS), gone)
    ga = gal(H_DIM, H_ROWS)
    _add_in_pieces(ga, g)
    assert ga.remove(gone) == 0 and ga.live() == len(live_rows)
    live = live_rows.tolist()
    for rot in range(5):
        q, where = _hostile_batch(rot)
        _assert_exact_per_query(q, g)
        full = R.scores(q, g)
        assert np.array_equal(full.astype(np.float32).astype(np.float64), full)
        fa = full[where["A"]]
        assert np.array_equal(fa, np.arange(H_ROWS) * 2.0 ** -18) and np.array_equal(full[where["B"]], -fa)
        assert np.all(full[where["C"]] == full[where["C"], 0]) and full[where["C"], 0] != 0
        assert len(np.unique(full[where["D"]])) == 2 and len(np.unique(full[where["E"]])) == 16
        for k in (1, 32):
            s, r = _check_search(ga, q, full, live_rows, 33, k, (name, rot, k))
            tag = (name, rot, k)
            assert r[where["A"]].tolist() == live[::-1][:k], tag                 # rising: the highest live rows, descending
            assert r[where["B"]].tolist() == live[:k], tag                       # falling: the lowest live rows
            assert r[where["C"]].tolist() == live[:k], tag                       # all equal: the tie rule alone
            assert len(set(_bits(s[where["C"]]).tolist())) == 1, tag
            assert r[where["D"]].tolist() == sorted(live, key=lambda j: (-(j >> 12), j))[:k], tag
            assert r[where["E"]].tolist() == sorted(live, key=lambda j: (-((j >> 8) & 15), j))[:k], tag
    if name == "none":
        assert r[where["A"]].tolist() == list(range(4096, 4096 - 32, -1)) and r[where["B"]].tolist() == list(range(32))
    if name == "the top 40 of A":
        assert r[where["A"]][0] == 4056 and r[where["B"]][0] == 0
    if name == "rows 0..39":
        assert r[where["A"]][0] == 4096 and r[where["B"]].tolist() == list(range(40, 72)) and r[where["C"]][0] == 40
    if name == "every even row":
        assert r[where["A"]].tolist() == list(range(4095, 4095 - 64, -2)) and r[where["B"]].tolist() == list(range(1, 65, 2))
        assert r[where["C"]].tolist() == list(range(1, 65, 2))


# ---- c. the capped grid ----
@functools.lru_cache(maxsize=None)
def _capped_case(cus):
    stride = 2 * cus * WAVES                 # blocks between two steps of one wave once the cap binds
    nblocks = 3 * stride + 5
    rows = 16 * nblocks - 3
    q, g, planted = _dyadic_case(32, rows, 33, 77)
    full = R.scores(q, g)
    assert np.array_equal(full.astype(np.float32).astype(np.float64), full)
    top33 = R.topk_of_scores(full, 33)[0]
    for a in (q, g, full, top33):
        a.setflags(write=False)
    return stride, nblocks, rows, q, g, planted, full, top33


def _capped_patterns(stride, nblocks, rows):
    def blocks(bs):
        return [r for b in bs for r in range(16 * b, 16 * b + 16) if r < rows]
    # Wave 7 (workgroup 1, wave 3) walks blocks 7, 7 + stride, 7 + 2 stride; 7 + 3 stride is past the gallery's 3 stride + 5
    # blocks.  Wave 4 walks four blocks, the last of them the gallery's partial last block.  Both walks are removed whole.
    assert 7 + 2 * stride < nblocks <= 7 + 3 * stride and 4 + 3 * stride == nblocks - 1
    walks = [7 + i * stride for i in range(3)] + [4 + i * stride for i in range(4)]
    return [("none", []), ("planted", [63, 2111]), ("one block", blocks([2 * stride + 9])), ("two waves' walks", sorted(blocks(walks)))]


@pytest.mark.parametrize("pattern", range(4), ids=["none", "planted", "one_block", "two_waves_walks"])
def test_exact_when_the_cap_on_workgroups_binds(rfd, gal, pattern):
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    stride, nblocks, rows, q, g, planted, full, top33 = _capped_case(cus)
    groups_max = 2 * cus
    assert -(-nblocks // (WAVES * 2)) > groups_max          # the cap is what binds: waves walk three and four blocks
    assert rows > groups_max * 128
    # at dim 32 the scores take few values: every query has equal scores among its best 33, rows of different strided blocks
    assert all(len(set(top33[i].tolist())) < 33 for i in range(33))
    name, gone = _capped_patterns(stride, nblocks, rows)[pattern]
    live_rows = np.setdiff1d(np.arange(rows), gone)
    ga = gal(32, rows)
    _add_in_pieces(ga, g)
    assert ga.remove(gone) == 0 and ga.live() == len(live_rows)
    for n, k in ((33, 32), (1, 5)):
        s, r = _check_search(ga, q, full, live_rows, n, k, (name, n, k))
        assert not np.isin(r, gone).any()
        ties = sum(len(set(_bits(s[i]).tolist())) < k for i in range(n))
        print("capped grid, %s, n %d k %d: %d of %d queries have equal scores among their results" % (name, n, k, ties, n))
    if name == "none":
        assert r[0].tolist() == planted[:5]                  # query 0's planted rows, equal scores, one of them the last row
    if name == "planted":
        assert r[0].tolist()[:4] == [p for p in planted if p not in gone][:4]


# ---- d. non-finite values in the device forms ----
def test_non_finite_values_in_the_device_forms(rfd, det, gal):
    """rfd.h: "a NaN score compares false with everything and is never selected (nor is a score of -inf)".  Several rows of each
    hostile kind, so that k = 32 exceeds the number of rows with a finite score; about +inf scores nothing is asserted beyond
    the reference order."""
    import torch
    L, dim, rows, nq, k = rfd.load_library(), 64, 50, 20, 32
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(13)
    g = rng.integers(-8, 9, (rows, dim)).astype(np.float64) / 64
    q = rng.integers(-8, 9, (nq, dim)).astype(np.float64) / 64
    finite_g = g.copy()
    nan_rows, pinf_rows, ninf_rows = [5, 15, 16, 31, 40, 44, 47], [17, 32, 38, 42, 46], [0, 20, 33, 41, 45, 48, 49]
    g[nan_rows, 9] = np.nan
    g[pinf_rows, 33] = np.inf      # queries are 0 there (a NaN score), positive (+inf) or negative (-inf)
    g[ninf_rows, 0] = -np.inf
    q[:, 33] = np.resize([0.0, 3 / 64, -2 / 64, 0.0, 0.0], nq)
    q[:, 0] = np.resize([5 / 64, 0.0, 1 / 64, -4 / 64], nq)
    nan_query = 3
    q_clean = q.copy()
    q[nan_query, 40] = np.nan
    # exactness of the finite scores, as in _dyadic_case
    assert np.array_equal(R.rne_bf16(finite_g), finite_g) and np.array_equal(R.rne_bf16(q_clean), q_clean)
    assert float((np.abs(q_clean) @ np.abs(finite_g).T).max()) * 2.0 ** 12 < 2.0 ** 24

    def expected(qs):
        with np.errstate(invalid="ignore"):
            full = (qs[:, None, :] * g[None, :, :]).sum(-1)      # f64, the non-finite values taking part
        return full, ~np.isnan(full) & ~np.isneginf(full)
    full, ok = expected(q)
    assert int(np.isfinite(full).sum(1).max()) < k and not ok[nan_query].any()
    assert np.isposinf(full).any() and np.isneginf(full).any() and np.isnan(full[:, pinf_rows]).any()
    fin = full[np.isfinite(full)]
    assert np.array_equal(fin.astype(np.float32).astype(np.float64), fin)

    d_g = torch.from_numpy(g.astype(np.float32)).to(dev)
    d_q = torch.from_numpy(q.astype(np.float32)).to(dev)
    d_qc = torch.from_numpy(q_clean.astype(np.float32)).to(dev)
    torch.cuda.synchronize()
    ga = gal(dim, rows + 2)
    first = C.c_int(-1)
    assert L.rfd_gallery_add_device(ga.g, d_g.data_ptr(), 7, C.byref(first)) == 0 and first.value == 0
    assert L.rfd_gallery_add_device(ga.g, d_g.data_ptr() + 7 * dim * 4, rows - 7, C.byref(first)) == 0 and first.value == 7

    def search(d, n):
        d_s = torch.full((n, k), 7.0, device=dev)
        d_r = torch.full((n, k), -7, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        assert L.rfd_gallery_search_device(ga.g, d.data_ptr(), n, k, d_s.data_ptr(), d_r.data_ptr(), 0) == 0
        return d_s.cpu().numpy(), d_r.cpu().numpy()

    def check(removed):
        short = 0
        full_c, ok_c = expected(q_clean)
        for n in (nq, 5):                                        # NMT = 2 and NMT = 1; the NaN query is in both
            s, r = search(d_q, n)
            for i in range(n):
                cols = np.array([j for j in np.flatnonzero(ok[i]) if j not in removed], np.int64)
                ref_s, ref_r = _masked_topk(full[i:i + 1], cols, k)
                tag = (removed, n, i)
                assert np.array_equal(r[i], ref_r[0]), tag
                f = np.isfinite(ref_s[0])
                assert np.array_equal(_bits(s[i][f]), _bits(ref_s[0][f])), tag
                assert np.all(r[i, len(cols):] == -1) and np.all(np.isneginf(s[i, len(cols):])), tag
                short += len(cols) < k
            assert np.all(r[nan_query] == -1) and np.all(np.isneginf(s[nan_query]))
            # the other queries return what they return in a batch without the NaN
            sc, rc = search(d_qc, n)
            others = np.arange(n) != nan_query
            assert np.array_equal(r[others], rc[others]) and np.array_equal(_bits(s[others]), _bits(sc[others]))
            assert rc[nan_query, 0] >= 0
        assert short >= 2                                        # the tails were looked at
    check(())
    gone = 2                                                     # a row with finite scores only
    assert gone not in nan_rows + pinf_rows + ninf_rows
    assert ga.remove([gone]) == 0 and ga.live() == rows - 1      # from here on the masked scan
    check((gone,))


# ---- e. more than two passes ----
def test_three_passes_share_the_workspace_in_stream_order(rfd, gal):
    dim, rows, n, k = 128, 333, 70, 7
    assert -(-n // MAX_QUERIES) == 3
    q, g, planted = _dyadic_case(dim, rows, n, 5)
    full = R.scores(q, g)
    assert np.array_equal(full.astype(np.float32).astype(np.float64), full)
    ga = gal(dim, rows)
    _add_in_pieces(ga, g)
    for gone in ([], [2, 63, 64, 200]):
        assert ga.remove(gone) == 0
        live_rows = np.setdiff1d(np.arange(rows), gone)
        s, r = _check_search(ga, q, full, live_rows, n, k, ("one call", len(gone)))
        parts = [ga.search(q[a:b], k) for a, b in ((0, 32), (32, 64), (64, 70))]
        assert all(p[0] == 0 for p in parts)
        assert np.array_equal(r, np.concatenate([p[2] for p in parts]))
        assert np.array_equal(_bits(s), _bits(np.concatenate([p[1] for p in parts])))
