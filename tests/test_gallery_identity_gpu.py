"""The gallery's identity search (include/rfd.h, "identities"; csrc/kernels_gallery.hip, the IDENT scan) through the C ABI,
against tests/gallery_identity_ref.py.  The data are dyadic, so every score is exact in f32 in any summation order (asserted on
the CPU first) and every comparison is bit for bit.  Every case asserts on the CPU, from the reference alone, that it is in the
regime it names, so a change of the launch rules makes it fail instead of pass emptily."""
import ctypes as C
import functools

import numpy as np
import pytest

import gallery_identity_ref as I
import gallery_ref as R
from test_gallery_gpu import _bits, _dyadic_case, det  # noqa: F401  (det: the module's detector fixture)
from test_gallery_edit_gpu import gal  # noqa: F401  (gal: makes EditGal galleries)
from test_gallery_adversarial_gpu import (H_ROWS, NK, WAVES, _add_in_pieces, _assert_exact_per_query, _capped_case, _hostile_batch,
                                          _hostile_gallery)

pytestmark = pytest.mark.gpu

NEG_INF = float("-inf")


# ---- the calls of this file on an EditGal (statuses returned, not raised) ----
def _i32(x):
    return np.ascontiguousarray(np.asarray(x, np.int64).reshape(-1), np.int32)


def _set_ids(ga, rows, ids):
    r, i = _i32(rows), _i32(ids)
    assert r.shape == i.shape
    return ga.L.rfd_gallery_set_identities(ga.g, r.ctypes.data, i.ctypes.data, r.shape[0])


def _get_ids(ga, row0, n):
    out = np.full(max(n, 1), -7, np.int32)
    return ga.L.rfd_gallery_get_identities(ga.g, row0, n, out.ctypes.data), out[:n]


def _labelled(ga):
    n = C.c_int(-7)
    assert ga.L.rfd_gallery_identities(ga.g, C.byref(n)) == 0
    return n.value


def _search_ids(ga, q, k, min_score=NEG_INF):
    q = np.ascontiguousarray(q, np.float32).reshape(-1, ga.dim)
    shape = (q.shape[0], max(k, 1))
    s, r, i = np.full(shape, 7.0, np.float32), np.full(shape, -7, np.int32), np.full(shape, -7, np.int32)
    st = ga.L.rfd_gallery_search_identities(ga.g, q.ctypes.data, q.shape[0], k, min_score, s.ctypes.data, r.ctypes.data, i.ctypes.data)
    return st, s, r, i


def _check(ga, q, full, ids, live, n, k, tag, min_score=NEG_INF):
    """the identity search of q[:n] equals the reference on the score matrix `full`, bit for bit"""
    ref_s, ref_r, ref_i = I.topk_of_scores(full[:n], ids, k, min_score, live)
    st, s, r, i = _search_ids(ga, q[:n], k, min_score)
    assert st == 0, tag
    assert np.array_equal(r, ref_r), tag
    assert np.array_equal(i, ref_i), tag
    assert np.array_equal(_bits(s), _bits(ref_s)), tag
    return s, r, i


def _exact(full):
    assert np.array_equal(full.astype(np.float32).astype(np.float64), full)


def _groups(rows, cus):
    """workgroups of a scan over `rows` rows (gallery_search_groups) and the blocks between two steps of one wave"""
    nblocks = -(-rows // 16)
    groups = max(1, min(2 * cus, -(-nblocks // (WAVES * 2))))
    return groups, groups * WAVES


def _cus():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


def _scan_lds_bytes(dim, n, k):
    """dynamic LDS of one identity scan: the queries' A fragments, then per wave and query k keys of 8 bytes and k identities"""
    nmt = 2 if n > 16 else 1
    return nmt * 16 * dim * 2 + WAVES * nmt * 16 * k * (8 + 4)


def _unplant(g, planted):
    """_dyadic_case's planted rows (the best possible row of query 0) become ordinary rows: copies of a neighbour"""
    for p in planted:
        g[p] = g[p - 1]


def _plant(g, q0, rows, levels):
    """rows[i] scores sum|q0| / 8 - levels[i] / 512 against q0 (|q0| >= 1/64 everywhere): the best possible row, lowered in
    element 0 by levels[i] steps of 1/64 of the row's value"""
    for r, lv in zip(rows, levels):
        g[r] = np.sign(q0) / 8
        g[r, 0] = np.sign(q0[0]) * (8 - lv) / 64


# ---- 1. one identity owns more than 32 best rows ----
@pytest.mark.parametrize("k,others", [(5, 5), (32, 39)])
def test_one_identity_owns_more_best_rows_than_a_list_holds(rfd, gal, k, others):
    dim, rows = 32, 300
    q, g, planted = _dyadic_case(dim, rows, 33, 900 + k)
    _unplant(g, planted)
    _plant(g, q[0], range(40), [r % 3 for r in range(40)])                  # rows 0..39: the best, on three score levels
    ids = np.full(rows, -1)
    ids[:40] = 7
    ids[40:] = 10 + np.arange(40, rows) % others                            # rows 200.. (and the rows before them) are the other identities
    assert len(set(ids.tolist())) == others + 1 >= k
    full = R.scores(q, g)
    _exact(full)
    plain_s, plain_r = R.topk_of_scores(full[:1], 32)
    assert set(plain_r[0].tolist()) <= set(range(40))                       # identity 7 holds all 32 places of the plain search:
    assert len(set(ids[plain_r[0]].tolist())) == 1 < k                      # deduplicating it on the host cannot give k identities
    assert full[0, 40:].max() < full[0, :40].min()
    groups, stride = _groups(rows, _cus())
    assert groups > 1 and 40 <= 16 * WAVES                                  # the 40 rows meet in one workgroup's lists, then in the merge
    ga = gal(dim, rows)
    _add_in_pieces(ga, g)
    assert _set_ids(ga, np.arange(rows), ids) == 0 and _labelled(ga) == rows
    for n in (1, 33):
        s, r, i = _check(ga, q, full, ids, None, n, k, (k, n))
        assert r[0, 0] == 0 and i[0, 0] == 7 and 7 not in i[0, 1:].tolist()
        assert np.all(r[0] >= 0) and len(set(i[0].tolist())) == k           # k identities came back


# ---- 2. one identity spread over places that meet only in a later reduction ----
@pytest.mark.parametrize("place", ["two waves of one workgroup", "two workgroups"])
@pytest.mark.parametrize("best_first", [True, False])
def test_one_identity_in_places_that_meet_in_a_later_reduction(rfd, gal, place, best_first):
    dim, rows, k = 32, 300, 5
    groups, stride = _groups(rows, _cus())
    early, late = (3, 20) if place == "two waves of one workgroup" else (3, 70)
    be, bl = early >> 4, late >> 4
    assert groups >= 2 and be < stride and bl < stride and be != bl        # two waves' first blocks
    assert (be // WAVES == bl // WAVES) == (place == "two waves of one workgroup")
    q, g, planted = _dyadic_case(dim, rows, 33, 950)
    _unplant(g, planted)
    _plant(g, q[0], [early, late], [0, 1] if best_first else [1, 0])
    _plant(g, q[0], [100, 150, 250], [2, 2, 3])                             # runners-up of other identities
    ids = 20 + np.arange(rows) % 9
    ids[[early, late]] = 5
    ids[::7] = -1
    ids[[early, late, 100, 150, 250]] = [5, 5, 6, -1, 8]
    full = R.scores(q, g)
    _exact(full)
    plain = R.topk_of_scores(full[:1], k)[1][0].tolist()
    assert early in plain[:2] and late in plain[:2]                        # without the rule the identity would come back twice
    ga = gal(dim, rows)
    _add_in_pieces(ga, g)
    assert _set_ids(ga, np.arange(rows), ids) == 0
    for n in (1, 33):
        s, r, i = _check(ga, q, full, ids, None, n, k, (place, best_first, n))
        assert r[0, 0] == (early if best_first else late) and i[0].tolist()[:4] == [5, 6, -1, 8]
        assert r[0].tolist()[1:4] == [100, 150, 250]


# ---- 3. hostile orders of arrival ----
@pytest.mark.parametrize("labels", ["row % m", "runs"])
@pytest.mark.parametrize("m", [8, 100])
def test_hostile_orders_of_arrival(rfd, gal, labels, m):
    g = _hostile_gallery()
    j = np.arange(H_ROWS)
    ids = j % m if labels == "row % m" else (j * m) // H_ROWS
    assert len(set(ids.tolist())) == m and np.bincount(ids).min() >= 40    # every identity has more rows than a list has keys
    first_row = {int(c): int(np.flatnonzero(ids == c)[0]) for c in range(m)}
    last_row = {int(c): int(np.flatnonzero(ids == c)[-1]) for c in range(m)}
    ga = gal(g.shape[1], H_ROWS)
    _add_in_pieces(ga, g)
    assert _set_ids(ga, j, ids) == 0
    for rot in (0, 3):
        q, where = _hostile_batch(rot)
        _assert_exact_per_query(q, g)
        full = R.scores(q, g)
        _exact(full)
        assert np.array_equal(full[where["A"]], j * 2.0 ** -18) and np.all(full[where["C"]] == full[where["C"], 0])
        for k in (1, 32):
            s, r, i = _check(ga, q, full, ids, None, 33, k, (labels, m, rot, k))
            kk = min(k, m)
            # rising with the row: every row replaces its identity's entry; the identities' LAST rows, descending
            assert r[where["A"]].tolist()[:kk] == sorted(last_row.values(), reverse=True)[:kk]
            # falling with the row: a later row of a listed identity is a worse duplicate; the identities' FIRST rows, ascending
            assert r[where["B"]].tolist()[:kk] == sorted(first_row.values())[:kk]
            # all equal: the lowest row of each identity, identities ordered by that row
            assert r[where["C"]].tolist()[:kk] == sorted(first_row.values())[:kk]
            assert np.all(r[where["C"]][kk:] == -1) and np.all(i[where["C"]][kk:] == -1)


# ---- 4. unlabelled and labelled rows mixed, every NMT / pass shape ----
def _mixed_ids(rows, seed):
    rng = np.random.default_rng(seed)
    ids = rng.integers(0, max(1, rows // 3), rows)
    ids[rng.random(rows) < 0.3] = -1
    return ids


@pytest.mark.parametrize("rows", [1, 40, 4097])
@pytest.mark.parametrize("dim", [32, 96])
def test_mixed_labelled_and_unlabelled_rows(rfd, gal, dim, rows):
    q, g, planted = _dyadic_case(dim, rows, 33, 2000 + dim + rows)
    ids = _mixed_ids(rows, rows)
    if rows > 64:
        ids[[2, 63, 64]] = [4, 4, -1]                                       # query 0's planted equal scores: one identity twice, one unlabelled
    full = R.scores(q, g)
    _exact(full)
    ga = gal(dim, rows + 3)
    _add_in_pieces(ga, g)
    lab = np.flatnonzero(ids >= 0)
    assert _set_ids(ga, lab, ids[lab]) == 0 and _labelled(ga) == len(lab)
    st, got = _get_ids(ga, 0, rows)
    assert st == 0 and np.array_equal(got, ids)
    for n, k in NK:
        s, r, i = _check(ga, q, full, ids, None, n, k, (dim, rows, n, k))
    if rows > 64:
        assert r[0].tolist()[:2] == [2, 64] and i[0].tolist()[:2] == [4, -1]


def test_mixed_rows_at_the_largest_lds_footprint(rfd, gal):
    dim, rows, n, k = 1024, 4097, 32, 32
    assert _scan_lds_bytes(dim, n, k) == 112 * 1024 and _scan_lds_bytes(dim, n, k) > _scan_lds_bytes(dim, n, k) - 16 * 1024 > 65536
    q, g, planted = _dyadic_case(dim, rows, n, 3100)
    ids = _mixed_ids(rows, 31)
    full = R.scores(q, g)
    _exact(full)
    ga = gal(dim, rows)
    _add_in_pieces(ga, g)
    lab = np.flatnonzero(ids >= 0)
    assert _set_ids(ga, lab, ids[lab]) == 0
    _check(ga, q, full, ids, None, n, k, "unmasked")
    gone = [5, 63, 2111, 4000]
    assert ga.remove(gone) == 0                                             # the masked identity scan at the same footprint
    live = np.ones(rows, bool)
    live[gone] = False
    _check(ga, q, full, ids, live, n, k, "masked")


# ---- 5. the array allocated but all -1, and all identities distinct: the existing kernel is the judge ----
@pytest.mark.parametrize("labels", ["all -1", "all distinct"])
def test_no_shared_identity_equals_the_plain_search(rfd, gal, labels):
    dim, rows = 96, 4097
    q, g, planted = _dyadic_case(dim, rows, 33, 4100)
    ga = gal(dim, rows)
    _add_in_pieces(ga, g)
    ids = np.full(rows, -1) if labels == "all -1" else np.random.default_rng(5).permutation(rows)
    assert _set_ids(ga, np.arange(rows), ids) == 0 and _labelled(ga) == (0 if labels == "all -1" else rows)
    for gone in ([], [2, 64, 1000]):
        assert ga.remove(gone) == 0
        for n, k in NK:
            st, ps, pr = ga.search(q[:n], k)
            st2, s, r, i = _search_ids(ga, q[:n], k)
            assert st == 0 and st2 == 0
            assert np.array_equal(r, pr) and np.array_equal(_bits(s), _bits(ps)), (labels, n, k)
            want = np.where(pr >= 0, ids[np.maximum(pr, 0)], -1)
            assert np.array_equal(i, want), (labels, n, k)


def test_a_gallery_without_identities_is_the_plain_search_plus_minus_one(rfd, gal):
    dim, rows = 64, 333
    q, g, planted = _dyadic_case(dim, rows, 33, 4200)
    ga = gal(dim, rows)
    _add_in_pieces(ga, g)
    for gone in ([], [2, 63]):
        assert ga.remove(gone) == 0
        for n, k in NK:
            st, ps, pr = ga.search(q[:n], k)
            st2, s, r, i = _search_ids(ga, q[:n], k)
            assert st == 0 and st2 == 0 and np.array_equal(r, pr) and np.array_equal(_bits(s), _bits(ps)) and np.all(i == -1)
    assert _labelled(ga) == 0 and np.all(_get_ids(ga, 0, rows)[1] == -1)


# ---- 6. at most r rows per identity and k r <= 32: the host-deduplicated plain search is the judge ----
@pytest.mark.parametrize("r_per,k", [(4, 8), (2, 5), (1, 32)])
def test_equals_the_host_deduplicated_plain_search(rfd, gal, r_per, k):
    dim, rows, n = 96, 1000, 33
    assert k * r_per <= 32
    q, g, planted = _dyadic_case(dim, rows, n, 4300 + k)
    ids = np.random.default_rng(k).permutation(np.arange(rows) // r_per)   # every identity has at most r_per rows, anywhere
    if r_per > 1:                                                           # query 0's planted rows 2 and 63 share an identity
        partner = next(int(p) for p in np.flatnonzero(ids == ids[2]) if p != 2)
        ids[[partner, 63]] = ids[[63, partner]]
        assert ids[2] == ids[63] and planted[:2] == [2, 63]
    assert np.bincount(ids).max() <= r_per
    ga = gal(dim, rows)
    _add_in_pieces(ga, g)
    assert _set_ids(ga, np.arange(rows), ids) == 0
    st, ps, pr = ga.search(q, k * r_per)
    st2, s, r, i = _search_ids(ga, q, k)
    assert st == 0 and st2 == 0
    folded = 0
    for a in range(n):
        seen, keep = set(), []
        for col, row in enumerate(pr[a]):
            if ids[row] not in seen:
                seen.add(ids[row])
                keep.append(col)
        folded += len(keep) < k * r_per
        assert len(keep) >= k                                               # k r rows hold at least k identities
        keep = keep[:k]
        assert np.array_equal(r[a], pr[a, keep]) and np.array_equal(_bits(s[a]), _bits(ps[a, keep])) and np.array_equal(i[a], ids[pr[a, keep]])
    assert folded > 0 or r_per == 1                                         # some query had one identity twice among its best rows


# ---- 7. with removals ----
def test_removals_promote_drop_and_unlabel(rfd, gal):
    dim, rows, k = 64, 200, 6
    q, g, planted = _dyadic_case(dim, rows, 33, 4400)
    _unplant(g, planted)
    _plant(g, q[0], [10, 90, 170, 30, 31], [0, 1, 2, 3, 4])                 # identity 3: rows 10, 90, 170; then rows 30 (id 4), 31 (-1)
    ids = 50 + np.arange(rows) % 20
    ids[[10, 90, 170, 30, 31]] = [3, 3, 3, 4, -1]
    full = R.scores(q, g)
    _exact(full)
    ga = gal(dim, rows)
    _add_in_pieces(ga, g)
    lab = np.flatnonzero(ids >= 0)
    assert _set_ids(ga, lab, ids[lab]) == 0
    ids, live = ids.copy(), np.ones(rows, bool)

    def step(tag, first_rows, first_ids):
        for n in (1, 33):
            s, r, i = _check(ga, q, full, ids, live, n, k, tag)
        assert r[0].tolist()[:len(first_rows)] == first_rows and i[0].tolist()[:len(first_ids)] == first_ids, tag
        st, got = _get_ids(ga, 0, len(ids))
        assert st == 0 and np.array_equal(got, ids), tag
        assert _labelled(ga) == I.labelled(ids, live), tag
        assert ga.live() == int(live.sum()), tag

    def remove(gone):
        assert ga.remove(gone) == 0
        live[gone] = False
        ids[gone] = -1                                                      # nothing of an erased enrolment stays

    step("all live", [10, 30, 31], [3, 4, -1])
    remove([10])
    step("the best row of identity 3 removed: its next row moves up", [90, 30, 31], [3, 4, -1])
    remove([90, 170, 90])
    step("all rows of identity 3 removed: the identity is gone", [30, 31], [4, -1])
    assert 3 not in _search_ids(ga, q[:1], 32)[3]
    # a reused hole is unlabelled; replace of a live row keeps its identity
    new = g[[10, 30]].copy()
    assert ga.replace([10, 30], new) == 0
    live[[10, 30]] = True
    step("row 10 revived", [10, 30, 31], [-1, 4, -1])
    assert _set_ids(ga, [10], [3]) == 0
    ids[10] = 3
    step("and labelled again", [10, 30, 31], [3, 4, -1])
    assert ga.L.rfd_gallery_clear(ga.g) == 0 and _labelled(ga) == 0
    assert ga.add(g[:50]) == (0, 0) and np.all(_get_ids(ga, 0, 50)[1] == -1)
    ids, live = np.full(50, -1), np.ones(50, bool)
    full = full[:, :50]
    step("after clear every row is unlabelled, in HBM too", [10, 30, 31], [-1, -1, -1])


# ---- 8. the capped grid ----
def test_one_identity_in_strided_blocks_of_one_waves_walk(rfd, gal):
    cus = _cus()
    stride, nblocks, rows, q, g, planted, full, top33 = _capped_case(cus)
    groups, st2 = _groups(rows, cus)
    assert -(-nblocks // (WAVES * 2)) > 2 * cus == groups and st2 == stride    # the cap on workgroups binds
    walk = [4 + i * stride for i in range(4)]                              # wave 4's blocks; the last is the gallery's partial last block
    assert walk[-1] == nblocks - 1 and rows % 16 != 0
    blk = np.arange(rows) >> 4
    ids = 2 + blk % 97                                                      # every other identity: whole blocks, spread over many waves
    ids[np.isin(blk, walk)] = 1                                             # identity 1: every row of the one walk
    ids[::5] = np.where(ids[::5] == 1, 1, -1)
    assert 64 in planted and rows - 1 in planted and ids[64] == 1 == ids[rows - 1] and (64 >> 4) == walk[0] and ((rows - 1) >> 4) == walk[-1]
    assert full[0, 64] == full[0, rows - 1] == full[0].max()               # the identity's two best keys tie: first and last block of the walk
    ga = gal(32, rows)
    _add_in_pieces(ga, g)
    lab = np.flatnonzero(ids >= 0)
    for at in range(0, len(lab), 30000):                                    # lists longer than one chunk of the call
        assert _set_ids(ga, lab[at:at + 30000], ids[lab][at:at + 30000]) == 0
    assert _labelled(ga) == len(lab)
    for n, k in ((33, 32), (1, 5)):
        s, r, i = _check(ga, q, full, ids, None, n, k, (n, k))
        assert 64 in r[0].tolist() and rows - 1 not in r[0].tolist() and i[0].tolist().count(1) == 1


# ---- 9. min_score ----
def test_min_score(rfd, gal):
    dim, rows, n, k = 64, 333, 33, 8
    q, g, _ = _dyadic_case(dim, rows, n, 4500)
    ids = np.arange(rows) % 60
    full = R.scores(q, g)
    _exact(full)
    ga = gal(dim, rows)
    _add_in_pieces(ga, g)
    assert _set_ids(ga, np.arange(rows), ids) == 0
    s0, r0, i0 = _check(ga, q, full, ids, None, n, k, "-inf")
    assert np.all(r0 >= 0)
    a = next(j for j in range(k - 1) if s0[1, j] > s0[1, j + 1])           # two neighbours of query 1 with different scores
    equal, between, above = float(s0[1, a]), float((np.float64(s0[1, a]) + np.float64(s0[1, a + 1])) / 2), float(full.max()) + 1.0
    assert s0[1, a + 1] < np.float32(between) < s0[1, a]
    s, r, i = _check(ga, q, full, ids, None, n, k, "equal", equal)
    assert r[1, a] == r0[1, a] and np.all(r[1, a + 1:] == -1) and np.all(np.isneginf(s[1, a + 1:])) and np.all(i[1, a + 1:] == -1)
    s, r, i = _check(ga, q, full, ids, None, n, k, "between", between)
    assert r[1, a] == r0[1, a] and r[1, a + 1] == -1
    kept = s0 >= np.float32(between)
    assert 0 < kept.sum() < kept.size and np.array_equal(r >= 0, kept)      # a suffix of each query's entries went
    s, r, i = _check(ga, q, full, ids, None, n, k, "above", above)
    assert np.all(r == -1) and np.all(i == -1) and np.all(np.isneginf(s))
    st, s, r, i = _search_ids(ga, q, k, float("nan"))
    assert st == rfd.RFD_ERR_INVALID_ARG and "min_score" in ga.err() and np.all(r == -7)


# ---- 10. stream order ----
def test_device_calls_run_in_stream_order_without_host_waits(rfd, det, gal):
    import torch
    L, dim, rows, n, k = rfd.load_library(), 64, 700, 33, 6
    dev = torch.device("cuda", 0)
    q, g, _ = _dyadic_case(dim, rows, n, 4600)
    ids = np.arange(rows) % 25
    gone = np.array([0, 3, 16, 350, 699, 3], np.int32)
    d_g = torch.from_numpy(g.astype(np.float32)).to(dev)
    d_q = torch.from_numpy(q.astype(np.float32)).to(dev)
    d_s = torch.full((n, k), 7.0, device=dev)
    d_r = torch.full((n, k), -7, dtype=torch.int32, device=dev)
    d_i = torch.full((n, k), -7, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    gd = gal(dim, rows)
    first = C.c_int(-1)
    all_rows, all_ids = _i32(np.arange(rows)), _i32(ids)
    assert L.rfd_gallery_add_device(gd.g, d_g.data_ptr(), rows, C.byref(first)) == 0 and first.value == 0
    assert L.rfd_gallery_set_identities(gd.g, all_rows.ctypes.data, all_ids.ctypes.data, rows) == 0
    assert L.rfd_gallery_remove(gd.g, gone.ctypes.data, len(gone)) == 0
    assert L.rfd_gallery_search_identities_device(gd.g, d_q.data_ptr(), n, k, NEG_INF, d_s.data_ptr(), d_r.data_ptr(), d_i.data_ptr(), 1) == 0
    assert L.rfd_sync(det._ctx) == 0
    s, r, i = d_s.cpu().numpy(), d_r.cpu().numpy(), d_i.cpu().numpy()
    gh = gal(dim, rows)                                                     # the synchronous host-form sequence
    assert gh.add(g) == (0, 0) and _set_ids(gh, np.arange(rows), ids) == 0 and gh.remove(gone) == 0
    st, hs, hr, hi = _search_ids(gh, q, k)
    assert st == 0 and np.array_equal(r, hr) and np.array_equal(i, hi) and np.array_equal(_bits(s), _bits(hs))
    live = np.ones(rows, bool)
    live[gone] = False
    ref = I.topk_of_scores(R.scores(q, g), ids, k, NEG_INF, live)
    assert np.array_equal(r, ref[1]) and np.array_equal(i, ref[2]) and np.array_equal(_bits(s), _bits(ref[0]))
    assert np.array_equal(_get_ids(gd, 0, rows)[1], np.where(live, ids, -1)) and _labelled(gd) == rows - 5


# ---- 11. non-finite values of the device forms ----
def test_non_finite_scores_of_labelled_rows_are_never_selected(rfd, det, gal):
    import torch
    L, dim, rows, nq, k = rfd.load_library(), 64, 50, 20, 32
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(17)
    g = rng.integers(-8, 9, (rows, dim)).astype(np.float64) / 64
    q = rng.integers(-8, 9, (nq, dim)).astype(np.float64) / 64
    q[:, 0], q[:, 9] = 5 / 64, 3 / 64
    finite_g = g.copy()
    nan_rows, ninf_rows = [5, 16, 31], [0, 20, 33]
    g[nan_rows, 9] = np.nan
    g[ninf_rows, 0] = -np.inf
    ids = np.arange(rows) % 6                                               # every identity has hostile rows and others
    ids[[7, 8]] = -1
    assert all(len(set(np.flatnonzero(ids == c).tolist()) - set(nan_rows + ninf_rows)) >= 1 for c in range(6))
    assert {int(ids[r]) for r in nan_rows + ninf_rows} >= {0, 2, 3, 4, 5}
    assert np.array_equal(R.rne_bf16(finite_g), finite_g) and np.array_equal(R.rne_bf16(q), q)
    assert float((np.abs(q) @ np.abs(finite_g).T).max()) * 2.0 ** 12 < 2.0 ** 24
    with np.errstate(invalid="ignore"):
        full = (q[:, None, :] * g[None, :, :]).sum(-1)
    assert np.isnan(full[:, nan_rows]).all() and np.isneginf(full[:, ninf_rows]).all()
    d_g = torch.from_numpy(g.astype(np.float32)).to(dev)
    d_q = torch.from_numpy(q.astype(np.float32)).to(dev)
    torch.cuda.synchronize()
    ga = gal(dim, rows)
    first = C.c_int(-1)
    assert L.rfd_gallery_add_device(ga.g, d_g.data_ptr(), rows, C.byref(first)) == 0
    lab = np.flatnonzero(ids >= 0)
    assert _set_ids(ga, lab, ids[lab]) == 0
    live = np.ones(rows, bool)
    for gone in ([], [2]):
        assert ga.remove(gone) == 0
        live[gone] = False
        ref_s, ref_r, ref_i = I.topk_of_scores(full, ids, k, NEG_INF, live)
        for n in (nq, 5):
            d_s = torch.full((n, k), 7.0, device=dev)
            d_r = torch.full((n, k), -7, dtype=torch.int32, device=dev)
            d_i = torch.full((n, k), -7, dtype=torch.int32, device=dev)
            torch.cuda.synchronize()
            assert L.rfd_gallery_search_identities_device(ga.g, d_q.data_ptr(), n, k, NEG_INF, d_s.data_ptr(), d_r.data_ptr(), d_i.data_ptr(), 0) == 0
            s, r, i = d_s.cpu().numpy(), d_r.cpu().numpy(), d_i.cpu().numpy()
            assert np.array_equal(r, ref_r[:n]) and np.array_equal(i, ref_i[:n]) and np.array_equal(_bits(s), _bits(ref_s[:n]))
            assert not np.isin(r, nan_rows + ninf_rows).any()
            assert all(set(i[a][r[a] >= 0].tolist()) == {-1, 0, 1, 2, 3, 4, 5} for a in range(n))   # their other rows still count
            assert np.all(r[:, 8:] == -1)                                   # six identities and two unlabelled rows: the tail is empty


# ---- 12. errors ----
def test_error_rules(rfd, gal):
    dim, rows, k = 32, 100, 5
    q, g, _ = _dyadic_case(dim, rows, 3, 4700)
    ga = gal(dim, rows + 5)
    _add_in_pieces(ga, g)
    ids = np.arange(rows) % 7
    assert _set_ids(ga, np.arange(rows), ids) == 0 and ga.remove([40]) == 0
    ids[40] = -1
    before = _search_ids(ga, q, k)

    def unchanged(tag):
        now = _search_ids(ga, q, k)
        assert now[0] == 0 and all(np.array_equal(x, y) for x, y in zip(before[1:], now[1:])), tag
        assert np.array_equal(_get_ids(ga, 0, rows)[1], ids) and _labelled(ga) == I.labelled(ids), tag

    bad = rfd.RFD_ERR_INVALID_ARG
    assert _set_ids(ga, [1, rows], [9, 9]) == bad and "rows[1] = %d" % rows in ga.err()
    unchanged("a row beyond the gallery")
    assert _set_ids(ga, [1, -1], [9, 9]) == bad and "rows[1] = -1" in ga.err()
    unchanged("a negative row")
    assert _set_ids(ga, [1, 40], [9, 9]) == bad and "rows[1] = 40" in ga.err() and "removed" in ga.err()
    unchanged("a removed row")
    assert _set_ids(ga, [1, 2, 1], [9, 9, 9]) == bad and "row 1 " in ga.err() and "more than once" in ga.err()
    unchanged("a row listed twice")
    assert _set_ids(ga, [1, 2], [9, -2]) == bad and "ids[1] = -2" in ga.err()
    unchanged("an invalid identity")
    assert _set_ids(ga, [], []) == 0
    unchanged("n = 0")
    assert _get_ids(ga, rows - 1, 2)[0] == bad and _get_ids(ga, -1, 1)[0] == bad
    st, s, r, i = _search_ids(ga, q, 0)
    assert st == bad
    assert _search_ids(ga, q, 33)[0] == rfd.RFD_ERR_CAPACITY and "RFD_GALLERY_MAX_K" in ga.err()
    assert _search_ids(ga, q[:0], k)[0] == 0
    # unlabelling by RFD_GALLERY_NO_IDENTITY is a valid call
    assert _set_ids(ga, [1], [rfd.NO_IDENTITY]) == 0
    ids[1] = -1
    full = R.scores(q, g)
    live = np.ones(rows, bool)
    live[40] = False
    _check(ga, q, full, ids, live, 3, k, "after unlabelling row 1")
    assert _labelled(ga) == I.labelled(ids, live)
