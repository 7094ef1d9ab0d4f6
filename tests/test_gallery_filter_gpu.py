"""The gallery's tags and filtered search (include/rfd.h, "tags"; csrc/kernels_gallery.hip, the TAGGED scan) through the C ABI,
against tests/gallery_filter_ref.py.  The data are dyadic, so every score is exact in f32 in any summation order (asserted on the
CPU first) and every comparison is bit for bit.  A query's result depends on neither n nor k beyond its own prefix, so every
case computes its reference once, for all its queries at k = 32, and compares slices of it."""
import ctypes as C

import numpy as np
import pytest

import gallery_filter_ref as F
import gallery_ref as R
from test_gallery_gpu import _bits, _dyadic_case, det  # noqa: F401  (det: the module's detector fixture)
from test_gallery_edit_gpu import EditGal, gal  # noqa: F401  (gal: makes EditGal galleries)
from test_gallery_adversarial_gpu import WAVES, _add_in_pieces, _capped_case
from test_gallery_identity_gpu import _cus, _exact, _groups, _plant, _search_ids, _set_ids, _unplant

pytestmark = pytest.mark.gpu

NEG_INF = float("-inf")
ALL = F.ALL


# ---- the calls of this file on an EditGal (statuses returned, not raised) ----
def _u32(x):
    return np.ascontiguousarray(np.asarray(x, np.int64).reshape(-1) & ALL, np.uint32)


def _i32(x):
    return np.ascontiguousarray(np.asarray(x, np.int64).reshape(-1), np.int32)


def _set_tags(ga, rows, tags):
    r, t = _i32(rows), _u32(tags)
    assert r.shape == t.shape
    return ga.L.rfd_gallery_set_tags(ga.g, r.ctypes.data, t.ctypes.data, r.shape[0])


def _get_tags(ga, row0, n):
    out = np.full(max(n, 1), 0xABCDABCD, np.uint32)
    return ga.L.rfd_gallery_get_tags(ga.g, row0, n, out.ctypes.data), out[:n]


def _search(ga, q, k, mask, value, min_score=NEG_INF):
    q = np.ascontiguousarray(q, np.float32).reshape(-1, ga.dim)
    m, v = _u32(mask), _u32(value)
    assert m.shape == v.shape == (q.shape[0],)
    shape = (q.shape[0], max(k, 1))
    s, r, i = np.full(shape, 7.0, np.float32), np.full(shape, -7, np.int32), np.full(shape, -7, np.int32)
    st = ga.L.rfd_gallery_search_filtered(ga.g, q.ctypes.data, q.shape[0], k, min_score, m.ctypes.data, v.ctypes.data, s.ctypes.data, r.ctypes.data,
                                          i.ctypes.data)
    return st, s, r, i


def _reference(full, ids, tags, mask, value, live=None, min_score=NEG_INF):
    """the reference of every query at k = 32; read-only"""
    ref = F.topk_of_scores(full, np.full(full.shape[1], -1) if ids is None else ids, tags, mask, value, 32, min_score, live)
    for a in ref:
        a.setflags(write=False)
    return ref


def _check(ga, q, ref, mask, value, n, k, tag, min_score=NEG_INF):
    """the filtered search of q[:n] equals the first n queries and k entries of the reference, bit for bit"""
    st, s, r, i = _search(ga, q[:n], k, mask[:n], value[:n], min_score)
    assert st == 0, (tag, ga.err())
    assert np.array_equal(r, ref[1][:n, :k]), tag
    assert np.array_equal(i, ref[2][:n, :k]), tag
    assert np.array_equal(_bits(s), _bits(ref[0][:n, :k])), tag
    return s, r, i


TAG_SET = np.array([0, 1, 2, 3, 0x80000001, 0xFFFFFFFF], np.int64)
# per query, in turn: everything; partitions 1, 0, 2; list bit 0; the top bit; a value outside its mask; a partition nobody is in;
# list bit 1 with the top bit clear
FILTERS = [(0, 0), (ALL, 1), (ALL, 0), (ALL, 2), (1, 1), (0x80000000, 0x80000000), (0xF, 0x10), (ALL, 0x12345678), (0x80000002, 2)]


def _filters(n, shift=0):
    f = [FILTERS[(a + shift) % len(FILTERS)] for a in range(n)]
    return np.array([m for m, v in f], np.int64), np.array([v for m, v in f], np.int64)


def _tags(rows, seed):
    return TAG_SET[np.random.default_rng(seed).integers(0, len(TAG_SET), rows)]


# ---- 1. geometry ----
@pytest.mark.parametrize("rows", [1, 15, 16, 17, 100, 129, 1000])
@pytest.mark.parametrize("dim", [32, 96, 256, 512])
def test_geometry_sweep(rfd, gal, dim, rows):
    """K-step counts 1, 3, 8, 16 against the prefetch depth of 8; a partial last block, a wave without a block, the second
    workgroup (129 rows: 9 blocks); both M-tile counts and several passes; a different filter for every query of a pass"""
    assert _groups(129, _cus())[0] == 2 and _groups(100, _cus())[0] == 1
    nq = 70
    q, g, planted = _dyadic_case(dim, rows, nq, 7000 + dim + rows)
    tags = _tags(rows, dim + rows)
    mask, value = _filters(nq, rows)
    full = R.scores(q, g)
    _exact(full)
    el = F.eligible(tags, mask, value)
    assert el[(0 - rows) % len(FILTERS)].all() and not el[(6 - rows) % len(FILTERS)].any() and not el[(7 - rows) % len(FILTERS)].any()
    ref = _reference(full, None, tags, mask, value)
    ga = gal(dim, rows + 3)
    _add_in_pieces(ga, g)
    assert _set_tags(ga, np.arange(rows), tags) == 0
    for n in (1, 16, 17, 32, 33, 70):
        for k in (1, 5, 32):
            s, r, i = _check(ga, q, ref, mask, value, n, k, (dim, rows, n, k))
            assert np.all(i == -1)                                          # no identities: the filtered row search
    if rows >= 100:
        assert (ref[1][:, 0] >= 0).sum() >= nq // 2 and (ref[1][:, 0] < 0).sum() >= 2 * (nq // len(FILTERS))


# ---- 2. every bit of the word ----
def test_every_bit_of_the_word(rfd, gal):
    dim, rows = 32, 34
    q, g, _ = _dyadic_case(dim, rows, 34, 7100)
    tags = np.array([1 << b for b in range(32)] + [0x80000000, 0xFFFFFFFF], np.int64)
    full = R.scores(q, g)
    _exact(full)
    ga = gal(dim, rows)
    _add_in_pieces(ga, g)
    assert _set_tags(ga, np.arange(rows), tags) == 0
    assert np.array_equal(_get_tags(ga, 0, rows)[1], tags.astype(np.uint32))
    bit = np.array([1 << b for b in range(32)], np.int64)
    st, s, r, i = _search(ga, q[:32], 4, bit, bit)                          # list b: row b and row 33 (all bits); row 32 too for bit 31
    assert st == 0
    for b in range(32):
        assert set(r[b][r[b] >= 0].tolist()) == {b, 33} | ({32} if b == 31 else set()), b
    tags[33] = 0
    assert _set_tags(ga, [33], [0]) == 0
    ref = _reference(full[:32], None, tags, bit, bit)
    s, r, i = _check(ga, q, ref, bit, bit, 32, 4, "one row per bit")
    assert r[:31, 0].tolist() == list(range(31)) and np.all(r[:31, 1:] == -1) and sorted(r[31, :2].tolist()) == [31, 32]
    # equality on the whole word
    tags[33] = 0xFFFFFFFF
    assert _set_tags(ga, [33], [0xFFFFFFFF]) == 0
    mask, value = np.full(4, ALL), np.array([0x80000000, 0xFFFFFFFF, 0x7FFFFFFF, 0])
    ref = _reference(full[:4], None, tags, mask, value)
    s, r, i = _check(ga, q, ref, mask, value, 4, 3, "whole word")
    assert sorted(r[0, :2].tolist()) == [31, 32] and r[0, 2] == -1 and r[1].tolist() == [33, -1, -1] and np.all(r[2:] == -1)


# ---- 3. ineligible rows never count ----
@pytest.mark.parametrize("k", [5, 32])
def test_ineligible_rows_with_the_best_scores_never_count(rfd, gal, k):
    dim, rows = 32, 300
    groups, stride = _groups(rows, _cus())
    assert groups == 3 and stride == 12 and rows > 16 * stride              # wave 0 of workgroup 0 walks blocks 0 and 12
    q, g, planted = _dyadic_case(dim, rows, 33, 7200)
    _unplant(g, planted)
    q[1] = q[2] = q[0]                                                      # the same vector under other filters
    # ineligible for query 0, the best scores of the gallery: the same block (rows 3, 5), the same wave's next block (195),
    # another wave of the workgroup (block 1: row 20), another workgroup (block 4: row 70)
    strong = [3, 5, 195, 20, 70]
    assert [r >> 4 for r in strong] == [0, 0, stride, 1, WAVES] and (195 >> 4) % stride == 0
    _plant(g, q[0], strong, [0, 0, 0, 1, 1])
    weak = [4, 6, 196, 21, 71, 250]                                          # eligible, beside them, weaker
    _plant(g, q[0], weak, [3, 4, 3, 5, 4, 6])
    tags = np.full(rows, 9, np.int64)
    tags[strong] = 1
    tags[weak] = 2
    full = R.scores(q, g)
    _exact(full)
    assert full[0, strong].min() > full[0, weak].max() and full[0, weak].min() > np.delete(full[0], strong + weak).max()
    mask, value = np.full(33, ALL), np.full(33, 9)
    mask[:3], value[:3] = [ALL, ALL, 3], [2, 1, 2]                           # query 2: tag & 3 == 2, the weak rows again
    ref = _reference(full, None, tags, mask, value)
    ga = gal(dim, rows)
    _add_in_pieces(ga, g)
    assert _set_tags(ga, np.arange(rows), tags) == 0
    for n in (1, 3, 33):
        s, r, i = _check(ga, q, ref, mask, value, n, k, (k, n))
        assert r[0].tolist()[:6] == [4, 196, 6, 71, 21, 250][:k] and not np.isin(r[0], strong).any()
        assert np.all(r[0, 6:] == -1) and np.all(np.isneginf(s[0, 6:]))      # k larger than the eligible rows: the tail is empty
        if n >= 3:
            assert r[1].tolist()[:5] == [3, 5, 195, 20, 70][:k] and np.all(r[1, 5:] == -1)
            assert np.array_equal(r[2], r[0]) and np.array_equal(_bits(s[2]), _bits(s[0]))


# ---- 4. sparse tenants: the lists never fill ----
@pytest.mark.parametrize("every", [64, 0])
def test_sparse_tenant(rfd, gal, every):
    dim, rows, n, k = 32, 4099, 33, 5
    q, g, planted = _dyadic_case(dim, rows, n, 7300)
    tags = np.zeros(rows, np.int64)
    if every:
        tags[5::every] = 0xC0000001                                         # one eligible row per 64
    else:
        tags[2111] = 0xC0000001                                             # one in the whole gallery
    members = np.flatnonzero(tags == 0xC0000001)
    assert len(members) == (64 if every else 1)
    mask, value = np.full(n, ALL), np.full(n, 0xC0000001)
    mask[5], value[5] = 0, 0                                                # one query of the pass sees everybody
    full = R.scores(q, g)
    _exact(full)
    ref = _reference(full, None, tags, mask, value)
    ga = gal(dim, rows)
    _add_in_pieces(ga, g)
    assert _set_tags(ga, members, tags[members]) == 0
    for nn in (1, n):
        s, r, i = _check(ga, q, ref, mask, value, nn, k, (every, nn))
        assert np.isin(r[0][r[0] >= 0], members).all() and (r[0] >= 0).sum() == min(k, len(members))
    assert not np.isin(r[5], members).all() and np.all(r[5] >= 0)


# ---- 5. removed rows (MASKED) x identities (IDENT) under the filter ----
@pytest.mark.parametrize("with_ids", [False, True])
@pytest.mark.parametrize("with_removed", [False, True])
def test_removed_rows_and_identities_under_the_filter(rfd, gal, with_removed, with_ids):
    dim, rows, nq = 64, 500, 33
    q, g, planted = _dyadic_case(dim, rows, nq, 7400)
    _unplant(g, planted)
    q[1] = q[0]
    # identity 3: its best row 10 has tag 1, its weaker row 90 tag 2.  identity 4: rows 30 and 170, both tag 1.  Row 31: unlabelled, tag 2
    _plant(g, q[0], [10, 90, 30, 170, 31, 400], [0, 2, 1, 1, 3, 4])
    ids = 50 + np.arange(rows) % 20
    ids[::9] = -1
    ids[[10, 90, 30, 170, 31, 400]] = [3, 3, 4, 4, -1, 5]
    tags = 1 + np.arange(rows) % 2
    tags[[10, 90, 30, 170, 31, 400]] = [1, 2, 1, 1, 2, 2]
    gone = [170, 400, 7, 499] if with_removed else []
    live = np.ones(rows, bool)
    live[gone] = False
    mask, value = _filters(nq)
    mask[:2], value[:2] = [ALL, ALL], [2, 1]
    full = R.scores(q, g)
    _exact(full)
    ga = gal(dim, rows)
    _add_in_pieces(ga, g)
    assert _set_tags(ga, np.arange(rows), tags) == 0
    if with_ids:
        lab = np.flatnonzero(ids >= 0)
        assert _set_ids(ga, lab, ids[lab]) == 0
    assert ga.remove(gone) == 0
    tags = np.where(live, tags, 0)
    ref = _reference(full, ids if with_ids else None, tags, mask, value, live)
    for n, k in ((1, 5), (17, 32), (33, 5), (16, 1)):
        s, r, i = _check(ga, q, ref, mask, value, n, k, (with_removed, with_ids, n, k))
    s, r, i = _check(ga, q, ref, mask, value, 2, 5, "the two planted queries")
    if with_ids:
        # for query 0 identity 3 is represented by its best ELIGIBLE row 90 and identity 4 is absent; for query 1, the next
        # query of the same pass, identity 3 has row 10 and identity 4 its best live row
        assert r[0].tolist()[:2] == [90, 31] and i[0].tolist()[:2] == [3, -1] and 4 not in i[0].tolist()
        assert r[1].tolist()[:2] == [10, 30] and i[1].tolist()[:2] == [3, 4] and i[1].tolist().count(4) == 1
        assert (5 in i[0].tolist()) == (not with_removed)
    else:
        assert r[0].tolist()[:2] == [90, 31] and r[1].tolist()[:2] == [10, 30] and (r[1, 2] == 170) == (not with_removed)
        assert np.all(i == -1)
    assert not np.isin(r, gone).any() or not with_removed


# ---- 6. the largest LDS footprint ----
def test_the_largest_lds_footprint(rfd, gal):
    dim, rows, n, k = 1024, 1000, 32, 32
    lds = 2 * 16 * dim * 2 + WAVES * 32 * k * (8 + 4) + 32 * 8                 # fragments, keys and identities, the pairs
    assert lds == 112 * 1024 + 256
    q, g, planted = _dyadic_case(dim, rows, n, 7500)
    ids = np.arange(rows) % 300
    tags = _tags(rows, 75)
    mask, value = _filters(n, 1)
    full = R.scores(q, g)
    _exact(full)
    ga = gal(dim, rows)
    _add_in_pieces(ga, g)
    assert _set_ids(ga, np.arange(rows), ids) == 0 and _set_tags(ga, np.arange(rows), tags) == 0
    _check(ga, q, _reference(full, ids, tags, mask, value), mask, value, n, k, "unmasked")
    gone = [5, 63, 640, 999]
    assert ga.remove(gone) == 0
    live = np.ones(rows, bool)
    live[gone] = False
    _check(ga, q, _reference(full, np.where(live, ids, -1), np.where(live, tags, 0), mask, value, live), mask, value, n, k, "masked")


# ---- 7. the capped grid ----
def test_the_capped_grid(rfd, gal):
    cus = _cus()
    stride, nblocks, rows, q, g, planted, full, top33 = _capped_case(cus)
    groups, st2 = _groups(rows, cus)
    assert -(-nblocks // (WAVES * 2)) > 2 * cus == groups and st2 == stride    # the cap on workgroups binds
    blk = np.arange(rows) >> 4
    tags = (blk % 5).astype(np.int64)                                        # whole blocks: a wave meets blocks with nothing eligible
    tags[planted] = [1, 2, 1, 2, 1, 2][:len(planted)]
    tags[rows - 1] = 1                                                       # the gallery's partial last block, the end of wave 4's walk
    assert 64 in planted and rows - 1 in planted and full[0, 64] == full[0, rows - 1] == full[0].max()
    n = 33
    mask, value = np.full(n, ALL), np.arange(n) % 6                           # partition 5 is empty
    mask[7], value[7] = 0, 0
    value[0] = 1                                                             # query 0, whose best rows are the planted ones: partition 1
    ref = _reference(full, None, tags, mask, value)
    ga = gal(32, rows)
    _add_in_pieces(ga, g)
    every = np.arange(rows)
    for at in range(0, rows, 30000):                                         # lists longer than one chunk of the call
        assert _set_tags(ga, every[at:at + 30000], tags[at:at + 30000]) == 0
    for nn, k in ((33, 32), (2, 5)):
        s, r, i = _check(ga, q, ref, mask, value, nn, k, (nn, k))
        assert np.all(tags[r[0]] == 1) and r[0].tolist()[:4] == [2, 64, 2112, rows - 1]   # equal scores: first and last block of wave 4's walk
    assert np.all(ref[1][5] == -1) and np.all(ref[1][7] >= 0)


# ---- 8. no filter is the identity search ----
def test_mask_and_value_zero_equal_the_identity_search(rfd, gal):
    dim, rows = 96, 1500
    q, g, planted = _dyadic_case(dim, rows, 33, 7600)
    ga = gal(dim, rows)
    _add_in_pieces(ga, g)
    zero = np.zeros(33, np.int64)

    def same(tag):
        for n, k in ((1, 1), (16, 32), (17, 5), (33, 32)):
            st, s, r, i = _search(ga, q[:n], k, zero[:n], zero[:n])
            st2, s2, r2, i2 = _search_ids(ga, q[:n], k)
            assert st == 0 and st2 == 0 and np.array_equal(r, r2) and np.array_equal(i, i2) and np.array_equal(_bits(s), _bits(s2)), (tag, n, k)
        return r, i
    r, i = same("before any tag, without identities")
    assert np.all(i == -1) and np.all(r >= 0)
    assert _set_tags(ga, np.arange(rows), _tags(rows, 76)) == 0
    same("tags set")
    assert _set_ids(ga, np.arange(rows), np.arange(rows) % 200) == 0
    r, i = same("identities set")
    assert np.all(i >= 0)
    assert ga.remove([2, 63, 64, 1499]) == 0
    same("rows removed")
    st, s, r, i = _search(ga, q, 5, zero, zero, 0.25)
    st2, s2, r2, i2 = _search_ids(ga, q, 5, 0.25)
    assert st == 0 and np.array_equal(r, r2) and np.array_equal(i, i2) and np.array_equal(_bits(s), _bits(s2)) and (r < 0).any() and (r >= 0).any()


# ---- 9. before any tag is set ----
def test_a_filtered_search_before_any_tag_is_set(rfd, gal):
    dim, rows, n, k = 64, 333, 33, 6
    q, g, _ = _dyadic_case(dim, rows, n, 7700)
    full = R.scores(q, g)
    _exact(full)
    ga = gal(dim, rows)
    _add_in_pieces(ga, g)
    assert np.all(_get_tags(ga, 0, rows)[1] == 0)
    mask, value = _filters(n)
    ref = _reference(full, None, np.zeros(rows, np.int64), mask, value)     # every row has tag 0
    s, r, i = _check(ga, q, ref, mask, value, n, k, "untagged")
    el = F.eligible(np.zeros(rows, np.int64), mask, value)
    assert np.array_equal(r[:, 0] >= 0, el.any(1)) and el.any(1).sum() in range(3, n)
    assert ga.remove([1]) == 0                                               # the array exists now: a remove zeroes through it
    live = np.ones(rows, bool)
    live[1] = False
    _check(ga, q, _reference(full, None, np.zeros(rows, np.int64), mask, value, live), mask, value, n, k, "untagged, one row removed")


# ---- 10. life cycle ----
def test_life_cycle(rfd, det, gal, tmp_path):
    dim, rows, n, k = 64, 200, 17, 8
    q, g, planted = _dyadic_case(dim, rows, n, 7800)
    _unplant(g, planted)
    _plant(g, q[0], [10, 90, 30], [0, 1, 2])
    full = R.scores(q, g)
    _exact(full)
    mask, value = np.full(n, ALL), np.arange(n) % 3
    mask[0], value[0] = ALL, 2
    tags, live = np.zeros(rows, np.int64), np.ones(rows, bool)
    ga = gal(dim, rows)
    _add_in_pieces(ga, g)

    def step(tag, first_rows):
        st, got = _get_tags(ga, 0, len(tags))
        assert st == 0 and np.array_equal(got, tags.astype(np.uint32)), tag
        s, r, i = _check(ga, q, _reference(full[:, :len(tags)], None, tags, mask, value, live), mask, value, n, k, tag)
        assert r[0].tolist()[:len(first_rows)] == first_rows, tag
        assert not np.isin(r, np.flatnonzero(~live)).any(), tag

    step("after add every tag is 0", [])
    assert np.all(_search(ga, q[:1], k, [ALL], [2])[2] == -1)
    tags[:] = np.arange(rows) % 3
    tags[[10, 90, 30]] = 2
    assert _set_tags(ga, np.arange(rows), tags) == 0
    step("set", [10, 90, 30])
    assert ga.remove([10, 11, 10]) == 0
    live[[10, 11]] = False
    tags[[10, 11]] = 0
    step("removed: the tag reads 0 and the row is never returned", [90, 30])
    assert ga.replace([10, 30], g[[10, 30]]) == 0
    live[10] = True
    step("replaced: a reused hole has tag 0, a corrected enrolment keeps its tag", [90, 30])
    zero_q = _search(ga, q[:1], 1, [ALL], [0])
    assert zero_q[0] == 0 and zero_q[2][0, 0] == 10                          # eligible only for queries that match 0
    tags[10] = 0x80000002
    assert _set_tags(ga, [10], [0x80000002]) == 0
    mask[0], value[0] = 3, 2
    step("set again", [10, 90, 30])
    # save / load: the file has no tags
    path = tmp_path / "tagged.rfdg"
    assert ga.save(path) == 0
    back = EditGal.load(rfd, det, path)
    gal.keep(back)
    assert back.status == 0 and np.all(_get_tags(back, 0, rows)[1] == 0)
    st, s, r, i = _search(back, q[:2], k, [0, 3], [0, 2])
    st2, s2, r2, i2 = _search_ids(ga, q[:1], k)
    assert st == 0 and st2 == 0 and np.array_equal(r[:1], r2) and np.array_equal(_bits(s[:1]), _bits(s2)) and np.all(r[1] == -1)
    step("the saved gallery keeps its tags", [10, 90, 30])
    assert ga.L.rfd_gallery_clear(ga.g) == 0
    assert ga.add(g[:50]) == (0, 0)
    tags, live = np.zeros(50, np.int64), np.ones(50, bool)
    step("after clear every tag is 0, in HBM too", [])


def test_device_calls_run_in_stream_order_without_host_waits(rfd, det, gal):
    import torch
    L, dim, rows, n, k = rfd.load_library(), 64, 700, 33, 6
    dev = torch.device("cuda", 0)
    q, g, _ = _dyadic_case(dim, rows, n, 7900)
    tags = _tags(rows, 79)
    mask, value = _filters(n, 2)
    gone = np.array([0, 3, 16, 350, 699, 3], np.int32)
    full = R.scores(q, g)
    _exact(full)
    d_g = torch.from_numpy(g.astype(np.float32)).to(dev)
    d_q = torch.from_numpy(q.astype(np.float32)).to(dev)
    d_m = torch.from_numpy(_u32(mask).view(np.int32)).to(dev)
    d_v = torch.from_numpy(_u32(value).view(np.int32)).to(dev)
    out = [(torch.full((n, k), 7.0, device=dev), torch.full((n, k), -7, dtype=torch.int32, device=dev), torch.full((n, k), -7, dtype=torch.int32, device=dev))
           for _ in range(2)]
    torch.cuda.synchronize()
    gd = gal(dim, rows)
    first = C.c_int(-1)
    all_rows, all_tags = _i32(np.arange(rows)), _u32(tags)

    def search(o):
        return L.rfd_gallery_search_filtered_device(gd.g, d_q.data_ptr(), n, k, NEG_INF, d_m.data_ptr(), d_v.data_ptr(), o[0].data_ptr(), o[1].data_ptr(),
                                                    o[2].data_ptr(), 1)
    assert L.rfd_gallery_add_device(gd.g, d_g.data_ptr(), rows, C.byref(first)) == 0 and first.value == 0
    assert L.rfd_gallery_set_tags(gd.g, all_rows.ctypes.data, all_tags.ctypes.data, rows) == 0
    assert search(out[0]) == 0
    assert L.rfd_gallery_remove(gd.g, gone.ctypes.data, len(gone)) == 0
    assert search(out[1]) == 0
    assert L.rfd_sync(det._ctx) == 0
    live = np.ones(rows, bool)
    for o, lv in zip(out, (None, live)):
        if lv is not None:
            lv[gone] = False
        ref = _reference(full, None, tags if lv is None else np.where(lv, tags, 0), mask, value, lv)
        s, r, i = (x.cpu().numpy() for x in o)
        assert np.array_equal(r, ref[1][:, :k]) and np.array_equal(i, ref[2][:, :k]) and np.array_equal(_bits(s), _bits(ref[0][:, :k])), lv is None
    assert np.array_equal(_get_tags(gd, 0, rows)[1], np.where(live, tags, 0).astype(np.uint32))
    # a remove leaves nothing of the tag in HBM: the removed rows, replaced, are eligible for tag 0 alone
    assert gd.replace(gone[:5], g[gone[:5]]) == 0
    st, s, r, i = _search(gd, q[:2], 32, [ALL, ALL], [0, 0])
    want = _reference(full[:2], None, np.where(live, tags, 0), [ALL, ALL], [0, 0])
    assert st == 0 and np.array_equal(r, want[1]) and set(gone.tolist()) <= set(np.flatnonzero(np.where(live, tags, 0) == 0).tolist())


# ---- 11. errors ----
def test_error_rules(rfd, gal):
    import torch
    dim, rows, k = 32, 100, 5
    q, g, _ = _dyadic_case(dim, rows, 3, 8000)
    ga = gal(dim, rows + 5)
    _add_in_pieces(ga, g)
    tags = (np.arange(rows) % 4).astype(np.int64)
    assert _set_tags(ga, np.arange(rows), tags) == 0 and ga.remove([40]) == 0
    tags[40] = 0
    mask, value = [ALL, 3, 0], [1, 2, 0]
    before = _search(ga, q, k, mask, value)
    assert before[0] == 0

    def unchanged(tag):
        now = _search(ga, q, k, mask, value)
        assert now[0] == 0 and all(np.array_equal(x, y) for x, y in zip(before[1:], now[1:])), tag
        assert np.array_equal(_get_tags(ga, 0, rows)[1], tags.astype(np.uint32)), tag

    bad = rfd.RFD_ERR_INVALID_ARG
    assert _set_tags(ga, [1, rows], [9, 9]) == bad and "rows[1] = %d" % rows in ga.err()
    unchanged("a row beyond the gallery")
    assert _set_tags(ga, [1, -1], [9, 9]) == bad and "rows[1] = -1" in ga.err()
    unchanged("a negative row")
    assert _set_tags(ga, [1, 40], [9, 9]) == bad and "rows[1] = 40" in ga.err() and "removed" in ga.err()
    unchanged("a removed row")
    assert _set_tags(ga, [1, 2, 1], [9, 9, 9]) == bad and "row 1 " in ga.err() and "more than once" in ga.err()
    unchanged("a row listed twice")
    assert _set_tags(ga, [], []) == 0
    assert ga.L.rfd_gallery_set_tags(ga.g, None, None, 0) == 0
    one = _i32([1])
    assert ga.L.rfd_gallery_set_tags(ga.g, one.ctypes.data, None, 1) == bad and ga.L.rfd_gallery_set_tags(ga.g, None, one.ctypes.data, 1) == bad
    unchanged("n = 0 and null lists")
    assert _get_tags(ga, rows - 1, 2)[0] == bad and _get_tags(ga, -1, 1)[0] == bad and _get_tags(ga, 0, 0)[0] == 0
    # the searches: k, min_score, null filters, non-finite queries; nothing is written
    assert _search(ga, q, 0, mask, value)[0] == bad
    assert _search(ga, q, 33, mask, value)[0] == rfd.RFD_ERR_CAPACITY and "RFD_GALLERY_MAX_K" in ga.err()
    st, s, r, i = _search(ga, q, k, mask, value, float("nan"))
    assert st == bad and "min_score" in ga.err() and np.all(r == -7)
    qq = np.ascontiguousarray(q, np.float32)
    m, v = _u32(mask), _u32(value)
    s, r, i = np.full((3, k), 7.0, np.float32), np.full((3, k), -7, np.int32), np.full((3, k), -7, np.int32)
    call = ga.L.rfd_gallery_search_filtered
    assert call(ga.g, qq.ctypes.data, 3, k, NEG_INF, None, v.ctypes.data, s.ctypes.data, r.ctypes.data, i.ctypes.data) == bad and "mask" in ga.err()
    assert call(ga.g, qq.ctypes.data, 3, k, NEG_INF, m.ctypes.data, None, s.ctypes.data, r.ctypes.data, i.ctypes.data) == bad and "value" in ga.err()
    assert call(ga.g, qq.ctypes.data, 0, k, NEG_INF, None, None, s.ctypes.data, r.ctypes.data, i.ctypes.data) == 0
    dcall = ga.L.rfd_gallery_search_filtered_device
    d_q, d_f, d_o = (torch.zeros(1024, dtype=torch.int32, device="cuda").data_ptr() for _ in range(3))   # real buffers, large enough for the calls
    assert dcall(ga.g, d_q, 3, k, NEG_INF, None, d_f, d_o, d_o, d_o, 0) == bad and dcall(ga.g, d_q, 3, k, NEG_INF, d_f, None, d_o, d_o, d_o, 0) == bad
    assert dcall(ga.g, d_q + 4, 3, k, NEG_INF, d_f, d_f, d_o, d_o, d_o, 0) == bad and "aligned" in ga.err()
    qq[1, 3] = np.inf
    assert call(ga.g, qq.ctypes.data, 3, k, NEG_INF, m.ctypes.data, v.ctypes.data, s.ctypes.data, r.ctypes.data, i.ctypes.data) == bad and "query 1" in ga.err()
    assert np.all(r == -7) and np.all(i == -7) and np.all(s == 7.0)
    unchanged("refused searches")
    # a value outside its mask is not an error: the query's result is empty
    st, s, r, i = _search(ga, q, k, [1, ALL, 0], [3, 2, 0])
    assert st == 0 and np.all(r[0] == -1) and np.all(np.isneginf(s[0])) and np.all(i[0] == -1) and np.all(r[1:] >= 0)
