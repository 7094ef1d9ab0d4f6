"""Removing and replacing rows of the on-device face gallery, and saving it to and loading it from a file (include/rfd.h,
"remove and replace", "gallery file"), through the C ABI.  The reference of every search is gallery_ref.topk_of_scores over the
LIVE columns of the score matrix, mapped back to row numbers: a gallery with removed rows must return what a gallery of its
live rows alone returns, bit for bit, because a score depends on its two vectors only and the order is total."""
import ctypes as C
import os

import numpy as np
import pytest

import gallery_ref as R
from test_gallery_gpu import Gal, _bits, _dyadic_case, _units, det  # noqa: F401  (det: the module's detector fixture)

pytestmark = pytest.mark.gpu


class EditGal(Gal):
    """test_gallery_gpu.Gal plus the calls of this file (statuses returned, not raised)"""

    @staticmethod
    def _list(rows):
        return np.ascontiguousarray(np.asarray(rows, np.int64).reshape(-1), np.int32)

    def remove(self, rows):
        r = self._list(rows)
        return self.L.rfd_gallery_remove(self.g, r.ctypes.data, r.shape[0])

    def replace(self, rows, x):
        r, x = self._list(rows), np.ascontiguousarray(x, np.float32).reshape(-1, self.dim)
        assert r.shape[0] == x.shape[0]
        return self.L.rfd_gallery_replace(self.g, r.ctypes.data, x.ctypes.data, r.shape[0])

    def live(self):
        n = C.c_int(-7)
        assert self.L.rfd_gallery_live(self.g, C.byref(n)) == 0
        return n.value

    def removed(self, cap=None):
        n = C.c_int(-7)
        assert self.L.rfd_gallery_removed(self.g, None, 0, C.byref(n)) == 0
        cap = n.value if cap is None else cap
        out = np.full(max(cap, 1), -7, np.int32)
        assert self.L.rfd_gallery_removed(self.g, out.ctypes.data, cap, C.byref(n)) == 0
        return n.value, out[:cap].tolist()

    def save(self, path):
        return self.L.rfd_gallery_save(self.g, os.fsencode(str(path)))

    @classmethod
    def load(cls, rfd, det, path, capacity=0):
        self = cls.__new__(cls)
        self.L, self.rfd, self.det, self.g = rfd.load_library(), rfd, det, C.c_void_p()
        self.status = self.L.rfd_gallery_load(det._ctx, os.fsencode(str(path)), capacity, C.byref(self.g))
        self.dim = self.size()[2] if self.status == 0 else 0
        return self


@pytest.fixture
def gal(rfd, det):
    made = []

    def make(dim, capacity):
        g = EditGal(rfd, det, dim, capacity)
        made.append(g)
        return g
    make.keep = made.append
    yield make
    for g in made:
        g.close()


def _masked_topk(full, live_rows, k):
    """topk_of_scores over the live columns of `full`, rows mapped back to gallery rows"""
    live_rows = np.asarray(live_rows, np.int64)
    s, r = R.topk_of_scores(full[:, live_rows], k)
    mapped = np.where(r >= 0, live_rows[np.maximum(r, 0)] if live_rows.size else -1, -1).astype(np.int32)
    return s, mapped


def _check_search(ga, q, full, live_rows, n, k, tag):
    ref_s, ref_r = _masked_topk(full[:n], live_rows, k)
    st, s, r = ga.search(q[:n], k)
    assert st == 0, tag
    assert np.array_equal(r, ref_r), tag
    assert np.array_equal(_bits(s), _bits(ref_s)), tag
    return s, r


# ---- 1. exact bits on dyadic data, four removal patterns ----
def _patterns(rows):
    keep3 = sorted({0, rows // 2, rows - 1})
    return [("planted", [p for p in (63, 2111) if p < rows]),
            ("block and last", sorted({p for p in list(range(16, 32)) + [rows - 1] if p < rows})),
            ("all but three", [p for p in range(rows) if p not in keep3]),
            ("all", list(range(rows)))]


@pytest.mark.parametrize("rows", [1, 15, 16, 17, 4097])
def test_scores_and_rows_are_exact_with_removed_rows(rfd, gal, rows):
    dim = 512
    q, g, planted = _dyadic_case(dim, rows, 33, 100 + rows)
    full = R.scores(q, g)
    assert np.array_equal(full.astype(np.float32).astype(np.float64), full)
    for name, gone in _patterns(rows):
        ga = gal(dim, rows)
        assert ga.add(g) == (0, 0)
        assert ga.remove(gone) == 0
        live_rows = np.setdiff1d(np.arange(rows), gone)
        assert ga.live() == len(live_rows) and ga.removed() == (len(gone), sorted(gone)) and ga.size()[0] == rows
        for n in (1, 3, 32, 33):
            for k in (1, 5, 32):
                s, r = _check_search(ga, q, full, live_rows, n, k, (rows, name, n, k))
                assert not np.isin(r, gone).any(), (rows, name, n, k)
                tail = min(k, len(live_rows))
                assert np.all(r[:, tail:] == -1) and np.all(np.isneginf(s[:, tail:])) and np.all(r[:, :tail] >= 0)
        if name == "planted" and rows == 4097:
            assert ga.search(q[:1], 5)[2][0, :4].tolist() == [2, 64, 2112, 4096]   # equal scores: the lower live row first
        ga.close()


@pytest.mark.parametrize("dim", [32, 128])
def test_exact_with_removed_rows_at_other_dims(rfd, gal, dim):
    rows = 4097 if dim == 32 else 333
    q, g, planted = _dyadic_case(dim, rows, 33, 7 + dim)
    ga = gal(dim, rows + 5)
    assert ga.add(g[:100]) == (0, 0) and ga.add(g[100:]) == (0, 100)
    gone = sorted({p for p in [2, 63] + list(range(16, 32)) + [rows - 1] if p < rows})
    assert ga.remove(gone) == 0
    live_rows = np.setdiff1d(np.arange(rows), gone)
    full = R.scores(q, g)
    for n, k in ((33, 5), (3, 32), (16, 1), (17, 7)):
        _check_search(ga, q, full, live_rows, n, k, (dim, n, k))


# ---- 2. a masked gallery equals a gallery of its survivors ----
def test_a_masked_gallery_equals_a_gallery_of_its_survivors(rfd, gal):
    dim, rows, n, k, rng = 512, 1300, 33, 32, np.random.default_rng(9)
    x = _units(rng, rows, dim)
    q = _units(rng, n, dim)
    q[:8] = x[rng.choice(rows, 8, replace=False)]        # some queries are enrolled rows, removed or not
    gone = np.sort(rng.choice(rows, rows // 3, replace=False))
    survivors = np.setdiff1d(np.arange(rows), gone)
    ga, gb = gal(dim, rows), gal(dim, rows)
    assert ga.add(x) == (0, 0) and ga.remove(gone) == 0
    assert gb.add(x[survivors]) == (0, 0)
    st_a, sa, ra = ga.search(q, k)
    st_b, sb, rb = gb.search(q, k)
    assert st_a == 0 and st_b == 0
    assert rb.min() >= 0 and np.array_equal(ra, survivors[rb].astype(np.int32))
    assert np.array_equal(_bits(sa), _bits(sb))


# ---- 3. erasure and bookkeeping ----
def test_erasure_and_bookkeeping(rfd, gal):
    dim, rng = 64, np.random.default_rng(3)
    x = _units(rng, 40, dim)
    want = R.rne_bf16(x).astype(np.float32)
    g = gal(dim, 64)
    assert g.add(x) == (0, 0) and g.live() == 40 and g.removed() == (0, [])
    assert g.remove([]) == 0 and g.live() == 40                      # n = 0: a no-op
    assert g.remove([17, 5, 17, 39]) == 0                             # duplicates allowed
    assert g.live() == 37 and g.removed() == (3, [5, 17, 39]) and g.size() == (40, 64, dim)
    assert g.removed(cap=2) == (3, [5, 17]) and g.removed(cap=0) == (3, [])
    got = g.get(0, 40)[1]
    erased = want.copy()
    erased[[5, 17, 39]] = 0.0
    assert np.array_equal(_bits(got), _bits(erased))                 # +0.0 bits in the removed rows, their neighbours untouched
    assert not _bits(got[[5, 17, 39]]).any()
    assert g.remove([5]) == 0 and g.remove([17, 39, 5]) == 0         # idempotent
    assert g.live() == 37 and g.removed() == (3, [5, 17, 39])
    assert np.array_equal(_bits(g.get(0, 40)[1]), _bits(erased))
    # add after remove appends at rows; the holes stay
    assert g.add(x[:3]) == (0, 40) and g.size()[0] == 43 and g.live() == 40 and g.removed() == (3, [5, 17, 39])
    st, s, r = g.search(x[[5, 0]], 2)
    assert st == 0 and r[0, 0] != 5 and r[1].tolist() == [0, 40]     # row 0 and its copy at 40: equal scores, the lower row first
    # clear forgets removals
    assert g.L.rfd_gallery_clear(g.g) == 0 and g.size()[0] == 0 and g.live() == 0 and g.removed() == (0, [])
    assert g.add(x[:20]) == (0, 0) and g.live() == 20 and g.removed() == (0, [])
    st, s, r = g.search(x[[5, 17]], 1)
    assert st == 0 and r[:, 0].tolist() == [5, 17]                   # rows 5 and 17 are live again: nothing of the old mask is left


# ---- 4. replace ----
def test_replace_writes_rne_bf16_and_revives(rfd, det, gal):
    import torch
    dim, rng = 512, np.random.default_rng(4)
    x = _units(rng, 50, dim)
    g = gal(dim, 50)
    assert g.add(x) == (0, 0)
    new = (rng.standard_normal((3, dim)) * 2.0 ** rng.integers(-18, -3, (3, dim))).astype(np.float32)   # short vectors: they win no search
    new[0, :4] = [1.00390625, -1.00390625, 1.01171875, -0.0]        # ties towards the even neighbour
    new[2] = _units(rng, 1, dim)[0]
    assert g.remove([7, 20]) == 0 and g.live() == 48
    assert g.replace([33, 7, 49], new) == 0                          # a live row, a removed row, the last row
    assert g.live() == 49 and g.removed() == (1, [20]) and g.size()[0] == 50
    want = R.rne_bf16(x).astype(np.float32)
    want[[33, 7, 49]] = R.rne_bf16(new).astype(np.float32)
    want[20] = 0.0
    assert np.array_equal(_bits(g.get(0, 50)[1]), _bits(want))
    st, s, r = g.search(new[2], 1)
    assert st == 0 and r[0, 0] == 49                                 # a search finds the new values
    st, s, r = g.search(x[[20, 7]], 1)
    assert st == 0 and 20 not in r and r[1, 0] != 7                  # the old values of rows 20 and 7 are gone
    # the device form equals the host form
    gd = gal(dim, 50)
    assert gd.add(x) == (0, 0) and gd.remove([7, 20]) == 0
    d_new = torch.from_numpy(new).to(torch.device("cuda", 0))
    torch.cuda.synchronize()
    rows = np.array([33, 7, 49], np.int32)
    assert gd.L.rfd_gallery_replace_device(gd.g, rows.ctypes.data, d_new.data_ptr(), 3) == 0
    assert gd.live() == 49 and gd.removed() == (1, [20])
    assert np.array_equal(_bits(gd.get(0, 50)[1]), _bits(want))
    q = _units(rng, 5, dim)
    assert all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(g.search(q, 6)[1:], gd.search(q, 6)[1:]))
    # reviving the last removed row: the gallery is whole again
    assert g.replace([20], x[20]) == 0 and g.live() == 50 and g.removed() == (0, [])
    assert np.array_equal(g.search(x[20], 1)[2], [[20]])


# ---- 5. stream order ----
def test_device_calls_run_in_stream_order_without_host_waits(rfd, det, gal):
    import torch
    L, dim, rows, n, k = rfd.load_library(), 512, 700, 33, 6
    dev = torch.device("cuda", 0)
    torch.manual_seed(5)
    raw = torch.randn(rows + 4, dim, device=dev)
    emb = torch.empty_like(raw)
    d_s = torch.full((n, k), 7.0, device=dev)
    d_r = torch.full((n, k), -7, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    gone = np.array([0, 3, 16, 17, 31, 350, 699, 3], np.int32)
    put = np.array([17, 5, 699, 120], np.int32)                       # two removed rows revived, two live rows corrected
    gd = gal(dim, rows)
    first = C.c_int(-1)
    assert L.rfd_normalize_embeddings_device(det._ctx, raw.data_ptr(), rows + 4, dim, emb.data_ptr()) == 0
    assert L.rfd_gallery_add_device(gd.g, emb.data_ptr(), rows, C.byref(first)) == 0 and first.value == 0
    assert L.rfd_gallery_remove(gd.g, gone.ctypes.data, len(gone)) == 0
    assert L.rfd_gallery_replace_device(gd.g, put.ctypes.data, emb.data_ptr() + rows * dim * 4, len(put)) == 0
    assert L.rfd_gallery_search_device(gd.g, emb.data_ptr(), n, k, d_s.data_ptr(), d_r.data_ptr(), 1) == 0
    assert L.rfd_sync(det._ctx) == 0
    s, r, e = d_s.cpu().numpy(), d_r.cpu().numpy(), emb.cpu().numpy()
    assert gd.live() == rows - 5 and gd.removed() == (5, [0, 3, 16, 31, 350])
    gh = gal(dim, rows)
    assert gh.add(e[:rows]) == (0, 0) and gh.remove(gone) == 0 and gh.replace(put, e[rows:]) == 0
    st, hs, hr = gh.search(e[:n], k)
    assert st == 0 and np.array_equal(r, hr) and np.array_equal(_bits(s), _bits(hs))
    assert np.array_equal(_bits(gd.get(0, rows)[1]), _bits(gh.get(0, rows)[1]))
    assert not np.isin(r, [0, 3, 16, 31, 350]).any()
    assert r[1, 0] == 1 and r[0, 0] != 0                              # a live row finds itself first, a removed one does not


# ---- 6. save and load ----
def test_save_and_load_round_trip(rfd, det, gal, tmp_path):
    dim, rows, n, k, rng = 512, 700, 33, 6, np.random.default_rng(6)
    x = _units(rng, rows, dim)
    q = _units(rng, n, dim)
    q[:4] = x[[1, 699, 16, 350]]
    g = gal(dim, rows)
    gone = [1, 16, 17, 18, 350, 698]
    assert g.add(x) == (0, 0) and g.remove(gone) == 0 and g.replace([17, 400], x[[2, 3]]) == 0
    gone = [1, 16, 18, 350, 698]
    path = tmp_path / "gallery.rfdg"
    assert g.save(path) == 0 and not os.path.exists(str(path) + ".tmp")
    assert rfd.gallery_file_info(path) == (dim, rows, rows - 5)
    values = g.get(0, rows)[1]
    mask = np.ones(rows, bool)
    mask[gone] = False
    # the file is what the numpy writer makes of get_rows and the mask, byte for byte
    twin = tmp_path / "twin.rfdg"
    rfd.gallery_file_write(twin, values, mask)
    assert path.read_bytes() == twin.read_bytes()
    before = g.search(q, k)
    assert before[0] == 0
    h = EditGal.load(rfd, det, path)
    gal.keep(h)
    assert h.status == 0 and h.size() == (rows, rows, dim) and h.live() == rows - 5 and h.removed() == (5, gone)
    assert np.array_equal(_bits(h.get(0, rows)[1]), _bits(values))
    after = h.search(q, k)
    assert after[0] == 0 and np.array_equal(after[2], before[2]) and np.array_equal(_bits(after[1]), _bits(before[1]))
    assert not np.isin(after[2], gone).any()
    # a smaller capacity than the rows is refused; a larger one leaves room, and add appends
    small = EditGal.load(rfd, det, path, capacity=rows - 1)
    assert small.status == rfd.RFD_ERR_CAPACITY and not small.g and "700 rows" in small.err()
    big = EditGal.load(rfd, det, path, capacity=rows + 10)
    gal.keep(big)
    assert big.status == 0 and big.size() == (rows, rows + 10, dim)
    assert big.add(x[:2]) == (0, rows) and big.live() == rows - 3 and big.removed() == (5, gone)
    st, s, r = big.search(x[[1, 0]], 2)
    assert st == 0 and r[0, 0] == rows + 1 and r[1].tolist() == [0, rows]   # row 1 is gone, its copy is not; row 0 and its copy tie
    # a file written by the numpy writer loads and searches like a gallery built by add and remove
    y = R.rne_bf16(_units(rng, 45, dim)).astype(np.float32)
    ymask = np.ones(45, bool)
    ymask[[0, 15, 16, 44]] = False
    stored = y.copy()
    stored[~ymask] = 0.0
    made = tmp_path / "made.rfdg"
    rfd.gallery_file_write(made, stored, ymask)
    a = EditGal.load(rfd, det, made)
    gal.keep(a)
    b = gal(dim, 45)
    assert a.status == 0 and b.add(y) == (0, 0) and b.remove(np.flatnonzero(~ymask)) == 0
    assert a.size() == (45, 45, dim) and a.live() == b.live() == 41 and a.removed() == b.removed()
    assert np.array_equal(_bits(a.get(0, 45)[1]), _bits(b.get(0, 45)[1]))
    ra, rb = a.search(q, k), b.search(q, k)
    assert ra[0] == 0 and rb[0] == 0 and np.array_equal(ra[2], rb[2]) and np.array_equal(_bits(ra[1]), _bits(rb[1]))
    # a malformed file creates nothing
    bad = tmp_path / "bad.rfdg"
    bad.write_bytes(made.read_bytes()[:-1])
    c = EditGal.load(rfd, det, bad)
    assert c.status == rfd.RFD_ERR_INVALID_ARG and not c.g and "length" in c.err()
    assert EditGal.load(rfd, det, tmp_path / "missing.rfdg").status == rfd.RFD_ERR_IO
    assert g.save(tmp_path / "no" / "such" / "dir.rfdg") == rfd.RFD_ERR_IO
    # the Python class over the same calls
    pg = det.load_gallery(path, capacity=rows + 1)
    assert (pg.dim, pg.capacity, pg.size(), pg.live()) == (dim, rows + 1, rows, rows - 5) and pg.removed().tolist() == gone
    ps, pr = pg.search(q, k)
    assert np.array_equal(pr, before[2]) and np.array_equal(_bits(ps), _bits(before[1]))
    pg.replace([1], x[1:2])
    pg.remove([2, 2])
    assert pg.live() == rows - 5 and pg.removed().tolist() == [2, 16, 18, 350, 698]
    again = tmp_path / "again.rfdg"
    pg.save(again)
    v2, m2 = rfd.gallery_file_read(again)
    assert np.array_equal(_bits(v2), _bits(pg.rows(0, rows))) and np.flatnonzero(~m2).tolist() == [2, 16, 18, 350, 698]
    pg.close()


# ---- 7. errors ----
def test_error_rules_of_remove_and_replace(rfd, det, gal):
    import torch
    dim, rng = 64, np.random.default_rng(7)
    x = _units(rng, 20, dim)
    g = gal(dim, 40)
    assert g.add(x) == (0, 0) and g.remove([4]) == 0
    stored = g.get(0, 20)[1]

    def unchanged():
        return g.live() == 19 and g.removed() == (1, [4]) and g.size()[0] == 20 and np.array_equal(_bits(g.get(0, 20)[1]), _bits(stored))
    # out-of-range rows: refused whole, the first offender named, nothing changed
    assert g.remove([3, 20, -1]) == rfd.RFD_ERR_INVALID_ARG and "rows[1] = 20" in g.err() and unchanged()
    assert g.remove([-1]) == rfd.RFD_ERR_INVALID_ARG and "rows[0] = -1" in g.err() and unchanged()
    assert g.replace([3, 39], x[:2]) == rfd.RFD_ERR_INVALID_ARG and "rows[1] = 39" in g.err() and unchanged()   # below capacity, not enrolled
    # a row listed twice in one replace
    assert g.replace([3, 8, 3], x[:3]) == rfd.RFD_ERR_INVALID_ARG and "row 3" in g.err() and "more than once" in g.err() and unchanged()
    # non-finite values in the host replace
    bad = x[:3].copy()
    bad[1, 9] = np.nan
    bad[2, 0] = np.inf
    assert g.replace([3, 8, 4], bad) == rfd.RFD_ERR_INVALID_ARG and "row 1" in g.err() and "element 9" in g.err() and unchanged()
    # an unaligned device pointer
    d = torch.zeros(2 * dim + 4, device=torch.device("cuda", 0))
    torch.cuda.synchronize()
    rows = np.array([3, 8], np.int32)
    assert g.L.rfd_gallery_replace_device(g.g, rows.ctypes.data, d.data_ptr() + 4, 2) == rfd.RFD_ERR_INVALID_ARG and "aligned" in g.err() and unchanged()
    assert g.L.rfd_gallery_replace_device(g.g, rows.ctypes.data, None, 2) == rfd.RFD_ERR_INVALID_ARG and unchanged()
    assert g.L.rfd_gallery_remove(g.g, None, 2) == rfd.RFD_ERR_INVALID_ARG and unchanged()
    assert g.replace([], x[:0]) == 0 and unchanged()                 # n = 0: a no-op
    n = C.c_int()
    assert g.L.rfd_gallery_removed(g.g, None, 3, C.byref(n)) == rfd.RFD_ERR_INVALID_ARG   # out may be null only when cap is 0
    # the Python class raises the same statuses
    pg = det.gallery(dim, 8)
    pg.add(x[:6])
    for call in (lambda: pg.remove([6]), lambda: pg.replace([0, 0], x[:2]), lambda: pg.replace([1], bad[1:2]),
                 lambda: pg.replace_device([1], d.data_ptr() + 4)):
        with pytest.raises(rfd.RfdError) as e:
            call()
        assert e.value.status == rfd.RFD_ERR_INVALID_ARG
    assert pg.live() == 6 and pg.removed().tolist() == []
    pg.replace_device([1], d.data_ptr())
    det.sync()
    assert not _bits(pg.rows(1, 1)).any() and pg.live() == 6
    with pytest.raises(rfd.RfdError) as e:
        det.load_gallery("/nonexistent/gallery.rfdg")
    assert e.value.status == rfd.RFD_ERR_IO
    pg.close()
