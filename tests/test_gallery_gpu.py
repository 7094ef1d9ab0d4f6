"""The on-device face gallery through the C ABI (include/rfd.h, "gallery") against tests/gallery_ref.py: storage bit for bit,
scores bit for bit on dyadic data, the (score descending, row ascending) order with planted equal scores, the documented error
bounds on random unit vectors, independence of a score from its position, the device forms, and the error rules."""
import ctypes as C

import numpy as np
import pytest

import gallery_ref as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def det(rfd):
    d = rfd.RetinaFaceDetection(image_size=(640, 640), max_batch_size=1, max_det=16)
    yield d
    d.close()


class Gal:
    """a gallery held through the raw C calls (statuses returned, not raised)"""

    def __init__(self, rfd, det, dim, capacity):
        self.L, self.rfd, self.det, self.dim, self.g = rfd.load_library(), rfd, det, dim, C.c_void_p()
        self.status = self.L.rfd_gallery_create(det._ctx, dim, capacity, C.byref(self.g))

    def close(self):
        if self.g:
            self.L.rfd_gallery_destroy(self.g)
        self.g = C.c_void_p()

    def size(self):
        rows, cap, dim = C.c_int(), C.c_int(), C.c_int()
        assert self.L.rfd_gallery_size(self.g, C.byref(rows), C.byref(cap), C.byref(dim)) == 0
        return rows.value, cap.value, dim.value

    def add(self, x):
        x = np.ascontiguousarray(x, np.float32).reshape(-1, self.dim)
        first = C.c_int(-7)
        return self.L.rfd_gallery_add(self.g, x.ctypes.data, x.shape[0], C.byref(first)), first.value

    def get(self, row0, n):
        out = np.full((n, self.dim), 7.0, np.float32)
        return self.L.rfd_gallery_get_rows(self.g, row0, n, out.ctypes.data), out

    def search(self, q, k):
        q = np.ascontiguousarray(q, np.float32).reshape(-1, self.dim)
        s, r = np.full((q.shape[0], max(k, 1)), 7.0, np.float32), np.full((q.shape[0], max(k, 1)), -7, np.int32)
        return self.L.rfd_gallery_search(self.g, q.ctypes.data, q.shape[0], k, s.ctypes.data, r.ctypes.data), s, r

    def err(self):
        return self.L.rfd_last_error().decode()


@pytest.fixture
def gal(rfd, det):
    made = []

    def make(dim, capacity):
        g = Gal(rfd, det, dim, capacity)
        made.append(g)
        return g
    yield make
    for g in made:
        g.close()


def _bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def _units(rng, n, dim):
    x = rng.standard_normal((n, dim))
    return (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32)


# ---- 1. storage ----
def test_storage_is_rne_bf16_of_the_input_bit_for_bit(rfd, gal):
    dim, rng = 512, np.random.default_rng(1)
    g = gal(dim, 60)
    assert g.status == 0 and g.size() == (0, 60, dim)
    x = (rng.standard_normal((54, dim)) * 2.0 ** rng.integers(-12, 3, (54, dim))).astype(np.float32)
    x[5, :8] = [0.0, -0.0, 1.00390625, -1.00390625, 1.01171875, 0.5, 65280.0, 2.0 ** -126]   # ties towards the even neighbour, below and above
    firsts, at = [], 0
    for n in (7, 30, 1, 16):   # starts and ends in the middle of 16-row blocks
        st, first = g.add(x[at:at + n])
        assert st == 0
        firsts.append(first)
        at += n
    assert firsts == [0, 7, 37, 38] and g.size()[0] == 54
    want = R.rne_bf16(x).astype(np.float32)
    assert np.array_equal(want.astype(np.float64), R.rne_bf16(x))   # bf16 values are exact in f32
    for row0 in range(54):
        for n in range(1, 54 - row0 + 1):
            st, got = g.get(row0, n)
            assert st == 0 and np.array_equal(_bits(got), _bits(want[row0:row0 + n])), (row0, n)
    assert g.get(50, 5)[0] == rfd.RFD_ERR_INVALID_ARG and g.get(-1, 2)[0] == rfd.RFD_ERR_INVALID_ARG
    # over capacity: refused whole, nothing added
    st, _ = g.add(x[:7])
    assert st == rfd.RFD_ERR_CAPACITY and "54 of 60" in g.err() and g.size()[0] == 54
    assert np.array_equal(_bits(g.get(0, 54)[1]), _bits(want))
    assert g.add(x[:0])[0] == 0 and g.size()[0] == 54   # n = 0: a no-op
    # clear: empty again, rows start at 0, and nothing of the old content is found
    assert g.L.rfd_gallery_clear(g.g) == 0 and g.size()[0] == 0
    assert g.get(0, 1)[0] == rfd.RFD_ERR_INVALID_ARG
    assert g.add(x[40:43]) == (0, 0) and g.size()[0] == 3
    assert np.array_equal(_bits(g.get(0, 3)[1]), _bits(want[40:43]))
    st, s, r = g.search(x[:2] * 0 + 1.0, 5)
    assert st == 0 and np.all(r[:, :3] >= 0) and np.all(r[:, 3:] == -1) and np.all(np.isneginf(s[:, 3:]))


# ---- 2. exact bits on dyadic data ----
def _dyadic_case(dim, rows, nq, seed):
    """values m * 2^-6, |m| <= 8: exact in bf16, and every partial sum of products is exact in f32 in any order (asserted).
    Query i's best possible row is sign(q_i) / 8; query 0's is planted at rows on both sides of workgroup boundaries and at the
    last row, the last query's at the last but one."""
    rng = np.random.default_rng(seed)
    g = rng.integers(-8, 9, (rows, dim)).astype(np.float64) / 64
    q = rng.integers(-8, 9, (nq, dim)).astype(np.float64) / 64
    q[q == 0] = 1 / 64   # so that sign(q) / 8 is the unique maximiser
    planted = sorted({p for p in (2, 63, 64, 2111, 2112, rows - 1) if 0 <= p < rows})
    for p in planted:
        g[p] = np.sign(q[0]) / 8
    if rows >= 4:
        g[rows - 2] = np.sign(q[nq - 1]) / 8
    assert np.array_equal(R.rne_bf16(g), g) and np.array_equal(R.rne_bf16(q), q)
    assert float((np.abs(q) @ np.abs(g).T).max()) * 2.0 ** 12 < 2.0 ** 24   # integers below 2^24 in units of 2^-12
    return q, g, planted


SIZES = [1, 15, 16, 17, 4097]


@pytest.mark.parametrize("rows", SIZES)
def test_scores_and_rows_are_exact_on_dyadic_data(rfd, gal, rows):
    dim = 512
    q, g, planted = _dyadic_case(dim, rows, 33, 100 + rows)
    ga = gal(dim, rows)
    assert ga.add(g) == (0, 0)
    full = R.scores(q, g)
    assert np.array_equal(full.astype(np.float32).astype(np.float64), full)
    for n in (1, 3, 32, 33):
        for k in (1, 5, 32):
            ref_s, ref_r = R.topk_of_scores(full[:n], k)
            st, s, r = ga.search(q[:n], k)
            assert st == 0
            assert np.array_equal(r, ref_r), (rows, n, k)
            assert np.array_equal(_bits(s), _bits(ref_s)), (rows, n, k)
            assert list(r[0, :min(k, len(planted))]) == planted[:k]        # equal scores: the lower row first
            if k > rows:
                assert np.all(r[:, rows:] == -1) and np.all(np.isneginf(s[:, rows:]))
    if rows >= 4:
        assert ga.search(q, 1)[2][32, 0] == rows - 2


@pytest.mark.parametrize("dim", [32, 128])
def test_exact_at_other_dims(rfd, gal, dim):
    rows = 4097 if dim == 32 else 333
    q, g, planted = _dyadic_case(dim, rows, 33, 7 + dim)
    ga = gal(dim, rows + 5)
    assert ga.add(g[:100]) == (0, 0) and ga.add(g[100:]) == (0, 100)
    full = R.scores(q, g)
    for n, k in ((33, 5), (3, 32), (16, 1), (17, 7)):
        ref_s, ref_r = R.topk_of_scores(full[:n], k)
        st, s, r = ga.search(q[:n], k)
        assert st == 0 and np.array_equal(r, ref_r) and np.array_equal(_bits(s), _bits(ref_s)), (dim, n, k)


# ---- 3. random unit vectors ----
RANDOM_SEED = 9   # chosen on the CPU: the smallest gap among every query's first k + 1 exact scores is 8.5 x (4 r)


def test_random_unit_vectors_meet_both_bounds_and_the_reference_rows(rfd, gal):
    dim, rows, n, k = 512, 5000, 32, 8
    rng = np.random.default_rng(RANDOM_SEED)
    g, q = _units(rng, rows, dim), _units(rng, n, dim)
    exact = R.scores(q, g)                          # f64, of the bf16-rounded vectors
    rad = R.accumulation_radius(q, g, exact)
    ref_s, ref_r = R.topk_of_scores(exact, k + 1)
    # decided on the CPU, before the GPU is touched: the first k + 1 scores of every query are pairwise more than 4 r apart, so
    # no admissible accumulation error can change a row
    for i in range(n):
        gaps = ref_s[i, :-1] - ref_s[i, 1:]
        assert np.all(gaps > 4 * rad[i, ref_r[i]].max()), (i, gaps.min(), rad[i, ref_r[i]].max())
    ga = gal(dim, rows)
    assert ga.add(g) == (0, 0)
    st, s, r = ga.search(q, k)
    assert st == 0
    sel = np.take_along_axis(exact, r.astype(np.int64), 1)
    err = np.abs(s.astype(np.float64) - sel)
    bound = np.take_along_axis(rad, r.astype(np.int64), 1)
    print("accumulation error / radius: max %.3f" % float((err / bound).max()))
    assert np.all(err <= bound)
    true = q.astype(np.float64) @ g.astype(np.float64).T
    err_in = np.abs(s.astype(np.float64) - np.take_along_axis(true, r.astype(np.int64), 1))
    bound_in = np.take_along_axis(R.input_bound(q, g), r.astype(np.int64), 1) + bound
    print("input rounding error / bound: max %.3f, largest error %.3g (2^-8 = %.3g)" % (float((err_in / bound_in).max()), float(err_in.max()), 2.0 ** -8))
    assert np.all(err_in <= bound_in) and float(err_in.max()) < 2.0 ** -8
    assert np.array_equal(r, ref_r[:, :k])


# ---- 4. a score does not depend on where its query or its row sits ----
def test_score_bits_do_not_depend_on_position(rfd, gal):
    dim, k, rng = 512, 32, np.random.default_rng(9)
    x = _units(rng, 1, dim)[0]
    near = x[None, :] + 0.05 * rng.standard_normal((300, dim)).astype(np.float32)
    near = (near / np.linalg.norm(near, axis=1, keepdims=True)).astype(np.float32)   # scores around 0.66: they stay the best rows
    others = _units(rng, 33, dim)
    ga = gal(dim, 1300)
    assert ga.add(near) == (0, 0)

    def results():
        out = []
        st, s, r = ga.search(x, k)                     # a batch of 1
        assert st == 0
        out.append((s[0], r[0]))
        for pos in (0, 31, 32):                        # a batch of 33: both M-tiles of the first pass, and the second pass
            b = others.copy()
            b[pos] = x
            st, s, r = ga.search(b, k)
            assert st == 0
            out.append((s[pos], r[pos]))
        return out
    before = results()
    assert ga.add(_units(rng, 1000, dim)) == (0, 300)  # other workgroups now score the same rows
    after = results()
    s0, r0 = before[0]
    assert len(set(r0.tolist())) == k and r0.min() >= 0
    for s, r in before + after:
        assert np.array_equal(r, r0) and np.array_equal(_bits(s), _bits(s0))


# ---- 5. device forms ----
def test_device_forms_equal_the_host_forms(rfd, det, gal):
    import torch
    L, dim, rows, n, k = rfd.load_library(), 512, 700, 40, 6
    dev = torch.device("cuda", 0)
    torch.manual_seed(3)
    raw = torch.randn(rows, dim, device=dev)
    emb = torch.empty_like(raw)
    d_s = torch.full((n, k), 7.0, device=dev)
    d_r = torch.full((n, k), -7, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    gd = gal(dim, rows)
    first = C.c_int(-1)
    # normalise -> enrol -> search the first n of them, back to back on the context's stream
    assert L.rfd_normalize_embeddings_device(det._ctx, raw.data_ptr(), rows, dim, emb.data_ptr()) == 0
    assert L.rfd_gallery_add_device(gd.g, emb.data_ptr(), rows, C.byref(first)) == 0 and first.value == 0
    assert gd.size()[0] == rows
    assert L.rfd_gallery_search_device(gd.g, emb.data_ptr(), n, k, d_s.data_ptr(), d_r.data_ptr(), 1) == 0
    assert L.rfd_sync(det._ctx) == 0
    s, r, e = d_s.cpu().numpy(), d_r.cpu().numpy(), emb.cpu().numpy()
    gh = gal(dim, rows)
    assert gh.add(e) == (0, 0)
    st, hs, hr = gh.search(e[:n], k)
    assert st == 0 and np.array_equal(r, hr) and np.array_equal(_bits(s), _bits(hs))
    assert np.array_equal(_bits(gd.get(0, rows)[1]), _bits(gh.get(0, rows)[1]))
    assert np.array_equal(r[:, 0], np.arange(n))           # a stored row finds itself first
    assert L.rfd_gallery_search_device(gd.g, emb.data_ptr() + 4, n, k, d_s.data_ptr(), d_r.data_ptr(), 0) == rfd.RFD_ERR_INVALID_ARG
    # the Python class over the same calls
    pg = det.gallery(dim, rows)
    assert pg.add(e) == 0 and pg.size() == rows
    ps, pr = pg.search(e[:n], k)
    assert np.array_equal(pr, hr) and np.array_equal(_bits(ps), _bits(hs)) and np.array_equal(_bits(pg.rows(3, 9)), _bits(gh.get(3, 9)[1]))
    pg.search_device(emb.data_ptr(), n, k, d_s.data_ptr(), d_r.data_ptr(), async_=False)
    assert np.array_equal(d_r.cpu().numpy(), hr)
    pg.clear()
    assert pg.size() == 0
    pg.close()


# ---- 6. errors ----
def test_error_rules(rfd, det, gal):
    dim, rng = 64, np.random.default_rng(4)
    bad = gal(48, 10)
    assert bad.status == rfd.RFD_ERR_INVALID_ARG and "multiple of 32" in bad.err() and not bad.g
    assert gal(2048, 10).status == rfd.RFD_ERR_INVALID_ARG and gal(64, 0).status == rfd.RFD_ERR_INVALID_ARG
    g = gal(dim, 40)
    assert g.status == 0
    q = _units(rng, 3, dim)
    # an empty gallery: all -1 / -inf
    st, s, r = g.search(q, 4)
    assert st == 0 and np.all(r == -1) and np.all(np.isneginf(s))
    x = _units(rng, 20, dim)
    assert g.add(x) == (0, 0)
    assert g.search(q, 0)[0] == rfd.RFD_ERR_INVALID_ARG
    assert g.search(q, -3)[0] == rfd.RFD_ERR_INVALID_ARG
    assert g.search(q, 33)[0] == rfd.RFD_ERR_CAPACITY and "RFD_GALLERY_MAX_K" in g.err()
    assert g.search(q[:0], 4)[0] == 0                  # n = 0: a no-op
    # non-finite values: refused by the host forms, the message names the first offender
    qn = q.copy()
    qn[2, 17] = np.nan
    qn[2, 40] = np.inf
    assert g.search(qn, 4)[0] == rfd.RFD_ERR_INVALID_ARG and "query 2" in g.err() and "element 17" in g.err()
    xn = x[:5].copy()
    xn[3, 63] = -np.inf
    st, _ = g.add(xn)
    assert st == rfd.RFD_ERR_INVALID_ARG and "row 3" in g.err() and "element 63" in g.err() and g.size()[0] == 20
    # the Python class raises the same statuses
    pg = det.gallery(dim, 8)
    with pytest.raises(rfd.RfdError) as e:
        pg.search(q, 33)
    assert e.value.status == rfd.RFD_ERR_CAPACITY
    with pytest.raises(rfd.RfdError) as e:
        pg.add(_units(rng, 9, dim))
    assert e.value.status == rfd.RFD_ERR_CAPACITY and pg.size() == 0
    pg.close()
    with pytest.raises(rfd.RfdError):
        det.gallery(48, 8)
