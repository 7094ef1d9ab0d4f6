"""tests/gallery_identity_ref.py checked against itself and against tests/gallery_ref.py, without a GPU: its two forms (one sort
per query; k rounds over all rows) agree on seeded cases with ties, all-equal scores, all identities -1 and all distinct, with
removed rows, thresholds and non-finite scores, and with every identity -1 it is gallery_ref.topk."""
import numpy as np
import pytest

import gallery_identity_ref as I
import gallery_ref as R


def _same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


def _cases():
    rng = np.random.default_rng(7)
    out = []
    for rows, m in ((1, 1), (5, 2), (40, 3), (40, 40), (97, 8), (97, 200)):
        s = rng.integers(-6, 7, (4, rows)).astype(np.float64) / 8          # few levels: many ties
        out.append(("row % m", s, np.arange(rows) % m))
        out.append(("runs", s, (np.arange(rows) * m) // rows))
        out.append(("random, some unlabelled", s, rng.integers(-1, m, rows)))
        out.append(("all unlabelled", s, np.full(rows, -1)))
        out.append(("all distinct", s, rng.permutation(rows)))
        out.append(("all scores equal", np.full((2, rows), 0.375), np.arange(rows) % m))
    return out


@pytest.mark.parametrize("k", [1, 5, 32])
def test_the_two_forms_agree(k):
    rng = np.random.default_rng(11)
    for name, s, ids in _cases():
        rows = s.shape[1]
        for live in (None, rng.random(rows) < 0.6, np.zeros(rows, bool)):
            for min_score in (-np.inf, 0.25, 0.3, 10.0):
                a = I.topk_of_scores(s, ids, k, min_score, live)
                b = I.brute_topk_of_scores(s, ids, k, min_score, live)
                assert _same(a, b), (name, rows, k, min_score)
                # the properties the header states, from the result alone
                sc, r, i = a
                for q in range(len(s)):
                    got = r[q][r[q] >= 0]
                    assert np.all(np.diff(np.flatnonzero(r[q] >= 0)) == 1) and (len(got) == 0 or r[q, 0] >= 0)   # empties are a suffix
                    lab = i[q][i[q] >= 0]
                    assert len(set(lab.tolist())) == len(lab) and len(set(got.tolist())) == len(got)
                    assert np.array_equal(i[q][:len(got)], np.asarray(ids)[got]) and np.array_equal(sc[q][:len(got)], s[q, got])
                    assert np.all(sc[q][:len(got)] >= min_score) and np.all(np.isneginf(sc[q][len(got):])) and np.all(i[q][len(got):] == -1)
                    keys = list(zip((-sc[q][:len(got)]).tolist(), got.tolist()))
                    assert keys == sorted(keys)


def test_all_unlabelled_is_the_plain_top_k():
    rng = np.random.default_rng(3)
    q = rng.integers(-8, 9, (5, 64)).astype(np.float64) / 64
    g = rng.integers(-8, 9, (77, 64)).astype(np.float64) / 64
    g[10] = g[3] = g[60]                                                    # equal scores for every query
    for k in (1, 7, 32, 100):
        s, r, i = I.topk(q, g, np.full(77, -1), k)
        ref_s, ref_r = R.topk(q, g, k)
        assert np.array_equal(s, ref_s) and np.array_equal(r, ref_r) and np.all(i == -1)
        assert _same((s, r, i), I.brute_topk_of_scores(R.scores(q, g), np.full(77, -1), k))


def test_identity_keys_and_non_finite_scores():
    # identity 4: rows 0, 2, 5; its best key is row 2 (0.5 at the lower of two rows); row 1 is unlabelled; identity 9: rows 3, 4
    s = np.array([[0.25, 0.5, 0.5, np.nan, -np.inf, 0.5, 0.125]])
    ids = np.array([4, -1, 4, 9, 9, 4, 0])
    for f in (I.topk_of_scores, I.brute_topk_of_scores):
        sc, r, i = f(s, ids, 4)
        assert r.tolist() == [[1, 2, 6, -1]] and i.tolist() == [[-1, 4, 0, -1]]           # identity 9 has no selectable row
        assert sc[0, :3].tolist() == [0.5, 0.5, 0.125] and np.isneginf(sc[0, 3])
        sc, r, i = f(s, ids, 4, min_score=0.5)
        assert r.tolist() == [[1, 2, -1, -1]]                                               # equal to the threshold: kept
        sc, r, i = f(s, ids, 4, live=np.array([1, 1, 0, 1, 1, 1, 1], bool))
        assert r.tolist() == [[1, 5, 6, -1]] and i.tolist() == [[-1, 4, 0, -1]]           # the next row of identity 4 moves up
    assert I.labelled(ids) == 6 and I.labelled(ids, np.array([1, 1, 0, 1, 1, 1, 0], bool)) == 4
