"""Independent restatement of the gallery's identity search (include/rfd.h, "identities"); pure numpy, no GPU (test
infrastructure), on top of gallery_ref.scores.

For each query: every identity's key is its best live row under the total order (score descending, row ascending); a row whose
identity is -1 is an identity of its own; the result is the k best identity keys under that same order: (score, row, identity).
Entries with not (score >= min_score) become the empty entry (-inf, -1, -1), and so does the tail beyond the identities there
are.  A NaN or -inf score is never selected.

Two forms, written differently on purpose: `topk_of_scores` sorts the rows once and keeps each identity's first occurrence;
`brute_topk_of_scores` makes k rounds over all rows, O(rows * k), and in each takes the best row whose identity is not out yet."""
import numpy as np

NO_IDENTITY = -1


def _usable(s_row, live):
    ok = ~np.isnan(s_row) & ~np.isneginf(s_row)
    return ok if live is None else ok & np.asarray(live, bool)


def _empty(n, k):
    return np.full((n, k), -np.inf), np.full((n, k), -1, np.int32), np.full((n, k), NO_IDENTITY, np.int32)


def _threshold(out, min_score):
    s, r, i = out
    below = ~(s >= min_score)
    s[below], r[below], i[below] = -np.inf, -1, NO_IDENTITY
    return s, r, i


def topk_of_scores(s, ids, k, min_score=-np.inf, live=None):
    """s [n, rows] f64, ids [rows] (>= 0 or -1), live [rows] bool or None -> (scores [n, k] f64, rows [n, k] i32, ids [n, k] i32)"""
    s, ids = np.asarray(s, np.float64), np.asarray(ids, np.int64)
    n, rows = s.shape
    assert ids.shape == (rows,) and np.all(ids >= NO_IDENTITY)
    own = np.where(ids >= 0, ids, -2 - np.arange(rows))           # an unlabelled row: a label nobody else has
    out = _empty(n, k)
    for q in range(n):
        cand = np.flatnonzero(_usable(s[q], live))
        order = cand[np.lexsort((cand, -s[q, cand]))]              # best key first
        _, first = np.unique(own[order], return_index=True)       # every identity's first occurrence = its best key
        keep = order[np.sort(first)][:k]
        out[0][q, :len(keep)], out[1][q, :len(keep)], out[2][q, :len(keep)] = s[q, keep], keep, ids[keep]
    return _threshold(out, min_score)


def brute_topk_of_scores(s, ids, k, min_score=-np.inf, live=None):
    """the same by k rounds over all rows"""
    s, ids = np.asarray(s, np.float64), np.asarray(ids, np.int64)
    n, rows = s.shape
    out = _empty(n, k)
    for q in range(n):
        usable = _usable(s[q], live)
        taken_ids, taken_rows = set(), set()
        for j in range(k):
            best = -1
            for r in range(rows):
                if not usable[r] or r in taken_rows or (ids[r] >= 0 and int(ids[r]) in taken_ids):
                    continue
                if best < 0 or s[q, r] > s[q, best]:               # rows ascend: an equal score keeps the lower row
                    best = r
            if best < 0:
                break
            out[0][q, j], out[1][q, j], out[2][q, j] = s[q, best], best, ids[best]
            taken_rows.add(best)
            if ids[best] >= 0:
                taken_ids.add(int(ids[best]))
    return _threshold(out, min_score)


def topk(queries, gallery, ids, k, min_score=-np.inf, live=None):
    import gallery_ref as R
    g = np.asarray(gallery, np.float64).reshape(-1, np.asarray(queries).shape[1])
    return topk_of_scores(R.scores(queries, g), ids, k, min_score, live)


def labelled(ids, live=None):
    """how many live rows carry an identity >= 0 (rfd_gallery_identities)"""
    ids = np.asarray(ids)
    return int(((ids >= 0) & (np.ones(len(ids), bool) if live is None else np.asarray(live, bool))).sum())
