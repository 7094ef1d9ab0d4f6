"""Independent restatement of the gallery's filtered search (include/rfd.h, "tags"); pure numpy, no GPU (test infrastructure),
on top of gallery_identity_ref.

Every row carries a uint32 tag and every query q a pair (mask[q], value[q]); row r is eligible for q iff (tag[r] & mask[q]) ==
value[q], in uint32 arithmetic.  The result of q is the identity search of q on the rows that are live and eligible for q.

Two forms, written differently on purpose: `topk_of_scores` folds the eligibility into the liveness and hands each query's row
of scores to gallery_identity_ref.topk_of_scores; `brute_topk_of_scores` makes k rounds over all rows with Python integers and
tests the eligibility of every row where it meets it."""
import numpy as np

import gallery_identity_ref as I

ALL = 0xFFFFFFFF


def _u32(x, n=None):
    a = np.asarray(x, np.int64).reshape(-1)
    assert np.all((a >= 0) & (a <= ALL)), "a tag, mask or value outside 32 bits"
    assert n is None or a.shape == (n,)
    return a.astype(np.uint32)


def eligible(tags, mask, value):
    """tags [rows], mask [n], value [n] -> bool [n, rows]"""
    t, m, v = _u32(tags), _u32(mask), _u32(value)
    return (t[None, :] & m[:, None]) == v[:, None]


def topk_of_scores(s, ids, tags, mask, value, k, min_score=-np.inf, live=None):
    """s [n, rows] f64, ids [rows] (>= 0 or -1), tags [rows] u32, mask / value [n] u32, live [rows] bool or None ->
    (scores [n, k] f64, rows [n, k] i32, ids [n, k] i32)"""
    s = np.asarray(s, np.float64)
    n, rows = s.shape
    tags, mask, value = _u32(tags, rows), _u32(mask, n), _u32(value, n)
    live = np.ones(rows, bool) if live is None else np.asarray(live, bool)
    out = I._empty(n, k)
    for q in range(n):
        live_q = live & ((tags & mask[q]) == value[q])
        for dst, src in zip(out, I.topk_of_scores(s[q:q + 1], ids, k, min_score, live_q)):
            dst[q] = src[0]
    return out


def brute_topk_of_scores(s, ids, tags, mask, value, k, min_score=-np.inf, live=None):
    """the same by k rounds over all rows"""
    s = np.asarray(s, np.float64)
    n, rows = s.shape
    tags, mask, value = [int(x) for x in _u32(tags, rows)], [int(x) for x in _u32(mask, n)], [int(x) for x in _u32(value, n)]
    ids = [int(x) for x in np.asarray(ids).reshape(-1)]
    out_s, out_r, out_i = [[-np.inf] * k for _ in range(n)], [[-1] * k for _ in range(n)], [[-1] * k for _ in range(n)]
    for q in range(n):
        taken_rows, taken_ids = set(), set()
        for j in range(k):
            best = None
            for r in range(rows):
                x = s[q, r]
                if x != x or x == -np.inf:                          # NaN and -inf are never selected
                    continue
                if live is not None and not live[r]:
                    continue
                if (tags[r] & mask[q]) != value[q]:
                    continue
                if r in taken_rows or (ids[r] >= 0 and ids[r] in taken_ids):
                    continue
                if best is None or x > s[q, best]:                  # rows ascend: an equal score keeps the lower row
                    best = r
            if best is None or not s[q, best] >= min_score:         # the best key left is below the threshold: so are all after it
                break
            out_s[q][j], out_r[q][j], out_i[q][j] = s[q, best], best, ids[best]
            taken_rows.add(best)
            if ids[best] >= 0:
                taken_ids.add(ids[best])
    return np.array(out_s, np.float64).reshape(n, k), np.array(out_r, np.int32).reshape(n, k), np.array(out_i, np.int32).reshape(n, k)
