"""Independent restatement of the gallery's self-join (include/rfd.h, "nearest"); pure numpy, no GPU (test infrastructure), on
top of gallery_ref.scores.

For every row a of [row0, row0 + n): the best row b under the total order (score descending, row ascending) among the rows that
are live, are not a, are allowed by the mode (OTHER_IDENTITY refuses id[a] >= 0 and id[b] == id[a]; an unlabelled row is an
identity of its own), agree with a under the tag mask, and whose score is neither NaN nor -inf and is >= min_score.  The entry
is (score, b, id[b]); where a is removed or no row qualifies it is the empty entry (-inf, -1, -1).

Two forms, written differently on purpose: `nearest_of_scores` masks whole rows of the score matrix and takes one lexsort per
row; `naive_nearest_of_scores` is the double loop, one candidate at a time."""
import numpy as np

OTHER_ROW, OTHER_IDENTITY = 0, 1
ALL = 0xFFFFFFFF


def _arrays(rows, ids, tags, live):
    ids = np.full(rows, -1, np.int64) if ids is None else np.asarray(ids, np.int64)
    tags = np.zeros(rows, np.int64) if tags is None else np.asarray(tags, np.int64) & ALL
    live = np.ones(rows, bool) if live is None else np.asarray(live, bool)
    assert ids.shape == tags.shape == live.shape == (rows,)
    return ids, tags, live


def nearest_of_scores(s, row0=0, n=None, mode=OTHER_ROW, min_score=-np.inf, tag_mask=0, ids=None, tags=None, live=None):
    """s [rows, rows] f64, s[a, b] = score(a, b) -> (scores [n] f64, rows [n] i32, ids [n] i32) of rows [row0, row0 + n)"""
    s = np.asarray(s, np.float64)
    rows = s.shape[0]
    assert s.shape == (rows, rows)
    n = rows - row0 if n is None else n
    ids, tags, live = _arrays(rows, ids, tags, live)
    masked = tags & (int(tag_mask) & ALL)
    out_s, out_r, out_i = np.full(n, -np.inf), np.full(n, -1, np.int32), np.full(n, -1, np.int32)
    every = np.arange(rows)
    for a in range(row0, row0 + n):
        if not live[a]:
            continue
        ok = live & (every != a) & (masked == masked[a]) & ~np.isnan(s[a]) & ~np.isneginf(s[a])
        if mode == OTHER_IDENTITY and ids[a] >= 0:
            ok &= ids != ids[a]
        with np.errstate(invalid="ignore"):
            ok &= s[a] >= min_score
        cand = np.flatnonzero(ok)
        if len(cand):
            b = cand[np.lexsort((cand, -s[a, cand]))[0]]
            out_s[a - row0], out_r[a - row0], out_i[a - row0] = s[a, b], b, ids[b]
    return out_s, out_r, out_i


def naive_nearest_of_scores(s, row0=0, n=None, mode=OTHER_ROW, min_score=-np.inf, tag_mask=0, ids=None, tags=None, live=None):
    """the same by the double loop"""
    s = np.asarray(s, np.float64)
    rows = s.shape[0]
    n = rows - row0 if n is None else n
    ids, tags, live = _arrays(rows, ids, tags, live)
    out_s, out_r, out_i = np.full(n, -np.inf), np.full(n, -1, np.int32), np.full(n, -1, np.int32)
    for a in range(row0, row0 + n):
        best = -1
        for b in range(rows):
            v = s[a, b]
            if b == a or not live[a] or not live[b] or v != v or v == -np.inf or not v >= min_score:
                continue
            if mode == OTHER_IDENTITY and ids[a] >= 0 and ids[b] == ids[a]:
                continue
            if (int(tags[a]) ^ int(tags[b])) & int(tag_mask) & ALL:
                continue
            if best < 0 or v > s[a, best]:   # rows ascend: an equal score keeps the lower row
                best = b
        if best >= 0:
            out_s[a - row0], out_r[a - row0], out_i[a - row0] = s[a, best], best, ids[best]
    return out_s, out_r, out_i


def nearest(gallery, **kw):
    """of stored values gallery [rows, dim] (rounded to bf16 here, as the gallery stores them; a removed row's values do not matter)"""
    import gallery_ref as R
    g = np.asarray(gallery, np.float64)
    return nearest_of_scores(R.scores(g, g), **kw)
