"""Independent restatement of the face gallery's contract (include/rfd.h, "gallery"); pure numpy, no GPU (test infrastructure).

- storage: RNE to bf16 of the f64 value itself, as tests/exact_ref.py rounds (frexp / round-half-even / ldexp; never through a
  second format);
- score: the exact f64 dot product of the rounded vectors (bf16 x bf16 products need 16 bits, a sum of <= 1024 of them far less
  than 53: every score here is exact);
- order: the k best rows under (score descending, row ascending) by a stable lexsort on (-score, row); a gallery of fewer than
  k rows leaves (-inf, -1) in the tail."""
import numpy as np

U = 2.0 ** -24  # f32 unit round-off


def rne_bf16(x):
    """array -> f64 array of the nearest-even bf16 values (8 significant bits); finite inputs"""
    x = np.asarray(x, np.float64)
    m, e = np.frexp(x)
    return np.ldexp(np.rint(m * 256.0), e - 8)   # np.rint rounds half to even


def scores(queries, gallery):
    """exact f64 scores [n, rows] of the bf16-rounded queries against the bf16-rounded gallery"""
    return rne_bf16(queries) @ rne_bf16(gallery).T


def topk_of_scores(s, k):
    """(scores [n, k] f64, rows [n, k] i32) of a score matrix [n, rows] under (score descending, row ascending)"""
    n, rows = s.shape
    out_s, out_r = np.full((n, k), -np.inf), np.full((n, k), -1, np.int32)
    for i in range(n):
        order = np.lexsort((np.arange(rows), -s[i]))[:k]   # last key is the primary one
        out_s[i, :len(order)], out_r[i, :len(order)] = s[i, order], order
    return out_s, out_r


def topk(queries, gallery, k):
    g = np.asarray(gallery, np.float64).reshape(-1, np.asarray(queries).shape[1])
    return topk_of_scores(scores(queries, g), k)


def accumulation_radius(queries, gallery, s):
    """r = 16 * 2^-24 * sqrt(K * sum_d p_d^2) + 2^-24 |S| per (query, row): tests/exact_ref.py's radius of an f32 sum of K exact
    products p_d in any order, plus the rounding of the result"""
    q, g = rne_bf16(queries), rne_bf16(gallery)
    k = q.shape[1]
    return 16.0 * U * np.sqrt(k * ((q * q) @ (g * g).T)) + U * np.abs(s)


def input_bound(queries, gallery):
    """(2 * 2^-9 + 2^-18) * sum_d |q_d g_d| per (query, row): how far the bf16 rounding of both inputs can move the exact dot
    product of the unrounded f32 inputs (rfd.h derives it)"""
    return (2.0 * 2.0 ** -9 + 2.0 ** -18) * (np.abs(np.asarray(queries, np.float64)) @ np.abs(np.asarray(gallery, np.float64)).T)
