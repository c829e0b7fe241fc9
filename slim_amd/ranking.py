"""Ranking metrics from the ranks of the held-out items (`Evaluator.ranks`): plain numpy over
``(ranks, indptr)``, in doubles, one value per evaluated position (user order).

``ranks[indptr[q]:indptr[q + 1]]`` are the ranks of the test entries of position q among that user's
candidates: 1 is the head of every list, 0 means the item is in no list of any length.  A test item listed
twice carries one rank twice and counts once, as one list slot does.  Users without test entries give 0.
"""
import numpy as np


def _rows(ranks, indptr):
    ranks = np.asarray(ranks)
    indptr = np.asarray(indptr, dtype=np.int64)
    for q in range(indptr.size - 1):
        row = ranks[indptr[q]:indptr[q + 1]]
        yield q, row.size, np.unique(row[row > 0])


def hit_rate(ranks, indptr, k):
    """Per position: distinct test items ranked <= k, over the length of the test row."""
    out = np.zeros(len(indptr) - 1, np.float64)
    for q, n, r in _rows(ranks, indptr):
        if n:
            out[q] = float(np.count_nonzero(r <= k)) / n
    return out


def ndcg(ranks, indptr, k):
    """Per position: sum of 1 / log2(1 + rank) over the distinct ranks <= k, over the ideal: the same sum
    over ranks 1 .. min(len, k)."""
    out = np.zeros(len(indptr) - 1, np.float64)
    for q, n, r in _rows(ranks, indptr):
        if n:
            r = r[r <= k].astype(np.float64)
            ideal = np.sum(1.0 / np.log2(1.0 + np.arange(1, min(n, int(k)) + 1, dtype=np.float64)))
            out[q] = np.sum(1.0 / np.log2(1.0 + r)) / ideal
    return out


def mrr(ranks, indptr):
    """Per position: 1 / the best (smallest non-zero) rank of the user's test items; 0 when none is ranked."""
    out = np.zeros(len(indptr) - 1, np.float64)
    for q, n, r in _rows(ranks, indptr):
        if r.size:
            out[q] = 1.0 / float(r.min())
    return out
