"""Shared by tests/test_exposure_*.py: the restatement of include/slim_gpu_exposure.h in Python ints and np.bincount
(the yardstick: never the code under test), list generators, and thin wrappers of the two list calls."""
import ctypes as C

import numpy as np

from slim_amd import _lib

P = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)  # noqa: E731

INT_FIELDS = ("lists", "slots", "tail_slots", "outside", "distinct", "ncols")
DOUBLE_FIELDS = ("coverage", "tail_share", "gini", "avg_pop")

WORKED = dict(ncols=6, ids=np.array([[0, 1, 2], [0, 2, 4], [0, 0, 5]], np.int32), counts=np.array([3, 2, 3], np.int32),
              cutoffs=(1, 3), fmarker=np.array([0, 0, 1, 1, 1, 1], np.int32),
              pop=np.array([10, 5, 3, 1, 1, 2], np.uint32))  # (the 4 of list 1 lies beyond its length)


def restate(ncols, ids, counts, cutoffs, pop=None, fmarker=None):
    """(E [K, ncols] uint32, one dict per cutoff): the header's definition, integers in Python ints, every double
    float(num) / float(den)."""
    ids = np.asarray(ids, np.int64)
    nlists = ids.shape[0]
    N = ids.shape[1] if ids.ndim == 2 else 0
    cnt = np.full(nlists, N, np.int64) if counts is None else np.asarray(counts, np.int64)
    ratio = lambda a, b: 0.0 if b == 0 else float(a) / float(b)  # noqa: E731
    Es, out = [], []
    for c in cutoffs:
        keep = np.arange(N)[None, :] < np.minimum(cnt, c)[:, None]
        v = ids.reshape(nlists, N)[keep]
        inside = (v >= 0) & (v < ncols)
        e = np.bincount(v[inside], minlength=ncols)
        x = sorted(int(t) for t in e)
        slots = sum(x)
        gnum = sum((2 * j - ncols - 1) * xj for j, xj in enumerate(x, 1))
        tail = 0 if fmarker is None else sum(int(e[i]) for i in range(ncols)
                                             if i >= len(fmarker) or fmarker[i] != 0)
        popnum = 0 if pop is None else sum(int(e[i]) * int(pop[i]) for i in range(ncols))
        distinct = int((e > 0).sum())
        out.append(dict(lists=nlists, slots=slots, tail_slots=tail, outside=int((~inside).sum()), distinct=distinct,
                        ncols=ncols, coverage=ratio(distinct, ncols), tail_share=ratio(tail, slots),
                        gini=ratio(gnum, ncols * slots), avg_pop=ratio(popnum, slots)))
        Es.append(e.astype(np.uint32))
    return np.array(Es, np.uint32).reshape(len(cutoffs), ncols), out


def _field(s, name):
    return s[name] if isinstance(s, dict) else getattr(s, name)


def same_summary(got, want):
    """Every integer equal, every double bit-equal; prints the first difference."""
    for k, w in enumerate(want):
        for name in INT_FIELDS:
            if int(_field(got[k], name)) != w[name]:
                print("cutoff %d: %s is %r, want %r" % (k, name, _field(got[k], name), w[name]))
                return False
        for name in DOUBLE_FIELDS:
            g = np.float64(_field(got[k], name))
            if g.view(np.int64) != np.float64(w[name]).view(np.int64):
                print("cutoff %d: %s is %r, want %r" % (k, name, g, w[name]))
                return False
    return True


def random_lists(rng, ncols, nlists, N, outside=False, hot=()):
    """ids [nlists, N] and counts [nlists] in [0, N]: every slot holds a valid id -- also beyond counts[q], so a
    counter that trusts a sentinel fails; repeats inside lists; `hot` ids drawn more often; with `outside` a few
    ids outside [0, ncols) in counted places."""
    ids = rng.integers(0, ncols, (nlists, N)).astype(np.int32)
    if len(hot):
        m = rng.random((nlists, N)) < 0.5
        ids[m] = rng.choice(np.asarray(hot, np.int32), size=int(m.sum()))
    if N > 1:
        rep = rng.random(nlists) < 0.3
        ids[rep, 1] = ids[rep, 0]
    counts = rng.integers(0, N + 1, nlists).astype(np.int32)
    if nlists > 2:
        counts[0], counts[1] = N, 0
    if N > 1 and nlists > 3:
        counts[2] = N - 1
    if outside and nlists:
        bad = np.array([-1, -7, ncols, ncols + 9, 2 ** 31 - 1, -2 ** 31], np.int64).astype(np.int32)
        rows = rng.integers(0, nlists, 12)
        ids[rows, 0] = bad[np.arange(12) % bad.size]
        counts[rows] = np.maximum(counts[rows], 1)
    return ids, counts


def _outputs(K, ncols, want_E, want_summary):
    E = np.zeros((K, max(ncols, 1)), np.uint32) if want_E else None
    summ = (_lib.Exposure * K)() if want_summary else None
    return E, summ


def call_host(lib, ncols, ids, counts, cutoffs, pop=None, fmarker=None, want_E=True, want_summary=True):
    """SLIMGPU_ListExposure: (status, E, summaries)."""
    ids = np.ascontiguousarray(ids, np.int32)
    cut = np.ascontiguousarray(cutoffs, np.int32)
    E, summ = _outputs(cut.size, ncols, want_E, want_summary)
    N = ids.shape[1] if ids.ndim == 2 else 1
    rc = lib.SLIMGPU_ListExposure(ncols, P(pop), P(fmarker), 0 if fmarker is None else fmarker.size, ids.shape[0], N,
                                  P(ids) if ids.size else None, P(counts), cut.size, P(cut), P(E),
                                  None if summ is None else C.cast(summ, C.c_void_p))
    return rc, E, summ


def call_device(lib, mat, ids, counts, cutoffs, fmarker=None, want_E=True, want_summary=True):
    """SLIMGPU_MatrixListExposure on a DeviceMatrix: (status, E, summaries)."""
    ids = np.ascontiguousarray(ids, np.int32)
    cut = np.ascontiguousarray(cutoffs, np.int32)
    E, summ = _outputs(cut.size, mat.ncols, want_E, want_summary)
    N = ids.shape[1] if ids.ndim == 2 else 1
    rc = lib.SLIMGPU_MatrixListExposure(mat.handle, P(fmarker), 0 if fmarker is None else fmarker.size, ids.shape[0],
                                        N, P(ids) if ids.size else None, P(counts), cut.size, P(cut), P(E),
                                        None if summ is None else C.cast(summ, C.c_void_p))
    return rc, E, summ
