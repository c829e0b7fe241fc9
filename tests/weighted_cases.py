"""Shared by tests/test_weighted_negatives*.py: THE WEIGHTED RULE of include/slim_gpu_sample.h restated in numpy FROM
THE HEADER'S TEXT (never from the C++), with the 128-bit product in 32-bit halves (pinned to Python integers by
tests/test_later_positions.py), the weight arrays of the tests, and the calls that make weighted sets.

The yardstick is never the code under test: the rows are numpy's, and the expected figures are those of the EXISTING
calls SLIMGPU_CandSetCreate + SLIMGPU_ModelEvaluateCandidates on numpy's rows.
"""
import ctypes as C

import numpy as np

from sampled_cases import GRID, GRID_L1, GRID_L2, P, U, csr, key

NAMES = ("counts", "zipf", "cliff")
# beyond GRID, on the 1 500-item cases: rows that phase 2 leaves short
SHORT = (("cliff", 700), ("zipf", 1450))
BATCH = 1024            # draws per numpy step; the rule does not know it


def grid(ncols):
    """(weights name, nnegs): the batch edge of 64 draws, both phases, full and short rows."""
    return [(w, n) for w in NAMES for n in GRID] + (list(SHORT) if ncols == 1500 else [])


def weights(name, R, n):
    """The weight arrays of the tests over n items, as uint32."""
    if name == "counts":
        w = np.bincount(R.indices, minlength=n)
    elif name == "zipf":
        rng = np.random.default_rng(77)
        w = 1_000_000 // (1 + rng.permutation(n))
        w[rng.choice(n, 100, replace=False)] = 0
    elif name == "cliff":
        p = np.random.default_rng(78).permutation(n)
        w = np.zeros(n, np.int64)
        w[p[:50]] = 4_000_000_000
        w[p[50:450]] = 1
    else:
        raise KeyError(name)
    assert w.min() >= 0 and w.max() < 2 ** 32
    return w.astype(np.uint32)


def hand_made(zero_tail):
    """The 40-item matrix of tests/test_sampled_candidates*.py -- nothing free, fewer than nnegs free, no test row,
    test ids outside and repeated -- with weights 1 + (i % 7), and with weight 0 on items 35-39."""
    hist = [list(range(40)), list(range(0, 35)), list(range(10, 24)), list(range(10, 25)), [1, 2, 3], []]
    test = [[39], [35, 3], [30], [30], [], [7, 7, 44]]
    w = (1 + np.arange(40) % 7).astype(np.uint32)
    if zero_tail:
        w[35:] = 0
    return csr(hist, 40), csr(test, 45), w


def prefix(w):
    """C[0 .. n]: C[i] = w[0] + ... + w[i-1] in 64 bits."""
    return np.concatenate([[0], np.cumsum(w.astype(U), dtype=U)]).astype(U)


def mulhi64_python(keys, m):
    """The upper 64 bits of key * m, exact: Python integers."""
    return np.array([(int(k) * int(m)) >> 64 for k in np.atleast_1d(keys)], dtype=U)


def mulhi64(keys, m):
    """The upper 64 bits of key * m in numpy, by the schoolbook product of 32-bit halves: each of the four partial
    products and each sum below stays under 2^64.  tests/test_later_positions.py pins it to mulhi64_python."""
    k, m = np.atleast_1d(np.asarray(keys, U)), U(int(m))
    lo32, s32 = U(0xFFFFFFFF), U(32)
    k0, k1, m0, m1 = k & lo32, k >> s32, m & lo32, m >> s32
    mid = k1 * m0 + ((k0 * m0) >> s32)                          # <= (2^32 - 1)^2 + 2^32 - 2
    mid2 = k0 * m1 + (mid & lo32)
    return k1 * m1 + (mid >> s32) + (mid2 >> s32)


def weighted_negatives(seed, u, X, nnegs, w, Cw=None):
    """(negatives, draws of phase 1 that were made, picks of phase 2) of user u, whose history and test ids inside
    [0, ncols) are the distinct ids X."""
    n = w.size
    Cw = prefix(w) if Cw is None else Cw
    T = int(Cw[n])
    assert T > 0
    D = 16 * nnegs + 1024
    taken = np.zeros(n, bool)
    taken[X] = True
    out, d = [], 0
    while d < D and len(out) < nnegs:                          # phase 1
        m = min(BATCH, D - d)
        r = mulhi64(key(seed, u, np.arange(d, d + m)), T)
        ids = np.searchsorted(Cw[1:], r, side="right")         # the i with C[i] <= r < C[i+1]
        ids = ids[~taken[ids]]
        _, first = np.unique(ids, return_index=True)           # a draw counts at its first occurrence
        seq = ids[np.sort(first)][:nnegs - len(out)]
        taken[seq] = True
        out += seq.tolist()
        d += m
    picks = 0
    if len(out) < nnegs:                                       # phase 2
        mass = np.where(taken, 0, w).astype(U)                 # F: positive weight, not in X, not accepted
        while len(out) < nnegs:
            left = int(mass.sum(dtype=U))
            if left == 0:
                break
            r = mulhi64(key(seed, u, D + picks), left)[0]
            i = int(np.searchsorted(np.cumsum(mass, dtype=U), r, side="right"))   # the running sum first exceeds r
            assert mass[i] > 0
            out.append(i)
            mass[i] = 0
            picks += 1
    return np.array(out, np.int32), min(d, D), picks


_ROWS = {}


def weighted_user(tag, R, tptr, tind, ncols, nnegs, seed, w, u):
    """weighted_negatives for one user, kept: a subset's rows are the whole set's rows of those users.  tag names
    the inputs (case, test rows, weights)."""
    k = (tag, nnegs, seed, u)
    if k not in _ROWS:
        t = tind[tptr[u]:tptr[u + 1]]
        both = np.concatenate([R.indices[R.indptr[u]:R.indptr[u + 1]], t])
        X = np.unique(both[(both >= 0) & (both < ncols)])
        _ROWS[k] = weighted_negatives(seed, u, X, nnegs, w, _ROWS.setdefault((tag, "C"), prefix(w)))
    return _ROWS[k]


def weighted_rows(tag, R, tptr, tind, ncols, nnegs, seed, w, users=None):
    """(indptr, indices) of the weighted set, as sampled_cases.sampled_rows lays the uniform one out."""
    nall = min(R.shape[0], tptr.size - 1)
    sel = set(range(nall)) if users is None else set(int(u) for u in users)
    ptr, ind = [0], []
    for u in range(nall):
        t = tind[tptr[u]:tptr[u + 1]]
        if u in sel and t.size:
            ind += weighted_user(tag, R, tptr, tind, ncols, nnegs, seed, w, u)[0].tolist() + t.tolist()
        ptr.append(len(ind))
    return np.array(ptr, np.int64), np.array(ind, np.int32)


def host_sample_weighted(lib, ncols, hr, ht, nnegs, seed, w, users=None):
    """SLIMGPU_CandSetSampleWeighted: (status, handle); w: uint32 array or None (popularity)."""
    h = C.c_void_p()
    u = None if users is None else np.ascontiguousarray(users, np.int32)
    w = None if w is None else np.ascontiguousarray(w, np.uint32)
    return lib.SLIMGPU_CandSetSampleWeighted(ncols, hr, ht, 0 if u is None else u.size, P(u), nnegs, seed, P(w),
                                             C.byref(h)), h


def device_sample_weighted(lib, ev, nnegs, seed, w):
    """SLIMGPU_EvalSetSampleCandidatesWeighted: (status, handle)."""
    h = C.c_void_p()
    w = None if w is None else np.ascontiguousarray(w, np.uint32)
    return lib.SLIMGPU_EvalSetSampleCandidatesWeighted(ev.handle, nnegs, seed, P(w), C.byref(h)), h


def grid_by_hand_popularity(R, T, nnegs, seed, users=None, nrcmds=10):
    """sampled_cases.grid_by_hand on numpy's popularity rows: the 2 x 2 grid through existing calls only."""
    from slim_amd.engine import DeviceMatrix
    mat = DeviceMatrix.from_scipy(R)
    mat.expect_solves(4)
    w = weights("counts", R, mat.ncols)
    rows = weighted_rows(("grid", object()), R, T.indptr.astype(np.int64), T.indices, mat.ncols, nnegs, seed, w,
                         users=users)
    cset = mat.candidate_set(rows)
    ev = mat.evaluator(T, nrcmds=nrcmds, users=users)
    prev, got = None, []
    for l1 in GRID_L1:
        for l2 in GRID_L2:
            cur, _ = mat.learn_resident(warm=prev, l1r=l1, l2r=l2, optTol=1e-7, niters=200)
            if prev is not None:
                prev.free()
            prev = cur
            got.append((l1, l2, ev.evaluate_candidates(cur, cset)[0], ev.evaluate(cur)))
    prev.free()
    for h in (ev, cset, mat):
        h.close()
    return got, int(rows[1].size)
