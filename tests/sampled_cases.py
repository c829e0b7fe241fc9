"""Shared by tests/test_sampled_candidates*.py: the sampler of include/slim_gpu_sample.h restated in numpy FROM THE
HEADER'S TEXT (never from the C++), test matrices over the cases of tests/filtered_cases.py, and the calls that
bring a set's rows back.

The yardstick is never the code under test: the rows are numpy's, and the expected figures are those of the
EXISTING calls SLIMGPU_CandSetCreate + SLIMGPU_ModelEvaluateCandidates on numpy's rows.
"""
import ctypes as C

import numpy as np
import scipy.sparse as sp

from slim_amd.constants import SLIM_OK

P = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)  # noqa: E731
U = np.uint64
G = U(0x9E3779B97F4A7C15)
GRID = (1, 63, 64, 65, 99)      # nnegs of the sparse rule: around the 64 draws of one batch
# on 1 500 items: at 700 a user is dense when E > 50, which most are and the short and the empty histories are not --
# both rules in one set; at 750 every user is (2 * (1 + 750) > 1 500)
DENSE = (700, 750)


def mix64(z):
    with np.errstate(over="ignore"):
        z = np.asarray(z, U)
        z = z ^ (z >> U(30))
        z = z * U(0xBF58476D1CE4E5B9)
        z = z ^ (z >> U(27))
        z = z * U(0x94D049BB133111EB)
        return z ^ (z >> U(31))


def base(seed, u):
    with np.errstate(over="ignore"):
        return mix64(U(seed) + G * U(u + 1))


def key(seed, u, d):
    with np.errstate(over="ignore"):
        return mix64(base(seed, u) + G * (np.asarray(d, U) + U(1)))


def item(seed, u, d, ncols):
    return (((key(seed, u, d) >> U(32)) * U(ncols)) >> U(32)).astype(np.int64)


def rule(E, nnegs, ncols):
    return "sparse" if 2 * (E + nnegs) <= ncols else "dense"


def negatives(seed, u, X, nnegs, ncols):
    """The negatives of user u, whose history and test ids inside [0, ncols) are the distinct ids X."""
    if rule(X.size, nnegs, ncols) == "sparse":
        draws = item(seed, u, np.arange(16 * nnegs + 1024), ncols)
        _, first = np.unique(draws, return_index=True)          # a draw counts at its first occurrence
        seq = draws[np.sort(first)]
        return seq[~np.isin(seq, X)][:nnegs].astype(np.int32)
    free = np.setdiff1d(np.arange(ncols), X)
    k = key(seed, u, free)
    return free[np.lexsort((free, k))][:min(nnegs, free.size)].astype(np.int32)


def sampled_rows(R, tptr, tind, ncols, nnegs, seed, users=None):
    """(indptr, indices) of the sampled set: min(rows of R, test rows) rows; a selected user with a test row gets its
    negatives, then the test row as given; every other row is empty."""
    nall = min(R.shape[0], tptr.size - 1)
    sel = set(range(nall)) if users is None else set(int(u) for u in users)
    ptr, ind = [0], []
    for u in range(nall):
        t = tind[tptr[u]:tptr[u + 1]]
        if u in sel and t.size:
            both = np.concatenate([R.indices[R.indptr[u]:R.indptr[u + 1]], t])
            X = np.unique(both[(both >= 0) & (both < ncols)])
            ind += negatives(seed, u, X, nnegs, ncols).tolist() + t.tolist()
        ptr.append(len(ind))
    return np.array(ptr, np.int64), np.array(ind, np.int32)


def held_out_rows(case, seed):
    """Test rows for a case, as a scipy CSR taken as it is: one-entry rows, user 5 with three entries, user 7 with an
    id of its history (and one outside), the empty-history users with a row, every 10th user (u % 10 == 3) without."""
    rng = np.random.default_rng(seed)
    ptr, ind = [0], []
    for u in range(case.nusers):
        hist = case.R.indices[case.R.indptr[u]:case.R.indptr[u + 1]]
        free = np.setdiff1d(np.arange(case.ncols), hist)
        if u % 10 != 3:
            row = rng.choice(free, size=3 if u == 5 else 1, replace=False).tolist()
            if u == 7:
                row = [int(hist[0])] + row
            ind += row
        ptr.append(len(ind))
    T = sp.csr_matrix((case.nusers, case.ncols), dtype=np.float32)
    T.indptr, T.indices, T.data = np.array(ptr, np.int32), np.array(ind, np.int32), np.ones(len(ind), np.float32)
    return T


def csr(rows, ncols):
    """A scipy CSR with exactly these rows (lists of ids, kept as given)."""
    M = sp.csr_matrix((len(rows), ncols), dtype=np.float32)
    M.indptr = np.cumsum([0] + [len(r) for r in rows]).astype(np.int32)
    M.indices = np.array([i for r in rows for i in r], np.int32)
    M.data = np.ones(M.indices.size, np.float32)
    return M


def set_rows(lib, cs):
    """SLIMGPU_CandSetInfo + SLIMGPU_CandSetRows: (indptr, indices, ncols)."""
    nrows, ncols, size = C.c_int32(), C.c_int32(), C.c_int64()
    assert lib.SLIMGPU_CandSetInfo(cs, C.byref(nrows), C.byref(ncols), C.byref(size)) == SLIM_OK
    ptr, ind = np.full(nrows.value + 1, -1, np.int64), np.full(size.value + 1, -7, np.int32)
    assert lib.SLIMGPU_CandSetRows(cs, P(ptr), P(ind)) == SLIM_OK
    assert ptr[-1] == size.value and ind[-1] == -7
    return ptr, ind[:-1], ncols.value


def host_sample(lib, ncols, hr, ht, nnegs, seed, users=None):
    """SLIMGPU_CandSetSample: (status, handle)."""
    h = C.c_void_p()
    u = None if users is None else np.ascontiguousarray(users, np.int32)
    return lib.SLIMGPU_CandSetSample(ncols, hr, ht, 0 if u is None else u.size, P(u), nnegs, seed, C.byref(h)), h


PAIR = r"(l1r: \S+ l2r: \S+ nnz:\s+\d+ hr: \S+ hr_head: \S+ hr_tail: \S+ arhr: \S+)"
GRID_L1, GRID_L2 = [1.0, 2.0], [1.0, 5.0]


def grid_by_hand(R, T, nnegs, seed, users=None, nrcmds=10):
    """The 2 x 2 grid through existing calls: learn_resident, then SLIMGPU_ModelEvaluateCandidates on a
    SLIMGPU_CandSetCreate set of numpy's rows, beside the full-catalogue evaluation.  Returns [(l1, l2, sampled,
    full)] and the entries of the set."""
    from slim_amd.engine import DeviceMatrix
    mat = DeviceMatrix.from_scipy(R)
    mat.expect_solves(4)
    rows = sampled_rows(R, T.indptr.astype(np.int64), T.indices, mat.ncols, nnegs, seed, users=users)
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


def check_grid_lines(lines, got, result=None):
    """The printed pair lines carry the by-hand sampled figures; the best pairs are chosen from them."""
    assert len(lines) == len(got) == 4
    best_hr = best_ar = (0.0, 0.0, 0.0, 0.0)
    for line, (l1, l2, g, full) in zip(lines, got):
        print(line, g, "full catalogue:", full["hr"], full["arhr"])
        assert g["nvalid"] > 0 and g["hr"] > 0
        assert "hr: %.4f hr_head: %.4f hr_tail: %.4f arhr: %.4f" % (g["hr"], g["hr_head"], g["hr_tail"],
                                                                    g["arhr"]) in line
        assert line.startswith("l1r: %.2e l2r: %.2e " % (l1, l2))
        if g["hr"] > best_hr[2]:
            best_hr = (l1, l2, g["hr"], g["arhr"])
        if g["arhr"] > best_ar[3]:
            best_ar = (l1, l2, g["hr"], g["arhr"])
    if result is not None:
        assert result == dict(bestHR=best_hr, bestAR=best_ar)      # the eight best-values, as doubles
