"""Shared by tests/test_filtered_lists*.py and tests/test_filtered_host.py: the inputs of tests/test_long_lists.py
(its generators are restated here) and the yardstick of the candidate filters (include/slim_gpu_filter.h).

The yardstick is never the code under test: the EXISTING host scorer (Py_SLIM_Predict under SLIM_PREDICT=cpu) is
asked once per case for lists of length ncols, the full ranking; the expected filtered list of length n is that
ranking with the disallowed and the excluded ids removed, cut at n.
"""
import ctypes as C
import os

import numpy as np
import scipy.sparse as sp

from slim_amd import _lib
from slim_amd.constants import SLIM_OK
from slim_amd.engine import DeviceMatrix, _scipy_to_model_handle

NO_HISTORY = (11, 150)
P = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731


def wrap(lib, M, binary=False):
    M = sp.csr_matrix(M)
    h = C.c_void_p()
    val = np.ascontiguousarray(M.data, np.float32)
    assert lib.Py_csr_wrapper(M.shape[0], np.ascontiguousarray(M.indptr, np.intp),
                              np.ascontiguousarray(M.indices, np.int32),
                              None if binary else P(val), C.byref(h)) == SLIM_OK
    return h


def make_model(nitems, lo, hi, ties, seed):
    rng = np.random.default_rng(seed)
    ptr, ind, val = [0], [], []
    for _ in range(nitems):
        k = int(rng.integers(lo, hi + 1))
        ind.append(np.sort(rng.choice(nitems, size=k, replace=False)))
        val.append(rng.choice([0.25, 0.5], size=k) if ties else rng.uniform(-0.2, 1.0, size=k))
        ptr.append(ptr[-1] + k)
    return sp.csr_matrix((np.concatenate(val).astype(np.float32), np.concatenate(ind).astype(np.int32), ptr),
                         shape=(nitems, nitems))


def make_history(nusers, nitems, density, empty, binary, seed):
    rng = np.random.default_rng(seed)
    R = sp.random(nusers, nitems, density=density, format="lil", random_state=rng, dtype=np.float32)
    for u in empty:
        R.rows[u], R.data[u] = [], []
    R = sp.csr_matrix(R)
    R.data[:] = 1.0 if binary else rng.integers(1, 6, R.nnz).astype(np.float32)
    R.sort_indices()
    return R


class Case(object):
    """Model, histories, their host handles and the host scorer's full ranking, computed once and read-only."""

    def __init__(self, lib, name):
        self.lib, self.name = lib, name
        if name == "wide":
            self.W = make_model(6000, 36, 44, True, seed=31)
            self.R = make_history(96, 6000, 0.05, (11,), True, seed=37)
        elif name.startswith("crowd-"):     # tests/crowd_cases.py: few items, many users
            ties = name == "crowd-ties"
            self.W = make_model(400, 8, 12, ties, seed=41 if ties else 43)
            self.R = make_history(2500, 400, 0.08, NO_HISTORY, ties, seed=47 if ties else 53)
        else:
            ties = name == "ties"
            self.W = make_model(1500, 8, 12, ties, seed=17 if ties else 7)
            self.R = make_history(300, 1500, 0.03, NO_HISTORY, ties, seed=23 if ties else 5)
        self.binary = name not in ("floats", "crowd-floats")
        self.nusers, self.ncols = self.R.shape[0], self.W.shape[1]
        self.full = self.ncols
        self.hw = _scipy_to_model_handle(lib, self.W)
        self.hr = wrap(lib, self.R, self.binary)
        ids = np.full(self.nusers * self.full, -1, np.int32)
        sc = np.zeros(self.nusers * self.full, np.float32)
        os.environ["SLIM_PREDICT"] = "cpu"
        try:
            assert lib.Py_SLIM_Predict(self.full, self.hw, self.hr, ids, sc) == SLIM_OK
        finally:
            del os.environ["SLIM_PREDICT"]
        self.ids, self.sc = ids.reshape(-1, self.full), sc.reshape(-1, self.full)
        self.ids.setflags(write=False)
        self.sc.setflags(write=False)
        self.ncand = (self.ids >= 0).sum(1)
        self._mat = self._model = None

    def expected(self, n, allowed=None, X=None, users=None):
        """The yardstick: (ids, scores, counts) of length n for `users` (None: all) -- the full ranking without
        the ids outside the boolean mask `allowed` and without the ids of row <user id> of the scipy CSR X (a
        user beyond its rows has no exclusions); -1 / 0 beyond a list."""
        users = np.arange(self.nusers) if users is None else np.asarray(users)
        ids = np.full((users.size, n), -1, np.int32)
        sc = np.zeros((users.size, n), np.float32)
        cnt = np.zeros(users.size, np.int32)
        for q, u in enumerate(users):
            full = self.ids[u, :self.ncand[u]]
            keep = np.ones(full.size, bool) if allowed is None else allowed[full]
            if X is not None and u < X.shape[0]:
                keep &= ~np.isin(full, X.indices[X.indptr[u]:X.indptr[u + 1]])
            m = min(n, int(keep.sum()))
            ids[q, :m] = full[keep][:m]
            sc[q, :m] = self.sc[u, :self.ncand[u]][keep][:m]
            cnt[q] = m
        return ids, sc, cnt

    def exclusions(self, seed, xusers=None):
        """0-30 ids per user (a scipy CSR with xusers rows, ids as drawn: repeats stay, no order): the user's
        unfiltered top 3, items of the history, never-touched items, one id twice; every 7th row empty."""
        rng = np.random.default_rng(seed)
        xusers = self.nusers if xusers is None else xusers
        ptr, ind = [0], []
        for u in range(xusers):
            row = []
            if u % 7 != 3:
                hist = self.R.indices[self.R.indptr[u]:self.R.indptr[u + 1]]
                free = np.setdiff1d(np.arange(self.ncols), np.concatenate([self.ids[u, :self.ncand[u]], hist]))
                if u % 5 != 4:      # (every 5th row holds only ids that change nothing)
                    row = self.ids[u, :min(3, self.ncand[u])].tolist()
                    row += rng.choice(self.ncols, size=int(rng.integers(0, 24)), replace=False).tolist()
                if hist.size:
                    row.append(int(hist[rng.integers(hist.size)]))
                if free.size:
                    row.append(int(free[rng.integers(free.size)]))
                if row and u % 2:
                    row += [row[0], row[0]]
                row = [row[j] for j in rng.permutation(len(row))]
                assert len(row) <= 30
            ind += row
            ptr.append(len(ind))
        # (built by hand: scipy's constructor from triplets would merge the repeats and sort the rows)
        X = sp.csr_matrix((xusers, self.ncols), dtype=np.float32)
        X.indptr, X.indices = np.array(ptr, np.int64), np.array(ind, np.int32)
        X.data = np.ones(len(ind), np.float32)
        return X

    @property
    def mat(self):
        if self._mat is None:
            self._mat = DeviceMatrix.from_scipy(self.R, binary=self.binary)
            self._model = self._mat.model_from_scipy(self.W)
        return self._mat

    @property
    def model(self):
        assert self.mat is not None
        return self._model

    def close(self):
        if self._model is not None:
            self._model.free()
            self._mat.close()
        self.lib.SLIM_FreeModel(C.byref(self.hw))
        self.lib.Py_csr_free(self.hr)


def make_filter(lib, ncols, allowed=None, blocked=None, X=None):
    """SLIMGPU_FilterCreate from id arrays / a scipy CSR taken as it is (repeats and order kept): (status, handle)."""
    h = C.c_void_p()
    items = allowed if blocked is None else blocked
    spare = np.zeros(1, np.int32)
    buf = None if items is None else np.concatenate((np.asarray(items, np.int32), spare))
    xptr = None if X is None else np.ascontiguousarray(X.indptr, np.int64)
    xind = None if X is None else np.concatenate((np.asarray(X.indices, np.int32), spare))
    rc = lib.SLIMGPU_FilterCreate(ncols, 0 if items is None else buf.size - 1, None if buf is None else P(buf),
                                  0 if blocked is None else 1, 0 if X is None else X.shape[0],
                                  None if X is None else P(xptr), None if X is None else P(xind), C.byref(h))
    return rc, h


def cases_fixture():
    made = {}

    def get(name):
        if name not in made:
            made[name] = Case(_lib.load(), name)
        return made[name]
    yield get
    for c in made.values():
        c.close()


def same(got, want):
    return all(np.array_equal(g, w) for g, w in zip(got, want))


# ---- figures and ranks from yardstick lists (tests/test_filtered_eval.py, tests/test_later_positions.py) -------------
KEYS = ("hr", "hr_head", "hr_tail", "arhr")
NKEYS = ("nvalid", "nvalid_head", "nvalid_tail")


def figures(d):
    return np.array([d[k] for k in KEYS]), np.array([d[k] for k in NKEYS], np.int32)


def assert_same(got, want, what=""):
    (mg, ng), (mw, nw) = got, want
    print(what, "got ", mg.tolist(), ng.tolist())
    print(what, "want", mw.tolist(), nw.tolist())
    assert ng.tolist() == nw.tolist(), what
    assert mg.dtype == mw.dtype == np.float64 and np.array_equal(mg, mw), what


def evaluate_lists(lib, ids, n, T, fm):
    """The existing SLIMGPU_Evaluate on the first n ranks of yardstick lists (one row per row of T)."""
    n = min(n, ids.shape[1])
    lists = np.ascontiguousarray(ids[:, :n])
    cnt = (lists >= 0).sum(1).astype(np.int32)
    ht = wrap(lib, T)
    met, nv = np.zeros(4), np.zeros(3, np.int32)
    assert lib.SLIMGPU_Evaluate(T.shape[0], n, lists.ravel(), cnt, ht, fm, fm.size, met, nv) == SLIM_OK, \
        _lib.last_error()
    lib.Py_csr_free(ht)
    return met, nv


def positions(ids, sc, T, users):
    """(rank, score) of every test entry of `users` by looking it up in the rows of ids / sc (row q: users[q])."""
    rank, score = [], []
    for q, u in enumerate(users):
        where = {int(i): r for r, i in enumerate(ids[q]) if i >= 0}
        for z in range(T.indptr[u], T.indptr[u + 1]):
            r = where.get(int(T.indices[z]))
            rank.append(0 if r is None else r + 1)
            score.append(0.0 if r is None else sc[q, r])
    return np.array(rank, np.int32), np.array(score, np.float32)
