"""Evaluation of a resident model at several list lengths and on a subset of the users, from ONE scoring
pass (SLIMGPU_EvalSetCreateAt / SLIMGPU_ModelEvaluateAt, include/slim_gpu_eval.h).  The bar: every row is,
bit for bit, what the entry points that existed before give for that list length on exactly the selected
users' rows -- SLIMGPU_ModelEvaluate of a one-cutoff eval set for all users, SLIMGPU_ModelPredict +
SLIMGPU_Evaluate on the host handle of the selected rows for a subset -- and, on the two golden data
sets, the oracle's host loop."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
import scipy.sparse as sp

import slim_oracle as O
from conftest import ROOT
from slim_amd import _lib
from slim_amd.constants import SLIM_ERROR_INPUT, SLIM_NOPTIONS, SLIM_OK
from slim_amd.engine import DeviceMatrix

pytestmark = pytest.mark.gpu

KEYS = ("hr", "hr_head", "hr_tail", "arhr")
NKEYS = ("nvalid", "nvalid_head", "nvalid_tail")


# ---- helpers (as in test_resident_eval.py) ---------------------------------------------------------------
def ratings(nrows, ncols, density, seed, binary):
    rng = np.random.default_rng(seed)
    R = sp.random(nrows, ncols, density=density, format="csr", random_state=rng, dtype=np.float32)
    R.data[:] = 1.0 if binary else rng.integers(1, 6, R.nnz).astype(np.float32)
    R.sort_indices()
    return R


def leave_out(R, seed, per_user=1, min_keep=1):
    """(train, test): `per_user` entries of every user with enough of them move to the test matrix."""
    rng = np.random.default_rng(seed)
    R = sp.csr_matrix(R)
    keep = np.ones(R.nnz, bool)
    for u in range(R.shape[0]):
        s, e = R.indptr[u], R.indptr[u + 1]
        if e - s >= per_user + min_keep:
            keep[s + rng.choice(e - s, size=per_user, replace=False)] = False
    rows = np.repeat(np.arange(R.shape[0]), np.diff(R.indptr))
    trn = sp.csr_matrix((R.data[keep], (rows[keep], R.indices[keep])), shape=R.shape)
    tst = sp.csr_matrix((np.ones((~keep).sum(), np.float32), (rows[~keep], R.indices[~keep])), shape=R.shape)
    trn.sort_indices()
    tst.sort_indices()
    return trn, tst


def wrap(lib, M):
    M = sp.csr_matrix(M)
    h = C.c_void_p()
    val = np.ascontiguousarray(M.data, np.float32)
    assert lib.Py_csr_wrapper(M.shape[0], np.ascontiguousarray(M.indptr, np.intp),
                              np.ascontiguousarray(M.indices, np.int32),
                              val.ctypes.data_as(C.c_void_p), C.byref(h)) == SLIM_OK
    return h


def marker(R, T):
    ncols = max(R.shape[1], int(R.indices.max()) + 1, int(T.indices.max()) + 1 if T.nnz else 0)
    return O.head_tail(sp.csr_matrix(R), ncols)


def two_step(lib, model, R, T, n, fm):
    """The lists-through-the-host path: SLIMGPU_ModelPredict on the host handle of R's rows, then
    SLIMGPU_Evaluate.  Returns (metrics as doubles, counts)."""
    hr, ht = wrap(lib, R), wrap(lib, T)
    ids = np.full(R.shape[0] * n, -1, np.int32)
    sc = np.zeros(R.shape[0] * n, np.float32)
    assert lib.SLIMGPU_ModelPredict(n, model.handle, hr, ids.ctypes.data_as(C.c_void_p),
                                    sc.ctypes.data_as(C.c_void_p)) == SLIM_OK, _lib.last_error()
    cnt = (ids.reshape(-1, n) >= 0).sum(1).astype(np.int32)
    met, nv = np.zeros(4), np.zeros(3, np.int32)
    nu = min(R.shape[0], T.shape[0])
    assert lib.SLIMGPU_Evaluate(nu, n, ids, cnt, ht, fm, fm.size, met, nv) == SLIM_OK, _lib.last_error()
    for h in (hr, ht):
        lib.Py_csr_free(h)
    return met, nv


def figures(d):
    return np.array([d[k] for k in KEYS]), np.array([d[k] for k in NKEYS], np.int32)


def assert_same(got, want, what=""):
    (mg, ng), (mw, nw) = got, want
    print(what, "got ", mg.tolist(), ng.tolist())
    print(what, "want", mw.tolist(), nw.tolist())
    assert ng.tolist() == nw.tolist(), what
    assert mg.dtype == mw.dtype == np.float64 and np.array_equal(mg, mw), what


def single_cutoff(mat, model, T, c, fm):
    """All users, one list length: the entry point that existed before."""
    ev = mat.evaluator(T, nrcmds=c, fmarker=fm)
    got = ev.evaluate(model)
    ev.close()
    return figures(got)


def at(mat, model, T, cutoffs, fm, users=None):
    """(rows of evaluate_at as (metrics, counts), stats, figures of evaluate())"""
    ev = mat.evaluator(T, fmarker=fm, cutoffs=cutoffs, users=users)
    rows = ev.evaluate_at(model)
    st = ev.stats()
    last = ev.evaluate(model)
    ev.close()
    assert [r["nrcmds"] for r in rows] == list(cutoffs)
    return [figures(r) for r in rows], st, figures(last)


# ---- 1. cutoffs are prefixes: golden data, against the one-cutoff entry point and the oracle ---------------------
@pytest.mark.parametrize("data", ["ml100k", "automotive"])
def test_cutoffs_are_prefixes(data, ml100k, automotive):
    R, T = ml100k if data == "ml100k" else automotive[:2]
    R, T = sp.csr_matrix(R), sp.csr_matrix(T)
    cutoffs = (1, 3, 5, 10, 20, 64)
    mat = DeviceMatrix.from_scipy(R)
    model, _ = mat.learn_resident(l1r=1.0, l2r=1.0, niters=100, seed=1)
    W = model.fetch()
    ev = mat.evaluator(T, cutoffs=cutoffs)       # fmarker=None: head / tail over the training rows
    rows = ev.evaluate_at(model)
    st = ev.stats()
    last = ev.evaluate(model)
    ev.close()
    assert st["path"] == 1 and st["d2h_bytes"] <= 8 + 32 * len(cutoffs)
    hrs = []
    for c, row in zip(cutoffs, rows):
        assert row["nrcmds"] == c
        assert_same(figures(row), single_cutoff(mat, model, T, c, None), "%s @%d" % (data, c))
        want = O.evaluate(W, R, T, c)
        assert row["nvalid"] == want["nvalid"] > 0
        g = np.array([row["hr"], row["arhr"]], np.float32)
        r = np.array([want["hr"], want["arhr"]], np.float32)
        assert np.array_equal(g, r), (c, g, r)
        hrs.append(row["hr"])
    print(data, hrs)
    assert all(a < b for a, b in zip(hrs, hrs[1:])), hrs      # hits do fall between the cutoffs
    assert_same(figures(last), figures(rows[-1]), "evaluate() is the largest cutoff")
    model.free()
    mat.close()


# ---- 2. the synthetic cases, test rows of three items ---------------------------------------------------------------
CASES = {
    "binary": lambda: (ratings(40000, 2500, 0.01, 5, True), True),
    "ratings": lambda: (ratings(20000, 500, 0.02, 6, False), False),
}


class _Cases(object):
    """The matrices, staged and solved once per module, on first use; references computed once."""

    def __init__(self):
        self.made = {}
        self.refs = {}

    def get(self, name):
        if name not in self.made:
            R, binary = CASES[name]()
            trn, tst = leave_out(R, seed=3, per_user=3)
            assert np.diff(tst.indptr).max() == 3
            mat = DeviceMatrix.from_scipy(trn, binary=binary)
            model, _ = mat.learn_resident(l1r=2.0, l2r=1.0, optTol=1e-5, niters=50, seed=1)
            assert model.nnz > 0
            self.made[name] = (trn, tst, mat, model, marker(trn, tst))
        return self.made[name]

    def ref(self, name, c):
        """two_step over every user at list length c (default geometry)."""
        if (name, c) not in self.refs:
            trn, tst, mat, model, fm = self.get(name)
            self.refs[(name, c)] = two_step(mat._lib, model, trn, tst, c, fm)
        return self.refs[(name, c)]

    def close(self):
        for trn, tst, mat, model, fm in self.made.values():
            model.free()
            mat.close()
        self.made = {}


@pytest.fixture(scope="module")
def cases():
    c = _Cases()
    yield c
    c.close()


BOTH = pytest.mark.parametrize("name", ["binary", "ratings"])
PATH1 = (2, 10, 33, 64)
PATH2 = (10, 64, 100, 128)


@BOTH
@pytest.mark.parametrize("cutoffs", [PATH1, PATH2])
def test_every_cutoff_equals_its_own_evaluation(cases, name, cutoffs):
    trn, tst, mat, model, fm = cases.get(name)
    rows, st, last = at(mat, model, tst, cutoffs, fm)
    assert st["path"] == (1 if cutoffs[-1] <= 64 else 2)
    assert st["w_rows_read"] == trn.nnz
    for c, row in zip(cutoffs, rows):
        assert_same(row, single_cutoff(mat, model, tst, c, fm), "%s @%d one cutoff" % (name, c))
        assert_same(row, cases.ref(name, c), "%s @%d two-step" % (name, c))
        assert row[1][0] > 0 and row[0][0] > 0 and row[0][3] > 0      # (no comparison of zeros)
    assert rows[0][0][0] < rows[-1][0][0]
    assert_same(last, rows[-1])


@BOTH
@pytest.mark.parametrize("env", [("SLIM_TOPN_CW", "64"), ("SLIM_TOPN_KEY", "64")])
def test_every_cutoff_with_many_chunks_and_wide_keys(cases, name, env, monkeypatch):
    trn, tst, mat, model, fm = cases.get(name)
    want = [cases.ref(name, c) for c in PATH1]      # default geometry
    monkeypatch.setenv(*env)
    rows, st, _ = at(mat, model, tst, PATH1, fm)
    assert st["path"] == 1
    for c, row, w in zip(PATH1, rows, want):
        assert_same(row, w, "%s @%d %s" % (name, c, env[0]))


# ---- 3. lists shorter than a cutoff -------------------------------------------------------------------------------------
def test_lists_shorter_than_a_cutoff():
    """300 x 12: a user has at most 12 - history candidates, fewer than the cutoffs 8 and 16."""
    R = ratings(300, 12, 0.4, 11, False)
    trn, tst = leave_out(R, seed=4, per_user=2)
    mat = DeviceMatrix.from_scipy(trn)
    model, _ = mat.learn_resident(l1r=0.1, l2r=0.1, niters=100, seed=1)
    assert model.nnz > 0
    fm = marker(trn, tst)
    cutoffs = (4, 8, 16)
    rows, st, last = at(mat, model, tst, cutoffs, fm)
    ids, _ = model.predict(mat, 16)
    assert ((ids >= 0).sum(1) < 8).any()            # lists that end before the second cutoff
    for c, row in zip(cutoffs, rows):
        assert_same(row, single_cutoff(mat, model, tst, c, fm), "@%d" % c)
        assert_same(row, two_step(mat._lib, model, trn, tst, c, fm), "@%d two-step" % c)
        assert row[0][0] > 0
    assert_same(last, rows[-1])
    model.free()
    mat.close()


# ---- 4. subsets ------------------------------------------------------------------------------------------------------------
def check_subset(mat, model, trn, tst, fm, users, cutoffs):
    S = np.asarray(users)
    rows, st, last = at(mat, model, tst, cutoffs, fm, users=S)
    Rs, Ts = sp.csr_matrix(trn[S]), sp.csr_matrix(tst[S])
    assert st["w_rows_read"] == Rs.nnz
    for c, row in zip(cutoffs, rows):
        assert_same(row, two_step(mat._lib, model, Rs, Ts, c, fm), "%d users @%d" % (S.size, c))
    assert_same(last, rows[-1])
    return rows, st


@BOTH
def test_subsets(cases, name):
    trn, tst, mat, model, fm = cases.get(name)
    nu = trn.shape[0]
    cutoffs = (3, 10)
    stride, _ = check_subset(mat, model, trn, tst, fm, np.arange(0, nu, 7), cutoffs)
    assert stride[-1][1][0] > 0 and stride[-1][0][0] > 0
    for S in ([0], [nu - 1], [0, nu - 1]):
        check_subset(mat, model, trn, tst, fm, S, cutoffs)
    # lists over 64: the wave kernel and k_user_terms look the user of a position up too
    long, st = check_subset(mat, model, trn, tst, fm, np.arange(3, nu, 7), (10, 100))
    assert st["path"] == 2 and long[-1][0][0] > long[0][0][0] > 0
    # a list of every user is users=None
    everyone, st, _ = at(mat, model, tst, cutoffs, fm, users=np.arange(nu))
    nobody_listed, st0, _ = at(mat, model, tst, cutoffs, fm)
    assert st["w_rows_read"] == st0["w_rows_read"] == trn.nnz and st["w_bytes"] == st0["w_bytes"]
    for c, a, b in zip(cutoffs, everyone, nobody_listed):
        assert_same(a, b, "@%d every user listed" % c)
        assert_same(a, cases.ref(name, c), "@%d two-step" % c)


def test_random_sample(cases):
    trn, tst, mat, model, fm = cases.get("ratings")
    nu = trn.shape[0]
    S = np.sort(np.random.default_rng(41).choice(nu, size=nu // 100, replace=False))
    rows, st = check_subset(mat, model, trn, tst, fm, S, (5, 20))
    assert rows[0][1][0] > 0 and rows[1][0][0] > 0
    # the byte model counts the selected users only
    W = sp.csr_matrix(model.fetch())
    assert st["w_bytes"] == 8.0 * float(np.diff(W.indptr)[sp.csr_matrix(trn[S]).indices].sum())


def test_subset_with_empty_test_rows_and_an_empty_history():
    R = ratings(3000, 300, 0.03, 2, False)
    trn, tst = leave_out(R, seed=1, per_user=2)
    trn, tst = sp.lil_matrix(trn), sp.lil_matrix(tst)
    for u in (0, 9, 10, 2999):
        tst[u, :] = 0                      # no test items
    trn[12, :] = 0                         # no history, test items kept
    trn[9, :] = 0                          # neither
    trn, tst = sp.csr_matrix(trn), sp.csr_matrix(tst)
    trn.eliminate_zeros()
    tst.eliminate_zeros()
    assert tst[12].nnz > 0 and trn[12].nnz == 0 and tst[9].nnz == 0 and trn[9].nnz == 0
    mat = DeviceMatrix.from_scipy(trn)
    model, _ = mat.learn_resident(l1r=1.0, l2r=1.0, niters=50, seed=1)
    fm = marker(trn, tst)
    S = np.array([0, 3, 9, 10, 11, 12, 13, 64, 65, 1500, 2998, 2999])
    rows, _ = check_subset(mat, model, trn, tst, fm, S, (2, 10, 64))
    assert rows[-1][1][0] == S.size - 4     # the users without test items are not valid
    check_subset(mat, model, trn, tst, fm, np.arange(0, 3000, 3), (2, 10, 64))
    check_subset(mat, model, trn, tst, fm, [9], (10,))         # nobody valid: zeros, as the host path
    rows, st = check_subset(mat, model, trn, tst, fm, S, (10, 128))
    assert st["path"] == 2 and rows[-1][1][0] == S.size - 4 and rows[-1][0][0] > 0
    model.free()
    mat.close()


# ---- 4b. SLIMGPU_Evaluate keeps lists of any length ---------------------------------------------------------------------
def test_evaluate_of_host_lists_longer_than_255(ml100k):
    """SLIMGPU_Evaluate (lists from the host) sets no upper bound on nrcmds and goes through the launches of
    the resident evaluation with one cutoff: lists of 256 and 300 from the host scorer (Py_SLIM_Predict above
    128) against the oracle's host loop, as float32 like test_cutoffs_are_prefixes; the figures at 44 differ,
    so hits beyond rank 44 count."""
    R, T = sp.csr_matrix(ml100k[0]), sp.csr_matrix(ml100k[1])
    mat = DeviceMatrix.from_scipy(R)
    lib = mat._lib
    hmodel, _ = mat.learn(l1r=1.0, l2r=1.0, niters=100, seed=1, return_handle=True)
    hmodel = C.c_void_p(hmodel)
    from slim_amd.engine import model_to_scipy
    W = model_to_scipy(lib, hmodel, free=False)
    nu = R.shape[0]
    hr, ht = wrap(lib, R), wrap(lib, T)
    fm = marker(R, T)
    short = O.evaluate(W, R, T, 44)
    for n in (256, 300):
        ids = np.full(nu * n, -1, np.int32)
        sc = np.zeros(nu * n, np.float32)
        assert lib.Py_SLIM_Predict(n, hmodel, hr, ids, sc) == SLIM_OK, _lib.last_error()
        cnt = (ids.reshape(-1, n) >= 0).sum(1).astype(np.int32)
        assert cnt.max() == n
        met, nv = np.zeros(4), np.zeros(3, np.int32)
        assert lib.SLIMGPU_Evaluate(nu, n, ids, cnt, ht, fm, fm.size, met, nv) == SLIM_OK, _lib.last_error()
        want = O.evaluate(W, R, T, n)
        print(n, met.tolist(), nv.tolist(), want, short)
        assert nv[0] == want["nvalid"] > 0
        g = np.array([met[0], met[3]], np.float32)
        r = np.array([want["hr"], want["arhr"]], np.float32)
        assert np.array_equal(g, r), (n, g, r)
        assert want["hr"] > short["hr"] > 0 and want["arhr"] > short["arhr"]
    for h in (hr, ht):
        lib.Py_csr_free(h)
    lib.SLIM_FreeModel(C.byref(hmodel))
    mat.close()


# ---- 5. steady state ---------------------------------------------------------------------------------------------------------
def test_steady_state(cases):
    trn, tst, mat, model, fm = cases.get("ratings")
    other, _ = mat.learn_resident(l1r=1.0, l2r=5.0, optTol=1e-5, niters=50, seed=1)
    cutoffs = (5, 10, 20)
    S = np.arange(0, trn.shape[0], 10)
    for users in (None, S):
        ev = mat.evaluator(tst, fmarker=fm, cutoffs=cutoffs, users=users)
        seen = {}
        for k, m in enumerate((model, other, model, other)):
            rows = [figures(r) for r in ev.evaluate_at(m)]
            st = ev.stats()
            print(k, st)
            assert st["h2d_bytes"] == 0 and 0 < st["d2h_bytes"] <= 8 + 32 * len(cutoffs)
            if k >= 1:
                assert st["device_allocs"] == 0
            if id(m) in seen:               # alternating models: each gives its own figures again
                for a, b in zip(rows, seen[id(m)]):
                    assert_same(a, b)
            seen[id(m)] = rows
        assert not np.array_equal(seen[id(model)][1][0], seen[id(other)][1][0])
        ev.close()
    other.free()


# ---- 6. refusals -----------------------------------------------------------------------------------------------------------------
def test_refusals(cases):
    trn, tst, mat, model, fm = cases.get("ratings")
    lib = mat._lib
    nrows = trn.shape[0]
    ht = wrap(lib, tst)
    st = C.c_int32(0)

    def create(cutoffs, users, nusers=None):
        cut = np.asarray(cutoffs, np.int32)
        sel = None if users is None else np.asarray(users, np.int32)
        st.value = 0
        h = lib.SLIMGPU_EvalSetCreateAt(mat.handle, ht, fm, fm.size, cut.size, cut.ctypes.data_as(C.c_void_p),
                                        (0 if sel is None else sel.size) if nusers is None else nusers,
                                        None if sel is None else sel.ctypes.data_as(C.c_void_p), C.byref(st))
        return h, st.value, _lib.last_error()

    bad = [((10, 5), None), ((5, 5), None), ((0,), None), ((129,), None), (tuple(range(1, 10)), None),
           ((10,), (3, 2)), ((10,), (2, 2)), ((10,), (-1,)), ((10,), (nrows,))]
    for cutoffs, users in bad:
        h, status, msg = create(cutoffs, users)
        assert not h and status == SLIM_ERROR_INPUT and msg, (cutoffs, users, msg)
    h, status, msg = create((10,), None, nusers=4)             # users == NULL needs nusers == 0
    assert not h and status == SLIM_ERROR_INPUT and msg
    h, status, msg = create((5, 10), (2, 3))
    assert h and status == SLIM_OK, msg
    h = C.c_void_p(h)
    met, nv = np.zeros(32), np.zeros(24, np.int32)
    for n in (1, 3):
        assert lib.SLIMGPU_ModelEvaluateAt(h, model.handle, n, met, nv) == SLIM_ERROR_INPUT
        assert _lib.last_error()
    assert lib.SLIMGPU_ModelEvaluateAt(h, model.handle, 2, met, nv) == SLIM_OK
    lib.SLIMGPU_EvalSetFree(C.byref(h))
    lib.Py_csr_free(ht)


# ---- 7. the grid -------------------------------------------------------------------------------------------------------------------
PAIR = r"(l1r: \S+ l2r: \S+ nnz:\s+\d+ hr: \S+ hr_head: \S+ hr_tail: \S+ arhr: \S+)"


def _mselect(trn, tst, l1s, l2s, capfd, stride):
    from slim_amd import SLIM, SLIMatrix
    params = {"dbglvl": 0, "algo": "cd", "nthreads": 1, "optTol": 1e-7, "niters": 200}
    if stride is not None:
        params["gpu_evalstride"] = stride
    trainmat = SLIMatrix(trn)
    valmat = SLIMatrix(tst, trainmat)
    model = SLIM()
    C.CDLL(None).fflush(None)
    capfd.readouterr()
    try:
        model.mselect(params, trainmat, valmat, l1s, l2s, nrcmds=10)
        err = None
    except RuntimeError as e:
        err = str(e)
    C.CDLL(None).fflush(None)
    return model, capfd.readouterr().out, err


def test_grid_on_every_third_user(automotive, monkeypatch, capfd, tmp_path):
    R, T = sp.csr_matrix(automotive[0]), sp.csr_matrix(automotive[1])
    nu = R.shape[0]
    l1s, l2s = [1.0, 2.0], [1.0, 5.0]
    monkeypatch.setenv("SLIM_GPU_NO_CARRY", "1")       # a pair's model does not depend on who solved before
    monkeypatch.setenv("SLIM_GPU_RESIDENT", "1")
    monkeypatch.setenv("SLIM_GPU_EVAL_RESIDENT", "1")
    model, out, err = _mselect(R, T, l1s, l2s, capfd, 3)
    assert err is None, err
    S = np.arange(0, nu, 3)
    assert "  evaluating every 3-th user: %d of %d\n" % (S.size, nu) in out
    lines = re.findall(PAIR, out)
    assert len(lines) == 4
    # the same grid by hand: the same solves, the eval set of users 0, 3, 6, ...
    mat = DeviceMatrix.from_scipy(R)
    mat.expect_solves(4)
    ev = mat.evaluator(T, nrcmds=10, users=S)
    prev, got = None, []
    for l1 in l1s:
        for l2 in l2s:
            cur, _ = mat.learn_resident(warm=prev, l1r=l1, l2r=l2, optTol=1e-7, niters=200)
            if prev is not None:
                prev.free()
            prev = cur
            got.append((l1, l2, ev.evaluate(cur)))
    prev.free()
    ev.close()
    mat.close()
    best_hr = best_ar = (0.0, 0.0, 0.0, 0.0)
    for line, (l1, l2, g) in zip(lines, got):
        print(line, g)
        assert g["nvalid"] > 0 and g["hr"] > 0
        assert "hr: %.4f " % g["hr"] in line and line.endswith("arhr: %.4f" % g["arhr"])
        assert line.startswith("l1r: %.2e l2r: %.2e " % (l1, l2))
        if g["hr"] > best_hr[2]:
            best_hr = (l1, l2, g["hr"], g["arhr"])
        if g["arhr"] > best_ar[3]:
            best_ar = (l1, l2, g["hr"], g["arhr"])
    assert model.mselect_result == dict(bestHR=best_hr, bestAR=best_ar)
    # all users give other figures: the stride was not ignored
    _, out_all, err = _mselect(R, T, l1s, l2s, capfd, None)
    assert err is None and "evaluating every" not in out_all
    assert re.findall(PAIR, out_all) != lines

    # the command-line program prints the same pair lines
    from slim_amd.io import write_csr_text
    trn_f, tst_f, l12 = str(tmp_path / "trn.csr"), str(tmp_path / "tst.csr"), str(tmp_path / "l12")
    write_csr_text(trn_f, R)
    write_csr_text(tst_f, sp.csr_matrix((T.data, T.indices, T.indptr), shape=T.shape))
    open(l12, "w").write("".join("%g %g\n" % (a, b) for a in l1s for b in l2s))
    p = subprocess.run([os.path.join(ROOT, "slim_amd", "bin", "slim_mselect"), "-nomodels", "-niters=200",
                        "-evalstride=3", trn_f, tst_f, l12], capture_output=True, text=True,
                       cwd=str(tmp_path), timeout=280)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "  evaluating every 3-th user: %d of %d\n" % (S.size, nu) in p.stdout
    assert re.findall(PAIR, p.stdout) == lines

    # without the evaluation in HBM a stride is refused before the first solve
    monkeypatch.setenv("SLIM_GPU_EVAL_RESIDENT", "0")
    _, out, err = _mselect(R, T, l1s, l2s, capfd, 3)
    assert err is not None and "EVALSTRIDE" in err, err
    assert "l1r:" not in out
    from slim_amd import SLIMatrix
    from slim_amd.interface import build_options, check_params
    params = {"gpu_evalstride": 3}
    check_params(params)
    params["nrcmds"] = 10
    iopt, dopt = build_options(params)
    assert iopt[22] == 3 and iopt.size == SLIM_NOPTIONS
    trainmat = SLIMatrix(R)
    valmat = SLIMatrix(T, trainmat)
    best = [C.c_double(0.0) for _ in range(8)]
    rc = _lib.load().Py_SLIM_Mselect(trainmat.handle, valmat.handle, iopt, dopt, np.array(l1s), np.array(l2s),
                                     2, 2, *[C.byref(b) for b in best])
    assert rc == SLIM_ERROR_INPUT and _lib.last_error()
