"""Evaluation in HBM (SLIMGPU_EvalSetCreate / ModelEvaluate / MatrixPredict, include/slim_gpu_eval.h):
the
evaluate half of a model-selection cell (src/programs/slim_mselect.c:122-187, src/libslim/pyapi.c:309-366)
on a resident model against the resident training matrix.  The bar: the four figures and three counts
are those of the lists-through-the-host path (SLIMGPU_ModelPredict + SLIMGPU_Evaluate) and of the
oracle's host loop, bit for bit, and from the second pair on nothing but those figures crosses PCIe."""
import ctypes as C
import re

import numpy as np
import pytest
import scipy.sparse as sp

import slim_oracle as O
from slim_amd import _lib
from slim_amd.constants import SLIM_ERROR_INPUT, SLIM_NOPTIONS, SLIM_OK
from slim_amd.engine import DeviceMatrix, Evaluator, eval_stats

pytestmark = pytest.mark.gpu


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
    """The lists-through-the-host path: SLIMGPU_ModelPredict on the host handle of R's rows (the ones of
    a binary matrix carry the values 1.0 the staged matrix implies), then SLIMGPU_Evaluate.  Returns
    (metrics as doubles, counts, ids, scores)."""
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
    return met, nv, ids, sc


def fused(mat, model, T, n, fm):
    ev = mat.evaluator(T, nrcmds=n, fmarker=fm)
    got = ev.evaluate(model)
    st = ev.stats()
    ev.close()
    met = np.array([got["hr"], got["hr_head"], got["hr_tail"], got["arhr"]])
    nv = np.array([got["nvalid"], got["nvalid_head"], got["nvalid_tail"]], np.int32)
    return met, nv, st


def assert_same(a, b):
    (ma, na), (mb, nb) = a[:2], b[:2]
    print("fused    ", ma.tolist(), na.tolist())
    print("two-step ", mb.tolist(), nb.tolist())
    assert na.tolist() == nb.tolist()
    assert ma.dtype == mb.dtype == np.float64 and np.array_equal(ma, mb)
    assert na[0] > 0 and ma[0] > 0      # (a comparison of zeros would show nothing)


# ---- 1. oracle parity -----------------------------------------------------------------------------
def test_resident_evaluation_matches_oracle(ml100k, automotive):
    """The comparison test_gpu_evaluation_matches_oracle makes for the list path, on the same data:
    equal counts, the four figures equal as float32."""
    lib = _lib.load()
    for R, T in (ml100k, automotive[:2]):
        R, T = sp.csr_matrix(R), sp.csr_matrix(T)
        mat = DeviceMatrix.from_scipy(R)
        model, _ = mat.learn_resident(l1r=1.0, l2r=1.0, niters=100, seed=1)
        W = model.fetch()
        for n in (10, 3):
            ev = mat.evaluator(T, nrcmds=n)        # fmarker=None: head / tail over the training rows
            assert isinstance(ev, Evaluator)
            got = ev.evaluate(model)
            ev.close()
            want = O.evaluate(W, R, T, n)
            print(n, got, want)
            assert [got["nvalid"], got["nvalid_head"], got["nvalid_tail"]] == \
                [want["nvalid"], want["nvalid_head"], want["nvalid_tail"]]
            g = np.array([got[k] for k in ("hr", "hr_head", "hr_tail", "arhr")], np.float32)
            r = np.array([want[k] for k in ("hr", "hr_head", "hr_tail", "arhr")], np.float32)
            assert np.array_equal(g, r), (g, r)
            assert want["nvalid"] > 0 and want["hr"] > 0
        model.free()
        mat.close()


# ---- 2. fused path == two-step path, bit for bit ------------------------------------------------------
def _synth_big():
    """About 200 000 x 4 000 with at least 4e6 entries, binary (slim_amd.synth, on the host)."""
    from slim_amd import synth
    ptr, ind, val = synth.generate_csr(200_000, 4_000, 4_400_000, seed=7, device="cpu")
    R = sp.csr_matrix((val.numpy(), ind.numpy(), ptr.numpy()), shape=(200_000, 4_000))
    assert R.nnz >= 4_000_000
    return R


CASES = {
    "binary": lambda: (ratings(40000, 2500, 0.01, 5, True), True),
    "ratings": lambda: (ratings(20000, 500, 0.02, 6, False), False),
    "big": lambda: (_synth_big(), True),
}


class _Cases(object):
    """The three matrices, staged and solved once per module, on first use."""

    def __init__(self):
        self.made = {}

    def get(self, name):
        if name not in self.made:
            R, binary = CASES[name]()
            trn, tst = leave_out(R, seed=3)
            mat = DeviceMatrix.from_scipy(trn, binary=binary)
            model, _ = mat.learn_resident(l1r=2.0, l2r=1.0, optTol=1e-5, niters=50, seed=1)
            assert model.nnz > 0
            self.made[name] = (trn, tst, mat, model)
        return self.made[name]

    def close(self):
        for trn, tst, mat, model in self.made.values():
            model.free()
            mat.close()
        self.made = {}


@pytest.fixture(scope="module")
def cases():
    c = _Cases()
    yield c
    c.close()


ALL = pytest.mark.parametrize("name", ["binary", "ratings", "big"])
SMALL = pytest.mark.parametrize("name", ["binary", "ratings"])


@ALL
def test_fused_equals_two_step(cases, name):
    trn, tst, mat, model = cases.get(name)
    lib = mat._lib
    fm = marker(trn, tst)
    f = fused(mat, model, tst, 10, fm)
    assert f[2]["path"] == 1
    assert_same(f, two_step(lib, model, trn, tst, 10, fm))


@SMALL
@pytest.mark.parametrize("n", [64, 100])
def test_fused_equals_two_step_long_lists(cases, name, n):
    """Lists of a wavefront's width are the chunk kernel's last; longer ones take the wave kernel with
    its lists in HBM, k_user_terms after it (path 2), all on the device."""
    trn, tst, mat, model = cases.get(name)
    fm = marker(trn, tst)
    f = fused(mat, model, tst, n, fm)
    assert f[2]["path"] == (1 if n <= 64 else 2)
    assert_same(f, two_step(mat._lib, model, trn, tst, n, fm))


@SMALL
@pytest.mark.parametrize("env", [("SLIM_TOPN_CW", "64"), ("SLIM_TOPN_KEY", "64")])
def test_fused_equals_two_step_many_chunks_and_wide_keys(cases, name, env, monkeypatch):
    trn, tst, mat, model = cases.get(name)
    fm = marker(trn, tst)
    want = two_step(mat._lib, model, trn, tst, 10, fm)     # default geometry
    monkeypatch.setenv(*env)
    f = fused(mat, model, tst, 10, fm)
    assert f[2]["path"] == 1
    assert_same(f, want)
    assert_same(f, two_step(mat._lib, model, trn, tst, 10, fm))


@SMALL
def test_fused_equals_two_step_on_odd_test_matrices(cases, name):
    trn, tst, mat, model = cases.get(name)
    lib = mat._lib
    nu, nc = trn.shape
    rng = np.random.default_rng(17)
    rows = np.repeat(np.arange(nu), np.diff(tst.indptr))
    # empty rows: every third user loses its test item
    k = rows % 3 != 0
    T1 = sp.csr_matrix((tst.data[k], (rows[k], tst.indices[k])), shape=tst.shape)
    assert (np.diff(T1.indptr) == 0).sum() >= nu // 3
    # several items per user: three held-out ones and a few random ones (history items among them)
    _, T2 = leave_out(sp.csr_matrix(trn + tst), seed=23, per_user=3)
    extra = sp.random(nu, nc, density=4.0 / nc, format="csr", random_state=rng, dtype=np.float32)
    T2 = sp.csr_matrix(T2 + extra)
    T2.data[:] = 1.0
    T2.sort_indices()
    assert np.diff(T2.indptr).max() >= 4
    # an item id beyond the training matrix's columns
    far = np.arange(0, nu, 11)
    T3 = sp.csr_matrix(sp.hstack([tst, sp.csr_matrix((np.ones(far.size, np.float32),
                                                      (far, np.full(far.size, 5))), shape=(nu, 7))]))
    T3.sort_indices()
    assert T3.indices.max() == nc + 5
    # fewer rows than the training matrix
    T4 = sp.csr_matrix(tst[: nu - nu // 5])
    for T in (T1, T2, T3, T4):
        fm = marker(trn, T)
        assert_same(fused(mat, model, T, 10, fm), two_step(lib, model, trn, T, 10, fm))
    # ... and a marker that stops short of the test ids (they count as tail, eval.hip:51)
    fm = marker(trn, tst)
    assert_same(fused(mat, model, T3, 10, fm), two_step(lib, model, trn, T3, 10, fm))


# ---- 3. SLIMGPU_MatrixPredict ---------------------------------------------------------------------------
@SMALL
@pytest.mark.parametrize("n", [10, 100])
def test_matrix_predict_equals_model_predict(cases, name, n):
    trn, tst, mat, model = cases.get(name)
    _, _, ids, sc = two_step(mat._lib, model, trn, tst, n, marker(trn, tst))
    got_ids, got_sc = model.predict(mat, n)
    st = eval_stats()
    assert got_ids.shape == got_sc.shape == (trn.shape[0], n)
    assert np.array_equal(got_ids.ravel(), ids) and np.array_equal(got_sc.ravel(), sc)
    assert (got_ids >= 0).any()
    assert st["path"] == (1 if n <= 64 else 2) and st["h2d_bytes"] == 0


# ---- 4. nothing crosses PCIe per pair ------------------------------------------------------------------------
@ALL
def test_nothing_but_the_figures_crosses_pcie(cases, name):
    trn, tst, mat, model = cases.get(name)
    fm = marker(trn, tst)
    ev = mat.evaluator(tst, nrcmds=10, fmarker=fm)
    nu = min(trn.shape[0], tst.shape[0])
    chain = [(2.0, 1.0), (2.0, 5.0), (1.0, 5.0)]
    prev = None
    for k, (l1, l2) in enumerate(chain):
        cur, _ = mat.learn_resident(warm=prev, l1r=l1, l2r=l2, optTol=1e-5, niters=50, seed=1)
        if prev is not None:
            prev.free()
        prev = cur
        got = ev.evaluate(cur)
        st = ev.stats()
        print(k, got, st)
        assert st["path"] == 1 and st["h2d_bytes"] == 0 and st["d2h_bytes"] <= 64
        if k >= 1:
            assert st["device_allocs"] == 0
        assert st["w_rows_read"] == int(trn.indptr[nu])
        # the byte model: 8 bytes per entry of every model row a history entry selects
        W = sp.csr_matrix(cur.fetch())
        assert st["w_bytes"] == 8.0 * float(np.diff(W.indptr)[trn.indices[: trn.indptr[nu]]].sum())
        assert st["kernel_ms"] > 0 and st["total_ms"] >= st["kernel_ms"]
    prev.free()
    ev.close()


def _mselect(trn, tst, l1s, l2s, capfd, params=None):
    from slim_amd import SLIM, SLIMatrix
    params = params or {"dbglvl": 0, "algo": "cd", "nthreads": 1, "optTol": 1e-7, "niters": 200}
    trainmat = SLIMatrix(trn)
    valmat = SLIMatrix(tst, trainmat)
    model = SLIM()
    C.CDLL(None).fflush(None)
    capfd.readouterr()
    model.mselect(params, trainmat, valmat, l1s, l2s, nrcmds=10)
    C.CDLL(None).fflush(None)
    out = capfd.readouterr().out
    lines = [re.sub(r" time: \S+", "", l) for l in out.splitlines() if l.startswith("l1r:")]
    return model, lines


# ---- 5. the grid end to end -------------------------------------------------------------------------------------
def test_mselect_prints_the_same_lines_with_and_without_the_resident_evaluation(monkeypatch, capfd):
    """SLIM.mselect on the 40 000 x 2 500 leave-one-out case of test_resident_model.py, the evaluation in
    HBM and switched off (SLIM_GPU_EVAL_RESIDENT=0: lists through the host).  SLIM_GPU_NO_CARRY=1 makes the
    models of the two runs identical, so every printed line (but its wall time) must be the same string."""
    rng = np.random.default_rng(31)
    R = sp.random(40000, 2500, density=0.01, format="csr", random_state=rng, dtype=np.float32)
    R.data[:] = 1.0
    R.sort_indices()
    trn, tst = leave_out(R, seed=31, min_keep=1)
    monkeypatch.setenv("SLIM_GPU_NO_CARRY", "1")
    monkeypatch.setenv("SLIM_GPU_RESIDENT", "1")
    res = {}
    for mode in ("1", "0"):
        monkeypatch.setenv("SLIM_GPU_EVAL_RESIDENT", mode)
        lib = _lib.load()
        model, lines = _mselect(trn, tst, [1.0, 2.0], [1.0, 5.0, 10.0], capfd)
        res[mode] = (lines, model.mselect_result)
        if mode == "1":     # the last pair went through the fused kernel, and brought down its figures only
            st = eval_stats(lib)
            print(st)
            assert st["path"] == 1 and st["device_allocs"] == 0 and st["h2d_bytes"] == 0
            assert 0 < st["d2h_bytes"] <= 64 and st["w_rows_read"] == trn.nnz
            stamp = st["total_ms"]
        else:               # switched off: no evaluation in HBM happened since
            assert eval_stats(lib)["total_ms"] == stamp
    print("\n".join(res["1"][0]))
    assert len(res["1"][0]) == 6
    assert res["1"][0] == res["0"][0]
    assert res["1"][1] == res["0"][1]
    assert float(re.search(r"hr: (\S+)", res["1"][0][0]).group(1)) > 0


# ---- 6. errors and fallbacks ------------------------------------------------------------------------------------------
def test_errors():
    R = ratings(3000, 300, 0.03, 2, True)
    trn, tst = leave_out(R, seed=1)
    mat = DeviceMatrix.from_scipy(trn, binary=True)
    lib = mat._lib
    fm = marker(trn, tst)
    model, _ = mat.learn_resident(l1r=1.0, l2r=1.0)
    ev = mat.evaluator(tst, fmarker=fm)
    met, nv = np.zeros(4), np.zeros(3, np.int32)
    assert lib.SLIMGPU_ModelEvaluate(ev.handle, None, met, nv) == SLIM_ERROR_INPUT
    assert lib.SLIMGPU_ModelEvaluate(None, model.handle, met, nv) == SLIM_ERROR_INPUT
    assert lib.SLIMGPU_ModelEvaluate(ev.handle, model.handle, met, nv) == SLIM_OK and nv[0] > 0
    st = C.c_int32(0)
    ht = wrap(lib, tst)
    assert not lib.SLIMGPU_EvalSetCreate(None, ht, fm, fm.size, 10, C.byref(st)) and st.value == SLIM_ERROR_INPUT
    assert not lib.SLIMGPU_EvalSetCreate(mat.handle, None, fm, fm.size, 10, C.byref(st)) and st.value == SLIM_ERROR_INPUT
    assert not lib.SLIMGPU_EvalSetCreate(mat.handle, ht, fm, fm.size, 0, C.byref(st)) and st.value == SLIM_ERROR_INPUT
    assert not lib.SLIMGPU_EvalSetCreate(mat.handle, ht, fm, fm.size, 129, C.byref(st)) and st.value == SLIM_ERROR_INPUT
    lib.Py_csr_free(ht)
    lib.SLIMGPU_EvalSetFree(C.byref(C.c_void_p(None)))    # no-op
    # a model of another matrix width
    other = DeviceMatrix.from_scipy(ratings(3000, 200, 0.03, 3, True), binary=True)
    narrow, _ = other.learn_resident(l1r=1.0, l2r=1.0)
    assert lib.SLIMGPU_ModelEvaluate(ev.handle, narrow.handle, met, nv) == SLIM_ERROR_INPUT
    assert "items" in _lib.last_error()
    ids, sc = np.zeros(3000 * 10, np.int32), np.zeros(3000 * 10, np.float32)
    assert lib.SLIMGPU_MatrixPredict(10, narrow.handle, mat.handle, ids, sc) == SLIM_ERROR_INPUT
    assert lib.SLIMGPU_MatrixPredict(10, None, mat.handle, ids, sc) == SLIM_ERROR_INPUT
    assert lib.SLIMGPU_MatrixPredict(10, model.handle, None, ids, sc) == SLIM_ERROR_INPUT
    assert lib.SLIMGPU_LastEvalStats(None) == SLIM_ERROR_INPUT
    for x in (ev, narrow, other, model, mat):
        (x.close if hasattr(x, "close") else x.free)()


def test_a_matrix_with_merged_duplicates_keeps_the_host_path(monkeypatch, capfd):
    """SLIM_GPU_DUPLICATES=sum merges repeated (user, item) pairs at staging: the staged rows are not the
    caller's any more, so the evaluation in HBM is refused and Py_SLIM_Mselect scores through the host
    handle as before -- with the figures of SLIM_GPU_RESIDENT=0."""
    R = ratings(6000, 400, 0.03, 8, False)
    trn, tst = leave_out(R, seed=2)
    ptr, ind, val = trn.indptr.copy(), trn.indices.copy(), trn.data.copy()
    # user 0's first entry once more, at the end of its row
    e = int(ptr[1])
    ind = np.insert(ind, e, ind[0])
    val = np.insert(val, e, 2.0)
    ptr[1:] += 1
    monkeypatch.setenv("SLIM_GPU_DUPLICATES", "sum")
    lib = _lib.load()
    st = C.c_int32(0)
    iopt = np.full(SLIM_NOPTIONS, -1, np.int32)
    h = lib.SLIMGPU_MatrixFromHost(trn.shape[0], np.ascontiguousarray(ptr, np.intp), ind.astype(np.int32),
                                   val.astype(np.float32).ctypes.data_as(C.c_void_p),
                                   iopt.ctypes.data_as(C.c_void_p), C.byref(st))
    assert h, _lib.last_error()
    mat = DeviceMatrix(h)
    fm = marker(trn, tst)
    ht = wrap(lib, tst)
    assert not lib.SLIMGPU_EvalSetCreate(mat.handle, ht, fm, fm.size, 10, C.byref(st))
    assert st.value == SLIM_ERROR_INPUT and "DUPLICATES" in _lib.last_error()
    model, _ = mat.learn_resident(l1r=1.0, l2r=1.0)
    ids, sc = np.zeros(trn.shape[0] * 10, np.int32), np.zeros(trn.shape[0] * 10, np.float32)
    assert lib.SLIMGPU_MatrixPredict(10, model.handle, mat.handle, ids, sc) == SLIM_ERROR_INPUT
    lib.Py_csr_free(ht)
    model.free()
    mat.close()
    # a matrix staged under the same switch without a repeated pair is the caller's: accepted
    clean = DeviceMatrix.from_scipy(trn)
    clean.evaluator(tst, fmarker=fm).close()
    clean.close()
    # the grid on the matrix with the repeated pair completes, on the host path
    dup = sp.csr_matrix((val, ind, ptr), shape=trn.shape)      # (not canonical: the repeated pair stays)
    assert dup.nnz == trn.nnz + 1
    monkeypatch.setenv("SLIM_GPU_NO_CARRY", "1")
    res = {}
    for mode in ("1", "0"):
        monkeypatch.setenv("SLIM_GPU_RESIDENT", mode)
        model, lines = _mselect(dup, tst, [1.0], [1.0, 5.0], capfd)
        res[mode] = (lines, model.mselect_result)
    assert len(res["1"][0]) == 2 and res["1"] == res["0"]
