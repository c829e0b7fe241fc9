"""Top-N lists of up to 4 096 items on the device (include/slim_gpu_lists.h: SLIMGPU_PredictLists,
SLIMGPU_ModelPredictLists, SLIMGPU_MatrixPredictLists) and the layers above them (Py_SLIM_Predict, SLIM.predict,
slim_predict, slim_mselect).  The yardstick is the host scorer (Py_SLIM_Predict under SLIM_PREDICT=cpu): ids
and float scores are compared with np.array_equal, the slots beyond a list keep the caller's fill.  The scorer's
order is total, so the host list of length n is the first n entries of the one long host list every case
computes once.

The inputs are those of tests/test_ranked_eval.py (its generators are restated here):
  ties    1 500 x 1 500 model, 8-12 entries per row of {0.25, 0.5}; 300 binary users, two of them empty: nearly
          every cut at 129 .. 300 falls inside a group of equal scores up to ~250 wide
  floats  the same shape, values uniform(-0.2, 1.0), ratings 1-5: no ties, negative scores at the cut
  wide    6 000 x 6 000 model, 36-44 entries per row of {0.25, 0.5}; 96 binary users: more than 4 096 candidates
"""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
import scipy.sparse as sp

import slim_oracle as O
from conftest import GOLDEN, ROOT
from slim_amd import _lib
from slim_amd.constants import SLIM_ERROR_INPUT, SLIM_OK
from slim_amd.engine import DeviceMatrix, _scipy_to_model_handle, eval_stats, list_stats

pytestmark = pytest.mark.gpu

NO_HISTORY = (11, 150)
TWIDTH = 1600
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


def make_test_rows(R, ids, nitems, seed):
    """The test rows of the ranked suite: 0-6 items in no order, from the host lists (any position), an item of
    the history, a never-touched item, an id beyond the model, one id twice, empty rows."""
    rng = np.random.default_rng(seed)
    ptr, ind = [0], []
    for u in range(R.shape[0]):
        hist = R.indices[R.indptr[u]:R.indptr[u + 1]]
        lst = ids[u][ids[u] >= 0]
        row = []
        if u % 7 != 3:
            n = int(rng.integers(1, 5))
            if lst.size:
                row += [int(lst[0])] if u % 4 == 0 else []
                row += rng.choice(lst, size=min(n, lst.size), replace=False).tolist()
            else:
                row += rng.choice(nitems, size=n, replace=False).tolist()
            if u % 5 == 0 and hist.size:
                row.append(int(hist[rng.integers(hist.size)]))
            if u % 5 == 1:
                free = np.setdiff1d(np.arange(nitems), np.concatenate([lst, hist]))
                row.append(int(free[rng.integers(free.size)]))
            if u % 5 == 2:
                row.append(int(rng.integers(nitems, TWIDTH)))
            if u % 5 == 3:
                row.append(row[0])
            row = list(dict.fromkeys(row[:-1]))[:5] + [row[-1]]
            row = [row[j] for j in rng.permutation(len(row))]
        ind += row
        ptr.append(len(ind))
    return sp.csr_matrix((np.ones(len(ind), np.float32), np.array(ind, np.int32), np.array(ptr)),
                         shape=(R.shape[0], TWIDTH))


class _Case(object):
    """Model, histories, their host handles and the host scorer's lists of length `full`, computed once."""

    def __init__(self, lib, name):
        self.lib, self.name = lib, name
        if name == "wide":
            self.W = make_model(6000, 36, 44, True, seed=31)
            self.R = make_history(96, 6000, 0.05, (11,), True, seed=37)
            self.full = 4097
        else:
            ties = name == "ties"
            self.W = make_model(1500, 8, 12, ties, seed=17 if ties else 7)
            self.R = make_history(300, 1500, 0.03, NO_HISTORY, ties, seed=23 if ties else 5)
            self.full = 1500
        self.binary = name != "floats"
        self.nusers = self.R.shape[0]
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

    def host(self, n):
        """The host scorer's lists of length n, sentinels beyond them, and the list lengths."""
        assert n <= self.full
        return (np.ascontiguousarray(self.ids[:, :n]), np.ascontiguousarray(self.sc[:, :n]),
                np.minimum(self.ncand, n).astype(np.int32))

    def tied_across(self, n):
        """(users whose n-th and (n+1)-th scores are equal, the widest group of equal scores across that cut)."""
        assert n + 1 <= self.full
        users, widest = 0, 0
        for u in range(self.nusers):
            if self.ncand[u] > n and self.sc[u, n - 1] == self.sc[u, n]:
                users += 1
                widest = max(widest, int((self.sc[u, :self.ncand[u]] == self.sc[u, n]).sum()))
        return users, widest

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


@pytest.fixture(scope="module")
def cases():
    made = {}

    def get(name):
        if name not in made:
            made[name] = _Case(_lib.load(), name)
        return made[name]
    yield get
    for c in made.values():
        c.close()


def call(fn, n, nusers, *handles, env=None, users=None, nslots=None):
    """One of the three entry points into sentinel-filled arrays: (status, ids, scores, counts, error text)."""
    ids = np.full((nusers, n if nslots is None else nslots), -1, np.int32)
    sc = np.zeros(ids.shape, np.float32)
    cnt = np.full(nusers, -7, np.int32)
    os.environ.update(env or {})
    try:
        if users is None and fn.__name__ != "SLIMGPU_MatrixPredictLists":
            rc = fn(n, *handles, P(ids), P(sc), P(cnt))
        else:
            rc = fn(n, *handles, 0 if users is None else users.size, None if users is None else P(users),
                    P(ids), P(sc), P(cnt))
    finally:
        for k in (env or {}):
            del os.environ[k]
    return rc, ids, sc, cnt, _lib.last_error()


def same(got, want):
    return all(np.array_equal(g, w) for g, w in zip(got, want))


BOTH = pytest.mark.parametrize("name", ["floats", "ties"])
GEOMETRIES = [{}, {"SLIM_TOPN_CW": "64"}, {"SLIM_TOPN_KEY": "64"}, {"SLIM_TOPN_WAVES": "16"}]
geometry = pytest.mark.parametrize("env", GEOMETRIES, ids=lambda e: "-".join("%s=%s" % kv for kv in e.items()) or "default")


# ---- 0. the inputs are what they are meant to be ---------------------------------------------------------------------
def test_inputs(cases):
    t, f, w = cases("ties"), cases("floats"), cases("wide")
    for n in (129, 192, 256, 300):
        users, widest = t.tied_across(n)
        print("ties @%d: %d users tied across the cut, widest group %d" % (n, users, widest))
        assert users >= 270 and widest >= 200
    assert (t.ncand < 300).sum() > 0 and (t.ncand[list(NO_HISTORY)] == 0).all()
    negative = int(((f.ncand >= 300) & (f.sc[:, 299] < 0)).sum())
    print("floats @300: %d users with a negative score at the cut" % negative)
    assert negative >= 50
    print("wide: %d users above 4 096 candidates, median %d" % ((w.ncand > 4096).sum(), np.median(w.ncand)))
    assert (w.ncand > 4096).sum() >= 90
    assert w.tied_across(4096)[1] >= 1000


# ---- 1. lists against the host ---------------------------------------------------------------------------------------
@BOTH
@geometry
def test_lists_equal_the_hosts(cases, name, env):
    c = cases(name)
    for n in (129, 192, 256, 300, 512):
        rc, ids, sc, cnt, err = call(c.lib.SLIMGPU_PredictLists, n, c.nusers, c.hw, c.hr, env=env)
        assert rc == SLIM_OK, err
        st = list_stats(c.lib)
        print(name, n, env, st)
        assert st["path"] == 4 and st["slices"] == 1 and st["candidates"] == int(c.ncand.sum())
        assert same((ids, sc, cnt), c.host(n)), (name, n, env)
        assert (cnt[list(NO_HISTORY)] == 0).all() and (ids[list(NO_HISTORY)] == -1).all()
    assert (c.host(512)[2] == 512).sum() <= 1          # at 512 every list but one is short


# ---- 2. the refinement passes ----------------------------------------------------------------------------------------
def test_refinement_on_score_and_key(cases):
    c = cases("ties")
    rc, ids, sc, cnt, err = call(c.lib.SLIMGPU_PredictLists, 192, c.nusers, c.hw, c.hr)
    assert rc == SLIM_OK, err
    plain = list_stats(c.lib)
    print("default", plain)
    assert same((ids, sc, cnt), c.host(192))
    assert plain["lds_sorts"] >= 270 and plain["refine_passes"] == 0 and plain["key_refines"] == 0
    rc, ids, sc, cnt, err = call(c.lib.SLIMGPU_PredictLists, 192, c.nusers, c.hw, c.hr,
                                 env={"SLIM_TOPN_LONG_SORT": "64"})
    assert rc == SLIM_OK, err
    st = list_stats(c.lib)
    print("sort area of 64", st)
    assert same((ids, sc, cnt), c.host(192))
    assert st["path"] == 4 and st["refine_passes"] > 0 and st["key_refines"] >= 200
    assert st["contenders"] == plain["contenders"] > 0


# ---- 3. the cap ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("env", [{}, {"SLIM_TOPN_LONG_SORT": "256"}], ids=["default", "sort=256"])
def test_lists_of_4096(cases, env):
    c = cases("wide")
    rc, ids, sc, cnt, err = call(c.lib.SLIMGPU_PredictLists, 4096, c.nusers, c.hw, c.hr, env=env)
    assert rc == SLIM_OK, err
    st = list_stats(c.lib)
    print(env, st)
    assert st["path"] == 4
    if env:
        assert st["key_refines"] >= 90                  # groups of ~1 100 equal scores, a sort area of 256
    assert same((ids, sc, cnt), c.host(4096))
    assert cnt[11] == 0 and (cnt == 4096).sum() >= 90


def test_lists_of_4097_are_refused(cases):
    c = cases("ties")
    for fn, handles in ((c.lib.SLIMGPU_PredictLists, (c.hw, c.hr)),
                        (c.lib.SLIMGPU_ModelPredictLists, (c.model.handle, c.hr)),
                        (c.lib.SLIMGPU_MatrixPredictLists, (c.model.handle, c.mat.handle))):
        for n in (4097, 0, -3):
            rc, ids, sc, cnt, err = call(fn, n, 8, *handles, nslots=4097)
            assert rc == SLIM_ERROR_INPUT and fn.__name__ in err
            assert (ids == -1).all() and (sc == 0).all() and (cnt == -7).all()


# ---- 4. against the existing kernels ---------------------------------------------------------------------------------
@BOTH
def test_short_lists_on_the_long_path_equal_the_chunk_and_wave_kernels(cases, name):
    c = cases(name)
    for n in (1, 7, 64, 65, 128):
        rc, ids, sc, cnt, err = call(c.lib.SLIMGPU_PredictLists, n, c.nusers, c.hw, c.hr,
                                     env={"SLIM_TOPN_KERNEL": "long"})
        assert rc == SLIM_OK, err
        assert list_stats(c.lib)["path"] == 4
        old_ids = np.full((c.nusers, n), -1, np.int32)
        old_sc = np.zeros((c.nusers, n), np.float32)
        assert c.lib.SLIMGPU_Predict(n, c.hw, c.hr, old_ids.reshape(-1), old_sc.reshape(-1)) == SLIM_OK
        assert same((ids, sc), (old_ids, old_sc)), (name, n)
        assert same((ids, sc, cnt), c.host(n)), (name, n)
        # without the switch the new entry point is on the old paths
        rc, ids2, sc2, cnt2, err = call(c.lib.SLIMGPU_PredictLists, n, c.nusers, c.hw, c.hr)
        assert rc == SLIM_OK and list_stats(c.lib)["path"] == (1 if n <= 64 else 2)
        assert same((ids2, sc2, cnt2), (ids, sc, cnt))


# ---- 5. the three entry points agree ---------------------------------------------------------------------------------
@BOTH
def test_entry_points_agree(cases, name):
    c = cases(name)
    lib, n = c.lib, 256
    want = c.host(n)
    rc, *host_model, err = call(lib.SLIMGPU_PredictLists, n, c.nusers, c.hw, c.hr)
    assert rc == SLIM_OK and same(host_model, want), err
    rc, *resident, err = call(lib.SLIMGPU_ModelPredictLists, n, c.nusers, c.model.handle, c.hr)
    assert rc == SLIM_OK and same(resident, want), err
    rc, *matrix, err = call(lib.SLIMGPU_MatrixPredictLists, n, c.nusers, c.model.handle, c.mat.handle)
    assert rc == SLIM_OK and same(matrix, want), err
    first = eval_stats(lib)
    assert first["path"] == 4 and list_stats(lib)["slices"] == 1
    rc, *again, err = call(lib.SLIMGPU_MatrixPredictLists, n, c.nusers, c.model.handle, c.mat.handle)
    assert rc == SLIM_OK and same(again, want)
    # (SLIMGPU_MatrixPredict owns its workspaces per call: so does this one, call after call)
    assert eval_stats(lib)["device_allocs"] == first["device_allocs"] > 0
    users = np.arange(0, c.nusers, 3, dtype=np.int32)
    rc, *some, err = call(lib.SLIMGPU_MatrixPredictLists, n, users.size, c.model.handle, c.mat.handle, users=users)
    assert rc == SLIM_OK and same(some, [w[users] for w in want]), err
    rc, *sliced, err = call(lib.SLIMGPU_MatrixPredictLists, n, c.nusers, c.model.handle, c.mat.handle,
                            env={"SLIM_TOPN_LONG_SLICE": "37"})
    assert rc == SLIM_OK and same(sliced, want), err
    assert list_stats(lib)["slices"] == 9 and list_stats(lib)["candidates"] == int(c.ncand.sum())
    rc, *sliced, err = call(lib.SLIMGPU_MatrixPredictLists, n, users.size, c.model.handle, c.mat.handle, users=users,
                            env={"SLIM_TOPN_LONG_SLICE": "37"})
    assert rc == SLIM_OK and same(sliced, [w[users] for w in want]) and list_stats(lib)["slices"] == 3
    rc, *sliced, err = call(lib.SLIMGPU_PredictLists, n, c.nusers, c.hw, c.hr, env={"SLIM_TOPN_LONG_SLICE": "37"})
    assert rc == SLIM_OK and same(sliced, want) and list_stats(lib)["slices"] == 9
    # the Python layer
    ids, sc, cnt = c.model.predict(c.mat, n, return_counts=True)
    assert same((ids, sc, cnt), want)
    ids, sc = c.model.predict(c.mat, n, users=users)
    assert same((ids, sc), [w[users] for w in want[:2]])
    # malformed user lists: nothing is written
    for bad in ([5, 3], [4, 4], [0, c.nusers], [-1, 2]):
        bad = np.array(bad, np.int32)
        rc, ids, sc, cnt, err = call(lib.SLIMGPU_MatrixPredictLists, n, 2, c.model.handle, c.mat.handle, users=bad)
        assert rc == SLIM_ERROR_INPUT and "SLIMGPU_MatrixPredictLists" in err
        assert (ids == -1).all() and (sc == 0).all() and (cnt == -7).all()


# ---- 6. refusals -----------------------------------------------------------------------------------------------------
def test_a_model_with_shuffled_rows(cases, monkeypatch):
    c = cases("floats")
    lib, n = c.lib, 200
    W = c.W.copy()
    rng = np.random.default_rng(11)
    for r in (3, 57, 1499):
        s, e = W.indptr[r], W.indptr[r + 1]
        p = rng.permutation(e - s)
        while np.all(np.diff(W.indices[s:e][p]) > 0):
            p = rng.permutation(e - s)
        W.indices[s:e], W.data[s:e] = W.indices[s:e][p], W.data[s:e][p]
    hw = wrap(lib, W)                                   # (Py_csr_wrapper keeps a row's order as given)
    C.cast(hw, C.POINTER(_lib.CsrView)).contents.ncols = 1500
    try:
        rc, ids, sc, cnt, err = call(lib.SLIMGPU_PredictLists, n, c.nusers, hw, c.hr)
        assert rc == SLIM_ERROR_INPUT and "row order" in err
        assert (ids == -1).all() and (sc == 0).all() and (cnt == -7).all()
        # no ties at the cut (floats): the order inside a model row cannot show in the host's lists
        want_ids, want_sc, _ = c.host(n)
        for policy, status in ((None, SLIM_OK), ("gpu", SLIM_ERROR_INPUT)):
            if policy:
                monkeypatch.setenv("SLIM_PREDICT", policy)
            ids = np.full(c.nusers * n, -1, np.int32)
            sc = np.zeros(c.nusers * n, np.float32)
            assert lib.Py_SLIM_Predict(n, hw, c.hr, ids, sc) == status
            if status == SLIM_OK:
                assert np.array_equal(ids.reshape(-1, n), want_ids) and np.array_equal(sc.reshape(-1, n), want_sc)
            else:
                assert (ids == -1).all() and "row order" in _lib.last_error()
    finally:
        lib.Py_csr_free(hw)


# ---- 7. the public layers --------------------------------------------------------------------------------------------
@BOTH
def test_py_slim_predict_on_the_device(cases, name, monkeypatch):
    c = cases(name)
    n = 300
    monkeypatch.setenv("SLIM_PREDICT", "gpu")
    ids = np.full(c.nusers * n, -1, np.int32)
    sc = np.zeros(c.nusers * n, np.float32)
    assert c.lib.Py_SLIM_Predict(n, c.hw, c.hr, ids, sc) == SLIM_OK, _lib.last_error()
    assert list_stats(c.lib)["path"] == 4
    want_ids, want_sc, _ = c.host(n)
    assert np.array_equal(ids.reshape(-1, n), want_ids) and np.array_equal(sc.reshape(-1, n), want_sc)


def test_slim_predict_of_300_on_automotive(automotive_triplets, monkeypatch):
    from slim_amd import SLIM, SLIMatrix
    trn, _ = automotive_triplets
    trainmat = SLIMatrix(trn)
    model = SLIM()
    model.train({"algo": "cd", "nthreads": 1, "l1r": 1.0, "l2r": 1.0, "niters": 20, "dbglvl": 0}, trainmat)
    got = {}
    for policy in ("cpu", "gpu"):
        monkeypatch.setenv("SLIM_PREDICT", policy)
        got[policy] = model.predict(trainmat, nrcmds=300, returnscores=True)
        if policy == "gpu":
            assert list_stats()["path"] == 4
    (out_c, sc_c), (out_g, sc_g) = got["cpu"], got["gpu"]
    assert out_c.keys() == out_g.keys() and len(out_c) > 1000
    for u in out_c:
        assert np.array_equal(out_c[u], out_g[u]) and np.array_equal(sc_c[u], sc_g[u])


def _cli(prog, *args, env, cwd):
    e = dict(os.environ)
    e.update(env)
    p = subprocess.run([os.path.join(ROOT, "slim_amd", "bin", prog)] + list(args), capture_output=True, text=True,
                       env=e, cwd=cwd, timeout=280)
    assert p.returncode == 0, p.stdout + p.stderr
    return p.stdout


def test_command_line_programs(tmp_path, ml100k):
    from slim_amd.io import write_csr_text
    trn, tst = os.path.join(GOLDEN, "ml100k-train.csr"), os.path.join(GOLDEN, "ml100k-test.csr")
    mdl = str(tmp_path / "m.model")
    write_csr_text(mdl, make_model(ml100k[0].shape[1], 30, 40, False, seed=3))
    files = {}
    for policy in ("cpu", "gpu"):
        out = str(tmp_path / ("recs_%s.txt" % policy))
        stdout = _cli("slim_predict", "-nrcmds=300", "-outfile=" + out, mdl, trn, tst, env={"SLIM_PREDICT": policy},
                      cwd=str(tmp_path))
        files[policy] = (open(out).read(), re.findall(r"hr: \S+ hr_head: \S+ hr_tail: \S+ arhr: \S+", stdout))
    assert files["cpu"] == files["gpu"] and files["cpu"][1]
    assert max(len(line.split()) for line in files["cpu"][0].splitlines()) == 600     # full lists of 300
    # the grid's host-model branch: lists of 200 from the device, the figures those of the host loop
    l12 = str(tmp_path / "l12")
    open(l12, "w").write("1 1\n5 1\n")
    pair = r"(l1r: \S+ l2r: \S+ nnz:\s+\d+ hr: \S+ hr_head: \S+ hr_tail: \S+ arhr: \S+)"
    lines = {}
    for policy in ("cpu", "auto"):
        stdout = _cli("slim_mselect", "-nomodels", "-niters=100", "-nrcmds=200", trn, tst, l12,
                      env={"SLIM_PREDICT": policy, "SLIM_GPU_RESIDENT": "0", "SLIM_GPU_NO_CARRY": "1"},
                      cwd=str(tmp_path))
        lines[policy] = re.findall(pair, stdout)
    assert len(lines["cpu"]) == 2 and lines["cpu"] == lines["auto"]


def test_python_grid_on_host_models(ml100k, monkeypatch, capfd):
    """Py_SLIM_Mselect with SLIM_GPU_RESIDENT=0: lists of 200 from the device, the host loop's lines."""
    from slim_amd import SLIM, SLIMatrix
    R, T = sp.csr_matrix(ml100k[0]), sp.csr_matrix(ml100k[1])
    T = sp.csr_matrix((T.data, T.indices, T.indptr), shape=R.shape)
    monkeypatch.setenv("SLIM_GPU_RESIDENT", "0")
    monkeypatch.setenv("SLIM_GPU_NO_CARRY", "1")
    pair = r"(l1r: \S+ l2r: \S+ nnz:\s+\d+ hr: \S+ hr_head: \S+ hr_tail: \S+ arhr: \S+)"
    lines = {}
    for policy in ("cpu", "auto"):
        monkeypatch.setenv("SLIM_PREDICT", policy)
        trainmat = SLIMatrix(R)
        valmat = SLIMatrix(T, trainmat)
        C.CDLL(None).fflush(None)
        capfd.readouterr()
        SLIM().mselect({"dbglvl": 0, "algo": "cd", "nthreads": 1, "optTol": 1e-7, "niters": 100}, trainmat, valmat,
                       [1.0], [1.0, 5.0], nrcmds=200)
        C.CDLL(None).fflush(None)
        lines[policy] = re.findall(pair, capfd.readouterr().out)
        if policy == "auto":
            assert list_stats()["path"] == 4
    assert len(lines["cpu"]) == 2 and lines["cpu"] == lines["auto"]


# ---- 8. ranks and lists are one order --------------------------------------------------------------------------------
def test_ranks_and_lists_are_one_order(cases):
    c = cases("ties")
    n = 512
    T = make_test_rows(c.R, c.ids, 1500, seed=3)
    fm = O.head_tail(sp.csr_matrix(c.R), TWIDTH)
    ev = c.mat.evaluator(T, fmarker=fm, ranked=True)
    rank, indptr, rscore = ev.ranks(c.model, scores=True)
    ev.close()
    rc, ids, sc, cnt, err = call(c.lib.SLIMGPU_MatrixPredictLists, n, c.nusers, c.model.handle, c.mat.handle)
    assert rc == SLIM_OK, err
    checked = 0
    for u in range(c.nusers):
        where = {int(i): r for r, i in enumerate(ids[u, :cnt[u]])}
        for z in range(indptr[u], indptr[u + 1]):
            r = where.get(int(T.indices[z]))
            if r is None:
                assert rank[z] == 0 or rank[z] > n
            else:
                assert rank[z] == r + 1 and rscore[z:z + 1].view(np.uint32) == sc[u, r:r + 1].view(np.uint32)
                checked += 1
    assert checked > c.nusers
