"""The rank of every held-out item among a user's candidates (include/slim_gpu_rank.h: SLIMGPU_ModelRanks,
SLIMGPU_ModelEvaluateRanked, SLIMGPU_ModelFromHost) and the evaluation of resident models at any list length.
The yardstick is the host scorer with the full list (Py_SLIM_Predict, SLIM_PREDICT=cpu, n = ncols): a test item
has rank r + 1 iff it stands at position r of that list, with that list's score bit for bit; an item that is in
no list has rank 0."""
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
from slim_amd.constants import SLIM_OK
from slim_amd.engine import DeviceMatrix, _scipy_to_model_handle

pytestmark = pytest.mark.gpu

KEYS = ("hr", "hr_head", "hr_tail", "arhr")
NKEYS = ("nvalid", "nvalid_head", "nvalid_tail")
NITEMS, NUSERS, TWIDTH = 1500, 300, 1600
NO_HISTORY = (11, 150)


def wrap(lib, M):
    M = sp.csr_matrix(M)
    h = C.c_void_p()
    val = np.ascontiguousarray(M.data, np.float32)
    assert lib.Py_csr_wrapper(M.shape[0], np.ascontiguousarray(M.indptr, np.intp),
                              np.ascontiguousarray(M.indices, np.int32),
                              val.ctypes.data_as(C.c_void_p), C.byref(h)) == SLIM_OK
    return h


def host_lists(lib, W, R, n, monkeypatch):
    """The host scorer's lists of length n for every row of R: (ids [nusers, n] with -1 beyond a list, scores)."""
    monkeypatch.setenv("SLIM_PREDICT", "cpu")
    hw, hr = _scipy_to_model_handle(lib, W), wrap(lib, R)
    ids = np.full(R.shape[0] * n, -1, np.int32)
    sc = np.zeros(R.shape[0] * n, np.float32)
    assert lib.Py_SLIM_Predict(n, hw, hr, ids, sc) == SLIM_OK
    lib.SLIM_FreeModel(C.byref(hw))
    lib.Py_csr_free(hr)
    monkeypatch.delenv("SLIM_PREDICT")
    return ids.reshape(-1, n), sc.reshape(-1, n)


def figures(d):
    return np.array([d[k] for k in KEYS]), np.array([d[k] for k in NKEYS], np.int32)


def assert_same(got, want, what=""):
    (mg, ng), (mw, nw) = got, want
    print(what, "got ", mg.tolist(), ng.tolist())
    print(what, "want", mw.tolist(), nw.tolist())
    assert ng.tolist() == nw.tolist(), what
    assert mg.dtype == mw.dtype == np.float64 and np.array_equal(mg, mw), what


def evaluate_lists(lib, ids, c, T, fm):
    """SLIMGPU_Evaluate on the first c ranks of the host lists."""
    c = min(c, ids.shape[1])
    lists = np.ascontiguousarray(ids[:, :c])
    cnt = (lists >= 0).sum(1).astype(np.int32)
    ht = wrap(lib, T)
    met, nv = np.zeros(4), np.zeros(3, np.int32)
    assert lib.SLIMGPU_Evaluate(min(ids.shape[0], T.shape[0]), c, lists.ravel(), cnt, ht, fm, fm.size, met,
                                nv) == SLIM_OK, _lib.last_error()
    lib.Py_csr_free(ht)
    return met, nv


# ---- the hand-made case: a 1 500 x 1 500 model, 300 users ------------------------------------------------------------
def make_model(ties, seed):
    rng = np.random.default_rng(seed)
    ptr, ind, val = [0], [], []
    for _ in range(NITEMS):
        k = int(rng.integers(8, 13))
        ind.append(np.sort(rng.choice(NITEMS, size=k, replace=False)))
        val.append(rng.choice([0.25, 0.5], size=k) if ties else rng.uniform(-0.2, 1.0, size=k))
        ptr.append(ptr[-1] + k)
    return sp.csr_matrix((np.concatenate(val).astype(np.float32), np.concatenate(ind).astype(np.int32), ptr),
                         shape=(NITEMS, NITEMS))


def make_history(binary, seed):
    rng = np.random.default_rng(seed)
    R = sp.random(NUSERS, NITEMS, density=0.03, format="lil", random_state=rng, dtype=np.float32)
    for u in NO_HISTORY:
        R.rows[u], R.data[u] = [], []
    R = sp.csr_matrix(R)
    R.data[:] = 1.0 if binary else rng.integers(1, 6, R.nnz).astype(np.float32)
    R.sort_indices()
    return R


def make_test_rows(R, ids, seed):
    """Test rows of 0-6 items in no particular order, built from the host lists: items of the list (any position),
    and by construction an item of the history, a never-touched item, an id beyond the model, one id listed twice,
    empty rows."""
    rng = np.random.default_rng(seed)
    ptr, ind = [0], []
    kinds = {"history": 0, "untouched": 0, "wide": 0, "twice": 0, "empty": 0, "five": 0}
    for u in range(NUSERS):
        hist = R.indices[R.indptr[u]:R.indptr[u + 1]]
        lst = ids[u][ids[u] >= 0]
        row = []
        if u % 7 == 3:
            kinds["empty"] += 1
        else:
            n = int(rng.integers(1, 5))
            if lst.size:
                row += [int(lst[0])] if u % 4 == 0 else []          # the head of the list
                row += rng.choice(lst, size=min(n, lst.size), replace=False).tolist()
            else:
                row += rng.choice(NITEMS, size=n, replace=False).tolist()
            if u % 5 == 0 and hist.size:
                row.append(int(hist[rng.integers(hist.size)]))
                kinds["history"] += 1
            if u % 5 == 1:
                free = np.setdiff1d(np.arange(NITEMS), np.concatenate([lst, hist]))
                row.append(int(free[rng.integers(free.size)]))
                kinds["untouched"] += 1
            if u % 5 == 2:
                row.append(int(rng.integers(NITEMS, TWIDTH)))
                kinds["wide"] += 1
            if u % 5 == 3:
                row.append(row[0])
                kinds["twice"] += 1
            row = list(dict.fromkeys(row[:-1]))[:5] + [row[-1]]    # distinct but for the one listed twice
            row = [row[j] for j in rng.permutation(len(row))]
            kinds["five"] += len(row) == 5
        assert len(row) <= 6
        ind += row
        ptr.append(len(ind))
    assert all(v > 0 for v in kinds.values()), kinds
    # (kept as built: rows in no order, one id twice)
    T = sp.csr_matrix((np.ones(len(ind), np.float32), np.array(ind, np.int32), np.array(ptr)), shape=(NUSERS, TWIDTH))
    return T


class _Case(object):
    def __init__(self, lib, name, monkeypatch):
        ties = name == "ties"
        self.W = make_model(ties, seed=17 if ties else 7)
        self.R = make_history(binary=ties, seed=23 if ties else 5)
        self.ids, self.sc = host_lists(lib, self.W, self.R, NITEMS, monkeypatch)
        self.T = make_test_rows(self.R, self.ids, seed=3)
        assert np.diff(self.T.indptr).max() >= 5 and self.T.indices.max() >= NITEMS
        # the reference ranks and scores, once
        self.rank = np.zeros(self.T.nnz, np.int32)
        self.score = np.zeros(self.T.nnz, np.float32)
        tied = 0
        for u in range(NUSERS):
            where = {int(i): r for r, i in enumerate(self.ids[u]) if i >= 0}
            for z in range(self.T.indptr[u], self.T.indptr[u + 1]):
                r = where.get(int(self.T.indices[z]))
                if r is not None:
                    self.rank[z], self.score[z] = r + 1, self.sc[u, r]
                    tied += (r > 0 and self.sc[u, r - 1] == self.sc[u, r]) or \
                            (r + 1 < len(where) and self.sc[u, r + 1] == self.sc[u, r])
        self.tied = tied
        assert (self.rank > 0).sum() > NUSERS and (self.rank == 0).sum() > NUSERS // 5
        assert self.rank.max() > 128                         # ranks beyond every list the device scorers form
        self.mat = DeviceMatrix.from_scipy(self.R, binary=ties)
        self.model = self.mat.model_from_scipy(self.W)
        self.fm = O.head_tail(sp.csr_matrix(self.R), TWIDTH)

    def close(self):
        self.model.free()
        self.mat.close()


@pytest.fixture(scope="module")
def cases():
    made = {}
    mp = pytest.MonkeyPatch()

    def get(name):
        if name not in made:
            made[name] = _Case(_lib.load(), name, mp)
        return made[name]
    yield get
    mp.undo()
    for c in made.values():
        c.close()


BOTH = pytest.mark.parametrize("name", ["floats", "ties"])
GEOMETRIES = [{}, {"SLIM_TOPN_CW": "64"}, {"SLIM_TOPN_KEY": "64"}, {"SLIM_TOPN_WAVES": "16"},
              {"SLIM_TOPN_RANK_GROUP": "2"}]


# ---- 1. ranks against the full lists -------------------------------------------------------------------------------
@BOTH
@pytest.mark.parametrize("env", GEOMETRIES, ids=lambda e: "-".join("%s=%s" % kv for kv in e.items()) or "default")
def test_ranks_are_the_positions_in_the_full_host_list(cases, name, env, monkeypatch):
    c = cases(name)
    if name == "ties":
        print("ranked test items tied with a neighbour in the host list:", c.tied)
        assert c.tied > 20
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    ev = c.mat.evaluator(c.T, fmarker=c.fm, ranked=True)
    ranks, indptr, scores = ev.ranks(c.model, scores=True)
    st = ev.stats()
    ev.close()
    assert indptr.tolist() == c.T.indptr.tolist() and ranks.size == c.T.nnz
    bad = np.flatnonzero(ranks != c.rank)
    print(name, env, "entries", ranks.size, "ranked", int((c.rank > 0).sum()), "max rank", int(c.rank.max()),
          "mismatches", bad.size, st)
    assert bad.size == 0, (bad[:10], ranks[bad[:10]], c.rank[bad[:10]])
    assert scores.dtype == np.float32 and np.array_equal(scores.view(np.uint32), c.score.view(np.uint32))
    assert st["path"] == 3 and st["d2h_bytes"] == 8 * c.T.nnz


@BOTH
def test_a_user_subset_gives_the_same_ranks(cases, name):
    c = cases(name)
    S = np.arange(0, NUSERS, 3)
    ev = c.mat.evaluator(c.T, fmarker=c.fm, ranked=True, users=S)
    ranks, indptr = ev.ranks(c.model)
    ev.close()
    want = np.concatenate([c.rank[c.T.indptr[u]:c.T.indptr[u + 1]] for u in S])
    assert indptr[-1] == want.size and np.array_equal(ranks, want)
    assert np.array_equal(np.diff(indptr), np.diff(c.T.indptr)[S])


# ---- 2. figures ---------------------------------------------------------------------------------------------------
@BOTH
def test_figures_up_to_128_are_those_of_evaluate_at(cases, name):
    c = cases(name)
    cutoffs = (1, 5, 10, 64, 65, 128)
    ev = c.mat.evaluator(c.T, fmarker=c.fm, cutoffs=cutoffs)
    want = ev.evaluate_at(c.model)
    got = ev.evaluate_ranked(c.model, cutoffs)           # an eval set of any creator serves
    ev.close()
    for k, cut in enumerate(cutoffs):
        assert got[k]["nrcmds"] == cut
        assert_same(figures(got[k]), figures(want[k]), "%s @%d" % (name, cut))
    assert got[0]["hr"] > 0 and got[0]["hr"] < got[-1]["hr"]


@BOTH
def test_figures_at_any_length_are_those_of_the_host_lists(cases, name):
    c = cases(name)
    cutoffs = (129, 300, 1500, 10 ** 6)
    ev = c.mat.evaluator(c.T, fmarker=c.fm, ranked=True)
    got = ev.evaluate_ranked(c.model, cutoffs)
    ev.close()
    for k, cut in enumerate(cutoffs):
        assert_same(figures(got[k]), evaluate_lists(c.mat._lib, c.ids, cut, c.T, c.fm), "%s @%d" % (name, cut))
    assert got[0]["hr"] < got[2]["hr"]                      # hits do fall beyond rank 129
    assert_same(figures(got[2]), figures(got[3]))            # 1 500 candidates at the most


@pytest.fixture(scope="module")
def learned(ml100k):
    R, T = sp.csr_matrix(ml100k[0]), sp.csr_matrix(ml100k[1])
    mat = DeviceMatrix.from_scipy(R)
    model, _ = mat.learn_resident(l1r=1.0, l2r=1.0, niters=100, seed=1)
    yield R, T, mat, model
    model.free()
    mat.close()


def test_ml100k_with_a_learned_model_against_the_oracle(learned):
    R, T, mat, model = learned
    W = model.fetch()
    ev = mat.evaluator(T, ranked=True)
    rows = ev.evaluate_ranked(model, (10, 300))
    ev.close()
    for row in rows:
        want = O.evaluate(W, R, T, row["nrcmds"])
        assert row["nvalid"] == want["nvalid"] > 0
        g = np.array([row["hr"], row["arhr"]], np.float32)
        r = np.array([want["hr"], want["arhr"]], np.float32)
        print(row["nrcmds"], g, r)
        assert np.array_equal(g, r), (row["nrcmds"], g, r)
    assert rows[0]["hr"] < rows[1]["hr"]


# ---- 3. resources and refusals -------------------------------------------------------------------------------------
def test_steady_state_slices_and_refusals(cases):
    c = cases("floats")
    nine = (1, 2, 3, 5, 8, 13, 100, 200, 1000)               # more than one slice of 8
    ev = c.mat.evaluator(c.T, fmarker=c.fm, ranked=True)
    first = ev.evaluate_ranked(c.model, nine)
    second = ev.evaluate_ranked(c.model, nine)
    st = ev.stats()
    print(st, "pre-pass %.3f ms" % ev.prepass_ms())
    assert st["device_allocs"] == 0 and st["h2d_bytes"] == 0 and st["d2h_bytes"] == 8 + 32 * 9 and st["path"] == 3
    assert st["w_bytes"] > 0 and 0 < ev.prepass_ms() <= st["kernel_ms"]
    for a, b in zip(first, second):
        assert_same(figures(a), figures(b))
    for k, cut in enumerate(nine):                            # every slice's rows are that cutoff's own figures
        assert_same(figures(second[k]), evaluate_lists(c.mat._lib, c.ids, cut, c.T, c.fm), "@%d" % cut)
    one = ev.evaluate_ranked(c.model, (200,))
    assert ev.stats()["d2h_bytes"] == 40
    assert_same(figures(one[0]), figures(second[7]))
    for bad in (tuple(range(1, 34)), (10, 5), (5, 5), (0, 3), ()):
        with pytest.raises(RuntimeError, match="SLIMGPU_ModelEvaluateRanked"):
            ev.evaluate_ranked(c.model, bad)
    with pytest.raises(RuntimeError, match="SLIMGPU_ModelEvaluate"):     # no list length: nothing for the lists' entry point
        ev.evaluate(c.model)
    ev.close()
    # a model with a shuffled row is refused
    W = c.W.copy()
    s = W.indptr[40]
    W.indices[s], W.indices[s + 1] = W.indices[s + 1], W.indices[s]
    with pytest.raises(RuntimeError, match="ascend"):
        c.mat.model_from_scipy(W)


def test_ranks_are_refused_where_the_chunk_scorer_cannot_serve(cases, monkeypatch):
    """Only the chunk kernel has a rank form: with the wave kernel pinned both ranked calls are refused and say
    why; without the pin the same eval set gives the reference ranks again.  (The pin is the only way to this
    refusal: a resident model with rows that do not ascend is refused when it is made.)"""
    c = cases("floats")
    ev = c.mat.evaluator(c.T, fmarker=c.fm, ranked=True)
    monkeypatch.setenv("SLIM_TOPN_KERNEL", "wave")
    why = r": ranks of the held-out items need the chunk scorer: .*\(SLIM_TOPN_KERNEL is set\)"
    with pytest.raises(RuntimeError, match="SLIMGPU_ModelRanks" + why):
        ev.ranks(c.model)
    with pytest.raises(RuntimeError, match="SLIMGPU_ModelEvaluateRanked" + why):
        ev.evaluate_ranked(c.model, (10,))
    monkeypatch.delenv("SLIM_TOPN_KERNEL")
    ranks, _ = ev.ranks(c.model)
    assert np.array_equal(ranks, c.rank) and ev.stats()["path"] == 3
    ev.close()


# ---- 4. an uploaded model is the learned model ---------------------------------------------------------------------------
def test_uploaded_model_gives_the_learned_models_ranks(learned):
    R, T, mat, model = learned
    up = mat.model_from_scipy(model.fetch())
    assert up.nnz == model.nnz
    ev = mat.evaluator(T, ranked=True)
    a, ia, sa = ev.ranks(model, scores=True)
    b, ib, sb = ev.ranks(up, scores=True)
    ev.close()
    up.free()
    assert (a > 0).sum() > 0 and np.array_equal(a, b) and np.array_equal(sa.view(np.uint32), sb.view(np.uint32))


def _views(lib, h):
    v = C.cast(h, C.POINTER(_lib.CsrView)).contents
    n = v.ncols
    cp = np.ctypeslib.as_array(v.colptr, shape=(n + 1,)).copy()
    nnz = int(cp[-1])
    return cp, np.ctypeslib.as_array(v.colind, shape=(max(nnz, 1),))[:nnz].copy(), \
        np.ctypeslib.as_array(v.colval, shape=(max(nnz, 1),))[:nnz].copy()


def test_warm_start_from_an_uploaded_model(monkeypatch):
    """learn_resident(warm=uploaded) == learn_resident(warm=learned) with the fold (SLIM_GPU_NO_CARRY=1), bit for
    bit, on the small matrix of test_resident_model.py."""
    monkeypatch.setenv("SLIM_GPU_NO_CARRY", "1")
    rng = np.random.default_rng(5)
    R = sp.random(900, 300, density=0.05, format="csr", random_state=rng, dtype=np.float32)
    R.data[:] = rng.integers(1, 6, R.nnz).astype(np.float32)
    mat = DeviceMatrix.from_scipy(R)
    lib = mat._lib
    kw = dict(optTol=1e-7, niters=200, seed=3)
    m1, _ = mat.learn_resident(l1r=2.0, l2r=1.0, **kw)
    up = mat.model_from_scipy(m1.fetch())
    a, sa = mat.learn_resident(warm=m1, l1r=2.0, l2r=5.0, **kw)
    b, sb = mat.learn_resident(warm=up, l1r=2.0, l2r=5.0, **kw)
    assert a.nnz == b.nnz > 0 and sa["sweeps"] == sb["sweeps"]
    ha, hb = a.fetch(return_handle=True), b.fetch(return_handle=True)
    for x, y in zip(_views(lib, ha), _views(lib, hb)):
        assert np.array_equal(x.view(np.uint8), y.view(np.uint8))
    for h in (ha, hb):
        lib.SLIM_FreeModel(C.byref(C.c_void_p(h)))
    for m in (m1, up, a, b):
        m.free()
    mat.close()


# ---- 5. the grid above 128 --------------------------------------------------------------------------------------------
PAIR = r"(l1r: \S+ l2r: \S+ nnz:\s+\d+ hr: \S+ hr_head: \S+ hr_tail: \S+ arhr: \S+)"


def _mselect(trn, tst, l1s, l2s, capfd, nrcmds, stride=None):
    from slim_amd import SLIM, SLIMatrix
    params = {"dbglvl": 0, "algo": "cd", "nthreads": 1, "optTol": 1e-7, "niters": 200}
    if stride is not None:
        params["gpu_evalstride"] = stride
    trainmat = SLIMatrix(trn)
    valmat = SLIMatrix(tst, trainmat)
    model = SLIM()
    C.CDLL(None).fflush(None)
    capfd.readouterr()
    model.mselect(params, trainmat, valmat, l1s, l2s, nrcmds=nrcmds)
    C.CDLL(None).fflush(None)
    return model, capfd.readouterr().out


def test_grid_with_lists_of_200_runs_resident(automotive, monkeypatch, capfd, tmp_path):
    R, T = sp.csr_matrix(automotive[0]), sp.csr_matrix(automotive[1])
    nu = R.shape[0]
    l1s, l2s = [1.0, 2.0], [1.0, 5.0]
    monkeypatch.setenv("SLIM_GPU_NO_CARRY", "1")       # a pair's model does not depend on who solved before
    monkeypatch.setenv("SLIM_GPU_RESIDENT", "1")
    monkeypatch.setenv("SLIM_GPU_EVAL_RESIDENT", "1")
    lib = _lib.load()
    model, out = _mselect(R, T, l1s, l2s, capfd, 200)
    lines = re.findall(PAIR, out)
    assert len(lines) == 4, out
    from slim_amd.engine import eval_stats
    assert eval_stats(lib)["path"] == 3                # the last pair was evaluated from ranks, in HBM
    # the same grid by hand: the resident chain and the ranked evaluation; each pair against host-scorer lists
    mat = DeviceMatrix.from_scipy(R)
    mat.expect_solves(4)
    ev = mat.evaluator(T, ranked=True)
    fm = O.head_tail(R, max(R.shape[1], T.shape[1]))
    prev, got = None, []
    for l1 in l1s:
        for l2 in l2s:
            cur, _ = mat.learn_resident(warm=prev, l1r=l1, l2r=l2, optTol=1e-7, niters=200)
            if prev is not None:
                prev.free()
            prev = cur
            g = ev.evaluate_ranked(cur, [200])[0]
            ids, _ = host_lists(lib, cur.fetch(), R, 200, monkeypatch)
            assert_same(figures(g), evaluate_lists(lib, ids, 200, T, fm), "pair %g %g" % (l1, l2))
            got.append((l1, l2, g))
    prev.free()
    ev.close()
    mat.close()
    for line, (l1, l2, g) in zip(lines, got):
        print(line, g)
        assert g["nvalid"] > 0 and g["hr"] > 0
        assert "hr: %.4f " % g["hr"] in line and line.endswith("arhr: %.4f" % g["arhr"])
        assert "hr_head: %.4f hr_tail: %.4f " % (g["hr_head"], g["hr_tail"]) in line
        assert line.startswith("l1r: %.2e l2r: %.2e " % (l1, l2))

    # the command-line program prints the same pair lines
    from slim_amd.io import write_csr_text
    trn_f, tst_f, l12 = str(tmp_path / "trn.csr"), str(tmp_path / "tst.csr"), str(tmp_path / "l12")
    write_csr_text(trn_f, R)
    write_csr_text(tst_f, sp.csr_matrix((T.data, T.indices, T.indptr), shape=T.shape))
    open(l12, "w").write("".join("%g %g\n" % (a, b) for a in l1s for b in l2s))
    exe = os.path.join(ROOT, "slim_amd", "bin", "slim_mselect")
    p = subprocess.run([exe, "-nomodels", "-niters=200", "-nrcmds=200", trn_f, tst_f, l12], capture_output=True,
                       text=True, cwd=str(tmp_path), timeout=280)
    assert p.returncode == 0, p.stdout + p.stderr
    assert re.findall(PAIR, p.stdout) == lines

    # a stride works above 128 too
    _, out3 = _mselect(R, T, l1s, l2s, capfd, 200, stride=3)
    assert "  evaluating every 3-th user: %d of %d\n" % (np.arange(0, nu, 3).size, nu) in out3
    lines3 = re.findall(PAIR, out3)
    assert len(lines3) == 4 and lines3 != lines
