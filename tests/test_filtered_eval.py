"""Evaluation and ranks under a candidate filter (include/slim_gpu_filter.h): SLIMGPU_ModelEvaluateAtFiltered,
SLIMGPU_ModelRanksFiltered, SLIMGPU_ModelEvaluateRankedFiltered, Py_SLIM_MselectFiltered and the Evaluator's
filter= keyword.

The yardstick is never the code under test: filtered_cases.Case.expected -- the unchanged host scorer's full
ranking, filtered in numpy.  Fed to the existing SLIMGPU_Evaluate it gives the figures, which are compared as
doubles with ==; its position lookup gives ranks and scores, compared with array_equal.  A test entry the
filter removes stays in its test row: a miss at every cutoff, rank 0, score 0, counted in every denominator.

  plain / ties / floats  1 500 x 1 500 model, 300 users: one chunk per wavefront
  wide                   6 000 x 6 000 model, 96 users: several chunks

Every case asserts, on the yardstick alone, that it is no empty test: at least 10 test entries lose their rank
to the filter, at least 10 move up, and HR differs from the unfiltered HR at every cutoff used up to 100.
"""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
import scipy.sparse as sp

import slim_oracle as O
from conftest import ROOT
from filtered_cases import KEYS, NKEYS, P, assert_same, cases_fixture, evaluate_lists, figures, positions, wrap
from slim_amd import _lib
from slim_amd.constants import SLIM_ERROR_INPUT, SLIM_OK
from slim_amd.engine import DeviceMatrix, ItemFilter, eval_stats

pytestmark = pytest.mark.gpu
cases = pytest.fixture(scope="module")(cases_fixture)
NAMES = ["plain", "ties", "floats", "wide"]
EVERY = pytest.mark.parametrize("name", NAMES)
LONG_ROW_USER, WIDE_ID_USER, LONG_ROW = 4, 2, 150


def make_test_rows(c, width):
    """Built from the host ranking so that every kind of entry occurs.  A user with candidates holds its unfiltered
    rank-1, rank-5 and (where it has that many) rank-41 item, one history item, one never-touched item and the
    rank-5 item a second time; every 6th user has no test row; one row holds an id beyond the model; one user
    has LONG_ROW entries (more than a pass of SLIM_TOPN_RANK_GROUP=64 serves)."""
    rng = np.random.default_rng(3)
    ptr, ind = [0], []
    kinds = dict(first=0, fifth=0, fortyfirst=0, history=0, untouched=0, twice=0, empty=0, wide=0, long=0)
    for u in range(c.nusers):
        row = []
        n = int(c.ncand[u])
        if u % 6 == 5:
            kinds["empty"] += 1
        elif n > 0:
            lst = c.ids[u, :n]
            hist = c.R.indices[c.R.indptr[u]:c.R.indptr[u + 1]]
            free = np.setdiff1d(np.arange(c.ncols), np.concatenate([lst, hist]))
            row.append(int(lst[0]))
            kinds["first"] += 1
            if n >= 5:
                row.append(int(lst[4]))
                kinds["fifth"] += 1
            if n >= 41:
                row.append(int(lst[40]))
                kinds["fortyfirst"] += 1
            row.append(int(hist[rng.integers(hist.size)]))
            kinds["history"] += 1
            if free.size:
                row.append(int(free[rng.integers(free.size)]))
                kinds["untouched"] += 1
            if n >= 5:
                row.append(int(lst[4]))
                kinds["twice"] += 1
            if u == WIDE_ID_USER:
                row.append(c.ncols + 7)
                kinds["wide"] += 1
            if u == LONG_ROW_USER:      # its ranking from rank 6 on, every other rank, up to LONG_ROW entries
                assert n >= 5 + 2 * LONG_ROW
                row += [int(i) for i in lst[5::2][:LONG_ROW - len(row)]]
                assert len(row) == LONG_ROW
                kinds["long"] += 1
        ind += row
        ptr.append(len(ind))
    assert all(v > 0 for v in kinds.values()), kinds
    # (kept as built: rows in no order, one id twice)
    return sp.csr_matrix((np.ones(len(ind), np.float32), np.array(ind, np.int32), np.array(ptr)),
                         shape=(c.nusers, width))


def straddling_mask(ncols):
    """Six items in ten allowed, with set and clear bits on both sides of ids 31/32, 63/64, of every multiple of 64
    (every chunk of every geometry begins at one) and at the last id."""
    allowed = np.random.default_rng(83).random(ncols) < 0.6
    allowed[31], allowed[32] = True, False
    for j, b in enumerate(range(64, ncols, 64)):
        allowed[b - 1], allowed[b] = j % 2 == 1, j % 2 == 0
    allowed[63], allowed[64] = False, True
    allowed[ncols - 2], allowed[ncols - 1] = False, True
    return allowed


class Setup(object):
    """Per case and once: the test rows, the marker, the filter's description, the yardstick's filtered and
    unfiltered rankings with the ranks and scores they give.  Read-only afterwards."""

    def __init__(self, c):
        self.c = c
        self.width = c.ncols + 100
        self.T = make_test_rows(c, self.width)
        self.fm = O.head_tail(sp.csr_matrix(c.R), self.width)
        self.allowed = straddling_mask(c.ncols)
        self.X = c.exclusions(seed=89, xusers=c.nusers - 10)     # the last ten users have no row
        self.users = np.arange(c.nusers)
        self.plain = (c.ids, c.sc)
        self.flt = c.expected(c.ncols, self.allowed, self.X)[:2]
        for a in self.flt:
            a.setflags(write=False)
        self.rank0, self.score0 = positions(c.ids, c.sc, self.T, self.users)
        self.rank, self.score = positions(self.flt[0], self.flt[1], self.T, self.users)
        self._figures = {}
        # the vacuous-pass cap, on the yardstick alone
        lost = int(((self.rank0 > 0) & (self.rank == 0)).sum())
        moved = int(((self.rank > 0) & (self.rank < self.rank0)).sum())
        print(c.name, "test entries", self.T.nnz, "lose their rank to the filter", lost, "move up", moved)
        assert lost >= 10 and moved >= 10
        for n in (1, 10, 64, 100):
            a, b = self.want(n)[0][0], self.want(n, filtered=False)[0][0]
            print(c.name, "HR@%d filtered %.6f unfiltered %.6f" % (n, a, b))
            assert a != b

    def want(self, n, filtered=True):
        """SLIMGPU_Evaluate's figures on the yardstick lists of length n."""
        if (n, filtered) not in self._figures:
            ids = self.flt[0] if filtered else self.plain[0]
            self._figures[(n, filtered)] = evaluate_lists(self.c.lib, ids, n, self.T, self.fm)
        return self._figures[(n, filtered)]

    def item_filter(self):
        return self.c.mat.item_filter(allowed=np.flatnonzero(self.allowed), exclusions=self.X)


@pytest.fixture(scope="module")
def setups(cases):
    made = {}

    def get(name):
        if name not in made:
            made[name] = Setup(cases(name))
        return made[name]
    return get


# ---- 1. filtered ranks ---------------------------------------------------------------------------------------------
@EVERY
@pytest.mark.parametrize("group", [None, "64"], ids=["one-pass", "groups-of-64"])
def test_filtered_ranks_are_the_positions_in_the_filtered_ranking(setups, name, group, monkeypatch):
    s = setups(name)
    c = s.c
    if group:
        monkeypatch.setenv("SLIM_TOPN_RANK_GROUP", group)
    flt = s.item_filter()
    ev = c.mat.evaluator(s.T, fmarker=s.fm, ranked=True)
    ranks, indptr, scores = ev.ranks(c.model, scores=True, filter=flt)
    st = ev.stats()
    plain = ev.ranks(c.model, scores=True)
    ev.close()
    flt.close()
    assert st["path"] == 3 and indptr.tolist() == s.T.indptr.tolist() and ranks.size == s.T.nnz
    bad = np.flatnonzero(ranks != s.rank)
    print(name, group, "entries", ranks.size, "ranked", int((s.rank > 0).sum()), "mismatches", bad.size)
    assert bad.size == 0, (bad[:10], ranks[bad[:10]], s.rank[bad[:10]])
    assert scores.dtype == np.float32 and np.array_equal(scores.view(np.uint32), s.score.view(np.uint32))
    # the unfiltered call is what it was
    assert np.array_equal(plain[0], s.rank0) and np.array_equal(plain[2].view(np.uint32), s.score0.view(np.uint32))


@EVERY
def test_filtered_ranks_of_a_user_subset_take_the_row_of_the_user_id(setups, name):
    s = setups(name)
    c = s.c
    S = np.arange(1, c.nusers - 10, 3, dtype=np.int32)         # strictly ascending, position q is user 3 q + 1
    rows = [sorted(set(s.X.indices[s.X.indptr[u]:s.X.indptr[u + 1]].tolist())) for u in range(s.X.shape[0])]
    assert any(rows[u] != rows[q] for q, u in enumerate(S) if u != q)
    flt = s.item_filter()
    ev = c.mat.evaluator(s.T, fmarker=s.fm, ranked=True, users=S)
    ranks, indptr, scores = ev.ranks(c.model, scores=True, filter=flt)
    ev.close()
    flt.close()
    ids, sc, _ = c.expected(c.ncols, s.allowed, s.X, S)
    want = positions(ids, sc, s.T, S)
    assert np.array_equal(np.diff(indptr), np.diff(s.T.indptr)[S])
    assert np.array_equal(ranks, want[0]) and np.array_equal(scores.view(np.uint32), want[1].view(np.uint32))
    # a scorer that took the exclusion row of the POSITION would give other ranks
    by_position = sp.csr_matrix((c.nusers, c.ncols), dtype=np.float32)
    lens = np.zeros(c.nusers, np.int64)
    lens[S] = np.diff(s.X.indptr)[:S.size]
    by_position.indptr = np.concatenate(([0], np.cumsum(lens)))
    by_position.indices = s.X.indices[:s.X.indptr[S.size]].copy()
    by_position.data = np.ones(by_position.indices.size, np.float32)
    wrong = positions(*c.expected(c.ncols, s.allowed, by_position, S)[:2], s.T, S)
    assert not np.array_equal(wrong[0], want[0])


# ---- 2. filtered evaluation: the chunk path, the wave path, the ranked evaluation ------------------------------------
@EVERY
def test_filtered_figures_are_those_of_evaluate_on_the_filtered_lists(setups, name):
    s = setups(name)
    c = s.c
    flt = s.item_filter()
    got = {}
    for what, cutoffs, path in (("chunk", (1, 10, 64), 1), ("wave", (10, 100), 2),
                                ("ranked", (1, 10, 100, 200, c.ncols), 3)):
        if what == "ranked":
            ev = c.mat.evaluator(s.T, fmarker=s.fm, ranked=True)
            rows = ev.evaluate_ranked(c.model, cutoffs, filter=flt)
        else:
            ev = c.mat.evaluator(s.T, fmarker=s.fm, cutoffs=cutoffs)
            rows = ev.evaluate_at(c.model, filter=flt)
            last = ev.evaluate(c.model, filter=flt)              # the longest lists' row
            assert all(last[k] == rows[-1][k] for k in KEYS + NKEYS)
        assert ev.stats()["path"] == path
        ev.close()
        for row, n in zip(rows, cutoffs):
            assert row["nrcmds"] == n
            assert_same(figures(row), s.want(n), "%s %s @%d" % (name, what, n))
            got[(what, n)] = figures(row)
    for a, b, n in (("chunk", "wave", 10), ("chunk", "ranked", 1), ("chunk", "ranked", 10), ("wave", "ranked", 10),
                    ("wave", "ranked", 100)):
        assert_same(got[(a, n)], got[(b, n)], "%s = %s @%d" % (a, b, n))
    # removed entries stay in the denominators
    assert got[("ranked", 10)][1].tolist() == s.want(10, filtered=False)[1].tolist()
    flt.close()


@EVERY
def test_filtered_figures_of_a_user_subset(setups, name):
    s = setups(name)
    c = s.c
    S = np.arange(1, c.nusers - 10, 3, dtype=np.int32)
    ids = c.expected(c.ncols, s.allowed, s.X, S)[0]
    TS = sp.csr_matrix(s.T)[S]
    flt = s.item_filter()
    for cutoffs in ((1, 10, 64), (10, 100)):
        ev = c.mat.evaluator(s.T, fmarker=s.fm, cutoffs=cutoffs, users=S)
        rows = ev.evaluate_at(c.model, filter=flt)
        ev.close()
        for row, n in zip(rows, cutoffs):
            assert_same(figures(row), evaluate_lists(c.lib, ids, n, TS, s.fm), "%s subset @%d" % (name, n))
    flt.close()


# ---- 3. no filter, and a filter that filters nothing -----------------------------------------------------------------
@EVERY
def test_null_and_permissive_filters_give_the_unfiltered_output(setups, name):
    s = setups(name)
    c = s.c
    none = sp.csr_matrix((0, c.ncols), dtype=np.float32)
    permissive = c.mat.item_filter(allowed=np.arange(c.ncols), exclusions=none)
    rows_only = c.mat.item_filter(exclusions=sp.csr_matrix((c.nusers, c.ncols), dtype=np.float32))
    ev = c.mat.evaluator(s.T, fmarker=s.fm, cutoffs=(1, 10, 64))
    wave = c.mat.evaluator(s.T, fmarker=s.fm, cutoffs=(10, 100))
    cuts = (1, 10, 100, 200, c.ncols)
    base = (ev.ranks(c.model, scores=True), ev.evaluate_at(c.model), wave.evaluate_at(c.model),
            ev.evaluate_ranked(c.model, cuts))
    assert np.array_equal(base[0][0], s.rank0)
    for n, row in zip((1, 10, 64), base[1]):
        assert_same(figures(row), s.want(n, filtered=False), "%s unfiltered @%d" % (name, n))
    for f in (None, permissive, rows_only):
        got = (ev.ranks(c.model, scores=True, filter=f), ev.evaluate_at(c.model, filter=f),
               wave.evaluate_at(c.model, filter=f), ev.evaluate_ranked(c.model, cuts, filter=f))
        assert np.array_equal(got[0][0], base[0][0])
        assert np.array_equal(got[0][2].view(np.uint32), base[0][2].view(np.uint32))
        assert got[1:] == base[1:]
    for f in (permissive, rows_only):
        f.close()
    ev.close()
    wave.close()


# ---- 4. stats and refusals -------------------------------------------------------------------------------------------
def test_steady_state_and_a_filter_of_another_width(setups):
    s = setups("floats")
    c = s.c
    lib = c.lib
    for make, call in ((dict(cutoffs=(1, 10, 64)), lambda ev, f: ev.evaluate_at(c.model, filter=f)),
                       (dict(cutoffs=(10, 100)), lambda ev, f: ev.evaluate_at(c.model, filter=f)),
                       (dict(ranked=True), lambda ev, f: ev.ranks(c.model, filter=f)),
                       (dict(ranked=True), lambda ev, f: ev.evaluate_ranked(c.model, (10, 200), filter=f))):
        flt = s.item_filter()
        ev = c.mat.evaluator(s.T, fmarker=s.fm, **make)
        call(ev, flt)
        first = ev.stats()
        assert first["h2d_bytes"] > 0                    # the filter's device copy, made by its first call
        for _ in range(2):
            call(ev, flt)
            st = ev.stats()
            print(make, st)
            assert st["device_allocs"] == 0 and st["h2d_bytes"] == 0
        ev.close()
        flt.close()
    # a filter made for another number of items: refused before anything is queued or written
    other = ItemFilter(c.ncols + 1, allowed=[0, 1, 2], lib=lib)
    ev = c.mat.evaluator(s.T, fmarker=s.fm, cutoffs=(10,))
    evr = c.mat.evaluator(s.T, fmarker=s.fm, ranked=True)
    met, nv = np.full(4, -3.0), np.full(3, -3, np.int32)
    assert lib.SLIMGPU_ModelEvaluateAtFiltered(ev.handle, c.model.handle, other.handle, 1, met, nv) == SLIM_ERROR_INPUT
    assert "filter" in _lib.last_error() and str(c.ncols + 1) in _lib.last_error()
    cut = np.array([10], np.int32)
    assert lib.SLIMGPU_ModelEvaluateRankedFiltered(evr.handle, c.model.handle, other.handle, 1, P(cut), met,
                                                   nv) == SLIM_ERROR_INPUT
    assert "filter" in _lib.last_error()
    rk, sc = np.full(s.T.nnz, -3, np.int32), np.full(s.T.nnz, -3.0, np.float32)
    assert lib.SLIMGPU_ModelRanksFiltered(evr.handle, c.model.handle, other.handle, P(rk), P(sc)) == SLIM_ERROR_INPUT
    assert "filter" in _lib.last_error()
    assert (met == -3).all() and (nv == -3).all() and (rk == -3).all() and (sc == -3).all()
    with pytest.raises(RuntimeError, match="SLIMGPU_ModelRanksFiltered"):
        evr.ranks(c.model, filter=other)
    for h in (ev, evr, other):
        h.close()


# ---- 5. the grid -------------------------------------------------------------------------------------------------------
PAIR = r"(l1r: \S+ l2r: \S+ nnz:\s+\d+ hr: \S+ hr_head: \S+ hr_tail: \S+ arhr: \S+)"
PARAMS = {"dbglvl": 0, "algo": "cd", "nthreads": 1, "optTol": 1e-7, "niters": 200}


def grid_filter(R, T):
    """A block set (every third item) and an exclusion matrix: every fourth user's held-out items and ten more."""
    rng = np.random.default_rng(97)
    blocked = np.arange(0, R.shape[1], 3)
    X = sp.lil_matrix(R.shape, dtype=np.float32)
    for u in range(0, R.shape[0], 4):
        for i in T.indices[T.indptr[u]:T.indptr[u + 1]].tolist() + rng.choice(R.shape[1], 10).tolist():
            X[u, i] = 1.0
    return blocked, sp.csr_matrix(X)


def test_the_grid_selects_under_the_filter(automotive, monkeypatch, capfd, tmp_path):
    from slim_amd import SLIM, SLIMatrix
    from slim_amd.interface import _prepare, build_options
    R, T = sp.csr_matrix(automotive[0]), sp.csr_matrix(automotive[1])
    l1s, l2s = [1.0, 2.0], [1.0, 5.0]
    blocked, X = grid_filter(R, T)
    monkeypatch.setenv("SLIM_GPU_NO_CARRY", "1")
    monkeypatch.setenv("SLIM_GPU_RESIDENT", "1")
    monkeypatch.setenv("SLIM_GPU_EVAL_RESIDENT", "1")
    trainmat = SLIMatrix(R)
    valmat, xmat = SLIMatrix(T, trainmat), SLIMatrix(X, trainmat)
    grids, lines = {}, {}
    for n in (10, 200):
        model = SLIM()
        C.CDLL(None).fflush(None)
        capfd.readouterr()
        model.mselect(dict(PARAMS), trainmat, valmat, l1s, l2s, nrcmds=n, blocked_items=blocked.tolist(), exclude=xmat)
        C.CDLL(None).fflush(None)
        out = capfd.readouterr().out
        assert eval_stats()["path"] == (1 if n == 10 else 3)
        lines[n] = re.findall(PAIR, out)
        assert len(lines[n]) == 4, out
        assert "  item filter: %d of %d items allowed, %d exclusion entries\n" % (
            R.shape[1] - blocked.size, R.shape[1], X.nnz) in out
        grids[n] = model.mselect_result
    # the same chain by hand: the best-HR pair's figures are those of its resident model under the filter
    mat = DeviceMatrix.from_scipy(R)
    mat.expect_solves(4)
    flt = mat.item_filter(blocked=blocked, exclusions=X)
    ev = mat.evaluator(T, nrcmds=10)
    evr = mat.evaluator(T, ranked=True)
    prev, seen = None, {10: [], 200: []}
    for l1 in l1s:
        for l2 in l2s:
            cur, _ = mat.learn_resident(warm=prev, l1r=l1, l2r=l2, optTol=1e-7, niters=200)
            if prev is not None:
                prev.free()
            prev = cur
            seen[10].append((l1, l2, ev.evaluate(cur, filter=flt), ev.evaluate(cur)))
            seen[200].append((l1, l2, evr.evaluate_ranked(cur, [200], filter=flt)[0], evr.evaluate_ranked(cur, [200])[0]))
    prev.free()
    for n in (10, 200):
        l1, l2, hr, arhr = grids[n]["bestHR"]
        mine = [g for a, b, g, _ in seen[n] if (a, b) == (l1, l2)]
        print(n, grids[n], mine)
        assert len(mine) == 1 and mine[0]["hr"] == hr and mine[0]["arhr"] == arhr and hr > 0
        assert hr == max(g["hr"] for _, _, g, _ in seen[n])
        assert all(g["hr"] != plain["hr"] and g["nvalid"] == plain["nvalid"] for _, _, g, plain in seen[n])
    for h in (ev, evr, flt, mat):
        h.close()

    # slim_mselect -blockfile -exclfile prints the same pair lines and the same header line
    from slim_amd.io import write_csr_text
    names = [str(tmp_path / f) for f in ("trn.csr", "tst.csr", "excl.csr", "l12", "blocked")]
    for f, M in zip(names, (R, sp.csr_matrix((T.data, T.indices, T.indptr), shape=T.shape), X)):
        write_csr_text(f, M)
    open(names[3], "w").write("".join("%g %g\n" % (a, b) for a in l1s for b in l2s))
    open(names[4], "w").write("".join("%d\n" % i for i in blocked))
    p = subprocess.run([os.path.join(ROOT, "slim_amd", "bin", "slim_mselect"), "-nomodels", "-niters=200", "-nrcmds=10",
                        "-blockfile=" + names[4], "-exclfile=" + names[2], names[0], names[1], names[3]],
                       capture_output=True, text=True, cwd=str(tmp_path), timeout=280)
    assert p.returncode == 0, p.stdout + p.stderr
    assert re.findall(PAIR, p.stdout) == lines[10]
    assert "  item filter: %d of %d items allowed, %d exclusion entries\n" % (
        R.shape[1] - blocked.size, R.shape[1], X.nnz) in p.stdout

    # without the evaluation in HBM there is no filtered grid: refused before the first solve
    monkeypatch.setenv("SLIM_GPU_EVAL_RESIDENT", "0")
    lib = _lib.load()
    view = _prepare(dict(PARAMS))
    view.set("nrcmds", 10)
    iopt, dopt = build_options(view)
    mat_filter = ItemFilter(R.shape[1], blocked=blocked, lib=lib)
    best = [C.c_double(0.0) for _ in range(8)]
    C.CDLL(None).fflush(None)
    capfd.readouterr()
    bad = lib.Py_SLIM_MselectFiltered(trainmat.handle, valmat.handle, iopt, dopt, np.array(l1s), np.array(l2s), 2, 2,
                                      *([C.byref(b) for b in best] + [mat_filter.handle]))
    C.CDLL(None).fflush(None)
    out = capfd.readouterr().out
    mat_filter.close()
    assert bad == SLIM_ERROR_INPUT and "Estimating" not in out
    assert "SLIM_GPU_EVAL_RESIDENT=0" in _lib.last_error()
