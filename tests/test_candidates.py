"""Candidate sets on the device (include/slim_gpu_cand.h): SLIMGPU_ScoreCandidates, SLIMGPU_MatrixScoreCandidates,
SLIMGPU_ModelEvaluateCandidates, and Py_SLIM_Predict_1vsk's route through them.

The yardstick is never the code under test: per user the existing host call Py_SLIM_GetTopN_1vsk with
nrcmds = nnegs = row length (tests/candidate_cases.py); for rows of one width also oracle predict_1vsk; for the
figures the existing SLIMGPU_Evaluate on the yardstick's lists.  Everything is compared bit for bit.

  floats / ties  1 500 x 1 500 model, 300 users: one chunk per wavefront, rated histories / heavy ties
  wide           6 000 x 6 000 model, 96 users: several chunks, a row of 4096 and one of 4097
"""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp

import slim_oracle as O
from candidate_cases import (P, buffers, candidate_rows, check_lists, check_slot_scores, make_set, untouched,
                             yardstick)
from filtered_cases import cases_fixture, wrap
from slim_amd import _lib
from slim_amd.constants import SLIM_ERROR_INPUT, SLIM_OK
from slim_amd.engine import eval_stats

pytestmark = pytest.mark.gpu
cases = pytest.fixture(scope="module")(cases_fixture)
EVERY = pytest.mark.parametrize("name", ["floats", "ties", "wide"])
LONG_USER = 7   # the user whose row has 4097 entries in `wide`


@pytest.fixture(scope="module")
def rows():
    """(indptr, indices, yardstick) of a case, once; long_row=False: `wide` without its row of 4097."""
    made = {}

    def get(case, long_row=True):
        key = (case.name, long_row)
        if key not in made:
            indptr, indices = candidate_rows(case, seed=61, long_row=long_row)
            made[key] = (indptr, indices, yardstick(case, indptr, indices))
            for a in (indptr, indices):
                a.setflags(write=False)
        return made[key]
    return get


def host_call(c, cs, n, bufs):
    return c.lib.SLIMGPU_ScoreCandidates(c.hw, c.hr, cs, n, *[P(b) for b in bufs])


def matrix_call(c, cs, users, n, bufs):
    u = None if users is None else np.ascontiguousarray(users, np.int32)
    return c.lib.SLIMGPU_MatrixScoreCandidates(c.model.handle, c.mat.handle, cs, 0 if u is None else u.size, P(u), n,
                                               *[P(b) for b in bufs])


# ---- 1. slot scores and lists ----------------------------------------------------------------------------------------
@EVERY
def test_slot_scores_and_lists(cases, rows, name):
    c = cases(name)
    indptr, indices, want = rows(c, long_row=False)
    rc, cs = make_set(c.lib, c.ncols, indptr, indices)
    assert rc == SLIM_OK, _lib.last_error()
    users = range(c.nusers)
    try:
        for n in (0, 1, 10, 64, 65, 4096):
            for what, call in (("host handles", lambda b: host_call(c, cs, n, b)),
                               ("resident", lambda b: matrix_call(c, cs, None, n, b))):
                bufs = buffers(indptr, c.nusers, n)
                assert call(bufs) == SLIM_OK, (what, n, _lib.last_error())
                assert eval_stats(c.lib)["path"] == 5
                check_slot_scores(bufs[0], indptr, indices, want, users, c.nusers)
                if n:
                    check_lists(bufs, indptr, want, users, n)
        # lists alone, scores alone
        bufs = buffers(indptr, c.nusers, 10)
        assert matrix_call(c, cs, None, 10, (None,) + bufs[1:3] + (None,)) == SLIM_OK
        assert matrix_call(c, cs, None, 0, (bufs[0], None, None, None)) == SLIM_OK
        check_slot_scores(bufs[0], indptr, indices, want, users, c.nusers)
        bufs[3][:] = [min(10, int(indptr[u + 1] - indptr[u])) for u in users]     # (not asked for: as the yardstick)
        check_lists(bufs, indptr, want, users, 10)
    finally:
        c.lib.SLIMGPU_CandSetFree(cs)
    # no empty test: repeated ids, scored history items, rows that score
    assert sum(np.unique(indices[indptr[u]:indptr[u + 1]]).size < indptr[u + 1] - indptr[u] for u in users) > 20
    assert sum((want[u][1] != 0).any() for u in users) > c.nusers // 2
    hist_scored = 0
    for u in users:
        h = c.R.indices[c.R.indptr[u]:c.R.indptr[u + 1]]
        hist_scored += bool((want[u][1][np.isin(want[u][0], h)] != 0).any())
    assert hist_scored >= 10


@pytest.mark.parametrize("env", [{"SLIM_TOPN_KEY": "64"}, {"SLIM_TOPN_WAVES": "16"}, {"SLIM_TOPN_CW": "64"},
                                 {"SLIM_CAND_BOUNDS": "search"}, {"SLIM_CAND_BOUNDS": "search", "SLIM_TOPN_CW": "192"}],
                         ids=lambda e: ",".join("%s=%s" % kv for kv in sorted(e.items())))
def test_every_geometry_of_the_chunk_kernel(cases, rows, env, monkeypatch):
    """64-bit keys (chunks of 1536 ids), 16 wavefronts, the narrowest chunks, and the search per chunk that serves
    when a row's chunk bounds do not fit the merge area: the same scores and lists."""
    c = cases("wide")
    indptr, indices, want = rows(c, long_row=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    rc, cs = make_set(c.lib, c.ncols, indptr, indices)
    assert rc == SLIM_OK
    try:
        bufs = buffers(indptr, c.nusers, 65)
        assert matrix_call(c, cs, None, 65, bufs) == SLIM_OK, _lib.last_error()
        check_slot_scores(bufs[0], indptr, indices, want, range(c.nusers), c.nusers)
        check_lists(bufs, indptr, want, range(c.nusers), 65)
    finally:
        c.lib.SLIMGPU_CandSetFree(cs)


# ---- 2. a user subset: the row of the user id, not of the position ---------------------------------------------------
@EVERY
def test_a_user_subset_takes_the_rows_of_its_user_ids(cases, rows, name):
    c = cases(name)
    indptr, indices, want = rows(c, long_row=False)
    S = np.array([u for u in range(3, c.nusers, 3) if u != 12], np.int32)
    assert any(indices[indptr[u]:indptr[u + 1]].tolist() != indices[indptr[q]:indptr[q + 1]].tolist()
               for q, u in enumerate(S))
    rc, cs = make_set(c.lib, c.ncols, indptr, indices)
    assert rc == SLIM_OK
    try:
        for n in (0, 10, 65):
            bufs = buffers(indptr, S.size, n)
            assert matrix_call(c, cs, S, n, bufs) == SLIM_OK, _lib.last_error()
            check_slot_scores(bufs[0], indptr, indices, want, S, c.nusers)
            if n:
                check_lists(bufs, indptr, want, S, n)
        # a set with fewer rows than the last selected user needs
        short = S[-1]
        rc, few = make_set(c.lib, c.ncols, indptr[:short + 1], indices[:indptr[short]])
        assert rc == SLIM_OK
        bufs = buffers(indptr, S.size, 10)
        assert matrix_call(c, few, S, 10, bufs) == SLIM_ERROR_INPUT and untouched(bufs)
        assert "SLIMGPU_MatrixScoreCandidates" in _lib.last_error() and "rows" in _lib.last_error()
        assert matrix_call(c, few, S[:-1], 10, bufs) == SLIM_OK
        c.lib.SLIMGPU_CandSetFree(few)
    finally:
        c.lib.SLIMGPU_CandSetFree(cs)


def test_the_python_layer(cases, rows):
    c = cases("ties")
    indptr, indices, want = rows(c)
    S = np.arange(1, c.nusers, 4, dtype=np.int32)
    X = sp.csr_matrix((c.nusers, c.ncols), dtype=np.float32)
    X.indptr, X.indices, X.data = indptr.copy(), indices.copy(), np.ones(indices.size, np.float32)
    for given in (X, (indptr, indices)):       # a scipy CSR taken as it is, or the two arrays
        cset = c.mat.candidate_set(given)
        slot, (ids, sc, cnt) = c.model.score_candidates(c.mat, cset, users=S, nrcmds=10)
        only = c.model.score_candidates(c.mat, cset)
        cset.close()
        assert slot.size == indices.size and ids.shape == sc.shape == (S.size, 10)
        for q, u in enumerate(S):
            n = min(10, int(indptr[u + 1] - indptr[u]))
            assert cnt[q] == n and np.array_equal(ids[q, :n], want[u][0][:n]) and (ids[q, n:] == -1).all()
            assert np.array_equal(sc[q, :n].view(np.int32), want[u][1][:n].view(np.int32)) and (sc[q, n:] == 0).all()
            assert np.array_equal(slot[indptr[u]:indptr[u + 1]], only[indptr[u]:indptr[u + 1]])
        unsel = np.setdiff1d(np.arange(c.nusers), S)
        assert all((slot[indptr[u]:indptr[u + 1]] == 0).all() for u in unsel)
        for u in range(c.nusers):
            s = only[indptr[u]:indptr[u + 1]]
            order = np.lexsort((np.arange(s.size), -s.astype(np.float64)))
            assert np.array_equal(s[order].view(np.int32), want[u][1].view(np.int32))
    with pytest.raises(ValueError, match="cptr"):
        c.mat.candidate_set((indptr[::-1], indices))


# ---- 3. rows too long for a list -------------------------------------------------------------------------------------
def test_long_rows_get_scores_but_no_lists(cases, rows):
    c = cases("wide")
    indptr, indices, want = rows(c)
    assert indptr[LONG_USER + 1] - indptr[LONG_USER] == 4097 and indptr[7] - indptr[6] == 4096
    rc, cs = make_set(c.lib, c.ncols, indptr, indices)
    assert rc == SLIM_OK
    users = range(c.nusers)
    try:
        for call in (lambda b: host_call(c, cs, 10, b), lambda b: matrix_call(c, cs, None, 10, b),
                     lambda b: matrix_call(c, cs, [5, LONG_USER, 9], 10, b)):
            bufs = buffers(indptr, c.nusers, 10)
            assert call(bufs) == SLIM_ERROR_INPUT and untouched(bufs)
            assert "4097" in _lib.last_error() and "user %d" % LONG_USER in _lib.last_error()
        for call in (lambda b: host_call(c, cs, 0, b), lambda b: matrix_call(c, cs, None, 0, b)):
            bufs = buffers(indptr, c.nusers, 0)
            assert call(bufs) == SLIM_OK, _lib.last_error()
            check_slot_scores(bufs[0], indptr, indices, want, users, c.nusers)
        S = np.array([u for u in users if u != LONG_USER], np.int32)
        bufs = buffers(indptr, S.size, 4096)
        assert matrix_call(c, cs, S, 4096, bufs) == SLIM_OK, _lib.last_error()
        check_slot_scores(bufs[0], indptr, indices, want, S, c.nusers)
        check_lists(bufs, indptr, want, S, 4096)
    finally:
        c.lib.SLIMGPU_CandSetFree(cs)


# ---- 4. Py_SLIM_Predict_1vsk's routing -------------------------------------------------------------------------------
def negatives(c, nnegs, seed):
    rng = np.random.default_rng(seed)
    neg = rng.integers(0, c.ncols, size=(c.nusers, nnegs)).astype(np.int32)
    neg[:, 0], neg[:, 1], neg[:, 2] = -1, c.ncols, neg[:, 3]            # unknown items, a repeated id
    neg[:, 4:7] = np.where(c.ids[:, :3] >= 0, c.ids[:, :3], 0)           # the unfiltered top 3
    return np.ascontiguousarray(neg)


def predict_1vsk(c, neg, n):
    ids, sc = np.full(c.nusers * n, -1, np.int32), np.zeros(c.nusers * n, np.float32)
    rc = c.lib.Py_SLIM_Predict_1vsk(n, neg.shape[1], c.hw, c.hr, neg.ravel(), ids, sc)
    return rc, ids.reshape(-1, n), sc.reshape(-1, n)


@pytest.mark.parametrize("name", ["floats", "ties"])
def test_predict_1vsk_routes_through_the_chunk_scorer(cases, name, monkeypatch):
    c = cases(name)
    monkeypatch.setenv("SLIM_PREDICT", "gpu")
    neg = negatives(c, 1100, seed=71)
    for n in (10, 1100):
        want = O.predict_1vsk(c.W, c.R, neg, nrcmds=n, binary=c.binary)
        rc, ids, sc = predict_1vsk(c, neg, n)
        assert rc == SLIM_OK, _lib.last_error()
        assert eval_stats(c.lib)["path"] == 5
        assert np.array_equal(ids, want[0]) and np.array_equal(sc.view(np.int32), want[1].view(np.int32))
    neg = negatives(c, 100, seed=73)
    want = O.predict_1vsk(c.W, c.R, neg, nrcmds=20, binary=c.binary)
    assert (want[1] != 0).any(1).sum() > c.nusers // 2
    for kernel in (None, "chunk"):
        if kernel:
            monkeypatch.setenv("SLIM_1VSK_KERNEL", kernel)
        rc, ids, sc = predict_1vsk(c, neg, 20)
        assert rc == SLIM_OK, _lib.last_error()
        assert np.array_equal(ids, want[0]) and np.array_equal(sc.view(np.int32), want[1].view(np.int32)), kernel


# ---- 5. refusals -----------------------------------------------------------------------------------------------------
def test_a_model_with_shuffled_rows_is_refused(cases, rows, monkeypatch):
    c = cases("floats")
    indptr, indices, _ = rows(c)
    W = c.W.copy()
    rng = np.random.default_rng(11)
    for r in (3, 57, 1499):
        s, e = W.indptr[r], W.indptr[r + 1]
        p = rng.permutation(e - s)
        while np.all(np.diff(W.indices[s:e][p]) > 0):
            p = rng.permutation(e - s)
        W.indices[s:e], W.data[s:e] = W.indices[s:e][p], W.data[s:e][p]
    hw = wrap(c.lib, W)                                   # (Py_csr_wrapper keeps a row's order as given)
    C.cast(hw, C.POINTER(_lib.CsrView)).contents.ncols = c.ncols
    rc, cs = make_set(c.lib, c.ncols, indptr, indices)
    assert rc == SLIM_OK
    try:
        bufs = buffers(indptr, c.nusers, 10)
        assert c.lib.SLIMGPU_ScoreCandidates(hw, c.hr, cs, 10, *[P(b) for b in bufs]) == SLIM_ERROR_INPUT
        assert "row order" in _lib.last_error() and untouched(bufs)
        monkeypatch.setenv("SLIM_PREDICT", "gpu")
        assert c.lib.Py_SLIM_ScoreCandidates(hw, c.hr, cs, 10, *[P(b) for b in bufs]) == SLIM_ERROR_INPUT
        assert "row order" in _lib.last_error() and untouched(bufs)
        # Py_SLIM_Predict_1vsk still answers, from the host: a candidate meets a model row once, so the order
        # inside the row cannot show in its sum
        monkeypatch.delenv("SLIM_PREDICT")
        neg = negatives(c, 1100, seed=71)
        want = O.predict_1vsk(c.W, c.R, neg, nrcmds=10, binary=c.binary)
        ids, sc = np.full(c.nusers * 10, -1, np.int32), np.zeros(c.nusers * 10, np.float32)
        assert c.lib.Py_SLIM_Predict_1vsk(10, 1100, hw, c.hr, neg.ravel(), ids, sc) == SLIM_OK
        assert np.array_equal(ids.reshape(-1, 10), want[0])
        assert np.array_equal(sc.reshape(-1, 10).view(np.int32), want[1].view(np.int32))
    finally:
        c.lib.SLIMGPU_CandSetFree(cs)
        c.lib.Py_csr_free(hw)
    # a set made for another number of items
    rc, cs = make_set(c.lib, c.ncols + 1, indptr, indices)
    assert rc == SLIM_OK
    for call in (lambda b: host_call(c, cs, 10, b), lambda b: matrix_call(c, cs, None, 10, b)):
        bufs = buffers(indptr, c.nusers, 10)
        assert call(bufs) == SLIM_ERROR_INPUT and untouched(bufs) and str(c.ncols + 1) in _lib.last_error()
    c.lib.SLIMGPU_CandSetFree(cs)


# ---- 6. evaluation ---------------------------------------------------------------------------------------------------
def held_out(c, indptr, indices, want, seed):
    """A test matrix with 0-3 items per user -- candidates of the user's row and others -- and a head / tail marker."""
    rng = np.random.default_rng(seed)
    T = sp.lil_matrix((c.nusers, c.ncols), dtype=np.float32)
    for u in range(c.nusers):
        row = indices[indptr[u]:indptr[u + 1]]
        row = row[(row >= 0) & (row < c.ncols)]
        k = int(rng.integers(0, 4))
        picks = rng.choice(row, size=min(k, row.size), replace=False).tolist() if row.size else []
        if u % 4 == 0:
            picks.append(int(rng.integers(c.ncols)))
        if u % 5 == 1 and row.size and 0 <= want[u][0][0] < c.ncols:
            picks.append(int(want[u][0][0]))        # (the head of the row's order: a hit at every cutoff)
        for it in picks:
            T[u, it] = 1.0
    return sp.csr_matrix(T), rng.integers(0, 2, c.ncols).astype(np.int32)


def evaluate_lists(c, want, indptr, users, n, T, fm):
    """The existing SLIMGPU_Evaluate on the first n of the yardstick's orders (position q: users[q])."""
    lists = np.full((len(users), n), -1, np.int32)
    cnt = np.zeros(len(users), np.int32)
    for q, u in enumerate(users):
        cnt[q] = min(n, int(indptr[u + 1] - indptr[u]))
        lists[q, :cnt[q]] = want[u][0][:cnt[q]]
    ht = wrap(c.lib, sp.csr_matrix(T)[np.asarray(users)])
    met, nv = np.zeros(4), np.zeros(3, np.int32)
    assert c.lib.SLIMGPU_Evaluate(len(users), n, lists.ravel(), cnt, ht, fm, fm.size, met, nv) == SLIM_OK, \
        _lib.last_error()
    c.lib.Py_csr_free(ht)
    return met, nv


@EVERY
def test_evaluation_of_candidate_lists(cases, rows, name):
    c = cases(name)
    indptr, indices, want = rows(c, long_row=False)
    T, fm = held_out(c, indptr, indices, want, seed=83)
    cutoffs = (1, 5, 10, 64)
    cset = c.mat.candidate_set((indptr, indices))
    hrs = []
    try:
        for users in (None, np.arange(2, c.nusers, 3, dtype=np.int32)):
            ev = c.mat.evaluator(T, fmarker=fm, cutoffs=cutoffs, users=users)
            got = ev.evaluate_candidates(c.model, cset)
            first = ev.stats()
            again = ev.evaluate_candidates(c.model, cset)
            st = ev.stats()
            ev.close()
            print(name, "second call", st)
            assert first["path"] == st["path"] == 5
            assert st["device_allocs"] == 0 and st["h2d_bytes"] == 0 and st["d2h_bytes"] <= 8 + 32 * len(cutoffs)
            sel = list(range(c.nusers)) if users is None else users.tolist()
            for row, row2, n in zip(got, again, cutoffs):
                met, nv = evaluate_lists(c, want, indptr, sel, n, T, fm)
                g = np.array([row[k] for k in ("hr", "hr_head", "hr_tail", "arhr")])
                gn = [row[k] for k in ("nvalid", "nvalid_head", "nvalid_tail")]
                print(name, n, "got ", g.tolist(), gn, "want", met.tolist(), nv.tolist())
                assert row["nrcmds"] == n and row == row2
                assert gn == nv.tolist() and np.array_equal(g, met)
                hrs.append(met[0])
    finally:
        cset.close()
    assert 0 < min(hrs) and len(set(hrs)) > 2      # no empty test: hits, and the cutoffs matter
    # the long row: an evaluation makes lists, so it is refused
    if name == "wide":
        indptr, indices, _ = rows(c)
        cset = c.mat.candidate_set((indptr, indices))
        ev = c.mat.evaluator(T, fmarker=fm, cutoffs=cutoffs)
        with pytest.raises(RuntimeError, match="4097"):
            ev.evaluate_candidates(c.model, cset)
        ev.close()
        cset.close()
