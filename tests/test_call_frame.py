"""The frame that every device entry point of the scorers stands in (slim_amd/csrc/call_frame.hpp, the evaluation
frame of resident_eval.hip): what a caller can see of it.  The order in which refusals are judged, with the outputs
of a refused call untouched; the edges of the shared staging (a user list of the last row, the full list given
explicitly, an eval set without a position, the slices of a long-list call); and the one per-evaluation invariant,
the staleness of the group rows.  Every expected value was read off the code before the host code was unified: the
file passes on that build as well (SLIM_AMD_LIB points the loader at another build of the library).

The calls that name themselves in a HIP failure (the two ranked calls under a filter) cannot be shown here: no test
provokes a device failure.  Their refusals carry the right name already and are part of the cases below.

The shape is tiny on purpose: 7 users x 12 items built here; the golden ml100k split where a real model is needed.
"""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp

from slim_amd import _lib
from slim_amd.constants import SLIM_ERROR_INPUT, SLIM_OK
from slim_amd.engine import CandidateSet, DeviceMatrix, ItemFilter, eval_stats, list_stats

NU, NI = 7, 12
P = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)  # noqa: E731
I32 = lambda *v: np.array(v, np.int32)  # noqa: E731


def tiny():
    """(R, T, W): 7 users x 12 items, one held-out item per user, a 12 x 12 model whose rows ascend."""
    rng = np.random.default_rng(11)
    R = sp.random(NU, NI, density=0.4, format="csr", random_state=rng, dtype=np.float32)
    R.data[:] = 1.0
    R = sp.csr_matrix(R + sp.csr_matrix((np.ones(NU, np.float32), (np.arange(NU), np.arange(NU))), shape=(NU, NI)))
    R.data[:] = 1.0
    R.sort_indices()
    T = sp.csr_matrix((np.ones(NU, np.float32), (np.arange(NU), (np.arange(NU) + 5) % NI)), shape=(NU, NI))
    W = sp.random(NI, NI, density=0.6, format="csr", random_state=rng, dtype=np.float32)
    W.setdiag(0)
    W.eliminate_zeros()
    W.sort_indices()
    return R, T, W


def refused(rc, name, reason):
    msg = _lib.last_error()
    print(rc, msg)
    return rc == SLIM_ERROR_INPUT and msg.startswith(name + ": ") and reason in msg


class Outputs(object):
    """Arrays handed to a call as outputs, filled with a pattern; untouched() after a refusal."""

    def __init__(self, **shapes):
        self.arrays, self.before = {}, {}
        for k, (n, dtype) in shapes.items():
            a = (np.arange(n) % 97 + 3).astype(dtype)
            self.arrays[k], self.before[k] = a, a.copy()

    def __getitem__(self, k):
        return P(self.arrays[k])

    def untouched(self):
        return all(np.array_equal(self.arrays[k], self.before[k]) for k in self.arrays)


# ---- refusal precedence without a device ------------------------------------------------------------------------
def test_ranked_cutoff_count_is_judged_before_the_handles():
    """SLIMGPU_ModelEvaluateRanked: ncutoffs = 0 wins over a null model (and a null eval set)."""
    lib = _lib.load()
    met, nv = np.full(4, 7.0), np.full(3, 7, np.int32)
    cut = I32(5)
    rc = lib.SLIMGPU_ModelEvaluateRanked(None, None, 0, P(cut), met, nv)
    assert refused(rc, "SLIMGPU_ModelEvaluateRanked", "between 1 and 32 cutoffs, not 0")
    assert (met == 7.0).all() and (nv == 7).all()


def test_host_explain_judges_nwhy_before_the_set():
    """SLIMGPU_ExplainCandidates (host handles): nwhy = 0 wins over a set made for another ncols; no device yet."""
    from slim_amd.engine import _wrap_rows
    lib = _lib.load()
    R, _, W = tiny()
    hw, hr = _wrap_rows(lib, W), _wrap_rows(lib, R)
    cs = CandidateSet(NI + 1, (np.arange(NU + 1, dtype=np.int64), np.zeros(NU, np.int32)), lib=lib)
    out = Outputs(items=(NU, np.int32), terms=(NU, np.float32), support=(NU, np.int32))
    try:
        rc = lib.SLIMGPU_ExplainCandidates(hw, hr, cs.handle, 0, out["items"], out["terms"], out["support"])
        assert refused(rc, "SLIMGPU_ExplainCandidates", "nwhy must be between 1 and 16, not 0")
        rc = lib.SLIMGPU_ExplainCandidates(hw, hr, cs.handle, 2, out["items"], out["terms"], out["support"])
        assert refused(rc, "SLIMGPU_ExplainCandidates", "the candidate set was made for 13 items, the model has 12")
        assert out.untouched()
    finally:
        cs.close()
        lib.Py_csr_free(hw)
        lib.Py_csr_free(hr)


# ---- on the device ----------------------------------------------------------------------------------------------
class Tiny(object):
    def __init__(self):
        self.lib = _lib.load()
        self.R, self.T, self.W = tiny()
        self.mat = DeviceMatrix.from_scipy(self.R)
        self.model = self.mat.model_from_scipy(self.W)
        self.fm = (np.arange(NI) % 2).astype(np.int32)
        rows = (np.arange(NU + 1, dtype=np.int64) * 3, (np.arange(3 * NU, dtype=np.int32) * 5) % NI)
        self.cset = CandidateSet(NI, rows, lib=self.lib)
        self.cset13 = CandidateSet(NI + 1, rows, lib=self.lib)
        self.filter13 = ItemFilter(NI + 1, blocked=[0], lib=self.lib)

    def evaluator(self, T=None, **kw):
        return self.mat.evaluator(self.T if T is None else T, fmarker=self.fm, **kw)

    def close(self):
        for o in (self.cset, self.cset13, self.filter13):
            o.close()
        self.model.free()
        self.mat.close()


@pytest.fixture(scope="module")
def t():
    d = Tiny()
    yield d
    d.close()


gpu = pytest.mark.gpu
DESC = I32(3, 1)     # a user list that does not ascend


@gpu
def test_score_candidates_judges_the_users_before_the_set(t):
    out = Outputs(slot=(3 * NU, np.float32), ids=(2 * 2, np.int32), sc=(2 * 2, np.float32), cnt=(2, np.int32))
    rc = t.lib.SLIMGPU_MatrixScoreCandidates(t.model.handle, t.mat.handle, t.cset13.handle, 2, P(DESC), 2, out["slot"],
                                             out["ids"], out["sc"], out["cnt"])
    assert refused(rc, "SLIMGPU_MatrixScoreCandidates", "the user ids must ascend strictly")
    assert out.untouched()


@gpu
def test_explain_judges_nwhy_then_the_users_then_the_set(t):
    out = Outputs(items=(3 * NU * 2, np.int32), terms=(3 * NU * 2, np.float32), support=(3 * NU, np.int32))
    call = lambda cs, nwhy: t.lib.SLIMGPU_MatrixExplainCandidates(  # noqa: E731
        t.model.handle, t.mat.handle, cs.handle, 2, P(DESC), nwhy, out["items"], out["terms"], out["support"])
    assert refused(call(t.cset, 0), "SLIMGPU_MatrixExplainCandidates", "nwhy must be between 1 and 16, not 0")
    assert refused(call(t.cset13, 2), "SLIMGPU_MatrixExplainCandidates", "the user ids must ascend strictly")
    assert out.untouched()


@gpu
def test_predict_lists_judges_its_arguments_then_the_users_then_the_filter(t):
    out = Outputs(ids=(2 * 4, np.int32), sc=(2 * 4, np.float32), cnt=(2, np.int32))
    rc = t.lib.SLIMGPU_MatrixPredictLists(0, t.model.handle, t.mat.handle, 2, P(DESC), out["ids"], out["sc"], out["cnt"])
    assert refused(rc, "SLIMGPU_MatrixPredictLists", "bad arguments (a resident model, a staged matrix, 1 <= nrcmds")
    rc = t.lib.SLIMGPU_MatrixPredictListsFiltered(4, t.model.handle, t.mat.handle, 2, P(DESC), t.filter13.handle,
                                                  out["ids"], out["sc"], out["cnt"])
    assert refused(rc, "SLIMGPU_MatrixPredictLists", "the user ids must ascend strictly")
    assert out.untouched()
    before = eval_stats(t.lib)
    rc = t.lib.SLIMGPU_MatrixPredictListsFiltered(4, t.model.handle, t.mat.handle, 2, P(I32(1, 3)), t.filter13.handle,
                                                  out["ids"], out["sc"], out["cnt"])
    assert refused(rc, "SLIMGPU_MatrixPredictLists", "13 items")      # (the loser, once it stands alone)
    assert out.untouched() and eval_stats(t.lib) == before


@gpu
def test_predict_exposure_judges_the_cutoffs_before_the_users(t):
    out = Outputs(E=(2 * NI, np.uint32))
    summ = (_lib.Exposure * 2)()
    rc = t.lib.SLIMGPU_MatrixPredictExposure(t.mat.handle, t.model.handle, 4, 2, P(DESC), None, P(t.fm), NI, 2,
                                             P(I32(3, 2)), out["E"], C.cast(summ, C.c_void_p))
    assert refused(rc, "SLIMGPU_MatrixPredictExposure", "the cutoffs must ascend strictly")
    assert out.untouched() and summ[0].lists == 0 and summ[1].slots == 0


@gpu
def test_evaluations_judge_their_counts_before_the_filter(t):
    ev, rk = t.evaluator(cutoffs=(5,)), t.evaluator(ranked=True)
    met, nv = np.full(8, 7.0), np.full(6, 7, np.int32)
    try:
        rc = t.lib.SLIMGPU_ModelEvaluateAtFiltered(ev.handle, t.model.handle, t.filter13.handle, 2, met, nv)
        assert refused(rc, "SLIMGPU_ModelEvaluateAtFiltered", "the eval set holds 1 list lengths, the call asks for 2")
        # an eval set without a list length: that wins over everything else, here a null model and the count
        rc = t.lib.SLIMGPU_ModelEvaluateExposure(rk.handle, None, t.filter13.handle, 1, met, nv, None, None)
        assert refused(rc, "SLIMGPU_ModelEvaluateExposure", "has no list length")
        rc = t.lib.SLIMGPU_ModelEvaluateRanked(rk.handle, None, 0, P(I32(5)), met, nv)
        assert refused(rc, "SLIMGPU_ModelEvaluateRanked", "between 1 and 32 cutoffs, not 0")
        # the filtered ranked calls name themselves in their refusals
        rc = t.lib.SLIMGPU_ModelEvaluateRankedFiltered(rk.handle, t.model.handle, t.filter13.handle, 1, P(I32(5)), met, nv)
        assert refused(rc, "SLIMGPU_ModelEvaluateRankedFiltered", "13 items")
        rc = t.lib.SLIMGPU_ModelRanksFiltered(rk.handle, t.model.handle, t.filter13.handle, None, None)
        assert refused(rc, "SLIMGPU_ModelRanksFiltered", "13 items")
        assert (met == 7.0).all() and (nv == 7).all()
    finally:
        ev.close()
        rk.close()


# ---- edges of the frame -----------------------------------------------------------------------------------------
@gpu
def test_the_last_row_alone_and_the_full_list_given_explicitly(t):
    ids, sc, cnt = t.model.predict(t.mat, nrcmds=5, return_counts=True)
    assert cnt.max() > 0
    one = t.model.predict(t.mat, nrcmds=5, users=[NU - 1], return_counts=True)
    st = eval_stats(t.lib)
    assert st["device_allocs"] >= 2 and st["d2h_bytes"] == 1 * (5 * 8 + 4) + 4
    for a, b in zip(one, (ids, sc, cnt)):
        assert a.tobytes() == b[NU - 1:].tobytes()
    full = t.model.predict(t.mat, nrcmds=5, users=np.arange(NU), return_counts=True)
    for a, b in zip(full, (ids, sc, cnt)):
        assert a.tobytes() == b.tobytes()
    # the same two edges through the candidate scorer, whose list upload is counted
    t.model.score_candidates(t.mat, t.cset)                         # (the set's device copy is made by its first call)
    slot = t.model.score_candidates(t.mat, t.cset)
    assert eval_stats(t.lib)["h2d_bytes"] == 0 and slot.any()
    last = t.model.score_candidates(t.mat, t.cset, users=[NU - 1])
    assert eval_stats(t.lib)["h2d_bytes"] == 4
    assert last[-3:].tobytes() == slot[-3:].tobytes() and not last[:-3].any()
    every = t.model.score_candidates(t.mat, t.cset, users=np.arange(NU))
    assert eval_stats(t.lib)["h2d_bytes"] == 4 * NU and every.tobytes() == slot.tobytes()


@gpu
def test_an_eval_set_without_a_position(t):
    """A test handle of 0 rows: nsel == 0.  Every evaluate call is SLIM_OK with zero figures, nothing runs."""
    T0 = sp.csr_matrix((0, NI), dtype=np.float32)
    ev = t.evaluator(T=T0, cutoffs=(3, 5))
    zero = lambda rows: all(r[k] == 0 for r in rows for k in r if k != "nrcmds" and k != "members")  # noqa: E731
    try:
        ev.set_groups(np.zeros(1, np.int32), 2)
        calls = (("at", lambda: ev.evaluate_at(t.model), (3, 5)),
                 ("exposure", lambda: ev.evaluate_exposure(t.model)[0], (3, 5)),
                 ("candidates", lambda: ev.evaluate_candidates(t.model, t.cset), (3, 5)),
                 ("ranked", lambda: ev.evaluate_ranked(t.model, (1, 4, 9)), (1, 4, 9)))
        for name, call, cut in calls:
            rows = call()
            st = ev.stats()
            print(name, rows, st)
            assert len(rows) == len(cut) and zero(rows), name
            down = 8 * (NI + 1) if name == "exposure" else 0     # (its first call fetches the matrix's column pointer)
            assert st["kernel_ms"] == 0 and st["d2h_bytes"] == down and st["w_rows_read"] == 0, name
            groups = ev.group_figures(cut)       # this call's rows (its own cutoff count), all zero
            assert len(groups) == 3 and all(zero(g) and len(g) == len(cut) for g in groups), name
        rk, _ = ev.ranks(t.model)
        assert rk.size == 0 and ev.stats()["kernel_ms"] == 0
    finally:
        ev.close()


@gpu
def test_three_slices_of_a_long_list_call(t, monkeypatch):
    """SLIM_TOPN_LONG_SLICE=3 on 7 users above 128 places: two full slices and a remainder of one."""
    N, cut = 130, I32(2, 130)
    monkeypatch.delenv("SLIM_TOPN_LONG_SLICE", raising=False)
    whole = t.model.predict(t.mat, nrcmds=N, return_counts=True)
    assert list_stats(t.lib)["slices"] == 1 and list_stats(t.lib)["path"] == 4
    monkeypatch.setenv("SLIM_TOPN_LONG_SLICE", "3")
    sliced = t.model.predict(t.mat, nrcmds=N, return_counts=True)
    ls, st = list_stats(t.lib), eval_stats(t.lib)
    assert ls["slices"] == 3 and ls["path"] == 4 and st["path"] == 4
    ids, _, cnt = sliced
    assert st["d2h_bytes"] == NU * (N * 8 + 4) + 40 + 4
    for a, b in zip(sliced, whole):
        assert a.tobytes() == b.tobytes()
    E, summ = t.model.exposure(t.mat, nrcmds=N, cutoffs=cut, fmarker=t.fm)
    assert list_stats(t.lib)["slices"] == 3 and list_stats(t.lib)["path"] == 4
    want = np.zeros((2, NI), np.uint32)
    for k, c in enumerate(cut):
        for q in range(NU):
            np.add.at(want[k], ids[q, :min(int(cnt[q]), int(c))], 1)
    assert np.array_equal(E, want) and [s["lists"] for s in summ] == [NU, NU]
    users = I32(0, 2, 3, 4, 6)       # a user list through the same loop: a slice of three, a remainder of two
    part = t.model.predict(t.mat, nrcmds=N, users=users, return_counts=True)
    assert list_stats(t.lib)["slices"] == 2
    for a, b in zip(part, whole):
        assert a.tobytes() == b[users].tobytes()


# ---- one invariant in one place ---------------------------------------------------------------------------------
@gpu
def test_every_evaluation_replaces_the_group_rows_and_ranks_leave_them(t):
    """With groups set, the rows on hand are those of the last figure-forming call, readable with its cutoff count
    only; SLIMGPU_ModelRanks between two of them leaves them as they are."""
    lib = t.lib
    ev = t.evaluator(cutoffs=(3, 5))
    groups = I32(0, 1, 0, 1, -1, 0, 1)
    met, nv = np.zeros(4 * 3 * 3), np.zeros(3 * 3 * 3, np.int32)

    def readable_with(n):
        for m in (1, 2, 3):
            rc = lib.SLIMGPU_EvalSetLastGroupFigures(ev.handle, m, P(met), P(nv))
            if m == n:
                assert rc == SLIM_OK, _lib.last_error()
            else:
                assert refused(rc, "SLIMGPU_EvalSetLastGroupFigures", "the last evaluation had %d cutoffs" % n)
    try:
        ev.set_groups(groups, 2)
        rc = lib.SLIMGPU_EvalSetLastGroupFigures(ev.handle, 2, P(met), P(nv))
        assert refused(rc, "SLIMGPU_EvalSetLastGroupFigures", "no evaluation has run since the groups were set")
        calls = ((lambda: ev.evaluate_at(t.model), (3, 5)),
                 (lambda: ev.evaluate_ranked(t.model, (1, 4, 9)), (1, 4, 9)),
                 (lambda: ev.evaluate_exposure(t.model)[0], (3, 5)),
                 (lambda: ev.evaluate_ranked(t.model, (7,)), (7,)),
                 (lambda: ev.evaluate_candidates(t.model, t.cset), (3, 5)),
                 (lambda: ev.evaluate_ranked(t.model, (2, 6, 12)), (2, 6, 12)))
        for call, cut in calls:
            own = call()
            readable_with(len(cut))
            rows = ev.group_figures(cut)
            assert [r["members"] for r in rows[2]] == [NU] * len(cut)
            for a, b in zip(rows[2], own):      # everybody's row is the call's own output
                assert all(a[k] == b[k] for k in b)
            assert all(sum(rows[g][k]["nvalid"] for g in (0, 1)) <= own[k]["nvalid"] for k in range(len(cut)))
            rk, _ = ev.ranks(t.model)           # no figures: the rows stay, bit for bit
            assert rk.size == NU
            readable_with(len(cut))
            again = ev.group_figures(cut)
            assert again == rows
    finally:
        ev.close()
