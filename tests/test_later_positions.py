"""The second and later positions of a workgroup in the per-user kernels: the samplers k_sample_negatives and
k_sample_weighted (their LDS bitmap is cleared by un-marking what a user marked), k_explain (the staged history records
are replaced behind a barrier) and every mode of the top-N scorer (merge areas, the long form's slab).

Each of them launches min(positions, CUs x workgroups per CU) workgroups, so a fixture of a few hundred users gives
every workgroup one position and never takes the way round.  The crowd fixtures of tests/crowd_cases.py are tiny in
items and large in users; every GPU test here reads the launch's SLIM_GPU_TRACE line and ASSERTS positions >
2 x workgroups -- on a device with more CUs it fails and says to enlarge the fixture, it never passes without testing
what it is for.

The yardsticks are those of the existing test files, never the code under test; everything is compared bit for bit.
"""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp

import crowd_cases as Cc
import weighted_cases as Wc
from candidate_cases import P, check_slot_scores, make_set
from explain_cases import buffers as why_buffers, check as check_why
from filtered_cases import Case, assert_same, evaluate_lists, figures, positions, same, wrap
from sampled_cases import host_sample, set_rows
from slim_amd import _lib
from slim_amd.constants import SLIM_OK

gpu = pytest.mark.gpu


# ---- fixtures, made once per module ----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def crowd():
    return Cc.SamplerCrowd()


@pytest.fixture(scope="module")
def why():
    c = Cc.ExplainCrowd(_lib.load())
    yield c
    c.close()


@pytest.fixture(scope="module")
def scorers():
    made = {}

    def get(name):
        if name not in made:
            made[name] = Cc.ScorerCrowd(Case(_lib.load(), "crowd-" + name))
        return made[name]
    yield get
    for s in made.values():
        s.c.close()


@pytest.fixture(scope="module")
def sampler_device(crowd):
    from slim_amd.engine import DeviceMatrix
    lib = _lib.load()
    mat = DeviceMatrix.from_scipy(crowd.R, binary=True)
    hr, ht = wrap(lib, crowd.R, binary=True), wrap(lib, crowd.T)
    yield lib, mat, hr, ht
    lib.Py_csr_free(hr)
    lib.Py_csr_free(ht)
    mat.close()


# ---- on the CPU: the helpers and the fixtures ------------------------------------------------------------------------
def test_mulhi64_in_halves_equals_python_integers():
    rng = np.random.default_rng(401)
    edges = np.array([0, 1, 2 ** 64 - 1, 2 ** 32 - 1, 2 ** 32, 2 ** 63], np.uint64)
    keys = np.concatenate((edges, rng.integers(0, 2 ** 64, 4000, dtype=np.uint64, endpoint=False)))
    for m in edges.tolist() + [50 * 4_000_000_000 + 400, 1_350_000] + rng.integers(0, 2 ** 64, 20, dtype=np.uint64).tolist():
        got = Wc.mulhi64(keys, m)
        assert got.dtype == np.uint64 and np.array_equal(got, Wc.mulhi64_python(keys, m)), m


def test_fixtures_do_their_job(crowd, why, scorers):
    # the samplers: the rules are where they are claimed to be
    E = np.array([crowd.X(u).size for u in range(crowd.nusers)])
    assert sorted(set(E.tolist())) == [1, 150, 151] and (E == 1).sum() == len(Cc.EMPTY)
    assert all(2 * (e + Cc.SPARSE) <= Cc.NITEMS for e in (1, 151))           # every user sparse
    assert all(2 * (e + Cc.DENSE) > Cc.NITEMS for e in (1, 151))             # every user dense
    assert sum(Cc.no_test_row(u) for u in range(crowd.nusers)) == crowd.nusers // 10
    assert crowd.subset.size > 2 * 4096 and (crowd.subset != np.arange(crowd.subset.size)).all()
    assert (np.diff(crowd.subset) > 0).all()
    for rule, nnegs in Cc.RULES:
        ptr, _ = crowd.rows(rule, nnegs)
        lens = np.diff(ptr)
        served = np.array([not Cc.no_test_row(u) for u in range(crowd.nusers)])
        assert (lens[~served] == 0).all() and (lens[served] == nnegs + 1).all(), rule      # full rows, empty rows
        for G in (1024, 2048, 4096):
            share, n = crowd.stale_share(rule, nnegs, G, stride=4)
            print("stale bits of the previous position would change %.1f %% of %d later rows: %s, nnegs %d, "
                  "%d workgroups" % (100 * share, n, rule, nnegs, G))
            assert share >= 0.9, (rule, G, share)
    # the cliff weights send later users to phase 2 as well, the popularity weights hardly anyone
    picks = np.array([Wc._ROWS[(("crowd", "cliff"), 45, Cc.SEED, u)][2] for u in range(4096, crowd.nusers)
                      if not Cc.no_test_row(u)])
    print("cliff: phase 2 picks of the users from 4096 on: min %d, mean %.1f" % (picks.min(), picks.mean()))
    assert (picks > 0).mean() > 0.99
    # the explanations: histories on both sides of the staging cap, empty ones, rows with every kind of entry
    hl = np.diff(why.hptr)
    assert (hl == 0).sum() >= 4 and (hl < Cc.STAGE).sum() > 1000 and (hl > Cc.STAGE).sum() > 1000
    assert all((hl == n).any() for n in (Cc.STAGE - 1, Cc.STAGE, Cc.STAGE + 1))
    assert why.nusers > 2 * 2048 and set(np.diff(why.indptr).tolist()) == set(range(8, 13))
    for u in (0, 2048, 4999):
        row = why.indices[why.indptr[u]:why.indptr[u + 1]]
        assert -1 in row and why.ncols in row and np.unique(row).size == row.size - 1
    support = np.array([t.size for slots in why.want.values() for _, _, t in slots])
    print("explanations: %d slots, support 0 in %d, above 3 in %d, above 6 in %d"
          % (support.size, (support == 0).sum(), (support > 3).sum(), (support > 6).sum()))
    assert (support == 0).sum() > 1000 and (support > 3).sum() > 100 and (support > 6).sum() > 10
    # the scorer modes: more than two positions per workgroup of 4 x 256, lists shorter and longer than 192
    for name in ("floats", "ties"):
        s = scorers(name)
        c = s.c
        assert c.nusers > 2 * 1024 and s.subset.size > 2 * 1024 and (s.subset != np.arange(s.subset.size)).all()
        assert (c.ncand < 192).any() and (c.ncand > 192).any() and (c.ncand == 0).sum() == 2
        moved = (s.flt[0][:, 0] != c.ids[:, 0]).sum()
        print(name, "candidates per user %d-%d, the filter changes the head of %d lists" % (c.ncand.min(), c.ncand.max(), moved))
        assert moved > c.nusers // 4 and np.diff(s.T.indptr).max() == 4 and (np.diff(s.T.indptr) == 0).sum() > 400


# ---- 1. the samplers -------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("rule,nnegs", Cc.RULES)
def test_sampled_rows_of_later_positions(crowd, sampler_device, rule, nnegs, monkeypatch, capfd):
    lib, mat, hr, ht = sampler_device
    monkeypatch.setenv("SLIM_GPU_TRACE", "1")
    weighted = rule in ("counts", "cliff")
    kernel = "k_sample_weighted" if weighted else "k_sample_negatives"
    fm = np.zeros(crowd.ncols, np.int32)
    assert mat.ncols == crowd.ncols
    for users in (None, crowd.subset):
        want = crowd.rows(rule, nnegs, users=users)
        ev = mat.evaluator(crowd.T, fmarker=fm, cutoffs=(10,), users=users)
        try:
            def call():
                if weighted:    # (the popularity weights are the resident matrix's own: NULL)
                    return Wc.device_sample_weighted(lib, ev, nnegs, Cc.SEED, None if rule == "counts" else crowd.w[rule])
                h = C.c_void_p()
                return lib.SLIMGPU_EvalSetSampleCandidates(ev.handle, nnegs, Cc.SEED, C.byref(h)), h
            (rc, cs), launches = Cc.trace_launches(capfd, call)
            assert rc == SLIM_OK, _lib.last_error()
            got = set_rows(lib, cs)
            lib.SLIMGPU_CandSetFree(cs)
        finally:
            ev.close()
        npos, G, rest = Cc.went_round(launches, kernel)
        assert npos == (crowd.nusers if users is None else users.size)
        # the fixture can see stale bits, from the restatement alone
        print("%s, nnegs %d: %d positions, %d workgroups%s" % (kernel, nnegs, npos, G, rest))
        if users is None:
            share, n = crowd.stale_share(rule, nnegs, G)
            print("stale bits would change %.1f %% of the %d later rows" % (100 * share, n))
            assert share >= 0.9
        if weighted:
            rc, hs = Wc.host_sample_weighted(lib, crowd.ncols, hr, ht, nnegs, Cc.SEED, crowd.w[rule], users=users)
        else:
            rc, hs = host_sample(lib, crowd.ncols, hr, ht, nnegs, Cc.SEED, users=users)
        assert rc == SLIM_OK, _lib.last_error()
        host = set_rows(lib, hs)
        lib.SLIMGPU_CandSetFree(hs)
        assert got[2] == host[2] == crowd.ncols
        for k in (0, 1):
            assert np.array_equal(got[k], want[k]), (rule, nnegs, users is None, "numpy", k, first_wrong(got, want, G))
            assert np.array_equal(host[k], want[k]), (rule, nnegs, users is None, "host", k)


def first_wrong(got, want, G):
    """The first user whose row differs, for the message: (user, user % workgroups, got row, wanted row)."""
    if not np.array_equal(got[0], want[0]):
        u = int(np.argmax(got[0] != want[0])) - 1
    else:
        u = int(np.searchsorted(want[0], int(np.argmax(got[1] != want[1])), "right")) - 1
    return u, u % G, got[1][got[0][u]:got[0][u + 1]].tolist(), want[1][want[0][u]:want[0][u + 1]].tolist()


# ---- 2. the explanations ---------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("nwhy,form", [(3, 4), (6, 16)])
def test_explanations_of_later_positions(why, nwhy, form, monkeypatch, capfd):
    c = why
    monkeypatch.setenv("SLIM_GPU_TRACE", "1")
    monkeypatch.setenv("SLIM_EXPLAIN_STAGE", str(Cc.STAGE))
    rc, cs = make_set(c.lib, c.ncols, c.indptr, c.indices)
    assert rc == SLIM_OK, _lib.last_error()
    kernel = "k_explain<%d>" % form
    many = np.array([u for u in range(c.nusers) if u % 11 != 0], np.int32)
    lists = [None, many] + [np.arange(2, 2 + 3 * n, 3, dtype=np.int32) for n in (255, 256, 257)]
    try:
        for users in lists:
            bufs = why_buffers(c.indptr, nwhy)
            u = None if users is None else np.ascontiguousarray(users, np.int32)

            def call():
                return c.lib.SLIMGPU_MatrixExplainCandidates(c.model.handle, c.mat.handle, cs, 0 if u is None else u.size,
                                                             P(u), nwhy, *[P(b) for b in bufs])
            rc, launches = Cc.trace_launches(capfd, call)
            assert rc == SLIM_OK, _lib.last_error()
            if users is None or users.size > 300:
                npos, G, rest = Cc.went_round(launches, kernel)
                print("%s: %d positions, %d workgroups%s" % (kernel, npos, G, rest))
                assert "%d staged entries" % Cc.STAGE in rest
            check_why(bufs, c.indptr, c.want, range(c.nusers) if users is None else users, c.nusers, nwhy)
        # the host handles go through the same kernel
        bufs = why_buffers(c.indptr, nwhy)
        rc, launches = Cc.trace_launches(
            capfd, lambda: c.lib.SLIMGPU_ExplainCandidates(c.hw, c.hr, cs, nwhy, *[P(b) for b in bufs]))
        assert rc == SLIM_OK, _lib.last_error()
        Cc.went_round(launches, kernel)
        check_why(bufs, c.indptr, c.want, range(c.nusers), c.nusers, nwhy)
    finally:
        c.lib.SLIMGPU_CandSetFree(cs)


# ---- 3. the scorer modes ---------------------------------------------------------------------------------------------
BOTH = pytest.mark.parametrize("name", ["floats", "ties"])
SETS = pytest.mark.parametrize("filtered", [False, True], ids=["plain", "filtered"])


def round_of(launches, mode, npos):
    got = Cc.went_round(launches, "top-N scorer (%s)" % mode, npos)
    print("top-N scorer (%s): %d positions, %d workgroups%s" % ((mode,) + got))
    return got


def users_of(s, subset):
    return (s.subset, s.subset) if subset else (None, np.arange(s.c.nusers))


@gpu
@BOTH
@SETS
def test_figures_of_later_positions(scorers, name, filtered, monkeypatch, capfd):
    """SLIMGPU_ModelEvaluateAt(Filtered): the chunk scorer's eval mode at (1, 10, 64), the wave kernel at (10, 100)."""
    s = scorers(name)
    c = s.c
    monkeypatch.setenv("SLIM_GPU_TRACE", "1")
    flt = s.item_filter() if filtered else None
    ids = s.lists(filtered)[0]
    try:
        for subset in (False, True):
            users, sel = users_of(s, subset)
            TS = sp.csr_matrix(s.T)[sel]
            for mode, cutoffs, path in (("eval", (1, 10, 64), 1), ("wave", (10, 100), 2)):
                ev = c.mat.evaluator(s.T, fmarker=s.fm, cutoffs=cutoffs, users=users)
                rows, launches = Cc.trace_launches(capfd, lambda: ev.evaluate_at(c.model, filter=flt))
                st = ev.stats()
                ev.close()
                assert st["path"] == path
                round_of(launches, mode, sel.size)
                for row, n in zip(rows, cutoffs):
                    assert_same(figures(row), evaluate_lists(c.lib, ids[sel], n, TS, s.fm), "%s %s @%d" % (name, mode, n))
    finally:
        if flt is not None:
            flt.close()


@gpu
@BOTH
@SETS
def test_ranks_of_later_positions(scorers, name, filtered, monkeypatch, capfd):
    """SLIMGPU_ModelRanks(Filtered) and SLIMGPU_ModelEvaluateRanked(Filtered): the chunk scorer's rank mode."""
    s = scorers(name)
    c = s.c
    monkeypatch.setenv("SLIM_GPU_TRACE", "1")
    flt = s.item_filter() if filtered else None
    ids, sc = s.lists(filtered)
    cuts = (1, 10, 200, c.ncols)
    try:
        for subset in (False, True):
            users, sel = users_of(s, subset)
            TS = sp.csr_matrix(s.T)[sel]
            ev = c.mat.evaluator(s.T, fmarker=s.fm, ranked=True, users=users)
            (ranks, indptr, scores), launches = Cc.trace_launches(
                capfd, lambda: ev.ranks(c.model, scores=True, filter=flt))
            round_of(launches, "rank", sel.size)
            rows, launches = Cc.trace_launches(capfd, lambda: ev.evaluate_ranked(c.model, cuts, filter=flt))
            round_of(launches, "rank", sel.size)
            ev.close()
            want = positions(ids[sel], sc[sel], s.T, sel)
            assert np.array_equal(np.diff(indptr), np.diff(s.T.indptr)[sel])
            assert np.array_equal(ranks, want[0]) and np.array_equal(scores.view(np.uint32), want[1].view(np.uint32))
            for row, n in zip(rows, cuts):
                assert_same(figures(row), evaluate_lists(c.lib, ids[sel], n, TS, s.fm), "%s ranked @%d" % (name, n))
    finally:
        if flt is not None:
            flt.close()


@gpu
@BOTH
def test_candidate_rows_of_later_positions(scorers, name, monkeypatch, capfd):
    """SLIMGPU_MatrixScoreCandidates and SLIMGPU_ModelEvaluateCandidates: the chunk scorer's cand mode."""
    s = scorers(name)
    c = s.c
    monkeypatch.setenv("SLIM_GPU_TRACE", "1")
    cutoffs = (1, 5, 10)
    cset = c.mat.candidate_set((s.cptr, s.cind))
    try:
        for subset in (False, True):
            users, sel = users_of(s, subset)
            slot = np.full(s.cind.size, np.float32(-3.5), np.float32)
            rc, launches = Cc.trace_launches(capfd, lambda: c.lib.SLIMGPU_MatrixScoreCandidates(
                c.model.handle, c.mat.handle, cset.handle, 0 if users is None else users.size, P(users), 0, P(slot),
                None, None, None))
            assert rc == SLIM_OK, _lib.last_error()
            round_of(launches, "cand", sel.size)
            check_slot_scores(slot, s.cptr, s.cind, s.corder, sel, c.nusers)
            ev = c.mat.evaluator(s.T, fmarker=s.fm, cutoffs=cutoffs, users=users)
            rows, launches = Cc.trace_launches(capfd, lambda: ev.evaluate_candidates(c.model, cset))
            ev.close()
            round_of(launches, "cand", sel.size)
            TS = sp.csr_matrix(s.T)[sel]
            for row, n in zip(rows, cutoffs):
                # (as tests/test_candidates.py: the first n of the row's order, dead entries among them)
                lists, cnt = np.full((sel.size, n), -1, np.int32), np.zeros(sel.size, np.int32)
                for q, u in enumerate(sel):
                    cnt[q] = min(n, s.corder[u][0].size)
                    lists[q, :cnt[q]] = s.corder[u][0][:cnt[q]]
                ht = wrap(c.lib, TS)
                met, nv = np.zeros(4), np.zeros(3, np.int32)
                assert c.lib.SLIMGPU_Evaluate(sel.size, n, lists.ravel(), cnt, ht, s.fm, s.fm.size, met, nv) == SLIM_OK
                c.lib.Py_csr_free(ht)
                assert_same(figures(row), (met, nv), "%s candidates @%d" % (name, n))
    finally:
        cset.close()


@gpu
@BOTH
@SETS
def test_lists_of_later_positions(scorers, name, filtered, monkeypatch, capfd):
    """SLIMGPU_MatrixPredictLists(Filtered): the chunk kernel at 10, the long form at 192 (its slab of scores is a
    workgroup's, carried from user to user) and the wave kernel at 100 under SLIM_TOPN_KERNEL=wave."""
    s = scorers(name)
    c = s.c
    monkeypatch.setenv("SLIM_GPU_TRACE", "1")
    flt = s.item_filter() if filtered else None
    try:
        for subset in (False, True):
            users, sel = users_of(s, subset)
            for mode, n, pin in (("chunk", 10, None), ("long", 192, None), ("wave", 100, "wave")):
                if pin:
                    monkeypatch.setenv("SLIM_TOPN_KERNEL", pin)
                else:
                    monkeypatch.delenv("SLIM_TOPN_KERNEL", raising=False)
                got, launches = Cc.trace_launches(
                    capfd, lambda: c.model.predict(c.mat, nrcmds=n, users=users, return_counts=True, filter=flt))
                round_of(launches, mode, sel.size)
                want = c.expected(n, s.allowed if filtered else None, s.X if filtered else None, sel)
                assert same(got, want), (name, mode, n, subset)
    finally:
        monkeypatch.delenv("SLIM_TOPN_KERNEL", raising=False)
        if flt is not None:
            flt.close()
