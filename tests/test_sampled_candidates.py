"""Sampled negatives on the device (include/slim_gpu_sample.h): SLIMGPU_EvalSetSampleCandidates.

The yardstick is never the code under test: the rows are those of the numpy restatement of the header's text
(tests/sampled_cases.py); the expected figures and scores are those of the EXISTING calls on numpy's rows --
SLIMGPU_CandSetCreate + SLIMGPU_ModelEvaluateCandidates, and candidate_cases.yardstick (Py_SLIM_GetTopN_1vsk).
Everything is compared bit for bit.
"""
import ctypes as C
import re

import numpy as np
import pytest
import scipy.sparse as sp

from candidate_cases import P, buffers, check_slot_scores, yardstick
from filtered_cases import cases_fixture, wrap
from sampled_cases import (DENSE, GRID, GRID_L1, GRID_L2, PAIR, check_grid_lines, csr, grid_by_hand, held_out_rows,
                           host_sample, sampled_rows, set_rows)
from slim_amd import _lib
from slim_amd.constants import SLIM_ERROR_INPUT, SLIM_OK, SLIMGPU_MAX_LIST
from slim_amd.engine import CandidateSet, DeviceMatrix, eval_stats

pytestmark = pytest.mark.gpu
cases = pytest.fixture(scope="module")(cases_fixture)
EVERY = pytest.mark.parametrize("name", ["floats", "ties", "wide"])
CUTOFFS = (1, 5, 10, 64)


def device_sample(lib, ev, nnegs, seed):
    h = C.c_void_p()
    return lib.SLIMGPU_EvalSetSampleCandidates(ev.handle, nnegs, seed, C.byref(h)), h


@EVERY
def test_device_rows_equal_the_host_call_and_the_restatement(cases, name):
    c = cases(name)
    T = held_out_rows(c, seed=91)
    tptr, tind = T.indptr.astype(np.int64), T.indices
    fm = np.zeros(c.ncols, np.int32)
    ht = wrap(c.lib, T)
    grid = GRID + (DENSE if c.ncols == 1500 else ())
    try:
        for users in (None, np.arange(0, c.nusers, 3, dtype=np.int32)):
            for ranked in (False, True):
                ev = c.mat.evaluator(T, fmarker=fm, cutoffs=CUTOFFS, users=users, ranked=ranked)
                try:
                    for nnegs in (grid if not ranked else (65,)):
                        want = sampled_rows(c.R, tptr, tind, c.ncols, nnegs, seed=5, users=users)
                        rc, cs = device_sample(c.lib, ev, nnegs, 5)
                        assert rc == SLIM_OK, _lib.last_error()
                        got = set_rows(c.lib, cs)
                        c.lib.SLIMGPU_CandSetFree(cs)
                        rc, hs = host_sample(c.lib, c.ncols, c.hr, ht, nnegs, 5, users=users)
                        assert rc == SLIM_OK, _lib.last_error()
                        host = set_rows(c.lib, hs)
                        c.lib.SLIMGPU_CandSetFree(hs)
                        assert got[2] == host[2] == c.ncols
                        for k in (0, 1):
                            assert np.array_equal(got[k], want[k]), (name, nnegs, users is None, "numpy", k)
                            assert np.array_equal(got[k], host[k]), (name, nnegs, users is None, "host", k)
                finally:
                    ev.close()
    finally:
        c.lib.Py_csr_free(ht)


def hand_made():
    """The 40-item matrix of tests/test_sampled_candidates_host.py: free = 0, free = nnegs - 1, the last sparse user,
    the first dense one, no test row, an empty history with a repeated and an outside test id."""
    hist = [list(range(39)) + [39], list(range(0, 35)), list(range(10, 24)), list(range(10, 25)), [1, 2, 3], []]
    test = [[39], [35, 3], [30], [30], [], [7, 7, 44]]
    return csr(hist, 40), csr(test, 45)


def test_the_hand_made_matrix_on_the_device():
    lib = _lib.load()
    R, T = hand_made()
    mat = DeviceMatrix.from_scipy(R, binary=True)
    try:
        assert mat.ncols == 40
        ev = mat.evaluator(T, fmarker=np.zeros(45, np.int32), cutoffs=(3,))
        for seed in (1, 2, 2 ** 63 + 11):
            want = sampled_rows(R, T.indptr.astype(np.int64), T.indices, 40, 5, seed)
            rc, cs = device_sample(lib, ev, 5, seed)
            assert rc == SLIM_OK, _lib.last_error()
            got = set_rows(lib, cs)
            lib.SLIMGPU_CandSetFree(cs)
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), seed
        assert np.diff(want[0]).tolist() == [1, 6, 6, 6, 0, 8]
        ev.close()
    finally:
        mat.close()


@EVERY
def test_figures_scores_and_the_eval_set_guarantee(cases, name):
    c = cases(name)
    T = held_out_rows(c, seed=91)
    tptr, tind = T.indptr.astype(np.int64), T.indices
    fm = np.random.default_rng(3).integers(0, 2, c.ncols).astype(np.int32)
    for users in (None, np.arange(0, c.nusers, 3, dtype=np.int32)):
        ev = c.mat.evaluator(T, fmarker=fm, cutoffs=CUTOFFS, users=users)
        want_rows = sampled_rows(c.R, tptr, tind, c.ncols, 99, seed=7, users=users)
        born = ev.sample_candidates(99, seed=7)
        made = c.mat.candidate_set(want_rows)
        try:
            assert isinstance(born, CandidateSet) and born.size == want_rows[1].size
            assert np.array_equal(born.indptr, want_rows[0])
            got = ev.evaluate_candidates(c.model, born)
            again = ev.evaluate_candidates(c.model, born)
            st = ev.stats()
            want = ev.evaluate_candidates(c.model, made)
            print(name, "sampled", [(r["nrcmds"], r["hr"], r["arhr"], r["nvalid"]) for r in got], "second call", st)
            assert got == want == again                     # every returned double and count
            assert st["path"] == 5 and st["device_allocs"] == 0 and st["h2d_bytes"] == 0
            assert st["d2h_bytes"] <= 8 + 32 * len(CUTOFFS)
            assert got[-1]["nvalid"] > 0 and 0 < got[-1]["hr"] <= 1
            full = ev.evaluate_at(c.model)
            assert [r["nvalid"] for r in full] == [r["nvalid"] for r in got]
            # the slot scores of the device-born rows against the existing host call's order
            sel = range(c.nusers) if users is None else users
            order = yardstick(c, want_rows[0], want_rows[1])
            bufs = buffers(want_rows[0], len(sel), 0)
            u = None if users is None else np.ascontiguousarray(users, np.int32)
            rc = c.lib.SLIMGPU_MatrixScoreCandidates(c.model.handle, c.mat.handle, born.handle,
                                                     0 if u is None else u.size, P(u), 0, P(bufs[0]), None, None, None)
            assert rc == SLIM_OK, _lib.last_error()
            check_slot_scores(bufs[0], want_rows[0], want_rows[1], order, sel, c.nusers)
            ptr, ind = born.rows()                          # the ids come down when asked
            assert np.array_equal(ptr, want_rows[0]) and np.array_equal(ind, want_rows[1])
        finally:
            born.close()
            made.close()
            ev.close()


def test_device_refusals_leave_out_untouched(cases):
    c = cases("floats")
    T = held_out_rows(c, seed=91)
    ev = c.mat.evaluator(T, fmarker=np.zeros(c.ncols, np.int32), cutoffs=(10,))
    SENTINEL = 0x5A5A
    try:
        for nnegs, word in ((0, "nnegs"), (-3, "nnegs"), (SLIMGPU_MAX_LIST - 2, str(SLIMGPU_MAX_LIST))):
            h = C.c_void_p(SENTINEL)
            rc = c.lib.SLIMGPU_EvalSetSampleCandidates(ev.handle, nnegs, 1, C.byref(h))
            assert rc == SLIM_ERROR_INPUT and h.value == SENTINEL
            assert "SLIMGPU_EvalSetSampleCandidates" in _lib.last_error() and word in _lib.last_error()
        assert c.lib.SLIMGPU_EvalSetSampleCandidates(ev.handle, 99, 1, None) == SLIM_ERROR_INPUT
        h = C.c_void_p(SENTINEL)
        assert c.lib.SLIMGPU_EvalSetSampleCandidates(None, 99, 1, C.byref(h)) == SLIM_ERROR_INPUT
        assert h.value == SENTINEL
    finally:
        ev.close()
    # a catalogue beyond the LDS bitmap: the limit is in the message
    wide = 524288 + 1
    R = sp.csr_matrix((np.ones(3, np.float32), np.array([0, 5, wide - 1], np.int32), np.array([0, 2, 3], np.int32)),
                      shape=(2, wide))
    Tw = sp.csr_matrix((np.ones(2, np.float32), np.array([7, 9], np.int32), np.array([0, 1, 2], np.int32)),
                       shape=(2, wide))
    mat = DeviceMatrix.from_scipy(R, binary=True)
    try:
        ev = mat.evaluator(Tw, fmarker=np.zeros(wide, np.int32), cutoffs=(10,))
        h = C.c_void_p(SENTINEL)
        rc = c.lib.SLIMGPU_EvalSetSampleCandidates(ev.handle, 99, 1, C.byref(h))
        assert rc == SLIM_ERROR_INPUT and h.value == SENTINEL and "524288" in _lib.last_error(), _lib.last_error()
        ev.close()
    finally:
        mat.close()


# ---- the grid --------------------------------------------------------------------------------------------------------
PARAMS = {"dbglvl": 0, "algo": "cd", "nthreads": 1, "optTol": 1e-7, "niters": 200}


def mselect(R, T, capfd, nrcmds=10, params=None, **kw):
    from slim_amd import SLIM, SLIMatrix
    trainmat = SLIMatrix(R)
    valmat = SLIMatrix(T, trainmat)
    model = SLIM()
    C.CDLL(None).fflush(None)
    capfd.readouterr()
    try:
        model.mselect(dict(PARAMS, **(params or {})), trainmat, valmat, GRID_L1, GRID_L2, nrcmds=nrcmds, **kw)
        err = None
    except RuntimeError as e:
        err = str(e)
    C.CDLL(None).fflush(None)
    return model, capfd.readouterr().out, err


def test_the_grid_on_sampled_negatives(automotive, monkeypatch, capfd):
    R, T = sp.csr_matrix(automotive[0]), sp.csr_matrix(automotive[1])
    nu = R.shape[0]
    monkeypatch.setenv("SLIM_GPU_NO_CARRY", "1")       # a pair's model does not depend on who solved before
    monkeypatch.setenv("SLIM_GPU_RESIDENT", "1")
    monkeypatch.setenv("SLIM_GPU_EVAL_RESIDENT", "1")
    got, entries = grid_by_hand(R, T, 99, seed=1)
    model, out, err = mselect(R, T, capfd, params={"gpu_evalnegs": 99})         # slot 23 = 99, slot 24 unset: seed 1
    assert err is None, err
    assert "  sampled negatives: nnegs 99, seed 1, %d candidate entries\n" % entries in out
    lines = re.findall(PAIR, out)
    check_grid_lines(lines, got, model.mselect_result)
    assert eval_stats()["path"] == 5
    # the unsampled grid prints other figures: the option was not ignored
    _, plain, err = mselect(R, T, capfd)
    assert err is None and "sampled negatives" not in plain
    assert len(re.findall(PAIR, plain)) == 4 and re.findall(PAIR, plain) != lines
    assert all(g["hr"] != full["hr"] and g["nvalid"] == full["nvalid"] for _, _, g, full in got)
    # another seed through the keyword arguments
    got7, _ = grid_by_hand(R, T, 99, seed=7)
    model, out, err = mselect(R, T, capfd, nnegs=99, negseed=7)
    assert err is None and "nnegs 99, seed 7," in out
    check_grid_lines(re.findall(PAIR, out), got7, model.mselect_result)
    assert [g for _, _, g, _ in got7] != [g for _, _, g, _ in got]
    # with EVALSTRIDE = 3: the negatives of user u are those of the whole set, the users are every third
    S = np.arange(0, nu, 3)
    got3, entries3 = grid_by_hand(R, T, 99, seed=1, users=S)
    model, out, err = mselect(R, T, capfd, params={"gpu_evalnegs": 99, "gpu_evalstride": 3})
    assert err is None, err
    assert "  evaluating every 3-th user: %d of %d\n" % (S.size, nu) in out
    assert "  sampled negatives: nnegs 99, seed 1, %d candidate entries\n" % entries3 in out and entries3 < entries
    check_grid_lines(re.findall(PAIR, out), got3, model.mselect_result)


def test_the_grid_refuses_what_it_cannot_sample(automotive, monkeypatch, capfd):
    """Each is SLIM_ERROR_INPUT with a text that says which, before any solve line is printed."""
    R, T = sp.csr_matrix(automotive[0]), sp.csr_matrix(automotive[1])
    monkeypatch.setenv("SLIM_GPU_RESIDENT", "1")
    monkeypatch.setenv("SLIM_GPU_EVAL_RESIDENT", "1")

    def refused(word, env=None, **kw):
        for k, v in (env or {}).items():
            monkeypatch.setenv(k, v)
        _, out, err = mselect(R, T, capfd, **kw)
        for k in env or {}:
            monkeypatch.setenv(k, "1")
        assert err is not None and "EVALNEGS" in err and word in err, (word, err)
        assert "l1r:" not in out and "Estimating" not in out, out
    refused("filter", nnegs=99, blocked_items=[0, 1, 2])
    refused("nrcmds is 129", nnegs=99, nrcmds=129)
    refused("ADMM", nnegs=99, params={"algo": "admm"})
    refused("several GPUs", nnegs=99, env={"SLIM_GPU_NGPUS": "2"})
    refused("SLIM_GPU_RESIDENT=0", nnegs=99, env={"SLIM_GPU_RESIDENT": "0"})
    refused("SLIM_GPU_EVAL_RESIDENT=0", nnegs=99, env={"SLIM_GPU_EVAL_RESIDENT": "0"})
    refused(str(SLIMGPU_MAX_LIST), nnegs=SLIMGPU_MAX_LIST)
    refused("at least 0", params={"gpu_evalnegs": -2})
    # the status itself
    from slim_amd import SLIMatrix
    from slim_amd.interface import build_options, check_params
    params = dict(PARAMS, gpu_evalnegs=99)
    check_params(params)
    params["nrcmds"] = 200
    iopt, dopt = build_options(params)
    assert iopt[23] == 99 and iopt[24] == -1
    trainmat = SLIMatrix(R)
    valmat = SLIMatrix(T, trainmat)
    best = [C.c_double(0.0) for _ in range(8)]
    rc = _lib.load().Py_SLIM_Mselect(trainmat.handle, valmat.handle, iopt, dopt, np.array(GRID_L1), np.array(GRID_L2),
                                     2, 2, *[C.byref(b) for b in best])
    assert rc == SLIM_ERROR_INPUT and "nrcmds is 200" in _lib.last_error()
