"""Popularity-weighted negatives on the device (THE WEIGHTED RULE of include/slim_gpu_sample.h):
SLIMGPU_EvalSetSampleCandidatesWeighted.

The yardstick is never the code under test: the rows are those of the numpy restatement of the header's text
(tests/weighted_cases.py); the expected figures are those of the EXISTING calls on numpy's rows --
SLIMGPU_CandSetCreate + SLIMGPU_ModelEvaluateCandidates.  Everything is compared bit for bit.
"""
import ctypes as C
import re

import numpy as np
import pytest
import scipy.sparse as sp

from filtered_cases import cases_fixture, wrap
from sampled_cases import GRID_L1, GRID_L2, PAIR, check_grid_lines, held_out_rows, sampled_rows, set_rows
from slim_amd import _lib
from slim_amd.constants import SLIM_ERROR_INPUT, SLIM_OK
from slim_amd.engine import CandidateSet, DeviceMatrix, eval_stats
from weighted_cases import (device_sample_weighted, grid, grid_by_hand_popularity, hand_made, host_sample_weighted,
                            weighted_rows, weights)

pytestmark = pytest.mark.gpu
cases = pytest.fixture(scope="module")(cases_fixture)
EVERY = pytest.mark.parametrize("name", ["floats", "ties", "wide"])
CUTOFFS = (1, 5, 10, 64)


@EVERY
def test_device_rows_equal_the_host_call_and_the_restatement(cases, name):
    c = cases(name)
    T = held_out_rows(c, seed=91)
    tptr, tind = T.indptr.astype(np.int64), T.indices
    fm = np.zeros(c.ncols, np.int32)
    ht = wrap(c.lib, T)
    try:
        for users in (None, np.arange(0, c.nusers, 3, dtype=np.int32)):
            for ranked in (False, True):
                ev = c.mat.evaluator(T, fmarker=fm, cutoffs=CUTOFFS, users=users, ranked=ranked)
                try:
                    for wname, nnegs in grid(c.ncols):
                        w = weights(wname, c.R, c.ncols)
                        want = weighted_rows((name, wname), c.R, tptr, tind, c.ncols, nnegs, 5, w, users=users)
                        rc, cs = device_sample_weighted(c.lib, ev, nnegs, 5, w)
                        assert rc == SLIM_OK, _lib.last_error()
                        got = set_rows(c.lib, cs)
                        c.lib.SLIMGPU_CandSetFree(cs)
                        rc, hs = host_sample_weighted(c.lib, c.ncols, c.hr, ht, nnegs, 5, w, users=users)
                        assert rc == SLIM_OK, _lib.last_error()
                        host = set_rows(c.lib, hs)
                        c.lib.SLIMGPU_CandSetFree(hs)
                        assert got[2] == host[2] == c.ncols
                        for k in (0, 1):
                            assert np.array_equal(got[k], want[k]), (name, wname, nnegs, users is None, ranked, "numpy", k)
                            assert np.array_equal(got[k], host[k]), (name, wname, nnegs, users is None, ranked, "host", k)
                    # NULL weights: the popularity of the resident matrix's columns
                    want = weighted_rows((name, "counts"), c.R, tptr, tind, c.ncols, 99, 5,
                                         weights("counts", c.R, c.ncols), users=users)
                    rc, cs = device_sample_weighted(c.lib, ev, 99, 5, None)
                    assert rc == SLIM_OK, _lib.last_error()
                    got = set_rows(c.lib, cs)
                    c.lib.SLIMGPU_CandSetFree(cs)
                    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
                    # the uniform call on the same eval set, after the weighted ones, is what it was
                    uni = sampled_rows(c.R, tptr, tind, c.ncols, 99, seed=5, users=users)
                    h = C.c_void_p()
                    assert c.lib.SLIMGPU_EvalSetSampleCandidates(ev.handle, 99, 5, C.byref(h)) == SLIM_OK
                    got = set_rows(c.lib, h)
                    c.lib.SLIMGPU_CandSetFree(h)
                    assert np.array_equal(got[0], uni[0]) and np.array_equal(got[1], uni[1])
                finally:
                    ev.close()
    finally:
        c.lib.Py_csr_free(ht)


@pytest.mark.parametrize("zero_tail", [False, True])
def test_the_hand_made_matrix_on_the_device(zero_tail):
    lib = _lib.load()
    R, T, w = hand_made(zero_tail)
    mat = DeviceMatrix.from_scipy(R, binary=True)
    try:
        assert mat.ncols == 40
        ev = mat.evaluator(T, fmarker=np.zeros(45, np.int32), cutoffs=(3,))
        for seed in (1, 2, 2 ** 63 + 11):
            want = weighted_rows(("hand", zero_tail), R, T.indptr.astype(np.int64), T.indices, 40, 5, seed, w)
            rc, cs = device_sample_weighted(lib, ev, 5, seed, w)
            assert rc == SLIM_OK, _lib.last_error()
            got = set_rows(lib, cs)
            lib.SLIMGPU_CandSetFree(cs)
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), seed
        assert np.diff(want[0]).tolist() == [1, 2 if zero_tail else 6, 6, 6, 0, 8]
        ev.close()
    finally:
        mat.close()


@EVERY
def test_figures_on_a_device_born_weighted_set(cases, name):
    c = cases(name)
    T = held_out_rows(c, seed=91)
    tptr, tind = T.indptr.astype(np.int64), T.indices
    fm = np.random.default_rng(3).integers(0, 2, c.ncols).astype(np.int32)
    counts = weights("counts", c.R, c.ncols)
    for users in (None, np.arange(0, c.nusers, 3, dtype=np.int32)):
        ev = c.mat.evaluator(T, fmarker=fm, cutoffs=CUTOFFS, users=users)
        want_rows = weighted_rows((name, "counts"), c.R, tptr, tind, c.ncols, 99, 7, counts, users=users)
        born = ev.sample_candidates(99, seed=7, weights="popularity")
        made = c.mat.candidate_set(want_rows)
        try:
            assert isinstance(born, CandidateSet) and born.size == want_rows[1].size
            assert np.array_equal(born.indptr, want_rows[0])
            got = ev.evaluate_candidates(c.model, born)
            again = ev.evaluate_candidates(c.model, born)
            st = ev.stats()
            want = ev.evaluate_candidates(c.model, made)
            print(name, "popularity", [(r["nrcmds"], r["hr"], r["arhr"], r["nvalid"]) for r in got], "second call", st)
            assert got == want == again                     # every returned double and count
            assert st["path"] == 5 and st["device_allocs"] == 0 and st["h2d_bytes"] == 0
            assert st["d2h_bytes"] <= 8 + 32 * len(CUTOFFS)
            assert got[-1]["nvalid"] > 0 and 0 < got[-1]["hr"] <= 1
            ptr, ind = born.rows()                          # the ids come down when asked
            assert np.array_equal(ptr, want_rows[0]) and np.array_equal(ind, want_rows[1])
            # an explicit array through the Python layer
            zipf = weights("zipf", c.R, c.ncols)
            z = ev.sample_candidates(65, seed=5, weights=zipf)
            zr = weighted_rows((name, "zipf"), c.R, tptr, tind, c.ncols, 65, 5, zipf, users=users)
            ptr, ind = z.rows()
            z.close()
            assert np.array_equal(ptr, zr[0]) and np.array_equal(ind, zr[1])
        finally:
            born.close()
            made.close()
            ev.close()


def test_device_refusals_leave_out_untouched(cases):
    c = cases("floats")
    T = held_out_rows(c, seed=91)
    ev = c.mat.evaluator(T, fmarker=np.zeros(c.ncols, np.int32), cutoffs=(10,))
    SENTINEL = 0x5A5A
    zipf = weights("zipf", c.R, c.ncols)
    try:
        for nnegs, w, word in ((0, zipf, "nnegs"), (-3, None, "nnegs"), (99, np.zeros(c.ncols, np.uint32), "T = 0")):
            h = C.c_void_p(SENTINEL)
            rc = c.lib.SLIMGPU_EvalSetSampleCandidatesWeighted(ev.handle, nnegs, 1, None if w is None else w.ctypes.data_as(C.c_void_p),
                                                               C.byref(h))
            assert rc == SLIM_ERROR_INPUT and h.value == SENTINEL
            assert "SLIMGPU_EvalSetSampleCandidatesWeighted" in _lib.last_error() and word in _lib.last_error()
        assert c.lib.SLIMGPU_EvalSetSampleCandidatesWeighted(ev.handle, 99, 1, None, None) == SLIM_ERROR_INPUT
        h = C.c_void_p(SENTINEL)
        assert c.lib.SLIMGPU_EvalSetSampleCandidatesWeighted(None, 99, 1, None, C.byref(h)) == SLIM_ERROR_INPUT
        assert h.value == SENTINEL
    finally:
        ev.close()


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


def test_the_grid_on_popularity_negatives(automotive, monkeypatch, capfd, tmp_path):
    """Py_SLIM_Mselect with slot 25, SLIM.mselect(negpop=True) and slim_mselect -evalnegs=99 -evalnegpop print the
    figures of the existing calls on numpy's popularity rows and choose the best pairs from them."""
    import os
    import subprocess
    from conftest import ROOT
    from slim_amd.io import write_csr_text
    MSELECT = os.path.join(ROOT, "slim_amd", "bin", "slim_mselect")
    R, T = sp.csr_matrix(automotive[0]), sp.csr_matrix(automotive[1])
    monkeypatch.setenv("SLIM_GPU_NO_CARRY", "1")       # a pair's model does not depend on who solved before
    monkeypatch.setenv("SLIM_GPU_RESIDENT", "1")
    monkeypatch.setenv("SLIM_GPU_EVAL_RESIDENT", "1")
    got, entries = grid_by_hand_popularity(R, T, 99, seed=1)
    header = "  sampled negatives: nnegs 99, seed 1, popularity, %d candidate entries\n" % entries
    model, out, err = mselect(R, T, capfd, params={"gpu_evalnegs": 99, "gpu_evalnegpop": 1})       # slots 23 and 25
    assert err is None, err
    assert header in out
    lines = re.findall(PAIR, out)
    check_grid_lines(lines, got, model.mselect_result)
    assert eval_stats()["path"] == 5
    model, out, err = mselect(R, T, capfd, nnegs=99, negpop=True)
    assert err is None and header in out
    check_grid_lines(re.findall(PAIR, out), got, model.mselect_result)
    # the uniform grid prints other figures and today's header line: the option was not ignored
    _, uni, err = mselect(R, T, capfd, nnegs=99)
    assert err is None and "  sampled negatives: nnegs 99, seed 1, %d candidate entries\n" % entries in uni
    assert "popularity" not in uni and re.findall(PAIR, uni) != lines
    # the command line
    names = [str(tmp_path / f) for f in ("trn.csr", "tst.csr", "l12")]
    write_csr_text(names[0], R)
    write_csr_text(names[1], sp.csr_matrix((T.data, T.indices, T.indptr), shape=T.shape))
    open(names[2], "w").write("".join("%g %g\n" % (a, b) for a in GRID_L1 for b in GRID_L2))
    p = subprocess.run([MSELECT, "-nomodels", "-niters=200", "-evalnegs=99", "-evalnegpop"] + names, capture_output=True,
                       text=True, cwd=str(tmp_path), timeout=280)
    assert p.returncode == 0, p.stdout + p.stderr
    assert header in p.stdout
    check_grid_lines(re.findall(PAIR, p.stdout), got)
    assert "best hr: %.4f at" % max(g["hr"] for _, _, g, _ in got) in p.stdout
    p = subprocess.run([MSELECT, "-nomodels", "-evalnegpop"] + names, capture_output=True, text=True, cwd=str(tmp_path),
                       timeout=60)
    assert p.returncode != 0 and "-evalnegs" in p.stdout + p.stderr and "l1r:" not in p.stdout


def test_negpop_without_negatives_is_refused_before_the_first_solve(automotive, monkeypatch, capfd):
    R, T = sp.csr_matrix(automotive[0]), sp.csr_matrix(automotive[1])
    monkeypatch.setenv("SLIM_GPU_RESIDENT", "1")
    monkeypatch.setenv("SLIM_GPU_EVAL_RESIDENT", "1")
    for kw in (dict(negpop=True), dict(params={"gpu_evalnegpop": 1}), dict(params={"gpu_evalnegpop": 1, "gpu_evalnegs": 0})):
        _, out, err = mselect(R, T, capfd, **kw)
        assert err is not None and "EVALNEGPOP" in err and "EVALNEGS is off" in err, err
        assert "l1r:" not in out and "Estimating" not in out, out
    _, out, err = mselect(R, T, capfd, params={"gpu_evalnegpop": 2, "gpu_evalnegs": 99})
    assert err is not None and "0 or 1" in err and "l1r:" not in out
