"""Exposure in the model-selection grid (slot 26, Py_SLIM_MselectExposure, SLIM.mselect(exposure=True),
slim_mselect -evalexposure) on the 2 x 2 grid of tests/sampled_cases.py.

The figures are first made by hand through existing calls -- learn_resident warm-chained as sampled_cases.grid_by_hand
chains it, ResidentModel.predict for the lists, np.bincount and Python ints (exposure_cases.restate) -- and every
front door must carry them; the pair lines and the best pairs must be those of a run with the slot off."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
import scipy.sparse as sp

import slim_oracle as O
from conftest import ROOT
from exposure_cases import restate
from sampled_cases import GRID_L1, GRID_L2, PAIR
from slim_amd import _lib
from slim_amd.constants import SLIM_ERROR_INPUT
from slim_amd.engine import DeviceMatrix

pytestmark = pytest.mark.gpu
MSELECT = os.path.join(ROOT, "slim_amd", "bin", "slim_mselect")
PARAMS = {"dbglvl": 0, "algo": "cd", "nthreads": 1, "optTol": 1e-7, "niters": 200}
EXPO = (r"  exposure@(\d+): coverage: (\S+) tail_share: (\S+) gini: (\S+) avg_pop: (\S+) distinct: (\d+) "
        r"slots: (\d+)")
NRCMDS = 10


def by_hand(R, T):
    """[(l1, l2, figures, summary)] of the grid: every pair's top-NRCMDS lists counted in numpy."""
    mat = DeviceMatrix.from_scipy(R)
    mat.expect_solves(4)
    nall = min(R.shape[0], T.shape[0])
    width = max(mat.ncols, int(T.indices.max()) + 1)
    fm = np.ascontiguousarray(O.head_tail(sp.csr_matrix(R), width), np.int32)
    pop = np.bincount(R.indices, minlength=mat.ncols).astype(np.uint32)
    ev = mat.evaluator(T, nrcmds=NRCMDS)
    prev, got = None, []
    for l1 in GRID_L1:
        for l2 in GRID_L2:
            cur, _ = mat.learn_resident(warm=prev, l1r=l1, l2r=l2, optTol=1e-7, niters=200)
            if prev is not None:
                prev.free()
            prev = cur
            ids, _, counts = cur.predict(mat, nrcmds=NRCMDS, users=np.arange(nall), return_counts=True)
            E, summ = restate(mat.ncols, ids, counts, (NRCMDS,), pop=pop, fmarker=fm)
            assert np.array_equal(E[0], np.bincount(ids[ids >= 0], minlength=mat.ncols))
            got.append((l1, l2, ev.evaluate(cur), summ[0]))
    prev.free()
    for h in (ev, mat):
        h.close()
    return got


def mselect(R, T, capfd, nrcmds=NRCMDS, params=None, **kw):
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


def check_lines(out, got):
    """Every pair line is followed by its exposure line, which carries the by-hand figures as printed."""
    pairs, expo = re.findall(PAIR, out), re.findall(EXPO, out)
    assert len(pairs) == len(expo) == len(got) == 4
    for line, e, (l1, l2, g, s) in zip(pairs, expo, got):
        print(line, e, s)
        assert line.startswith("l1r: %.2e l2r: %.2e " % (l1, l2))
        assert "hr: %.4f hr_head: %.4f hr_tail: %.4f arhr: %.4f" % (g["hr"], g["hr_head"], g["hr_tail"],
                                                                    g["arhr"]) in line
        assert e == (str(NRCMDS), "%.4f" % s["coverage"], "%.4f" % s["tail_share"], "%.4f" % s["gini"],
                     "%.2f" % s["avg_pop"], str(s["distinct"]), str(s["slots"]))
    assert len(re.findall(PAIR + r"[^\n]*\n  exposure@", out)) == 4
    return pairs


def test_the_grid_with_exposure(automotive, monkeypatch, capfd, tmp_path):
    R, T = sp.csr_matrix(automotive[0]), sp.csr_matrix(automotive[1])
    monkeypatch.setenv("SLIM_GPU_NO_CARRY", "1")       # a pair's model does not depend on who solved before
    monkeypatch.setenv("SLIM_GPU_RESIDENT", "1")
    monkeypatch.setenv("SLIM_GPU_EVAL_RESIDENT", "1")
    got = by_hand(R, T)
    # the by-hand figures are no empty lists, and not every item is shown
    assert all(s["slots"] > s["distinct"] > 1 and s["coverage"] < 1 and s["gini"] > 0 for _, _, _, s in got)
    # Py_SLIM_MselectExposure through SLIM.mselect(exposure=True): lines, cells, best pairs
    model, out, err = mselect(R, T, capfd, exposure=True)
    assert err is None, err
    pairs = check_lines(out, got)
    names = ("coverage", "tail_share", "gini", "avg_pop")
    assert len(model.last_exposure) == 4
    for cell, (l1, l2, g, s) in zip(model.last_exposure, got):
        assert (cell["l1"], cell["l2"]) == (l1, l2) and (cell["hr"], cell["arhr"]) == (g["hr"], g["arhr"])
        assert [np.float64(cell[k]).view(np.int64) for k in names] == [np.float64(s[k]).view(np.int64) for k in names]
    with_result = model.mselect_result
    # slot 26 off: the same pair lines, no exposure line, the same best pairs; no table
    plain_model, plain, err = mselect(R, T, capfd)
    assert err is None and "exposure@" not in plain
    assert re.findall(PAIR, plain) == pairs and plain_model.mselect_result == with_result
    assert plain_model.last_exposure is None
    # the command line
    from slim_amd.io import write_csr_text
    files = [str(tmp_path / f) for f in ("trn.csr", "tst.csr", "l12")]
    write_csr_text(files[0], R)
    write_csr_text(files[1], sp.csr_matrix((T.data, T.indices, T.indptr), shape=T.shape))
    open(files[2], "w").write("".join("%g %g\n" % (a, b) for a in GRID_L1 for b in GRID_L2))
    p = subprocess.run([MSELECT, "-nomodels", "-niters=200", "-evalexposure"] + files, capture_output=True, text=True,
                       cwd=str(tmp_path), timeout=280)
    assert p.returncode == 0, p.stdout + p.stderr
    check_lines(p.stdout, got)
    p = subprocess.run([MSELECT, "-nomodels", "-evalexposure", "-evalnegs=50"] + files, capture_output=True, text=True,
                       cwd=str(tmp_path), timeout=60)
    assert p.returncode != 0 and "evalnegs" in p.stdout + p.stderr and "l1r:" not in p.stdout


def test_the_grid_refuses_before_the_first_solve(automotive, monkeypatch, capfd):
    R, T = sp.csr_matrix(automotive[0]), sp.csr_matrix(automotive[1])
    monkeypatch.setenv("SLIM_GPU_RESIDENT", "1")
    monkeypatch.setenv("SLIM_GPU_EVAL_RESIDENT", "1")

    def refused(word, env=None, **kw):
        for k, v in (env or {}).items():
            monkeypatch.setenv(k, v)
        _, out, err = mselect(R, T, capfd, **kw)
        for k in env or {}:
            monkeypatch.setenv(k, "1")
        assert err is not None and "EVALEXPOSURE" in err and word in err, (word, err)
        assert "l1r:" not in out and "Estimating" not in out, out
    refused("SLIM_OPTION_GPU_EVALNEGS is on", params={"gpu_evalexposure": 1, "gpu_evalnegs": 99})
    refused("nrcmds is 200", exposure=True, nrcmds=200)
    refused("ADMM", exposure=True, params={"algo": "admm"})
    refused("several GPUs", exposure=True, env={"SLIM_GPU_NGPUS": "2"})
    refused("SLIM_GPU_RESIDENT=0", exposure=True, env={"SLIM_GPU_RESIDENT": "0"})
    refused("SLIM_GPU_EVAL_RESIDENT=0", params={"gpu_evalexposure": 1}, env={"SLIM_GPU_EVAL_RESIDENT": "0"})
    refused("must be 0 or 1", params={"gpu_evalexposure": 2})
    # the status itself
    from slim_amd import SLIMatrix
    from slim_amd.interface import build_options, check_params
    params = dict(PARAMS, gpu_evalexposure=1)
    check_params(params)
    params["nrcmds"] = 200
    iopt, dopt = build_options(params)
    assert iopt[26] == 1
    trainmat = SLIMatrix(R)
    valmat = SLIMatrix(T, trainmat)
    best = [C.c_double(0.0) for _ in range(8)]
    rc = _lib.load().Py_SLIM_Mselect(trainmat.handle, valmat.handle, iopt, dopt, np.array(GRID_L1), np.array(GRID_L2),
                                     2, 2, *[C.byref(b) for b in best])
    assert rc == SLIM_ERROR_INPUT and "nrcmds is 200" in _lib.last_error()
