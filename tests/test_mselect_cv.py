"""Py_SLIM_MselectCV and SLIMGPU_GridOpenOn (include/slim_gpu_split.h, include/slim_gpu_grid.h): the grid
cross-validated on one matrix.  The bar: every (fold, pair) row of its cells is, bit for bit, what the grid on the HOST
handles that SLIMGPU_SplitHost makes for that fold gives (SLIMGPU_GridOpen / GridSolve, which Py_SLIM_Mselect loops
over) -- the head / tail figures included, so the marker formed from the column pointer is SLIM_DetermineHeadAndTail's
-- and the best pairs are those of the means recomputed here."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import scipy.sparse as sp

from conftest import GOLDEN, ROOT
from slim_amd import _lib
from slim_amd.constants import SLIM_ALGO, SLIM_ERROR_INPUT, SLIM_OK, Opt
from slim_amd.engine import DeviceMatrix, make_options
from split_cases import LEAVE_OUT

pytestmark = pytest.mark.gpu

F, HELD, MINKEEP, SEED = 3, 1, 1, 77
L1, L2 = [1.0, 5.0], [1.0, 10.0]
NRCMDS, NITERS = 10, 60


def options():
    iopt, dopt = make_options(niters=NITERS, seed=1)
    iopt[Opt.NRCMDS] = NRCMDS
    return iopt, dopt


def wrap(lib, R):
    h = C.c_void_p()
    assert lib.Py_csr_wrapper(R.shape[0], np.ascontiguousarray(R.indptr, np.intp),
                              np.ascontiguousarray(R.indices, np.int32),
                              np.ascontiguousarray(R.data, np.float32).ctypes.data_as(C.c_void_p), C.byref(h)) == SLIM_OK
    return h


def run_cv(lib, R, cells=True):
    """Py_SLIM_MselectCV on R: (status, the eight outputs, cells [F][pairs][CV_CELL])."""
    iopt, dopt = options()
    spec = _lib.Split(LEAVE_OUT, F, 0, HELD, MINKEEP, SEED)
    best = [C.c_double(-1.0) for _ in range(8)]
    out = np.zeros((F, len(L1) * len(L2), _lib.CV_CELL), np.float64)
    h = wrap(lib, R)
    rc = lib.Py_SLIM_MselectCV(h, iopt, dopt, np.array(L1), np.array(L2), len(L1), len(L2), C.byref(spec), None,
                               *([C.byref(b) for b in best] + [out.ctypes.data_as(C.c_void_p) if cells else None]))
    lib.Py_csr_free(h)
    return rc, [b.value for b in best], out


@pytest.fixture(scope="module")
def cv(ml100k):
    lib = _lib.load()
    rc, best, cells = run_cv(lib, ml100k[0])
    assert rc == SLIM_OK, _lib.last_error()
    return best, cells


@pytest.fixture(scope="module")
def by_fold(ml100k):
    """Per fold: the cells of the grid on the host handles of SLIMGPU_SplitHost, and Py_SLIM_Mselect's eight outputs
    on the same handles."""
    lib = _lib.load()
    data = wrap(lib, ml100k[0])
    out = []
    for f in range(F):
        spec = _lib.Split(LEAVE_OUT, F, f, HELD, MINKEEP, SEED)
        trn, tst = C.c_void_p(), C.c_void_p()
        assert lib.SLIMGPU_SplitHost(data, C.byref(spec), C.byref(trn), C.byref(tst)) == SLIM_OK
        iopt, dopt = options()
        grid = C.c_void_p()
        assert lib.SLIMGPU_GridOpen(trn, tst, iopt, dopt, 0, len(L1) * len(L2), None, C.byref(grid)) == SLIM_OK
        rows = []
        for a in L1:
            for b in L2:
                c = _lib.GridCell()
                assert lib.SLIMGPU_GridSolve(grid, a, b, C.byref(c)) == SLIM_OK
                rows.append([float(f), c.l1r, c.l2r] + list(c.metrics) + [float(v) for v in c.nvalid] + [float(c.nnz)])
        lib.SLIMGPU_GridFree(C.byref(grid))
        iopt, dopt = options()
        best = [C.c_double(-1.0) for _ in range(8)]
        assert lib.Py_SLIM_Mselect(trn, tst, iopt, dopt, np.array(L1), np.array(L2), len(L1), len(L2),
                                   *[C.byref(b) for b in best]) == SLIM_OK
        out.append((np.array(rows, np.float64), [b.value for b in best]))
        lib.Py_csr_free(trn)
        lib.Py_csr_free(tst)
    lib.Py_csr_free(data)
    return out


def best_of(rows):
    """Py_SLIM_Mselect's choice over rows of (l1, l2, hr, arhr): strict > in the order given."""
    bh, ba = (0.0, 0.0, 0.0, 0.0), (0.0, 0.0, 0.0, 0.0)
    for l1, l2, hr, arhr in rows:
        if hr > bh[2]:
            bh = (l1, l2, hr, arhr)
        if arhr > ba[3]:
            ba = (l1, l2, hr, arhr)
    return list(bh) + list(ba)


def test_every_cell_is_the_fold_grid_on_host_split_handles(cv, by_fold):
    _, cells = cv
    for f in range(F):
        want, mselect_best = by_fold[f]
        print("fold", f, "cv", cells[f][:, 3:7].tolist(), "host", want[:, 3:7].tolist())
        assert cells[f].tobytes() == want.tobytes(), "fold %d: cells differ from the grid on host-split handles" % f
        # ... and Py_SLIM_Mselect on those handles returns the best of exactly these figures
        assert best_of([(r[1], r[2], r[3], r[6]) for r in want]) == mselect_best
        assert (want[:, 7] > 300).all() and (want[:, 4:6] > 0).all(), "a fold evaluates users, head and tail"


def test_the_best_pairs_are_those_of_the_means(cv):
    best, cells = cv
    rows = []
    for p in range(cells.shape[1]):
        hr = arhr = 0.0
        for f in range(F):      # summed as doubles in fold order, divided by F
            hr += cells[f, p, 3]
            arhr += cells[f, p, 6]
        rows.append((cells[0, p, 1], cells[0, p, 2], hr / F, arhr / F))
    assert [(r[0], r[1]) for r in rows] == [(a, b) for a in L1 for b in L2]
    assert best == best_of(rows)
    assert best[2] > 0 and best[7] > 0


def test_resident_0_gives_the_same_cells(cv, tmp_path):
    """SLIM_GPU_RESIDENT=0: the folds are split on the host and the grids opened from host handles."""
    code = r"""
import sys
sys.path.insert(0, %r); sys.path.insert(0, %r)
import numpy as np
import test_mselect_cv as T
from slim_amd import _lib
from slim_amd.io import read_csr_text
rc, best, cells = T.run_cv(_lib.load(), read_csr_text(%r))
assert rc == 1, _lib.last_error()
np.save(sys.argv[1], cells)
np.save(sys.argv[2], np.array(best))
""" % (ROOT, os.path.join(ROOT, "tests"), os.path.join(GOLDEN, "ml100k-train.csr"))
    env = dict(os.environ, SLIM_GPU_RESIDENT="0")
    paths = [str(tmp_path / "cells.npy"), str(tmp_path / "best.npy")]
    r = subprocess.run([sys.executable, "-c", code] + paths, env=env, capture_output=True, text=True, timeout=280)
    assert r.returncode == 0, r.stderr[-3000:]
    assert "split on the host" in r.stdout
    best, cells = cv
    got = np.load(paths[0])
    print("resident", cells[:, :, 3:7].tolist(), "host route", got[:, :, 3:7].tolist())
    assert got.tobytes() == cells.tobytes()
    assert np.load(paths[1]).tolist() == best


def test_python_mselect_cv_keeps_the_table(cv, ml100k, capfd):
    from slim_amd import SLIM, SLIMatrix
    best, cells = cv
    model = SLIM()
    data = SLIMatrix(sp.csr_matrix(ml100k[0]))
    params = dict(niters=NITERS, gpu_seed=1)
    model.mselect(params, data, None, L1, L2, NRCMDS, cv=F, cv_mode="leave_out", cv_held=HELD, cv_minkeep=MINKEEP,
                  cv_seed=SEED)
    out = capfd.readouterr().out
    for f in range(F):
        assert "fold %d of %d" % (f, F) in out
    assert len(re.findall(r"^l1r: \S+ l2r: \S+ hr: \S+ \(min \S+ max \S+\) arhr: ", out, re.M)) == len(L1) * len(L2)
    assert len(model.last_cv) == F and len(model.last_cv[0]) == len(L1) * len(L2)
    for f in range(F):
        for p, row in enumerate(model.last_cv[f]):
            assert [row[k] for k in ("hr", "hr_head", "hr_tail", "arhr")] == cells[f, p, 3:7].tolist()
            assert (row["fold"], row["l1"], row["l2"], row["nnz"]) == (f, cells[f, p, 1], cells[f, p, 2], int(cells[f, p, 10]))
    assert list(model.mselect_result["bestHR"]) + list(model.mselect_result["bestAR"]) == best
    with pytest.raises(TypeError, match="tstdata=None"):
        model.mselect(params, data, data, L1, L2, NRCMDS, cv=F)
    with pytest.raises(TypeError, match="does not combine"):
        model.mselect(params, data, None, L1, L2, NRCMDS, cv=F, exposure=True)


def test_grid_open_on_refuses_what_needs_host_rows_and_leaves_the_matrix(ml100k):
    lib = _lib.load()
    mat = DeviceMatrix.from_scipy(ml100k[0])
    trn, tst = mat.split(mode="leave_out", nfolds=F, fold=0, nheld=HELD, minkeep=MINKEEP, seed=SEED)
    ht = wrap(lib, tst)
    iopt, dopt = options()
    iopt[Opt.ALGO] = SLIM_ALGO["admm"]
    grid = C.c_void_p(0x1234)
    assert lib.SLIMGPU_GridOpenOn(trn.handle, ht, iopt, dopt, 0, 4, None, C.byref(grid)) == SLIM_ERROR_INPUT
    assert "SLIMGPU_GridOpenOn" in _lib.last_error() and "ADMM" in _lib.last_error() and grid.value == 0x1234
    iopt, dopt = options()
    iopt[Opt.NRCMDS] = 0
    assert lib.SLIMGPU_GridOpenOn(trn.handle, ht, iopt, dopt, 0, 4, None, C.byref(grid)) == SLIM_ERROR_INPUT
    # the matrix is still the caller's: it answers, and a grid opened on it now takes it over
    assert trn.column_view()[0][-1] == trn.nnz
    iopt, dopt = options()
    assert lib.SLIMGPU_GridOpenOn(trn.handle, ht, iopt, dopt, 0, 1, None, C.byref(grid)) == SLIM_OK
    trn.handle = None   # (the grid's now)
    c = _lib.GridCell()
    assert lib.SLIMGPU_GridSolve(grid, 1.0, 1.0, C.byref(c)) == SLIM_OK and c.nvalid[0] > 300
    lib.SLIMGPU_GridFree(C.byref(grid))
    lib.Py_csr_free(ht)
    mat.close()


def test_cv_refusals(ml100k):
    lib = _lib.load()
    h = wrap(lib, ml100k[0])
    iopt, dopt = options()
    best = [C.c_double(0.0) for _ in range(8)]
    for spec, word in ((_lib.Split(LEAVE_OUT, 65, 0, 2, 1, 1), "nfolds * nheld"), (_lib.Split(1, 1, 0, 1, 1, 1), "nfolds"),
                       (_lib.Split(LEAVE_OUT, 2, 0, 1, 0, 1), "minkeep")):
        rc = lib.Py_SLIM_MselectCV(h, iopt, dopt, np.array(L1), np.array(L2), 2, 2, C.byref(spec), None,
                                   *([C.byref(b) for b in best] + [None]))
        assert rc == SLIM_ERROR_INPUT and word in _lib.last_error() and "Py_SLIM_MselectCV" in _lib.last_error()
    lib.Py_csr_free(h)
