"""One grid evaluator behind three doors (slim_amd/csrc/grid_eval.cpp): Py_SLIM_Mselect*, slim_mselect and the
SLIMGPU_Grid* calls themselves (include/slim_gpu_grid.h) print the same pair and exposure lines, time apart, in
every evaluation mode of a small synthetic grid."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
import scipy.sparse as sp

import slim_oracle as O
from conftest import ROOT
from filtered_cases import make_filter, wrap
from sampled_cases import PAIR
from slim_amd import _lib
from slim_amd.constants import SLIM_ALGO, SLIM_NOPTIONS, SLIM_OK, Opt
from slim_amd.io import write_csr_text

pytestmark = pytest.mark.gpu
MSELECT = os.path.join(ROOT, "slim_amd", "bin", "slim_mselect")
NUSERS, NITEMS, NITERS = 300, 100, 30
L1, L2 = [0.1, 0.5], [0.5, 2.0]
BLOCKED = [0, 3, 17, 42, 99]
EXPO = r"(  exposure@\d+: coverage: \S+ tail_share: \S+ gini: \S+ avg_pop: \S+ distinct: \d+ slots: \d+)"
# mode: (option slots, environment, slim_mselect's arguments, with the filter)
MODES = {
    "plain": ({Opt.NRCMDS: 10}, {}, ["-nrcmds=10"], False),
    "ranked": ({Opt.NRCMDS: 200}, {}, ["-nrcmds=200"], False),
    "stride": ({Opt.GPU_EVALSTRIDE: 3}, {}, ["-evalstride=3"], False),
    "negatives": ({Opt.GPU_EVALNEGS: 50}, {}, ["-evalnegs=50"], False),
    "negatives_by_popularity": ({Opt.GPU_EVALNEGS: 50, Opt.GPU_EVALNEGPOP: 1}, {}, ["-evalnegs=50", "-evalnegpop"],
                                False),
    "exposure": ({Opt.GPU_EVALEXPOSURE: 1}, {}, ["-evalexposure"], False),
    "filter": ({}, {}, [], True),
    "filter_exposure": ({Opt.GPU_EVALEXPOSURE: 1}, {}, ["-evalexposure"], True),
    "resident0": ({}, {"SLIM_GPU_RESIDENT": "0"}, [], False),
    "eval_resident0": ({}, {"SLIM_GPU_EVAL_RESIDENT": "0"}, [], False),
}


def make_case(d):
    """Five tastes of twenty items each, popular items first in every taste: head and tail both populated.  Most
    users hold one item of their taste out; every tenth has no test row."""
    rng = np.random.default_rng(11)
    weight = 1.0 / np.arange(1, 21)
    rows, cols, held = [], [], []
    for u in range(NUSERS):
        own = 20 * (u % 5) + rng.choice(20, size=9, replace=False, p=weight / weight.sum())
        stray = rng.integers(0, NITEMS, size=2)
        items = np.unique(np.concatenate((own[1:], stray)))
        items = items[items != own[0]]
        rows += [u] * items.size
        cols += list(items)
        held.append(own[0])
    rows, cols = rows + [0, 1], cols + [NITEMS - 1, 0]     # (the catalogue is as wide as it says)
    R = sp.csr_matrix((np.ones(len(rows), np.float32), (rows, cols)), shape=(NUSERS, NITEMS))
    R.data[:] = 1.0     # (a stray that repeats an item is no second rating)
    R.sort_indices()
    tested = [u for u in range(NUSERS) if u % 10 != 9 and R[u, held[u]] == 0]
    T = sp.csr_matrix((np.ones(len(tested), np.float32), (tested, [held[u] for u in tested])), shape=(NUSERS, NITEMS))
    marker = np.asarray(O.head_tail(R, NITEMS))
    assert 0 < marker.sum() < NITEMS and len(tested) > NUSERS // 2
    files = [os.path.join(d, f) for f in ("trn.csr", "tst.csr", "l12", "blocked")]
    write_csr_text(files[0], R)
    write_csr_text(files[1], T)
    open(files[2], "w").write("".join("%g %g\n" % (a, b) for a in L1 for b in L2))
    open(files[3], "w").write("".join("%d\n" % i for i in BLOCKED))
    return R, T, files


@pytest.fixture(scope="module")
def case(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("doors"))
    R, T, files = make_case(d)
    lib = _lib.load()
    trn, tst = wrap(lib, R), wrap(lib, T)
    rc, flt = make_filter(lib, NITEMS, blocked=BLOCKED)
    assert rc == SLIM_OK
    yield lib, trn, tst, flt, files, d
    lib.SLIMGPU_FilterFree(flt)
    for h in (trn, tst):
        lib.Py_csr_free(h)


def options(slots):
    iopt, dopt = np.full(SLIM_NOPTIONS, -1, np.int32), np.full(SLIM_NOPTIONS, -1.0)
    for k, v in ((Opt.DBGLVL, 0), (Opt.NNBRS, 0), (Opt.SIMTYPE, 0), (Opt.ALGO, SLIM_ALGO["cd"]), (Opt.NTHREADS, 1),
                 (Opt.MAXNITERS, NITERS)):
        iopt[k] = v
    dopt[Opt.OPTTOL] = 1e-7
    for k, v in slots.items():
        iopt[k] = v
    return iopt, dopt


def lines_of(out):
    """The pair lines and the exposure lines in the order printed, without the time."""
    return [re.sub(r" time: \S+", "", m.group(0)) for m in re.finditer(PAIR + r"[^\n]*|" + EXPO, out)]


def through_the_library(case, capfd, slots, filtered):
    lib, trn, tst, flt = case[:4]
    iopt, dopt = options(slots)
    best = [C.c_double(0.0) for _ in range(8)]
    args = [trn, tst, iopt, dopt, np.array(L1), np.array(L2), 2, 2] + [C.byref(b) for b in best]
    C.CDLL(None).fflush(None)
    capfd.readouterr()
    rc = lib.Py_SLIM_MselectFiltered(*(args + [flt])) if filtered else lib.Py_SLIM_Mselect(*args)
    C.CDLL(None).fflush(None)
    out = capfd.readouterr().out
    assert rc == SLIM_OK, _lib.last_error()
    return lines_of(out)


def through_the_program(case, extra, filtered):
    files, cwd = case[4], case[5]
    cmd = [MSELECT, "-nomodels", "-niters=%d" % NITERS] + extra + (["-blockfile=" + files[3]] if filtered else [])
    p = subprocess.run(cmd + files[:3], capture_output=True, text=True, cwd=cwd, timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr
    return lines_of(p.stdout)


def through_the_grid(case, slots, filtered):
    """SLIMGPU_Grid* from here: the lines in the library's formats, and the nnz of the last model fetched."""
    lib, trn, tst, flt = case[:4]
    iopt, dopt = options(slots)
    nrcmds = 10 if iopt[Opt.NRCMDS] == -1 else int(iopt[Opt.NRCMDS])
    grid = C.c_void_p()
    rc = lib.SLIMGPU_GridOpen(trn, tst, iopt, dopt, 0, len(L1) * len(L2), flt if filtered else None, C.byref(grid))
    assert rc == SLIM_OK and grid.value, _lib.last_error()
    lines, cell = [], _lib.GridCell()
    try:
        for l1 in L1:
            for l2 in L2:
                assert lib.SLIMGPU_GridSolve(grid, l1, l2, C.byref(cell)) == SLIM_OK, _lib.last_error()
                assert (cell.l1r, cell.l2r) == (l1, l2) and cell.nvalid[0] >= 1 and cell.solve_seconds >= 0
                m = cell.metrics
                lines.append("l1r: %.2e l2r: %.2e nnz: %7d hr: %.4f hr_head: %.4f hr_tail: %.4f arhr: %.4f"
                             % (l1, l2, cell.nnz, m[0], m[1], m[2], m[3]))
                assert bool(cell.has_exposure) == (iopt[Opt.GPU_EVALEXPOSURE] == 1)
                if cell.has_exposure:
                    e = cell.exposure
                    lines.append("  exposure@%d: coverage: %.4f tail_share: %.4f gini: %.4f avg_pop: %.2f distinct: %d "
                                 "slots: %d" % (nrcmds, e.coverage, e.tail_share, e.gini, e.avg_pop, e.distinct,
                                                e.slots))
        status = C.c_int32(0)
        model = lib.SLIMGPU_GridModel(grid, C.byref(status))
        assert model and status.value == SLIM_OK, _lib.last_error()
        view = C.cast(model, C.POINTER(_lib.CsrView)).contents
        nnz = int(view.rowptr[view.nrows])
        assert lib.SLIMGPU_GridModel(grid, C.byref(status)) == model     # the grid's until the next solve
    finally:
        lib.SLIMGPU_GridFree(C.byref(grid))
    assert grid.value is None
    return lines, nnz


@pytest.mark.parametrize("mode", list(MODES))
def test_the_three_doors_print_the_same(case, monkeypatch, capfd, mode):
    slots, env, extra, filtered = MODES[mode]
    for k in ("SLIM_GPU_NGPUS", "SLIM_GPU_RESIDENT", "SLIM_GPU_EVAL_RESIDENT"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    library = through_the_library(case, capfd, slots, filtered)
    program = through_the_program(case, extra, filtered)
    grid, nnz = through_the_grid(case, slots, filtered)
    for line in library:
        print(line)
    per_pair = 2 if slots.get(Opt.GPU_EVALEXPOSURE) == 1 else 1
    assert len(library) == per_pair * len(L1) * len(L2)
    assert library == program
    assert library == grid
    pairs = [line for line in library if line.startswith("l1r:")]
    assert nnz == int(re.search(r"nnz:\s+(\d+)", pairs[-1]).group(1)) and nnz > 0
