"""A model-selection grid evaluated per user group and chosen on one group (include/slim_gpu_groups.h): a 2 x 2 grid
on ml100k with three history bands through Py_SLIM_MselectGrouped, against the grid object solved pair by pair
(SLIMGPU_GridSolve + SLIMGPU_GridLastGroups), against Py_SLIM_MselectFiltered for what must not change, and through
slim_mselect and SLIM.mselect."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
import scipy.sparse as sp

from conftest import ROOT
from filtered_cases import wrap
from slim_amd import _lib
from slim_amd.constants import SLIM_ALGO, SLIM_NOPTIONS, SLIM_OK, Opt

pytestmark = pytest.mark.gpu
MSELECT = os.path.join(ROOT, "slim_amd", "bin", "slim_mselect")
L1, L2 = [1.0, 2.0], [1.0, 5.0]
PAIRS = [(a, b) for a in L1 for b in L2]
# the golden ml100k rows hold 19 to 736 items: three bands that all have users
BOUNDS = (40, 100)
GROUP = r"  group (\d+): members: (\d+) hr: (\S+) hr_head: (\S+) hr_tail: (\S+) arhr: (\S+) nvalid: (\d+)"
P = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)  # noqa: E731


@pytest.fixture(scope="module")
def inputs(ml100k):
    lib = _lib.load()
    R, T = sp.csr_matrix(ml100k[0]), sp.csr_matrix(ml100k[1])
    groups = np.searchsorted(BOUNDS, np.diff(R.indptr), side="right").astype(np.int32)
    assert np.bincount(groups, minlength=3).min() > 50
    trn, tst = wrap(lib, R), wrap(lib, T)
    yield lib, trn, tst, R, T, groups
    for h in (trn, tst):
        lib.Py_csr_free(h)


@pytest.fixture(autouse=True)
def environment(monkeypatch):
    monkeypatch.setenv("SLIM_GPU_NO_CARRY", "1")       # a pair's model does not depend on who solved before
    monkeypatch.setenv("SLIM_GPU_RESIDENT", "1")
    monkeypatch.setenv("SLIM_GPU_EVAL_RESIDENT", "1")


def options(slots=()):
    iopt, dopt = np.full(SLIM_NOPTIONS, -1, np.int32), np.full(SLIM_NOPTIONS, -1.0)
    iopt[Opt.ALGO], iopt[Opt.MAXNITERS], iopt[Opt.NRCMDS] = SLIM_ALGO["cd"], 200, 10
    dopt[Opt.OPTTOL] = 1e-7
    for k, v in dict(slots).items():
        iopt[k] = v
    return iopt, dopt


def grouped(inputs, capfd, select, slots=()):
    """Py_SLIM_MselectGrouped: (status, the eight outputs, cells [4][4][9], stdout)."""
    lib, trn, tst, _, _, groups = inputs
    iopt, dopt = options(slots)
    best = [C.c_double(0.0) for _ in range(8)]
    cells = np.zeros((4, 4, _lib.GROUP_CELL))
    capfd.readouterr()
    rc = lib.Py_SLIM_MselectGrouped(trn, tst, iopt, dopt, np.array(L1), np.array(L2), 2, 2,
                                    *([C.byref(b) for b in best] + [None, 3, P(groups), select, P(cells)]))
    C.CDLL(None).fflush(None)
    return rc, [b.value for b in best], cells, capfd.readouterr().out


def pair_by_pair(inputs, slots=()):
    """The grid object: [(cell metrics, cell nvalid, group metrics [4][4], group nvalid [4][3])] in solve order."""
    lib, trn, tst, _, _, groups = inputs
    iopt, dopt = options(slots)
    grid = C.c_void_p(None)
    assert lib.SLIMGPU_GridOpen(trn, tst, iopt, dopt, 0, 4, None, C.byref(grid)) == SLIM_OK, _lib.last_error()
    out = []
    try:
        assert lib.SLIMGPU_GridSetGroups(grid, 3, P(groups), -1) == SLIM_OK, _lib.last_error()
        # the members are those of the users the grid evaluates; no pair yet, no rows yet
        stride = max(int(dict(slots).get(Opt.GPU_EVALSTRIDE, 1)), 1)
        users = np.arange(0, groups.size, stride)
        n, members = C.c_int32(0), np.zeros(4, np.int32)
        assert lib.SLIMGPU_GridGroupInfo(grid, C.byref(n), P(members)) == SLIM_OK and n.value == 3
        assert members.tolist() == np.bincount(groups[users], minlength=3).tolist() + [users.size]
        met, nv = np.zeros((4, 4)), np.zeros((4, 3), np.int32)
        assert lib.SLIMGPU_GridLastGroups(grid, P(met), P(nv)) != SLIM_OK
        assert "the last pair was not evaluated per group" in _lib.last_error()
        for l1, l2 in PAIRS:
            cell = _lib.GridCell()
            assert lib.SLIMGPU_GridSolve(grid, l1, l2, C.byref(cell)) == SLIM_OK, _lib.last_error()
            met, nv = np.zeros((4, 4)), np.zeros((4, 3), np.int32)
            assert lib.SLIMGPU_GridLastGroups(grid, P(met), P(nv)) == SLIM_OK, _lib.last_error()
            out.append((np.array(cell.metrics[:]), list(cell.nvalid[:]), met, nv))
        assert lib.SLIMGPU_GridSetGroups(grid, 3, P(groups), -1) != SLIM_OK     # not after the first solve
        assert "before the first solve" in _lib.last_error()
    finally:
        lib.SLIMGPU_GridFree(C.byref(grid))
    return out


def assert_cells(cells, solved):
    for at, ((l1, l2), (cmet, cnv, met, nv)) in enumerate(zip(PAIRS, solved)):
        for g in range(4):
            row = cells[at, g]
            print(at, g, row.tolist(), met[g].tolist(), nv[g].tolist())
            assert (row[0], row[1]) == (l1, l2)
            assert np.array_equal(row[2:6], met[g]) and row[6:9].tolist() == nv[g].tolist()
        assert np.array_equal(met[3], cmet) and nv[3].tolist() == cnv        # everybody: the pair's own figures
        assert nv[:3].sum(0).tolist() == cnv                                  # every user is in a band


def best_by_the_loops_rule(cells, g):
    """(l1, l2, hr, arhr) twice: the first pair with the largest HR of group row g, then with the largest ARHR."""
    out = []
    for col in (2, 5):
        at = int(np.argmax(cells[:, g, col]))       # (argmax takes the first of equals, as `>` in solve order does)
        out += [cells[at, g, 0], cells[at, g, 1], cells[at, g, 2], cells[at, g, 5]]
    return out


def test_cells_are_the_grid_objects_rows_and_the_plain_outputs_stand(inputs, capfd):
    lib, trn, tst = inputs[:3]
    rc, best, cells, out = grouped(inputs, capfd, -1)
    assert rc == SLIM_OK, _lib.last_error()
    assert_cells(cells, pair_by_pair(inputs))
    assert (cells[:, :, 2] > 0).all()
    # one line per group behind every pair line, carrying the cells as printed
    lines = re.findall(GROUP, out)
    assert len(lines) == 12 and "  user groups: 3, pairs chosen on everybody\n" in out
    members = np.bincount(inputs[5], minlength=3)
    for at in range(4):
        for g in range(3):
            row = cells[at, g]
            assert lines[3 * at + g] == (str(g), str(members[g]), "%.4f" % row[2], "%.4f" % row[3], "%.4f" % row[4],
                                         "%.4f" % row[5], str(int(row[6])))
    # select_group = -1 chooses as Py_SLIM_MselectFiltered does, bit for bit
    iopt, dopt = options()
    plain = [C.c_double(0.0) for _ in range(8)]
    capfd.readouterr()
    assert lib.Py_SLIM_MselectFiltered(trn, tst, iopt, dopt, np.array(L1), np.array(L2), 2, 2,
                                       *([C.byref(b) for b in plain] + [None])) == SLIM_OK
    C.CDLL(None).fflush(None)
    plain_out = capfd.readouterr().out
    assert [np.float64(b.value).view(np.int64) for b in plain] == [np.float64(b).view(np.int64) for b in best]
    assert "group" not in plain_out
    pair = r"(l1r: \S+ l2r: \S+ nnz:\s+\d+ hr: \S+ hr_head: \S+ hr_tail: \S+ arhr: \S+)"
    assert re.findall(pair, plain_out) == re.findall(pair, out) and len(re.findall(pair, out)) == 4
    # l1HR, l2HR, HRHR, ARHR, l1AR, l2AR, HRAR, ARAR: the first best of the everybody rows
    w = best_by_the_loops_rule(cells, 3)
    assert best == [w[0], w[1], w[2], w[3], w[4], w[5], w[6], w[7]]


def test_the_pairs_are_chosen_on_the_selected_group(inputs, capfd):
    rc, best, cells, out = grouped(inputs, capfd, 0)
    assert rc == SLIM_OK, _lib.last_error()
    assert "pairs chosen on group 0\n" in out
    assert best == best_by_the_loops_rule(cells, 0)
    # ... which is not what everybody's rows choose on this grid, or at least not their figures
    assert best != best_by_the_loops_rule(cells, 3)


@pytest.mark.parametrize("slots", [{Opt.GPU_EVALSTRIDE: 3}, {Opt.GPU_EVALNEGS: 99}], ids=["stride3", "negs99"])
def test_combined_with_the_stride_and_with_sampled_negatives(inputs, capfd, slots):
    rc, best, cells, out = grouped(inputs, capfd, 1, slots)
    assert rc == SLIM_OK, _lib.last_error()
    assert_cells(cells, pair_by_pair(inputs, slots))
    assert best == best_by_the_loops_rule(cells, 1)
    users = np.arange(0, inputs[3].shape[0], 3 if Opt.GPU_EVALSTRIDE in slots else 1)
    members = np.bincount(inputs[5][users], minlength=3)
    assert [int(m) for _, m, *_ in re.findall(GROUP, out)[:3]] == members.tolist()
    assert (cells[:, :3, 6] <= members[None, :]).all() and cells[:, 3, 6].max() <= users.size


def test_slim_mselect_and_the_python_call(inputs, capfd, tmp_path):
    from slim_amd import SLIM, SLIMatrix
    from slim_amd.io import write_csr_text
    _, _, _, R, T, groups = inputs
    files = [str(tmp_path / f) for f in ("trn.csr", "tst.csr", "l12")]
    write_csr_text(files[0], R)
    write_csr_text(files[1], T)
    open(files[2], "w").write("".join("%g %g\n" % p for p in PAIRS))

    def cli(*options):
        return subprocess.run([MSELECT, "-nomodels", "-niters=200"] + list(options) + files, capture_output=True,
                              text=True, cwd=str(tmp_path), timeout=280)

    def python(**kw):
        trainmat = SLIMatrix(R)
        model = SLIM()
        params = {"dbglvl": 0, "algo": "cd", "nthreads": 1, "optTol": 1e-7, "niters": 200}
        try:
            wide = sp.csr_matrix((T.data, T.indices, T.indptr), shape=R.shape)
            model.mselect(params, trainmat, SLIMatrix(wide, trainmat), L1, L2, nrcmds=10, **kw)
            return model, None
        except RuntimeError as e:
            return model, str(e)
    # bands in which every group has users
    p = cli("-evalhistbands=40,100", "-evalselectgroup=0")
    assert p.returncode == 0, p.stdout + p.stderr
    model, err = python(history_bands=BOUNDS, select_group=0)
    assert err is None, err
    lines = re.findall(GROUP, p.stdout)
    assert len(lines) == 12 and len(model.last_groups) == 4
    members = np.bincount(groups, minlength=3)
    for at, pair in enumerate(model.last_groups):
        assert [r["group"] for r in pair] == [0, 1, 2, -1]
        for g in range(3):
            r = pair[g]
            assert lines[3 * at + g] == (str(g), str(members[g]), "%.4f" % r["hr"], "%.4f" % r["hr_head"],
                                         "%.4f" % r["hr_tail"], "%.4f" % r["arhr"], str(r["nvalid"]))
    l1, l2, hr, _ = model.mselect_result["bestHR"]
    a1, a2, _, ar = model.mselect_result["bestAR"]
    assert "best hr: %.4f at l1 %.4g l2 %.4g; best arhr: %.4f at l1 %.4g l2 %.4g\n" % (hr, l1, l2, ar, a1, a2) in p.stdout
    assert hr == max(pair[0]["hr"] for pair in model.last_groups)
    # the same groups from a file, and as an array: the same lines, the same choice
    gfile = str(tmp_path / "groups")
    open(gfile, "w").write("".join("%d\n" % g for g in groups))
    q = cli("-evalgroupfile=" + gfile, "-evalselectgroup=0")
    assert q.returncode == 0 and re.findall(GROUP, q.stdout) == lines
    assert re.findall(r"best hr: [^\n]*", q.stdout) == re.findall(r"best hr: [^\n]*", p.stdout)
    by_array, err = python(groups=groups, select_group=0)
    assert err is None and by_array.last_groups == model.last_groups
    assert by_array.mselect_result == model.mselect_result
    capfd.readouterr()
    # bands 5,20 on these rows: nobody has under 5 items, so group 0 is empty.  The first pair's lines say so, and
    # both doors end there, at the same pair: no pair can be chosen on a group without a valid user
    p = cli("-evalhistbands=5,20", "-evalselectgroup=0")
    short = int((np.diff(R.indptr) < 20).sum())
    lines = re.findall(GROUP, p.stdout)
    assert p.returncode == 1 and len(lines) == 3 and short > 0, p.stdout + p.stderr
    assert lines[0] == ("0", "0", "0.0000", "0.0000", "0.0000", "0.0000", "0")
    assert lines[1][:2] == ("1", str(short)) and lines[2][:2] == ("2", str(R.shape[0] - short))
    assert p.stdout.count("l1r: ") == 1 and "l1r: 1.00e+00 l2r: 1.00e+00" in p.stdout and "best hr" not in p.stdout
    assert p.stderr == "Group 0 has no evaluated user with a test row: no pair can be chosen on it.\n"
    model, err = python(history_bands=(5, 20), select_group=0)
    assert err is not None and "l1=1.0000, l2=1.0000" in err and model.last_groups is None
    # chosen on everybody, the same bands run through: the lines of group 0 stay zeros
    p = cli("-evalhistbands=5,20")
    lines = re.findall(GROUP, p.stdout)
    assert p.returncode == 0 and len(lines) == 12
    assert all(lines[3 * at] == ("0", "0", "0.0000", "0.0000", "0.0000", "0.0000", "0") for at in range(4))
