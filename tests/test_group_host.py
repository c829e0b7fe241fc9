"""User groups without a device (include/slim_gpu_groups.h): SLIMGPU_GroupPartition, the definition in code, against
a numpy stable argsort; the names; every refusal that needs no GPU -- the partition's, Py_SLIM_MselectGrouped's and
the Python argument checks."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import scipy.sparse as sp

from conftest import ROOT
from filtered_cases import wrap
from slim_amd import _lib
from slim_amd.constants import SLIM_ALGO, SLIM_ERROR_INPUT, SLIM_NOPTIONS, SLIM_OK, Opt
from slim_amd.engine import group_partition

P = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)  # noqa: E731


def test_the_names_are_declared_exported_and_bound():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "slim_gpu_groups.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b((?:SLIMGPU|Py_SLIM)_\w+)\s*\(", text))
    assert declared == set(_lib.GROUP_SYMBOLS) and len(declared) == 10
    raw = C.CDLL(_lib.LIB_PATH)
    for name in declared:
        assert hasattr(raw, name), "libslim.so does not export %s" % name
    assert "#define SLIMGPU_MAX_GROUPS %d\n" % _lib.MAX_GROUPS in text and _lib.MAX_GROUPS == 1024
    assert re.search(r"#define SLIMGPU_GROUP_CELL %d\b" % _lib.GROUP_CELL, text) and _lib.GROUP_CELL == 9
    assert '#include "slim_gpu_groups.h"' in open(os.path.join(ROOT, "include", "slim_gpu.h")).read()


def by_argsort(groups, ngroups, users, nsel):
    """The yardstick: a stable argsort of the positions' groups, positions of group -1 dropped."""
    g = groups[users] if users is not None else groups[:nsel]
    order = np.argsort(g, kind="stable")
    order = order[g[order] >= 0]
    offsets = np.concatenate(([0], np.cumsum(np.bincount(g[g >= 0], minlength=ngroups))))
    return order.astype(np.int32), offsets.astype(np.int64)


def draw(rng, nall, ngroups, none=0.1, upto=None):
    g = rng.integers(0, ngroups if upto is None else upto, nall).astype(np.int32)
    g[rng.random(nall) < none] = -1
    return g


@pytest.mark.parametrize("nsel", [1, 64, 65, 500])
@pytest.mark.parametrize("ngroups, upto", [(1, None), (7, None), (7, 3), (1024, None)],
                         ids=["one-group", "seven", "empty-groups", "1024"])
def test_every_user_evaluated(nsel, ngroups, upto):
    rng = np.random.default_rng(nsel * 31 + ngroups)
    groups = draw(rng, nsel, ngroups, upto=upto)
    order, offsets = group_partition(groups, ngroups)
    want_order, want_offsets = by_argsort(groups, ngroups, None, nsel)
    assert np.array_equal(order, want_order) and np.array_equal(offsets, want_offsets)
    for g in range(ngroups):        # ascending inside a group, and exactly its members
        mine = order[offsets[g]:offsets[g + 1]]
        assert np.array_equal(mine, np.flatnonzero(groups == g))
    assert offsets[-1] == (groups >= 0).sum()


@pytest.mark.parametrize("nsel", [1, 64, 65, 211])
@pytest.mark.parametrize("ngroups", [1, 5, 1024])
def test_a_listed_user_set(nsel, ngroups):
    rng = np.random.default_rng(nsel * 17 + ngroups)
    nall = 700
    groups = draw(rng, nall, ngroups)
    users = np.sort(rng.choice(nall, size=nsel, replace=False)).astype(np.int32)
    order, offsets = group_partition(groups, ngroups, users=users)
    want_order, want_offsets = by_argsort(groups, ngroups, users, nsel)
    assert np.array_equal(order, want_order) and np.array_equal(offsets, want_offsets)
    # by user id: a position is listed under the group of ITS USER
    for g in range(min(ngroups, 5)):
        assert np.array_equal(users[order[offsets[g]:offsets[g + 1]]], users[groups[users] == g])


def test_the_first_rows_only_and_nobody_in_a_group():
    groups = np.array([2, -1, 0, 2, 1, 0, 0], np.int32)
    order, offsets = group_partition(groups, 3, nsel=4)
    assert order.tolist() == [2, 0, 3] and offsets.tolist() == [0, 1, 1, 3]
    order, offsets = group_partition(np.full(9, -1, np.int32), 4)
    assert order.size == 0 and offsets.tolist() == [0] * 5
    # the worked example of the header
    g = np.array([1, 0, 0, 2, 0, 0, -1, 0, 0, 1, 0, 0, 1], np.int32)
    order, offsets = group_partition(g, 3, users=[0, 3, 6, 9, 12])
    assert order.tolist() == [0, 3, 4, 1] and offsets.tolist() == [0, 0, 3, 4]


def test_the_partition_refuses_and_writes_nothing():
    lib = _lib.load()
    groups = np.array([0, 1, 2, 1], np.int32)
    users = np.array([0, 2], np.int32)

    def refused(nsel, users_, nall, ngroups, g, word):
        order, offsets = np.full(8, 7, np.int32), np.full(2000, 7, np.int64)
        rc = lib.SLIMGPU_GroupPartition(nsel, P(users_), nall, ngroups, P(g), P(order), P(offsets))
        text = _lib.last_error()
        print(text)
        return (rc == SLIM_ERROR_INPUT and text.startswith("SLIMGPU_GroupPartition: ") and word in text and
                (order == 7).all() and (offsets == 7).all())
    assert refused(4, None, 4, 2, groups, "user 2 has group 2, outside [-1, 2)")
    assert refused(4, None, 4, 3, np.array([0, -2, 1, 1], np.int32), "user 1 has group -2")
    assert refused(4, None, 4, 0, groups, "between 1 and 1024 groups, not 0")
    assert refused(4, None, 4, 1025, groups, "between 1 and 1024 groups, not 1025")
    assert refused(2, np.array([0, 4], np.int32), 4, 3, groups, "user 4 is outside [0, 4)")
    assert refused(5, None, 4, 3, groups, "5 positions and 4 users")
    assert refused(4, None, 4, 3, None, "bad arguments")
    # an id outside the range is refused wherever it stands, evaluated or not
    assert refused(2, users, 4, 2, groups, "user 2 has group 2")
    with pytest.raises(ValueError, match="SLIMGPU_GroupPartition"):
        group_partition(groups, 2)
    with pytest.raises(ValueError, match="one integer group per user"):
        group_partition(np.array([0.5, 1.0]), 2)


# ---- Py_SLIM_MselectGrouped: what is refused before anything is staged -------------------------------------------------
@pytest.fixture(scope="module")
def small():
    """12 users, 9 items; every user holds one item out (tests/test_grid_refusals_host.py)."""
    lib = _lib.load()
    rng = np.random.default_rng(7)
    R = sp.csr_matrix((rng.random((12, 9)) < 0.4).astype(np.float32))
    T = sp.csr_matrix((np.ones(12, np.float32), (np.arange(12), np.arange(12) % 9)), shape=(12, 9))
    trn, tst = wrap(lib, R), wrap(lib, T)
    yield lib, trn, tst, R, T
    for h in (trn, tst):
        lib.Py_csr_free(h)


def grouped(lib, trn, tst, ngroups, groups, select, slots=()):
    iopt, dopt = np.full(SLIM_NOPTIONS, -1, np.int32), np.full(SLIM_NOPTIONS, -1.0)
    iopt[Opt.ALGO], iopt[Opt.MAXNITERS] = SLIM_ALGO["cd"], 20
    for k, v in dict(slots).items():
        iopt[k] = v
    best = [C.c_double(0.0) for _ in range(8)]
    return lib.Py_SLIM_MselectGrouped(trn, tst, iopt, dopt, np.array([1.0, 2.0]), np.array([0.5]), 2, 1,
                                      *([C.byref(b) for b in best] + [None, ngroups, P(groups), select, None]))


@pytest.mark.parametrize("ngroups, groups, select, word", [
    (3, [0, 1, 2, 0, 1, 2, 0, 1, 2, 0, 1, 2], 3, "select_group 3 is outside [-1, 3)"),
    (3, [0, 1, 2, 0, 1, 2, 0, 1, 2, 0, 1, 2], -2, "select_group -2 is outside [-1, 3)"),
    (3, [0, 1, 2, 0, 1, 3, 0, 1, 2, 0, 1, 2], 0, "user 5 has group 3, outside [-1, 3)"),
    (3, [0, 1, 2, 0, 1, 2, 0, 1, 2, 0, 1, -5], 0, "user 11 has group -5"),
    (0, [0] * 12, -1, "between 1 and 1024 groups, not 0"),
    (1025, [0] * 12, -1, "between 1 and 1024 groups, not 1025"),
    (2, None, 0, "bad arguments"),
])
def test_mselect_grouped_refuses_bad_groups(small, capfd, ngroups, groups, select, word):
    lib, trn, tst = small[:3]
    capfd.readouterr()
    rc = grouped(lib, trn, tst, ngroups, None if groups is None else np.array(groups, np.int32), select)
    C.CDLL(None).fflush(None)
    out = capfd.readouterr().out
    text = _lib.last_error()
    print(text)
    assert rc == SLIM_ERROR_INPUT and text.startswith("Py_SLIM_MselectGrouped: ") and word in text
    assert "l1r:" not in out and "Estimating" not in out


def test_a_grid_without_the_evaluation_in_hbm_refuses_groups(small, capfd):
    """ADMM leaves no model in HBM and stages nothing: the grid opens, and refuses the groups before any solve."""
    lib, trn, tst = small[:3]
    groups = (np.arange(12) % 3).astype(np.int32)
    capfd.readouterr()
    rc = grouped(lib, trn, tst, 3, groups, 0, slots={Opt.ALGO: SLIM_ALGO["admm"]})
    C.CDLL(None).fflush(None)
    out = capfd.readouterr().out
    text = _lib.last_error()
    assert rc == SLIM_ERROR_INPUT and text.startswith("SLIMGPU_GridSetGroups: groups need the evaluation in HBM")
    assert "l1r:" not in out and "Estimating" not in out
    # ... and through the grid object
    iopt, dopt = np.full(SLIM_NOPTIONS, -1, np.int32), np.full(SLIM_NOPTIONS, -1.0)
    iopt[Opt.ALGO] = SLIM_ALGO["admm"]
    grid = C.c_void_p(None)
    assert lib.SLIMGPU_GridOpen(trn, tst, iopt, dopt, 0, 2, None, C.byref(grid)) == SLIM_OK
    try:
        assert lib.SLIMGPU_GridSetGroups(grid, 3, P(groups), 0) == SLIM_ERROR_INPUT
        assert "evaluation in HBM" in _lib.last_error()
        assert lib.SLIMGPU_GridSetGroups(grid, 3, P(groups), 3) == SLIM_ERROR_INPUT
        assert "select_group 3" in _lib.last_error()
        assert lib.SLIMGPU_GridSetGroups(grid, 3, None, 0) == SLIM_ERROR_INPUT
        met, nv = np.zeros(16), np.zeros(12, np.int32)
        assert lib.SLIMGPU_GridLastGroups(grid, P(met), P(nv)) == SLIM_ERROR_INPUT
        assert _lib.last_error() == "SLIMGPU_GridLastGroups: no groups are set on this grid"
        n = C.c_int32(7)
        assert lib.SLIMGPU_GridGroupInfo(grid, C.byref(n), None) == SLIM_ERROR_INPUT and n.value == 7
        assert _lib.last_error() == "SLIMGPU_GridGroupInfo: no groups are set on this grid"
        assert lib.SLIMGPU_GridGroupInfo(None, C.byref(n), None) == SLIM_ERROR_INPUT
    finally:
        lib.SLIMGPU_GridFree(C.byref(grid))


# ---- SLIM.mselect(groups=..., history_bands=..., select_group=...): the argument checks --------------------------------
def test_the_python_argument_checks(small):
    from slim_amd.interface import SLIM, SLIMatrix, _user_groups
    lib, _, _, R, T = small
    trn, tst = SLIMatrix(R), SLIMatrix(T)
    params = {"algo": "cd", "niters": 20}
    call = lambda **kw: SLIM().mselect(params, trn, tst, [1.0], [0.5], 5, **kw)  # noqa: E731
    g = (np.arange(12) % 3).astype(np.int64)
    for kw, word in (
            (dict(groups=g, history_bands=[2, 5]), "at most one of groups and history_bands"),
            (dict(select_group=0), "give groups or history_bands"),
            (dict(groups=g, select_group=3), "select_group must be a group, 0 to 2"),
            (dict(groups=g, select_group=-1), "select_group must be a group"),
            (dict(groups=g, select_group=1.0), "select_group must be a group"),
            (dict(groups=g[:11]), "one integer group per user row of trndata \\(12\\)"),
            (dict(groups=g * 0.5), "one integer group per user row"),
            (dict(groups=np.full(12, -1)), "puts no user into a group"),
            (dict(groups=g - 2), "a group must be -1"),
            (dict(groups=g + 1022), "a group must be -1"),
            (dict(groups={0: 1.5}), "integer groups"),
            (dict(history_bands=[5, 5]), "ascending integers"),
            (dict(history_bands=[0, 5]), "ascending integers"),
            (dict(history_bands=[]), "ascending integers"),
            (dict(history_bands=[2.5]), "ascending integers"),
            (dict(groups=g, exposure=True), "does not combine with groups")):
        with pytest.raises(TypeError, match=word):
            call(**kw)
    # an array as it is; a dict through the user map, unknown users ignored, unnamed users in no group; the bands
    out, n = _user_groups(lib, trn, g, None)
    assert out.dtype == np.int32 and out.tolist() == g.tolist() and n == 3
    out, n = _user_groups(lib, trn, {0: 2, 11: 0, 99: 5, -4: 1}, None)
    assert out.tolist() == [2] + [-1] * 10 + [0] and n == 3
    out, n = _user_groups(lib, trn, None, [2, 4])
    lengths = np.diff(R.indptr)
    assert out.tolist() == np.searchsorted([2, 4], lengths, side="right").tolist() and n == 3
    assert _user_groups(lib, trn, None, None) == (None, 0)
    # ids that are not row numbers: ijv triplets with a user map
    trip = SLIMatrix(np.array([[70, 5, 1.0], [30, 6, 1.0], [70, 6, 1.0], [50, 5, 1.0]]))
    out, n = _user_groups(lib, trip, {30: 1, 50: 0, 31: 4}, None)
    assert out.tolist() == [-1, 1, 0] and n == 2
