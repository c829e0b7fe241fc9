"""The transfer contract and the refusals of the per-group evaluation (include/slim_gpu_groups.h): from the second
evaluation after the groups were set nothing is allocated and nothing goes up, the group rows add 32 bytes per cutoff
and group to what comes down; a refusal leaves the eval set as it was."""
import ctypes as C

import numpy as np
import pytest

from group_cases import Data, assert_rows_equal, edge_groups, leave_out, ratings
from slim_amd import _lib
from slim_amd.constants import SLIM_ERROR_INPUT, SLIM_OK

pytestmark = pytest.mark.gpu
P = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
SIZES = (0, 1, 63, 64, 65)


@pytest.fixture(scope="module")
def synth():
    R, T = leave_out(ratings(300, 200, 0.08, seed=3), seed=4, per_user=2)
    d = Data(R, T)
    yield d
    d.close()


@pytest.mark.parametrize("cutoffs", [(10,), (5, 10, 20, 64), (1, 5, 10, 20, 64, 100, 127, 128)],
                         ids=["one", "four", "eight"])
@pytest.mark.parametrize("ngroups_extra", [0, 58], ids=["six-groups", "64-groups"])
def test_transfers_of_the_lists_path(synth, cutoffs, ngroups_extra):
    groups, ngroups = edge_groups(synth.nusers, seed=3, sizes=SIZES)
    ngroups += ngroups_extra        # (further groups without members)
    K = len(cutoffs)
    ev = synth.evaluator(cutoffs=cutoffs)
    try:
        ev.evaluate_at(synth.model)
        ev.evaluate_at(synth.model)
        plain = ev.stats()
        assert plain["d2h_bytes"] == 8 + 32 * K and plain["device_allocs"] == 0 and plain["h2d_bytes"] == 0
        ev.set_groups(groups, ngroups)
        ev.evaluate_at(synth.model)
        ev.evaluate_at(synth.model)
        st = ev.stats()
        print(plain, st)
        assert st["device_allocs"] == 0 and st["h2d_bytes"] == 0
        assert st["d2h_bytes"] == plain["d2h_bytes"] + 32 * K * ngroups
        assert st["path"] == plain["path"] and st["w_rows_read"] == plain["w_rows_read"]
    finally:
        ev.close()


def test_transfers_of_the_ranked_path(synth):
    groups, ngroups = edge_groups(synth.nusers, seed=3, sizes=SIZES)
    cut = (1, 2, 5, 10, 20, 50, 100, 128, 150, 199)
    ev = synth.evaluator(ranked=True)
    try:
        ev.evaluate_ranked(synth.model, cut)
        ev.evaluate_ranked(synth.model, cut)
        plain = ev.stats()
        ev.set_groups(groups, ngroups)
        ev.evaluate_ranked(synth.model, cut)
        ev.evaluate_ranked(synth.model, cut)
        st = ev.stats()
        assert st["device_allocs"] == 0 and st["h2d_bytes"] == 0
        assert st["d2h_bytes"] == plain["d2h_bytes"] + 32 * len(cut) * ngroups
    finally:
        ev.close()


def test_refusals_leave_the_eval_set_usable(synth):
    lib = _lib.load()
    groups, ngroups = edge_groups(synth.nusers, seed=3, sizes=SIZES)
    ev = synth.evaluator(cutoffs=(10,))
    h = ev.handle

    def refused(rc, name):
        return rc == SLIM_ERROR_INPUT and _lib.last_error().startswith(name + ": ")
    try:
        ev.set_groups(groups, ngroups)
        ev.evaluate_at(synth.model)
        before = ev.group_figures()
        bad = groups.copy()
        bad[17] = ngroups
        low = groups.copy()
        low[0] = -2
        name = "SLIMGPU_EvalSetSetGroups"
        assert refused(lib.SLIMGPU_EvalSetSetGroups(h, ngroups, P(bad)), name)
        assert "user 17 has group %d" % ngroups in _lib.last_error()
        assert refused(lib.SLIMGPU_EvalSetSetGroups(h, ngroups, P(low)), name)
        assert refused(lib.SLIMGPU_EvalSetSetGroups(h, 0, P(groups)), name)
        assert refused(lib.SLIMGPU_EvalSetSetGroups(h, _lib.MAX_GROUPS + 1, P(groups)), name)
        assert refused(lib.SLIMGPU_EvalSetSetGroups(h, -5, P(groups)), name)
        assert refused(lib.SLIMGPU_EvalSetSetGroups(h, 2 ** 31 - 1, P(groups)), name)
        assert refused(lib.SLIMGPU_EvalSetSetGroups(h, ngroups, None), name)
        assert refused(lib.SLIMGPU_EvalSetSetGroups(None, ngroups, P(groups)), name)
        name = "SLIMGPU_EvalSetSetHistoryBands"
        for bounds in ([5, 5], [5, 2], [0, 3], [-1]):
            b = np.array(bounds, np.int32)
            assert refused(lib.SLIMGPU_EvalSetSetHistoryBands(h, b.size, P(b)), name), bounds
        b = np.arange(1, _lib.MAX_GROUPS + 1, dtype=np.int32)
        assert refused(lib.SLIMGPU_EvalSetSetHistoryBands(h, b.size, P(b)), name)       # 1025 groups
        assert refused(lib.SLIMGPU_EvalSetSetHistoryBands(h, 0, P(b)), name)
        assert refused(lib.SLIMGPU_EvalSetSetHistoryBands(h, 2, None), name)
        met, nv = np.zeros(4 * (ngroups + 1)), np.zeros(3 * (ngroups + 1), np.int32)
        name = "SLIMGPU_EvalSetLastGroupFigures"
        assert refused(lib.SLIMGPU_EvalSetLastGroupFigures(h, 2, P(met), P(nv)), name)
        assert refused(lib.SLIMGPU_EvalSetLastGroupFigures(h, 1, None, P(nv)), name)
        for n in (0, -3, 33, 2 ** 31 - 1):
            assert refused(lib.SLIMGPU_EvalSetLastGroupFigures(h, n, P(met), P(nv)), name), n
        assert not met.any() and not nv.any()
        # the groups that were set still stand, with the rows they gave
        n = C.c_int32(0)
        assert lib.SLIMGPU_EvalSetGroupInfo(h, C.byref(n), None) == SLIM_OK and n.value == ngroups
        after = ev.group_figures()
        for g in range(ngroups + 1):
            assert_rows_equal(after[g], before[g], "group %d" % g)
        ev.evaluate_at(synth.model)
        again = ev.group_figures()
        for g in range(ngroups + 1):
            assert_rows_equal(again[g], before[g], "group %d, evaluated again" % g)
        # the bands at their limit: 1023 bounds, 1024 groups
        b = np.arange(1, _lib.MAX_GROUPS, dtype=np.int32)
        assert lib.SLIMGPU_EvalSetSetHistoryBands(h, b.size, P(b)) == SLIM_OK, _lib.last_error()
        assert lib.SLIMGPU_EvalSetGroupInfo(h, C.byref(n), None) == SLIM_OK and n.value == _lib.MAX_GROUPS
        ev.clear_groups()
        assert refused(lib.SLIMGPU_EvalSetGroupInfo(h, C.byref(n), None), "SLIMGPU_EvalSetGroupInfo")
        assert refused(lib.SLIMGPU_EvalSetLastGroupFigures(h, 1, P(met), P(nv)), "SLIMGPU_EvalSetLastGroupFigures")
    finally:
        ev.close()
