"""Per-group figures from the one scoring pass of an evaluation (include/slim_gpu_groups.h), the lists path:
SLIMGPU_ModelEvaluateAt with groups set against the same call on an eval set made for each group's users
(tests/group_cases.py has the yardstick).  Bit for bit: float64 metrics by np.array_equal, counts exactly."""
import numpy as np
import pytest

from group_cases import (Data, assert_rows_equal, check_group_rows, edge_groups, evaluated_members, figures,
                         leave_out, ratings, without_rows)

pytestmark = pytest.mark.gpu

ONE = (10,)
EIGHT = (1, 5, 10, 20, 64, 100, 127, 128)     # every slot of an eval set; the chunk path ends at 64, the wave path serves
SYNTH_SIZES = (0, 1, 63, 64, 65)              # (300 users have no room for a group of 128 beside these)


@pytest.fixture(scope="module")
def ml(ml100k):
    d = Data(ml100k[0], without_rows(ml100k[1]))
    yield d
    d.close()


@pytest.fixture(scope="module")
def synth():
    R, T = leave_out(ratings(300, 200, 0.08, seed=3), seed=4, per_user=2)
    d = Data(R, without_rows(T))
    yield d
    d.close()


def run(data, groups, ngroups, cutoffs, users=None, only=None):
    ev = data.evaluator(cutoffs=cutoffs, users=users)
    try:
        ev.set_groups(groups, ngroups)
        return check_group_rows(data, ev, groups, ngroups, lambda e: e.evaluate_at(data.model), cutoffs, users=users,
                                only=only)
    finally:
        ev.close()


@pytest.mark.parametrize("cutoffs", [ONE, EIGHT], ids=["one", "eight"])
def test_edge_sizes_on_ml100k(ml, cutoffs):
    assert ml.R.shape == (934, 1683)        # (the golden ml100k split: users with a held-out item)
    groups, ngroups = edge_groups(ml.nusers, seed=11)
    sizes = np.bincount(groups[groups >= 0], minlength=ngroups).tolist()
    assert sizes[:6] == [0, 1, 63, 64, 65, 128] and sizes[6] == 934 - 37 - 321 and (groups == -1).sum() == 37
    for g in range(2, ngroups):     # users without a test row are spread through every group (of more than one)
        m = evaluated_members(groups, g)
        assert (~ml.has_test[m]).any() and ml.has_test[m].any(), g
    own, rows = run(ml, groups, ngroups, cutoffs)
    assert own[-1]["hr"] > 0 and sum(r[-1]["hr"] > 0 for r in rows[:ngroups]) >= 4


@pytest.mark.parametrize("cutoffs", [ONE, EIGHT], ids=["one", "eight"])
def test_edge_sizes_on_the_synthetic_matrix(synth, cutoffs):
    assert synth.R.shape == (300, 200) and set(np.unique(synth.R.data)) <= {1.0, 2.0, 3.0, 4.0, 5.0}
    assert np.diff(synth.T.indptr).max() == 2
    groups, ngroups = edge_groups(synth.nusers, seed=13, sizes=SYNTH_SIZES)
    own, _ = run(synth, groups, ngroups, cutoffs)
    assert own[-1]["nvalid"] > 200


def test_the_everybody_row_is_the_ungrouped_call(ml):
    groups, ngroups = edge_groups(ml.nusers, seed=11)
    ev = ml.evaluator(cutoffs=EIGHT)
    try:
        plain = ev.evaluate_at(ml.model)
        ev.set_groups(groups, ngroups)
        grouped = ev.evaluate_at(ml.model)
        assert_rows_equal(grouped, plain, "grouped call, own output")
        assert_rows_equal(ev.group_figures()[ngroups], plain, "row of everybody")
        last = ev.evaluate(ml.model)         # SLIMGPU_ModelEvaluate: all the eval set's cutoffs are formed
        assert figures(last)[0].tolist() == figures(plain[-1])[0].tolist()
        assert_rows_equal(ev.group_figures()[ngroups], plain, "after evaluate()")
    finally:
        ev.close()


def test_groups_go_by_user_id_on_a_strided_eval_set(ml):
    """Every 3rd user is evaluated, so position q holds user 3q.  The group under test is made of users 3q >= 3 only:
    each sits at a position that is not its id, and the positions 3q themselves belong to other users' groups."""
    users = np.arange(0, ml.nusers, 3, dtype=np.int32)
    groups = np.full(ml.nusers, 1, np.int32)
    chosen = users[5::2]                   # user ids; their positions are 5, 7, ...: never equal to the ids
    groups[chosen] = 0
    groups[np.arange(1, ml.nusers, 3)] = 2          # never evaluated: an empty group on this eval set
    groups[users[:3]] = -1
    assert (chosen != np.arange(users.size)[5::2]).all()
    # grouping by position would read groups[q]: a different set of positions, hence different rows
    by_position = np.flatnonzero(groups[:users.size] == 0)
    assert by_position.tolist() != np.flatnonzero(groups[users] == 0).tolist()
    own, rows = run(ml, groups, 3, EIGHT, users=users)
    assert rows[0][0]["members"] == chosen.size and rows[2][0]["members"] == 0
    assert rows[0][-1]["nvalid"] > 0


def test_one_group_holding_everybody(synth):
    groups = np.zeros(synth.nusers, np.int32)
    ev = synth.evaluator(cutoffs=EIGHT)
    try:
        ev.set_groups(groups, 1)
        own = ev.evaluate_at(synth.model)
        rows = ev.group_figures()
        assert_rows_equal(rows[0], own, "the one group")
        assert_rows_equal(rows[1], own, "everybody")
    finally:
        ev.close()


def test_1024_groups_on_160_users(ml):
    """One user per group for the first 160 groups, 864 empty ones; an eval set of 160 listed users."""
    users = np.arange(3, 3 + 5 * 160, 5, dtype=np.int32)
    groups = np.full(ml.nusers, -1, np.int32)
    groups[users] = np.random.default_rng(5).permutation(160)
    sampled = np.random.default_rng(6).choice(160, size=16, replace=False).tolist()
    own, rows = run(ml, groups, 1024, ONE, users=users, only=sampled)
    assert len(rows) == 1025
    for g in range(160, 1024):           # (check_group_rows has compared every empty group with zeros; once more)
        assert figures(rows[g][0])[0].tolist() == [0.0] * 4 and figures(rows[g][0])[1] == [0, 0, 0]
    assert sum(rows[g][0]["nvalid"] for g in range(160)) == own[0]["nvalid"]


def test_history_bands(ml):
    lengths = np.diff(ml.R.indptr)
    bounds = np.array([2, 5, 20, 100, int(lengths.max()) + 1], np.int32)    # the last band stays empty
    want_groups = np.searchsorted(bounds, lengths, side="right").astype(np.int32)
    ev = ml.evaluator(cutoffs=EIGHT)
    try:
        ev.set_history_bands(bounds)
        members = ev.group_members()
        assert members.tolist() == np.bincount(want_groups, minlength=6).tolist() + [ml.nusers]
        assert members[5] == 0 and (members[:5] > 0).sum() >= 3
        ev.evaluate_at(ml.model)
        banded = ev.group_figures()
        ev.set_groups(want_groups, 6)
        ev.evaluate_at(ml.model)
        listed = ev.group_figures()
        for g in range(7):
            assert_rows_equal(banded[g], listed[g], "band %d" % g)
    finally:
        ev.close()
    # ... and on listed users: the length is that of the user, not of the position
    users = np.arange(1, ml.nusers, 4, dtype=np.int32)
    ev = ml.evaluator(cutoffs=ONE, users=users)
    try:
        ev.set_history_bands(bounds[:4])
        assert ev.group_members().tolist() == np.bincount(want_groups[users], minlength=5).tolist() + [users.size]
    finally:
        ev.close()


def test_set_twice_then_clear(synth):
    first, n1 = edge_groups(synth.nusers, seed=21, sizes=SYNTH_SIZES)
    second = (np.arange(synth.nusers) % 3).astype(np.int32)
    ev = synth.evaluator(cutoffs=ONE)
    try:
        plain = ev.evaluate_at(synth.model)
        ev.evaluate_at(synth.model)
        plain_stats = ev.stats()
        ev.set_groups(first, n1)
        with pytest.raises(RuntimeError, match="no evaluation has run"):
            ev.group_figures()
        ev.set_groups(second, 3)             # the second assignment rules
        check_group_rows(synth, ev, second, 3, lambda e: e.evaluate_at(synth.model), ONE)
        with pytest.raises(RuntimeError, match="cutoffs"):
            ev.group_figures((5, 10))
        ev.clear_groups()
        with pytest.raises(RuntimeError, match="no groups are set"):
            ev.group_figures()
        again = ev.evaluate_at(synth.model)
        st = ev.stats()
        assert_rows_equal(again, plain, "after clear_groups")
        assert st["d2h_bytes"] == plain_stats["d2h_bytes"] == 8 + 32 and st["device_allocs"] == 0
        assert st["h2d_bytes"] == 0
    finally:
        ev.close()
