"""Shared by tests/test_group_*.py: inputs and the yardstick of the per-group evaluation (include/slim_gpu_groups.h).

The yardstick is never the code under test: row (g, k) of a grouped call must equal, bit for bit, row k of the SAME
call on an eval set made for exactly the group's evaluated users (SLIMGPU_EvalSetCreateAt / CreateRanked with a user
list), entry points that existed before groups did.  Membership is restated in numpy from the group array.
"""
import numpy as np
import scipy.sparse as sp

import slim_oracle as O
from slim_amd.engine import DeviceMatrix

KEYS = ("hr", "hr_head", "hr_tail", "arhr")
NKEYS = ("nvalid", "nvalid_head", "nvalid_tail")
# the sizes at the kernel's edges (one wavefront walks a group 64 positions at a time): an empty group, one position,
# one short of a wavefront, exactly one, one more, exactly two; then the rest; 37 users in no group
EDGE_SIZES = (0, 1, 63, 64, 65, 128)
NO_GROUP = 37


def ratings(nrows, ncols, density, seed):
    rng = np.random.default_rng(seed)
    R = sp.random(nrows, ncols, density=density, format="csr", random_state=rng, dtype=np.float32)
    R.data[:] = rng.integers(1, 6, R.nnz).astype(np.float32)
    R.sort_indices()
    return R


def leave_out(R, seed, per_user=2, min_keep=1):
    """(train, test): `per_user` entries of every user with enough of them move to the test matrix."""
    rng = np.random.default_rng(seed)
    R = sp.csr_matrix(R)
    keep = np.ones(R.nnz, bool)
    for u in range(R.shape[0]):
        s, e = R.indptr[u], R.indptr[u + 1]
        if e - s >= per_user + min_keep:
            keep[s + rng.choice(e - s, size=per_user, replace=False)] = False
    rows = np.repeat(np.arange(R.shape[0]), np.diff(R.indptr))
    trn = sp.csr_matrix((R.data[keep], (rows[keep], R.indices[keep])), shape=R.shape)
    tst = sp.csr_matrix((np.ones((~keep).sum(), np.float32), (rows[~keep], R.indices[~keep])), shape=R.shape)
    trn.sort_indices()
    tst.sort_indices()
    return trn, tst


def without_rows(T, every=7, first=3):
    """T with the test rows of users first, first + every, ... emptied: users that are evaluated and not valid."""
    T = sp.lil_matrix(T)
    for u in range(first, T.shape[0], every):
        T.rows[u], T.data[u] = [], []
    T = sp.csr_matrix(T)
    T.sort_indices()
    return T


def edge_groups(nusers, seed, sizes=EDGE_SIZES, no_group=NO_GROUP):
    """(groups, ngroups): the users, shuffled, dealt to groups of `sizes`, then `no_group` users to -1, the rest to
    one last group.  Shuffled, so the members of a group lie all over the positions."""
    assert sum(sizes) + no_group < nusers
    perm = np.random.default_rng(seed).permutation(nusers)
    groups = np.full(nusers, len(sizes), np.int32)
    at = 0
    for g, n in enumerate(sizes):
        groups[perm[at:at + n]] = g
        at += n
    groups[perm[at:at + no_group]] = -1
    return groups, len(sizes) + 1


class Data(object):
    """A staged training matrix, its test rows and marker, and one resident model, made once per module."""

    def __init__(self, R, T, model=None, **learn):
        self.R, self.T = sp.csr_matrix(R), sp.csr_matrix(T)
        self.nusers = min(self.R.shape[0], self.T.shape[0])
        self.mat = DeviceMatrix.from_scipy(self.R)
        ncols = max(self.mat.ncols, int(self.T.indices.max()) + 1 if self.T.nnz else 0)
        self.fm = np.ascontiguousarray(O.head_tail(self.R, ncols), np.int32)
        opts = dict(l1r=1.0, l2r=1.0, niters=100, seed=1)
        opts.update(learn)
        self.model = self.mat.learn_resident(**opts)[0]
        self.has_test = np.diff(self.T.indptr)[:self.nusers] > 0

    def evaluator(self, cutoffs=(10,), users=None, ranked=False):
        users = None if users is None else np.ascontiguousarray(users, np.int32)
        return self.mat.evaluator(self.T, fmarker=self.fm, cutoffs=cutoffs, users=users, ranked=ranked)

    def close(self):
        self.model.free()
        self.mat.close()


def figures(row):
    return np.array([row[k] for k in KEYS]), [row[k] for k in NKEYS]


def assert_rows_equal(got, want, what=""):
    """Rows of dicts (one per cutoff): float64 metrics by np.array_equal, counts exactly."""
    assert len(got) == len(want), what
    for k, (g, w) in enumerate(zip(got, want)):
        (mg, ng), (mw, nw) = figures(g), figures(w)
        print(what, "cutoff", g["nrcmds"], "got ", mg.tolist(), ng, "want", mw.tolist(), nw)
        assert g["nrcmds"] == w["nrcmds"], what
        assert ng == nw, (what, k)
        assert mg.dtype == mw.dtype == np.float64 and np.array_equal(mg, mw), (what, k)


def evaluated_members(groups, g, users=None):
    """The evaluated users of group g, ascending: restated from the group array, by user id."""
    users = np.arange(groups.size) if users is None else np.asarray(users)
    return users[groups[users] == g].astype(np.int32)


def check_group_rows(data, ev, groups, ngroups, call, cutoffs, users=None, ranked=False, only=None):
    """`ev` has the groups set.  Runs call(ev) (a list of row dicts, one per cutoff), then checks every group row of
    ev.group_figures(): against call() on an evaluator of the group's evaluated users; zeros for an empty group; the
    row of everybody against the call's own output; the counts against each other.  Returns (own, group rows)."""
    own = call(ev)
    cut = [r["nrcmds"] for r in own]
    rows = ev.group_figures(cut)
    assert len(rows) == ngroups + 1
    nsel = data.nusers if users is None else len(users)
    assert_rows_equal(rows[ngroups], own, "everybody")
    assert all(r["members"] == nsel for r in rows[ngroups])
    totals = np.zeros((len(cut), 3), np.int64)
    for g in list(range(ngroups)) + [-1]:
        members = evaluated_members(groups, g, users)
        if g >= 0:
            assert all(r["members"] == members.size for r in rows[g]), g
        if members.size == 0:
            if g >= 0:
                for r in rows[g]:
                    assert figures(r)[0].tolist() == [0.0] * 4 and figures(r)[1] == [0, 0, 0], (g, r)
            continue
        if g >= 0 and only is not None and g not in only:
            totals += np.array([figures(r)[1] for r in rows[g]])
            continue
        sub = data.evaluator(cutoffs=cutoffs, users=members, ranked=ranked)
        try:
            want = call(sub)
        finally:
            sub.close()
        if g >= 0:
            assert_rows_equal(rows[g], want, "group %d (%d members)" % (g, members.size))
        totals += np.array([figures(r)[1] for r in want])
    assert totals.tolist() == [figures(r)[1] for r in own], "the groups and group -1 add up to everybody"
    return own, rows
