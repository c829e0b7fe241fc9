"""Per-group figures (include/slim_gpu_groups.h) through the other evaluations of an eval set: ranked, filtered,
candidate sets, exposure.  One group assignment (the kernel's edge sizes, tests/group_cases.py); every group row
against the same call on an eval set made for the group's users, bit for bit."""
import numpy as np
import pytest
import scipy.sparse as sp

from group_cases import Data, assert_rows_equal, check_group_rows, edge_groups, without_rows

pytestmark = pytest.mark.gpu

CUTOFFS = (5, 10, 100)
RANKED = (1, 2, 5, 10, 20, 50, 100, 128, 200, 500)    # ten: the terms workspace holds eight, so two slices


@pytest.fixture(scope="module")
def ml(ml100k):
    d = Data(ml100k[0], without_rows(ml100k[1]))
    d.groups, d.ngroups = edge_groups(d.nusers, seed=11)
    yield d
    d.close()


def grouped(ml, cutoffs=CUTOFFS, ranked=False):
    ev = ml.evaluator(cutoffs=cutoffs, ranked=ranked)
    ev.set_groups(ml.groups, ml.ngroups)
    return ev


def test_ranked_across_the_slice_of_eight(ml):
    ev = grouped(ml, ranked=True)
    try:
        own, rows = check_group_rows(ml, ev, ml.groups, ml.ngroups, lambda e: e.evaluate_ranked(ml.model, RANKED),
                                     CUTOFFS, ranked=True)
        assert [r["nrcmds"] for r in own] == list(RANKED)
        big = rows[6]       # (the rest: 585 users) the rows of the second slice are not those of the first
        assert big[9]["hr"] > big[7]["hr"] > big[1]["hr"] > 0
    finally:
        ev.close()


def test_filtered(ml):
    rng = np.random.default_rng(41)
    allowed = np.flatnonzero(rng.random(ml.mat.ncols) < 0.5)
    X = sp.random(ml.nusers, ml.mat.ncols, density=0.01, format="csr", random_state=rng, dtype=np.float32)
    flt = ml.mat.item_filter(allowed=allowed, exclusions=X)
    ev = grouped(ml)
    try:
        plain = ev.evaluate_at(ml.model)
        own, _ = check_group_rows(ml, ev, ml.groups, ml.ngroups, lambda e: e.evaluate_at(ml.model, filter=flt), CUTOFFS)
        assert 0 < own[-1]["hr"] < plain[-1]["hr"]
    finally:
        ev.close()
        flt.close()


def test_candidates(ml):
    ev = grouped(ml)
    cset = ev.sample_candidates(99, seed=7)
    try:
        own, _ = check_group_rows(ml, ev, ml.groups, ml.ngroups, lambda e: e.evaluate_candidates(ml.model, cset),
                                  CUTOFFS)
        assert own[0]["hr"] > 0
    finally:
        cset.close()
        ev.close()


def test_exposure(ml):
    ev = grouped(ml)
    plain = ml.evaluator(cutoffs=CUTOFFS)
    try:
        wantfig, (wantE, wantS) = plain.evaluate_exposure(ml.model)
        got = {}

        def call(e):
            fig, expo = e.evaluate_exposure(ml.model)
            got[e] = expo
            return fig
        own, _ = check_group_rows(ml, ev, ml.groups, ml.ngroups, call, CUTOFFS)
        assert_rows_equal(own, wantfig, "the accuracy rows of the grouped exposure call")
        E, S = got[ev]
        assert np.array_equal(E, wantE) and S == wantS and E.sum() > 0      # the exposure is everybody's, unchanged
    finally:
        plain.close()
        ev.close()
