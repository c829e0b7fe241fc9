"""Explanations on the device (include/slim_gpu_explain.h): SLIMGPU_ExplainCandidates,
SLIMGPU_MatrixExplainCandidates and ResidentModel.explain_lists.

The yardstick is never the code under test: numpy over the case's scipy model (tests/explain_cases.py, tied to the
existing 1-vs-k scorer by tests/test_explain_host.py).  Everything is compared bit for bit.

  floats / ties  1 500 x 1 500 model, 300 users, histories of about 45: rated histories / equal terms as the rule
  wide           6 000 x 6 000 model, 96 users, histories of about 300, a candidate row of 4096
  edges          200 x 200 model, histories of 0, 1, 63, 64, 65, 128, 129 and 200 in an order of their own, a stored
                 0.0 and a stored -0.0 in one column, a history that repeats items, rows of the whole catalogue
SLIM_EXPLAIN_STAGE=64 puts the histories of 65 and more across the boundary between the staged records and the ones
read in place; SLIM_EXPLAIN_FORM=16 takes the kernel with 16 places per lane where nwhy would take the one with 4.
"""
import numpy as np
import pytest

from candidate_cases import P, make_set
from explain_cases import buffers, check, explain_cases_fixture, sum_in_position_order, positions_of, untouched
from slim_amd import _lib
from slim_amd.constants import SLIM_ERROR_INPUT, SLIM_OK
from slim_amd.engine import eval_stats

pytestmark = pytest.mark.gpu
cases = pytest.fixture(scope="module")(explain_cases_fixture)
EVERY = pytest.mark.parametrize("name", ["floats", "ties", "wide", "edges"])


def host_call(c, cs, nwhy, bufs):
    return c.lib.SLIMGPU_ExplainCandidates(c.hw, c.hr, cs, nwhy, *[P(b) for b in bufs])


def matrix_call(c, cs, users, nwhy, bufs):
    u = None if users is None else np.ascontiguousarray(users, np.int32)
    return c.lib.SLIMGPU_MatrixExplainCandidates(c.model.handle, c.mat.handle, cs, 0 if u is None else u.size, P(u),
                                                 nwhy, *[P(b) for b in bufs])


def staged_users(c):
    return getattr(c, "nstaged", c.nusers)     # (edges: the history that repeats items has no staged row)


# ---- 1. both calls against the yardstick -----------------------------------------------------------------------------
@EVERY
def test_explanations_on_the_device(cases, name, monkeypatch):
    c = cases(name)
    indptr, indices, want = cases.rows(name)
    rc, cs = make_set(c.lib, c.ncols, indptr, indices)
    assert rc == SLIM_OK, _lib.last_error()
    runs = [(nwhy, stage, None) for nwhy in (1, 3, 4, 5, 16) for stage in (None, "64")]
    runs += [(nwhy, stage, "16") for nwhy in (1, 3) for stage in (None, "64")]
    try:
        for nwhy, stage, form in runs:
            for key, value in (("SLIM_EXPLAIN_STAGE", stage), ("SLIM_EXPLAIN_FORM", form)):
                if value is None:
                    monkeypatch.delenv(key, raising=False)
                else:
                    monkeypatch.setenv(key, value)
            what = "nwhy %d, stage %s, form %s" % (nwhy, stage, form)
            bufs = buffers(indptr, nwhy)
            assert host_call(c, cs, nwhy, bufs) == SLIM_OK, _lib.last_error()
            assert eval_stats(c.lib)["path"] == 6, what
            check(bufs, indptr, want, range(c.nusers), c.nusers, nwhy)
            bufs = buffers(indptr, nwhy)
            assert matrix_call(c, cs, None, nwhy, bufs) == SLIM_OK, _lib.last_error()
            assert eval_stats(c.lib)["path"] == 6, what
            check(bufs, indptr, want, range(staged_users(c)), c.nusers, nwhy)
    finally:
        c.lib.SLIMGPU_CandSetFree(cs)


# ---- 2. user lists ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["floats", "edges"])
def test_a_user_list_goes_by_user_id(cases, name):
    c = cases(name)
    indptr, indices, want = cases.rows(name)
    rc, cs = make_set(c.lib, c.ncols, indptr, indices)
    assert rc == SLIM_OK
    n = staged_users(c)
    try:
        for users in (np.arange(0, n, 3), np.array([min(5, n - 2)]), np.array([n - 1])):
            for nwhy in (3, 16):
                bufs = buffers(indptr, nwhy)
                assert matrix_call(c, cs, users, nwhy, bufs) == SLIM_OK, _lib.last_error()
                check(bufs, indptr, want, users, c.nusers, nwhy)
        # support alone
        bufs = buffers(indptr, 3)
        assert matrix_call(c, cs, np.arange(0, n, 3), 3, (None, None, bufs[2])) == SLIM_OK, _lib.last_error()
        full = buffers(indptr, 3)
        assert matrix_call(c, cs, np.arange(0, n, 3), 3, full) == SLIM_OK
        assert np.array_equal(bufs[2], full[2]) and untouched((bufs[0], bufs[1], buffers(indptr, 3)[2]))
    finally:
        c.lib.SLIMGPU_CandSetFree(cs)


# ---- 3. the device against the host loop -----------------------------------------------------------------------------
def test_the_device_equals_the_host_loop(cases, monkeypatch):
    c = cases("wide")
    indptr, indices, _ = cases.rows("wide")
    rc, cs = make_set(c.lib, c.ncols, indptr, indices)
    assert rc == SLIM_OK
    try:
        for nwhy in (3, 16):
            host = buffers(indptr, nwhy)
            monkeypatch.setenv("SLIM_PREDICT", "cpu")
            assert c.lib.Py_SLIM_ExplainCandidates(c.hw, c.hr, cs, nwhy, *[P(b) for b in host]) == SLIM_OK
            monkeypatch.setenv("SLIM_PREDICT", "gpu")
            routed = buffers(indptr, nwhy)
            assert c.lib.Py_SLIM_ExplainCandidates(c.hw, c.hr, cs, nwhy, *[P(b) for b in routed]) == SLIM_OK
            assert eval_stats(c.lib)["path"] == 6
            dev = buffers(indptr, nwhy)
            assert matrix_call(c, cs, None, nwhy, dev) == SLIM_OK, _lib.last_error()
            for got in (routed, dev):
                assert np.array_equal(got[0], host[0]) and np.array_equal(got[2], host[2])
                assert np.array_equal(got[1].view(np.int32), host[1].view(np.int32))
        assert (host[2] > 3).any() and (host[2] == 0).any()    # (slots with more terms than places, and with none)
    finally:
        c.lib.SLIMGPU_CandSetFree(cs)


# ---- 4. what a second call costs -------------------------------------------------------------------------------------
def test_the_second_call_allocates_and_uploads_nothing(cases):
    c = cases("floats")
    indptr, indices, _ = cases.rows("floats")
    rc, cs = make_set(c.lib, c.ncols, indptr, indices)
    assert rc == SLIM_OK
    try:
        for users in (None, np.arange(0, c.nusers, 3, dtype=np.int32)):
            first = buffers(indptr, 16)
            assert matrix_call(c, cs, users, 16, first) == SLIM_OK, _lib.last_error()
            st1 = eval_stats(c.lib)
            second = buffers(indptr, 16)
            assert matrix_call(c, cs, users, 16, second) == SLIM_OK
            st2 = eval_stats(c.lib)
            assert st1["device_allocs"] > 0 and st1["path"] == st2["path"] == 6
            assert st2["device_allocs"] == 0, st2
            assert st2["h2d_bytes"] == (0 if users is None else users.nbytes), st2
            assert st2["d2h_bytes"] > 0 and st2["kernel_ms"] > 0
            assert all(np.array_equal(a.view(np.int32), b.view(np.int32)) for a, b in zip(first, second))
    finally:
        c.lib.SLIMGPU_CandSetFree(cs)


# ---- 5. refusals -----------------------------------------------------------------------------------------------------
def test_refusals_leave_every_buffer_untouched(cases):
    c, other = cases("floats"), cases("edges")
    indptr, indices, _ = cases.rows("floats")
    rc, cs = make_set(c.lib, c.ncols, indptr, indices)
    assert rc == SLIM_OK
    calls = {"SLIMGPU_ExplainCandidates": lambda s, nwhy, b: host_call(c, s, nwhy, b),
             "SLIMGPU_MatrixExplainCandidates": lambda s, nwhy, b: matrix_call(c, s, None, nwhy, b)}
    try:
        for who, call in calls.items():
            for nwhy in (0, 17):
                bufs = buffers(indptr, 17)
                assert call(cs, nwhy, bufs) == SLIM_ERROR_INPUT and untouched(bufs)
                assert who in _lib.last_error() and "nwhy" in _lib.last_error()
            bufs = buffers(indptr, 3)
            assert call(cs, 3, (bufs[0], None, bufs[2])) == SLIM_ERROR_INPUT and untouched(bufs)
            assert who in _lib.last_error()
        # a matrix and a model of different widths
        bufs = buffers(indptr, 3)
        rc = c.lib.SLIMGPU_MatrixExplainCandidates(other.model.handle, c.mat.handle, cs, 0, None, 3,
                                                   *[P(b) for b in bufs])
        assert rc == SLIM_ERROR_INPUT and untouched(bufs)
        assert "SLIMGPU_MatrixExplainCandidates" in _lib.last_error() and "items" in _lib.last_error()
        # a user list that does not ascend
        bufs = buffers(indptr, 3)
        assert matrix_call(c, cs, np.array([4, 2]), 3, bufs) == SLIM_ERROR_INPUT and untouched(bufs)
    finally:
        c.lib.SLIMGPU_CandSetFree(cs)
    # a set made for another number of items, a set with too few rows
    for ncols, rows in ((c.ncols + 1, c.nusers), (c.ncols, c.nusers - 1)):
        rc, cs = make_set(c.lib, ncols, indptr[:rows + 1], indices[:indptr[rows]])
        assert rc == SLIM_OK
        try:
            for who, call in calls.items():
                bufs = buffers(indptr, 3)
                assert call(cs, 3, bufs) == SLIM_ERROR_INPUT and who in _lib.last_error() and untouched(bufs)
        finally:
            c.lib.SLIMGPU_CandSetFree(cs)


# ---- 6. lists that predict returned ----------------------------------------------------------------------------------
def test_explain_lists_adds_up_to_the_list_scores(cases):
    """The top 10 of `floats`: at nwhy = 16 the terms of every listed item, back in position order and added from
    0.0f, are the score predict returned for it, bit for bit."""
    c = cases("floats")
    ids, scores, counts = c.model.predict(c.mat, nrcmds=10, return_counts=True)
    indptr, items, terms, support = c.model.explain_lists(c.mat, ids, counts, nwhy=16)
    assert indptr[-1] == counts.sum() == support.size and items.shape == terms.shape == (support.size, 16)
    checked = 0
    for u in range(c.nusers):
        hist = c.R.indices[c.R.indptr[u]:c.R.indptr[u + 1]]
        for r in range(int(counts[u])):
            e = int(indptr[u]) + r
            n = int(support[e])
            assert n >= 1, "user %d: a listed item without a term" % u
            assert (items[e, min(n, 16):] == -1).all() and (terms[e, min(n, 16):] == 0).all()
            if n > 16:
                continue
            s = sum_in_position_order(positions_of(hist, items[e, :n]), terms[e, :n])
            assert np.float32(s).view(np.int32) == scores[u, r].view(np.int32), "user %d rank %d" % (u, r)
            checked += 1
    assert checked > 10 * c.nusers // 2
    # a user list: the same explanations, position by position
    users = np.arange(1, c.nusers, 4, dtype=np.int32)
    ids2, _, counts2 = c.model.predict(c.mat, nrcmds=10, users=users, return_counts=True)
    indptr2, items2, terms2, support2 = c.model.explain_lists(c.mat, ids2, counts2, nwhy=16, users=users)
    for q, u in enumerate(users):
        a, b = slice(int(indptr[u]), int(indptr[u + 1])), slice(int(indptr2[q]), int(indptr2[q + 1]))
        assert np.array_equal(items[a], items2[b]) and np.array_equal(support[a], support2[b])
        assert np.array_equal(terms[a].view(np.int32), terms2[b].view(np.int32))
