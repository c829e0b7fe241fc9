"""Sampled negatives without a device (include/slim_gpu_sample.h): SLIMGPU_CandSetSample's rows, read back through
SLIMGPU_CandSetRows, against the numpy restatement of the header's text (tests/sampled_cases.py), bit for bit; the
refusals; the Python layer."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from filtered_cases import NO_HISTORY, cases_fixture, wrap
from sampled_cases import DENSE, GRID, P, csr, held_out_rows, host_sample, rule, sampled_rows, set_rows
from slim_amd import _lib
from slim_amd.constants import SLIM_ERROR_INPUT, SLIM_OK, SLIMGPU_MAX_LIST, Opt

cases = pytest.fixture(scope="module")(cases_fixture)
NAMES = {"SLIMGPU_EvalSetSampleCandidates", "SLIMGPU_CandSetSample", "SLIMGPU_CandSetRows", "SLIMGPU_CandSetInfo"}


def test_the_names_are_declared_exported_and_bound():
    text = open(os.path.join(ROOT, "include", "slim_gpu_sample.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b((?:Py|SLIMGPU)_\w+)\s*\(", text))
    assert declared == NAMES == set(_lib.SAMPLE_SYMBOLS)
    raw = C.CDLL(_lib.LIB_PATH)
    for name in declared:
        assert hasattr(raw, name), "libslim.so does not export %s" % name
    cand = open(os.path.join(ROOT, "include", "slim_gpu_cand.h")).read()
    assert '#include "slim_gpu_sample.h"' in cand
    assert re.search(r"SLIM_OPTION_GPU_EVALNEGS = 23\b", cand) and re.search(r"SLIM_OPTION_GPU_EVALSEED = 24\b", cand)
    assert Opt.GPU_EVALNEGS == 23 and Opt.GPU_EVALSEED == 24
    for other in (_lib.EXPORTED_SYMBOLS, _lib.EVAL_SYMBOLS, _lib.EVAL_AT_SYMBOLS, _lib.PLANES_SYMBOLS, _lib.RANK_SYMBOLS,
                  _lib.LIST_SYMBOLS, _lib.FILTER_SYMBOLS, _lib.FILTERED_EVAL_SYMBOLS, _lib.CAND_SYMBOLS):
        assert not declared & set(other)


def check_rows(got, want, R, ncols, nnegs):
    """Bit-equal to numpy's, and what the rule promises of any sampler: distinct, eligible negatives."""
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    assert got[0].dtype == np.int64 and got[1].dtype == np.int32


@pytest.mark.parametrize("name", ["floats", "ties", "wide"])
def test_host_rows_equal_the_restatement(cases, name):
    c = cases(name)
    T = held_out_rows(c, seed=91)
    ht = wrap(c.lib, T)
    tptr, tind = T.indptr.astype(np.int64), T.indices
    grid = GRID + (DENSE if c.ncols == 1500 else ())
    try:
        for nnegs in grid:
            want = sampled_rows(c.R, tptr, tind, c.ncols, nnegs, seed=5)
            rc, cs = host_sample(c.lib, c.ncols, c.hr, ht, nnegs, 5)
            assert rc == SLIM_OK, _lib.last_error()
            got = set_rows(c.lib, cs)
            c.lib.SLIMGPU_CandSetFree(cs)
            assert got[2] == c.ncols
            check_rows(got, want, c.R, c.ncols, nnegs)
            # what the rows must look like, whoever made them
            E = []
            for u in range(c.nusers):
                row = want[1][want[0][u]:want[0][u + 1]]
                t = tind[tptr[u]:tptr[u + 1]]
                if t.size == 0:
                    assert row.size == 0
                    continue
                hist = c.R.indices[c.R.indptr[u]:c.R.indptr[u + 1]]
                X = np.union1d(hist, t)
                E.append(X.size)
                neg = row[:row.size - t.size]
                assert np.array_equal(row[neg.size:], t)                    # the test row stands behind, as given
                assert neg.size == min(nnegs, c.ncols - X.size)
                assert np.unique(neg).size == neg.size and not np.isin(neg, X).any()
                assert neg.min() >= 0 and neg.max() < c.ncols
            rules = {rule(e, nnegs, c.ncols) for e in E}
            assert rules == {700: {"dense", "sparse"}, 750: {"dense"}}.get(nnegs, {"sparse"}), (nnegs, rules)
            if nnegs == 700:
                assert sum(rule(e, nnegs, c.ncols) == "dense" for e in E) > len(E) // 4
        # the matrix holds what the issue asks for
        lens = np.diff(tptr)
        assert lens[5] == 3 and (lens == 1).sum() > c.nusers // 2 and (lens == 0).sum() >= c.nusers // 10
        assert tind[tptr[7]] in c.R.indices[c.R.indptr[7]:c.R.indptr[7 + 1]]
        assert all(lens[u] == 1 and c.R.indptr[u + 1] == c.R.indptr[u] for u in NO_HISTORY if u < c.nusers)
        # two seeds, two sets; one seed, one set
        a = sampled_rows(c.R, tptr, tind, c.ncols, 99, seed=6)
        rc, cs = host_sample(c.lib, c.ncols, c.hr, ht, 99, 6)
        assert rc == SLIM_OK
        got6 = set_rows(c.lib, cs)
        c.lib.SLIMGPU_CandSetFree(cs)
        five = sampled_rows(c.R, tptr, tind, c.ncols, 99, seed=5)
        assert np.array_equal(got6[1], a[1]) and not np.array_equal(got6[1], five[1])
        assert np.array_equal(got6[0], five[0])                                      # (the same lengths)
        # a user list: the rows of the user ids, the others empty
        S = np.arange(2, c.nusers, 3, dtype=np.int32)
        want = sampled_rows(c.R, tptr, tind, c.ncols, 65, seed=5, users=S)
        rc, cs = host_sample(c.lib, c.ncols, c.hr, ht, 65, 5, users=S)
        assert rc == SLIM_OK, _lib.last_error()
        sub = set_rows(c.lib, cs)
        c.lib.SLIMGPU_CandSetFree(cs)
        check_rows(sub, want, c.R, c.ncols, 65)
        full = sampled_rows(c.R, tptr, tind, c.ncols, 65, seed=5)
        for u in range(c.nusers):
            row = sub[1][sub[0][u]:sub[0][u + 1]]
            if u in set(S.tolist()):
                assert np.array_equal(row, full[1][full[0][u]:full[0][u + 1]])      # (the user id, not the position)
            else:
                assert row.size == 0
    finally:
        c.lib.Py_csr_free(ht)


def test_a_hand_made_matrix_at_the_edges_of_both_rules():
    """40 items, nnegs = 5.  E counts the history united with the test row.  User 0: free = 0.  User 1: free = 4 =
    nnegs - 1.  User 2: E = 15, exactly 2 * (E + nnegs) = ncols, the last sparse user.  User 3: E = 16, one past it.
    User 4: no test row.  User 5: an empty history, a test id twice and one beyond the catalogue."""
    lib = _lib.load()
    ncols, nnegs = 40, 5
    hist = [list(range(39)), list(range(0, 35)), list(range(10, 24)), list(range(10, 25)), [1, 2, 3], []]
    test = [[39], [35, 3], [30], [30], [], [7, 7, 44]]
    R, T = csr(hist, ncols), csr(test, ncols + 5)
    E = [np.union1d(h, [t for t in tt if t < ncols]).size for h, tt in zip(hist, test)]
    assert E[:4] == [40, 36, 15, 16]
    assert [rule(e, nnegs, ncols) for e in E[:4]] == ["dense", "dense", "sparse", "dense"]
    assert 2 * (E[2] + nnegs) == ncols
    hr, ht = wrap(lib, R, binary=True), wrap(lib, T, binary=True)
    try:
        for seed in (1, 2, 2 ** 63 + 11):
            want = sampled_rows(R, T.indptr.astype(np.int64), T.indices, ncols, nnegs, seed)
            rc, cs = host_sample(lib, ncols, hr, ht, nnegs, seed)
            assert rc == SLIM_OK, _lib.last_error()
            got = set_rows(lib, cs)
            lib.SLIMGPU_CandSetFree(cs)
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), seed
            assert np.diff(want[0]).tolist() == [0 + 1, 4 + 2, 5 + 1, 5 + 1, 0, 5 + 3]
            assert sorted(want[1][want[0][1]:want[0][1] + 4].tolist()) == [36, 37, 38, 39]    # free < nnegs: all of it
            assert want[1][-3:].tolist() == [7, 7, 44]
    finally:
        lib.Py_csr_free(hr)
        lib.Py_csr_free(ht)


def test_refusals_leave_out_untouched(cases):
    c = cases("floats")
    T = held_out_rows(c, seed=91)
    ht = wrap(c.lib, T)
    long_t = T.copy()
    long_t.indices = np.concatenate([np.arange(9, dtype=np.int32), T.indices])      # user 0: ten test entries
    long_t.indptr = T.indptr.copy()
    long_t.indptr[1:] += 9
    long_t.data = np.ones(long_t.indices.size, np.float32)
    hl = wrap(c.lib, long_t)
    SENTINEL = 0x5A5A
    try:
        def refused(word, ncols=c.ncols, t=ht, nnegs=99, users=None, nusers=None):
            h = C.c_void_p(SENTINEL)
            u = None if users is None else np.ascontiguousarray(users, np.int32)
            n = (0 if u is None else u.size) if nusers is None else nusers
            rc = c.lib.SLIMGPU_CandSetSample(ncols, c.hr, t, n, P(u), nnegs, 1, C.byref(h))
            assert rc == SLIM_ERROR_INPUT and h.value == SENTINEL, (word, rc)
            assert "SLIMGPU_CandSetSample" in _lib.last_error() and word in _lib.last_error(), _lib.last_error()
        refused("nnegs", nnegs=0)
        refused("nnegs", nnegs=-1)
        refused("ncols", ncols=0)
        refused(str(SLIMGPU_MAX_LIST), nnegs=SLIMGPU_MAX_LIST)                  # + a test row of one entry
        refused(str(SLIMGPU_MAX_LIST), nnegs=SLIMGPU_MAX_LIST - 9, t=hl)        # + user 0's ten
        refused("ascend", users=[4, 4])
        refused("outside", users=[0, c.nusers])
        refused("nusers", nusers=3)
        assert c.lib.SLIMGPU_CandSetSample(c.ncols, c.hr, ht, 0, None, 99, 1, None) == SLIM_ERROR_INPUT
        # the longest SELECTED test row counts: without user 0 the same nnegs is served
        h = C.c_void_p()
        S = np.arange(1, 40, dtype=np.int32)
        assert c.lib.SLIMGPU_CandSetSample(c.ncols, c.hr, hl, S.size, P(S), SLIMGPU_MAX_LIST - 9, 1, C.byref(h)) \
            == SLIM_OK, _lib.last_error()
        ptr, ind, _ = set_rows(c.lib, h)
        c.lib.SLIMGPU_CandSetFree(h)
        # (1 500 items: every user is dense and gets every free item, fewer than nnegs)
        assert ptr[1] == 0 and 0 < ptr[2] - ptr[1] < SLIMGPU_MAX_LIST - 9
        assert c.lib.SLIMGPU_CandSetRows(None, None, None) == SLIM_ERROR_INPUT
        assert c.lib.SLIMGPU_CandSetInfo(None, None, None, None) == SLIM_ERROR_INPUT
    finally:
        c.lib.Py_csr_free(ht)
        c.lib.Py_csr_free(hl)


def test_the_python_layer_and_the_host_scorer(cases, monkeypatch):
    """sample_candidates / CandidateSet.from_handle / .rows(), and a sampled set through the existing host scorer."""
    from candidate_cases import buffers, check_lists, check_slot_scores, yardstick
    from slim_amd.engine import CandidateSet, sample_candidates
    c = cases("ties")
    T = held_out_rows(c, seed=91)
    want = sampled_rows(c.R, T.indptr.astype(np.int64), T.indices, c.ncols, 99, seed=3)
    cset = sample_candidates(c.R, T, 99, seed=3, ncols=c.ncols)
    try:
        assert isinstance(cset, CandidateSet) and cset.ncols == c.ncols and cset.nusers == c.nusers
        assert cset.size == want[1].size and np.array_equal(cset.indptr, want[0])
        ptr, ind = cset.rows()
        assert np.array_equal(ptr, want[0]) and np.array_equal(ind, want[1])
        monkeypatch.setenv("SLIM_PREDICT", "cpu")
        order = yardstick(c, ptr, ind)
        bufs = buffers(ptr, c.nusers, 10)
        assert c.lib.Py_SLIM_ScoreCandidates(c.hw, c.hr, cset.handle, 10, *[P(b) for b in bufs]) == SLIM_OK
        check_slot_scores(bufs[0], ptr, ind, order, range(c.nusers), c.nusers)
        check_lists(bufs, ptr, order, range(c.nusers), 10)
    finally:
        cset.close()
    with pytest.raises(ValueError, match="nnegs"):
        sample_candidates(c.R, T, 0)
