"""Popularity-weighted negatives without a device (THE WEIGHTED RULE of include/slim_gpu_sample.h):
SLIMGPU_CandSetSampleWeighted's rows, read back through SLIMGPU_CandSetRows, against the numpy restatement of the
header's text (tests/weighted_cases.py), bit for bit; the refusals; the Python layer; and that the sampler is
weighted, not merely deterministic."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from filtered_cases import cases_fixture, wrap
from sampled_cases import P, csr, held_out_rows, host_sample, sampled_rows, set_rows
from slim_amd import _lib
from slim_amd.constants import SLIM_ERROR_INPUT, SLIM_OK, Opt
from weighted_cases import (grid, hand_made, host_sample_weighted, weighted_negatives, weighted_rows, weighted_user, weights)

cases = pytest.fixture(scope="module")(cases_fixture)
NAMES = {"SLIMGPU_EvalSetSampleCandidatesWeighted", "SLIMGPU_CandSetSampleWeighted", "SLIMGPU_LastSampleKernelMs"}


def test_the_names_and_the_slot_are_declared_exported_and_bound():
    text = open(os.path.join(ROOT, "include", "slim_gpu_wsample.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b((?:Py|SLIMGPU)_\w+)\s*\(", text))
    assert declared == NAMES == set(_lib.WSAMPLE_SYMBOLS)
    raw = C.CDLL(_lib.LIB_PATH)
    for name in declared:
        assert hasattr(raw, name), "libslim.so does not export %s" % name
    sample = open(os.path.join(ROOT, "include", "slim_gpu_sample.h")).read()
    assert '#include "slim_gpu_wsample.h"' in sample and "THE WEIGHTED RULE" in sample
    assert "not built" not in sample.split("THE WEIGHTED RULE")[0]
    cand = open(os.path.join(ROOT, "include", "slim_gpu_cand.h")).read()
    assert re.search(r"SLIM_OPTION_GPU_EVALNEGPOP = 25\b", cand) and Opt.GPU_EVALNEGPOP == 25
    assert not declared & set(_lib.SAMPLE_SYMBOLS)


def got_rows(c, ht, nnegs, seed, w, users=None):
    rc, cs = host_sample_weighted(c.lib, c.ncols, c.hr, ht, nnegs, seed, w, users=users)
    assert rc == SLIM_OK, _lib.last_error()
    got = set_rows(c.lib, cs)
    c.lib.SLIMGPU_CandSetFree(cs)
    assert got[2] == c.ncols and got[0].dtype == np.int64 and got[1].dtype == np.int32
    return got


@pytest.mark.parametrize("name", ["floats", "ties", "wide"])
def test_host_rows_equal_the_restatement(cases, name):
    c = cases(name)
    T = held_out_rows(c, seed=91)
    ht = wrap(c.lib, T)
    tptr, tind = T.indptr.astype(np.int64), T.indices
    S = np.arange(0, c.nusers, 3, dtype=np.int32)
    try:
        for wname, nnegs in grid(c.ncols):
            w = weights(wname, c.R, c.ncols)
            for users in (None, S):
                want = weighted_rows((name, wname), c.R, tptr, tind, c.ncols, nnegs, 5, w, users=users)
                got = got_rows(c, ht, nnegs, 5, w, users=users)
                assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), (wname, nnegs, users is None)
            # what the rows must look like, whoever made them
            short = 0
            for u in range(c.nusers):
                row = want[1][want[0][u]:want[0][u + 1]]
                t = tind[tptr[u]:tptr[u + 1]]
                if t.size == 0 or u % 3:
                    assert row.size == 0
                    continue
                X = np.union1d(c.R.indices[c.R.indptr[u]:c.R.indptr[u + 1]], t)
                neg = row[:row.size - t.size]
                assert np.array_equal(row[neg.size:], t)                        # the test row stands behind, as given
                free = np.setdiff1d(np.flatnonzero(w), X).size                  # eligible items of positive weight
                assert neg.size == min(nnegs, free)                             # short only when fewer exist
                assert np.unique(neg).size == neg.size and not np.isin(neg, X).any() and (w[neg] > 0).all()
                short += neg.size < nnegs
            assert (short > 0) == ((wname, nnegs) in (("cliff", 700), ("zipf", 1450))), (wname, nnegs, short)
        # NULL weights are the popularity of trn's rows
        counts = weights("counts", c.R, c.ncols)
        for nnegs in (64, 99):
            a, b = got_rows(c, ht, nnegs, 5, None), got_rows(c, ht, nnegs, 5, counts)
            assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
        # the unweighted call is what it was
        want = sampled_rows(c.R, tptr, tind, c.ncols, 99, seed=5)
        rc, cs = host_sample(c.lib, c.ncols, c.hr, ht, 99, 5)
        assert rc == SLIM_OK
        uni = set_rows(c.lib, cs)
        c.lib.SLIMGPU_CandSetFree(cs)
        assert np.array_equal(uni[0], want[0]) and np.array_equal(uni[1], want[1])
        assert not np.array_equal(uni[1], b[1])
    finally:
        c.lib.Py_csr_free(ht)


def test_input_guard_the_phases_the_restatement_reaches(cases):
    """A guard on the INPUTS, not on the library (it runs the restatement only and passes without the feature): the
    inputs reach what they were chosen for (floats, every 5th user, seed 5): counts and zipf end in phase 1
    with full rows; cliff reaches phase 2 for every user with the draw guard exhausted -- full rows up to 99, of which
    phase 2 picks all but the heavy items the user may have (at most 50), short rows at 700; zipf at 1450 reaches
    phase 2 with short rows."""
    c = cases("floats")
    T = held_out_rows(c, seed=91)
    tptr, tind = T.indptr.astype(np.int64), T.indices
    users = [u for u in range(0, c.nusers, 5) if tptr[u + 1] > tptr[u]]
    assert len(users) == 60

    def run(wname, nnegs):
        w = weights(wname, c.R, c.ncols)
        return [weighted_user(("floats", wname), c.R, tptr, tind, c.ncols, nnegs, 5, w, u) for u in users]
    for wname in ("counts", "zipf"):
        for nnegs in (1, 63, 64, 65, 99, 700):
            assert all(neg.size == nnegs and picks == 0 for neg, _, picks in run(wname, nnegs)), (wname, nnegs)
    for nnegs in (63, 64, 65, 99):
        res = run("cliff", nnegs)
        print("cliff", nnegs, "phase-2 picks per user:", min(p for _, _, p in res), "to", max(p for _, _, p in res))
        assert all(neg.size == nnegs and d == 16 * nnegs + 1024 and nnegs - 50 <= picks < nnegs for neg, d, picks in res)
    assert all(neg.size < 700 and picks > 0 for neg, _, picks in run("cliff", 700))
    res = run("zipf", 1450)
    assert all(picks > 0 for _, _, picks in res) and any(neg.size < 1450 for neg, _, _ in res)
    assert int(weights("cliff", c.R, c.ncols).astype(np.uint64).sum()) > 2 ** 32


@pytest.mark.parametrize("zero_tail", [False, True])
def test_a_hand_made_matrix(zero_tail):
    lib = _lib.load()
    ncols, nnegs = 40, 5
    R, T, w = hand_made(zero_tail)
    hr, ht = wrap(lib, R, binary=True), wrap(lib, T, binary=True)
    try:
        for seed in (1, 2, 2 ** 63 + 11):
            want = weighted_rows(("hand", zero_tail), R, T.indptr.astype(np.int64), T.indices, ncols, nnegs, seed, w)
            rc, cs = host_sample_weighted(lib, ncols, hr, ht, nnegs, seed, w)
            assert rc == SLIM_OK, _lib.last_error()
            got = set_rows(lib, cs)
            lib.SLIMGPU_CandSetFree(cs)
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), seed
            # user 0: nothing free; user 1: items 36-39 free, none of them with a weight under zero_tail
            assert np.diff(want[0]).tolist() == [0 + 1, (0 if zero_tail else 4) + 2, 5 + 1, 5 + 1, 0, 5 + 3]
            if not zero_tail:
                assert sorted(want[1][want[0][1]:want[0][1] + 4].tolist()) == [36, 37, 38, 39]
            assert want[1][-3:].tolist() == [7, 7, 44]
            assert not zero_tail or (want[1][want[0][2]:want[0][3] - 1] < 35).all()
    finally:
        lib.Py_csr_free(hr)
        lib.Py_csr_free(ht)


def test_refusals_leave_out_untouched(cases):
    c = cases("floats")
    T = held_out_rows(c, seed=91)
    ht = wrap(c.lib, T)
    SENTINEL = 0x5A5A
    try:
        def refused(word, nnegs=99, w=None, hr=c.hr):
            h = C.c_void_p(SENTINEL)
            rc = c.lib.SLIMGPU_CandSetSampleWeighted(c.ncols, hr, ht, 0, None, nnegs, 1, P(w), C.byref(h))
            assert rc == SLIM_ERROR_INPUT and h.value == SENTINEL, (word, rc)
            assert "SLIMGPU_CandSetSampleWeighted" in _lib.last_error() and word in _lib.last_error(), _lib.last_error()
        refused("T = 0", w=np.zeros(c.ncols, np.uint32))
        refused("nnegs", nnegs=0)
        refused("nnegs", nnegs=-1, w=weights("zipf", c.R, c.ncols))
        empty = wrap(c.lib, csr([[] for _ in range(c.nusers)], c.ncols), binary=True)      # no popularity at all
        try:
            refused("T = 0", hr=empty)
        finally:
            c.lib.Py_csr_free(empty)
        assert c.lib.SLIMGPU_CandSetSampleWeighted(c.ncols, c.hr, ht, 0, None, 99, 1, None, None) == SLIM_ERROR_INPUT
    finally:
        c.lib.Py_csr_free(ht)


def test_the_sampler_is_weighted(cases):
    """floats, user 0, zipf, one negative, seeds 0 ... 3999: the frequency of each of the five heaviest eligible
    items lies within 4 binomial standard deviations sqrt(p (1 - p) / 4000) of p = w_i / sum of the eligible
    weights.  A condition, not a measurement (the restatement's largest deviation is 1.2)."""
    c = cases("floats")
    T = held_out_rows(c, seed=91)
    ht = wrap(c.lib, T)
    w = weights("zipf", c.R, c.ncols)
    u, N = 0, 4000
    X = np.union1d(c.R.indices[c.R.indptr[u]:c.R.indptr[u + 1]], T.indices[T.indptr[u]:T.indptr[u + 1]])
    elig = w.astype(np.float64)
    elig[X] = 0
    heavy = np.argsort(-elig, kind="stable")[:5]
    one = np.array([u], np.int32)
    seen = np.zeros(c.ncols, np.int64)
    try:
        for seed in range(N):
            rc, cs = host_sample_weighted(c.lib, c.ncols, c.hr, ht, 1, seed, w, users=one)
            assert rc == SLIM_OK
            ptr, ind, _ = set_rows(c.lib, cs)
            c.lib.SLIMGPU_CandSetFree(cs)
            seen[ind[ptr[u]]] += 1
            if seed < 40:
                assert ind[ptr[u]] == weighted_negatives(seed, u, X, 1, w)[0][0]
    finally:
        c.lib.Py_csr_free(ht)
    worst = 0.0
    for i in heavy:
        p = elig[i] / elig.sum()
        dev = abs(seen[i] / N - p) / np.sqrt(p * (1 - p) / N)
        print("item %d: weight %d, p %.4f, frequency %.4f, %.2f standard deviations" % (i, w[i], p, seen[i] / N, dev))
        assert dev <= 4.0
        worst = max(worst, dev)
    assert seen[X].sum() == 0 and seen[w == 0].sum() == 0


def test_the_python_layer(cases):
    from slim_amd.engine import CandidateSet, popularity_weights, sample_candidates
    c = cases("ties")
    T = held_out_rows(c, seed=91)
    tptr, tind = T.indptr.astype(np.int64), T.indices
    counts = weights("counts", c.R, c.ncols)
    pw = popularity_weights(c.R)
    assert pw.dtype == np.uint32 and np.array_equal(pw, counts)
    p75 = popularity_weights(c.R, alpha=0.75)
    assert p75.dtype == np.uint32 and np.array_equal(p75, np.rint(counts.astype(np.float64) ** 0.75 * 1024).astype(np.uint32))
    want = weighted_rows(("ties", "counts"), c.R, tptr, tind, c.ncols, 99, 5, counts)
    for wts in ("popularity", pw, counts.astype(np.int64)):
        cset = sample_candidates(c.R, T, 99, seed=5, ncols=c.ncols, weights=wts)
        try:
            assert isinstance(cset, CandidateSet) and cset.ncols == c.ncols
            ptr, ind = cset.rows()
            assert np.array_equal(ptr, want[0]) and np.array_equal(ind, want[1])
        finally:
            cset.close()
    want75 = weighted_rows(("ties", "p75"), c.R, tptr, tind, c.ncols, 64, 5, p75)
    cset = sample_candidates(c.R, T, 64, seed=5, ncols=c.ncols, weights=p75)
    ptr, ind = cset.rows()
    cset.close()
    assert np.array_equal(ptr, want75[0]) and np.array_equal(ind, want75[1])
    for bad in (counts[:-1], -counts.astype(np.int64) - 1, counts.astype(np.float64), "uniform",
                counts.astype(np.int64) + 2 ** 32):
        with pytest.raises(ValueError, match="weights"):
            sample_candidates(c.R, T, 99, ncols=c.ncols, weights=bad)
    with pytest.raises(ValueError, match="T = 0"):
        sample_candidates(c.R, T, 99, ncols=c.ncols, weights=np.zeros(c.ncols, np.uint32))
    # the option rides along
    from slim_amd.interface import build_options, check_params
    params = {"gpu_evalnegs": 99, "gpu_evalnegpop": 1}
    iopt, _ = build_options(check_params(params))
    assert iopt[23] == 99 and iopt[25] == 1
    iopt, _ = build_options(check_params({}))
    assert iopt[25] == -1
