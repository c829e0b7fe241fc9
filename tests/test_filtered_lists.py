"""Candidate filters on the device scorers (include/slim_gpu_filter.h): SLIMGPU_PredictListsFiltered,
SLIMGPU_ModelPredictListsFiltered, SLIMGPU_MatrixPredictListsFiltered and ResidentModel.predict(filter=...).

The yardstick (tests/filtered_cases.py) is the existing, unfiltered host scorer asked once per case for the full
ranking; the expected filtered list of length n is that ranking without the disallowed and the excluded ids, cut at
n.  Ids, float scores, counts and the untouched fill are compared with np.array_equal: no tolerances.

  ties / floats  1 500 x 1 500 model, 300 users, two of them empty: one chunk per wavefront, 1 500 is no multiple of 32
  wide           6 000 x 6 000 model, 96 users: several chunks, more than 4 096 unfiltered candidates
"""
import os

import numpy as np
import pytest
import scipy.sparse as sp

from filtered_cases import NO_HISTORY, P, cases_fixture, make_filter, same
from slim_amd import _lib
from slim_amd.constants import SLIM_OK
from slim_amd.engine import eval_stats, list_stats

pytestmark = pytest.mark.gpu
cases = pytest.fixture(scope="module")(cases_fixture)
BOTH = pytest.mark.parametrize("name", ["floats", "ties"])


def path_of(n):
    return 1 if n <= 64 else (2 if n <= 128 else 4)


def call(c, entry, n, flt, env=None, users=None):
    """One of the three filtered entry points ("host", "model", "matrix") into sentinel-filled arrays."""
    nu = c.nusers if users is None else users.size
    ids = np.full((nu, n), -1, np.int32)
    sc = np.zeros((nu, n), np.float32)
    cnt = np.full(nu, -7, np.int32)
    lib = c.lib
    os.environ.update(env or {})
    try:
        if entry == "host":
            rc = lib.SLIMGPU_PredictListsFiltered(n, c.hw, c.hr, flt, P(ids), P(sc), P(cnt))
        elif entry == "model":
            rc = lib.SLIMGPU_ModelPredictListsFiltered(n, c.model.handle, c.hr, flt, P(ids), P(sc), P(cnt))
        else:
            rc = lib.SLIMGPU_MatrixPredictListsFiltered(n, c.model.handle, c.mat.handle, 0 if users is None else nu,
                                                        None if users is None else P(users), flt, P(ids), P(sc), P(cnt))
    finally:
        for k in (env or {}):
            del os.environ[k]
    assert rc == SLIM_OK, _lib.last_error()
    return ids, sc, cnt


class Filter(object):
    def __init__(self, c, **kw):
        self.c = c
        rc, self.h = make_filter(c.lib, c.ncols, **kw)
        assert rc == SLIM_OK, _lib.last_error()

    def __enter__(self):
        return self.h

    def __exit__(self, *a):
        self.c.lib.SLIMGPU_FilterFree(self.h)


# ---- 1. a random allow set at every length, on every path ------------------------------------------------------------
@BOTH
def test_allow_set_at_every_length(cases, name):
    c = cases(name)
    allowed = np.random.default_rng(41).random(c.ncols) < 0.4
    with Filter(c, allowed=np.flatnonzero(allowed)) as flt:
        for n in (1, 10, 64, 65, 128, 129, 300, 1500):
            got = call(c, "host", n, flt)
            assert list_stats(c.lib)["path"] == path_of(n)
            assert same(got, c.expected(n, allowed)), (name, n)
            assert (got[2][list(NO_HISTORY)] == 0).all() and (got[0][list(NO_HISTORY)] == -1).all()
            if n == 10:     # not an empty test: the filter changes most lists
                plain = c.expected(n)
                differ = np.any(got[0] != plain[0], axis=1).sum()
                print(name, "lists of 10 changed by the allow set: %d of %d" % (differ, (plain[2] > 0).sum()))
                assert differ >= (plain[2] > 0).sum() / 2


# ---- 2. every chunk edge, every bitmap word edge, the last id ---------------------------------------------------------
@pytest.mark.parametrize("env", [{}, {"SLIM_TOPN_KERNEL": "long"}], ids=["default", "long"])
@pytest.mark.parametrize("rem, complement", [(0, False), (31, False), (0, True), (31, True)])
def test_word_edges_on_several_chunks(cases, rem, complement, env):
    c = cases("wide")
    allowed = (np.arange(c.ncols) % 32 == rem) != complement
    assert (c.ncand > 4096).sum() >= 90
    with Filter(c, allowed=np.flatnonzero(allowed)) as flt:
        for n in (64, 128, 4096):
            got = call(c, "host", n, flt, env=env)
            assert list_stats(c.lib)["path"] == (4 if env else path_of(n))
            want = c.expected(n, allowed)
            assert same(got, want), (rem, complement, n, env)
            if n == 4096:   # more than 4 096 candidates before the filter, fewer after: exactly the survivors
                short = (c.ncand > 4096) & (want[2] < 4096)
                assert short.sum() >= (90 if not complement else 0)
                assert complement or (want[2][short] > 0).all()
    # (the sets put an edge of the allowed ids at the first and at the last bit of every bitmap word, hence at
    # every chunk edge; the last id, 5 999, is bit 15 of a short last word: barred by the sets, allowed by the rest)
    assert allowed[c.ncols - 1] == complement


# ---- 3. the block form, the degenerate sets, the no-op filter ---------------------------------------------------------
@BOTH
def test_block_form_and_degenerate_sets(cases, name):
    c = cases(name)
    allowed = np.random.default_rng(43).random(c.ncols) < 0.4
    for n in (10, 300):
        want = c.expected(n, allowed)
        with Filter(c, blocked=np.flatnonzero(~allowed)) as flt:
            assert same(call(c, "host", n, flt), want)
        with Filter(c, allowed=[]) as flt:              # nothing may be shown: untouched output
            ids, sc, cnt = call(c, "host", n, flt)
            assert (cnt == 0).all() and (ids == -1).all() and (sc == 0).all()
        one = int(c.ids[0, 0])                          # user 0's best item, and nothing else
        mask = np.zeros(c.ncols, bool)
        mask[one] = True
        with Filter(c, allowed=[one, one]) as flt:
            got = call(c, "host", n, flt)
            assert same(got, c.expected(n, mask)) and got[2][0] == 1 and got[0][0, 0] == one and got[2].max() == 1
        # filters that filter nothing: the unfiltered call, bit for bit -- with and without a bitmap on the device
        plain = c.expected(n)
        unfiltered = np.full((c.nusers, n), -1, np.int32), np.zeros((c.nusers, n), np.float32), np.zeros(c.nusers, np.int32)
        assert c.lib.SLIMGPU_PredictLists(n, c.hw, c.hr, *[P(a) for a in unfiltered]) == SLIM_OK
        assert same(unfiltered, plain)
        for kw in ({}, {"blocked": []}, {"allowed": np.arange(c.ncols)}, {"X": c.exclusions(1, xusers=0)}):
            with Filter(c, **kw) as flt:
                assert same(call(c, "host", n, flt), unfiltered), sorted(kw)
        assert same(call(c, "host", n, None), unfiltered)


# ---- 4. per-user exclusions, by user id --------------------------------------------------------------------------------
@BOTH
def test_exclusions_alone_and_with_an_allow_set(cases, name):
    c = cases(name)
    allowed = np.random.default_rng(47).random(c.ncols) < 0.4
    X = c.exclusions(seed=53, xusers=c.nusers - 10)      # the last ten users have no row
    lens = np.diff(X.indptr)
    assert lens.max() <= 30 and (lens == 0).sum() >= 30 and lens.max() >= 20
    for kw, mask in (({"X": X}, None), ({"X": X, "allowed": np.flatnonzero(allowed)}, allowed)):
        with Filter(c, **kw) as flt:
            for n in (3, 10, 64, 128, 300):
                got = call(c, "host", n, flt)
                assert list_stats(c.lib)["path"] == path_of(n)
                assert same(got, c.expected(n, mask, X)), (name, sorted(kw), n)
    # the top 3 vanish and the list closes up; the users without a row keep theirs
    with Filter(c, X=X) as flt:
        ids, sc, cnt = call(c, "host", 10, flt)
    plain = c.expected(10)
    hit = [u for u in range(c.nusers - 10) if u % 7 != 3 and u % 5 != 4 and c.ncand[u] >= 45]
    assert len(hit) > 100
    for u in hit:
        assert not set(plain[0][u, :3]) & set(ids[u]) and cnt[u] == 10
    assert np.array_equal(ids[-10:], plain[0][-10:])


@BOTH
def test_exclusion_rows_go_by_user_id(cases, name):
    c = cases(name)
    lib = c.lib
    allowed = np.random.default_rng(59).random(c.ncols) < 0.4
    X = c.exclusions(seed=61)
    users = np.arange(0, c.nusers, 3, dtype=np.int32)
    # what a scorer that took the exclusion row of the POSITION would apply: row q of X at user users[q]
    by_position = sp.csr_matrix((c.nusers, c.ncols), dtype=np.float32)
    lens = np.zeros(c.nusers, np.int64)
    lens[users] = np.diff(X.indptr)[:users.size]
    by_position.indptr = np.concatenate(([0], np.cumsum(lens)))
    by_position.indices = X.indices[:X.indptr[users.size]].copy()
    by_position.data = np.ones(by_position.indices.size, np.float32)
    with Filter(c, X=X, allowed=np.flatnonzero(allowed)) as flt:
        for n in (10, 128, 300):
            # the three entry points agree with each other and with the yardstick
            want = c.expected(n, allowed, X)
            for entry in ("host", "model", "matrix"):
                assert same(call(c, entry, n, flt), want), (name, entry, n)
            assert eval_stats(lib)["path"] == path_of(n)
            # every third user: position q is user 3 q (a scorer that took row q of X would fail)
            got = call(c, "matrix", n, flt, users=users)
            assert same(got, c.expected(n, allowed, X, users)), (name, n)
            assert not same(got, c.expected(n, allowed, by_position, users))
        # slices of the long form: a slice's position q is user user0 + q
        n, want = 300, c.expected(300, allowed, X)
        for entry in ("host", "model", "matrix"):
            got = call(c, entry, n, flt, env={"SLIM_TOPN_LONG_SLICE": "37"})
            assert list_stats(lib)["slices"] == 9 and list_stats(lib)["path"] == 4
            assert same(got, want), (name, entry)
        got = call(c, "matrix", n, flt, users=users, env={"SLIM_TOPN_LONG_SLICE": "37"})
        assert list_stats(lib)["slices"] == 3 and same(got, c.expected(n, allowed, X, users))
        # the device copy was made once: the second and third call of a shape allocate the same
        call(c, "matrix", n, flt)
        second = eval_stats(lib)["device_allocs"]
        call(c, "matrix", n, flt)
        assert eval_stats(lib)["device_allocs"] == second


# ---- 5. the Python layer -----------------------------------------------------------------------------------------------
def test_resident_model_predict_with_a_filter(cases):
    c = cases("ties")
    allowed = np.random.default_rng(67).random(c.ncols) < 0.4
    X = c.exclusions(seed=71)
    users = np.arange(1, c.nusers, 3, dtype=np.int32)
    with pytest.raises(ValueError):
        c.mat.item_filter(allowed=[1], blocked=[2])
    with pytest.raises(ValueError):
        c.mat.item_filter(allowed=[c.ncols])
    for kw, mask, rows in (({"allowed": np.flatnonzero(allowed)}, allowed, None),
                           ({"blocked": np.flatnonzero(~allowed), "exclusions": X}, allowed, X),
                           ({"exclusions": X}, None, X)):
        flt = c.mat.item_filter(**kw)
        for n in (10, 300):
            assert same(c.model.predict(c.mat, n, return_counts=True, filter=flt), c.expected(n, mask, rows))
            assert same(c.model.predict(c.mat, n, users=users, filter=flt), c.expected(n, mask, rows, users)[:2])
        flt.close()
    assert same(c.model.predict(c.mat, 10, return_counts=True), c.expected(10))


def test_py_slim_predict_filtered_on_the_device(cases, monkeypatch):
    c = cases("floats")
    allowed = np.random.default_rng(73).random(c.ncols) < 0.4
    X = c.exclusions(seed=79)
    monkeypatch.setenv("SLIM_PREDICT", "gpu")
    with Filter(c, X=X, allowed=np.flatnonzero(allowed)) as flt:
        for n in (10, 300):
            ids = np.full(c.nusers * n, -1, np.int32)
            sc = np.zeros(c.nusers * n, np.float32)
            assert c.lib.Py_SLIM_PredictFiltered(n, c.hw, c.hr, flt, ids, sc) == SLIM_OK, _lib.last_error()
            assert list_stats(c.lib)["path"] == path_of(n)
            assert same((ids.reshape(-1, n), sc.reshape(-1, n)), c.expected(n, allowed, X)[:2])
