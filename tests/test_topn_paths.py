"""The branches of the top-N scorers that the parity suites do not reach: a host model whose rows are
not sorted by id (the on-demand row-order check, the wave kernel behind it, the refusal of a pinned
chunk kernel), the list lengths around the chunk kernel's limit of 64 and the scorer's of 128, and
the 1-vs-k scorer's refusal of rows that do not ascend strictly.

Everything is tiny: a 300-item model with about 10 entries per row, 200 users.  The handles are built
with Py_csr_wrapper directly, which keeps the order of a row's entries as given.
"""
import ctypes as C
import functools
import os

import numpy as np
import pytest
import scipy.sparse as sp

import slim_oracle as O
from slim_amd import _lib
from slim_amd.constants import SLIM_ERROR_INPUT, SLIM_OK

NITEMS, NUSERS = 300, 200
SHUFFLED_ROWS = (3, 57, 299)
SEED = 11
CHUNK = {"SLIM_TOPN_KERNEL": "chunk"}


@functools.lru_cache(maxsize=None)
def _data():
    """ptr / ind / val of the sorted model, of its copy with three shuffled rows and of its copy with a
    repeated id, and the two histories (binary: no values; rated 1-5)."""
    rng = np.random.default_rng(SEED)
    rows = [np.sort(rng.choice(NITEMS, size=int(rng.integers(8, 13)), replace=False)) for _ in range(NITEMS)]
    ptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.intp)
    ind = np.concatenate(rows).astype(np.int32)
    val = rng.random(ind.size, dtype=np.float32)
    assert ind.max() == NITEMS - 1          # Py_csr_wrapper: ncols = largest id + 1
    u_ind, u_val = ind.copy(), val.copy()
    for r in SHUFFLED_ROWS:
        s, e = ptr[r], ptr[r + 1]
        p = rng.permutation(e - s)
        while np.all(np.diff(ind[s:e][p]) > 0):
            p = rng.permutation(e - s)
        u_ind[s:e], u_val[s:e] = ind[s:e][p], val[s:e][p]
    d_ind = ind.copy()                       # row 10: its second id once more in the slot behind it
    d_ind[ptr[10] + 2] = d_ind[ptr[10] + 1]
    H = sp.random(NUSERS, NITEMS, density=0.03, format="csr", random_state=rng, dtype=np.float32)
    H.sort_indices()
    H.data = rng.integers(1, 6, H.nnz).astype(np.float32)
    W = sp.csr_matrix((val, ind, ptr), shape=(NITEMS, NITEMS))
    return {"ptr": ptr, "sorted": (ind, val), "unsorted": (u_ind, u_val), "repeated": (d_ind, val),
            "H": H, "W": W}


def _wrap(lib, nrows, ptr, ind, val):
    h = C.c_void_p()
    vp = val.ctypes.data_as(C.c_void_p) if val is not None else C.c_void_p()
    assert lib.Py_csr_wrapper(nrows, np.ascontiguousarray(ptr, np.intp), np.ascontiguousarray(ind, np.int32), vp,
                              C.byref(h)) == SLIM_OK
    return h


@pytest.fixture(scope="module")
def handles():
    lib = _lib.load()
    D = _data()
    H = D["H"]
    hs = {k: _wrap(lib, NITEMS, D["ptr"], *D[k]) for k in ("sorted", "unsorted", "repeated")}
    hs["binary"] = _wrap(lib, NUSERS, H.indptr, H.indices, None)
    hs["rated"] = _wrap(lib, NUSERS, H.indptr, H.indices, np.ascontiguousarray(H.data, np.float32))
    yield hs
    for h in hs.values():
        lib.Py_csr_free(h)


_host_lists = {}


def _host(handles, model, hist, n):
    """The host scorer's lists, computed once per case."""
    key = (model, hist, n)
    if key not in _host_lists:
        lib = _lib.load()
        ids = np.full(NUSERS * n, -1, np.int32)
        sc = np.zeros(NUSERS * n, np.float32)
        os.environ["SLIM_PREDICT"] = "cpu"
        try:
            assert lib.Py_SLIM_Predict(n, handles[model], handles[hist], ids, sc) == SLIM_OK
        finally:
            del os.environ["SLIM_PREDICT"]
        ids.setflags(write=False)
        sc.setflags(write=False)
        _host_lists[key] = (ids, sc)
    return _host_lists[key]


def _gpu(handles, model, hist, n, env=None):
    """SLIMGPU_Predict into sentinel-filled arrays: (status, ids, scores, last_error)."""
    lib = _lib.load()
    ids = np.full(NUSERS * n, -1, np.int32)
    sc = np.zeros(NUSERS * n, np.float32)
    os.environ.update(env or {})
    try:
        rc = lib.SLIMGPU_Predict(n, handles[model], handles[hist], ids, sc)
    finally:
        for k in (env or {}):
            del os.environ[k]
    return rc, ids, sc, _lib.last_error()


def _untouched(ids, sc):
    return bool((ids == -1).all() and (sc == 0).all())


HISTS = ["binary", "rated"]


@pytest.mark.parametrize("hist", HISTS)
def test_host_scorer_on_shuffled_rows_gives_the_oracles_lists(handles, hist):
    """Without ties among a user's best N + 1 the order of a model row's entries cannot show in the
    lists: every candidate still receives one addition per history item, in history order."""
    n = 7
    D = _data()
    ids_w, sc_w = O.predict(D["W"], D["H"], n + 1, binary=hist == "binary")
    valid = ids_w >= 0
    tied = valid[:, 1:] & (sc_w[:, 1:] == sc_w[:, :-1])
    assert not tied.any(), "the seed leaves ties inside the first N + 1"
    ids_o, sc_o = O.predict(D["W"], D["H"], n, binary=hist == "binary")
    ids_c, sc_c = _host(handles, "unsorted", hist, n)
    assert np.array_equal(ids_c.reshape(NUSERS, n), ids_o)
    assert np.array_equal(sc_c.reshape(NUSERS, n), sc_o)


@pytest.mark.gpu
@pytest.mark.parametrize("hist", HISTS)
def test_unsorted_model_is_served_by_the_wave_kernel(handles, hist):
    n = 7
    rc, ids, sc, err = _gpu(handles, "unsorted", hist, n)
    assert rc == SLIM_OK, err
    ids_c, sc_c = _host(handles, "unsorted", hist, n)
    assert np.array_equal(ids, ids_c) and np.array_equal(sc, sc_c)


@pytest.mark.gpu
@pytest.mark.parametrize("hist", HISTS)
def test_unsorted_model_refuses_the_pinned_chunk_kernel(handles, hist):
    rc, ids, sc, err = _gpu(handles, "unsorted", hist, 7, CHUNK)
    assert rc == SLIM_ERROR_INPUT
    assert "model rows sorted" in err
    assert _untouched(ids, sc)


@pytest.mark.gpu
@pytest.mark.parametrize("hist", HISTS)
@pytest.mark.parametrize("n,env", [(65, None), (64, CHUNK)])
def test_list_lengths_around_the_chunk_kernels_limit(handles, hist, n, env):
    rc, ids, sc, err = _gpu(handles, "sorted", hist, n, env)
    assert rc == SLIM_OK, err
    ids_c, sc_c = _host(handles, "sorted", hist, n)
    assert np.array_equal(ids, ids_c) and np.array_equal(sc, sc_c)
    assert (ids_c.reshape(NUSERS, n)[:, -1] == -1).any()   # short lists: slots behind them stay as filled


@pytest.mark.gpu
@pytest.mark.parametrize("hist", HISTS)
def test_lists_of_65_refuse_the_pinned_chunk_kernel(handles, hist):
    rc, ids, sc, err = _gpu(handles, "sorted", hist, 65, CHUNK)
    assert rc == SLIM_ERROR_INPUT
    assert "model rows sorted" in err
    assert _untouched(ids, sc)


@pytest.mark.gpu
@pytest.mark.parametrize("hist", HISTS)
def test_lists_of_129_are_refused(handles, hist):
    rc, ids, sc, err = _gpu(handles, "sorted", hist, 129)
    assert rc == SLIM_ERROR_INPUT
    assert _untouched(ids, sc)


def _one_vs_k(handles, model, hist, neg, n):
    lib = _lib.load()
    ids = np.full(NUSERS * n, -1, np.int32)
    sc = np.zeros(NUSERS * n, np.float32)
    rc = lib.SLIMGPU_Predict1vsK(n, neg.shape[1], handles[model], handles[hist], neg.reshape(-1).copy(), ids, sc)
    return rc, ids, sc, _lib.last_error()


@functools.lru_cache(maxsize=None)
def _negatives():
    neg = np.random.default_rng(SEED + 1).integers(0, NITEMS, size=(NUSERS, 20)).astype(np.int32)
    neg.setflags(write=False)
    return neg


@pytest.mark.gpu
@pytest.mark.parametrize("hist", HISTS)
def test_1vsk_on_the_sorted_model_matches_the_oracle(handles, hist):
    n = 5
    D = _data()
    rc, ids, sc, err = _one_vs_k(handles, "sorted", hist, _negatives(), n)
    assert rc == SLIM_OK, err
    ids_o, sc_o = O.predict_1vsk(D["W"], D["H"], _negatives(), n, binary=hist == "binary")
    assert np.array_equal(ids.reshape(NUSERS, n), ids_o)
    assert np.array_equal(sc.reshape(NUSERS, n), sc_o)


@pytest.mark.gpu
@pytest.mark.parametrize("hist", HISTS)
@pytest.mark.parametrize("model", ["unsorted", "repeated"])
def test_1vsk_refuses_rows_that_do_not_ascend_strictly(handles, hist, model):
    rc, ids, sc, err = _one_vs_k(handles, model, hist, _negatives(), 5)
    assert rc == SLIM_ERROR_INPUT
    assert "not ascending" in err
    assert _untouched(ids, sc)
