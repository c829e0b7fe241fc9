"""SLIMGPU_SplitHost (include/slim_gpu_split.h) against the numpy restatement of the header's rule
(tests/split_cases.py), the properties the rule promises, asserted on the library's output, and the refusals.  No GPU."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp

from sampled_cases import key
from slim_amd import _lib
from slim_amd.constants import SLIM_ERROR_INPUT, SLIM_OK
from split_cases import (FOLDS, LEAVE_OUT, assert_same_rows, edge_lengths, entry_keys, host_split, rows_matrix,
                         split_rows, takes_part)

NCOLS = 1500
SEED = 20240917
# (mode, F, h): leave-out over F in {1, 2, 5} and h in {1, 3}; folds needs F >= 2 and reads no h
CASES = [(LEAVE_OUT, F, h) for F in (1, 2, 5) for h in (1, 3)] + [(FOLDS, F, 1) for F in (2, 5)]


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def matrix_for(F, h, m, ratings):
    return rows_matrix(edge_lengths(F, h, m), NCOLS, seed=7 * F + h + m, ratings=ratings)


def test_vectorised_keys_are_the_headers_key():
    R = matrix_for(2, 1, 1, True)
    rows, _, k = entry_keys(R, SEED)
    for u in (0, 5, 123, R.shape[0] - 1):
        ids = R.indices[R.indptr[u]:R.indptr[u + 1]]
        assert np.array_equal(k[rows == u], key(SEED, u, ids.astype(np.int64)))


@pytest.mark.parametrize("ratings", [True, False], ids=["ratings", "binary"])
@pytest.mark.parametrize("m", [1, 2])
@pytest.mark.parametrize("mode,F,h", CASES)
def test_host_split_equals_the_restatement_and_keeps_its_promises(lib, mode, F, h, m, ratings):
    R = matrix_for(F, h, m, ratings)
    binary = not ratings
    lens = np.diff(R.indptr)
    need = F * h + m
    if mode == LEAVE_OUT:  # the edges of the rule are among the rows
        assert {0, 1, need - 1, need, 63, 64, 65, 5000} <= set(lens.tolist())
    tests = []
    for f in range(F):
        part = takes_part(R, mode, F, f, h, m, SEED)
        assert 2 * part.sum() >= R.shape[0], "at least half of the users take part"
        assert (~part).any(), "at least one user does not take part"
        st, trn, tst = host_split(lib, R, mode, F, f, h, m, SEED, binary=binary)
        assert st == SLIM_OK, _lib.last_error()
        want_trn, want_tst = split_rows(R, mode, F, f, h, m, SEED, binary=binary)
        assert_same_rows(trn, want_trn, "train rows, fold %d" % f)
        assert_same_rows(tst, want_tst, "test rows, fold %d" % f)
        tests.append(tst)
        # train U test = the source row as a multiset, both in source order; a user outside keeps its row
        assert trn[0].size == tst[0].size == R.shape[0] + 1
        for u in range(R.shape[0]):
            a0, a1 = R.indptr[u], R.indptr[u + 1]
            src_ids, src_vals = R.indices[a0:a1], R.data[a0:a1]
            t_ids, b_ids = trn[1][trn[0][u]:trn[0][u + 1]], tst[1][tst[0][u]:tst[0][u + 1]]
            t_vals = None if binary else trn[2][trn[0][u]:trn[0][u + 1]]
            b_vals = None if binary else tst[2][tst[0][u]:tst[0][u + 1]]
            if not part[u]:
                assert b_ids.size == 0 and np.array_equal(t_ids, src_ids)
                assert binary or np.array_equal(t_vals, src_vals)
                continue
            ia = ib = 0  # a walk of the source row must consume both halves exactly, each in its own order
            for i, v in zip(src_ids, src_vals):
                if ib < b_ids.size and b_ids[ib] == i and (binary or b_vals[ib] == v):
                    ib += 1
                else:
                    assert ia < t_ids.size and t_ids[ia] == i and (binary or t_vals[ia] == v)
                    ia += 1
            assert ia == t_ids.size and ib == b_ids.size
            if mode == LEAVE_OUT:
                assert b_ids.size == h, "a user that takes part holds out exactly h entries"
            else:
                assert b_ids.size >= 1 and t_ids.size >= m
    # over the folds: leave-out test rows are disjoint; folds-mode test rows partition the row (counting the folds
    # the user takes part in: there the held entries are exactly the fold's)
    for u in range(R.shape[0]):
        seen = [tuple(t[1][t[0][u]:t[0][u + 1]].tolist()) for t in tests]
        flat = [i for s in seen for i in s]
        assert len(flat) == len(set(flat)), "user %d: an entry is held out in two folds" % u
        if mode == FOLDS and all(len(s) > 0 for s in seen):
            assert sorted(flat) == sorted(R.indices[R.indptr[u]:R.indptr[u + 1]].tolist())


def test_values_travel_with_their_entries(lib):
    R = matrix_for(2, 1, 1, True)
    R.data = np.arange(1, R.nnz + 1, dtype=np.float32)  # every value names its entry
    st, trn, tst = host_split(lib, R, LEAVE_OUT, 2, 1, 1, 1, SEED)
    assert st == SLIM_OK
    both = np.concatenate((trn[2], tst[2]))
    assert np.array_equal(np.sort(both), R.data)
    assert np.array_equal(R.indices[(tst[2] - 1).astype(np.int64)], tst[1])
    assert np.array_equal(R.indices[(trn[2] - 1).astype(np.int64)], trn[1])


def test_engine_split_host_returns_scipy_halves(lib):
    from slim_amd.engine import split_host
    R = matrix_for(5, 1, 1, True)
    trn, tst = split_host(R, mode="leave_out", nfolds=5, fold=3, nheld=1, minkeep=1, seed=SEED)
    want_trn, want_tst = split_rows(R, LEAVE_OUT, 5, 3, 1, 1, SEED)
    assert trn.shape == tst.shape == R.shape
    assert_same_rows((trn.indptr.astype(np.int64), trn.indices, trn.data), want_trn, "train")
    assert_same_rows((tst.indptr.astype(np.int64), tst.indices, tst.data), want_tst, "test")
    with pytest.raises(ValueError, match="nfolds \\* nheld"):
        split_host(R, mode="leave_out", nfolds=65, fold=0, nheld=2)


@pytest.mark.parametrize("spec,word", [
    ((2, 2, 0, 1, 1), "mode"),
    ((LEAVE_OUT, 0, 0, 1, 1), "nfolds"),
    ((FOLDS, 1, 0, 1, 1), "nfolds"),
    ((LEAVE_OUT, 3, 3, 1, 1), "fold 3"),
    ((LEAVE_OUT, 3, -1, 1, 1), "fold -1"),
    ((LEAVE_OUT, 3, 0, 0, 1), "nheld"),
    ((LEAVE_OUT, 3, 0, 1, 0), "minkeep"),
    ((FOLDS, 3, 0, 1, 0), "minkeep"),
    ((LEAVE_OUT, 43, 0, 3, 1), "nfolds * nheld is 129"),
], ids=lambda x: x if isinstance(x, str) else None)
def test_refusals_leave_the_outputs_untouched(lib, spec, word):
    R = matrix_for(2, 1, 1, True)
    ptr, ind = np.ascontiguousarray(R.indptr, np.intp), np.ascontiguousarray(R.indices, np.int32)
    h = C.c_void_p()
    assert lib.Py_csr_wrapper(R.shape[0], ptr, ind, None, C.byref(h)) == SLIM_OK
    s = _lib.Split(*spec, SEED)
    trn, tst = C.c_void_p(0x1234), C.c_void_p(0x5678)
    assert lib.SLIMGPU_SplitHost(h, C.byref(s), C.byref(trn), C.byref(tst)) == SLIM_ERROR_INPUT
    assert word in _lib.last_error() and "SLIMGPU_SplitHost" in _lib.last_error()
    assert (trn.value, tst.value) == (0x1234, 0x5678)
    lib.Py_csr_free(h)


def test_the_largest_leave_out_selection_is_accepted(lib):
    R = rows_matrix([200, 129, 128, 0], NCOLS, seed=3)
    for f in (0, 63):
        st, trn, tst = host_split(lib, R, LEAVE_OUT, 64, f, 2, 1, SEED)
        assert st == SLIM_OK
        want = split_rows(R, LEAVE_OUT, 64, f, 2, 1, SEED)
        assert_same_rows(trn, want[0], "train")
        assert_same_rows(tst, want[1], "test")
        assert np.diff(tst[0]).tolist() == [2, 2, 0, 0]


def test_a_repeated_id_is_ordered_by_its_position(lib):
    # equal (key, item): the position in the row decides, so the first of two equal entries is held out first
    M = sp.csr_matrix((1, 4), dtype=np.float32)
    M.indptr, M.indices = np.array([0, 6], np.int32), np.array([2, 2, 2, 2, 2, 2], np.int32)
    M.data = np.arange(1, 7, dtype=np.float32)
    for f in range(3):
        st, trn, tst = host_split(lib, M, LEAVE_OUT, 3, f, 1, 1, SEED)
        assert st == SLIM_OK and tst[2].tolist() == [f + 1.0]
        assert_same_rows(tst, split_rows(M, LEAVE_OUT, 3, f, 1, 1, SEED)[1], "test")
        assert trn[2].tolist() == [v for v in range(1, 7) if v != f + 1]


def test_a_negative_id_is_refused(lib):
    M = sp.csr_matrix((2, 4), dtype=np.float32)
    M.indptr, M.indices, M.data = np.array([0, 2, 3], np.int32), np.array([1, -2, 3], np.int32), np.ones(3, np.float32)
    st, _, _ = host_split(lib, M, LEAVE_OUT, 1, 0, 1, 1, SEED)
    assert st == SLIM_ERROR_INPUT and "below 0" in _lib.last_error()


def test_null_arguments_are_input_errors(lib):
    s = _lib.Split(LEAVE_OUT, 1, 0, 1, 1, 1)
    out = C.c_void_p()
    assert lib.SLIMGPU_SplitHost(None, C.byref(s), C.byref(out), C.byref(out)) == SLIM_ERROR_INPUT


def test_slimatrix_split_carries_the_id_maps(lib):
    from slim_amd import SLIM, SLIMatrix
    # triplets with raw ids: the halves answer in the data's dense ids and keep its maps
    rng = np.random.default_rng(4)
    users, items = ["u%d" % k for k in range(40)], [1000 + 3 * k for k in range(60)]
    trip = [[users[u], items[i], float(rng.integers(1, 6))] for u in range(40)
            for i in rng.permutation(60)[:rng.integers(0, 12)]]
    data = SLIMatrix(trip)
    trn, tst = SLIM.split(data, mode="leave_out", nfolds=2, fold=1, nheld=2, minkeep=1, seed=SEED)
    assert type(trn) is SLIMatrix and type(tst) is SLIMatrix
    for half in (trn, tst):
        assert (half.nUsers, half.nItems) == (data.nUsers, data.nItems)
        assert half.user2id == data.user2id and half.item2id == data.item2id
        assert np.array_equal(half.id2item, data.id2item) and np.array_equal(half.id2user, data.id2user)
    from split_cases import handle_rows
    src = handle_rows(lib, data.handle, free=False)
    R = sp.csr_matrix((src[2], src[1], src[0]), shape=(data.nUsers, data.nItems))
    want = split_rows(R, LEAVE_OUT, 2, 1, 2, 1, SEED)
    assert_same_rows(handle_rows(lib, trn.handle, free=False), want[0], "train")
    assert_same_rows(handle_rows(lib, tst.handle, free=False), want[1], "test")
    assert want[1][1].size > 0
    with pytest.raises(TypeError, match="could not be split"):
        data.split(mode="folds", nfolds=1)
