"""SLIMGPU_MatrixSplit (include/slim_gpu_split.h, slim_amd/csrc/split.hip): the split made where the staged matrix
lies.  The bar: its test rows, and its train rows read back through the column view, are SLIMGPU_SplitHost's and the
numpy restatement's (tests/split_cases.py) bit for bit, on every lane mapping of the two passes; nothing goes up and
only the test half comes down; a model learnt on the train half is the model learnt on the host split's train rows."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import scipy.sparse as sp

from slim_amd import _lib
from slim_amd.constants import SLIM_ERROR_INPUT, SLIM_OK
from slim_amd.engine import KERNEL_AUTO, DeviceMatrix, eval_stats
from split_cases import FOLDS, LEAVE_OUT, assert_same_rows, edge_lengths, host_split, rows_matrix, split_rows, takes_part

pytestmark = pytest.mark.gpu

SEED = 20240917
MODE = {LEAVE_OUT: "leave_out", FOLDS: "folds"}
SOURCE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "slim_amd", "csrc", "split.hip")


def source_constant(name):
    """A `constexpr int name = value;` of split.hip: the tests build their rows from the kernels' own edges."""
    with open(SOURCE) as f:
        m = re.search(r"constexpr int %s = (\d+);" % name, f.read())
    assert m, "split.hip no longer names " + name
    return int(m.group(1))


SHORT_ROW = source_constant("kSplitShortRow")
WAVE_ROW = source_constant("kSplitWaveRow")
LONG_PIECE = source_constant("kSplitLongPiece")


def sorted_rows(ptr, ind, val, shape):
    M = sp.csr_matrix((np.ones(ind.size, np.float32) if val is None else val, ind, ptr), shape=shape)
    M.sort_indices()
    return M


def check_split(R, mode, F, f, h, m, binary=False, resplit=False):
    """One device split against the host call and the restatement; returns the device train matrix's stats."""
    lib = _lib.load()
    R = sp.csr_matrix(R)
    st, h_trn, h_tst = host_split(lib, R, mode, F, f, h, m, SEED, binary=binary)
    assert st == SLIM_OK, _lib.last_error()
    want_trn, want_tst = split_rows(R, mode, F, f, h, m, SEED, binary=binary)
    assert_same_rows(h_trn, want_trn, "host train rows")
    assert_same_rows(h_tst, want_tst, "host test rows")
    mat = DeviceMatrix.from_scipy(R, binary=binary)
    trn, tst = mat.split(mode=MODE[mode], nfolds=F, fold=f, nheld=h, minkeep=m, seed=SEED)
    stats = eval_stats()
    # the test half, as it came down: order and values included
    got_tst = (tst.indptr.astype(np.int64), tst.indices, None if binary else tst.data)
    assert_same_rows(got_tst, want_tst, "device test rows")
    assert tst.shape[0] == R.shape[0]
    # the train half, read back through the column view and transposed
    assert (trn.nrows, trn.nnz) == (R.shape[0], int(want_trn[0][-1]))
    assert trn.ncols == max(int(want_trn[1].max()) + 1 if want_trn[1].size else 0, 1)
    colptr, colind, colval, _ = trn.column_view()
    back = sp.csc_matrix((np.ones(colind.size, np.float32) if binary else colval, colind, colptr),
                         shape=(trn.nrows, trn.ncols)).tocsr()
    back.sort_indices()
    want = sorted_rows(want_trn[0], want_trn[1], want_trn[2], (trn.nrows, trn.ncols))
    assert np.array_equal(back.indptr, want.indptr) and np.array_equal(back.indices, want.indices)
    assert back.data.tobytes() == want.data.tobytes()
    # no bytes up; down: one row pointer, the test rows (ids, and values unless binary) and the 12 bytes that the
    # staging of the train half reads for itself -- a second download of anything would show
    nt = int(want_tst[0][-1])
    assert stats["path"] == _lib.EVAL_PATH_SPLIT and stats["h2d_bytes"] == 0
    assert 0 < stats["d2h_bytes"] <= 8 * (R.shape[0] + 1) + (4 if binary else 8) * nt + 12
    if resplit:
        # the ORDER of the train rows: the train half split again, in two folds, brings every entry down in its row's
        # order, and must equal the host split of the host train rows
        T = sp.csr_matrix((R.shape[0], trn.ncols), dtype=np.float32)
        T.indptr, T.indices = h_trn[0].astype(np.int32), h_trn[1]
        T.data = np.ones(h_trn[1].size, np.float32) if binary else h_trn[2]
        for f2 in range(2):
            t2, s2 = trn.split(mode="folds", nfolds=2, fold=f2, minkeep=1, seed=SEED + 1)
            _, _, w2 = host_split(lib, T, FOLDS, 2, f2, 1, 1, SEED + 1, binary=binary)
            assert_same_rows((s2.indptr.astype(np.int64), s2.indices, None if binary else s2.data), w2,
                             "test rows of the train half split again")
            t2.close()
    trn.close()
    mat.close()
    return stats


@pytest.mark.parametrize("mode,F,f,h,m,binary", [
    (LEAVE_OUT, 5, 0, 3, 2, False),
    (LEAVE_OUT, 5, 4, 3, 2, False),
    (LEAVE_OUT, 2, 1, 1, 1, True),
    (LEAVE_OUT, 1, 0, 1, 1, False),
    (LEAVE_OUT, 64, 63, 2, 1, False),   # the largest selection: the 128 smallest keys of a row
    (FOLDS, 5, 2, 1, 2, False),
    (FOLDS, 2, 0, 1, 1, True),
])
def test_device_split_equals_host_split_and_restatement(mode, F, f, h, m, binary):
    # the matrix of the host tests (about 300 users, 1 500 items, the edge lengths of the rule) and a few rows more
    R = rows_matrix(edge_lengths(min(F, 5), min(h, 3), m) + [F * h + m - 1, F * h + m, 300, 2500], 1500, seed=11,
                    ratings=not binary)
    part = takes_part(R, mode, F, f, h, m, SEED)
    assert part.any() and (~part).any()
    assert 2 * part.sum() >= R.shape[0] or F * h > 15, "at least half of the users take part"
    check_split(R, mode, F, f, h, m, binary=binary, resplit=(f == 0 or binary))


def test_a_single_user():
    for L in (0, 1, 7, 300):
        R = rows_matrix([L], 1500, seed=L)
        check_split(R, LEAVE_OUT, 2, 1, 3, 1)
        check_split(R, FOLDS, 3, 1, 1, 1)


def test_only_empty_rows_except_one():
    lengths = [0] * 700
    lengths[413] = 90
    R = rows_matrix(lengths, 1500, seed=2)
    for mode, F, f, h in ((LEAVE_OUT, 3, 2, 2), (FOLDS, 3, 0, 1)):
        assert takes_part(R, mode, F, f, h, 1, SEED).sum() == 1
        check_split(R, mode, F, f, h, 1)


def test_rows_at_the_class_edges_and_beyond_a_workgroup_piece():
    # a row longer than the largest piece a workgroup takes at once (and than the floor of 40 000 over 60 000 items),
    # rows on both sides of every class edge, and rows of whole pieces
    longest = max(40000, 3 * LONG_PIECE + 17, WAVE_ROW + LONG_PIECE + 1)
    lengths = [longest, SHORT_ROW, SHORT_ROW + 1, WAVE_ROW, WAVE_ROW + 1, WAVE_ROW + LONG_PIECE, 2 * LONG_PIECE,
               LONG_PIECE + 1, 0, 3, 191, 192, 193, 256, 257, 129, 130, 5 * LONG_PIECE - 1]
    R = rows_matrix(lengths, 60000, seed=5)
    assert R.shape[1] >= 60000 and np.diff(R.indptr).max() > LONG_PIECE
    for mode, F, f, h, m in ((LEAVE_OUT, 64, 63, 2, 1), (LEAVE_OUT, 1, 0, 1, 1), (LEAVE_OUT, 4, 2, 32, 2),
                             (FOLDS, 5, 3, 1, 1)):
        assert takes_part(R, mode, F, f, h, m, SEED).any()
        check_split(R, mode, F, f, h, m, resplit=(F == 64))


def test_more_short_rows_than_one_grid_stride_step():
    # the short-row form takes 16 rows per workgroup on at most 8 workgroups per compute unit: 70 000 rows and more
    # are several steps of its grid-stride loop on 256 compute units
    nrows, ncols = 70001, 1500
    assert nrows > 256 * 8 * (256 // 16)
    rng = np.random.default_rng(9)
    lens = rng.integers(0, 13, nrows)
    lens[-1], lens[0], lens[40000] = 12, SHORT_ROW, SHORT_ROW + 1
    ptr = np.concatenate(([0], np.cumsum(lens)))
    rows = np.repeat(np.arange(nrows), lens)
    pos = np.arange(ptr[-1]) - np.repeat(ptr[:-1], lens)
    # distinct ids per row in no order: a stride coprime to ncols from a random start
    ind = ((rng.integers(0, ncols, nrows)[rows] + pos * 7919) % ncols).astype(np.int32)
    R = sp.csr_matrix((nrows, ncols), dtype=np.float32)
    R.indptr, R.indices, R.data = ptr.astype(np.int32), ind, rng.integers(1, 6, ind.size).astype(np.float32)
    for mode, F, f, h, m in ((LEAVE_OUT, 3, 1, 2, 1), (FOLDS, 3, 2, 1, 2)):
        part = takes_part(R, mode, F, f, h, m, SEED)
        assert part[-1] or mode == FOLDS
        assert part.sum() > nrows // 4 and (~part).sum() > nrows // 8
        check_split(R, mode, F, f, h, m)


def test_refusals(monkeypatch):
    lib = _lib.load()
    R = rows_matrix([5, 9, 0, 20], 64, seed=1)
    mat = DeviceMatrix.from_scipy(R)
    for spec, word in (((2, 2, 0, 1, 1), "mode"), ((FOLDS, 1, 0, 1, 1), "nfolds"), ((LEAVE_OUT, 2, 2, 1, 1), "fold 2"),
                       ((LEAVE_OUT, 2, 0, 0, 1), "nheld"), ((LEAVE_OUT, 2, 0, 1, 0), "minkeep"),
                       ((LEAVE_OUT, 65, 0, 2, 1), "nfolds * nheld is 130")):
        s = _lib.Split(*spec, SEED)
        trn, tst = C.c_void_p(0x1234), C.c_void_p(0x5678)
        assert lib.SLIMGPU_MatrixSplit(mat.handle, C.byref(s), C.byref(trn), C.byref(tst)) == SLIM_ERROR_INPUT
        assert word in _lib.last_error() and "SLIMGPU_MatrixSplit" in _lib.last_error()
        assert (trn.value, tst.value) == (0x1234, 0x5678)
    mat.close()
    # a matrix whose repeated pairs were merged at staging: its rows are not the caller's
    monkeypatch.setenv("SLIM_GPU_DUPLICATES", "sum")
    D = sp.csr_matrix((2, 8), dtype=np.float32)
    D.indptr, D.indices, D.data = np.array([0, 3, 5], np.int32), np.array([4, 1, 4, 2, 3], np.int32), np.ones(5, np.float32)
    merged = DeviceMatrix.from_scipy(D)
    with pytest.raises(ValueError, match="merged"):
        merged.split(mode="leave_out", nfolds=1, nheld=1)
    merged.close()


def test_a_model_learnt_on_the_train_half_is_the_host_splits_model(ml100k):
    def views(h):  # both views of a host model, copied
        v = C.cast(h, C.POINTER(_lib.CsrView)).contents
        n = int(v.ncols)
        cp = np.ctypeslib.as_array(v.colptr, shape=(n + 1,)).copy()
        rp = np.ctypeslib.as_array(v.rowptr, shape=(n + 1,)).copy()
        nnz = int(cp[-1])
        return [cp, rp] + [np.ctypeslib.as_array(p, shape=(nnz,)).copy() for p in (v.colind, v.colval, v.rowind, v.rowval)]

    R, _ = ml100k
    lib = _lib.load()
    spec = dict(mode="leave_out", nfolds=3, fold=1, nheld=1, minkeep=1, seed=SEED)
    mat = DeviceMatrix.from_scipy(R)
    trn, tst = mat.split(**spec)
    st, h_trn, h_tst = host_split(lib, R, LEAVE_OUT, 3, 1, 1, 1, SEED)
    assert st == SLIM_OK and tst.nnz == int(h_tst[0][-1]) > R.shape[0] // 2
    T = sp.csr_matrix((R.shape[0], int(h_trn[1].max()) + 1), dtype=np.float32)
    T.indptr, T.indices, T.data = h_trn[0].astype(np.int32), h_trn[1], h_trn[2]
    ref = DeviceMatrix.from_scipy(T)
    kw = dict(l1r=1.0, l2r=1.0, optTol=1e-7, niters=200, seed=1, kernel=KERNEL_AUTO)
    models = []
    for m in (trn, ref):
        d, stats = m.learn_resident(**kw)
        models.append((d, d.fetch(return_handle=True), stats["kernel"]))
    assert models[0][2] == models[1][2] and models[0][0].nnz > 0
    for x, y in zip(views(models[0][1]), views(models[1][1])):
        assert x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes()
    for d, hmodel, _ in models:
        lib.SLIM_FreeModel(C.byref(C.c_void_p(hmodel)))
        d.free()
    for m in (trn, ref, mat):
        m.close()
