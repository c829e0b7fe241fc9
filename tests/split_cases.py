"""The split of include/slim_gpu_split.h restated in numpy, written from the header's text (never from the C++), and
the matrices the split tests share.  mix64, G and key are those of tests/sampled_cases.py, which restates the
sampler's hash from include/slim_gpu_sample.h (entry_keys is key() for every entry at once)."""
import ctypes as C

import numpy as np
import scipy.sparse as sp

from sampled_cases import G, U, mix64
from slim_amd import _lib
from slim_amd.constants import SLIM_OK

LEAVE_OUT, FOLDS = 0, 1


def mulhi64(a, b):
    """The upper 64 bits of the 128-bit product a * b, per element, for b below 2^32 (exact in 64-bit pieces)."""
    a = np.asarray(a, U)
    hi, lo = a >> U(32), a & U(0xFFFFFFFF)
    return (hi * U(b) + ((lo * U(b)) >> U(32))) >> U(32)


def entry_keys(R, seed):
    """(user of every stored entry, its position in the row, key(seed, user, item)), for all entries at once."""
    lens = np.diff(R.indptr)
    rows = np.repeat(np.arange(R.shape[0]), lens)
    pos = np.arange(R.indices.size) - np.repeat(R.indptr[:-1], lens)
    with np.errstate(over="ignore"):
        b = mix64(U(seed) + G * (rows.astype(U) + U(1)))                # base(seed, u)
        k = mix64(b + G * (R.indices.astype(U) + U(1)))                 # key(seed, u, i)
    return rows, pos, k


def held_entries(R, mode, F, f, h, m, seed):
    """The rule of the header: a boolean per stored entry of R (scipy CSR, rows as stored), True = held out in
    fold f."""
    R = sp.csr_matrix(R)
    lens = np.diff(R.indptr)
    rows, pos, k = entry_keys(R, seed)
    if mode == LEAVE_OUT:
        # every row ordered by (key, item, position), ascending (lexsort: the last key is the primary one); a user
        # takes part when L >= F * h + m and holds out ranks [f * h, (f + 1) * h)
        order = np.lexsort((pos, R.indices, k, rows))
        rank = np.empty(order.size, np.int64)
        rank[order] = np.arange(order.size) - np.repeat(R.indptr[:-1], lens)
        return (lens >= F * h + m)[rows] & (rank >= f * h) & (rank < (f + 1) * h)
    # entry (u, i) belongs to fold mulhi64(key, F); a user takes part in fold f with >= m outside and >= 1 inside
    inside = mulhi64(k, F) == U(f)
    cnt = np.bincount(rows[inside], minlength=R.shape[0])
    return inside & ((cnt >= 1) & (lens - cnt >= m))[rows]


def split_rows(R, mode, F, f, h, m, seed, binary=False):
    """(train, test) as (indptr, indices, data-or-None) triples: both keep the source row order and values, both
    have the source's number of rows."""
    R = sp.csr_matrix(R)
    held = held_entries(R, mode, F, f, h, m, seed)
    rows = np.repeat(np.arange(R.shape[0]), np.diff(R.indptr))
    out = []
    for sel in (~held, held):
        ptr = np.concatenate(([0], np.cumsum(np.bincount(rows[sel], minlength=R.shape[0])))).astype(np.int64)
        out.append((ptr, R.indices[sel].astype(np.int32), None if binary else R.data[sel].astype(np.float32)))
    return tuple(out)


def takes_part(R, mode, F, f, h, m, seed):
    """Per user, whether it takes part in fold f (it holds something out)."""
    R = sp.csr_matrix(R)
    rows = np.repeat(np.arange(R.shape[0]), np.diff(R.indptr))
    return np.bincount(rows[held_entries(R, mode, F, f, h, m, seed)], minlength=R.shape[0]) > 0


def rows_matrix(lengths, ncols, seed, ratings=True):
    """A scipy CSR with rows of exactly these lengths: distinct ids in random (unsorted) order, ratings 1-5 or ones.
    A row draws from [0, ncols); one longer than ncols / 2 draws from the first 2 * length ids instead, so that it
    holds no id twice (the 5 000-entry row of a 1 500-item matrix)."""
    rng = np.random.default_rng(seed)
    ptr = np.concatenate(([0], np.cumsum(lengths))).astype(np.int64)
    ind = np.concatenate([rng.permutation(max(ncols, 2 * n))[:n] for n in lengths] +
                         [np.zeros(0, np.int64)]).astype(np.int32)
    val = (rng.integers(1, 6, ind.size) if ratings else np.ones(ind.size)).astype(np.float32)
    M = sp.csr_matrix((len(lengths), max(ncols, int(ind.max()) + 1 if ind.size else 0)), dtype=np.float32)
    M.indptr, M.indices, M.data = ptr.astype(np.int32 if ptr[-1] < 2 ** 31 else np.int64), ind, val
    return M


def edge_lengths(F, h, m, nusers=300):
    """About 300 row lengths: the edges the issue lists (0, 1, need - 1, need, 63, 64, 65, one row of 5 000), rows
    around the kernels' own class edges, and a spread in which most users take part and some cannot."""
    need = F * h + m
    rng = np.random.default_rng(1000 * F + 10 * h + m)
    fixed = [0, 1, max(need - 1, 0), need, 63, 64, 65, 5000, 16, 17, 2, 15, 128, 129, 1024, 1025, 0, 3]
    rest = rng.integers(0, 120, nusers - len(fixed)).tolist()
    lengths = fixed + rest
    return [int(x) for x in np.array(lengths)[rng.permutation(len(lengths))]]


def host_split(lib, R, mode, F, f, h, m, seed, binary=False):
    """SLIMGPU_SplitHost on a scipy matrix's rows: ((ptr, ind, val), (ptr, ind, val)), val None for binary."""
    R = sp.csr_matrix(R)
    ptr = np.ascontiguousarray(R.indptr, np.intp)
    ind = np.ascontiguousarray(R.indices, np.int32)
    val = None if binary else np.ascontiguousarray(R.data, np.float32)
    h_in = C.c_void_p()
    assert lib.Py_csr_wrapper(R.shape[0], ptr, ind, None if val is None else val.ctypes.data_as(C.c_void_p),
                              C.byref(h_in)) == SLIM_OK
    spec = _lib.Split(mode, F, f, h, m, seed)
    trn, tst = C.c_void_p(), C.c_void_p()
    st = lib.SLIMGPU_SplitHost(h_in, C.byref(spec), C.byref(trn), C.byref(tst))
    lib.Py_csr_free(h_in)
    if st != SLIM_OK:
        return st, None, None
    out = tuple(handle_rows(lib, x) for x in (trn, tst))
    return st, out[0], out[1]


def handle_rows(lib, handle, free=True):
    """(indptr, indices, data-or-None) copied out of a host handle's row view."""
    view = C.cast(handle, C.POINTER(_lib.CsrView)).contents
    n = int(view.nrows)
    ptr = np.ctypeslib.as_array(view.rowptr, shape=(n + 1,)).astype(np.int64)
    nnz = int(ptr[-1])
    ind = np.ctypeslib.as_array(view.rowind, shape=(nnz,)).copy() if nnz else np.zeros(0, np.int32)
    val = None
    if view.rowval:
        val = np.ctypeslib.as_array(view.rowval, shape=(nnz,)).copy() if nnz else np.zeros(0, np.float32)
    if free:
        lib.Py_csr_free(handle)
    return ptr, ind, val


def assert_same_rows(got, want, what):
    assert np.array_equal(got[0], want[0]), what + ": row pointers differ"
    assert np.array_equal(got[1], want[1]), what + ": ids differ"
    assert (got[2] is None) == (want[2] is None), what + ": one side carries values, the other none"
    if want[2] is not None:
        assert got[2].tobytes() == want[2].tobytes(), what + ": values differ"
