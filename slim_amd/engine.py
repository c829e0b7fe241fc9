"""Python handle on the engine extensions of libslim.so (SLIMGPU_*, include/slim_gpu.h):
a training matrix staged in HBM and repeated / column-sharded CD solves on it.

Used by bench.py, the multi-GPU helper (slim_amd/distributed.py) and the parity
tests.  Device buffers are passed as raw pointers (``tensor.data_ptr()``); torch is
plumbing only and is not imported here.
"""
import ctypes as C

import numpy as np
import scipy.sparse as sp

from . import _lib
from .constants import SLIM_NOPTIONS, SLIM_OK, Opt

KERNEL_AUTO, KERNEL_WAVE_LDS, KERNEL_WAVE_HBM, KERNEL_TILE, KERNEL_TILE16, KERNEL_GRAM = 0, 1, 2, 3, 4, 5
KERNEL_GRAM_FSLIM = 6   # FSLIM in item space (nnbrs > 0, ratings > 0); never chosen by KERNEL_AUTO


def make_options(l1r=1.0, l2r=1.0, optTol=1e-7, niters=10000, seed=1, col_begin=None,
                 col_end=None, kernel=KERNEL_AUTO, device=None, dbglvl=0, cluster=None, nnbrs=0,
                 simtype=0, heavy_tiles=None, heavy_cluster=None, ngpus=None, shard=None):
    iopt = np.full(SLIM_NOPTIONS, -1, dtype=np.int32)
    dopt = np.full(SLIM_NOPTIONS, -1.0, dtype=np.float64)
    iopt[Opt.DBGLVL] = dbglvl
    iopt[Opt.MAXNITERS] = niters
    iopt[Opt.GPU_SEED] = seed
    iopt[Opt.GPU_KERNEL] = kernel
    iopt[Opt.NNBRS] = nnbrs
    iopt[Opt.SIMTYPE] = simtype
    if col_begin is not None:
        iopt[Opt.GPU_COLBEGIN] = col_begin
    if col_end is not None:
        iopt[Opt.GPU_COLEND] = col_end
    if device is not None:
        iopt[Opt.GPU_DEVICE] = device
    if cluster is not None:
        iopt[Opt.GPU_CLUSTER] = cluster
    if heavy_tiles is not None:
        iopt[Opt.GPU_HEAVYTILES] = heavy_tiles
    if heavy_cluster is not None:
        iopt[Opt.GPU_HEAVYCLUSTER] = heavy_cluster
    if ngpus is not None:
        iopt[Opt.GPU_NGPUS] = ngpus
    if shard is not None:  # (index, count)
        iopt[Opt.GPU_SHARDINDEX], iopt[Opt.GPU_SHARDCOUNT] = shard
    dopt[Opt.L1R], dopt[Opt.L2R], dopt[Opt.OPTTOL] = l1r, l2r, optTol
    return iopt, dopt


def model_to_scipy(lib, handle, free=True):
    """Copy a model handle (slim_csr_t) into a scipy CSC matrix (column iC =
    regressors of item iC) and optionally release the handle."""
    view = C.cast(handle, C.POINTER(_lib.CsrView)).contents
    n = int(view.ncols)
    colptr = np.ctypeslib.as_array(view.colptr, shape=(n + 1,)).astype(np.int64)
    nnz = int(colptr[-1])
    if nnz:
        colind = np.ctypeslib.as_array(view.colind, shape=(nnz,)).copy()
        colval = np.ctypeslib.as_array(view.colval, shape=(nnz,)).copy()
    else:
        colind = np.zeros(0, np.int32)
        colval = np.zeros(0, np.float32)
    W = sp.csc_matrix((colval, colind, colptr), shape=(n, n))
    if free:
        h = C.c_void_p(handle if isinstance(handle, int) else handle.value)
        lib.SLIM_FreeModel(C.byref(h))
    return W


class ColumnStats(object):
    def __init__(self, lib, ncols):
        self.nacols = np.zeros(ncols, np.int32)
        self.sweeps = np.zeros(ncols, np.int32)
        self.conv = np.zeros(ncols, np.int32)
        self.G = np.zeros(ncols, np.int64)
        self.D = np.zeros(ncols, np.int64)
        self.U = np.zeros(ncols, np.int64)
        rc = lib.SLIMGPU_LastColumnStats(ncols, *[a.ctypes.data_as(C.c_void_p) for a in
                                                  (self.nacols, self.sweeps, self.conv, self.G,
                                                   self.D, self.U)])
        if rc != SLIM_OK:
            raise RuntimeError("SLIMGPU_LastColumnStats failed (%d)" % rc)


class ResidentModel(object):
    """A learned model that stays in HBM (SLIMGPU_LearnResident): both views on the device, usable as
    the next solve's warm start without an upload; `fetch()` forms SLIM_Learn's host model."""

    def __init__(self, lib, handle):
        self._lib = lib
        self.handle = C.c_void_p(handle)

    @property
    def nnz(self):
        return int(self._lib.SLIMGPU_ModelNnz(self.handle))

    def fetch_begin(self):
        """Start the copy to the host on its own stream + host thread (runs beside the next solve)."""
        st = self._lib.SLIMGPU_ModelFetchBegin(self.handle)
        if st != SLIM_OK:
            raise RuntimeError("SLIMGPU_ModelFetchBegin failed (%d): %s" % (st, _lib.last_error()))

    def fetch(self, return_handle=False):
        """The host model (joins a begun fetch): scipy CSC, or the slim_t handle (SLIM_FreeModel)."""
        st = C.c_int32(0)
        h = self._lib.SLIMGPU_ModelFetch(self.handle, C.byref(st))
        if not h:
            raise RuntimeError("SLIMGPU_ModelFetch failed (%d): %s" % (st.value, _lib.last_error()))
        return h if return_handle else model_to_scipy(self._lib, h)

    def predict(self, device_matrix, nrcmds=10, users=None, return_counts=False, filter=None):
        """SLIMGPU_MatrixPredictLists: top-N (1 <= nrcmds <= 4096) of every row of the staged matrix, or of
        the rows in `users` (strictly ascending ids), scored in HBM (only the lists come down).  Returns
        (ids, scores) of shape [rows, nrcmds], and the list lengths with return_counts; ids are -1 and
        scores 0 beyond a user's list.  filter: an ItemFilter (DeviceMatrix.item_filter) that narrows the
        candidates (SLIMGPU_MatrixPredictListsFiltered); its exclusion rows go by user id."""
        nrcmds = int(nrcmds)
        if users is not None:
            users = np.ascontiguousarray(users, np.int32)
        n = device_matrix.nrows if users is None else users.size
        ids = np.full(n * nrcmds, -1, np.int32)
        scores = np.zeros(n * nrcmds, np.float32)
        counts = np.zeros(n, np.int32)
        who = (0 if users is None else users.size, None if users is None else users.ctypes.data_as(C.c_void_p))
        out = (ids.ctypes.data_as(C.c_void_p), scores.ctypes.data_as(C.c_void_p), counts.ctypes.data_as(C.c_void_p))
        if filter is None:
            st = self._lib.SLIMGPU_MatrixPredictLists(nrcmds, self.handle, device_matrix.handle, *(who + out))
        else:
            st = self._lib.SLIMGPU_MatrixPredictListsFiltered(nrcmds, self.handle, device_matrix.handle,
                                                              *(who + (filter.handle,) + out))
        if st != SLIM_OK:
            raise RuntimeError("SLIMGPU_MatrixPredictLists%s failed (%d): %s"
                               % ("" if filter is None else "Filtered", st, _lib.last_error()))
        out = (ids.reshape(n, nrcmds), scores.reshape(n, nrcmds))
        return out + (counts,) if return_counts else out

    def exposure(self, device_matrix, nrcmds=10, cutoffs=None, users=None, filter=None, fmarker=None):
        """SLIMGPU_MatrixPredictExposure: how often every item stands in the lists predict() would return with the
        same nrcmds / users / filter, cut at each of `cutoffs` (ascending, at most 8, the last <= nrcmds; None:
        (nrcmds,)).  The lists are counted where they are made: only the counters come down.  fmarker (0 head /
        1 tail per item) gives the tail share.  Returns (E [len(cutoffs), ncols] uint32, summaries): one dict per
        cutoff with the fields of slimgpu_exposure_t (include/slim_gpu_exposure.h) and "nrcmds"."""
        nrcmds = int(nrcmds)
        cut = _cutoff_array((nrcmds,) if cutoffs is None else cutoffs)
        if users is not None:
            users = np.ascontiguousarray(users, np.int32)
        fm = None if fmarker is None else np.ascontiguousarray(fmarker, np.int32)
        E = np.zeros((max(cut.size, 1), device_matrix.ncols), np.uint32)
        summ = (_lib.Exposure * max(cut.size, 1))()
        st = self._lib.SLIMGPU_MatrixPredictExposure(
            device_matrix.handle, self.handle, nrcmds, 0 if users is None else users.size, _ptr(users),
            None if filter is None else filter.handle, _ptr(fm), 0 if fm is None else fm.size, cut.size, _ptr(cut),
            _ptr(E), C.cast(summ, C.c_void_p))
        if st != SLIM_OK:
            raise RuntimeError("SLIMGPU_MatrixPredictExposure failed (%d): %s" % (st, _lib.last_error()))
        return E[:cut.size], _exposure_dicts(summ, cut)

    def score_candidates(self, device_matrix, cset, users=None, nrcmds=None):
        """SLIMGPU_MatrixScoreCandidates: the 1-vs-k scores of the candidate rows of a CandidateSet
        (DeviceMatrix.candidate_set) for every row of the staged matrix, or for the rows in `users` (strictly
        ascending ids; the candidate row of a user goes by its id).  Returns the slot scores, laid out like the set
        (cset.indptr; 0 in the rows of users not selected), and with nrcmds also (ids, scores, counts) of shape
        [rows, nrcmds]: every row in order (score descending, then slot), ids -1 and scores 0 beyond a list."""
        if users is not None:
            users = np.ascontiguousarray(users, np.int32)
        n = device_matrix.nrows if users is None else users.size
        k = 0 if nrcmds is None else int(nrcmds)
        slot = np.zeros(max(cset.size, 1), np.float32)
        ids = np.full(max(n * k, 1), -1, np.int32)
        scores = np.zeros(max(n * k, 1), np.float32)
        counts = np.zeros(max(n, 1), np.int32)
        st = self._lib.SLIMGPU_MatrixScoreCandidates(
            self.handle, device_matrix.handle, cset.handle, 0 if users is None else users.size,
            None if users is None else users.ctypes.data_as(C.c_void_p), k, slot.ctypes.data_as(C.c_void_p),
            ids.ctypes.data_as(C.c_void_p), scores.ctypes.data_as(C.c_void_p), counts.ctypes.data_as(C.c_void_p))
        if st != SLIM_OK:
            raise RuntimeError("SLIMGPU_MatrixScoreCandidates failed (%d): %s" % (st, _lib.last_error()))
        slot = slot[:cset.size]
        if nrcmds is None:
            return slot
        return slot, (ids[:n * k].reshape(n, k), scores[:n * k].reshape(n, k), counts[:n])

    def explain(self, device_matrix, cset, users=None, nwhy=3):
        """SLIMGPU_MatrixExplainCandidates: which history items carry the score of every candidate of a CandidateSet
        (include/slim_gpu_explain.h), for every row of the staged matrix or for the rows in `users` (strictly
        ascending ids; the candidate row of a user goes by its id).  Returns (why_items, why_terms, support) laid out
        like the set: [entries, nwhy], [entries, nwhy] and [entries].  support counts all the terms of a slot; a slot
        holds its min(nwhy, support) largest terms (term descending, then history position) with the engine ids of
        their history items, -1 and 0 beyond them and in the rows of users not selected."""
        nwhy = int(nwhy)
        if users is not None:
            users = np.ascontiguousarray(users, np.int32)
        n = max(cset.size, 1)
        items = np.full(n * max(nwhy, 1), -1, np.int32)
        terms = np.zeros(n * max(nwhy, 1), np.float32)
        support = np.zeros(n, np.int32)
        st = self._lib.SLIMGPU_MatrixExplainCandidates(
            self.handle, device_matrix.handle, cset.handle, 0 if users is None else users.size,
            None if users is None else users.ctypes.data_as(C.c_void_p), nwhy, items.ctypes.data_as(C.c_void_p),
            terms.ctypes.data_as(C.c_void_p), support.ctypes.data_as(C.c_void_p))
        if st != SLIM_OK:
            raise RuntimeError("SLIMGPU_MatrixExplainCandidates failed (%d): %s" % (st, _lib.last_error()))
        return (items[:cset.size * nwhy].reshape(cset.size, nwhy), terms[:cset.size * nwhy].reshape(cset.size, nwhy),
                support[:cset.size])

    def explain_lists(self, device_matrix, ids, counts, nwhy=3, users=None):
        """Explains lists that predict() returned: `ids` [positions, nrcmds] and `counts` [positions] as predict gave
        them for `users` (None: every row).  The candidate set holds, for the user of position q, the first counts[q]
        ids of row q; it is explained and freed.  Returns (indptr, why_items, why_terms, support): entry
        indptr[q] + r is item ids[q, r], with explain()'s three arrays."""
        ids = np.asarray(ids, np.int32)
        counts = np.asarray(counts, np.int64).ravel()
        if users is not None:
            users = np.ascontiguousarray(users, np.int32)
        who = np.arange(device_matrix.nrows) if users is None else users
        if ids.ndim != 2 or ids.shape[0] != who.size or counts.size != who.size:
            raise ValueError("explain_lists: ids [positions, nrcmds] and counts [positions] for %d positions" % who.size)
        rows = np.zeros(device_matrix.nrows, np.int64)
        rows[who] = counts
        rowptr = np.concatenate((np.zeros(1, np.int64), np.cumsum(rows)))
        keep = np.arange(ids.shape[1])[None, :] < counts[:, None]
        cset = CandidateSet(device_matrix.ncols, (rowptr, ids[keep]), lib=self._lib)  # (users ascend: row-major order)
        try:
            items, terms, support = self.explain(device_matrix, cset, users=users, nwhy=nwhy)
        finally:
            cset.close()
        return np.concatenate((np.zeros(1, np.int64), np.cumsum(counts))), items, terms, support

    def free(self):
        if self.handle:
            self._lib.SLIMGPU_ModelFree(C.byref(self.handle))
            self.handle = C.c_void_p(None)

    def __del__(self):
        try:
            self.free()
        except Exception:   # noqa: BLE001 -- interpreter shutdown
            pass


class ItemFilter(object):
    """A candidate filter of the top-N lists (SLIMGPU_FilterCreate, include/slim_gpu_filter.h) over `ncols`
    items; owns the handle.  allowed / blocked: item ids (at most one of the two; allowed=[] allows nothing);
    exclusions: a scipy matrix whose row u holds the items never shown to user u."""

    def __init__(self, ncols, allowed=None, blocked=None, exclusions=None, lib=None):
        if allowed is not None and blocked is not None:
            raise ValueError("item filter: pass at most one of allowed / blocked")
        self._lib = lib or _lib.load()
        self.handle = C.c_void_p()
        self.ncols = int(ncols)
        items = allowed if blocked is None else blocked
        if items is not None:   # (one spare element: an empty set still has an address)
            ids = np.ascontiguousarray(items, dtype=np.int32).ravel()
            buf = np.concatenate((ids, np.zeros(1, np.int32)))
        xusers, xptr, xind = 0, None, None
        if exclusions is not None:
            X = sp.csr_matrix(exclusions)
            xusers = X.shape[0]
            xptr = np.ascontiguousarray(X.indptr, dtype=np.int64)
            xind = np.concatenate((np.asarray(X.indices, dtype=np.int32), np.zeros(1, np.int32)))
        st = self._lib.SLIMGPU_FilterCreate(
            self.ncols, 0 if items is None else ids.size, None if items is None else buf.ctypes.data_as(C.c_void_p),
            0 if blocked is None else 1, xusers, None if xptr is None else xptr.ctypes.data_as(C.c_void_p),
            None if xind is None else xind.ctypes.data_as(C.c_void_p), C.byref(self.handle))
        if st != SLIM_OK:
            self.handle = C.c_void_p()
            raise ValueError("SLIMGPU_FilterCreate failed (%d): %s" % (st, _lib.last_error()))

    def close(self):
        if self.handle is not None and self.handle.value:
            self._lib.SLIMGPU_FilterFree(self.handle)
        self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:   # noqa: BLE001 -- interpreter shutdown
            pass


class CandidateSet(object):
    """Per-user candidate rows (SLIMGPU_CandSetCreate, include/slim_gpu_cand.h) over `ncols` items; owns the handle.
    rows: a scipy CSR taken as it is (its indptr / indices: no order, repeats and ids outside the items allowed),
    or the pair (indptr, indices).  Row u holds the candidates of user u."""

    def __init__(self, ncols, rows, lib=None):
        self._lib = lib or _lib.load()
        self.handle = C.c_void_p()
        self.ncols = int(ncols)
        indptr, indices = (rows.indptr, rows.indices) if sp.issparse(rows) else rows
        self.indptr = np.ascontiguousarray(indptr, dtype=np.int64).ravel()
        if self.indptr.size < 1:
            raise ValueError("candidate set: the row pointer needs at least one entry")
        self.nusers = self.indptr.size - 1
        # (one spare element: an empty set still has an address)
        ind = np.concatenate((np.asarray(indices, dtype=np.int32).ravel(), np.zeros(1, np.int32)))
        self.size = ind.size - 1
        st = self._lib.SLIMGPU_CandSetCreate(self.ncols, self.nusers, self.indptr.ctypes.data_as(C.c_void_p),
                                             ind.ctypes.data_as(C.c_void_p), C.byref(self.handle))
        if st != SLIM_OK:
            self.handle = C.c_void_p()
            raise ValueError("SLIMGPU_CandSetCreate failed (%d): %s" % (st, _lib.last_error()))

    @classmethod
    def from_handle(cls, handle, lib=None):
        """Adopt a set this class did not create (SLIMGPU_EvalSetSampleCandidates, SLIMGPU_CandSetSample); the object
        owns the handle from here on.  Only the row pointer is read: the ids of a set born on the device stay there
        until rows() asks."""
        self = cls.__new__(cls)
        self._lib = lib or _lib.load()
        self.handle = handle if isinstance(handle, C.c_void_p) else C.c_void_p(handle)
        nrows, ncols, size = C.c_int32(), C.c_int32(), C.c_int64()
        st = self._lib.SLIMGPU_CandSetInfo(self.handle, C.byref(nrows), C.byref(ncols), C.byref(size))
        if st != SLIM_OK:
            self.handle = None
            raise ValueError("SLIMGPU_CandSetInfo failed (%d): %s" % (st, _lib.last_error()))
        self.ncols, self.nusers, self.size = ncols.value, nrows.value, size.value
        self.indptr = np.zeros(self.nusers + 1, np.int64)
        st = self._lib.SLIMGPU_CandSetRows(self.handle, self.indptr.ctypes.data_as(C.c_void_p), None)
        if st != SLIM_OK:
            raise RuntimeError("SLIMGPU_CandSetRows failed (%d): %s" % (st, _lib.last_error()))
        return self

    def rows(self):
        """SLIMGPU_CandSetRows: (indptr, indices), copies of the set's rows (a set born on the device brings its ids
        down on the first call)."""
        ind = np.zeros(self.size + 1, np.int32)
        st = self._lib.SLIMGPU_CandSetRows(self.handle, None, ind.ctypes.data_as(C.c_void_p))
        if st != SLIM_OK:
            raise RuntimeError("SLIMGPU_CandSetRows failed (%d): %s" % (st, _lib.last_error()))
        return self.indptr.copy(), ind[:self.size]

    def close(self):
        if self.handle is not None and self.handle.value:
            self._lib.SLIMGPU_CandSetFree(self.handle)
        self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:   # noqa: BLE001 -- interpreter shutdown
            pass


def popularity_weights(R, alpha=1.0):
    """Sampling weights from item popularity, for the `weights` of the samplers: the column counts of R (uint32) for
    alpha == 1, else rint(counts ** alpha * 1024) -- alpha = 0.75 is word2vec's.  A host convenience: the array it
    returns is the contract, not the exponent."""
    R = sp.csr_matrix(R)
    counts = np.bincount(R.indices, minlength=R.shape[1]).astype(np.int64)
    if alpha == 1:
        return counts.astype(np.uint32)
    w = np.rint(counts.astype(np.float64) ** float(alpha) * 1024.0)
    if w.size and w.max() >= 2.0 ** 32:
        raise ValueError("popularity_weights: a weight reaches 2^32")
    return w.astype(np.uint32)


def _sampling_weights(weights, ncols):
    """weights of the samplers -> (weighted, uint32 array or None): None: uniform; "popularity": NULL weights; else
    ncols non-negative integers below 2^32."""
    if weights is None:
        return False, None
    if isinstance(weights, str):
        if weights != "popularity":
            raise ValueError('weights: None, "popularity" or an array of ncols integers, not %r' % weights)
        return True, None
    w = np.asarray(weights)
    if w.ndim != 1 or w.size != ncols:
        raise ValueError("weights: %d items need %d weights, not an array of shape %s" % (ncols, ncols, w.shape))
    if w.dtype.kind not in "iu" or (w.size and (int(w.min()) < 0 or int(w.max()) >= 2 ** 32)):
        raise ValueError("weights: non-negative integers below 2^32")
    return True, np.ascontiguousarray(w, dtype=np.uint32)


def sample_candidates(trn, tst, nnegs, seed=1, users=None, ncols=None, lib=None, weights=None):
    """SLIMGPU_CandSetSample (include/slim_gpu_sample.h): the 1-vs-k candidate set made on the host -- per user with a
    test row `nnegs` sampled items outside its history and test row, then the test row.  trn / tst: scipy matrices,
    one row per user; users: ascending user ids (None: every user); ncols: the catalogue (None: the wider of the
    two).  weights (SLIMGPU_CandSetSampleWeighted): None: uniform; "popularity": in proportion to the entries trn has
    of every item; an array of ncols non-negative integers below 2^32 (popularity_weights makes one).  The rows equal
    those of Evaluator.sample_candidates for the same seed and weights."""
    lib = lib or _lib.load()
    trn, tst = sp.csr_matrix(trn), sp.csr_matrix(tst)
    ncols = max(trn.shape[1], tst.shape[1]) if ncols is None else int(ncols)
    weighted, w = _sampling_weights(weights, ncols)
    sel = None if users is None else np.ascontiguousarray(users, dtype=np.int32).ravel()
    ht, hs = _wrap_rows(lib, trn), _wrap_rows(lib, tst)
    h = C.c_void_p()
    name = "SLIMGPU_CandSetSampleWeighted" if weighted else "SLIMGPU_CandSetSample"
    args = (ncols, ht, hs, 0 if sel is None else sel.size, None if sel is None else sel.ctypes.data_as(C.c_void_p),
            int(nnegs), int(seed))
    try:
        if weighted:
            st = lib.SLIMGPU_CandSetSampleWeighted(*(args + (None if w is None else w.ctypes.data_as(C.c_void_p),
                                                             C.byref(h))))
        else:
            st = lib.SLIMGPU_CandSetSample(*(args + (C.byref(h),)))
    finally:
        lib.Py_csr_free(ht)
        lib.Py_csr_free(hs)
    if st != SLIM_OK:
        raise ValueError("%s failed (%d): %s" % (name, st, _lib.last_error()))
    return CandidateSet.from_handle(h, lib=lib)


def eval_stats(lib=None):
    """Counters of the most recent ModelEvaluate / MatrixPredict on this thread, as a dict."""
    st = _lib.EvalStats()
    (lib or _lib.load()).SLIMGPU_LastEvalStats(C.byref(st))
    return st.as_dict()


def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _cutoff_array(cutoffs):
    return np.ascontiguousarray(np.atleast_1d(np.asarray(cutoffs)), np.int32)


def _exposure_dicts(summ, cut):
    return [dict(summ[k].as_dict(), nrcmds=int(c)) for k, c in enumerate(cut)]


def _exposure_lists(ids, counts):
    ids = np.ascontiguousarray(ids, np.int32)
    if ids.ndim != 2:
        raise ValueError("list_exposure: ids is [lists, nrcmds]")
    if counts is not None:
        counts = np.ascontiguousarray(counts, np.int32).ravel()
        if counts.size != ids.shape[0]:
            raise ValueError("list_exposure: one count per list")
    return ids, counts


def list_exposure(ids, counts, ncols, cutoffs, pop=None, fmarker=None, lib=None):
    """SLIMGPU_ListExposure, on the host: E[k, i] = the places p < min(counts[q], cutoffs[k]) of the lists
    ids [lists, nrcmds] that hold item i (counts None: every list is full).  pop (uint32 per item) gives avg_pop,
    fmarker (0 head / 1 tail) the tail share.  Returns (E [len(cutoffs), ncols] uint32, summaries) as
    ResidentModel.exposure does."""
    lib = lib or _lib.load()
    ids, counts = _exposure_lists(ids, counts)
    cut = _cutoff_array(cutoffs)
    pop = None if pop is None else np.ascontiguousarray(pop, np.uint32)
    fm = None if fmarker is None else np.ascontiguousarray(fmarker, np.int32)
    if pop is not None and pop.size != ncols:
        raise ValueError("list_exposure: pop has one entry per item")
    E = np.zeros((max(cut.size, 1), max(int(ncols), 1)), np.uint32)
    summ = (_lib.Exposure * max(cut.size, 1))()
    st = lib.SLIMGPU_ListExposure(int(ncols), _ptr(pop), _ptr(fm), 0 if fm is None else fm.size, ids.shape[0],
                                  ids.shape[1], _ptr(ids), _ptr(counts), cut.size, _ptr(cut), _ptr(E),
                                  C.cast(summ, C.c_void_p))
    if st != SLIM_OK:
        raise RuntimeError("SLIMGPU_ListExposure failed (%d): %s" % (st, _lib.last_error()))
    return E[:cut.size], _exposure_dicts(summ, cut)


def _group_array(groups, what):
    groups = np.asarray(groups)
    if groups.ndim != 1 or groups.dtype.kind not in "iu":
        raise ValueError("%s: one integer group per user" % what)
    return np.ascontiguousarray(groups, np.int32)


def group_partition(groups, ngroups, users=None, nsel=None, lib=None):
    """SLIMGPU_GroupPartition, on the host: the definition of the per-group rows.  groups holds one group per user
    (-1: none); the positions are `users` (ascending ids) or, with users None, the first nsel users (default: all).
    Returns (order, offsets): order[offsets[g]:offsets[g + 1]] are the positions of group g, ascending."""
    lib = lib or _lib.load()
    groups = _group_array(groups, "group_partition")
    users = None if users is None else np.ascontiguousarray(users, np.int32).ravel()
    n = users.size if users is not None else (groups.size if nsel is None else int(nsel))
    order = np.zeros(max(n, 1), np.int32)
    offsets = np.zeros(max(int(ngroups), 0) + 1, np.int64)
    st = lib.SLIMGPU_GroupPartition(n, _ptr(users), groups.size, int(ngroups), _ptr(groups), _ptr(order),
                                    _ptr(offsets))
    if st != SLIM_OK:
        raise ValueError("SLIMGPU_GroupPartition failed (%d): %s" % (st, _lib.last_error()))
    return order[:int(offsets[-1])], offsets


def list_stats(lib=None):
    """Counters of the most recent PredictLists / ModelPredictLists / MatrixPredictLists on this thread."""
    st = _lib.ListStats()
    (lib or _lib.load()).SLIMGPU_LastListStats(C.byref(st))
    return st.as_dict()


def _wrap_rows(lib, M):
    """Host handle (Py_csr_wrapper) of a scipy matrix's rows; release with Py_csr_free."""
    M = sp.csr_matrix(M)
    ptr = np.ascontiguousarray(M.indptr, dtype=np.intp)
    ind = np.ascontiguousarray(M.indices, dtype=np.int32)
    val = np.ascontiguousarray(M.data, dtype=np.float32)
    h = C.c_void_p()
    st = lib.Py_csr_wrapper(M.shape[0], ptr, ind, val.ctypes.data_as(C.c_void_p), C.byref(h))
    if st != SLIM_OK:
        raise RuntimeError("Py_csr_wrapper failed (%d)" % st)
    return h


def _rows_to_scipy(lib, handle, ncols=None, free=True):
    """The row view of a host handle (slim_csr_t) as a scipy CSR matrix; a handle without values gives ones.
    ncols None: the handle's width (largest id + 1)."""
    view = C.cast(handle, C.POINTER(_lib.CsrView)).contents
    n = int(view.nrows)
    ptr = np.ctypeslib.as_array(view.rowptr, shape=(n + 1,)).astype(np.int64)
    nnz = int(ptr[-1])
    ind = np.ctypeslib.as_array(view.rowind, shape=(nnz,)).copy() if nnz else np.zeros(0, np.int32)
    if nnz and view.rowval:
        val = np.ctypeslib.as_array(view.rowval, shape=(nnz,)).copy()
    else:
        val = np.ones(nnz, np.float32)
    width = max(int(view.ncols), 0) if ncols is None else int(ncols)
    if free:
        lib.Py_csr_free(handle)
    return sp.csr_matrix((val, ind, ptr), shape=(n, width))


SPLIT_MODES = {"leave_out": _lib.SPLIT_LEAVE_OUT, "folds": _lib.SPLIT_FOLDS}


def make_split(mode="leave_out", nfolds=1, fold=0, nheld=1, minkeep=1, seed=1):
    """A slimgpu_split_t (include/slim_gpu_split.h, which states the rule).  mode: "leave_out" (every user that takes
    part holds out `nheld` entries per fold) or "folds" (entry (u, i) belongs to one of `nfolds` folds by its hash)."""
    if mode not in SPLIT_MODES and mode not in SPLIT_MODES.values():
        raise ValueError("split: mode is 'leave_out' or 'folds', not %r" % (mode,))
    return _lib.Split(SPLIT_MODES.get(mode, mode), int(nfolds), int(fold), int(nheld), int(minkeep),
                      int(seed) & 0xFFFFFFFFFFFFFFFF)


def split_host(R, mode="leave_out", nfolds=1, fold=0, nheld=1, minkeep=1, seed=1, binary=False, lib=None):
    """SLIMGPU_SplitHost: one interactions matrix R (scipy, one row per user, entries as stored) split on the host
    into (train, test), two scipy CSR matrices of R's shape with R's row order and values.  binary=True passes no
    values (the halves then carry ones).  The rows equal those of DeviceMatrix.split for the same parameters."""
    lib = lib or _lib.load()
    R = sp.csr_matrix(R)
    ptr = np.ascontiguousarray(R.indptr, dtype=np.intp)
    ind = np.ascontiguousarray(R.indices, dtype=np.int32)
    val = None if binary else np.ascontiguousarray(R.data, dtype=np.float32)
    h = C.c_void_p()
    st = lib.Py_csr_wrapper(R.shape[0], ptr, ind, _ptr(val), C.byref(h))
    if st != SLIM_OK:
        raise RuntimeError("Py_csr_wrapper failed (%d)" % st)
    spec = make_split(mode, nfolds, fold, nheld, minkeep, seed)
    trn, tst = C.c_void_p(), C.c_void_p()
    try:
        st = lib.SLIMGPU_SplitHost(h, C.byref(spec), C.byref(trn), C.byref(tst))
    finally:
        lib.Py_csr_free(h)
    if st != SLIM_OK:
        raise ValueError("SLIMGPU_SplitHost failed (%d): %s" % (st, _lib.last_error()))
    return _rows_to_scipy(lib, trn, R.shape[1]), _rows_to_scipy(lib, tst, R.shape[1])


class Evaluator(object):
    """The test set of a grid staged in HBM (SLIMGPU_EvalSetCreateAt): `evaluate(resident_model)` scores
    the model against the staged training matrix and brings down HR / ARHR only -- of the longest
    lists; `evaluate_at(resident_model)` gives the figures of every list length, from the same pass.
    Every call takes filter=<ItemFilter> (DeviceMatrix.item_filter): the candidates are then the filter's, a
    test entry it removes stays in the denominators and is a miss (rank 0, score 0); exclusion rows go by user id."""

    def __init__(self, lib, handle, matrix, cutoffs=(10,), indptr=None):
        self._lib = lib
        self.handle = C.c_void_p(handle)
        self._matrix = matrix      # borrowed by the eval set: keep it alive
        self.cutoffs = tuple(int(c) for c in cutoffs)
        self.indptr = indptr       # ranks(): where every position's test entries start

    def evaluate(self, model, filter=None):
        if filter is not None:  # (the last row of the filtered call: the longest lists)
            return {k: v for k, v in self.evaluate_at(model, filter=filter)[-1].items() if k != "nrcmds"}
        met = np.zeros(4, np.float64)
        nv = np.zeros(3, np.int32)
        st = self._lib.SLIMGPU_ModelEvaluate(self.handle, model.handle, met, nv)
        if st != SLIM_OK:
            raise RuntimeError("SLIMGPU_ModelEvaluate failed (%d): %s" % (st, _lib.last_error()))
        return {"hr": met[0], "hr_head": met[1], "hr_tail": met[2], "arhr": met[3],
                "nvalid": int(nv[0]), "nvalid_head": int(nv[1]), "nvalid_tail": int(nv[2])}

    def evaluate_at(self, model, filter=None):
        """SLIMGPU_ModelEvaluateAt(Filtered): one dict per list length (evaluate()'s keys and "nrcmds")."""
        n = len(self.cutoffs)
        met = np.zeros(4 * n, np.float64)
        nv = np.zeros(3 * n, np.int32)
        if filter is None:
            st = self._lib.SLIMGPU_ModelEvaluateAt(self.handle, model.handle, n, met, nv)
        else:
            st = self._lib.SLIMGPU_ModelEvaluateAtFiltered(self.handle, model.handle, filter.handle, n, met, nv)
        if st != SLIM_OK:
            raise RuntimeError("SLIMGPU_ModelEvaluateAt%s failed (%d): %s"
                               % ("" if filter is None else "Filtered", st, _lib.last_error()))
        return [{"nrcmds": c, "hr": met[4 * k], "hr_head": met[4 * k + 1], "hr_tail": met[4 * k + 2],
                 "arhr": met[4 * k + 3], "nvalid": int(nv[3 * k]), "nvalid_head": int(nv[3 * k + 1]),
                 "nvalid_tail": int(nv[3 * k + 2])} for k, c in enumerate(self.cutoffs)]

    def evaluate_exposure(self, model, filter=None):
        """SLIMGPU_ModelEvaluateExposure: evaluate_at()'s list and, from the same scoring pass, the exposure of the
        lists behind it at the eval set's cutoffs, users and marker: (figures, (E, summaries)) with E
        [len(cutoffs), ncols] uint32 and one dict per cutoff (slimgpu_exposure_t's fields and "nrcmds")."""
        n = len(self.cutoffs)
        met = np.zeros(4 * max(n, 1), np.float64)
        nv = np.zeros(3 * max(n, 1), np.int32)
        E = np.zeros((max(n, 1), self._matrix.ncols), np.uint32)
        summ = (_lib.Exposure * max(n, 1))()
        st = self._lib.SLIMGPU_ModelEvaluateExposure(self.handle, model.handle,
                                                     None if filter is None else filter.handle, n, met, nv,
                                                     _ptr(E), C.cast(summ, C.c_void_p))
        if st != SLIM_OK:
            raise RuntimeError("SLIMGPU_ModelEvaluateExposure failed (%d): %s" % (st, _lib.last_error()))
        figures = [{"nrcmds": c, "hr": met[4 * k], "hr_head": met[4 * k + 1], "hr_tail": met[4 * k + 2],
                    "arhr": met[4 * k + 3], "nvalid": int(nv[3 * k]), "nvalid_head": int(nv[3 * k + 1]),
                    "nvalid_tail": int(nv[3 * k + 2])} for k, c in enumerate(self.cutoffs)]
        return figures, (E[:n], _exposure_dicts(summ, self.cutoffs))

    def ranks(self, model, scores=False, filter=None):
        """SLIMGPU_ModelRanks(Filtered): the rank of every test entry of the evaluated users among the user's candidates
        (1 = the head of every list; 0 = in no list of any length).  Returns (ranks, indptr[, scores]): the
        entries of position q are ranks[indptr[q]:indptr[q + 1]], in the order of the user's test row."""
        n = int(self._lib.SLIMGPU_EvalSetEntries(self.handle))
        rk = np.zeros(max(n, 1), np.int32)
        sc = np.zeros(max(n, 1), np.float32) if scores else None
        out = (rk.ctypes.data_as(C.c_void_p), None if sc is None else sc.ctypes.data_as(C.c_void_p))
        if filter is None:
            st = self._lib.SLIMGPU_ModelRanks(self.handle, model.handle, *out)
        else:
            st = self._lib.SLIMGPU_ModelRanksFiltered(self.handle, model.handle, filter.handle, *out)
        if st != SLIM_OK:
            raise RuntimeError("SLIMGPU_ModelRanks%s failed (%d): %s"
                               % ("" if filter is None else "Filtered", st, _lib.last_error()))
        return (rk[:n], self.indptr, sc[:n]) if scores else (rk[:n], self.indptr)

    def evaluate_ranked(self, model, cutoffs, filter=None):
        """SLIMGPU_ModelEvaluateRanked(Filtered): one dict per cutoff (evaluate_at()'s keys), at ANY list lengths
        (ascending, at most 32), from the ranks of the held-out items -- no list is formed."""
        cut = np.ascontiguousarray(cutoffs, dtype=np.int32).ravel()
        n = cut.size
        met = np.zeros(4 * max(n, 1), np.float64)
        nv = np.zeros(3 * max(n, 1), np.int32)
        if filter is None:
            st = self._lib.SLIMGPU_ModelEvaluateRanked(self.handle, model.handle, n, cut.ctypes.data_as(C.c_void_p),
                                                       met, nv)
        else:
            st = self._lib.SLIMGPU_ModelEvaluateRankedFiltered(self.handle, model.handle, filter.handle, n,
                                                               cut.ctypes.data_as(C.c_void_p), met, nv)
        if st != SLIM_OK:
            raise RuntimeError("SLIMGPU_ModelEvaluateRanked%s failed (%d): %s"
                               % ("" if filter is None else "Filtered", st, _lib.last_error()))
        return [{"nrcmds": int(c), "hr": met[4 * k], "hr_head": met[4 * k + 1], "hr_tail": met[4 * k + 2],
                 "arhr": met[4 * k + 3], "nvalid": int(nv[3 * k]), "nvalid_head": int(nv[3 * k + 1]),
                 "nvalid_tail": int(nv[3 * k + 2])} for k, c in enumerate(cut)]

    def evaluate_candidates(self, model, cset):
        """SLIMGPU_ModelEvaluateCandidates: one dict per list length (evaluate_at()'s keys) for the lists the
        model makes of the users' candidate rows (a CandidateSet) -- HR on sampled negatives, in HBM."""
        n = len(self.cutoffs)
        met = np.zeros(4 * max(n, 1), np.float64)
        nv = np.zeros(3 * max(n, 1), np.int32)
        st = self._lib.SLIMGPU_ModelEvaluateCandidates(self.handle, model.handle, cset.handle, n, met, nv)
        if st != SLIM_OK:
            raise RuntimeError("SLIMGPU_ModelEvaluateCandidates failed (%d): %s" % (st, _lib.last_error()))
        return [{"nrcmds": c, "hr": met[4 * k], "hr_head": met[4 * k + 1], "hr_tail": met[4 * k + 2],
                 "arhr": met[4 * k + 3], "nvalid": int(nv[3 * k]), "nvalid_head": int(nv[3 * k + 1]),
                 "nvalid_tail": int(nv[3 * k + 2])} for k, c in enumerate(self.cutoffs)]

    def set_groups(self, groups, ngroups=None):
        """SLIMGPU_EvalSetSetGroups: groups[u] in [0, ngroups) or -1 for every user row of the test matrix (by USER ID,
        whatever the evaluated users are; ngroups None: the largest group + 1).  While set, every evaluate* call also
        forms the figures of every group from its one scoring pass: group_figures()."""
        groups = _group_array(groups, "set_groups")
        if ngroups is None:
            ngroups = int(groups.max()) + 1 if groups.size else 0
        st = self._lib.SLIMGPU_EvalSetSetGroups(self.handle, int(ngroups), _ptr(groups))
        if st != SLIM_OK:
            raise ValueError("SLIMGPU_EvalSetSetGroups failed (%d): %s" % (st, _lib.last_error()))

    def set_history_bands(self, bounds):
        """SLIMGPU_EvalSetSetHistoryBands: the group of a user is the number of bounds (ascending, >= 1) its history
        length reaches: len(bounds) + 1 groups, group 0 with the shortest histories."""
        bounds = _group_array(np.atleast_1d(bounds), "set_history_bands")
        st = self._lib.SLIMGPU_EvalSetSetHistoryBands(self.handle, bounds.size, _ptr(bounds))
        if st != SLIM_OK:
            raise ValueError("SLIMGPU_EvalSetSetHistoryBands failed (%d): %s" % (st, _lib.last_error()))

    def clear_groups(self):
        self._lib.SLIMGPU_EvalSetClearGroups(self.handle)

    def group_members(self):
        """The evaluated positions of every group, then all of them (SLIMGPU_EvalSetGroupInfo)."""
        n = C.c_int32(0)
        if self._lib.SLIMGPU_EvalSetGroupInfo(self.handle, C.byref(n), None) != SLIM_OK:
            raise RuntimeError("SLIMGPU_EvalSetGroupInfo failed: %s" % _lib.last_error())
        members = np.zeros(n.value + 1, np.int32)
        self._lib.SLIMGPU_EvalSetGroupInfo(self.handle, C.byref(n), _ptr(members))
        return members

    def group_figures(self, cutoffs=None):
        """SLIMGPU_EvalSetLastGroupFigures: the rows of the most recent evaluate* call per group -- one list per group,
        everybody last, of the dicts evaluate_at() returns plus "members".  cutoffs: those of the call when it was
        evaluate_ranked (default: the eval set's; evaluate() has them all)."""
        cut = self.cutoffs if cutoffs is None else tuple(int(c) for c in np.atleast_1d(cutoffs))
        members = self.group_members()
        n, rows = len(cut), members.size
        met = np.zeros(4 * max(n, 1) * rows, np.float64)
        nv = np.zeros(3 * max(n, 1) * rows, np.int32)
        st = self._lib.SLIMGPU_EvalSetLastGroupFigures(self.handle, n, _ptr(met), _ptr(nv))
        if st != SLIM_OK:
            raise RuntimeError("SLIMGPU_EvalSetLastGroupFigures failed (%d): %s" % (st, _lib.last_error()))
        met, nv = met.reshape(rows, -1, 4), nv.reshape(rows, -1, 3)
        return [[{"nrcmds": c, "hr": met[g, k, 0], "hr_head": met[g, k, 1], "hr_tail": met[g, k, 2],
                  "arhr": met[g, k, 3], "nvalid": int(nv[g, k, 0]), "nvalid_head": int(nv[g, k, 1]),
                  "nvalid_tail": int(nv[g, k, 2]), "members": int(members[g])} for k, c in enumerate(cut)]
                for g in range(rows)]

    def sample_candidates(self, nnegs, seed=1, weights=None):
        """SLIMGPU_EvalSetSampleCandidates: the 1-vs-k CandidateSet of this eval set's users, made on the device --
        `nnegs` sampled items outside the user's history and test row, then the test row (a score tie goes to the
        negative).  Reproducible from the seed; evaluate_candidates(model, that set) gives HR / ARHR on sampled
        negatives.  It costs about what evaluate() costs: a protocol, not a speed-up.  weights
        (SLIMGPU_EvalSetSampleCandidatesWeighted): None: uniform; "popularity": in proportion to the entries the
        resident matrix has of every item; an array of ncols non-negative integers below 2^32."""
        h = C.c_void_p()
        weighted, w = _sampling_weights(weights, self._matrix.ncols if weights is not None else 0)
        if weighted:
            name = "SLIMGPU_EvalSetSampleCandidatesWeighted"
            st = self._lib.SLIMGPU_EvalSetSampleCandidatesWeighted(
                self.handle, int(nnegs), int(seed), None if w is None else w.ctypes.data_as(C.c_void_p), C.byref(h))
        else:
            name = "SLIMGPU_EvalSetSampleCandidates"
            st = self._lib.SLIMGPU_EvalSetSampleCandidates(self.handle, int(nnegs), int(seed), C.byref(h))
        if st != SLIM_OK:
            raise RuntimeError("%s failed (%d): %s" % (name, st, _lib.last_error()))
        return CandidateSet.from_handle(h, lib=self._lib)

    def prepass_ms(self):
        """Milliseconds of the pre-pass (the test entries' scores and keys) of the most recent ranked call."""
        return float(self._lib.SLIMGPU_LastRankPrepassMs())

    def stats(self):
        return eval_stats(self._lib)

    def close(self):
        if self.handle is not None and self.handle.value:
            self._lib.SLIMGPU_EvalSetFree(C.byref(self.handle))
        self.handle = None
        self._matrix = None

    def __del__(self):
        try:
            self.close()
        except Exception:   # noqa: BLE001 -- interpreter shutdown
            pass


class DeviceMatrix(object):
    """Training matrix resident in HBM (CSR + column view + norms)."""

    def __init__(self, handle, keepalive=None):
        self._lib = _lib.load()
        self.handle = C.c_void_p(handle)
        self._keep = keepalive
        self._host_rows = None
        nr, nc, nz = C.c_int32(), C.c_int32(), C.c_int64()
        self._lib.SLIMGPU_MatrixInfo(self.handle, C.byref(nr), C.byref(nc), C.byref(nz))
        self.nrows, self.ncols, self.nnz = nr.value, nc.value, nz.value
        self.device = int(self._lib.SLIMGPU_MatrixDevice(self.handle))   # the HIP device of its buffers

    @classmethod
    def from_scipy(cls, R, binary=False, device=None):
        lib = _lib.load()
        R = sp.csr_matrix(R)
        ptr = np.ascontiguousarray(R.indptr, dtype=np.intp)
        ind = np.ascontiguousarray(R.indices, dtype=np.int32)
        val = None if binary else np.ascontiguousarray(R.data, dtype=np.float32)
        iopt, _ = make_options(device=device)
        st = C.c_int32(0)
        h = lib.SLIMGPU_MatrixFromHost(R.shape[0], ptr, ind,
                                       None if val is None else val.ctypes.data_as(C.c_void_p),
                                       iopt.ctypes.data_as(C.c_void_p), C.byref(st))
        if not h:
            raise RuntimeError("SLIMGPU_MatrixFromHost failed (%d): %s" % (st.value, _lib.last_error()))
        m = cls(h)
        m._host_rows = (R.shape[0], ptr, ind)   # evaluator(): the head / tail split is over these rows
        return m

    @classmethod
    def from_device_ptrs(cls, nrows, ncols, rowptr_ptr, rowind_ptr, rowval_ptr, keepalive=None,
                         device=None):
        """Adopt int64 rowptr / int32 rowind / float32 rowval (or 0) already in HBM."""
        lib = _lib.load()
        iopt, _ = make_options(device=device)
        st = C.c_int32(0)
        h = lib.SLIMGPU_MatrixFromDevice(nrows, ncols, C.c_void_p(rowptr_ptr),
                                         C.c_void_p(rowind_ptr),
                                         C.c_void_p(rowval_ptr) if rowval_ptr else None,
                                         iopt.ctypes.data_as(C.c_void_p), C.byref(st))
        if not h:
            raise RuntimeError("SLIMGPU_MatrixFromDevice failed (%d): %s" % (st.value, _lib.last_error()))
        return cls(h, keepalive)

    def close(self):
        if self.handle is not None and self.handle.value:
            self._lib.SLIMGPU_MatrixFree(C.byref(self.handle))
        self.handle = None
        self._keep = None
        self._host_rows = None

    __del__ = close

    def split(self, mode="leave_out", nfolds=1, fold=0, nheld=1, minkeep=1, seed=1):
        """SLIMGPU_MatrixSplit: this matrix split where it lies (include/slim_gpu_split.h states the rule).  Returns
        (DeviceMatrix, test): the train half, staged on this matrix's device from arrays that never left it, and the
        held-out entries as a scipy CSR matrix of this matrix's shape -- the only part that crosses to the host.
        The rows equal split_host's for the same parameters, bit for bit; eval_stats() reports the call."""
        spec = make_split(mode, nfolds, fold, nheld, minkeep, seed)
        trn, tst = C.c_void_p(), C.c_void_p()
        st = self._lib.SLIMGPU_MatrixSplit(self.handle, C.byref(spec), C.byref(trn), C.byref(tst))
        if st != SLIM_OK:
            raise ValueError("SLIMGPU_MatrixSplit failed (%d): %s" % (st, _lib.last_error()))
        return DeviceMatrix(trn.value), _rows_to_scipy(self._lib, tst, self.ncols)

    def column_view(self):
        colptr = np.zeros(self.ncols + 1, np.int64)
        colind = np.zeros(max(self.nnz, 1), np.int32)
        colval = np.zeros(max(self.nnz, 1), np.float32)
        cnorm = np.zeros(self.ncols, np.float32)
        rc = self._lib.SLIMGPU_MatrixGetColumnView(
            self.handle, *[a.ctypes.data_as(C.c_void_p) for a in (colptr, colind, colval, cnorm)])
        if rc != SLIM_OK:
            raise RuntimeError("SLIMGPU_MatrixGetColumnView failed: %s" % _lib.last_error())
        return colptr, colind[:self.nnz], colval[:self.nnz], cnorm

    def column_cost(self):
        cost = np.zeros(self.ncols, np.int64)
        rc = self._lib.SLIMGPU_MatrixColumnCost(self.handle, cost.ctypes.data_as(C.c_void_p))
        if rc != SLIM_OK:
            raise RuntimeError("SLIMGPU_MatrixColumnCost failed")
        return cost

    def learn(self, imodel=None, return_handle=False, columns=None, **opts):
        """SLIMGPU_Learn (or SLIMGPU_LearnColumns when an explicit list of item columns is
        given).  Returns (W as scipy CSC, stats dict)."""
        iopt, dopt = make_options(**opts)
        st = C.c_int32(0)
        ih = None
        tmp = None
        if imodel is not None:
            if isinstance(imodel, (int, C.c_void_p)):
                ih = imodel
            else:  # scipy matrix -> temporary handle with a column view
                tmp = _scipy_to_model_handle(self._lib, imodel)
                ih = tmp
        if columns is not None:
            cols = np.ascontiguousarray(columns, dtype=np.int32)
            h = self._lib.SLIMGPU_LearnColumns(self.handle, cols.size, cols,
                                               iopt.ctypes.data_as(C.c_void_p),
                                               dopt.ctypes.data_as(C.c_void_p), ih, C.byref(st))
        else:
            h = self._lib.SLIMGPU_Learn(self.handle, iopt.ctypes.data_as(C.c_void_p),
                                        dopt.ctypes.data_as(C.c_void_p), ih, C.byref(st))
        if tmp is not None:
            self._lib.SLIM_FreeModel(C.byref(tmp))
        if not h:
            raise RuntimeError("SLIMGPU_Learn failed (%d): %s" % (st.value, _lib.last_error()))
        stats = _lib.Stats()
        self._lib.SLIMGPU_LastStats(C.byref(stats))
        if return_handle:
            return h, stats.as_dict()
        return model_to_scipy(self._lib, h), stats.as_dict()

    def learn_resident(self, warm=None, **opts):
        """SLIMGPU_LearnResident: like learn(), but the model stays in HBM (ResidentModel); `warm`
        is a ResidentModel of an earlier solve (no upload).  Returns (ResidentModel, stats dict)."""
        iopt, dopt = make_options(**opts)
        st = C.c_int32(0)
        h = self._lib.SLIMGPU_LearnResident(self.handle, iopt.ctypes.data_as(C.c_void_p),
                                            dopt.ctypes.data_as(C.c_void_p),
                                            warm.handle if warm is not None else None, C.byref(st))
        if not h:
            raise RuntimeError("SLIMGPU_LearnResident failed (%d): %s" % (st.value, _lib.last_error()))
        stats = _lib.Stats()
        self._lib.SLIMGPU_LastStats(C.byref(stats))
        return ResidentModel(self._lib, h), stats.as_dict()

    def model_from_scipy(self, W):
        """SLIMGPU_ModelFromHost: a model given as a scipy matrix (row i = the scores item i gives; the transpose
        of what learn() returns as columns is the same matrix) made resident on this matrix's device, for the
        resident scorers and as a warm start.  The ids of every row must ascend strictly."""
        W = sp.csr_matrix(W)
        ptr = np.ascontiguousarray(W.indptr, dtype=np.intp)
        ind = np.ascontiguousarray(W.indices, dtype=np.int32)
        val = np.ascontiguousarray(W.data, dtype=np.float32)
        hw = C.c_void_p()
        st = self._lib.Py_csr_wrapper(W.shape[0], ptr, ind, val.ctypes.data_as(C.c_void_p), C.byref(hw))
        if st != SLIM_OK:
            raise RuntimeError("Py_csr_wrapper failed (%d)" % st)
        C.cast(hw, C.POINTER(_lib.CsrView)).contents.ncols = W.shape[1]
        st = C.c_int32(0)
        try:
            h = self._lib.SLIMGPU_ModelFromHost(self.handle, hw, C.byref(st))
        finally:
            self._lib.Py_csr_free(hw)
        if not h:
            raise RuntimeError("SLIMGPU_ModelFromHost failed (%d): %s" % (st.value, _lib.last_error()))
        return ResidentModel(self._lib, h)

    def evaluator(self, T, nrcmds=10, fmarker=None, R=None, cutoffs=None, users=None, ranked=False):
        """SLIMGPU_EvalSetCreateAt: stage the test matrix T (scipy, one row per user) for evaluations
        of resident models against this matrix.  cutoffs: the list lengths (ascending, at most 8 of
        1..128; None: [nrcmds]), all served by one scoring pass.  users: ascending user ids to evaluate
        (None: every user).  fmarker=None: SLIM_DetermineHeadAndTail over the
        training rows with ncols = the larger of the two matrices' widths, as Py_SLIM_Mselect does
        (the rows from_scipy staged; R, a scipy matrix, for a matrix adopted from device pointers).
        ranked=True: SLIMGPU_EvalSetCreateRanked, an eval set with no list length, for ranks() and
        evaluate_ranked() (which every eval set serves)."""
        T = sp.csr_matrix(T)
        if fmarker is None:
            if R is not None:
                R = sp.csr_matrix(R)
                rows = (R.shape[0], np.ascontiguousarray(R.indptr, dtype=np.intp),
                        np.ascontiguousarray(R.indices, dtype=np.int32))
            else:
                rows = self._host_rows
            if rows is None:
                raise ValueError("evaluator: give fmarker, or the training rows R to derive it from")
            tmax = int(T.indices.max()) + 1 if T.nnz else 0
            ncols = max(self.ncols, tmax, 1)
            p = self._lib.SLIM_DetermineHeadAndTail(rows[0], ncols, rows[1], rows[2])
            fmarker = np.ctypeslib.as_array(p, shape=(ncols,)).copy()
            C.CDLL(None).free(p)
        fmarker = np.ascontiguousarray(fmarker, dtype=np.int32)
        cut = np.ascontiguousarray([nrcmds] if cutoffs is None else cutoffs, dtype=np.int32).ravel()
        sel = None if users is None else np.ascontiguousarray(users, dtype=np.int32).ravel()
        ht = _wrap_rows(self._lib, T)
        st = C.c_int32(0)
        nsel, psel = (0, None) if sel is None else (sel.size, sel.ctypes.data_as(C.c_void_p))
        try:
            if ranked:
                h = self._lib.SLIMGPU_EvalSetCreateRanked(self.handle, ht, fmarker, fmarker.size, nsel, psel,
                                                          C.byref(st))
            else:
                h = self._lib.SLIMGPU_EvalSetCreateAt(self.handle, ht, fmarker, fmarker.size, cut.size,
                                                      cut.ctypes.data_as(C.c_void_p), nsel, psel, C.byref(st))
        finally:
            self._lib.Py_csr_free(ht)
        if not h:
            raise RuntimeError("SLIMGPU_EvalSetCreate%s failed (%d): %s" % ("Ranked" if ranked else "At", st.value,
                                                                            _lib.last_error()))
        # where every position's test entries start (ranks()): the evaluated users are the listed ones, or the
        # first min(matrix rows, test rows)
        nall = min(self.nrows, T.shape[0])
        lens = np.diff(T.indptr)[:nall] if sel is None else np.diff(T.indptr)[sel]
        indptr = np.concatenate(([0], np.cumsum(lens, dtype=np.int64)))
        return Evaluator(self._lib, h, self, () if ranked else cut.tolist(), indptr)

    def item_filter(self, allowed=None, blocked=None, exclusions=None):
        """SLIMGPU_FilterCreate over this matrix's items: an ItemFilter for ResidentModel.predict(filter=...) and
        for the Evaluator's calls.
        Pass at most one of allowed / blocked (item ids); exclusions: a scipy CSR over user rows."""
        return ItemFilter(self.ncols, allowed, blocked, exclusions, lib=self._lib)

    def candidate_set(self, C_rows):
        """SLIMGPU_CandSetCreate over this matrix's items: a CandidateSet (row u = the candidates of user u; a scipy
        CSR taken as it is, or (indptr, indices)) for ResidentModel.score_candidates and
        Evaluator.evaluate_candidates."""
        return CandidateSet(self.ncols, C_rows, lib=self._lib)

    def sample_candidates(self, trn, tst, nnegs, seed=1, users=None, weights=None):
        """SLIMGPU_CandSetSample over this matrix's items: the host form of Evaluator.sample_candidates (trn: the
        scipy rows this matrix was staged from; the same rows for the same seed and weights)."""
        return sample_candidates(trn, tst, nnegs, seed=seed, users=users, ncols=self.ncols, lib=self._lib,
                                 weights=weights)

    def list_exposure(self, ids, counts, cutoffs, fmarker=None):
        """SLIMGPU_MatrixListExposure: list_exposure() of a caller's lists counted on this matrix's device; ncols and
        pop (the column counts) are the matrix's.  The outputs equal the host call's bit for bit."""
        ids, counts = _exposure_lists(ids, counts)
        cut = _cutoff_array(cutoffs)
        fm = None if fmarker is None else np.ascontiguousarray(fmarker, np.int32)
        E = np.zeros((max(cut.size, 1), self.ncols), np.uint32)
        summ = (_lib.Exposure * max(cut.size, 1))()
        st = self._lib.SLIMGPU_MatrixListExposure(self.handle, _ptr(fm), 0 if fm is None else fm.size, ids.shape[0],
                                                  ids.shape[1], _ptr(ids), _ptr(counts), cut.size, _ptr(cut), _ptr(E),
                                                  C.cast(summ, C.c_void_p))
        if st != SLIM_OK:
            raise RuntimeError("SLIMGPU_MatrixListExposure failed (%d): %s" % (st, _lib.last_error()))
        return E[:cut.size], _exposure_dicts(summ, cut)

    def column_stats(self):
        return ColumnStats(self._lib, self.ncols)

    def expect_solves(self, n):
        """Announce n solves of this matrix (a grid): KERNEL_AUTO may then build G = R^T R once
        and solve in item space (SLIMGPU_MatrixExpectSolves)."""
        self._lib.SLIMGPU_MatrixExpectSolves(self.handle, int(n))

    # -- G = R^T R of item-space CD in row blocks (slim_gpu.h; slim_amd.distributed.build_gram_sharded)
    def gram_build_rows(self, row_begin, row_end):
        """Form rows [row_begin, row_end) of G on this handle (every entry of each)."""
        st = self._lib.SLIMGPU_MatrixGramBuildRows(self.handle, int(row_begin), int(row_end))
        if st != SLIM_OK:
            raise RuntimeError("SLIMGPU_MatrixGramBuildRows failed (%d): %s" % (st, _lib.last_error()))

    def gram_view(self):
        """(device pointer, floats per row, rows) of the handle's G."""
        p, ld, n = C.c_void_p(), C.c_int64(), C.c_int32()
        st = self._lib.SLIMGPU_MatrixGramView(self.handle, C.byref(p), C.byref(ld), C.byref(n))
        if st != SLIM_OK:
            raise RuntimeError("SLIMGPU_MatrixGramView failed (%d): %s" % (st, _lib.last_error()))
        return p.value, ld.value, n.value

    def gram_rows_tensor(self, row_begin, row_end):
        """Rows [row_begin, row_end) of G as a torch tensor that ALIASES the engine's buffer
        (a contiguous (rows, ld) float32 block on this handle's device)."""
        import torch
        ptr, ld, n = self.gram_view()
        if not 0 <= row_begin <= row_end <= n:
            raise ValueError("gram_rows_tensor: rows [%d, %d) outside [0, %d)" % (row_begin, row_end, n))

        class _Alias:
            pass
        a = _Alias()
        a.__cuda_array_interface__ = {
            "shape": (int(row_end - row_begin), int(ld)), "typestr": "<f4",
            "data": (int(ptr) + 4 * int(ld) * int(row_begin), False), "version": 2, "strides": None}
        # (on the handle's device, not the current one: a copy instead of an alias would swallow
        # the broadcast of build_gram_sharded and commit a G with missing rows)
        t = torch.as_tensor(a, device=torch.device("cuda", self.device))
        if t.numel() and t.data_ptr() != a.__cuda_array_interface__["data"][0]:
            raise RuntimeError("gram_rows_tensor: torch copied the block instead of aliasing it")
        return t

    def gram_commit(self):
        """Every row of G is in place: item-space solves may use it (byte planes are formed)."""
        st = self._lib.SLIMGPU_MatrixGramCommit(self.handle)
        if st != SLIM_OK:
            raise RuntimeError("SLIMGPU_MatrixGramCommit failed (%d): %s" % (st, _lib.last_error()))

    def gram_planes(self):
        """Host copies of the byte planes the handle holds (SLIMGPU_MatrixGramPlanes; the layout is
        in include/slim_gpu_planes.h) as a dict of numpy arrays: lo (ncols, ldb), base (ncols, 8192),
        hi (the pool, slack included), hi_off, hi_k, hi2_k, diag, meta (ncols, 4), rank_of, item_of,
        and the ints ncols, nchunks, ldb.  RuntimeError when the handle holds none."""
        import torch
        p = _lib.GramPlanes()
        st = self._lib.SLIMGPU_MatrixGramPlanes(self.handle, C.byref(p))
        if st != SLIM_OK:
            raise RuntimeError("SLIMGPU_MatrixGramPlanes failed (%d): %s" % (st, _lib.last_error()))
        n, ldb = int(p.ncols), int(p.ldb)
        dev = torch.device("cuda", self.device)
        torch.cuda.synchronize(dev)

        def fetch(ptr, shape, dtype):
            out = np.empty(shape, dtype)
            if out.size:
                class _Alias:
                    pass
                a = _Alias()
                a.__cuda_array_interface__ = {"shape": (out.nbytes,), "typestr": "|u1", "data": (int(ptr), False),
                                              "version": 2, "strides": None}
                out.view(np.uint8).reshape(-1)[:] = torch.as_tensor(a, device=dev).cpu().numpy()
            return out
        return {"ncols": n, "nchunks": int(p.nchunks), "ldb": ldb,
                "lo": fetch(p.lo, (n, ldb), np.uint8), "base": fetch(p.base, (n, 8192), np.uint8),
                "hi": fetch(p.hi, (int(p.hi_bytes),), np.uint8), "hi_off": fetch(p.hi_off, (n,), np.int64),
                "hi_k": fetch(p.hi_k, (n,), np.int32), "hi2_k": fetch(p.hi2_k, (n,), np.int32),
                "diag": fetch(p.diag, (n,), np.float32), "meta": fetch(p.meta, (n, 4), np.uint32),
                "rank_of": fetch(p.rank_of, (n,), np.int32),
                "item_of": fetch(p.item_of, (16 * int(p.nchunks),), np.int32)}


def _scipy_to_model_handle(lib, W):
    """Model handle (row + column views) from a scipy matrix, via the text-free
    route: Py_csr_wrapper on W's rows, then a binary round trip adds columns."""
    import os
    import tempfile
    Wr = sp.csr_matrix(W)
    Wr.sort_indices()
    h = C.c_void_p()
    ptr = np.ascontiguousarray(Wr.indptr, dtype=np.intp)
    ind = np.ascontiguousarray(Wr.indices, dtype=np.int32)
    val = np.ascontiguousarray(Wr.data, dtype=np.float32)
    if ind.size == 0 or ind.max() + 1 < Wr.shape[1]:
        pass  # ncols of the handle = max id + 1; fixed up by the binary round trip below
    lib.Py_csr_wrapper(Wr.shape[0], ptr, ind, val.ctypes.data_as(C.c_void_p), C.byref(h))
    view = C.cast(h, C.POINTER(_lib.CsrView)).contents
    view.ncols = Wr.shape[1]
    fd, path = tempfile.mkstemp(suffix=".slimbin")
    os.close(fd)
    try:
        lib.SLIM_WriteModel(h, path.encode())
        out = C.c_void_p(lib.SLIM_ReadModel(path.encode()))
    finally:
        os.unlink(path)
        lib.Py_csr_free(h)
    return out
