"""Host-side mirror of the reference's Python package (``from SLIM import SLIM,
SLIMatrix``) on top of the MI355X engine's libslim.so.

Same class names, method names, argument meaning, defaults, printed messages
and error behaviour as /root/reference/python-package/SLIM/core.py; the code is
new.  Everything numerical happens behind the C ABI (include/slim.h,
include/slim_gpu.h): training on the GPU, top-N scoring in the library.

Reference anchors: parameter defaults and validation core.py:46-242, SLIMatrix
core.py:245-385 (id mapping in first-appearance order :289-351, marshalling
dtypes :353-362), SLIM core.py:388-683.
"""
import ctypes as C
import numbers
import os
import time

import numpy as np
import scipy.sparse as sp

from . import _lib
from .constants import (SLIM_ALGO, SLIM_NOPTIONS, SLIM_OK, SLIM_SIMTYPE, Opt)

try:  # pandas is optional, exactly as in the reference
    from pandas import DataFrame
    PANDAS_INSTALLED = True
except Exception:  # pragma: no cover
    DataFrame = None
    PANDAS_INSTALLED = False


# ---------------------------------------------------------------------------
# parameters
# ---------------------------------------------------------------------------
def _is_int(v):
    return type(v) is int


def _is_real(v):
    return isinstance(v, (int, float)) and not isinstance(v, bool)


# name -> (default, predicate, complaint)
_PARAMS = (
    ("dbglvl", 0, lambda v: _is_int(v) and v >= 0,
     "Please select dbglvl from {0, 1, 2, 4, 16, 2048}."),
    ("nnbrs", 0, lambda v: _is_int(v) and v >= 0,
     "Please provide non-negative integer value for nnbrs."),
    ("simtype", "cos", lambda v: v in SLIM_SIMTYPE,
     "Please select simtytpe from {'cos', 'jacc', 'dotp'}."),
    ("algo", "cd", lambda v: v in SLIM_ALGO, "Please select algo from {'admm', 'cd'}."),
    ("nthreads", 1, lambda v: _is_int(v) and v > 0,
     "Please provide positive integer value for nthreads."),
    ("niters", 50, lambda v: _is_int(v) and v > 0,
     "Please provide positive integer value for niters."),
    ("nrcmds", 10, lambda v: _is_int(v) and v > 0,
     "Please provide positive integer value for nrcmds."),
    ("l1r", 1.0, lambda v: _is_real(v) and v >= 0, "Please provide non-negative value for l1r."),
    ("l2r", 1.0, lambda v: _is_real(v) and v >= 0, "Please provide non-negative value for l2r."),
    ("optTol", 1e-7, lambda v: _is_real(v) and v >= 0,
     "Please provide non-negative value for optTol."),
)


class _ParamView(object):
    """Uniform get/set/has over a dict or an attribute bag (argparse namespace...)."""

    def __init__(self, params):
        self.p = params
        self.is_dict = isinstance(params, dict)

    def has(self, k):
        return (k in self.p) if self.is_dict else hasattr(self.p, k)

    def get(self, k):
        return self.p[k] if self.is_dict else getattr(self.p, k)

    def set(self, k, v):
        if self.is_dict:
            self.p[k] = v
        else:
            setattr(self.p, k, v)


def check_params(params):
    """Validate ``params`` and fill in the defaults *in place* (the reference
    does the same, core.py:46-198).  Raises TypeError on a bad value."""
    view = _ParamView(params)
    for name, default, good, complaint in _PARAMS:
        if view.has(name):
            if not good(view.get(name)):
                raise TypeError(complaint)
        else:
            view.set(name, default)
    if view.get("nnbrs") > 0 and view.get("algo") != "cd":
        print("A fSLIM model cannot be trained with ADMM. Changing the algorithm to "
              "coordinate descent.")
        view.set("algo", "cd")
    view.set("ordered", 0)  # accepted by the C API, never implemented upstream
    return view


def build_options(params):
    """(ioptions, doptions) arrays for the C API (core.py:200-242)."""
    view = params if isinstance(params, _ParamView) else _ParamView(params)
    iopt = np.full(SLIM_NOPTIONS, -1, dtype=np.int32)
    dopt = np.full(SLIM_NOPTIONS, -1.0, dtype=np.float64)
    iopt[Opt.DBGLVL] = view.get("dbglvl")
    iopt[Opt.NNBRS] = view.get("nnbrs")
    iopt[Opt.SIMTYPE] = SLIM_SIMTYPE[view.get("simtype")]
    iopt[Opt.ALGO] = SLIM_ALGO[view.get("algo")]
    iopt[Opt.NTHREADS] = view.get("nthreads")
    iopt[Opt.ORDERED] = view.get("ordered")
    iopt[Opt.MAXNITERS] = view.get("niters")
    iopt[Opt.NRCMDS] = view.get("nrcmds")
    dopt[Opt.L1R] = view.get("l1r")
    dopt[Opt.L2R] = view.get("l2r")
    dopt[Opt.OPTTOL] = view.get("optTol")
    # engine extensions ride along when present (include/slim_gpu.h)
    for key, slot in (("gpu_seed", Opt.GPU_SEED), ("gpu_evalstride", Opt.GPU_EVALSTRIDE),
                      ("gpu_evalnegs", Opt.GPU_EVALNEGS), ("gpu_evalseed", Opt.GPU_EVALSEED),
                      ("gpu_evalnegpop", Opt.GPU_EVALNEGPOP), ("gpu_evalexposure", Opt.GPU_EVALEXPOSURE),
                      ("gpu_device", Opt.GPU_DEVICE),
                      ("gpu_kernel", Opt.GPU_KERNEL), ("gpu_colbegin", Opt.GPU_COLBEGIN),
                      ("gpu_colend", Opt.GPU_COLEND)):
        if view.has(key):
            iopt[slot] = int(view.get(key))
    return iopt, dopt


def _prepare(params):
    if not isinstance(params, dict) and not hasattr(params, "__dict__"):
        raise TypeError("Parameter type %s is not supported!" % type(params).__name__)
    return check_params(params)


# ---------------------------------------------------------------------------
# SLIMatrix
# ---------------------------------------------------------------------------
def _enumerate_first_seen(keys, table=None, names=None):
    """Dense ids in order of first appearance (dict insertion order)."""
    table = {} if table is None else table
    names = [] if names is None else names
    for k in keys:
        if k not in table:
            table[k] = len(names)
            names.append(k)
    return table, names


class SLIMatrix(object):
    """Training / history matrix handed to :class:`SLIM`.

    ``data``: scipy CSR (ids = positions) or user-item-rating triplets as a
    list of lists, a 2-d numpy array or a pandas DataFrame (raw ids are mapped
    to dense ids in first-appearance order).  ``oldmat``: a SLIMatrix or SLIM
    whose id maps should be reused (events outside them are dropped)."""

    def __init__(self, data, oldmat=None):
        self._lib = _lib.load()
        self.handle = None
        if sp.isspmatrix_csr(data):
            self.nUsers, self.nItems = data.shape
            if isinstance(oldmat, SLIMatrix) and (self.nUsers != oldmat.nUsers or
                                                  self.nItems != oldmat.nItems):
                raise TypeError("The size of the input matrix does not match the size of oldmat.")
            if isinstance(oldmat, SLIM) and self.nItems != oldmat.id2item.size:
                raise TypeError("The size of the input matrix does not match the size of oldmat.")
            self.id2item = np.arange(self.nItems)
            self.item2id = self.id2item
            self.id2user = np.arange(self.nUsers)
            self.user2id = self.id2user
            self._set_csr(data)
        elif isinstance(data, (list, np.ndarray)):
            self.data_from_np2d(data, oldmat)
        elif PANDAS_INSTALLED and isinstance(data, DataFrame):
            self.data_from_np2d(data.values, oldmat)
        else:
            raise TypeError(
                "Input data type %s is not supported. Please provide ijv triplets in "
                "numpy.ndarray/list[List]/pandas.DataFrame or a row based sparse matrix in "
                "scipy csr_matrix." % type(data).__name__)

    def __del__(self):
        try:
            if self.handle is not None:
                self._lib.Py_csr_free(self.handle)
                self.handle = None
        except Exception:
            pass

    def data_from_np2d(self, data, oldmat=None):
        if oldmat is not None:
            assert isinstance(oldmat, (SLIMatrix, SLIM)), \
                "Please feed in a SLIMatrix object or a SLIM model for oldmat."
            self.id2item = oldmat.id2item.copy()
            self.item2id = oldmat.item2id.copy()
            if isinstance(oldmat, SLIMatrix):
                self.id2user = oldmat.id2user.copy()
                self.user2id = oldmat.user2id.copy()
            else:  # a model knows items only: users are enumerated afresh
                self.user2id, self.id2user = _enumerate_first_seen(t[0] for t in data)
        else:
            self.user2id, users = _enumerate_first_seen(t[0] for t in data)
            self.item2id, items = _enumerate_first_seen(t[1] for t in data)
            self.id2user = np.array(users)
            self.id2item = np.array(items)

        rows, cols, vals, missed = [], [], [], 0
        u2i, i2i = self.user2id, self.item2id
        for t in data:
            if t[0] in u2i and t[1] in i2i:
                rows.append(u2i[t[0]])
                cols.append(i2i[t[1]])
                vals.append(t[2])
            else:
                missed += 1
        if missed:
            print("%d of the events fall out of the range of oldmat. Partial entries collected."
                  % missed)
        self.nUsers = len(self.id2user)
        self.nItems = len(self.id2item)
        self._set_csr(sp.csr_matrix((vals, (rows, cols)), shape=(self.nUsers, self.nItems)))

    def split(self, mode="leave_out", nfolds=1, fold=0, nheld=1, minkeep=1, seed=1):
        """SLIMGPU_SplitHost (include/slim_gpu_split.h states the rule): this matrix split into (train, test), two
        SLIMatrix objects with this matrix's id maps and shape.  mode "leave_out": every user with at least
        nfolds * nheld + minkeep entries holds out nheld of them in each fold; "folds": every entry belongs to one of
        nfolds folds.  The same parameters always give the same rows.  (An engine extension.)"""
        from .engine import make_split
        spec = make_split(mode, nfolds, fold, nheld, minkeep, seed)
        halves = C.c_void_p(), C.c_void_p()
        rc = self._lib.SLIMGPU_SplitHost(self.handle, C.byref(spec), C.byref(halves[0]), C.byref(halves[1]))
        if rc != SLIM_OK:
            raise TypeError("The matrix could not be split. [%s]" % _lib.last_error())
        out = []
        for h in halves:
            m = SLIMatrix.__new__(SLIMatrix)
            m._lib, m.handle = self._lib, h
            m.nUsers, m.nItems = self.nUsers, self.nItems
            m.id2item, m.item2id = self.id2item.copy(), self.item2id.copy()
            m.id2user, m.user2id = self.id2user.copy(), self.user2id.copy()
            out.append(m)
        return tuple(out)

    def _set_csr(self, R):
        handle = C.c_void_p()
        indptr = np.ascontiguousarray(R.indptr, dtype=np.intp)
        indices = np.ascontiguousarray(R.indices, dtype=np.int32)
        values = np.ascontiguousarray(R.data, dtype=np.float32)
        rc = self._lib.Py_csr_wrapper(R.shape[0], indptr, indices,
                                      values.ctypes.data_as(C.c_void_p), C.byref(handle))
        if rc != SLIM_OK:
            raise RuntimeError("Py_csr_wrapper failed (%d): %s" % (rc, _lib.last_error()))
        self.handle = handle


# ---------------------------------------------------------------------------
# candidate filters (SLIM.predict, SLIM.mselect)
# ---------------------------------------------------------------------------
def _known_items(item2id, items, ncols):
    """Dense ids (below ncols) of the original item ids that item2id knows; the others are dropped."""
    known = []
    is_dict = isinstance(item2id, dict)
    for it in items:
        if is_dict:
            j = item2id.get(it, -1)
        else:
            j = int(it) if isinstance(it, numbers.Integral) and 0 <= it < len(item2id) else -1
        if 0 <= j < ncols:
            known.append(j)
    return np.asarray(known, dtype=np.int32)


def _candidate_filter(lib, item2id, nitems, ncols, data, allowed_items, blocked_items, exclude):
    """An ItemFilter over `ncols` items: original ids through item2id (a model's map in predict, the training
    matrix's in mselect), the rows of `exclude` put in the order of data's users."""
    from .engine import ItemFilter
    if allowed_items is not None and blocked_items is not None:
        raise TypeError("Please provide at most one of allowed_items and blocked_items.")
    allowed = None if allowed_items is None else _known_items(item2id, allowed_items, ncols)
    blocked = None if blocked_items is None else _known_items(item2id, blocked_items, ncols)
    rows = None
    if exclude is not None:
        assert type(exclude) == SLIMatrix, "exclude must be a SLIMatrix object."
        assert exclude.nItems == nitems, "The shape of exclude should match the model."
        nnz = C.c_int(0)
        lib.Py_csr_stat(exclude.handle, C.byref(nnz))
        ptr = np.zeros(exclude.nUsers + 1, dtype=np.int32)
        ind = np.zeros(max(nnz.value, 1), dtype=np.int32)
        val = np.ones(max(nnz.value, 1), dtype=np.float32)
        lib.Py_csr_export(exclude.handle, ptr, ind, val)
        if isinstance(data.user2id, dict):
            xdict = isinstance(exclude.user2id, dict)
            src = [exclude.user2id.get(k, -1) if xdict else (k if 0 <= k < exclude.nUsers else -1)
                   for k in data.user2id]   # (dense ids ascend in insertion order)
        else:
            src = [u if u < exclude.nUsers else -1 for u in range(data.nUsers)]
        xptr, xind = [0], []
        for r in src:
            if r >= 0:
                row = ind[ptr[r]:ptr[r + 1]]
                xind.extend(row[row < ncols].tolist())
            xptr.append(len(xind))
        rows = sp.csr_matrix((np.ones(len(xind), np.float32), np.asarray(xind, np.int32),
                              np.asarray(xptr, np.int64)), shape=(len(src), max(ncols, 1)))
    return ItemFilter(ncols, allowed, blocked, rows, lib=lib)


def _user_groups(lib, trndata, groups, history_bands):
    """(group per user row of trndata as int32, ngroups) of mselect's groups / history_bands; (None, 0) without."""
    if groups is not None and history_bands is not None:
        raise TypeError("Please provide at most one of groups and history_bands.")
    if groups is None and history_bands is None:
        return None, 0
    if history_bands is not None:
        bounds = np.asarray(history_bands)
        if (bounds.ndim != 1 or bounds.size < 1 or bounds.dtype.kind not in "iu" or bounds.min() < 1 or
                (np.diff(bounds) <= 0).any() or bounds.size >= _lib.MAX_GROUPS):
            raise TypeError("history_bands must be ascending integers, each at least 1.")
        nnz = C.c_int(0)
        lib.Py_csr_stat(trndata.handle, C.byref(nnz))
        ptr = np.zeros(trndata.nUsers + 1, dtype=np.int32)
        ind = np.zeros(max(nnz.value, 1), dtype=np.int32)
        val = np.ones(max(nnz.value, 1), dtype=np.float32)
        lib.Py_csr_export(trndata.handle, ptr, ind, val)
        return (np.ascontiguousarray(np.searchsorted(bounds, np.diff(ptr), side="right"), np.int32),
                int(bounds.size) + 1)
    if isinstance(groups, dict):
        out = np.full(trndata.nUsers, -1, np.int32)
        known = trndata.user2id
        for user, g in groups.items():
            if not isinstance(g, (int, np.integer)):
                raise TypeError("groups must map user ids to integer groups.")
            row = known.get(user, -1) if isinstance(known, dict) else (user if 0 <= user < trndata.nUsers else -1)
            if row >= 0:
                out[row] = g
    else:
        out = np.asarray(groups)
        if out.ndim != 1 or out.dtype.kind not in "iu" or out.size != trndata.nUsers:
            raise TypeError("groups must hold one integer group per user row of trndata (%d)." % trndata.nUsers)
        out = np.ascontiguousarray(out, np.int32)
    if out.size and (out.min() < -1 or out.max() >= _lib.MAX_GROUPS):
        raise TypeError("a group must be -1 (none) or 0 to %d." % (_lib.MAX_GROUPS - 1))
    if not out.size or out.max() < 0:
        raise TypeError("groups puts no user into a group.")
    return out, int(out.max()) + 1


# ---------------------------------------------------------------------------
# SLIM
# ---------------------------------------------------------------------------
class SLIM(object):
    """Item-item sparse linear model; ``train`` runs on the GPU engine."""

    def __init__(self):
        self._lib = _lib.load()
        self.ismodel = 0
        self.handle = None

    def __del__(self):
        try:
            if self.handle is not None:
                self._lib.Py_csr_free(self.handle)
                self.handle = None
        except Exception:
            pass

    # -- training ------------------------------------------------------------
    def train(self, params, data):
        assert type(data) == SLIMatrix, "trndata must be a SLIMatrix object."
        self.nItems = data.nItems
        iopt, dopt = build_options(_prepare(params))
        handle = C.c_void_p()
        t0 = time.time()
        rc = self._lib.Py_SLIM_Learn(data.handle, iopt, dopt, C.byref(handle))
        elapsed = time.time() - t0
        if self.handle is not None:
            self._lib.Py_csr_free(self.handle)
        self.ismodel = rc
        self.handle = handle if rc == SLIM_OK else None
        self.id2item = data.id2item.copy()
        self.item2id = data.item2id.copy()
        if rc != SLIM_OK:
            raise RuntimeError("Something went wrong with model estimation. [%s]"
                               % _lib.last_error())
        print("Learning takes %.3f secs." % elapsed)

    @staticmethod
    def split(data, mode="leave_out", nfolds=1, fold=0, nheld=1, minkeep=1, seed=1):
        """SLIMatrix.split of `data`: (train, test) as two SLIMatrix with data's id maps."""
        assert type(data) == SLIMatrix, "data must be a SLIMatrix object."
        return data.split(mode=mode, nfolds=nfolds, fold=fold, nheld=nheld, minkeep=minkeep, seed=seed)

    def _mselect_cv(self, params, data, arrayl1, arrayl2, nrcmds, allowed_items, blocked_items, exclude, nnegs,
                    negseed, negpop, cv, cv_mode, cv_held, cv_minkeep, cv_seed):
        """mselect(cv=F): Py_SLIM_MselectCV on one matrix (include/slim_gpu_split.h)."""
        from .engine import make_split
        assert type(data) == SLIMatrix, "trndata must be a SLIMatrix object."
        if not (isinstance(cv, (int, np.integer)) and not isinstance(cv, bool) and cv >= 1):
            raise TypeError("cv must be the number of folds, at least 1.")
        assert type(arrayl1) in [list, np.ndarray], "Please provide a list of l1 values."
        assert type(arrayl2) in [list, np.ndarray], "Please provide a list of l2 values."
        if len(arrayl1) < 1:
            raise TypeError("The l1 array must not be empty.")
        if len(arrayl2) < 1:
            raise TypeError("The l2 array must not be empty.")
        view = _prepare(params)
        view.set("nrcmds", nrcmds)
        iopt, dopt = build_options(view)
        if nnegs:
            iopt[Opt.GPU_EVALNEGS], iopt[Opt.GPU_EVALSEED] = int(nnegs), int(negseed)
        if negpop:
            iopt[Opt.GPU_EVALNEGPOP] = 1
        spec = make_split(cv_mode, cv, 0, cv_held, cv_minkeep, cv_seed)
        flt = None
        if not (allowed_items is None and blocked_items is None and exclude is None):
            # (the train half of a fold is as wide as its largest item id + 1: in a fold that holds the widest item's
            # only entries out it is narrower than the data, and the grid then refuses the filter)
            ncols = max(int(C.cast(data.handle, C.POINTER(_lib.CsrView)).contents.ncols), 1)
            flt = _candidate_filter(self._lib, data.item2id, data.nItems, ncols, data, allowed_items, blocked_items,
                                    exclude)
        l1 = np.ascontiguousarray(np.sort(arrayl1), dtype=np.float64)
        l2 = np.ascontiguousarray(np.sort(arrayl2), dtype=np.float64)
        best = [C.c_double(0.0) for _ in range(8)]
        cells = np.zeros((int(cv), l1.size * l2.size, _lib.CV_CELL), np.float64)
        t0 = time.time()
        try:
            rc = self._lib.Py_SLIM_MselectCV(data.handle, iopt, dopt, l1, l2, l1.size, l2.size, C.byref(spec),
                                             None if flt is None else flt.handle,
                                             *([C.byref(b) for b in best] + [cells.ctypes.data_as(C.c_void_p)]))
        finally:
            if flt is not None:
                flt.close()
        elapsed = time.time() - t0
        l1hr, l2hr, hrhr, arhr, l1ar, l2ar, hrar, arar = [b.value for b in best]
        if rc != SLIM_OK:
            raise RuntimeError(
                "Something went wrong with model estimation or evaluation when l1=%.4f, "
                "l2=%.4f. Please check the input matrix. [%s]" % (l1hr, l2hr, _lib.last_error()))
        print("Model selection takes %.3f secs." % elapsed)
        print("The best mean HR over %d folds is achieved by, l1: %.4f, l2:%.4f, HR:%.4f, AR:%.4f."
              % (cv, l1hr, l2hr, hrhr, arhr))
        print("The best mean AR over %d folds is achieved by, l1: %.4f, l2:%.4f, HR:%.4f, AR:%.4f."
              % (cv, l1ar, l2ar, hrar, arar))
        self.mselect_result = dict(bestHR=(l1hr, l2hr, hrhr, arhr), bestAR=(l1ar, l2ar, hrar, arar))
        names = ("fold", "l1", "l2", "hr", "hr_head", "hr_tail", "arhr", "nvalid", "nvalid_head", "nvalid_tail", "nnz")
        ints = ("fold", "nvalid", "nvalid_head", "nvalid_tail", "nnz")
        self.last_cv = [[{k: (int(v) if k in ints else float(v)) for k, v in zip(names, row)} for row in fold]
                        for fold in cells]

    def mselect(self, params, trndata, tstdata, arrayl1, arrayl2, nrcmds, allowed_items=None, blocked_items=None,
                exclude=None, nnegs=0, negseed=1, negpop=False, exposure=False, groups=None, history_bands=None,
                select_group=None, cv=None, cv_mode="leave_out", cv_held=1, cv_minkeep=1, cv_seed=1):
        """cv=F (include/slim_gpu_split.h): trndata is the ONE interactions matrix and tstdata must be None; the
        library holds items out itself, reproducibly from cv_seed, and runs the grid once per fold.  cv_mode
        "leave_out": every user with at least F * cv_held + cv_minkeep entries holds out cv_held of them in each
        fold; "folds": every entry belongs to one of F folds, and a user takes part in a fold that leaves it
        cv_minkeep entries.  A pair is judged by the mean of its fold figures; the table stays on the object as
        last_cv: one list per fold of one dict per pair, in the order solved, with fold, l1, l2, hr, hr_head, hr_tail,
        arhr, nvalid, nvalid_head, nvalid_tail, nnz.  It combines with the filter arguments, nnegs and negpop, and not
        with exposure=True, groups or history_bands.
        groups / history_bands (at most one; include/slim_gpu_groups.h): every pair is also evaluated per user group,
        from the same scoring pass.  groups: an integer array over trndata's user rows (0 .. ngroups-1, or -1 for no
        group), or a dict {ORIGINAL user id: group} mapped through trndata's user map -- users the map does not know
        are ignored, users the dict does not name are in no group.  history_bands: ascending bounds >= 1; the group of
        a user is the number of bounds the length of its training row reaches.  One more line is printed per group
        and the table stays on the object as last_groups: one list per pair, in the order solved, of one dict per
        group and a last one for everybody (group -1) with l1, l2, hr, hr_head, hr_tail, arhr, nvalid, nvalid_head,
        nvalid_tail.  select_group=g: the best pairs are chosen on group g's figures.  It needs the evaluation in HBM,
        combines with the filter arguments, nnegs and params["gpu_evalexposure"], and not with exposure=True (the
        exposure table is everybody's).
        exposure=True (or params["gpu_evalexposure"] = 1): besides HR / ARHR every pair reports what its lists show
        (include/slim_gpu_exposure.h) -- catalogue coverage, tail share, Gini and mean popularity of the top-nrcmds
        lists, counted on the device where the evaluation makes them.  One more line is printed per pair and the
        table stays on the object as last_exposure: one dict per pair, in the order solved, with l1, l2, hr, arhr,
        coverage, tail_share, gini, avg_pop.  The best pairs are chosen as before.  It needs the evaluation in HBM and
        nrcmds <= 128, combines with the filter arguments and does not combine with nnegs.
        nnegs > 0 (or params["gpu_evalnegs"] / ["gpu_evalseed"]): evaluate every pair 1-vs-k -- each held-out item
        against nnegs sampled items outside the user's history and test row, drawn once on the device from negseed
        (include/slim_gpu_sample.h); a score tie goes to the negative.  It takes no filter, needs nrcmds <= 128 and
        the evaluation in HBM, and costs about what the full-catalogue evaluation costs.  negpop=True (or
        params["gpu_evalnegpop"] = 1): the negatives are drawn in proportion to item popularity, not uniformly;
        without nnegs that is refused.
        allowed_items / blocked_items / exclude: evaluate every pair under a candidate filter, with the rules
        of predict() -- ORIGINAL item ids through trndata's maps, at most one of allowed and blocked, unknown ids
        ignored, exclude a SLIMatrix whose rows are put in the order of trndata's users.  A held-out item the
        filter removes counts as a miss.  (An engine extension; it needs the evaluation in HBM.)"""
        if not isinstance(exposure, (bool, np.bool_)):
            raise TypeError("exposure must be True or False.")
        self.last_cv = None
        if cv is not None:
            if tstdata is not None:
                raise TypeError("cv holds items out of trndata itself: pass tstdata=None, or no cv.")
            if exposure or groups is not None or history_bands is not None or select_group is not None:
                raise TypeError("cv does not combine with exposure=True, groups, history_bands or select_group.")
            return self._mselect_cv(params, trndata, arrayl1, arrayl2, nrcmds, allowed_items, blocked_items, exclude,
                                    nnegs, negseed, negpop, cv, cv_mode, cv_held, cv_minkeep, cv_seed)
        if exposure and nnegs:
            raise TypeError("exposure=True does not combine with nnegs: the exposure of sampled lists is not built.")
        assert type(trndata) == SLIMatrix, "trndata must be a SLIMatrix object."
        assert type(tstdata) == SLIMatrix, "tstdata must be a SLIMatrix object."
        if allowed_items is not None and blocked_items is not None:
            raise TypeError("Please provide at most one of allowed_items and blocked_items.")
        group_of_user, ngroups = _user_groups(self._lib, trndata, groups, history_bands)
        if group_of_user is None and select_group is not None:
            raise TypeError("select_group chooses on a user group: give groups or history_bands.")
        if group_of_user is not None and exposure:
            raise TypeError("exposure=True does not combine with groups: the exposure table is everybody's.")
        if select_group is not None and not (isinstance(select_group, (int, np.integer)) and
                                             0 <= select_group < ngroups):
            raise TypeError("select_group must be a group, 0 to %d." % (ngroups - 1))
        assert type(arrayl1) in [list, np.ndarray], "Please provide a list of l1 values."
        assert type(arrayl2) in [list, np.ndarray], "Please provide a list of l2 values."
        view = _prepare(params)
        view.set("nrcmds", nrcmds)
        iopt, dopt = build_options(view)
        if nnegs:
            iopt[Opt.GPU_EVALNEGS], iopt[Opt.GPU_EVALSEED] = int(nnegs), int(negseed)
        if negpop:
            iopt[Opt.GPU_EVALNEGPOP] = 1
        if len(arrayl1) < 1:
            raise TypeError("The l1 array must not be empty.")
        if len(arrayl2) < 1:
            raise TypeError("The l2 array must not be empty.")
        best = [C.c_double(0.0) for _ in range(8)]
        grid = (trndata.handle, tstdata.handle, iopt, dopt,
                np.ascontiguousarray(np.sort(arrayl1), dtype=np.float64),
                np.ascontiguousarray(np.sort(arrayl2), dtype=np.float64),
                len(arrayl1), len(arrayl2)) + tuple(C.byref(b) for b in best)
        t0 = time.time()
        self.last_exposure = None
        self.last_groups = None
        cells = np.zeros((len(arrayl1) * len(arrayl2), _lib.EXPOSURE_CELL), np.float64) if exposure else None
        if group_of_user is not None:
            cells = np.zeros((len(arrayl1) * len(arrayl2), ngroups + 1, _lib.GROUP_CELL), np.float64)
            flt = None
            if not (allowed_items is None and blocked_items is None and exclude is None):
                ncols = max(int(C.cast(trndata.handle, C.POINTER(_lib.CsrView)).contents.ncols), 1)
                flt = _candidate_filter(self._lib, trndata.item2id, trndata.nItems, ncols, trndata, allowed_items,
                                        blocked_items, exclude)
            try:
                rc = self._lib.Py_SLIM_MselectGrouped(*(grid + (
                    None if flt is None else flt.handle, ngroups, group_of_user.ctypes.data_as(C.c_void_p),
                    -1 if select_group is None else int(select_group), cells.ctypes.data_as(C.c_void_p))))
            finally:
                if flt is not None:
                    flt.close()
        elif exposure and allowed_items is None and blocked_items is None and exclude is None:
            rc = self._lib.Py_SLIM_MselectExposure(*(grid + (None, cells.ctypes.data_as(C.c_void_p))))
        elif allowed_items is None and blocked_items is None and exclude is None:
            rc = self._lib.Py_SLIM_Mselect(*grid)
        else:   # the models of the grid are as wide as the staged training matrix: its largest item id + 1
            ncols = max(int(C.cast(trndata.handle, C.POINTER(_lib.CsrView)).contents.ncols), 1)
            flt = _candidate_filter(self._lib, trndata.item2id, trndata.nItems, ncols, trndata, allowed_items,
                                    blocked_items, exclude)
            try:
                if exposure:
                    rc = self._lib.Py_SLIM_MselectExposure(*(grid + (flt.handle, cells.ctypes.data_as(C.c_void_p))))
                else:
                    rc = self._lib.Py_SLIM_MselectFiltered(*(grid + (flt.handle,)))
            finally:
                flt.close()
        elapsed = time.time() - t0
        l1hr, l2hr, hrhr, arhr, l1ar, l2ar, hrar, arar = [b.value for b in best]
        if rc != SLIM_OK:
            raise RuntimeError(
                "Something went wrong with model estimation or evaluation when l1=%.4f, "
                "l2=%.4f. Please check the input matrix. [%s]" % (l1hr, l2hr, _lib.last_error()))
        print("Model selection takes %.3f secs." % elapsed)
        print("The best HR is achieved by, l1: %.4f, l2:%.4f, HR:%.4f, AR:%.4f."
              % (l1hr, l2hr, hrhr, arhr))
        print("The best AR is achieved by, l1: %.4f, l2:%.4f, HR:%.4f, AR:%.4f."
              % (l1ar, l2ar, hrar, arar))
        self.mselect_result = dict(bestHR=(l1hr, l2hr, hrhr, arhr), bestAR=(l1ar, l2ar, hrar, arar))
        if group_of_user is not None:
            names = ("l1", "l2", "hr", "hr_head", "hr_tail", "arhr")
            counts = ("nvalid", "nvalid_head", "nvalid_tail")
            self.last_groups = [[dict(dict(zip(names, (float(v) for v in row[:6]))),
                                      group=g if g < ngroups else -1, **dict(zip(counts, (int(v) for v in row[6:]))))
                                 for g, row in enumerate(pair)] for pair in cells]
        if exposure:
            names = ("l1", "l2", "hr", "arhr", "coverage", "tail_share", "gini", "avg_pop")
            self.last_exposure = [dict(zip(names, (float(v) for v in row))) for row in cells]

    # -- prediction ----------------------------------------------------------
    def _candidate_filter(self, data, allowed_items, blocked_items, exclude):
        """The ItemFilter of predict(): original ids through the model's item map, the rows of `exclude` put in
        the order of data's users."""
        ncols = int(C.cast(self.handle, C.POINTER(_lib.CsrView)).contents.ncols)
        return _candidate_filter(self._lib, self.item2id, self.nItems, ncols, data, allowed_items, blocked_items,
                                 exclude)

    def predict(self, data, nrcmds=10, outfile=None, negitems=None, nnegs=0, returnscores=False,
                allowed_items=None, blocked_items=None, exclude=None):
        """allowed_items / blocked_items (at most one): ORIGINAL item ids that alone may / may not be
        recommended; exclude: a SLIMatrix built against the same maps whose row of a user holds the items never
        shown to that user.  Ids the model does not know are ignored.  (An engine extension: the reference's
        predict has no filters.)"""
        if self.ismodel != SLIM_OK:
            raise TypeError("Model not found. Please train a model.")
        assert self.nItems == data.nItems, \
            "The shape of the input matrix should match the model."
        filtered = not (allowed_items is None and blocked_items is None and exclude is None)
        if filtered and negitems is not None:
            raise TypeError("Item filters do not apply to the prediction over negative items.")
        res = np.full(data.nUsers * nrcmds, -1, dtype=np.int32)
        scores = np.zeros(data.nUsers * nrcmds, dtype=np.float32)
        user_is_dict = isinstance(data.user2id, dict)

        if negitems is not None:
            assert nnegs >= nrcmds, ("The number of negative items must be larger than the "
                                     "number of items to be recommended.")
            if user_is_dict:
                assert data.user2id.keys() == negitems.keys(), \
                    "The users in the negative items should be the same with the input matrix."
            else:
                assert np.array_equal(data.user2id, np.array(sorted(negitems.keys()))), \
                    "The users in the negative items should be the same with the input matrix."
            cand = np.full(data.nUsers * nnegs, -1, dtype=np.int32)
            unknown = 0
            for user, items in negitems.items():
                assert len(items) == nnegs, "The number of negative items should match nngs."
                base = data.user2id[user] * nnegs
                for j, it in enumerate(items):
                    try:
                        cand[base + j] = self.item2id[it]
                    except (KeyError, IndexError):
                        unknown += 1
            if unknown:
                print("%d negative items not in the training set." % unknown)
            rc = self._lib.Py_SLIM_Predict_1vsk(nrcmds, nnegs, self.handle, data.handle, cand,
                                                res, scores)
        elif filtered:
            flt = self._candidate_filter(data, allowed_items, blocked_items, exclude)
            try:
                rc = self._lib.Py_SLIM_PredictFiltered(nrcmds, self.handle, data.handle, flt.handle, res, scores)
            finally:
                flt.close()
        else:
            rc = self._lib.Py_SLIM_Predict(nrcmds, self.handle, data.handle, res, scores)
        if rc != SLIM_OK:
            raise RuntimeError(
                "Something went wrong during prediction. Please check 1) if the model is "
                "estimated correctly; 2) if the input matrix for prediction is correct.")

        # unfilled slots hold -1 and, as in the reference (core.py:584), index the
        # item map from the end
        res = np.asarray(self.id2item)[res].reshape(data.nUsers, nrcmds)
        scores = scores.reshape(data.nUsers, nrcmds)
        pairs = data.user2id.items() if user_is_dict else ((k, k) for k in data.user2id)
        out, outscores = {}, {}
        for key, row in pairs:
            out[key] = res[row, :]
            outscores[key] = scores[row, :]
        if outfile:
            with open(outfile, "w") as f:
                for key, value in out.items():
                    f.write(str(key) + ": " + np.array2string(value, max_line_width=np.inf) + "\n")
                    if returnscores:
                        f.write(str(key) + ": " +
                                np.array2string(outscores[key], max_line_width=np.inf) + "\n")
        return (out, outscores) if returnscores else out

    def rerank(self, data, candidates, nrcmds=None, returnscores=False):
        """Order the caller's own candidates per user (an engine extension, include/slim_gpu_cand.h): `candidates`
        maps a user of `data` to a sequence of ORIGINAL item ids, of any length per user.  Every candidate gets its
        1-vs-k score (history items are scored too; an item the model does not know scores 0 and is counted like
        predict does); returns a dict from user to the items in model order -- score descending, ties in the
        order given -- cut at nrcmds, and a dict of their scores with returnscores."""
        if self.ismodel != SLIM_OK:
            raise TypeError("Model not found. Please train a model.")
        assert self.nItems == data.nItems, "The shape of the input matrix should match the model."
        user_is_dict = isinstance(data.user2id, dict)
        rows = [None] * data.nUsers
        for user, items in candidates.items():
            try:
                rows[int(data.user2id[user])] = (user, list(items))
            except (KeyError, IndexError):
                raise KeyError("rerank: user %r is not in the input matrix" % (user,))
        cptr = np.zeros(data.nUsers + 1, np.int64)
        for u, r in enumerate(rows):
            cptr[u + 1] = cptr[u] + (len(r[1]) if r else 0)
        cind = np.full(int(cptr[-1]) + 1, -1, np.int32)
        unknown = 0
        for u, r in enumerate(rows):
            for j, it in enumerate(r[1] if r else ()):
                try:
                    cind[cptr[u] + j] = self.item2id[it]
                except (KeyError, IndexError):
                    unknown += 1
        if unknown:
            print("%d candidate items not in the training set." % unknown)
        ncols = int(C.cast(self.handle, C.POINTER(_lib.CsrView)).contents.ncols)
        cs = C.c_void_p()
        if self._lib.SLIMGPU_CandSetCreate(ncols, data.nUsers, cptr.ctypes.data_as(C.c_void_p),
                                           cind.ctypes.data_as(C.c_void_p), C.byref(cs)) != SLIM_OK:
            raise RuntimeError("Something went wrong with the candidate set. [%s]" % _lib.last_error())
        slot = np.zeros(cind.size, np.float32)
        try:
            rc = self._lib.Py_SLIM_ScoreCandidates(self.handle, data.handle, cs, 0, slot.ctypes.data_as(C.c_void_p),
                                                   None, None, None)
        finally:
            self._lib.SLIMGPU_CandSetFree(cs)
        if rc != SLIM_OK:
            raise RuntimeError("Something went wrong during prediction. [%s]" % _lib.last_error())
        out, outscores = {}, {}
        for u, r in enumerate(rows):
            if r is None:
                continue
            sc = slot[cptr[u]:cptr[u + 1]]
            order = np.argsort(-sc, kind="stable")     # score descending, then slot ascending
            if nrcmds is not None:
                order = order[:nrcmds]
            out[r[0]] = [r[1][j] for j in order]
            outscores[r[0]] = sc[order]
        return (out, outscores) if returnscores else out

    def explain(self, data, lists, nwhy=3):
        """Why the model scores an item for a user (an engine extension, include/slim_gpu_explain.h): `lists` maps a
        user of `data` to a sequence of ORIGINAL item ids, as predict() and rerank() return them.  Returns a dict from
        user to one list per item, [(original id of a history item, term), ...]: the at most nwhy (1 to 16) largest
        terms r[u, h] * w[h, item] of the item's score, term descending, ties in history order.  An item the model
        does not know gets an empty explanation and is counted like rerank does."""
        if self.ismodel != SLIM_OK:
            raise TypeError("Model not found. Please train a model.")
        assert self.nItems == data.nItems, "The shape of the input matrix should match the model."
        nwhy = int(nwhy)
        rows = [None] * data.nUsers
        for user, items in lists.items():
            try:
                rows[int(data.user2id[user])] = (user, list(items))
            except (KeyError, IndexError):
                raise KeyError("explain: user %r is not in the input matrix" % (user,))
        cptr = np.zeros(data.nUsers + 1, np.int64)
        for u, r in enumerate(rows):
            cptr[u + 1] = cptr[u] + (len(r[1]) if r else 0)
        cind = np.full(int(cptr[-1]) + 1, -1, np.int32)
        unknown = 0
        for u, r in enumerate(rows):
            for j, it in enumerate(r[1] if r else ()):
                try:
                    cind[cptr[u] + j] = self.item2id[it]
                except (KeyError, IndexError):
                    unknown += 1
        if unknown:
            print("%d candidate items not in the training set." % unknown)
        ncols = int(C.cast(self.handle, C.POINTER(_lib.CsrView)).contents.ncols)
        cs = C.c_void_p()
        if self._lib.SLIMGPU_CandSetCreate(ncols, data.nUsers, cptr.ctypes.data_as(C.c_void_p),
                                           cind.ctypes.data_as(C.c_void_p), C.byref(cs)) != SLIM_OK:
            raise RuntimeError("Something went wrong with the candidate set. [%s]" % _lib.last_error())
        why = np.full(cind.size * max(nwhy, 1), -1, np.int32)
        terms = np.zeros(cind.size * max(nwhy, 1), np.float32)
        support = np.zeros(cind.size, np.int32)
        try:
            rc = self._lib.Py_SLIM_ExplainCandidates(self.handle, data.handle, cs, nwhy,
                                                     why.ctypes.data_as(C.c_void_p), terms.ctypes.data_as(C.c_void_p),
                                                     support.ctypes.data_as(C.c_void_p))
        finally:
            self._lib.SLIMGPU_CandSetFree(cs)
        if rc != SLIM_OK:
            raise RuntimeError("Something went wrong during the explanation. [%s]" % _lib.last_error())
        id2item = np.asarray(self.id2item)
        out = {}
        for u, r in enumerate(rows):
            if r is None:
                continue
            per_item = []
            for j in range(len(r[1])):
                e = int(cptr[u]) + j
                n = min(nwhy, int(support[e]))
                hs = id2item[why[e * nwhy:e * nwhy + n]]
                per_item.append([(hs[k].item(), float(terms[e * nwhy + k])) for k in range(n)])
            out[r[0]] = per_item
        return out

    # -- persistence -----------------------------------------------------------
    def save_model(self, modelfname, mapfname):
        if self.ismodel != SLIM_OK:
            raise RuntimeError("Not exist a model to save.")
        self._lib.Py_csr_save(self.handle, modelfname.encode("utf-8"))
        np.savetxt(mapfname, self.id2item, fmt="%s")

    def load_model(self, modelfname, mapfname):
        if not (os.path.isfile(modelfname) and os.path.isfile(mapfname)):
            raise RuntimeError("File does not exist or invalid filename.")
        if self.ismodel == SLIM_OK and self.handle is not None:
            self._lib.Py_csr_free(self.handle)
        handle = C.c_void_p()
        self.ismodel = self._lib.Py_csr_load(C.byref(handle), modelfname.encode("utf-8"))
        self.handle = handle if self.ismodel == SLIM_OK else None
        try:
            self.id2item = np.genfromtxt(mapfname, dtype=np.int32)
        except Exception:
            self.id2item = np.genfromtxt(mapfname)
        self.id2item = np.atleast_1d(self.id2item)
        self.item2id = {self.id2item[i]: i for i in range(len(self.id2item))}
        self.nItems = len(self.id2item)
        if self.ismodel != SLIM_OK:
            raise RuntimeError("Fail to laod the model.")

    def to_csr(self, returnmap=False):
        if self.ismodel != SLIM_OK:
            raise RuntimeError("Not exist a model to export.")
        nnz = C.c_int(0)
        self._lib.Py_csr_stat(self.handle, C.byref(nnz))
        view = C.cast(self.handle, C.POINTER(_lib.CsrView)).contents
        nrows = max(int(view.nrows), 0)
        indptr = np.zeros(max(self.nItems, nrows) + 1, dtype=np.int32)
        indices = np.zeros(nnz.value, dtype=np.int32)
        data = np.ones(nnz.value, dtype=np.float32)
        self._lib.Py_csr_export(self.handle, indptr, indices, data)
        indptr[nrows + 1:] = indptr[nrows]  # trailing unrated items: empty rows
        model = sp.csr_matrix((data, indices, indptr[:self.nItems + 1]),
                              shape=(self.nItems, self.nItems))
        return (model, self.id2item[:]) if returnmap else model
