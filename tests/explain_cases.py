"""Shared by tests/test_explain.py and tests/test_explain_host.py: the yardstick of the explanations
(include/slim_gpu_explain.h) and the hand-built case `edges`.

The yardstick is never the code under test: pure numpy over the case's scipy model and its history arrays.  Per slot
the terms are np.float32(r) * np.float32(w) over the history positions whose model row stores the slot's id, ordered
by (-term, position) with a stable lexsort on values, so that -0.0 ties with 0.0.
"""
import ctypes as C

import numpy as np
import scipy.sparse as sp

from candidate_cases import CNT_FILL, ID_FILL, SC_FILL
from filtered_cases import make_model
from slim_amd.constants import SLIM_OK
from slim_amd.engine import DeviceMatrix, _scipy_to_model_handle

EDGE_LENGTHS = (0, 1, 63, 64, 65, 128, 129, 200)


def history_arrays(case):
    """(hptr, hind, hval): the histories as the host handle of the case holds them (hval None: binary)."""
    if hasattr(case, "hptr"):
        return case.hptr, case.hind, case.hval
    return (np.asarray(case.R.indptr, np.int64), np.asarray(case.R.indices, np.int32),
            None if case.binary else np.asarray(case.R.data, np.float32))


def live_slots(row, ncols):
    """Slot -> True where the slot carries the score: an id inside [0, ncols), of a repeated id the last one."""
    last = {}
    for j, i in enumerate(row.tolist()):
        if 0 <= i < ncols:
            last[i] = j
    live = np.zeros(row.size, bool)
    live[list(last.values())] = True
    return live


def yardstick_terms(case, indptr, indices, users=None):
    """{user: [per slot (positions, items, terms)]}: ALL the terms of every slot in the order of the explanation
    (term descending, then position ascending); three empty arrays for a slot that carries nothing."""
    hptr, hind, hval = history_arrays(case)
    W = case.W
    wptr, wind, wval = W.indptr, W.indices, W.data.astype(np.float32)
    nothing = (np.zeros(0, np.int64), np.zeros(0, np.int32), np.zeros(0, np.float32))
    out = {}
    for u in (range(min(hptr.size, indptr.size) - 1) if users is None else users):
        hist = hind[hptr[u]:hptr[u + 1]]
        r = np.ones(hist.size, np.float32) if hval is None else hval[hptr[u]:hptr[u + 1]].astype(np.float32)
        has_row = (hist >= 0) & (hist < W.shape[0])
        pieces = [np.arange(wptr[h], wptr[h + 1]) if ok else np.zeros(0, np.int64) for h, ok in zip(hist, has_row)]
        at = np.concatenate(pieces) if pieces else np.zeros(0, np.int64)
        pos = np.repeat(np.arange(hist.size), [p.size for p in pieces]) if pieces else np.zeros(0, np.int64)
        cols = wind[at]
        terms = (r[pos] * wval[at]).astype(np.float32)      # float32 * float32: the product rounded on its own
        by_col = np.argsort(cols, kind="stable")            # (stable: positions ascend inside a column)
        cols_sorted = cols[by_col]
        row = indices[indptr[u]:indptr[u + 1]]
        live = live_slots(row, case.ncols)
        slots = []
        for j, i in enumerate(row.tolist()):
            if not live[j]:
                slots.append(nothing)
                continue
            sel = by_col[np.searchsorted(cols_sorted, i, "left"):np.searchsorted(cols_sorted, i, "right")]
            p, t = pos[sel], terms[sel]
            order = np.lexsort((p, -t))                     # values, not bits: -0.0 == 0.0
            slots.append((p[order].astype(np.int64), hist[p[order]].astype(np.int32), t[order]))
        out[u] = slots
    return out


def sum_in_position_order(positions, terms):
    """The float32 sum of the terms from 0.0f, one addition each, in history order."""
    s = np.float32(0.0)
    for k in np.argsort(positions, kind="stable"):
        s = np.float32(s + terms[k])
    return s


def positions_of(hist, items):
    """History positions of an explanation's items: equal items take their positions in ascending order (equal
    terms come back in position order)."""
    used, out = {}, []
    where = {}
    for p, h in enumerate(hist.tolist()):
        where.setdefault(h, []).append(p)
    for h in items.tolist():
        k = used.get(h, 0)
        out.append(where[h][k])
        used[h] = k + 1
    return np.array(out, np.int64)


def buffers(indptr, nwhy):
    """(why_items, why_terms, support) of one call, preset with the sentinels of candidate_cases."""
    n = max(int(indptr[-1]), 1)
    return (np.full(n * nwhy, ID_FILL, np.int32), np.full(n * nwhy, SC_FILL, np.float32),
            np.full(n, CNT_FILL, np.int32))


def untouched(bufs):
    items, terms, support = bufs
    return bool((items == ID_FILL).all() and (terms == np.float32(SC_FILL)).all() and (support == CNT_FILL).all())


_dense = {}     # id(yardstick) -> its first 16 places as arrays, made once


def dense(want, indptr):
    """(items [entries, 16], terms [entries, 16], support [entries]) of a yardstick; sentinels beyond a slot's terms."""
    if id(want) not in _dense:
        n = int(indptr[-1])
        items, terms = np.full((n, 16), ID_FILL, np.int32), np.full((n, 16), SC_FILL, np.float32)
        support = np.zeros(n, np.int32)
        for u, slots in want.items():
            for j, (_, w_items, w_terms) in enumerate(slots):
                e, m = int(indptr[u]) + j, min(16, w_terms.size)
                items[e, :m], terms[e, :m], support[e] = w_items[:m], w_terms[:m], w_terms.size
        _dense[id(want)] = (want, items, terms, support)
    return _dense[id(want)][1:]


def check(bufs, indptr, want, users, nrows_total, nwhy):
    """Rows of `users`: support is the number of ALL terms, the first min(nwhy, support) places hold the yardstick's
    items and the bits of its terms, every place beyond keeps its sentinel; a slot that carries nothing has
    support 0 and nothing else; rows of other users keep every sentinel, support included."""
    items, terms, support = bufs
    w_items, w_terms, w_support = dense(want, indptr)
    n = int(indptr[nrows_total])
    sel = np.zeros(n, bool)
    for u in users:
        sel[int(indptr[u]):int(indptr[u + 1])] = True
    place = (np.arange(nwhy)[None, :] < np.minimum(w_support, nwhy)[:n, None]) & sel[:, None]
    exp_i = np.where(place, w_items[:n, :nwhy], ID_FILL).astype(np.int32)
    exp_t = np.where(place, w_terms[:n, :nwhy], np.float32(SC_FILL)).astype(np.float32)
    exp_s = np.where(sel, w_support[:n], CNT_FILL).astype(np.int32)
    got_i, got_t = items[:n * nwhy].reshape(n, nwhy), terms[:n * nwhy].reshape(n, nwhy)
    bad = (got_i != exp_i).any(1) | (got_t.view(np.int32) != exp_t.view(np.int32)).any(1) | (support[:n] != exp_s)
    if bad.any():
        e = int(np.argmax(bad))
        u = int(np.searchsorted(indptr, e, "right")) - 1
        raise AssertionError("user %d slot %d (%s): support %d items %s terms %s, not %d %s %s" % (
            u, e - int(indptr[u]), "selected" if sel[e] else "not selected", support[e], got_i[e], got_t[e], exp_s[e],
            exp_i[e], exp_t[e]))


class Edges(object):
    """The hand-built case: a 200 x 200 model of 0.25 / 0.5 with two coefficients of one column overwritten with -0.0
    (the earlier row) and 0.0; binary histories of the lengths EDGE_LENGTHS in an order that is not the order of the
    ids, and as user 8 of the HOST handle a history that holds items twice (a staged matrix takes users 0-7).
    Candidate rows: the whole catalogue plus -1, ncols and a repeated id, shuffled."""
    name, binary = "edges", True

    def __init__(self, lib):
        self.lib = lib
        rng = np.random.default_rng(71)
        W = make_model(200, 8, 12, ties=True, seed=73)
        Wc = W.tocsc()
        col = int(np.argmax(np.diff(Wc.indptr) >= 2))
        a, b = Wc.indices[Wc.indptr[col]:Wc.indptr[col] + 2]         # a < b: two rows that store `col`
        for row, zero in ((a, -0.0), (b, 0.0)):
            k = W.indptr[row] + int(np.searchsorted(W.indices[W.indptr[row]:W.indptr[row + 1]], col))
            assert W.indices[k] == col
            W.data[k] = zero
        self.W, self.zero_col, self.zero_rows = W, col, (int(a), int(b))
        self.ncols = 200
        rows = []
        for n in EDGE_LENGTHS:
            ids = rng.choice(200, size=n, replace=False)
            if n >= 2:      # the two zero rows in every history of two or more: -0.0 in front of 0.0, and behind it
                ids = np.concatenate(([a, b] if n % 2 else [b, a], np.setdiff1d(ids, [a, b])[:n - 2]))
                ids[2:] = ids[2:][rng.permutation(n - 2)]
            rows.append(ids.astype(np.int32))
        twice = rng.choice(200, size=40, replace=False).astype(np.int32)
        rows.append(np.concatenate((twice, twice[:7], [a, b, a])).astype(np.int32))
        self.nusers, self.nstaged = len(rows), len(rows) - 1
        self.hptr = np.concatenate(([0], np.cumsum([r.size for r in rows]))).astype(np.int64)
        self.hind = np.concatenate(rows).astype(np.int32)
        self.hval = None
        self.hw = _scipy_to_model_handle(lib, W)
        self.hr = self._history_handle(self.nusers)
        ptr, ind = [0], []
        for _ in range(self.nusers):
            row = np.concatenate((np.arange(200), [-1, 200, col, int(rng.integers(200))]))
            ind.append(row[rng.permutation(row.size)])
            ptr.append(ptr[-1] + row.size)
        self.indptr, self.indices = np.array(ptr, np.int64), np.concatenate(ind).astype(np.int32)
        self._mat = self._model = None

    def _history_handle(self, nrows):
        """Py_csr_wrapper over the first rows as they are (scipy's constructor would not keep a repeated item)."""
        h = C.c_void_p()
        n = int(self.hptr[nrows])
        assert self.lib.Py_csr_wrapper(nrows, np.ascontiguousarray(self.hptr[:nrows + 1], np.intp),
                                       np.ascontiguousarray(self.hind[:n], np.int32), None, C.byref(h)) == SLIM_OK
        return h

    @property
    def mat(self):
        if self._mat is None:
            n = int(self.hptr[self.nstaged])
            R = sp.csr_matrix((self.nstaged, 200), dtype=np.float32)
            R.indptr, R.indices = self.hptr[:self.nstaged + 1].copy(), self.hind[:n].copy()
            R.data = np.ones(n, np.float32)
            self._mat = DeviceMatrix.from_scipy(R, binary=True)
            self._model = self._mat.model_from_scipy(self.W)
        return self._mat

    @property
    def model(self):
        assert self.mat is not None
        return self._model

    def close(self):
        if self._model is not None:
            self._model.free()
            self._mat.close()
        self.lib.SLIM_FreeModel(C.byref(self.hw))
        self.lib.Py_csr_free(self.hr)


def explain_cases_fixture():
    """cases_fixture of filtered_cases with `edges` beside its three; candidate rows and yardsticks are made once per
    (case, seed) and shared."""
    from filtered_cases import Case
    from slim_amd import _lib
    made, rows = {}, {}

    def get(name):
        if name not in made:
            made[name] = Edges(_lib.load()) if name == "edges" else Case(_lib.load(), name)
        return made[name]

    def get_rows(name, seed=83):
        """(indptr, indices, yardstick terms) of the case."""
        from candidate_cases import candidate_rows
        if (name, seed) not in rows:
            c = get(name)
            ptr, ind = (c.indptr, c.indices) if name == "edges" else candidate_rows(c, seed, long_row=False)
            rows[(name, seed)] = (ptr, ind, yardstick_terms(c, ptr, ind))
        return rows[(name, seed)]
    get.rows = get_rows
    yield get
    for c in made.values():
        c.close()
