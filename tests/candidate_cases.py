"""Shared by tests/test_candidates.py and tests/test_candidates_host.py: candidate rows over the cases of
tests/filtered_cases.py and the yardstick of the candidate sets (include/slim_gpu_cand.h).

The yardstick is never the code under test: per user, the EXISTING host call Py_SLIM_GetTopN_1vsk with
nrcmds = nnegs = row length gives the row's full order with its scores.  A slot-score array passes when sorting its
slots by (score descending, slot ascending) reproduces that order's ids and scores bit for bit.
"""
import ctypes as C

import numpy as np

from slim_amd.constants import SLIM_OK

P = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)  # noqa: E731
CHUNK_WIDTHS = (1536, 2304)     # the chunk scorer's two widths: 64-bit and 32-bit discovery keys
ID_FILL, SC_FILL, CNT_FILL = -7, -3.5, -9   # what a call must leave where it writes nothing


def candidate_rows(case, seed, nrows=None, long_row=True):
    """(indptr, indices) with `nrows` rows (default: one per user), built by hand: lengths 0, 1, 63, 64, 65, one row
    of 1100 (above the old cap), in `wide` one of 4096 and one of 4097, the rest random 2-70; contents: items of
    the user's history, the user's unfiltered top 3 (the first of them three times), never-touched items, -1 and
    ncols, ids 0 and ncols - 1, the ids on both sides of every multiple of the two chunk widths; shuffled."""
    rng = np.random.default_rng(seed)
    n, nrows = case.ncols, case.nusers if nrows is None else nrows
    lengths = {0: 0, 1: 1, 2: 63, 3: 64, 4: 65, 5: 1100}
    if case.name == "wide":     # (long_row=False: without the row that is too long for a list)
        lengths.update({6: 4096, 7: 4097} if long_row else {6: 4096})
    edges = sorted({m + d for w in CHUNK_WIDTHS for m in range(w, n, w) for d in (-1, 0)})
    ptr, ind = [0], []
    for u in range(nrows):
        L = lengths.get(u, int(rng.integers(2, 71)))
        special = [-1, n, 0, n - 1] + edges
        if u < case.nusers:
            hist = case.R.indices[case.R.indptr[u]:case.R.indptr[u + 1]]
            top = case.ids[u, :min(3, case.ncand[u])].tolist()
            free = np.setdiff1d(np.arange(n), np.concatenate([case.ids[u, :case.ncand[u]], hist]))
            special += top + top[:1] * 2
            special += rng.choice(hist, size=min(3, hist.size), replace=False).tolist()
            special += rng.choice(free, size=min(2, free.size), replace=False).tolist()
        special = [special[j] for j in rng.permutation(len(special))]
        row = special[:L] + rng.integers(0, n, size=max(0, L - len(special))).tolist()
        ind += [row[j] for j in rng.permutation(len(row))]
        ptr.append(len(ind))
    return np.array(ptr, np.int64), np.array(ind, np.int32)


def yardstick(case, indptr, indices):
    """Per user u < case.nusers: (ids, scores) of the row in the host's order, from Py_SLIM_GetTopN_1vsk."""
    lib, out = case.lib, []
    for u in range(min(case.nusers, indptr.size - 1)):
        row = np.ascontiguousarray(indices[indptr[u]:indptr[u + 1]])
        if row.size == 0:
            out.append((np.zeros(0, np.int32), np.zeros(0, np.float32)))
            continue
        h0, h1 = case.R.indptr[u], case.R.indptr[u + 1]
        hist = np.ascontiguousarray(case.R.indices[h0:h1], np.int32)
        val = None if case.binary else np.ascontiguousarray(case.R.data[h0:h1], np.float32)
        ids, sc = np.full(row.size, ID_FILL, np.int32), np.full(row.size, SC_FILL, np.float32)
        spare = np.zeros(1, np.int32)   # (an empty history still has an address)
        n = lib.Py_SLIM_GetTopN_1vsk(case.hw, hist.size, hist if hist.size else spare, P(val), row.size, ids, sc,
                                     row.size, row, 0)
        assert n == row.size
        out.append((ids, sc))
    return out


def make_set(lib, ncols, indptr, indices):
    """SLIMGPU_CandSetCreate: (status, handle)."""
    h = C.c_void_p()
    ptr = None if indptr is None else np.ascontiguousarray(indptr, np.int64)
    ind = np.concatenate((np.asarray(indices, np.int32), np.zeros(1, np.int32)))
    nrows = 0 if ptr is None else ptr.size - 1
    return lib.SLIMGPU_CandSetCreate(ncols, nrows, P(ptr), P(ind), C.byref(h)), h


def buffers(indptr, npos, nrcmds):
    """Output arrays of one call, preset with the sentinels: (slot_scores, ids, scores, counts)."""
    return (np.full(max(int(indptr[-1]), 1), SC_FILL, np.float32), np.full(max(npos * nrcmds, 1), ID_FILL, np.int32),
            np.full(max(npos * nrcmds, 1), SC_FILL, np.float32), np.full(max(npos, 1), CNT_FILL, np.int32))


def untouched(bufs):
    slot, ids, sc, cnt = bufs
    return bool((slot == np.float32(SC_FILL)).all() and (ids == ID_FILL).all() and (sc == np.float32(SC_FILL)).all()
                and (cnt == CNT_FILL).all())


def check_slot_scores(slot, indptr, indices, want, users, nrows_total):
    """Rows of `users`: their order reproduces the yardstick's; every other row keeps its sentinel."""
    sel = set(int(u) for u in users)
    for u in range(nrows_total):
        s = slot[indptr[u]:indptr[u + 1]]
        if u not in sel:
            assert (s == np.float32(SC_FILL)).all(), "row of unselected user %d was written" % u
            continue
        order = np.lexsort((np.arange(s.size), -s.astype(np.float64)))
        ids, sc = want[u]
        assert np.array_equal(indices[indptr[u]:indptr[u + 1]][order], ids), "user %d: order" % u
        assert np.array_equal(s[order].view(np.int32), sc.view(np.int32)), "user %d: scores" % u


def check_lists(bufs, indptr, want, users, nrcmds):
    """Position q holds the first min(nrcmds, row length) of its user's order; the slots beyond keep the sentinels."""
    _, ids, sc, cnt = bufs
    for q, u in enumerate(users):
        n = min(nrcmds, int(indptr[u + 1] - indptr[u]))
        assert cnt[q] == n, "user %d: count %d, not %d" % (u, cnt[q], n)
        got_i, got_s = ids[q * nrcmds:(q + 1) * nrcmds], sc[q * nrcmds:(q + 1) * nrcmds]
        assert np.array_equal(got_i[:n], want[u][0][:n]), "user %d: list ids" % u
        assert np.array_equal(got_s[:n].view(np.int32), want[u][1][:n].view(np.int32)), "user %d: list scores" % u
        assert (got_i[n:] == ID_FILL).all() and (got_s[n:] == np.float32(SC_FILL)).all(), "user %d: beyond" % u
