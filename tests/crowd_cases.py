"""Shared by tests/test_later_positions.py: "crowd" fixtures -- tiny in items, large in users -- for the per-user
kernels, which launch min(positions, CUs x per CU) workgroups and let each serve several positions one after the
other, re-using its LDS state.  A fixture of a few hundred users gives every workgroup one position; these give some
workgroup three, which the tests assert from the SLIM_GPU_TRACE line of the launch (trace_launches, went_round).

The yardsticks are the ones the existing tests use, never the code under test: the numpy restatements of
tests/sampled_cases.py and tests/weighted_cases.py, the numpy terms of tests/explain_cases.py, the host scorer's full
ranking of tests/filtered_cases.py.

stale_share is a condition on the sampler fixture, from the restatement alone: had a workgroup left the bits of the
user it served before (its history, its test row, its accepted negatives) set in its LDS bitmap, how many of the later
rows would come out different?  A fixture on which few would could not see that bug.
"""
import ctypes as C
import re
import sys

import numpy as np
import scipy.sparse as sp

import sampled_cases as S
from slim_amd.constants import SLIM_OK
import weighted_cases as Wc

# ---- the trace line --------------------------------------------------------------------------------------------------
LAUNCH = re.compile(r"\[trace\] ([^:\n]+): (\d+) positions, (\d+) workgroups([^\n]*)")


def trace_launches(capfd, call):
    """Runs call() and returns (its result, [(kernel, positions, workgroups, rest of the line)]) from the library's
    stderr; SLIM_GPU_TRACE must be set by the caller (monkeypatch)."""
    C.CDLL(None).fflush(None)
    before = capfd.readouterr()
    out = call()
    C.CDLL(None).fflush(None)
    err = capfd.readouterr().err
    with capfd.disabled():      # what the test printed so far is shown, not dropped
        sys.stdout.write(before.out)
    return out, [(m.group(1), int(m.group(2)), int(m.group(3)), m.group(4)) for m in LAUNCH.finditer(err)]


def went_round(launches, kernel, positions=None):
    """The launch of `kernel` (a prefix of its name) with `positions` positions (None: the only one): asserts that it
    has more than two positions per workgroup, so that some workgroup served three; returns (positions, workgroups,
    rest of the line)."""
    hits = [l for l in launches if l[0].startswith(kernel) and (positions is None or l[1] == positions)]
    assert hits, "no trace line of %s (%s positions) among %s" % (kernel, positions, launches)
    _, npos, groups, rest = hits[0]
    assert npos > 2 * groups, ("%s: %d positions on %d workgroups: no workgroup serves three positions on this device. "
                               "Enlarge the crowd fixture (tests/crowd_cases.py) to more than %d positions."
                               % (hits[0][0], npos, groups, 2 * groups))
    return npos, groups, rest


# ---- the samplers ----------------------------------------------------------------------------------------------------
NITEMS, NUSERS, HIST = 600, 9000, 150
EMPTY = (7, 1500, 4097, 8999)          # users with an empty history (and a test row)
SEED = 5
SPARSE, DENSE = 20, 300                # nnegs of the uniform rule: 2 * (151 + 20) <= 600; 2 * (1 + 300) > 600
# (rule, nnegs): counts reach phase 2 seldom, cliff always -- 50 heavy items carry all draws of phase 1, a history
# takes about 12 of them, and the rest of the 45 comes from the items of weight 1 in phase 2
RULES = (("sparse", SPARSE), ("dense", DENSE), ("counts", 99), ("cliff", 45))


def no_test_row(u):
    return u % 10 == 3


class SamplerCrowd(object):
    """600 items, 9 000 users: 150 distinct history items drawn per user (EMPTY: none), one test item outside the
    history, every 10th user without a test row.  Expected rows are made once per (rule, users) and kept."""

    def __init__(self):
        rng = np.random.default_rng(101)
        hist, test = [], []
        for u in range(NUSERS):
            h = np.zeros(0, np.int64) if u in EMPTY else np.sort(rng.choice(NITEMS, HIST, replace=False))
            free = np.setdiff1d(np.arange(NITEMS), h)
            hist.append(h)
            test.append(np.zeros(0, np.int64) if no_test_row(u) else free[rng.integers(free.size, size=1)])
        self.R, self.T = self._csr(hist), self._csr(test)
        self.tptr, self.tind = self.T.indptr.astype(np.int64), self.T.indices
        self.ncols, self.nusers = NITEMS, NUSERS
        self.w = {"counts": Wc.weights("counts", self.R, NITEMS), "cliff": Wc.weights("cliff", self.R, NITEMS)}
        # more than 2 x 4096 positions, ascending, users[q] != q from the first on
        self.subset = np.array([u for u in range(NUSERS) if u % 12 != 0], np.int32)
        self._rows = {}

    @staticmethod
    def _csr(rows):
        M = sp.csr_matrix((len(rows), NITEMS), dtype=np.float32)
        M.indptr = np.cumsum([0] + [r.size for r in rows]).astype(np.int32)
        M.indices = np.concatenate(rows).astype(np.int32)
        M.data = np.ones(M.indices.size, np.float32)
        return M

    def X(self, u):
        """The taken ids of user u: history and test row."""
        return np.union1d(self.R.indices[self.R.indptr[u]:self.R.indptr[u + 1]],
                          self.tind[self.tptr[u]:self.tptr[u + 1]])

    def rows(self, rule, nnegs, users=None):
        """(indptr, indices) of the set: sampled_cases.sampled_rows / weighted_cases.weighted_rows."""
        k = (rule, nnegs, users is None)
        if k not in self._rows:
            if rule in ("sparse", "dense"):
                got = S.sampled_rows(self.R, self.tptr, self.tind, NITEMS, nnegs, SEED, users=users)
            else:
                got = Wc.weighted_rows(("crowd", rule), self.R, self.tptr, self.tind, NITEMS, nnegs, SEED,
                                       self.w[rule], users=users)
            for a in got:
                a.setflags(write=False)
            self._rows[k] = got
        return self._rows[k]

    def negatives_of(self, rule, nnegs, u):
        ptr, ind = self.rows(rule, nnegs)
        return ind[ptr[u]:ptr[u + 1] - (self.tptr[u + 1] - self.tptr[u])]

    def with_stale_bits(self, rule, nnegs, u, taken):
        """The negatives of user u had the ids `taken` been marked in the bitmap (the rule is still chosen from
        the user's own ids, as the kernel counts only the bits it sets itself)."""
        if rule in ("counts", "cliff"):
            return Wc.weighted_negatives(SEED, u, taken, nnegs, self.w[rule],
                                         Wc._ROWS.setdefault((("crowd", rule), "C"), Wc.prefix(self.w[rule])))[0]
        if S.rule(self.X(u).size, nnegs, NITEMS) == "sparse":
            draws = S.item(SEED, u, np.arange(16 * nnegs + 1024), NITEMS)
            _, first = np.unique(draws, return_index=True)
            seq = draws[np.sort(first)]
            return seq[~np.isin(seq, taken)][:nnegs].astype(np.int32)
        free = np.setdiff1d(np.arange(NITEMS), taken)
        return free[np.lexsort((free, S.key(SEED, u, free)))][:min(nnegs, free.size)].astype(np.int32)

    def stale_share(self, rule, nnegs, G, users=None, stride=1):
        """Among the positions p >= G that have a test row (every `stride`-th of them): the share whose row changes
        when the bits of the position its workgroup (p % G) served before -- X and the accepted negatives of the last
        position p - kG with a test row; one without marks nothing -- are still set.  Returns (share, positions)."""
        users = np.arange(NUSERS) if users is None else users
        last, differ, seen, n = {}, 0, 0, 0
        for p, u in enumerate(users.tolist()):
            if no_test_row(u):
                continue
            prev = last.get(p % G)
            last[p % G] = u
            if p < G:
                continue
            seen += 1
            if seen % stride:
                continue
            n += 1
            if prev is None:
                continue
            taken = np.union1d(np.union1d(self.X(u), self.X(prev)), self.negatives_of(rule, nnegs, prev))
            differ += not np.array_equal(self.with_stale_bits(rule, nnegs, u, taken), self.negatives_of(rule, nnegs, u))
        return differ / max(n, 1), n


# ---- the explanations ------------------------------------------------------------------------------------------------
STAGE = 16          # SLIM_EXPLAIN_STAGE of the crowd runs: histories of 2 to 40 entries lie on both sides of it


class ExplainCrowd(object):
    """5 000 users over a 200 x 200 model of 0.25 / 0.5 with 30 to 40 entries a row (equal terms are the rule), in the style of
    explain_cases.Edges: rated histories of 2 to 40 items (a few empty) in an order that is not the order of the ids;
    candidate rows of 8 to 12 entries with -1, ncols and a repeated id among them.  The yardstick's terms are made
    once."""
    name, binary, nusers, ncols = "crowd", False, 5000, 200

    def __init__(self, lib):
        from explain_cases import yardstick_terms
        from filtered_cases import make_model
        from slim_amd.engine import _scipy_to_model_handle
        self.lib = lib
        rng = np.random.default_rng(211)
        self.W = make_model(200, 30, 40, ties=True, seed=223)
        lens = rng.integers(2, 41, self.nusers)
        lens[[5, 2047, 2048, 4999]] = 0
        lens[[6, 2049, 4096]] = (STAGE - 1, STAGE, STAGE + 1)
        rows = [rng.choice(200, size=int(n), replace=False).astype(np.int32) for n in lens]
        self.hptr = np.concatenate(([0], np.cumsum(lens))).astype(np.int64)
        self.hind = np.concatenate(rows).astype(np.int32)
        self.hval = rng.integers(1, 6, self.hind.size).astype(np.float32)
        ptr, ind = [0], []
        for u in range(self.nusers):
            n = int(rng.integers(8, 13))
            row = rng.choice(200, size=n - 3, replace=False)
            row = np.concatenate((row, [-1, 200, row[0]]))
            ind.append(row[rng.permutation(n)])
            ptr.append(ptr[-1] + n)
        self.indptr, self.indices = np.array(ptr, np.int64), np.concatenate(ind).astype(np.int32)
        self.want = yardstick_terms(self, self.indptr, self.indices)
        self.hw = _scipy_to_model_handle(lib, self.W)
        self.hr = C.c_void_p()
        assert lib.Py_csr_wrapper(self.nusers, np.ascontiguousarray(self.hptr, np.intp), self.hind,
                                  self.hval.ctypes.data_as(C.c_void_p), C.byref(self.hr)) == SLIM_OK
        self._mat = self._model = None

    @property
    def mat(self):
        if self._mat is None:
            from slim_amd.engine import DeviceMatrix
            R = sp.csr_matrix((self.nusers, 200), dtype=np.float32)
            R.indptr, R.indices, R.data = self.hptr.copy(), self.hind.copy(), self.hval.copy()
            self._mat = DeviceMatrix.from_scipy(R)
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


# ---- the scorer modes ------------------------------------------------------------------------------------------------
class ScorerCrowd(object):
    """filtered_cases.Case("crowd-floats" / "crowd-ties"): 2 500 users x 400 items, the host scorer's full ranking as
    yardstick; with it, once: test rows (the user's rank-1 and rank-5 item, a history item, a never-touched item;
    every 6th user none), a head / tail marker, an allow set with per-user exclusions and the filtered ranking, and
    candidate rows of 8 to 12 ids with the order the host's 1-vs-k call gives them."""

    def __init__(self, case):
        from candidate_cases import yardstick
        self.c = c = case
        rng = np.random.default_rng(307)
        ptr, ind = [0], []
        for u in range(c.nusers):
            n = int(c.ncand[u])
            if u % 6 != 5 and n > 0:
                lst = c.ids[u, :n]
                hist = c.R.indices[c.R.indptr[u]:c.R.indptr[u + 1]]
                free = np.setdiff1d(np.arange(c.ncols), np.concatenate([lst, hist]))
                ind += [int(lst[0]), int(lst[min(4, n - 1)]), int(hist[rng.integers(hist.size)])]
                if free.size:
                    ind.append(int(free[rng.integers(free.size)]))
            ptr.append(len(ind))
        self.T = sp.csr_matrix((np.ones(len(ind), np.float32), np.array(ind, np.int32), np.array(ptr)),
                               shape=(c.nusers, c.ncols))
        self.fm = rng.integers(0, 2, c.ncols).astype(np.int32)
        self.allowed = rng.random(c.ncols) < 0.6
        self.X = c.exclusions(seed=311, xusers=c.nusers - 10)
        self.flt = c.expected(c.ncols, self.allowed, self.X)[:2]
        cptr, cind = [0], []
        for u in range(c.nusers):
            n = int(rng.integers(8, 13))
            row = rng.integers(0, c.ncols, n - 2).tolist() + [-1, c.ncols]
            if c.ncand[u]:
                row[0] = int(c.ids[u, 0])
            cind += [row[j] for j in rng.permutation(n)]
            cptr.append(len(cind))
        self.cptr, self.cind = np.array(cptr, np.int64), np.array(cind, np.int32)
        self.corder = yardstick(c, self.cptr, self.cind)
        # more than 2 x 1024 positions, ascending, users[q] != q from the first on
        self.subset = np.array([u for u in range(c.nusers) if u % 9 != 0], np.int32)

    def item_filter(self):
        return self.c.mat.item_filter(allowed=np.flatnonzero(self.allowed), exclusions=self.X)

    def lists(self, filtered):
        return self.flt if filtered else (self.c.ids, self.c.sc)
