"""Exposure from the scoring pass of an evaluation (SLIMGPU_ModelEvaluateExposure) and of a lists call
(SLIMGPU_MatrixPredictExposure), on the cases of tests/filtered_cases.py.

The yardstick is never the code under test: filtered_cases.Case.expected -- the unchanged host scorer's full
ranking, filtered and cut in numpy -- counted with np.bincount and summarised in Python ints
(exposure_cases.restate).  The figures must be those of Evaluator.evaluate_at on the same set, bit for bit."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp

import slim_oracle as O
from exposure_cases import restate, same_summary
from filtered_cases import cases_fixture
from slim_amd import _lib
from slim_amd.constants import SLIM_ERROR_INPUT, SLIM_OK
from slim_amd.engine import eval_stats, list_stats

pytestmark = pytest.mark.gpu
cases = pytest.fixture(scope="module")(cases_fixture)
NAMES = ["floats", "ties", "wide"]
KEYS = ("hr", "hr_head", "hr_tail", "arhr")
NKEYS = ("nrcmds", "nvalid", "nvalid_head", "nvalid_tail")


class Setup(object):
    """Per case and once: test rows (rank 1 and rank 5 of every user with candidates; every 6th user none), the
    marker, the column counts, a filter's description: an allow set of half the items and exclusion rows."""

    def __init__(self, c):
        self.c = c
        ptr, ind = [0], []
        for u in range(c.nusers):
            n = int(c.ncand[u])
            if u % 6 != 5 and n > 0:
                ind += [int(c.ids[u, 0])] + ([int(c.ids[u, 4])] if n >= 5 else [])
            ptr.append(len(ind))
        self.T = sp.csr_matrix((np.ones(len(ind), np.float32), np.array(ind, np.int32), np.array(ptr)),
                               shape=(c.nusers, c.ncols))
        self.fm = np.ascontiguousarray(O.head_tail(sp.csr_matrix(c.R), c.ncols), np.int32)
        self.pop = np.bincount(c.R.indices, minlength=c.ncols).astype(np.uint32)
        self.allowed = np.random.default_rng(41).random(c.ncols) < 0.5
        self.X = c.exclusions(seed=89)
        self.subset = np.arange(2, c.nusers, 3)     # every third user; user 11 has no history
        assert c.mat.ncols == c.ncols

    def item_filter(self):
        return self.c.mat.item_filter(allowed=np.flatnonzero(self.allowed), exclusions=self.X)

    def want(self, cutoffs, users, filtered):
        """(E, summaries, counts of the longest lists) of the yardstick lists at every cutoff."""
        n = cutoffs[-1]
        ids, _, cnt = self.c.expected(n, self.allowed if filtered else None, self.X if filtered else None, users)
        E, summ = restate(self.c.ncols, ids, cnt, cutoffs, pop=self.pop, fmarker=self.fm)
        for k, ck in enumerate(cutoffs):    # the issue's statement of the counts, word for word
            lists = self.c.expected(ck, self.allowed if filtered else None, self.X if filtered else None, users)[0]
            assert np.array_equal(E[k], np.bincount(lists[lists >= 0], minlength=self.c.ncols))
        return E, summ, cnt


@pytest.fixture(scope="module")
def setups(cases):
    made = {}

    def get(name):
        if name not in made:
            made[name] = Setup(cases(name))
        return made[name]
    return get


def bits(rows, keys):
    return [np.float64(r[k]).view(np.int64) for r in rows for k in keys]


def no_empty_test(E, cnt, longest, some_never=True):
    """The conditions on the inputs, on the yardstick: a short list, an empty one, an item shown twice, one never."""
    assert (cnt < longest).any() and (cnt == 0).any()
    assert (E[-1] >= 2).any() and (not some_never or (E[-1] == 0).any())


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("cutoffs", [(1, 5, 10, 64), (3, 100, 128)], ids=["chunk", "wave"])
@pytest.mark.parametrize("subset", [False, True], ids=["everybody", "every-third"])
@pytest.mark.parametrize("filtered", [False, True], ids=["plain", "filtered"])
def test_evaluate_exposure(setups, name, cutoffs, subset, filtered):
    s = setups(name)
    c = s.c
    users = s.subset if subset else None
    wantE, wantS, cnt = s.want(cutoffs, users, filtered)
    no_empty_test(wantE, cnt, cutoffs[-1])
    flt = s.item_filter() if filtered else None
    ev = c.mat.evaluator(s.T, fmarker=s.fm, cutoffs=cutoffs, users=users)
    try:
        plain = ev.evaluate_at(c.model, filter=flt)
        path = eval_stats()["path"]
        fig, (E, summ) = ev.evaluate_exposure(c.model, filter=flt)
        assert np.array_equal(E, wantE)
        assert same_summary(summ, wantS)
        assert [d["nrcmds"] for d in summ] == list(cutoffs)
        print("figures", fig)
        assert bits(fig, KEYS) == bits(plain, KEYS) and [[r[k] for k in NKEYS] for r in fig] == \
            [[r[k] for k in NKEYS] for r in plain]
        assert any(r["hr"] > 0 for r in plain)
        # the second call: nothing allocated, nothing sent, the figures and the counters come down
        fig2, (E2, summ2) = ev.evaluate_exposure(c.model, filter=flt)
        st = eval_stats()
        print("stats", st)
        K = len(cutoffs)
        assert st["device_allocs"] == 0 and st["h2d_bytes"] == 0
        assert 0 < st["d2h_bytes"] <= 8 + 32 * K + 4 * K * c.ncols
        assert st["path"] == path and path == (1 if cutoffs[-1] <= 64 else 2)
        assert np.array_equal(E2, wantE) and same_summary(summ2, wantS) and bits(fig2, KEYS) == bits(plain, KEYS)
        # ... and the plain evaluation after it is what it was
        again = ev.evaluate_at(c.model, filter=flt)
        assert bits(again, KEYS) == bits(plain, KEYS)
    finally:
        ev.close()
        if flt is not None:
            flt.close()


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("nrcmds", [10, 200, "ncols"])
@pytest.mark.parametrize("subset,filtered", [(False, False), (True, True)], ids=["everybody-plain", "third-filtered"])
def test_predict_exposure(setups, name, nrcmds, subset, filtered):
    s = setups(name)
    c = s.c
    n = min(c.ncols, _lib.MAX_LIST) if nrcmds == "ncols" else nrcmds
    cutoffs = (1, n // 2, n)
    users = s.subset if subset else None
    wantE, wantS, cnt = s.want(cutoffs, users, filtered)
    # (lists as long as the catalogue show every item of "ties" and "wide" unless a filter removes some)
    no_empty_test(wantE, cnt, n, some_never=filtered or nrcmds != "ncols")
    if n == c.ncols:
        assert (cnt < n).all()      # the long lists are longer than every candidate count
    elif nrcmds == "ncols":
        assert n == _lib.MAX_LIST   # (wide: the longest list there is)
    flt = s.item_filter() if filtered else None
    try:
        E, summ = c.model.exposure(c.mat, nrcmds=n, cutoffs=cutoffs, users=users, filter=flt, fmarker=s.fm)
        assert np.array_equal(E, wantE)
        assert same_summary(summ, wantS)
        assert list_stats()["path"] == (4 if n > 128 else 2 if n > 64 else 1)
        # one cutoff by default: the lists' own length; no marker: no tail
        E1, s1 = c.model.exposure(c.mat, nrcmds=n, users=users, filter=flt)
        assert np.array_equal(E1[0], wantE[-1]) and s1[0]["tail_slots"] == 0 and s1[0]["slots"] == wantS[-1]["slots"]
    finally:
        if flt is not None:
            flt.close()


def test_long_slices_add_into_the_same_counters(setups, monkeypatch):
    s = setups("floats")
    c = s.c
    cutoffs = (7, 300)
    wantE, wantS, _ = s.want(cutoffs, None, False)
    monkeypatch.setenv("SLIM_TOPN_LONG_SLICE", "37")
    E, summ = c.model.exposure(c.mat, nrcmds=300, cutoffs=cutoffs, fmarker=s.fm)
    assert list_stats()["slices"] == (c.nusers + 36) // 37 and list_stats()["path"] == 4
    assert np.array_equal(E, wantE) and same_summary(summ, wantS)


def test_refusals(setups):
    s = setups("floats")
    c = s.c
    lib = c.lib
    met, nv = np.zeros(32), np.zeros(24, np.int32)
    E = np.full((8, c.ncols), 7, np.uint32)

    def refused(ev, flt, K, text):
        rc = lib.SLIMGPU_ModelEvaluateExposure(ev.handle, c.model.handle, flt, K, met, nv, E.ctypes.data, None)
        print(_lib.last_error())
        return rc == SLIM_ERROR_INPUT and text in _lib.last_error() and (E == 7).all() and not met.any()

    ranked = c.mat.evaluator(s.T, fmarker=s.fm, ranked=True)
    two = c.mat.evaluator(s.T, fmarker=s.fm, cutoffs=(5, 10))
    other = None
    try:
        assert refused(ranked, None, 1, "SLIMGPU_EvalSetCreateRanked")
        assert refused(two, None, 1, "list lengths")
        assert refused(two, None, 3, "list lengths")
        other = c.mat.item_filter(allowed=[1, 2, 3])
        narrow = C.c_void_p()
        items = np.array([1, 2], np.int32)
        assert lib.SLIMGPU_FilterCreate(c.ncols - 1, 2, items.ctypes.data, 0, 0, None, None, C.byref(narrow)) == SLIM_OK
        assert refused(two, narrow, 2, "SLIMGPU_ModelEvaluateExposure")
        lib.SLIMGPU_FilterFree(narrow)
        with pytest.raises(RuntimeError, match="SLIMGPU_MatrixPredictExposure"):
            c.model.exposure(c.mat, nrcmds=10, cutoffs=(5, 11))
        with pytest.raises(RuntimeError, match="SLIMGPU_MatrixPredictExposure"):
            c.model.exposure(c.mat, nrcmds=10, cutoffs=(5, 5))
        with pytest.raises(RuntimeError, match="SLIMGPU_MatrixPredictExposure"):
            c.model.exposure(c.mat, nrcmds=_lib.MAX_LIST + 1)
    finally:
        ranked.close()
        two.close()
        if other is not None:
            other.close()
