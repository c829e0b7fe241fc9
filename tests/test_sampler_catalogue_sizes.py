"""The device samplers (include/slim_gpu_sample.h) across catalogue sizes: from one item to the documented bound
SLIMGPU_SAMPLE_MAX_NCOLS = 524 288, which the other tests only meet from the refused side.

Phase 2 of k_sample_weighted keeps the remaining mass per block of 1 024 items and lets lane l scan the block sums
[l * per, (l + 1) * per), per = ceil(blocks / 64).  The fixtures elsewhere have 1 500 or 6 000 items: per == 1, the
walk inside a lane never runs.  Beyond 65 536 items it does (per = 2 at 100 000, 8 at the bound), the dynamic LDS
passes 64 KB, and the uniform sampler's dense rule reaches its largest geometry: 64 KB of bitmap, 16 KB of ids, 64 KB
of sort records.

The yardstick is never the code under test: the numpy restatements of tests/sampled_cases.py and
tests/weighted_cases.py.  Everything is compared bit for bit.
"""
import ctypes as C

import numpy as np
import pytest

from crowd_cases import trace_launches
from sampled_cases import csr, negatives, rule, sampled_rows, set_rows
from slim_amd import _lib
from slim_amd.constants import SLIM_OK
from weighted_cases import device_sample_weighted, weighted_rows, weighted_user, weights

SMALL = (1, 31, 32, 33, 63, 64, 65, 1023, 1024, 1025)
LARGE = (65536, 65537, 100000, 131073, 524287, 524288)      # per = 1, 2, 2, 3, 8, 8
SEED = 11
NUSERS, NO_ROW, WIDE_ROW, HALF = 10, 3, 5, 9


def nnegs_of(ncols):
    return min(300, ncols)


_inputs = {}


def inputs(ncols, half=False):
    """(R, T): 10 users with histories of up to 8 items -- user 0 rates item 0 and the last item, so that the staged
    matrix has ncols columns --, a test row of one item, none for user NO_ROW, an id beyond the catalogue for user
    WIDE_ROW; half: the history of user HALF is every other item, ncols / 2 of them."""
    if (ncols, half) not in _inputs:
        rng = np.random.default_rng(1000 + ncols)
        hist = [np.unique([0, ncols - 1]).tolist()]
        hist += [np.unique(rng.integers(0, ncols, int(rng.integers(0, 9)))).tolist() for _ in range(1, NUSERS)]
        if half:
            hist[HALF] = list(range(1, ncols, 2))[:ncols // 2]
        test = [[int(rng.integers(0, ncols))] for _ in range(NUSERS)]
        test[NO_ROW], test[WIDE_ROW] = [], [ncols + 3]
        _inputs[(ncols, half)] = (csr(hist, ncols), csr(test, ncols + 8))
    return _inputs[(ncols, half)]


def weight_array(name, ncols):
    """cliff: tests/weighted_cases.py's (50 items carry nearly all the mass, up to 400 have weight 1, the rest 0),
    with weight 1 forced on item 0, on the last item and on the first item of the last block of 1 024.  zipf:
    1 000 000 // rank under a seeded permutation, a quarter of the items (100 at most) with weight 0."""
    if name == "cliff":
        w = weights("cliff", None, ncols).copy()
        w[[0, ncols - 1, (ncols - 1) >> 10 << 10]] = 1
        return w
    rng = np.random.default_rng(77)
    w = 1_000_000 // (1 + rng.permutation(ncols))
    w[rng.choice(ncols, min(100, ncols // 4), replace=False)] = 0
    return w.astype(np.uint32)


def weighted_want(name, ncols):
    R, T = inputs(ncols)
    return weighted_rows(("sizes", ncols, name), R, T.indptr.astype(np.int64), T.indices, ncols, nnegs_of(ncols), SEED,
                         weight_array(name, ncols))


def phase_two_blocks(ncols):
    """The blocks of 1 024 items in which phase 2 picked, over all users, under the cliff weights."""
    R, T = inputs(ncols)
    weighted_want("cliff", ncols)
    blocks, total = [], 0
    for u in range(NUSERS):
        if u == NO_ROW:
            continue
        neg, _, picks = weighted_user(("sizes", ncols, "cliff"), R, T.indptr.astype(np.int64), T.indices, ncols,
                                      nnegs_of(ncols), SEED, weight_array("cliff", ncols), u)
        blocks += (neg[neg.size - picks:] >> 10).tolist()
        total += picks
    return np.array(blocks), total


# ---- on the CPU: the fixture reaches what it is for ------------------------------------------------------------------
@pytest.mark.parametrize("ncols", LARGE)
def test_phase_two_picks_in_every_lanes_walk(ncols):
    """From the restatement's return values alone: phase 2 picked in block 0, in the last block and in a block of
    every residue block % per -- the first, every middle and the last block a lane walks."""
    nblk = (ncols + 1023) >> 10
    per = (nblk + 63) >> 6
    blocks, total = phase_two_blocks(ncols)
    print("%d items: %d blocks, per %d, %d picks of phase 2 in %d blocks" % (ncols, nblk, per, total,
                                                                            np.unique(blocks).size))
    assert per == {65536: 1, 65537: 2, 100000: 2, 131073: 3, 524287: 8, 524288: 8}[ncols]
    assert total > 200 * (NUSERS - 1)
    assert 0 in blocks and nblk - 1 in blocks
    assert set((blocks % per).tolist()) == set(range(per))


def test_small_catalogues_give_short_and_full_rows():
    lens = {}
    for ncols in SMALL:
        for name in ("cliff", "zipf"):
            ptr, _ = weighted_want(name, ncols)
            lens[(ncols, name)] = np.diff(ptr)
    # at up to 33 items nobody gets nnegs negatives; at 1 023 and more, under zipf, everybody with a test row does
    assert all((lens[(n, w)] < nnegs_of(n) + 1).all() for n in (1, 31, 32, 33) for w in ("cliff", "zipf"))
    assert all((np.delete(lens[(n, "zipf")], NO_ROW) == 301).all() for n in (1023, 1024, 1025))
    assert all(lens[k][NO_ROW] == 0 for k in lens)


# ---- on the device ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def staged():
    """The staged matrix of a size (and of its variant with the half-catalogue history), made once."""
    from slim_amd.engine import DeviceMatrix
    made = {}

    def get(ncols, half=False):
        if (ncols, half) not in made:
            m = DeviceMatrix.from_scipy(inputs(ncols, half)[0], binary=True)
            assert m.ncols == ncols
            made[(ncols, half)] = m
        return made[(ncols, half)]
    yield get
    for m in made.values():
        m.close()


def sample(lib, mat, T, ncols, nnegs, w, capfd):
    """One device call under SLIM_GPU_TRACE: ((indptr, indices, ncols), the trace line's tail)."""
    ev = mat.evaluator(T, fmarker=np.zeros(ncols + 8, np.int32), cutoffs=(1,))
    try:
        def call():
            if w is not None:
                return device_sample_weighted(lib, ev, nnegs, SEED, w)
            h = C.c_void_p()
            return lib.SLIMGPU_EvalSetSampleCandidates(ev.handle, nnegs, SEED, C.byref(h)), h
        (rc, cs), launches = trace_launches(capfd, call)
        assert rc == SLIM_OK, _lib.last_error()
        got = set_rows(lib, cs)
        lib.SLIMGPU_CandSetFree(cs)
    finally:
        ev.close()
    kernel = "k_sample_weighted" if w is not None else "k_sample_negatives"
    lines = [l for l in launches if l[0] == kernel]
    assert len(lines) == 1 and lines[0][1] == NUSERS, launches
    return got, lines[0][3]


def lds_bytes(rest):
    return int(rest.split(" bytes of LDS")[0].split()[-1])


@pytest.mark.gpu
@pytest.mark.parametrize("ncols", SMALL + LARGE)
def test_weighted_rows_at_every_size(staged, ncols, monkeypatch, capfd):
    monkeypatch.setenv("SLIM_GPU_TRACE", "1")
    lib = _lib.load()
    T = inputs(ncols)[1]
    per = (((ncols + 1023) >> 10) + 63) >> 6
    for name in ("cliff", "zipf"):
        want = weighted_want(name, ncols)
        got, rest = sample(lib, staged(ncols), T, ncols, nnegs_of(ncols), weight_array(name, ncols), capfd)
        print("%d items, %s:%s" % (ncols, name, rest))
        assert rest.endswith("per %d" % per)
        assert (lds_bytes(rest) > 64 * 1024) == (ncols >= 524287)
        assert got[2] == ncols
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), (ncols, name)


@pytest.mark.gpu
@pytest.mark.parametrize("ncols", SMALL + LARGE)
def test_uniform_rows_at_every_size(staged, ncols, monkeypatch, capfd):
    """nnegs = 5: from 31 items on every user falls under the sparse rule."""
    monkeypatch.setenv("SLIM_GPU_TRACE", "1")
    lib = _lib.load()
    R, T = inputs(ncols)
    tptr = T.indptr.astype(np.int64)
    if ncols >= 31:
        assert all(rule(np.diff(R.indptr)[u] + 1, 5, ncols) == "sparse" for u in range(NUSERS))
    want = sampled_rows(R, tptr, T.indices, ncols, 5, SEED)
    got, rest = sample(lib, staged(ncols), T, ncols, 5, None, capfd)
    print("%d items, uniform:%s" % (ncols, rest))
    assert got[2] == ncols and np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), ncols


@pytest.mark.gpu
@pytest.mark.parametrize("ncols,nnegs", [(65537, 300), (524288, 300), (524288, 4095)])
def test_the_dense_rule_on_large_catalogues(staged, ncols, nnegs, monkeypatch, capfd):
    """One user whose history is half the catalogue is dense, the others are sparse; at 524 288 items and 4 095
    negatives the launch holds 64 KB of bitmap, 16 KB of ids and 64 KB of sort records."""
    monkeypatch.setenv("SLIM_GPU_TRACE", "1")
    lib = _lib.load()
    R, T = inputs(ncols, half=True)
    tptr = T.indptr.astype(np.int64)
    both = [np.concatenate((R.indices[R.indptr[u]:R.indptr[u + 1]], T.indices[tptr[u]:tptr[u + 1]])) for u in range(NUSERS)]
    E = [np.unique(b[b < ncols]).size for b in both]
    assert [rule(e, nnegs, ncols) for e in E] == ["sparse"] * HALF + ["dense"]
    want = sampled_rows(R, tptr, T.indices, ncols, nnegs, SEED)
    assert np.diff(want[0]).tolist() == [nnegs + 1 if u != NO_ROW else 0 for u in range(NUSERS)]
    got, rest = sample(lib, staged(ncols, True), T, ncols, nnegs, None, capfd)
    print("%d items, nnegs %d, uniform with a dense user:%s" % (ncols, nnegs, rest))
    assert rest.endswith(", sort records")
    if nnegs == 4095:
        assert lds_bytes(rest) == 64 * 1024 + 16 * 1024 + 64 * 1024
    assert got[2] == ncols and np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), (ncols, nnegs)
    # the dense user's row is the restatement's own dense rule
    X = np.union1d(R.indices[R.indptr[HALF]:R.indptr[HALF + 1]], T.indices[tptr[HALF]:tptr[HALF + 1]])
    assert np.array_equal(got[1][got[0][HALF]:got[0][HALF] + nnegs], negatives(SEED, HALF, X, nnegs, ncols))
