"""The exposure kernel (slim_amd/csrc/exposure.hip) through SLIMGPU_MatrixListExposure against SLIMGPU_ListExposure
on synthetic lists, bit for bit, counters and summaries -- and the host call against np.bincount, so that the two
cannot be wrong together.  The shapes are the smallest at which the kernel can go wrong: catalogue sizes around the
edges of any power-of-two window, shares of one to many workgroups, rows that are no multiple of the 16-byte loads,
every list holding the same head item, more band counters than LDS holds."""
import numpy as np
import pytest
import scipy.sparse as sp

from exposure_cases import call_device, call_host, random_lists, restate, same_summary
from slim_amd import _lib
from slim_amd.constants import SLIM_ERROR_INPUT, SLIM_OK
from slim_amd.engine import DeviceMatrix

pytestmark = pytest.mark.gpu

POW2 = [2 ** k + d for k in range(10, 18) for d in (-1, 0, 1)]


@pytest.fixture(scope="module")
def matrices():
    """A three-row staged matrix per catalogue size: the last item is rated, so the matrix has `ncols` columns."""
    made = {}

    def get(ncols):
        if ncols not in made:
            rng = np.random.default_rng(ncols)
            rows = [[0, ncols - 1], [ncols - 1], sorted(set(rng.integers(0, ncols, 40).tolist()))]
            ind = np.concatenate([np.unique(r) for r in rows]).astype(np.int32)
            ptr = np.cumsum([0] + [np.unique(r).size for r in rows])
            R = sp.csr_matrix((np.ones(ind.size, np.float32), ind, ptr), shape=(3, ncols))
            m = DeviceMatrix.from_scipy(R, binary=True)
            assert m.ncols == ncols
            made[ncols] = (m, np.bincount(ind, minlength=ncols).astype(np.uint32))
        return made[ncols]
    yield get
    for m, _ in made.values():
        m.close()


def edge_ids(ncols):
    """the first and the last id and the ids around every power of two inside the catalogue"""
    hot = {0, ncols - 1}
    k = 1
    while k < ncols:
        hot |= {i for i in (k - 1, k, k + 1) if 0 <= i < ncols}
        k *= 2
    return sorted(hot)


def check(lib, matrices, ncols, ids, counts, cutoffs, seed=0, numpy_too=True):
    mat, pop = matrices(ncols)
    fmarker = np.random.default_rng(seed).integers(0, 2, ncols).astype(np.int32)
    rc, E, summ = call_device(lib, mat, ids, counts, cutoffs, fmarker=fmarker)
    assert rc == SLIM_OK, _lib.last_error()
    rc, hE, hsumm = call_host(lib, ncols, ids, counts, cutoffs, pop=pop, fmarker=fmarker)
    assert rc == SLIM_OK, _lib.last_error()
    assert np.array_equal(E, hE)
    want = [s.as_dict() for s in hsumm]
    assert same_summary(summ, want)
    if numpy_too:
        nE, nsumm = restate(ncols, ids, counts, cutoffs, pop=pop, fmarker=fmarker)
        assert np.array_equal(E, nE) and same_summary(summ, nsumm)
    return E, want


@pytest.mark.parametrize("ncols", [1, 63, 64, 65] + POW2)
def test_window_edges(matrices, ncols):
    lib = _lib.load()
    rng = np.random.default_rng(ncols)
    ids, counts = random_lists(rng, ncols, 600, 10, outside=True, hot=edge_ids(ncols))
    E, want = check(lib, matrices, ncols, ids, counts, (3, 10), seed=ncols, numpy_too=ncols <= 4097)
    assert E[1, 0] > 0 and E[1, ncols - 1] > 0 and want[1]["outside"] > 0


def test_more_band_counters_than_lds_holds(matrices):
    lib = _lib.load()
    ncols = 100003
    rng = np.random.default_rng(3)
    ids, counts = random_lists(rng, ncols, 3000, 24, outside=True, hot=edge_ids(ncols))
    E, _ = check(lib, matrices, ncols, ids, counts, (1, 2, 3, 5, 8, 13, 21, 24), numpy_too=False)
    assert 8 * ncols * 4 > 160 * 1024 and E[7, ncols - 1] > 0
    assert np.array_equal(E[7], np.bincount(
        ids[(np.arange(24)[None, :] < counts[:, None]) & (ids >= 0) & (ids < ncols)], minlength=ncols))


@pytest.mark.parametrize("window", [1, 64, 1000])
def test_forced_windows(matrices, monkeypatch, window):
    """SLIM_EXPOSURE_WINDOW puts many window edges inside a small catalogue; the counts do not depend on it."""
    lib = _lib.load()
    monkeypatch.setenv("SLIM_EXPOSURE_WINDOW", str(window))
    ncols = 1025
    ids, counts = random_lists(np.random.default_rng(window), ncols, 500, 7, outside=True, hot=edge_ids(ncols))
    check(lib, matrices, ncols, ids, counts, (2, 7), seed=window)


@pytest.mark.parametrize("nlists", [0, 1, 63, 64, 65, 1000, 70001])
def test_shares(matrices, nlists):
    lib = _lib.load()
    ncols = 1500
    ids, counts = random_lists(np.random.default_rng(nlists), ncols, nlists, 10, outside=nlists > 0,
                               hot=edge_ids(ncols))
    check(lib, matrices, ncols, ids, counts, (1, 5, 10), seed=nlists)
    check(lib, matrices, ncols, ids, None, (10,), seed=nlists)          # counts == NULL


@pytest.mark.parametrize("N,nlists", [(1, 1000), (64, 1000), (128, 1000), (200, 1000), (4096, 40), (7, 1001), (3, 5)])
@pytest.mark.parametrize("fill", ["full", "zero", "random"])
def test_lengths(matrices, N, nlists, fill):
    lib = _lib.load()
    ncols = 4097
    rng = np.random.default_rng(N)
    ids, counts = random_lists(rng, ncols, nlists, N, hot=edge_ids(ncols))
    if fill == "full":
        counts[:] = N
    elif fill == "zero":
        counts[:] = 0
    cutoffs = sorted({1, (N + 1) // 2, N})
    E, want = check(lib, matrices, ncols, ids, counts, cutoffs, seed=N)
    assert (want[-1]["slots"] == 0) == (fill == "zero")


def test_contention(matrices):
    """70 001 lists that all hold item 0 at place 0 and the last item at their last place; 70 001 identical lists."""
    lib = _lib.load()
    ncols, n, N = 1500, 70001, 10
    rng = np.random.default_rng(11)
    ids = rng.integers(1, ncols - 1, (n, N)).astype(np.int32)
    ids[:, 0], ids[:, N - 1] = 0, ncols - 1
    cutoffs = (1, 4, 9, 10)
    E, _ = check(lib, matrices, ncols, ids, None, cutoffs)
    assert (E[:, 0] == n).all()
    assert E[:3, ncols - 1].tolist() == [0, 0, 0] and E[3, ncols - 1] == n
    same = np.tile(rng.permutation(ncols)[:N].astype(np.int32), (n, 1))
    E, want = check(lib, matrices, ncols, same, None, cutoffs)
    assert sorted(E[3][same[0]].tolist()) == [n] * N and want[3]["distinct"] == N


def test_bands(matrices):
    """K = 8 with the cutoffs (1, 2, 3, 5, 8, 13, 21, N): lists shorter than 3 leave the later bands empty."""
    lib = _lib.load()
    ncols, N = 1500, 30
    rng = np.random.default_rng(5)
    ids, counts = random_lists(rng, ncols, 2000, N, outside=True, hot=edge_ids(ncols))
    cutoffs = (1, 2, 3, 5, 8, 13, 21, N)
    check(lib, matrices, ncols, ids, counts, cutoffs)
    short = np.minimum(counts, 2).astype(np.int32)
    E, want = check(lib, matrices, ncols, ids, short, cutoffs)
    assert all(np.array_equal(E[k], E[1]) for k in range(2, 8)) and want[7]["slots"] == want[1]["slots"] > 0


def test_outputs_are_optional_and_refusals_write_nothing(matrices):
    lib = _lib.load()
    ncols = 1500
    mat, pop = matrices(ncols)
    ids, counts = random_lists(np.random.default_rng(1), ncols, 300, 10)
    rc, E, _ = call_device(lib, mat, ids, counts, (5, 10), want_summary=False)
    assert rc == SLIM_OK
    rc, _, summ = call_device(lib, mat, ids, counts, (5, 10), want_E=False)
    assert rc == SLIM_OK
    nE, nsumm = restate(ncols, ids, counts, (5, 10), pop=pop)
    assert np.array_equal(E, nE) and same_summary(summ, nsumm)
    for bad_cut, bad_counts in (((10, 5), counts), ((5, 11), counts), ((5, 10), np.full(300, 11, np.int32))):
        cut = np.ascontiguousarray(bad_cut, np.int32)
        E = np.full((2, ncols), 7, np.uint32)
        rc = lib.SLIMGPU_MatrixListExposure(mat.handle, None, 0, 300, 10, ids.ctypes.data, bad_counts.ctypes.data, 2,
                                            cut.ctypes.data, E.ctypes.data, None)
        assert rc == SLIM_ERROR_INPUT and _lib.last_error().startswith("SLIMGPU_MatrixListExposure: ")
        assert (E == 7).all()
    # the Python call
    E2, dicts = mat.list_exposure(ids, counts, (5, 10))
    assert np.array_equal(E2, nE) and same_summary(dicts, nsumm)
