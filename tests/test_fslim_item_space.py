"""FSLIM in item space (KERNEL_GRAM_FSLIM, slim_amd/csrc/cd_fslim_gram.hpp): the neighbour lists are
read off rows of G = R^T R and the descent runs on the neighbourhood's block of G, in the tile
kernel's visiting order -- so the oracle's tile walk (slim_oracle.learn_cd_tile with nnbrs) checks it
visit for visit, with the bars the tile FSLIM kernel and the item-space kernel already meet:
maxdiff 2e-5 (the walk itself reproduces the oracle to <= 1e-6 on these matrices), the same
neighbour counts, the same sweep counts on >= 98 % of the columns."""
import os
import re

import numpy as np
import pytest
import scipy.sparse as sp

import slim_oracle as O
from slim_amd import SLIM, SLIMatrix, _lib
from slim_amd.engine import KERNEL_GRAM, KERNEL_TILE, DeviceMatrix

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNEL_GRAM_FSLIM = 6   # (pinned here; test_kernel_id_is_six holds the package and the header to it)

gpu = pytest.mark.gpu


def maxdiff(a, b):
    d = abs(sp.csc_matrix(a) - sp.csc_matrix(b))
    return float(d.max()) if d.nnz else 0.0


def pattern_diff(a, b):
    pa = sp.csc_matrix(a).copy()
    pb = sp.csc_matrix(b).copy()
    pa.data[:] = 1
    pb.data[:] = 1
    return int(abs(pa - pb).sum())


def same_bits(a, b):
    a, b = sp.csc_matrix(a), sp.csc_matrix(b)
    return a.nnz == b.nnz and maxdiff(a, b) == 0.0


def _r11():
    """3000 users x 500 items, binary, 3 % dense, columns 17 and 250 empty: with dotp nearly every
    column has a tie across the cut, no column has more than 489 co-rated columns, two have none."""
    rng = np.random.default_rng(11)
    R = sp.random(3000, 500, density=0.03, format="lil", random_state=rng, dtype=np.float32)
    R[:, 17] = 0
    R[:, 250] = 0
    R = sp.csr_matrix(R)
    R.eliminate_zeros()
    R.data[:] = 1.0
    R = sp.csr_matrix((R.data, R.indices, R.indptr), shape=(3000, 500))
    R.sort_indices()
    return R


def _random_ratings(nu, ni, density, seed):
    rng = np.random.default_rng(seed)
    R = sp.random(nu, ni, density=density, format="csr", random_state=rng, dtype=np.float32)
    R.data = rng.integers(1, 6, R.nnz).astype(np.float32)
    R.sort_indices()
    return R


@pytest.fixture(scope="module")
def mats(ml100k, automotive):
    return {"r11": _r11(), "ml100k": ml100k[0], "automotive": sp.csr_matrix(automotive[0])}


_oracle_cache = {}


def oracle(mats, name, nnbrs, simtype, **kw):
    """learn_cd_tile's (W, column stats, error, objective), computed once per case."""
    key = (name, nnbrs, simtype, tuple(sorted(kw.items())))
    if key not in _oracle_cache:
        args = dict(tileP=32, maxniters=200, seed=2, nthreads=8, nnbrs=nnbrs, simtype=simtype, return_stats=True)
        args.update(kw)
        _oracle_cache[key] = O.learn_cd_tile(mats[name], **args)
    return _oracle_cache[key]


@pytest.fixture(scope="module")
def devs(mats):
    """One handle per matrix for the whole module: G is built by the first kernel-6 solve of each."""
    made = {}

    def get(name):
        if name not in made:
            made[name] = DeviceMatrix.from_scipy(mats[name], binary=(name == "r11"))
        return made[name]
    yield get
    for m in made.values():
        m.close()


# ---- CPU ---------------------------------------------------------------------------------------
def test_kernel_id_is_six():
    from slim_amd import engine
    assert engine.KERNEL_GRAM_FSLIM == KERNEL_GRAM_FSLIM == 6
    text = open(os.path.join(ROOT, "include", "slim_gpu.h")).read()
    assert int(re.search(r"SLIMGPU_KERNEL_GRAM_FSLIM\s*=\s*(\d+)", text).group(1)) == 6


def test_fixture_has_ties_at_the_cut_and_empty_neighbourhoods(mats):
    R = mats["r11"]
    assert R.shape == (3000, 500) and R.getnnz(axis=0)[499] > 0
    assert R.getnnz(axis=0)[17] == 0 and R.getnnz(axis=0)[250] == 0
    G = (R.T @ R).toarray()
    ties = 0
    for it in range(500):
        a = G[it].copy()
        a[it] = 0
        s = np.sort(a[a > 0])[::-1]
        ties += int(len(s) > 64 and s[63] == s[64])
    assert ties >= 400            # 489 measured
    for nnbrs in (64, 600):
        nac = oracle(mats, "r11", nnbrs, 2)[1]["nacols"][:500]
        assert nac.min() == 0 and nac.max() == min(nnbrs, 489)


# ---- 1. against the oracle's tile walk ---------------------------------------------------------
CASES = [("r11", n) for n in (1, 64, 65, 129, 600)] + [("ml100k", 40), ("ml100k", 5000), ("automotive", 10)]


@gpu
@pytest.mark.parametrize("simtype", [0, 1, 2])
@pytest.mark.parametrize("name,nnbrs", CASES)
def test_matches_the_oracle_tile_walk(mats, devs, name, nnbrs, simtype):
    """Both sides of every switch: 64 / 65 neighbours (one wavefront step, 16 KB / 64 KB block),
    128 / 129 (block in LDS / gathered), 1, and more neighbours than candidates (600; 5000)."""
    m = devs(name)
    W, st = m.learn(kernel=KERNEL_GRAM_FSLIM, seed=2, nnbrs=nnbrs, simtype=simtype, niters=200)
    cs = m.column_stats()
    Wo, so, err_o, obj_o = oracle(mats, name, nnbrs, simtype)
    n = mats[name].shape[1]
    sweeps_equal = float((cs.sweeps[:n] == so["sweeps"][:n]).mean())
    print("%s nnbrs %d simtype %d: maxdiff %.3e pattern %d sweeps equal %.4f D %d/%d U %d/%d obj %.6e/%.6e"
          % (name, nnbrs, simtype, maxdiff(W, Wo), pattern_diff(W, Wo), sweeps_equal, cs.D.sum(), so["D"].sum(),
             cs.U.sum(), so["U"].sum(), st["objval"], obj_o))
    assert st["kernel"] == 6
    assert np.array_equal(cs.nacols[:n], so["nacols"][:n])
    assert maxdiff(W, Wo) <= 2e-5 and pattern_diff(W, Wo) <= 4
    assert sweeps_equal >= 0.98
    assert abs(cs.D.sum() - so["D"].sum()) <= 0.01 * so["D"].sum()
    assert abs(cs.U.sum() - so["U"].sum()) <= 0.01 * so["U"].sum()
    assert abs(st["objval"] - obj_o) <= 1e-4 * obj_o


# ---- 2. the two forms of the solver ------------------------------------------------------------
@gpu
@pytest.mark.parametrize("nnbrs", [64, 129])
def test_gathered_form_equals_the_default_form_bit_for_bit(mats, devs, monkeypatch, nnbrs):
    m = devs("r11")
    W, _ = m.learn(kernel=KERNEL_GRAM_FSLIM, seed=2, nnbrs=nnbrs, simtype=0, niters=200)
    monkeypatch.setenv("SLIM_GPU_FSLIM_BLOCK", "0")
    Wg, st = m.learn(kernel=KERNEL_GRAM_FSLIM, seed=2, nnbrs=nnbrs, simtype=0, niters=200)
    assert st["kernel"] == 6 and W.nnz > 0
    assert same_bits(W, Wg)


@gpu
def test_slices_of_the_work_list_change_nothing(mats, devs, monkeypatch):
    """The lists of a long work list go through in slices of whole tiles: forced to 3 tiles here."""
    m = devs("r11")
    W, _ = m.learn(kernel=KERNEL_GRAM_FSLIM, seed=2, nnbrs=65, simtype=1, niters=200)
    monkeypatch.setenv("SLIM_GPU_FSLIM_SLICE_TILES", "3")
    Ws, _ = m.learn(kernel=KERNEL_GRAM_FSLIM, seed=2, nnbrs=65, simtype=1, niters=200)
    assert W.nnz > 0 and same_bits(W, Ws)


# ---- 3. against the tile FSLIM kernel on the large-matrix shape --------------------------------
@gpu
def test_matches_the_tile_fslim_kernel_and_builds_g_once():
    R = _random_ratings(40000, 3000, 0.004, 5)   # work vectors beyond 64 KB: AUTO takes the tile path
    m = DeviceMatrix.from_scipy(R)
    W, st = m.learn(kernel=KERNEL_GRAM_FSLIM, seed=2, nnbrs=20, l2r=0.5)
    cs = m.column_stats()
    assert st["kernel"] == 6 and st["gram_build_ms"] > 0
    W2, st2 = m.learn(kernel=KERNEL_GRAM_FSLIM, seed=2, nnbrs=20, l2r=0.5)
    assert st2["gram_build_ms"] == 0 and same_bits(W, W2)
    Wt, stt = m.learn(kernel=KERNEL_TILE, cluster=1, seed=2, nnbrs=20, l2r=0.5)
    ct = m.column_stats()
    assert stt["kernel"] == KERNEL_TILE
    print("maxdiff %.3e, sweeps equal %.4f" % (maxdiff(W, Wt), (cs.sweeps == ct.sweeps).mean()))
    assert np.array_equal(cs.nacols, ct.nacols) and cs.nacols.max() == 20
    assert maxdiff(W, Wt) <= 5e-5
    assert (cs.sweeps == ct.sweeps).mean() >= 0.98
    m.close()


# ---- 4. work-list shapes -----------------------------------------------------------------------
@gpu
def test_column_ranges_sets_and_shards(mats, devs):
    """A sub-range has its own tiles, hence its own order: its columns are compared to the oracle's full
    model at a tolerance where the order no longer shows (optTol 1e-12), as the item-space kernel's
    ranges are.  Shards keep the tiles of the full list: bit for bit."""
    m = devs("r11")
    kw = dict(kernel=KERNEL_GRAM_FSLIM, seed=2, nnbrs=64, simtype=0, optTol=1e-12, niters=100000)
    Wo = oracle(mats, "r11", 64, 0, optTol=1e-12, maxniters=100000)[0]
    for b, e in ((0, 37), (37, 38), (38, 200)):
        Wp, _ = m.learn(col_begin=b, col_end=e, **kw)
        assert Wp[:, b:e].nnz > 0 and Wp[:, :b].nnz == 0 and Wp[:, e:].nnz == 0
        assert maxdiff(Wp[:, b:e], Wo[:, b:e]) <= 2e-5
    cols = np.array([3, 499, 250, 100, 17, 41, 42, 43, 300], np.int32)
    Wc, _ = m.learn(columns=cols, **kw)
    rest = np.setdiff1d(np.arange(500), cols)
    assert Wc[:, rest].nnz == 0 and maxdiff(Wc[:, cols], Wo[:, cols]) <= 2e-5
    W, _ = m.learn(kernel=KERNEL_GRAM_FSLIM, seed=2, nnbrs=64, simtype=0, niters=200)
    halves = [m.learn(kernel=KERNEL_GRAM_FSLIM, seed=2, nnbrs=64, simtype=0, niters=200, shard=(k, 2))[0]
              for k in (0, 1)]
    assert halves[0].nnz > 0 and halves[1].nnz > 0
    assert same_bits(halves[0] + halves[1], W)


# ---- 5. lifetime of the float G ----------------------------------------------------------------
@gpu
def test_float_g_is_rebuilt_after_the_planes_took_over(mats, monkeypatch):
    monkeypatch.setenv("SLIM_GPU_DROP_G_MIN_GB", "0")   # a small G is dropped too once it is packed
    R = mats["r11"]
    m = DeviceMatrix.from_scipy(R, binary=True)
    kw = dict(kernel=KERNEL_GRAM_FSLIM, seed=2, nnbrs=64, simtype=0, niters=200)
    W1, s1 = m.learn(**kw)
    assert s1["gram_build_ms"] > 0
    Wg, sg = m.learn(kernel=KERNEL_GRAM, seed=2)       # packs the planes, drops the floats
    assert sg["kernel"] == KERNEL_GRAM
    with pytest.raises(RuntimeError):
        m.gram_view()                                  # the floats are gone
    W2, s2 = m.learn(**kw)
    assert s2["gram_build_ms"] > 0 and same_bits(W1, W2)
    m.close()
    fresh = DeviceMatrix.from_scipy(R, binary=True)
    Wf, _ = fresh.learn(kernel=KERNEL_GRAM, seed=2)
    assert same_bits(Wg, Wf)
    fresh.close()


# ---- 6. boundary behaviour ---------------------------------------------------------------------
@gpu
def test_refusals(mats, devs):
    m = devs("r11")
    with pytest.raises(RuntimeError, match="nnbrs > 0"):
        m.learn(kernel=KERNEL_GRAM_FSLIM, nnbrs=0)
    Rn = mats["ml100k"].copy()
    Rn.data[5] = -1.0
    mn = DeviceMatrix.from_scipy(Rn)
    with pytest.raises(RuntimeError, match="ratings > 0"):
        mn.learn(kernel=KERNEL_GRAM_FSLIM, nnbrs=10)
    assert "co-rat" in _lib.last_error()
    mn.close()
    rng = np.random.default_rng(3)
    Rw = sp.random(2000, 6000, density=0.002, format="lil", random_state=rng, dtype=np.float32)
    Rw[0, 5999] = 1.0
    Rw = sp.csr_matrix(Rw)
    Rw.data[:] = 1.0
    mw = DeviceMatrix.from_scipy(Rw, binary=True)
    assert mw.ncols == 6000
    with pytest.raises(RuntimeError, match="4096"):
        mw.learn(kernel=KERNEL_GRAM_FSLIM, nnbrs=5000)
    mw.close()


@gpu
def test_warm_start_is_ignored_and_resident_models_work(mats, devs):
    m = devs("automotive")
    kw = dict(kernel=KERNEL_GRAM_FSLIM, seed=2, nnbrs=10, simtype=1, niters=100)
    W, _ = m.learn(**kw)
    Wother, _ = m.learn(kernel=KERNEL_GRAM_FSLIM, seed=5, nnbrs=30, simtype=0, l1r=0.1, niters=100)
    Ww, _ = m.learn(imodel=Wother, **kw)
    assert W.nnz > 0 and same_bits(W, Ww)
    rm, st = m.learn_resident(**kw)
    assert st["kernel"] == 6
    assert same_bits(rm.fetch(), W)
    rm.free()


@gpu
def test_python_api_reaches_the_kernel(automotive_triplets, devs):
    trn, _ = automotive_triplets
    model = SLIM()
    model.train({"algo": "cd", "nthreads": 1, "l1r": 1.0, "l2r": 1.0, "optTol": 1e-7, "niters": 100,
                 "nnbrs": 10, "simtype": "jac", "gpu_kernel": 6, "gpu_seed": 2}, SLIMatrix(trn))
    W, st = devs("automotive").learn(kernel=KERNEL_GRAM_FSLIM, seed=2, nnbrs=10, simtype=1, niters=100,
                                     l1r=1.0, l2r=1.0, optTol=1e-7)
    assert st["kernel"] == 6 and same_bits(model.to_csr(), W)
