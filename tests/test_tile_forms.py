"""Every workgroup form of the residual (tile) kernel against the oracle's tile walk.

finish_path() (engine.hip) picks cd_tile_kernel out of a grid of instantiations (tile_inst.hpp):
tile width P in {32, 16} x NW in {16, 8} wavefronts per workgroup x valued / binary x the forms
cold (FOLD = 0, P = 32 only), rowfold (FOLD = 2, P = 32 only), colfold (the base instantiation,
FOLD = 1: every P = 16 solve, P = 32 warm starts under SLIM_GPU_FOLD=col, and everything at
SLIM_GPU_TRACE>=2, where it is the profiled one) and fslim (P = 32 only).  NW is chosen from the
number of tiles (8 from 2 x CUs tiles up), so small matrices never see the 8-wavefront half unless
SLIM_GPU_TILE_NW forces it, which is what these tests do.  NW changes the workgroup chunk
(64 NW nnz), the problems per wavefront (P / NW), the stride of every `i += NW` loop and the shape
of the cross-wavefront reductions (cd_tile.hpp).

Reference: O.learn_cd_tile, the fp64 restatement walking the tile's visiting order, with the same
tileP, seed, penalties, previous model, neighbour count and similarity.  The checks are the
suite's own for the same order, fp32 against fp64, on random ratings (test_gpu_parity.py):
max |dW| <= 5e-5, the same active-set sizes, >= 98 % of the sweep counts, the objective to 1e-4
relative -- and the engine's `[trace] tile kernel:` line proves which instantiation ran.  Nothing
is asserted between the NW = 8 and the NW = 16 model of one case: their cross-wavefront sums add
in different orders.

Only test_automatic_wavefront_count runs at optTol=1e-10 (see there); everything else runs at the
default optTol of 1e-7 (the item-count edges' range sums at 1e-12, as test_tile_kernel_ml100k does)."""
import functools
import re

import numpy as np
import pytest
import scipy.sparse as sp

import slim_oracle as O
from slim_amd.engine import KERNEL_TILE, KERNEL_TILE16, DeviceMatrix

TRACE = re.compile(r"\[trace\] tile kernel: P (\d+), (\d+) wavefronts, form (\w+), (valued|binary)(, profiled)?")

# the edges of both workgroup chunks: 64 NW = 512 (NW = 8) and 1024 (NW = 16) nnz, one wavefront
# (64), and slices of 2 and 3 chunks
LADDER = (1, 2, 63, 64, 65, 511, 512, 513, 1023, 1024, 1025, 1537, 2049)
LADDER_USERS = 4096
# penalties of the ladder solves, chosen on the CPU (test_fixtures_do_their_job holds the conditions)
L1R, L2R = 1.0, 0.5
FIRST = dict(l1r=3.0, l2r=1.0)      # the solve whose model warm-starts the next one
EDGE_COUNTS = (1, 7, 8, 9, 15, 16, 17, 31, 32, 33, 65)
GEOMS = (dict(cluster=1, heavy_tiles=0), dict(cluster=4, heavy_tiles=0),
         dict(cluster=2, heavy_tiles=1, heavy_cluster=4))
KERNEL = {32: KERNEL_TILE, 16: KERNEL_TILE16}
PNW = [(32, 8), (32, 16), (16, 8), (16, 16)]


def maxdiff(a, b):
    d = abs(sp.csc_matrix(a) - sp.csc_matrix(b))
    return float(d.max()) if d.nnz else 0.0


def pattern_diff(a, b):
    pa = sp.csc_matrix(a).copy()
    pb = sp.csc_matrix(b).copy()
    pa.data[:] = 1
    pb.data[:] = 1
    return int(abs(pa - pb).sum())


# ---- fixtures (seeded; the oracle's results are computed once and shared, never written to) ------
@functools.lru_cache(maxsize=None)
def ladder(nitems=96, binary=False):
    """LADDER_USERS x nitems, column j of LADDER[j % 13] users drawn without replacement, ratings
    1-5 (binary: all 1)."""
    rng = np.random.default_rng(20 + nitems)
    rows, cols = [], []
    for j in range(nitems):
        n = LADDER[j % len(LADDER)]
        rows.append(rng.choice(LADDER_USERS, n, replace=False))
        cols.append(np.full(n, j))
    rows, cols = np.concatenate(rows), np.concatenate(cols)
    data = rng.integers(1, 6, rows.size).astype(np.float32)
    R = sp.csr_matrix((data, (rows, cols)), shape=(LADDER_USERS, nitems))
    R.sort_indices()
    if binary:
        R.data[:] = 1.0
    return R


def random_ratings(nu, ni, density, seed):
    """Random ratings 1-5 with no empty column (the oracle sizes the model by the last rated item)."""
    rng = np.random.default_rng(seed)
    R = sp.random(nu, ni, density=density, format="lil", random_state=rng, dtype=np.float32)
    for j in np.flatnonzero(np.diff(R.tocsc().indptr) == 0):
        R[rng.integers(nu), j] = 1.0
    R = sp.csr_matrix(R)
    R.data = rng.integers(1, 6, R.nnz).astype(np.float32)
    R.sort_indices()
    return R


@functools.lru_cache(maxsize=None)
def _edge_matrix():
    return random_ratings(3000, 65, 0.05, 31)


def edges(n=65):
    """The first n item columns of a 3000 x 65 random-ratings matrix (~150 ratings per column)."""
    return sp.csr_matrix(_edge_matrix()[:, :n])


@functools.lru_cache(maxsize=None)
def wide(nitems):
    """~3000 users x nitems, ~6 ratings per column: many tiles, little work in each."""
    return random_ratings(3000, nitems, 0.002, 41)


@functools.lru_cache(maxsize=None)
def ladder_oracle(P, binary=False, warm=False, nitems=96, nnbrs=0, simtype=0, maxniters=10000):
    """(W, column stats, objective) of the oracle's tile walk over the ladder; warm: from the
    oracle's own model at the penalties FIRST."""
    R = ladder(nitems, binary)
    kw = dict(tileP=P, seed=3, nthreads=8, binary=binary)
    imodel = O.learn_cd_tile(R, **FIRST, **kw) if warm else None
    W, so, _, obj = O.learn_cd_tile(R, l1r=L1R, l2r=L2R, imodel=imodel, nnbrs=nnbrs, simtype=simtype,
                                    maxniters=maxniters, return_stats=True, **kw)
    return W, so, obj


@functools.lru_cache(maxsize=None)
def ladder_oracle_first(P, binary=False, nitems=96):
    return O.learn_cd_tile(ladder(nitems, binary), tileP=P, seed=3, nthreads=8, binary=binary, **FIRST)


def test_fixtures_do_their_job():
    """The ladder holds every slice length, and at the chosen penalties its solves are not trivial:
    a model of >= 500 coefficients, most columns sweeping more than once, and a warm start that
    saves sweeps.  The edge matrix has no empty column at any cut."""
    for nitems in (96, 256):
        lengths = np.diff(ladder(nitems).tocsc().indptr)
        assert set(lengths) == set(LADDER)
        assert ladder(nitems).data.min() == 1 and ladder(nitems).data.max() == 5
        assert np.all(ladder(nitems, True).data == 1)
    for P in (32, 16):
        for binary in (False, True):
            W, so, _ = ladder_oracle(P, binary)
            assert W.nnz >= 500
            assert (so["sweeps"] > 1).mean() >= 0.5
            Ww, sw, _ = ladder_oracle(P, binary, warm=True)
            assert Ww.nnz >= 500
            assert sw["sweeps"].sum() < so["sweeps"].sum()
            assert ladder_oracle_first(P, binary).nnz >= 200   # something to fold
    assert np.diff(edges().tocsc().indptr).min() >= 1
    W, so, _, _ = O.learn_cd_tile(edges(), tileP=32, seed=3, nthreads=8, l1r=L1R, l2r=L2R, return_stats=True)
    assert W.nnz >= 500 and (so["sweeps"] > 1).mean() >= 0.5


# ---- the GPU side --------------------------------------------------------------------------------
@pytest.fixture(autouse=True)
def _env(monkeypatch):
    monkeypatch.setenv("SLIM_GPU_TRACE", "1")
    for k in ("SLIM_GPU_TILE_NW", "SLIM_GPU_FOLD", "SLIM_GPU_HI_PREFETCH", "SLIM_GPU_XCD", "SLIM_GPU_HEAVY"):
        monkeypatch.delenv(k, raising=False)


def solve(m, capfd, expect, **kw):
    """One solve whose trace line must name the instantiation `expect` = (P, NW, form, valued |
    binary, profiled) -> (W, stats, column stats)."""
    capfd.readouterr()
    W, st = m.learn(seed=3, kernel=KERNEL[expect[0]], **kw)
    cs = m.column_stats()
    got = [(int(p), int(nw), f, v, bool(pr)) for p, nw, f, v, pr in TRACE.findall(capfd.readouterr().err)]
    assert got == [tuple(expect)], got
    return W, st, cs


@pytest.fixture
def check(record_property):
    """The suite's checks of a same-order solve against the fp64 walk, on the solved columns; the
    figures go into the test's report (record_property: --junitxml shows them)."""
    def compare(tag, W, st, cs, Wo, so, obj_o, cols=slice(None), tol=5e-5):
        d = maxdiff(W[:, cols], Wo[:, cols])
        same = (cs.sweeps[cols] == so["sweeps"][cols]).mean()
        record_property(tag, "maxdiff %.3e, sweeps equal %.4f, objval rel %.2e"
                        % (d, same, abs(st["objval"] - obj_o) / obj_o))
        assert d <= tol
        assert np.array_equal(cs.nacols[cols], so["nacols"][cols])
        assert same >= 0.98
        assert abs(st["objval"] - obj_o) <= 1e-4 * obj_o
    return compare


def kind(binary):
    return "binary" if binary else "valued"


def cold_form(P):
    return "cold" if P == 32 else "colfold"     # 16-wide tiles have the base instantiation only


@pytest.mark.gpu
@pytest.mark.timeout(120, method="thread")
@pytest.mark.parametrize("binary", [False, True])
@pytest.mark.parametrize("P,NW", PNW)
def test_cold_on_the_ladder(P, NW, binary, monkeypatch, capfd, check):
    """Cold solves: no clusters, clusters of 4, a heavy phase (clusters of 4, then of 2)."""
    monkeypatch.setenv("SLIM_GPU_TILE_NW", str(NW))
    m = DeviceMatrix.from_scipy(ladder(96, binary), binary=binary)
    for geom in GEOMS:
        W, st, cs = solve(m, capfd, (P, NW, cold_form(P), kind(binary), False), l1r=L1R, l2r=L2R, **geom)
        check("P%d NW%d %s %s %s" % (P, NW, cold_form(P), kind(binary), geom), W, st, cs,
              *ladder_oracle(P, binary))
    m.close()


@pytest.mark.gpu
@pytest.mark.timeout(120, method="thread")
@pytest.mark.parametrize("binary", [False, True])
@pytest.mark.parametrize("NW", [8, 16])
@pytest.mark.parametrize("P,fold", [(32, "row"), (32, "col"), (16, "col")])
def test_warm_on_the_ladder(P, fold, NW, binary, monkeypatch, capfd, check):
    """Warm starts, visit for visit: the model of a solve at l1r = 3 folded into the residual row
    by row or column by column (16-wide tiles: always by column), then the sweeps at smaller
    penalties, in the three geometries."""
    monkeypatch.setenv("SLIM_GPU_TILE_NW", str(NW))
    monkeypatch.setenv("SLIM_GPU_FOLD", fold)
    form = "rowfold" if fold == "row" else "colfold"
    m = DeviceMatrix.from_scipy(ladder(96, binary), binary=binary)
    for geom in GEOMS:
        first, _, _ = solve(m, capfd, (P, NW, cold_form(P), kind(binary), False), **FIRST, **geom)
        assert maxdiff(first, ladder_oracle_first(P, binary)) <= 5e-5
        W, st, cs = solve(m, capfd, (P, NW, form, kind(binary), False), l1r=L1R, l2r=L2R, imodel=first, **geom)
        check("P%d NW%d %s %s %s" % (P, NW, form, kind(binary), geom), W, st, cs,
              *ladder_oracle(P, binary, warm=True))
    m.close()


@pytest.mark.gpu
@pytest.mark.parametrize("NW", [8, 16])
@pytest.mark.parametrize("P,fold", [(32, "row"), (32, "col"), (16, "col")])
def test_warm_from_negative_entries(P, fold, NW, monkeypatch, capfd, check):
    """estimate.c:456-464: a negative entry of the previous model starts at 0 -- the warm start
    from a model holding some equals, bit for bit, the one from that model without them, and both
    match the oracle started from the model as given."""
    monkeypatch.setenv("SLIM_GPU_TILE_NW", str(NW))
    monkeypatch.setenv("SLIM_GPU_FOLD", fold)
    form = "rowfold" if fold == "row" else "colfold"
    first = sp.csc_matrix(ladder_oracle_first(P))
    bad = first.copy()
    bad.data[::7] = -0.25                           # every 7th coefficient becomes negative
    dropped = bad.copy()
    dropped.data[dropped.data < 0] = 0.0
    dropped.eliminate_zeros()
    assert 0 < dropped.nnz < bad.nnz
    m = DeviceMatrix.from_scipy(ladder())
    Wb, st, cs = solve(m, capfd, (P, NW, form, "valued", False), l1r=L1R, l2r=L2R, imodel=bad)
    Wd, _, csd = solve(m, capfd, (P, NW, form, "valued", False), l1r=L1R, l2r=L2R, imodel=dropped)
    assert maxdiff(Wb, Wd) == 0.0 and np.array_equal(cs.sweeps, csd.sweeps)
    Wo, so, _, obj_o = O.learn_cd_tile(ladder(), tileP=P, seed=3, nthreads=8, l1r=L1R, l2r=L2R, imodel=bad,
                                       return_stats=True)
    check("P%d NW%d %s valued, negative entries" % (P, NW, form), Wb, st, cs, Wo, so, obj_o)
    m.close()


@pytest.mark.gpu
@pytest.mark.timeout(120, method="thread")
@pytest.mark.parametrize("simtype", [0, 1, 2])
@pytest.mark.parametrize("NW", [8, 16])
def test_fslim_on_the_ladder(NW, simtype, monkeypatch, capfd, check):
    """FSLIM (32-wide tiles only): the neighbours selected from the screen sums, 10 of them and
    more than there are candidates; the checks of test_fslim_tile_kernel_matches_oracle (2e-5, the
    same neighbour counts, at most 4 pattern differences) on top of the common ones."""
    monkeypatch.setenv("SLIM_GPU_TILE_NW", str(NW))
    m = DeviceMatrix.from_scipy(ladder())
    for cluster in (1, 4):
        for nnbrs in (10, 5000):
            W, st, cs = solve(m, capfd, (32, NW, "fslim", "valued", False), l1r=L1R, l2r=L2R, nnbrs=nnbrs,
                              simtype=simtype, cluster=cluster, niters=200)
            Wo, so, obj_o = ladder_oracle(32, nnbrs=nnbrs, simtype=simtype, maxniters=200)
            check("P32 NW%d fslim valued, simtype %d cluster %d nnbrs %d" % (NW, simtype, cluster, nnbrs),
                  W, st, cs, Wo, so, obj_o, tol=2e-5)
            assert cs.nacols.max() <= nnbrs
            assert pattern_diff(W, Wo) <= 4
    m.close()


@pytest.mark.gpu
@pytest.mark.parametrize("P,NW", PNW)
def test_item_count_edges(P, NW, monkeypatch, capfd, check, record_property):
    """Item counts around P / NW problems per wavefront, a last tile narrower than NW, a single
    problem -- as matrices of that many items and as column ranges of the 65-item one; and three
    ranges that are no multiples of the tile add up to the one-call model."""
    monkeypatch.setenv("SLIM_GPU_TILE_NW", str(NW))
    expect = (P, NW, cold_form(P), "valued", False)
    full = DeviceMatrix.from_scipy(edges())
    for n in EDGE_COUNTS:
        R = edges(n)
        m = DeviceMatrix.from_scipy(R)
        W, st, cs = solve(m, capfd, expect, l1r=L1R, l2r=L2R, cluster=1)
        Wo, so, _, obj_o = O.learn_cd_tile(R, tileP=P, seed=3, nthreads=4, l1r=L1R, l2r=L2R, return_stats=True)
        assert W.shape == Wo.shape == (n, n)
        if n == 1:                      # one item has no neighbours: an empty model, objective 0
            assert W.nnz == Wo.nnz == 0 and cs.nacols[0] == so["nacols"][0] == 0
        else:
            check("P%d NW%d %s valued, %d items" % (P, NW, cold_form(P), n), W, st, cs, Wo, so, obj_o)
        m.close()
        W, st, cs = solve(full, capfd, expect, l1r=L1R, l2r=L2R, cluster=1, col_begin=0, col_end=n)
        Wo, so, _, obj_o = O.learn_cd_tile(edges(), tileP=P, order=O.tile_work_order(edges(), 0, n), seed=3,
                                           nthreads=4, l1r=L1R, l2r=L2R, return_stats=True)
        check("P%d NW%d %s valued, columns 0..%d of 65" % (P, NW, cold_form(P), n), W, st, cs, Wo, so, obj_o,
              cols=slice(0, n))
        assert W[:, n:].nnz == 0
    tight = dict(l1r=L1R, l2r=L2R, optTol=1e-12, niters=100000, cluster=1)
    whole, _, _ = solve(full, capfd, expect, **tight)
    parts = [solve(full, capfd, expect, col_begin=b, col_end=e, **tight)[0] for b, e in ((0, 37), (37, 38), (38, 65))]
    d = maxdiff(parts[0] + parts[1] + parts[2], whole)
    record_property("P%d NW%d ranges against one call" % (P, NW), "maxdiff %.3e" % d)
    assert d <= 2e-5
    full.close()


@pytest.mark.gpu
@pytest.mark.timeout(120, method="thread")
@pytest.mark.parametrize("P,NW", PNW)
def test_profiled_instantiations(P, NW, monkeypatch, capfd, check):
    """SLIM_GPU_TRACE=2 runs the profiled base instantiation, whatever the start: a cold solve goes
    through the kernel that holds the warm-start code, and a warm start of a 32-wide tile folds by
    column, not by row.  Same models."""
    monkeypatch.setenv("SLIM_GPU_TILE_NW", str(NW))
    monkeypatch.setenv("SLIM_GPU_TRACE", "2")
    for binary in (False, True):
        m = DeviceMatrix.from_scipy(ladder(96, binary), binary=binary)
        expect = (P, NW, "colfold", kind(binary), True)
        for cluster in (1, 4):
            W, st, cs = solve(m, capfd, expect, l1r=L1R, l2r=L2R, cluster=cluster)
            check("P%d NW%d colfold profiled %s cold cluster %d" % (P, NW, kind(binary), cluster), W, st, cs,
                  *ladder_oracle(P, binary))
            first, _, _ = solve(m, capfd, expect, cluster=cluster, **FIRST)
            assert maxdiff(first, ladder_oracle_first(P, binary)) <= 5e-5
            W, st, cs = solve(m, capfd, expect, l1r=L1R, l2r=L2R, cluster=cluster, imodel=first)
            check("P%d NW%d colfold profiled %s warm cluster %d" % (P, NW, kind(binary), cluster), W, st, cs,
                  *ladder_oracle(P, binary, warm=True))
        m.close()


@pytest.mark.gpu
@pytest.mark.timeout(120, method="thread")
@pytest.mark.parametrize("NW", [8, 16])
def test_heavy_prefetch_switch_changes_nothing(NW, monkeypatch, capfd, check):
    """SLIM_GPU_HI_PREFETCH=0: the heavy phase requests a slice's first ids when it needs them
    instead of a visit early.  When ids arrive never touches arithmetic: the same model bit for
    bit, the same sweeps, cold and warm (row fold)."""
    monkeypatch.setenv("SLIM_GPU_TILE_NW", str(NW))
    geom = GEOMS[2]
    m = DeviceMatrix.from_scipy(ladder())
    runs = {}
    for prefetch in (None, "0"):
        if prefetch is not None:
            monkeypatch.setenv("SLIM_GPU_HI_PREFETCH", prefetch)
        W, st, cs = solve(m, capfd, (32, NW, "cold", "valued", False), l1r=L1R, l2r=L2R, **geom)
        check("P32 NW%d cold valued, heavy phase, prefetch %s" % (NW, prefetch), W, st, cs, *ladder_oracle(32))
        first, _, _ = solve(m, capfd, (32, NW, "cold", "valued", False), **FIRST, **geom)
        Ww, stw, csw = solve(m, capfd, (32, NW, "rowfold", "valued", False), l1r=L1R, l2r=L2R, imodel=first, **geom)
        check("P32 NW%d rowfold valued, heavy phase, prefetch %s" % (NW, prefetch), Ww, stw, csw,
              *ladder_oracle(32, warm=True))
        runs[prefetch] = (W, cs.sweeps, Ww, csw.sweeps)
    a, b = runs[None], runs["0"]
    assert maxdiff(a[0], b[0]) == 0.0 and np.array_equal(a[1], b[1])
    assert maxdiff(a[2], b[2]) == 0.0 and np.array_equal(a[3], b[3])
    m.close()


@pytest.mark.gpu
@pytest.mark.timeout(120, method="thread")
@pytest.mark.parametrize("NW", [8, 16])
@pytest.mark.parametrize("P", [32, 16])
def test_xcd_placement_switch_changes_nothing(P, NW, monkeypatch, capfd, check):
    """SLIM_GPU_XCD=0: cluster members are not placed on one XCD.  Placement only: the same model
    bit for bit, the same sweeps, cold and warm."""
    # run_launches() turns the placement on when the device has 8 XCDs (CUs / 32 == 8) and the
    # launch size L = min(tiles, workgroup slots / cluster) * cluster satisfies L % 8 == 0 and
    # (L / 8) % cluster == 0 (no heavy phase).  256 items are 8 tiles of 32 or 16 tiles of 16; with
    # clusters of 4 on 256 CUs (>= 128 slots, 32 clusters at least) L = 32 or 64, L / 8 = 4 or 8:
    # the default run has it on.
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    assert cus % 32 == 0 and cus // 32 == 8, "not 8 XCDs of 32 CUs: the placement is off and the switch does nothing"
    monkeypatch.setenv("SLIM_GPU_TILE_NW", str(NW))
    m = DeviceMatrix.from_scipy(ladder(256))
    warm_form = "rowfold" if P == 32 else "colfold"
    runs = {}
    for xcd in (None, "0"):
        if xcd is not None:
            monkeypatch.setenv("SLIM_GPU_XCD", xcd)
        W, st, cs = solve(m, capfd, (P, NW, cold_form(P), "valued", False), l1r=L1R, l2r=L2R, cluster=4)
        check("P%d NW%d %s valued, cluster 4, 256 items, XCD %s" % (P, NW, cold_form(P), xcd), W, st, cs,
              *ladder_oracle(P, nitems=256))
        first, _, _ = solve(m, capfd, (P, NW, cold_form(P), "valued", False), cluster=4, **FIRST)
        Ww, stw, csw = solve(m, capfd, (P, NW, warm_form, "valued", False), l1r=L1R, l2r=L2R, imodel=first,
                             cluster=4)
        check("P%d NW%d %s valued, cluster 4, 256 items, XCD %s" % (P, NW, warm_form, xcd), Ww, stw, csw,
              *ladder_oracle(P, warm=True, nitems=256))
        runs[xcd] = (W, cs.sweeps, Ww, csw.sweeps)
    a, b = runs[None], runs["0"]
    assert maxdiff(a[0], b[0]) == 0.0 and np.array_equal(a[1], b[1])
    assert maxdiff(a[2], b[2]) == 0.0 and np.array_equal(a[3], b[3])
    m.close()


@pytest.mark.gpu
@pytest.mark.parametrize("past,NW", [(1, 8), (0, 8), (-1, 16)])
@pytest.mark.parametrize("P", [32, 16])
def test_automatic_wavefront_count(P, past, NW, capfd, check):
    """Without SLIM_GPU_TILE_NW: 8 wavefronts from 2 x CUs tiles up, 16 below -- every column of a
    matrix one tile past the boundary, the boundary itself and one tile short of it, each model
    against the oracle on its columns.

    Run at optTol=1e-10, as test_item_space_100k_items_the_lds_groups_of_g is: on this matrix (6
    ratings per column, ~120 coefficients each) the fp32 and the fp64 descent stop a
    default-tolerance solve further apart than 5e-5, with 8 and with 16 wavefronts alike (measured
    at optTol=1e-7, P = 32: 5.3e-4 and 2.5e-4 at 8, 8.3e-5 at 16; P = 16: 5.3e-5 and 1.8e-4 at 8,
    1.6e-4 at 16; objectives equal to 1e-9, > 99.9 % of the sweep counts equal)."""
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    R = wide(P * 2 * cus + P)
    n = P * (2 * cus + past)
    tight = dict(l1r=L1R, l2r=L2R, optTol=1e-10)
    m = DeviceMatrix.from_scipy(R)
    W, st, cs = solve(m, capfd, (P, NW, cold_form(P), "valued", False), cluster=1, col_begin=0, col_end=n,
                      niters=100000, **tight)
    Wo, so, _, obj_o = O.learn_cd_tile(R, tileP=P, order=O.tile_work_order(R, 0, n), seed=3, nthreads=16,
                                       maxniters=100000, return_stats=True, **tight)
    assert Wo[:, :n].nnz >= 10000
    check("P%d NW%d %s valued, chosen automatically, %d tiles" % (P, NW, cold_form(P), n // P), W, st, cs,
          Wo, so, obj_o, cols=slice(0, n))
    m.close()
