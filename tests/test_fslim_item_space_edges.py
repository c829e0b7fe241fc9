"""Kernel 6, FSLIM in item space (slim_amd/csrc/cd_fslim_gram.hpp: fslim_gram_select_kernel,
fslim_gram_union_kernel, cd_fslim_gram_kernel<BLOCK>) and its host plan (engine.hip: choose_kernel,
finish_path, alloc_slabs, the slice loop of run_launches) at the edges of its lists and catalogues.
test_fslim_item_space.py checks the kernel on catalogues of up to 3000 items and lists of up to 489; here:

  small catalogues  2 ... 257 items, every pair of columns co-rated, nnbrs above the item count: nn = ncols - 1
                    and nunion = ncols on both sides of 64 and of 128 together (the `k += 64` loops, the batches
                    of 64 permutation positions, the 128-entry visit queue, a last tile of one problem); block
                    form at strides 64 and 128, gathered at 192 and 256; 8 wavefronts for 2 problems; the
                    select kernel's row split with 1, 2, 3 and 4 wavefronts owning a segment;
  a catalogue past  8300 items: 260 bitmap words, 2 per thread of the union kernel, 126 threads past the end;
  8192              6 wavefronts of the block form at stride 64, 1 at stride 128; ties at the cut under all
                    three similarities;
  long lists        1344 ... 4096 neighbours that are really there: 4, 3, 2 and 1 wavefronts of the gathered
                    form, 115 KB of wavefront state; the refusal past 4096 and min(nnbrs, ncols - 1) = 4096;
  sweep caps        niters 1, 2, 3 (sweeps = niters + 1, conv = 0) and the 50 nnz cap;
  dyadic ratings    multiples of 1/4: G is exact in fp32, so no neighbour set can differ by rounding;
  the arena retry   a launch that overflows its arena: the pending columns in new tiles, and in new slices;
  slices x shards   one tile per slice, three shards, bit for bit the plain model.

Reference: slim_oracle.learn_cd_tile(nnbrs=, simtype=, tiles=), the fp64 restatement in the tile order, with
the seed, penalties and maxniters of the solve.  Bars: those of test_matches_the_oracle_tile_walk, on the
columns both sides solved -- nacols equal, maxdiff <= 2e-5, pattern_diff <= 4, D and U within 1 %, the objective
to 1e-4 relative, the sweep counts equal on >= 98 % of the columns.  The last is a share: it is asserted per
case from 200 columns on, and for every family over the family's pooled columns.  Across a regrouping of tiles
(the arena retry) the order differs: optTol = 1e-12, niters = 100000, maxdiff <= 2e-5 and equal nacols, as
test_column_ranges_sets_and_shards has it.

Shards: shard k of n holds the tiles k, k + n, ... of the unsharded work list -- work_list() in engine.hip
deals granules of 32 entries round-robin, cd_fslim_gram.hpp keys a tile's order by gkey = (p >> 5) *
shard_count + shard_index, and test_column_ranges_sets_and_shards adds two halves to the plain model bit for
bit.  So shard (43, 44) of 4200 items is the tiles 43, 87 and 131, each checked against tiles=(t, 1).

Every solve runs under SLIM_GPU_TRACE=1 and asserts its `[trace] item-space FSLIM:` line: the form, the list
stride and the wavefronts per workgroup.  finish_path prints it once per solve, not per launch (engine.hip is
among the sources that the committed counter figures of profiles/pmc_traffic.json are keyed to, so the trace
stays as it is here); that the arena retry launched again follows from an arena smaller than the model."""
import functools
import os

import numpy as np
import pytest
import scipy.sparse as sp

import fslim_cases as F
from library_output import stderr_of_the_library
from slim_amd.engine import DeviceMatrix

KERNEL_GRAM_FSLIM = 6
gpu = pytest.mark.gpu

# what the cases below are there for: test_fixtures_do_their_job recomputes every entry from the sources
SMALL_PLAN = {n: ("block in LDS", 64, 8) for n in (2, 3, 33, 63, 64, 65)}
SMALL_PLAN.update({n: ("block in LDS", 128, 2) for n in (66, 127, 128, 129)})
SMALL_PLAN.update({n: ("gathered", 192, 4) for n in (130, 192, 193)})
SMALL_PLAN.update({n: ("gathered", 256, 4) for n in (256, 257)})
BIG_PLAN = {20: ("block in LDS", 64, 6), 100: ("block in LDS", 128, 1), 129: ("gathered", 192, 4)}
LONG_PLAN = {n: ("gathered", F.round_up(n, 64), w) for n, w in zip(F.LONG_NNBRS, F.LONG_WAVES)}
PAST_PLAN = ("gathered", 4096, 1)
R11_PLAN = {64: ("block in LDS", 64, 7), 65: ("block in LDS", 128, 2)}


# ---- CPU -------------------------------------------------------------------------------------------------
def test_fixtures_do_their_job():
    """What the GPU cases rely on, from the matrices, the oracle and the sources alone."""
    k = F.constants()
    assert k["max_nbrs"] == 4096 and k["union_threads"] == 256 and k["select_threads"] == 256
    inst = open(os.path.join(F.CSRC, "fslim_gram_inst.hip")).read()
    assert "size_t b = 7 * sizeof(float) * (size_t)stride + 128 * sizeof(int32_t);" in inst
    assert "b += sizeof(uint16_t) * (size_t)tab_n + sizeof(float) * (size_t)stride * (size_t)stride;" in inst
    assert "return (b + 15) / 16 * 16;" in inst

    # -- the wavefront counts, recomputed from the constants and finish_path's formula
    for n, expect in SMALL_PLAN.items():
        assert F.plan(n, n + 5) == expect, n
    assert sorted(SMALL_PLAN) == list(F.SMALL_SIZES)
    for nnbrs, expect in BIG_PLAN.items():
        assert F.plan(8300, nnbrs) == expect, nnbrs
    for nnbrs, expect in LONG_PLAN.items():
        assert F.plan(4200, nnbrs) == expect, nnbrs
    assert F.plan(4097, 5000) == PAST_PLAN and min(5000, 4200 - 1) > k["max_nbrs"]
    for nnbrs, expect in R11_PLAN.items():
        assert F.plan(500, nnbrs) == expect, nnbrs
    # every count a form can have is run: 8, 7, 6 (stride 64); 2, 1 (stride 128); 4, 3, 2, 1 (gathered), and
    # the counts change where the cases stand
    assert [F.plan(n, 20)[2] for n in (256, 257, 500, 2048, 8300)] == [8, 7, 7, 6, 6]
    assert [F.plan(n, 100)[2] for n in (500, 3584, 3585, 8300)] == [2, 2, 1, 1]
    assert [F.plan(5000, n)[2] for n in (1344, 1345, 1792, 1793, 2688, 2689, 4096)] == [4, 3, 3, 2, 2, 1, 1]
    assert 7 * 4 * 4096 + 512 == 115200            # the state of a wavefront at the bound

    # -- small catalogues: every pair co-rated, so nn = ncols - 1 and nunion = ncols; the oracle converges
    for n in F.SMALL_SIZES:
        R = F.small(n)
        assert R.shape == (400, n) and np.all(R.data == 1.0) and np.all(R.getnnz(axis=0) == 120)
        assert F.all_pairs_corated(R)
        for s in (0, 1, 2) if n in F.SMALL_ALL_SIMTYPES else (0,):
            so = F.walk(("small", n, False), n + 5, s, **F.SMALL_KW)[1]
            assert np.all(so["nacols"] == n - 1) and np.all(so["conv"] == 1) and so["sweeps"].max() <= 14, (n, s)
    assert [n for n in F.SMALL_SIZES if n % 32 == 1 and n > 1] == [33, 65, 129, 193, 257]   # a last tile of one problem
    assert {F.select_segments(n) for n in F.SMALL_SIZES} == {1, 2, 3, 4}
    assert all(F.select_segments(n) < 4 for n in F.SMALL_SIZES if n <= 192)

    # -- the catalogue past 8192
    R = F.big()
    assert R.shape == (3000, 8300) and F.union_chunk(8192) == 1 and F.union_chunk(8300) == 2
    assert (260 + 1) // 2 < k["union_threads"]      # threads past the end of the bitmap
    cand = F.candidates(R)
    assert cand.min() >= 129                        # 2007 ... 2316: every list is full
    Rc = R.tocsc()
    ties = 0
    for it in np.random.default_rng(0).choice(8300, 100, replace=False):
        a = np.asarray((R.T @ Rc[:, it]).todense()).ravel()
        a[it] = 0
        s = np.sort(a[a > 0])[::-1]
        ties += int(s[19] == s[20])
    assert ties >= 80                               # 95
    assert len(F.work_order("big")) - 32 * F.BIG_TILES[-1] == 12
    for nnbrs, s in F.BIG_CASES:
        for t in F.BIG_TILES:
            so = F.walk("big", nnbrs, s, tiles=(t, 1), **F.BIG_KW)[1][F.tile_columns("big", t)]
            assert np.all(so["nacols"] == nnbrs) and np.all(so["conv"] == 1)
    assert not np.all(F.big(True).data == 1.0) and np.all(F.big(True).data * 4 == np.round(F.big(True).data * 4))
    assert not np.all(F.small(130, True).data == 1.0) and F.all_pairs_corated(F.small(130, True))

    # -- long lists: the neighbours are there; shard (43, 44) is the tiles 43, 87, 131
    assert F.candidates(F.long_lists()).min() >= 4096          # 4184 ... 4199
    assert F.candidates(F.long_lists(4097)).max() == 4096      # 4082 ... 4096
    assert [t for t in range(132) if t % F.LONG_SHARD[1] == F.LONG_SHARD[0]] == [43, 87, 131] and 4200 - 131 * 32 == 8
    assert [t for t in range(129) if t % F.PAST_SHARD[1] == F.PAST_SHARD[0]] == [42, 85, 128] and 4097 - 128 * 32 == 1
    for nnbrs in (F.LONG_NNBRS[0], F.LONG_NNBRS[-1]):
        _, so, _, cols = F.walk_tiles("long", nnbrs, F.LONG_SIMTYPE, (43, 87, 131), **F.LONG_KW)
        assert cols.size == 72 and np.all(so["nacols"][cols] == nnbrs) and np.all(so["conv"][cols] == 1)
    _, so, _, cols = F.walk_tiles("past", 5000, F.LONG_SIMTYPE, (42, 85, 128), **F.LONG_KW)
    assert cols.size == 65 and so["nacols"][cols].max() == 4096 and np.all(so["conv"][cols] == 1)

    # -- the caps
    for niters in (1, 2, 3):
        so = F.walk(("small", 66, False), 71, 0, maxniters=niters, **F.SMALL_KW)[1]
        assert np.all(so["sweeps"] == niters + 1) and not so["conv"].any()
    R = F.short_columns()
    so = F.walk("short", 135, 0, **F.SHORT_KW)[1]
    for item, n in F.SHORT_ITEMS.items():
        assert R.getnnz(axis=0)[item] == n and so["sweeps"][item] == 50 * n + 1 and so["nacols"][item] > 0
    rest = np.setdiff1d(np.arange(130), list(F.SHORT_ITEMS))
    assert np.all(so["sweeps"][rest] == 121) and not so["conv"].any()


# ---- GPU: handles and solves ----------------------------------------------------------------------------
_handles = {}


def device(name):
    """One handle per matrix for the whole module: G is built by its first solve."""
    if name not in _handles:
        R = F.matrix(name)
        _handles[name] = DeviceMatrix.from_scipy(R, binary=bool(np.all(R.data == 1.0)))
    return _handles[name]


@pytest.fixture(scope="module", autouse=True)
def _handles_closed():
    yield
    for m in _handles.values():
        m.close()
    _handles.clear()


def traced(fn, expect, env=None):
    """fn() under SLIM_GPU_TRACE=1 -> its result; the solve's one FSLIM line must name `expect` = (form, stride,
    wavefronts per workgroup)."""
    with stderr_of_the_library(dict(env or {}, SLIM_GPU_TRACE="1")) as err:
        out = fn()
    got = F.TRACE.findall(err[0])
    forms = [(g[0], int(g[1]), int(g[2])) for g in got]
    assert forms == [expect], (forms, expect)
    return out


def solve(name, expect, env=None, **kw):
    """One kernel-6 solve -> (W, stats, column stats)."""
    m = device(name) if not isinstance(name, DeviceMatrix) else name

    def run():
        W, st = m.learn(kernel=KERNEL_GRAM_FSLIM, seed=F.SEED, **kw)
        return W, st, m.column_stats()
    W, st, cs = traced(run, expect, env)
    assert st["kernel"] == KERNEL_GRAM_FSLIM
    return W, st, cs


def passes(figs):
    for f in figs:
        print(f)
    bad = [b for f in figs for b in f.failures()]
    assert not bad, "\n".join(bad)


def pooled(tag, figs):
    eq, n = F.pooled_sweeps(figs)
    print("%s: sweeps equal on %d of %d pooled columns (%.4f)" % (tag, eq, n, eq / n))
    assert eq >= 0.98 * n


# ---- 1. small catalogues -----------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def small_run(ncols, simtype, dyadic=False):
    name = ("small", ncols, dyadic)
    nnbrs = ncols + 5
    W, st, cs = solve(name, SMALL_PLAN[ncols], nnbrs=nnbrs, simtype=simtype, niters=200, **F.SMALL_KW)
    assert st["ncols_solved"] == ncols
    assert np.all(cs.nacols[:ncols] == ncols - 1)      # nn = ncols - 1: a full tile's union is every item
    Wo, so, _, obj_o = F.walk(name, nnbrs, simtype, **F.SMALL_KW)
    return F.Figures("%d items%s, simtype %d, %s" % (ncols, ", dyadic" if dyadic else "", simtype, SMALL_PLAN[ncols]),
                     W, cs, Wo, so, np.arange(ncols), st["objval"], obj_o)


@gpu
@pytest.mark.parametrize("ncols,simtype", F.SMALL_CASES)
def test_small_catalogues(ncols, simtype):
    """nn and nunion at 1, 2, 32, 62 ... 66, 126 ... 129, 191, 192, 255, 256 together."""
    fig = small_run(ncols, simtype)
    passes([fig])
    assert fig.conv


@gpu
def test_small_catalogues_sweep_counts_pooled():
    pooled("small catalogues", [small_run(n, s) for n, s in F.SMALL_CASES])


# ---- 2. a catalogue past 8192 items ------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def big_run(nnbrs, simtype, dyadic=False):
    """-> (at nnbrs = 20 the whole model against the whole walk, else None; [the tiles BIG_TILES against
    tiles=(k, 1)])."""
    name = "big dyadic" if dyadic else "big"
    tag = "8300 items%s, nnbrs %d, simtype %d, %s" % (", dyadic" if dyadic else "", nnbrs, simtype, BIG_PLAN[nnbrs])
    W, st, cs = solve(name, BIG_PLAN[nnbrs], nnbrs=nnbrs, simtype=simtype, niters=200, **F.BIG_KW)
    assert st["ncols_solved"] == 8300
    whole = None
    if nnbrs == 20:
        Wo, so, _, obj_o = F.walk(name, nnbrs, simtype, **F.BIG_KW)
        whole = F.Figures(tag + ", whole", W, cs, Wo, so, np.arange(8300), st["objval"], obj_o)
    tiles = []
    for t in F.BIG_TILES:
        Wt, sot, _, _ = F.walk(name, nnbrs, simtype, tiles=(t, 1), **F.BIG_KW)
        tiles.append(F.Figures(tag + ", tile %d" % t, W, cs, Wt, sot, F.tile_columns(name, t)))
    return whole, tiles


@gpu
@pytest.mark.parametrize("nnbrs,simtype", F.BIG_CASES)
def test_catalogue_past_8192(nnbrs, simtype):
    """Two bitmap words per thread in the union kernel and threads past the bitmap's end; 6 wavefronts on one
    queue (stride 64), 1 (stride 128), the gathered form; ties at the cut of 20 under cos, jac and dotp."""
    whole, tiles = big_run(nnbrs, simtype)
    passes(([whole] if whole else []) + tiles)
    assert tiles[-1].ncols == 12


@gpu
def test_catalogue_past_8192_sweep_counts_pooled():
    pooled("8300 items, tiles", [f for c in F.BIG_CASES for f in big_run(*c)[1]])
    pooled("8300 items, whole", [big_run(*c)[0] for c in F.BIG_CASES if c[0] == 20])


# ---- 3. long lists -------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def long_run(name, nnbrs):
    ncols, shard, plan = (4200, F.LONG_SHARD, LONG_PLAN.get(nnbrs)) if name == "long" else (4097, F.PAST_SHARD, PAST_PLAN)
    tiles = tuple(range(shard[0], (ncols + 31) // 32, shard[1]))
    W, st, cs = solve(name, plan, nnbrs=nnbrs, simtype=F.LONG_SIMTYPE, niters=200, shard=shard, **F.LONG_KW)
    Wo, so, obj_o, cols = F.walk_tiles(name, nnbrs, F.LONG_SIMTYPE, tiles, **F.LONG_KW)
    assert st["ncols_solved"] == cols.size
    assert W.nnz == W[:, cols].nnz and cs.nacols[cols].max() == min(nnbrs, 4096)
    return F.Figures("%d items, nnbrs %d, %s" % (ncols, nnbrs, plan), W, cs, Wo, so, cols, st["objval"], obj_o)


@gpu
@pytest.mark.parametrize("nnbrs", F.LONG_NNBRS)
def test_long_lists(nnbrs):
    """Lists of 1344 ... 4096 neighbours, every one filled: 4, 3, 3, 2, 1, 1 wavefronts per workgroup, each with
    its state at wave * wave_lds; tiles 43, 87 and 131 (8 problems) of the work list, as shard (43, 44)."""
    passes([long_run("long", nnbrs)])


@gpu
def test_long_lists_at_the_bound_of_4096():
    """min(nnbrs, ncols - 1) = 4199 is refused; 4096 (4097 items, nnbrs 5000) runs, and its last tile holds one
    problem."""
    with pytest.raises(RuntimeError, match="4096"):
        device("long").learn(kernel=KERNEL_GRAM_FSLIM, seed=F.SEED, nnbrs=5000, simtype=F.LONG_SIMTYPE, **F.LONG_KW)
    passes([long_run("past", 5000)])


@gpu
def test_long_lists_sweep_counts_pooled():
    pooled("long lists", [long_run("long", n) for n in F.LONG_NNBRS] + [long_run("past", 5000)])


# ---- 4. sweep caps -------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("niters", [1, 2, 3])
def test_exhausted_sweep_loop(niters):
    """niters sweeps and no convergence: sweeps = niters + 1, conv = 0 on every column, the oracle's model."""
    name = ("small", 66, False)
    W, st, cs = solve(name, SMALL_PLAN[66], nnbrs=71, simtype=0, niters=niters, **F.SMALL_KW)
    Wo, so, _, obj_o = F.walk(name, 71, 0, maxniters=niters, **F.SMALL_KW)
    fig = F.Figures("66 items, %d sweeps" % niters, W, cs, Wo, so, np.arange(66), st["objval"], obj_o)
    passes([fig])
    assert np.all(cs.sweeps[:66] == niters + 1) and not cs.conv[:66].any()
    assert fig.sweeps_equal == 66 and fig.conv


@gpu
def test_sweeps_stop_at_50_nnz():
    """Columns of 1 and 2 users among columns of 120, optTol = 0 and niters = 120: 51, 101 and 121 sweeps."""
    W, st, cs = solve("short", F.plan(130, 135), nnbrs=135, simtype=0, niters=F.SHORT_KW["maxniters"],
                                optTol=F.SHORT_KW["optTol"])
    Wo, so, _, obj_o = F.walk("short", 135, 0, **F.SHORT_KW)
    fig = F.Figures("130 items, short columns", W, cs, Wo, so, np.arange(130), st["objval"], obj_o)
    passes([fig])
    for item, n in F.SHORT_ITEMS.items():
        assert cs.sweeps[item] == 50 * n + 1
    assert np.array_equal(cs.sweeps[:130], so["sweeps"][:130]) and not cs.conv[:130].any()


# ---- 5. dyadic ratings ---------------------------------------------------------------------------------------
DYADIC_BIG = [(20, 0), (20, 1), (20, 2), (129, 0)]


@gpu
@pytest.mark.parametrize("simtype", [0, 1, 2])
def test_dyadic_ratings_130_items(simtype):
    fig = small_run(130, simtype, True)
    passes([fig])
    assert fig.conv


@gpu
@pytest.mark.parametrize("nnbrs,simtype", DYADIC_BIG)
def test_dyadic_ratings_8300_items(nnbrs, simtype):
    """Ratings in {0.25, 0.5, ..., 5}: every entry of G is exact in fp32 whatever the order of its sum."""
    whole, tiles = big_run(nnbrs, simtype, True)
    passes(([whole] if whole else []) + tiles)


@gpu
def test_dyadic_ratings_sweep_counts_pooled():
    pooled("dyadic, 130 items", [small_run(130, s, True) for s in (0, 1, 2)])
    pooled("dyadic, 8300 items, tiles", [f for c in DYADIC_BIG for f in big_run(*c, True)[1]])


# ---- 6. a launch that overflows its arena ------------------------------------------------------------------
TIGHT = dict(nnbrs=64, simtype=0, optTol=1e-12, niters=100000)


@gpu
def test_arena_overflow_regroups_the_pending_columns():
    """An arena of a third of the model: the columns that did not fit form new tiles (another order, hence the
    tight tolerance), and the handle's next solve is the model of a handle
    that never overflowed, bit for bit."""
    R = F.matrix("r11")
    Wo, so, _, _ = F.walk("r11", 64, 0, optTol=1e-12, maxniters=100000)
    never = DeviceMatrix.from_scipy(R, binary=True)
    m = DeviceMatrix.from_scipy(R, binary=True)
    try:
        W0, st0, cs0 = solve(never, R11_PLAN[64], **TIGHT)
        assert maxdiff_and_nacols("plain", W0, cs0, Wo, so)
        arena = max(1024, int(st0["nnzW"]) // 3)
        assert 2 * arena < st0["nnzW"]                 # one launch cannot hold the model: the retry runs
        env = {"SLIM_GPU_ARENA": str(arena)}
        W1, st1, cs1 = solve(m, R11_PLAN[64], env=env, **TIGHT)
        assert W1.nnz == st1["nnzW"] and maxdiff_and_nacols("learn, arena of a third", W1, cs1, Wo, so)

        def resident():
            rm, st = m.learn_resident(kernel=KERNEL_GRAM_FSLIM, seed=F.SEED, **TIGHT)
            cs = m.column_stats()
            W = rm.fetch()
            rm.free()
            return W, st, cs
        W2, st2, cs2 = traced(resident, R11_PLAN[64], env)
        assert st2["kernel"] == KERNEL_GRAM_FSLIM and W2.nnz == st2["nnzW"]
        assert maxdiff_and_nacols("learn_resident + fetch, arena of a third", W2, cs2, Wo, so)

        W3, _, _ = solve(m, R11_PLAN[64], **TIGHT)
        assert F.same_bits(W3, W0)
    finally:
        never.close()
        m.close()


def maxdiff_and_nacols(tag, W, cs, Wo, so):
    d, nac = F.maxdiff(W, Wo), bool(np.array_equal(cs.nacols[:500], so["nacols"][:500]))
    print("%s: maxdiff %.3e, nacols equal %s, nnz %d / %d" % (tag, d, nac, W.nnz, Wo.nnz))
    return W.nnz > 0 and d <= 2e-5 and nac


@gpu
def test_arena_overflow_in_slices():
    """The same with one tile per slice: the retry's columns go through in slices of their own."""
    m = device("r11")
    W0, st0, _ = solve(m, R11_PLAN[64], **TIGHT)
    Wo, so, _, _ = F.walk("r11", 64, 0, optTol=1e-12, maxniters=100000)
    arena = max(1024, int(st0["nnzW"]) // 3)
    assert 2 * arena < st0["nnzW"]
    env = {"SLIM_GPU_ARENA": str(arena), "SLIM_GPU_FSLIM_SLICE_TILES": "1"}
    W1, st1, cs1 = solve(m, R11_PLAN[64], env=env, **TIGHT)
    assert maxdiff_and_nacols("one tile per slice, arena of a third", W1, cs1, Wo, so)


# ---- 7. slices with shards -------------------------------------------------------------------------------------
@gpu
def test_slices_with_shards_add_up_to_the_plain_model():
    m = device("r11")
    kw = dict(nnbrs=65, simtype=1, niters=200)
    W, _, _ = solve(m, R11_PLAN[65], **kw)
    assert W.nnz > 0
    total = sp.csc_matrix(W.shape, dtype=np.float32)
    for k in range(3):
        tiles = range(k, 16, 3)
        ncols = sum(min(32, 500 - 32 * t) for t in tiles)
        Wk, stk, _ = solve(m, R11_PLAN[65], env={"SLIM_GPU_FSLIM_SLICE_TILES": "1"}, shard=(k, 3), **kw)
        assert stk["ncols_solved"] == ncols and Wk.nnz > 0
        total = total + Wk
    assert F.same_bits(total, W)
