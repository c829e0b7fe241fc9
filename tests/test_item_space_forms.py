"""Every form of the item-space solver (coordinate descent on G = R^T R) against the oracle's tile
walk, at the item counts where the form changes and at the edges of the union list's batches.

finish_path() (engine.hip) picks the kernel of an item-space solve from the item count alone:
  * G as floats (cd_gram.hpp), gram_geometry(): <NW,V> = <4,2> <8,2> <16,2> <16,5> <16,10> up to
    ncols_pad (items rounded up to 64) 2048, 4096, 8192, 20480 and kGramMaxColsPad = 40832, beyond
    that <8,0> (g in HBM; SLIM_GPU_GRAM_NW=16: <16,0>);
  * G as byte planes (cd_gramr.hpp), gramr_kernel(): <KR,KL> = <1,0> <3,0> <6,0> <10,3> for up to
    1, 3, 6 and 13 groups of 8192 ranks (8192, 24576, 49152, 106496 items), the row streamed by
    register loads or through the LDS ring (SLIM_GPU_GRAMR_DMA; <10,3> has the ring only), <3,0>
    with 128 VGPRs (WPS 4) or, under SLIM_GPU_GRAMR_WPS=2, with 256 (WPS 2);
    beyond 106496 items nothing is packed and the float <8,0> runs.
The engine's `[trace] item-space kernel:` line proves which one ran.

Reference: O.learn_cd_tile, the fp64 restatement walking the tile's visiting order, started from
the same model.  The checks are the suite's own for this comparison (test_gpu_parity.py): max |dW|
<= 5e-5, the same active-set sizes, >= 95 % of the sweep counts (the figure of
test_packed_gram_of_ratings_third_plane_everywhere for 64 columns), the objective to 1e-4 relative
where a whole matrix is solved; the large forms at optTol=1e-10 with 2e-5 and 90 %, as
test_item_space_100k_items_the_lds_groups_of_g has them.  Between the forms of one size the check is
the strict one of _item_space_modes: EQUAL models, sweeps, D and U.

Every comparison of a test is made and printed before the test fails on any of them."""
import functools
import os
import re

import numpy as np
import pytest
import scipy.sparse as sp

import slim_oracle as O
from library_output import stderr_of_the_library
from slim_amd.engine import KERNEL_GRAM, DeviceMatrix

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "slim_amd", "csrc")
TRACE = re.compile(r"\[trace\] item-space kernel: (.*)")

# ---- the boundaries (C++: test_boundaries_are_the_sources pins them to the sources) --------------
FLOAT_FORMS = ((2048, (4, 2)), (4096, (8, 2)), (8192, (16, 2)), (20480, (16, 5)), (40832, (16, 10)))
FLOAT_HBM = (8, 0)                      # beyond kGramMaxColsPad = 40832
GROUP = 8192                            # ranks per group of g (kPackGroup = 16 * kGramrNT)
PACKED_FORMS = ((1, (1, 0, 4)), (3, (3, 0, 4)), (6, (6, 0, 2)), (13, (10, 3, 2)))   # groups -> <KR,KL>, WPS
PACKED_MAX = 13 * GROUP                 # 106496 items
LDS_RANK0 = 10 * GROUP                  # 81920: the first rank <10,3> holds in LDS

SMALL = (1, 2, 15, 16, 17, 33, 63, 64, 65, 127, 129)
FLOAT_SWITCHES = (2048, 2049, 4096, 4097, 8192, 8193, 20480, 20481, 40832, 40833)
PACKED_EDGES = (8191, 8192, 8193, 24576, 24577, 49152, 49153)
EDGE_SIZES = SMALL + tuple(sorted(set(FLOAT_SWITCHES + PACKED_EDGES)))
LARGE_SIZES = (81920, 81936, 106496, 106497)

SEED = 3
COLD = dict(l1r=0.5, l2r=1.0)           # binary, ~20 ratings a column: G > 0.5 is "co-rated"
WARM = dict(l1r=0.3, l2r=3.0)           # (the same active sets: the previous model is folded whole)
LADDER_COLD = dict(l1r=1.0, l2r=0.5)
LADDER_FIRST = dict(l1r=3.0, l2r=1.0)


def float_form(ncols):
    pad = (ncols + 63) // 64 * 64
    for upto, form in FLOAT_FORMS:
        if pad <= upto:
            return form
    return FLOAT_HBM


def packed_form(ncols):
    """(KR, KL, WPS) or None where nothing is packed."""
    groups = ((ncols + 15) // 16 + 511) // 512
    for upto, form in PACKED_FORMS:
        if groups <= upto:
            return form
    return None


def modes(ncols, keep_g=True):
    """[(environment, the trace's text)]: the float kernel, the packed one with register loads and
    through the ring; <3,0> also with 256 VGPRs, the float kernel with g in HBM also with 16
    wavefronts."""
    out = []
    base = {"SLIM_GPU_KEEP_G": "1"} if keep_g else {}
    f, p = float_form(ncols), packed_form(ncols)
    if keep_g or p is None:
        out.append((dict(base, SLIM_GPU_NO_GRAMR="1"), "float <%d,%d>" % f))
        if ncols in (40833, 49153):
            out.append((dict(base, SLIM_GPU_NO_GRAMR="1", SLIM_GPU_GRAM_NW="16"), "float <16,0>"))
    if p is not None:
        for dma in ("0", "1"):
            loads = "ring" if dma == "1" or p[0] == 10 else "register"
            out.append((dict(base, SLIM_GPU_GRAMR_DMA=dma), "packed <%d,%d>, %s loads, WPS %d" % (p[0], p[1], loads, p[2])))
            if 8193 <= ncols <= 24576:
                out.append((dict(base, SLIM_GPU_GRAMR_DMA=dma, SLIM_GPU_GRAMR_WPS="2"),
                            "packed <3,0>, %s loads, WPS 2" % loads))
    return out


def maxdiff(a, b):
    d = abs(sp.csc_matrix(a) - sp.csc_matrix(b))
    return float(d.max()) if d.nnz else 0.0


# ---- the host's side of a fixture ------------------------------------------------------------------
def popularity_order(R):
    """item_of (rank -> id): ratings per item descending, ties by id; rank_of; ratings per item."""
    nnzc = np.diff(sp.csc_matrix(R).indptr)
    item_of = np.lexsort((np.arange(nnzc.size), -nnzc)).astype(np.int64)
    rank_of = np.empty_like(item_of)
    rank_of[item_of] = np.arange(item_of.size)
    return item_of, rank_of, nnzc


def column_cost(R):
    """The engine's cost of a column: the row lengths of its users, summed (SLIMGPU_MatrixColumnCost)."""
    Rr = sp.csr_matrix(R)
    Rc = Rr.tocsc()
    deg = np.diff(Rr.indptr).astype(np.int64)
    return np.add.reduceat(np.concatenate([deg[Rc.indices], [0]]), Rc.indptr[:-1]) * (np.diff(Rc.indptr) > 0)


def work_order(R, cols=None):
    """The work list of a solve of `cols` (None: all): most expensive first, stable."""
    cost = column_cost(R)
    cols = np.arange(R.shape[1], dtype=np.int32) if cols is None else np.asarray(cols, np.int32)
    return cols[np.argsort(-cost[cols], kind="stable")]


def tile_unions(R, order, l1r, binary):
    """The union list of every tile of 32 of `order`: the ids i with G[c, i] > l1r for a column c != i
    of the tile."""
    Rc = sp.csc_matrix(R, dtype=np.float64)
    if binary:
        Rc.data[:] = 1.0
    out = []
    for b in range(0, len(order), 32):
        tile = np.asarray(order[b:b + 32])
        G = sp.coo_matrix(Rc[:, tile].T @ Rc)
        act = (G.data > l1r) & (tile[G.row] != G.col)
        out.append(np.unique(G.col[act]))
    return out


def plant_last_rank(Rc, c, rng, cols=None):
    """The item of the last rank (the fewest ratings, ties by id) gets users of column c in place of
    its own, as many as it had: it stays last, and it is co-rated with c.  With `cols`, the columns
    to be solved: the first draw of those users with which every tile of the work list holds a
    column co-rated with the item, so that it is on every tile's union list."""
    item_of, _, nnzc = popularity_order(Rc)
    last = int(item_of[-1])
    assert last != c and nnzc[last] <= nnzc[c]
    users_c = Rc.indices[Rc.indptr[c]:Rc.indptr[c + 1]]
    Rr = sp.csr_matrix(Rc)
    for _ in range(200):
        users = np.sort(rng.choice(users_c, nnzc[last], replace=False))
        Rc.indices[Rc.indptr[last]:Rc.indptr[last + 1]] = users
        if cols is None:
            return last
        co = np.setdiff1d(np.concatenate([Rr.indices[Rr.indptr[u]:Rr.indptr[u + 1]] for u in users]), [last])
        order = work_order(Rc, cols)
        if all(np.isin(order[b:b + 32], co).any() for b in range(0, len(order), 32)):
            return last
    raise AssertionError("no draw puts the item of the last rank on every tile's union list")


def random_binary(nusers, ncols, density, rng):
    """nusers x ncols, binary, no empty column (the oracle sizes the model by the last rated item)."""
    R = sp.random(nusers, ncols, density=density, format="coo", random_state=rng, dtype=np.float32)
    empty = np.flatnonzero(np.bincount(R.col, minlength=ncols) == 0)
    rows = np.concatenate([R.row, rng.integers(0, nusers, empty.size)])
    cols = np.concatenate([R.col, empty])
    Rc = sp.csc_matrix((np.ones(rows.size, np.float32), (rows, cols)), shape=(nusers, ncols))
    Rc.sort_indices()
    return Rc


def as_csr(Rc):
    R = sp.csr_matrix(Rc)
    R.sort_indices()
    return R


# ---- 1. item-count edges ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def edge(ncols):
    """(R, columns to solve or None for all, the planted item or None).  2000 users, binary, density
    0.01, no empty column; the item of the last rank is co-rated with a solved column c (see
    plant_last_rank): the most popular item, and from 2048 items up the item of the middle rank.
    From 2048 items up 96 columns are solved: the 32 most popular, the 32 least popular and the 32
    around c by rank."""
    rng = np.random.default_rng(1000 + ncols)
    Rc = random_binary(2000, ncols, 0.01, rng)
    if ncols == 1:
        return as_csr(Rc), None, None
    item_of = popularity_order(Rc)[0]
    mid = ncols // 2
    c = int(item_of[mid] if ncols >= 2048 else item_of[0])
    cols = None
    if ncols >= 2048:   # (the planting keeps every item's number of ratings, hence the ranks)
        cols = np.unique(np.concatenate([item_of[:32], item_of[-32:], item_of[mid - 16:mid + 16]])).astype(np.int32)
    last = plant_last_rank(Rc, c, rng, cols)
    return as_csr(Rc), cols, last


@functools.lru_cache(maxsize=None)
def edge_oracle(ncols, warm=False, maxniters=10000, l1r=None):
    """(W, column stats, objective) of the oracle's walk over the solved tiles; warm: from its own
    cold model, at the penalties WARM."""
    R, cols, _ = edge(ncols)
    kw = dict(WARM if warm else COLD)
    if l1r is not None:
        kw["l1r"] = l1r
    imodel = edge_oracle(ncols)[0] if warm else None
    W, so, _, obj = O.learn_cd_tile(R, tileP=32, order=work_order(R, cols), seed=SEED, nthreads=8, binary=True,
                                    imodel=imodel, maxniters=maxniters, return_stats=True, **kw)
    return W, so, obj


def last_chunk_ranks(ncols):
    return np.arange((ncols - 1) // 16 * 16, ncols)


@pytest.mark.parametrize("ncols", EDGE_SIZES)
def test_fixtures_do_their_job(ncols):
    """No column is empty; the popularity order puts the planted item last; the oracle's model, cold
    and warm, has a coefficient on a rank of the last chunk; from 2048 items up the union list of
    every solved tile reaches the last group of 8192 ranks (below, where all columns are solved and
    there is one group, that of the tile with the planted item's partner does)."""
    R, cols, last = edge(ncols)
    assert R.shape == (2000, ncols) and np.all(R.data == 1.0)
    item_of, rank_of, nnzc = popularity_order(R)
    assert nnzc.min() >= 1
    if ncols == 1:
        assert edge_oracle(1)[0].nnz == 0
        return
    assert item_of[-1] == last
    lastc = set(item_of[last_chunk_ranks(ncols)])
    for warm in (False, True):
        W = edge_oracle(ncols, warm)[0].tocoo()
        assert lastc & set(W.row[W.data != 0]), "no coefficient on the last chunk"
    order = work_order(R, cols)
    assert cols is None or 64 <= len(cols) <= 128
    unions = tile_unions(R, order, COLD["l1r"], True)
    first_of_last_group = (ncols - 1) // GROUP * GROUP
    reach = [u.size > 0 and rank_of[u].max() >= first_of_last_group for u in unions]
    if ncols >= 2048:
        assert all(reach), reach
        assert all(last in u for u in unions)      # (at 8193, 24577, 49153 items it IS the last group)
    else:
        assert any(reach)


def solve(m, env, expect, **kw):
    """One item-space solve under `env` whose trace line must read `expect` -> (W, stats, column stats)."""
    with stderr_of_the_library(dict(env, SLIM_GPU_TRACE="1")) as err:
        W, st = m.learn(kernel=KERNEL_GRAM, seed=SEED, **kw)
        cs = m.column_stats()
    assert st["kernel"] == KERNEL_GRAM
    got = TRACE.findall(err[0])
    assert got == [expect], (got, expect)
    return W, st, cs


class Checks(object):
    """Collects what failed, so that a test reports every figure before it fails."""

    def __init__(self):
        self.failed = []

    def that(self, ok, what):
        if not ok:
            self.failed.append(what)

    def against_oracle(self, tag, run, oracle, cols, whole, tol=5e-5, sweeps=0.95):
        W, st, cs = run
        Wo, so, obj_o = oracle
        cols = np.arange(Wo.shape[1]) if cols is None else cols
        d = maxdiff(W[:, cols], Wo[:, cols])
        same = float((cs.sweeps[cols] == so["sweeps"][cols]).mean())
        nac = bool(np.array_equal(cs.nacols[cols], so["nacols"][cols]))
        rel = abs(st["objval"] - obj_o) / abs(obj_o) if obj_o else abs(st["objval"])
        print("%s: maxdiff %.3e, nacols equal %s, sweeps equal %.4f, objval rel %.2e, nnz %d (oracle %d, up to %d sweeps)"
              % (tag, d, nac, same, rel, W.nnz, Wo[:, cols].nnz, so["sweeps"][cols].max()))
        self.that(W.shape == Wo.shape, "%s: shape %s against %s" % (tag, W.shape, Wo.shape))
        self.that(W.nnz == W[:, cols].nnz, "%s: coefficients outside the solved columns" % tag)
        self.that(d <= tol, "%s: maxdiff %.3e > %.0e" % (tag, d, tol))
        self.that(nac, "%s: nacols differ" % tag)
        self.that(same >= sweeps, "%s: sweeps equal on %.4f < %.2f" % (tag, same, sweeps))
        if whole:
            self.that(rel <= 1e-4, "%s: objective %.6e against %.6e" % (tag, st["objval"], obj_o))

    def forms_equal(self, tag, runs, names):
        W0, _, c0 = runs[0]
        for (W, _, cs), name in zip(runs[1:], names[1:]):
            d = maxdiff(W0, W)
            eq = all(np.array_equal(getattr(c0, k), getattr(cs, k)) for k in ("sweeps", "D", "U", "nacols"))
            print("%s: %s against %s: maxdiff %.3e, sweeps / D / U equal %s" % (tag, name, names[0], d, eq))
            self.that(d == 0.0, "%s: %s differs from %s by %.3e" % (tag, name, names[0], d))
            self.that(eq, "%s: sweeps, D or U of %s differ from %s" % (tag, name, names[0]))

    def done(self):
        assert not self.failed, "\n".join(self.failed)


def every_form(chk, tag, m, ncols, cols, oracle, keep_g=True, tol=5e-5, sweeps=0.95, **kw):
    """One solve per form of `ncols` items: each against the oracle, all EQUAL to the first."""
    forms = modes(ncols, keep_g)
    runs = [solve(m, env, expect, columns=cols, **kw) for env, expect in forms]
    names = [expect + "".join(" %s=%s" % (k[9:], v) for k, v in sorted(env.items()) if k != "SLIM_GPU_KEEP_G")
             for env, expect in forms]
    for run, name in zip(runs, names):
        chk.against_oracle("%s, %s" % (tag, name), run, oracle, cols, whole=cols is None, tol=tol, sweeps=sweeps)
    chk.forms_equal(tag, runs, names)
    return runs


@pytest.mark.gpu
@pytest.mark.timeout(120, method="thread")
@pytest.mark.parametrize("ncols", EDGE_SIZES)
def test_item_count_edges(ncols):
    """Every form of one item count, cold and warm-started from the oracle's cold model (so that no
    difference of the first solve enters the second); up to 129 items also capped at one and at two
    sweeps and with an l1r above every entry of G (no active set anywhere)."""
    R, cols, _ = edge(ncols)
    chk = Checks()
    with stderr_of_the_library({"SLIM_GPU_KEEP_G": "1"}):
        m = DeviceMatrix.from_scipy(R, binary=True)
    try:
        chk.that(np.array_equal(m.column_cost(), column_cost(R)), "column costs")
        every_form(chk, "%d items, cold" % ncols, m, ncols, cols, edge_oracle(ncols), **COLD)
        every_form(chk, "%d items, warm" % ncols, m, ncols, cols, edge_oracle(ncols, True),
                   imodel=edge_oracle(ncols)[0], **WARM)
        if ncols <= 129:
            for n in (1, 2):
                every_form(chk, "%d items, %d sweeps" % (ncols, n), m, ncols, cols,
                           edge_oracle(ncols, maxniters=n), niters=n, **COLD)
            runs = every_form(chk, "%d items, no active set" % ncols, m, ncols, cols, edge_oracle(ncols, l1r=1e4),
                              **dict(COLD, l1r=1e4))
            chk.that(all(W.nnz == 0 and not cs.nacols.any() for W, _, cs in runs), "an active set at l1r = 1e4")
    finally:
        m.close()
    chk.done()


# ---- 2. the large forms ----------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def large(ncols):
    """(R, the 128 columns to solve, the planted item): 4000 users, density 0.005, binary, uniform
    popularity (test_item_space_100k_items_the_lds_groups_of_g's matrix at another width); the item
    of the last rank co-rated with the most popular one; solved: the 64 most and the 64 least
    popular items."""
    rng = np.random.default_rng(2000 + ncols)
    Rc = random_binary(4000, ncols, 0.005, rng)
    item_of = popularity_order(Rc)[0]
    last = plant_last_rank(Rc, int(item_of[0]), rng)
    cols = np.sort(np.concatenate([item_of[:64], item_of[-64:]])).astype(np.int32)
    return as_csr(Rc), cols, last


LARGE_KW = dict(optTol=1e-10)   # (as the 100 000-item test, for its reason: ~540 coefficients a column)


@functools.lru_cache(maxsize=None)
def large_oracle(ncols, warm=False):
    R, cols, _ = large(ncols)
    imodel = large_oracle(ncols)[0] if warm else None
    W, so, _, obj = O.learn_cd_tile(R, tileP=32, order=work_order(R, cols), seed=SEED, nthreads=8, binary=True,
                                    imodel=imodel, return_stats=True, **(WARM if warm else COLD), **LARGE_KW)
    return W, so, obj


@pytest.mark.parametrize("ncols", LARGE_SIZES)
def test_large_fixtures_do_their_job(ncols):
    """The planted item is last; where <10,3> has live LDS ranks (>= 81920) the oracle's model has
    coefficients on them: at 81936 on the one LDS chunk, at 106496 on more than 10 % of the entries."""
    R, cols, last = large(ncols)
    item_of, rank_of, nnzc = popularity_order(R)
    assert nnzc.min() >= 1 and item_of[-1] == last and last in cols and cols.size == 128
    for warm in (False, True):
        W = large_oracle(ncols, warm)[0].tocoo()
        ranks = rank_of[W.row[W.data != 0]]
        assert ranks.size > 1000
        assert ranks.max() >= (ncols - 1) // 16 * 16            # the last chunk
        if ncols == 81920:
            assert ranks.max() < LDS_RANK0
        if ncols == 81936:
            assert (ranks >= LDS_RANK0).any()
        if ncols == 106496:
            assert (ranks >= LDS_RANK0).mean() > 0.1


@pytest.mark.gpu
@pytest.mark.timeout(600, method="thread")
@pytest.mark.parametrize("ncols", LARGE_SIZES)
def test_large_forms_at_their_edges(ncols):
    """<10,3> with no live LDS rank (81920 items), with one LDS chunk (81936) and with every slot
    full (106496); one item more and nothing is packed: the float <8,0> runs on 4 ncols_pad bytes a
    row.  Up to 81936 items both forms of G stay on the handle and the models are EQUAL; beyond, G
    is 45 GB and each size has the form it would have in use."""
    R, cols, _ = large(ncols)
    keep = ncols <= 81936
    chk = Checks()
    with stderr_of_the_library({"SLIM_GPU_KEEP_G": "1"} if keep else {}):
        m = DeviceMatrix.from_scipy(R, binary=True)
    try:
        kw = dict(keep_g=keep, tol=2e-5, sweeps=0.9)
        cold = every_form(chk, "%d items, cold" % ncols, m, ncols, cols, large_oracle(ncols), **kw, **COLD, **LARGE_KW)
        every_form(chk, "%d items, warm" % ncols, m, ncols, cols, large_oracle(ncols, True),
                   imodel=large_oracle(ncols)[0], **kw, **WARM, **LARGE_KW)
        st = cold[0][1]
        if ncols > PACKED_MAX:
            assert packed_form(ncols) is None and len(cold) == 1
            chk.that(st["gram_bytes"] == st["gram_rows"] * 4.0 * ((ncols + 63) // 64 * 64), "the float rows' byte model")
        else:
            stp = cold[-1][1]
            chk.that(0 < stp["gram_bytes"] < 0.5 * stp["gram_rows"] * 4.0 * ncols, "the packed rows' byte model")
    finally:
        m.close()
    chk.done()


# ---- 3. union lists and batches ----------------------------------------------------------------------
BLOCKS = (1, 2, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 512, 513)
BLOCK_USERS = 48


@functools.lru_cache(maxsize=None)
def union_ladder():
    """Independent blocks of m items for m in BLOCKS, each with its own 48 users: a user rates each
    item of their block with probability 0.7, ratings 1-5, and the block's first user rates them
    all -- so any two items of a block are co-rated (G >= 1 from that user, ~23 users more), none
    across blocks.  -> (R, first item of every block)."""
    rng = np.random.default_rng(77)
    first = np.concatenate([[0], np.cumsum(BLOCKS)])
    blocks = []
    for m in BLOCKS:
        mask = rng.random((BLOCK_USERS, m)) < 0.7
        mask[0, :] = True
        blocks.append(sp.csr_matrix(mask * rng.integers(1, 6, mask.shape).astype(np.float32)))
    R = sp.block_diag(blocks, format="csr", dtype=np.float32)
    R.sort_indices()
    return R, first[:-1]


def ladder_tile(k):
    """The tile of block k: its first min(m, 32) columns."""
    first = union_ladder()[1]
    return np.arange(first[k], first[k] + min(BLOCKS[k], 32), dtype=np.int32)


@functools.lru_cache(maxsize=None)
def ladder_oracle(k, warm=False):
    R = union_ladder()[0]
    kw = dict(tileP=32, order=work_order(R, ladder_tile(k)), seed=SEED, nthreads=4)
    imodel = ladder_first(k) if warm else None
    W, so, _, obj = O.learn_cd_tile(R, imodel=imodel, return_stats=True, **LADDER_COLD, **kw)
    return W, so, obj


@functools.lru_cache(maxsize=None)
def ladder_first(k):
    R = union_ladder()[0]
    return O.learn_cd_tile(R, tileP=32, order=work_order(R, ladder_tile(k)), seed=SEED, nthreads=4, **LADDER_FIRST)


def test_union_ladder_does_its_job():
    """At l1r = 1 the tile of a block of m items has a union list of exactly m items (m = 1: none)
    and active sets of m - 1, by G = R^T R and by the oracle; the solves sweep more than once, leave
    coefficients, and the warm start has a model to fold."""
    R, first = union_ladder()
    assert R.shape == (BLOCK_USERS * len(BLOCKS), sum(BLOCKS)) and R.data.min() == 1 and R.data.max() == 5
    assert float_form(R.shape[1]) == (8, 2) and packed_form(R.shape[1]) == (1, 0, 4)
    for k, m in enumerate(BLOCKS):
        tile = ladder_tile(k)
        for l1r in (LADDER_COLD["l1r"], LADDER_FIRST["l1r"]):
            (u,) = tile_unions(R, work_order(R, tile), l1r, False)
            assert u.size == (m if m > 1 else 0)
            assert u.size == 0 or (u.min() == first[k] and u.max() == first[k] + m - 1)
        for warm in (False, True):
            W, so, _ = ladder_oracle(k, warm)
            assert np.all(so["nacols"][tile] == m - 1)
            if m > 2:
                assert W[:, tile].nnz >= m and so["sweeps"][tile].max() > 1
        assert m <= 2 or ladder_first(k)[:, tile].nnz > 0


@pytest.mark.gpu
@pytest.mark.parametrize("m", BLOCKS)
def test_union_list_lengths(m):
    """One tile whose union list has exactly m items -- no batch at all, one visit, a batch of 63, a
    full one, one visit into the next, ..., eight batches and one visit -- in the three forms, cold
    and warm-started from the oracle's model at other penalties."""
    R = union_ladder()[0]
    k = BLOCKS.index(m)
    tile = ladder_tile(k)
    ncols = R.shape[1]
    chk = Checks()
    with stderr_of_the_library({"SLIM_GPU_KEEP_G": "1"}):
        dev = DeviceMatrix.from_scipy(R)
    try:
        every_form(chk, "union of %d, cold" % m, dev, ncols, tile, ladder_oracle(k), **LADDER_COLD)
        every_form(chk, "union of %d, warm" % m, dev, ncols, tile, ladder_oracle(k, True), imodel=ladder_first(k),
                   **LADDER_COLD)
    finally:
        dev.close()
    chk.done()


NBANDS, BAND, BAND_USERS = 8, 1024, 600
BANDED_KW = dict(l1r=0.5, l2r=1.0)


@functools.lru_cache(maxsize=None)
def banded():
    """8 bands of 1024 items; an item of band b has exactly 40 - 3 b users, drawn from the band's own
    600.  Binary.  Rank = id, so band b is the 1024 ranks whose g wavefront b of <1,0> holds:
    wavefront = ((rank >> 4) & 511) >> 6."""
    rng = np.random.default_rng(88)
    rows, ptr = [], [0]
    for j in range(NBANDS * BAND):
        b = j // BAND
        rows.append(np.sort(rng.choice(BAND_USERS, 40 - 3 * b, replace=False)) + b * BAND_USERS)
        ptr.append(ptr[-1] + rows[-1].size)
    rows = np.concatenate(rows)
    Rc = sp.csc_matrix((np.ones(rows.size, np.float32), rows, np.asarray(ptr)), shape=(NBANDS * BAND_USERS, NBANDS * BAND))
    return as_csr(Rc)


def banded_tile(t):
    """Tiles 0-7: 32 columns of band t (every coordinate of every batch in ONE wavefront's registers);
    tile 8: 4 columns of each band (the batches spread over all eight)."""
    if t < NBANDS:
        return np.arange(t * BAND + 100, t * BAND + 132, dtype=np.int32)
    return np.concatenate([np.arange(b * BAND + 500, b * BAND + 504) for b in range(NBANDS)]).astype(np.int32)


@functools.lru_cache(maxsize=None)
def banded_oracle(t, warm=False):
    R = banded()
    imodel = banded_oracle(t)[0] if warm else None
    W, so, _, obj = O.learn_cd_tile(R, tileP=32, order=work_order(R, banded_tile(t)), seed=SEED, nthreads=8, binary=True,
                                    imodel=imodel, return_stats=True, **(WARM if warm else BANDED_KW))
    return W, so, obj


def test_banded_fixture_does_its_job():
    """Rank = id; every coefficient of a band's tile lies in the band, those of the mixed tile in all
    eight; the tiles are not trivial."""
    R = banded()
    item_of, _, nnzc = popularity_order(R)
    assert np.array_equal(item_of, np.arange(NBANDS * BAND))
    assert np.array_equal(nnzc, np.repeat(40 - 3 * np.arange(NBANDS), BAND))
    assert float_form(R.shape[1]) == (16, 2) and packed_form(R.shape[1]) == (1, 0, 4)
    for t in range(NBANDS + 1):
        for warm in (False, True):
            W, so, _ = banded_oracle(t, warm)
            W = W.tocoo()
            wavefront = ((W.row[W.data != 0] >> 4) & 511) >> 6
            assert wavefront.size >= 500 and so["sweeps"].max() > 1
            if t < NBANDS:
                assert np.all(wavefront == t)
            else:
                assert set(wavefront) == set(range(NBANDS))


@pytest.mark.gpu
@pytest.mark.parametrize("t", range(NBANDS + 1))
def test_batches_of_one_wavefront_and_of_all(t):
    """<1,0>: a tile whose every visit reads a g that wavefront t exports, for each of the eight, and
    one whose batches take entries from all of them; float and packed, cold and warm."""
    R = banded()
    tile = banded_tile(t)
    ncols = R.shape[1]
    chk = Checks()
    with stderr_of_the_library({"SLIM_GPU_KEEP_G": "1"}):
        dev = DeviceMatrix.from_scipy(R, binary=True)
    try:
        every_form(chk, "tile %d, cold" % t, dev, ncols, tile, banded_oracle(t), **BANDED_KW)
        every_form(chk, "tile %d, warm" % t, dev, ncols, tile, banded_oracle(t, True), imodel=banded_oracle(t)[0], **WARM)
    finally:
        dev.close()
    chk.done()


# ---- the numbers above are the sources' ----------------------------------------------------------------
def test_boundaries_are_the_sources():
    """The item counts at which gram_geometry() and gramr_kernel() switch, read out of the C++."""
    def text(name):
        return open(os.path.join(CSRC, name)).read()
    hpp = text("gram_inst.hpp")
    static_lds = int(re.search(r"constexpr int kGramStaticLds = (\d+);", hpp).group(1))
    assert re.search(r"constexpr int kGramMaxColsPad = \(160 \* 1024 - kGramStaticLds\) / 4 / 64 \* 64;", hpp)
    max_pad = (160 * 1024 - static_lds) // 4 // 64 * 64
    geom = text("gram_inst.hip")
    steps = re.findall(r"if \(n4 <= (\d+) \* (\d+)\) \{ \*nw = (\d+); \*v = (\d+); \}", geom)
    last = re.search(r"else \{ \*nw = (\d+); \*v = (\d+); \}", geom)
    hbm = re.search(r"if \(ncols_pad > kGramMaxColsPad\) \{.*?\*nw = (\d+);.*?\*v = (\d+);", geom, re.S)
    forms = [(4 * int(a) * int(b), (int(nw), int(v))) for a, b, nw, v in steps]
    forms.append((max_pad, (int(last.group(1)), int(last.group(2)))))
    assert tuple(forms) == FLOAT_FORMS
    assert (int(hbm.group(1)), int(hbm.group(2))) == FLOAT_HBM
    assert "cd_gram_kernel<16, 0>" in geom and "cd_gram_kernel<8, 0>" in geom
    pack = text("gram_pack.hpp")
    nt = int(re.search(r"constexpr int kGramrNT = (\d+);", pack).group(1))
    group = int(re.search(r"constexpr int kPackGroup = (\d+);", pack).group(1))
    most = int(re.search(r"constexpr int kGramrMaxGroups = (\d+);", pack).group(1))
    assert group == GROUP == 16 * nt and most * group == PACKED_MAX
    inst = text("gramr_inst.hip")
    ks = [int(k) for k in re.findall(r"if \(k <= (\d+)\)", inst)] + [most]
    assert re.search(r"else if \(k <= kGramrMaxGroups\)", inst)
    krs = [int(k) for k in re.findall(r"\*kr = (\d+);", inst)]
    kl = int(re.search(r"\*kl = (\d+);\n", inst.split("kGramrMaxGroups)")[1]).group(1))
    assert [(k, kr) for k, kr in zip(ks, krs)] == [(k, f[0]) for k, f in PACKED_FORMS]
    assert kl == PACKED_FORMS[-1][1][1] and LDS_RANK0 == krs[-1] * group
    # every boundary has a case on either side
    for upto, _ in FLOAT_FORMS:
        assert upto in EDGE_SIZES and upto + 1 in EDGE_SIZES
        assert float_form(upto) != float_form(upto + 1)
    for groups, _ in PACKED_FORMS[:-1]:
        assert groups * GROUP in EDGE_SIZES and groups * GROUP + 1 in EDGE_SIZES
        assert packed_form(groups * GROUP) != packed_form(groups * GROUP + 1)
    assert PACKED_MAX in LARGE_SIZES and PACKED_MAX + 1 in LARGE_SIZES and packed_form(PACKED_MAX + 1) is None
    assert LDS_RANK0 in LARGE_SIZES and LDS_RANK0 + 16 in LARGE_SIZES
