"""Fixtures and checks of test_carried_g.py: matrices on which every carrying form of the packed
item-space kernel solves ALL columns in a few seconds, the oracle's own warm chains over a few
tiles of such a solve, and the two verdicts on stats["gram_rows"] -- "carried" and "folded".

A row of G is read once for the set-up of a column, once per kept coefficient of the previous model
for the fold (cd.c:108-110 in item space) and once per coefficient a sweep moves.  A step that starts
from the carried g (cd_gramr.hpp: g_load) reads neither the set-up row nor a fold row, so against the
same step folded it saves more than 0.9 x nnz(previous model) rows; a step that folds reads what the
folded control reads."""
import functools

import numpy as np
import scipy.sparse as sp

import slim_oracle as O
from library_output import stderr_of_the_library
from slim_amd.engine import KERNEL_GRAM, DeviceMatrix, model_to_scipy
from test_item_space_forms import (SEED, TRACE, Checks, as_csr, maxdiff, modes, plant_last_rank,
                                   popularity_order, random_binary, work_order)
from test_resident_model import free, same_model

# (l1r, l2r): cold, then l2 moves twice (carried), l1 moves (folds), l2 moves (carried).  Binary with
# ~20 ratings a column: G > 0.5 is "co-rated", so 0.5 and 0.3 select the same active sets.
CHAIN = ((0.5, 1.0), (0.5, 3.0), (0.5, 0.3), (0.3, 0.3), (0.3, 2.0))
CARRIED = (1, 2, 4)
# the nine l2 values of tests/golden/l12file for l1 = 0.5 in file order, then back in one step
L2_OF_THE_GRID = (0.1, 0.5, 1.0, 2.0, 3.0, 4.0, 5.0, 7.5, 10.0)
LONG_CHAIN = tuple((0.5, l2) for l2 in L2_OF_THE_GRID) + ((0.5, 0.1),)
LONG_KW = dict(optTol=1e-10)

# items -> (form, groups of 8192 ranks in use, users): ~20 ratings a column everywhere; the users grow
# with the items so that a row holds ~10 ratings and a column ~200 co-rated items -- ALL columns are
# solved (nothing else can carry), and at 2000 users a model of 24 577 items would hold 10^8 coefficients
SIZES = {17: ((1, 0, 4), 1, 2000), 8192: ((1, 0, 4), 1, 16000), 8193: ((3, 0, 4), 2, 16000),
         24577: ((6, 0, 2), 4, 48000)}
BINARY, RATED, RATED_HOT = 0, 1, 2
HOT = 3   # RATED_HOT: that many items rated 4 or 5 by 60 % of the users, G between them >= 65 536


@functools.lru_cache(maxsize=None)
def grid(ncols, kind=BINARY):
    """(R, the planted item's partner c, the planted item).  No empty column; the item of the last
    rank is co-rated with c (plant_last_rank): the item of the middle rank, below 2048 items the most
    popular one.  RATED: the same pattern with integer ratings 1-5.  RATED_HOT: HOT more-than-popular
    items besides, so that rows of G hold entries beyond 65 535 (the hi2 plane)."""
    users = SIZES[ncols][2]
    rng = np.random.default_rng(4000 + ncols)
    Rc = random_binary(users, ncols, 20.0 / users, rng)
    if kind == RATED_HOT:
        raters = [np.flatnonzero(rng.random(users) < 0.6) for _ in range(HOT)]
        hot = sp.csc_matrix((np.ones(sum(r.size for r in raters), np.float32),
                             (np.concatenate(raters), np.repeat(np.arange(HOT), [r.size for r in raters]))), shape=Rc.shape)
        Rc = sp.csc_matrix((Rc + hot) > 0, dtype=np.float32)
        Rc.sort_indices()
    item_of = popularity_order(Rc)[0]
    c = int(item_of[ncols // 2] if ncols >= 2048 else item_of[0])
    last = plant_last_rank(Rc, c, rng)
    if kind != BINARY:
        Rc.data[:] = rng.integers(1, 6, Rc.nnz).astype(np.float32)
    if kind == RATED_HOT:
        for h in range(HOT):
            Rc.data[Rc.indptr[h]:Rc.indptr[h + 1]] = rng.integers(4, 6, Rc.indptr[h + 1] - Rc.indptr[h])
    return as_csr(Rc), c, last


@functools.lru_cache(maxsize=None)
def walked(ncols, kind=BINARY):
    """(the work list of an all-column solve, the tiles the oracle walks, their columns): the first
    tile, the median, the last, and the one holding the planted item's partner."""
    R, c, _ = grid(ncols, kind)
    order = work_order(R)
    ntiles = (ncols + 31) // 32
    tiles = sorted({0, ntiles // 2, ntiles - 1, int(np.flatnonzero(order == c)[0]) // 32})
    cols = np.concatenate([order[32 * k:32 * k + 32] for k in tiles])
    return order, tiles, cols


def oracle_walk(R, order, tiles, binary, imodel, **kw):
    """(W, column stats) of O.learn_cd_tile over `tiles` of the work list, each keyed by its position."""
    W, so = None, None
    for k in tiles:
        Wk, sk, _, _ = O.learn_cd_tile(R, tileP=32, order=order, tiles=(k, 1), seed=SEED, nthreads=8, binary=binary,
                                       imodel=imodel, return_stats=True, **kw)
        cols = order[32 * k:32 * k + 32]
        W = Wk if W is None else W + Wk
        so = sk.copy() if so is None else so
        so[cols] = sk[cols]
    return sp.csc_matrix(W), so


@functools.lru_cache(maxsize=None)
def oracle_chain(ncols, kind=BINARY, chain=CHAIN, maxniters=10000, optTol=1e-7):
    """[(W, column stats)] along `chain`: every step from the oracle's OWN previous model (estimate.c:
    453-464, cd.c:108-110 -- the fold a carried step skips), over the walked tiles only."""
    R, _, _ = grid(ncols, kind)
    order, tiles, _ = walked(ncols, kind)
    out, prev = [], None
    for l1, l2 in chain:
        W, so = oracle_walk(R, order, tiles, kind == BINARY, prev, l1r=l1, l2r=l2, maxniters=maxniters, optTol=optTol)
        out.append((W, so))
        prev = W
    return out


def last_chunk_in_use(ncols):
    """The ranks of the last chunk of 16 of the last group in use."""
    return np.arange((ncols - 1) // 16 * 16, ncols)


def packed_modes(ncols):
    """[(environment, trace text, short name)] of every packed mode of the size: register loads and
    the ring, <3,0> also with 256 VGPRs."""
    return [(env, expect, expect[7:] if expect.startswith("packed ") else expect) for env, expect in modes(ncols, keep_g=False)]


# ---- the device's side ---------------------------------------------------------------------------------
def bit_equal(lib, ha, hb):
    """Two host model handles hold the same views: offsets, ids and values."""
    try:
        same_model(lib, ha, hb)
        return True
    except AssertionError:
        return False


def run_chain(m, env, expect, chain, **kw):
    """The chain on handle `m`, every step a resident all-column solve warm-started from the one
    before, the previous model freed after the next solve returned (the grid loop's order) ->
    [(W, stats, column stats)].  The trace line of every step must read `expect`.
    A step that moves l1 must fold, and what a fold gives depends on the model it folds: the NO_CARRY
    chain arrives there with a model a rounding apart, and reads a handful of rows more or fewer.  The
    control of such a step is therefore the host warm start from THIS chain's previous model
    (SLIMGPU_Learn: it folds, always), run right after it: stats["refold"] = (its gram_rows, whether
    its model is this step's bit for bit, whether sweeps and D are equal)."""
    out, prev, prev_h = [], None, None
    lib = m._lib
    try:
        for k, (l1, l2) in enumerate(chain):
            opts = dict(kernel=KERNEL_GRAM, seed=SEED, l1r=l1, l2r=l2, **kw)
            with stderr_of_the_library(dict(env, SLIM_GPU_TRACE="1")) as err:
                cur, st = m.learn_resident(warm=prev, **opts)
                cs = m.column_stats()
            got = TRACE.findall(err[0])
            assert st["kernel"] == KERNEL_GRAM and got == [expect], (got, expect)
            cur_h = cur.fetch(return_handle=True)
            if k and l1 != chain[k - 1][0] and "SLIM_GPU_NO_CARRY" not in env:
                with stderr_of_the_library(dict(env)):
                    h, sh = m.learn(imodel=prev_h, return_handle=True, **opts)
                st["refold"] = (sh["gram_rows"], bit_equal(lib, h, cur_h), st["sweeps"] == sh["sweeps"] and st["D"] == sh["D"])
                free(lib, h)
            out.append((model_to_scipy(lib, cur_h, free=False), st, cs))
            if prev is not None:
                prev.free()
                free(lib, prev_h)
            prev, prev_h = cur, cur_h
    finally:
        if prev is not None:
            prev.free()
            free(lib, prev_h)
    return out


NO_CARRY = {"SLIM_GPU_NO_CARRY": "1"}


class ChainChecks(Checks):
    """Checks plus the verdicts on a step of a chain."""

    def step_against_oracle(self, tag, run, oracle, cols, tol=5e-5, sweeps=0.95, l2_only=False):
        W, st, cs = run
        Wo, so = oracle
        d = maxdiff(W[:, cols], Wo[:, cols])
        same = float((cs.sweeps[cols] == so["sweeps"][cols]).mean())
        nac = bool(np.array_equal(cs.nacols[cols], so["nacols"][cols]))
        top, top_o = int(cs.sweeps[cols].max()), int(so["sweeps"][cols].max())
        print("%s: maxdiff %.3e, nacols equal %s, sweeps equal %.4f, most sweeps %d (oracle %d), nnz %d (oracle %d)"
              % (tag, d, nac, same, top, top_o, W[:, cols].nnz, Wo[:, cols].nnz))
        self.that(W.shape == Wo.shape, "%s: shape %s against %s" % (tag, W.shape, Wo.shape))
        self.that(d <= tol, "%s: maxdiff %.3e > %.0e" % (tag, d, tol))
        self.that(nac, "%s: nacols differ" % tag)
        if sweeps is not None:
            self.that(same >= sweeps, "%s: sweeps equal on %.4f < %.2f" % (tag, same, sweeps))
        if l2_only:
            self.that(top <= top_o, "%s: %d sweeps, the oracle's l2 step takes %d at most" % (tag, top, top_o))
        return d

    def carried(self, tag, rows, control_rows, prev_nnz):
        bound = control_rows - int(0.9 * prev_nnz)
        print("%s: gram_rows %d, folded control %d, previous model %d coefficients: carried needs <= %d"
              % (tag, rows, control_rows, prev_nnz, bound))
        self.that(rows <= bound, "%s: not carried: gram_rows %d > %d" % (tag, rows, bound))

    def folded(self, tag, rows, control_rows):
        print("%s: gram_rows %d, folded control %d: folded needs them equal" % (tag, rows, control_rows))
        self.that(rows == control_rows, "%s: gram_rows %d, the folded control's %d" % (tag, rows, control_rows))

    def chain_rows(self, tag, runs, control, carried=CARRIED):
        """Which steps of a chain carried, by the rows of G they read against the folded control's."""
        for k, ((_, st, _), (_, sf, _)) in enumerate(zip(runs, control)):
            if k in carried:
                self.carried("%s, step %d" % (tag, k), st["gram_rows"], sf["gram_rows"], control[k - 1][0].nnz)
            elif "refold" in st:     # l1 moved: against the host warm start from this chain's own previous model
                rows, same, counts = st["refold"]
                print("%s, step %d: the host warm start's model bit for bit %s, its sweeps and D %s" % (tag, k, same, counts))
                self.that(same and counts, "%s, step %d: not the host warm start from its own previous model" % (tag, k))
                self.folded("%s, step %d" % (tag, k), st["gram_rows"], rows)
            else:
                self.that(k == 0, "%s, step %d: a warm step without a control of its own" % (tag, k))
                self.folded("%s, step %d" % (tag, k), st["gram_rows"], sf["gram_rows"])


def chains_of_every_mode(chk, tag, ncols, kind, chain, oracle, tol=5e-5, **kw):
    """One handle, one chain per packed mode and one folded control chain: each step of each against the
    oracle's chain on the walked tiles and by its gram_rows, the modes EQUAL to the first at every
    step.  -> ({name: runs}, control, the handle's byte planes with RATED_HOT)"""
    R = grid(ncols, kind)[0]
    cols = walked(ncols, kind)[2]
    carried = [k for k in range(1, len(chain)) if chain[k][0] == chain[k - 1][0]]
    m = DeviceMatrix.from_scipy(R, binary=kind == BINARY)
    try:
        forms = packed_modes(ncols)
        control = run_chain(m, dict(forms[0][0], **NO_CARRY), forms[0][1], chain, **kw)
        runs = {name: run_chain(m, env, expect, chain, **kw) for env, expect, name in forms}
        planes = m.gram_planes() if kind == RATED_HOT else None
    finally:
        m.close()
    for name, rs in [("folded control", control)] + list(runs.items()):
        for k, (run, orc) in enumerate(zip(rs, oracle)):
            chk.step_against_oracle("%s, %s, step %d %s" % (tag, name, k, chain[k]), run, orc, cols, tol=tol,
                                    l2_only=k in carried)
        if rs is not control:
            chk.chain_rows("%s, %s" % (tag, name), rs, control, carried)
    names = list(runs)
    for k in range(len(chain)):
        chk.forms_equal("%s, step %d" % (tag, k), [runs[n][k] for n in names], names)
    return runs, control, planes


def kkt(R, W, cols, l1, l2, binary):
    """(max |a_i.(y - Ax) - l2 x_i - l1| over x_i > 0, max of a_i.(y - Ax) - l1 over x_i = 0, i != iC)
    of the columns `cols` of W, in fp64 from R: the optimality conditions of the elastic-net NNLS."""
    A = sp.csc_matrix(R, dtype=np.float64)
    if binary:
        A.data[:] = 1.0
    X = np.asarray(W[:, cols].todense(), dtype=np.float64)
    grad = np.asarray(A.T @ (A[:, cols].toarray() - A @ X))   # [i, k] = a_i . (y_k - A x_k)
    pos = X > 0
    off = ~pos
    off[cols, np.arange(len(cols))] = False
    assert X.min() >= 0 and not pos[cols, np.arange(len(cols))].any()
    return float(np.abs(grad - l2 * X - l1)[pos].max()), float((grad - l1)[off].max())
