"""The g that resident grid chains carry from solve to solve (cd_gramr.hpp: g_save / g_load; engine.hip:
learn_plan decides whose buffer it is and whether it may be read) -- the only solver state that
survives a call and is never recomputed.  A stale or misplaced g does not crash: it gives a model
that is a little wrong.  So every form that carries, and every transition of the buffer's ownership,
is held against something that is NOT the carry:

  1. <1,0> (17 and 8192 items), <3,0> (8193: two groups in use, a slot of three) and <6,0> (24 577:
     four in use, a slot of six), register loads and ring, <3,0> also with 256 VGPRs, binary and with
     ratings 1-5 (hi and hi2 planes), converged and capped at one and two sweeps: every step of a
     five-step chain against the fp64 oracle warm-started from ITS previous model, and the modes of
     one size EQUAL to each other at every step;
  2. the nine l2 values of the grid's l1 row and one step back, nine carried steps in a row: the
     oracle's chain at every step, and the KKT conditions of the last model from R in fp64;
  3. the transitions: wherever the engine must fold, the host warm start's model bit for bit
     (test_resident_model_is_the_host_model_cold_and_warm pins that fold as SLIM_Learn's);
  4. a carried step that overflows its arena and is solved again, and the step after it.

Whether a step carried is read off stats["gram_rows"] (carried_g_cases.py).  Every comparison of a test
is made and printed before the test fails on any of them."""
import functools
import os

import numpy as np
import pytest
import scipy.sparse as sp

import slim_oracle as O
from carried_g_cases import (BINARY, CHAIN, HOT, LONG_CHAIN, LONG_KW, NO_CARRY, RATED, RATED_HOT, SIZES,
                             ChainChecks, bit_equal, chains_of_every_mode, grid, kkt, last_chunk_in_use, oracle_chain, packed_modes,
                             run_chain, walked)
from library_output import stderr_of_the_library
from slim_amd.engine import KERNEL_GRAM, KERNEL_TILE, DeviceMatrix, model_to_scipy
from test_item_space_forms import GROUP, SEED, maxdiff, packed_form, popularity_order
from test_resident_model import free, ratings, views


@pytest.fixture(autouse=True)
def _the_carry_is_on(monkeypatch):
    for k in ("SLIM_GPU_NO_CARRY", "SLIM_GPU_ARENA", "SLIM_GPU_GRAMR_DMA", "SLIM_GPU_GRAMR_WPS", "SLIM_GPU_NO_GRAMR"):
        monkeypatch.delenv(k, raising=False)


# ---- 1. every carrying form against the oracle -------------------------------------------------------
FORM_CASES = [(n, BINARY) for n in sorted(SIZES)] + [(8193, RATED_HOT)]
CAPS = (1, 2)


def moved(chain_models, k):
    return maxdiff(chain_models[k][0], chain_models[k - 1][0])


def check_fixture(ncols, kind, chain, oracle):
    """What every fixture of this file must show: no empty column, the expected form, and along the
    oracle's chain non-empty models with a coefficient on the last chunk in use, every step that
    moves l2 alone moving a coefficient by more than 1e-3 (so that no carried step is trivially right)."""
    R, c, last = grid(ncols, kind)
    order, tiles, cols = walked(ncols, kind)
    item_of, rank_of, nnzc = popularity_order(R)
    assert R.shape == (SIZES[ncols][2], ncols) and nnzc.min() >= 1 and item_of[-1] == last
    assert packed_form(ncols) == SIZES[ncols][0] and (ncols + GROUP - 1) // GROUP == SIZES[ncols][1]
    assert (R.data == 1.0).all() if kind == BINARY else set(np.unique(R.data)) == {1.0, 2.0, 3.0, 4.0, 5.0}
    assert c in cols and len(set(cols)) == len(cols) == sum(min(32, ncols - 32 * k) for k in tiles)
    lastc = set(item_of[last_chunk_in_use(ncols)])
    for k, (W, so) in enumerate(oracle):
        Wc = W.tocoo()
        assert Wc.nnz > 0 and W[:, cols].nnz == W.nnz, k
        assert lastc & set(Wc.row[Wc.data != 0]), "step %d: no coefficient on the last chunk in use" % k
        if k and chain[k][0] == chain[k - 1][0]:
            assert moved(oracle, k) > 1e-3, k
    return R, rank_of, cols


@pytest.mark.parametrize("ncols,kind", FORM_CASES)
def test_form_fixtures_do_their_job(ncols, kind):
    """check_fixture's properties; with RATED_HOT besides: the HOT items hold the first ranks, are
    columns of the first walked tile and co-rated with columns of it (on its union list: their rows
    of G are read), and G between them exceeds 65 535 -- those rows have a hi2 plane."""
    R, rank_of, cols = check_fixture(ncols, kind, CHAIN, oracle_chain(ncols, kind))
    if kind == RATED_HOT:
        hot = np.arange(HOT)
        G = np.asarray((R[:, hot].T @ R).todense(), dtype=np.float64)
        assert sorted(rank_of[hot]) == list(range(HOT)) and set(hot) <= set(cols[:32])
        assert (G[:, hot][~np.eye(HOT, dtype=bool)] >= 65536).all()
        assert (G[:, cols[:32]] > 0.5).any(axis=1).all()


@pytest.mark.parametrize("n", CAPS)
def test_capped_fixture_does_its_job(n):
    oracle = oracle_chain(17, BINARY, CHAIN, maxniters=n)
    check_fixture(17, BINARY, CHAIN, oracle)
    full = oracle_chain(17)
    stopped = [int((so["conv"][so["nacols"] > 0] == 0).sum()) for _, so in oracle]
    print("columns stopped by the cap of %d, per step: %s" % (n, stopped))
    assert stopped[0] > 0 and any(stopped[1:]), "the cap stops no solve that hands its g on"
    assert any(maxdiff(W, Wf) > 0 for (W, _), (Wf, _) in zip(oracle, full)), "the cap changes nothing"


@pytest.mark.gpu
@pytest.mark.timeout(120, method="thread")
@pytest.mark.parametrize("ncols,kind", FORM_CASES)
def test_every_carrying_form_along_a_chain(ncols, kind):
    """CHAIN through every packed mode of the size, all columns solved, steps 1, 2 and 4 from the
    carried g: per step and walked tile max |dW| <= 5e-5 against the oracle's own warm chain, equal
    nacols, >= 95 % equal sweep counts, a carried step within the oracle's sweep counts, and carried
    / folded by gram_rows; the modes EQUAL at every step (a g that came back in another thread's place
    breaks that at once).  Step 3 moves l1 and must fold: it is the host warm start from the chain's
    own step-2 model bit for bit, with its gram_rows (carried_g_cases.run_chain says why the NO_CARRY
    chain is no control for it: it differed by 2 to 138 rows of 10^2 ... 10^7).  With ratings the rows
    of the HOT items hold a hi2 plane.  Measured on an MI355X: max |dW| 1.8e-7 binary, 3.9e-6 with
    ratings, every sweep count the oracle's, every mode equal to the first at every step."""
    chk = ChainChecks()
    tag = "%d items%s" % (ncols, "" if kind == BINARY else ", ratings 1-5")
    _, _, planes = chains_of_every_mode(chk, tag, ncols, kind, CHAIN, oracle_chain(ncols, kind))
    if kind == RATED_HOT:
        print("%s: hi_k %s, hi2_k %s of the hot rows" % (tag, planes["hi_k"][:HOT], planes["hi2_k"][:HOT]))
        chk.that((planes["hi2_k"][:HOT] >= 1).all() and (planes["hi_k"][:HOT] >= 1).all(), "no hi2 plane on the hot rows")
    chk.done()


@pytest.mark.gpu
@pytest.mark.parametrize("n", CAPS)
def test_capped_sweeps_leave_their_own_g(n):
    """The chain at 17 items with every solve stopped after n sweeps: the g a solve leaves when it has
    not converged is still that solve's, so the next step is the oracle's capped warm step."""
    chk = ChainChecks()
    chains_of_every_mode(chk, "17 items, %d sweeps" % n, 17, BINARY, CHAIN, oracle_chain(17, BINARY, CHAIN, maxniters=n),
                         niters=n)
    chk.done()


# ---- 2. nine carried steps in a row ------------------------------------------------------------------
LONG = 8193
LONG_CASES = [(BINARY, 2e-5), (RATED, 5e-5)]


@pytest.mark.parametrize("kind,tol", LONG_CASES)
def test_long_chain_fixture_does_its_job(kind, tol):
    assert LONG_CHAIN[:9] == tuple((0.5, l2) for l2 in (0.1, 0.5, 1.0, 2.0, 3.0, 4.0, 5.0, 7.5, 10.0))
    assert LONG_CHAIN[9] == (0.5, 0.1) and len(LONG_CHAIN) == 10
    pairs = [tuple(map(float, ln.split())) for ln in open(os.path.join(os.path.dirname(__file__), "golden", "l12file")) if ln.strip()]
    assert [p for p in pairs if p[0] == 0.5] == list(LONG_CHAIN[:9])
    oracle = oracle_chain(LONG, kind, LONG_CHAIN, **LONG_KW)
    check_fixture(LONG, kind, LONG_CHAIN, oracle)
    assert moved(oracle, 9) > 0.05      # the step back moves coefficients a long way


@pytest.mark.gpu
@pytest.mark.timeout(120, method="thread")
@pytest.mark.parametrize("kind,tol", LONG_CASES)
def test_nine_carried_steps_in_a_row(kind, tol):
    """LONG_CHAIN at 8193 items (<3,0>, register loads), optTol 1e-10, each step's fp32 g handed to the
    next nine times over.  Two references, neither of them the carry: the oracle's own warm chain,
    max |dW| <= 2e-5 (5e-5 with ratings) at EVERY step; and the KKT conditions of the last model
    (l2 > 0: the minimiser is unique, no trajectory enters) from R in fp64 on the walked columns,
    <= 2e-3.  Each figure is printed beside the folded control chain's, which must pass both itself.
    The sweep share is 90 % here, the forms suite's figure at this optTol.
    Measured on an MI355X, carried (folded control): max |dW| per step 5.6e-8 ... 7.7e-7 at the step
    back (3.7e-8 ... 3.3e-7), with ratings <= 6.0e-8 (<= 2.4e-7): no growth along the chain; KKT on the
    kept coefficients 1.7e-5 (1.7e-5), with ratings 4.4e-4 (4.3e-4); on the zero ones the gradient
    stays 4e-4 and 7e-4 BELOW l1."""
    chk = ChainChecks()
    R = grid(LONG, kind)[0]
    cols = walked(LONG, kind)[2]
    oracle = oracle_chain(LONG, kind, LONG_CHAIN, **LONG_KW)
    env, expect, _ = packed_modes(LONG)[0]
    assert expect == "packed <3,0>, register loads, WPS 4"
    m = DeviceMatrix.from_scipy(R, binary=kind == BINARY)
    try:
        control = run_chain(m, dict(env, **NO_CARRY), expect, LONG_CHAIN, **LONG_KW)
        runs = run_chain(m, env, expect, LONG_CHAIN, **LONG_KW)
    finally:
        m.close()
    tag = "ten steps%s" % ("" if kind == BINARY else ", ratings 1-5")
    for k in range(len(LONG_CHAIN)):
        t = "%s, step %d %s" % (tag, k, LONG_CHAIN[k])
        df = chk.step_against_oracle(t + ", folded control", control[k], oracle[k], cols, tol=tol, sweeps=0.9)
        dc = chk.step_against_oracle(t + ", carried", runs[k], oracle[k], cols, tol=tol, sweeps=0.9)
        print("%s: max |dW| against the oracle: carried %.3e, folded %.3e" % (t, dc, df))
    chk.chain_rows(tag, runs, control, carried=range(1, len(LONG_CHAIN)))
    l1, l2 = LONG_CHAIN[-1]
    (pc, zc), (pf, zf) = (kkt(R, rs[-1][0], cols, l1, l2, kind == BINARY) for rs in (runs, control))
    print("%s: KKT of the last model: |grad - l2 x - l1| on x > 0: carried %.3e, folded %.3e; grad - l1 on x = 0: "
          "carried %.3e, folded %.3e" % (tag, pc, pf, zc, zf))
    for name, p, z in (("carried", pc, zc), ("folded control", pf, zf)):
        chk.that(p <= 2e-3, "%s, %s: KKT on the kept coefficients %.3e > 2e-3" % (tag, name, p))
        chk.that(z <= 2e-3, "%s, %s: KKT on the zero coefficients %.3e > 2e-3" % (tag, name, z))
    chk.done()


# ---- 3. transitions of ownership ---------------------------------------------------------------------
SMALL_SHAPE = (30000, 700, 0.01)        # (test_g_carried_from_pair_to_pair_gives_the_folded_models' matrix)
SMALL_KW = dict(optTol=1e-7, niters=300, seed=SEED, kernel=KERNEL_GRAM)
A_PAIR = (1.0, 10.0)    # ~300 ratings a column (l2 far below that moves nothing), ~3 co-ratings a pair
TIGHT_KW = dict(optTol=1e-11, niters=2000, seed=SEED, kernel=KERNEL_GRAM)
ARENA_CHAIN = (A_PAIR, (1.0, 300.0), (1.0, 30.0))


@functools.lru_cache(maxsize=None)
def small_R(seed=21):
    return ratings(*SMALL_SHAPE, seed=seed, binary=True)


@functools.lru_cache(maxsize=None)
def small_oracle(chain, optTol, maxniters):
    """[(W, column stats)] of the oracle's walk over every tile of the small matrix along `chain`."""
    out, prev = [], None
    for l1, l2 in chain:
        W, so, _, _ = O.learn_cd_tile(small_R(), tileP=32, seed=SEED, nthreads=8, binary=True, imodel=prev, l1r=l1, l2r=l2,
                                      optTol=optTol, maxniters=maxniters, return_stats=True)
        out.append((sp.csc_matrix(W), so))
        prev = W
    return out


def test_small_fixtures_do_their_job():
    """700 items: <1,0>; the oracle's models along the chains of parts 3 and 4 are non-empty and every
    l2 step moves a coefficient by more than 1e-3; the second matrix differs from the first."""
    assert packed_form(SMALL_SHAPE[1]) == (1, 0, 4)
    assert abs(small_R(21) - small_R(22)).nnz > 0 and small_R(21).shape == small_R(22).shape
    for chain, tol, it in (((A_PAIR, (1.0, 300.0)), 1e-7, 300), (ARENA_CHAIN, 1e-11, 2000)):
        oracle = small_oracle(chain, tol, it)
        for k, (W, so) in enumerate(oracle):
            assert W.nnz > 10000 and so["sweeps"].max() < it
            assert k == 0 or moved(oracle, k) > 1e-3


class Small(object):
    """The small matrix on the device, and every handle and model made on the way (freed by close())."""

    def __init__(self, seed=21):
        self.R = small_R(seed)
        self.mat = DeviceMatrix.from_scipy(self.R, binary=True)
        self.lib = self.mat._lib
        self.handles, self.models = [], []

    def resident(self, warm, pair, env=None, **kw):
        with stderr_of_the_library(dict(env or {})):
            d, st = self.mat.learn_resident(warm=warm, l1r=pair[0], l2r=pair[1], **dict(SMALL_KW, **kw))
        self.models.append(d)
        return d, st

    def fetched(self, d):
        self.handles.append(d.fetch(return_handle=True))
        return self.handles[-1]

    def host(self, imodel, pair, **kw):
        """The yardstick: SLIMGPU_Learn warm-started from a host handle -- it folds, always."""
        h, st = self.mat.learn(imodel=imodel, return_handle=True, l1r=pair[0], l2r=pair[1], **dict(SMALL_KW, **kw))
        self.handles.append(h)
        return h, st

    def scipy(self, h):
        return model_to_scipy(self.lib, h, free=False)

    def close(self):
        for h in self.handles:
            free(self.lib, h)
        for d in self.models:
            d.free()
        self.mat.close()


def must_fold(chk, tag, s, d, st, warm_h, pair, **kw):
    """The resident model d of a step from `warm_h`'s model is the host warm start's, bit for bit, with
    its sweeps, D and gram_rows."""
    h, sh = s.host(warm_h, pair, **kw)
    eq = bit_equal(s.lib, h, s.fetched(d))
    print("%s: equal to the host warm start bit for bit %s, sweeps %d / %d, D %d / %d"
          % (tag, eq, st["sweeps"], sh["sweeps"], st["D"], sh["D"]))
    chk.that(eq, "%s: not the host warm start's model" % tag)
    chk.that(st["sweeps"] == sh["sweeps"] and st["D"] == sh["D"], "%s: sweeps or D differ from the host warm start's" % tag)
    chk.folded(tag, st["gram_rows"], sh["gram_rows"])


def must_carry(chk, tag, s, d, st, warm_h, pair, tol=2e-5, **kw):
    """The step read no fold rows (against the host warm start, which folds), and its model is the
    folded one to the parity tolerance with the sweep counts within 1 %."""
    h, sh = s.host(warm_h, pair, **kw)
    dW = maxdiff(d.fetch(), s.scipy(h))
    print("%s: maxdiff to the host warm start %.3e, sweeps %d / %d" % (tag, dW, st["sweeps"], sh["sweeps"]))
    chk.carried(tag, st["gram_rows"], sh["gram_rows"], s.scipy(warm_h).nnz)
    chk.that(dW <= tol, "%s: maxdiff to the folded model %.3e > %.0e" % (tag, dW, tol))
    chk.that(abs(st["sweeps"] - sh["sweeps"]) <= 0.01 * sh["sweeps"], "%s: sweeps %d against %d" % (tag, st["sweeps"], sh["sweeps"]))


@pytest.fixture
def small():
    made = []

    def make(seed=21):
        made.append(Small(seed))
        return made[-1]
    yield make
    for s in made:
        s.close()


@pytest.mark.gpu
def test_a_warm_model_used_twice_carries_once(small):
    """A -> C moves l2: carried, and A's buffer goes to C.  A -> D moves l2 again: A has no g any
    more, D folds.  C -> E: carried."""
    chk, s = ChainChecks(), small()
    A, _ = s.resident(None, A_PAIR)            # (cold: the same with and without the carry)
    hA = s.fetched(A)
    C_, st = s.resident(A, (1.0, 300.0))
    must_carry(chk, "A -> C", s, C_, st, hA, (1.0, 300.0))
    D, st = s.resident(A, (1.0, 30.0))
    must_fold(chk, "A -> D, A's g gone", s, D, st, hA, (1.0, 30.0))
    E, st = s.resident(C_, (1.0, 30.0))
    must_carry(chk, "C -> E", s, E, st, s.fetched(C_), (1.0, 30.0))
    chk.done()


@pytest.mark.gpu
def test_a_model_of_another_matrix_folds(small):
    """A model learned on another handle of the same shape holds the g of other ratings: the step
    folds; and on its own handle that model still carries afterwards."""
    chk, s, other = ChainChecks(), small(21), small(22)
    A2, _ = other.resident(None, A_PAIR)
    hA2 = other.fetched(A2)
    B, st = s.resident(A2, (1.0, 300.0))
    must_fold(chk, "another handle's model", s, B, st, hA2, (1.0, 300.0))
    C2, st = other.resident(A2, (1.0, 300.0))
    must_carry(chk, "that model on its own handle", other, C2, st, hA2, (1.0, 300.0))
    chk.done()


@pytest.mark.gpu
def test_an_uploaded_model_folds(small):
    chk, s = ChainChecks(), small()
    A, _ = s.resident(None, A_PAIR)
    up = s.mat.model_from_scipy(A.fetch())
    s.models.append(up)
    B, st = s.resident(up, (1.0, 300.0))
    must_fold(chk, "an uploaded model", s, B, st, s.fetched(A), (1.0, 300.0))
    chk.done()


@pytest.mark.gpu
def test_a_moved_l1_folds(small):
    """l1 moves (and l2 with it or not): the active sets change, the g of the other l1 is no start."""
    chk, s = ChainChecks(), small()
    A, _ = s.resident(None, A_PAIR)
    hA = s.fetched(A)
    B, st = s.resident(A, (2.0, 10.0))
    must_fold(chk, "l1 moved", s, B, st, hA, (2.0, 10.0))
    A2, _ = s.resident(None, A_PAIR)
    B2, st = s.resident(A2, (2.0, 300.0))
    must_fold(chk, "l1 and l2 moved", s, B2, st, hA, (2.0, 300.0))
    # (B took A's buffer and wrote its own g at l1 = 2: the next l2 step carries from it)
    C_, st = s.resident(B, (2.0, 300.0))
    must_carry(chk, "the l2 step after it", s, C_, st, s.fetched(B), (2.0, 300.0))
    chk.done()


@pytest.mark.gpu
def test_a_step_without_the_carry_between_two_others(small):
    """A -> B under SLIM_GPU_NO_CARRY=1 -> C with the switch off again: B folds and leaves no g, so C
    folds too."""
    chk, s = ChainChecks(), small()
    A, _ = s.resident(None, A_PAIR)
    B, st = s.resident(A, (1.0, 300.0), env=NO_CARRY)
    must_fold(chk, "the step under NO_CARRY", s, B, st, s.fetched(A), (1.0, 300.0))
    C_, st = s.resident(B, (1.0, 30.0))
    must_fold(chk, "the step after it", s, C_, st, s.fetched(B), (1.0, 30.0))
    chk.done()


@pytest.mark.gpu
def test_a_step_on_another_kernel_between_two_others(small):
    """A -> B on the tile kernel: nothing carries and A keeps its buffer.  A -> C on the packed kernel
    with l2 moved then carries from A: by gram_rows, and C is the oracle's warm step."""
    chk, s = ChainChecks(), small()
    chain = (A_PAIR, (1.0, 300.0))
    oracle = small_oracle(chain, SMALL_KW["optTol"], SMALL_KW["niters"])
    A, st = s.resident(None, A_PAIR)
    every = np.arange(s.mat.ncols)
    chk.step_against_oracle("A, cold", (A.fetch(), st, s.mat.column_stats()), oracle[0], every)
    hA = s.fetched(A)
    B, st = s.resident(A, (1.0, 30.0), kernel=KERNEL_TILE)
    chk.that(st["kernel"] == KERNEL_TILE, "the middle step ran kernel %d" % st["kernel"])
    hB, _ = s.host(hA, (1.0, 30.0), kernel=KERNEL_TILE)
    chk.that(bit_equal(s.lib, hB, s.fetched(B)), "the tile kernel's step is not the host warm start's")
    C_, st = s.resident(A, (1.0, 300.0))
    cs = s.mat.column_stats()
    chk.step_against_oracle("A -> C after the tile kernel", (C_.fetch(), st, cs), oracle[1], every, l2_only=True)
    must_carry(chk, "A -> C after the tile kernel", s, C_, st, hA, (1.0, 300.0))
    chk.done()


@pytest.mark.gpu
def test_a_fetch_begun_before_the_solve_that_takes_the_buffer(small):
    """fetch_begin() on the warm model copies beside the carried solve that moves its g away: the
    fetched model is a second fetch's and the host model of that pair."""
    chk, s = ChainChecks(), small()
    A, _ = s.resident(None, A_PAIR)
    A.fetch_begin()
    C_, st = s.resident(A, (1.0, 300.0))
    f1, f2 = s.fetched(A), s.fetched(A)
    hA, _ = s.host(None, A_PAIR)
    chk.that(bit_equal(s.lib, f1, f2), "the begun fetch differs from a second fetch")
    chk.that(bit_equal(s.lib, f1, hA), "the begun fetch is not the host model of the pair")
    must_carry(chk, "A -> C beside the fetch", s, C_, st, hA, (1.0, 300.0))
    chk.done()


@pytest.mark.gpu
def test_freeing_the_warm_model_right_after_the_next_solve(small):
    """The grid loop frees the previous model as soon as the next solve has returned.  The same chain
    with every model kept to the end gives the same models bit for bit, all three steps carried."""
    chk = ChainChecks()
    chain = ((1.0, 300.0), (1.0, 30.0), (1.0, 100.0))
    got = []
    for free_early in (True, False):
        s = small()
        prev, _ = s.resident(None, A_PAIR)
        hs = []
        for k, pair in enumerate(chain):
            warm_h = s.fetched(prev)
            cur, st = s.resident(prev, pair)
            if free_early:
                prev.free()
            must_carry(chk, "freed %s, step %d" % ("early" if free_early else "at the end", k + 1), s, cur, st, warm_h, pair)
            hs.append(s.fetched(cur))
            prev = cur
        got.append((s, hs))
    (s0, h0), (s1, h1) = got
    for k, (a, b) in enumerate(zip(h0, h1)):
        chk.that(bit_equal(s0.lib, a, b), "step %d: freeing the warm model early changed the model" % (k + 1))
    chk.done()


# ---- 4. a carried step that overflows its arena ------------------------------------------------------
@pytest.mark.gpu
def test_a_carried_step_that_overflows_its_arena(small):
    """A cold, B carried with an arena of a third of its coefficients, C carried.  B's first launch
    loads g and overwrites every slot in place; the columns that did not fit are solved again and must
    FOLD (their slots already hold this solve's g, x is the warm model's); C then reads a buffer two
    launches wrote.  optTol 1e-11: the retry regroups tiles (as
    test_resident_model_when_a_column_overflows_its_arena, whose checks of the views these are) -- the
    columns solved again are visited in another order than the oracle's walk visits them, so no share
    of equal sweep counts is asked here (measured: 89 % on B, 100 % on C), the active sets are.
    Measured on an MI355X: B 1.9e-7 and C 7.6e-8 from the oracle, B's nnz 3 from the control's."""
    chk, s = ChainChecks(), small()
    oracle = small_oracle(ARENA_CHAIN, TIGHT_KW["optTol"], TIGHT_KW["niters"])
    kw = dict(optTol=TIGHT_KW["optTol"], niters=TIGHT_KW["niters"])
    every = np.arange(s.mat.ncols)
    A, _ = s.resident(None, ARENA_CHAIN[0], **kw)
    hA = s.fetched(A)
    hB, sB = s.host(hA, ARENA_CHAIN[1], **kw)                  # the folded control: B's nnz, its gram_rows
    A1, _ = s.resident(None, ARENA_CHAIN[0], **kw)
    B1, s1 = s.resident(A1, ARENA_CHAIN[1], **kw)              # carried, everything fits
    arena = max(1024, int(sB["nnzW"]) // 3)
    B, st = s.resident(A, ARENA_CHAIN[1], env={"SLIM_GPU_ARENA": str(arena)}, **kw)
    csB = s.mat.column_stats()
    f = s.fetched(B)
    cp, ci, cv, rp, ri, rv = views(s.lib, f)
    n = s.mat.ncols
    Wc = sp.csc_matrix((cv, ci, cp), shape=(n, n))
    Wr = sp.csr_matrix((rv, ri, rp), shape=(n, n))
    print("B: arena %d for %d coefficients; gram_rows %d (carried and fitting %d, folded %d); nnz %d"
          % (arena, sB["nnzW"], st["gram_rows"], s1["gram_rows"], sB["gram_rows"], cp[-1]))
    chk.that(cp[-1] == rp[-1] == st["nnzW"] == B.nnz, "B: nnz of the views, the stats and the model differ")
    chk.that(abs(int(cp[-1]) - int(sB["nnzW"])) <= 5, "B: nnz %d against the control's %d" % (cp[-1], sB["nnzW"]))
    chk.that(all(np.all(np.diff(ci[cp[k]:cp[k + 1]]) > 0) and np.all(np.diff(ri[rp[k]:rp[k + 1]]) > 0) for k in range(n)),
             "B: ids not strictly ascending in a column or row")
    chk.that(abs(Wc - Wr.tocsc()).nnz == 0, "B: the two views are different matrices")
    # (the columns solved again folded: their fold rows are back, the others' are not)
    chk.that(s1["gram_rows"] < st["gram_rows"] < sB["gram_rows"], "B: no column was solved again, or every one folded")
    chk.step_against_oracle("B, carried and overflowing", (Wc, st, csB), oracle[1], every, tol=2e-5, sweeps=None)
    C_, st = s.resident(B, ARENA_CHAIN[2], **kw)
    csC = s.mat.column_stats()
    chk.step_against_oracle("C, from the g of two launches", (C_.fetch(), st, csC), oracle[2], every, tol=2e-5, sweeps=None)
    must_carry(chk, "C, from the g of two launches", s, C_, st, f, ARENA_CHAIN[2], **kw)
    chk.done()
