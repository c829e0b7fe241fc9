"""Every form of the one-wavefront-per-item solver (cd_wave.hpp) against the oracle walking the same
visiting order, at the sizes where its loops change shape.

finish_path() (engine.hip) runs cd_wave_kernel<USE_LDS, HAS_VAL> whenever the work vectors fit the
LDS (KERNEL_AUTO up to 64 KiB, KERNEL_WAVE_LDS up to 160 KiB) and as the fallback of the tile path.
A form is {lds, hbm} (the work vectors in LDS or in a slab of HBM per wavefront) x {valued, binary}
x {atomic, ordered} (the sums a_i . y by float atomics, or in a fixed order: fractional ratings,
or SLIM_GPU_EXACT_GRAM=1 on any matrix).  The engine's `[trace] wave kernel:` line proves which one
ran, with how many wavefronts and how many bytes of LDS each.

The cases: columns of 0 .. 193 ratings (the two registers per lane of a visited column and its
strided tail); active sets of 0 .. 4 coordinates (the fill and the drain of the three-stage visit
pipeline); 1 .. 129 items and 1 .. 65 users (the 64-wide passes); dynamic LDS of exactly 64 KiB,
one step more, exactly 160 KiB and the refusal beyond; launches in which a wavefront solves a
second and a third column; sweeps ended by the cap min(50 nnz, niters); previous models narrower
than the matrix, with entries outside the active set, on the diagonal and below 1e-7; FSLIM's
selection at exact ties and at 1 .. 129 neighbours.

Reference: O.learn_cd(order=ORDER_PERM, aty=ATY_GRAM), the fp64 restatement in the wave kernel's
own visiting order, with the same seed, penalties, optTol, sweep limit, previous model, neighbour
count, similarity and binary flag.  The checks are the suite's own for this comparison
(test_gpu_parity.py: test_random_ratings, test_tile_kernel_ratings_and_warm_start,
test_ml100k_same_order_as_oracle): max |dW| <= 5e-5, the same active-set sizes and G, the same D on
every column whose sweep count agrees, >= 98 % of the sweep counts (pooled over the sizes of an
item-count or user-count test, whose matrices are smaller than 100 columns), objective and error
to 1e-4 relative where a whole matrix is solved.  Between the LDS and the HBM kernel of one case
the check is the strict one of test_kernels_and_shards_agree: EQUAL models, sweeps, D and U (the
ratings are integers or the sums ordered, so no sum depends on an arrival order).

Every comparison of a test is made and printed before the test fails on any of them."""
import functools
import re

import numpy as np
import pytest
import scipy.sparse as sp

import slim_oracle as O
from library_output import stderr_of_the_library
from slim_amd.constants import SLIM_ERROR_INPUT
from slim_amd.engine import KERNEL_AUTO, KERNEL_WAVE_HBM, KERNEL_WAVE_LDS, DeviceMatrix

TRACE = re.compile(r"\[trace\] wave kernel: (lds|hbm), (valued|binary), sums (atomic|ordered), "
                   r"(\d+) wavefronts, (\d+) bytes of LDS")
KERNEL = {"lds": KERNEL_WAVE_LDS, "hbm": KERNEL_WAVE_HBM}
WHERE = ("lds", "hbm")
SEED = 3

# ratings per column of the ladder: nothing, the pipeline's fill (1, 2, 3), one register per lane
# (64), two (128), and strided tails of one entry, of a whole pass (192) and of a pass and one
LADDER = (0, 1, 2, 3, 63, 64, 65, 127, 128, 129, 191, 192, 193)
LADDER_USERS, LADDER_ITEMS = 512, 104
COLD = dict(l1r=1.0, l2r=0.5)
FIRST = dict(l1r=3.0, l2r=1.0)          # the solve whose model warm-starts the next one
# (kind of ratings, SLIM_GPU_EXACT_GRAM set): the four forms of sums x values, and fractional ratings
LADDER_FORMS = (("valued", False), ("valued", True), ("binary", False), ("binary", True), ("fractional", False))
# penalties (chosen on the CPU) at which the active sets of the ladder hold every size 0 .. 4 and
# one >= 65: test_fixtures_do_their_job holds the condition
SMALL_SETS = {"valued": (dict(l1r=1.0, l2r=0.5), dict(l1r=12.0, l2r=0.5), dict(l1r=20.0, l2r=0.5)),
              "binary": (dict(l1r=1.0, l2r=0.5), dict(l1r=28.0, l2r=0.5), dict(l1r=56.0, l2r=0.5))}
ITEM_COUNTS = (1, 2, 63, 64, 65, 127, 128, 129)
USER_COUNTS = (1, 63, 64, 65)
LDS_USERS = ((16128, 65536), (16129, 65792), (40704, 163840))     # users -> bytes of LDS (128 items)
LDS_REFUSED = 40705
WARM_FIRST = dict(l1r=20.0, l2r=0.5)    # the 512 x 100 matrix: ~95 % of the co-rating sums pass 20,
WARM_SECOND = dict(l1r=80.0, l2r=0.5)   # ~25 % pass 80
NARROW = 70
TIE_NNBRS = (1, 63, 64, 65, 129)


def round_up(a, b):
    return (a + b - 1) // b * b


def lds_need(nrows, ncols):
    """Bytes of the work vectors: r over the users, aTy / ids and x over the items (choose_kernel())."""
    return 4 * (round_up(max(nrows, 1), 64) + 2 * round_up(ncols, 64))


def maxdiff(a, b):
    d = abs(sp.csc_matrix(a) - sp.csc_matrix(b))
    return float(d.max()) if d.nnz else 0.0


# ---- fixtures (seeded; the oracle's results are computed once and shared, never written to) ------
def columns_of(nusers, lengths, rng, extra=()):
    """nusers x len(lengths), column j of lengths[j] users drawn without replacement, ratings 1-5;
    extra: (user, item) pairs rated on top."""
    rows = [rng.choice(nusers, n, replace=False) for n in lengths]
    cols = [np.full(n, j) for j, n in enumerate(lengths)]
    rows, cols = np.concatenate(rows), np.concatenate(cols)
    have = set(zip(rows.tolist(), cols.tolist()))
    more = [p for p in extra if p not in have]
    if more:
        rows = np.concatenate([rows, [u for u, _ in more]])
        cols = np.concatenate([cols, [j for _, j in more]])
    data = rng.integers(1, 6, rows.size).astype(np.float32)
    R = sp.csr_matrix((data, (rows, cols)), shape=(nusers, len(lengths)))
    R.sort_indices()
    return R


@functools.lru_cache(maxsize=None)
def ladder(kind="valued"):
    """512 x 104, column j of LADDER[j % 13] users; ratings 1-5, all 1 (binary) or uniform in
    [0.5, 5) (fractional), on the same pattern."""
    rng = np.random.default_rng(7)
    R = columns_of(LADDER_USERS, [LADDER[j % len(LADDER)] for j in range(LADDER_ITEMS)], rng)
    if kind == "binary":
        R.data[:] = 1.0
    elif kind == "fractional":
        # (a seed at which no co-rating sum comes within 1e-3 relative of a penalty: test_fixtures_do_their_job)
        R.data = np.random.default_rng(106).uniform(0.5, 5.0, R.nnz).astype(np.float32)
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
def _item_matrix():
    return random_ratings(3000, ITEM_COUNTS[-1], 0.05, 31)


@functools.lru_cache(maxsize=None)
def items(n):
    """The first n item columns of a 3000 x 129 random-ratings matrix (~150 ratings per column)."""
    return sp.csr_matrix(_item_matrix()[:, :n])


@functools.lru_cache(maxsize=None)
def users(nu):
    """nu users x 70 items, a rating with probability 0.3."""
    return random_ratings(nu, 70, 0.3, 50 + nu)


@functools.lru_cache(maxsize=None)
def lds_matrix(nusers):
    """nusers x 128, 300 ratings per column, and the last user rates the first and the last item:
    the top of r is read and written."""
    rng = np.random.default_rng(nusers)
    return columns_of(nusers, [300] * 128, rng, extra=((nusers - 1, 0), (nusers - 1, 127)))


@functools.lru_cache(maxsize=None)
def one_per_cu():
    """24000 x 300, 200 ratings per column: 98 560 bytes of work vectors, one wavefront per CU."""
    return columns_of(24000, [200] * 300, np.random.default_rng(61))


@functools.lru_cache(maxsize=None)
def many_columns():
    """256 x 2600, 12 ratings per column: more columns than a device holds wavefronts of 22 016 bytes."""
    return columns_of(256, [12] * 2600, np.random.default_rng(62))


@functools.lru_cache(maxsize=None)
def warm_matrix():
    return columns_of(512, [60] * 100, np.random.default_rng(71))


def gram(R):
    """R^T R in float64 (dense)."""
    Rd = sp.csc_matrix(R, dtype=np.float64)
    return np.asarray((Rd.T @ Rd).todense())


@functools.lru_cache(maxsize=None)
def previous_model():
    """(model of shape (100, 70), the planted entries): the first 70 columns of the oracle's solve at
    WARM_FIRST, plus an entry on the diagonal, an entry of 5e-8 on a row that is active at
    WARM_SECOND, and entries of 0.3 on rows that the screen of WARM_SECOND rejects."""
    R = warm_matrix()
    W = sp.lil_matrix(reference(R, **WARM_FIRST)[0])[:, :NARROW]
    G = gram(R)
    off = ~np.eye(G.shape[0], dtype=bool)
    active = (G > WARM_SECOND["l1r"]) & off
    Wd = W.toarray()
    planted = {"diagonal": (5, 5), "rejected": []}
    W[5, 5] = 0.25
    i = int(np.flatnonzero(active[:, 9] & (Wd[:, 9] == 0))[0])
    W[i, 9] = 5e-8
    planted["tiny"] = (i, 9)
    for j in (0, 17, 64, 69):
        i = int(np.flatnonzero(~active[:, j] & off[:, j] & (Wd[:, j] == 0))[0])
        W[i, j] = 0.3
        planted["rejected"].append((i, j))
    return sp.csc_matrix(W, dtype=np.float32), planted


@functools.lru_cache(maxsize=None)
def ties():
    """Binary, 512 users, 160 columns of exactly 80 ratings and copies of the first 40 behind them:
    every similarity is a function of a co-rating count alone, column k and column 160 + k tie
    exactly with every other column, and the tie goes to the lower id."""
    R = sp.csc_matrix(columns_of(512, [80] * 160, np.random.default_rng(81)))
    R = sp.csr_matrix(sp.hstack([R, R[:, :40]]))
    R.data[:] = 1.0
    R.sort_indices()
    return R


def similarities(R, simtype):
    """FSLIM's similarities in float64, [candidate i, column c] (neighbors.c:82-83, 107-109: the
    norms of the jac form are not squared), -inf where i is no candidate of c; and the inputs that
    decide them, (a, sum of squares of i)."""
    G = gram(R)
    sq = np.diag(G).copy()
    cn = np.sqrt(sq)
    pattern = sp.csc_matrix(R, dtype=np.float64)
    pattern.data[:] = 1.0
    co = np.asarray((pattern.T @ pattern).todense()) > 0
    np.fill_diagonal(co, False)
    with np.errstate(divide="ignore", invalid="ignore"):
        if simtype == 0:
            S = G / cn[:, None]
        elif simtype == 1:
            S = G / (cn[:, None] + cn[None, :] - G)
        else:
            S = G.copy()
    S[~co] = -np.inf
    return S, G, sq


def reference(R, binary=False, niters=10000, **kw):
    """(W, column stats, error, objective) of the oracle in the wave kernel's visiting order."""
    return O.learn_cd(R, order=O.ORDER_PERM, aty=O.ATY_GRAM, seed=SEED, nthreads=8, binary=binary,
                      maxniters=niters, return_stats=True, **kw)


@functools.lru_cache(maxsize=None)
def ladder_reference(kind="valued", warm=False, first=False, **kw):
    """The oracle on the ladder: at COLD, at FIRST, or at COLD from its own model at FIRST; kw
    replaces penalties and limits."""
    R = ladder(kind)
    if first:
        return reference(R, kind == "binary", **FIRST)
    imodel = ladder_reference(kind, first=True)[0] if warm else None
    return reference(R, kind == "binary", imodel=imodel, **dict(COLD, **kw))


@functools.lru_cache(maxsize=None)
def reference_of(fixture, *args, **kw):
    """The oracle on fixture(*args), an integer-ratings matrix."""
    return reference(fixture(*args), **kw)


def test_fixtures_do_their_job():
    """The conditions the cases rest on, all on the CPU."""
    # the ladder: every length, the last column rated, non-trivial solves, a warm start that saves sweeps
    for kind in ("valued", "binary", "fractional"):
        R = ladder(kind)
        lengths = np.diff(R.tocsc().indptr)
        assert R.shape == (LADDER_USERS, LADDER_ITEMS) and set(lengths) == set(LADDER) and lengths[-1] > 0
        W, so, _, _ = ladder_reference(kind)
        assert W.shape == (LADDER_ITEMS, LADDER_ITEMS) and W.nnz >= 500
        assert (so["sweeps"] > 1).mean() >= 0.5 and so["conv"][lengths > 0].all()     # (an empty column: no sweep)
        Ww, sw, _, _ = ladder_reference(kind, warm=True)
        assert ladder_reference(kind, first=True)[0].nnz >= 100 and sw["sweeps"].sum() < so["sweeps"].sum()
    assert ladder("valued").data.min() == 1 and ladder("valued").data.max() == 5
    assert np.all(ladder("binary").data == 1)
    # fractional ratings: no co-rating sum so close to a penalty that fp32 and fp64 could screen differently
    frac = ladder("fractional")
    assert np.any(frac.data != np.round(frac.data))
    G = gram(frac)[~np.eye(LADDER_ITEMS, dtype=bool)]
    for l1 in (COLD["l1r"], FIRST["l1r"]):
        assert np.abs(G - l1).min() > 1e-3 * l1
    # small active sets: every size 0 .. 4 and one >= 65, pooled over the penalties of a kind
    for kind, pairs in SMALL_SETS.items():
        assert len(pairs) <= 3
        sizes = set()
        for kw in pairs:
            sizes |= set(ladder_reference(kind, **kw)[1]["nacols"].tolist())
        assert {0, 1, 2, 3, 4} <= sizes and max(sizes) >= 65, sorted(sizes)
    # sweep limits: at optTol = 0 only the cap ends a column
    so = ladder_reference("valued", optTol=0.0, niters=120)[1]
    nnz = np.diff(ladder("valued").tocsc().indptr)
    assert np.array_equal(so["sweeps"], np.minimum(50 * nnz, 120) + 1) and not so["conv"].any()
    assert {1, 51, 101, 121} <= set(so["sweeps"].tolist())
    for n in (1, 2):
        so = ladder_reference("valued", niters=n)[1]
        assert so["sweeps"].max() == n + 1 and (so["conv"] == 0).sum() >= 50
    # item and user counts: no empty column at any cut, solves that sweep
    assert np.diff(_item_matrix().tocsc().indptr).min() >= 1
    assert reference_of(items, 1, **COLD)[0].nnz == 0
    for n in ITEM_COUNTS[1:]:
        assert reference_of(items, n, **COLD)[1]["sweeps"].max() > 1
    for nu in USER_COUNTS:
        assert users(nu).shape == (nu, 70) and np.diff(users(nu).tocsc().indptr).min() >= 1
        assert reference_of(users, nu, **COLD)[0].nnz >= 70
    # LDS sizes: the bytes, the last user's ratings
    for nu, nbytes in LDS_USERS:
        R = lds_matrix(nu)
        assert lds_need(*R.shape) == nbytes and R[nu - 1, 0] > 0 and R[nu - 1, 127] > 0
        assert reference_of(lds_matrix, nu, **COLD)[0].nnz >= 1000
    assert LDS_USERS[0][1] == 64 * 1024 and LDS_USERS[2][1] == 160 * 1024
    assert lds_need(LDS_REFUSED, 128) > 160 * 1024
    # later columns of a wavefront
    assert 80 * 1024 < lds_need(*one_per_cu().shape) == 98560
    assert lds_need(*many_columns().shape) == 22016
    assert reference_of(one_per_cu, **COLD)[0].nnz >= 10000
    assert reference_of(many_columns, l1r=0.5, l2r=0.5)[0].nnz >= 10000
    # warm-start forms: the planted entries are what they are meant to be
    R = warm_matrix()
    prev, planted = previous_model()
    G = gram(R)
    assert prev.shape == (100, NARROW)
    first = (G > WARM_FIRST["l1r"]) & ~np.eye(100, dtype=bool)
    second = (G > WARM_SECOND["l1r"]) & ~np.eye(100, dtype=bool)
    assert second.sum() >= 1000 and (first & ~second).sum() >= 1000     # a strict subset
    assert (np.abs(prev.toarray()) > 1e-7)[:, :NARROW][~second[:, :NARROW]].sum() >= 20    # entries to drop
    i, j = planted["diagonal"]
    assert i == j and prev[i, j] == np.float32(0.25)
    i, j = planted["tiny"]
    assert second[i, j] and 0 < prev[i, j] <= 1e-7
    for i, j in planted["rejected"]:
        assert not second[i, j] and i != j and prev[i, j] == np.float32(0.3)
    Ww, sw, _, _ = reference(R, imodel=prev, **WARM_SECOND)
    Wc, sc, _, _ = reference_of(warm_matrix, **WARM_SECOND)
    assert Ww.nnz >= 500 and (sw["sweeps"][:NARROW] != sc["sweeps"][:NARROW]).sum() >= 10      # the model is felt
    assert maxdiff(Ww[:, NARROW:], Wc[:, NARROW:]) == 0.0
    # FSLIM ties: every column has as many neighbours as asked for
    R = ties()
    assert R.shape == (512, 200) and np.all(np.diff(R.tocsc().indptr) == 80)
    assert (R[:, :40] != R[:, 160:]).nnz == 0
    for simtype in (0, 1, 2):
        for nnbrs in TIE_NNBRS:
            assert np.all(ties_reference(simtype, nnbrs)[1]["nacols"] == nnbrs)
    # FSLIM on the ladder: the 10th and the 11th candidate are equal by their inputs or clearly apart
    R = ladder("valued")
    for simtype in (0, 1, 2):
        S, G, sq = similarities(R, simtype)
        for c in range(LADDER_ITEMS):
            order = np.lexsort((np.arange(LADDER_ITEMS), -S[:, c]))
            a, b = order[9], order[10]
            if not np.isfinite(S[b, c]):
                continue                    # at most 10 candidates: nothing is cut
            same_inputs = G[a, c] == G[b, c] and (simtype == 2 or sq[a] == sq[b])
            assert same_inputs or abs(S[a, c] - S[b, c]) > 1e-5 * abs(S[a, c]), (simtype, c)
        assert ladder_reference("valued", nnbrs=10, simtype=simtype)[1]["nacols"].max() == 10


@functools.lru_cache(maxsize=None)
def ties_reference(simtype, nnbrs):
    return reference(ties(), binary=True, nnbrs=nnbrs, simtype=simtype, **COLD)


# ---- the GPU side --------------------------------------------------------------------------------
@pytest.fixture(autouse=True)
def _env(monkeypatch):
    for k in ("SLIM_GPU_EXACT_GRAM", "SLIM_GPU_TRACE", "SLIM_GPU_NO_GRAMCD", "SLIM_GPU_GRAMCD"):
        monkeypatch.delenv(k, raising=False)


class Run(object):
    def __init__(self, W, st, cs, wavefronts, lds):
        self.W, self.st, self.cs, self.wavefronts, self.lds = W, st, cs, wavefronts, lds


def traced(m, ordered=False, **kw):
    """One solve under SLIM_GPU_TRACE=1 -> (W, stats, column stats, the wave kernel's trace lines)."""
    env = {"SLIM_GPU_TRACE": "1"}
    if ordered:
        env["SLIM_GPU_EXACT_GRAM"] = "1"
    with stderr_of_the_library(env) as err:
        W, st = m.learn(seed=SEED, **kw)
        cs = m.column_stats()
    return W, st, cs, TRACE.findall(err[0])


def solve(m, where, kind, ordered=False, **kw):
    """One solve by the wave kernel `where` whose trace line must name the form; the stats must
    name the kernel and its bytes of LDS."""
    W, st, cs, got = traced(m, ordered, kernel=KERNEL[where], **kw)
    sums = "ordered" if ordered or kind == "fractional" else "atomic"
    values = "binary" if kind == "binary" else "valued"
    nbytes = lds_need(m.nrows, m.ncols) if where == "lds" else 0
    assert [g[:3] for g in got] == [(where, values, sums)], (got, where, values, sums)
    wavefronts, lds = int(got[0][3]), int(got[0][4])
    assert st["kernel"] == KERNEL[where] and st["lds_bytes"] == lds == nbytes, (st["kernel"], st["lds_bytes"], lds, nbytes)
    assert st["nwaves"] == wavefronts
    return Run(W, st, cs, wavefronts, lds)


class Checks(object):
    """Collects what failed, so that a test reports every figure before it fails."""

    def __init__(self):
        self.failed = []
        self.pool = {}

    def that(self, ok, what):
        if not ok:
            self.failed.append(what)

    def against_oracle(self, tag, run, ref, whole=True, pool=None):
        """The suite's checks of a same-order solve; pool: the sweep counts are judged by
        pooled_sweeps() over every comparison with that key instead of here."""
        W, st, cs = run.W, run.st, run.cs
        Wo, so, err_o, obj_o = ref
        d = maxdiff(W, Wo) if W.shape == Wo.shape else float("inf")
        agree = cs.sweeps == so["sweeps"]
        same = float(agree.mean())
        nac = bool(np.array_equal(cs.nacols, so["nacols"]))
        G = bool(np.array_equal(cs.G, so["G"]))
        D = bool(np.array_equal(cs.D[agree], so["D"][agree]))
        rel_o = abs(st["objval"] - obj_o) / obj_o if obj_o else abs(st["objval"])
        rel_e = abs(st["error"] - err_o) / err_o if err_o else abs(st["error"])
        print("%s: maxdiff %.3e, nacols equal %s, G equal %s, D equal %s, sweeps equal %.4f (%d of %d), objval rel %.2e, "
              "error rel %.2e, nnz %d (oracle %d, up to %d sweeps)"
              % (tag, d, nac, G, D, same, agree.sum(), agree.size, rel_o, rel_e, W.nnz, Wo.nnz, so["sweeps"].max()))
        self.that(W.shape == Wo.shape, "%s: shape %s against %s" % (tag, W.shape, Wo.shape))
        self.that(d <= 5e-5, "%s: maxdiff %.3e > 5e-5" % (tag, d))
        self.that(nac, "%s: nacols differ" % tag)
        self.that(G, "%s: G differs" % tag)
        self.that(D, "%s: D differs on columns of equal sweep counts" % tag)
        if pool is None:
            self.that(same >= 0.98, "%s: sweeps equal on %.4f < 0.98" % (tag, same))
        else:
            a, n = self.pool.get(pool, (0, 0))
            self.pool[pool] = (a + int(agree.sum()), n + agree.size)
        if whole:
            self.that(rel_o <= 1e-4, "%s: objective %.6e against %.6e" % (tag, st["objval"], obj_o))
            self.that(rel_e <= 1e-4, "%s: error %.6e against %.6e" % (tag, st["error"], err_o))

    def pooled_sweeps(self):
        for key, (a, n) in sorted(self.pool.items()):
            print("%s: sweeps equal on %d of %d columns, %.4f" % (key, a, n, a / n))
            self.that(n >= 100 and a >= 0.98 * n, "%s: sweeps equal on %d of %d columns" % (key, a, n))

    def equal(self, tag, a, b, cols=slice(None)):
        """EQUAL models, sweeps, D and U of two runs (on `cols`)."""
        d = maxdiff(a.W[:, cols], b.W[:, cols])
        eq = all(np.array_equal(getattr(a.cs, k)[cols], getattr(b.cs, k)[cols]) for k in ("sweeps", "D", "U", "nacols"))
        print("%s: maxdiff %.3e, sweeps / D / U equal %s" % (tag, d, eq))
        self.that(d == 0.0, "%s: models differ by %.3e" % (tag, d))
        self.that(eq, "%s: sweeps, D or U differ" % tag)

    def done(self):
        assert not self.failed, "\n".join(self.failed)


def both(chk, tag, m, kind, ref, ordered=False, whole=True, pool=None, **kw):
    """The LDS and the HBM kernel on one case: each against the oracle, and EQUAL to each other."""
    runs = [solve(m, where, kind, ordered, **kw) for where in WHERE]
    for where, run in zip(WHERE, runs):
        chk.against_oracle("%s, %s" % (tag, where), run, ref, whole, None if pool is None else "%s, %s" % (pool, where))
    chk.equal("%s, hbm against lds" % tag, runs[1], runs[0])
    return runs


def staged(R, kind="valued"):
    return DeviceMatrix.from_scipy(R, binary=kind == "binary")


# ---- 1. column lengths -----------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("kind,ordered", LADDER_FORMS)
def test_column_length_ladder(kind, ordered):
    """Columns of 0 .. 193 ratings, visited (two registers per lane and the strided tail) and
    solved: cold, at the penalties FIRST, and warm-started from the oracle's model at FIRST (so
    that no difference of the first solve enters the second), in every form."""
    chk = Checks()
    m = staged(ladder(kind), kind)
    tag = "ladder, %s, %s" % (kind, "ordered" if ordered or kind == "fractional" else "atomic")
    try:
        both(chk, tag + ", cold", m, kind, ladder_reference(kind), ordered, **COLD)
        both(chk, tag + ", first", m, kind, ladder_reference(kind, first=True), ordered, **FIRST)
        both(chk, tag + ", warm", m, kind, ladder_reference(kind, warm=True), ordered,
             imodel=ladder_reference(kind, first=True)[0], **COLD)
    finally:
        m.close()
    chk.done()


# ---- 2. small active sets --------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["valued", "binary"])
def test_small_active_sets(kind):
    """Active sets of 0, 1, 2, 3 and 4 coordinates (the visit pipeline filled under na > 0, 1, 2 and
    drained under p + 1, 2, 3 < na) beside sets of more than a wavefront's 64."""
    chk = Checks()
    m = staged(ladder(kind), kind)
    seen = set()
    try:
        for kw in SMALL_SETS[kind]:
            runs = both(chk, "ladder, %s, l1r %g" % (kind, kw["l1r"]), m, kind, ladder_reference(kind, **kw), **kw)
            seen |= set(runs[0].cs.nacols.tolist())
    finally:
        m.close()
    chk.that({0, 1, 2, 3, 4} <= seen and max(seen) >= 65, "active-set sizes solved: %s" % sorted(seen))
    chk.done()


# ---- 3. item and user counts -----------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("ordered", [False, True])
def test_item_count_edges(ordered):
    """1 .. 129 items: the ballot compaction of the active list and the `ib` loop of the ordered
    sums in passes of 64.  One item has no neighbour: an empty model."""
    chk = Checks()
    for n in ITEM_COUNTS:
        m = staged(items(n))
        try:
            runs = both(chk, "%d items, %s" % (n, "ordered" if ordered else "atomic"), m, "valued",
                        reference_of(items, n, **COLD), ordered, pool="item counts", **COLD)
        finally:
            m.close()
        if n == 1:
            chk.that(all(r.W.shape == (1, 1) and r.W.nnz == 0 and r.cs.nacols[0] == 0 for r in runs),
                     "one item: the model is not empty")
    chk.pooled_sweeps()
    chk.done()


@pytest.mark.gpu
@pytest.mark.parametrize("ordered", [False, True])
def test_user_count_edges(ordered):
    """1, 63, 64 and 65 users: the clear and the loss passes over the residual in strides of 64."""
    chk = Checks()
    for nu in USER_COUNTS:
        m = staged(users(nu))
        try:
            both(chk, "%d users, %s" % (nu, "ordered" if ordered else "atomic"), m, "valued",
                 reference_of(users, nu, **COLD), ordered, pool="user counts", **COLD)
        finally:
            m.close()
    chk.pooled_sweeps()
    chk.done()


# ---- 4. LDS sizes ----------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("nusers,nbytes", LDS_USERS)
def test_lds_size_edges(nusers, nbytes):
    """Work vectors of exactly 64 KiB (the last size KERNEL_AUTO gives the LDS kernel, and the last
    that needs no raised limit), of 64 KiB + 256 bytes (the first that does) and of exactly 160 KiB,
    the whole LDS of a CU; the HBM kernel gives the same model."""
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    chk = Checks()
    m = staged(lds_matrix(nusers))
    try:
        W, st, _, got = traced(m, kernel=KERNEL_AUTO, **COLD)
        if nbytes <= 64 * 1024:
            chk.that(st["kernel"] == KERNEL_WAVE_LDS and st["lds_bytes"] == nbytes and [g[0] for g in got] == ["lds"],
                     "KERNEL_AUTO at %d bytes: kernel %d, %s" % (nbytes, st["kernel"], got))
        else:
            chk.that(st["kernel"] != KERNEL_WAVE_LDS and st["lds_bytes"] == 0 and [g for g in got if g[0] == "lds"] == [],
                     "KERNEL_AUTO at %d bytes: kernel %d, %s" % (nbytes, st["kernel"], got))
        runs = both(chk, "%d users, %d bytes" % (nusers, nbytes), m, "valued", reference_of(lds_matrix, nusers, **COLD), **COLD)
        chk.that(runs[0].lds == nbytes, "%d bytes of LDS, not %d" % (runs[0].lds, nbytes))
        chk.that(runs[0].wavefronts == min(128, cus * min(16, 160 * 1024 // nbytes)),
                 "%d wavefronts on %d CUs" % (runs[0].wavefronts, cus))
        if nbytes <= 64 * 1024:
            chk.that(maxdiff(W, runs[0].W) == 0.0, "KERNEL_AUTO's model is not the LDS kernel's")
    finally:
        m.close()
    chk.done()


@pytest.mark.gpu
def test_lds_refusal_one_user_beyond():
    """64 bytes more than the LDS of a CU: SLIM_ERROR_INPUT, and nothing is launched."""
    m = staged(lds_matrix(LDS_REFUSED))
    try:
        with stderr_of_the_library({"SLIM_GPU_TRACE": "1"}) as err:
            with pytest.raises(RuntimeError) as e:
                m.learn(seed=SEED, kernel=KERNEL_WAVE_LDS, **COLD)
        assert "(%d)" % SLIM_ERROR_INPUT in str(e.value) and "do not fit the 160 KiB LDS" in str(e.value)
        assert "[trace] wave kernel" not in err[0]
        # the handle is still good: the HBM kernel solves the same matrix
        run = solve(m, "hbm", "valued", **COLD)
        chk = Checks()
        chk.against_oracle("%d users, hbm" % LDS_REFUSED, run, reference_of(lds_matrix, LDS_REFUSED, **COLD))
        chk.done()
    finally:
        m.close()


# ---- 5. a wavefront's later columns ----------------------------------------------------------------
@pytest.mark.gpu
def test_second_columns_one_wavefront_per_cu():
    """More than 80 KiB of work vectors: one wavefront per CU, and with more columns than CUs
    wavefronts pull a second one, reusing r, aTy / ids and x."""
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    R = one_per_cu()
    chk = Checks()
    m = staged(R)
    try:
        runs = both(chk, "24000 x 300", m, "valued", reference_of(one_per_cu, **COLD), **COLD)
    finally:
        m.close()
    assert runs[0].wavefronts == min(R.shape[1], cus), (runs[0].wavefronts, cus)
    assert R.shape[1] > runs[0].wavefronts, "%d columns on %d wavefronts: no wavefront solves a second column" \
        % (R.shape[1], runs[0].wavefronts)
    chk.done()


@pytest.mark.gpu
def test_later_columns_of_many():
    """2600 cheap columns: more than the wavefronts of either kernel, so the queue hands most
    wavefronts a second column while others still run their first."""
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    R = many_columns()
    kw = dict(l1r=0.5, l2r=0.5)
    chk = Checks()
    m = staged(R)
    try:
        runs = both(chk, "256 x 2600", m, "valued", reference_of(many_columns, **kw), **kw)
    finally:
        m.close()
    per_cu = {"lds": min(16, 160 * 1024 // lds_need(*R.shape)), "hbm": 8}
    for where, run in zip(WHERE, runs):
        assert run.wavefronts == min(R.shape[1], cus * per_cu[where]), (where, run.wavefronts, cus)
        assert R.shape[1] > run.wavefronts, "%s: %d columns on %d wavefronts: no wavefront solves a second column" \
            % (where, R.shape[1], run.wavefronts)
    chk.done()


# ---- 6. sweep limits -------------------------------------------------------------------------------
@pytest.mark.gpu
def test_sweep_cap_ends_every_column():
    """optTol = 0 (it reaches the kernel: decode_options() replaces only -1): no sweep converges, the
    cap min(50 nnz, niters) ends every column, and the count is the cap + 1 (cd.c:140)."""
    R = ladder("valued")
    cap = np.minimum(50 * np.diff(R.tocsc().indptr), 120)
    chk = Checks()
    m = staged(R)
    try:
        runs = both(chk, "ladder, optTol 0, niters 120", m, "valued", ladder_reference("valued", optTol=0.0, niters=120),
                    optTol=0.0, niters=120, **COLD)
        for where, run in zip(WHERE, runs):
            chk.that(np.array_equal(run.cs.sweeps, cap + 1), "%s: sweeps are not min(50 nnz, 120) + 1" % where)
            chk.that(not run.cs.conv.any(), "%s: a column converged at optTol 0" % where)
        for n in (1, 2):
            runs = both(chk, "ladder, niters %d" % n, m, "valued", ladder_reference("valued", niters=n), niters=n, **COLD)
            for where, run in zip(WHERE, runs):
                chk.that(run.cs.sweeps.max() == n + 1, "%s: more than %d sweeps" % (where, n + 1))
    finally:
        m.close()
    chk.done()


# ---- 7. warm-start forms ---------------------------------------------------------------------------
@pytest.mark.gpu
def test_warm_start_forms():
    """A previous model narrower than the matrix, with an entry on the diagonal, one of 5e-8 (not
    folded: cd.c:108-110) and entries outside the active set: the oracle given the same model; the
    columns the model does not have equal a cold solve; FSLIM ignores the model (estimate.c:424-431)."""
    R = warm_matrix()
    prev, _ = previous_model()
    chk = Checks()
    m = staged(R)
    try:
        warm = both(chk, "512 x 100, warm from 70 columns", m, "valued", reference(R, imodel=prev, **WARM_SECOND),
                    imodel=prev, **WARM_SECOND)
        cold = both(chk, "512 x 100, cold", m, "valued", reference_of(warm_matrix, **WARM_SECOND), **WARM_SECOND)
        for where, w, c in zip(WHERE, warm, cold):
            chk.equal("%s: columns %d.. warm against cold" % (where, NARROW), w, c, cols=slice(NARROW, None))
            chk.that((w.cs.sweeps[:NARROW] != c.cs.sweeps[:NARROW]).any(),
                     "%s: the previous model changed no sweep count" % where)
        ref = reference(R, nnbrs=10, **WARM_SECOND)
        plain = both(chk, "512 x 100, FSLIM", m, "valued", ref, nnbrs=10, **WARM_SECOND)
        given = both(chk, "512 x 100, FSLIM with a previous model", m, "valued", ref, nnbrs=10, imodel=prev, **WARM_SECOND)
        for where, a, b in zip(WHERE, given, plain):
            chk.equal("%s: FSLIM with a previous model against without" % where, a, b)
    finally:
        m.close()
    chk.done()


# ---- 8. FSLIM's selection --------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("simtype", [0, 1, 2])
def test_fslim_exact_ties(simtype):
    """Similarities that tie exactly go to the lower id; 1, 63, 64, 65 and 129 neighbours: the rank
    pass that sorts the selection by id runs in blocks of 64."""
    chk = Checks()
    m = staged(ties(), "binary")
    try:
        for nnbrs in TIE_NNBRS:
            runs = both(chk, "ties, simtype %d, nnbrs %d" % (simtype, nnbrs), m, "binary", ties_reference(simtype, nnbrs),
                        nnbrs=nnbrs, simtype=simtype, **COLD)
            chk.that(all(np.all(r.cs.nacols == nnbrs) for r in runs), "nnbrs %d: a column has another number" % nnbrs)
    finally:
        m.close()
    chk.done()


@pytest.mark.gpu
@pytest.mark.parametrize("simtype", [0, 1, 2])
def test_fslim_on_the_ladder(simtype):
    """Ten neighbours out of candidates of unequal lengths, and fewer candidates than that."""
    chk = Checks()
    m = staged(ladder("valued"))
    try:
        runs = both(chk, "ladder, FSLIM, simtype %d" % simtype, m, "valued",
                    ladder_reference("valued", nnbrs=10, simtype=simtype), nnbrs=10, simtype=simtype, **COLD)
        chk.that(all(r.cs.nacols.max() == 10 for r in runs), "more or never 10 neighbours")
    finally:
        m.close()
    chk.done()
