"""G = R^T R as the tile kernel's screen pass forms it (cd_tile.hpp, gram_mode 3; engine.hip,
build_gram) against the co-rating counts themselves: R^T R in int64 on the host.  For a binary
matrix and for ratings 1-5 every entry of G is an integer below 2^24, so float32 holds it exactly
and the comparison is equality, entry for entry -- for every form of the builder (bit-sliced
counters, the ballot form, either in user passes, the line-gathering form on binary and valued
matrices, row blocks, the build inside learn), each proven to have run by the builder's
SLIM_GPU_TRACE line.  G is read before any commit: a commit may pack it and drop the floats.

At the end, the dense path's own R^T R and blocked Cholesky (admm.hip) at the edges of its 64-wide
blocks, against the oracle."""
import ctypes as C
import re

import numpy as np
import pytest
import scipy.sparse as sp

import slim_oracle as O
from slim_amd import _lib
from slim_amd.constants import SLIM_NOPTIONS, SLIM_OK, Opt
from slim_amd.engine import KERNEL_GRAM, DeviceMatrix, model_to_scipy

pytestmark = pytest.mark.gpu

TRACE = re.compile(r"\[trace\] G builder: form (\w+), clusters of (\d+), pass (\d+) of (\d+), "
                   r"(\d+) users at most per member")
PASSES = {"SLIM_GPU_TEST_HOOKS": "1", "SLIM_GPU_TEST_GBITS_ROWS": "300"}


@pytest.fixture(autouse=True)
def _trace(monkeypatch):
    monkeypatch.setenv("SLIM_GPU_TRACE", "1")
    for k in ("SLIM_GPU_GBITS", "SLIM_GPU_NO_GBITS", "SLIM_GPU_NO_GPASSES", "SLIM_GPU_TEST_HOOKS",
              "SLIM_GPU_TEST_GBITS_ROWS"):
        monkeypatch.delenv(k, raising=False)


def setenv(monkeypatch, env):
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def launches(capfd):
    """The G builder's launches since the last look at stderr: (form, cluster, pass, passes, largest
    user range) each."""
    return [(f, int(k), int(p), int(n), int(r)) for f, k, p, n, r in TRACE.findall(capfd.readouterr().err)]


def ran_as(ls, form, passes=1):
    """Every launch was of that form, and they were passes 1 .. passes of one build."""
    assert ls, "the G builder left no trace line"
    assert {l[0] for l in ls} == {form}, ls
    assert [l[2] for l in ls] == list(range(1, passes + 1)) and {l[3] for l in ls} == {passes}, ls


def build(R, binary, capfd, block=None):
    """Rows `block` (default: all) of G on a fresh handle -> (handle, G as numpy (ncols, ld), launches)."""
    mat = DeviceMatrix.from_scipy(R, binary=binary)
    assert mat.ncols == R.shape[1]
    capfd.readouterr()
    b, e = block if block is not None else (0, mat.ncols)
    mat.gram_build_rows(b, e)
    ls = launches(capfd)
    return mat, read_gram(mat), ls


def read_gram(mat):
    import torch
    torch.cuda.synchronize()
    return mat.gram_rows_tensor(0, mat.ncols).cpu().numpy().copy()


def reference(R, fractional=False):
    """R^T R on the host: int64 (float64 for fractional ratings), every entry below 2^24."""
    Rh = sp.csr_matrix(R).astype(np.float64 if fractional else np.int64)
    if not fractional:
        assert np.array_equal(Rh.data, sp.csr_matrix(R).data), "ratings are not integers"
    Gref = np.asarray((Rh.T @ Rh).todense())
    assert Gref.shape == (R.shape[1], R.shape[1])
    assert Gref.max() < 2 ** 24
    return Gref


def work_positions(mat, block=None):
    """Position of every item in the builder's work list: cost order, a row block's items first."""
    cost = mat.column_cost()
    order = np.argsort(-cost, kind="stable")
    if block is not None:
        inb = (order >= block[0]) & (order < block[1])
        order = np.concatenate([order[inb], order[~inb]])
    pos = np.empty(mat.ncols, np.int64)
    pos[order] = np.arange(mat.ncols)
    return pos


def differences(G, want, bad, pos, what):
    """The first few wrong entries with what locates them: both items' work-list positions, their
    tiles, and whether the entry is a tile's own write or the mirror write of the other item's tile."""
    rows, cols = np.nonzero(bad)
    out = ["%s: %d of %d entries differ" % (what, rows.size, bad.size)]
    for r, c in list(zip(rows, cols))[:8]:
        if c >= pos.size:
            out.append("  G[%d, %d] = %r in the padding (row at work-list position %d, tile %d)"
                       % (r, c, float(G[r, c]), pos[r], pos[r] // 32))
            continue
        side = "own write of row %d's tile" % r if pos[r] // 32 <= pos[c] // 32 else \
               "mirror write by column %d's tile" % c
        out.append("  G[%d, %d] = %r, want %r; work-list positions %d (tile %d) and %d (tile %d); %s"
                   % (r, c, float(G[r, c]), float(want[r, c]), pos[r], pos[r] // 32, pos[c], pos[c] // 32, side))
    return "\n".join(out)


def check_gram(G, R, mat, Gref=None, block=None, rows=None):
    """G (ncols, ld) as read from the handle is R^T R exactly: every entry, the symmetry of the
    mirror writes, the diagonal against the column sums of squares, zeros in the padding.  rows
    (b, e): only those rows are promised (a row block; `block` is what the work list was built for)."""
    ncols = R.shape[1]
    Gref = reference(R) if Gref is None else Gref
    assert Gref.max() < 2 ** 24
    want = Gref.astype(np.float32)
    pos = work_positions(mat, block)
    b, e = rows if rows is not None else (0, ncols)
    assert G.dtype == np.float32 and G.shape[0] == ncols and G.shape[1] >= ncols and G.shape[1] % 64 == 0
    sel = np.zeros((ncols, 1), bool)
    sel[b:e] = True
    bad = (G[:, :ncols] != want) & sel
    assert not bad.any() and np.array_equal(G[b:e, :ncols], want[b:e]), differences(G, want, bad, pos, "G vs R^T R")
    if rows is None:
        asym = G[:, :ncols] != G[:, :ncols].T
        assert not asym.any(), differences(G, G[:, :ncols].T, asym, pos, "G vs its transpose")
    Rc = sp.csr_matrix(R)
    sumsq = np.bincount(Rc.indices, weights=Rc.data.astype(np.float64) ** 2, minlength=ncols)
    assert np.array_equal(np.diagonal(G)[b:e], sumsq[b:e].astype(np.float32)), \
        "diagonal vs column sums of squares, first at item %d" % (b + int(np.argmax(np.diagonal(G)[b:e] != sumsq[b:e])))
    pad = (G != 0) & sel
    pad[:, :ncols] = False
    assert not pad.any(), differences(G, want, pad, pos, "writes outside a row")


def ratings(nrows, ncols, density, seed, binary):
    rng = np.random.default_rng(seed)
    R = sp.random(nrows, ncols, density=density, format="csr", random_state=rng, dtype=np.float32)
    R.data[:] = 1.0 if binary else rng.integers(1, 6, R.nnz).astype(np.float32)
    return R


# ---- 1. every form on one random matrix ---------------------------------------------------------
@pytest.fixture(scope="module")
def random_binary():
    R = ratings(40000, 600, 0.01, seed=11, binary=True)
    return R, reference(R)


@pytest.mark.parametrize("env,binary,form,passes", [
    ({}, True, "bits2", 1),
    ({"SLIM_GPU_GBITS": "1"}, True, "bits1", 1),
    (PASSES, True, "bits2", 5),
    (dict(PASSES, SLIM_GPU_GBITS="1"), True, "bits1", 5),
    ({"SLIM_GPU_NO_GBITS": "1"}, True, "lines", 1),
    ({}, False, "lines", 1),
], ids=["bits2", "bits1", "bits2-passes", "bits1-passes", "lines", "lines-valued"])
def test_every_form_holds_the_co_rating_counts(random_binary, monkeypatch, capfd, env, binary, form, passes):
    """The same 0/1 matrix through every form of the builder: each equals R^T R itself, not merely
    the other forms.  1250 users per member against a pretended capacity of 300 rows: 5 user passes,
    the later four adding into G.  binary=False stages the ones as values: the valued instantiation
    of the line-gathering form."""
    R, Gref = random_binary
    setenv(monkeypatch, env)
    mat, G, ls = build(R, binary, capfd)
    ran_as(ls, form, passes)
    assert all(l[1] == 32 for l in ls) or form == "lines"
    check_gram(G, R, mat, Gref)
    mat.close()


# ---- 2. the top of the counter planes -----------------------------------------------------------
LADDER = (36000, 32768, 32767, 4097, 257, 65, 9, 1)
PER, MEMBERS = 36000, 32


@pytest.fixture(scope="module")
def ladder():
    """32 x 36 000 users, 64 items, 8 ratings in every row, so that the equal-nnz split gives the 32
    members exactly 36 000 users each.  With v = u % 36000, user u rates ladder item j iff
    v < LADDER[j]; the row is filled up to 8 entries with distinct items of the other 56.  Within a
    member the co-count of ladder items i, j is min(LADDER[i], LADDER[j]): 36 000, 32 768, 32 767,
    4 097, ... -- every one of the 16 counter planes, both sides of 2^15."""
    nu = PER * MEMBERS
    u = np.arange(nu, dtype=np.int64)
    k = ((u % PER)[:, None] < np.array(LADDER)[None, :]).sum(1)
    t = np.arange(8)[None, :]
    idx = np.sort(np.where(t < k[:, None], t, 8 + (u[:, None] * 7 + t) % 56), axis=1).astype(np.int32)
    R = sp.csr_matrix((np.ones(nu * 8, np.float32), idx.ravel(), np.arange(nu + 1, dtype=np.int64) * 8),
                      shape=(nu, 64))
    assert R.nnz == 9216000 and (np.diff(idx, axis=1) > 0).all()
    for mk in (0, MEMBERS - 1):   # the per-member counts the planes have to hold
        blk = R[mk * PER:(mk + 1) * PER].astype(np.int64)
        Gm = np.asarray((blk.T @ blk).todense())
        assert Gm.max() == 36000 >= 32768
        for i in range(8):
            for j in range(8):
                assert Gm[i, j] == min(LADDER[i], LADDER[j])
    return R, reference(R)


@pytest.mark.parametrize("gbits,form", [(None, "bits2"), ("1", "bits1")])
def test_counts_at_and_above_two_to_the_fifteenth(ladder, monkeypatch, capfd, gbits, form):
    """Per-member counts of 32 767, 32 768 and 36 000 (the host side asserts them, see ladder): the
    carry chain of the bit-sliced counter up to its top plane, in one launch (a member's 36 000
    words are 144 384 bytes of LDS, under the cap).  The same through the ballot form."""
    R, Gref = ladder
    if gbits:
        monkeypatch.setenv("SLIM_GPU_GBITS", gbits)
    mat, G, ls = build(R, True, capfd)
    ran_as(ls, form, 1)
    assert ls[0][1] == 32 and ls[0][4] == PER, ls
    assert Gref[0, 0] == PER * MEMBERS and Gref[1, 2] == 32767 * MEMBERS
    check_gram(G, R, mat, Gref)
    mat.close()


# ---- 3. item-count edges ------------------------------------------------------------------------
EDGE_FORMS = [(False, "bits2"), (False, "bits1"), (True, "lines")]   # binary twice, ratings 1-5


def edge_matrix(ncols, valued, seed=5, fractional=False):
    """20 000 users, ~2 % dense; users without ratings in a block at the start, in the middle and at
    the end; two items without ratings in the middle of the id range (ncols >= 5)."""
    nu = 20000
    rng = np.random.default_rng(seed + ncols)
    mask = rng.random((nu, ncols)) < 0.02
    mask[:700] = False
    mask[9000:10500] = False
    mask[19300:] = False
    if ncols >= 5:
        mask[:, ncols // 2] = False
        mask[:, ncols // 3] = False
    mask[5000, ncols - 1] = True   # (the last item is rated: the staging takes ncols from the ids)
    R = sp.csr_matrix(mask.astype(np.float32))
    if fractional:
        R.data[:] = rng.uniform(0.5, 2.5, R.nnz).astype(np.float32)
    elif valued:
        R.data[:] = rng.integers(1, 6, R.nnz).astype(np.float32)
    return R


@pytest.mark.parametrize("valued,form", EDGE_FORMS, ids=["bits2", "bits1", "ratings"])
@pytest.mark.parametrize("ncols", [1, 31, 32, 33, 63, 64, 65, 97])
def test_item_count_edges(monkeypatch, capfd, ncols, valued, form):
    """One partial tile, work lists that are no multiple of 32 or 64, a last tile with fewer than 32
    problems, unrated items inside the id range, blocks of users without ratings.  Binary: the
    bit-sliced form and the ballot form; ratings 1-5: the line-gathering form, sums exact below 2^24."""
    R = edge_matrix(ncols, valued)
    nnz_col = np.diff(sp.csc_matrix(R).indptr)
    assert nnz_col[-1] > 0 and (ncols < 5 or (nnz_col[ncols // 2] == 0 and nnz_col[ncols // 3] == 0))
    if form == "bits1":
        monkeypatch.setenv("SLIM_GPU_GBITS", "1")
    mat, G, ls = build(R, not valued, capfd)
    ran_as(ls, form, 1)
    check_gram(G, R, mat)
    mat.close()


# ---- 4. slice-length edges ----------------------------------------------------------------------
SLICE_NNZ = (0, 1, 31, 32, 63, 64, 65, 255, 256, 257, 33)   # the last one is 1 (mod 32)
NFILL = 20


def slice_matrix(spread, valued, seed=9):
    """20 000 users x 31 items: items 0..19 carry the bulk (every user rates about half of them),
    items 20..30 have exactly SLICE_NNZ ratings.  spread=False: an item's users are the LAST users,
    all inside the last member's range (the bulk decides the equal-nnz split), so its slices are one
    long one and 31 empty ones; spread=True: they are spaced evenly, so most slices hold 0 or 1.
    The last item of the column view has 33 ratings: the 32-id step of the lane that walks its last
    slice reads on past the end of the view, into the slack."""
    nu = 20000
    rng = np.random.default_rng(seed)
    mask = np.zeros((nu, NFILL + len(SLICE_NNZ)), bool)
    mask[:, :NFILL] = rng.random((nu, NFILL)) < 0.5
    for j, n in enumerate(SLICE_NNZ):
        users = (np.arange(n) * nu) // max(n, 1) + j if spread else nu - 1 - np.arange(n)
        mask[users, NFILL + j] = True
    R = sp.csr_matrix(mask.astype(np.float32))
    if valued:
        R.data[:] = rng.integers(1, 6, R.nnz).astype(np.float32)
    assert tuple(np.diff(sp.csc_matrix(R).indptr)[NFILL:]) == SLICE_NNZ and SLICE_NNZ[-1] % 32 == 1
    return R


@pytest.mark.parametrize("valued,form", EDGE_FORMS, ids=["bits2", "bits1", "ratings"])
@pytest.mark.parametrize("spread", [False, True], ids=["long-slices", "short-slices"])
def test_slice_length_edges(monkeypatch, capfd, spread, valued, form):
    """Column slices of length 0, 1, 31 .. 33, 63 .. 65, 255 .. 257 (long form) or mostly 0 and 1
    (spread form), the tail of the column view among them."""
    R = slice_matrix(spread, valued)
    if form == "bits1":
        monkeypatch.setenv("SLIM_GPU_GBITS", "1")
    mat, G, ls = build(R, not valued, capfd)
    ran_as(ls, form, 1)
    check_gram(G, R, mat)
    mat.close()


# ---- 5. no pass count fits ----------------------------------------------------------------------
def test_falls_back_to_lines_when_no_pass_count_fits(capfd):
    """2 000 000 users, 1 500 000 of them in one run without ratings: that run lies inside ONE range
    of any equal-nnz split, so no number of user passes brings a member's range under the LDS cap
    and the planner gives up the word form.  The line-gathering form then forms the same exact G."""
    rng = np.random.default_rng(3)
    nrated, nu, ncols = 500000, 2000000, 100
    rows = np.repeat(np.arange(nrated, dtype=np.int64), 6)
    rows = np.where(rows < nrated // 2, rows, rows + (nu - nrated))
    R = sp.coo_matrix((np.ones(rows.size, np.float32), (rows, rng.integers(0, ncols, rows.size))),
                      shape=(nu, ncols)).tocsr()
    R.sum_duplicates()
    R.data[:] = 1.0
    assert R.shape == (nu, ncols) and (np.diff(R.indptr)[nrated // 2:nu - nrated // 2] == 0).all()
    mat, G, ls = build(R, True, capfd)
    ran_as(ls, "lines", 1)
    check_gram(G, R, mat)
    mat.close()


# ---- 6. row blocks ------------------------------------------------------------------------------
# (the 1500 users without ratings in the middle of edge_matrix lie in one range of any split: a
# pretended capacity of 300 rows would send the builder to the line form, as in the 2M-user case
# above; 1900 rows hold a range of 64 -- about 310 rated users + those 1500 -- but not one of 32)
BLOCK_PASSES = dict(PASSES, SLIM_GPU_TEST_GBITS_ROWS="1900")
BLOCK_FORMS = [({}, False, "bits2", 1), (BLOCK_PASSES, False, "bits2", None), ({}, True, "lines", 1)]


@pytest.mark.parametrize("env,valued,form,passes", BLOCK_FORMS, ids=["bits2", "passes", "ratings"])
def test_row_blocks(monkeypatch, capfd, env, valued, form, passes):
    """SLIMGPU_MatrixGramBuildRows on 97 items: a block of rows [b, e) on a fresh handle holds those
    rows of R^T R over all 97 columns (nothing is promised about the other rows), for blocks that
    are empty, one row, the last row, inside a tile, a whole tile and everything; three blocks in
    turn on one handle make the whole G.  In the bit-sliced form, in user passes (two: see
    BLOCK_PASSES) and on ratings 1-5."""
    R = edge_matrix(97, valued, seed=21)
    Gref = reference(R)
    setenv(monkeypatch, env)
    for blk in ((0, 0), (0, 1), (96, 97), (17, 45), (32, 64), (0, 97)):
        mat, G, ls = build(R, not valued, capfd, block=blk)
        if blk[0] == blk[1]:
            assert not ls and not G.any()
        else:
            if passes is None:   # (as many as the split needs, but passes: later ones add into G)
                passes = ls[0][3]
                assert passes > 1, ls
            ran_as(ls, form, passes)
            check_gram(G, R, mat, Gref, block=blk, rows=blk)
        mat.close()
    mat = DeviceMatrix.from_scipy(R, binary=not valued)
    capfd.readouterr()
    for blk in ((0, 17), (17, 45), (45, 97)):
        mat.gram_build_rows(*blk)
        ran_as(launches(capfd), form, passes)
    check_gram(read_gram(mat), R, mat, Gref)
    mat.close()


# ---- 7. the build inside learn ------------------------------------------------------------------
def test_the_build_inside_learn(random_binary, capfd):
    """learn(kernel=KERNEL_GRAM) on a handle without G builds it on the way (gram_for_solve: all
    rows in one list, no block partition): the same exact G; a second solve builds nothing and
    leaves G as it is."""
    R, Gref = random_binary
    mat = DeviceMatrix.from_scipy(R, binary=True)
    capfd.readouterr()
    cols = np.arange(5, 12, dtype=np.int32)
    W1, s1 = mat.learn(kernel=KERNEL_GRAM, columns=cols, niters=50)
    ran_as(launches(capfd), "bits2", 1)
    assert s1["kernel"] == KERNEL_GRAM and s1["gram_build_ms"] > 0 and W1.nnz > 0
    G1 = read_gram(mat)
    check_gram(G1, R, mat, Gref)
    W2, s2 = mat.learn(kernel=KERNEL_GRAM, columns=cols, niters=50)
    assert s2["gram_build_ms"] == 0 and not launches(capfd)
    assert np.array_equal(read_gram(mat), G1) and abs(W1 - W2).nnz == 0
    mat.close()


# ---- 8. fractional ratings ----------------------------------------------------------------------
@pytest.mark.parametrize("ncols", [33, 97])
def test_fractional_ratings_within_the_rounding_bound(capfd, ncols):
    """Ratings in [0.5, 2.5): against R^T R in float64 under the bound that ANY order of float32
    summation satisfies -- n_ij positive products, each rounded once, summed in n_ij - 1 additions,
    plus the additions of up to 32 members' partial sums: |G - Gref| <= (n_ij + 33) 2^-24 Gref,
    n_ij the co-rating count of the pair.  A dropped or doubled term is off by 1 / n_ij, orders of
    magnitude more at these counts (n_ij <= ~450).  The sums are formed in a fixed order
    (exact_gram): a second handle gives the same bits.  The mirror writes and the padding stay exact."""
    R = edge_matrix(ncols, True, fractional=True)
    Gref = reference(R, fractional=True)
    P = sp.csr_matrix(R).copy()
    P.data[:] = 1.0
    nij = reference(P)
    mat, G, ls = build(R, False, capfd)
    ran_as(ls, "lines", 1)
    pos = work_positions(mat)
    bound = (nij + 33) * 2.0 ** -24 * Gref
    bad = np.abs(G[:, :ncols].astype(np.float64) - Gref) > bound
    assert not bad.any(), differences(G, Gref, bad, pos, "G vs R^T R beyond the rounding bound")
    # (a mirror write copies the sum; the two entries of a pair INSIDE one tile are both formed by
    # that tile, one over the users of either item: each within the bound, not the same bits)
    apart = (pos // 32)[:, None] != (pos // 32)[None, :]
    asym = (G[:, :ncols] != G[:, :ncols].T) & apart
    assert not asym.any(), differences(G, G[:, :ncols].T, asym, pos, "G vs its transpose, across tiles")
    assert not G[:, ncols:].any()
    mat2, G2, ls2 = build(R, False, capfd)
    ran_as(ls2, "lines", 1)
    assert np.array_equal(G.view(np.uint32), G2.view(np.uint32))
    mat.close()
    mat2.close()


# ---- the dense path: R^T R and the blocked Cholesky of admm.hip at the block edges --------------
@pytest.mark.parametrize("binary", [False, True], ids=["ratings", "binary"])
@pytest.mark.parametrize("m", [1, 63, 64, 65, 128])
def test_admm_block_edges_match_oracle(m, binary):
    """SLIM_Learn(algo = admm) factors R^T R + (l2 + rho) I in 64 x 64 blocks (k_potf2 + rocBLAS
    updates): one partial block without a trailing update (1, 63), exact multiples of the block
    (64, 128) and one row beyond (65) -- with ratings and with rowval = NULL, the binary branch of
    k_gram_dense.  Same assertions as test_admm_matches_oracle."""
    lib = _lib.load()
    rng = np.random.default_rng(100 + m)
    mask = rng.random((3000, m)) < (0.3 if m == 1 else 0.05)
    mask[7, m - 1] = True
    R = sp.csr_matrix(mask.astype(np.float32))
    R.data[:] = 1.0 if binary else rng.integers(1, 6, R.nnz).astype(np.float32)
    R.sort_indices()
    io = np.full(SLIM_NOPTIONS, -1, np.int32)
    do = np.full(SLIM_NOPTIONS, -1.0, np.float64)
    io[Opt.ALGO] = 0
    do[Opt.L1R], do[Opt.L2R] = 1.0, 1.0
    st = C.c_int32(0)
    val = R.data.astype(np.float32)
    h = lib.SLIM_Learn(R.shape[0], R.indptr.astype(np.intp), R.indices.astype(np.int32),
                       None if binary else val.ctypes.data_as(C.c_void_p),
                       io.ctypes.data_as(C.c_void_p), do.ctypes.data_as(C.c_void_p), None, C.byref(st))
    assert h and st.value == SLIM_OK, _lib.last_error()
    W = sp.csr_matrix(model_to_scipy(lib, h))
    Wo = O.learn_admm(R, l1r=1.0, l2r=1.0, nthreads=8, binary=binary)
    assert W.shape == Wo.shape == (m, m)
    d = abs(W - Wo)
    assert (float(d.max()) if d.nnz else 0.0) <= 1e-6
    assert abs(W.nnz - Wo.nnz) <= max(4, Wo.nnz // 10000)   # entries at the edge of > 0
    assert W.diagonal().max() <= 1e-3 and (W.nnz == 0 or W.data.min() > 0)
    assert m == 1 or Wo.nnz > 0
