"""The byte planes of G = R^T R (gram_pack.hpp) as SLIMGPU_MatrixGramPlanes shows them, for the
form that streams transposed tiles of G (the default) -- every case twice over:

  A. decoded (lo + 16 base + 256 hi + 65536 hi2, diag at the row's own rank) they are R^T R in
     integers on the host, columns in popularity order; rank_of / item_of, diag and the four fields
     of the row records against the host as well;
  B. every array, padding included, equals what a second handle packs with SLIM_GPU_PACK_GATHER=1
     (the per-row gathering kernels): that pins the minimal prefix and the choice of the base bytes,
     which a decode cannot see.  The "G packed" trace line proves which form ran.

G is built with gram_build_rows(0, ncols) + gram_commit(); below 8 GB the floats stay."""
import re

import numpy as np
import pytest
import scipy.sparse as sp

from library_output import stderr_of_the_library
from slim_amd.engine import KERNEL_GRAM, DeviceMatrix

gpu = pytest.mark.gpu

PACKED = re.compile(r"\[trace\] G packed \(([a-z ]+)\):")
ARRAYS = ("lo", "base", "hi", "hi_off", "hi_k", "hi2_k", "diag", "meta", "rank_of", "item_of")
GROUP = 8192            # ranks per group of a plane
CG = GROUP // 16        # chunks per group


# ---- the host's side ----------------------------------------------------------------------------
def popularity_order(R):
    """item_of (rank -> id): ratings per item descending, ties by id; and rank_of."""
    nnzc = np.diff(sp.csc_matrix(R).indptr)
    item_of = np.lexsort((np.arange(nnzc.size), -nnzc)).astype(np.int64)
    rank_of = np.empty_like(item_of)
    rank_of[item_of] = np.arange(item_of.size)
    return item_of, rank_of, nnzc


def gram_rows(R, rows):
    """Rows `rows` of R^T R in int64."""
    Rc = sp.csc_matrix(R).astype(np.int64)
    assert np.array_equal(Rc.data, sp.csc_matrix(R).data), "ratings are not integers"
    if len(rows) <= 512:   # (a few rows of a large matrix: sparse x dense, exact in float64)
        return np.asarray(Rc.T @ Rc[:, rows].toarray().astype(np.float64)).T.astype(np.int64)
    return np.asarray((Rc[:, rows].T @ Rc).todense())


def scan_rule(v, own):
    """gram_pack_scan's rule on one row in rank order (v, the row's own rank `own` left out):
    (hi_k, hi2_k, base byte per chunk as stored behind the prefix)."""
    n = v.size
    nch = (n + 15) // 16
    ch = np.full(nch * 16, -1, np.int64)
    ch[:n] = v
    ch[own] = -1
    ch = ch.reshape(nch, 16)
    there = ch >= 0
    big = np.iinfo(np.int64).max
    mn = np.where(there, ch, big).min(1)
    mx = np.where(there, ch, 0).max(1)
    b = np.where(mn == big, 0, np.minimum(mn >> 4, 255))
    need1 = np.nonzero(mx - 16 * b > 255)[0]
    need2 = np.nonzero(mx >= 65536)[0]
    last1 = need1[-1] if need1.size else -1
    last2 = need2[-1] if need2.size else -1
    return (last1 + CG) // CG, (last2 + CG) // CG, b


def decode(P, rows):
    """Rows `rows` of the planes P as integers, (len(rows), ncols) in rank order."""
    n, nch = P["ncols"], P["nchunks"]
    c = np.arange(nch * 16) // 16
    where_b = (c % CG) * 16 + c // CG
    out = np.empty((len(rows), n), np.int64)
    for at, i in enumerate(rows):
        v = P["lo"][i].astype(np.int64) + 16 * P["base"][i][where_b].astype(np.int64)
        off = int(P["hi_off"][i])
        n1, n2 = int(P["hi_k"][i]) * GROUP, int(P["hi2_k"][i]) * GROUP
        m1, m2 = min(n1, v.size), min(n2, v.size)
        v[:m1] += 256 * P["hi"][off:off + m1].astype(np.int64)
        v[:m2] += 65536 * P["hi"][off + n1:off + n1 + m2].astype(np.int64)
        v[P["rank_of"][i]] = int(P["diag"][i])
        out[at] = v[:n]
    return out


def first_wrong(got, want, rows, item_of, what):
    bad = np.argwhere(got != want)
    lines = ["%s: %d of %d entries differ" % (what, len(bad), got.size)]
    for a, r in bad[:8]:
        lines.append("  row (item) %d, rank %d (item %d, chunk %d, group %d): planes give %d, R^T R has %d"
                     % (rows[a], r, item_of[r], r // 16, r // GROUP, got[a, r], want[a, r]))
    return "\n".join(lines)


def check_against_host(P, R, rows=None):
    """Assertion A."""
    n = R.shape[1]
    item_of, rank_of, nnzc = popularity_order(R)
    assert P["ncols"] == n and P["nchunks"] == (n + 15) // 16 and P["ldb"] == 16 * P["nchunks"]
    assert np.array_equal(P["rank_of"], rank_of), "rank_of"
    assert np.array_equal(P["item_of"][:n], item_of) and (P["item_of"][n:] == -1).all(), "item_of"
    rows = np.arange(n) if rows is None else np.asarray(rows)
    want = gram_rows(R, rows)
    assert want.max() < 2 ** 24
    got = decode(P, rows)
    assert np.array_equal(got, want[:, item_of]), first_wrong(got, want[:, item_of], rows, item_of, "planes vs R^T R")
    Rr = sp.csr_matrix(R)
    sumsq = np.bincount(Rr.indices, weights=Rr.data.astype(np.float64) ** 2, minlength=n).astype(np.float32)
    assert np.array_equal(P["diag"], sumsq), "diag, first at item %d" % int(np.argmax(P["diag"] != sumsq))
    meta = P["meta"]
    word0 = rank_of.astype(np.uint32) | (P["hi_k"].astype(np.uint32) << 17) | (P["hi2_k"].astype(np.uint32) << 21)
    assert np.array_equal(meta[:, 0], word0), "row record: rank | hi_k << 17 | hi2_k << 21"
    assert np.array_equal(meta[:, 1].astype(np.int64) * GROUP, P["hi_off"]), "row record: hi_off / 8192"
    assert np.array_equal(meta[:, 2], nnzc.astype(np.uint32)), "row record: nnz of the column"
    assert np.array_equal(meta[:, 3], sumsq.view(np.uint32)), "row record: bits of G_ii"
    # the pool: a row's hi groups, then its hi2 groups, rows in id order, one group of slack behind
    size = (P["hi_k"].astype(np.int64) + P["hi2_k"]) * GROUP
    assert np.array_equal(P["hi_off"], np.cumsum(size) - size) and P["hi"].size == size.sum() + GROUP


def check_same_planes(P, Q, what="streamed tiles vs gathers"):
    """Assertion B."""
    for k in ("ncols", "nchunks", "ldb"):
        assert P[k] == Q[k], k
    for k in ARRAYS:
        a, b = P[k], Q[k]
        assert a.shape == b.shape and a.dtype == b.dtype, "%s: %s" % (what, k)
        if not np.array_equal(a, b):
            at = np.argwhere(a != b)
            raise AssertionError("%s: %s differs in %d of %d places, first at %s: %r against %r"
                                 % (what, k, len(at), a.size, tuple(at[0]), a[tuple(at[0])], b[tuple(at[0])]))


# ---- the device's side --------------------------------------------------------------------------
def committed(R, binary, gather, blocks=None):
    """A fresh handle with G built (in `blocks`, default one call) and committed -> (handle, forms
    the trace names: [] when nothing was packed)."""
    env = {"SLIM_GPU_TRACE": "1", "SLIM_GPU_PACK_GATHER": "1" if gather else "0"}
    with stderr_of_the_library(env) as err:
        mat = DeviceMatrix.from_scipy(R, binary=binary)
        assert mat.ncols == R.shape[1]
        for b, e in blocks or ((0, mat.ncols),):
            mat.gram_build_rows(b, e)
        mat.gram_commit()
    return mat, PACKED.findall(err[0])


def planes_of(R, binary, gather, blocks=None):
    mat, forms = committed(R, binary, gather, blocks)
    assert forms == ["gathers" if gather else "streamed tiles"], forms
    P = mat.gram_planes()
    mat.close()
    return P


def both_ways(R, binary, rows=None):
    """Assertions A and B for one matrix; returns the planes of the streamed form."""
    P = planes_of(R, binary, gather=False)
    check_against_host(P, R, rows)
    Q = planes_of(R, binary, gather=True)
    check_same_planes(P, Q)
    return P


def maxdiff(a, b):
    d = abs(sp.csc_matrix(a) - sp.csc_matrix(b))
    return float(d.max()) if d.nnz else 0.0


def random_ratings(nu, ni, density, seed, binary):
    rng = np.random.default_rng(seed)
    R = sp.random(nu, ni, density=density, format="csr", random_state=rng, dtype=np.float32)
    R.data = np.ones(R.nnz, np.float32) if binary else rng.integers(1, 6, R.nnz).astype(np.float32)
    R.sort_indices()
    return R


# ---- 1. item-count edges ------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("ncols", [1, 15, 16, 17, 63, 64, 65, 127, 129, 8191, 8192, 8193])
def test_item_count_edges(ncols):
    """2000 users at density 0.01, binary: a last chunk of 1, 15 and 16 ranks, one item block of the
    tile walk and one item beyond (64, 65), two tiles of 8 chunk slots and one chunk beyond (127,
    129), one group of 8192 ranks, one rank short of it and a second group of one chunk (8193)."""
    rng = np.random.default_rng(100 + ncols)
    mask = rng.random((2000, ncols)) < 0.01
    mask[5, ncols - 1] = True    # (the last item is rated: the staging takes ncols from the ids)
    both_ways(sp.csr_matrix(mask.astype(np.float32)), True)


# ---- 2. three groups, every prefix length -------------------------------------------------------
NU3, NI3 = 6000, 16484            # two full groups, 100 ranks of a third, a last chunk of 4
PLANTED = (3000, 9000, 12000, 16400)


def three_group_matrix():
    """Popularity min(0.6, 100 / (r + 1)) + 0.06 for the item the generator draws r-th, every item's
    users drawn on their own; ids are a random permutation of that order.  Then, by rank, the users
    of the items at ranks 3000, 9000, 12000 and 16400 are copied onto the item of the next rank: the
    two rows of a pair hold an entry as large as their diagonal right beside it, hundreds above
    the chunk's level, so their hi planes reach to that chunk -- the first, second and third group --
    while nearly every other row has none."""
    rng = np.random.default_rng(5)
    p = np.minimum(0.6, 100.0 / (np.arange(NI3) + 1.0)) + 0.06
    ids = rng.permutation(NI3)
    cols, users = [], []
    for r0 in range(0, NI3, 1024):
        m = rng.random((min(1024, NI3 - r0), NU3)) < p[r0:r0 + 1024, None]
        rr, uu = np.nonzero(m)
        cols.append(ids[r0 + rr])
        users.append(uu)
    cols, users = np.concatenate(cols), np.concatenate(users)
    M = sp.csc_matrix((np.ones(cols.size, np.float32), (users, cols)), shape=(NU3, NI3))
    item_of, _, _ = popularity_order(M)
    of = [M.indices[M.indptr[j]:M.indptr[j + 1]] for j in range(NI3)]
    for r in PLANTED:
        of[item_of[r + 1]] = of[item_of[r]]
    ptr = np.concatenate([[0], np.cumsum([u.size for u in of])])
    R = sp.csc_matrix((np.ones(ptr[-1], np.float32), np.concatenate(of), ptr), shape=(NU3, NI3)).tocsr()
    R.sort_indices()
    planted = [int(item_of[r + d]) for r in PLANTED for d in (0, 1)]
    return R, planted


@pytest.fixture(scope="module")
def three_groups():
    R, planted = three_group_matrix()
    item_of, rank_of, _ = popularity_order(R)
    rng = np.random.default_rng(6)
    rows = np.concatenate([planted, rng.choice(NI3, 256, replace=False)])
    return R, planted, rows


def test_three_group_fixture_holds_every_prefix_length(three_groups):
    """The fixture's own properties, on the host (gram_pack_scan's rule, scan_rule above): the planted
    rows need 1, 1, 2, 2, 2, 2, 3 and 3 groups of the hi plane, the most popular rows (all but a
    few), the least popular ones and ranks 1000-1063 none; no row has a hi2 plane; the base bytes of
    the chunks behind the prefix are in use (levels up to the 2600 co-ratings of two popular items:
    bytes beyond 160) in over 10^5 chunks of 200 sampled rows."""
    R, planted, _ = three_groups
    assert R.shape == (NU3, NI3) and 9.2e6 < R.nnz < 9.4e6
    item_of, rank_of, _ = popularity_order(R)

    def rule(items):
        G = gram_rows(R, np.asarray(items))[:, item_of]
        return [scan_rule(G[a], rank_of[i]) for a, i in enumerate(items)]
    got = rule(planted)
    assert [g[0] for g in got] == [1, 1, 2, 2, 2, 2, 3, 3] and all(g[1] == 0 for g in got)
    others = [i for i in item_of[-66:] if i not in planted][:64]
    assert sum(g[0] == 0 for g in rule(item_of[:64])) >= 60
    assert all(g[0] == 0 for g in rule(others)) and all(g[0] == 0 for g in rule(item_of[1000:1064]))
    sample = rule(np.random.default_rng(7).choice(NI3, 200, replace=False))
    assert all(g[1] == 0 for g in sample)
    assert max(g[2].max() for g in sample + rule(item_of[:64])) >= 160
    assert sum(int((g[2][g[0] * CG:] > 0).sum()) for g in sample) > 10 ** 5


@pytest.fixture(scope="module")
def three_group_handles(three_groups):
    R = three_groups[0]
    made = [committed(R, True, gather) for gather in (False, True)]
    yield made
    for mat, _ in made:
        mat.close()


@gpu
def test_three_groups_every_prefix_length(three_groups, three_group_handles):
    """A on the planted rows and 256 random ones (not the dense 16 484^2 product), hi_k of those
    rows by the scan's rule on the host; B on everything."""
    R, planted, rows = three_groups
    (ms, fs), (mg, fg) = three_group_handles
    assert fs == ["streamed tiles"] and fg == ["gathers"]
    P, Q = ms.gram_planes(), mg.gram_planes()
    check_against_host(P, R, rows)
    assert [int(P["hi_k"][i]) for i in planted] == [1, 1, 2, 2, 2, 2, 3, 3]
    item_of, rank_of, _ = popularity_order(R)
    G = gram_rows(R, rows)[:, item_of]
    for a, i in enumerate(rows):
        k1, k2, b = scan_rule(G[a], rank_of[i])
        assert (P["hi_k"][i], P["hi2_k"][i]) == (k1, k2), "item %d (rank %d)" % (i, rank_of[i])
        c = np.arange(k1 * CG, b.size)     # behind the prefix: the chunk's base byte; inside: 0
        assert np.array_equal(P["base"][i][(c % CG) * 16 + c // CG], b[c]), "base bytes of item %d" % i
    check_same_planes(P, Q)


@gpu
def test_models_equal_the_gather_forms(three_groups, three_group_handles):
    """256 columns through the byte-plane kernel, cold and warm-started from the cold model with
    another l2, on the planes of either form: EQUAL models, the same bytes of G streamed."""
    (ms, _), (mg, _) = three_group_handles
    cols = np.arange(0, NI3, NI3 // 256, dtype=np.int32)[:256]
    kw = dict(kernel=KERNEL_GRAM, columns=cols, seed=2, l1r=1.0, l2r=1.0)
    Ws, ss = ms.learn(**kw)
    Wg, sg = mg.learn(**kw)
    assert Ws.nnz > 1000 and maxdiff(Ws, Wg) == 0.0
    assert 0 < ss["gram_bytes"] == sg["gram_bytes"] < ss["gram_rows"] * 4.0 * NI3   # (the packed kernel ran)
    Ws2, ss2 = ms.learn(imodel=Ws, **dict(kw, l2r=3.0))
    Wg2, sg2 = mg.learn(imodel=Wg, **dict(kw, l2r=3.0))
    assert Ws2.nnz > 1000 and maxdiff(Ws2, Wg2) == 0.0 and maxdiff(Ws2, Ws) > 0.0
    assert 0 < ss2["gram_bytes"] == sg2["gram_bytes"]


# ---- 3. the third plane -------------------------------------------------------------------------
@gpu
def test_third_plane_of_three_hot_items():
    """70 000 users x 40 items, items 0-2 rated by all: entries of 70 000."""
    rng = np.random.default_rng(3)
    R = sp.random(70000, 40, density=0.2, format="lil", random_state=rng, dtype=np.float32)
    R[:, :3] = 1.0
    R = sp.csr_matrix(R)
    R.data[:] = 1.0
    R.sort_indices()
    P = both_ways(R, True)
    assert P["hi2_k"].max() == 1 and P["hi_k"].max() == 1


@gpu
def test_third_plane_in_every_row():
    """60 000 x 400 at density 0.3 with ratings 1-5: nearly every entry beyond 65 535."""
    rng = np.random.default_rng(21)
    R = sp.random(60000, 400, density=0.3, format="csr", random_state=rng, dtype=np.float32)
    R.data = rng.choice(np.arange(1, 6), size=R.nnz, p=[.05, .05, .1, .3, .5]).astype(np.float32)
    R.sort_indices()
    P = both_ways(R, False)
    assert (P["hi2_k"] == 1).all() and (P["hi_k"] == 1).all()


# ---- 4. integer ratings, and what cannot be packed ----------------------------------------------
@gpu
def test_integer_ratings():
    both_ways(random_ratings(40000, 3000, 0.004, 5, binary=False), False)


@gpu
@pytest.mark.parametrize("how", ["one-rating-halved", "all-halved"])
def test_refuses_a_gram_matrix_that_is_not_integer_valued(how):
    """The matrix of test_integer_ratings with ONE rating set to 0.5 (a few entries of G end in .5:
    the scan has to see them among 9 million) and with all ratings halved: no planes, a solve with
    KERNEL_GRAM runs the float kernel, and all of it as with SLIM_GPU_PACK_GATHER=1."""
    R = random_ratings(40000, 3000, 0.004, 5, binary=False)
    if how == "all-halved":
        R.data *= 0.5
    else:
        u = 20000
        assert R.indptr[u + 1] - R.indptr[u] >= 2
        R.data[R.indptr[u]] = 0.5
        G = np.asarray((R.T.astype(np.float64) @ R.astype(np.float64)).todense())
        assert 0 < (G != np.floor(G)).sum() <= 2 * 64
    cols = np.arange(0, 3000, 47, dtype=np.int32)
    models = []
    for gather in (False, True):
        mat, forms = committed(R, False, gather)
        assert forms == [], forms
        with pytest.raises(RuntimeError, match="no byte planes"):
            mat.gram_planes()
        W, st = mat.learn(kernel=KERNEL_GRAM, columns=cols, seed=2, l1r=0.25, l2r=0.25)
        assert st["kernel"] == KERNEL_GRAM and st["gram_bytes"] == st["gram_rows"] * 4.0 * 3008   # (floats)
        assert st["gram_build_ms"] == 0 and W.nnz > 0
        models.append(W)
        mat.close()
    assert maxdiff(models[0], models[1]) == 0.0


# ---- 5. row blocks ------------------------------------------------------------------------------
@gpu
def test_row_blocks_then_commit():
    """G built in three gram_build_rows blocks and then committed: the planes of the one-call build."""
    R = random_ratings(20000, 600, 0.02, 9, binary=True)
    P = planes_of(R, True, gather=False)
    Pb = planes_of(R, True, gather=False, blocks=((0, 170), (170, 171), (171, 600)))
    check_against_host(Pb, R)
    check_same_planes(Pb, P, "three row blocks vs one call")
