"""The bit-sliced G builder reading its ids from the 16-bit, range-relative view interleaved by
groups of 64 work-list positions (engine.hip, build_gview; cd_tile.hpp, S.gview) against the same
builder reading the column view (SLIM_GPU_GVIEW=0): every case builds G both ways, proves from the
builder's trace line which id source ran, and compares G with R^T R in int64 on the host -- every
entry, the symmetry, the diagonal, zeros in the padding (check_gram of test_gram_builder) -- never
only with the other path.

The padding of the view (its bytes over 2 bytes per nnz) is in the trace line.  A slice is stored
in pieces of 8 ids, the last one filled up, and a row of a group's block holds the pieces of the
lanes that still have one: the view is the sum of every slice's length / 8, rounded up, times 16
bytes.  The random case's slices are ~12.5 ids long (400 per column over 32 members), mostly two
pieces: ~1.3, under the bound of 1.5 set for this matrix (rows of all 64 lanes up to the group's
longest slice, ~21 ids there, would be 2.078).  Computed on the host from the slice lengths and
reported the same by the engine."""
import re

import numpy as np
import pytest
import scipy.sparse as sp

from slim_amd.engine import KERNEL_GRAM, DeviceMatrix
from test_gram_builder import (BLOCK_PASSES, LADDER, NFILL, PASSES, PER, TRACE, check_gram, edge_matrix, ladder,  # noqa: F401
                               random_binary, ran_as, read_gram, reference, setenv, work_positions)

pytestmark = pytest.mark.gpu

SOURCE = re.compile(r"\[trace\] G builder: ids from (view|csc)"
                    r"(?:, (\d+) bytes = ([0-9.]+) x 2 bytes per nnz, built in ([0-9.]+) ms)?")
SOURCES = [("view", None), ("csc", "0")]   # (what the trace line must say, SLIM_GPU_GVIEW)


@pytest.fixture(autouse=True)
def _trace(monkeypatch):
    monkeypatch.setenv("SLIM_GPU_TRACE", "1")
    for k in ("SLIM_GPU_GBITS", "SLIM_GPU_NO_GBITS", "SLIM_GPU_NO_GPASSES", "SLIM_GPU_TEST_HOOKS",
              "SLIM_GPU_TEST_GBITS_ROWS", "SLIM_GPU_GVIEW", "SLIM_GPU_GPART16"):
        monkeypatch.delenv(k, raising=False)


def traced(capfd):
    """(the builder's launches, the id source lines) since the last look at stderr."""
    err = capfd.readouterr().err
    ls = [(f, int(k), int(p), int(n), int(r)) for f, k, p, n, r in TRACE.findall(err)]
    return ls, SOURCE.findall(err)


def select(monkeypatch, gview):
    if gview is None:
        monkeypatch.delenv("SLIM_GPU_GVIEW", raising=False)
    else:
        monkeypatch.setenv("SLIM_GPU_GVIEW", gview)


def ran_from(ls, src, source, nnz):
    """Every launch named its id source, all the same one; the view's bytes are whole pieces of
    16 bytes and its padding figure is those bytes over 2 nnz.  -> the padding (view only)."""
    assert len(src) == len(ls) and {s[0] for s in src} == {source}, (ls, src)
    if source != "view":
        return None
    assert len({s[1] for s in src}) == 1, src   # one view per build, shared by its passes
    nbytes, ratio = int(src[0][1]), float(src[0][2])
    assert nbytes > 0 and nbytes % 16 == 0 and abs(ratio - nbytes / (2.0 * nnz)) < 1e-3, src
    return ratio


def build_checked(R, monkeypatch, capfd, source, gview, passes=1, block=None, Gref=None):
    """G (rows `block`) on a fresh handle with that id source: ran as bits2 from it, equals R^T R."""
    select(monkeypatch, gview)
    mat = DeviceMatrix.from_scipy(R, binary=True)
    capfd.readouterr()
    b, e = block if block is not None else (0, mat.ncols)
    mat.gram_build_rows(b, e)
    ls, src = traced(capfd)
    if passes is None:
        passes = ls[0][3]
        assert passes > 1, ls
    ran_as(ls, "bits2", passes)
    ratio = ran_from(ls, src, source, R.nnz)
    check_gram(read_gram(mat), R, mat, Gref, block=block, rows=block)
    mat.close()
    return ratio


def split_bounds(R, nr=32):
    """The engine's equal-nnz user ranges (ensure_split): range j starts at the first user whose row
    pointer reaches j nnz / nr."""
    rowptr = sp.csr_matrix(R).indptr.astype(np.int64)
    ub = [0] + [int(np.searchsorted(rowptr, R.nnz // nr * j, side="left")) for j in range(1, nr)] + [R.shape[0]]
    return np.maximum.accumulate(np.minimum(ub, R.shape[0]))


def slice_lengths(R, ub, order):
    """[work-list position][range]: ids of that column inside that user range."""
    coo = sp.coo_matrix(R)
    L = np.zeros((R.shape[1], len(ub) - 1), np.int64)
    np.add.at(L, (coo.col, np.searchsorted(ub, coo.row, side="right") - 1), 1)
    return L[order]


def view_pieces(L):
    """Pieces of 8 ids the view holds: every slice's length / 8, rounded up."""
    return int(((L + 7) // 8).sum())


def view_rows(L):
    """Rows of every (group of 64 positions, range): the longest slice of the group / 8, rounded up."""
    n, nr = L.shape
    Lp = np.zeros(((n + 63) // 64 * 64, nr), np.int64)
    Lp[:n] = L
    return (Lp.reshape(-1, 64, nr).max(axis=1) + 7) // 8


# ---- 1. random ----------------------------------------------------------------------------------
@pytest.mark.parametrize("source,gview", SOURCES)
@pytest.mark.parametrize("env,passes", [({}, 1), (PASSES, 5), ({"SLIM_GPU_GPART16": "0"}, 1)],
                         ids=["one-launch", "passes", "float-partials"])
def test_random(random_binary, monkeypatch, capfd, env, passes, source, gview):
    """40 000 x 600 at 1 %: in one launch, and in five user passes whose later four add into G and
    read their own 32 ranges' blocks of the one view; and with the members' partial counts left as
    floats (SLIM_GPU_GPART16=0) instead of 16-bit numbers."""
    R, Gref = random_binary
    setenv(monkeypatch, env)
    build_checked(R, monkeypatch, capfd, source, gview, passes=passes, Gref=Gref)


def test_padding_of_the_random_case(random_binary, monkeypatch, capfd):
    """The view's padding on the random case in one launch, <= 1.5 as set for it: slices of 12.5
    ids on average, two pieces of 8 for most of them -- see the module's docstring.  The engine's
    figure is checked against the slice lengths first."""
    R, Gref = random_binary
    select(monkeypatch, None)
    mat = DeviceMatrix.from_scipy(R, binary=True)
    order = np.argsort(work_positions(mat))
    capfd.readouterr()
    mat.gram_build_rows(0, mat.ncols)
    ls, src = traced(capfd)
    ratio = ran_from(ls, src, "view", R.nnz)
    mat.close()
    want = view_pieces(slice_lengths(R, split_bounds(R), order)) * 16 / (2.0 * R.nnz)
    print("padding of the view on the random case: %.3f (from the slice lengths: %.3f)" % (ratio, want))
    assert abs(ratio - want) < 1e-3
    assert ratio <= 1.5


# ---- 2. group edges -----------------------------------------------------------------------------
@pytest.mark.parametrize("source,gview", SOURCES)
@pytest.mark.parametrize("ncols", [1, 33, 63, 64, 65, 97, 129, 161])
def test_group_edges(monkeypatch, capfd, ncols, source, gview):
    """A partial last group, tiles whose base is an odd multiple of 32 (they start in the middle of a
    group: 33 .. 161 items), unrated items inside a group.  An entry written for a position in front
    of a tile's base would land in an earlier tile's rows or mirror entries: the comparison is with
    R^T R, every entry."""
    build_checked(edge_matrix(ncols, False), monkeypatch, capfd, source, gview)


@pytest.mark.parametrize("source,gview", SOURCES)
@pytest.mark.parametrize("ncols", [97, 129])
def test_group_edges_in_passes(monkeypatch, capfd, ncols, source, gview):
    """The same in user passes (two, see BLOCK_PASSES): a second add of a recounted position would
    double its entries."""
    setenv(monkeypatch, BLOCK_PASSES)
    build_checked(edge_matrix(ncols, False), monkeypatch, capfd, source, gview, passes=None)


# ---- 3. padding ---------------------------------------------------------------------------------
EDGE_NNZ = (0, 1, 7, 8, 9, 15, 16, 17, 63, 64, 65)
SPARSE_NNZ = EDGE_NNZ * 4 + (0,) * 19 + (1,)   # 64 items, 23 of them unrated; the last one is rated


def padding_matrix(spread, seed=13):
    """20 000 users x (20 + 64) items.  Items 0 .. 19 carry the bulk (every user rates about half of
    them: slices of ~300 ids); the 64 others have SPARSE_NNZ ratings -- spread=False: by the LAST
    users, all inside the last member's range; spread=True: by users spaced evenly.  The first and
    the last user of every member's range rate every bulk item (found as a fixed point: filling a
    row moves the equal-nnz bounds)."""
    nu = 20000
    rng = np.random.default_rng(seed)
    mask = np.zeros((nu, NFILL + len(SPARSE_NNZ)), bool)
    mask[:, :NFILL] = rng.random((nu, NFILL)) < 0.5
    for j, n in enumerate(SPARSE_NNZ):
        users = (np.arange(n) * nu) // max(n, 1) + j if spread else nu - 1 - np.arange(n)
        mask[users, NFILL + j] = True
    for _ in range(100):
        ub = split_bounds(sp.csr_matrix(mask.astype(np.float32)))
        ends = np.concatenate([ub[:-1], ub[1:] - 1])
        if mask[ends, :NFILL].all():
            break
        mask[ends, :NFILL] = True
    R = sp.csr_matrix(mask.astype(np.float32))
    ub = split_bounds(R)
    assert mask[np.concatenate([ub[:-1], ub[1:] - 1]), :NFILL].all() and (np.diff(ub) > 100).all()
    assert tuple(np.diff(sp.csc_matrix(R).indptr)[NFILL:]) == SPARSE_NNZ
    return R, ub


@pytest.mark.parametrize("source,gview", SOURCES)
@pytest.mark.parametrize("spread", [False, True], ids=["last-range", "spread"])
def test_padding(monkeypatch, capfd, spread, source, gview):
    """One group of 64 positions mixes lanes of several hundred ids with slices of 0, 1, 7 .. 9,
    15 .. 17, 63 .. 65 (last-range form; 0 .. 3 in the spread form); the second group holds 20 of the
    unrated items: every slice of a range is empty there (no rows at all).  The first and the last
    user of every member's range rate every bulk item: a sentinel that aliased local index 0 or the
    range's last would count."""
    R, ub = padding_matrix(spread)
    select(monkeypatch, gview)
    mat = DeviceMatrix.from_scipy(R, binary=True)
    L = slice_lengths(R, ub, np.argsort(work_positions(mat)))
    rows = view_rows(L)
    assert rows.shape == (2, 32) and (rows[1] == 0).any() and rows[0].min() >= 30
    if not spread:
        assert set(EDGE_NNZ) <= set(L[:64, 31]) and L[:64, 31].max() > 250
    else:
        assert {0, 1, 2} <= set(L[:64].ravel()) and L[:64].max() > 250
    capfd.readouterr()
    mat.gram_build_rows(0, mat.ncols)
    ls, src = traced(capfd)
    ran_as(ls, "bits2", 1)
    assert ls[0][4] == int(np.diff(ub).max()), (ls, np.diff(ub).max())   # the split assumed above is the engine's
    ratio = ran_from(ls, src, source, R.nnz)
    if source == "view":
        assert abs(ratio - view_pieces(L) * 16 / (2.0 * R.nnz)) < 1e-3
    check_gram(read_gram(mat), R, mat)
    mat.close()


# ---- 4. above 2^15 local users ------------------------------------------------------------------
@pytest.mark.parametrize("source,gview", SOURCES)
def test_relative_ids_above_two_to_the_fifteenth(ladder, monkeypatch, capfd, source, gview):   # noqa: F811
    """32 x 36 000 users: relative ids reach 35 999 and every user holds 8 ratings, the high ones
    too.  An id read as a signed 16-bit number, or a sentinel at or below 35 999, fails the counts."""
    R, Gref = ladder
    assert Gref[0, 0] == PER * 32 and LADDER[0] == PER > 2 ** 15
    build_checked(R, monkeypatch, capfd, source, gview, Gref=Gref)


# ---- 5. row blocks ------------------------------------------------------------------------------
@pytest.mark.parametrize("source,gview", SOURCES)
def test_row_blocks(monkeypatch, capfd, source, gview):
    """97 items: block (17, 45) alone, then (0, 17) -> (17, 45) -> (45, 97) on one handle -- every
    block partitions the work list its own way and gets its own view."""
    R = edge_matrix(97, False, seed=21)
    Gref = reference(R)
    build_checked(R, monkeypatch, capfd, source, gview, block=(17, 45), Gref=Gref)
    mat = DeviceMatrix.from_scipy(R, binary=True)
    capfd.readouterr()
    for blk in ((0, 17), (17, 45), (45, 97)):
        mat.gram_build_rows(*blk)
        ls, src = traced(capfd)
        ran_as(ls, "bits2", 1)
        ran_from(ls, src, source, R.nnz)
    check_gram(read_gram(mat), R, mat, Gref)
    mat.close()


# ---- 6. the build inside learn ------------------------------------------------------------------
def test_the_build_inside_learn(random_binary, monkeypatch, capfd):   # noqa: F811
    """learn(kernel=KERNEL_GRAM) builds G on the way, from the view or from the column view: the same
    G = R^T R, the same model; a second solve on the handle builds nothing."""
    R, Gref = random_binary
    cols = np.arange(5, 12, dtype=np.int32)
    W = {}
    for source, gview in SOURCES:
        select(monkeypatch, gview)
        mat = DeviceMatrix.from_scipy(R, binary=True)
        capfd.readouterr()
        W[source], s1 = mat.learn(kernel=KERNEL_GRAM, columns=cols, niters=50)
        ls, src = traced(capfd)
        ran_as(ls, "bits2", 1)
        ran_from(ls, src, source, R.nnz)
        assert s1["kernel"] == KERNEL_GRAM and s1["gram_build_ms"] > 0 and W[source].nnz > 0
        check_gram(read_gram(mat), R, mat, Gref)
        W2, s2 = mat.learn(kernel=KERNEL_GRAM, columns=cols, niters=50)
        ls, src = traced(capfd)
        assert s2["gram_build_ms"] == 0 and not ls and not src
        assert abs(W[source] - W2).nnz == 0
        mat.close()
    assert abs(W["view"] - W["csc"]).nnz == 0
