"""The G builder's store form (cd_tile.hpp, gram_store_lines: a tile's sums leave in 256-byte runs of
64 consecutive column ids) and the pass that fills the mirror half after the build's last launch
(gram_sym.hpp), on the path that forms all of G in one work list -- the build inside learn.

G is read through SLIMGPU_MatrixGramView before any commit and compared, entry for entry, with
R^T R formed in int64 on the host, and with the G of the form before both (SLIM_GPU_GLINES=0: one
thread per entry, mirror stores from the tile kernel), which must hold the same bits.  The pad
columns are zero and G equals its transpose exactly.  Shapes sit around the 64-column run and the
32-item tile; every matrix has unrated columns and one column that every user rated."""
import re

import numpy as np
import pytest
import scipy.sparse as sp

from slim_amd.engine import KERNEL_GRAM, DeviceMatrix

pytestmark = pytest.mark.gpu

FORM = re.compile(r"\[trace\] G builder: form (\w+), clusters of (\d+), pass (\d+) of (\d+)")
MIRROR = re.compile(r"\[trace\] G builder: mirror half filled")
PASSES = {"SLIM_GPU_TEST_HOOKS": "1", "SLIM_GPU_TEST_GBITS_ROWS": "300"}
SWITCHES = ("SLIM_GPU_GLINES", "SLIM_GPU_GBITS", "SLIM_GPU_NO_GBITS", "SLIM_GPU_NO_GPASSES", "SLIM_GPU_TEST_HOOKS",
            "SLIM_GPU_TEST_GBITS_ROWS", "SLIM_GPU_GPART16", "SLIM_GPU_GVIEW")
NCOLS = [31, 33, 63, 64, 65, 97, 129]


@pytest.fixture(autouse=True)
def _env(monkeypatch):
    monkeypatch.setenv("SLIM_GPU_TRACE", "1")
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)


def matrix(ncols, kind, nu=1500, seed=3):
    """nu users, ~3 % dense; items ncols // 2 and ncols // 3 unrated, item 1 rated by every user, the
    last item rated (the staging takes ncols from the ids).  kind: binary, ratings (1-5) or signed
    (fractional, both signs: sums that are negative or cancel in part)."""
    rng = np.random.default_rng(seed + 7 * ncols)
    mask = rng.random((nu, ncols)) < 0.03
    mask[:, 1] = True
    mask[:, ncols // 2] = False
    mask[:, ncols // 3] = False
    mask[nu // 2, ncols - 1] = True
    R = sp.csr_matrix(mask.astype(np.float32))
    if kind == "ratings":
        R.data[:] = rng.integers(1, 6, R.nnz).astype(np.float32)
    elif kind == "signed":
        R.data[:] = rng.uniform(-2.0, 2.5, R.nnz).astype(np.float32)
    nnz_col = np.diff(sp.csc_matrix(R).indptr)
    assert nnz_col[1] == nu and nnz_col[ncols // 2] == 0 and nnz_col[ncols // 3] == 0 and nnz_col[-1] > 0
    return R


def reference(R):
    Rh = sp.csr_matrix(R).astype(np.int64)
    assert np.array_equal(Rh.data, sp.csr_matrix(R).data), "ratings are not integers"
    Gref = np.asarray((Rh.T @ Rh).todense())
    assert Gref.max() < 2 ** 24
    return Gref.astype(np.float32)


def read_gram(mat):
    import torch
    torch.cuda.synchronize()
    return mat.gram_rows_tensor(0, mat.ncols).cpu().numpy().copy()


def full_build(R, binary, monkeypatch, capfd, env=None, glines=None):
    """The build inside learn on a fresh handle (all rows in one work list) -> (G as numpy (ncols, ld),
    the model, the builder's launches, how many times the mirror pass ran, stderr)."""
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in (env or {}).items():
        monkeypatch.setenv(k, v)
    if glines is not None:
        monkeypatch.setenv("SLIM_GPU_GLINES", str(glines))
    mat = DeviceMatrix.from_scipy(R, binary=binary)
    assert mat.ncols == R.shape[1]
    capfd.readouterr()
    W, stats = mat.learn(kernel=KERNEL_GRAM, columns=np.arange(min(6, mat.ncols), dtype=np.int32), niters=20)
    err = capfd.readouterr().err
    assert stats["kernel"] == KERNEL_GRAM and stats["gram_build_ms"] > 0
    G = read_gram(mat)
    mat.close()
    return G, W, FORM.findall(err), len(MIRROR.findall(err)), err


def check_exact(G, Gref):
    ncols = Gref.shape[0]
    assert G.dtype == np.float32 and G.shape[0] == ncols and G.shape[1] >= ncols and G.shape[1] % 64 == 0
    bad = np.argwhere(G[:, :ncols] != Gref)
    assert bad.size == 0, "G vs R^T R: %d entries differ, first %s" % (len(bad), bad[:8].tolist())
    assert not G[:, ncols:].any(), "writes into the pad columns"
    assert np.array_equal(G[:, :ncols], G[:, :ncols].T)


def same_bits(G, H):
    return G.shape == H.shape and np.array_equal(G.view(np.uint32), H.view(np.uint32))


FORMS = [({}, "binary", "bits2"), ({"SLIM_GPU_GBITS": "1"}, "binary", "bits1"),
         ({"SLIM_GPU_NO_GBITS": "1"}, "binary", "lines"), ({}, "ratings", "lines")]


@pytest.mark.parametrize("env,kind,form", FORMS, ids=["bits2", "bits1", "lines", "lines-ratings"])
@pytest.mark.parametrize("ncols", NCOLS)
def test_every_form_at_the_run_and_tile_edges(monkeypatch, capfd, ncols, env, kind, form):
    """Item counts around the 64-column run and the 32-item tile (from 97 on, tiles start at odd
    multiples of 32; 31 and 33: one partial run; 65, 129: a run of one column), every form of the
    counting pass: whole lines + the mirror pass hold R^T R exactly, and the bits of the form before."""
    R = matrix(ncols, kind)
    Gref = reference(R)
    G, _, ls, nmirror, _ = full_build(R, kind == "binary", monkeypatch, capfd, env)
    assert ls and {l[0] for l in ls} == {form} and nmirror == 1, (ls, nmirror)
    check_exact(G, Gref)
    G1, _, ls1, nmirror1, _ = full_build(R, kind == "binary", monkeypatch, capfd, env, glines=1)
    assert {l[0] for l in ls1} == {form} and nmirror1 == 0
    check_exact(G1, Gref)
    G0, _, ls0, nmirror0, _ = full_build(R, kind == "binary", monkeypatch, capfd, env, glines=0)
    assert {l[0] for l in ls0} == {form} and nmirror0 == 0
    check_exact(G0, Gref)
    assert same_bits(G, G0) and same_bits(G1, G0)


@pytest.mark.parametrize("ncols", [97, 129])
def test_user_passes_accumulate_and_the_mirror_pass_comes_last(monkeypatch, capfd, ncols):
    """bits2 in user passes (a pretended capacity of 300 rows against 625 users per member): the
    later passes add into G through the same runs, and the mirror pass runs once, after the last."""
    R = matrix(ncols, "binary", nu=20000)
    Gref = reference(R)
    G, _, ls, nmirror, err = full_build(R, True, monkeypatch, capfd, PASSES)
    npass = int(ls[0][3])
    assert npass > 1 and [int(l[2]) for l in ls] == list(range(1, npass + 1)) and {l[0] for l in ls} == {"bits2"}, ls
    assert nmirror == 1 and MIRROR.search(err).start() > max(m.start() for m in FORM.finditer(err))
    check_exact(G, Gref)
    G0, _, ls0, nmirror0, _ = full_build(R, True, monkeypatch, capfd, PASSES, glines=0)
    assert len(ls0) == npass and nmirror0 == 0
    assert same_bits(G, G0)


@pytest.mark.parametrize("ncols", [33, 97, 129])
def test_signed_fractional_ratings_keep_their_bits(monkeypatch, capfd, ncols):
    """Ratings in [-2, 2.5): the members' sums are added in the same order and the mirror pass goes by
    position, not by value, so the three forms hold the same bits -- negative sums among them --, the
    transpose is exact across tiles, and the sums are right within float32 rounding."""
    R = matrix(ncols, "signed")
    G, _, ls, nmirror, _ = full_build(R, False, monkeypatch, capfd)
    assert {l[0] for l in ls} == {"lines"} and nmirror == 1
    G1 = full_build(R, False, monkeypatch, capfd, glines=1)[0]
    G0 = full_build(R, False, monkeypatch, capfd, glines=0)[0]
    assert same_bits(G, G0) and same_bits(G1, G0)
    assert (G < 0).any() and not G[:, ncols:].any()
    R64 = sp.csr_matrix(R).astype(np.float64)
    Gref = np.asarray((R64.T @ R64).todense())
    A64 = abs(R64)
    bound = (1500 + 33) * 2.0 ** -24 * np.asarray((A64.T @ A64).todense())  # (any order of float32 summation)
    assert (np.abs(G[:, :ncols] - Gref) <= bound).all()
    # the two entries of a pair inside one tile are both formed by that tile, over either item's users
    mat = DeviceMatrix.from_scipy(R, binary=False)
    order = np.argsort(-mat.column_cost(), kind="stable")
    mat.close()
    pos = np.empty(ncols, np.int64)
    pos[order] = np.arange(ncols)
    apart = (pos // 32)[:, None] != (pos // 32)[None, :]
    assert not ((G[:, :ncols] != G[:, :ncols].T) & apart).any()


@pytest.mark.parametrize("kind", ["binary", "ratings"])
def test_row_blocks_equal_the_rows_of_the_full_build(monkeypatch, capfd, kind):
    """SLIMGPU_MatrixGramBuildRows keeps the mirror stores in the tile kernel and runs no pass: blocks
    whose edges are off the 32 and 64 grids hold the rows of the full build."""
    ncols = 129
    R = matrix(ncols, kind)
    G, _, _, nmirror, _ = full_build(R, kind == "binary", monkeypatch, capfd)
    assert nmirror == 1
    check_exact(G, reference(R))
    for b, e in ((0, 1), (17, 45), (33, 97), (63, 65), (100, 129), (0, 129)):
        mat = DeviceMatrix.from_scipy(R, binary=kind == "binary")
        capfd.readouterr()
        mat.gram_build_rows(b, e)
        err = capfd.readouterr().err
        assert FORM.search(err) and not MIRROR.search(err)
        Gb = read_gram(mat)
        mat.close()
        assert same_bits(Gb[b:e], G[b:e]), (b, e)


@pytest.mark.parametrize("kind", ["binary", "ratings"])
def test_the_model_of_a_solve_is_the_same(monkeypatch, capfd, kind):
    """The item-space solve that follows the build: the same model, bit for bit, from either form."""
    R = matrix(129, kind)
    _, W, _, nmirror, _ = full_build(R, kind == "binary", monkeypatch, capfd)
    _, W0, _, nmirror0, _ = full_build(R, kind == "binary", monkeypatch, capfd, glines=0)
    assert nmirror == 1 and nmirror0 == 0 and W.nnz > 0
    W, W0 = sp.csc_matrix(W), sp.csc_matrix(W0)
    assert np.array_equal(W.indptr, W0.indptr) and np.array_equal(W.indices, W0.indices)
    assert np.array_equal(W.data.view(np.uint32), W0.data.view(np.uint32))
