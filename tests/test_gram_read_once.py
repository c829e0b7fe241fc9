"""The G builder's read-once sum (cd_tile.hpp, gram_store_lines with SolveArgs::gram_read): a wavefront
takes the members' partial sums of a 64-column block a quarter at a time -- 16 columns, every 16-byte
piece requested once -- and turns them into the 256-byte runs of G through a staging tile in LDS.

G is read through SLIMGPU_MatrixGramView before any commit and held to R^T R formed in int64 on the
host, to the bits of the four-round read (SLIM_GPU_GREAD=0) and of the form before whole lines
(SLIM_GPU_GLINES=0).  The trace names the read that ran: every case asserts which, so a launch that
fell back to the four rounds cannot pass as the new path.  Shapes sit around the quarter (16 columns),
the run (64) and the 32-item tile.

(The narrowed clear of a fresh G and its poison hook are not in the build -- profiles/r10 has why --,
so there is no poison case here: every build clears all of G, as before.)"""
import re

import numpy as np
import pytest
import scipy.sparse as sp

from slim_amd.engine import KERNEL_GRAM, DeviceMatrix

pytestmark = pytest.mark.gpu

FORM = re.compile(r"\[trace\] G builder: form (\w+), clusters of (\d+), pass (\d+) of (\d+)")
ONCE = re.compile(r"\[trace\] G builder: sums read once")
ROUNDS = re.compile(r"\[trace\] G builder: sums read in rounds \(([^)]*)\)")
MIRROR = re.compile(r"\[trace\] G builder: mirror half filled")
PASSES = {"SLIM_GPU_TEST_HOOKS": "1", "SLIM_GPU_TEST_GBITS_ROWS": "300"}
SWITCHES = ("SLIM_GPU_GLINES", "SLIM_GPU_GREAD", "SLIM_GPU_GBITS", "SLIM_GPU_NO_GBITS", "SLIM_GPU_NO_GPASSES",
            "SLIM_GPU_TEST_HOOKS", "SLIM_GPU_TEST_GBITS_ROWS", "SLIM_GPU_GPART16",
            "SLIM_GPU_GVIEW", "SLIM_GPU_TILE_NW")
FORMS = [({}, "binary", "bits2"), ({"SLIM_GPU_GBITS": "1"}, "binary", "bits1"),
         ({"SLIM_GPU_NO_GBITS": "1"}, "binary", "lines"), ({}, "ratings", "lines")]
FORM_IDS = ["bits2", "bits1", "lines", "lines-ratings"]


@pytest.fixture(autouse=True)
def _env(monkeypatch):
    monkeypatch.setenv("SLIM_GPU_TRACE", "1")
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)


def matrix(ncols, kind, nu=1500, seed=5, every=(1,)):
    """nu users, ~3 % dense; items ncols // 2 and ncols // 3 unrated, the items of `every` rated by
    every user, the last item rated (the staging takes ncols from the ids).  kind: binary, ratings
    (1-5) or signed (fractional, both signs)."""
    rng = np.random.default_rng(seed + 11 * ncols)
    mask = rng.random((nu, ncols)) < 0.03
    for c in every:
        mask[:, c] = True
    mask[:, ncols // 2] = False
    mask[:, ncols // 3] = False
    mask[nu // 2, ncols - 1] = True
    R = sp.csr_matrix(mask.astype(np.float32))
    if kind == "ratings":
        R.data[:] = rng.integers(1, 6, R.nnz).astype(np.float32)
    elif kind == "signed":
        R.data[:] = rng.uniform(-2.0, 2.5, R.nnz).astype(np.float32)
    nnz_col = np.diff(sp.csc_matrix(R).indptr)
    assert all(nnz_col[c] == nu for c in every) and nnz_col[ncols // 2] == 0 and nnz_col[ncols // 3] == 0
    assert nnz_col[-1] > 0
    return R


_REF = {}


def reference(R, key):
    """R^T R in int64, once per matrix (the tests only read it)."""
    if key not in _REF:
        Rh = sp.csr_matrix(R).astype(np.int64)
        assert np.array_equal(Rh.data, sp.csr_matrix(R).data), "ratings are not integers"
        Gref = np.asarray((Rh.T @ Rh).todense())
        assert Gref.max() < 2 ** 24
        Gref = Gref.astype(np.float32)
        Gref.setflags(write=False)
        _REF[key] = Gref
    return _REF[key]


def read_gram(mat):
    import torch
    torch.cuda.synchronize()
    return mat.gram_rows_tensor(0, mat.ncols).cpu().numpy().copy()


def full_build(R, binary, monkeypatch, capfd, env=None):
    """The build inside learn on a fresh handle (all rows in one work list) -> (G as numpy (ncols, ld),
    the model, stderr)."""
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in (env or {}).items():
        monkeypatch.setenv(k, v)
    mat = DeviceMatrix.from_scipy(R, binary=binary)
    assert mat.ncols == R.shape[1]
    capfd.readouterr()
    W, stats = mat.learn(kernel=KERNEL_GRAM, columns=np.arange(min(6, mat.ncols), dtype=np.int32), niters=20)
    err = capfd.readouterr().err
    assert stats["kernel"] == KERNEL_GRAM and stats["gram_build_ms"] > 0
    G = read_gram(mat)
    mat.close()
    return G, W, err


def reads(err):
    """(launches of the builder, of them: read once, read in rounds with their reasons)"""
    return len(FORM.findall(err)), len(ONCE.findall(err)), ROUNDS.findall(err)


def check_exact(G, Gref):
    ncols = Gref.shape[0]
    assert G.dtype == np.float32 and G.shape[0] == ncols and G.shape[1] >= ncols and G.shape[1] % 64 == 0
    assert not np.isnan(G).any(), "entries that nobody wrote"
    bad = np.argwhere(G[:, :ncols] != Gref)
    assert bad.size == 0, "G vs R^T R: %d entries differ, first %s" % (len(bad), bad[:8].tolist())
    assert not G[:, ncols:].any(), "the pad columns are not zero"
    assert np.array_equal(G[:, :ncols], G[:, :ncols].T)


def same_bits(G, H):
    return G.shape == H.shape and np.array_equal(G.view(np.uint32), H.view(np.uint32))


@pytest.mark.parametrize("env,kind,form", FORMS, ids=FORM_IDS)
@pytest.mark.parametrize("ncols", [15, 16, 17, 47, 48, 49, 64, 79, 80, 81, 129, 193])
def test_quarter_run_edges(monkeypatch, capfd, ncols, env, kind, form):
    """Item counts around the 16-column quarter of a run, in every form of the counting pass: the
    read-once sum holds R^T R exactly, zero pads, a symmetric G, and the bits of the four-round read.
    Every form's launch holds the staging tiles (16 wavefronts: 135 168 bytes next to 19 KB of static
    LDS), so the default must be the read-once body, and SLIM_GPU_GREAD=0 the rounds."""
    R = matrix(ncols, kind)
    Gref = reference(R, (ncols, kind))
    G, _, err = full_build(R, kind == "binary", monkeypatch, capfd, env)
    assert {l[0] for l in FORM.findall(err)} == {form} and len(MIRROR.findall(err)) == 1
    assert reads(err) == (1, 1, []), err
    check_exact(G, Gref)
    G4, _, err4 = full_build(R, kind == "binary", monkeypatch, capfd, dict(env, SLIM_GPU_GREAD="0"))
    assert {l[0] for l in FORM.findall(err4)} == {form}
    assert reads(err4) == (1, 0, ["SLIM_GPU_GREAD=0"]), err4
    check_exact(G4, Gref)
    assert same_bits(G, G4)


@pytest.mark.parametrize("ncols", [49, 129])
def test_workgroups_of_eight_wavefronts_hold_their_tiles(monkeypatch, capfd, ncols):
    """SLIM_GPU_TILE_NW=8 on the line-gathering form: two workgroups per CU, 67 584 bytes of staging
    tiles each -- still the read-once body, the same bits as the rounds."""
    R = matrix(ncols, "ratings")
    env = {"SLIM_GPU_TILE_NW": "8"}
    G, _, err = full_build(R, False, monkeypatch, capfd, env)
    assert "P 32, 8 wavefronts" in err and reads(err) == (1, 1, []), err
    check_exact(G, reference(R, (ncols, "ratings")))
    G4, _, err4 = full_build(R, False, monkeypatch, capfd, dict(env, SLIM_GPU_GREAD="0"))
    assert reads(err4) == (1, 0, ["SLIM_GPU_GREAD=0"])
    assert same_bits(G, G4)


def test_counts_in_both_half_words_and_across_members(monkeypatch, capfd):
    """20 000 users, 97 columns, items 1 and 2 rated by every user: each of the 32 members holds 625
    in the low (item at an even tile slot) or high half of a word, and their sum, 20 000, needs the
    carry out of no single member's 16 bits.  One launch and user passes (a pretended capacity of 300
    rows: the later passes add into G through the same staging tile): exact, and the bits of the
    form before whole lines."""
    ncols = 97
    R = matrix(ncols, "binary", nu=20000, every=(1, 2))
    Gref = reference(R, (ncols, "binary", 20000))
    assert Gref[1, 2] == 20000 and Gref[1, 1] == 20000
    G, _, err = full_build(R, True, monkeypatch, capfd)
    assert {l[0] for l in FORM.findall(err)} == {"bits2"} and reads(err) == (1, 1, [])
    check_exact(G, Gref)
    G0, _, err0 = full_build(R, True, monkeypatch, capfd, {"SLIM_GPU_GLINES": "0"})
    assert reads(err0) == (1, 0, []) and not MIRROR.search(err0)
    assert same_bits(G, G0)
    Gp, _, errp = full_build(R, True, monkeypatch, capfd, PASSES)
    ls = FORM.findall(errp)
    npass = int(ls[0][3])
    assert npass > 1 and [int(l[2]) for l in ls] == list(range(1, npass + 1)) and {l[0] for l in ls} == {"bits2"}
    assert reads(errp) == (npass, npass, []), errp
    check_exact(Gp, Gref)
    Gp0, _, errp0 = full_build(R, True, monkeypatch, capfd, dict(PASSES, SLIM_GPU_GLINES="0"))
    assert len(FORM.findall(errp0)) == npass and reads(errp0)[1:] == (0, [])
    assert same_bits(Gp, Gp0)


@pytest.mark.parametrize("ncols", [49, 129])
def test_signed_fractional_ratings_keep_their_bits(monkeypatch, capfd, ncols):
    """Ratings in [-2, 2.5): the K partial sums of an entry are added in member order by all three
    bodies, so they hold the same bits, negative sums among them."""
    R = matrix(ncols, "signed")
    G, _, err = full_build(R, False, monkeypatch, capfd)
    assert {l[0] for l in FORM.findall(err)} == {"lines"} and reads(err) == (1, 1, [])
    G4, _, err4 = full_build(R, False, monkeypatch, capfd, {"SLIM_GPU_GREAD": "0"})
    assert reads(err4) == (1, 0, ["SLIM_GPU_GREAD=0"])
    G0, _, err0 = full_build(R, False, monkeypatch, capfd, {"SLIM_GPU_GLINES": "0"})
    assert reads(err0) == (1, 0, [])
    assert same_bits(G, G4) and same_bits(G, G0)
    assert (G < 0).any() and not np.isnan(G).any() and not G[:, ncols:].any()


@pytest.mark.parametrize("kind", ["binary", "ratings"])
def test_row_blocks_equal_the_rows_of_the_full_build(monkeypatch, capfd, kind):
    """SLIMGPU_MatrixGramBuildRows (mirror stores in the tile kernel, no pass) reads once as well;
    blocks off the 16, 32 and 64 grids hold the rows of the full build."""
    ncols = 129
    R = matrix(ncols, kind)
    G, _, err = full_build(R, kind == "binary", monkeypatch, capfd)
    assert reads(err) == (1, 1, [])
    check_exact(G, reference(R, (ncols, kind)))
    for b, e in ((17, 45), (63, 65)):
        mat = DeviceMatrix.from_scipy(R, binary=kind == "binary")
        capfd.readouterr()
        mat.gram_build_rows(b, e)
        err = capfd.readouterr().err
        assert reads(err) == (1, 1, []) and not MIRROR.search(err), err
        Gb = read_gram(mat)
        mat.close()
        assert not np.isnan(Gb).any()
        assert same_bits(Gb[b:e], G[b:e]), (b, e)


@pytest.mark.parametrize("kind", ["binary", "ratings"])
def test_the_model_of_a_solve_is_the_same(monkeypatch, capfd, kind):
    """The item-space solve that follows the build: the same model, bit for bit, from either read."""
    R = matrix(129, kind)
    _, W, err = full_build(R, kind == "binary", monkeypatch, capfd)
    _, W4, err4 = full_build(R, kind == "binary", monkeypatch, capfd, {"SLIM_GPU_GREAD": "0"})
    assert reads(err) == (1, 1, []) and reads(err4) == (1, 0, ["SLIM_GPU_GREAD=0"]) and W.nnz > 0
    W, W4 = sp.csc_matrix(W), sp.csc_matrix(W4)
    assert np.array_equal(W.indptr, W4.indptr) and np.array_equal(W.indices, W4.indices)
    assert np.array_equal(W.data.view(np.uint32), W4.data.view(np.uint32))
