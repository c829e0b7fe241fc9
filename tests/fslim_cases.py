"""Fixtures of test_fslim_item_space_edges.py: the matrices, the oracle's walks over them (computed
once per process), the solver's plan restated from the sources, and the comparison with its bars.

Every matrix is seeded; its columns have a FIXED number of users drawn without replacement, so that
with binary ratings every column has the same norm and cos and jac tie wherever dotp ties."""
import functools
import os
import re

import numpy as np
import scipy.sparse as sp

import slim_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "slim_amd", "csrc")
SEED = 2
TRACE = re.compile(r"\[trace\] item-space FSLIM: form (block in LDS|gathered), lists of (\d+), (\d+) wavefronts per "
                   r"workgroup")


# ---- the solver's plan, restated (test_fixtures_do_their_job holds it to the sources) -------------
@functools.lru_cache(maxsize=None)
def constants():
    """kFslimMaxNbrs, kFslimBlockMaxStride, kFslimMaxWaves, kFslimUnionThreads of fslim_gram_inst.hpp; the LDS
    budget (KB) and the gathered form's wavefront limit of finish_path (engine.hip)."""
    hpp = open(os.path.join(CSRC, "fslim_gram_inst.hpp")).read()
    eng = open(os.path.join(CSRC, "engine.hip")).read()

    def const(name):
        return int(re.search(r"constexpr int %s = (\d+);" % name, hpp).group(1))
    waves = re.search(r"p\.f_waves = \(int\)std::max<size_t>\(1, std::min<size_t>\(p\.f_block \? kFslimMaxWaves : (\d+), "
                      r"\(size_t\((\d+)\) << 10\) / p\.f_wave_lds\)\);", eng)
    assert waves, "finish_path no longer sizes f_waves the way this module restates it"
    return dict(max_nbrs=const("kFslimMaxNbrs"), block_max_stride=const("kFslimBlockMaxStride"),
                max_waves=const("kFslimMaxWaves"), union_threads=const("kFslimUnionThreads"),
                select_threads=const("kFslimSelectThreads"), gathered_waves=int(waves.group(1)),
                budget_kb=int(waves.group(2)))


def round_up(a, b):
    return (a + b - 1) // b * b


def plan(ncols, nnbrs):
    """(form, stride, wavefronts per workgroup) as finish_path chooses them and fslim_wave_lds sizes
    a wavefront's share."""
    k = constants()
    stride = max(64, round_up(min(nnbrs, ncols - 1), 64))
    block = stride <= k["block_max_stride"]
    lds = 7 * 4 * stride + 128 * 4
    if block:
        lds += 2 * round_up(min(32 * stride, round_up(ncols, 64)), 8) + 4 * stride * stride
    lds = round_up(lds, 16)
    waves = max(1, min(k["max_waves"] if block else k["gathered_waves"], (k["budget_kb"] << 10) // lds))
    return ("block in LDS" if block else "gathered"), stride, waves


def union_chunk(ncols):
    """Bitmap words per thread of fslim_gram_union_kernel."""
    nt = constants()["union_threads"]
    return ((ncols + 31) // 32 + nt - 1) // nt


def select_segments(ncols):
    """How many of the select kernel's wavefronts own a piece of the row."""
    nw = constants()["select_threads"] // 64
    pad = round_up(ncols, 64)
    seg = (pad // 64 + nw - 1) // nw * 64
    return sum(1 for w in range(nw) if w * seg < pad)


# ---- matrices ----------------------------------------------------------------------------------------
def fixed_columns(nusers, ncols, per_col, seed, dyadic=False):
    """nusers x ncols CSR, every column with exactly per_col users drawn without replacement; ratings 1, or
    (dyadic) multiples of 1/4 up to 5: their products and sums are exact in fp32, so no entry of G -- hence no
    neighbour set -- depends on the order of a sum."""
    rng = np.random.default_rng(seed)
    rows = np.concatenate([np.sort(rng.choice(nusers, per_col, replace=False)) for _ in range(ncols)])
    vals = np.ones(rows.size, np.float32)
    if dyadic:
        vals = (rng.integers(1, 21, rows.size) * 0.25).astype(np.float32)
    Rc = sp.csc_matrix((vals, rows, np.arange(ncols + 1, dtype=np.int64) * per_col), shape=(nusers, ncols))
    R = sp.csr_matrix(Rc)
    R.sort_indices()
    return R


def candidates(R):
    """Co-rated columns per item."""
    B = sp.csr_matrix(R, dtype=np.float32, copy=True)
    B.data[:] = 1.0
    G = sp.csr_matrix(B.T @ B)
    G.setdiag(0)
    G.eliminate_zeros()
    return np.diff(G.indptr)


def all_pairs_corated(R):
    return bool(np.all(candidates(R) == R.shape[1] - 1))


SMALL_SIZES = (2, 3, 33, 63, 64, 65, 66, 127, 128, 129, 130, 192, 193, 256, 257)
SMALL_ALL_SIMTYPES = (2, 33, 64, 65, 66, 129, 130, 257)   # the other sizes run simtype 0 only
SMALL_CASES = [(n, s) for n in SMALL_SIZES for s in ((0, 1, 2) if n in SMALL_ALL_SIMTYPES else (0,))]
SMALL_KW = dict(l1r=1.0, l2r=1.0)


@functools.lru_cache(maxsize=None)
def small(ncols, dyadic=False):
    """400 users, columns of 120: the first seed at which every pair of columns is co-rated, so that
    nn = ncols - 1 for every problem and nunion = ncols for every tile of two or more."""
    for k in range(20):
        R = fixed_columns(400, ncols, 120, 5000 + 100 * k + ncols, dyadic)
        if all_pairs_corated(R):
            return R
    raise AssertionError("no seed co-rates every pair of %d columns" % ncols)


@functools.lru_cache(maxsize=None)
def big(dyadic=False):
    """3000 users, 8300 items, columns of 30: 260 bitmap words, 2 per thread of the union kernel; with dotp
    an entry of G is 1, 2 or 3, so nearly every list of 20 is cut inside a run of ties."""
    return fixed_columns(3000, 8300, 30, 8300, dyadic)


BIG_CASES = [(20, 0), (20, 1), (20, 2), (100, 0), (129, 0)]
BIG_TILES = (0, 1, 130, 259)    # the first two, a middle one, the last (12 problems)
BIG_KW = dict(l1r=1.0, l2r=1.0)


@functools.lru_cache(maxsize=None)
def long_lists(ncols=4200):
    """600 users, columns of 60: nearly every item is co-rated with every other."""
    return fixed_columns(600, ncols, 60, 4200 + ncols)


LONG_NNBRS = (1344, 1400, 1408, 1856, 2752, 4096)
LONG_WAVES = (4, 3, 3, 2, 1, 1)   # (1400 rounds up to lists of 1408: three wavefronts, as 1408)
LONG_KW = dict(l1r=2.0, l2r=1.0)
LONG_SIMTYPE = 2
LONG_SHARD = (43, 44)           # tiles 43, 87 and 131 of 132; the last holds 8 problems
PAST_SHARD = (42, 43)           # 4097 items: tiles 42, 85 and 128 of 129; the last holds 1 problem


@functools.lru_cache(maxsize=None)
def short_columns():
    """400 users x 130 items, columns of 120 -- except items 5 and 70 (1 user) and 9 and 100 (2 users), whose
    sweeps are capped at 50 and 100 (estimate.c:448-449)."""
    R = sp.lil_matrix(small(130))
    rng = np.random.default_rng(50)
    for item, n in ((5, 1), (70, 1), (9, 2), (100, 2)):
        R[:, item] = 0
        for u in rng.choice(400, n, replace=False):
            R[u, item] = 1.0
    R = sp.csr_matrix(R)
    R.eliminate_zeros()
    R.sort_indices()
    return R


SHORT_ITEMS = {5: 1, 70: 1, 9: 2, 100: 2}
# No penalties keep a short column from converging within 50 sweeps (tried: l1r / l2r = 1e-3 / 1e-3, 1e-2 / 1e-2,
# 0.1 / 0.01, 0.1 / 0.1, 0.5 / 0.1, lists of 20 and of 135: 5 to 7 sweeps each).  optTol = 0 does: `dlt < 0` never
# holds, so a column of 1 user stops at 50 sweeps, one of 2 at 100 and every other at maxniters = 120.
SHORT_KW = dict(optTol=0.0, maxniters=120)


def r11():
    """test_fslim_item_space.py's 3000 x 500 matrix: ties at nearly every cut, two empty columns."""
    rng = np.random.default_rng(11)
    R = sp.random(3000, 500, density=0.03, format="lil", random_state=rng, dtype=np.float32)
    R[:, 17] = 0
    R[:, 250] = 0
    R = sp.csr_matrix(R)
    R.eliminate_zeros()
    R.data[:] = 1.0
    R = sp.csr_matrix((R.data, R.indices, R.indptr), shape=(3000, 500))
    R.sort_indices()
    return R


MATRICES = {"r11": r11, "big": big, "big dyadic": lambda: big(True), "long": long_lists,
            "past": lambda: long_lists(4097), "short": short_columns}


@functools.lru_cache(maxsize=None)
def matrix(name):
    if isinstance(name, tuple):
        return small(*name[1:])
    return MATRICES[name]()


# ---- the oracle ----------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def work_order(name):
    return O.tile_work_order(matrix(name))


def tile_columns(name, t):
    return work_order(name)[32 * t:32 * t + 32]


@functools.lru_cache(maxsize=None)
def _walk(name, nnbrs, simtype, tiles, kw):
    args = dict(tileP=32, maxniters=200, seed=SEED, nthreads=8, nnbrs=nnbrs, simtype=simtype, return_stats=True,
                order=work_order(name), tiles=tiles)
    args.update(dict(kw))
    return O.learn_cd_tile(matrix(name), **args)


def walk(name, nnbrs, simtype, tiles=None, **kw):
    """learn_cd_tile's (W, column stats, error, objective) over the whole work list of matrix `name`, or over
    tiles=(first, count) of it; once per case."""
    return _walk(name, nnbrs, simtype, tiles, tuple(sorted(kw.items())))


def walk_tiles(name, nnbrs, simtype, tiles, **kw):
    """The walks of single tiles put together: (W, column stats, objective, the columns)."""
    parts = [walk(name, nnbrs, simtype, tiles=(t, 1), **kw) for t in tiles]
    cols = np.concatenate([tile_columns(name, t) for t in tiles])
    stats = parts[0][1].copy()
    for t, p in zip(tiles, parts):
        c = tile_columns(name, t)
        stats[c] = p[1][c]
    W = parts[0][0]
    for p in parts[1:]:
        W = W + p[0]
    return sp.csc_matrix(W), stats, sum(p[3] for p in parts), cols


# ---- the comparison ------------------------------------------------------------------------------------
def maxdiff(a, b):
    d = abs(sp.csc_matrix(a) - sp.csc_matrix(b))
    return float(d.max()) if d.nnz else 0.0


def pattern_diff(a, b):
    pa = sp.csc_matrix(a).copy()
    pb = sp.csc_matrix(b).copy()
    pa.data[:] = 1
    pb.data[:] = 1
    return int(abs(pa - pb).sum())


def same_bits(a, b):
    a, b = sp.csc_matrix(a), sp.csc_matrix(b)
    return a.nnz == b.nnz and maxdiff(a, b) == 0.0


class Figures(object):
    """One comparison with the oracle on the columns both sides solved."""

    def __init__(self, tag, W, cs, Wo, so, cols, objval=None, obj_o=None):
        cols = np.asarray(cols)
        self.tag = tag
        self.ncols = cols.size
        self.maxdiff = maxdiff(W[:, cols], Wo[:, cols])
        self.pattern = pattern_diff(W[:, cols], Wo[:, cols])
        self.nacols = bool(np.array_equal(cs.nacols[cols], so["nacols"][cols]))
        self.sweeps_equal = int((cs.sweeps[cols] == so["sweeps"][cols]).sum())
        self.conv = bool(np.array_equal(cs.conv[cols], so["conv"][cols]))
        self.D, self.D_o = int(cs.D[cols].sum()), int(so["D"][cols].sum())
        self.U, self.U_o = int(cs.U[cols].sum()), int(so["U"][cols].sum())
        self.objval, self.obj_o = objval, obj_o
        self.most_sweeps = int(so["sweeps"][cols].max()) if cols.size else 0

    def __str__(self):
        obj = "" if self.obj_o is None else ", objective %.6e / %.6e" % (self.objval, self.obj_o)
        return ("%s: %d columns, maxdiff %.3e, pattern_diff %d, nacols equal %s, sweeps equal %d / %d (oracle: up to %d), "
                "D %d / %d, U %d / %d%s" % (self.tag, self.ncols, self.maxdiff, self.pattern, self.nacols,
                                           self.sweeps_equal, self.ncols, self.most_sweeps, self.D, self.D_o, self.U,
                                           self.U_o, obj))

    def failures(self):
        """The bars of test_matches_the_oracle_tile_walk; the sweep share only where it means something (from
        200 columns; below, the family's pooled share is asserted)."""
        bad = []
        if not self.nacols:
            bad.append("nacols differ")
        if not self.maxdiff <= 2e-5:
            bad.append("maxdiff %.3e > 2e-5" % self.maxdiff)
        if not self.pattern <= 4:
            bad.append("pattern_diff %d > 4" % self.pattern)
        if not abs(self.D - self.D_o) <= 0.01 * self.D_o:
            bad.append("D %d against %d" % (self.D, self.D_o))
        if not abs(self.U - self.U_o) <= 0.01 * self.U_o:
            bad.append("U %d against %d" % (self.U, self.U_o))
        if self.obj_o is not None and not abs(self.objval - self.obj_o) <= 1e-4 * abs(self.obj_o):
            bad.append("objective %.6e against %.6e" % (self.objval, self.obj_o))
        if self.ncols >= 200 and not self.sweeps_equal >= 0.98 * self.ncols:
            bad.append("sweeps equal on %d of %d" % (self.sweeps_equal, self.ncols))
        return ["%s: %s" % (self.tag, b) for b in bad]


def pooled_sweeps(figs):
    eq, n = sum(f.sweeps_equal for f in figs), sum(f.ncols for f in figs)
    return eq, n
