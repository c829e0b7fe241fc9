#!/usr/bin/env python3
"""FSLIM on C4 (1M users x 100K items, binary; slim_amd.synth): the tile kernel's FSLIM form against
FSLIM in item space (KERNEL_GRAM_FSLIM, cd_fslim_gram.hpp).  cos, l1 = l2 = 1.  One step per process,
one handle per process:

  tile NNBRS  : (i)   the benchmark's 8192-column step on KERNEL_TILE; the model is kept for `item`
  item NNBRS  : (ii)  the same step on kernel 6 from a fresh handle (G built inside the time), compared
                      with the model `tile` left; (iii) the same call again, G there
  all NNBRS   : (iv)  all 100 000 columns on kernel 6 (fresh handle: G build reported apart)
  tileall NNBRS :     all columns on the tile kernel (only worth running if (i) projects under ten minutes)

Run the steps each under its own time limit, chained so that a failed step ends the chain, e.g.
  timeout -k 10 600 python scripts/fslim_item_space.py tile 10 && \
  timeout -k 10 300 python scripts/fslim_item_space.py item 10 && \
  timeout -k 10 300 python scripts/fslim_item_space.py all 10
OUT (environment, default: the temporary directory) is where `tile` leaves its model."""
import os
import sys
import tempfile
import time

import numpy as np
import scipy.sparse as sp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OUT = os.environ.get("OUT", tempfile.gettempdir())
STEP_COLS = 8192


def stage(workload="c4", seed=1):
    import torch
    from slim_amd import synth
    from slim_amd.engine import DeviceMatrix
    dev = torch.device("cuda", 0)
    nrows, ncols, target = synth.CONFIGS[workload]
    t0 = time.perf_counter()
    rowptr, rowind, rowval = synth.generate_csr(nrows, ncols, target, seed=seed, device=dev)
    torch.cuda.synchronize()
    m = DeviceMatrix.from_device_ptrs(nrows, ncols, rowptr.data_ptr(), rowind.data_ptr(), 0,
                                      keepalive=(rowptr, rowind, rowval), device=0)
    print("staged %s: %d x %d, nnz %d, %.1f s" % (workload, m.nrows, m.ncols, m.nnz, time.perf_counter() - t0),
          flush=True)
    return m


def maxdiff(a, b):
    d = abs(sp.csc_matrix(a) - sp.csc_matrix(b))
    return float(d.max()) if d.nnz else 0.0


def run(mat, tag, **kw):
    t0 = time.perf_counter()
    W, st = mat.learn(**kw)
    dt = time.perf_counter() - t0
    cs = mat.column_stats()
    print("%s: kernel %d, wall %.3f s, kernel_ms %.1f, gram_build_ms %.1f, nnzW %d, sweeps %d, nacols max %d"
          % (tag, st["kernel"], dt, st["kernel_ms"], st["gram_build_ms"], st["nnzW"], st["sweeps"],
             int(cs.nacols.max())), flush=True)
    return W, st, cs


def main():
    from slim_amd.engine import KERNEL_GRAM_FSLIM, KERNEL_TILE
    what, nnbrs = sys.argv[1], int(sys.argv[2])
    kw = dict(l1r=1.0, l2r=1.0, optTol=1e-7, niters=10000, seed=1, nnbrs=nnbrs, simtype=0)
    kept = os.path.join(OUT, "fslim_tile_step_nnbrs%d.npz" % nnbrs)
    mat = stage()
    if what == "tile":
        W, st, _ = run(mat, "(i) nnbrs %d, %d columns, tile kernel" % (nnbrs, STEP_COLS), kernel=KERNEL_TILE,
                       col_begin=0, col_end=STEP_COLS, **kw)
        print("    all %d columns at this rate: %.0f s" % (mat.ncols, st["kernel_ms"] * 1e-3 * mat.ncols / STEP_COLS))
        os.makedirs(OUT, exist_ok=True)
        sp.save_npz(kept, sp.csc_matrix(W))
    elif what == "item":
        W, st, cs = run(mat, "(ii) nnbrs %d, %d columns, kernel 6, fresh handle" % (nnbrs, STEP_COLS),
                        kernel=KERNEL_GRAM_FSLIM, col_begin=0, col_end=STEP_COLS, **kw)
        if os.path.exists(kept):
            Wt = sp.load_npz(kept)
            print("    (ii) against (i): max|dW| %.3e, nnz %d / %d" % (maxdiff(W, Wt), W.nnz, Wt.nnz))
        else:
            print("    (ii) against (i): no model of step (i) found")
        W2, _, _ = run(mat, "(iii) the same, G there", kernel=KERNEL_GRAM_FSLIM, col_begin=0, col_end=STEP_COLS, **kw)
        print("    same model twice: %s" % (maxdiff(W, W2) == 0.0))
    elif what == "all":
        run(mat, "(iv) nnbrs %d, all %d columns, kernel 6, fresh handle" % (nnbrs, mat.ncols),
            kernel=KERNEL_GRAM_FSLIM, **kw)
        run(mat, "(iv) again, G there", kernel=KERNEL_GRAM_FSLIM, **kw)
    elif what == "tileall":
        run(mat, "nnbrs %d, all %d columns, tile kernel" % (nnbrs, mat.ncols), kernel=KERNEL_TILE, **kw)
    else:
        raise SystemExit(__doc__)
    mat.close()


if __name__ == "__main__":
    main()
