"""-gpukernel of slim_learn / slim_mselect: the engine's kernel selection (slimgpu_kernel_et) from the
command line, which is how a CLI user reaches FSLIM in item space (kernel 6)."""
import os
import subprocess

import pytest
import scipy.sparse as sp

from slim_amd.engine import DeviceMatrix
from slim_amd.io import read_csr_text

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
BIN = os.path.join(ROOT, "slim_amd", "bin")


@pytest.mark.parametrize("prog", ["slim_learn", "slim_mselect"])
def test_help_lists_the_option(prog):
    r = subprocess.run([os.path.join(BIN, prog), "-help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "-gpukernel=i" in r.stdout


@pytest.mark.gpu
def test_slim_learn_gpukernel_6_writes_the_engine_model(tmp_path, ml100k):
    trn = os.path.join(GOLDEN, "ml100k-train.csr")
    out = str(tmp_path / "fslim.model")
    r = subprocess.run([os.path.join(BIN, "slim_learn"), "-l1r=1", "-l2r=1", "-nnbrs=20", "-simtype=jac",
                        "-gpukernel=6", trn, out], capture_output=True, text=True, timeout=200)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    m = DeviceMatrix.from_scipy(ml100k[0])
    W, st = m.learn(kernel=6, nnbrs=20, simtype=1, l1r=1.0, l2r=1.0, optTol=1e-7, niters=10000, seed=1)
    m.close()
    assert st["kernel"] == 6 and W.nnz > 0
    n = W.shape[0]
    F = read_csr_text(out, nrows=n)            # the row view of W, one line per row
    F = sp.csr_matrix((F.data, F.indices, F.indptr), shape=(n, n))
    d = abs(F - sp.csr_matrix(W))
    assert F.nnz == W.nnz and (d.max() if d.nnz else 0.0) == 0.0
