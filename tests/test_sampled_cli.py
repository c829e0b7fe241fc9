"""slim_mselect -evalnegs / -evalseed (include/slim_gpu_sample.h): the command-line grid on sampled negatives prints
the figures that the existing candidate evaluation gives on the numpy restatement's rows (tests/sampled_cases.py)."""
import os
import re
import subprocess

import numpy as np
import pytest
import scipy.sparse as sp

from conftest import ROOT
from sampled_cases import GRID_L1, GRID_L2, PAIR, check_grid_lines, grid_by_hand

MSELECT = os.path.join(ROOT, "slim_amd", "bin", "slim_mselect")


def files(tmp_path, R, T):
    from slim_amd.io import write_csr_text
    names = [str(tmp_path / f) for f in ("trn.csr", "tst.csr", "l12")]
    write_csr_text(names[0], R)
    write_csr_text(names[1], sp.csr_matrix((T.data, T.indices, T.indptr), shape=T.shape))
    open(names[2], "w").write("".join("%g %g\n" % (a, b) for a in GRID_L1 for b in GRID_L2))
    return names


def run(tmp_path, names, *options):
    return subprocess.run([MSELECT, "-nomodels", "-niters=200"] + list(options) + names, capture_output=True, text=True,
                          cwd=str(tmp_path), timeout=280)


@pytest.mark.gpu
def test_slim_mselect_on_sampled_negatives(automotive, monkeypatch, tmp_path):
    R, T = sp.csr_matrix(automotive[0]), sp.csr_matrix(automotive[1])
    monkeypatch.setenv("SLIM_GPU_NO_CARRY", "1")
    monkeypatch.setenv("SLIM_GPU_RESIDENT", "1")
    monkeypatch.setenv("SLIM_GPU_EVAL_RESIDENT", "1")
    names = files(tmp_path, R, T)
    got, entries = grid_by_hand(R, T, 99, seed=1)
    p = run(tmp_path, names, "-evalnegs=99")
    assert p.returncode == 0, p.stdout + p.stderr
    assert "  sampled negatives: nnegs 99, seed 1, %d candidate entries\n" % entries in p.stdout
    check_grid_lines(re.findall(PAIR, p.stdout), got)
    best = max(g["hr"] for _, _, g, _ in got)
    assert "best hr: %.4f at" % best in p.stdout
    # a seed, and every third user
    S = np.arange(0, R.shape[0], 3)
    got3, entries3 = grid_by_hand(R, T, 99, seed=5, users=S)
    p = run(tmp_path, names, "-evalnegs=99", "-evalseed=5", "-evalstride=3")
    assert p.returncode == 0, p.stdout + p.stderr
    assert "  sampled negatives: nnegs 99, seed 5, %d candidate entries\n" % entries3 in p.stdout
    check_grid_lines(re.findall(PAIR, p.stdout), got3)
    # refused before any solve line
    for options, word in ((("-evalnegs=99", "-nrcmds=200"), "128"), (("-evalnegs=99", "-blockfile=" + names[2]), "filter"),
                          (("-evalnegs=-1",), "Invalid"), (("-evalnegs=4096",), "4096")):
        p = run(tmp_path, names, *options)
        assert p.returncode != 0 and word in p.stdout + p.stderr and "l1r:" not in p.stdout, (options, p.stdout, p.stderr)
    monkeypatch.setenv("SLIM_GPU_EVAL_RESIDENT", "0")
    p = run(tmp_path, names, "-evalnegs=99")
    assert p.returncode != 0 and "SLIM_GPU_EVAL_RESIDENT=0" in p.stdout + p.stderr and "l1r:" not in p.stdout


def test_the_usage_names_the_options():
    p = subprocess.run([MSELECT, "-help"], capture_output=True, text=True, timeout=60)
    assert p.returncode == 0 and "-evalnegs=i" in p.stdout and "-evalseed=i" in p.stdout
