"""slim_mselect -cvfolds (include/slim_gpu_split.h): one data file, the pairs of the l12 file run once per fold through
the library's cross-validated driver."""
import os
import re
import subprocess

import pytest
import scipy.sparse as sp

from conftest import ROOT

MSELECT = os.path.join(ROOT, "slim_amd", "bin", "slim_mselect")
PAIRS = [(1.0, 1.0), (2.0, 5.0)]
SUMMARY = r"l1r: \S+ l2r: \S+ hr: (\S+) \(min (\S+) max (\S+)\) arhr: (\S+) \(min (\S+) max (\S+)\)"


def files(tmp_path, R):
    from slim_amd.io import write_csr_text
    names = [str(tmp_path / f) for f in ("data.csr", "l12")]
    write_csr_text(names[0], R)
    open(names[1], "w").write("".join("%g %g\n" % p for p in PAIRS))
    return names


def run(tmp_path, *argv):
    return subprocess.run([MSELECT, "-niters=200"] + list(argv), capture_output=True, text=True, cwd=str(tmp_path),
                          timeout=280)


@pytest.mark.gpu
def test_slim_mselect_cvfolds_prints_the_folds_and_the_means(automotive, tmp_path):
    names = files(tmp_path, sp.csr_matrix(automotive[0]))
    p = run(tmp_path, "-cvfolds=2", "-cvseed=3", *names)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "cross-validation: 2 folds, leave-out, nheld: 1, minkeep: 1, seed: 3" in p.stdout
    heads = re.findall(r"^fold (\d+) of 2: (\d+) held-out entries$", p.stdout, re.M)
    assert [h[0] for h in heads] == ["0", "1"] and heads[0][1] == heads[1][1] and int(heads[0][1]) > 0
    # per fold one line per pair, then one summary line per pair whose mean lies between its minimum and maximum
    assert len(re.findall(r"^l1r: \S+ l2r: \S+ nnz:", p.stdout, re.M)) == 2 * len(PAIRS)
    sums = re.findall(SUMMARY, p.stdout)
    assert len(sums) == len(PAIRS)
    for s in sums:
        hr, lo, hi, ar, alo, ahi = (float(x) for x in s)
        assert lo <= hr <= hi and alo <= ar <= ahi and hi > 0
    assert "best mean hr: %.4f at" % max(float(s[0]) for s in sums) in p.stdout
    assert not [f for f in os.listdir(str(tmp_path)) if f.endswith(".model")], "no model files in a cross-validated run"
    # the folds mode, and the same seed twice gives the same output but for the times
    q = run(tmp_path, "-cvfolds=2", "-cvmode=folds", "-cvminkeep=2", *names)
    assert q.returncode == 0 and "cross-validation: 2 folds, folds, minkeep: 2, seed: 1" in q.stdout
    again = run(tmp_path, "-cvfolds=2", "-cvseed=3", *names)
    strip = lambda text: re.sub(r"time: \S+", "", text)  # noqa: E731
    assert strip(again.stdout) == strip(p.stdout)


def test_three_files_with_cvfolds_is_a_usage_error(tmp_path):
    names = [str(tmp_path / f) for f in ("a", "b", "c")]
    for n in names:
        open(n, "w").write("0 1\n")
    p = run(tmp_path, "-cvfolds=2", *names)
    assert p.returncode != 0 and "two files, not three" in p.stderr and "l1r:" not in p.stdout
    for argv, word in ((("-cvheld=2",) + tuple(names), "needs -cvfolds"),
                       (("-cvfolds=2", "-cvmode=weekly") + tuple(names[:2]), "Invalid -cvmode"),
                       (("-cvfolds=1", "-cvmode=folds") + tuple(names[:2]), "Invalid -cvfolds"),
                       (("-cvfolds=65", "-cvheld=2") + tuple(names[:2]), "above 128"),
                       (("-cvfolds=2", "-evalhistbands=3") + tuple(names[:2]), "does not combine")):
        p = run(tmp_path, *argv)
        assert p.returncode != 0 and word in p.stderr, (argv, p.stderr)


def test_the_usage_names_the_cv_options():
    p = subprocess.run([MSELECT, "-help"], capture_output=True, text=True, timeout=60)
    assert p.returncode == 0 and "-cvfolds=F" in p.stdout and "data-file l12-file" in p.stdout
