"""slim_mselect -evalgroupfile / -evalhistbands / -evalselectgroup (include/slim_gpu_groups.h): what the program
refuses on its own, before the library sees the grid.  No device needed."""
import os
import subprocess

import numpy as np
import pytest
import scipy.sparse as sp

from conftest import ROOT

MSELECT = os.path.join(ROOT, "slim_amd", "bin", "slim_mselect")


@pytest.fixture()
def names(tmp_path):
    from slim_amd.io import write_csr_text
    rng = np.random.default_rng(7)
    R = sp.csr_matrix((rng.random((12, 9)) < 0.4).astype(np.float32))
    T = sp.csr_matrix((np.ones(12, np.float32), (np.arange(12), np.arange(12) % 9)), shape=(12, 9))
    out = [str(tmp_path / f) for f in ("trn.csr", "tst.csr", "l12")]
    write_csr_text(out[0], R)
    write_csr_text(out[1], T)
    open(out[2], "w").write("1 0.5\n")
    return out


def group_file(tmp_path, groups):
    path = str(tmp_path / "groups")
    open(path, "w").write("".join("%d\n" % g for g in groups))
    return path


def dies(tmp_path, names, *options):
    p = subprocess.run([MSELECT, "-nomodels", "-niters=20"] + list(options) + names, capture_output=True, text=True,
                       cwd=str(tmp_path), timeout=60)
    print(p.stderr)
    assert p.returncode == 1 and "l1r:" not in p.stdout and "Estimating" not in p.stdout
    return p.stderr


def test_the_two_sources_exclude_each_other(tmp_path, names):
    g = group_file(tmp_path, [0, 1] * 6)
    err = dies(tmp_path, names, "-evalgroupfile=" + g, "-evalhistbands=2,5")
    assert err == "The -evalgroupfile and -evalhistbands options cannot be used together.\n"


def test_a_group_file_with_the_wrong_row_count(tmp_path, names):
    for groups in ([0, 1] * 5 + [0], [0, 1] * 6 + [1]):
        err = dies(tmp_path, names, "-evalgroupfile=" + group_file(tmp_path, groups))
        assert err == "The -evalgroupfile holds %d groups, the training matrix has 12 user rows.\n" % len(groups)
    assert "does not exist" in dies(tmp_path, names, "-evalgroupfile=" + str(tmp_path / "nowhere"))
    assert "bad group -2" in dies(tmp_path, names, "-evalgroupfile=" + group_file(tmp_path, [0] * 11 + [-2]))
    assert "bad group 1024" in dies(tmp_path, names, "-evalgroupfile=" + group_file(tmp_path, [0] * 11 + [1024]))
    assert "no user into a group" in dies(tmp_path, names, "-evalgroupfile=" + group_file(tmp_path, [-1] * 12))
    open(str(tmp_path / "words"), "w").write("0\n1\nx\n")
    assert "bad group in" in dies(tmp_path, names, "-evalgroupfile=" + str(tmp_path / "words"))


@pytest.mark.parametrize("bands", ["", "5,", ",5", "5,5", "20,5", "0,5", "-3", "2;5", "2,x", "2.5", "2,5 "])
def test_a_malformed_band_list(tmp_path, names, bands):
    assert dies(tmp_path, names, "-evalhistbands=" + bands) == "Invalid -evalhistbands of %s.\n" % bands


def test_the_selected_group(tmp_path, names):
    g = group_file(tmp_path, [0, 1, -1] * 4)
    assert "needs -evalgroupfile or -evalhistbands" in dies(tmp_path, names, "-evalselectgroup=0")
    for bad in ("2", "-1", "7"):
        err = dies(tmp_path, names, "-evalgroupfile=" + g, "-evalselectgroup=" + bad)
        assert err == "Invalid -evalselectgroup of %s: the groups are 0 to 1.\n" % bad
    assert "the groups are 0 to 2" in dies(tmp_path, names, "-evalhistbands=2,5", "-evalselectgroup=3")


def test_the_usage_names_the_options():
    p = subprocess.run([MSELECT, "-help"], capture_output=True, text=True, timeout=60)
    assert p.returncode == 0
    for word in ("-evalgroupfile=file", "-evalhistbands=b0,b1,..", "-evalselectgroup=g"):
        assert word in p.stdout
