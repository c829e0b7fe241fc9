"""Evaluation, ranks and the grid under a candidate filter, without a device: the four entry points of
include/slim_gpu_filter_eval.h are declared, exported and bound; SLIM.mselect's filter arguments; the filter
options of slim_mselect (those of slim_predict, from the one copy in cli_common.hpp)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
import scipy.sparse as sp

from conftest import GOLDEN, ROOT
from slim_amd import _lib

BIN = os.path.join(ROOT, "slim_amd", "bin")
NAMES = {"SLIMGPU_ModelEvaluateAtFiltered", "SLIMGPU_ModelRanksFiltered", "SLIMGPU_ModelEvaluateRankedFiltered",
         "Py_SLIM_MselectFiltered"}


def test_the_four_names_are_declared_exported_and_bound():
    text = open(os.path.join(ROOT, "include", "slim_gpu_filter_eval.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b((?:Py|SLIMGPU)_\w+)\s*\(", text))
    assert declared == NAMES == set(_lib.FILTERED_EVAL_SYMBOLS)
    raw = C.CDLL(_lib.LIB_PATH)
    lib = _lib.load()
    for name in declared:
        assert hasattr(raw, name), "libslim.so does not export %s" % name
        assert getattr(lib, name).argtypes is not None and getattr(lib, name).restype is C.c_int32
    assert '#include "slim_gpu_filter_eval.h"' in open(os.path.join(ROOT, "include", "slim_gpu_filter.h")).read()
    for other in (_lib.EXPORTED_SYMBOLS, _lib.EVAL_SYMBOLS, _lib.EVAL_AT_SYMBOLS, _lib.PLANES_SYMBOLS,
                  _lib.RANK_SYMBOLS, _lib.LIST_SYMBOLS, _lib.FILTER_SYMBOLS):
        assert not declared & set(other)
    # the filter goes behind the model; the grid takes it last, behind Py_SLIM_Mselect's own arguments
    assert len(lib.Py_SLIM_MselectFiltered.argtypes) == len(lib.Py_SLIM_Mselect.argtypes) + 1
    assert lib.Py_SLIM_MselectFiltered.argtypes[:-1] == lib.Py_SLIM_Mselect.argtypes
    for plain, filtered in (("SLIMGPU_ModelEvaluateAt", "SLIMGPU_ModelEvaluateAtFiltered"),
                            ("SLIMGPU_ModelRanks", "SLIMGPU_ModelRanksFiltered"),
                            ("SLIMGPU_ModelEvaluateRanked", "SLIMGPU_ModelEvaluateRankedFiltered")):
        a, b = getattr(lib, plain).argtypes, getattr(lib, filtered).argtypes
        assert list(b[:2]) + list(b[3:]) == list(a) and b[2] is C.c_void_p


def test_the_old_header_no_longer_says_not_built():
    text = open(os.path.join(ROOT, "include", "slim_gpu_filter.h")).read()
    left = text[text.index("Not built:"):text.index("*/")]
    assert "history items" in left and "skipping" in left and "evaluation" not in left.lower()


def test_mselect_takes_at_most_one_item_set():
    from slim_amd import SLIM, SLIMatrix
    R = sp.csr_matrix(np.eye(4, dtype=np.float32))
    trn = SLIMatrix(R)
    tst = SLIMatrix(R, trn)
    with pytest.raises(TypeError, match="at most one of allowed_items and blocked_items"):
        SLIM().mselect({"algo": "cd"}, trn, tst, [1.0], [1.0], nrcmds=10, allowed_items=[0], blocked_items=[1])


def _mselect(*args):
    return subprocess.run([os.path.join(BIN, "slim_mselect")] + list(args), capture_output=True, text=True, timeout=120)


def test_slim_mselect_names_and_checks_the_filter_options(tmp_path):
    out = _mselect("-help").stdout
    for opt in ("-allowfile", "-blockfile", "-exclfile"):
        assert opt in out
    # the usage text of the three options is slim_predict's
    usage = subprocess.run([os.path.join(BIN, "slim_predict"), "-help"], capture_output=True, text=True,
                           timeout=120).stdout
    lines = [ln for ln in usage.splitlines() if "allowfile" in ln or "exclfile" in ln]
    assert len(lines) == 2 and all(ln in out for ln in lines)
    a, b = str(tmp_path / "a"), str(tmp_path / "b")
    for f in (a, b):
        open(f, "w").write("1\n2\n")
    files = [os.path.join(GOLDEN, "ml100k-train.csr"), os.path.join(GOLDEN, "ml100k-test.csr"),
             os.path.join(GOLDEN, "l12file")]
    both = _mselect("-allowfile=" + a, "-blockfile=" + b, *files)
    pred = subprocess.run([os.path.join(BIN, "slim_predict"), "-allowfile=" + a, "-blockfile=" + b] + files[:2],
                          capture_output=True, text=True, timeout=120)
    assert both.returncode != 0 and pred.returncode != 0
    assert both.stderr == pred.stderr == "The -allowfile and -blockfile options cannot be used together.\n"
    missing = _mselect("-exclfile=" + str(tmp_path / "nothing"), *files)
    assert missing.returncode != 0 and "nothing does not exist" in missing.stderr
