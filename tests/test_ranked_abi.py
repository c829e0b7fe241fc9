"""The entry points of the ranked evaluation (include/slim_gpu_rank.h: the rank of every held-out item among
a user's candidates, evaluation of resident models at any list length) are declared, exported and bound, refuse
null handles without a device, and slim_amd/ranking.py computes the metrics it documents.  No GPU needed."""
import ctypes as C
import os
import re

import numpy as np

from conftest import ROOT
from slim_amd import _lib, ranking
from slim_amd.constants import SLIM_ERROR_INPUT

NEW = {
    "SLIMGPU_EvalSetCreateRanked": ("slimgpu_evalset_t *", ["slimgpu_matrix_t *mat", "slim_t *tsthandle",
                                                            "const int32_t *fmarker", "int32_t fm_ncols",
                                                            "int32_t nusers", "const int32_t *users",
                                                            "int32_t *r_status"]),
    "SLIMGPU_EvalSetEntries": ("int64_t", ["const slimgpu_evalset_t *es"]),
    "SLIMGPU_ModelRanks": ("int32_t", ["slimgpu_evalset_t *es", "const slimgpu_model_t *model", "int32_t *ranks",
                                       "float *scores"]),
    "SLIMGPU_ModelEvaluateRanked": ("int32_t", ["slimgpu_evalset_t *es", "const slimgpu_model_t *model",
                                                "int32_t ncutoffs", "const int32_t *cutoffs", "double *metrics",
                                                "int32_t *nvalid"]),
    "SLIMGPU_ModelFromHost": ("slimgpu_model_t *", ["slimgpu_matrix_t *mat", "slim_t *model", "int32_t *r_status"]),
    "SLIMGPU_LastRankPrepassMs": ("double", ["void"]),
}


def _header(name="slim_gpu_rank.h"):
    text = open(os.path.join(ROOT, "include", name)).read()
    return re.sub(r"/\*.*?\*/", "", text, flags=re.S)


def test_the_six_names_are_declared_exported_and_bound():
    text = re.sub(r"\s+", " ", _header())
    raw = C.CDLL(_lib.LIB_PATH)
    for name, (res, args) in NEW.items():
        m = re.search(r"([\w ]+\*?) ?\b%s ?\(([^)]*)\)" % name, text)
        assert m, "%s is not declared in slim_gpu_rank.h" % name
        assert m.group(1).strip().replace(" *", "*") == res.strip().replace(" *", "*"), (name, m.group(1))
        assert [a.strip() for a in m.group(2).split(",")] == args, name
        assert hasattr(raw, name), "libslim.so does not export %s" % name
        r, a = _lib._RANK_SIGNATURES[name]
        assert len(a) == (0 if args == ["void"] else len(args)), name
    assert set(NEW) == set(_lib.RANK_SYMBOLS) and len(_lib.RANK_SYMBOLS) == 6
    declared = set(re.findall(r"\b(SLIMGPU_\w+)\s*\(", _header()))
    assert declared == set(NEW)
    assert re.search(r"#define SLIMGPU_MAX_RANK_CUTOFFS 32\b", _header()) and _lib.MAX_RANK_CUTOFFS == 32
    assert '#include "slim_gpu_rank.h"' in open(os.path.join(ROOT, "include", "slim_gpu.h")).read()
    # a table of its own: the tables before it keep their names, test_abi's count of 46 is untouched
    for other in (_lib.EXPORTED_SYMBOLS, _lib.EVAL_SYMBOLS, _lib.EVAL_AT_SYMBOLS, _lib.PLANES_SYMBOLS):
        assert not set(NEW) & set(other)
    assert len(_lib.EXPORTED_SYMBOLS) == 46 and len(_lib.EVAL_SYMBOLS) == 5 and len(_lib.EVAL_AT_SYMBOLS) == 2
    main = _header("slim.h") + _header("slim_gpu.h")
    assert not any(re.search(r"\b%s\s*\(" % n, main) for n in NEW)
    lib = _lib.load()
    assert lib.SLIMGPU_ModelRanks.restype is C.c_int32
    assert lib.SLIMGPU_EvalSetEntries.restype is C.c_int64
    assert lib.SLIMGPU_ModelFromHost.restype is C.c_void_p
    assert lib.SLIMGPU_LastRankPrepassMs.restype is C.c_double


def test_null_handles_are_refused_without_a_device():
    lib = _lib.load()
    st = C.c_int32(0)
    fm = np.zeros(4, np.int32)
    assert not lib.SLIMGPU_EvalSetCreateRanked(None, None, fm, 4, 0, None, C.byref(st))
    assert st.value == SLIM_ERROR_INPUT and _lib.last_error()
    assert lib.SLIMGPU_EvalSetEntries(None) == -1
    rk = np.zeros(4, np.int32)
    assert lib.SLIMGPU_ModelRanks(None, None, rk.ctypes.data_as(C.c_void_p), None) == SLIM_ERROR_INPUT
    assert _lib.last_error()
    cut = np.array([5, 200], np.int32)
    met, nv = np.zeros(8), np.zeros(6, np.int32)
    assert lib.SLIMGPU_ModelEvaluateRanked(None, None, 2, cut.ctypes.data_as(C.c_void_p), met, nv) == SLIM_ERROR_INPUT
    assert _lib.last_error()
    # the cutoffs are checked before anything else: none, too many, not ascending, below 1
    many = np.arange(1, 34, dtype=np.int32)
    for n, c in ((0, cut), (33, many), (2, np.array([7, 7], np.int32)), (2, np.array([0, 3], np.int32))):
        assert lib.SLIMGPU_ModelEvaluateRanked(None, None, n, c.ctypes.data_as(C.c_void_p), np.zeros(4 * 33),
                                               np.zeros(3 * 33, np.int32)) == SLIM_ERROR_INPUT
    assert lib.SLIMGPU_ModelEvaluateRanked(None, None, 1, None, met, nv) == SLIM_ERROR_INPUT
    st.value = 0
    assert not lib.SLIMGPU_ModelFromHost(None, None, C.byref(st))
    assert st.value == SLIM_ERROR_INPUT and _lib.last_error()
    assert lib.SLIMGPU_LastRankPrepassMs() >= 0.0


def test_ranking_metrics_on_five_users():
    # user 0: ranks 1 and 4; user 1: nothing ranked; user 2: no test items; user 3: one item listed twice
    # (rank 2 twice: one hit) and one at rank 300; user 4: a single item at rank 3
    ranks = np.array([1, 4, 0, 0, 2, 2, 300, 3], np.int32)
    indptr = np.array([0, 2, 4, 4, 7, 8])
    l2 = np.log2
    hr3 = ranking.hit_rate(ranks, indptr, 3)
    assert hr3.dtype == np.float64 and hr3.tolist() == [1 / 2, 0.0, 0.0, 1 / 3, 1.0]
    assert ranking.hit_rate(ranks, indptr, 300).tolist() == [1.0, 0.0, 0.0, 2 / 3, 1.0]
    assert ranking.hit_rate(ranks, indptr, 1).tolist() == [1 / 2, 0.0, 0.0, 0.0, 0.0]
    nd = ranking.ndcg(ranks, indptr, 3)
    ideal2 = 1 / l2(2) + 1 / l2(3)
    ideal3 = ideal2 + 1 / l2(4)
    want = [(1 / l2(2)) / ideal2, 0.0, 0.0, (1 / l2(3)) / ideal3, (1 / l2(4)) / (1 / l2(2))]
    assert nd.dtype == np.float64 and np.allclose(nd, want, rtol=1e-15, atol=0)
    nd300 = ranking.ndcg(ranks, indptr, 300)
    want300 = [(1 / l2(2) + 1 / l2(5)) / ideal2, 0.0, 0.0, (1 / l2(3) + 1 / l2(301)) / ideal3, (1 / l2(4)) / 1.0]
    assert np.allclose(nd300, want300, rtol=1e-15, atol=0)
    assert ranking.mrr(ranks, indptr).tolist() == [1.0, 0.0, 0.0, 1 / 2, 1 / 3]
