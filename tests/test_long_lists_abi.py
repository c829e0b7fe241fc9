"""The entry points of the long top-N lists (include/slim_gpu_lists.h) are declared, exported and bound, and
refuse bad arguments before any device call: SLIM_ERROR_INPUT, a SLIMGPU_LastError text, untouched outputs.
No GPU needed."""
import ctypes as C
import os
import re

import numpy as np

from conftest import ROOT
from slim_amd import _lib, constants
from slim_amd.constants import SLIM_ERROR_INPUT, SLIM_OK

NEW = {
    "SLIMGPU_PredictLists": ["int32_t nrcmds", "slim_t *model", "slim_t *trn", "int32_t *output", "float *scores",
                             "int32_t *counts"],
    "SLIMGPU_ModelPredictLists": ["int32_t nrcmds", "const slimgpu_model_t *model", "slim_t *trn", "int32_t *output",
                                  "float *scores", "int32_t *counts"],
    "SLIMGPU_MatrixPredictLists": ["int32_t nrcmds", "const slimgpu_model_t *model", "slimgpu_matrix_t *mat",
                                   "int32_t nusers", "const int32_t *users", "int32_t *output", "float *scores",
                                   "int32_t *counts"],
    "SLIMGPU_LastListStats": ["slimgpu_list_stats_t *out"],
}
P = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731


def _header(name="slim_gpu_lists.h"):
    text = open(os.path.join(ROOT, "include", name)).read()
    return re.sub(r"/\*.*?\*/", "", text, flags=re.S)


def test_the_names_are_declared_exported_and_bound():
    text = re.sub(r"\s+", " ", _header())
    raw = C.CDLL(_lib.LIB_PATH)
    for name, args in NEW.items():
        m = re.search(r"int32_t %s ?\(([^)]*)\)" % name, text)
        assert m, "%s is not declared in slim_gpu_lists.h" % name
        assert [a.strip() for a in m.group(1).split(",")] == args, name
        assert hasattr(raw, name), "libslim.so does not export %s" % name
        res, a = _lib._LIST_SIGNATURES[name]
        assert res is C.c_int32 and len(a) == len(args), name
    assert set(NEW) == set(_lib.LIST_SYMBOLS)
    assert set(re.findall(r"\b(SLIMGPU_\w+)\s*\(", _header())) == set(NEW)
    assert re.search(r"#define SLIMGPU_MAX_LIST 4096\b", _header())
    assert _lib.MAX_LIST == 4096 and constants.SLIMGPU_MAX_LIST == 4096
    assert '#include "slim_gpu_lists.h"' in open(os.path.join(ROOT, "include", "slim_gpu.h")).read()
    # a table of its own: the tables before it keep their names and counts
    for other in (_lib.EXPORTED_SYMBOLS, _lib.EVAL_SYMBOLS, _lib.EVAL_AT_SYMBOLS, _lib.PLANES_SYMBOLS,
                  _lib.RANK_SYMBOLS):
        assert not set(NEW) & set(other)
    assert len(_lib.EXPORTED_SYMBOLS) == 46 and len(_lib.RANK_SYMBOLS) == 6
    # slimgpu_list_stats_t as the header lays it out: two int32, five int64
    assert C.sizeof(_lib.ListStats) == 48
    assert [f for f, _ in _lib.ListStats._fields_] == re.findall(
        r"\b(\w+)(?=[,;])", re.search(r"typedef struct slimgpu_list_stats_t \{(.*?)\}", _header(), re.S).group(1))
    # the eval stats keep their layout
    assert C.sizeof(_lib.EvalStats) == 56


def _wrap(lib, M):
    h = C.c_void_p()
    assert lib.Py_csr_wrapper(M.shape[0], np.ascontiguousarray(M.indptr, np.intp),
                              np.ascontiguousarray(M.indices, np.int32), P(np.ascontiguousarray(M.data, np.float32)),
                              C.byref(h)) == SLIM_OK
    return h


def test_bad_arguments_are_refused_without_a_device():
    import scipy.sparse as sp
    lib = _lib.load()
    W = sp.random(40, 40, density=0.2, format="csr", random_state=np.random.default_rng(1), dtype=np.float32)
    H = sp.random(6, 40, density=0.2, format="csr", random_state=np.random.default_rng(2), dtype=np.float32)
    hw, hr = _wrap(lib, W), _wrap(lib, H)
    ids = np.full(6 * 4097, -1, np.int32)
    sc = np.zeros(6 * 4097, np.float32)
    cnt = np.full(6, -7, np.int32)
    users = np.array([0, 1], np.int32)

    def untouched():
        return bool((ids == -1).all() and (sc == 0).all() and (cnt == -7).all())

    for n in (0, 4097, -1):                          # the bounds, with good handles
        assert lib.SLIMGPU_PredictLists(n, hw, hr, P(ids), P(sc), P(cnt)) == SLIM_ERROR_INPUT
        assert "SLIMGPU_PredictLists" in _lib.last_error() and "4096" in _lib.last_error() and untouched()
    for n in (0, 10, 200, 4096, 4097):               # null handles, at any length
        assert lib.SLIMGPU_PredictLists(n, None, hr, P(ids), P(sc), P(cnt)) == SLIM_ERROR_INPUT
        assert _lib.last_error() and untouched()
        assert lib.SLIMGPU_PredictLists(n, hw, None, P(ids), P(sc), None) == SLIM_ERROR_INPUT
        assert _lib.last_error() and untouched()
        assert lib.SLIMGPU_ModelPredictLists(n, None, hr, P(ids), P(sc), P(cnt)) == SLIM_ERROR_INPUT
        assert "SLIMGPU_ModelPredictLists" in _lib.last_error() and untouched()
        assert lib.SLIMGPU_MatrixPredictLists(n, None, None, 0, None, P(ids), P(sc), P(cnt)) == SLIM_ERROR_INPUT
        assert "SLIMGPU_MatrixPredictLists" in _lib.last_error() and untouched()
        assert lib.SLIMGPU_MatrixPredictLists(n, None, None, 2, P(users), P(ids), P(sc), None) == SLIM_ERROR_INPUT
        assert _lib.last_error() and untouched()
    assert lib.SLIMGPU_PredictLists(200, hw, hr, None, P(sc), P(cnt)) == SLIM_ERROR_INPUT and untouched()
    assert lib.SLIMGPU_PredictLists(200, hw, hr, P(ids), None, P(cnt)) == SLIM_ERROR_INPUT and untouched()
    assert lib.SLIMGPU_LastListStats(None) == SLIM_ERROR_INPUT
    st = _lib.ListStats()
    assert lib.SLIMGPU_LastListStats(C.byref(st)) == SLIM_OK
    # the old entry points keep their bound and their text
    assert lib.SLIMGPU_Predict(129, hw, hr, ids, sc) == SLIM_ERROR_INPUT
    assert "1 <= nrcmds <= 128" in _lib.last_error() and untouched()
    lib.Py_csr_free(hw)
    lib.Py_csr_free(hr)
