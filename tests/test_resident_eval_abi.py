"""The entry points of the evaluation in HBM (include/slim_gpu_eval.h: SLIMGPU_EvalSetCreate & co) are
exported by libslim.so with the declared prototypes.  No GPU needed."""
import ctypes as C
import os
import re

import numpy as np

from conftest import ROOT
from slim_amd import _lib
from slim_amd.constants import SLIM_ERROR_INPUT, SLIM_OK

NEW = {
    "SLIMGPU_EvalSetCreate": ("slimgpu_evalset_t *", ["slimgpu_matrix_t *mat", "slim_t *tsthandle",
                                                      "const int32_t *fmarker", "int32_t fm_ncols",
                                                      "int32_t nrcmds", "int32_t *r_status"]),
    "SLIMGPU_EvalSetFree": ("void", ["slimgpu_evalset_t **es"]),
    "SLIMGPU_ModelEvaluate": ("int32_t", ["slimgpu_evalset_t *es", "const slimgpu_model_t *model",
                                          "double *metrics", "int32_t *nvalid"]),
    "SLIMGPU_MatrixPredict": ("int32_t", ["int32_t nrcmds", "const slimgpu_model_t *model",
                                          "slimgpu_matrix_t *mat", "int32_t *output", "float *scores"]),
    "SLIMGPU_LastEvalStats": ("int32_t", ["slimgpu_eval_stats_t *out"]),
}


def _header():
    text = open(os.path.join(ROOT, "include", "slim_gpu_eval.h")).read()
    return re.sub(r"/\*.*?\*/", "", text, flags=re.S)


def test_new_symbols_are_declared_exported_and_bound():
    text = re.sub(r"\s+", " ", _header())
    raw = C.CDLL(_lib.LIB_PATH)
    for name, (res, args) in NEW.items():
        m = re.search(r"([\w ]+\*?) ?\b%s ?\(([^)]*)\)" % name, text)
        assert m, "%s is not declared in slim_gpu_eval.h" % name
        assert m.group(1).strip().replace(" *", "*") == res.strip().replace(" *", "*"), (name, m.group(1))
        got = [a.strip() for a in m.group(2).split(",")]
        assert got == args, (name, got)
        assert hasattr(raw, name), "libslim.so does not export %s" % name
        assert name in _lib.EVAL_SYMBOLS
        r, a = _lib._EVAL_SIGNATURES[name]
        assert len(a) == len(args)
    assert set(NEW) == set(_lib.EVAL_SYMBOLS)
    # slim_gpu.h pulls the new header in, so one include still gives a C caller everything
    assert '#include "slim_gpu_eval.h"' in open(os.path.join(ROOT, "include", "slim_gpu.h")).read()
    assert _lib._EVAL_SIGNATURES["SLIMGPU_EvalSetCreate"][0] is C.c_void_p
    assert _lib._EVAL_SIGNATURES["SLIMGPU_EvalSetFree"][0] is None
    assert _lib._EVAL_SIGNATURES["SLIMGPU_ModelEvaluate"][0] is C.c_int32


def test_eval_stats_layout():
    """slimgpu_eval_stats_t: two int32, two int64, two doubles, an int64 and a double, in that order."""
    text = _header()
    body = re.search(r"typedef struct slimgpu_eval_stats_t \{(.*?)\} slimgpu_eval_stats_t;", text, flags=re.S).group(1)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            ctype, names = decl.split(None, 1)
            fields += [(n.strip(), ctype) for n in names.split(",")]
    ctypes_of = {"int32_t": C.c_int32, "int64_t": C.c_int64, "double": C.c_double}
    assert [(n, ctypes_of[t]) for n, t in fields] == list(_lib.EvalStats._fields_)
    assert C.sizeof(_lib.EvalStats) == 56 and _lib.EvalStats.w_bytes.offset == 48


def test_null_arguments_are_refused_without_a_device():
    lib = _lib.load()
    st = C.c_int32(0)
    fm = np.zeros(4, np.int32)
    assert not lib.SLIMGPU_EvalSetCreate(None, None, fm, 4, 10, C.byref(st)) and st.value == SLIM_ERROR_INPUT
    assert lib.SLIMGPU_ModelEvaluate(None, None, np.zeros(4), np.zeros(3, np.int32)) == SLIM_ERROR_INPUT
    assert lib.SLIMGPU_MatrixPredict(10, None, None, np.zeros(10, np.int32), np.zeros(10, np.float32)) == SLIM_ERROR_INPUT
    assert lib.SLIMGPU_LastEvalStats(None) == SLIM_ERROR_INPUT
    out = _lib.EvalStats()
    assert lib.SLIMGPU_LastEvalStats(C.byref(out)) == SLIM_OK
    lib.SLIMGPU_EvalSetFree(C.byref(C.c_void_p(None)))   # no-op
