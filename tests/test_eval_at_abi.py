"""The entry points of the evaluation at several list lengths and on a subset of the users
(include/slim_gpu_eval.h: SLIMGPU_EvalSetCreateAt, SLIMGPU_ModelEvaluateAt) and the option slot of the
grid are declared, exported and bound.  No GPU needed."""
import ctypes as C
import os
import re

import numpy as np

from conftest import ROOT
from slim_amd import _lib
from slim_amd.constants import SLIM_ERROR_INPUT, SLIM_NOPTIONS, Opt
from slim_amd.interface import build_options

NEW = {
    "SLIMGPU_EvalSetCreateAt": ("slimgpu_evalset_t *", ["slimgpu_matrix_t *mat", "slim_t *tsthandle",
                                                        "const int32_t *fmarker", "int32_t fm_ncols",
                                                        "int32_t ncutoffs", "const int32_t *cutoffs",
                                                        "int32_t nusers", "const int32_t *users",
                                                        "int32_t *r_status"]),
    "SLIMGPU_ModelEvaluateAt": ("int32_t", ["slimgpu_evalset_t *es", "const slimgpu_model_t *model",
                                            "int32_t ncutoffs", "double *metrics", "int32_t *nvalid"]),
}


def _header():
    text = open(os.path.join(ROOT, "include", "slim_gpu_eval.h")).read()
    return re.sub(r"/\*.*?\*/", "", text, flags=re.S)


def test_symbols_are_declared_exported_and_bound():
    text = re.sub(r"\s+", " ", _header())
    raw = C.CDLL(_lib.LIB_PATH)
    for name, (res, args) in NEW.items():
        m = re.search(r"([\w ]+\*?) ?\b%s ?\(([^)]*)\)" % name, text)
        assert m, "%s is not declared in slim_gpu_eval.h" % name
        assert m.group(1).strip().replace(" *", "*") == res.strip().replace(" *", "*"), (name, m.group(1))
        assert [a.strip() for a in m.group(2).split(",")] == args, name
        assert hasattr(raw, name), "libslim.so does not export %s" % name
        r, a = _lib._EVAL_AT_SIGNATURES[name]
        assert len(a) == len(args)
    assert set(NEW) == set(_lib.EVAL_AT_SYMBOLS)
    assert _lib._EVAL_AT_SIGNATURES["SLIMGPU_EvalSetCreateAt"][0] is C.c_void_p
    assert _lib._EVAL_AT_SIGNATURES["SLIMGPU_ModelEvaluateAt"][0] is C.c_int32
    assert re.search(r"#define SLIMGPU_MAX_CUTOFFS 8\b", _header()) and _lib.MAX_CUTOFFS == 8
    # the table of the evaluation in HBM keeps its five names
    assert len(_lib.EVAL_SYMBOLS) == 5 and not set(NEW) & set(_lib.EVAL_SYMBOLS)
    # loaded prototypes are attached
    lib = _lib.load()
    assert lib.SLIMGPU_ModelEvaluateAt.restype is C.c_int32


def test_null_arguments_are_refused_without_a_device():
    lib = _lib.load()
    st = C.c_int32(0)
    fm = np.zeros(4, np.int32)
    cut = np.array([5, 10], np.int32)
    assert not lib.SLIMGPU_EvalSetCreateAt(None, None, fm, 4, 2, cut.ctypes.data_as(C.c_void_p), 0, None,
                                           C.byref(st))
    assert st.value == SLIM_ERROR_INPUT and _lib.last_error()
    st.value = 0
    assert not lib.SLIMGPU_EvalSetCreateAt(None, None, fm, 4, 1, None, 0, None, C.byref(st))
    assert st.value == SLIM_ERROR_INPUT
    assert lib.SLIMGPU_ModelEvaluateAt(None, None, 2, np.zeros(8), np.zeros(6, np.int32)) == SLIM_ERROR_INPUT
    assert lib.SLIMGPU_ModelEvaluateAt(None, None, 0, np.zeros(8), np.zeros(6, np.int32)) == SLIM_ERROR_INPUT
    assert lib.SLIMGPU_ModelEvaluateAt(None, None, 9, np.zeros(36), np.zeros(27, np.int32)) == SLIM_ERROR_INPUT


def test_option_slot():
    assert Opt.GPU_EVALSTRIDE == 22 and 22 < SLIM_NOPTIONS
    assert re.search(r"SLIM_OPTION_GPU_EVALSTRIDE = 22\b", _header())
    from slim_amd.interface import check_params
    for params, want in (({"gpu_evalstride": 5}, 5), ({}, -1)):
        check_params(params)                 # fills in the defaults of the other keys
        params.setdefault("nrcmds", 10)
        iopt, _ = build_options(params)
        assert iopt[22] == want
