"""Loader for the in-tree C-ABI library slim_amd/libslim.so.

The library is the product: there is no Python or CPU fallback for training.
If it is missing, or if a call reports an error, the caller gets an exception
that says so.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# SLIM_AMD_LIB points at another build of the same library (A/B comparisons of kernels)
LIB_PATH = os.environ.get("SLIM_AMD_LIB") or os.path.join(_HERE, "libslim.so")

f64_1d = np.ctypeslib.ndpointer(dtype=np.float64, ndim=1, flags="C_CONTIGUOUS")
f32_1d = np.ctypeslib.ndpointer(dtype=np.float32, ndim=1, flags="C_CONTIGUOUS")
i32_1d = np.ctypeslib.ndpointer(dtype=np.int32, ndim=1, flags="C_CONTIGUOUS")
i64_1d = np.ctypeslib.ndpointer(dtype=np.int64, ndim=1, flags="C_CONTIGUOUS")
isz_1d = np.ctypeslib.ndpointer(dtype=np.intp, ndim=1, flags="C_CONTIGUOUS")


class Stats(C.Structure):
    """slimgpu_stats_t (include/slim_gpu.h)."""
    _fields_ = [("ncols_solved", C.c_int32), ("kernel", C.c_int32), ("nwaves", C.c_int32),
                ("lds_bytes", C.c_int32), ("setup_ms", C.c_double), ("kernel_ms", C.c_double),
                ("gather_ms", C.c_double), ("total_ms", C.c_double),
                ("G", C.c_int64), ("D", C.c_int64), ("U", C.c_int64), ("nnzW", C.c_int64),
                ("sweeps", C.c_int64), ("visits", C.c_int64), ("alg_bytes", C.c_double),
                ("error", C.c_double), ("objval", C.c_double), ("gram_build_ms", C.c_double),
                ("gram_rows", C.c_int64), ("gram_bytes", C.c_double),
                ("gram_alloc_ms", C.c_double), ("gram_sums_ms", C.c_double),
                ("gram_sums_kernel_ms", C.c_double), ("gram_pack_ms", C.c_double)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class EvalStats(C.Structure):
    """slimgpu_eval_stats_t (include/slim_gpu_eval.h)."""
    _fields_ = [("path", C.c_int32), ("device_allocs", C.c_int32), ("h2d_bytes", C.c_int64),
                ("d2h_bytes", C.c_int64), ("kernel_ms", C.c_double), ("total_ms", C.c_double),
                ("w_rows_read", C.c_int64), ("w_bytes", C.c_double)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class CsrView(C.Structure):
    """slim_csr_t (include/slim_gpu.h): the object behind every handle."""
    _fields_ = ([("nrows", C.c_int32), ("ncols", C.c_int32),
                 ("rowptr", C.POINTER(C.c_ssize_t)), ("colptr", C.POINTER(C.c_ssize_t)),
                 ("rowind", C.POINTER(C.c_int32)), ("colind", C.POINTER(C.c_int32))] +
                [(n, C.POINTER(C.c_int32)) for n in
                 ("rowids", "colids", "rlabels", "clabels", "rmap", "cmap")] +
                [(n, C.POINTER(C.c_float)) for n in
                 ("rowval", "colval", "rnorms", "cnorms", "rsums", "csums", "rsizes",
                  "csizes", "rvols", "cvols", "rwgts", "cwgts")])


_SIGNATURES = {
    # slim.h
    "SLIM_iSetDefaults": (C.c_int32, [i32_1d]),
    "SLIM_dSetDefaults": (C.c_int32, [f64_1d]),
    "SLIM_Learn": (C.c_void_p, [C.c_int32, isz_1d, i32_1d, C.c_void_p, C.c_void_p, C.c_void_p,
                                C.c_void_p, C.POINTER(C.c_int32)]),
    "SLIM_GetTopN": (C.c_int32, [C.c_void_p, C.c_int32, i32_1d, C.c_void_p, C.c_void_p,
                                 C.c_int32, i32_1d, f32_1d]),
    "SLIM_WriteModel": (C.c_int32, [C.c_void_p, C.c_char_p]),
    "SLIM_ReadModel": (C.c_void_p, [C.c_char_p]),
    "SLIM_FreeModel": (None, [C.POINTER(C.c_void_p)]),
    "SLIM_DetermineHeadAndTail": (C.POINTER(C.c_int32), [C.c_int32, C.c_int32, isz_1d, i32_1d]),
    # Py_* (slim_gpu.h section 2)
    "Py_csr_wrapper": (C.c_int32, [C.c_int32, isz_1d, i32_1d, C.c_void_p, C.c_void_p]),
    "Py_csr_save": (C.c_int32, [C.c_void_p, C.c_char_p]),
    "Py_csr_load": (C.c_int32, [C.c_void_p, C.c_char_p]),
    "Py_csr_free": (C.c_int32, [C.c_void_p]),
    "Py_csr_stat": (C.c_int32, [C.c_void_p, C.c_void_p]),
    "Py_csr_export": (C.c_int32, [C.c_void_p, i32_1d, i32_1d, f32_1d]),
    "Py_SLIM_Learn": (C.c_int32, [C.c_void_p, i32_1d, f64_1d, C.c_void_p]),
    "Py_SLIM_Mselect": (C.c_int32, [C.c_void_p, C.c_void_p, i32_1d, f64_1d, f64_1d, f64_1d,
                                    C.c_int32, C.c_int32] + [C.c_void_p] * 8),
    "Py_SLIM_GetTopN": (C.c_int32, [C.c_void_p, C.c_int32, i32_1d, C.c_void_p, C.c_int32,
                                    i32_1d, f32_1d, C.c_int32]),
    "Py_SLIM_GetTopN_1vsk": (C.c_int32, [C.c_void_p, C.c_int32, i32_1d, C.c_void_p, C.c_int32,
                                         i32_1d, f32_1d, C.c_int32, i32_1d, C.c_int32]),
    "Py_SLIM_Predict": (C.c_int32, [C.c_int32, C.c_void_p, C.c_void_p, i32_1d, f32_1d]),
    "Py_SLIM_Predict_1vsk": (C.c_int32, [C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, i32_1d,
                                         i32_1d, f32_1d]),
    # SLIMGPU_* (slim_gpu.h section 3)
    "SLIMGPU_MatrixFromHost": (C.c_void_p, [C.c_int32, isz_1d, i32_1d, C.c_void_p, C.c_void_p,
                                            C.POINTER(C.c_int32)]),
    "SLIMGPU_MatrixFromDevice": (C.c_void_p, [C.c_int32, C.c_int32, C.c_void_p, C.c_void_p,
                                              C.c_void_p, C.c_void_p, C.POINTER(C.c_int32)]),
    "SLIMGPU_MatrixFree": (None, [C.POINTER(C.c_void_p)]),
    "SLIMGPU_MatrixInfo": (C.c_int32, [C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_int32),
                                       C.POINTER(C.c_int64)]),
    "SLIMGPU_MatrixGetColumnView": (C.c_int32, [C.c_void_p] * 5),
    "SLIMGPU_MatrixColumnCost": (C.c_int32, [C.c_void_p, C.c_void_p]),
    "SLIMGPU_MatrixExpectSolves": (None, [C.c_void_p, C.c_int32]),
    "SLIMGPU_MatrixDevice": (C.c_int32, [C.c_void_p]),
    "SLIMGPU_MatrixGramBuildRows": (C.c_int32, [C.c_void_p, C.c_int32, C.c_int32]),
    "SLIMGPU_MatrixGramView": (C.c_int32, [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_int64),
                                           C.POINTER(C.c_int32)]),
    "SLIMGPU_MatrixGramCommit": (C.c_int32, [C.c_void_p]),
    "SLIMGPU_Learn": (C.c_void_p, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                   C.POINTER(C.c_int32)]),
    "SLIMGPU_LearnResident": (C.c_void_p, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                           C.POINTER(C.c_int32)]),
    "SLIMGPU_ModelNnz": (C.c_int64, [C.c_void_p]),
    "SLIMGPU_ModelFetchBegin": (C.c_int32, [C.c_void_p]),
    "SLIMGPU_ModelFetch": (C.c_void_p, [C.c_void_p, C.POINTER(C.c_int32)]),
    "SLIMGPU_ModelFree": (None, [C.POINTER(C.c_void_p)]),
    "SLIMGPU_ModelPredict": (C.c_int32, [C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "SLIMGPU_LearnColumns": (C.c_void_p, [C.c_void_p, C.c_int32, i32_1d, C.c_void_p, C.c_void_p,
                                          C.c_void_p, C.POINTER(C.c_int32)]),
    "SLIMGPU_Predict": (C.c_int32, [C.c_int32, C.c_void_p, C.c_void_p, i32_1d, f32_1d]),
    "SLIMGPU_Predict1vsK": (C.c_int32, [C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, i32_1d,
                                        i32_1d, f32_1d]),
    "SLIMGPU_Evaluate": (C.c_int32, [C.c_int32, C.c_int32, i32_1d, i32_1d, C.c_void_p, i32_1d,
                                     C.c_int32, f64_1d, i32_1d]),
    "SLIMGPU_LastStats": (C.c_int32, [C.POINTER(Stats)]),
    "SLIMGPU_LastColumnStats": (C.c_int32, [C.c_int32] + [C.c_void_p] * 6),
    "SLIMGPU_DeviceCount": (C.c_int32, []),
    "SLIMGPU_LastError": (C.c_char_p, []),
}

EXPORTED_SYMBOLS = tuple(_SIGNATURES)

# evaluation in HBM (include/slim_gpu_eval.h)
_EVAL_SIGNATURES = {
    "SLIMGPU_EvalSetCreate": (C.c_void_p, [C.c_void_p, C.c_void_p, i32_1d, C.c_int32, C.c_int32,
                                           C.POINTER(C.c_int32)]),
    "SLIMGPU_EvalSetFree": (None, [C.POINTER(C.c_void_p)]),
    "SLIMGPU_ModelEvaluate": (C.c_int32, [C.c_void_p, C.c_void_p, f64_1d, i32_1d]),
    "SLIMGPU_MatrixPredict": (C.c_int32, [C.c_int32, C.c_void_p, C.c_void_p, i32_1d, f32_1d]),
    "SLIMGPU_LastEvalStats": (C.c_int32, [C.POINTER(EvalStats)]),
}

EVAL_SYMBOLS = tuple(_EVAL_SIGNATURES)

# ... at several list lengths and on a subset of the users, from one scoring pass
_EVAL_AT_SIGNATURES = {
    "SLIMGPU_EvalSetCreateAt": (C.c_void_p, [C.c_void_p, C.c_void_p, i32_1d, C.c_int32, C.c_int32, C.c_void_p,
                                             C.c_int32, C.c_void_p, C.POINTER(C.c_int32)]),
    "SLIMGPU_ModelEvaluateAt": (C.c_int32, [C.c_void_p, C.c_void_p, C.c_int32, f64_1d, i32_1d]),
}

EVAL_AT_SYMBOLS = tuple(_EVAL_AT_SIGNATURES)


class GramPlanes(C.Structure):
    """slimgpu_gram_planes_t (include/slim_gpu_planes.h): device pointers and sizes."""
    _fields_ = ([("ncols", C.c_int32), ("nchunks", C.c_int32), ("ldb", C.c_int64), ("hi_bytes", C.c_int64)] +
                [(n, C.c_void_p) for n in ("lo", "base", "hi", "hi_off", "hi_k", "hi2_k", "diag", "meta",
                                           "rank_of", "item_of")])


# a look at the byte planes of G (include/slim_gpu_planes.h)
_PLANES_SIGNATURES = {
    "SLIMGPU_MatrixGramPlanes": (C.c_int32, [C.c_void_p, C.POINTER(GramPlanes)]),
}

PLANES_SYMBOLS = tuple(_PLANES_SIGNATURES)
MAX_CUTOFFS = 8     # SLIMGPU_MAX_CUTOFFS

# the rank of every held-out item: evaluation at any list length (include/slim_gpu_rank.h)
_RANK_SIGNATURES = {
    "SLIMGPU_EvalSetCreateRanked": (C.c_void_p, [C.c_void_p, C.c_void_p, i32_1d, C.c_int32, C.c_int32, C.c_void_p,
                                                 C.POINTER(C.c_int32)]),
    "SLIMGPU_EvalSetEntries": (C.c_int64, [C.c_void_p]),
    "SLIMGPU_ModelRanks": (C.c_int32, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "SLIMGPU_ModelEvaluateRanked": (C.c_int32, [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, f64_1d, i32_1d]),
    "SLIMGPU_ModelFromHost": (C.c_void_p, [C.c_void_p, C.c_void_p, C.POINTER(C.c_int32)]),
    "SLIMGPU_LastRankPrepassMs": (C.c_double, []),
}

RANK_SYMBOLS = tuple(_RANK_SIGNATURES)
MAX_RANK_CUTOFFS = 32   # SLIMGPU_MAX_RANK_CUTOFFS


class ListStats(C.Structure):
    """slimgpu_list_stats_t (include/slim_gpu_lists.h)."""
    _fields_ = [("path", C.c_int32), ("slices", C.c_int32), ("candidates", C.c_int64), ("contenders", C.c_int64),
                ("refine_passes", C.c_int64), ("lds_sorts", C.c_int64), ("key_refines", C.c_int64)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


# top-N lists of up to SLIMGPU_MAX_LIST items on the device (include/slim_gpu_lists.h); output / scores /
# counts / users are passed as pointers (counts and users may be None)
_LIST_SIGNATURES = {
    "SLIMGPU_PredictLists": (C.c_int32, [C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "SLIMGPU_ModelPredictLists": (C.c_int32, [C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                              C.c_void_p]),
    "SLIMGPU_MatrixPredictLists": (C.c_int32, [C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p,
                                               C.c_void_p, C.c_void_p, C.c_void_p]),
    "SLIMGPU_LastListStats": (C.c_int32, [C.POINTER(ListStats)]),
}

LIST_SYMBOLS = tuple(_LIST_SIGNATURES)
MAX_LIST = 4096         # SLIMGPU_MAX_LIST

# candidate filters for those lists (include/slim_gpu_filter.h): item allow / block sets, per-user exclusions
_FILTER_SIGNATURES = {
    "SLIMGPU_FilterCreate": (C.c_int32, [C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p,
                                         C.c_void_p, C.POINTER(C.c_void_p)]),
    "SLIMGPU_FilterFree": (None, [C.c_void_p]),
    "SLIMGPU_PredictListsFiltered": (C.c_int32, [C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                                 C.c_void_p, C.c_void_p]),
    "SLIMGPU_ModelPredictListsFiltered": (C.c_int32, [C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                                      C.c_void_p, C.c_void_p]),
    "SLIMGPU_MatrixPredictListsFiltered": (C.c_int32, [C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p,
                                                       C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "Py_SLIM_PredictFiltered": (C.c_int32, [C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, i32_1d, f32_1d]),
}

FILTER_SYMBOLS = tuple(_FILTER_SIGNATURES)

# evaluation, ranks and the model-selection grid under a filter (include/slim_gpu_filter_eval.h): the unfiltered
# calls' arguments with the filter handle behind the model (the grid: as its last argument)
_FILTERED_EVAL_SIGNATURES = {
    "SLIMGPU_ModelEvaluateAtFiltered": (C.c_int32, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, f64_1d, i32_1d]),
    "SLIMGPU_ModelRanksFiltered": (C.c_int32, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "SLIMGPU_ModelEvaluateRankedFiltered": (C.c_int32, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p,
                                                        f64_1d, i32_1d]),
    "Py_SLIM_MselectFiltered": (C.c_int32, [C.c_void_p, C.c_void_p, i32_1d, f64_1d, f64_1d, f64_1d,
                                            C.c_int32, C.c_int32] + [C.c_void_p] * 9),
}

FILTERED_EVAL_SYMBOLS = tuple(_FILTERED_EVAL_SIGNATURES)

# per-user candidate sets scored and ordered on the device (include/slim_gpu_cand.h); slot_scores / output / scores /
# counts / users are passed as pointers (any may be None)
_CAND_SIGNATURES = {
    "SLIMGPU_CandSetCreate": (C.c_int32, [C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.POINTER(C.c_void_p)]),
    "SLIMGPU_CandSetFree": (None, [C.c_void_p]),
    "SLIMGPU_ScoreCandidates": (C.c_int32, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p,
                                            C.c_void_p, C.c_void_p]),
    "SLIMGPU_MatrixScoreCandidates": (C.c_int32, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p,
                                                  C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "SLIMGPU_ModelEvaluateCandidates": (C.c_int32, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, f64_1d, i32_1d]),
    "Py_SLIM_ScoreCandidates": (C.c_int32, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p,
                                            C.c_void_p, C.c_void_p]),
}

CAND_SYMBOLS = tuple(_CAND_SIGNATURES)

# sampled negatives for the 1-vs-k protocol (include/slim_gpu_sample.h): candidate sets made on the device or on the
# host, and the rows of any set copied out; users / cptr / cind are passed as pointers (any may be None)
_SAMPLE_SIGNATURES = {
    "SLIMGPU_EvalSetSampleCandidates": (C.c_int32, [C.c_void_p, C.c_int32, C.c_uint64, C.POINTER(C.c_void_p)]),
    "SLIMGPU_CandSetSample": (C.c_int32, [C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32,
                                          C.c_uint64, C.POINTER(C.c_void_p)]),
    "SLIMGPU_CandSetRows": (C.c_int32, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "SLIMGPU_CandSetInfo": (C.c_int32, [C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_int32),
                                        C.POINTER(C.c_int64)]),
}

SAMPLE_SYMBOLS = tuple(_SAMPLE_SIGNATURES)

# popularity-weighted negatives (include/slim_gpu_wsample.h): the two samplers under the weighted rule; weights is a
# pointer to ncols uint32 (None: popularity)
_WSAMPLE_SIGNATURES = {
    "SLIMGPU_EvalSetSampleCandidatesWeighted": (C.c_int32, [C.c_void_p, C.c_int32, C.c_uint64, C.c_void_p,
                                                            C.POINTER(C.c_void_p)]),
    "SLIMGPU_CandSetSampleWeighted": (C.c_int32, [C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32,
                                                  C.c_uint64, C.c_void_p, C.POINTER(C.c_void_p)]),
    "SLIMGPU_LastSampleKernelMs": (C.c_double, []),
}

WSAMPLE_SYMBOLS = tuple(_WSAMPLE_SIGNATURES)

# explanations: the history items behind a candidate's score (include/slim_gpu_explain.h); why_items / why_terms /
# support / users are passed as pointers (any may be None)
_EXPLAIN_SIGNATURES = {
    "SLIMGPU_ExplainCandidates": (C.c_int32, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p,
                                              C.c_void_p]),
    "SLIMGPU_MatrixExplainCandidates": (C.c_int32, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p,
                                                    C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]),
    "Py_SLIM_ExplainCandidates": (C.c_int32, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p,
                                              C.c_void_p]),
}

EXPLAIN_SYMBOLS = tuple(_EXPLAIN_SIGNATURES)
MAX_WHY = 16            # SLIMGPU_MAX_WHY


class Exposure(C.Structure):
    """slimgpu_exposure_t (include/slim_gpu_exposure.h): the summary of one cutoff."""
    _fields_ = [("lists", C.c_int64), ("slots", C.c_int64), ("tail_slots", C.c_int64), ("outside", C.c_int64),
                ("distinct", C.c_int32), ("ncols", C.c_int32), ("coverage", C.c_double), ("tail_share", C.c_double),
                ("gini", C.c_double), ("avg_pop", C.c_double)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


# exposure of top-N lists (include/slim_gpu_exposure.h): per-item counts and their summaries; pop / fmarker / ids /
# counts / users / cutoffs / exposure / summary are passed as pointers (those the header lets be NULL may be None)
_EXPOSURE_SIGNATURES = {
    "SLIMGPU_ListExposure": (C.c_int32, [C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_int64, C.c_int32,
                                         C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]),
    "SLIMGPU_MatrixListExposure": (C.c_int32, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int64, C.c_int32, C.c_void_p,
                                               C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]),
    "SLIMGPU_MatrixPredictExposure": (C.c_int32, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p,
                                                  C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p,
                                                  C.c_void_p, C.c_void_p]),
    "SLIMGPU_ModelEvaluateExposure": (C.c_int32, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, f64_1d, i32_1d,
                                                  C.c_void_p, C.c_void_p]),
    "Py_SLIM_MselectExposure": (C.c_int32, [C.c_void_p, C.c_void_p, i32_1d, f64_1d, f64_1d, f64_1d,
                                            C.c_int32, C.c_int32] + [C.c_void_p] * 10),
}

EXPOSURE_SYMBOLS = tuple(_EXPOSURE_SIGNATURES)
EXPOSURE_CELL = 8       # SLIMGPU_EXPOSURE_CELL: l1, l2, HR, ARHR, coverage, tail_share, gini, avg_pop



class GridCell(C.Structure):
    """slimgpu_grid_cell_t (include/slim_gpu_grid.h): what one solved pair of a grid gives."""
    _fields_ = [("l1r", C.c_double), ("l2r", C.c_double), ("nnz", C.c_int64), ("metrics", C.c_double * 4),
                ("nvalid", C.c_int32 * 3), ("has_exposure", C.c_int32), ("exposure", Exposure),
                ("solve_seconds", C.c_double)]


# the model-selection grid's evaluator (include/slim_gpu_grid.h): what Py_SLIM_Mselect* and slim_mselect loop over
_GRID_SIGNATURES = {
    "SLIMGPU_GridOpen": (C.c_int32, [C.c_void_p, C.c_void_p, i32_1d, f64_1d, C.c_int32, C.c_int32, C.c_void_p,
                                     C.POINTER(C.c_void_p)]),
    "SLIMGPU_GridDescribe": (None, [C.c_void_p]),
    "SLIMGPU_GridSolve": (C.c_int32, [C.c_void_p, C.c_double, C.c_double, C.POINTER(GridCell)]),
    "SLIMGPU_GridModel": (C.c_void_p, [C.c_void_p, C.POINTER(C.c_int32)]),
    "SLIMGPU_GridFree": (None, [C.POINTER(C.c_void_p)]),
}

GRID_SYMBOLS = tuple(_GRID_SIGNATURES)

# per-group figures of an evaluation and a grid that selects on a group (include/slim_gpu_groups.h); the arrays are
# passed as pointers
_GROUP_SIGNATURES = {
    "SLIMGPU_EvalSetSetGroups": (C.c_int32, [C.c_void_p, C.c_int32, C.c_void_p]),
    "SLIMGPU_EvalSetSetHistoryBands": (C.c_int32, [C.c_void_p, C.c_int32, C.c_void_p]),
    "SLIMGPU_EvalSetClearGroups": (None, [C.c_void_p]),
    "SLIMGPU_EvalSetGroupInfo": (C.c_int32, [C.c_void_p, C.POINTER(C.c_int32), C.c_void_p]),
    "SLIMGPU_EvalSetLastGroupFigures": (C.c_int32, [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]),
    "SLIMGPU_GroupPartition": (C.c_int32, [C.c_int32, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p,
                                           C.c_void_p]),
    "SLIMGPU_GridSetGroups": (C.c_int32, [C.c_void_p, C.c_int32, C.c_void_p, C.c_int32]),
    "SLIMGPU_GridGroupInfo": (C.c_int32, [C.c_void_p, C.POINTER(C.c_int32), C.c_void_p]),
    "SLIMGPU_GridLastGroups": (C.c_int32, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "Py_SLIM_MselectGrouped": (C.c_int32, [C.c_void_p, C.c_void_p, i32_1d, f64_1d, f64_1d, f64_1d,
                                           C.c_int32, C.c_int32] + [C.c_void_p] * 9 +
                               [C.c_int32, C.c_void_p, C.c_int32, C.c_void_p]),
}

GROUP_SYMBOLS = tuple(_GROUP_SIGNATURES)
MAX_GROUPS = 1024       # SLIMGPU_MAX_GROUPS
GROUP_CELL = 9          # SLIMGPU_GROUP_CELL: l1, l2, HR, HR_head, HR_tail, ARHR, nvalid, nvalid_head, nvalid_tail


class Split(C.Structure):
    """slimgpu_split_t (include/slim_gpu_split.h): the parameters of a train / test split."""
    _fields_ = [("mode", C.c_int32), ("nfolds", C.c_int32), ("fold", C.c_int32), ("nheld", C.c_int32),
                ("minkeep", C.c_int32), ("seed", C.c_uint64)]


# one matrix split into train and test, on the host or where the staged matrix lies (include/slim_gpu_split.h), and
# the grid on a staged matrix and cross-validated over such folds
_SPLIT_SIGNATURES = {
    "SLIMGPU_SplitHost": (C.c_int32, [C.c_void_p, C.POINTER(Split), C.POINTER(C.c_void_p), C.POINTER(C.c_void_p)]),
    "SLIMGPU_MatrixSplit": (C.c_int32, [C.c_void_p, C.POINTER(Split), C.POINTER(C.c_void_p), C.POINTER(C.c_void_p)]),
    "SLIMGPU_GridOpenOn": (C.c_int32, [C.c_void_p, C.c_void_p, i32_1d, f64_1d, C.c_int32, C.c_int32, C.c_void_p,
                                       C.POINTER(C.c_void_p)]),
    "Py_SLIM_MselectCV": (C.c_int32, [C.c_void_p, i32_1d, f64_1d, f64_1d, f64_1d, C.c_int32, C.c_int32,
                                      C.POINTER(Split), C.c_void_p] + [C.c_void_p] * 9),
    "SLIMGPU_MselectCVPairs": (C.c_int32, [C.c_void_p, i32_1d, f64_1d, C.c_int32, f64_1d, f64_1d, C.POINTER(Split),
                                           C.c_void_p, f64_1d, C.c_void_p]),
}

SPLIT_SYMBOLS = tuple(_SPLIT_SIGNATURES)
SPLIT_LEAVE_OUT, SPLIT_FOLDS = 0, 1     # SLIMGPU_SPLIT_LEAVE_OUT, SLIMGPU_SPLIT_FOLDS
SPLIT_MAX_HELD = 128                    # SLIMGPU_SPLIT_MAX_HELD
EVAL_PATH_SPLIT = 7                     # SLIMGPU_EVAL_PATH_SPLIT
CV_CELL = 11                            # SLIMGPU_CV_CELL: fold, l1, l2, HR, HR_head, HR_tail, ARHR, 3 nvalid, nnz

_lib = None


def load():
    """Return the ctypes handle of libslim.so with every prototype attached."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            "slim_amd: %s is missing -- build it with `python -c 'import __graft_entry__ as g; "
            "g.build()'` (hipcc, gfx950). There is no CPU fallback for SLIM training." % LIB_PATH)
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in (list(_SIGNATURES.items()) + list(_EVAL_SIGNATURES.items()) +
                              list(_EVAL_AT_SIGNATURES.items()) + list(_PLANES_SIGNATURES.items()) +
                              list(_RANK_SIGNATURES.items()) + list(_LIST_SIGNATURES.items()) +
                              list(_FILTER_SIGNATURES.items()) + list(_FILTERED_EVAL_SIGNATURES.items()) +
                              list(_CAND_SIGNATURES.items()) + list(_SAMPLE_SIGNATURES.items()) +
                              list(_WSAMPLE_SIGNATURES.items()) + list(_EXPLAIN_SIGNATURES.items()) +
                              list(_EXPOSURE_SIGNATURES.items()) + list(_GRID_SIGNATURES.items()) +
                              list(_GROUP_SIGNATURES.items()) + list(_SPLIT_SIGNATURES.items())):
        if os.environ.get("SLIM_AMD_LIB") and not hasattr(lib, name):
            continue  # an older build used for an A/B run may lack the newest entry points
        fn = getattr(lib, name)  # AttributeError here = ABI drift, fail loudly
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def last_error():
    msg = load().SLIMGPU_LastError()
    return msg.decode("utf-8", "replace") if msg else ""
