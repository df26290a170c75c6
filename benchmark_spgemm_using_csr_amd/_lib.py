"""ctypes binding of libbhsparse_hip.so (include/bhsparse_hip.h).

No fallback: if the HIP library is missing or fails to load this raises — the
product path never routes through a CPU implementation.
"""
import ctypes as C
import os
import subprocess
import sys

_HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(_HERE, "csrc")
# BHSPARSE_HIP_LIB: alternate build of the same library (measurement variants); never a fallback
SO_PATH = os.environ.get("BHSPARSE_HIP_LIB") or os.path.join(CSRC, "libbhsparse_hip.so")
HEADER = os.path.join(os.path.dirname(_HERE), "include", "bhsparse_hip.h")

BHS_SUCCESS = 0
BHS_ERR_INVALID_ARG = -1
BHS_ERR_NO_DEVICE = -2
BHS_ERR_ALLOC = -3
BHS_ERR_LAUNCH = -4
BHS_ERR_NNZ_OVERFLOW = -5
BHS_ERR_NOT_READY = -6
BHS_ERR_INTERNAL = -7
BHS_ERR_PEER = -8


class KernelStat(C.Structure):
    _fields_ = [("name", C.c_char_p), ("launches", C.c_int), ("ms", C.c_double),
                ("rows", C.c_int64), ("products", C.c_int64), ("nnz_out", C.c_int64),
                ("nnzA_rows", C.c_int64)]


class Select(C.Structure):
    """bhs_select (include/bhsparse_hip.h, "entry selection")"""
    _fields_ = [("flags", C.c_uint32), ("top_k", C.c_int32), ("band_lo", C.c_int64), ("band_hi", C.c_int64),
                ("abs_tol", C.c_double), ("rel_tol", C.c_double)]


BHS_SEL_BAND, BHS_SEL_DROP_DIAG, BHS_SEL_KEEP_DIAG, BHS_SEL_ABS, BHS_SEL_REL, BHS_SEL_TOPK = 1, 2, 4, 8, 16, 32

# the semirings of bhs_spgemm_semiring* (include/bhsparse_hip.h, "semiring multiply")
(BHS_SR_PLUS_TIMES, BHS_SR_MIN_PLUS, BHS_SR_MAX_PLUS, BHS_SR_MAX_TIMES, BHS_SR_MIN_MAX, BHS_SR_MAX_MIN, BHS_SR_OR_AND,
 BHS_SR_PLUS_PAIR) = range(8)
SEMIRINGS = {"plus_times": BHS_SR_PLUS_TIMES, "min_plus": BHS_SR_MIN_PLUS, "max_plus": BHS_SR_MAX_PLUS,
             "max_times": BHS_SR_MAX_TIMES, "min_max": BHS_SR_MIN_MAX, "max_min": BHS_SR_MAX_MIN, "or_and": BHS_SR_OR_AND,
             "plus_pair": BHS_SR_PLUS_PAIR}

# bhs_csr_reduce_device / bhs_csr_scale_device (include/bhsparse_hip.h, "reduce / scale")
BHS_AXIS_ROWS, BHS_AXIS_COLS, BHS_AXIS_ALL, BHS_AXIS_DIAG = range(4)
(BHS_RED_PLUS, BHS_RED_MIN, BHS_RED_MAX, BHS_RED_ABS_PLUS, BHS_RED_ABS_MAX, BHS_RED_SQ_PLUS, BHS_RED_COUNT) = range(7)
BHS_RED_OFFDIAG = 1
BHS_SCALE_LEFT_DIV, BHS_SCALE_RIGHT_DIV = 1, 2

# bhs_csr_sddmm_device (include/bhsparse_hip.h, "sampled dense-dense product")
BHS_SDDMM_TIMES_M = 1

# bhs_csr_fsai_device (include/bhsparse_hip.h, "approximate inverse")
BHS_FSAI_MAX_ROW = 128

# bhs_csr_spmv_semiring_device / bhs_csr_spmm_semiring_device (include/bhsparse_hip.h, "semiring CSR x dense")
BHS_MV_ACCUM, BHS_MV_MASK_COMPLEMENT = 1, 2

# bhs_csr_gs_device (include/bhsparse_hip.h, "colouring and relaxation")
BHS_GS_FORWARD, BHS_GS_BACKWARD, BHS_GS_SYMMETRIC, BHS_GS_VERIFY = 1, 2, 3, 4

# bhs_csr_relax_device (include/bhsparse_hip.h, "relaxation and fused products")
BHS_RELAX_ZERO_GUESS = 1

# bhs_csr_levels_device / bhs_csr_trsv_device (include/bhsparse_hip.h, "triangular solve and ILU(0)")
BHS_TRI_LOWER, BHS_TRI_UPPER, BHS_TRI_UNIT_DIAG = 1, 2, 4

# bhs_csr_spanning_forest_device (include/bhsparse_hip.h, "spanning forest")
BHS_FOREST_MAXIMUM, BHS_FOREST_ABS = 1, 2

# bhs_csr_cfsplit_device (include/bhsparse_hip.h, "C/F splitting and interpolation")
BHS_CF_DEGREE = 1

# bhs_csr_betweenness_device (include/bhsparse_hip.h, "betweenness centrality")
BHS_BC_ACCUMULATE = 1

# bhs_coo_assemble_device / bhs_coo_assemble_values_device (include/bhsparse_hip.h, "assembly")
BHS_COO_SUM, BHS_COO_FIRST, BHS_COO_LAST, BHS_COO_KEEP, BHS_COO_IGNORE_NEGATIVE = 0, 1, 2, 3, 4
COO_COMBINE = {"sum": BHS_COO_SUM, "first": BHS_COO_FIRST, "last": BHS_COO_LAST, "keep": BHS_COO_KEEP}


# every symbol include/bhsparse_hip.h declares: (restype, argtypes)
_vp, _i, _i64 = C.c_void_p, C.c_int, C.c_int64
SYMBOLS = {
    "bhs_create": (_i, [C.POINTER(_vp), _i, C.POINTER(_i)]),
    "bhs_destroy": (_i, [_vp]),
    "bhs_set_verbose": (_i, [_vp, _i]),
    "bhs_set_data": (_i, [_vp, _i, _i, _i, _i, _vp, _vp, _vp, _i, _vp, _vp, _vp]),
    "bhs_set_data_device": (_i, [_vp, _i, _i, _i, _i, _vp, _vp, _vp, _i, _vp, _vp, _vp]),
    "bhs_free_data": (_i, [_vp]),
    "bhs_warmup": (_i, [_vp]),
    "bhs_spgemm": (_i, [_vp, _vp, C.POINTER(_i64), C.POINTER(_i), C.POINTER(C.c_double)]),
    "bhs_spgemm_symbolic": (_i, [_vp, C.POINTER(_i64), C.POINTER(_i)]),
    "bhs_set_output_device": (_i, [_vp, _vp, _vp, _i64]),
    "bhs_spgemm_numeric": (_i, [_vp, _i, _i]),
    "bhs_spgemm_finish": (_i, [_vp, C.POINTER(C.c_double)]),
    "bhs_get_stream": (_i, [_vp, C.POINTER(_vp)]),
    "bhs_get_nnzC": (_i, [_vp, C.POINTER(_i)]),
    "bhs_get_C": (_i, [_vp, _vp, _vp]),
    "bhs_get_rowptrC": (_i, [_vp, _vp]),
    "bhs_get_C_device": (_i, [_vp, C.POINTER(_vp), C.POINTER(_vp), C.POINTER(_vp)]),
    "bhs_csr_sort_indices_device": (_i, [_vp, _i, _vp, _vp, _vp]),
    "bhs_get_kernel_stats": (_i, [_vp, C.POINTER(KernelStat), _i]),
    "bhs_set_option": (_i, [_vp, C.c_char_p, _i64]),
    "bhs_get_info": (_i, [_vp, C.c_char_p, C.POINTER(_i64)]),
    "bhs_get_class_tables_device": (_i, [_vp, C.POINTER(_vp), C.POINTER(_vp), C.POINTER(_vp), C.POINTER(_i), C.POINTER(_i), C.POINTER(_i)]),
    "bhs_expand_class_columns_device": (_i, [_vp, _i, _i, _vp, _vp, _vp, _i, _vp, _vp]),
    "bhs_spgemm_masked_device": (_i, [_vp, _vp, _vp, _i, _vp, C.POINTER(_i64), C.POINTER(C.c_double)]),
    "bhs_spgemm_masked": (_i, [_vp, _vp, _vp, _i, _vp, C.POINTER(_i64), C.POINTER(C.c_double)]),
    "bhs_csr_add_symbolic_device": (_i, [_vp, _i, _i, _i, _vp, _vp, _i, _vp, _vp, _vp, C.POINTER(_i), C.POINTER(_i)]),
    "bhs_csr_add_numeric_device": (_i, [_vp, _i, _i, C.c_double, _i, _vp, _vp, _vp, C.c_double, _i, _vp, _vp, _vp, _vp, _vp, _vp,
                                        C.POINTER(C.c_double)]),
    "bhs_spgemm_add_device": (_i, [_vp, C.c_double, C.c_double, _i, _vp, _vp, _vp, _vp, C.POINTER(_i64), C.POINTER(_i),
                                   C.POINTER(C.c_double)]),
    "bhs_spgemm_add": (_i, [_vp, C.c_double, C.c_double, _i, _vp, _vp, _vp, _vp, C.POINTER(_i64), C.POINTER(_i),
                            C.POINTER(C.c_double)]),
    "bhs_csr_select_symbolic_device": (_i, [_vp, _i, _i, _i, _vp, _vp, _vp, C.POINTER(Select), _vp, C.POINTER(_i)]),
    "bhs_csr_select_numeric_device": (_i, [_vp, _i, _i, _i, _vp, _vp, _vp, C.POINTER(Select), _vp, _vp, _vp, C.POINTER(C.c_double)]),
    "bhs_spgemm_select_device": (_i, [_vp, C.POINTER(Select), _vp, C.POINTER(_i64), C.POINTER(_i), C.POINTER(C.c_double)]),
    "bhs_spgemm_select": (_i, [_vp, C.POINTER(Select), _vp, C.POINTER(_i64), C.POINTER(_i), C.POINTER(C.c_double)]),
    "bhs_csr_transpose_device": (_i, [_vp, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, C.POINTER(C.c_double)]),
    "bhs_csr_transpose_values_device": (_i, [_vp, _i, _vp, _vp, _vp, C.POINTER(C.c_double)]),
    "bhs_spgemm_semiring_masked_device": (_i, [_vp, _i, _vp, _vp, _i, _vp, C.POINTER(_i64), C.POINTER(C.c_double)]),
    "bhs_spgemm_semiring_masked": (_i, [_vp, _i, _vp, _vp, _i, _vp, C.POINTER(_i64), C.POINTER(C.c_double)]),
    "bhs_spgemm_semiring": (_i, [_vp, _i, _vp, C.POINTER(_i64), C.POINTER(_i), C.POINTER(C.c_double)]),
    "bhs_csr_extract_symbolic_device": (_i, [_vp, _i, _i, _i, _vp, _vp, _i, _vp, _i, _vp, _vp, C.POINTER(_i)]),
    "bhs_csr_extract_numeric_device": (_i, [_vp, _i, _i, _i, _vp, _vp, _vp, _i, _vp, _i, _vp, _i, _vp, _vp, _vp, _vp,
                                            C.POINTER(C.c_double)]),
    "bhs_csr_reduce_device": (_i, [_vp, _i, _i, _i, _vp, _vp, _vp, _i, _i, _i, _vp, C.POINTER(C.c_double)]),
    "bhs_csr_scale_device": (_i, [_vp, _i, _i, _i, _vp, _vp, _vp, C.c_double, _vp, _vp, _i, _vp, C.POINTER(C.c_double)]),
    "bhs_csr_spmv_device": (_i, [_vp, _i, _i, _i, _vp, _vp, _vp, C.c_double, _vp, C.c_double, _vp, C.POINTER(C.c_double)]),
    "bhs_csr_spmm_device": (_i, [_vp, _i, _i, _i, _vp, _vp, _vp, _i, C.c_double, _vp, C.c_longlong, C.c_double, _vp, C.c_longlong,
                                 C.POINTER(C.c_double)]),
    "bhs_csr_sddmm_device": (_i, [_vp, _i, _i, _i, _vp, _vp, _vp, _i, C.c_double, _vp, C.c_longlong, _vp, C.c_longlong, C.c_double,
                                  _vp, C.c_uint, C.POINTER(C.c_double)]),
    "bhs_csr_fsai_device": (_i, [_vp, _i, _i, _vp, _vp, _vp, _i, _vp, _vp, _vp, _i, C.POINTER(_i), C.POINTER(C.c_double)]),
    "bhs_csr_spmv_semiring_device": (_i, [_vp, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _i, _vp, _vp, C.POINTER(C.c_longlong),
                                          C.POINTER(C.c_double)]),
    "bhs_csr_spmm_semiring_device": (_i, [_vp, _i, _i, _i, _i, _vp, _vp, _vp, _i, _vp, C.c_longlong, _i, _vp, C.c_longlong, _vp,
                                          C.c_longlong, C.POINTER(C.c_longlong), C.POINTER(C.c_double)]),
    "bhs_csr_push_semiring_device": (_i, [_vp, _i, _i, _i, _i, _vp, _vp, _vp, _i, _vp, _i, _vp, C.c_longlong, _i, _vp, C.c_longlong,
                                          _vp, C.c_longlong, _vp, C.POINTER(_i), C.POINTER(C.c_longlong), C.POINTER(C.c_double)]),
    "bhs_csr_aggregate_device": (_i, [_vp, _i, _i, _vp, _vp, _vp, C.c_uint, _i, _vp, _vp, C.POINTER(_i), C.POINTER(_i),
                                      C.POINTER(C.c_double)]),
    "bhs_csr_color_device": (_i, [_vp, _i, _i, _vp, _vp, _vp, C.c_uint, _i, _vp, _vp, _vp, C.POINTER(_i), C.POINTER(_i),
                                  C.POINTER(C.c_double)]),
    "bhs_csr_gs_device": (_i, [_vp, _i, _i, _vp, _vp, _vp, _vp, _i, _vp, _vp, _vp, _vp, _vp, C.c_double, _i, _i,
                               C.POINTER(C.c_double)]),
    "bhs_csr_levels_device": (_i, [_vp, _i, _i, _vp, _vp, _i, _vp, _vp, _vp, C.POINTER(_i), C.POINTER(_i), C.POINTER(C.c_double)]),
    "bhs_csr_trsv_device": (_i, [_vp, _i, _i, _vp, _vp, _vp, _i, _vp, _vp, C.c_double, _vp, _vp, _i, C.POINTER(C.c_double)]),
    "bhs_csr_ilu0_device": (_i, [_vp, _i, _i, _vp, _vp, _vp, _i, _vp, _vp, _i, C.POINTER(_i), C.POINTER(C.c_double)]),
    "bhs_csr_components_device": (_i, [_vp, _i, _i, _vp, _vp, _i, _vp, _vp, _vp, C.POINTER(_i), C.POINTER(_i), C.POINTER(C.c_double)]),
    "bhs_csr_scc_device": (_i, [_vp, _i, _i, _vp, _vp, _i, _vp, _vp, _vp, C.POINTER(_i), C.POINTER(_i), C.POINTER(_i),
                                C.POINTER(C.c_double)]),
    "bhs_csr_rcm_device": (_i, [_vp, _i, _i, _vp, _vp, _i, _vp, _vp, _vp, C.POINTER(_i), C.POINTER(_i), C.POINTER(_i), C.POINTER(_i),
                                C.POINTER(C.c_double)]),
    "bhs_csr_kcore_device": (_i, [_vp, _i, _i, _vp, _vp, _i, _vp, _vp, C.POINTER(_i), C.POINTER(_i), C.POINTER(C.c_double)]),
    "bhs_csr_sssp_device": (_i, [_vp, _i, _i, _vp, _vp, _vp, _i, _vp, C.c_double, _i, _vp, _vp, C.POINTER(_i), C.POINTER(_i),
                                 C.POINTER(C.c_double)]),
    "bhs_csr_betweenness_device": (_i, [_vp, _i, _i, _vp, _vp, _i, _vp, _vp, _i, _vp, _i, _vp, _vp, _vp, C.POINTER(_i), C.POINTER(_i),
                                        C.POINTER(C.c_double)]),
    "bhs_csr_match_device": (_i, [_vp, _i, _i, _vp, _vp, _vp, C.c_uint, _i, _vp, _vp, C.POINTER(_i), C.POINTER(_i),
                                  C.POINTER(C.c_double)]),
    "bhs_csr_spanning_forest_device": (_i, [_vp, _i, _i, _vp, _vp, _vp, _i, _vp, _vp, _vp, _vp, C.POINTER(_i), C.POINTER(_i),
                                            C.POINTER(C.c_double)]),
    "bhs_csr_cfsplit_device": (_i, [_vp, _i, _i, _vp, _vp, _vp, C.c_uint, _i, _vp, _vp, C.POINTER(_i), C.POINTER(_i),
                                    C.POINTER(C.c_double)]),
    "bhs_csr_interp_symbolic_device": (_i, [_vp, _i, _i, _vp, _vp, _i, _vp, _vp, _vp, _i, _vp, C.POINTER(C.c_longlong),
                                            C.POINTER(C.c_double)]),
    "bhs_csr_interp_numeric_device": (_i, [_vp, _i, _i, _vp, _vp, _vp, _i, _vp, _vp, _vp, _i, _vp, C.c_longlong, _vp, _vp, _i,
                                           C.POINTER(C.c_double)]),
    "bhs_coo_assemble_device": (_i, [_vp, _i, _i, _i, _vp, _vp, _vp, _i, _vp, _vp, _vp, _vp, _vp, C.POINTER(_i), C.POINTER(_i),
                                     C.POINTER(C.c_double)]),
    "bhs_coo_assemble_values_device": (_i, [_vp, _i, _vp, _i, _vp, _vp, _i, _vp, C.POINTER(C.c_double)]),
    "bhs_csr_relax_device": (_i, [_vp, _i, _i, _vp, _vp, _vp, _vp, _i, C.POINTER(C.c_double), _vp, _vp, _vp, C.c_uint,
                                  C.POINTER(C.c_double)]),
    "bhs_chebyshev_coefficients": (_i, [C.c_double, C.c_double, _i, C.POINTER(C.c_double)]),
    "bhs_csr_spmv_dots_device": (_i, [_vp, _i, _i, _i, _vp, _vp, _vp, C.c_double, _vp, C.c_double, _vp, _vp, _vp,
                                      C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    "bhs_strerror": (C.c_char_p, [_i]),
    "bhs_version": (C.c_char_p, []),
}

# value_type float build of the same sources (-DBHS_VALUE_FLOAT; README.md:84-86 of the reference)
SO_PATH_F32 = os.path.join(CSRC, "libbhsparse_hip_f32.so")
_lib = None
_libs = {}


# the device sources, by base name: the translation unit, then every header of csrc/, so that a new header is a staleness
# input of build() and part of source_digest() without being listed here (the Makefile's HDRS names the same files)
SOURCES = ("bhsparse_hip.hip",) + tuple(sorted(f for f in os.listdir(CSRC) if f.endswith((".hip.h", ".inc.h"))))


def source_digest():
    """Short hash of the device sources: keys measurements (profiles/hbm_traffic.json) to the build they came from."""
    import hashlib
    hsh = hashlib.sha256()
    for f in SOURCES:
        path = os.path.join(CSRC, f)
        if os.path.exists(path):
            hsh.update(f.encode())
            hsh.update(open(path, "rb").read())
    return hsh.hexdigest()[:16]


def build(force=False):
    """Compile libbhsparse_hip.so and libbhsparse_hip_f32.so for gfx950 with hipcc (cross-compiles without a GPU)."""
    srcs = [os.path.join(CSRC, f) for f in SOURCES if os.path.exists(os.path.join(CSRC, f))] + [HEADER]
    outs = [os.path.join(CSRC, "libbhsparse_hip.so"), SO_PATH_F32]
    stale = any(not os.path.exists(o) or any(os.path.getmtime(s) > os.path.getmtime(o) for s in srcs) for o in outs)
    if force or stale:
        subprocess.check_call(["make", "-C", CSRC, "-s", "-j2"] + (["-B"] if force else []))
    return SO_PATH


def load(f32=False):
    """The double library (default) or the float one.  Raises if it is not built: no fallback."""
    global _lib
    path = SO_PATH_F32 if f32 else SO_PATH
    if path not in _libs:
        if not os.path.exists(path):
            raise ImportError(
                "%s is not built (%s). Run `python -c 'import __graft_entry__ as g; "
                "g.build()'` or `make -C %s`. There is no CPU fallback." % (os.path.basename(path), path, CSRC))
        # PyTorch-ROCm wheels bundle their own libamdhip64 / libhsa-runtime64, and two HSA runtimes in one
        # process cannot both own the GPU (the one initialised second reports no device).  When torch is
        # installed, let it load its runtime first: this library then binds to the same copy by soname.
        if "torch" not in sys.modules:
            try:
                import torch  # noqa: F401
            except ImportError:
                pass
        L = C.CDLL(path)
        for name, (res, args) in SYMBOLS.items():
            f = getattr(L, name)      # AttributeError if the library does not export it
            f.restype = res
            f.argtypes = args
        _libs[path] = L
    if not f32:
        _lib = _libs[path]
    return _libs[path]


def strerror(code):
    return load().bhs_strerror(int(code)).decode()
