"""CPU tests of the interfaces of the reductions and the diagonal scaling (bhs_csr_reduce_device, bhs_csr_scale_device): both
libraries export the entry points the header declares, the build tracks the new sources, the Python facades carry them, the
C++ facade's extension methods compile and link against the C-ABI library (tests/reduce; tests/test_reduce_gpu.py runs the
same binary on a GPU), and the numpy restatement (tests/reduceref.py) agrees with a case written out by hand and with scipy."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

from conftest import ROOT
import reduceref as rr

from benchmark_spgemm_using_csr_amd import _lib

ENTRY = ("bhs_csr_reduce_device", "bhs_csr_scale_device")
FAMILIES = ("reduce_short", "reduce_wave", "reduce_long", "reduce_cols", "reduce_all", "reduce_finish", "scale_short",
            "scale_wave", "scale_long")
CONSTANTS = {"BHS_AXIS_ROWS": 0, "BHS_AXIS_COLS": 1, "BHS_AXIS_ALL": 2, "BHS_AXIS_DIAG": 3, "BHS_RED_PLUS": 0, "BHS_RED_MIN": 1,
             "BHS_RED_MAX": 2, "BHS_RED_ABS_PLUS": 3, "BHS_RED_ABS_MAX": 4, "BHS_RED_SQ_PLUS": 5, "BHS_RED_COUNT": 6,
             "BHS_RED_OFFDIAG": 1, "BHS_SCALE_LEFT_DIV": 1, "BHS_SCALE_RIGHT_DIV": 2}
DEMO_DIR = os.path.join(ROOT, "tests", "reduce")


def test_header_declares_the_entry_points_and_constants():
    txt = open(_lib.HEADER).read()
    decl = set(re.findall(r"BHS_API\s+[\w\s\*]+?\b(bhs_\w+)\s*\(", txt))
    for name in ENTRY:
        assert name in decl
        assert name in _lib.SYMBOLS
    assert len(_lib.SYMBOLS["bhs_csr_reduce_device"][1]) == 12
    assert len(_lib.SYMBOLS["bhs_csr_scale_device"][1]) == 13
    assert _lib.SYMBOLS["bhs_csr_scale_device"][1][7] is C.c_double
    assert "---- reduce / scale" in txt
    for fam in FAMILIES:
        assert fam in txt, fam
    for name, value in CONSTANTS.items():
        assert re.search(r"\b%s\s*=\s*%d\b" % (name, value), txt), name
        assert getattr(_lib, name) == value, name
        assert getattr(rr, name.replace("BHS_AXIS_", "").replace("BHS_RED_", "").replace("BHS_SCALE_", "")) == value, name
    for words in ("bit-for-bit functions of the input on every axis", "may differ from run to run", "partly written"):
        assert words in txt, words


def test_both_libraries_export_the_entry_points(hiplib):
    for path in (_lib.SO_PATH, _lib.SO_PATH_F32):
        raw = C.CDLL(path)
        for name in ENTRY:
            assert getattr(raw, name) is not None
        blob = open(path, "rb").read()
        for kern in (b"k_red_short", b"k_red_wave", b"k_red_long", b"k_red_rowlen", b"k_red_cols", b"k_red_all", b"k_red_finish",
                     b"k_sc_check", b"k_sc_flat", b"k_sc_short", b"k_sc_wave", b"k_sc_long"):
            assert kern in blob, (path, kern)


def test_sources_are_tracked_by_the_build():
    assert "bhs_reduce.hip.h" in _lib.SOURCES and "bhs_host_reduce.inc.h" in _lib.SOURCES
    mk = open(os.path.join(_lib.CSRC, "Makefile")).read()
    assert "bhs_reduce.hip.h" in mk and "bhs_host_reduce.inc.h" in mk
    unit = open(os.path.join(_lib.CSRC, "bhsparse_hip.hip")).read()
    incs = re.findall(r'#include "(bhs_host_\w+\.inc\.h)"', unit)
    at = incs.index("bhs_host_reduce.inc.h")
    assert incs[at - 1] == "bhs_host_transpose.inc.h" and incs[at + 1] == "bhs_host_semiring.inc.h"
    host = open(os.path.join(_lib.CSRC, "bhs_host_reduce.inc.h")).read()
    assert '#include "bhs_reduce.hip.h"' in host                    # (the kernels' header comes with the host part)


def test_null_handle_is_rejected(hiplib):
    inv = _lib.BHS_ERR_INVALID_ARG
    assert hiplib.bhs_csr_reduce_device(None, 0, 0, 0, None, None, None, 0, 0, 0, None, None) == inv
    assert hiplib.bhs_csr_scale_device(None, 0, 0, 0, None, None, None, 1.0, None, None, 0, None, None) == inv


def test_python_facade_has_the_calls():
    from benchmark_spgemm_using_csr_amd import facade
    for name in ("csr_reduce_raw_device", "csr_scale_raw_device", "csr_reduce_device", "csr_scale_device"):
        assert callable(getattr(facade.bhsparse, name, None)), name
    for name in ("reduce_csr", "scale_csr", "diagonal_csr", "normalize_csr", "smoothed_prolongator_csr"):
        assert callable(getattr(facade, name, None)), name
    bh = facade.bhsparse()
    assert bh.reduce_ms == 0.0 and bh.scale_ms == 0.0
    # without a platform the raw calls answer, they do not crash
    assert bh.csr_reduce_raw_device(0, 0, 0, None, None, None, 0, 0, 0, None) == _lib.BHS_ERR_NOT_READY
    assert bh.csr_scale_raw_device(0, 0, 0, None, None, None, 1.0, None, None, 0, None) == _lib.BHS_ERR_NOT_READY


def test_cpp_facade_extension_builds(hiplib):
    src = open(os.path.join(ROOT, "benchmark_spgemm_using_csr_amd", "host", "bhsparse.h")).read()
    flat = re.sub(r"\s+", " ", src)
    assert ("int csr_reduce_device(int m, int n, int nnzX, const value_type *d_valX, const index_type *d_rowPtrX, "
            "const index_type *d_colIndX, int axis, int op, int flags, value_type *d_out);") in flat
    assert ("int csr_scale_device(int m, int n, int nnzX, const value_type *d_valX, const index_type *d_rowPtrX, "
            "const index_type *d_colIndX, double alpha, const value_type *d_left, const value_type *d_right, int flags, "
            "value_type *d_valZ);") in flat
    subprocess.check_call(["make", "-C", DEMO_DIR, "-s"])
    demo = os.path.join(DEMO_DIR, "reduce_demo")
    assert os.access(demo, os.X_OK)
    out = subprocess.run(["nm", "-D", "--undefined-only", demo], capture_output=True, text=True).stdout
    for name in ENTRY:
        assert name in out


# ---------------------------------------------------------------- the reference against a case written out by hand
# 5 x 7.  row 0 not ascending, with the diagonal pair (0, 0) twice; row 1 empty; row 2 holds -0 and +0 (the latter on the
# diagonal); row 3 a NaN and the pair (3, 3) twice.
NAN = np.nan
XP = np.array([0, 4, 4, 7, 10, 12], np.int32)
XJ = np.array([5, 2, 0, 0, 1, 2, 6, 0, 3, 3, 6, 4], np.int32)
XX = np.array([1, 2, 3, 4, -0.0, 0.0, 5, NAN, 6, -7, 8, -9], np.float64)
INF = np.inf


def same(got, want):
    want = np.asarray(want, got.dtype)
    return (got.shape == want.shape and np.array_equal(np.isnan(got), np.isnan(want)) and
            np.array_equal(got[~np.isnan(got)].view(np.uint64 if got.dtype == np.float64 else np.uint32),
                           want[~np.isnan(want)].view(np.uint64 if got.dtype == np.float64 else np.uint32)))


def test_reduceref_by_hand():
    red = lambda axis, op, flags=0, vals=XX, dt=np.float64: rr.reduce(5, 7, XP, XJ, vals, axis, op, flags, dt)   # noqa: E731
    out, S, K = red(rr.ROWS, rr.PLUS)
    assert out.dtype == np.float64 and same(out, [10, 0, 5, NAN, -1])
    assert K.tolist() == [4, 0, 3, 3, 2] and S[0] == 10 and S[4] == 17 and S[1] == 0
    assert same(red(rr.ROWS, rr.MIN)[0], [1, INF, -0.0, NAN, -9]) and red(rr.ROWS, rr.MIN)[1] is None
    assert same(red(rr.ROWS, rr.MAX)[0], [4, -INF, 5, NAN, 8])
    assert same(red(rr.ROWS, rr.ABS_PLUS)[0], [10, 0, 5, NAN, 17])
    assert same(red(rr.ROWS, rr.ABS_MAX)[0], [4, 0, 5, NAN, 9])
    assert same(red(rr.ROWS, rr.SQ_PLUS)[0], [30, 0, 25, NAN, 145])
    assert same(red(rr.ROWS, rr.COUNT)[0], [4, 0, 3, 3, 2])         # (COUNT never looks at the NaN)
    assert same(red(rr.ROWS, rr.PLUS, rr.OFFDIAG)[0], [3, 0, 5, NAN, 8])
    assert same(red(rr.ROWS, rr.COUNT, rr.OFFDIAG)[0], [2, 0, 2, 1, 1])
    assert same(red(rr.COLS, rr.PLUS)[0], [NAN, 0.0, 2, -1, -9, 1, 13])     # (column 1 holds -0 alone: a zero sum is +0)
    assert same(red(rr.COLS, rr.MIN)[0], [NAN, -0.0, 0.0, -7, -9, 1, 5])
    assert same(red(rr.COLS, rr.MAX)[0], [NAN, -0.0, 2, 6, -9, 1, 8])
    assert same(red(rr.COLS, rr.ABS_MAX)[0], [NAN, 0.0, 2, 7, 9, 1, 8])
    assert same(red(rr.COLS, rr.COUNT)[0], [3, 1, 2, 2, 1, 1, 2])
    assert same(red(rr.COLS, rr.MAX, rr.OFFDIAG)[0], [NAN, -0.0, 2, -INF, -INF, 1, 8])
    assert same(red(rr.ALL, rr.PLUS)[0], [NAN]) and same(red(rr.ALL, rr.COUNT)[0], [12]) and same(red(rr.ALL, rr.ABS_MAX)[0], [NAN])
    assert same(red(rr.ALL, rr.COUNT, rr.OFFDIAG)[0], [6])
    assert same(red(rr.DIAG, rr.PLUS)[0], [7, 0, 0.0, -1, -9])      # (duplicate pairs reduce together)
    assert same(red(rr.DIAG, rr.MIN)[0], [3, INF, 0.0, -7, -9])
    assert same(red(rr.DIAG, rr.COUNT)[0], [2, 0, 1, 2, 1])
    # without values every entry counts as 1; the float build rounds once
    assert same(red(rr.ROWS, rr.PLUS, vals=None)[0], [4, 0, 3, 3, 2]) and same(red(rr.COLS, rr.MAX, vals=None)[0], [1] * 7)
    out = red(rr.ROWS, rr.SQ_PLUS, vals=XX * 0.1, dt=np.float32)[0]
    x32 = (XX * 0.1).astype(np.float32).astype(np.float64)
    assert out.dtype == np.float32 and out[4] == np.float32(x32[10] ** 2 + x32[11] ** 2)
    # rectangular the other way: the diagonal has min(m, n) values
    assert len(rr.reduce(7, 5, np.array([0, 1, 1, 1, 1, 1, 1, 1]), [0], [2.0], rr.DIAG, rr.PLUS)[0]) == 5
    # empty shapes: ALL still gives the identity
    for op, ident in ((rr.PLUS, 0.0), (rr.MIN, INF), (rr.MAX, -INF), (rr.ABS_MAX, 0.0), (rr.COUNT, 0.0)):
        assert same(rr.reduce(0, 0, [0], [], [], rr.ALL, op)[0], [ident])


def test_scaleref_by_hand():
    left, right = [2, 3, 4, 0.5, -1], [1, 2, 3, 4, 5, 6, 7]
    z = rr.scale(5, 7, XP, XJ, XX, -2.0, left, None, rr.LEFT_DIV)
    assert same(z, [-1, -2, -3, -4, 0.0, -0.0, -2.5, NAN, -24, 28, 16, -18])
    z = rr.scale(5, 7, XP, XJ, XX, 1.0, left, right)
    assert same(z, [12, 12, 6, 8, -0.0, 0.0, 140, NAN, 12, -14, -56, 45])
    z = rr.scale(5, 7, XP, XJ, XX, 0.5, None, right, rr.RIGHT_DIV)
    assert same(z[:4], [0.5 / 6, 1.0 / 3, 1.5, 2.0])
    with np.errstate(all="ignore"):
        z = rr.scale(5, 7, XP, XJ, XX, 1.0, [0, 1, 0, 1, 1], None, rr.LEFT_DIV, np.float32)   # division by zero follows IEEE
    assert z.dtype == np.float32 and np.all(np.isposinf(z[:4])) and np.isnan(z[4]) and np.isnan(z[5]) and z[6] == INF


def test_reduceref_names_what_must_be_refused():
    assert rr.invalid(5, 7, XP, XJ, rr.COLS, rr.PLUS, rr.OFFDIAG) is None
    assert rr.invalid(5, 7, XP, XJ, 4, rr.PLUS) == "unknown axis"
    assert rr.invalid(5, 7, XP, XJ, rr.ROWS, 7) == "unknown op"
    assert rr.invalid(5, 7, XP, XJ, rr.ROWS, rr.PLUS, 2) == "unknown flag"
    assert rr.invalid(5, 7, XP, XJ, rr.DIAG, rr.PLUS, rr.OFFDIAG) == "OFFDIAG with DIAG"
    p = XP.copy(); p[0] = 1
    assert rr.invalid(5, 7, p, XJ, rr.ROWS, rr.PLUS) == "rowPtrX[0] != 0"
    p = XP.copy(); p[-1] = 11
    assert rr.invalid(5, 7, p, XJ, rr.ALL, rr.PLUS) == "rowPtrX[m] != nnzX"
    p = XP.copy(); p[2] = 3
    assert rr.invalid(5, 7, p, XJ, rr.ROWS, rr.COUNT) == "decreasing rowPtrX"
    j = XJ.copy(); j[11] = 7
    for axis, flags, want in ((rr.ROWS, 0, None), (rr.ALL, 0, None), (rr.ROWS, rr.OFFDIAG, "column of X out of range"),
                              (rr.COLS, 0, "column of X out of range"), (rr.DIAG, 0, "column of X out of range")):
        assert rr.invalid(5, 7, XP, j, axis, rr.PLUS, flags) == want
    # 3 x 2: row 2 is not below min(m, n), the diagonal never reads it
    assert rr.invalid(3, 2, [0, 1, 2, 3], [0, 1, 5], rr.DIAG, rr.PLUS) is None
    assert rr.invalid(3, 2, [0, 1, 2, 3], [0, 1, 5], rr.COLS, rr.PLUS) == "column of X out of range"
    assert rr.invalid_scale(5, 7, XP, j, True, False) is None and rr.invalid_scale(5, 7, XP, j, True, True) == "column of X out of range"
    assert rr.invalid_scale(5, 7, XP, XJ, False, True, rr.LEFT_DIV) == "DIV without its vector"
    assert rr.invalid_scale(5, 7, XP, XJ, True, True, 4) == "unknown flag"
    p = XP.copy(); p[2] = 3
    assert rr.invalid_scale(5, 7, p, XJ, False, False) == "decreasing rowPtrX"


def test_reduceref_against_scipy():
    import scipy.sparse as sp
    for seed in range(12):
        rng = np.random.default_rng(500 + seed)
        m, n = int(rng.integers(1, 60)), int(rng.integers(1, 60))
        S = sp.random(m, n, density=float(rng.choice([0.05, 0.3])), format="csr", random_state=np.random.RandomState(seed))
        S.data = rng.integers(-9, 10, S.nnz).astype(np.float64)     # small integers (explicit zeros among them): every sum is exact
        S.sort_indices()
        Xp, Xj, Xx = S.indptr.astype(np.int32), S.indices.astype(np.int32), S.data.copy()
        for i in range(m):                                          # the rows in a random order: the result may not depend on it
            o = rng.permutation(Xp[i + 1] - Xp[i]) + Xp[i]
            Xj[Xp[i]:Xp[i + 1]], Xx[Xp[i]:Xp[i + 1]] = Xj[o], Xx[o]
        red = lambda axis, op, flags=0: rr.reduce(m, n, Xp, Xj, Xx, axis, op, flags)[0]   # noqa: E731
        assert np.array_equal(red(rr.ROWS, rr.PLUS), np.asarray(S.sum(axis=1)).ravel()), seed
        assert np.array_equal(red(rr.COLS, rr.PLUS), np.asarray(S.sum(axis=0)).ravel()), seed
        assert red(rr.ALL, rr.PLUS)[0] == S.sum()
        assert np.array_equal(red(rr.DIAG, rr.PLUS), S.diagonal()), seed
        assert np.array_equal(red(rr.ROWS, rr.COUNT), S.getnnz(axis=1)) and np.array_equal(red(rr.COLS, rr.COUNT), S.getnnz(axis=0))
        assert red(rr.ALL, rr.COUNT)[0] == S.nnz
        off = S - sp.diags(S.diagonal(), shape=(m, n), format="csr") if m == n else None
        if off is not None:
            assert np.array_equal(red(rr.ROWS, rr.PLUS, rr.OFFDIAG), np.asarray(off.sum(axis=1)).ravel()), seed
        # max and min of the STORED entries (scipy's own max / min count the implicit zeros): row by row
        for axis, M in ((rr.ROWS, S), (rr.COLS, S.tocsc())):
            want_max = np.array([M.data[M.indptr[i]:M.indptr[i + 1]].max(initial=-np.inf) for i in range(len(M.indptr) - 1)])
            want_min = np.array([M.data[M.indptr[i]:M.indptr[i + 1]].min(initial=np.inf) for i in range(len(M.indptr) - 1)])
            assert np.array_equal(red(axis, rr.MAX), want_max) and np.array_equal(red(axis, rr.MIN), want_min), seed
        assert np.array_equal(red(rr.ROWS, rr.ABS_MAX), np.asarray(abs(S).max(axis=1).todense()).ravel()), seed
        assert np.array_equal(red(rr.ROWS, rr.SQ_PLUS), np.asarray(S.multiply(S).sum(axis=1)).ravel()), seed
        # the scale: diags(l) @ S @ diags(r) on S's pattern
        l, r = rng.integers(1, 5, m).astype(np.float64), rng.integers(1, 5, n).astype(np.float64)
        Z = (sp.diags(l) @ S @ sp.diags(r)).tocsr()
        got = sp.csr_matrix((rr.scale(m, n, Xp, Xj, Xx, 1.0, l, r), Xj, Xp), shape=(m, n))
        assert abs(Z - got).sum() == 0
        Zd = rr.scale(m, n, Xp, Xj, Xx, 3.0, l, None, rr.LEFT_DIV)
        assert np.array_equal(Zd, Xx / l[np.repeat(np.arange(m), np.diff(Xp))] * 3.0)
