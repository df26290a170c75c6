"""CPU tests of the interfaces of CSR x dense (bhs_csr_spmv_device, bhs_csr_spmm_device): both libraries export the entry
points the header declares, the build tracks the new sources, benchmark_spgemm_using_csr_amd/dense.py carries the calls,
the C++ facade's extension methods compile and link against the C-ABI library (tests/spmv; tests/test_spmv_gpu.py runs the
same binary on a GPU), and the numpy restatement (tests/spmvref.py) agrees with a case written out by hand and with scipy."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np

from conftest import ROOT
import spmvref as sr

from benchmark_spgemm_using_csr_amd import _lib

ENTRY = ("bhs_csr_spmv_device", "bhs_csr_spmm_device")
FAMILIES = ("spmv_short", "spmv_wave", "spmv_long", "spmm_short", "spmm_wave", "spmm_long")
DEMO_DIR = os.path.join(ROOT, "tests", "spmv")


def test_header_declares_the_entry_points():
    txt = open(_lib.HEADER).read()
    decl = set(re.findall(r"BHS_API\s+[\w\s\*]+?\b(bhs_\w+)\s*\(", txt))
    for name in ENTRY:
        assert name in decl
        assert name in _lib.SYMBOLS
    spmv, spmm = _lib.SYMBOLS["bhs_csr_spmv_device"][1], _lib.SYMBOLS["bhs_csr_spmm_device"][1]
    assert len(spmv) == 12 and spmv[7] is C.c_double and spmv[9] is C.c_double
    assert len(spmm) == 15 and spmm[7] is C.c_int and spmm[8] is C.c_double and spmm[11] is C.c_double
    assert spmm[10] is C.c_longlong and spmm[13] is C.c_longlong     # ldX, ldY: long long
    assert "---- CSR x dense" in txt
    for fam in FAMILIES:
        assert fam in txt, fam
    for words in ("beta == 0 never reads d_y", "alpha == 0 takes no shortcut", "arrays give the same bits",
                  "partly written", "Nothing is ever written outside the m x k elements of Y"):
        assert words in txt, words
    # the families' names are what the host part books its launches under
    host = open(os.path.join(_lib.CSRC, "bhs_host_spmv.inc.h")).read()
    for fam in FAMILIES:
        assert '"%s"' % fam in host, fam


def test_both_libraries_export_the_entry_points(hiplib):
    for path in (_lib.SO_PATH, _lib.SO_PATH_F32):
        raw = C.CDLL(path)
        for name in ENTRY:
            assert getattr(raw, name) is not None
        blob = open(path, "rb").read()
        for kern in (b"k_mv_short", b"k_mv_wave", b"k_mv_long"):
            assert kern in blob, (path, kern)


def test_sources_are_tracked_by_the_build():
    assert "bhs_spmv.hip.h" in _lib.SOURCES and "bhs_host_spmv.inc.h" in _lib.SOURCES
    mk = open(os.path.join(_lib.CSRC, "Makefile")).read()
    assert "bhs_spmv.hip.h" in mk and "bhs_host_spmv.inc.h" in mk
    unit = open(os.path.join(_lib.CSRC, "bhsparse_hip.hip")).read()
    incs = re.findall(r'#include "(bhs_host_\w+\.inc\.h)"', unit)
    assert incs.index("bhs_host_spmv.inc.h") > incs.index("bhs_host_side.inc.h")     # (it runs on the side operations' plumbing)
    assert incs[-4:] == ["bhs_host_transpose.inc.h", "bhs_host_reduce.inc.h", "bhs_host_semiring.inc.h", "bhs_host_extract.inc.h"]
    assert "SideWs mvWs;" in unit
    assert "release(h->mvWs)" in open(os.path.join(_lib.CSRC, "bhs_host_cabi.inc.h")).read()
    host = open(os.path.join(_lib.CSRC, "bhs_host_spmv.inc.h")).read()
    assert '#include "bhs_spmv.hip.h"' in host                      # (the kernels' header comes with the host part)
    kernels = open(os.path.join(_lib.CSRC, "bhs_spmv.hip.h")).read()
    assert "asm" not in kernels and "atomic" not in kernels.replace("no atomics", "")


def test_null_handle_is_rejected(hiplib):
    inv = _lib.BHS_ERR_INVALID_ARG
    assert hiplib.bhs_csr_spmv_device(None, 0, 0, 0, None, None, None, 1.0, None, 0.0, None, None) == inv
    assert hiplib.bhs_csr_spmm_device(None, 0, 0, 0, None, None, None, 1, 1.0, None, 1, 0.0, None, 1, None) == inv


def test_dense_module_has_the_calls():
    from benchmark_spgemm_using_csr_amd import dense, facade
    for name in ("csr_spmv_raw_device", "csr_spmm_raw_device", "csr_spmv_device", "csr_spmm_device", "spmv_csr", "spmm_csr",
                 "residual_csr"):
        assert callable(getattr(dense, name, None)), name
        assert not hasattr(facade.bhsparse, name), name             # functions of a handle, not methods of it
    assert list(inspect.signature(dense.csr_spmv_device).parameters) == ["bh", "m", "n", "A", "x", "alpha", "beta", "y"]
    assert list(inspect.signature(dense.csr_spmm_device).parameters) == ["bh", "m", "n", "A", "X", "alpha", "beta", "Y"]
    assert list(inspect.signature(dense.spmv_csr).parameters) == ["m", "n", "Ap", "Aj", "Ax", "x", "alpha", "beta", "y",
                                                                  "value_dtype", "device"]
    bh = facade.bhsparse()
    assert bh.spmv_ms == 0.0
    # without a platform the raw calls answer, they do not crash
    assert dense.csr_spmv_raw_device(bh, 0, 0, 0, None, None, None, 1.0, None, 0.0, None) == _lib.BHS_ERR_NOT_READY
    assert dense.csr_spmm_raw_device(bh, 0, 0, 0, None, None, None, 1, 1.0, None, 1, 0.0, None, 1) == _lib.BHS_ERR_NOT_READY


def test_cpp_facade_extension_builds(hiplib):
    src = open(os.path.join(ROOT, "benchmark_spgemm_using_csr_amd", "host", "bhsparse.h")).read()
    flat = re.sub(r"\s+", " ", src)
    assert ("int csr_spmv_device(int m, int n, int nnzA, const value_type *d_valA, const index_type *d_rowPtrA, "
            "const index_type *d_colIndA, double alpha, const value_type *d_x, double beta, value_type *d_y);") in flat
    assert ("int csr_spmm_device(int m, int n, int nnzA, const value_type *d_valA, const index_type *d_rowPtrA, "
            "const index_type *d_colIndA, int k, double alpha, const value_type *d_X, long long ldX, double beta, "
            "value_type *d_Y, long long ldY);") in flat
    subprocess.check_call(["make", "-C", DEMO_DIR, "-s"])
    demo = os.path.join(DEMO_DIR, "spmv_demo")
    assert os.access(demo, os.X_OK)
    out = subprocess.run(["nm", "-D", "--undefined-only", demo], capture_output=True, text=True).stdout
    for name in ENTRY:
        assert name in out


# ---------------------------------------------------------------- the reference against a case written out by hand
# 5 x 7.  row 0 not ascending, with the pair (0, 0) twice; row 1 empty; row 2 holds -0 and +0; row 3 a NaN and the pair
# (3, 3) twice; row 4 an Inf.
NAN, INF = np.nan, np.inf
AP = np.array([0, 4, 4, 7, 10, 12], np.int32)
AJ = np.array([5, 2, 0, 0, 1, 2, 6, 0, 3, 3, 6, 4], np.int32)
AX = np.array([1, 2, 3, 4, -0.0, 0.0, 5, NAN, 6, -7, INF, -9], np.float64)
XV = np.array([1, 2, 3, 4, 5, 6, 7], np.float64)


def same(got, want):
    want = np.asarray(want, got.dtype)
    return got.shape == want.shape and np.array_equal(np.isnan(got), np.isnan(want)) and bool(np.all((got == want) | np.isnan(got)))


def test_spmvref_by_hand():
    y, S, K = sr.spmv(5, 7, AP, AJ, AX, XV)
    assert y.dtype == np.float64 and same(y, [19, 0, 35, NAN, INF])
    assert K.tolist() == [6, 2, 5, 5, 4] and S[0] == 19 and S[1] == 0 and S[2] == 35 and S[3] == INF and S[4] == INF
    # alpha and beta: t = alpha s, then + beta y only where beta != 0
    yold = np.array([1, NAN, 2, 3, 4], np.float64)
    assert same(sr.spmv(5, 7, AP, AJ, AX, XV, 2.0, 0.0, yold)[0], [38, 0, 70, NAN, INF])       # (y's NaN is never read)
    assert same(sr.spmv(5, 7, AP, AJ, AX, XV, 2.0, -1.0, yold)[0], [37, NAN, 68, NAN, INF])
    out, S, _ = sr.spmv(5, 7, AP, AJ, AX, XV, -2.0, 3.0, np.array([1, 1, 1, 1, 1.0]))
    assert same(out, [-35, 3, -67, NAN, -INF]) and S[0] == 41 and S[1] == 3
    # alpha == 0 takes no shortcut: 0 * Inf and 0 * NaN are NaN, 0 * finite is 0
    assert same(sr.spmv(5, 7, AP, AJ, AX, XV, 0.0, 0.0)[0], [0, 0, 0, NAN, NAN])
    # an x of zeros against the Inf: NaN by IEEE
    assert same(sr.spmv(5, 7, AP, AJ, AX, np.zeros(7))[0], [0, 0, 0, NAN, NAN])
    # without values every entry counts as 1
    assert same(sr.spmv(5, 7, AP, AJ, None, XV)[0], [11, 0, 12, 9, 12])
    # k columns: column c is (c + 1) x
    X = np.outer(XV, [1, 2, 3])
    Y, S, K = sr.spmm(5, 7, AP, AJ, AX, X)
    assert Y.shape == (5, 3) and same(Y[:, 1], [38, 0, 70, NAN, INF]) and same(Y[:, 2], [57, 0, 105, NAN, INF])
    assert K.shape == (5, 3) and K[:, 2].tolist() == [6, 2, 5, 5, 4]
    # the float build: inputs rounded to float first, products and sums in double, one rounding
    out = sr.spmv(5, 7, AP, AJ, np.where(np.isfinite(AX), AX * 0.1, 0.0), XV * 0.1, dtype=np.float32)[0]
    a32, x32 = (np.where(np.isfinite(AX), AX * 0.1, 0.0)).astype(np.float32).astype(np.float64), (XV * 0.1).astype(np.float32).astype(np.float64)
    assert out.dtype == np.float32 and out[2] == np.float32(a32[4] * x32[1] + a32[5] * x32[2] + a32[6] * x32[6])
    # empty shapes
    assert sr.spmv(0, 7, [0], [], [], XV)[0].shape == (0,) and same(sr.spmv(3, 0, [0, 0, 0, 0], [], [], [])[0], [0, 0, 0])
    assert same(sr.spmv(2, 0, [0, 0, 0], [], [], [], 1.0, 2.0, [1.0, -3.0])[0], [2, -6])


def test_spmvref_names_what_must_be_refused():
    assert sr.invalid(5, 7, AP, AJ) is None and sr.invalid(5, 7, AP, AJ, 3, 4, 5) is None
    assert sr.invalid(-1, 7, AP, AJ) == "negative size" and sr.invalid(5, -1, AP, AJ) == "negative size"
    assert sr.invalid(5, 7, AP, AJ, 0) == "k < 1"
    assert sr.invalid(5, 7, AP, AJ, 3, 2, 3) == "ldX < k" and sr.invalid(5, 7, AP, AJ, 3, 3, 2) == "ldY < k"
    assert sr.invalid(5, 7, None, AJ) == "NULL rowPtrA"
    assert sr.invalid(5, 7, AP, AJ, has_x=False) == "NULL x" and sr.invalid(5, 7, AP, AJ, has_y=False) == "NULL y"
    assert sr.invalid(5, 7, [0] * 6, [], has_x=False) is None and sr.invalid(0, 7, [0], [], has_y=False) is None
    assert sr.invalid(5, 7, AP, AJ, overlap=True) == "y overlaps an input"
    p = AP.copy(); p[0] = 1
    assert sr.invalid(5, 7, p, AJ) == "rowPtrA[0] != 0"
    p = AP.copy(); p[-1] = 11
    assert sr.invalid(5, 7, p, AJ) == "rowPtrA[m] != nnzA"
    p = AP.copy(); p[2] = 3
    assert sr.invalid(5, 7, p, AJ) == "decreasing rowPtrA"
    for col in (7, -1):
        j = AJ.copy(); j[11] = col
        assert sr.invalid(5, 7, AP, j) == "column of A out of range"
    assert set(sr.HOST_REFUSALS).isdisjoint(sr.DEVICE_REFUSALS) and len(sr.HOST_REFUSALS) == 9 and len(sr.DEVICE_REFUSALS) == 4


def test_spmvref_against_scipy():
    import scipy.sparse as sp
    for seed in range(12):
        rng = np.random.default_rng(700 + seed)
        m, n, k = int(rng.integers(1, 60)), int(rng.integers(1, 60)), int(rng.integers(1, 7))
        M = sp.random(m, n, density=float(rng.choice([0.05, 0.3])), format="csr", random_state=np.random.RandomState(seed))
        M.data = rng.integers(-9, 10, M.nnz).astype(np.float64)     # small integers (explicit zeros among them): every sum is exact
        M.sort_indices()
        Ap, Aj, Ax = M.indptr.astype(np.int32), M.indices.astype(np.int32), M.data.copy()
        for i in range(m):                                          # the rows in a random order: the result may not depend on it
            o = rng.permutation(Ap[i + 1] - Ap[i]) + Ap[i]
            Aj[Ap[i]:Ap[i + 1]], Ax[Ap[i]:Ap[i + 1]] = Aj[o], Ax[o]
        # duplicates add up: every entry once more with another value
        Ap2 = (2 * Ap).astype(np.int32)
        rows = np.repeat(np.arange(m), np.diff(Ap))
        o = np.argsort(np.concatenate((rows, rows)), kind="stable")
        extra = rng.integers(-9, 10, len(Ax)).astype(np.float64)
        Aj2, Ax2 = np.concatenate((Aj, Aj))[o], np.concatenate((Ax, extra))[o]
        M2 = M + sp.csr_matrix((extra, Aj, Ap), shape=(m, n))
        X, Y = rng.integers(-5, 6, (n, k)).astype(np.float64), rng.integers(-5, 6, (m, k)).astype(np.float64)
        for alpha, beta in ((1.0, 0.0), (-2.0, 3.0), (0.5, -1.0)):
            want = alpha * (M @ X) + beta * Y
            got, S, K = sr.spmm(m, n, Ap, Aj, Ax, X, alpha, beta, Y)
            assert np.array_equal(got, want), seed
            assert np.array_equal(S, abs(alpha) * (abs(M) @ abs(X)) + abs(beta) * abs(Y)), seed
            assert np.array_equal(K[:, 0], np.diff(Ap) + 2), seed
            assert np.array_equal(sr.spmm(m, n, Ap2, Aj2, Ax2, X, alpha, beta, Y)[0], alpha * (M2 @ X) + beta * Y), seed
        assert np.array_equal(sr.spmv(m, n, Ap, Aj, Ax, X[:, 0])[0], M @ X[:, 0]), seed
        ones = sp.csr_matrix((np.ones(M.nnz), M.indices, M.indptr), shape=(m, n))
        assert np.array_equal(sr.spmv(m, n, Ap, Aj, None, X[:, 0], dtype=np.float32)[0], (ones @ X[:, 0]).astype(np.float32)), seed
