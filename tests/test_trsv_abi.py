"""CPU tests of the level sets (bhs_csr_levels_device), the sparse triangular solve (bhs_csr_trsv_device), ILU(0) in place
(bhs_csr_ilu0_device) and the ILU(0)-preconditioned CG on top of them: the header declares the three entry points and the
ctypes lists match them, both libraries export them, the build tracks the new sources, the C++ facade's methods compile and
link (tests/trsv; tests/test_trsv_gpu.py runs the same binary on a GPU); the numpy restatement (tests/iluref.py) agrees with
cases written out by hand, with scipy's triangular solve and with the identity that defines ILU(0); amg.py's ILU-PCG, run on
the restatements in place of the device calls, needs at most half of plain CG's iterations in natural order and at most two
thirds in colour order, where the factors have as many levels as there are colours."""
import ctypes as C
import functools
import inspect
import os
import re
import subprocess

import numpy as np
import pytest
import scipy.sparse as sp
import torch
from scipy.sparse.linalg import spsolve_triangular

from conftest import ROOT
import aggref as ar
import gsref as gr
import iluref as ir
from test_aggregate_abi import HostHandle, host_spmv
from test_gs_abi import host_color, kinds_of

from benchmark_spgemm_using_csr_amd import _lib

ENTRIES = ("bhs_csr_levels_device", "bhs_csr_trsv_device", "bhs_csr_ilu0_device")
FAMILIES = ("levels_pass", "levels_order", "trsv_level", "ilu0_level")
DEMO_DIR = os.path.join(ROOT, "tests", "trsv")
SEEDS = (0, 1, 12345)
GRIDS = (("poisson5pt", 33, 33), ("poisson5pt", 64, 64), ("poisson9pt", 20, 20), ("poisson27pt", 9, 9, 9), ("poisson27pt", 16, 16, 16))


# ---------------------------------------------------------------- the interfaces
def test_header_declares_the_entry_points():
    txt = open(_lib.HEADER).read()
    decl = set(re.findall(r"BHS_API\s+[\w\s\*]+?\b(bhs_\w+)\s*\(", txt))
    vp, i = C.c_void_p, C.c_int
    for entry, count in zip(ENTRIES, (12, 14, 12)):
        assert entry in decl and entry in _lib.SYMBOLS
        res, args = _lib.SYMBOLS[entry]
        want = ["int" if t is i else "double" if t is C.c_double else "ptr" for t in args]
        assert res is i and kinds_of(txt, entry) == want and len(want) == count, entry
    assert _lib.SYMBOLS[ENTRIES[0]][1][:6] == [vp, i, i, vp, vp, i] and _lib.SYMBOLS[ENTRIES[1]][1][9] is C.c_double
    sections = re.findall(r"/\* ---- ([^-]+?) -+", txt)
    assert sections[-1] == "triangular solve and ILU(0)" and sections[-2] == "measurement"
    sect = txt[txt.index("---- triangular solve and ILU(0)"):]
    assert txt.index("bhs_version(void)") < txt.index("---- triangular solve and ILU(0)")   # behind the last declaration before it
    for fam in FAMILIES:
        assert fam in sect, fam
    for words in ("alues are NOT TAKEN", "exactly one", "the diagonal included, is ignored", "function of the pattern",
                  "only rise and never pass the true level", "DEPENDS ON TIMING", "BHS_ERR_INTERNAL", "n + 1 passes", "CAPACITY",
                  "BHS_ERR_ALLOC", "2^26", "tridiagonal matrix of 2^20 rows", "n == 0 succeeds", "HOST array",
                  "summed in double from +0", "one rounding to the value type", "IEEE results where a_ii is 0", "FIRST entry with j == i",
                  "d_x == d_b exactly is allowed", "Rows that are not listed are untouched", "One control round trip per call",
                  "NOT fused into one launch", "profiles/trsv_case.md", "strictly ascending", "Owner computes",
                  "unit diagonal is not stored", "smallest listed row whose pivot"):
        assert words in sect, words
    for name, value in (("BHS_TRI_LOWER", 1), ("BHS_TRI_UPPER", 2), ("BHS_TRI_UNIT_DIAG", 4)):
        assert re.search(r"#define %s\s+%d\b" % (name, value), sect) and getattr(_lib, name) == value
    host = open(os.path.join(_lib.CSRC, "bhs_host_trsv.inc.h")).read()
    for fam in FAMILIES:
        assert '"%s"' % fam in host, fam


def test_both_libraries_export_the_entry_points(hiplib):
    for path in (_lib.SO_PATH, _lib.SO_PATH_F32):
        raw = C.CDLL(path)
        blob = open(path, "rb").read()
        for entry in ENTRIES:
            assert getattr(raw, entry) is not None
        for kern in (b"k_lev_pass", b"k_trsv_level", b"k_ilu0_level"):
            assert kern in blob, (path, kern)
        assert b"k_trsv_fused" not in blob, path                     # measured slower and left out (profiles/trsv_case.md)


def test_sources_are_tracked_by_the_build():
    files = ("bhs_trsv.hip.h", "bhs_ilu0.hip.h", "bhs_host_trsv.inc.h")
    mk = open(os.path.join(_lib.CSRC, "Makefile")).read()
    for f in files:
        assert f in _lib.SOURCES and f in mk, f
    unit = open(os.path.join(_lib.CSRC, "bhsparse_hip.hip")).read()
    incs = re.findall(r'#include "(bhs_host_\w+\.inc\.h)"', unit)
    assert incs[incs.index("bhs_host_color.inc.h") + 1] == "bhs_host_trsv.inc.h"
    assert "SideWs trsvWs;" in unit
    cabi = open(os.path.join(_lib.CSRC, "bhs_host_cabi.inc.h")).read()
    assert "release(h->trsvWs)" in cabi and '"trsv_fuse"' not in cabi   # (no fused kernel, no option: profiles/trsv_case.md)
    host = open(os.path.join(_lib.CSRC, "bhs_host_trsv.inc.h")).read()
    assert '#include "bhs_trsv.hip.h"' in host and '#include "bhs_ilu0.hip.h"' in host
    assert host.count("guarded(h,") == 3 and "BHS_ERR_INTERNAL" in host
    # the order of the levels is the colouring's, called, not copied: one scan in the library's colouring, none here
    assert "co_order(" in host and "side_scan(" not in host and "k_col_count" not in host
    color = open(os.path.join(_lib.CSRC, "bhs_host_color.inc.h")).read()
    assert color.count("side_scan(") == 1 and "int co_order(" in color
    call = host[host.index("int ts_call("):host.index("typedef void (*TsKernel)")]
    assert call.count("side_read_ctl(") == 1                          # one control round trip per solve / factorisation, at its end
    for f in files[:2]:
        code = re.sub(r"//.*", "", open(os.path.join(_lib.CSRC, f)).read())
        assert "asm" not in code
        assert not re.search(r"\bwhile\s*\(\s*(1|true)\s*\)|for\s*\(\s*;\s*;\s*\)", code)   # nothing spins
        assert len(re.findall(r"__global__", code)) == len(re.findall(r"__global__ __launch_bounds__\(256\)", code))
    # results are written by plain stores: the atomics are the levels-in-use maximum and the pivot's minimum
    trsv = re.sub(r"//.*", "", open(os.path.join(_lib.CSRC, "bhs_trsv.hip.h")).read())
    assert sorted(re.findall(r"atomic\w+\s*\(([^,]+),", trsv)) == ["&sTop", "ctl + CO_NCOL"]
    ilu = re.sub(r"//.*", "", open(os.path.join(_lib.CSRC, "bhs_ilu0.hip.h")).read())
    assert re.findall(r"(atomic\w+)\s*\(([^,]+),", ilu) == [("atomicMin", "ctl + TS_PIVOT")]
    assert "int* level," in trsv and "value_t* x," in trsv and "value_t* Ax," in ilu   # plain pointers where reads meet writes


def test_null_handle_and_missing_platform(hiplib):
    inv = _lib.BHS_ERR_INVALID_ARG
    assert hiplib.bhs_csr_levels_device(None, 0, 0, None, None, _lib.BHS_TRI_LOWER, None, None, None, None, None, None) == inv
    assert hiplib.bhs_csr_trsv_device(None, 0, 0, None, None, None, 0, None, None, 1.0, None, None, _lib.BHS_TRI_LOWER, None) == inv
    assert hiplib.bhs_csr_ilu0_device(None, 0, 0, None, None, None, 0, None, None, 0, None, None) == inv
    from benchmark_spgemm_using_csr_amd import amg, facade
    bh = facade.bhsparse()
    assert amg.levels_raw_device(bh, 0, 0, None, None, 1, None, None, None) == _lib.BHS_ERR_NOT_READY
    assert amg.trsv_raw_device(bh, 0, 0, None, None, None, 0, None, None, 1.0, None, None, 1) == _lib.BHS_ERR_NOT_READY
    assert amg.ilu0_raw_device(bh, 0, 0, None, None, None, 0, None, None, 0) == _lib.BHS_ERR_NOT_READY


def test_python_module_has_the_calls():
    from benchmark_spgemm_using_csr_amd import amg
    sig = lambda f: list(inspect.signature(f).parameters)           # noqa: E731
    dflt = lambda f: {k: v.default for k, v in inspect.signature(f).parameters.items() if v.default is not inspect.Parameter.empty}   # noqa: E731
    assert sig(amg.levels_raw_device) == ["bh", "n", "nnzA", "d_rowPtrA", "d_colIndA", "flags", "d_level", "d_order", "d_levelPtr"]
    assert sig(amg.levels_device) == ["bh", "n", "A", "upper"] and dflt(amg.levels_device) == {"upper": False}
    assert sig(amg.trsv_raw_device) == ["bh", "n", "nnzA", "d_rowPtrA", "d_colIndA", "d_valA", "nlevels", "h_levelPtr", "d_order", "alpha",
                                        "d_b", "d_x", "flags"]
    assert sig(amg.trsv_device) == ["bh", "A", "levels", "b", "x", "alpha", "upper", "unit_diag"]
    assert dflt(amg.trsv_device) == {"alpha": 1.0, "upper": False, "unit_diag": False}
    assert sig(amg.ilu0_raw_device) == ["bh", "n", "nnzA", "d_rowPtrA", "d_colIndA", "d_valA", "nlevels", "h_levelPtr", "d_order", "flags"]
    assert sig(amg.ilu0_device) == ["bh", "A", "levels"]
    assert sig(amg.ilu0_setup_device) == ["bh", "A", "ordering", "seed"] and dflt(amg.ilu0_setup_device) == {"ordering": "natural", "seed": 0}
    assert sig(amg.ilu0_apply_device) == ["bh", "M", "r", "z"]
    assert sig(amg.ilu0_pcg_device) == ["bh", "A", "b", "tol", "maxiter", "ordering"]
    assert dflt(amg.ilu0_pcg_device) == {"tol": 1e-8, "maxiter": 100, "ordering": "colour"}
    assert sig(amg.pcg_device) == ["bh", "levels", "b", "tol", "maxiter", "smoother"]         # as they were
    assert sig(amg.solve_device) == ["bh", "levels", "b", "tol", "maxiter"]
    with pytest.raises(ValueError):
        amg.ilu0_setup_device(None, (torch.zeros(2, dtype=torch.int32),), ordering="rcm")


def test_cpp_facade_extension_builds(hiplib):
    src = open(os.path.join(ROOT, "benchmark_spgemm_using_csr_amd", "host", "bhsparse.h")).read()
    flat = re.sub(r"\s+", " ", src)
    assert ("int csr_levels_device(int n, int nnzA, const index_type *d_rowPtrA, const index_type *d_colIndA, int flags, "
            "index_type *d_level, index_type *d_order, index_type *d_levelPtr, int *nlevels_out, int *passes_out);") in flat
    assert ("int csr_trsv_device(int n, int nnzA, const index_type *d_rowPtrA, const index_type *d_colIndA, const value_type *d_valA, "
            "int nlevels, const index_type *h_levelPtr, const index_type *d_order, double alpha, const value_type *d_b, "
            "value_type *d_x, int flags);") in flat
    assert ("int csr_ilu0_device(int n, int nnzA, const index_type *d_rowPtrA, const index_type *d_colIndA, value_type *d_valA, "
            "int nlevels, const index_type *h_levelPtr, const index_type *d_order, int flags, int *pivot_out);") in flat
    subprocess.check_call(["make", "-C", DEMO_DIR, "-s"])
    demo = os.path.join(DEMO_DIR, "trsv_demo")
    assert os.access(demo, os.X_OK)
    out = subprocess.run(["nm", "-D", "--undefined-only", demo], capture_output=True, text=True).stdout
    for entry in ENTRIES:
        assert entry in out
    assert "tests/trsv/trsv_demo" in open(os.path.join(ROOT, ".gitignore")).read().split()


# ---------------------------------------------------------------- the restatement by hand
def csr(rows, n):
    """(Ap, Aj, Ax) from a list of rows of (column, value) pairs, kept in the order given"""
    Ap = np.zeros(n + 1, np.int32)
    Aj, Ax = [], []
    for i, row in enumerate(rows):
        Aj += [c for c, _ in row]
        Ax += [v for _, v in row]
        Ap[i + 1] = len(Aj)
    return Ap, np.array(Aj, np.int32), np.array(Ax, np.float64)


def test_a_path_of_seven_by_hand():
    """0 - 1 - ... - 6, tridiagonal with 2 on the diagonal and -1 beside it: the lower triangle chains every row to the one
    before it -- level(i) = i, seven levels of one row; the upper triangle the other way round, level(i) = 6 - i.
    L x = b with b = 1: x_0 = 1/2, x_i = (1 + x_{i-1}) / 2 = 1 - 2^-(i+1)."""
    n = 7
    rows = [[(j, 2.0 if j == i else -1.0) for j in (i - 1, i, i + 1) if 0 <= j < n] for i in range(n)]
    Ap, Aj, Ax = csr(rows, n)
    level, nlevels, order, ptr = ir.levels(n, Ap, Aj)
    assert level.tolist() == list(range(7)) and nlevels == 7 and order.tolist() == list(range(7)) and ptr.tolist() == list(range(8))
    ulevel, unl, uorder, uptr = ir.levels(n, Ap, Aj, upper=True)
    assert ulevel.tolist() == list(range(6, -1, -1)) and unl == 7 and uorder.tolist() == list(range(6, -1, -1))
    assert level.dtype == np.int32 and order.dtype == np.int32 and ptr.dtype == np.int32
    x = ir.trsv(n, Ap, Aj, Ax, ptr, order, np.ones(n), np.zeros(n))
    assert x.tolist() == [1.0 - 2.0 ** -(i + 1) for i in range(n)]
    # the upper solve mirrors it; alpha scales b; a unit diagonal divides by nothing
    xu = ir.trsv(n, Ap, Aj, Ax, uptr, uorder, np.ones(n), np.zeros(n), upper=True)
    assert xu.tolist() == x.tolist()[::-1]
    assert ir.trsv(n, Ap, Aj, Ax, ptr, order, np.ones(n), np.zeros(n), alpha=-2.0).tolist() == (-2.0 * x).tolist()
    assert ir.trsv(n, Ap, Aj, Ax, ptr, order, np.ones(n), np.zeros(n), unit_diag=True).tolist() == [float(i + 1) for i in range(n)]
    # rows that are not listed stay
    part = ir.trsv(n, Ap, Aj, Ax, ptr[:4], order, np.ones(n), np.full(n, 9.0))
    assert part.tolist() == x.tolist()[:3] + [9.0] * 4
    # ILU(0) of a tridiagonal matrix is its LU: u_0 = 2, l_i = -1 / u_{i-1}, u_i = 2 + l_i = (i + 2) / (i + 1)
    val, pivot = ir.ilu0(n, Ap, Aj, Ax)
    assert pivot == -1
    Lm, Um = ir.split(n, Ap, Aj, val)
    assert np.allclose(Um.diagonal(), [(i + 2.0) / (i + 1.0) for i in range(n)], rtol=1e-15, atol=0)
    assert np.allclose((Lm @ Um).toarray(), sp.csr_matrix((Ax, Aj, Ap), shape=(n, n)).toarray(), rtol=0, atol=1e-15)


def test_an_arrow_a_repeated_column_and_the_diagonal_by_hand():
    # an arrow pointing down-right: the last row and column are full.  Lower: rows 0 .. n-2 have no entry below the
    # diagonal (level 0), the last row reads them all (level 1).  Upper: every row but the last reads the last one.
    n = 6
    rows = [[(i, 4.0), (n - 1, 1.0)] for i in range(n - 1)] + [[(j, 1.0) for j in range(n - 1)] + [(n - 1, 8.0)]]
    Ap, Aj, Ax = csr(rows, n)
    level, nlevels, order, ptr = ir.levels(n, Ap, Aj)
    assert level.tolist() == [0] * 5 + [1] and nlevels == 2 and ptr.tolist() == [0, 5, 6]
    ulevel, unl, uorder, uptr = ir.levels(n, Ap, Aj, upper=True)
    assert ulevel.tolist() == [1] * 5 + [0] and uorder.tolist() == [5, 0, 1, 2, 3, 4] and uptr.tolist() == [0, 1, 6]
    x = ir.trsv(n, Ap, Aj, Ax, ptr, order, np.full(n, 4.0), np.zeros(n))
    assert x.tolist() == [1.0] * 5 + [(4.0 - 5.0) / 8.0]
    # the arrow is closed under elimination: ILU(0) is LU, and only the corner changes: 8 - 5 * (1 / 4)
    val, pivot = ir.ilu0(n, Ap, Aj, Ax)
    assert pivot == -1 and val[-1] == 8.0 - 5.0 / 4.0 and val[Ap[n - 1]:-1].tolist() == [0.25] * 5
    # a row with a repeated column, out of order, and entries of the other triangle: the level does not care, the solve
    # adds both entries up and takes the FIRST diagonal entry
    rows = [[(0, 2.0)], [(1, 4.0), (0, 1.0)], [(3, 5.0), (1, 1.0), (2, 8.0), (1, 2.0), (0, 1.0), (2, 16.0)], [(3, 1.0)]]
    Ap, Aj, Ax = csr(rows, 4)
    level, nlevels, order, ptr = ir.levels(4, Ap, Aj)
    assert level.tolist() == [0, 1, 2, 0] and order.tolist() == [0, 3, 1, 2] and ptr.tolist() == [0, 2, 3, 4]
    x = ir.trsv(4, Ap, Aj, Ax, ptr, order, np.array([2.0, 5.0, 12.0, 7.0]), np.zeros(4))
    assert x.tolist() == [1.0, 1.0, (12.0 - 1.0 - 2.0 - 1.0) / 8.0, 7.0]
    assert ir.levels(4, Ap, Aj, upper=True)[0].tolist() == [0, 0, 1, 0]
    # without a diagonal entry a row has level 0 all the same, a unit solve works, a plain one is refused
    Ap, Aj, Ax = csr([[], [(0, 3.0)]], 2)
    assert ir.levels(2, Ap, Aj)[0].tolist() == [0, 1]
    assert ir.trsv(2, Ap, Aj, Ax, [0, 1, 2], [0, 1], np.ones(2), np.zeros(2), unit_diag=True).tolist() == [1.0, -2.0]
    with pytest.raises(ValueError):
        ir.trsv(2, Ap, Aj, Ax, [0, 1, 2], [0, 1], np.ones(2), np.zeros(2))
    # a pivot that is exactly 0: row 1 of [[1, 2], [2, 4]]
    Ap, Aj, Ax = csr([[(0, 1.0), (1, 2.0)], [(0, 2.0), (1, 4.0)]], 2)
    val, pivot = ir.ilu0(2, Ap, Aj, Ax)
    assert pivot == 1 and val.tolist() == [1.0, 2.0, 2.0, 0.0]
    assert ir.levels(0, np.zeros(1, np.int32), np.zeros(0, np.int32))[1] == 0


def test_the_lane_sum_is_the_butterfly():
    """L lanes, lane q mod L takes entry q; the lanes meet 0 + 1, 2 + 3, then the pairs: written out for L = 4 and six terms"""
    t = [1e16, 1.0, -1e16, 1.0, 1.0, 1.0]
    assert ir.lane_sum(t, 4) == ((1e16 + 1.0) + (1.0 + 1.0)) + (-1e16 + 1.0)
    assert ir.lane_sum(t, 1) == ((((1e16 + 1.0) - 1e16) + 1.0) + 1.0) + 1.0
    assert ir.lane_sum([], 16) == 0.0 and ir.lanes_per_row(1089, 5313) == 4 and ir.lanes_per_row(300, 898) == 1
    assert ir.lanes_per_row(729, 15625) == 16 and ir.lanes_per_row(140, 9800) == 64


# ---------------------------------------------------------------- the restatement against scipy
@functools.lru_cache(maxsize=None)
def cases():
    return ar.gpu_cases()


@pytest.mark.parametrize("name", ("path300", "poisson5pt_33", "poisson27pt_9", "uniform2048", "star1024", "two_k70"))
def test_the_solve_agrees_with_scipy(name):
    n, Sp, Sj = cases()[name]
    rng = np.random.default_rng(3)
    r = np.repeat(np.arange(n), np.diff(Sp))
    Ax = rng.uniform(-1.0, 1.0, len(Sj))
    Ax[r == Sj] = np.diff(Sp)[r[r == Sj]] + 1.0                       # dominant: the solves are well conditioned
    A = sp.csr_matrix((Ax, Sj, Sp), shape=(n, n))
    if not np.all(A.diagonal() != 0):
        A = (A + sp.diags(np.where(A.diagonal() == 0, float(np.diff(Sp).max()) + 1.0, 0.0))).tocsr()
    A.sort_indices()
    Ap, Aj, Ax = A.indptr, A.indices, A.data
    b = rng.standard_normal(n)
    for upper in (False, True):
        level, nlevels, order, ptr = ir.levels(n, Ap, Aj, upper)
        assert ptr[0] == 0 and ptr[-1] == n and np.all(np.diff(ptr) > 0) and np.array_equal(np.sort(order), np.arange(n))
        for c in range(nlevels):
            part = order[ptr[c]:ptr[c + 1]]
            assert np.all(level[part] == c) and np.all(np.diff(part) > 0)
        T = (sp.triu(A) if upper else sp.tril(A)).tocsr()
        got = ir.trsv(n, Ap, Aj, Ax, ptr, order, b, np.zeros(n), alpha=0.5, upper=upper)
        want = spsolve_triangular(T, 0.5 * b, lower=not upper)
        assert np.allclose(got, want, rtol=0, atol=1e-12 * np.abs(want).max()), (name, upper)
        # a unit diagonal: D^-1 A, whose stored diagonal of ones is ignored, not divided by
        Au = Ax / A.diagonal()[np.repeat(np.arange(n), np.diff(Ap))]
        got = ir.trsv(n, Ap, Aj, Au, ptr, order, b, np.zeros(n), upper=upper, unit_diag=True)
        want = spsolve_triangular(T, A.diagonal() * b, lower=not upper)
        assert np.allclose(got, want, rtol=0, atol=1e-12 * np.abs(want).max()), (name, upper, "unit")
    if name == "path300":
        assert ir.levels(n, Ap, Aj)[1] == 300
    if name == "poisson5pt_33":
        assert ir.levels(n, Ap, Aj)[1] == 65
    if name == "poisson27pt_9":
        assert ir.levels(n, Ap, Aj)[1] == 57                         # nx + 2 ny + 4 nz - 6
    if name == "two_k70":
        assert ir.levels(n, Ap, Aj)[1] == 70 and np.all(np.diff(ir.levels(n, Ap, Aj)[3]) == 2)


@pytest.mark.parametrize("args", GRIDS[:4] + (("poisson7pt", 10, 10, 10),), ids=lambda a: "%s_%d" % (a[0], a[1]))
def test_the_restatement_satisfies_the_ilu0_identity(args):
    """(L U)_ij = a_ij on the pattern, within (m_ij + 2) u (sum_k |l_ik| |u_kj| + |a_ij|) in both value types -- every update of
    an entry and the division commit one rounding of the value type; and off the pattern L U is NOT A (the fill is dropped)"""
    n, Ap, Aj, Ax = ar.poisson(*args)
    for dtype, u in ((np.float64, 2.0 ** -53), (np.float32, 2.0 ** -24)):
        val, pivot = ir.ilu0(n, Ap, Aj, Ax, dtype)
        err, most = ir.identity_error(n, Ap, Aj, Ax, val)
        print("%s %s: identity error %.3g u, at most %d updates an entry" % (args, np.dtype(dtype).name, err / u, most))
        assert pivot == -1 and val.dtype == dtype and err <= u
    Lm, Um = ir.split(n, Ap, Aj, val)
    assert abs(Lm @ Um - sp.csr_matrix((Ax, Aj, Ap), shape=(n, n))).max() > 1e-3


# ---------------------------------------------------------------- ILU-PCG on the restatements
def host_levels(bh, n, A, upper=False):
    level, nlevels, order, ptr = ir.levels(n, A[0].numpy(), A[1].numpy(), upper)
    bh.levels_ms, bh.levels_nlevels, bh.levels_passes = 0.5, nlevels, 8
    bh.calls.append("levels_upper" if upper else "levels_lower")
    return torch.from_numpy(level), nlevels, torch.from_numpy(order), ptr


def host_trsv(bh, A, levels, b, x, alpha=1.0, upper=False, unit_diag=False):
    n = int(A[0].numel()) - 1
    M = HostHandle.mat(A, (n, n))
    T = (sp.triu(M) if upper else sp.tril(M)).tocsr()
    assert levels[3][-1] == n                                         # every row is listed
    bh.calls.append("trsv_upper" if upper else "trsv_lower")
    x.copy_(torch.from_numpy(spsolve_triangular(T, alpha * b.numpy(), lower=not upper, unit_diagonal=unit_diag)))   # in place
    return x


def host_ilu0(bh, A, levels):
    n = int(A[0].numel()) - 1
    val, pivot = ir.ilu0(n, A[0].numpy(), A[1].numpy(), A[2].numpy())
    bh.ilu0_ms, bh.ilu0_pivot = 0.5, pivot
    bh.calls.append("ilu0")
    A[2].copy_(torch.from_numpy(val))                                 # in place, as the device call
    return A


def host_permuted(bh, n, A, perm):
    p = perm.numpy().astype(np.int64)
    bh.calls.append("permute")
    return HostHandle.tens(HostHandle.mat(A, (n, n))[p][:, p])


@pytest.fixture
def on_the_host(monkeypatch):
    from benchmark_spgemm_using_csr_amd import amg
    monkeypatch.setattr(amg, "color_device", host_color)
    monkeypatch.setattr(amg, "levels_device", host_levels)
    monkeypatch.setattr(amg, "trsv_device", host_trsv)
    monkeypatch.setattr(amg, "ilu0_device", host_ilu0)
    monkeypatch.setattr(amg, "_permuted_device", host_permuted)
    monkeypatch.setattr(amg, "csr_spmv_device", host_spmv)
    return amg


@pytest.mark.parametrize("args", GRIDS, ids=lambda a: "%s_%d" % (a[0], a[1]))
def test_ilu_pcg_iterations(on_the_host, args):
    """Poisson values, a random right-hand side, to 1e-8: CG preconditioned with ILU(0) needs at most 1/2 of plain CG's
    iterations in natural order (measured with the restatement, seeds 0, 1 and 12345: 0.33 .. 0.43) and at most 2/3 in colour
    order (0.47 .. 0.55); in colour order both factors have as many levels as there are colours; amg.ilu0_pcg_device, run on
    the restatements, is the restatement's iteration."""
    amg = on_the_host
    n, Ap, Aj, Ax = ar.poisson(*args)
    A = sp.csr_matrix((Ax, Aj, Ap), shape=(n, n))
    setups = {o: ir.ilu0_setup(A, o) for o in ("natural", "colour")}
    ncolors = setups["colour"]["ncolors"]
    assert setups["colour"]["nlevels"] == (ncolors, ncolors) and ncolors == gr.colouring(n, Ap, Aj, 0)[1]
    assert setups["natural"]["nlevels"][0] > 3 * ncolors and setups["natural"]["pivot"] == setups["colour"]["pivot"] == -1
    for seed in SEEDS:
        b = np.random.default_rng(seed).standard_normal(n)
        _, plain, _ = ir.pcg(A, b, None, 1e-8, 1000)
        its = {}
        for o, M in setups.items():
            x, its[o], res = ir.pcg(A, b, lambda r: ir.ilu0_apply(M, r), 1e-8, 1000)     # noqa: B023
            assert res[-1] <= 1e-8 * res[0] and np.linalg.norm(b - A @ x) <= 1.01e-8 * np.linalg.norm(b)
        print("%s seed %d: plain %d, natural %d (%.3f), colour %d (%.3f), colours %d, levels %s"
              % (args, seed, plain, its["natural"], its["natural"] / plain, its["colour"], its["colour"] / plain, ncolors,
                 setups["natural"]["nlevels"]))
        assert 2 * its["natural"] <= plain, (args, seed, its, plain)
        assert 3 * its["colour"] <= 2 * plain, (args, seed, its, plain)
        if seed == 0:
            tb = torch.from_numpy(b)
            for o in ("natural", "colour"):
                bh = HostHandle()
                x, got, res = amg.ilu0_pcg_device(bh, HostHandle.tens(A), tb, 1e-8, 200, ordering=o)
                assert got == its[o] and len(res) == got + 1 and res[-1] <= 1e-8 * res[0], (args, o, got, its[o])
                assert np.linalg.norm(b - A @ x.numpy()) <= 1.01e-8 * np.linalg.norm(b)
                head = ["select", "transpose", "add", "color", "permute"] if o == "colour" else []
                assert bh.calls == head + ["levels_lower", "levels_upper", "ilu0"] + ["trsv_lower", "trsv_upper"] * got, (o, bh.calls[:12])
