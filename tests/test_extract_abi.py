"""CPU tests of the extraction's interfaces (bhs_csr_extract_symbolic_device, bhs_csr_extract_numeric_device): both libraries
export the entry points the header declares, the build tracks the new sources, the Python facades carry them, the C++
facade's extension methods compile and link against the C-ABI library (tests/extract; tests/test_extract_gpu.py runs the same
binary on a GPU), and the numpy restatement (tests/extractref.py) agrees with a case written out by hand and with scipy."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

from conftest import ROOT
import extractref as ex

from benchmark_spgemm_using_csr_amd import _lib

EXTRACT = ("bhs_csr_extract_symbolic_device", "bhs_csr_extract_numeric_device")
FAMILIES = ("extract_map", "extract_count", "extract_scan", "extract_short", "extract_wave", "extract_long")
DEMO_DIR = os.path.join(ROOT, "tests", "extract")


def test_header_declares_the_extract_entry_points():
    txt = open(_lib.HEADER).read()
    decl = set(re.findall(r"BHS_API\s+[\w\s\*]+?\b(bhs_\w+)\s*\(", txt))
    for name in EXTRACT:
        assert name in decl
        assert name in _lib.SYMBOLS
    assert len(_lib.SYMBOLS["bhs_csr_extract_symbolic_device"][1]) == 12
    assert len(_lib.SYMBOLS["bhs_csr_extract_numeric_device"][1]) == 17
    assert "---- extract" in txt
    for fam in FAMILIES + ("extract_reordered_rows", "bhs_csr_transpose_values_device(h, nnzZ, d_valX, d_perm, d_valZ"):
        assert fam in txt, fam


def test_both_libraries_export_the_extract_entry_points(hiplib):
    for path in (_lib.SO_PATH, _lib.SO_PATH_F32):
        raw = C.CDLL(path)
        for name in EXTRACT:
            assert getattr(raw, name) is not None
        blob = open(path, "rb").read()
        for kern in (b"k_ex_map", b"k_ex_count", b"k_ex_count_long", b"k_ex_fill_short", b"k_ex_fill_wave", b"k_ex_fill_long"):
            assert kern in blob, (path, kern)


def test_extract_sources_are_tracked_by_the_build():
    assert "bhs_extract.hip.h" in _lib.SOURCES and "bhs_host_extract.inc.h" in _lib.SOURCES
    mk = open(os.path.join(_lib.CSRC, "Makefile")).read()
    assert "bhs_extract.hip.h" in mk and "bhs_host_extract.inc.h" in mk
    unit = open(os.path.join(_lib.CSRC, "bhsparse_hip.hip")).read()
    assert re.findall(r'#include "(bhs_host_\w+\.inc\.h)"', unit)[-2:] == ["bhs_host_semiring.inc.h", "bhs_host_extract.inc.h"]
    host = open(os.path.join(_lib.CSRC, "bhs_host_extract.inc.h")).read()
    assert '#include "bhs_extract.hip.h"' in host                   # (the kernels' header comes with the host part)


def test_null_handle_is_rejected_by_the_extract_entry_points(hiplib):
    inv = _lib.BHS_ERR_INVALID_ARG
    assert hiplib.bhs_csr_extract_symbolic_device(None, 0, 0, 0, None, None, 0, None, 0, None, None, None) == inv
    assert hiplib.bhs_csr_extract_numeric_device(None, 0, 0, 0, None, None, None, 0, None, 0, None, 0, None, None, None, None,
                                                 None) == inv


def test_python_facade_has_the_extraction():
    from benchmark_spgemm_using_csr_amd import facade
    for name in ("csr_extract_symbolic_device", "csr_extract_numeric_device", "csr_extract_raw_device", "csr_extract_device"):
        assert callable(getattr(facade.bhsparse, name, None)), name
    assert callable(getattr(facade, "extract_csr", None))
    assert callable(getattr(facade, "permute_csr", None))
    assert facade.bhsparse().extract_ms == 0.0
    # without a platform the raw calls answer, they do not crash
    assert facade.bhsparse().csr_extract_symbolic_device(0, 0, 0, None, None, 0, None, 0, None, None)[0] == _lib.BHS_ERR_NOT_READY


def test_cpp_facade_extract_extension_builds(hiplib):
    src = open(os.path.join(ROOT, "benchmark_spgemm_using_csr_amd", "host", "bhsparse.h")).read()
    flat = re.sub(r"\s+", " ", src)
    assert ("int csr_extract_symbolic_device(int m, int n, int nnzX, const index_type *d_rowPtrX, const index_type *d_colIndX, "
            "int mI, const index_type *d_rows, int nJ, const index_type *d_cols, index_type *d_rowPtrZ, int *nnzZ_out);") in flat
    assert ("int csr_extract_numeric_device(int m, int n, int nnzX, const value_type *d_valX, const index_type *d_rowPtrX, "
            "const index_type *d_colIndX, int mI, const index_type *d_rows, int nJ, const index_type *d_cols, int nnzZ, "
            "const index_type *d_rowPtrZ, index_type *d_colIndZ, value_type *d_valZ, index_type *d_perm);") in flat
    subprocess.check_call(["make", "-C", DEMO_DIR, "-s"])
    demo = os.path.join(DEMO_DIR, "extract_demo")
    assert os.access(demo, os.X_OK)
    out = subprocess.run(["nm", "-D", "--undefined-only", demo], capture_output=True, text=True).stdout
    for name in EXTRACT:
        assert name in out


# ---------------------------------------------------------------- the reference against a case written out by hand
# 5 x 7.  row 0 unsorted with the pair (0, 2) twice; row 1 empty; a NaN with a payload and a -0; rows with a repeat, cols
# descending (column 3 and 4 are not named).
NAN_PAYLOAD = np.array([0x7FF8000000000ABC], np.uint64).view(np.float64)[0]
ROWS = [
    ([5, 2, 0, 2], [1.0, 2.0, 3.0, 4.0]),
    ([], []),
    ([1, 6], [-0.0, 5.0]),
    ([0, 2, 3], [NAN_PAYLOAD, 6.0, 7.0]),
    ([6, 5], [8.0, 9.0]),
]
XP = np.cumsum([0] + [len(c) for c, _ in ROWS]).astype(np.int32)
XJ = np.array([c for cs, _ in ROWS for c in cs], np.int32)
XX = np.array([v for _, vs in ROWS for v in vs], np.float64)
TAKE_ROWS = [3, 0, 1, 2, 0]
TAKE_COLS = [6, 5, 2, 1, 0]                                         # places: 6 -> 0, 5 -> 1, 2 -> 2, 1 -> 3, 0 -> 4


def test_extractref_by_hand():
    Zp, Zj, Zx, perm, reordered = ex.extract(5, 7, XP, XJ, XX, TAKE_ROWS, TAKE_COLS)
    assert Zp.dtype == np.int32 and Zj.dtype == np.int32 and perm.dtype == np.int32 and Zx.dtype == np.float64
    assert Zp.tolist() == [0, 2, 6, 6, 8, 12]
    #                      X row 3 | X row 0     | X row 2 | X row 0 again
    assert Zj.tolist() == [2, 4, 1, 2, 2, 4, 0, 3, 1, 2, 2, 4]
    assert perm.tolist() == [7, 6, 0, 1, 3, 2, 5, 4, 0, 1, 3, 2]
    # the duplicate pair (0, 2): 2.0 came first in X and comes first in Z
    want = np.array([6.0, NAN_PAYLOAD, 1.0, 2.0, 4.0, 3.0, 5.0, -0.0, 1.0, 2.0, 4.0, 3.0])
    assert np.array_equal(Zx.view(np.uint64), want.view(np.uint64))
    assert Zx.view(np.uint64)[1] == 0x7FF8000000000ABC and Zx.view(np.uint64)[7] == 0x8000000000000000
    assert np.array_equal(Zx.view(np.uint64), XX[perm].view(np.uint64))
    assert reordered == 4                                           # every row with two entries or more: cols descend


def test_extractref_defaults_float_and_pattern_only():
    Zp, Zj, Zx, perm, reordered = ex.extract(5, 7, XP, XJ, XX.astype(np.float32))
    assert Zx.dtype == np.float32 and np.array_equal(Zp, XP) and reordered == 2      # (row 0 and row 4 are put in order)
    assert Zj[:4].tolist() == [0, 2, 2, 5] and perm[:4].tolist() == [2, 1, 3, 0] and np.array_equal(Zj[4:9], XJ[4:9]) and Zj[9:].tolist() == [5, 6]
    Zp2, Zj2, none, perm2, _ = ex.extract(5, 7, XP, XJ)
    assert none is None and np.array_equal(Zp, Zp2) and np.array_equal(Zj, Zj2) and np.array_equal(perm, perm2)
    # a row gather leaves ascending rows alone
    Zp, Zj, Zx, perm, reordered = ex.extract(5, 7, XP, XJ, XX, rows=[4, 3, 1])
    assert Zp.tolist() == [0, 2, 5, 5] and Zj.tolist() == [5, 6, 0, 2, 3] and perm.tolist() == [10, 9, 6, 7, 8] and reordered == 1
    # empty selections
    Zp, Zj, Zx, perm, reordered = ex.extract(5, 7, XP, XJ, XX, rows=[], cols=[1])
    assert Zp.tolist() == [0] and len(Zj) == len(Zx) == len(perm) == 0 and reordered == 0
    Zp, Zj, Zx, perm, reordered = ex.extract(5, 7, XP, XJ, XX, cols=[])
    assert Zp.tolist() == [0] * 6 and len(Zj) == 0
    Zp, Zj, _, _, _ = ex.extract(0, 0, np.zeros(1, np.int32), np.zeros(0, np.int32))
    assert Zp.tolist() == [0] and len(Zj) == 0


def test_extractref_names_what_must_be_refused():
    assert ex.invalid(5, 7, XP, XJ, TAKE_ROWS, TAKE_COLS) is None
    assert ex.invalid(5, 7, XP, XJ, [0, 5], None) == "row index out of range"
    assert ex.invalid(5, 7, XP, XJ, [-1], None) == "row index out of range"
    assert ex.invalid(5, 7, XP, XJ, None, [0, 7]) == "column index out of range"
    assert ex.invalid(5, 7, XP, XJ, None, [3, 1, 3]) == "repeated column index"
    assert ex.invalid(5, 7, XP, XJ, None, None, mI=4) == "rows NULL with mI != m"
    assert ex.invalid(5, 7, XP, XJ, None, None, nJ=6) == "cols NULL with nJ != n"
    p = XP.copy(); p[0] = 1
    assert ex.invalid(5, 7, p, XJ) == "rowPtrX[0] != 0"
    p = XP.copy(); p[-1] = 10
    assert ex.invalid(5, 7, p, XJ) == "rowPtrX[m] != nnzX"
    p = XP.copy(); p[2] = 7
    assert ex.invalid(5, 7, p, XJ, [0]) == "decreasing rowPtrX"      # (everywhere, named by rows or not)
    j = XJ.copy(); j[9] = 7
    assert ex.invalid(5, 7, XP, j) == "column of X out of range"
    assert ex.invalid(5, 7, XP, j, [0, 1, 2, 3]) is None            # (row 4 is never read)


def test_extractref_against_scipy():
    import scipy.sparse as sp
    for seed in range(12):
        rng = np.random.default_rng(300 + seed)
        m, n = int(rng.integers(1, 60)), int(rng.integers(1, 60))
        S = sp.random(m, n, density=float(rng.choice([0.05, 0.3])), format="csr", random_state=np.random.RandomState(seed))
        S.sort_indices()
        Xp, Xj, Xx = S.indptr.astype(np.int32), S.indices.astype(np.int32), S.data.copy()
        for i in range(m):                                          # the rows in a random order: the result may not depend on it
            o = rng.permutation(Xp[i + 1] - Xp[i]) + Xp[i]
            Xj[Xp[i]:Xp[i + 1]], Xx[Xp[i]:Xp[i + 1]] = Xj[o], Xx[o]
        rows = rng.integers(0, m, int(rng.integers(0, 2 * m))) if seed % 3 else rng.permutation(m)
        cols = rng.permutation(n)[:int(rng.integers(0, n + 1))]
        Zp, Zj, Zx, perm, _ = ex.extract(m, n, Xp, Xj, Xx, rows, cols)
        W = S[rows][:, cols].tocsr()
        W.sort_indices()
        assert W.shape == (len(rows), len(cols))
        assert np.array_equal(W.indptr, Zp) and np.array_equal(W.indices, Zj) and np.array_equal(W.data, Zx), seed
        assert np.array_equal(Xx[perm], Zx)
