"""CPU tests of the transpose's interfaces (bhs_csr_transpose_device, bhs_csr_transpose_values_device): both libraries export
the entry points the header declares, the build tracks the new sources, the Python facades carry them, the C++ facade's
extension method compiles and links against the C-ABI library (tests/transpose; tests/test_transpose_gpu.py runs the same
binary on a GPU), and the numpy restatement (tests/transposeref.py) agrees with a case written out by hand."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

from conftest import ROOT
import transposeref as tr

from benchmark_spgemm_using_csr_amd import _lib

TRANSPOSE = ("bhs_csr_transpose_device", "bhs_csr_transpose_values_device")
DEMO_DIR = os.path.join(ROOT, "tests", "transpose")


def test_header_declares_the_transpose_entry_points():
    txt = open(_lib.HEADER).read()
    decl = set(re.findall(r"BHS_API\s+[\w\s\*]+?\b(bhs_\w+)\s*\(", txt))
    for name in TRANSPOSE:
        assert name in decl
        assert name in _lib.SYMBOLS
    assert len(_lib.SYMBOLS["bhs_csr_transpose_device"][1]) == 12
    assert len(_lib.SYMBOLS["bhs_csr_transpose_values_device"][1]) == 6
    assert "---- transpose" in txt
    for fam in ("transpose_count", "transpose_scan", "transpose_scatter", "transpose_short", "transpose_wave", "transpose_long",
                "transpose_values"):
        assert fam in txt, fam


def test_both_libraries_export_the_transpose_entry_points(hiplib):
    for path in (_lib.SO_PATH, _lib.SO_PATH_F32):
        raw = C.CDLL(path)
        for name in TRANSPOSE:
            assert getattr(raw, name) is not None
        blob = open(path, "rb").read()
        for kern in (b"k_tr_count", b"k_tr_scatter", b"k_tr_fill_short", b"k_tr_fill_wave", b"k_tr_fill_long", b"k_tr_values"):
            assert kern in blob, (path, kern)


def test_transpose_sources_are_tracked_by_the_build():
    assert "bhs_transpose.hip.h" in _lib.SOURCES and "bhs_host_transpose.inc.h" in _lib.SOURCES
    mk = open(os.path.join(_lib.CSRC, "Makefile")).read()
    assert "bhs_transpose.hip.h" in mk and "bhs_host_transpose.inc.h" in mk
    unit = open(os.path.join(_lib.CSRC, "bhsparse_hip.hip")).read()
    kernel_includes = re.findall(r'#include "(bhs_\w+\.hip\.h)"', unit)
    assert kernel_includes[-1] == "bhs_transpose.hip.h"             # (last: the kernels before it keep their place)


def test_null_handle_is_rejected_by_the_transpose_entry_points(hiplib):
    inv = _lib.BHS_ERR_INVALID_ARG
    assert hiplib.bhs_csr_transpose_device(None, 0, 0, 0, None, None, None, None, None, None, None, None) == inv
    assert hiplib.bhs_csr_transpose_values_device(None, 0, None, None, None, None) == inv


def test_python_facade_has_the_transpose():
    from benchmark_spgemm_using_csr_amd import facade
    for name in ("csr_transpose_device", "csr_transpose_values_device", "csr_transpose_raw_device"):
        assert callable(getattr(facade.bhsparse, name, None)), name
    assert callable(getattr(facade, "csr_transpose", None))
    assert callable(getattr(facade, "galerkin_csr", None))
    assert facade.bhsparse().transpose_ms == 0.0


def test_cpp_facade_transpose_extension_builds(hiplib):
    src = open(os.path.join(ROOT, "benchmark_spgemm_using_csr_amd", "host", "bhsparse.h")).read()
    flat = re.sub(r"\s+", " ", src)
    assert ("int csr_transpose_device(int m, int n, int nnzX, const value_type *d_valX, const index_type *d_rowPtrX, "
            "const index_type *d_colIndX, index_type *d_rowPtrT, index_type *d_colIndT, value_type *d_valT, "
            "index_type *d_perm);") in flat
    subprocess.check_call(["make", "-C", DEMO_DIR, "-s"])
    demo = os.path.join(DEMO_DIR, "transpose_demo")
    assert os.access(demo, os.X_OK)
    out = subprocess.run(["nm", "-D", "--undefined-only", demo], capture_output=True, text=True).stdout
    assert "bhs_csr_transpose_device" in out


# ---------------------------------------------------------------- the reference against a case written out by hand
# 5 x 7.  row 0 unsorted with the pair (0, 2) twice; row 1 empty; column 4 empty; a NaN with a payload and a -0.
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


def test_transposeref_by_hand():
    Tp, Tj, Tx, perm = tr.transpose(5, 7, XP, XJ, XX)
    assert Tp.dtype == np.int32 and Tj.dtype == np.int32 and perm.dtype == np.int32 and Tx.dtype == np.float64
    assert Tp.tolist() == [0, 2, 3, 6, 7, 7, 9, 11]                  # column 4: empty
    assert Tj.tolist() == [0, 3, 2, 0, 0, 3, 3, 0, 4, 2, 4]
    assert perm.tolist() == [2, 6, 4, 1, 3, 7, 8, 0, 10, 5, 9]
    # the duplicate pair (0, 2): 2.0 came first in X and comes first in row 2 of T
    want = np.array([3.0, NAN_PAYLOAD, -0.0, 2.0, 4.0, 6.0, 7.0, 1.0, 9.0, 5.0, 8.0])
    assert np.array_equal(Tx.view(np.uint64), want.view(np.uint64))
    assert Tx.view(np.uint64)[1] == 0x7FF8000000000ABC and Tx.view(np.uint64)[2] == 0x8000000000000000
    assert np.array_equal(Tx.view(np.uint64), XX[perm].view(np.uint64))


def test_transposeref_float_pattern_only_and_empty():
    Tp, Tj, Tx, perm = tr.transpose(5, 7, XP, XJ, XX.astype(np.float32))
    assert Tx.dtype == np.float32 and len(Tx) == 11
    Tp2, Tj2, none, perm2 = tr.transpose(5, 7, XP, XJ)
    assert none is None and np.array_equal(Tp, Tp2) and np.array_equal(Tj, Tj2) and np.array_equal(perm, perm2)
    Tp, Tj, Tx, perm = tr.transpose(0, 3, np.zeros(1, np.int32), np.zeros(0, np.int32), np.zeros(0))
    assert Tp.tolist() == [0, 0, 0, 0] and len(Tj) == len(Tx) == len(perm) == 0
    Tp, Tj, Tx, perm = tr.transpose(3, 0, np.zeros(4, np.int32), np.zeros(0, np.int32), np.zeros(0))
    assert Tp.tolist() == [0]


def test_transposeref_twice_is_the_row_sorted_matrix():
    Tp, Tj, Tx, _ = tr.transpose(5, 7, XP, XJ, XX)
    Up, Uj, Ux, _ = tr.transpose(7, 5, Tp, Tj, Tx)
    Sj, Sx = tr.sort_rows(5, XP, XJ, XX)
    assert np.array_equal(Up, XP) and np.array_equal(Uj, Sj) and np.array_equal(Ux.view(np.uint64), Sx.view(np.uint64))
    assert Sj[:4].tolist() == [0, 2, 2, 5] and Sx[:4].tolist() == [3.0, 2.0, 4.0, 1.0]
