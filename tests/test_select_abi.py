"""CPU tests of the entry selection's interfaces (bhs_csr_select_{symbolic,numeric}_device, bhs_spgemm_select[_device]): both
libraries export the entry points the header declares, the Python facades carry them, the C++ facade's extension method
compiles and links against the C-ABI library (tests/select; tests/test_select_gpu.py runs the same binary on a GPU), and the
numpy restatement of the rule (tests/selectref.py) agrees with expectations written out by hand."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

from conftest import ROOT
import selectref as sr

from benchmark_spgemm_using_csr_amd import _lib

SELECT = ("bhs_csr_select_symbolic_device", "bhs_csr_select_numeric_device", "bhs_spgemm_select_device", "bhs_spgemm_select")
DEMO_DIR = os.path.join(ROOT, "tests", "select")


def test_header_declares_the_select_entry_points():
    txt = open(_lib.HEADER).read()
    decl = set(re.findall(r"BHS_API\s+[\w\s\*]+?\b(bhs_\w+)\s*\(", txt))
    for name in SELECT:
        assert name in decl
        assert name in _lib.SYMBOLS
    assert "typedef struct bhs_select" in txt and '"select_dropped"' in txt
    for flag, value in (("BAND", 1), ("DROP_DIAG", 2), ("KEEP_DIAG", 4), ("ABS", 8), ("REL", 16), ("TOPK", 32)):
        assert re.search(r"BHS_SEL_%s\s*=\s*%d\b" % (flag, value), txt), flag
        assert getattr(_lib, "BHS_SEL_" + flag) == value == getattr(sr, flag)
    assert C.sizeof(_lib.Select) == 40


def test_both_libraries_export_the_select_entry_points(hiplib):
    for path in (_lib.SO_PATH, _lib.SO_PATH_F32):
        raw = C.CDLL(path)
        for name in SELECT:
            assert getattr(raw, name) is not None
    blob = open(_lib.SO_PATH, "rb").read()
    for kern in (b"k_sel_count", b"k_sel_count_long", b"k_sel_bin", b"k_sel_fill"):
        assert kern in blob


def test_select_sources_are_tracked_by_the_build():
    assert "bhs_select.hip.h" in _lib.SOURCES and "bhs_host_select.inc.h" in _lib.SOURCES
    mk = open(os.path.join(_lib.CSRC, "Makefile")).read()
    assert "bhs_select.hip.h" in mk and "bhs_host_select.inc.h" in mk


def test_null_handle_is_rejected_by_the_select_entry_points(hiplib):
    nnz, nnzct = C.c_int(0), C.c_int64(0)
    spec = _lib.Select()
    inv = _lib.BHS_ERR_INVALID_ARG
    assert hiplib.bhs_csr_select_symbolic_device(None, 0, 0, 0, None, None, None, C.byref(spec), None, C.byref(nnz)) == inv
    assert hiplib.bhs_csr_select_numeric_device(None, 0, 0, 0, None, None, None, C.byref(spec), None, None, None, None) == inv
    assert hiplib.bhs_spgemm_select_device(None, C.byref(spec), None, C.byref(nnzct), C.byref(nnz), None) == inv
    assert hiplib.bhs_spgemm_select(None, C.byref(spec), None, None, None, None) == inv


def test_python_facade_has_the_select():
    from benchmark_spgemm_using_csr_amd import facade
    for name in ("csr_select_symbolic_device", "csr_select_numeric_device", "csr_select_device", "spgemm_select",
                 "spgemm_select_device"):
        assert callable(getattr(facade.bhsparse, name, None)), name
    assert callable(getattr(facade, "csr_select", None))
    assert callable(getattr(facade, "spgemm_select_csr", None))
    s = facade.select_spec(band=(None, -1), abs_tol=0.0, top_k=3)
    assert s.flags == 1 | 8 | 32 and s.band_lo == -2 ** 63 and s.band_hi == -1 and s.top_k == 3


def test_cpp_facade_select_extension_builds(hiplib):
    src = open(os.path.join(ROOT, "benchmark_spgemm_using_csr_amd", "host", "bhsparse.h")).read()
    flat = re.sub(r"\s+", " ", src)
    assert "int spgemm_select(const bhs_select &sel);" in flat
    subprocess.check_call(["make", "-C", DEMO_DIR, "-s"])
    demo = os.path.join(DEMO_DIR, "select_demo")
    assert os.access(demo, os.X_OK)
    out = subprocess.run(["nm", "-D", "--undefined-only", demo], capture_output=True, text=True).stdout
    assert "bhs_spgemm_select" in out


# ---------------------------------------------------------------- the reference against expectations written by hand
NAN, INF = float("nan"), float("inf")
# 6 x 6.  row 0: a tie at the cut (|v| = 5 three times); row 1: a NaN and +-0; row 2: an Inf, unsorted; row 3: empty;
# row 4: diagonal only; row 5: mixed
ROWS = [
    ([0, 1, 2, 3, 4, 5], [1.0, -5.0, 5.0, 2.0, 5.0, 7.0]),
    ([0, 1, 2, 4], [0.0, NAN, -0.0, 3.0]),
    ([5, 2, 0], [-INF, 1.0, 4.0]),
    ([], []),
    ([4], [0.5]),
    ([0, 3, 5], [8.0, -2.0, 1.0]),
]
XP = np.cumsum([0] + [len(c) for c, _ in ROWS]).astype(np.int32)
XJ = np.array([c for cs, _ in ROWS for c in cs], np.int32)
XX = np.array([v for _, vs in ROWS for v in vs], np.float64)


def run(**kw):
    Zp, Zj, Zx = sr.select(6, 6, XP, XJ, XX, sr.Spec(**kw))
    return [list(map(int, Zj[Zp[i]:Zp[i + 1]])) for i in range(6)], Zx


def test_selectref_position():
    assert run(flags=sr.BAND, band_lo=-2 ** 63, band_hi=-1)[0] == [[], [0], [0], [], [], [0, 3]]            # tril(X, -1)
    assert run(flags=sr.BAND, band_lo=0, band_hi=1)[0] == [[0, 1], [1, 2], [2], [], [4], [5]]
    assert run(flags=sr.DROP_DIAG)[0] == [[1, 2, 3, 4, 5], [0, 2, 4], [5, 0], [], [], [0, 3]]
    assert run(flags=sr.BAND, band_lo=-2 ** 63, band_hi=2 ** 63 - 1)[0] == [c for c, _ in ROWS]


def test_selectref_abs_and_rel():
    cols, vals = run(flags=sr.ABS, abs_tol=0.0)                     # +-0 go, the NaN and the Inf stay
    assert cols == [[0, 1, 2, 3, 4, 5], [1, 4], [5, 2, 0], [], [4], [0, 3, 5]]
    assert np.isnan(vals[6]) and vals[8] == -INF
    assert run(flags=sr.ABS, abs_tol=2.0)[0] == [[1, 2, 4, 5], [1, 4], [5, 0], [], [], [0]]
    # rowmax: 7, NaN (REL drops nothing), Inf (everything finite goes), -, 0.5, 8
    assert run(flags=sr.REL, rel_tol=0.5)[0] == [[1, 2, 4, 5], [0, 1, 2, 4], [5], [], [4], [0]]
    # KEEP_DIAG with REL, the strength-of-connection form: the diagonal stays and does not enter the maximum
    # row 0: max over {5, 5, 2, 5, 7}; row 1: NaN on the diagonal no longer blinds REL: max = 3; row 5: max over {8, 2}
    assert run(flags=sr.REL | sr.KEEP_DIAG, rel_tol=0.5)[0] == [[0, 1, 2, 4, 5], [1, 4], [5, 2], [], [4], [0, 5]]


def test_selectref_topk_ties_nan_and_order():
    # row 0, k = 3: 7, then the first two of the three 5s; row 1: NaN above everything; row 2: Inf first, order preserved
    assert run(flags=sr.TOPK, top_k=3)[0] == [[1, 2, 5], [0, 1, 4], [5, 2, 0], [], [4], [0, 3, 5]]
    assert run(flags=sr.TOPK, top_k=1)[0] == [[5], [1], [5], [], [4], [0]]
    assert run(flags=sr.TOPK, top_k=0)[0] == [[], [], [], [], [], []]
    # row 1 with k = 2: NaN, 3; with k = 3 the tie between +0 and -0 goes to the first
    assert run(flags=sr.TOPK, top_k=2)[0][1] == [1, 4]
    # KEEP_DIAG is not counted in top_k
    assert run(flags=sr.TOPK | sr.KEEP_DIAG, top_k=1)[0] == [[0, 5], [1, 4], [5, 2], [], [4], [0, 5]]
    # all stages: band [-5, 5], ABS 1, REL 0.5, top 2
    got = run(flags=sr.BAND | sr.ABS | sr.REL | sr.TOPK, band_lo=-5, band_hi=5, abs_tol=1.0, rel_tol=0.5, top_k=2)[0]
    assert got == [[1, 5], [1, 4], [5], [], [], [0]]


def test_selectref_keeps_bits():
    Zp, Zj, Zx = sr.select(6, 6, XP, XJ, XX.astype(np.float32), sr.Spec(flags=sr.ABS, abs_tol=0.0))
    assert Zx.dtype == np.float32 and Zp[-1] == len(Zj) == len(Zx) == 15
