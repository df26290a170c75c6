"""CPU tests of the masked multiply's interfaces (bhs_spgemm_masked[_device]): both libraries export the entry points the
header declares, the Python facades carry them, and the C++ facade's extension method compiles and links against the
C-ABI library (tests/masked; tests/test_masked_gpu.py runs the same binary on a GPU)."""
import ctypes as C
import os
import re
import subprocess

from conftest import ROOT

from benchmark_spgemm_using_csr_amd import _lib

MASKED = ("bhs_spgemm_masked", "bhs_spgemm_masked_device")
DEMO_DIR = os.path.join(ROOT, "tests", "masked")


def test_header_declares_the_masked_entry_points():
    txt = open(_lib.HEADER).read()
    decl = set(re.findall(r"BHS_API\s+[\w\s\*]+?\b(bhs_\w+)\s*\(", txt))
    for name in MASKED:
        assert name in decl
        assert name in _lib.SYMBOLS
    assert "masked_max_table_log2" in txt and "masked_hub_min_products" in txt


def test_both_libraries_export_the_masked_entry_points(hiplib):
    for path in (_lib.SO_PATH, _lib.SO_PATH_F32):
        raw = C.CDLL(path)
        for name in MASKED:
            assert getattr(raw, name) is not None
    blob = open(_lib.SO_PATH, "rb").read()
    for kern in (b"k_masked_scan", b"k_masked_lds", b"k_masked_long", b"k_masked_hub"):
        assert kern in blob


def test_masked_sources_are_tracked_by_the_build():
    assert "bhs_masked.hip.h" in _lib.SOURCES and "bhs_host_masked.inc.h" in _lib.SOURCES
    mk = open(os.path.join(_lib.CSRC, "Makefile")).read()
    assert "bhs_masked.hip.h" in mk and "bhs_host_masked.inc.h" in mk


def test_null_handle_is_rejected_by_the_masked_entry_points(hiplib):
    nnzct = C.c_int64(0)
    assert hiplib.bhs_spgemm_masked(None, None, None, 0, None, C.byref(nnzct), None) == _lib.BHS_ERR_INVALID_ARG
    assert hiplib.bhs_spgemm_masked_device(None, None, None, 0, None, None, None) == _lib.BHS_ERR_INVALID_ARG


def test_python_facade_has_the_masked_multiply():
    from benchmark_spgemm_using_csr_amd import facade
    assert callable(getattr(facade.bhsparse, "spgemm_masked", None))
    assert callable(getattr(facade.bhsparse, "spgemm_masked_device", None))
    assert callable(getattr(facade, "spgemm_masked_csr", None))


def test_cpp_facade_masked_extension_builds(hiplib):
    src = open(os.path.join(ROOT, "benchmark_spgemm_using_csr_amd", "host", "bhsparse.h")).read()
    flat = re.sub(r"\s+", " ", src)
    assert "int spgemm_masked(int *csrRowPtrM, int *csrColIndM, int nnzM, value_type *csrValC);" in flat
    assert "not part of the reference" in src
    subprocess.check_call(["make", "-C", DEMO_DIR, "-s"])
    demo = os.path.join(DEMO_DIR, "masked_demo")
    assert os.access(demo, os.X_OK)
    out = subprocess.run(["nm", "-D", "--undefined-only", demo], capture_output=True, text=True).stdout
    assert "bhs_spgemm_masked" in out
