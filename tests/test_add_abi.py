"""CPU tests of the sparse add's interfaces (bhs_csr_add_{symbolic,numeric}_device, bhs_spgemm_add[_device]): both libraries
export the entry points the header declares, the Python facades carry them, and the C++ facade's extension method compiles
and links against the C-ABI library (tests/add; tests/test_add_gpu.py runs the same binary on a GPU)."""
import ctypes as C
import os
import re
import subprocess

from conftest import ROOT

from benchmark_spgemm_using_csr_amd import _lib

ADD = ("bhs_csr_add_symbolic_device", "bhs_csr_add_numeric_device", "bhs_spgemm_add_device", "bhs_spgemm_add")
DEMO_DIR = os.path.join(ROOT, "tests", "add")


def test_header_declares_the_add_entry_points():
    txt = open(_lib.HEADER).read()
    decl = set(re.findall(r"BHS_API\s+[\w\s\*]+?\b(bhs_\w+)\s*\(", txt))
    for name in ADD:
        assert name in decl
        assert name in _lib.SYMBOLS
    assert '"add_inplace"' in txt and '"add_inplace_used"' in txt


def test_both_libraries_export_the_add_entry_points(hiplib):
    for path in (_lib.SO_PATH, _lib.SO_PATH_F32):
        raw = C.CDLL(path)
        for name in ADD:
            assert getattr(raw, name) is not None
    blob = open(_lib.SO_PATH, "rb").read()
    for kern in (b"k_add_count", b"k_add_fill", b"k_add_inplace", b"k_add_bin", b"k_add_check"):
        assert kern in blob


def test_add_sources_are_tracked_by_the_build():
    assert "bhs_add.hip.h" in _lib.SOURCES and "bhs_host_add.inc.h" in _lib.SOURCES
    mk = open(os.path.join(_lib.CSRC, "Makefile")).read()
    assert "bhs_add.hip.h" in mk and "bhs_host_add.inc.h" in mk


def test_null_handle_is_rejected_by_the_add_entry_points(hiplib):
    nnz, inside, nnzct = C.c_int(0), C.c_int(0), C.c_int64(0)
    inv = _lib.BHS_ERR_INVALID_ARG
    assert hiplib.bhs_csr_add_symbolic_device(None, 0, 0, 0, None, None, 0, None, None, None, C.byref(nnz), C.byref(inside)) == inv
    assert hiplib.bhs_csr_add_numeric_device(None, 0, 0, 1.0, 0, None, None, None, 1.0, 0, None, None, None, None, None, None,
                                             None) == inv
    assert hiplib.bhs_spgemm_add_device(None, 1.0, 1.0, 0, None, None, None, None, C.byref(nnzct), C.byref(nnz), None) == inv
    assert hiplib.bhs_spgemm_add(None, 1.0, 1.0, 0, None, None, None, None, None, None, None) == inv


def test_python_facade_has_the_add():
    from benchmark_spgemm_using_csr_amd import facade
    assert callable(getattr(facade.bhsparse, "spgemm_add", None))
    assert callable(getattr(facade.bhsparse, "spgemm_add_device", None))
    assert callable(getattr(facade, "csr_add", None))
    assert callable(getattr(facade, "spgemm_add_csr", None))


def test_cpp_facade_add_extension_builds(hiplib):
    src = open(os.path.join(ROOT, "benchmark_spgemm_using_csr_amd", "host", "bhsparse.h")).read()
    flat = re.sub(r"\s+", " ", src)
    assert ("int spgemm_add(value_type alpha, value_type beta, int nnzD, value_type *csrValD, int *csrRowPtrD, "
            "int *csrColIndD);") in flat
    subprocess.check_call(["make", "-C", DEMO_DIR, "-s"])
    demo = os.path.join(DEMO_DIR, "add_demo")
    assert os.access(demo, os.X_OK)
    out = subprocess.run(["nm", "-D", "--undefined-only", demo], capture_output=True, text=True).stdout
    assert "bhs_spgemm_add" in out
