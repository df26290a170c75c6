"""CPU tests of the assembly's interfaces (bhs_coo_assemble_device, bhs_coo_assemble_values_device): both libraries export the
entry points the header declares, the header's constants equal the binding's, the build tracks the new sources, the Python
layers carry the calls, the host refusals that need no device refuse, and the C++ facade's extension methods compile and
link against the C-ABI library (tests/assemble; tests/test_assemble_gpu.py runs the same binary on a GPU)."""
import ctypes as C
import os
import re
import subprocess

from conftest import ROOT

from benchmark_spgemm_using_csr_amd import _lib

ASSEMBLE = ("bhs_coo_assemble_device", "bhs_coo_assemble_values_device")
DEMO_DIR = os.path.join(ROOT, "tests", "assemble")
FAMILIES = ("assemble_count", "assemble_scan", "assemble_scatter", "assemble_short", "assemble_wave", "assemble_long",
            "assemble_dedupe", "assemble_values", "assemble_check")


def test_header_declares_the_assembly_entry_points():
    txt = open(_lib.HEADER).read()
    decl = set(re.findall(r"BHS_API\s+[\w\s\*]+?\b(bhs_\w+)\s*\(", txt))
    for name in ASSEMBLE:
        assert name in decl
        assert name in _lib.SYMBOLS
    assert len(_lib.SYMBOLS["bhs_coo_assemble_device"][1]) == 16
    assert len(_lib.SYMBOLS["bhs_coo_assemble_values_device"][1]) == 9
    assert "---- assembly" in txt
    for fam in FAMILIES:
        assert fam in txt, fam


def test_header_constants_equal_the_bindings():
    txt = open(_lib.HEADER).read()
    found = dict(re.findall(r"\b(BHS_COO_\w+)\s*=\s*(\d+)", txt))
    assert sorted(found) == ["BHS_COO_FIRST", "BHS_COO_IGNORE_NEGATIVE", "BHS_COO_KEEP", "BHS_COO_LAST", "BHS_COO_SUM"]
    for name, value in found.items():
        assert getattr(_lib, name) == int(value), name
    assert (_lib.BHS_COO_SUM, _lib.BHS_COO_FIRST, _lib.BHS_COO_LAST, _lib.BHS_COO_KEEP, _lib.BHS_COO_IGNORE_NEGATIVE) == (0, 1, 2, 3, 4)
    assert _lib.COO_COMBINE == {"sum": 0, "first": 1, "last": 2, "keep": 3}


def test_both_libraries_export_the_assembly_entry_points(hiplib):
    for path in (_lib.SO_PATH, _lib.SO_PATH_F32):
        raw = C.CDLL(path)
        for name in ASSEMBLE:
            assert getattr(raw, name) is not None
        blob = open(path, "rb").read()
        for kern in (b"k_as_count", b"k_as_scatter", b"k_as_sort_short", b"k_as_sort_wave", b"k_as_sort_long", b"k_as_flag", b"k_as_emit",
                     b"k_as_rowptr", b"k_as_check_map", b"k_as_values"):
            assert kern in blob, (path, kern)
        for fam in FAMILIES:
            assert fam.encode() in blob, (path, fam)


def test_assembly_sources_are_tracked_by_the_build():
    assert "bhs_assemble.hip.h" in _lib.SOURCES and "bhs_host_assemble.inc.h" in _lib.SOURCES
    mk = open(os.path.join(_lib.CSRC, "Makefile")).read()
    assert "bhs_assemble.hip.h" in mk and "bhs_host_assemble.inc.h" in mk
    unit = open(os.path.join(_lib.CSRC, "bhsparse_hip.hip")).read()
    hosts = re.findall(r'#include "(bhs_host_\w+\.inc\.h)"', unit)
    assert hosts.index("bhs_host_assemble.inc.h") == hosts.index("bhs_host_cfsplit.inc.h") + 1


def test_host_refusals_that_need_no_device(hiplib):
    inv = _lib.BHS_ERR_INVALID_ARG
    for lib in (hiplib, _lib.load(f32=True)):
        assert lib.bhs_coo_assemble_device(None, 0, 0, 0, None, None, None, 0, None, None, None, None, None, None, None, None) == inv
        assert lib.bhs_coo_assemble_values_device(None, 0, None, 0, None, None, 0, None, None) == inv


def test_python_layers_have_the_assembly():
    import benchmark_spgemm_using_csr_amd as pkg
    from benchmark_spgemm_using_csr_amd import assemble
    for name in ("coo_assemble_raw_device", "coo_assemble_device", "coo_values_device", "coo_to_csr", "canonical_csr_device",
                 "symmetric_from_edges_device"):
        assert callable(getattr(assemble, name, None)), name
        assert getattr(pkg, name) is getattr(assemble, name), name
    assert callable(assemble.coo_values_raw_device)
    import pytest
    with pytest.raises(ValueError):
        assemble._flags("mean")
    assert assemble._flags("last", True) == 6 and assemble._flags("sum") == 0


def test_cpp_facade_assembly_extension_builds(hiplib):
    src = open(os.path.join(ROOT, "benchmark_spgemm_using_csr_amd", "host", "bhsparse.h")).read()
    flat = re.sub(r"\s+", " ", src)
    assert ("int coo_assemble_device(int m, int n, int nnzIn, const index_type *d_rowInd, const index_type *d_colInd, "
            "const value_type *d_valIn, int flags, index_type *d_rowPtrZ, index_type *d_colIndZ, value_type *d_valZ, "
            "index_type *d_entryPtr, index_type *d_perm, int *nnzZ_out, int *nkept_out);") in flat
    assert ("int coo_assemble_values_device(int nnzIn, const value_type *d_valIn, int nnzZ, const index_type *d_entryPtr, "
            "const index_type *d_perm, int flags, value_type *d_valZ);") in flat
    subprocess.check_call(["make", "-C", DEMO_DIR, "-s"])
    demo = os.path.join(DEMO_DIR, "assemble_demo")
    assert os.access(demo, os.X_OK)
    out = subprocess.run(["nm", "-D", "--undefined-only", demo], capture_output=True, text=True).stdout
    assert "bhs_coo_assemble_device" in out and "bhs_coo_assemble_values_device" in out
