"""CPU tests of the connected components (bhs_csr_components_device): the header declares the entry point and the ctypes list
matches it, both libraries export it, the build tracks the new sources and the handle keeps and releases the workspace, a
NULL handle and a handle without a platform are refused, the C++ facade's method compiles and links (tests/components;
tests/test_components_gpu.py runs the same binary on a GPU), graph.py has the calls; the numpy restatement
(tests/ccref.py) agrees with scipy on every pattern of the GPU tests and with a case written out by hand, and its
synchronous pass needs a number of rounds that only a pass with hooking and pointer jumping can reach."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import pytest
import scipy.sparse as sp
from scipy.sparse.csgraph import connected_components

from conftest import ROOT
import aggref as ar
import ccref
import scantiles as st
from test_gs_abi import kinds_of

from benchmark_spgemm_using_csr_amd import _lib

ENTRY = "bhs_csr_components_device"
FAMILIES = ("components_pass", "components_number")
FILES = ("bhs_components.hip.h", "bhs_host_components.inc.h")
DEMO_DIR = os.path.join(ROOT, "tests", "components")
# (q, c) of scantiles.cliques for the six roles of scantiles.ROLES, in that order.  The numbering scans one count per 64
# vertices (the roots among them), so T = ceil(q c / 64) counts are scanned and n = q c is chosen around 64 * SCAN_TILE.
CLIQUES = ((3, 174763), (0, 0), (3, 7), (3, 174762), (5, 314634), (3, 174740))


def scanned(q, c):
    return st.words(q * c)


# ---------------------------------------------------------------- the interfaces
def test_header_declares_the_entry_point():
    txt = open(_lib.HEADER).read()
    decl = set(re.findall(r"BHS_API\s+[\w\s\*]+?\b(bhs_\w+)\s*\(", txt))
    vp, i = C.c_void_p, C.c_int
    assert ENTRY in decl and ENTRY in _lib.SYMBOLS
    res, args = _lib.SYMBOLS[ENTRY]
    want = ["int" if t is i else "double" if t is C.c_double else "ptr" for t in args]
    assert res is i and kinds_of(txt, ENTRY) == want and len(want) == 12
    assert args[:9] == [vp, i, i, vp, vp, i, vp, vp, vp]
    sections = re.findall(r"/\* ---- ([^-]+?) -+", txt)
    assert "connected components" in sections
    at = txt.index("---- connected components")
    sect = txt[at:txt.index("/* ----", at + 1)]
    assert ENTRY in sect
    for fam in FAMILIES:
        assert fam in sect, fam
    for words in ("alues are NOT TAKEN", "WEAK connectivity", "need not be symmetric", "smallest vertex index", "function of the pattern",
                  "a word only ever falls", "atomic minimum", "hooking", "pointer jumping", "DEPENDS ON TIMING", "BHS_ERR_INTERNAL",
                  "n + 1 passes", "CAPACITY", "d_compSize without d_comp", "n == 0 succeeds", "Nothing spins",
                  "profiles/components_case.md"):
        assert words in sect, words
    host = open(os.path.join(_lib.CSRC, FILES[1])).read()
    for fam in FAMILIES:
        assert '"%s"' % fam in host, fam


def test_both_libraries_export_the_entry_point(hiplib):
    for path in (_lib.SO_PATH, _lib.SO_PATH_F32):
        raw = C.CDLL(path)
        assert getattr(raw, ENTRY) is not None
        blob = open(path, "rb").read()
        for kern in (b"k_cc_pass", b"k_cc_flag", b"k_cc_number", b"k_cc_clear"):
            assert kern in blob, (path, kern)


def test_sources_are_tracked_by_the_build():
    mk = open(os.path.join(_lib.CSRC, "Makefile")).read()
    for f in FILES:
        assert f in _lib.SOURCES and f in mk, f
    unit = open(os.path.join(_lib.CSRC, "bhsparse_hip.hip")).read()
    incs = re.findall(r'#include "(bhs_host_\w+\.inc\.h)"', unit)
    assert incs[incs.index("bhs_host_trsv.inc.h") + 1] == "bhs_host_components.inc.h"
    assert "SideWs ccWs;" in unit
    cabi = open(os.path.join(_lib.CSRC, "bhs_host_cabi.inc.h")).read()
    assert "release(h->ccWs)" in cabi
    host = open(os.path.join(_lib.CSRC, FILES[1])).read()
    assert '#include "bhs_components.hip.h"' in host and host.count("guarded(h,") == 1 and "BHS_ERR_INTERNAL" in host
    assert "kCcBatch = 8" in host and host.count("side_scan(") == 1   # the library's scan, called
    code = re.sub(r"//.*", "", open(os.path.join(_lib.CSRC, FILES[0])).read())
    assert "asm" not in code
    assert not re.search(r"\bwhile\s*\(\s*(1|true)\s*\)|for\s*\(\s*;\s*;\s*\)", code)   # nothing spins
    assert len(re.findall(r"__global__", code)) == len(re.findall(r"__global__ __launch_bounds__\(256\)", code))
    # the parents: a plain pointer where reads meet writes, and after the start no write but an atomic minimum
    assert "int* parent," in code
    pass_kernel = code[code.index("void k_cc_pass"):code.index("void k_cc_flag")]
    assert not re.search(r"parent\s*\[[^\]]*\]\s*=[^=]", pass_kernel)
    touched = pass_kernel.count("cc_load(parent + ") + pass_kernel.count("cc_lower(parent + ")
    assert pass_kernel.count("parent") == touched + 1 and pass_kernel.count("cc_lower(parent + ") >= 4   # (+ 1: the parameter)
    assert re.findall(r"\b(atomic\w+)\s*\(\s*p\b", code) == ["atomicMin"]


def test_null_handle_and_missing_platform(hiplib):
    inv = _lib.BHS_ERR_INVALID_ARG
    assert hiplib.bhs_csr_components_device(None, 0, 0, None, None, 0, None, None, None, None, None, None) == inv
    one = (C.c_int * 2)(0, 0)
    out = (C.c_int * 1)(-5)
    assert hiplib.bhs_csr_components_device(None, 1, 0, one, None, 0, out, None, None, None, None, None) == inv and out[0] == -5
    from benchmark_spgemm_using_csr_amd import facade, graph
    bh = facade.bhsparse()
    assert graph.components_raw_device(bh, 0, 0, None, None, 0, None, None, None) == _lib.BHS_ERR_NOT_READY
    assert graph.components_raw_device(bh, 1, 0, None, None, 1, None, None, None) == _lib.BHS_ERR_NOT_READY
    assert not hasattr(bh, "components_ncomp") and not hasattr(bh, "components_passes") and not hasattr(bh, "components_ms")


def test_python_module_has_the_calls():
    from benchmark_spgemm_using_csr_amd import graph
    sig = lambda f: list(inspect.signature(f).parameters)           # noqa: E731
    assert sig(graph.components_raw_device) == ["bh", "n", "nnz", "dAp", "dAj", "flags", "root", "comp", "size"]
    assert sig(graph.components_device) == ["bh", "n", "A"]
    assert sig(graph.component_lists_device) == ["bh", "n", "comp", "ncomp"]
    assert sig(graph.components_csr) == ["n", "Ap", "Aj", "device"]
    assert sig(graph.largest_component_csr)[:4] == ["n", "Ap", "Aj", "Ax"]
    assert sig(graph.bfs_levels_frontier_device) == ["bh", "n", "A", "sources", "At", "push_below"]   # as it was


def test_cpp_facade_extension_builds(hiplib):
    src = open(os.path.join(ROOT, "benchmark_spgemm_using_csr_amd", "host", "bhsparse.h")).read()
    flat = re.sub(r"\s+", " ", src)
    assert ("int csr_components_device(int n, int nnzS, const index_type *d_rowPtrS, const index_type *d_colIndS, int flags, "
            "index_type *d_root, index_type *d_comp, index_type *d_compSize, int *ncomp_out, int *passes_out);") in flat
    subprocess.check_call(["make", "-C", DEMO_DIR, "-s"])
    demo = os.path.join(DEMO_DIR, "components_demo")
    assert os.access(demo, os.X_OK)
    out = subprocess.run(["nm", "-D", "--undefined-only", demo], capture_output=True, text=True).stdout
    assert ENTRY in out
    assert "tests/components/components_demo" in open(os.path.join(ROOT, ".gitignore")).read().split()


# ---------------------------------------------------------------- the restatement
def scipy_components(n, Ap, Aj):
    """scipy's weak components, renumbered by smallest vertex"""
    k, lab = connected_components(sp.csr_matrix((np.ones(len(Aj)), Aj, Ap), shape=(n, n)), directed=True, connection="weak")
    first = np.full(k, n, np.int64)
    np.minimum.at(first, lab, np.arange(n))
    root = first[lab].astype(np.int32)
    rank = np.cumsum(root == np.arange(n)) - 1
    comp = rank[root].astype(np.int32)
    return root, comp, np.bincount(comp, minlength=k).astype(np.int32), k


def patterns():
    """name -> (n, Ap, Aj): every pattern of tests/test_components_gpu.py whose answer comes from ccref"""
    cases = dict(ar.gpu_cases())
    cases["random_directed"] = ccref.random_directed()
    cases["no_entries"] = ccref.no_entries()
    cases["star_centre_last"] = ccref.star_centre_last()
    cases["relabelled_path"] = ccref.relabelled_path()
    cases["by_hand"] = ccref.by_hand()
    cases["cliques_3_7"] = st.cliques(3, 7)[:3]
    return cases


def test_the_restatement_agrees_with_scipy():
    for name, (n, Ap, Aj) in patterns().items():
        root, comp, sizes, ncomp = ccref.components(n, Ap, Aj)
        wroot, wcomp, wsizes, wncomp = scipy_components(n, Ap, Aj)
        assert ncomp == wncomp and np.array_equal(root, wroot) and np.array_equal(comp, wcomp) and np.array_equal(sizes, wsizes), name
        assert root.dtype == comp.dtype == sizes.dtype == np.int32 and sizes.sum() == n, name
    n, Ap, Aj = ccref.random_directed()
    assert 7500 < ccref.components(n, Ap, Aj)[3] < 8500               # "about 8000 components"
    S = sp.csr_matrix((np.ones(len(Aj)), Aj, Ap), shape=(n, n))
    S.sum_duplicates()
    assert (S != S.T).nnz > 0 and S.nnz < len(Aj)                    # not symmetric, and with repeats
    n, Ap, Aj = ccref.star_centre_last()
    assert len(Aj) > 64 * n and np.diff(Ap)[n - 1] == 1023            # a whole wave a row; the centre is the last index
    assert ccref.components(n, Ap, Aj)[3] == 501


def test_the_clique_sizes_reach_the_six_roles():
    """the (q, c) pairs put the numbering's scanned count, one per 64 vertices, at scantiles.ROLES in order; the answer on
    cliques has a closed form from `members`, which the restatement confirms at a small size"""
    assert tuple(st.role_of(scanned(q, c)) for q, c in CLIQUES) == st.ROLES
    assert st.SCAN_TILE == 8192
    n, Sp, Sj, members, clique_of = st.cliques(3, 7)
    root, comp, sizes, ncomp = ccref.components(n, Sp, Sj)
    assert np.array_equal(root, members[clique_of, 0]) and ncomp == 7 and np.all(sizes == 3)
    assert np.array_equal(comp, np.argsort(np.argsort(members[:, 0]))[clique_of])


def test_the_synchronous_pass_jumps():
    """14 rounds in the issue's restatement, 11 in this one (which hooks with the row's minimum) on the relabelled path of
    32 768: at most 16, where plain minimum-label propagation needs thousands"""
    n, Ap, Aj = ccref.relabelled_path()
    passes = ccref.sync_passes(n, Ap, Aj)
    print("relabelled path of %d: %d synchronous passes" % (n, passes))
    assert passes <= 16
    n, Ap, Aj = ccref.relabelled_path(4096, 1)
    assert ccref.sync_passes(n, Ap, Aj) <= 13 and ccref.components(n, Ap, Aj)[3] == 1


def test_seven_vertices_by_hand():
    """0 -> 1 twice; 5 -> 2 and 2 -> 6 one way only; a self-loop on 3; 4 alone: {0, 1}, {2, 5, 6}, {3}, {4}"""
    n, Ap, Aj = ccref.by_hand()
    assert Ap.tolist() == [0, 2, 2, 3, 4, 4, 5, 5] and Aj.tolist() == [1, 1, 6, 3, 2]
    root, comp, sizes, ncomp = ccref.components(n, Ap, Aj)
    assert root.tolist() == [0, 0, 2, 3, 4, 2, 2]
    assert comp.tolist() == [0, 0, 1, 2, 3, 1, 1]
    assert sizes.tolist() == [2, 3, 1, 1] and ncomp == 4
    assert ccref.components(0, np.zeros(1, np.int32), np.zeros(0, np.int32))[3] == 0
