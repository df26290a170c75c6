"""CPU tests of the strongly connected components (bhs_csr_scc_device): the header declares the entry point and the ctypes
list matches it, both libraries export it, the build tracks the new sources and the handle keeps and releases the workspace, a
NULL handle and a handle without a platform are refused, the C++ facade's method compiles and links (tests/scc;
tests/test_scc_gpu.py runs the same binary on a GPU), graph.py has the calls; the numpy restatement (tests/sccref.py) agrees
with scipy's strong components on every pattern of the GPU tests, with the closed forms of its own inputs and with a case
written out by hand."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import scipy.sparse as sp
from scipy.sparse.csgraph import connected_components

from conftest import ROOT
import aggref as ar
import ccref
import scantiles as st
import sccref
from test_gs_abi import kinds_of

from benchmark_spgemm_using_csr_amd import _lib

ENTRY = "bhs_csr_scc_device"
FAMILIES = ("scc_trim", "scc_forward", "scc_backward", "scc_decide", "scc_number")
KERNELS = (b"k_scc_mark", b"k_scc_trim", b"k_scc_start", b"k_scc_forward", b"k_scc_seed", b"k_scc_backward", b"k_scc_decide")
FILES = ("bhs_scc.hip.h", "bhs_host_scc.inc.h")
DEMO_DIR = os.path.join(ROOT, "tests", "scc")
# (q, c) of sccref.ring_pairs for the six roles of scantiles.ROLES, in that order.  The numbering scans one count per 64
# vertices (the roots among them), so T = ceil(q c / 64) counts are scanned and n = q c is chosen around 64 * SCAN_TILE: the
# components' own pairs, whose rings need q >= 2 or no vertex at all.
RINGS = ((3, 174763), (0, 0), (3, 7), (3, 174762), (5, 314634), (3, 174740))


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
    assert res is i and kinds_of(txt, ENTRY) == want and len(want) == 13
    assert args[:9] == [vp, i, i, vp, vp, i, vp, vp, vp]
    sections = re.findall(r"/\* ---- ([^-]+?) -+", txt)
    assert "strongly connected components" in sections
    at = txt.index("---- strongly connected components")
    sect = txt[at:txt.index("/* ----", at + 1)]
    assert ENTRY in sect
    for fam in FAMILIES:
        assert fam in sect, fam
    for words in ("alues are NOT TAKEN", "directed edge", "needs no transpose", "Rows need not be sorted", "self-loops change nothing",
                  "smallest vertex index", "function of the pattern alone", "AND *rounds_out", "ITS FIXED POINT", "Trim", "Forward labels",
                  "Backward reach", "Decide", "plain stores of one value", "A word only ever falls", "atomic minimum",
                  "Flags only rise", "DEPENDS ON TIMING", "BHS_ERR_INTERNAL", "n + 1 passes", "n + 1 rounds", "CAPACITY",
                  "d_compSize without d_comp", "n == 0 succeeds", "Nothing spins", "nothing stays queued", "profiles/scc_case.md"):
        assert words in sect, words
    host = open(os.path.join(_lib.CSRC, FILES[1])).read()
    for fam in FAMILIES:
        assert '"%s"' % fam in host, fam


def test_both_libraries_export_the_entry_point(hiplib):
    for path in (_lib.SO_PATH, _lib.SO_PATH_F32):
        raw = C.CDLL(path)
        assert getattr(raw, ENTRY) is not None
        blob = open(path, "rb").read()
        for kern in KERNELS:
            assert kern in blob, (path, kern)


def test_sources_are_tracked_by_the_build():
    mk = open(os.path.join(_lib.CSRC, "Makefile")).read()
    for f in FILES:
        assert f in _lib.SOURCES and f in mk, f
    unit = open(os.path.join(_lib.CSRC, "bhsparse_hip.hip")).read()
    incs = re.findall(r'#include "(bhs_host_\w+\.inc\.h)"', unit)
    assert incs.count("bhs_host_scc.inc.h") == 1 and incs.index("bhs_host_scc.inc.h") > incs.index("bhs_host_components.inc.h")
    assert "SideWs sccWs;" in unit
    cabi = open(os.path.join(_lib.CSRC, "bhs_host_cabi.inc.h")).read()
    assert "release(h->ccWs); release(h->sccWs)" in cabi
    host = open(os.path.join(_lib.CSRC, FILES[1])).read()
    assert '#include "bhs_scc.hip.h"' in host and host.count("guarded(h,") == 1 and "BHS_ERR_INTERNAL" in host
    assert "kSccBatch = 8" in host and host.count("side_scan(") == 1 and host.count("side_passes(") == 1 and host.count("side_rounds(") == 1
    assert "side_open(" in host and "side_aliased(" in host and "side_nothing(" in host and "with_lanes(" in host
    for kern in ("k_cc_flag", "k_cc_clear", "k_cc_number"):
        assert host.count(kern + ",") == 1, kern                     # the components' numbering, launched
    raw = open(os.path.join(_lib.CSRC, FILES[0])).read()
    assert '#include "bhs_components.hip.h"' in raw
    code = re.sub(r"//.*", "", raw)
    assert "asm" not in code
    assert not re.search(r"\bwhile\s*\(|for\s*\(\s*;\s*;\s*\)", code)   # nothing spins: no while at all
    assert len(re.findall(r"__global__", code)) == len(re.findall(r"__global__ __launch_bounds__\(256\)", code)) == len(KERNELS)
    assert "k_cc_flag" not in code and "k_cc_number" not in code    # unchanged, not copied
    # the labels: a plain pointer where reads meet writes; after the start no write but an atomic minimum
    fwd = code[code.index("void k_scc_forward"):code.index("void k_scc_seed")]
    assert "int* lab," in fwd
    assert not re.search(r"lab\s*\[[^\]]*\]\s*=[^=]", fwd)
    touched = fwd.count("cc_load(lab + ") + fwd.count("cc_lower(lab + ")
    assert fwd.count("lab") == touched + 1 and fwd.count("cc_lower(lab + ") == 2   # (+ 1: the parameter)
    assert not re.findall(r"\batomic(?!Add\b)\w+\s*\(", code)        # the file's own atomics are the counts; the minimum is cc_lower's
    comp = re.sub(r"//.*", "", open(os.path.join(_lib.CSRC, "bhs_components.hip.h")).read())
    assert "return atomicMin(p, v) > v" in comp[comp.index("cc_lower"):]
    for other in ("k_scc_mark", "k_scc_trim", "k_scc_seed", "k_scc_backward", "k_scc_decide"):
        body = code[code.index("void " + other):]
        body = body[:body.index("__global__")] if "__global__" in body else body
        assert "cc_lower" not in body and not re.search(r"\blab\s*\[[^\]]*\]\s*=[^=]", body), other
    # every row kernel loops over its blocks: the grids are capped
    assert code.count("+= gridDim.x") == len(KERNELS)


def test_null_handle_and_missing_platform(hiplib):
    inv = _lib.BHS_ERR_INVALID_ARG
    assert hiplib.bhs_csr_scc_device(None, 0, 0, None, None, 0, None, None, None, None, None, None, None) == inv
    one = (C.c_int * 2)(0, 0)
    out = (C.c_int * 1)(-5)
    counts = (C.c_int * 3)(-5, -5, -5)
    at = lambda k: C.cast(C.byref(counts, 4 * k), C.POINTER(C.c_int))   # noqa: E731
    assert hiplib.bhs_csr_scc_device(None, 1, 0, one, None, 0, out, None, None, at(0), at(1), at(2), None) == inv
    assert out[0] == -5 and list(counts) == [-5, -5, -5]
    from benchmark_spgemm_using_csr_amd import facade, graph
    bh = facade.bhsparse()
    assert graph.scc_raw_device(bh, 0, 0, None, None, 0, None, None, None) == _lib.BHS_ERR_NOT_READY
    assert graph.scc_raw_device(bh, 1, 0, None, None, 1, None, None, None) == _lib.BHS_ERR_NOT_READY
    for name in ("scc_nscc", "scc_rounds", "scc_passes", "scc_ms"):
        assert not hasattr(bh, name), name


def test_python_module_has_the_calls():
    from benchmark_spgemm_using_csr_amd import graph
    sig = lambda f: list(inspect.signature(f).parameters)           # noqa: E731
    assert sig(graph.scc_raw_device) == ["bh", "n", "nnz", "dAp", "dAj", "flags", "root", "comp", "size"]
    assert sig(graph.scc_device) == ["bh", "n", "A"]
    assert sig(graph.scc_csr) == ["n", "Ap", "Aj", "device"]
    assert sig(graph.condensation_device) == ["bh", "n", "A", "comp", "nscc"]
    assert sig(graph.largest_scc_csr)[:4] == ["n", "Ap", "Aj", "Ax"]
    assert sig(graph.component_lists_device) == ["bh", "n", "comp", "ncomp"]     # as it was: it serves the SCCs' lists
    assert sig(graph.components_raw_device) == ["bh", "n", "nnz", "dAp", "dAj", "flags", "root", "comp", "size"]


def test_cpp_facade_extension_builds(hiplib):
    src = open(os.path.join(ROOT, "benchmark_spgemm_using_csr_amd", "host", "bhsparse.h")).read()
    flat = re.sub(r"\s+", " ", src)
    assert ("int csr_scc_device(int n, int nnzS, const index_type *d_rowPtrS, const index_type *d_colIndS, int flags, "
            "index_type *d_root, index_type *d_comp, index_type *d_compSize, int *nscc_out, int *rounds_out, int *passes_out);") in flat
    subprocess.check_call(["make", "-C", DEMO_DIR, "-s"])
    demo = os.path.join(DEMO_DIR, "scc_demo")
    assert os.access(demo, os.X_OK)
    out = subprocess.run(["nm", "-D", "--undefined-only", demo], capture_output=True, text=True).stdout
    assert ENTRY in out
    assert "tests/scc/scc_demo" in open(os.path.join(ROOT, ".gitignore")).read().split()
    main = open(os.path.join(DEMO_DIR, "scc_demo.cpp")).read()
    assert "3000" in main and "PASS" in main and "lowlink" in main  # a host Tarjan of its own


# ---------------------------------------------------------------- the restatement
def scipy_scc(n, Ap, Aj):
    """scipy's strong components on the canonical matrix (it does not return on repeated entries), renumbered by smallest
    vertex"""
    Aj = Aj[:Ap[n]]                                                   # (entries behind rowPtr[n] are not the pattern's)
    S = sp.csr_matrix((np.ones(len(Aj)), Aj, Ap), shape=(n, n), copy=True)
    S.sum_duplicates()                                                # (in place: on a copy, the patterns are shared)
    k, lab = connected_components(S, directed=True, connection="strong")
    first = np.full(k, n, np.int64)
    np.minimum.at(first, lab, np.arange(n))
    root = first[lab].astype(np.int32)
    rank = np.cumsum(root == np.arange(n)) - 1
    comp = rank[root].astype(np.int32)
    return root, comp, np.bincount(comp, minlength=k).astype(np.int32), k


def patterns():
    """name -> (n, Ap, Aj): every pattern of tests/test_scc_gpu.py whose answer comes from sccref"""
    cases = dict(ar.gpu_cases())
    cases["random_directed"] = ccref.random_directed()
    cases["no_entries"] = ccref.no_entries()
    cases["star_centre_last"] = ccref.star_centre_last()
    cases["ccref_by_hand"] = ccref.by_hand()
    cases["relabelled_path_4096"] = ccref.relabelled_path(4096, 1)
    cases["random_30000"] = sccref.random_graph(20000, 30000, 21)
    cases["random_60000"] = sccref.random_graph(20000, 60000, 22)
    cases["one_way_path"] = sccref.one_way_path()
    cases["one_way_ring"] = sccref.one_way_ring()
    cases["by_hand"] = sccref.by_hand()
    cases["ring_chain_up"] = sccref.ring_chain(5, 6, True)
    cases["ring_chain_down"] = sccref.ring_chain(5, 6, False)
    cases["ring_chain_70"] = sccref.ring_chain(70, 3, True)
    cases["ring_pairs_3_7"] = sccref.ring_pairs(3, 7)[:3]
    return cases


def test_the_restatement_agrees_with_scipy():
    for name, (n, Ap, Aj) in patterns().items():
        root, comp, sizes, nscc, rounds = sccref.scc(n, Ap, Aj)
        wroot, wcomp, wsizes, wnscc = scipy_scc(n, Ap, Aj)
        assert nscc == wnscc and np.array_equal(root, wroot) and np.array_equal(comp, wcomp) and np.array_equal(sizes, wsizes), name
        assert root.dtype == comp.dtype == sizes.dtype == np.int32 and sizes.sum() == n and rounds >= 1, name
        # the direction does not matter
        troot, tcomp, tsizes, tnscc, _ = sccref.scc(*sccref.transposed(n, Ap, Aj))
        assert tnscc == nscc and np.array_equal(troot, root) and np.array_equal(tcomp, comp) and np.array_equal(tsizes, sizes), name
    assert sccref.scc(*sccref.one_way_path())[3] == 3000 and sccref.scc(*sccref.one_way_ring())[3:] == (1, 1)
    assert sccref.scc(*sccref.random_graph(20000, 30000, 21))[3] > 10000 > sccref.scc(*sccref.random_graph(20000, 60000, 22))[3] > 1000
    assert sccref.scc(0, np.zeros(1, np.int32), np.zeros(0, np.int32))[3:] == (0, 0)


def test_a_weak_answer_is_another():
    """the inputs on which the connected components' answer fails"""
    for n, Ap, Aj in (sccref.by_hand(), sccref.ring_chain(5, 6, True), sccref.ring_chain(5, 6, False)):
        assert sccref.scc(n, Ap, Aj)[3] > ccref.components(n, Ap, Aj)[3]


def test_ring_chains_take_their_rounds():
    for q, c, ascending in ((5, 6, True), (5, 6, False), (70, 3, True)):
        got = sccref.scc(*sccref.ring_chain(q, c, ascending))
        want = sccref.ring_chain_answer(q, c, ascending)
        assert all(np.array_equal(a, b) for a, b in zip(got, want)), (q, c, ascending)
    assert sccref.scc(*sccref.ring_chain(5, 6, True))[4] == 6 and sccref.scc(*sccref.ring_chain(5, 6, False))[4] == 1
    n, Ap, Aj = sccref.ring_chain(70, 3, True)
    assert n == 210 and len(Aj) == n + 2


def test_the_ring_sizes_reach_the_six_roles():
    """the (q, c) pairs put the numbering's scanned count, one per 64 vertices, at scantiles.ROLES in order; the answer on
    ring pairs has a closed form from `members`, which the restatement confirms at small sizes"""
    assert tuple(st.role_of(scanned(q, c)) for q, c in RINGS) == st.ROLES
    assert st.SCAN_TILE == 8192 and all(q >= 2 or q * c == 0 for q, c in RINGS)
    for q, c in ((3, 7), (5, 40), (33, 9), (2, 2)):
        n, Sp, Sj, members, _ = sccref.ring_pairs(q, c)
        got = sccref.scc(n, Sp, Sj)
        want = sccref.ring_pairs_answer(q, c)
        assert all(np.array_equal(a, b) for a, b in zip(got, want)), (q, c)
        assert got[3] == c and np.all(got[2] == q) and len(Sj) == n + c // 2
    assert sccref.ring_pairs_answer(3, 7)[4] == 2                     # (a bridge from the smaller ring: a second round)
    assert sccref.ring_pairs(0, 0)[0] == 0 and sccref.ring_pairs_answer(0, 0)[3:] == (0, 0)


def test_nine_vertices_by_hand():
    """{0, 1, 2} feeds {3, 4}: two rounds; 5 (a self-loop, nothing enters), 6 (isolated), 7 and 8 (a one-way tail) are trimmed"""
    n, Ap, Aj = sccref.by_hand()
    assert n == 9 and Ap.tolist() == [0, 2, 3, 5, 6, 8, 10, 10, 11, 11] and Aj.tolist() == [1, 1, 2, 0, 3, 4, 3, 7, 5, 3, 8]
    root, comp, sizes, nscc, rounds = sccref.scc(n, Ap, Aj)
    assert root.tolist() == sccref.BY_HAND_ROOT == [0, 0, 0, 3, 3, 5, 6, 7, 8]
    assert comp.tolist() == sccref.BY_HAND_COMP == [0, 0, 0, 1, 1, 2, 3, 4, 5]
    assert sizes.tolist() == sccref.BY_HAND_SIZES == [3, 2, 1, 1, 1, 1] and nscc == 6 and rounds == 2
