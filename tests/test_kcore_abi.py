"""CPU tests of the k-core decomposition (bhs_csr_kcore_device): the header declares the entry point in its section and the
ctypes list matches it, both libraries export it, the build tracks the two new sources and the handle keeps and releases the
workspace, a NULL handle and a handle without a platform are refused, the C++ facade's method compiles and links (tests/kcore;
tests/test_kcore_gpu.py runs the same binary on a GPU), graph.py has the calls; the numpy restatement (tests/coreref.py) agrees
with networkx's core_number and with its own bucket peel on every input of the GPU tests, meets the closed forms, and its
k-truss agrees with networkx's k_truss edge sets.

The issue's figures for its uniform graph (kmax 5, 22 rounds) and its R-MAT-like graph (kmax 42, 105 rounds, 38 levels) are
those of a generator and seed it does not give; coreref's seeded graphs have kmax 5 in 24 rounds and kmax 65 in 127 rounds
over 48 levels with a row of 1291, asserted below.  The closed forms are the issue's."""
import ctypes as C
import inspect
import os
import re
import subprocess

import networkx as nx
import numpy as np
import pytest

from conftest import ROOT
import coreref as R
import gridpass as gp
from test_gs_abi import kinds_of

from benchmark_spgemm_using_csr_amd import _lib

ENTRY = "bhs_csr_kcore_device"
FAMILIES = ("kcore_check", "kcore_peel", "kcore_advance")
KERNELS = (b"k_core_begin", b"k_core_peel", b"k_core_min", b"k_core_gather", b"k_core_advance")
FILES = ("bhs_kcore.hip.h", "bhs_host_kcore.inc.h")
DEMO_DIR = os.path.join(ROOT, "tests", "kcore")


# ---------------------------------------------------------------- the interfaces
def test_header_declares_the_entry_point():
    txt = open(_lib.HEADER).read()
    decl = set(re.findall(r"BHS_API\s+[\w\s\*]+?\b(bhs_\w+)\s*\(", txt))
    vp, i = C.c_void_p, C.c_int
    assert ENTRY in decl and ENTRY in _lib.SYMBOLS
    res, args = _lib.SYMBOLS[ENTRY]
    want = ["int" if t is i else "double" if t is C.c_double else "ptr" for t in args]
    assert res is i and kinds_of(txt, ENTRY) == want and len(want) == 11
    assert args[:8] == [vp, i, i, vp, vp, i, vp, vp]
    assert txt.count("/* ---- k-core decomposition -") == 1
    at = txt.index("---- k-core decomposition")
    sect = txt[at:txt.index("/* ----", at + 1)]
    assert ENTRY in sect
    for fam in FAMILIES:
        assert fam in sect, fam
    flat = re.sub(r"\s*\n \*\s*", " ", sect)                          # (the comment's line breaks)
    for words in ("alues are NOT TAKEN", "STRICTLY ASCENDING", "STRUCTURALLY SYMMETRIC", "allowed and ignored", "binary search",
                  "k_r = max(k_{r-1}, the smallest degree among the vertices still present)", "SIMULTANEOUSLY", "core = k_r and round = r",
                  "the degeneracy", "core_number", "BEFORE d_core or d_round is written", "nothing stays queued", "flags other than 0",
                  "n == 0 succeeds", "function of the pattern alone", "DEPENDS ON TIMING", "NOT AN OUTPUT", "old == k + 1",
                  "atomicSub(deg + u, 1), unconditionally", "plain stores", "exactly once", "level jump", "ONE thread",
                  "8 passes a control round trip", "BHS_ERR_INTERNAL when more than n + 1 passes", "Nothing spins",
                  "no output is written by an atomic", "profiles/kcore_case.md", "DESIGN.md 4.27"):
        assert words in flat, words
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
    assert incs.count("bhs_host_kcore.inc.h") == 1 and incs.index("bhs_host_kcore.inc.h") > incs.index("bhs_host_side.inc.h")
    assert "SideWs coreWs;" in unit
    cabi = open(os.path.join(_lib.CSRC, "bhs_host_cabi.inc.h")).read()
    assert "release(h->coreWs)" in cabi
    host = open(os.path.join(_lib.CSRC, FILES[1])).read()
    assert '#include "bhs_kcore.hip.h"' in host and host.count("guarded(h,") == 1 and "BHS_ERR_INTERNAL" in host
    assert "kCoreBatch = 8" in host and host.count("side_passes(") == 1 and host.count("with_lanes(") == 2
    assert "side_open(" in host and "side_aliased(" in host and "side_nothing(" in host
    assert "side_end(" in host and host.count("side_read_ctl(") == 1 and "side_close(" in host   # the loop's round trips, and the close
    assert host.count("k_rcm_check<") == 1 and "rcmWs" not in host   # the check's kernel under this call's record and workspace
    raw = open(os.path.join(_lib.CSRC, FILES[0])).read()
    assert '#include "bhs_rcm.hip.h"' in raw
    code = re.sub(r"//.*", "", raw)
    assert "asm" not in code and "k_rcm_check" not in code            # included, not copied
    assert not re.search(r"\bwhile\s*\(|for\s*\(\s*;\s*;\s*\)", code)   # nothing spins: no while at all
    assert len(re.findall(r"__global__", code)) == len(KERNELS)
    assert code.count("+= gridDim.x") == 3                            # the peel, the minimum and the gather loop over their blocks
    assert sorted(set(re.findall(r"\batomic\w+", code))) == ["atomicAdd", "atomicMin", "atomicOr", "atomicSub"]
    for out in ("core", "round"):                                     # no output is written by an atomic
        assert not re.search(r"atomic\w+\(\s*&?\s*%s\b" % out, code), out
    drop = code[code.index("void core_drop"):code.index("void k_core_peel")]
    assert "atomicSub(deg + u, 1)" in drop and "old != k + 1" in drop and "core[u] = k;" in drop
    peel = code[code.index("void k_core_peel"):code.index("void k_core_min")]
    assert peel.count("core_drop(") == 2 and peel.count("__syncthreads()") == 3 and "kCoreLong * L" in peel   # a long row: a wave
    advance = code[code.index("void k_core_advance"):]
    assert "blockIdx.x != 0 || threadIdx.x != 0" in advance           # one thread


def test_null_handle_and_missing_platform(hiplib):
    inv = _lib.BHS_ERR_INVALID_ARG
    assert hiplib.bhs_csr_kcore_device(None, 0, 0, None, None, 0, None, None, None, None, None) == inv
    one = (C.c_int * 2)(0, 0)
    out = (C.c_int * 1)(-5)
    counts = (C.c_int * 2)(-5, -5)
    at = lambda k: C.cast(C.byref(counts, 4 * k), C.POINTER(C.c_int))   # noqa: E731
    assert hiplib.bhs_csr_kcore_device(None, 1, 0, one, None, 0, out, None, at(0), at(1), None) == inv
    assert out[0] == -5 and list(counts) == [-5] * 2
    from benchmark_spgemm_using_csr_amd import facade, graph
    bh = facade.bhsparse()
    assert graph.kcore_raw_device(bh, 0, 0, None, None, 0, None, None) == _lib.BHS_ERR_NOT_READY
    assert graph.kcore_raw_device(bh, 1, 0, None, None, 7, None, None) == _lib.BHS_ERR_NOT_READY
    for name in ("kcore_kmax", "kcore_rounds", "kcore_ms"):
        assert not hasattr(bh, name), name


def test_python_module_has_the_calls():
    from benchmark_spgemm_using_csr_amd import graph
    sig = lambda f: list(inspect.signature(f).parameters)           # noqa: E731
    assert sig(graph.kcore_raw_device) == ["bh", "n", "nnz", "dAp", "dAj", "flags", "core", "round"]
    assert sig(graph.kcore_device) == ["bh", "n", "A"]
    assert sig(graph.kcore_csr) == ["n", "Ap", "Aj", "device"]
    assert sig(graph.degeneracy_order_device) == ["round"]
    assert sig(graph.kcore_subgraph_device) == ["bh", "n", "A", "core", "k"]
    assert sig(graph.ktruss_device) == ["bh", "n", "A", "k"]
    assert sig(graph.ktruss_csr)[:4] == ["n", "Ap", "Aj", "k"]
    src = inspect.getsource(graph.ktruss_device)
    assert "BHS_SR_PLUS_PAIR" in src and "csr_select_device" in src and "2.5" in src and "BHS_SEL_DROP_DIAG" in src


def test_cpp_facade_extension_builds(hiplib):
    src = open(os.path.join(ROOT, "benchmark_spgemm_using_csr_amd", "host", "bhsparse.h")).read()
    flat = re.sub(r"\s+", " ", src)
    assert ("int csr_kcore_device(int n, int nnzS, const index_type *d_rowPtrS, const index_type *d_colIndS, int flags, "
            "index_type *d_core, index_type *d_round, int *kmax_out, int *rounds_out);") in flat
    subprocess.check_call(["make", "-C", DEMO_DIR, "-s"])
    demo = os.path.join(DEMO_DIR, "kcore_demo")
    assert os.access(demo, os.X_OK)
    out = subprocess.run(["nm", "-D", "--undefined-only", demo], capture_output=True, text=True).stdout
    assert ENTRY in out
    assert "tests/kcore/kcore_demo" in open(os.path.join(ROOT, ".gitignore")).read().split()
    main = open(os.path.join(DEMO_DIR, "kcore_demo.cpp")).read()
    assert "1443" in main and "PASS" in main and "bucket peel" in main   # a host bucket peel of its own
    assert '"kcore"' in open(os.path.join(ROOT, "__graft_entry__.py")).read()


# ---------------------------------------------------------------- the restatement
def graph_of(n, Sp, Sj):
    G = nx.Graph()
    G.add_nodes_from(range(n))
    r, c = R.pairs_of(n, Sp, Sj)
    G.add_edges_from(zip(r[r < c].tolist(), c[r < c].tolist()))
    return G


def edges_of(n, Tp, Tj):
    r, c = R.pairs_of(n, Tp, Tj)
    return set(zip(r[r < c].tolist(), c[r < c].tolist()))


@pytest.mark.parametrize("name", R.CASES)
def test_the_restatement_equals_networkx_and_the_bucket_peel(name):
    n, Sp, Sj = R.case(name)
    assert R.refusal(n, Sp, Sj) is None
    core, rnd, kmax, rounds = R.answer(name)
    cn = nx.core_number(graph_of(n, Sp, Sj))
    assert np.array_equal(core, np.array([cn[v] for v in range(n)], np.int32)), name
    assert np.array_equal(core, R.bucket_peel(n, Sp, Sj)), name
    assert core.dtype == rnd.dtype == np.int32 and kmax == core.max() and rounds == rnd.max() and rnd.min() == 1
    assert len(np.unique(rnd)) == rounds                              # no round is empty
    order = np.lexsort((np.arange(n), rnd))                           # the degeneracy ordering's property
    assert np.all(R.later_neighbours(n, Sp, Sj, order) <= core)
    if name in R.CLOSED:
        assert (set(core.tolist()), kmax, rounds) == R.CLOSED[name][1:], name


def test_the_closed_forms_vertex_by_vertex():
    """before the relabelling, where a vertex's place says what it is"""
    core, rnd, kmax, rounds = R.peel(*R.cliques((3, 7, 7, 20)))
    assert core.tolist() == [2] * 3 + [6] * 14 + [19] * 20 and rnd.tolist() == [1] * 3 + [2] * 14 + [3] * 20
    core, rnd, kmax, rounds = R.peel(*R.hub())
    assert core.tolist() == [2, 2, 2] + [1] * 1000 + [0, 0] and rnd.tolist() == [3, 3, 3] + [2] * 1000 + [1, 1]
    assert np.diff(R.hub()[1])[0] == 1002                             # the hub's degree falls from 1002 to 2 in one round
    core, rnd, kmax, rounds = R.peel(*R.leaves3())
    assert core.tolist() == [1, 1, 1, 1] and rnd.tolist() == [2, 1, 1, 1] and (kmax, rounds) == (1, 2)
    core, rnd, kmax, rounds = R.peel(*R.path(7))
    assert rnd.tolist() == [1, 2, 3, 4, 3, 2, 1] and (kmax, rounds) == (1, 4)
    core, rnd, kmax, rounds = R.peel(*R.grid5(5))
    assert set(core.tolist()) == {2} and rounds == 5 and rnd[12] == 5 and rnd[0] == 1
    assert R.peel(0, np.zeros(1, np.int32), np.zeros(0, np.int32))[2:] == (0, 0)
    pattern, core = R.cliques35(gp.cap_rows(1, 1))                    # the capped case of the GPU tests at one CU
    got = R.peel(*pattern)
    assert np.array_equal(got[0], core) and got[2:] == (4, 2) and np.array_equal(got[1], core // 2)
    assert 256 * gp.CAP_A < (core == 2).sum() < pattern[0]            # the first frontier: more than the cap's workgroups hold
    assert R.lanes(pattern[0], len(pattern[2])) == 1


def test_the_other_inputs_are_what_the_tests_need():
    core, rnd, kmax, rounds = R.answer("uniform4096")
    assert (kmax, rounds) == (5, 24)
    core, rnd, kmax, rounds = R.answer("rmat12")
    n, Sp, Sj = R.case("rmat12")
    assert (kmax, rounds, len(np.unique(core))) == (65, 127, 48) and np.diff(Sp).max() > 1024   # level jumps and hub rows
    assert [R.lanes(R.case("band%d" % L)[0], len(R.case("band%d" % L)[2])) for L in gp.LANES] == list(gp.LANES)
    assert all(100 < R.answer("band%d" % L)[3] < 1000 for L in gp.LANES)   # the depth stays in the hundreds


def test_the_restatement_refuses_what_the_device_refuses():
    n, Sp, Sj = R.grid5(5)
    assert R.refusal(n, Sp, Sj) is None
    bad = Sj.copy(); bad[Sp[3]], bad[Sp[3] + 1] = bad[Sp[3] + 1], bad[Sp[3]]   # noqa: E702
    assert R.refusal(n, Sp, bad) == "ascending"
    q = int(np.flatnonzero(Sj[Sp[7]:Sp[8]] != 7)[0]) + Sp[7]          # one mirror entry missing
    assert R.refusal(n, np.where(np.arange(n + 1) > 7, Sp - 1, Sp), np.delete(Sj, q)) == "symmetric"
    far = Sj.copy(); far[4] = n                                      # noqa: E702
    assert R.refusal(n, Sp, far) == "column"
    assert R.refusal(n, Sp, Sj, nnz=len(Sj) - 1) == "row pointer"
    with pytest.raises(ValueError):
        R.peel(n, Sp, bad)


@pytest.mark.parametrize("k", (2, 3, 4, 5, 9))
def test_the_truss_restatement_equals_networkx(k):
    n, Sp, Sj = R.planted(1024, 8, (6, 9, 12), 21)
    Tp, Tj, sup, iterations = R.ktruss(n, Sp, Sj, k)
    if k > 2:
        assert edges_of(n, Tp, Tj) == {(min(a, b), max(a, b)) for a, b in nx.k_truss(graph_of(n, Sp, Sj), k).edges()}
        assert len(Tj) > 0 and sup.min() >= k - 2 and iterations >= 2
    else:
        assert len(Tj) == len(Sj) and iterations == 1
    assert np.array_equal(sup, R.supports(n, Tp, Tj))                 # the values are the triangle counts inside T
    assert R.refusal(n, Tp, Tj) is None                               # symmetric


def test_the_truss_of_a_clique():
    n, Sp, Sj = R.cliques((8,), diag=True)
    Tp, Tj, sup, iterations = R.ktruss(n, Sp, Sj, 8)
    assert len(Tj) == 56 and set(sup.tolist()) == {6} and iterations == 1
    Tp, Tj, sup, iterations = R.ktruss(n, Sp, Sj, 9)
    assert len(Tj) == 0 and iterations == 1
