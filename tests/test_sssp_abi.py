"""CPU tests of the shortest paths (bhs_csr_sssp_device): the header declares the entry point in its section and the ctypes
list matches it, both libraries export it with its kernels, the build tracks the two new sources and the handle keeps and
releases the workspace, the call shapes that need no device are refused, the C++ facade's method compiles and links
(tests/sssp; tests/test_sssp_gpu.py runs the same binary on a GPU), graph.py has the calls; and the restatement
(tests/ssspref.py): its heap Dijkstra equals scipy's bit for bit in double where scipy reads the input as it is written, and
networkx's on a small graph; its synchronous bucket passes give the heap loop's bits in both value types for every delta and
under a shuffled edge order; its parents obey the rule."""
import ctypes as C
import inspect
import os
import re
import subprocess

import networkx as nx
import numpy as np
import pytest
import scipy.sparse as sp
from scipy.sparse.csgraph import dijkstra as scipy_dijkstra

from conftest import ROOT
import ssspref as R
from test_gs_abi import kinds_of

from benchmark_spgemm_using_csr_amd import _lib

ENTRY = "bhs_csr_sssp_device"
FAMILIES = ("sssp_check", "sssp_seed", "sssp_relax", "sssp_advance", "sssp_parents", "sssp_finish")
KERNELS = (b"k_sssp_check", b"k_sssp_seed", b"k_sssp_relax", b"k_sssp_min", b"k_sssp_gather", b"k_sssp_advance", b"k_sssp_parents",
           b"k_sssp_roots", b"k_sssp_finish")
FILES = ("bhs_sssp.hip.h", "bhs_host_sssp.inc.h")
DEMO_DIR = os.path.join(ROOT, "tests", "sssp")
DELTAS = (1e-3, 1.0, 1e4, np.inf)


# ---------------------------------------------------------------- the interfaces
def test_header_declares_the_entry_point():
    txt = open(_lib.HEADER).read()
    decl = set(re.findall(r"BHS_API\s+[\w\s\*]+?\b(bhs_\w+)\s*\(", txt))
    vp, i, d = C.c_void_p, C.c_int, C.c_double
    assert ENTRY in decl and ENTRY in _lib.SYMBOLS
    res, args = _lib.SYMBOLS[ENTRY]
    want = ["int" if t is i else "double" if t is d else "ptr" for t in args]
    assert res is i and kinds_of(txt, ENTRY) == want and len(want) == 15
    assert args[:12] == [vp, i, i, vp, vp, vp, i, vp, d, i, vp, vp]
    assert txt.count("/* ---- shortest paths -") == 1
    at = txt.index("---- shortest paths")
    sect = txt[at:txt.index("/* ----", at + 1)]
    assert ENTRY in sect
    flat = re.sub(r"\s*\n \*\s*", " ", sect)                          # (the comment's line breaks)
    for words in ("OUT-EDGE matrix", "edge i -> j", "Rows need not be sorted", "parallel edges", "never improves anything",
                  "+Inf never relaxes", "-0 counts as 0", "ONE rounding to value_type an edge", "MONOTONE", "min is EXACT",
                  "a textbook Dijkstra in double", "for every delta", "changes the work, never the result", "frontier Bellman-Ford",
                  "breadth-first levels", "SMALLEST u", "fl(d[u] + w) == d[v] AND d[u] < d[v]", "-1 for a source", "-2 for a reached vertex",
                  "STRICTLY SMALLER distance", "forest rooted at the sources", "sssp_buckets", "sssp_loose", "SYNCHRONOUS",
                  "NaN or negative", "BEFORE d_dist or d_parent is written", "nothing stays queued", "flags other than 0",
                  "n == 0 succeeds", "integer atomicMin is the relaxation", "EQUAL to the minimum", "empty buckets cost nothing",
                  "8 passes a control round trip", "BHS_ERR_INTERNAL when more than 2 n + 2 passes", "Nothing spins", "plain stores",
                  "profiles/sssp_case.md"):
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
    assert incs.count("bhs_host_sssp.inc.h") == 1 and incs.index("bhs_host_sssp.inc.h") == incs.index("bhs_host_kcore.inc.h") + 1
    assert "SideWs ssspWs;" in unit
    cabi = open(os.path.join(_lib.CSRC, "bhs_host_cabi.inc.h")).read()
    assert "release(h->ssspWs)" in cabi and '"sssp_buckets"' in cabi and '"sssp_loose"' in cabi
    side = open(os.path.join(_lib.CSRC, "bhs_host_side.inc.h")).read()
    assert "return side_passes_within(h, ws, n, batch, clearInts, ctlInts, passes_out, launch);" in side   # side_passes as it was
    host = open(os.path.join(_lib.CSRC, FILES[1])).read()
    assert '#include "bhs_sssp.hip.h"' in host and host.count("guarded(h,") == 1 and "BHS_ERR_INTERNAL" in host
    assert "kSsspBatch = 8" in host and host.count("side_passes_within(") == 1 and "2 * (long long)d.n + 2" in host
    assert "side_open(" in host and "side_aliased(" in host and "side_nothing(" in host
    assert "side_end(" in host and host.count("side_read_ctl(") == 1 and "side_close(" in host   # the loop's round trips, and the close
    raw = open(os.path.join(_lib.CSRC, FILES[0])).read()
    code = re.sub(r"//.*", "", raw)
    assert "asm" not in code
    assert not re.search(r"\bwhile\s*\(|for\s*\(\s*;\s*;\s*\)", code)   # nothing spins: no while at all
    assert len(re.findall(r"__global__", code)) == len(KERNELS)
    assert sorted(set(re.findall(r"\batomic\w+", code))) == ["atomicAdd", "atomicExch", "atomicMin", "atomicOr"]
    for out in ("outDist", "outPar"):                                 # no output is written by an atomic
        assert not re.search(r"atomic\w+\(\s*&?\s*%s\b" % out, code), out
        assert len(re.findall(r"\b%s\[\w+\]\s*=" % out, code)) == 1, out   # ... and by one kernel alone
    edge = code[code.index("void ss_edge"):code.index("void k_sssp_relax")]
    assert "fp contract(off)" in edge and "atomicMin(dist + u, nb)" in edge and "atomicExch(stamp + u, tag) == tag" in edge
    assert "(unsigned)at >= (unsigned)d.n" in edge
    relax = code[code.index("void k_sssp_relax"):code.index("void k_sssp_min")]
    assert relax.count("ss_edge(") == 2 and relax.count("__syncthreads()") == 3 and "kSsLong * L" in relax   # a long row: a wave
    advance = code[code.index("void k_sssp_advance"):code.index("void k_sssp_parents")]
    assert "blockIdx.x != 0 || threadIdx.x != 0" in advance           # one thread


def test_refused_call_shapes_that_need_no_device(hiplib):
    inv = _lib.BHS_ERR_INVALID_ARG
    assert hiplib.bhs_csr_sssp_device(None, 0, 0, None, None, None, 0, None, 1.0, 0, None, None, None, None, None) == inv
    one = (C.c_int * 2)(0, 0)
    src = (C.c_int * 1)(0)
    out = (C.c_double * 1)(-5.0)
    counts = (C.c_int * 2)(-5, -5)
    at = lambda k: C.cast(C.byref(counts, 4 * k), C.POINTER(C.c_int))   # noqa: E731
    assert hiplib.bhs_csr_sssp_device(None, 1, 0, one, None, None, 1, src, 1.0, 0, out, None, at(0), at(1), None) == inv
    assert out[0] == -5.0 and list(counts) == [-5] * 2
    from benchmark_spgemm_using_csr_amd import facade, graph
    bh = facade.bhsparse()
    assert graph.sssp_delta_raw_device(bh, 0, 0, None, None, None, 0, None, 1.0, 0, None, None) == _lib.BHS_ERR_NOT_READY
    assert graph.sssp_delta_raw_device(bh, 1, 0, None, None, None, 1, None, -1.0, 7, None, None) == _lib.BHS_ERR_NOT_READY
    for name in ("sssp_reached", "sssp_passes", "sssp_ms"):
        assert not hasattr(bh, name), name


def test_python_module_has_the_calls():
    from benchmark_spgemm_using_csr_amd import graph
    sig = lambda f: list(inspect.signature(f).parameters)           # noqa: E731
    assert sig(graph.sssp_delta_raw_device) == ["bh", "n", "nnz", "dGp", "dGj", "dGx", "nsrc", "dsources", "delta", "flags", "dist",
                                                "parent"]
    assert sig(graph.sssp_delta_device) == ["bh", "n", "G", "sources", "delta", "parents"]
    assert sig(graph.sssp_delta_csr)[:7] == ["n", "Gp", "Gj", "Gx", "sources", "delta", "parents"]
    assert sig(graph.path_from_parents) == ["parent", "target"]
    assert sig(graph.bfs_levels_queue_device) == ["bh", "n", "G", "sources"]
    assert "profiles/sssp_case.md" in graph.sssp_delta_device.__doc__ and "sssp_delta_" in graph.__doc__
    assert graph.path_from_parents(np.array([-1, 0, 1, -1, -2, 4]), 2) == [0, 1, 2]
    assert graph.path_from_parents(np.array([-1, 0, 1, -1, -2, 4]), 3) == [3]
    for target in (4, 5):
        with pytest.raises(ValueError):
            graph.path_from_parents(np.array([-1, 0, 1, -1, -2, 4]), target)
    with pytest.raises(ValueError):
        graph.path_from_parents(np.array([1, 0]), 0)                  # no forest: the walk is bounded


def test_cpp_facade_extension_builds(hiplib):
    src = open(os.path.join(ROOT, "benchmark_spgemm_using_csr_amd", "host", "bhsparse.h")).read()
    flat = re.sub(r"\s+", " ", src)
    assert ("int csr_sssp_device(int n, int nnzG, const index_type *d_rowPtrG, const index_type *d_colIndG, const value_type *d_valG, "
            "int nsrc, const index_type *d_sources, double delta, int flags, value_type *d_dist, index_type *d_parent, "
            "int *reached_out, int *passes_out);") in flat
    subprocess.check_call(["make", "-C", DEMO_DIR, "-s"])
    demo = os.path.join(DEMO_DIR, "sssp_demo")
    assert os.access(demo, os.X_OK)
    out = subprocess.run(["nm", "-D", "--undefined-only", demo], capture_output=True, text=True).stdout
    assert ENTRY in out
    assert "tests/sssp/sssp_demo" in open(os.path.join(ROOT, ".gitignore")).read().split()
    main = open(os.path.join(DEMO_DIR, "sssp_demo.cpp")).read()
    assert "1776" in main and "PASS" in main and "host loop" in main  # a host relaxation loop of its own
    assert '"sssp"' in open(os.path.join(ROOT, "__graft_entry__.py")).read()


# ---------------------------------------------------------------- the restatement
def test_the_heap_loop_equals_scipy_bit_for_bit():
    n, Gp, Gj, Gx = R.positive()
    assert np.all(Gx > 0) and np.all(np.isfinite(Gx)) and R.refusal(n, Gp, Gj, Gx, [0]) is None
    M = sp.csr_matrix((Gx, Gj, Gp), shape=(n, n))
    assert M.nnz == len(Gj)                                           # no repeated entry, no explicit zero: scipy reads what is written
    for s in (0, 3, n - 1):
        got = R.dijkstra(n, Gp, Gj, Gx, [s])
        assert got.tobytes() == scipy_dijkstra(M, indices=s).tobytes(), s
    both = R.dijkstra(n, Gp, Gj, Gx, [3, n - 1, 3])
    assert both.tobytes() == scipy_dijkstra(M, indices=[3, n - 1], min_only=True).tobytes()


def test_the_heap_loop_equals_networkx():
    n, Gp, Gj, Gx = R.positive(60, 3, seed=8)
    G = nx.DiGraph()
    G.add_nodes_from(range(n))
    r = np.repeat(np.arange(n), np.diff(Gp))
    G.add_weighted_edges_from(zip(r.tolist(), Gj.tolist(), Gx.tolist()))
    want = nx.single_source_dijkstra_path_length(G, 7)
    got = R.dijkstra(n, Gp, Gj, Gx, [7])
    assert {v: float(got[v]) for v in range(n) if np.isfinite(got[v])} == want


@pytest.mark.parametrize("dtype", (np.float64, np.float32), ids=("f64", "f32"))
def test_the_bucket_passes_give_dijkstras_bits_for_every_delta(dtype):
    n, Gp, Gj, Gx = R.uniform()
    src = [5, 77, 5]
    want = R.dijkstra(n, Gp, Gj, Gx, src, dtype)
    seen = set()
    for delta in DELTAS:
        dist, passes, buckets = R.simulate(n, Gp, Gj, Gx, src, delta, dtype)
        assert dist.tobytes() == want.tobytes(), delta
        assert 1 <= buckets <= passes <= 2 * n + 2
        seen.add((passes, buckets))
    assert len(seen) == len(DELTAS)                                   # delta changes the work
    assert R.simulate(n, Gp, Gj, Gx, src, np.inf, dtype)[2] == 1
    # a shuffled edge order inside the rows: the same bits
    rng = np.random.default_rng(1)
    key = np.repeat(np.arange(n), np.diff(Gp)) + rng.random(len(Gj))
    o = np.argsort(key)
    assert R.simulate(n, Gp, Gj[o], Gx[o], src, 1.0, dtype)[0].tobytes() == want.tobytes()


def test_the_inputs_are_what_the_tests_need():
    n, Gp, Gj, Gx = R.uniform()
    r = np.repeat(np.arange(n), np.diff(Gp))
    assert np.any(r == Gj) and np.any(np.diff(Gj) < 0) and np.any(np.isinf(Gx)) and np.any(np.signbit(Gx)) and np.any(Gx == 0)
    pairs = r.astype(np.int64) * n + Gj
    assert len(np.unique(pairs)) < len(pairs)                         # repeated entries
    pos = Gx[(Gx > 0) & np.isfinite(Gx)]
    assert np.log10(pos.max() / pos.min()) > 15                       # 16 decades
    for dtype in (np.float64, np.float32):
        a = R.answer(n, Gp, Gj, Gx, [5, 77, 5], 1.0, dtype)
        assert a["loose"] > 0 and a["reached"] > n // 2
        ok = a["parent"] >= 0
        assert np.all(a["dist"][a["parent"][ok]] < a["dist"][ok])     # a strictly smaller distance: a forest
    for L in (1, 4, 16, 64):
        g = R.star_padded(L)
        assert R.lanes(g[0], len(g[2])) == L and np.diff(g[1])[0] == 5000 and np.diff(g[1])[1] == 300 and 5000 > 32 * L
    a = R.answer(*R.zero_cycle(), [0], 1.0)
    assert a["parent"].tolist() == [-1, 0, -2] and a["dist"].tolist() == [0.0, 2.0, 2.0] and a["loose"] == 1
    for delta, buckets in ((1.0, 2049), (np.inf, 1), (0.25, 2049)):
        a = R.answer(*R.path(2049), [0], delta)
        assert (a["passes"], a["buckets"]) == (2049, buckets) and a["dist"][-1] == 2048.0
    a = R.answer(*R.path(2049, 1000.0), [0], 1.0)
    assert (a["passes"], a["buckets"]) == (2049, 2049) and a["dist"][-1] == 2048000.0   # the empty buckets between add no pass


def test_the_restatement_refuses_what_the_device_refuses():
    n, Gp, Gj, Gx = R.positive(60, 3, seed=8)
    assert R.refusal(n, Gp, Gj, Gx, [0]) is None
    bad = Gx.copy(); bad[5] = -1.0                                   # noqa: E702
    assert R.refusal(n, Gp, Gj, bad, [0]) == "weight"
    bad[5] = np.nan
    assert R.refusal(n, Gp, Gj, bad, [0]) == "weight"
    bad[5] = -0.0
    assert R.refusal(n, Gp, Gj, bad, [0]) is None
    c = Gj.copy(); c[9] = n                                          # noqa: E702
    assert R.refusal(n, Gp, c, Gx, [0]) == "column"
    p = Gp.copy(); p[10] = p[11] + 1                                 # noqa: E702
    assert R.refusal(n, p, Gj, Gx, [0]) == "row pointer"
    assert R.refusal(n, Gp, Gj, Gx, [0, n]) == "source"
