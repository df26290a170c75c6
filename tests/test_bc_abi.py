"""CPU tests of the betweenness centrality (bhs_csr_betweenness_device): the header declares the entry point in its section
and the ctypes list matches it, both libraries export it with its kernels, the build tracks the two new sources and the
handle keeps and releases the workspace, the call shapes that need no device are refused, the C++ facade's method compiles
and links (tests/bc; tests/test_bc_gpu.py runs the same binary on a GPU), graph.py has the calls; and the restatement
(tests/bcref.py): it equals networkx's betweenness_centrality_subset on directed, undirected and multigraph inputs within a
bound worked out below, closed forms bit for bit, and itself under a shuffle of the entries inside rows where every sum is
exact."""
import ctypes as C
import inspect
import os
import re
import subprocess

import networkx as nx
import numpy as np
import pytest

from conftest import ROOT
import bcref as R
from test_gs_abi import kinds_of

from benchmark_spgemm_using_csr_amd import _lib

ENTRY = "bhs_csr_betweenness_device"
FAMILIES = ("bc_check", "bc_seed", "bc_expand", "bc_count", "bc_back", "bc_finish")
KERNELS = (b"k_bc_check", b"k_bc_seed", b"k_bc_expand", b"k_bc_count", b"k_bc_advance", b"k_bc_back", b"k_bc_finish")
FILES = ("bhs_bc.hip.h", "bhs_host_bc.inc.h")
DEMO_DIR = os.path.join(ROOT, "tests", "bc")


# ---------------------------------------------------------------- the interfaces
def test_header_declares_the_entry_point():
    txt = open(_lib.HEADER).read()
    decl = set(re.findall(r"BHS_API\s+[\w\s\*]+?\b(bhs_\w+)\s*\(", txt))
    vp, i, d = C.c_void_p, C.c_int, C.c_double
    assert ENTRY in decl and ENTRY in _lib.SYMBOLS
    res, args = _lib.SYMBOLS[ENTRY]
    want = ["int" if t is i else "double" if t is d else "ptr" for t in args]
    assert res is i and kinds_of(txt, ENTRY) == want and len(want) == 17
    assert args[:14] == [vp, i, i, vp, vp, i, vp, vp, i, vp, i, vp, vp, vp]
    assert args[14:] == [C.POINTER(i), C.POINTER(i), C.POINTER(d)]   # the shape facade.bhsparse._counted expects
    assert txt.count("/* ---- betweenness centrality -") == 1
    at = txt.index("---- betweenness centrality")
    assert txt.index("---- shortest paths") < at < txt.index("---- spanning forest")   # placed after "shortest paths"
    sect = txt[at:txt.index("/* ----", at + 1)]
    assert ENTRY in sect and "#define BHS_BC_ACCUMULATE 1" in sect and _lib.BHS_BC_ACCUMULATE == 1
    flat = re.sub(r"\s*\n \*\s*", " ", sect)                          # (the comment's line breaks)
    for words in ("OUT-EDGE matrix", "edge i -> j", "IN-EDGES", "the SAME arrays", "Rows need not be sorted", "parallel edges",
                  "count in sigma", "Loops never qualify", "does not verify T = G^T", "out of bounds whatever T holds",
                  "a repeated source counts again", "level[s] = 0", "-1 where v is not reached", "sigma[s] = 1", "ROW v OF T",
                  "level[u] == level[v] - 1", "On the deepest level delta[u] = 0", "delta[u] = sigma[u] * S", "ROW u OF G",
                  "(1 + delta[v]) / sigma[v]", "level[v] == level[u] + 1", "a true division, contraction off",
                  "bc[u] = fl(bc[u] + delta[u])", "0 < level[u] < the deepest level", "in list order", "sigma passes 2^53",
                  "more than 32 L entries takes L_row = 64", "lane p mod L_row", "ascending p, starting from +0",
                  "t[l] = t[l] + t[l ^ off] for off = L_row / 2, ..., 1", "contributes nothing", "stays +Inf", "Inf * 0",
                  "0x7FF8000000000000", "BHS_BC_ACCUMULATE: d_bc is added to instead of zero-filled",
                  "k chained single-source calls", "of the LAST source", "a multiple of 8 per source", "bc_levels", "bc_overflow",
                  "bc_work_passes", "need no bound data", "walks entries, not rows", "writes none of d_bc, d_level, d_sigma",
                  "nothing stays queued", "flags other than BHS_BC_ACCUMULATE or 0", "Inputs may alias each other",
                  "n == 0 succeeds", "integer atomicCAS", "no atomic and ONE writer", "8 passes a control round trip",
                  "BHS_ERR_INTERNAL when more than n + 1 passes", "max(deepest - 1, 0) launches", "no round trip", "plain stores",
                  "Nothing spins", "profiles/bc_case.md"):
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
    assert incs.count("bhs_host_bc.inc.h") == 1 and incs.index("bhs_host_bc.inc.h") == incs.index("bhs_host_sssp.inc.h") + 1
    assert "SideWs bcWs;" in unit
    cabi = open(os.path.join(_lib.CSRC, "bhs_host_cabi.inc.h")).read()
    assert "release(h->bcWs)" in cabi and all('"%s"' % k in cabi for k in ("bc_levels", "bc_overflow", "bc_work_passes"))
    at = {k: cabi.index('"%s"' % k) for k in ("bc_levels", "bc_overflow", "bc_work_passes")}
    assert max(at.values()) < cabi.index("if (!h->hasData) return BHS_ERR_NOT_READY;", cabi.index("int bhs_get_info"))   # no bound data
    host = open(os.path.join(_lib.CSRC, FILES[1])).read()
    assert '#include "bhs_bc.hip.h"' in host and host.count("guarded(h,") == 1 and "BHS_ERR_INTERNAL" in host
    assert "kBcBatch = 8" in host and host.count("side_passes_within(") == 1 and "(long long)d.n + 1" in host
    assert "side_open(" in host and "side_aliased(" in host and "side_nothing(" in host
    assert "side_end(" in host and host.count("side_read_ctl(") == 1 and "side_close(" in host   # the loops' round trips, and the close
    back = host[host.index("for (int lev = deepest - 1; lev >= 1; --lev)"):host.index("return BHS_SUCCESS", host.index("for (int lev"))]
    assert "side_read_ctl" not in back and "wait_stream" not in back and "hipStreamSynchronize" not in back   # no round trip
    raw = open(os.path.join(_lib.CSRC, FILES[0])).read()
    code = re.sub(r"//.*", "", raw)
    assert "asm" not in code
    assert not re.search(r"\bwhile\s*\(|for\s*\(\s*;\s*;\s*\)", code)   # nothing spins: no while at all
    assert len(re.findall(r"__global__", code)) == len(KERNELS)
    assert sorted(set(re.findall(r"\batomic\w+", code))) == ["atomicAdd", "atomicCAS", "atomicOr"]
    for target in re.findall(r"\batomic\w+\(\s*&?\s*([\w\.]+)", code):   # integer atomics on the workspace alone
        assert target in ("ctl", "w.level", "sCount"), target
    assert "float" not in code and "value_t" not in code              # every number a double
    for body in ("double bc_fold", "double bc_term", "void k_bc_back"):
        at = code.index(body)
        assert "fp contract(off)" in code[at:at + 1500], body
    for out in ("bc", "outLevel", "outSigma"):                        # no output is written by an atomic
        assert not re.search(r"atomic\w+\(\s*&?\s*%s\b" % out, code), out
    advance = code[code.index("void k_bc_advance"):code.index("void k_bc_back")]
    assert "blockIdx.x != 0 || threadIdx.x != 0" in advance           # one thread


def test_refused_call_shapes_that_need_no_device(hiplib):
    inv = _lib.BHS_ERR_INVALID_ARG
    f = hiplib.bhs_csr_betweenness_device
    assert f(None, 0, 0, None, None, 0, None, None, 0, None, 0, None, None, None, None, None, None) == inv
    one = (C.c_int * 2)(0, 0)
    src = (C.c_int * 1)(0)
    out = (C.c_double * 1)(-5.0)
    counts = (C.c_int * 2)(-5, -5)
    at = lambda k: C.cast(C.byref(counts, 4 * k), C.POINTER(C.c_int))   # noqa: E731
    assert f(None, 1, 0, one, None, 0, one, None, 1, src, 0, out, None, None, at(0), at(1), None) == inv
    assert out[0] == -5.0 and list(counts) == [-5] * 2
    from benchmark_spgemm_using_csr_amd import facade, graph
    bh = facade.bhsparse()
    assert graph.betweenness_raw_device(bh, 0, 0, None, None, 0, None, None, 0, None, 0, None, None, None) == _lib.BHS_ERR_NOT_READY
    assert graph.betweenness_raw_device(bh, 1, 0, None, None, 0, None, None, 1, None, 7, None, None, None) == _lib.BHS_ERR_NOT_READY
    for name in ("bc_reached", "bc_passes", "bc_ms"):
        assert not hasattr(bh, name), name


def test_python_module_has_the_calls():
    from benchmark_spgemm_using_csr_amd import graph
    sig = lambda f: list(inspect.signature(f).parameters)           # noqa: E731
    assert sig(graph.betweenness_raw_device) == ["bh", "n", "nnzG", "dGp", "dGj", "nnzT", "dTp", "dTj", "nsrc", "dsources", "flags",
                                                 "bc", "level", "sigma"]
    assert sig(graph.betweenness_device) == ["bh", "n", "G", "sources", "Gt", "accumulate", "last"]
    assert sig(graph.betweenness_csr) == ["n", "Gp", "Gj", "sources", "directed", "normalized", "device"]
    assert sig(graph.betweenness_sample_csr)[:4] == ["n", "Gp", "Gj", "k"]
    assert sig(graph.closeness_device) == ["bh", "n", "G", "sources"]
    assert "profiles/bc_case.md" in graph.betweenness_device.__doc__ and "betweenness_" in graph.__doc__
    raw = np.array([0.0, 6.0, 2.0, 0.0])
    assert graph._bc_scaled(raw, 4, True, False).tolist() == raw.tolist()
    assert graph._bc_scaled(raw, 4, False, False).tolist() == [0.0, 3.0, 1.0, 0.0]          # networkx halves an undirected graph's
    assert graph._bc_scaled(raw, 4, False, True).tolist() == (raw / 6.0).tolist()           # ... and normalises by (n - 1)(n - 2)
    assert graph._bc_scaled(raw, 4, True, False, 2.0).tolist() == [0.0, 12.0, 4.0, 0.0]     # the pivots' n / k
    with pytest.raises(ValueError):
        graph.betweenness_sample_csr(4, None, None, 5)


@pytest.mark.parametrize("directed", (True, False))
@pytest.mark.parametrize("normalized", (True, False))
def test_all_vertices_as_pivots_give_the_exact_value(monkeypatch, directed, normalized):
    """the raw sums are scaled once: with k = n the estimate IS betweenness_csr's value, in all four conventions (the device
    call replaced by its raw sums, so this needs no GPU)"""
    from benchmark_spgemm_using_csr_amd import graph
    raw = np.array([0.0, 6.0, 2.0, 0.0, 7.0])
    seen = []

    def sums(n, Gp, Gj, sources, directed_, device):
        seen.append((None if sources is None else list(sources), directed_))
        return raw.copy(), {}
    monkeypatch.setattr(graph, "_betweenness_raw_csr", sums)
    exact, _ = graph.betweenness_csr(5, None, None, None, directed, normalized)
    est, info = graph.betweenness_sample_csr(5, None, None, 5, 3, directed, normalized)
    assert est.tobytes() == exact.tobytes() and info["pivots"].tolist() == list(range(5))
    assert seen == [(None, directed), (list(range(5)), directed)]     # nothing is halved before the one scaling
    want = raw / 12.0 if normalized else raw if directed else raw / 2.0   # networkx: (n - 1)(n - 2) = 12 un-halved; else halved
    assert np.allclose(exact, want, rtol=2.0 ** -52, atol=0.0)
    half, _ = graph.betweenness_sample_csr(5, None, None, 2, 3, directed, normalized)
    assert np.allclose(half, want * 2.5, rtol=2.0 ** -51, atol=0.0)   # n / k


def test_cpp_facade_extension_builds(hiplib):
    src = open(os.path.join(ROOT, "benchmark_spgemm_using_csr_amd", "host", "bhsparse.h")).read()
    flat = re.sub(r"\s+", " ", src)
    assert ("int csr_betweenness_device(int n, int nnzG, const index_type *d_rowPtrG, const index_type *d_colIndG, int nnzT, "
            "const index_type *d_rowPtrT, const index_type *d_colIndT, int nsrc, const index_type *d_sources, int flags, "
            "double *d_bc, index_type *d_level, double *d_sigma, int *reached_out, int *passes_out);") in flat
    subprocess.check_call(["make", "-C", DEMO_DIR, "-s"])
    demo = os.path.join(DEMO_DIR, "bc_demo")
    assert os.access(demo, os.X_OK)
    out = subprocess.run(["nm", "-D", "--undefined-only", demo], capture_output=True, text=True).stdout
    assert ENTRY in out
    assert "tests/bc/bc_demo" in open(os.path.join(ROOT, ".gitignore")).read().split()
    main = open(os.path.join(DEMO_DIR, "bc_demo.cpp")).read()
    assert "456" in main and "PASS" in main and "host loop" in main   # a host Brandes of its own
    assert '"bc"' in open(os.path.join(ROOT, "__graft_entry__.py")).read()
    n, Gp, Gj = R.grid_with_diagonals()                               # the restatement of the demo's graph is that graph
    assert n == 456 and R.lanes(n, len(Gj)) == 4 and Gj[:3].tolist() == [1, 24, 25]


# ---------------------------------------------------------------- the restatement against networkx
def bound(n, nnz):
    """All terms are positive, so nothing cancels, and a value passes through at most three roundings a DAG edge (the term's
    add and division, the lane's add) and one a vertex (the product) in each of the two implementations: a relative
    (3 nnz + n) 2^-52"""
    return (3 * nnz + n) * 2.0 ** -52


def nx_subset(n, r, c, sources, directed):
    G = nx.DiGraph() if directed else nx.Graph()
    G.add_nodes_from(range(n))
    G.add_edges_from(zip(r.tolist(), c.tolist()))
    got = nx.betweenness_centrality_subset(G, [int(s) for s in sources], list(range(n)), normalized=False)
    return np.array([got[v] for v in range(n)])


def close(a, b, rel, what):
    print("%s: largest relative difference %.3g, bound %.3g" % (what, np.max(np.abs(a - b) / np.maximum(np.maximum(a, b), 1e-300)), rel))
    assert np.all(np.abs(a - b) <= rel * np.maximum(a, b)), what


def test_the_restatement_equals_networkx_directed():
    rng = np.random.default_rng(21)
    n, m = 200, 1500
    r, c = rng.integers(0, n, m), rng.integers(0, n, m)
    key = np.unique(r * n + c)                                        # a simple digraph; loops stay
    r, c = key // n, key % n
    g = R.shuffled(*R.csr(n, r, c), 3)
    assert n <= 300 and len(g[2]) <= 3000 and np.any(r == c)
    a = R.answer(*g, *R.transposed(*g), np.arange(n))
    close(a["bc"], nx_subset(n, r, c, np.arange(n), True), bound(n, len(g[2])), "directed, all sources")
    some = [5, 17, 5, 150]                                            # a repeated source counts again: networkx lists it twice
    a = R.answer(*g, *R.transposed(*g), some)
    close(a["bc"], nx_subset(n, r, c, some, True), bound(n, len(g[2])), "directed, a list with a repeat")


def test_the_restatement_equals_networkx_undirected():
    rng = np.random.default_rng(22)
    n, m = 150, 600
    r, c = rng.integers(0, n, m), rng.integers(0, n, m)
    keep = r != c
    key = np.unique(np.minimum(r, c)[keep] * n + np.maximum(r, c)[keep])
    lo, hi = key // n, key % n
    g = R.shuffled(*R.csr(n, np.r_[lo, hi], np.r_[hi, lo]), 4)
    assert len(g[2]) <= 3000
    a = R.answer(*g, g[1], g[2], np.arange(n))                        # T is G
    close(0.5 * a["bc"], nx_subset(n, lo, hi, np.arange(n), False), bound(n, len(g[2])), "undirected")


def test_the_restatement_equals_networkx_with_parallel_edges():
    """networkx's MultiDiGraph walks neighbours, not edges, so parallel edges fall together there; with a vertex of its own
    on EVERY edge they are distinct paths of a simple digraph, all distances double, and the shortest paths between the
    original vertices are the multigraph's one to one"""
    rng = np.random.default_rng(23)
    n, m = 60, 300
    r, c = rng.integers(0, n, m), rng.integers(0, n, m)
    r, c = np.r_[r, r[:80]], np.r_[c, c[:80]]                         # 80 edges twice, some of them three times
    m = len(r)
    g = R.csr(n, r, c)
    pairs = r.astype(np.int64) * n + c
    assert len(np.unique(pairs)) < m - 60 and n + m <= 3000
    a = R.answer(*g, *R.transposed(*g), np.arange(n))
    mid = n + np.arange(m)
    H = nx.DiGraph()
    H.add_nodes_from(range(n + m))
    H.add_edges_from(zip(r.tolist(), mid.tolist()))
    H.add_edges_from(zip(mid.tolist(), c.tolist()))
    got = nx.betweenness_centrality_subset(H, list(range(n)), list(range(n)), normalized=False)
    close(a["bc"], np.array([got[v] for v in range(n)]), bound(n, m), "parallel edges")
    M = nx.MultiDiGraph()
    M.add_edges_from(zip(r.tolist(), c.tolist()))
    collapsed = nx.betweenness_centrality_subset(M, list(range(n)), list(range(n)), normalized=False)
    assert not np.allclose(a["bc"], [collapsed.get(v, 0.0) for v in range(n)])   # (what the subdivision is for)


# ---------------------------------------------------------------- closed forms, bit for bit
def test_closed_forms_bit_for_bit():
    n = 37
    g = R.path(n)
    a = R.answer(*g, *R.transposed(*g), np.arange(n))
    i = np.arange(n, dtype=np.float64)
    assert a["bc"].tobytes() == (i * (n - 1 - i)).tobytes()           # i sources before, n - 1 - i targets behind
    assert (a["reached"], a["levels"], a["work"]) == (n * (n + 1) // 2,) * 3 and a["overflow"] == 0
    assert a["passes"] == sum(R.launched(d) for d in range(n)) and a["backs"] == sum(max(d - 1, 0) for d in range(n))
    assert a["level"].tolist() == [-1] * (n - 1) + [0] and a["sigma"].tolist() == [0.0] * (n - 1) + [1.0]   # the last source's
    n = 50
    g = R.star(n)
    a = R.answer(*g, g[1], g[2], np.arange(n))
    assert a["bc"].tobytes() == np.r_[float((n - 1) * (n - 2)), np.zeros(n - 1)].tobytes()   # every ordered pair of leaves
    g = R.diamond()
    a = R.answer(*g, *R.transposed(*g), np.arange(5))
    assert a["bc"].tobytes() == np.array([0.0, 1.0, 1.0, 3.0, 0.0]).tobytes()
    a = R.answer(*g, *R.transposed(*g), [0])
    assert a["sigma"].tolist() == [1.0, 1.0, 1.0, 2.0, 2.0] and a["level"].tolist() == [0, 1, 1, 2, 3]
    assert a["bc"].tobytes() == np.array([0.0, 1.0, 1.0, 1.0, 0.0]).tobytes()   # delta[3] = 1, delta[1] = delta[2] = (1 + 1) / 2
    start = np.array([1.0, 2.0, 3.0, 4.0, 5.0])
    assert R.answer(*g, *R.transposed(*g), [0], start)["bc"].tolist() == [1.0, 3.0, 4.0, 5.0, 5.0]   # ACCUMULATE


def test_a_shuffle_inside_rows_changes_nothing_where_every_sum_is_exact():
    widths = [2, 4, 8, 2, 16, 4, 2, 8]                                # dyadic: sigma a power of two below 2^53, every quotient exact
    g = R.stages(widths)
    want = R.answer(*g, *R.transposed(*g), np.arange(g[0]))
    assert want["sigma"].max() < 2.0 ** 53
    for seed in (1, 2):
        h = R.shuffled(*g, seed)
        Tp, Tj = R.transposed(*h)
        _, Tp, Tj = R.shuffled(h[0], Tp, Tj, seed + 10)
        assert np.any(h[2] != g[2])
        got = R.answer(*h, Tp, Tj, np.arange(g[0]))
        assert got["bc"].tobytes() == want["bc"].tobytes() and got["sigma"].tobytes() == want["sigma"].tobytes()


def test_the_inputs_are_what_the_gpu_tests_need():
    g = R.stages([3, 5, 7] * 15, seed=5)                              # inexact sums: the order inside rows matters
    a = R.answer(*g, *R.transposed(*g), [0])
    assert a["sigma"].max() > 2.0 ** 53 and a["overflow"] == 0 and np.all(np.isfinite(a["bc"]))
    g = R.stages([3, 5, 7] * 15, seed=5, drop=0.15)                   # (fully joined, a stage's terms are all alike and only the RULE shows; with edges left out the ORDER shows too)
    a = R.answer(*g, *R.transposed(*g), [0])
    assert a["sigma"].max() > 2.0 ** 53 and a["levels"] == 46 and a["reached"] == g[0]
    h = R.shuffled(*g, 6)
    Tp, Tj = R.transposed(*h)
    b = R.answer(*h, *R.shuffled(h[0], Tp, Tj, 7)[1:], [0])
    assert b["sigma"].tobytes() != a["sigma"].tobytes() or b["bc"].tobytes() != a["bc"].tobytes()   # only the stated order gives the bits
    g = R.diamonds(1030)
    a = R.answer(*g, *R.transposed(*g), [0])
    assert a["overflow"] == 1 and np.isinf(a["sigma"]).any() and np.isnan(a["bc"]).any() and a["levels"] == 2061
    assert set(a["bc"].view(np.uint64)[np.isnan(a["bc"])].tolist()) == {int(R.NAN_WORD)}
    assert R.refusal(*g, *R.transposed(*g), [0]) is None
    n, Gp, Gj = g
    Tp, Tj = R.transposed(*g)
    bad = Gj.copy(); bad[9] = n                                      # noqa: E702
    badT = Tj.copy(); badT[3] = -1                                   # noqa: E702
    assert R.refusal(n, Gp, bad, Tp, Tj, [0]) == "column" and R.refusal(n, Gp, Gj, Tp, badT, [0]) == "column"
    p = Gp.copy(); p[10] = p[11] + 1                                 # noqa: E702
    assert R.refusal(n, p, Gj, Tp, Tj, [0]) == "row pointer" and R.refusal(n, Gp, Gj, p, Tj, [0]) == "row pointer"
    assert R.refusal(n, Gp, Gj, Tp, Tj, [0, n]) == "source" and R.refusal(n, Gp, Gj, Tp, Tj, [-1]) == "source"
