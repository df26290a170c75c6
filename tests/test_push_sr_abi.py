"""CPU tests of the interfaces of sparse frontier x CSR (bhs_csr_push_semiring_device): both libraries export the entry
point the header declares and contain its kernels, the build tracks the new sources, dense.py and graph.py carry the calls,
the C++ facade's extension method compiles and links against the C-ABI library (tests/push; tests/test_push_sr_gpu.py runs
the same binary on a GPU), the numpy restatement (tests/pushref.py) agrees with a case written out by hand and with the pull
reference on the transpose, and graph.py's frontier loops, run on the restatements in place of the device calls, agree with
scipy.sparse.csgraph and with the pull-only loops."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from conftest import ROOT
import pushref as pr
import semiringref as srf
import spmvsrref as sr

from benchmark_spgemm_using_csr_amd import _lib

ENTRY = "bhs_csr_push_semiring_device"
FAMILIES = ("push_degrees", "push_scan", "push_edges", "push_compact")
DEMO_DIR = os.path.join(ROOT, "tests", "push")
NAMES = tuple(pr.SEMIRINGS)
NAN, INF = np.nan, np.inf


def test_header_declares_the_entry_point():
    txt = open(_lib.HEADER).read()
    decl = set(re.findall(r"BHS_API\s+[\w\s\*]+?\b(bhs_\w+)\s*\(", txt))
    assert ENTRY in decl and ENTRY in _lib.SYMBOLS
    vp, i, ll = C.c_void_p, C.c_int, C.c_longlong
    assert _lib.SYMBOLS[ENTRY] == (i, [vp, i, i, i, i, vp, vp, vp, i, vp, i, vp, ll, i, vp, ll, vp, ll, vp, C.POINTER(i),
                                       C.POINTER(ll), C.POINTER(C.c_double)])
    # the ctypes signature against the declaration's own parameter list
    flat = re.sub(r"/\*.*?\*/", " ", txt, flags=re.S)
    params = re.search(r"%s\s*\((.*?)\);" % ENTRY, flat, re.S).group(1).split(",")
    kinds = []
    for p in params:
        p = " ".join(p.split())
        kinds.append("ptr" if "*" in p else "ll" if p.startswith("long long") else "int")
    want = ["ll" if t is ll else "int" if t is i else "ptr" for t in _lib.SYMBOLS[ENTRY][1]]
    assert kinds == want and len(kinds) == 22
    assert "---- sparse frontier x CSR" in txt and txt.index("---- sparse frontier x CSR") > txt.index("---- semiring CSR x dense")
    assert txt.index("---- sparse frontier x CSR") < txt.index("---- input preparation")
    for fam in FAMILIES:
        assert fam in txt, fam
    host = open(os.path.join(_lib.CSRC, "bhs_host_push_sr.inc.h")).read()
    for fam in FAMILIES:
        assert '"%s"' % fam in host, fam
    sect = txt[txt.index("---- sparse frontier x CSR"):txt.index("---- input preparation")]
    for words in ("BHS_SR_PLUS_TIMES is refused on the host", "bit-for-bit function of its input", "rounding is monotone",
                  "NOT READ AT ALL", "ALWAYS accumulates", "neither read nor written", "test-and-set", "ascending, each once",
                  "compare-and-swap", "partly written", "BHS_MV_MASK_COMPLEMENT is the only flag"):
        assert words in sect, words


def test_both_libraries_export_the_entry_point(hiplib):
    for path in (_lib.SO_PATH, _lib.SO_PATH_F32):
        raw = C.CDLL(path)
        assert getattr(raw, ENTRY) is not None
        blob = open(path, "rb").read()
        for kern in (b"k_push_degrees", b"k_push_edges", b"k_push_count", b"k_push_compact"):
            assert kern in blob, (path, kern)


def test_sources_are_tracked_by_the_build():
    assert "bhs_push_sr.hip.h" in _lib.SOURCES and "bhs_host_push_sr.inc.h" in _lib.SOURCES
    mk = open(os.path.join(_lib.CSRC, "Makefile")).read()
    assert "bhs_push_sr.hip.h" in mk and "bhs_host_push_sr.inc.h" in mk
    unit = open(os.path.join(_lib.CSRC, "bhsparse_hip.hip")).read()
    incs = re.findall(r'#include "(bhs_host_\w+\.inc\.h)"', unit)
    assert incs[incs.index("bhs_host_spmv_sr.inc.h") + 1] == "bhs_host_push_sr.inc.h"     # directly after the pull part
    assert "SideWs pushWs;" in unit
    assert "release(h->pushWs)" in open(os.path.join(_lib.CSRC, "bhs_host_cabi.inc.h")).read()
    host = open(os.path.join(_lib.CSRC, "bhs_host_push_sr.inc.h")).read()
    assert '#include "bhs_push_sr.hip.h"' in host and "guarded(h," in host and host.count("side_scan(") == 2
    assert "semiring == BHS_SR_PLUS_TIMES" in host
    kernels = open(os.path.join(_lib.CSRC, "bhs_push_sr.hip.h")).read()
    assert "asm" not in kernels and "atomicCAS(" in kernels
    assert not re.search(r"atomic(Min|Max|Add)\s*\(", kernels)      # no hardware min / max / add touches Y
    assert len(re.findall(r"__global__", kernels)) == len(re.findall(r"__global__ __launch_bounds__\(256\)", kernels)) == 4


def test_null_handle_and_missing_platform(hiplib):
    assert hiplib.bhs_csr_push_semiring_device(None, 1, 0, 0, 0, None, None, None, 0, None, 1, None, 1, 0, None, 1, None, 1, None, None,
                                               None, None) == _lib.BHS_ERR_INVALID_ARG
    from benchmark_spgemm_using_csr_amd import dense, facade
    bh = facade.bhsparse()
    assert bh.push_next == 0
    assert dense.csr_push_semiring_raw_device(bh, "min_plus", 0, 0, 0, None, None, None, 0, None, 1, None, 1, 0, None, 1, None, 1,
                                              None) == _lib.BHS_ERR_NOT_READY


def test_python_modules_have_the_calls():
    from benchmark_spgemm_using_csr_amd import dense, facade, graph
    sig = lambda f: list(inspect.signature(f).parameters)           # noqa: E731
    assert sig(dense.csr_push_semiring_raw_device)[:19] == ["bh", "semiring", "m", "n", "nnzG", "d_valG", "d_rowPtrG", "d_colIndG", "nf",
                                                            "d_fidx", "k", "d_F", "ldF", "flags", "d_M", "ldM", "d_Y", "ldY", "d_next"]
    assert sig(dense.csr_push_semiring_device) == ["bh", "semiring", "m", "n", "G", "fidx", "F", "Y", "mask", "complement", "want_list"]
    assert not hasattr(facade.bhsparse, "csr_push_semiring_device")  # a function of a handle, not a method of it
    assert sig(graph.bfs_levels_frontier_device) == ["bh", "n", "A", "sources", "At", "push_below"]
    assert sig(graph.sssp_frontier_device) == ["bh", "n", "A", "sources", "At", "max_rounds", "push_below"]
    for name in ("bfs_levels_frontier_csr", "sssp_frontier_csr"):
        assert callable(getattr(graph, name, None)), name
    # the existing four keep their signatures
    assert sig(graph.bfs_levels_device) == ["bh", "n", "A", "sources"]
    assert sig(graph.sssp_device) == ["bh", "n", "A", "sources", "max_sweeps"]
    assert sig(graph.bfs_levels_csr)[:5] == ["n", "Ap", "Aj", "Ax", "sources"] and sig(graph.sssp_csr)[:5] == ["n", "Ap", "Aj", "Ax", "sources"]
    doc = " ".join(graph.sssp_frontier_device.__doc__.split())
    assert "Floating add is monotone" in doc and "min is exact" in doc and "least fixed point" in doc and "left-to-right" in doc
    assert "plus_times" in dense.csr_push_semiring_device.__doc__


def test_plus_times_is_named_as_refused():
    assert "plus_times" not in pr.SEMIRINGS and len(pr.SEMIRINGS) == 7
    assert "plus_times" in pr.HOST_REFUSALS
    G = (np.array([0, 1]), np.array([0]))
    assert pr.invalid(1, 1, G[0], G[1], 1, [0], semiring=_lib.BHS_SR_PLUS_TIMES) == "plus_times"
    assert pr.invalid(1, 1, G[0], G[1], 1, [0], semiring=_lib.BHS_SR_PLUS_PAIR) is None


def test_cpp_facade_extension_builds(hiplib):
    src = open(os.path.join(ROOT, "benchmark_spgemm_using_csr_amd", "host", "bhsparse.h")).read()
    flat = re.sub(r"\s+", " ", src)
    assert ("int csr_push_semiring_device(int semiring, int m, int n, int nnzG, const value_type *d_valG, "
            "const index_type *d_rowPtrG, const index_type *d_colIndG, int nf, const index_type *d_fidx, int k, "
            "const value_type *d_F, long long ldF, int flags, const value_type *d_M, long long ldM, value_type *d_Y, "
            "long long ldY, index_type *d_next, int *next_count_out, long long *changed_out);") in flat
    subprocess.check_call(["make", "-C", DEMO_DIR, "-s"])
    demo = os.path.join(DEMO_DIR, "push_demo")
    assert os.access(demo, os.X_OK)
    out = subprocess.run(["nm", "-D", "--undefined-only", demo], capture_output=True, text=True).stdout
    assert ENTRY in out
    assert "tests/push/push_demo" in open(os.path.join(ROOT, ".gitignore")).read().split()


# ---------------------------------------------------------------- the reference against a case written out by hand
# G is 5 x 4.  row 0 not ascending, with the pair (0, 1) twice; row 1 empty; row 2 holds -0 and +0 as values; row 3 a NaN;
# row 4 the infinities.
GP = np.array([0, 4, 4, 6, 8, 10], np.int32)
GJ = np.array([3, 1, 0, 1, 0, 2, 1, 2, 0, 3], np.int32)
GX = np.array([2, 5, 1, 3, -0.0, 0.0, NAN, 4, INF, -INF], np.float64)


def same(got, want):
    return srf.same_bits(np.asarray(got, np.float64), np.asarray(want, np.float64))


def test_pushref_by_hand():
    v = lambda name, fidx, F, Y, **kw: pr.push_semiring(name, 5, 4, GP, GJ, GX, fidx, F, np.array(Y, np.float64), **kw)   # noqa: E731
    # row 0 with f = 10: products into column 3: 2 + 10; column 1: 5 + 10 and 3 + 10; column 0: 1 + 10
    out, changed, nxt = v("min_plus", [0], [10.0], [INF, 14, 5, 12])
    assert same(out, [11, 13, 5, 12]) and changed == 2 and nxt.tolist() == [0, 1] and nxt.dtype == np.int32
    # the empty row reaches nothing; a vertex listed twice pushes twice (min is idempotent: as once)
    out, changed, nxt = v("min_plus", [1, 0, 0], [3.0, 10.0, 9.0], [INF, 14, 5, 12])
    assert same(out, [10, 12, 5, 11]) and changed == 3 and nxt.tolist() == [0, 1, 3]
    # ... but plus_pair counts each listing, and each duplicate pair: column 1 gets 2 per listing
    out, changed, nxt = v("plus_pair", [0, 0, 1], [7.0, 7.0, 7.0], [0, 0.5, -3, INF])
    assert same(out, [2, 4.5, -3, INF]) and changed == 2 and nxt.tolist() == [0, 1]    # (Inf + 1 is no change; row 2 is not reached)
    # row 2: -0 * 1 = -0 into column 0, +0 * 1 = +0 into column 2; -0 below +0, and neither is a change against a zero
    out, changed, nxt = v("max_times", [2], [1.0], [-0.0, 9, -0.0, 9])
    assert same(out, [-0.0, 9, 0.0, 9]) and changed == 0 and len(nxt) == 0
    out, changed, nxt = v("max_times", [2], [1.0], [-INF, 9, -1.0, 9])
    assert same(out, [-0.0, 9, 0.0, 9]) and changed == 2
    # row 3: NaN + f into column 1 (NaN wins, a change), 4 + f into column 2; a NaN that is there stays and is no change
    out, changed, nxt = v("min_plus", [3], [1.0], [0, 0, 7, NAN])
    assert same(out, [0, NAN, 5, NAN]) and changed == 2 and nxt.tolist() == [1, 2]
    out, changed, nxt = v("max_min", [3], [1.0], [0, NAN, 0.5, 0])
    assert same(out, [0, NAN, 1, 0]) and changed == 1 and nxt.tolist() == [2]
    # row 4: Inf + f into column 0, -Inf + f into column 3
    out, changed, nxt = v("max_plus", [4], [1.0], [0, 0, 0, 0])
    assert same(out, [INF, 0, 0, 0]) and changed == 1
    assert same(v("min_plus", [4], [1.0], [0, 0, 0, 0])[0], [0, 0, 0, -INF])
    assert same(v("min_max", [4], [1.0], [INF, 0, 0, INF])[0], [INF, 0, 0, 1])        # max(Inf, 1), max(-Inf, 1), then min
    # or_and: a value of G or F that is zero gives 0; a Y that is reached is normalised (5 -> 1: a change), one that is not
    # reached keeps its bits; NaN is non-zero
    out, changed, nxt = v("or_and", [2, 3], [1.0, 1.0], [0, 0, 5, 7])
    assert same(out, [0, 1, 1, 7]) and changed == 2 and nxt.tolist() == [1, 2]
    out, changed, nxt = v("or_and", [0], [0.0], [0, -0.0, 0, NAN])
    assert same(out, [0, 0.0, 0, 1]) and changed == 1 and nxt.tolist() == [3]         # (-0 -> +0: no change; NaN -> 1 is one)
    # one mask value of each kind: a number and NaN (set), -0 and +0 (not set); then the complement
    mask = np.array([3.0, NAN, -0.0, 0.0])
    out, changed, nxt = v("min_plus", [0, 3], [10.0, 1.0], [INF, INF, INF, INF], mask=mask)
    assert same(out, [11, NAN, INF, INF]) and changed == 2 and nxt.tolist() == [0, 1]
    out, changed, nxt = v("min_plus", [0, 3], [10.0, 1.0], [INF, INF, INF, INF], mask=mask, complement=True)
    assert same(out, [INF, INF, 5, 12]) and changed == 2 and nxt.tolist() == [2, 3]
    # k columns, the float build: inputs rounded to float first, a rounding per update
    F = np.array([[10.0, 0.1]])
    out, changed, nxt = pr.push_semiring("min_plus", 5, 4, GP, GJ, GX, [0], F, np.full((4, 2), INF), dtype=np.float32)
    f32 = np.float64(np.float32(0.1))
    assert out.dtype == np.float32 and out.shape == (4, 2) and out[1, 1] == np.float32(3 + f32) and changed == 6 and nxt.tolist() == [0, 1, 3]
    # empty shapes
    out, changed, nxt = pr.push_semiring("max_min", 5, 4, GP, GJ, GX, [], np.zeros((0, 1)), np.zeros(4))
    assert same(out, np.zeros(4)) and changed == 0 and len(nxt) == 0
    out, changed, nxt = pr.push_semiring("max_min", 0, 0, [0], [], [], [], np.zeros((0, 2)), np.zeros((0, 2)))
    assert out.shape == (0, 2) and changed == 0 and len(nxt) == 0


def test_pushref_names_what_must_be_refused():
    ok = lambda **kw: pr.invalid(5, 4, GP, GJ, kw.pop("nf", 2), kw.pop("fidx", [0, 4]), **kw)   # noqa: E731
    assert ok() is None and ok(k=3, ldF=4, ldY=5, has_mask=True, ldM=3, flags=2, semiring=7) is None
    assert pr.invalid(-1, 4, GP, GJ, 0, []) == "negative size" and pr.invalid(5, 4, GP, GJ, -1, []) == "negative size"
    assert ok(k=0) == "k < 1" and ok(k=3, ldF=2) == "ldF < k" and ok(k=3, ldY=2) == "ldY < k"
    assert pr.invalid(5, 4, None, GJ, 0, []) == "NULL rowPtrG" and pr.invalid(5, 4, GP, None, 0, [], nnzG=3) == "NULL colIndG"
    assert pr.invalid(5, 4, GP, GJ, 2, None) == "NULL fidx" and ok(has_F=False) == "NULL F" and ok(has_Y=False) == "NULL Y"
    assert ok(semiring=8) == "unknown semiring" and ok(semiring=-1) == "unknown semiring" and ok(semiring=0) == "plus_times"
    assert ok(flags=1) == "unknown flag" and ok(flags=4) == "unknown flag"          # (BHS_MV_ACCUM is no flag of this call)
    assert ok(k=3, has_mask=True, ldM=2) == "ldM < k" and ok(k=3, ldM=2) is None
    assert ok(flags=2) == "complement without a mask" and ok(overlap=True) == "an output overlaps an input"
    assert ok(fidx=[0, 5]) == "fidx out of range" and ok(fidx=[-1, 0]) == "fidx out of range"
    p = GP.copy(); p[3] = 3                                           # row 2 runs from 4 to 3; rows 0, 1, 3, 4 are in order
    assert pr.invalid(5, 4, p, GJ, 2, [0, 2]) == "bad row pointer in a pushed row"
    assert pr.invalid(5, 4, p, GJ, 2, [0, 4]) is None               # ... which nobody looks at while row 2 is not pushed
    p = GP.copy(); p[5] = 11
    assert pr.invalid(5, 4, p, GJ, 1, [4]) == "bad row pointer in a pushed row" and pr.invalid(5, 4, p, GJ, 1, [3]) is None
    for col in (4, -1):
        j = GJ.copy(); j[9] = col
        assert pr.invalid(5, 4, GP, j, 1, [4]) == "column out of range in a pushed row"
        assert pr.invalid(5, 4, GP, j, 4, [0, 1, 2, 3]) is None
    assert set(pr.HOST_REFUSALS).isdisjoint(pr.DEVICE_REFUSALS) and len(pr.HOST_REFUSALS) == 15 and len(pr.DEVICE_REFUSALS) == 3


def transpose(m, n, Ap, Aj, Ax):
    """(Tp, Tj, Tx) of the n x m transpose, duplicates kept"""
    rows = np.repeat(np.arange(m), np.diff(Ap))
    order = np.argsort(Aj, kind="stable")
    Tp = np.zeros(n + 1, np.int64)
    np.cumsum(np.bincount(Aj, minlength=n), out=Tp[1:])
    return Tp, rows[order], None if Ax is None else Ax[order]


@pytest.mark.parametrize("name", NAMES)
def test_pushref_against_the_pull_reference(name):
    """push(G = A^T, fidx = every row, F = X) into Y preset to the identity is spmm_semiring(A, X), bit for bit; for
    plus_pair that is the rows' entry counts."""
    for seed in range(6):
        rng = np.random.default_rng(1200 + seed)
        m, n, k = int(rng.integers(1, 40)), int(rng.integers(1, 40)), int(rng.integers(1, 6))
        lens = rng.integers(0, min(n, 9) + 1, m)
        lens[rng.integers(0, m)] = 0
        Ap = np.zeros(m + 1, np.int64)
        np.cumsum(lens, out=Ap[1:])
        Aj = np.concatenate([rng.integers(0, n, L) for L in lens] + [np.zeros(0, np.int64)])    # duplicates among them
        Ax = srf.edge_values(rng, len(Aj), plus_safe=True)
        X = srf.edge_values(rng, n * k, plus_safe=True).reshape(n, k)
        Gp, Gj, Gx = transpose(m, n, Ap, Aj, Ax)                     # n x m: row j pushes to the rows of A that hold column j
        for dtype in (np.float64, np.float32):
            want, want_changed = sr.spmm_semiring(name, m, n, Ap, Aj, Ax, X, dtype=dtype)
            Y0 = np.full((m, k), srf.identity(name), dtype)
            perm = rng.permutation(n)                                # the list's order does not matter
            got, changed, nxt = pr.push_semiring(name, n, m, Gp, Gj, Gx, perm, X[perm], Y0, dtype=dtype)
            assert srf.same_bits(got, want), (name, seed, dtype)
            assert changed == want_changed, (name, seed, dtype)
            with np.errstate(invalid="ignore"):
                differs = ~((got == Y0) | (np.isnan(got) & np.isnan(Y0)))
            assert changed == np.count_nonzero(differs) and np.array_equal(nxt, np.flatnonzero(differs.any(axis=1)))
            if name == "plus_pair":
                assert np.array_equal(got, np.repeat(lens[:, None], k, axis=1).astype(dtype))


# ---------------------------------------------------------------- graph.py's loops on the references, against scipy
def reference_pull(bh, semiring, m, n, A, X, Y=None, mask=None, accumulate=False, complement=False):
    """dense.csr_spmm_semiring_device on host tensors, computed by the numpy reference"""
    Ap, Aj, Ax = (None if t is None else t.numpy() for t in A)
    out, changed = sr.spmm_semiring(semiring, m, n, Ap, Aj, Ax, X.numpy(), None if Y is None else Y.numpy(),
                                    None if mask is None else mask.numpy(), accumulate, complement)
    Y.copy_(torch.from_numpy(out))
    bh.spmv_ms, bh.spmv_changed = 0.5, changed
    bh.calls.append("pull")
    return Y, changed


def reference_push(bh, semiring, m, n, G, fidx, F, Y, mask=None, complement=False, want_list=True):
    """dense.csr_push_semiring_device on host tensors, computed by the numpy reference"""
    Gp, Gj, Gx = (None if t is None else t.numpy() for t in G)
    assert fidx.dtype == torch.int32 and F.shape == (fidx.numel(), Y.shape[1])
    out, changed, nxt = pr.push_semiring(semiring, m, n, Gp, Gj, Gx, fidx.numpy(), F.numpy(), Y.numpy(),
                                         None if mask is None else mask.numpy(), complement)
    Y.copy_(torch.from_numpy(out))
    bh.spmv_ms, bh.spmv_changed, bh.push_next = 0.25, changed, len(nxt)
    bh.calls.append("push")
    return Y, changed, torch.from_numpy(nxt)


def scipy_levels_and_distances(n, Ap, Aj, Ax, sources):
    """(BFS levels, Bellman-Ford distances) by scipy.sparse.csgraph of the graph whose entry A(i, j) is an edge j -> i"""
    import scipy.sparse as sp
    from scipy.sparse import csgraph
    G = sp.csr_matrix((Ax, Aj, Ap), shape=(n, n)).T.tocsr()         # (csgraph reads G[i, j] as an edge i -> j)
    hops = csgraph.shortest_path(G, method="D", unweighted=True, indices=list(sources)).T
    dist = csgraph.bellman_ford(G, indices=list(sources)).T
    return np.where(np.isfinite(hops), hops + 1, 0.0), dist


def random_digraph(n, degree, seed):
    """a directed graph without duplicate edges, weights 1 .. 9 (csgraph would add duplicates up; an explicit zero is no edge to it)"""
    rng = np.random.default_rng(seed)
    pairs = np.unique(np.stack([rng.integers(0, n, n * degree), rng.integers(0, n, n * degree)], axis=1), axis=0)
    Ap = np.zeros(n + 1, np.int32)
    np.cumsum(np.bincount(pairs[:, 0], minlength=n), out=Ap[1:])
    return Ap, pairs[:, 1].astype(np.int32), rng.integers(1, 10, len(pairs)).astype(np.float64)


def path_graph(n):
    """the directed path 0 -> 1 -> .. -> n - 1 in the pull form: row v holds column v - 1; the edge into v weighs v"""
    Ap = np.concatenate([[0], np.arange(n)]).astype(np.int32)
    return Ap, np.arange(n - 1, dtype=np.int32), np.arange(1, n, dtype=np.float64)


def tensors(Ap, Aj, Ax):
    return torch.from_numpy(np.ascontiguousarray(Ap, np.int32)), torch.from_numpy(np.ascontiguousarray(Aj, np.int32)), torch.from_numpy(Ax)


def test_frontier_loops_on_the_references_against_scipy(monkeypatch):
    from benchmark_spgemm_using_csr_amd import facade, graph
    monkeypatch.setattr(graph, "csr_spmm_semiring_device", reference_pull)
    monkeypatch.setattr(graph, "csr_push_semiring_device", reference_push)
    bh = facade.bhsparse()
    bh.calls = []
    cases = [(n, random_digraph(n, degree, 400 + seed)) for seed, (n, degree) in enumerate(((40, 2), (60, 1), (25, 4)))]
    cases.append((60, path_graph(60)))
    for case, (n, (Ap, Aj, Ax)) in enumerate(cases):
        A = tensors(Ap, Aj, Ax)
        At = tensors(*transpose(n, n, Ap.astype(np.int64), Aj.astype(np.int64), Ax))
        for sources in ([0, n // 2, n - 1], [0]):
            levels, dist = scipy_levels_and_distances(n, Ap, Aj, Ax, sources)
            pull_levels, pull_dist = graph.bfs_levels_device(bh, n, A, sources), graph.sssp_device(bh, n, A, sources)
            assert np.array_equal(pull_levels.numpy(), levels) and np.array_equal(pull_dist.numpy(), dist)
            for push_below in (0, 4, float("inf")):
                bh.calls.clear()
                got = graph.bfs_levels_frontier_device(bh, n, A, sources, At=At, push_below=push_below)
                assert np.array_equal(got.numpy(), levels), (case, push_below)
                assert torch.equal(got, pull_levels)
                kinds = set(bh.calls)
                assert kinds == ({"pull"} if push_below == 0 else {"push"} if push_below == float("inf") else kinds)
                if push_below == float("inf") and len(sources) == 1:
                    assert len(bh.calls) == int(levels.max())        # a call per level: the last one finds nothing
                bh.calls.clear()
                got = graph.sssp_frontier_device(bh, n, A, sources, At=At, push_below=push_below)
                assert np.array_equal(got.numpy(), dist), (case, push_below)
                assert torch.equal(got, pull_dist)
                assert set(bh.calls) == ({"pull"} if push_below == 0 else {"push"} if push_below == float("inf") else set(bh.calls))
        # with push for frontiers of at most five vertices both directions are taken, and switched between both ways: a
        # source alone is a small frontier, the middle levels are not, the last ones are again
        if case == 0:
            for loop in (graph.bfs_levels_frontier_device, graph.sssp_frontier_device):
                bh.calls.clear()
                loop(bh, n, A, [0], At=At, push_below=8)
                assert bh.calls[0] == "push" and "pull" in bh.calls and "push" in bh.calls[bh.calls.index("pull"):], bh.calls
    n, (Ap, Aj, Ax) = cases[-1]
    At = tensors(*transpose(n, n, Ap.astype(np.int64), Aj.astype(np.int64), Ax))
    lv, steps, ms, pushes = graph._bfs_frontier(bh, n, tensors(Ap, Aj, Ax), [0], At, float("inf"))
    assert steps == pushes == 60 and ms == 0.25 * 60
    # a cycle of negative weight is reported, not looped over for ever
    Ap, Aj, Ax = np.array([0, 1, 2, 3], np.int32), np.array([2, 0, 1], np.int32), np.array([1.0, 1.0, -3.0])
    At = tensors(*transpose(3, 3, Ap.astype(np.int64), Aj.astype(np.int64), Ax))
    for push_below in (0, 4, float("inf")):
        with pytest.raises(facade.BhsparseError):
            graph.sssp_frontier_device(bh, 3, tensors(Ap, Aj, Ax), 0, At=At, push_below=push_below)
    d, rounds, _, _ = graph._sssp_frontier(bh, 3, tensors(Ap, Aj, np.abs(Ax)), 0, tensors(*transpose(3, 3, Ap.astype(np.int64), Aj.astype(np.int64), np.abs(Ax))),
                                           None, float("inf"))
    assert d[:, 0].tolist() == [0.0, 1.0, 4.0] and rounds == 3
