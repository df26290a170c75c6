"""CPU tests of the interfaces of semiring CSR x dense (bhs_csr_spmv_semiring_device, bhs_csr_spmm_semiring_device): both
libraries export the entry points the header declares, the build tracks the new sources, dense.py and graph.py carry the
calls, the C++ facade's extension methods compile and link against the C-ABI library (tests/srmv; tests/test_spmv_sr_gpu.py
runs the same binary on a GPU), the numpy restatement (tests/spmvsrref.py) agrees with a case written out by hand, with the
semiring multiply's reference and with the plus-times reference, and graph.py's loops, run on that restatement in place
of the device call, agree with scipy.sparse.csgraph."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from conftest import ROOT
import semiringref as srf
import spmvref
import spmvsrref as sr

from benchmark_spgemm_using_csr_amd import _lib

ENTRY = ("bhs_csr_spmv_semiring_device", "bhs_csr_spmm_semiring_device")
FAMILIES = ("srmv_short", "srmv_wave", "srmv_long")
DEMO_DIR = os.path.join(ROOT, "tests", "srmv")
NAMES = tuple(srf.SEMIRINGS)


def test_header_declares_the_entry_points_and_the_flags():
    txt = open(_lib.HEADER).read()
    decl = set(re.findall(r"BHS_API\s+[\w\s\*]+?\b(bhs_\w+)\s*\(", txt))
    for name in ENTRY:
        assert name in decl and name in _lib.SYMBOLS
    assert re.search(r"enum\s*\{\s*BHS_MV_ACCUM\s*=\s*1\s*,\s*BHS_MV_MASK_COMPLEMENT\s*=\s*2\s*\}", txt)
    assert (_lib.BHS_MV_ACCUM, _lib.BHS_MV_MASK_COMPLEMENT) == (1, 2) == (sr.ACCUM, sr.COMPLEMENT)
    vp, i, ll = C.c_void_p, C.c_int, C.c_longlong
    pll, pd = C.POINTER(C.c_longlong), C.POINTER(C.c_double)
    assert _lib.SYMBOLS[ENTRY[0]] == (i, [vp, i, i, i, i, vp, vp, vp, vp, i, vp, vp, pll, pd])
    assert _lib.SYMBOLS[ENTRY[1]] == (i, [vp, i, i, i, i, vp, vp, vp, i, vp, ll, i, vp, ll, vp, ll, pll, pd])
    assert "---- semiring CSR x dense" in txt and txt.index("---- semiring CSR x dense") > txt.index("---- CSR x dense")
    for fam in FAMILIES:
        assert fam in txt, fam
    host = open(os.path.join(_lib.CSRC, "bhs_host_spmv_sr.inc.h")).read()
    for fam in FAMILIES:
        assert '"%s"' % fam in host, fam
    for words in ("y_old is never read", "NaN is set, -0 and +0 are not", "is not walked at all", "COMPLEMENT with a\n *   NULL mask is refused",
                  "NaN over NaN counts as unchanged", "No atomics touch Y", "partly written", "M may overlap X"):
        assert words in txt, words


def test_both_libraries_export_the_entry_points(hiplib):
    for path in (_lib.SO_PATH, _lib.SO_PATH_F32):
        raw = C.CDLL(path)
        for name in ENTRY:
            assert getattr(raw, name) is not None
        blob = open(path, "rb").read()
        for kern in (b"k_smv_short", b"k_smv_wave", b"k_smv_long"):
            assert kern in blob, (path, kern)


def test_sources_are_tracked_by_the_build():
    assert "bhs_spmv_sr.hip.h" in _lib.SOURCES and "bhs_host_spmv_sr.inc.h" in _lib.SOURCES
    mk = open(os.path.join(_lib.CSRC, "Makefile")).read()
    assert "bhs_spmv_sr.hip.h" in mk and "bhs_host_spmv_sr.inc.h" in mk
    unit = open(os.path.join(_lib.CSRC, "bhsparse_hip.hip")).read()
    incs = re.findall(r'#include "(bhs_host_\w+\.inc\.h)"', unit)
    assert incs[incs.index("bhs_host_spmv.inc.h") + 1] == "bhs_host_spmv_sr.inc.h"     # directly after the plus-times part
    assert incs.index("bhs_host_spmv_sr.inc.h") < incs.index("bhs_host_semiring.inc.h")
    assert "SideWs srmvWs;" in unit
    assert "release(h->srmvWs)" in open(os.path.join(_lib.CSRC, "bhs_host_cabi.inc.h")).read()
    host = open(os.path.join(_lib.CSRC, "bhs_host_spmv_sr.inc.h")).read()
    assert '#include "bhs_spmv_sr.hip.h"' in host and "bhs_semiring.hip.h\"" not in host
    kernels = open(os.path.join(_lib.CSRC, "bhs_spmv_sr.hip.h")).read()
    assert '#include "bhs_spmv.hip.h"' in kernels and "asm" not in kernels
    # the one integer atomic per workgroup on the control word, one on its LDS word; none on Y
    assert len(re.findall(r"atomic\w+\(", kernels)) == 2 and "atomicAdd(sChg" in kernels and "ctl + SMV_CHANGED" in kernels


def test_null_handle_is_rejected(hiplib):
    inv = _lib.BHS_ERR_INVALID_ARG
    assert hiplib.bhs_csr_spmv_semiring_device(None, 1, 0, 0, 0, None, None, None, None, 0, None, None, None, None) == inv
    assert hiplib.bhs_csr_spmm_semiring_device(None, 1, 0, 0, 0, None, None, None, 1, None, 1, 0, None, 1, None, 1, None, None) == inv


def test_python_modules_have_the_calls():
    from benchmark_spgemm_using_csr_amd import dense, facade, graph
    for name in ("csr_spmv_semiring_raw_device", "csr_spmm_semiring_raw_device", "csr_spmm_semiring_device", "spmm_semiring_csr"):
        assert callable(getattr(dense, name, None)), name
        assert not hasattr(facade.bhsparse, name), name             # functions of a handle, not methods of it
    for name in ("bfs_levels_device", "sssp_device", "bfs_levels_csr", "sssp_csr"):
        assert callable(getattr(graph, name, None)), name
    sig = lambda f: list(inspect.signature(f).parameters)           # noqa: E731
    assert sig(dense.csr_spmv_semiring_raw_device) == ["bh", "semiring", "m", "n", "nnzA", "d_valA", "d_rowPtrA", "d_colIndA", "d_x",
                                                       "flags", "d_mask", "d_y"]
    assert sig(dense.csr_spmm_semiring_raw_device) == ["bh", "semiring", "m", "n", "nnzA", "d_valA", "d_rowPtrA", "d_colIndA", "k",
                                                       "d_X", "ldX", "flags", "d_M", "ldM", "d_Y", "ldY"]
    assert sig(dense.csr_spmm_semiring_device) == ["bh", "semiring", "m", "n", "A", "X", "Y", "mask", "accumulate", "complement"]
    assert sig(dense.spmm_semiring_csr)[:11] == ["semiring", "m", "n", "Ap", "Aj", "Ax", "X", "Y", "mask", "accumulate", "complement"]
    assert sig(graph.bfs_levels_device) == ["bh", "n", "A", "sources"]
    assert sig(graph.sssp_device) == ["bh", "n", "A", "sources", "max_sweeps"]
    for f in (graph.bfs_levels_device, graph.sssp_device):
        assert "edge j -> i" in f.__doc__
    assert "csr_transpose" in graph.__doc__
    bh = facade.bhsparse()
    assert bh.spmv_ms == 0.0 and bh.spmv_changed == 0 and type(bh.spmv_changed) is int
    # without a platform the raw calls answer, they do not crash
    nr = _lib.BHS_ERR_NOT_READY
    assert dense.csr_spmv_semiring_raw_device(bh, "min_plus", 0, 0, 0, None, None, None, None, 0, None, None) == nr
    assert dense.csr_spmm_semiring_raw_device(bh, _lib.BHS_SR_OR_AND, 0, 0, 0, None, None, None, 1, None, 1, 0, None, 1, None, 1) == nr
    assert [dense.semiring_identity(s) for s in NAMES] == [srf.identity(s) for s in NAMES]


def test_cpp_facade_extension_builds(hiplib):
    src = open(os.path.join(ROOT, "benchmark_spgemm_using_csr_amd", "host", "bhsparse.h")).read()
    flat = re.sub(r"\s+", " ", src)
    assert ("int csr_spmv_semiring_device(int semiring, int m, int n, int nnzA, const value_type *d_valA, "
            "const index_type *d_rowPtrA, const index_type *d_colIndA, const value_type *d_x, int flags, "
            "const value_type *d_mask, value_type *d_y, long long *changed_out);") in flat
    assert ("int csr_spmm_semiring_device(int semiring, int m, int n, int nnzA, const value_type *d_valA, "
            "const index_type *d_rowPtrA, const index_type *d_colIndA, int k, const value_type *d_X, long long ldX, int flags, "
            "const value_type *d_M, long long ldM, value_type *d_Y, long long ldY, long long *changed_out);") in flat
    subprocess.check_call(["make", "-C", DEMO_DIR, "-s"])
    demo = os.path.join(DEMO_DIR, "srmv_demo")
    assert os.access(demo, os.X_OK)
    out = subprocess.run(["nm", "-D", "--undefined-only", demo], capture_output=True, text=True).stdout
    for name in ENTRY:
        assert name in out
    assert "tests/srmv/srmv_demo" in open(os.path.join(ROOT, ".gitignore")).read().split()


# ---------------------------------------------------------------- the reference against a case written out by hand
# 5 x 4.  row 0 not ascending, with the pair (0, 1) twice; row 1 empty; row 2 holds -0 and +0 as values; row 3 a NaN;
# row 4 the infinities.
NAN, INF = np.nan, np.inf
AP = np.array([0, 4, 4, 6, 8, 10], np.int32)
AJ = np.array([3, 1, 0, 1, 0, 2, 1, 2, 0, 3], np.int32)
AX = np.array([2, 5, 1, 3, -0.0, 0.0, NAN, 4, INF, -INF], np.float64)
XV = np.array([1, -2, 0.5, 4], np.float64)


def same(got, want):
    return srf.same_bits(np.asarray(got, np.float64), np.asarray(want, np.float64))


def test_spmvsrref_by_hand():
    v = lambda name, **kw: sr.spmv_semiring(name, 5, 4, AP, AJ, AX, XV, **kw)   # noqa: E731
    # products of row 0: 2 (x) 4, 5 (x) -2, 1 (x) 1, 3 (x) -2
    assert same(v("plus_times")[0], [8 - 10 + 1 - 6, 0, 0.0, NAN, NAN]) and v("plus_times")[1] == 3
    assert same(v("min_plus")[0], [1, INF, 0.5, NAN, -INF]) and v("min_plus")[1] == 4
    assert same(v("max_plus")[0], [6, -INF, 1, NAN, INF])            # (row 2: -0 + 1, +0 + 0.5)
    assert same(v("max_times")[0], [8, -INF, 0.0, NAN, INF])        # (row 2: -0 * 1 = -0 below +0 * 0.5 = +0)
    assert same(v("min_max")[0], [1, INF, 0.5, NAN, 4])             # max(a, b), then min: row 2 max(-0, 1) = 1, max(+0, .5) = .5
    assert same(v("max_min")[0], [2, -INF, 0.0, NAN, 1])            # row 2: min(-0, 1) = -0, min(+0, .5) = +0 -> max is +0
    assert same(v("or_and")[0], [1, 0, 0, 1, 1])                    # (row 2: both values are zero; NaN is non-zero)
    assert v("or_and")[1] == 3
    assert same(v("plus_pair")[0], [4, 0, 2, 2, 2]) and v("plus_pair")[1] == 4
    assert same(sr.spmv_semiring("plus_times", 5, 4, AP, AJ, None, XV)[0], [4 - 2 + 1 - 2, 0, 1.5, -1.5, 5])
    # one mask value of each kind: a number, NaN (set), -0 and +0 (not set), and the complement
    mask = np.array([3.0, NAN, -0.0, 0.0, 1.0])
    y0 = np.array([-7.0, -7, -7, -7, -7])
    out, changed = v("min_plus", y=y0, mask=mask)
    assert same(out, [1, INF, -7, -7, -INF]) and changed == 2       # (row 1: the identity over the identity is no change)
    out, changed = v("min_plus", y=y0, mask=mask, complement=True)
    assert same(out, [-7, -7, 0.5, NAN, -7]) and changed == 2
    assert same(v("min_plus", mask=mask)[0], [1, INF, NAN, NAN, -INF])   # without Y: nothing is written where not selected
    # accumulate: y_old (+) t; a NaN y_old stays NaN and is no change; y_old is what `changed` compares with
    yold = np.array([0.5, 3, NAN, 2, -INF])
    out, changed = v("min_plus", y=yold, accumulate=True)
    assert same(out, [0.5, 3, NAN, NAN, -INF]) and changed == 1     # only row 3: a number became NaN
    out, changed = v("max_plus", y=yold, accumulate=True)
    assert same(out, [6, 3, NAN, NAN, INF]) and changed == 3
    out, changed = v("plus_times", y=yold, accumulate=True)
    assert same(out, [-6.5, 3, NAN, NAN, NAN]) and changed == 3
    out, changed = v("or_and", y=np.array([0, 5, -0.0, NAN, 1.0]), accumulate=True)
    assert same(out, [1, 1, 0, 1, 1]) and changed == 3              # (5 -> 1 and NaN -> 1 differ as numbers; -0 -> +0 does not)
    out, changed = v("plus_pair", y=yold, accumulate=True, mask=mask)
    assert same(out, [4.5, 3, NAN, 2, -INF]) and changed == 1
    # k columns, the float build: inputs rounded to float first, one rounding at the end
    X = np.stack([XV, XV * 0.1], axis=1)
    out, changed = sr.spmm_semiring("min_plus", 5, 4, AP, AJ, AX, X, dtype=np.float32)
    x32 = X.astype(np.float32).astype(np.float64)
    assert out.dtype == np.float32 and out.shape == (5, 2) and out[0, 1] == np.float32(1 + x32[0, 1]) and changed == 8
    # empty shapes
    assert sr.spmv_semiring("max_min", 0, 4, [0], [], [], XV)[0].shape == (0,)
    assert same(sr.spmv_semiring("max_min", 3, 0, [0, 0, 0, 0], [], [], [])[0], [-INF] * 3)


def test_spmvsrref_names_what_must_be_refused():
    assert sr.invalid(5, 4, AP, AJ) is None and sr.invalid(5, 4, AP, AJ, 3, 4, 5, has_mask=True, ldM=3, flags=3, semiring=7) is None
    assert sr.invalid(-1, 4, AP, AJ) == "negative size" and sr.invalid(5, 4, AP, AJ, 0) == "k < 1"
    assert sr.invalid(5, 4, AP, AJ, 3, 2, 3) == "ldX < k" and sr.invalid(5, 4, AP, AJ, 3, 3, 2) == "ldY < k"
    assert sr.invalid(5, 4, None, AJ) == "NULL rowPtrA"
    assert sr.invalid(5, 4, AP, AJ, has_x=False) == "NULL x" and sr.invalid(5, 4, AP, AJ, has_y=False) == "NULL y"
    assert sr.invalid(5, 4, AP, AJ, semiring=8) == "unknown semiring" and sr.invalid(5, 4, AP, AJ, semiring=-1) == "unknown semiring"
    assert sr.invalid(5, 4, AP, AJ, flags=4) == "unknown flag"
    assert sr.invalid(5, 4, AP, AJ, 3, has_mask=True, ldM=2) == "ldM < k" and sr.invalid(5, 4, AP, AJ, 3, ldM=2) is None
    assert sr.invalid(5, 4, AP, AJ, flags=2) == "complement without a mask"
    assert sr.invalid(5, 4, AP, AJ, overlap=True) == "y overlaps an input"
    p = AP.copy(); p[0] = 1
    assert sr.invalid(5, 4, p, AJ) == "rowPtrA[0] != 0"
    p = AP.copy(); p[-1] = 9
    assert sr.invalid(5, 4, p, AJ) == "rowPtrA[m] != nnzA"
    p = AP.copy(); p[2] = 3
    assert sr.invalid(5, 4, p, AJ) == "decreasing rowPtrA"
    for col in (4, -1):
        j = AJ.copy(); j[9] = col
        assert sr.invalid(5, 4, AP, j) == "column of A out of range"
        # ... where it is read: not in a row none of whose elements is selected; the row pointer everywhere
        assert sr.invalid(5, 4, AP, j, rows_read=[1, 1, 1, 1, 0]) is None
        assert sr.invalid(5, 4, AP, j, rows_read=[0, 0, 0, 0, 1]) == "column of A out of range"
    p = AP.copy(); p[2] = 3
    assert sr.invalid(5, 4, p, AJ, rows_read=[0] * 5) == "decreasing rowPtrA"
    assert set(sr.HOST_REFUSALS).isdisjoint(sr.DEVICE_REFUSALS) and len(sr.HOST_REFUSALS) == 13 and len(sr.DEVICE_REFUSALS) == 4


@pytest.mark.parametrize("name", NAMES)
def test_spmvsrref_against_the_semiring_multiply(name):
    """X written as a CSR matrix that holds every element, M as the full m x k pattern: the semiring multiply's reference
    gives the same bits, the identity on empty rows included."""
    for seed in range(6):
        rng = np.random.default_rng(900 + seed)
        m, n, k = int(rng.integers(1, 40)), int(rng.integers(1, 40)), int(rng.integers(1, 6))
        lens = rng.integers(0, min(n, 9) + 1, m)
        lens[rng.integers(0, m)] = 0
        Ap = np.zeros(m + 1, np.int64)
        np.cumsum(lens, out=Ap[1:])
        Aj = np.concatenate([rng.integers(0, n, L) for L in lens] + [np.zeros(0, np.int64)])    # duplicates among them
        integers = name == "plus_times"                              # (sums of small integers: exact in any order)
        safe = name in ("min_plus", "max_plus")
        Ax = srf.edge_values(rng, len(Aj), plus_safe=safe or integers, integers=integers)
        X = srf.edge_values(rng, n * k, plus_safe=safe or integers, integers=integers).reshape(n, k)
        if integers:
            Ax, X = np.where(np.isfinite(Ax), Ax, 2.0), np.where(np.isfinite(X), X, -3.0)
        for dtype in (np.float64, np.float32):
            a, x = Ax.astype(dtype).astype(np.float64), X.astype(dtype).astype(np.float64)
            B = (np.arange(n + 1) * k, np.tile(np.arange(k), n), x.ravel())
            want = srf.semiring_masked(name, m, k, (Ap, Aj, a), B, np.arange(m + 1) * k, np.tile(np.arange(k), m), dtype)
            got, changed = sr.spmm_semiring(name, m, n, Ap, Aj, Ax, X, dtype=dtype)
            if name == "plus_times":                                 # (the sign of a zero sum is not specified: as numbers)
                assert got.dtype == want.dtype and np.array_equal(got.ravel(), want), (name, seed, dtype)
            else:
                assert srf.same_bits(got.ravel(), want), (name, seed, dtype)
            ident = np.asarray(srf.identity(name), dtype)
            with np.errstate(invalid="ignore"):
                assert changed == np.count_nonzero(~((got == ident) | (np.isnan(got) & np.isnan(ident)))), (name, seed)
            assert np.all(got[lens == 0] == ident)


def test_spmvsrref_against_the_plus_times_reference():
    for seed in range(6):
        rng = np.random.default_rng(950 + seed)
        m, n, k = int(rng.integers(1, 50)), int(rng.integers(1, 50)), int(rng.integers(1, 6))
        lens = rng.integers(0, 12, m)
        Ap = np.zeros(m + 1, np.int64)
        np.cumsum(lens, out=Ap[1:])
        Aj = np.concatenate([rng.integers(0, n, L) for L in lens] + [np.zeros(0, np.int64)])
        Ax = rng.integers(-4, 5, len(Aj)).astype(np.float64)
        X, Y = rng.integers(-3, 4, (n, k)).astype(np.float64), rng.integers(-3, 4, (m, k)).astype(np.float64)
        for dtype in (np.float64, np.float32):
            assert np.array_equal(sr.spmm_semiring("plus_times", m, n, Ap, Aj, Ax, X, dtype=dtype)[0],
                                  spmvref.spmm(m, n, Ap, Aj, Ax, X, dtype=dtype)[0]), seed
            assert np.array_equal(sr.spmm_semiring("plus_times", m, n, Ap, Aj, Ax, X, Y, accumulate=True, dtype=dtype)[0],
                                  spmvref.spmm(m, n, Ap, Aj, Ax, X, 1.0, 1.0, Y, dtype)[0]), seed
            assert np.array_equal(sr.spmm_semiring("plus_pair", m, n, Ap, Aj, Ax, X, dtype=dtype)[0],
                                  np.repeat(lens[:, None], k, axis=1).astype(dtype)), seed


# ---------------------------------------------------------------- graph.py's loops on the reference, against scipy
def reference_step(bh, semiring, m, n, A, X, Y=None, mask=None, accumulate=False, complement=False):
    """dense.csr_spmm_semiring_device on host tensors, computed by the numpy reference"""
    Ap, Aj, Ax = (None if t is None else t.numpy() for t in A)
    out, changed = sr.spmm_semiring(semiring, m, n, Ap, Aj, Ax, X.numpy(), None if Y is None else Y.numpy(),
                                    None if mask is None else mask.numpy(), accumulate, complement)
    Y.copy_(torch.from_numpy(out))
    bh.spmv_ms, bh.spmv_changed = 0.5, changed
    return Y, changed


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


def test_graph_loops_on_the_reference_against_scipy(monkeypatch):
    from benchmark_spgemm_using_csr_amd import facade, graph
    monkeypatch.setattr(graph, "csr_spmm_semiring_device", reference_step)
    bh = facade.bhsparse()
    for seed, (n, degree) in enumerate(((40, 2), (60, 1), (25, 4))):
        Ap, Aj, Ax = random_digraph(n, degree, 300 + seed)
        A = (torch.from_numpy(Ap), torch.from_numpy(Aj), torch.from_numpy(Ax))
        sources = [0, n // 2, n - 1]
        levels, dist = scipy_levels_and_distances(n, Ap, Aj, Ax, sources)
        assert (levels == 0).any() or degree > 1
        assert np.array_equal(graph.bfs_levels_device(bh, n, A, sources).numpy(), levels), seed
        assert np.array_equal(graph.sssp_device(bh, n, A, sources).numpy(), dist), seed
        assert np.array_equal(graph.bfs_levels_device(bh, n, A, n // 2).numpy()[:, 0], levels[:, 1]), seed
        lv, steps, ms = graph._bfs(bh, n, A, sources)
        assert steps == int(levels.max()) and ms == 0.5 * steps     # (the last step finds nothing new)
    # a cycle of negative weight is reported, not looped over for ever
    Ap, Aj, Ax = np.array([0, 1, 2, 3], np.int32), np.array([2, 0, 1], np.int32), np.array([1.0, 1.0, -3.0])
    with pytest.raises(facade.BhsparseError):
        graph.sssp_device(bh, 3, (torch.from_numpy(Ap), torch.from_numpy(Aj), torch.from_numpy(Ax)), 0)
    d, sweeps, _ = graph._sssp(bh, 3, (torch.from_numpy(Ap), torch.from_numpy(Aj), torch.from_numpy(np.abs(Ax))), 0, None)
    assert d[:, 0].tolist() == [0.0, 1.0, 4.0] and sweeps == 3
