"""CPU tests of the aggregation (bhs_csr_aggregate_device) and of the multigrid setup on top of it: the numpy restatement
(tests/aggref.py) agrees with itself -- the library's rounds against the greedy distance-2 independent set by its definition
-- and with cases written out by hand; the structural properties hold on every symmetric case the GPU tests run; both
libraries export the entry point the header declares and contain its kernels, the build tracks the new sources, the C++
facade's extension method compiles and links (tests/aggregate; tests/test_aggregate_gpu.py runs the same binary on a GPU);
amg.py's setup and cycle, run on numpy / scipy restatements in place of the device calls, build the hierarchy scipy builds;
and the reference hierarchy converges."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import pytest
import scipy.sparse as sp
import torch

from conftest import ROOT
import aggref as ar

from benchmark_spgemm_using_csr_amd import _lib

ENTRY = "bhs_csr_aggregate_device"
FAMILIES = ("agg_init", "agg_near", "agg_decide", "agg_scan", "agg_join")
DEMO_DIR = os.path.join(ROOT, "tests", "aggregate")
SEEDS = (0, 1, 12345)


# ---------------------------------------------------------------- the interfaces
def test_header_declares_the_entry_point():
    txt = open(_lib.HEADER).read()
    decl = set(re.findall(r"BHS_API\s+[\w\s\*]+?\b(bhs_\w+)\s*\(", txt))
    assert ENTRY in decl and ENTRY in _lib.SYMBOLS
    vp, i = C.c_void_p, C.c_int
    assert _lib.SYMBOLS[ENTRY] == (i, [vp, i, i, vp, vp, vp, C.c_uint, i, vp, vp, C.POINTER(i), C.POINTER(i), C.POINTER(C.c_double)])
    # the ctypes signature against the declaration's own parameter list
    flat = re.sub(r"/\*.*?\*/", " ", txt, flags=re.S)
    params = re.search(r"%s\s*\((.*?)\);" % ENTRY, flat, re.S).group(1).split(",")
    kinds = []
    for p in params:
        p = " ".join(p.split())
        kinds.append("ptr" if "*" in p else "uint" if p.startswith("unsigned") else "int")
    want = ["uint" if t is C.c_uint else "int" if t is i else "ptr" for t in _lib.SYMBOLS[ENTRY][1]]
    assert kinds == want and len(kinds) == 13
    assert txt.index("---- sparse frontier x CSR") < txt.index("---- aggregation") < txt.index("---- input preparation")
    sections = re.findall(r"/\* ---- ([^-]+?) -+", txt)
    assert sections[sections.index("sparse frontier x CSR") + 1] == "aggregation"
    assert sections[sections.index("aggregation") + 1] == "input preparation"
    sect = txt[txt.index("---- aggregation"):txt.index("---- input preparation")]
    for fam in FAMILIES:
        assert fam in sect, fam
    for words in ("values are NOT TAKEN", "0x9e3779b9", "0x85ebca6b", "0xc2b2ae35", "prio31(i) << 31 | i", "greedy distance-2",
                  "ascending vertex order", "never its own", "singleton aggregate", "Non-symmetric S", "the double and the float",
                  "BHS_ERR_INTERNAL", "after n + 1 rounds", "ahead of the dependent read", "n == 0 succeeds"):
        assert words in sect, words
    host = open(os.path.join(_lib.CSRC, "bhs_host_aggregate.inc.h")).read()
    for fam in FAMILIES:
        assert '"%s"' % fam in host, fam


def test_both_libraries_export_the_entry_point(hiplib):
    for path in (_lib.SO_PATH, _lib.SO_PATH_F32):
        raw = C.CDLL(path)
        assert getattr(raw, ENTRY) is not None
        blob = open(path, "rb").read()
        for kern in (b"k_agg_init", b"k_agg_near", b"k_agg_decide", b"k_agg_count", b"k_agg_number", b"k_agg_join"):
            assert kern in blob, (path, kern)


def test_sources_are_tracked_by_the_build():
    assert "bhs_aggregate.hip.h" in _lib.SOURCES and "bhs_host_aggregate.inc.h" in _lib.SOURCES
    mk = open(os.path.join(_lib.CSRC, "Makefile")).read()
    assert "bhs_aggregate.hip.h" in mk and "bhs_host_aggregate.inc.h" in mk
    unit = open(os.path.join(_lib.CSRC, "bhsparse_hip.hip")).read()
    incs = re.findall(r'#include "(bhs_host_\w+\.inc\.h)"', unit)
    assert incs[incs.index("bhs_host_push_sr.inc.h") + 1] == "bhs_host_aggregate.inc.h"
    assert "SideWs aggWs;" in unit
    assert "release(h->aggWs)" in open(os.path.join(_lib.CSRC, "bhs_host_cabi.inc.h")).read()
    host = open(os.path.join(_lib.CSRC, "bhs_host_aggregate.inc.h")).read()
    assert '#include "bhs_aggregate.hip.h"' in host and "guarded(h," in host and host.count("side_scan(") == 1
    assert host.count("BHS_ERR_INTERNAL") >= 2 and "side_read_ctl(" in host
    kernels = open(os.path.join(_lib.CSRC, "bhs_aggregate.hip.h")).read()
    code = re.sub(r"//.*", "", kernels)
    assert "asm" not in code and not re.search(r"atomic\w*\s*\(", code)      # no atomics on results (the count goes through smv_count)
    assert not re.search(r"\bwhile\s*\(\s*(1|true)\s*\)|for\s*\(\s*;\s*;\s*\)", code)   # nothing spins
    assert len(re.findall(r"__global__", code)) == len(re.findall(r"__global__ __launch_bounds__\(256\)", code)) == 6


def test_null_handle_and_missing_platform(hiplib):
    assert hiplib.bhs_csr_aggregate_device(None, 0, 0, None, None, None, 0, 0, None, None, None, None, None) == _lib.BHS_ERR_INVALID_ARG
    from benchmark_spgemm_using_csr_amd import amg, facade
    bh = facade.bhsparse()
    assert amg.aggregate_raw_device(bh, 0, 0, None, None, None, 0, 0, None, None) == _lib.BHS_ERR_NOT_READY


def test_python_module_has_the_calls():
    from benchmark_spgemm_using_csr_amd import amg, facade
    sig = lambda f: list(inspect.signature(f).parameters)           # noqa: E731
    assert sig(amg.aggregate_raw_device) == ["bh", "n", "nnzS", "d_rowPtrS", "d_colIndS", "d_prio", "seed", "flags", "d_agg", "d_roots"]
    assert sig(amg.aggregate_device) == ["bh", "n", "S", "seed", "prio"]
    assert sig(amg.strength_device) == ["bh", "n", "A", "theta"]
    assert sig(amg.tentative_device) == ["bh", "n", "agg", "nagg", "cand"]
    assert sig(amg.sa_setup_device) == ["handles", "n", "A", "theta", "omega", "max_levels", "min_coarse", "seed"]
    assert sig(amg.sa_setup_csr)[:9] == ["n", "Ap", "Aj", "Ax", "theta", "omega", "max_levels", "min_coarse", "seed"]
    assert sig(amg.vcycle_device)[:7] == ["bh", "levels", "b", "x", "omega_jacobi", "pre", "post"]
    assert sig(amg.solve_device) == ["bh", "levels", "b", "tol", "maxiter"]
    assert not hasattr(facade.bhsparse, "aggregate_device")         # a function of a handle, not a method of it
    assert "atomic" not in inspect.getsource(amg.tentative_device).replace("no scattered sum", "")


def test_cpp_facade_extension_builds(hiplib):
    src = open(os.path.join(ROOT, "benchmark_spgemm_using_csr_amd", "host", "bhsparse.h")).read()
    flat = re.sub(r"\s+", " ", src)
    assert ("int csr_aggregate_device(int n, int nnzS, const index_type *d_rowPtrS, const index_type *d_colIndS, "
            "const unsigned *d_prio, unsigned seed, int flags, index_type *d_agg, index_type *d_roots, int *nagg_out, "
            "int *rounds_out);") in flat
    subprocess.check_call(["make", "-C", DEMO_DIR, "-s"])
    demo = os.path.join(DEMO_DIR, "aggregate_demo")
    assert os.access(demo, os.X_OK)
    out = subprocess.run(["nm", "-D", "--undefined-only", demo], capture_output=True, text=True).stdout
    assert ENTRY in out
    assert "tests/aggregate/aggregate_demo" in open(os.path.join(ROOT, ".gitignore")).read().split()


# ---------------------------------------------------------------- the restatement
def test_the_hash_by_hand():
    # vertex 0, seed 0, the header's five lines step by step
    h = 0x9e3779b9
    h ^= h >> 16
    h = (h * 0x85ebca6b) & 0xFFFFFFFF
    h ^= h >> 13
    h = (h * 0xc2b2ae35) & 0xFFFFFFFF
    h ^= h >> 16
    assert int(ar.hash32(0, 0)) == h and int(ar.hash32(5, 5)) == h   # (i ^ seed) alone enters
    k = ar.keys(4, 7)
    assert k.dtype == np.uint64 and [int(x) & 0x7FFFFFFF for x in k] == [0, 1, 2, 3]
    assert [int(x) >> 31 for x in k] == [int(ar.hash32(i, 7)) >> 1 for i in range(4)] and int(k.max()) < 1 << 62
    assert [int(x) >> 31 for x in ar.keys(3, 0, [5, 4, 0xFFFFFFFF])] == [2, 2, 0x7FFFFFFF]


def test_a_path_of_seven_by_hand():
    """0 - 1 - 2 - 3 - 4 - 5 - 6 with priorities 10 50 20 30 40 90 60 (prio31: half of each).  Descending: 5, 6, 1, 4, 3, 2, 0.
    5 is a root and shuts out 3, 4, 6; 1 is the next one free (6 is out) and shuts out 0, 2, 3.  Roots {1, 5}, numbered
    ascending: 1 -> 0, 5 -> 1.  Pass 1: 0 and 2 join 1; 4 and 6 join 5.  Pass 2: 3 has the placed neighbours 2 (prio 20) and 4
    (prio 40): it joins 4's aggregate, 1."""
    n = 7
    Sp = np.array([0, 1, 3, 5, 7, 9, 11, 12], np.int32)
    Sj = np.array([1, 0, 2, 1, 3, 2, 4, 3, 5, 4, 6, 5], np.int32)
    prio = [10, 50, 20, 30, 40, 90, 60]
    agg, nagg, roots, rounds = ar.aggregate(n, Sp, Sj, 0, prio)
    assert nagg == 2 and roots.tolist() == [1, 5] and agg.tolist() == [0, 0, 0, 1, 1, 1, 1]
    assert rounds == 2                                               # 5 in the first round, 1 once 3 and 6 are out
    assert agg.dtype == np.int32 and roots.dtype == np.int32
    # the lowest bit of a priority is dropped: 41 ties with 40, the index decides -- nothing changes for vertex 4 here
    assert ar.aggregate(n, Sp, Sj, 0, [10, 50, 20, 30, 41, 90, 60])[0].tolist() == agg.tolist()
    # with 2 above 4, vertex 3 goes the other way
    assert ar.aggregate(n, Sp, Sj, 0, [10, 50, 44, 30, 40, 90, 60])[0].tolist() == [0, 0, 0, 0, 1, 1, 1]


def test_star_and_cliques():
    n, Sp, Sj = ar.star(1024)
    for seed in range(8):
        agg, nagg, roots, rounds = ar.aggregate(n, Sp, Sj, seed)
        assert nagg == 1 and not agg.any() and rounds <= 2           # every vertex is within two steps of every other
    n, Sp, Sj = ar.two_cliques(70)
    for seed in SEEDS:
        agg, nagg, roots, _ = ar.aggregate(n, Sp, Sj, seed)
        assert nagg == 2 and agg[:70].tolist() == [0] * 70 and agg[70:].tolist() == [1] * 70


@pytest.mark.parametrize("name", sorted(ar.gpu_cases()))
def test_rounds_equal_greedy_and_the_structure_holds(name):
    n, Sp, Sj = ar.gpu_cases()[name]
    prios = [None, np.random.default_rng(1).integers(0, 2 ** 32, n, dtype=np.uint64), np.full(n, 12)]
    for seed, prio in [(s, None) for s in SEEDS] + [(0, p) for p in prios[1:]]:
        key = ar.keys(n, seed, prio)
        root, rounds = ar.rounds(n, Sp, Sj, key)
        assert np.array_equal(root, ar.greedy(n, Sp, Sj, key)), (name, seed)
        assert 1 <= rounds <= n
        agg, roots = ar.join(n, Sp, Sj, key, root)
        ar.check_structure(n, Sp, Sj, agg, len(roots), roots)
    deg = np.diff(Sp)
    if name == "powerlaw3000":
        assert deg.max() > 512                                       # a hub beyond every lanes-per-row and wave boundary
    if name == "roadlike40":
        assert (deg == 1).any()                                      # isolated vertices (the diagonal alone)
    if name == "uniform2048":
        assert deg.max() >= 12


def test_invalid_names_what_is_refused():
    n, Sp, Sj = ar.gpu_cases()["poisson5pt_33"]
    nnz = len(Sj)
    assert ar.invalid(n, nnz, Sp, Sj) is None and ar.invalid(0, 0, None, None) is None
    assert ar.invalid(-1, 0, Sp, Sj) == "negative size" and ar.invalid(n, nnz, Sp, Sj, flags=1) == "unknown flag"
    assert ar.invalid(n, nnz, Sp, Sj, has_agg=False) == "NULL array" and ar.invalid(n, nnz, Sp, Sj, overlap=True) == "an output overlaps an input"
    for col in (n, -1):
        j = Sj.copy()
        j[7] = col
        assert ar.invalid(n, nnz, Sp, j) == "column out of range"
    p = Sp.copy()
    p[100] = p[99] - 1
    assert ar.invalid(n, nnz, p, Sj) == "bad row pointer"
    p = Sp.copy()
    p[n] = nnz + 3
    assert ar.invalid(n, nnz, p, Sj) == "bad row pointer"


# ---------------------------------------------------------------- the hierarchy on the restatements
COARSE = {("poisson5pt", 33, 33): (162, 158, 169), ("poisson9pt", 20, 20): (34, 36, 36), ("poisson7pt", 10, 10, 10): (109, 102, 105),
          ("poisson27pt", 9, 9, 9): (25, 24, 27)}
CONVERGE = (("poisson5pt", 33, 33), ("poisson5pt", 64, 64), ("poisson9pt", 20, 20), ("poisson7pt", 10, 10, 10),
            ("poisson27pt", 9, 9, 9), ("poisson27pt", 16, 16, 16))


def test_coarse_sizes():
    for args, want in COARSE.items():
        n, Ap, Aj, _ = ar.poisson(*args)
        assert tuple(ar.aggregate(n, Ap, Aj, seed)[1] for seed in SEEDS) == want, args


@pytest.mark.parametrize("args", CONVERGE, ids=lambda a: "%s_%d" % (a[0], a[1]))
def test_ten_cycles_converge(args):
    """Ten V(1,1) cycles, omega = 2/3, theta = 0, min_coarse 40, Poisson values, a random right-hand side: the tenth
    residual is below 0.75^10 of the first."""
    n, Ap, Aj, Ax = ar.poisson(*args)
    A = sp.csr_matrix((Ax, Aj, Ap), shape=(n, n))
    for seed in SEEDS:
        levels, sizes = ar.sa_setup(A, seed=seed)
        assert len(levels) >= 2
        b = np.random.default_rng(seed).standard_normal(n)
        x = np.zeros(n)
        for _ in range(10):
            x = ar.vcycle(levels, b, x)
        rate = (np.linalg.norm(b - A @ x) / np.linalg.norm(b)) ** 0.1
        print("%s seed %d: sizes %s, average reduction %.3f" % (args, seed, sizes, rate))
        assert rate < 0.75, (args, seed, rate)


class HostHandle(object):
    """the device methods amg.py calls, computed by scipy on host tensors"""
    _vdt = np.dtype(np.float64)

    def __init__(self):
        self.select_ms = self.transpose_ms = self.add_ms = self.reduce_ms = self.scale_ms = 0.125
        self.stage_ms = [0.25] * 4
        self.calls = []

    @staticmethod
    def mat(X, shape, ones=False):
        p, j, x = X
        data = np.ones(j.numel()) if (ones or x is None) else x.numpy().astype(np.float64)
        return sp.csr_matrix((data, j.numpy(), p.numpy()), shape=shape)

    @staticmethod
    def tens(M, values=True):
        M = sp.csr_matrix(M)
        M.sort_indices()
        return (torch.from_numpy(M.indptr.astype(np.int32)), torch.from_numpy(M.indices.astype(np.int32)),
                torch.from_numpy(M.data.astype(np.float64)) if values else None)

    def csr_select_device(self, m, n, X, spec, values=True):
        assert spec.flags == _lib.BHS_SEL_REL | _lib.BHS_SEL_KEEP_DIAG and not values
        self.calls.append("select")
        A = self.mat(X, (m, n))
        r = np.repeat(np.arange(m), np.diff(A.indptr))
        diag = r == A.indices
        rowmax = np.zeros(m)
        np.maximum.at(rowmax, r[~diag], np.abs(A.data[~diag]))
        keep = ~(np.abs(A.data) < spec.rel_tol * rowmax[r]) | diag
        return self.tens(sp.csr_matrix((np.ones(int(keep.sum())), (r[keep], A.indices[keep])), shape=(m, n)), False)

    def csr_transpose_device(self, m, n, X, values=True, perm=False):
        self.calls.append("transpose")
        keep = values and X[2] is not None
        T = ar.on_pattern(self.mat(X, (m, n)).T, self.mat(X, (m, n), ones=True).T)
        return self.tens(T, keep) + (None,)

    def csr_add_device(self, m, n, alpha, X, beta, Y):
        self.calls.append("add")
        Z = ar.on_pattern(alpha * self.mat(X, (m, n)) + beta * self.mat(Y, (m, n)), self.mat(X, (m, n), True) + self.mat(Y, (m, n), True))
        return self.tens(Z) + (0,)

    def csr_reduce_device(self, m, n, X, axis, op, offdiag=False):
        self.calls.append("reduce")
        A = self.mat(X, (m, n))
        if (axis, op) == (_lib.BHS_AXIS_DIAG, _lib.BHS_RED_PLUS):
            return torch.from_numpy(A.diagonal().copy())
        assert (axis, op) == (_lib.BHS_AXIS_ROWS, _lib.BHS_RED_SQ_PLUS)
        return torch.from_numpy(np.asarray(A.multiply(A).sum(axis=1)).ravel())

    def csr_scale_device(self, m, n, X, alpha=1.0, left=None, right=None, left_div=False, right_div=False, out=None):
        self.calls.append("scale")
        A = self.mat(X, (m, n))
        r = np.repeat(np.arange(m), np.diff(A.indptr))
        v = alpha * A.data
        if left is not None:
            v = v / left.numpy()[r] if left_div else v * left.numpy()[r]
        if right is not None:
            v = v / right.numpy()[A.indices] if right_div else v * right.numpy()[A.indices]
        return torch.from_numpy(v)

    def initData_device(self, m, k, n, nnzA, Ax, Ap, Aj, nnzB, Bx, Bp, Bj):
        assert nnzA == Aj.numel() and nnzB == Bj.numel()
        self.A, self.B = (Ap, Aj, Ax), (Bp, Bj, Bx)
        self.dims = (m, k, n)
        return 0

    def _product(self):
        m, k, n = self.dims
        A, B = self.mat(self.A, (m, k)), self.mat(self.B, (k, n))
        return A @ B, self.mat(self.A, (m, k), True) @ self.mat(self.B, (k, n), True)

    def spgemm(self):
        self.calls.append("spgemm")
        self.C = self.tens(ar.on_pattern(*self._product()))
        return 0

    def spgemm_add_device(self, alpha, beta, nnzD, Dx, Dp, Dj):
        self.calls.append("spgemm_add")
        m, _, n = self.dims
        AB, pat = self._product()
        D = self.mat((Dp, Dj, Dx), (m, n))
        self.C = self.tens(ar.on_pattern(alpha * AB + beta * D, pat + self.mat((Dp, Dj, Dx), (m, n), True)))
        return 0

    def get_nnzC(self):
        return int(self.C[1].numel())

    def get_C_device(self):
        return self.C                                                # (host tensors stand in for the device addresses)

    def free_mem(self):
        return 0


def host_spmv(bh, m, n, A, x, alpha=1.0, beta=0.0, y=None):
    out = alpha * (HostHandle.mat(A, (m, n)) @ x.numpy())
    if y is not None and beta != 0.0:
        out = out + beta * y.numpy()
    return torch.from_numpy(out)


def host_aggregate(bh, n, S, seed=0, prio=None):
    agg, nagg, roots, rounds = ar.aggregate(n, S[0].numpy(), S[1].numpy(), seed, prio)
    bh.aggregate_ms, bh.aggregate_nagg, bh.aggregate_rounds = 0.5, nagg, rounds
    bh.calls.append("aggregate")
    return torch.from_numpy(agg), nagg, torch.from_numpy(roots)


@pytest.fixture
def on_the_host(monkeypatch):
    from benchmark_spgemm_using_csr_amd import amg
    monkeypatch.setattr(amg, "aggregate_device", host_aggregate)
    monkeypatch.setattr(amg, "csr_spmv_device", host_spmv)
    monkeypatch.setattr(amg, "_result_device", lambda bh, rows, dev: tuple(t.clone() for t in bh.get_C_device()))
    return amg


def rel(got, want):
    want = sp.csr_matrix(want)
    return abs(got - want).max() / abs(want).max()


@pytest.mark.parametrize("args", (("poisson5pt", 33, 33), ("poisson27pt", 9, 9, 9)), ids=("poisson5pt_33", "poisson27pt_9"))
def test_setup_and_cycle_on_the_restatements(on_the_host, args):
    amg = on_the_host
    n, Ap, Aj, Ax = ar.poisson(*args)
    A = sp.csr_matrix((Ax, Aj, Ap), shape=(n, n))
    dA = HostHandle.tens(A)
    h1, h2 = HostHandle(), HostHandle()
    omega = 2.0 / 3.0
    levels, info = amg.sa_setup_device((h1, h2), n, dA, seed=1)
    ref_levels, ref_sizes = ar.sa_setup(A, seed=1)
    assert [rec["n"] for rec in info] == [n] + ref_sizes and len(levels) == len(ref_levels)
    assert h1.calls[:6] == ["select", "transpose", "add", "aggregate", "transpose", "reduce"]
    for lvl, (Al, P, R) in enumerate(levels[:-1]):
        rows, nc = info[lvl]["n"], info[lvl]["nagg"]
        Am, Pm, Rm = HostHandle.mat(Al, (rows, rows)), HostHandle.mat(P, (rows, nc)), HostHandle.mat(R, (nc, rows))
        Ac = HostHandle.mat(levels[lvl + 1][0], (nc, nc))
        assert rel(Ac, Pm.T @ Am @ Pm) <= 1e-12                      # the Galerkin product
        assert rel(Rm, Pm.T) == 0.0
        assert rel(Pm, ref_levels[lvl][1]) <= 1e-12 and rel(Am, ref_levels[lvl][0]) <= 1e-12
        # the tentative prolongator of this level's aggregates: unit columns, and P coarse_cand = (I - omega D^-1 A) 1
        S = amg.strength_device(h1, rows, Al, 0.0)
        agg, nagg, _ = amg.aggregate_device(h1, rows, S, 1)
        assert nagg == nc
        T, cc = amg.tentative_device(h1, rows, agg, nagg)
        Tm = HostHandle.mat(T, (rows, nc))
        assert np.allclose(np.sqrt(np.asarray(Tm.multiply(Tm).sum(axis=0)).ravel()), 1.0, rtol=0, atol=1e-14)
        assert np.array_equal(Tm.indices, agg.numpy()) and np.array_equal(Tm.indptr, np.arange(rows + 1))
        ones = np.ones(rows)
        want = ones - omega * (Am @ ones) / Am.diagonal()
        assert np.allclose(Pm @ cc.numpy(), want, rtol=0, atol=1e-13)
        assert set(info[lvl]) == {"n", "nnz", "nagg", "rounds", "strength_ms", "aggregate_ms", "prolongator_ms", "galerkin_ms"}
    assert levels[-1][1] is None and levels[-1][2] is None and set(info[-1]) == {"n", "nnz"}
    # the cycle and the solver against the scipy restatement
    b = np.random.default_rng(4).standard_normal(n)
    x = amg.vcycle_device(h1, levels, torch.from_numpy(b), torch.zeros(n, dtype=torch.float64))
    want = ar.vcycle(ref_levels, b, np.zeros(n))
    assert np.allclose(x.numpy(), want, rtol=0, atol=1e-12 * np.abs(want).max())
    x, cycles, res = amg.solve_device(h1, levels, torch.from_numpy(b), 1e-8, 100)
    _, ref_cycles, ref_res = ar.solve(ref_levels, b, 1e-8, 100)
    assert cycles == ref_cycles and res[-1] <= 1e-8 * res[0]
    assert np.linalg.norm(b - A @ x.numpy()) <= 1.01e-8 * np.linalg.norm(b)


def test_setup_stops_where_it_should(on_the_host):
    amg = on_the_host
    n, Ap, Aj, Ax = ar.poisson("poisson5pt", 33, 33)
    dA = HostHandle.tens(sp.csr_matrix((Ax, Aj, Ap), shape=(n, n)))
    levels, info = amg.sa_setup_device((HostHandle(), HostHandle()), n, dA, max_levels=2)
    assert len(levels) == 2 and info[1]["n"] == 162
    levels, info = amg.sa_setup_device((HostHandle(), HostHandle()), n, dA, min_coarse=200)
    assert [rec["n"] for rec in info] == [1089, 162]
    levels, info = amg.sa_setup_device((HostHandle(), HostHandle()), n, dA, min_coarse=2000)
    assert len(levels) == 1 and levels[0][1] is None
    made = []

    class Owned(HostHandle):
        def freePlatform(self):
            made.append(self)
    levels, info = amg.sa_setup_device(Owned, n, dA)
    assert len(made) == 2 and [rec["n"] for rec in info] == [1089, 162, 14]
