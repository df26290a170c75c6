"""The level sets (bhs_csr_levels_device), the sparse triangular solve (bhs_csr_trsv_device), ILU(0) in place
(bhs_csr_ilu0_device) and the ILU(0)-preconditioned CG of benchmark_spgemm_using_csr_amd/amg.py, on the GPU, both builds.

Reference: tests/iluref.py, the contract of include/bhsparse_hip.h ("triangular solve and ILU(0)") restated in numpy.  The
levels are a function of the pattern, so d_level, d_order, the offsets and nlevels are compared exactly.  The solve and the
factorisation are compared bit for bit where every intermediate is a small dyadic number -- the solve's right-hand side is
made from an integer solution, the factorisation's matrix from integer factors -- and by componentwise backward error
(the solve) and the defining identity on the pattern (the factorisation) on random values.  Sentinels sit behind every output;
they must be intact, also after a refused call."""
import functools
import os
import subprocess

import numpy as np
import pytest
import scipy.sparse as sp
import torch

from conftest import ROOT
import aggref as ar
import iluref as ir

from benchmark_spgemm_using_csr_amd import _lib, amg
from benchmark_spgemm_using_csr_amd.facade import BHSPARSE_HIP, NUM_PLATFORMS, bhsparse

pytestmark = pytest.mark.gpu

DTYPES = (np.float64, np.float32)
INV = _lib.BHS_ERR_INVALID_ARG
LOWER, UPPER, UNIT = _lib.BHS_TRI_LOWER, _lib.BHS_TRI_UPPER, _lib.BHS_TRI_UNIT_DIAG
PAD = 64
SENT = -7
XSENT = -123.5
LEVEL_FAMILIES = {"levels_pass", "levels_order"}
TRSV_FAMILIES = {"trsv_level"}
PATTERNS = ("one_with_diag", "one_without_diag", "path300", "poisson5pt_33", "poisson27pt_9", "uniform2048", "powerlaw3000",
            "star1024", "two_k70", "lower_random")


def new_handle(dtype=np.float64):
    plats = [False] * NUM_PLATFORMS
    plats[BHSPARSE_HIP] = True
    bh = bhsparse(value_dtype=dtype)
    assert bh.initPlatform(plats) == 0
    return bh


@pytest.fixture(scope="module", params=DTYPES, ids=("f64", "f32"))
def hd(request):
    bh = new_handle(request.param)
    yield bh, request.param
    bh.freePlatform()


def up(a, dt):
    return torch.from_numpy(np.ascontiguousarray(a, dt).copy()).cuda()


def tdt(dtype):
    return torch.float32 if dtype == np.float32 else torch.float64


def unit(dtype):
    return 2.0 ** -53 if dtype == np.float64 else 2.0 ** -24


def launches(bh):
    return {s["name"]: s["launches"] for s in bh.kernel_stats() if s["launches"] > 0}


@functools.lru_cache(maxsize=None)
def pattern(name):
    """(n, Ap, Aj): aggref's symmetric patterns as they are (with and without diagonal entries), and a random strictly lower,
    non-symmetric one whose rows are not ascending"""
    if name == "lower_random":
        rng = np.random.default_rng(23)
        n = 1500
        rows = [rng.integers(0, i, min(i, int(rng.integers(0, 7)))) for i in range(n)]     # (repeats and any order inside a row)
        Ap = np.zeros(n + 1, np.int32)
        np.cumsum([len(r) for r in rows], out=Ap[1:])
        return n, Ap, np.concatenate(rows).astype(np.int32)
    return ar.gpu_cases()[name]


@functools.lru_cache(maxsize=None)
def with_diagonal(name):
    """the pattern with a diagonal entry in every row, rows strictly ascending: (n, Ap, Aj)"""
    n, Ap, Aj = pattern(name)
    S = sp.csr_matrix((np.ones(len(Aj)), Aj, Ap), shape=(n, n)) + sp.identity(n, format="csr")
    S = S.tocsr()
    S.sum_duplicates()
    S.sort_indices()
    return n, S.indptr.astype(np.int32), S.indices.astype(np.int32)


@functools.lru_cache(maxsize=None)
def level_reference(name, upper, diagonal=False):
    n, Ap, Aj = with_diagonal(name) if diagonal else pattern(name)
    return ir.levels(n, Ap, Aj, upper)


# ---------------------------------------------------------------- the levels
def levels_run(bh, n, Ap, Aj, flags=LOWER, want=0, what="", nnz=None):
    """The device's answer (level, nlevels, order, levelPtr, passes) as numpy; the sentinels behind the outputs are checked."""
    dAp = up(Ap, np.int32) if len(Ap) else torch.zeros(1, dtype=torch.int32).cuda()
    dAj = up(Aj, np.int32) if len(Aj) else torch.zeros(1, dtype=torch.int32).cuda()
    room = max(n, 0)
    level = torch.full((room + PAD,), SENT, dtype=torch.int32).cuda()
    order = torch.full((room + PAD,), SENT, dtype=torch.int32).cuda()
    lptr = torch.full((room + 1 + PAD,), SENT, dtype=torch.int32).cuda()
    torch.cuda.synchronize()
    bh.levels_nlevels = bh.levels_passes = -1
    err = amg.levels_raw_device(bh, n, len(Aj) if nnz is None else nnz, dAp, dAj if len(Aj) else None, flags, level, order, lptr)
    assert err == want, (what, err)
    assert bool((level[room:] == SENT).all()) and bool((order[room:] == SENT).all()), (what, "written past the end")
    assert bool((lptr[room + 1:] == SENT).all()), (what, "written past the end of d_levelPtr")
    if want != 0:
        assert bh.levels_nlevels == -1
        return None
    nlevels = bh.levels_nlevels
    assert bh.levels_ms >= 0.0 and set(launches(bh)) <= LEVEL_FAMILIES, (what, launches(bh))
    if n:
        assert bool((lptr[nlevels + 1:] == SENT).all()), (what, "written behind d_levelPtr[nlevels]")
    return (level[:n].cpu().numpy(), nlevels, order[:n].cpu().numpy(),
            lptr[:nlevels + 1].cpu().numpy() if n else np.zeros(1, np.int32), bh.levels_passes)


def levels_check(got, want, what):
    level, nlevels, order, ptr, passes = got
    wlevel, wnlevels, worder, wptr = want
    assert nlevels == wnlevels, (what, nlevels, wnlevels)
    assert np.array_equal(level, wlevel), (what, "levels")
    assert np.array_equal(order, worder), (what, "order")
    assert np.array_equal(ptr, wptr), (what, "offsets")
    assert passes >= 1 or nlevels == 0, (what, passes)


def test_levels_empty(hd):
    bh, _ = hd
    for flags in (LOWER, UPPER):
        got = levels_run(bh, 0, np.zeros(1, np.int32), np.zeros(0, np.int32), flags, what="n = 0")
        assert got[1] == 0 and got[4] == 0 and len(got[0]) == 0


@pytest.mark.parametrize("name", PATTERNS)
def test_levels_against_the_restatement(hd, name):
    bh, _ = hd
    n, Ap, Aj = pattern(name)
    for upper in (False, True):
        want = level_reference(name, upper)
        levels_check(levels_run(bh, n, Ap, Aj, UPPER if upper else LOWER, what=(name, upper)), want, (name, upper))
    counts = {"path300": 300, "poisson5pt_33": 65, "poisson27pt_9": 57, "two_k70": 70, "star1024": 2, "one_with_diag": 1,
              "one_without_diag": 1}
    if name in counts:
        assert level_reference(name, False)[1] == counts[name] == level_reference(name, True)[1]
    if name == "powerlaw3000":
        assert np.diff(Ap).max() > 512                               # a hub row beyond every lanes-per-row
    if name == "lower_random":
        assert level_reference(name, True)[1] == 1                   # nothing above the diagonal: one level


def test_levels_handles_and_libraries_agree():
    n, Ap, Aj = pattern("uniform2048")
    outs = []
    for dtype in DTYPES:
        bh = new_handle(dtype)
        try:
            outs.append(levels_run(bh, n, Ap, Aj, LOWER))
            outs.append(levels_run(bh, n, Ap, Aj, LOWER))            # the same handle again
        finally:
            bh.freePlatform()
    for got in outs:
        levels_check(got, level_reference("uniform2048", False), "handles")


def test_levels_refusals(hd):
    bh, _ = hd
    n, Ap, Aj = pattern("poisson5pt_33")
    nnz = len(Aj)
    for flags, what in ((0, "neither triangle"), (LOWER | UPPER, "both triangles"), (LOWER | UNIT, "a flag of the solve"), (8, "an unknown flag")):
        levels_run(bh, n, Ap, Aj, flags, want=INV, what=what)
    bad = Aj.copy(); bad[nnz // 2] = n                               # noqa: E702
    levels_run(bh, n, Ap, bad, want=INV, what="a column equal to n")
    bad = Aj.copy(); bad[5] = -1                                     # noqa: E702
    levels_run(bh, n, Ap, bad, want=INV, what="a column of -1")
    p = Ap.copy(); p[100] = p[99] - 1                                # noqa: E702
    levels_run(bh, n, p, Aj, want=INV, what="a decreasing row pointer")
    p = Ap.copy(); p[n] = nnz + 3                                    # noqa: E702
    levels_run(bh, n, p, Aj, want=INV, what="a last row pointer above nnzA", nnz=nnz)
    levels_run(bh, -1, Ap, Aj, want=INV, what="negative n")
    dAp, dAj = up(Ap, np.int32), up(Aj, np.int32)
    a, b, c = (torch.full((n + 1,), SENT, dtype=torch.int32).cuda() for _ in range(3))
    torch.cuda.synchronize()
    assert amg.levels_raw_device(bh, n, nnz, dAp, dAj, LOWER, dAj, b, c) == INV
    assert amg.levels_raw_device(bh, n, nnz, dAp, dAj, LOWER, a, a, c) == INV
    assert amg.levels_raw_device(bh, n, nnz, dAp, dAj, LOWER, a, b, b[n // 2:]) == INV
    assert amg.levels_raw_device(bh, n, nnz, dAp, dAj, LOWER, a, None, c) == INV
    assert np.array_equal(dAj.cpu().numpy(), Aj) and all(bool((t == SENT).all()) for t in (a, b, c))
    levels_check(levels_run(bh, n, Ap, Aj, LOWER, what="after the refusals"), level_reference("poisson5pt_33", False), "after the refusals")


# ---------------------------------------------------------------- the solve
class Tri(object):
    """a matrix on the device in a handle's value type, with the levels of both of its triangles (the restatement's)"""

    def __init__(self, n, Ap, Aj, Ax, dtype):
        self.n, self.nnz, self.dtype = n, len(Aj), dtype
        self.host = (np.asarray(Ap, np.int32), np.asarray(Aj, np.int32), np.asarray(Ax, np.float64))
        self.A = (up(Ap, np.int32), up(Aj, np.int32) if len(Aj) else None, up(Ax, dtype) if len(Aj) else None)
        self.lev = {}
        for upper in (False, True):
            _, nlevels, order, ptr = ir.levels(n, Ap, Aj, upper)
            self.lev[upper] = (nlevels, ptr, order, up(order, np.int32))

    def x(self, values):
        x = torch.full((self.n + PAD,), XSENT, dtype=tdt(self.dtype)).cuda()
        x[:self.n] = up(values, self.dtype)
        return x

    def run(self, bh, b, x=None, alpha=1.0, flags=LOWER, ptr=None, order=None, A=None, want=0, what="", families=None):
        """b: n values; x: a padded buffer of self.x(), or None for the solve in place on a padded copy of b.  Returns x as
        float64 on the host."""
        upper = bool(flags & UPPER)
        nlevels, hptr, _, dorder = self.lev[upper]
        hptr = hptr if ptr is None else ptr
        db = self.x(b)
        dx = db if x is None else x
        A = self.A if A is None else A
        torch.cuda.synchronize()
        err = amg.trsv_raw_device(bh, self.n, self.nnz, A[0], A[1], A[2], len(hptr) - 1, hptr, dorder if order is None else order,
                                  alpha, db, dx, flags)
        assert err == want, (what, err)
        assert bool((dx[self.n:] == XSENT).all()) and bool((db[self.n:] == XSENT).all()), (what, "written past the end")
        if want == 0:
            assert bh.trsv_ms >= 0.0 and set(launches(bh)) <= (TRSV_FAMILIES if families is None else families), (what, launches(bh))
        return dx[:self.n].cpu().numpy().astype(np.float64)


@functools.lru_cache(maxsize=None)
def exact_case(name):
    """(n, Ap, Aj, Ax, x*, b of the lower solve, b of the upper solve) for alpha = 1/2: off-diagonal entries integers in
    [-3, 3], diagonals 1/2, 1, 2 or 4, x* integers in [-8, 8] and b = 2 T x*, integers -- every row's sum, alpha b - s and
    the quotient are small integers or halves of them, exact in both value types in whatever order and however fused"""
    n, Ap, Aj = with_diagonal(name)
    rng = np.random.default_rng(31)
    r = np.repeat(np.arange(n), np.diff(Ap))
    Ax = rng.integers(-3, 4, len(Aj)).astype(np.float64)
    Ax[r == Aj] = rng.choice([0.5, 1.0, 2.0, 4.0], int((r == Aj).sum()))
    xs = rng.integers(-8, 9, n).astype(np.float64)
    A = sp.csr_matrix((Ax, Aj, Ap), shape=(n, n))
    return n, Ap, Aj, Ax, xs, 2.0 * (sp.tril(A) @ xs), 2.0 * (sp.triu(A) @ xs)


@pytest.mark.parametrize("name", PATTERNS)
def test_solve_bit_for_bit_on_exact_values(hd, name):
    """in place (d_x == d_b), both triangles: the integer solution, which is also what the restatement returns, bit for bit
    in both builds; a launch per level"""
    bh, dtype = hd
    n, Ap, Aj, Ax, xs, bl, bu = exact_case(name)
    assert np.array_equal(bl, np.round(bl)) and np.array_equal(bu, np.round(bu))
    T = Tri(n, Ap, Aj, Ax, dtype)
    for upper, b in ((False, bl), (True, bu)):
        nlevels, ptr, order, _ = T.lev[upper]
        want = ir.trsv(n, Ap, Aj, Ax, ptr, order, b, np.zeros(n), 0.5, upper, dtype=dtype).astype(np.float64)
        assert np.array_equal(want, xs)
        got = T.run(bh, b, None, 0.5, UPPER if upper else LOWER, what=(name, upper))
        assert np.array_equal(got, xs), (name, upper, int(np.flatnonzero(got != xs)[0]))
        assert launches(bh) == {"trsv_level": nlevels}, (name, launches(bh))      # (none of the levels is empty)
        assert bh.set_option("trsv_fuse", 0) == INV                  # no such option: thin levels are not fused


@functools.lru_cache(maxsize=None)
def random_case(name):
    """(n, Ap, Aj, Ax, b): float32 numbers, so that one matrix serves both builds; diagonally dominant"""
    n, Ap, Aj = with_diagonal(name)
    rng = np.random.default_rng(37)
    r = np.repeat(np.arange(n), np.diff(Ap))
    Ax = rng.uniform(-1.0, 1.0, len(Aj)).astype(np.float32).astype(np.float64)
    rowsum = np.bincount(r[r != Aj], weights=np.abs(Ax[r != Aj]), minlength=n)
    Ax[r == Aj] = (np.ceil(rowsum) + 1.0) * rng.choice([-1.0, 1.0], n)
    return n, Ap, Aj, Ax, rng.standard_normal(n).astype(np.float32).astype(np.float64)


def backward_error(n, Ap, Aj, Ax, x, b, alpha, upper, unit_diag, u):
    """max over the rows of |sum_j t_ij x_j - alpha b_i| / (2 ((len_i + 3) 2^-53 + u) (sum_j |t_ij| |x_j| + |alpha b_i|)), in
    float64 on the host; len_i the entries of row i of the triangle.  The first term is the double summation and division,
    the second the one rounding to the value type; the factor 2 is headroom, not a fit."""
    r = np.repeat(np.arange(n), np.diff(Ap))
    keep = (Aj > r) if upper else (Aj < r)
    if not unit_diag:
        keep = keep | (Aj == r)
    T = sp.csr_matrix((Ax[keep], (r[keep], Aj[keep])), shape=(n, n))
    if unit_diag:
        T = T + sp.identity(n, format="csr")
    T = T.tocsr()
    res = np.abs(T @ x - alpha * b)
    scale = abs(T) @ np.abs(x) + np.abs(alpha * b)
    length = np.diff(T.indptr)
    bound = 2.0 * ((length + 3.0) * 2.0 ** -53 + u) * scale
    return float(np.max(res / np.where(bound > 0, bound, 1.0)))


@pytest.mark.parametrize("name", PATTERNS)
def test_solve_backward_error_on_random_values(hd, name):
    bh, dtype = hd
    n, Ap, Aj, Ax, b = random_case(name)
    T = Tri(n, Ap, Aj, Ax, dtype)
    r = np.repeat(np.arange(n), np.diff(Ap))
    scaled = (Ax / Ax[r == Aj][r]).astype(np.float32).astype(np.float64)   # D^-1 A: the unit-diagonal solves stay bounded
    Tu = Tri(n, Ap, Aj, scaled, dtype)
    for upper in (False, True):
        flags = UPPER if upper else LOWER
        x = T.run(bh, b, T.x(np.zeros(n)), -0.75, flags, what=(name, upper))
        err = backward_error(n, Ap, Aj, Ax, x, b, -0.75, upper, False, unit(dtype))
        xu = Tu.run(bh, b, Tu.x(np.zeros(n)), 1.0, flags | UNIT, what=(name, upper, "unit"))
        erru = backward_error(n, Ap, Aj, scaled, xu, b, 1.0, upper, True, unit(dtype))
        print("%s %s upper %d: backward error %.3g and %.3g (unit diagonal) of the bound" % (name, np.dtype(dtype).name, upper, err, erru))
        assert np.all(np.isfinite(x)) and np.all(np.isfinite(xu)) and err <= 1.0 and erru <= 1.0, (name, upper, err, erru)


def test_solve_repeats_and_handles_agree(hd):
    bh, dtype = hd
    n, Ap, Aj, Ax, b = random_case("uniform2048")
    T = Tri(n, Ap, Aj, Ax, dtype)
    first = T.run(bh, b, T.x(np.zeros(n)))
    again = T.run(bh, b, T.x(np.zeros(n)))
    other = new_handle(dtype)
    try:
        third = T.run(other, b, T.x(np.zeros(n)))
    finally:
        other.freePlatform()
    inplace = T.run(bh, b, None)
    for got in (again, third, inplace):
        assert np.array_equal(first, got)


def test_solve_leaves_unlisted_rows_alone(hd):
    bh, dtype = hd
    n, Ap, Aj, Ax, xs, bl, _ = exact_case("poisson27pt_9")
    T = Tri(n, Ap, Aj, Ax, dtype)
    nlevels, ptr, order, _ = T.lev[False]
    keep = nlevels - 5
    x0 = np.full(n, 77.0)
    got = T.run(bh, bl, T.x(x0), 0.5, LOWER, ptr=ptr[:keep + 1])
    rest, done = order[ptr[keep]:], order[:ptr[keep]]
    assert len(rest) > 0 and np.array_equal(got[rest], x0[rest]) and np.array_equal(got[done], xs[done])
    # no level at all: nothing happens, nothing is launched
    assert np.array_equal(T.run(bh, bl, T.x(x0), 0.5, LOWER, ptr=np.zeros(1, np.int32)), x0)
    # a row without a diagonal entry: level 0 like any other, fine with a unit diagonal, refused without
    n1, Ap1, Aj1 = pattern("one_without_diag")
    one = Tri(n1, Ap1, Aj1, np.zeros(0), dtype)
    assert one.run(bh, np.array([3.0]), None, 2.0, LOWER | UNIT).tolist() == [6.0]
    one.run(bh, np.array([3.0]), None, 2.0, LOWER, want=INV, what="a listed row without a diagonal entry")


def test_solve_takes_the_first_diagonal_entry_and_adds_repeats(hd):
    """rows out of order, a column twice, two diagonal entries: the hand case of tests/test_trsv_abi.py on the device"""
    bh, dtype = hd
    Ap = np.array([0, 1, 3, 9, 10], np.int32)
    Aj = np.array([0, 1, 0, 3, 1, 2, 1, 0, 2, 3], np.int32)
    Ax = np.array([2.0, 4.0, 1.0, 5.0, 1.0, 8.0, 2.0, 1.0, 16.0, 1.0])
    T = Tri(4, Ap, Aj, Ax, dtype)
    assert T.lev[False][1].tolist() == [0, 2, 3, 4]
    got = T.run(bh, np.array([2.0, 5.0, 12.0, 7.0]), None)
    assert got.tolist() == [1.0, 1.0, 1.0, 7.0]


def test_solve_refusals(hd):
    bh, dtype = hd
    n, Ap, Aj, Ax, xs, bl, _ = exact_case("poisson5pt_33")
    T = Tri(n, Ap, Aj, Ax, dtype)
    nlevels, ptr, order, dorder = T.lev[False]
    for flags, what in ((0, "neither triangle"), (LOWER | UPPER, "both triangles"), (UNIT, "a unit diagonal of neither"),
                        (LOWER | 8, "an unknown flag")):
        T.run(bh, bl, None, 0.5, flags, want=INV, what=what)
    for bad, what in ((np.concatenate([[1], ptr[1:]]), "does not start at 0"), (np.concatenate([ptr[:2], [ptr[1] - 1], ptr[3:]]), "falls"),
                      (np.concatenate([ptr[:-1], [n + 1]]), "ends beyond n")):
        T.run(bh, bl, None, 0.5, LOWER, ptr=bad.astype(np.int32), want=INV, what="h_levelPtr " + what)
    o = dorder.clone(); o[7] = n                                     # noqa: E702
    T.run(bh, bl, None, 0.5, LOWER, order=o, want=INV, what="an order entry equal to n")
    o = dorder.clone(); o[0] = -1                                    # noqa: E702
    T.run(bh, bl, None, 0.5, LOWER, order=o, want=INV, what="an order entry of -1")
    j = T.A[1].clone(); j[11] = n                                    # noqa: E702
    T.run(bh, bl, None, 0.5, LOWER, A=(T.A[0], j, T.A[2]), want=INV, what="a column equal to n")
    p = T.A[0].clone(); p[100] = p[99] - 1                           # noqa: E702
    T.run(bh, bl, None, 0.5, LOWER, A=(p, T.A[1], T.A[2]), want=INV, what="a decreasing row pointer")
    # the diagonal entry of row 40 turned into one more entry of its left neighbour: a listed row without a diagonal
    j = T.A[1].clone()
    q = int(np.flatnonzero((np.repeat(np.arange(n), np.diff(Ap)) == 40) & (Aj == 40))[0])
    j[q] = 39
    T.run(bh, bl, None, 0.5, LOWER, A=(T.A[0], j, T.A[2]), want=INV, what="a missing diagonal")
    T.run(bh, bl, None, 0.5, LOWER | UNIT, A=(T.A[0], j, T.A[2]), what="the same with a unit diagonal")
    # x overlapping b partly, and the values
    both = torch.full((2 * n,), XSENT, dtype=tdt(dtype)).cuda()
    torch.cuda.synchronize()
    args = (n, T.nnz, T.A[0], T.A[1], T.A[2], nlevels, ptr, dorder, 0.5)
    assert amg.trsv_raw_device(bh, *args, both[:n], both[n // 2:n // 2 + n], LOWER) == INV
    assert amg.trsv_raw_device(bh, *args, both[1:n + 1], both[:n], LOWER) == INV
    assert amg.trsv_raw_device(bh, *args, both[:n], T.A[2], LOWER) == INV
    assert amg.trsv_raw_device(bh, *args, None, both[:n], LOWER) == INV
    assert bool((both == XSENT).all())
    assert np.array_equal(T.run(bh, bl, None, 0.5, LOWER, what="after the refusals"), xs)


# ---------------------------------------------------------------- ILU(0)
def ilu_run(bh, T, want=0, what="", A=None, ptr=None, order=None):
    """the factorisation of T's values on a padded copy: (values as float64, pivot)"""
    nlevels, hptr, _, dorder = T.lev[False]
    hptr = hptr if ptr is None else ptr
    val = torch.full((T.nnz + PAD,), XSENT, dtype=tdt(T.dtype)).cuda()
    val[:T.nnz] = T.A[2] if A is None else A[2]
    A = T.A if A is None else A
    torch.cuda.synchronize()
    bh.ilu0_pivot = -2
    err = amg.ilu0_raw_device(bh, T.n, T.nnz, A[0], A[1], val, len(hptr) - 1, hptr, dorder if order is None else order, 0)
    assert err == want, (what, err)
    assert bool((val[T.nnz:] == XSENT).all()), (what, "written past the end of d_valA")
    if want != 0:
        assert bh.ilu0_pivot == -2
        return None, None
    assert bh.ilu0_ms >= 0.0 and set(launches(bh)) <= {"ilu0_level"}, (what, launches(bh))
    assert launches(bh).get("ilu0_level", 0) == int(np.count_nonzero(np.diff(hptr))), (what, launches(bh))
    return val[:T.nnz].cpu().numpy().astype(np.float64), bh.ilu0_pivot


def closed_pattern(name):
    """patterns closed under elimination, as dense 0/1 matrices: the factors of a matrix on them lie on them"""
    if name == "tridiagonal300":
        n = 300
        P = (np.abs(np.subtract.outer(np.arange(n), np.arange(n))) <= 1)
    elif name == "two_dense70":
        n = 140
        P = np.zeros((n, n), bool)
        P[:70, :70] = P[70:, 70:] = True
    else:                                                             # an arrow pointing down-right
        n = 200
        P = np.eye(n, dtype=bool)
        P[n - 1, :] = P[:, n - 1] = True
    return n, P


@functools.lru_cache(maxsize=None)
def factor_case(name, zero_pivot=-1):
    """(n, Ap, Aj, Ax, values of L0 and U0 on the pattern): A := L0 U0 with L0 unit lower, its off-diagonal entries integers in
    [-3, 3], U0 upper with off-diagonal entries integers in [-3, 3] and diagonal entries 1/2, 1, 2 or 4 (0 at zero_pivot);
    explicit zeros stay in the pattern.  Every intermediate of the elimination is a small dyadic number."""
    n, P = closed_pattern(name)
    rng = np.random.default_rng(41)
    L0 = np.tril(rng.integers(-3, 4, (n, n)), -1) * P + np.eye(n)
    U0 = np.triu(rng.integers(-3, 4, (n, n)), 1) * P + np.diag(rng.choice([0.5, 1.0, 2.0, 4.0], n))
    if zero_pivot >= 0:
        U0[zero_pivot, zero_pivot] = 0.0
    A = L0 @ U0
    assert not np.any(A[~P])                                          # closed: no fill
    r, c = np.nonzero(P)
    Ap = np.zeros(n + 1, np.int32)
    np.cumsum(np.bincount(r, minlength=n), out=Ap[1:])
    return n, Ap, c.astype(np.int32), A[r, c], np.where(r > c, L0[r, c], U0[r, c])


@pytest.mark.parametrize("name", ("tridiagonal300", "two_dense70", "arrow200"))
def test_ilu0_returns_the_integer_factors_bit_for_bit(hd, name):
    bh, dtype = hd
    n, Ap, Aj, Ax, want = factor_case(name)
    ref, rpivot = ir.ilu0(n, Ap, Aj, Ax, dtype)
    assert np.array_equal(ref.astype(np.float64), want) and rpivot == -1
    got, pivot = ilu_run(bh, Tri(n, Ap, Aj, Ax, dtype), what=name)
    assert pivot == -1 and np.array_equal(got, want), (name, pivot)
    if name == "two_dense70":
        assert ir.lanes_per_row(n, len(Aj)) == 64 and ir.levels(n, Ap, Aj)[1] == 70


def test_ilu0_reports_the_planted_pivot(hd):
    bh, dtype = hd
    for name, row in (("two_dense70", 93), ("tridiagonal300", 17), ("arrow200", 199)):
        n, Ap, Aj, Ax, _ = factor_case(name, row)
        got, pivot = ilu_run(bh, Tri(n, Ap, Aj, Ax, dtype), what=(name, row))
        assert pivot == row == ir.ilu0(n, Ap, Aj, Ax, dtype)[1], (name, pivot)
        assert got[int(np.flatnonzero((np.repeat(np.arange(n), np.diff(Ap)) == row) & (Aj == row))[0])] == 0.0


@pytest.mark.parametrize("name", ("poisson5pt_33", "poisson27pt_9", "uniform2048"))
def test_ilu0_identity_on_random_values(hd, name):
    """|(L U)_ij - a_ij| <= (m_ij + 2) u (sum_k |l_ik| |u_kj| + |a_ij|) on the pattern, m_ij the updates of the entry"""
    bh, dtype = hd
    n, Ap, Aj, Ax, _ = random_case(name)
    got, pivot = ilu_run(bh, Tri(n, Ap, Aj, Ax, dtype), what=name)
    err, most = ir.identity_error(n, Ap, Aj, Ax, got)
    print("%s %s: identity error %.3g u, at most %d updates an entry" % (name, np.dtype(dtype).name, err / unit(dtype), most))
    assert pivot == -1 and err <= unit(dtype), (name, err / unit(dtype))
    again, _ = ilu_run(bh, Tri(n, Ap, Aj, Ax, dtype), what=name)
    assert np.array_equal(got, again)


def test_ilu0_refusals(hd):
    bh, dtype = hd
    n, Ap, Aj, Ax, _ = random_case("poisson5pt_33")
    T = Tri(n, Ap, Aj, Ax, dtype)
    nlevels, ptr, order, dorder = T.lev[False]
    r = np.repeat(np.arange(n), np.diff(Ap))
    # row 50 with two of its columns swapped: not ascending
    j = T.A[1].clone()
    a = int(Ap[50])
    j[a], j[a + 1] = int(Aj[a + 1]), int(Aj[a])
    ilu_run(bh, T, want=INV, what="an unsorted row", A=(T.A[0], j, T.A[2]))
    # row 40 without its diagonal entry: the entry names column 39 again (also not ascending), or the row ends before it
    j = T.A[1].clone()
    j[int(np.flatnonzero((r == 40) & (Aj == 40))[0])] = 39
    ilu_run(bh, T, want=INV, what="a missing diagonal", A=(T.A[0], j, T.A[2]))
    n1, Ap1, Aj1 = 3, np.array([0, 1, 2, 4], np.int32), np.array([0, 0, 1, 2], np.int32)      # row 1 holds column 0 alone
    ilu_run(bh, Tri(n1, Ap1, Aj1, np.ones(4), dtype), want=INV, what="a row without a diagonal entry")
    j = T.A[1].clone(); j[11] = n                                    # noqa: E702
    ilu_run(bh, T, want=INV, what="a column equal to n", A=(T.A[0], j, T.A[2]))
    ilu_run(bh, T, want=INV, what="h_levelPtr falls", ptr=np.concatenate([ptr[:2], [ptr[1] - 1], ptr[3:]]).astype(np.int32))
    o = dorder.clone(); o[3] = n                                     # noqa: E702
    ilu_run(bh, T, want=INV, what="an order entry equal to n", order=o)
    torch.cuda.synchronize()
    assert amg.ilu0_raw_device(bh, n, T.nnz, T.A[0], T.A[1], T.A[2].clone(), nlevels, ptr, dorder, 1) == INV       # flags must be 0
    # the values overlapping an input: the lower bidiagonal of a path of 8 vertices, its columns and its values two views into
    # one tensor, the values shifted by one element
    Pp = np.array([0, 1, 3, 5, 7, 9, 11, 13, 15], np.int32)
    Pj = np.array([0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7], np.int32)
    both = torch.zeros(16, dtype=tdt(dtype)).cuda()
    cols = both.view(torch.int32)[:15]
    cols.copy_(up(Pj, np.int32))
    before = both.clone()
    rows8 = np.arange(9, dtype=np.int32)                             # (row i is level i: the level pointer, and the order)
    dPp, do8 = up(Pp, np.int32), up(rows8[:8], np.int32)
    torch.cuda.synchronize()
    bh.ilu0_pivot = -2
    assert amg.ilu0_raw_device(bh, 8, 15, dPp, cols, both[1:], 8, rows8, do8, 0) == INV and bh.ilu0_pivot == -2
    assert torch.equal(both.view(torch.uint8), before.view(torch.uint8))
    got, pivot = ilu_run(bh, T, what="after the refusals")
    assert pivot == -1 and ir.identity_error(n, Ap, Aj, Ax, got)[0] <= unit(dtype)


def test_refused_between_symbolic_and_finish():
    n, Ap, Aj, Ax, xs, bl, _ = exact_case("poisson5pt_33")
    T = Tri(n, Ap, Aj, Ax, np.float64)
    bh = new_handle()
    try:
        assert bh.initData_device(n, n, n, T.nnz, T.A[2], T.A[0], T.A[1], T.nnz, T.A[2], T.A[0], T.A[1]) == 0
        assert bh.spgemm_symbolic() == 0
        levels_run(bh, n, Ap, Aj, LOWER, want=INV, what="a multiply is open")
        assert np.array_equal(T.run(bh, bl, None, 0.5, LOWER, want=INV, what="a multiply is open"), bl)
        ilu_run(bh, T, want=INV, what="a multiply is open")
        assert bh.spgemm_numeric(0, n) == 0 and bh.spgemm_finish() == 0
        levels_check(levels_run(bh, n, Ap, Aj, LOWER), level_reference("poisson5pt_33", False, True), "after finish")
        assert np.array_equal(T.run(bh, bl, None, 0.5, LOWER, what="after finish"), xs)
        bh.free_mem()
    finally:
        bh.freePlatform()


# ---------------------------------------------------------------- ILU-PCG
def test_ilu_pcg_on_poisson27pt_9():
    """1e-8 relative residual in double, both orderings: the restatement's iterations +- 1; in colour order both factors have
    as many levels as colours and an application of the preconditioner is exactly 2 ncolors solve kernels"""
    n, Ap, Aj, Ax = ar.poisson("poisson27pt", 9, 9, 9)
    Amat = sp.csr_matrix((Ax, Aj, Ap), shape=(n, n))
    b = np.random.default_rng(0).standard_normal(n)
    A = (up(Ap, np.int32), up(Aj, np.int32), up(Ax, np.float64))
    db = up(b, np.float64)
    bh = new_handle()
    try:
        for ordering in ("natural", "colour"):
            _, want, _ = ir.ilu0_pcg(Amat, b, 1e-8, 100, ordering)
            x, its, res = amg.ilu0_pcg_device(bh, A, db, 1e-8, 100, ordering)
            print("poisson27pt 9^3 %s: %d iterations, the restatement %d" % (ordering, its, want))
            assert abs(its - want) <= 1 and len(res) == its + 1 and res[-1] <= 1e-8 * res[0]
            assert np.linalg.norm(b - Amat @ x.cpu().numpy()) <= 1.01e-8 * np.linalg.norm(b)
        M = amg.ilu0_setup_device(bh, A, "colour")
        ref = ir.ilu0_setup(Amat, "colour")
        ncolors = M["ncolors"]
        assert ncolors == ref["ncolors"] and M["lower"][1] == M["upper"][1] == ncolors and M["pivot"] == -1
        assert np.array_equal(M["perm"].cpu().numpy(), ref["perm"])
        count = 0
        y = db.clone()
        for upper in (False, True):
            amg.trsv_device(bh, M["LU"], M["upper" if upper else "lower"], y, y, upper=upper, unit_diag=not upper)
            assert launches(bh) == {"trsv_level": ncolors}, (upper, launches(bh))
            count += sum(launches(bh).values())
        assert count == 2 * ncolors
        z = amg.ilu0_apply_device(bh, M, db, torch.empty_like(db))
        want_z = ir.ilu0_apply(ref, b)
        assert np.allclose(z.cpu().numpy(), want_z, rtol=0, atol=1e-12 * np.abs(want_z).max())
    finally:
        bh.freePlatform()


def test_cpp_demo_runs():
    demo_dir = os.path.join(ROOT, "tests", "trsv")
    subprocess.check_call(["make", "-C", demo_dir, "-s"])
    out = subprocess.run([os.path.join(demo_dir, "trsv_demo")], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "trsv poisson5pt 33x33: levels 65 and 65 PASS" in out.stdout
