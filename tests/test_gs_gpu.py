"""The colouring (bhs_csr_color_device), the multicolour Gauss-Seidel sweep (bhs_csr_gs_device) and the cycle and PCG of
benchmark_spgemm_using_csr_amd/amg.py on top of them, on the GPU, both builds.

Reference: tests/gsref.py, the contract of include/bhsparse_hip.h ("colouring and relaxation") restated in numpy.  The
colouring is a function of (pattern, priorities or seed) alone, so d_color, d_order, the offsets, ncolors and rounds are
compared exactly.  The sweep is compared within steps * (maxrowlen + 4) * u * scale (gsref.error_bound), and bit for bit
where every value is a dyadic rational.  Sentinels sit behind every output; they must be intact, also after a refused call."""
import functools
import os
import subprocess

import numpy as np
import pytest
import scipy.sparse as sp
import torch

from conftest import ROOT
import aggref as ar
import gsref as gr

from benchmark_spgemm_using_csr_amd import _lib, amg, gallery
from benchmark_spgemm_using_csr_amd.dense import csr_spmv_device
from benchmark_spgemm_using_csr_amd.facade import BHSPARSE_HIP, NUM_PLATFORMS, bhsparse

pytestmark = pytest.mark.gpu

DTYPES = (np.float64, np.float32)
INV = _lib.BHS_ERR_INVALID_ARG
PAD = 64
SENT = -7
XSENT = -123.5
COLOR_FAMILIES = {"color_round", "color_order"}
GS_FAMILIES = {"gs_forward", "gs_backward"}
SEEDS = (0, 1, 12345)
FLAGS = {gr.FORWARD: _lib.BHS_GS_FORWARD, gr.BACKWARD: _lib.BHS_GS_BACKWARD, gr.SYMMETRIC: _lib.BHS_GS_SYMMETRIC}


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


def families(bh):
    return {s["name"] for s in bh.kernel_stats() if s["launches"] > 0}


@functools.lru_cache(maxsize=None)
def cases():
    return ar.gpu_cases()


@functools.lru_cache(maxsize=None)
def reference(name, seed):
    n, Sp, Sj = cases()[name]
    return gr.colouring(n, Sp, Sj, seed)


@functools.lru_cache(maxsize=None)
def reference_prio(name):
    """(priorities, the restatement's answer with them): one array of caller priorities a pattern"""
    n, Sp, Sj = cases()[name]
    prio = np.random.default_rng(5).integers(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32)
    return prio, gr.colouring(n, Sp, Sj, 99, prio)


# ---------------------------------------------------------------- the colouring
def color_run(bh, n, Sp, Sj, seed=0, prio=None, flags=0, want=0, what="", nnz=None):
    """The device's answer (color, ncolors, order, colorPtr, rounds) as numpy; the sentinels behind the outputs are checked."""
    dSp = up(Sp, np.int32) if len(Sp) else torch.zeros(1, dtype=torch.int32).cuda()
    dSj = up(Sj, np.int32) if len(Sj) else torch.zeros(1, dtype=torch.int32).cuda()
    dprio = None if prio is None else up(np.asarray(prio, np.uint32).view(np.int32), np.int32)
    room = max(n, 0)
    color = torch.full((room + PAD,), SENT, dtype=torch.int32).cuda()
    order = torch.full((room + PAD,), SENT, dtype=torch.int32).cuda()
    cptr = torch.full((room + 1 + PAD,), SENT, dtype=torch.int32).cuda()
    torch.cuda.synchronize()
    bh.color_ncolors = bh.color_rounds = -1
    err = amg.color_raw_device(bh, n, len(Sj) if nnz is None else nnz, dSp, dSj if len(Sj) else None, dprio, seed, flags, color,
                               order, cptr)
    assert err == want, (what, err)
    assert bool((color[room:] == SENT).all()) and bool((order[room:] == SENT).all()), (what, "written past the end")
    assert bool((cptr[room + 1:] == SENT).all()), (what, "written past the end of d_colorPtr")
    if want != 0:
        assert bh.color_ncolors == -1
        return None
    ncolors = bh.color_ncolors
    assert bh.color_ms >= 0.0 and families(bh) <= COLOR_FAMILIES, (what, families(bh))
    if n:
        assert bool((cptr[ncolors + 1:] == SENT).all()), (what, "written behind d_colorPtr[ncolors]")
    return color[:n].cpu().numpy(), ncolors, order[:n].cpu().numpy(), cptr[:ncolors + 1].cpu().numpy() if n else np.zeros(1, np.int32), bh.color_rounds


def color_check(got, want, what):
    color, ncolors, order, ptr, rounds = got
    wcolor, wncolors, worder, wptr, wrounds = want
    assert ncolors == wncolors and rounds == wrounds, (what, ncolors, wncolors, rounds, wrounds)
    assert np.array_equal(color, wcolor), (what, "colours")
    assert np.array_equal(order, worder), (what, "order")
    assert np.array_equal(ptr, wptr), (what, "offsets")


def test_color_empty(hd):
    bh, _ = hd
    got = color_run(bh, 0, np.zeros(1, np.int32), np.zeros(0, np.int32), what="n = 0")
    assert got[1] == 0 and got[4] == 0 and len(got[0]) == 0


@pytest.mark.parametrize("name", ("one_with_diag", "one_without_diag", "two_one_edge", "path300", "poisson5pt_33", "poisson9pt_20",
                                  "poisson27pt_9", "uniform2048", "powerlaw3000", "roadlike40", "star1024", "two_k70"))
def test_color_patterns_and_seeds(hd, name):
    bh, _ = hd
    n, Sp, Sj = cases()[name]
    for seed in SEEDS:
        color_check(color_run(bh, n, Sp, Sj, seed, what=(name, seed)), reference(name, seed), (name, seed))
    prio, want = reference_prio(name)
    color_check(color_run(bh, n, Sp, Sj, 99, prio=prio, what=(name, "prio")), want, (name, "caller priorities"))
    if name == "two_k70":
        assert reference(name, 0)[1] == 70 and reference(name, 0)[4] == 70   # beyond the window of 64 colours
    if name == "star1024":
        assert reference(name, 0)[1] == 2
    if name == "powerlaw3000":
        assert np.diff(Sp).max() > 512                               # a hub beyond every lanes-per-row


def test_color_priorities_that_tie(hd):
    bh, _ = hd
    n, Sp, Sj = cases()["uniform2048"]
    rng = np.random.default_rng(5)
    prio = rng.integers(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32)
    prio[:7] = (0, 1, 0xFFFFFFFF, 0xFFFFFFFE, 0x80000000, 2, 3)   # the lowest bit is dropped: ties, broken by index
    color_check(color_run(bh, n, Sp, Sj, 99, prio=prio, what="prio"), gr.colouring(n, Sp, Sj, 99, prio), "caller priorities")


def test_color_equal_priorities_on_a_path(hd):
    """ties are broken by index: the greatest index wins, one vertex a round down the path -- 300 rounds, 2 colours"""
    bh, _ = hd
    n, Sp, Sj = cases()["path300"]
    prio = np.full(n, 12, np.uint32)
    want = gr.colouring(n, Sp, Sj, 0, prio)
    assert want[4] == 300 and want[1] == 2
    color_check(color_run(bh, n, Sp, Sj, 0, prio=prio, what="equal priorities"), want, "equal priorities")


def test_color_libraries_handles_and_repeats_agree():
    n, Sp, Sj = cases()["uniform2048"]
    want = reference("uniform2048", 12345)
    outs = []
    for dtype in DTYPES:
        bh = new_handle(dtype)
        try:
            outs.append(color_run(bh, n, Sp, Sj, 12345))
            outs.append(color_run(bh, n, Sp, Sj, 12345))             # the same handle again
        finally:
            bh.freePlatform()
    for got in outs:
        color_check(got, want, "handles")


def test_color_non_symmetric(hd):
    bh, _ = hd
    Ap, Aj = gallery.uniform_csr(2048, 4, seed=9)
    color, ncolors, order, ptr, rounds = color_run(bh, 2048, Ap, Aj, 0, what="non-symmetric")
    assert 1 <= ncolors <= 2048 and rounds >= 1
    assert color.min() == 0 and color.max() == ncolors - 1
    worder, wptr = gr.order_of(color)
    assert np.array_equal(order, worder) and np.array_equal(ptr, wptr)


def test_color_refusals(hd):
    bh, _ = hd
    n, Sp, Sj = cases()["poisson5pt_33"]
    nnz = len(Sj)
    bad = Sj.copy(); bad[nnz // 2] = n                               # noqa: E702
    color_run(bh, n, Sp, bad, want=INV, what="a column equal to n")
    bad = Sj.copy(); bad[5] = -1                                     # noqa: E702
    color_run(bh, n, Sp, bad, want=INV, what="a column of -1")
    p = Sp.copy(); p[100] = p[99] - 1                                # noqa: E702
    color_run(bh, n, p, Sj, want=INV, what="a decreasing row pointer")
    p = Sp.copy(); p[n] = nnz + 3                                    # noqa: E702
    color_run(bh, n, p, Sj, want=INV, what="a last row pointer above nnzS", nnz=nnz)
    color_run(bh, n, Sp, Sj, flags=1, want=INV, what="flags = 1")
    color_run(bh, -1, Sp, Sj, want=INV, what="negative n")
    # overlapping arrays: d_color on d_colIndS, d_order on d_color, d_colorPtr inside d_order; a NULL output
    dSp, dSj = up(Sp, np.int32), up(Sj, np.int32)
    a, b, c = (torch.full((n + 1,), SENT, dtype=torch.int32).cuda() for _ in range(3))
    torch.cuda.synchronize()
    assert amg.color_raw_device(bh, n, nnz, dSp, dSj, None, 0, 0, dSj, b, c) == INV
    assert amg.color_raw_device(bh, n, nnz, dSp, dSj, None, 0, 0, a, a, c) == INV
    assert amg.color_raw_device(bh, n, nnz, dSp, dSj, None, 0, 0, a, b, b[n // 2:]) == INV
    assert amg.color_raw_device(bh, n, nnz, dSp, dSj, None, 0, 0, a, None, c) == INV
    assert np.array_equal(dSj.cpu().numpy(), Sj) and all(bool((t == SENT).all()) for t in (a, b, c))
    # the next valid call on the same handle is correct
    color_check(color_run(bh, n, Sp, Sj, 0, what="after the refusals"), reference("poisson5pt_33", 0), "after the refusals")


# ---------------------------------------------------------------- the sweep
@functools.lru_cache(maxsize=None)
def matrix(name):
    """(n, Ap, Aj, Ax, diag, b, x0, colouring of the pattern with seed 1): every value a float32 number, so that one reference
    serves both builds; uniform2048 and powerlaw3000 are made strictly diagonally dominant"""
    rng = np.random.default_rng(17)
    if name in ("poisson5pt_33", "poisson27pt_9"):
        n, Ap, Aj, Ax = ar.poisson(*{"poisson5pt_33": ("poisson5pt", 33, 33), "poisson27pt_9": ("poisson27pt", 9, 9, 9)}[name])
    else:
        n, Ap, Aj = cases()[name]
        r = np.repeat(np.arange(n), np.diff(Ap))
        Ax = rng.uniform(-1.0, 1.0, len(Aj)).astype(np.float32).astype(np.float64)
        rowsum = np.bincount(r[r != Aj], weights=np.abs(Ax[r != Aj]), minlength=n)
        Ax[r == Aj] = np.ceil(rowsum[r[r == Aj]]) + 1.0
    A = sp.csr_matrix((Ax, Aj, Ap), shape=(n, n))
    diag = A.diagonal().copy()
    if name not in ("poisson5pt_33", "poisson27pt_9"):
        diag = np.ceil(rowsum) + 1.0                                  # also where a row has no diagonal entry: d_i is the caller's
    b = rng.standard_normal(n).astype(np.float32).astype(np.float64)
    x0 = rng.standard_normal(n).astype(np.float32).astype(np.float64)
    return n, np.asarray(Ap, np.int32), np.asarray(Aj, np.int32), Ax, diag, b, x0, gr.colouring(n, Ap, Aj, 1)


@functools.lru_cache(maxsize=None)
def sweep_reference(name, direction, omega, sweeps):
    n, Ap, Aj, Ax, diag, b, x0, (_, _, order, ptr, _) = matrix(name)
    return gr.sweep(Ap, Aj, Ax, diag, ptr, order, b, x0, omega, sweeps, direction)


class Dev(object):
    """a matrix of matrix() on the device in a handle's value type"""

    def __init__(self, name, dtype):
        n, Ap, Aj, Ax, diag, b, x0, (color, ncolors, order, ptr, _) = matrix(name)
        self.n, self.nnz, self.ncolors, self.ptr = n, len(Aj), ncolors, ptr
        self.A = (up(Ap, np.int32), up(Aj, np.int32), up(Ax, dtype))
        self.diag, self.b, self.x0 = up(diag, dtype), up(b, dtype), x0
        self.color, self.order = up(color, np.int32), up(order, np.int32)
        self.dtype = dtype

    def x(self, values=None):
        x = torch.full((self.n + PAD,), XSENT, dtype=torch.float32 if self.dtype == np.float32 else torch.float64).cuda()
        x[:self.n] = up(self.x0 if values is None else values, self.dtype)
        return x

    def run(self, bh, x, omega=1.0, sweeps=1, flags=_lib.BHS_GS_SYMMETRIC, ptr=None, color="own", order=None, want=0, what=""):
        ptr = self.ptr if ptr is None else ptr
        torch.cuda.synchronize()
        err = amg.gs_raw_device(bh, self.n, self.nnz, self.A[0], self.A[1], self.A[2], self.diag, len(ptr) - 1, ptr,
                                self.order if order is None else order, self.color if isinstance(color, str) else color, self.b, x,
                                omega, sweeps, flags)
        assert err == want, (what, err)
        assert bool((x[self.n:] == XSENT).all()), (what, "written past the end of d_x")
        if want == 0:
            assert bh.gs_ms >= 0.0 and families(bh) <= GS_FAMILIES, (what, families(bh))
        return x[:self.n].cpu().numpy().astype(np.float64)


# (mean row lengths 4.9, 21, 8, 8: four and sixteen lanes a row; path300 at 3 and two_k70 at 70 take one lane and sixty-four)
MATRICES = ("poisson5pt_33", "poisson27pt_9", "uniform2048", "powerlaw3000", "path300", "two_k70")


@pytest.mark.parametrize("name", MATRICES)
def test_sweep_against_the_restatement(hd, name):
    """forward, backward and symmetric, omega 1 and 0.8, one sweep and two: within steps * (maxrowlen + 4) * u * scale"""
    bh, dtype = hd
    n, Ap, Aj, Ax, diag, b, x0, _ = matrix(name)
    D = Dev(name, dtype)
    u = 2.0 ** -53 if dtype == np.float64 else 2.0 ** -24
    if name == "powerlaw3000":
        assert np.diff(Ap).max() == 567                               # the hub row, beyond every L
    for direction in (gr.FORWARD, gr.BACKWARD, gr.SYMMETRIC):
        for omega in (1.0, 0.8):
            for sweeps in (1, 2):
                what = (name, np.dtype(dtype).name, direction, omega, sweeps)
                want = sweep_reference(name, direction, omega, sweeps)
                got = D.run(bh, D.x(), omega, sweeps, FLAGS[direction], what=what)
                steps = sweeps * len(gr.passes(D.ncolors, direction))
                bound = gr.error_bound(Ap, Aj, Ax, diag, b, (x0, want), steps, u)
                err = float(np.abs(got - want).max())
                print("%s %s %s omega %.1f sweeps %d: error %.3g, bound %.3g" % (what[:3] + (omega, sweeps, err, bound)))
                assert err <= bound, (what, err, bound)
                assert not np.array_equal(got, x0)


def test_sweep_bit_for_bit_on_dyadic_values():
    """poisson5pt (diagonal 4, -1 beside it) with integer b and x0, one forward sweep, omega = 1, in double: every value is an
    integer over a power of 4 no greater than 4^colours, within 53 bits -- the restatement and the device agree bit for bit"""
    n, Ap, Aj, Ax, diag, _, _, (color, ncolors, order, ptr, _) = matrix("poisson5pt_33")
    assert np.all(diag == 4.0) and ncolors <= 5
    rng = np.random.default_rng(3)
    b = rng.integers(-8, 9, n).astype(np.float64)
    x0 = rng.integers(-8, 9, n).astype(np.float64)
    want = gr.sweep(Ap, Aj, Ax, diag, ptr, order, b, x0, 1.0, 1, gr.FORWARD)
    assert np.array_equal(want * 4.0 ** ncolors, np.round(want * 4.0 ** ncolors))
    D = Dev("poisson5pt_33", np.float64)
    D.b = up(b, np.float64)
    bh = new_handle()
    try:
        got = D.run(bh, D.x(x0), 1.0, 1, _lib.BHS_GS_FORWARD)
    finally:
        bh.freePlatform()
    assert np.array_equal(got, want)


def test_sweep_repeats_bit_for_bit(hd):
    bh, dtype = hd
    D = Dev("uniform2048", dtype)
    first = D.run(bh, D.x(), 0.8, 2, _lib.BHS_GS_SYMMETRIC)
    again = D.run(bh, D.x(), 0.8, 2, _lib.BHS_GS_SYMMETRIC)
    other = new_handle(dtype)
    try:
        third = D.run(other, D.x(), 0.8, 2, _lib.BHS_GS_SYMMETRIC)
    finally:
        other.freePlatform()
    assert np.array_equal(first, again) and np.array_equal(first, third)
    # without d_color (no verification asked for)
    assert np.array_equal(D.run(bh, D.x(), 0.8, 2, _lib.BHS_GS_SYMMETRIC, color=None), first)


def test_sweep_leaves_unlisted_rows_alone(hd):
    bh, dtype = hd
    n, Ap, Aj, Ax, diag, b, x0, (_, ncolors, order, ptr, _) = matrix("poisson27pt_9")
    D = Dev("poisson27pt_9", dtype)
    keep = ncolors - 2
    got = D.run(bh, D.x(), 1.0, 1, _lib.BHS_GS_SYMMETRIC, ptr=ptr[:keep + 1])
    rest = order[ptr[keep]:]
    assert len(rest) > 0 and np.array_equal(got[rest], x0[rest])
    want = gr.sweep(Ap, Aj, Ax, diag, ptr[:keep + 1], order, b, x0, 1.0, 1, gr.SYMMETRIC)
    u = 2.0 ** -53 if dtype == np.float64 else 2.0 ** -24
    assert np.abs(got - want).max() <= gr.error_bound(Ap, Aj, Ax, diag, b, (x0, want), 2 * keep, u)
    # sweeps == 0 and no colours: nothing happens
    assert np.array_equal(D.run(bh, D.x(), 1.0, 0, _lib.BHS_GS_FORWARD), x0)
    assert np.array_equal(D.run(bh, D.x(), 1.0, 1, _lib.BHS_GS_FORWARD, ptr=np.zeros(1, np.int32)), x0)


def test_sweep_verifies_the_colouring(hd):
    bh, dtype = hd
    n, Sp, Sj = cases()["path300"]
    Ax = np.where(np.repeat(np.arange(n), np.diff(Sp)) == Sj, 4.0, -1.0)
    color, ncolors, order, ptr, _ = gr.colouring(n, Sp, Sj, 0)
    assert ncolors <= 3
    A = (up(Sp, np.int32), up(Sj, np.int32), up(Ax, dtype))
    d, b = up(np.full(n, 4.0), dtype), up(np.ones(n), dtype)
    tdt = torch.float32 if dtype == np.float32 else torch.float64
    verify = _lib.BHS_GS_FORWARD | _lib.BHS_GS_VERIFY

    def call(ptr, order, color, flags):
        x = torch.zeros(n, dtype=tdt).cuda()
        torch.cuda.synchronize()
        return amg.gs_raw_device(bh, n, len(Sj), A[0], A[1], A[2], d, len(ptr) - 1, ptr, order, color, b, x, 1.0, 1, flags), x
    zeros, every = up(np.zeros(n), np.int32), up(np.arange(n), np.int32)
    assert call(np.array([0, n], np.int32), every, zeros, verify)[0] == INV           # one colour for a path: improper
    assert call(np.array([0, n], np.int32), every, None, verify)[0] == INV            # VERIFY needs d_color
    err, x = call(ptr, up(order, np.int32), up(color, np.int32), verify)
    assert err == 0
    want = gr.sweep(Sp, Sj, Ax, np.full(n, 4.0), ptr, order, np.ones(n), np.zeros(n), 1.0, 1, gr.FORWARD)
    assert np.allclose(x.cpu().numpy(), want, rtol=1e-6, atol=0)
    # a proper colouring whose colour numbers disagree with the offsets: a listed row of another colour
    assert call(ptr, up(order, np.int32), up((color + 1) % ncolors, np.int32), verify)[0] == INV
    # gs_device passes the switch on
    coloring = (up(color, np.int32), ncolors, up(order, np.int32), ptr)
    x = amg.gs_device(bh, A, d, coloring, b, torch.zeros(n, dtype=tdt).cuda(), direction="forward", verify=True)
    assert np.allclose(x.cpu().numpy(), want, rtol=1e-6, atol=0)
    with pytest.raises(amg.BhsparseError):
        amg.gs_device(bh, A, d, (zeros, 1, every, np.array([0, n], np.int32)), b, torch.zeros(n, dtype=tdt).cuda(), verify=True)


def test_sweep_refusals(hd):
    bh, dtype = hd
    D = Dev("poisson5pt_33", dtype)
    n, ptr = D.n, D.ptr
    x = D.x()
    for bad, what in ((np.concatenate([[1], ptr[1:]]), "does not start at 0"), (np.concatenate([ptr[:2], [ptr[1] - 1], ptr[3:]]), "falls"),
                      (np.concatenate([ptr[:-1], [n + 1]]), "ends beyond n")):
        D.run(bh, x, ptr=bad.astype(np.int32), want=INV, what="h_colorPtr " + what)
    D.run(bh, x, flags=0, want=INV, what="no direction")
    D.run(bh, x, flags=8 | _lib.BHS_GS_FORWARD, want=INV, what="an unknown flag")
    D.run(bh, x, sweeps=-1, want=INV, what="negative sweeps")
    # on the device: an order entry that is no row, a column out of range, a bad row pointer
    order = D.order.clone(); order[7] = n                            # noqa: E702
    D.run(bh, D.x(), order=order, want=INV, what="an order entry equal to n")
    order = D.order.clone(); order[0] = -1                           # noqa: E702
    D.run(bh, D.x(), order=order, want=INV, what="an order entry of -1")
    Aj = D.A[1].clone(); Aj[11] = n                                  # noqa: E702
    keep, D.A = D.A, (D.A[0], Aj, D.A[2])
    D.run(bh, D.x(), want=INV, what="a column equal to n")
    Ap = keep[0].clone(); Ap[100] = Ap[99] - 1                       # noqa: E702
    D.A = (Ap, keep[1], keep[2])
    D.run(bh, D.x(), want=INV, what="a decreasing row pointer")
    D.A = keep
    # x overlapping b, the diagonal and the values
    torch.cuda.synchronize()
    args = (D.n, D.nnz, D.A[0], D.A[1], D.A[2])
    assert amg.gs_raw_device(bh, *args, D.diag, D.ncolors, ptr, D.order, D.color, D.b, D.b, 1.0, 1, 1) == INV
    assert amg.gs_raw_device(bh, *args, D.diag, D.ncolors, ptr, D.order, D.color, D.b, D.diag, 1.0, 1, 1) == INV
    if D.nnz >= n:
        assert amg.gs_raw_device(bh, *args, D.diag, D.ncolors, ptr, D.order, D.color, D.b, D.A[2], 1.0, 1, 1) == INV
    assert amg.gs_raw_device(bh, *args, None, D.ncolors, ptr, D.order, D.color, D.b, D.x(), 1.0, 1, 1) == INV   # d_diag is required
    # the next valid call on the same handle is correct
    want = sweep_reference("poisson5pt_33", gr.SYMMETRIC, 1.0, 1)
    got = D.run(bh, D.x(), what="after the refusals")
    assert np.allclose(got, want, rtol=0, atol=1e-5 * np.abs(want).max())


def test_refused_between_symbolic_and_finish():
    D = Dev("poisson5pt_33", np.float64)
    n, Ap, Aj = D.n, D.A[0], D.A[1]
    bh = new_handle()
    try:
        assert bh.initData_device(n, n, n, D.nnz, D.A[2], Ap, Aj, D.nnz, D.A[2], Ap, Aj) == 0
        assert bh.spgemm_symbolic() == 0
        x = D.x()
        D.run(bh, x, want=INV, what="a multiply is open")
        assert np.array_equal(x[:n].cpu().numpy(), D.x0)
        c, o, p = (torch.full((n + 1,), SENT, dtype=torch.int32).cuda() for _ in range(3))
        torch.cuda.synchronize()
        assert amg.color_raw_device(bh, n, D.nnz, Ap, Aj, None, 0, 0, c, o, p) == INV
        assert bool((c == SENT).all())
        assert bh.spgemm_numeric(0, n) == 0 and bh.spgemm_finish() == 0
        assert amg.color_raw_device(bh, n, D.nnz, Ap, Aj, None, 1, 0, c, o, p) == 0
        assert np.array_equal(c[:n].cpu().numpy(), matrix("poisson5pt_33")[7][0])
        D.run(bh, D.x(), what="after finish")
        bh.free_mem()
    finally:
        bh.freePlatform()


# ---------------------------------------------------------------- the cycle, PCG
@functools.lru_cache(maxsize=None)
def amg_reference(name):
    """(A, b, Jacobi cycles, Gauss-Seidel cycles, PCG iterations) of the scipy restatement, seed 0"""
    n, Ap, Aj, Ax = ar.poisson(*{"poisson5pt_33": ("poisson5pt", 33, 33), "poisson27pt_9": ("poisson27pt", 9, 9, 9)}[name])
    A = sp.csr_matrix((Ax, Aj, Ap), shape=(n, n))
    levels, _ = ar.sa_setup(A)
    smoothers = gr.smoother_setup(levels)
    b = np.random.default_rng(0).standard_normal(n)
    _, jacobi, _ = ar.solve(levels, b, 1e-8, 100)
    _, cycles, res = gr.solve_gs(levels, smoothers, b, 1e-8, 100)
    _, its, pres = gr.pcg(levels, smoothers, b, 1e-8, 100)
    assert res[-1] <= 1e-8 * res[0] and pres[-1] <= 1e-8 * pres[0]
    return (n, Ap, Aj, Ax), A, b, jacobi, cycles, its


@pytest.mark.parametrize("name", ("poisson5pt_33", "poisson27pt_9"))
def test_gs_cycles_and_pcg(name):
    """1e-8 relative residual in double: Gauss-Seidel cycles within the restatement's cycles + 2, PCG within its iterations
    + 2; the smoothers' colourings are the restatement's; solve_device does what it did"""
    (n, Ap, Aj, Ax), Amat, b, ref_jacobi, ref_cycles, ref_its = amg_reference(name)
    A = (up(Ap, np.int32), up(Aj, np.int32), up(Ax, np.float64))
    db = up(b, np.float64)
    h1, h2 = new_handle(), new_handle()
    try:
        levels, _ = amg.sa_setup_device((h1, h2), n, A)
        smoothers = amg.smoother_setup_device(h1, levels)
        want = gr.colouring(n, Ap, Aj, 0)
        color, ncolors, order, ptr = smoothers[0][1]
        assert ncolors == want[1] and np.array_equal(color.cpu().numpy(), want[0]) and np.array_equal(ptr, want[3])
        assert isinstance(ptr, np.ndarray) and ptr.dtype == np.int32 and smoothers[0][0].is_cuda
        x = torch.zeros_like(db)
        res, cycles = [float(torch.linalg.norm(db))], 0
        while res[-1] > 1e-8 * res[0] and cycles < 100:
            x = amg.vcycle_device(h1, levels, db, x, smoother="gs", smoothers=smoothers)
            res.append(float(torch.linalg.norm(csr_spmv_device(h1, n, n, A, x, alpha=-1.0, beta=1.0, y=db.clone()))))
            cycles += 1
        xp, its, pres = amg.pcg_device(h1, levels, db, 1e-8, 100)
        xj, jacobi, jres = amg.solve_device(h1, levels, db, 1e-8, 100)
        # solve_device is the Jacobi cycle it was: the same bits as cycling by hand with the defaults
        xh = torch.zeros_like(db)
        for _ in range(jacobi):
            xh = amg.vcycle_device(h1, levels, db, xh)
    finally:
        h1.freePlatform()
        h2.freePlatform()
    print("%s: gs %d cycles (restatement %d), pcg %d iterations (%d), jacobi %d cycles (%d)"
          % (name, cycles, ref_cycles, its, ref_its, jacobi, ref_jacobi))
    nb = np.linalg.norm(b)
    assert res[-1] <= 1e-8 * res[0] and cycles <= ref_cycles + 2
    assert np.linalg.norm(b - Amat @ x.cpu().numpy()) <= 1.01e-8 * nb
    assert pres[-1] <= 1e-8 * pres[0] and its <= ref_its + 2 and len(pres) == its + 1
    assert np.linalg.norm(b - Amat @ xp.cpu().numpy()) <= 1.01e-8 * nb
    assert jres[-1] <= 1e-8 * jres[0] and jacobi <= ref_jacobi + 2 and torch.equal(xh, xj)


def test_cpp_demo_runs():
    demo_dir = os.path.join(ROOT, "tests", "gs")
    subprocess.check_call(["make", "-C", demo_dir, "-s"])
    out = subprocess.run([os.path.join(demo_dir, "gs_demo")], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    _, ncolors, _, _, rounds = gr.colouring(*cases()["poisson5pt_33"], 0)
    assert "gs poisson5pt 33x33 seed 0: ncolors %d rounds %d PASS" % (ncolors, rounds) in out.stdout
