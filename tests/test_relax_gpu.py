"""bhs_csr_relax_device on the GPU, both builds.

Reference: tests/relaxref.py, the contract of include/bhsparse_hip.h ("relaxation and fused products") restated in numpy.
Exact cases -- small signed integers in A, b and x, powers of two in diag and in the coefficients -- are compared as
numbers; where several steps follow each other the matrix holds at most four non-zero values a row, so that every row sum
stays exact in double whatever its order (a step adds at most 3 bits of magnitude and 3 fractional bits to x).  Real
values are held against the bound of tests/valuecheck.py for ANY order of a step's K = entries + 5 operations, no entry
excluded.  x and d carry sentinels behind their end."""
import functools

import numpy as np
import pytest
import torch

import relaxref as rr
import spmvref as sr
from helpers import wide_values
from test_spmv_gpu import LADDER, N_LADDER, bits, new_handle, rows_matrix, same_numbers, tdt, up
from valuecheck import check_values

from benchmark_spgemm_using_csr_amd import _lib, amg
from benchmark_spgemm_using_csr_amd.facade import bhsparse

pytestmark = pytest.mark.gpu

DTYPES = (np.float64, np.float32)
INV = _lib.BHS_ERR_INVALID_ARG
SENTINEL = -7.0
PAD = 64
COEF = np.array([(0.0, 1.0), (0.5, 0.5), (0.25, 2.0), (0.5, 1.0)])   # powers of two; step 0 reads no d


@pytest.fixture(scope="module", params=DTYPES, ids=("f64", "f32"))
def hd(request):
    bh = new_handle(request.param)
    yield bh, request.param
    bh.freePlatform()


def stats(bh):
    return {s["name"]: s["launches"] for s in bh.kernel_stats() if s["launches"] > 0}


def expected_stats(Ap, steps, zero):
    lens = np.diff(np.asarray(Ap, np.int64))
    passes = steps - (1 if zero else 0)
    want = {}
    if zero:
        want["relax_zero"] = 1
    if passes:
        want["relax_short"] = passes
        if np.any((lens > 32) & (lens <= 1024)):
            want["relax_wave"] = passes
        if np.any(lens > 1024):
            want["relax_long"] = passes
    if steps - 1 <= (1 if zero else 0):
        want["relax_finish"] = 1
    return want


@functools.lru_cache(maxsize=None)
def square(n, sparse_values, seed=5):
    """n x n: the ladder's lengths (twice) among rows of 0 .. 8 entries where n allows it, columns in no order, duplicates;
    sparse_values: all but four values a row are zero, the rest +-1"""
    rng = np.random.default_rng(seed)
    lens = rng.integers(0, min(9, n + 1), n)
    if n >= 5000:
        lens[rng.choice(n, 2 * len(LADDER), replace=False)] = LADDER + LADDER
    _, _, (Ap, Aj, Ax) = rows_matrix(lens, n, seed + 1)
    if sparse_values:
        keep = np.zeros(len(Ax), bool)
        for i in range(n):
            if Ap[i + 1] > Ap[i]:
                keep[rng.choice(np.arange(Ap[i], Ap[i + 1]), min(4, Ap[i + 1] - Ap[i]), replace=False)] = True
        Ax = np.where(keep, np.sign(Ax) + (Ax == 0), 0.0)
    diag = 2.0 ** rng.integers(0, 3, n)
    return Ap, Aj, Ax, diag


def vectors(n, seed):
    rng = np.random.default_rng(seed)
    return (rng.integers(-3, 4, n).astype(np.float64), rng.integers(-3, 4, n).astype(np.float64),
            rng.integers(-3, 4, n).astype(np.float64))


def call(bh, dtype, n, A, diag, coef, b, x, d, zero=False, values=True, want=0, nan_x=False):
    """(x, d) of the device after the call, numpy; d None: a NULL d_d.  The sentinels behind both are checked."""
    Ap, Aj, Ax = A
    t = tdt(dtype)
    dx = torch.full((n + PAD,), SENTINEL, dtype=t).cuda()
    dx[:n] = float("nan") if nan_x else up(x, dtype)
    dd = None
    if d is not None:
        dd = torch.full((n + PAD,), SENTINEL, dtype=t).cuda()
        dd[:n] = up(d, dtype)
    dAp, dAj = up(Ap, np.int32), up(np.concatenate([Aj, [0]]), np.int32)
    dAx = up(np.concatenate([Ax, [0]]), dtype) if values else None
    ddiag, db = up(np.concatenate([diag, [1]]), dtype), up(np.concatenate([b, [0]]), dtype)
    before = None if dd is None else dd.clone()
    x0 = dx.clone()
    torch.cuda.synchronize()
    err = amg.relax_raw_device(bh, n, len(Aj), dAx, dAp, dAj, ddiag, len(coef), coef, db, dx, dd, rr.ZERO_GUESS if zero else 0)
    assert err == want, (err, want)
    assert bool((dx[n:] == SENTINEL).all()) and (dd is None or bool((dd[n:] == SENTINEL).all())), "written past the end"
    if want:
        assert np.array_equal(bits(dx.cpu().numpy()), bits(x0.cpu().numpy())), "x written by a refused call"
        assert dd is None or np.array_equal(bits(dd.cpu().numpy()), bits(before.cpu().numpy())), "d written by a refused call"
    else:
        assert stats(bh) == expected_stats(Ap, len(coef), zero), (stats(bh), expected_stats(Ap, len(coef), zero))
        assert bh.relax_ms >= 0.0
    return dx[:n].cpu().numpy(), (None if dd is None else dd[:n].cpu().numpy())


# ---------------------------------------------------------------- exact cases
def test_one_step_on_the_ladder_is_exact(hd):
    bh, dtype = hd
    n = N_LADDER
    Ap, Aj, Ax, diag = square(n, False)
    assert sorted(np.diff(Ap)[np.diff(Ap) > 8]) == sorted(v for v in LADDER + LADDER if v > 8)
    assert 5000 * 4 * 3 + 3 < 2 ** 24                               # every sum an integer that both builds hold exactly
    b, x, d = vectors(n, 1)
    for coef in (COEF[:1], np.array([(0.5, 2.0)])):
        for values in (True, False):
            rx, rd, _, _ = rr.relax(n, Ap, Aj, Ax if values else None, diag, coef, b, x, d, dtype=dtype)
            gx, gd = call(bh, dtype, n, (Ap, Aj, Ax), diag, coef, b, x, d, values=values)
            same_numbers(gx, rx, ("x", values))
            same_numbers(gd, rd, ("d", values))
    # without d: a == 0
    rx, _, _, _ = rr.relax(n, Ap, Aj, Ax, diag, COEF[:1], b, x, dtype=dtype)
    gx, gd = call(bh, dtype, n, (Ap, Aj, Ax), diag, COEF[:1], b, x, None)
    same_numbers(gx, rx, "no d")


@pytest.mark.parametrize("steps", (1, 2, 3, 4))
def test_steps_are_exact(hd, steps):
    bh, dtype = hd
    n = N_LADDER
    Ap, Aj, Ax, diag = square(n, True)
    b, x, d = vectors(n, 2)
    for zero in (False, True):
        rx, rd, _, _ = rr.relax(n, Ap, Aj, Ax, diag, COEF[:steps], b, x, d, zero_guess=zero, dtype=dtype)
        gx, gd = call(bh, dtype, n, (Ap, Aj, Ax), diag, COEF[:steps], b, x, d, zero=zero, nan_x=zero)
        same_numbers(gx, rx, ("x", steps, zero))
        same_numbers(gd, rd, ("d", steps, zero))
    # Jacobi sweeps keep no d
    jac = np.array([(0.0, 0.5)] * steps)
    rx, _, _, _ = rr.relax(n, Ap, Aj, Ax, diag, jac, b, x, dtype=dtype)
    same_numbers(call(bh, dtype, n, (Ap, Aj, Ax), diag, jac, b, x, None)[0], rx, ("jacobi", steps))


@pytest.mark.parametrize("n", (0, 1, 255, 256, 257))
def test_small_sizes(hd, n):
    bh, dtype = hd
    Ap, Aj, Ax, diag = square(n, True, seed=20 + n)
    b, x, d = vectors(n, 3)
    for steps in (1, 3):
        for zero in (False, True):
            rx, rd, _, _ = rr.relax(n, Ap, Aj, Ax, diag, COEF[:steps], b, x, d, zero_guess=zero, dtype=dtype)
            gx, gd = call(bh, dtype, n, (Ap, Aj, Ax), diag, COEF[:steps], b, x, d, zero=zero, nan_x=zero)
            same_numbers(gx, rx, (n, steps, zero))
            same_numbers(gd, rd, (n, steps, zero))


@pytest.mark.parametrize("steps", (1, 3))
def test_no_row_reads_an_x_of_its_own_step(hd, steps):
    """A = 4 I + a cyclic shift by 1000: every row reads an x that another workgroup rewrites in the same step"""
    bh, dtype = hd
    n = N_LADDER
    rng = np.random.default_rng(8)
    Ap = np.arange(0, 2 * n + 1, 2).astype(np.int32)
    Aj = np.stack([(np.arange(n) + 1000) % n, np.arange(n)], axis=1).ravel().astype(np.int32)
    Ax = np.stack([rng.integers(-2, 3, n), np.full(n, 4)], axis=1).ravel().astype(np.float64)
    diag = np.full(n, 4.0)
    b, x, d = vectors(n, 4)
    rx, rd, _, _ = rr.relax(n, Ap, Aj, Ax, diag, COEF[:steps], b, x, d, dtype=dtype)
    gx, gd = call(bh, dtype, n, (Ap, Aj, Ax), diag, COEF[:steps], b, x, d)
    same_numbers(gx, rx, ("shift x", steps))
    same_numbers(gd, rd, ("shift d", steps))


# ---------------------------------------------------------------- real values
def real_case(dtype, seed=31):
    n = N_LADDER
    Ap, Aj, _, _ = square(n, False)
    rng = np.random.default_rng(seed)
    r_ = lambda v: np.ascontiguousarray(v, dtype).astype(np.float64)   # noqa: E731
    Ax, diag = r_(wide_values(len(Aj), rng)), r_(1.0 + rng.random(n))
    b, x, d = r_(wide_values(n, rng)), r_(wide_values(n, rng)), r_(wide_values(n, rng))
    return n, (Ap, Aj, Ax), diag, b, x, d


def test_real_values_within_the_bound(hd):
    bh, dtype = hd
    n, A, diag, b, x, d = real_case(dtype)
    mode = "f64" if dtype == np.float64 else "f32_once"
    for coef in (np.array([(0.0, 0.7)]), np.array([(0.3, 1.9)])):
        rx, rd, S, K = rr.relax(n, A[0], A[1], A[2], diag, coef, b, x, d, dtype=np.float64)
        gx, gd = call(bh, dtype, n, A, diag, coef, b, x, d)
        worst = check_values(rx, S, K, gx, mode, "x: "), check_values(rd, S - np.abs(x), K - 1, gd, mode, "d: ")   # (d: without the addition to x)
        print("one step %s %s: worst err/bound x %.3g, d %.3g" % (coef.tolist(), mode, worst[0], worst[1]))


def test_chaining_and_repeatability(hd):
    bh, dtype = hd
    n, A, diag, b, x, d = real_case(dtype, 32)
    coef = amg.chebyshev_coefficients(0.3, 1.1, 3)
    for zero in (False, True):
        gx, gd = call(bh, dtype, n, A, diag, coef, b, x, d, zero=zero)
        cx, cd = x, d
        for s in range(3):
            cx, cd = call(bh, dtype, n, A, diag, coef[s:s + 1], b, cx, cd, zero=zero and s == 0)
        assert np.array_equal(bits(gx), bits(cx)) and np.array_equal(bits(gd), bits(cd)), zero
        again = call(bh, dtype, n, A, diag, coef, b, x, d, zero=zero)
        assert np.array_equal(bits(gx), bits(again[0])) and np.array_equal(bits(gd), bits(again[1]))
        other = new_handle(dtype)
        try:
            fresh = call(other, dtype, n, A, diag, coef, b, x, d, zero=zero)
        finally:
            other.freePlatform()
        assert np.array_equal(bits(gx), bits(fresh[0])) and np.array_equal(bits(gd), bits(fresh[1]))
    # the zero guess is the call on x = 0, as numbers
    zx, zd = call(bh, dtype, n, A, diag, coef, b, x, d, zero=True, nan_x=True)
    px, pd = call(bh, dtype, n, A, diag, coef, b, np.zeros(n), d)
    same_numbers(zx, px, "zero guess x")
    same_numbers(zd, pd, "zero guess d")


# ---------------------------------------------------------------- the Chebyshev polynomial on the device
def test_diagonal_matrix_gives_the_closed_form(hd):
    bh, dtype = hd
    lmin, lmax = 0.3, 1.1
    theta, delta = (lmax + lmin) / 2, (lmax - lmin) / 2
    lam = np.ascontiguousarray(np.concatenate([np.linspace(lmin, lmax, 257), [lmin / 2, 1.02 * lmax]]), dtype).astype(np.float64)
    n = len(lam)
    A = (np.arange(n + 1).astype(np.int32), np.arange(n).astype(np.int32), lam)
    eps = float(np.finfo(dtype).eps)
    for steps in range(1, 7):
        coef = amg.chebyshev_coefficients(lmin, lmax, steps)
        gx, _ = call(bh, dtype, n, A, np.ones(n), coef, np.zeros(n), np.ones(n), np.zeros(n))
        want = rr.chebyshev_value(steps, (theta - lam) / delta) / rr.chebyshev_value(steps, theta / delta)
        err = float(np.abs(gx.astype(np.float64) - want).max())
        print("steps %d %s: off the closed form by %.2f eps" % (steps, np.dtype(dtype).name, err / eps))
        assert err <= 64 * steps * eps, (steps, err / eps)


# ---------------------------------------------------------------- refusals
def test_device_refusals_leave_x_and_d_untouched(hd):
    bh, dtype = hd
    n = N_LADDER
    Ap, Aj, Ax, diag = square(n, True)
    nnz = len(Aj)
    lens = np.diff(Ap)
    p0 = Ap.copy(); p0[0] = 1
    pm = Ap.copy(); pm[-1] = nnz - 1
    big = int(np.flatnonzero(lens == 5000)[0])
    pd = Ap.copy(); pd[big + 1] = Ap[big] - 1 if Ap[big] > 0 else Ap[big + 2] + 1
    cases = [("rowPtrA[0] != 0", p0, Aj), ("rowPtrA[m] != nnzA", pm, Aj), ("decreasing rowPtrA", pd, Aj)]
    for L, col in ((5, -1), (17, n), (65, n), (65, -1), (5000, n), (5000, -1)):     # a bad column in every bin
        j = Aj.copy()
        j[Ap[int(np.flatnonzero(lens == L)[0])] + L // 2] = col
        cases.append(("column of A out of range", Ap, j))
    b, x, d = vectors(n, 6)
    for word, p, j in cases:
        assert sr.invalid(n, n, p, j) == word and word in sr.DEVICE_REFUSALS
        for zero in (False, True):
            call(bh, dtype, n, (p, j, Ax), diag, COEF[:3], b, x, d, zero=zero, want=INV)
        call(bh, dtype, n, (p, j, Ax), diag, COEF[:1], b, x, d, want=INV)
        # the handle still answers a valid call
        rx, rd, _, _ = rr.relax(n, Ap, Aj, Ax, diag, COEF[:3], b, x, d, dtype=dtype)
        same_numbers(call(bh, dtype, n, (Ap, Aj, Ax), diag, COEF[:3], b, x, d)[0], rx, "after " + word)


def test_host_refusals_write_nothing(hd):
    bh, dtype = hd
    n = 257
    Ap, Aj, Ax, diag = square(n, True, seed=20 + n)
    t = tdt(dtype)
    dAp, dAj, dAx, ddiag = up(Ap, np.int32), up(Aj, np.int32), up(Ax, dtype), up(diag, dtype)
    db = torch.ones(n, dtype=t).cuda()
    dx = torch.full((2 * n + PAD,), SENTINEL, dtype=t).cuda()
    dd = torch.full((n + PAD,), SENTINEL, dtype=t).cuda()
    torch.cuda.synchronize()
    ok = dict(n=n, nnz=len(Aj), Ax=dAx, Ap=dAp, Aj=dAj, diag=ddiag, steps=2, coef=COEF[:2], b=db, x=dx, d=dd, flags=0)

    def go(**kw):
        a = dict(ok, **kw)
        return amg.relax_raw_device(bh, a["n"], a["nnz"], a["Ax"], a["Ap"], a["Aj"], a["diag"], a["steps"], a["coef"], a["b"], a["x"],
                                    a["d"], a["flags"])
    nan, inf = float("nan"), float("inf")
    refused = {
        "negative size": (go(n=-1), go(nnz=-1)),
        "steps < 1": (go(steps=0), go(steps=-2)),
        "NULL coef": (go(coef=None),),
        "non-finite coefficient": (go(coef=[(0.0, nan), (0.5, 1.0)]), go(coef=[(0.0, 1.0), (inf, 1.0)])),
        "unknown flags": (go(flags=2), go(flags=5)),
        "NULL rowPtrA": (go(Ap=None),),
        "NULL colIndA": (go(Aj=None),),
        "NULL diag, b or x": (go(diag=None), go(b=None), go(x=None)),
        "NULL d with a != 0": (go(d=None),),
        "overlap": (go(x=db), go(x=ddiag), go(x=dAx), go(d=db), go(d=dx), go(d=dx[n - 1:]), go(x=dd), go(d=dAp)),
    }
    for word, codes in refused.items():
        assert all(c == INV for c in codes), (word, codes)
    assert bool((dx == SENTINEL).all()) and bool((dd == SENTINEL).all()), "written by a refused call"
    assert go(d=None, coef=[(0.0, 1.0), (0.0, 0.5)]) == 0           # a NULL d_d is legal where every a is 0
    assert go(n=0, nnz=0, Ap=up(np.zeros(1), np.int32), Aj=None, Ax=None, diag=None, b=None, x=None, d=None) == 0
    assert amg.relax_raw_device(bhsparse(dtype), 0, 0, None, None, None, None, 1, COEF[:1], None, None, None, 0) == _lib.BHS_ERR_NOT_READY


def test_refused_between_symbolic_and_finish():
    n = 257
    Ap, Aj, Ax, diag = square(n, True, seed=20 + n)
    dA = (up(Ap, np.int32), up(Aj, np.int32), up(Ax, np.float64))
    x = torch.full((n,), SENTINEL, dtype=torch.float64).cuda()
    ones = torch.ones(n, dtype=torch.float64).cuda()
    bh = new_handle()
    try:
        assert bh.initData_device(n, n, n, len(Aj), dA[2], dA[0], dA[1], len(Aj), dA[2], dA[0], dA[1]) == 0
        assert bh.spgemm_symbolic() == 0
        assert amg.relax_raw_device(bh, n, len(Aj), dA[2], dA[0], dA[1], ones, 1, COEF[:1], ones, x, None, 0) == INV
        assert bool((x == SENTINEL).all())
        assert bh.spgemm_numeric(0, n) == 0 and bh.spgemm_finish() == 0
        assert amg.relax_raw_device(bh, n, len(Aj), dA[2], dA[0], dA[1], ones, 1, COEF[:1], ones, x, None, 0) == 0
        bh.free_mem()
    finally:
        bh.freePlatform()


def test_cpp_demo_runs():
    import os
    import subprocess
    from conftest import ROOT
    demo_dir = os.path.join(ROOT, "tests", "relax")
    subprocess.check_call(["make", "-C", demo_dir, "-s"])
    out = subprocess.run([os.path.join(demo_dir, "relax_demo")], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "relax / spmv_dots 6 x 6, 16 entries: PASS" in out.stdout


@pytest.mark.parametrize("dtype", DTYPES)
def test_tensor_calls(dtype):
    n = 257
    Ap, Aj, Ax, diag = square(n, True, seed=20 + n)
    b, x, _ = vectors(n, 9)
    dA = (up(Ap, np.int32), up(Aj, np.int32), up(Ax, dtype))
    bh = new_handle(dtype)
    try:
        dx = up(x, dtype)
        out = amg.relax_device(bh, dA, up(diag, dtype), up(b, dtype), dx, COEF[:3])
        assert out.data_ptr() == dx.data_ptr()
        same_numbers(out.cpu().numpy(), rr.relax(n, Ap, Aj, Ax, diag, COEF[:3], b, x, np.zeros(n), dtype=dtype)[0], "relax_device")
        dx = torch.full((n,), float("nan"), dtype=tdt(dtype)).cuda()
        amg.jacobi_device(bh, dA, up(diag, dtype), up(b, dtype), dx, 0.5, 2, zero_guess=True)
        same_numbers(dx.cpu().numpy(), rr.relax(n, Ap, Aj, Ax, diag, [(0.0, 0.5)] * 2, b, x, zero_guess=True, dtype=dtype)[0], "jacobi")
    finally:
        bh.freePlatform()
