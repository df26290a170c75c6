"""CSR x dense (bhs_csr_spmv_device, bhs_csr_spmm_device) on the GPU, both builds.

Reference: tests/spmvref.py, the contract of include/bhsparse_hip.h ("CSR x dense") restated in numpy.  Small integers are
compared as numbers (the sign of a zero is not specified, a NaN in class and place); real values against the bound of
tests/valuecheck.py for ANY order of a row's K = entries + 2 operations (Higham §3.1: the products' sum, the scaling by
alpha, the addition of beta y) -- a derived bound, no entry excluded.  Every output array carries sentinels behind its end
and in the gaps of its leading dimension, X's gap columns hold NaN, and wherever beta == 0 the output is prefilled with
NaN: none of it may reach a result, nothing may be written there.  The kernel families that ran are compared with what k
and the row lengths predict."""
import functools
import os
import subprocess

import numpy as np
import pytest
import torch

from conftest import ROOT, load_golden
from helpers import random_csr, wide_values
import spmvref as sr
from valuecheck import check_values

from benchmark_spgemm_using_csr_amd import _lib, dense
from benchmark_spgemm_using_csr_amd.facade import BHSPARSE_HIP, NUM_PLATFORMS, BhsparseError, bhsparse

pytestmark = pytest.mark.gpu

DTYPES = (np.float64, np.float32)
INV = _lib.BHS_ERR_INVALID_ARG
SENTINEL = -7.0
PAD = 64
KS = (1, 2, 3, 4, 5, 8, 9, 16, 17, 32, 33, 64, 65, 130)


# ---------------------------------------------------------------- helpers
def new_handle(dtype=np.float64, options=None):
    plats = [False] * NUM_PLATFORMS
    plats[BHSPARSE_HIP] = True
    bh = bhsparse(value_dtype=dtype)
    assert bh.initPlatform(plats) == 0
    for key, val in (options or {}).items():
        assert bh.set_option(key, val) == 0, key
    return bh


@pytest.fixture(scope="module", params=DTYPES, ids=("f64", "f32"))
def hd(request):
    bh = new_handle(request.param)
    yield bh, request.param
    bh.freePlatform()


def bits(x):
    x = np.ascontiguousarray(x)
    return x.view(np.uint64 if x.dtype == np.float64 else np.uint32)


def up(a, dt):
    return torch.from_numpy(np.ascontiguousarray(a, dt).copy()).cuda()


def tdt(dtype):
    return torch.float32 if np.dtype(dtype) == np.dtype(np.float32) else torch.float64


def families(bh):
    return {s["name"] for s in bh.kernel_stats() if s["launches"] > 0}


def expected_families(Ap, k):
    lens = np.diff(np.asarray(Ap, np.int64))
    prefix = "spmv" if k == 1 else "spmm"
    fam = {prefix + "_short"}
    if np.any((lens > 32) & (lens <= 1024)):
        fam.add(prefix + "_wave")
    if np.any(lens > 1024):
        fam.add(prefix + "_long")
    return fam


def same_numbers(got, ref, what):
    """equal as numbers: +-0 compare equal, a NaN in class and place"""
    assert got.dtype == ref.dtype and got.shape == ref.shape, (what, got.dtype, got.shape, ref.shape)
    gn, rn = np.isnan(got), np.isnan(ref)
    assert np.array_equal(gn, rn), (what, "NaN in other places", np.argwhere(gn != rn)[:5])
    bad = np.argwhere(~rn & (got != ref))
    assert len(bad) == 0, (what, len(bad), bad[:5], got[tuple(bad[0])], ref[tuple(bad[0])])


class Dev:
    """A on the device, uploaded once per (matrix, dtype)"""

    def __init__(self, m, n, A, dtype):
        self.m, self.n, self.dtype = m, n, dtype
        self.Ap, self.Aj = np.ascontiguousarray(A[0], np.int32), np.ascontiguousarray(A[1], np.int32)
        self.Ax = None if A[2] is None else np.ascontiguousarray(A[2], dtype)
        self.nnz = len(self.Aj)
        self.d = (up(self.Ap, np.int32), up(self.Aj, np.int32), None if self.Ax is None else up(self.Ax, dtype))


def run(bh, D, X, alpha=1.0, beta=0.0, Y=None, gap=0, values=True, vector_call=None, want=0, what=""):
    """The device's answer (numpy, m x k) to X (numpy, n x k) and Y (numpy m x k; None with beta == 0: the output is then
    prefilled with NaN).  gap: ld = k + gap for X and Y.  The sentinels behind Y and in its gaps are checked, X's gaps hold
    NaN; with want == 0 the families that ran too.  vector_call: bhs_csr_spmv_device (default where k == 1 and gap == 0)."""
    m, n, k = D.m, D.n, X.shape[1]
    ld = k + gap
    t = tdt(D.dtype)
    dX = torch.full((max(n, 1), ld), float("nan"), dtype=t).cuda()
    dX[:n, :k] = up(X, D.dtype)
    buf = torch.full((m * ld + PAD,), SENTINEL, dtype=t).cuda()
    view = buf[:m * ld].view(m, ld)
    view[:, :k] = float("nan") if Y is None else up(Y, D.dtype)
    assert Y is not None or beta == 0.0
    torch.cuda.synchronize()
    dAx = D.d[2] if values else None
    if vector_call is None:
        vector_call = k == 1 and gap == 0
    if vector_call:
        err = dense.csr_spmv_raw_device(bh, m, n, D.nnz, dAx, D.d[0], D.d[1], alpha, dX, beta, buf)
    else:
        err = dense.csr_spmm_raw_device(bh, m, n, D.nnz, dAx, D.d[0], D.d[1], k, alpha, dX, ld, beta, buf, ld)
    assert err == want, (what, k, gap, err)
    assert bool((buf[m * ld:] == SENTINEL).all()), (what, k, gap, "written past the end of Y")
    assert bool((view[:, k:] == SENTINEL).all()), (what, k, gap, "written into the gaps of Y's leading dimension")
    if want == 0:
        assert families(bh) == expected_families(D.Ap, k), (what, k, families(bh), expected_families(D.Ap, k))
        assert bh.spmv_ms >= 0.0
    return view[:, :k].cpu().numpy()


# ---------------------------------------------------------------- the matrices
LADDER = (0, 1, 16, 17, 32, 33, 64, 65, 1024, 1025, 5000)
N_LADDER = 6007


def rows_matrix(lens, n, seed):
    """rows of these lengths in this order: columns in no order, duplicate pairs in the rows that have room, small signed
    integers (zeros among them) as values"""
    rng = np.random.default_rng(seed)
    lens = np.asarray(lens, np.int64)
    m = len(lens)
    Ap = np.zeros(m + 1, np.int32)
    np.cumsum(lens, out=Ap[1:])
    Aj = np.concatenate([rng.choice(n, L, replace=False) for L in lens] + [np.zeros(0, np.int64)]).astype(np.int32)
    for i in range(m):
        a, L = Ap[i], lens[i]
        if L >= 16:
            Aj[a + 5] = Aj[a + 4]                                   # a duplicate pair, side by side ...
            Aj[a + L - 1] = Aj[a]                                   # ... and at the row's two ends
    Ax = rng.integers(-4, 5, Ap[-1]).astype(np.float64)
    return m, n, (Ap, Aj, Ax)


@functools.lru_cache(maxsize=None)
def ladder_matrix(order):
    """every length of the ladder twice in a random order between a first and a last row of `order`'s lengths"""
    rng = np.random.default_rng(41)
    first, last = order
    mid = list(LADDER + LADDER)
    mid.remove(first)
    mid.remove(last)
    lens = [first] + list(rng.permutation(mid)) + [last]
    return rows_matrix(lens, N_LADDER, 42)


@functools.lru_cache(maxsize=None)
def alone_matrix(length):
    """300 short rows and ONE row of this length in their midst: a queue of one row"""
    rng = np.random.default_rng(43)
    lens = list(rng.integers(0, 33, 300))
    lens[137] = length
    return rows_matrix(lens, N_LADDER, 44)


@functools.lru_cache(maxsize=None)
def random_matrix(m, n, seed, density=0.05):
    rng = np.random.default_rng(seed)
    Ap, Aj, _ = random_csr(m, n, density, rng, empty_rows=(3, m - 1) if m > 4 else ())
    Aj = np.array(Aj, np.int32)
    for i in range(m):
        o = rng.permutation(Ap[i + 1] - Ap[i]) + Ap[i]
        Aj[Ap[i]:Ap[i + 1]] = Aj[o]
    return m, n, (Ap, Aj, rng.integers(-4, 5, len(Aj)).astype(np.float64))


def empty_matrix(m, n):
    return m, n, (np.zeros(m + 1, np.int32), np.zeros(0, np.int32), np.zeros(0))


MATRICES = {
    "ladder 33..1025": lambda: ladder_matrix((33, 1025)),
    "ladder 1025..33": lambda: ladder_matrix((1025, 33)),
    "33 alone": lambda: alone_matrix(33),
    "1025 alone": lambda: alone_matrix(1025),
    "rectangular": lambda: random_matrix(300, 457, 31),
    "one row": lambda: random_matrix(1, 500, 32, 0.2),
    "one column": lambda: rows_matrix([1, 0, 1, 1, 0] * 60, 1, 33),
    "short rows": lambda: random_matrix(700, 300, 34, 0.03),
    "empty rows": lambda: empty_matrix(300, 40),
    "no rows": lambda: empty_matrix(0, 40),
    "no columns": lambda: empty_matrix(40, 0),
    "nothing": lambda: empty_matrix(0, 0),
}


@functools.lru_cache(maxsize=None)
def dev(name, dtype):
    m, n, A = MATRICES[name]()
    return Dev(m, n, A, dtype)


def int_dense(rows, k, seed):
    return np.random.default_rng(seed).integers(-3, 4, (rows, k)).astype(np.float64)


@functools.lru_cache(maxsize=None)
def ladder_reference(k, dtype):
    """X, Y and the reference of alpha = -2, beta = 1 on the first ladder matrix: computed once per k"""
    m, n, A = MATRICES["ladder 33..1025"]()
    X, Y = int_dense(n, k, 100 + k), int_dense(m, k, 200 + k)
    return X, Y, sr.spmm(m, n, A[0], A[1], A[2], X, -2.0, 1.0, Y, dtype)[0]


# ---------------------------------------------------------------- small integers: equal as numbers
def test_the_ladder_holds_every_bin_edge():
    m, n, A = MATRICES["ladder 33..1025"]()
    lens = np.diff(A[0])
    assert sorted(lens) == sorted(LADDER + LADDER) and lens[0] == 33 and lens[-1] == 1025 and n >= 5000
    lens = np.diff(MATRICES["ladder 1025..33"]()[2][0])
    assert lens[0] == 1025 and lens[-1] == 33
    for L in (33, 1025):
        lens = np.diff(MATRICES["%d alone" % L]()[2][0])
        assert np.count_nonzero(lens > 32) == 1 and lens.max() == L
    assert np.diff(MATRICES["short rows"]()[2][0]).max() <= 32
    m, n, A = MATRICES["ladder 33..1025"]()
    # every sum of the exact tests stays an integer below 2^24: exact in both builds whatever the order
    assert 5000 * 4 * 3 * 2 + 2 * 3 < 2 ** 24


@pytest.mark.parametrize("name", sorted(MATRICES))
def test_small_integers_are_exact(hd, name):
    bh, dtype = hd
    D = dev(name, dtype)
    for k in (1, 5):
        X, Y = int_dense(D.n, k, 11), int_dense(D.m, k, 12)
        for alpha in (1.0, -2.0):
            for beta in (1.0, -1.0, 2.0, 0.0):
                ref = sr.spmm(D.m, D.n, D.Ap, D.Aj, D.Ax, X, alpha, beta, Y, dtype)[0]
                got = run(bh, D, X, alpha, beta, Y if beta else None, what=name)
                same_numbers(got, ref, (name, k, alpha, beta))
        # without values: A's pattern of ones
        ref = sr.spmm(D.m, D.n, D.Ap, D.Aj, None, X, -2.0, 1.0, Y, dtype)[0]
        same_numbers(run(bh, D, X, -2.0, 1.0, Y, values=False, what=name + " pattern"), ref, (name, k, "pattern"))
    if name == "short rows":                                        # no row beyond the short bin: one family, no round trip
        assert families(bh) == {"spmm_short"}
        run(bh, D, int_dense(D.n, 1, 13))
        assert families(bh) == {"spmv_short"}


@pytest.mark.parametrize("gap", (0, 3))
@pytest.mark.parametrize("k", KS)
def test_every_column_count_on_the_ladder(hd, k, gap):
    bh, dtype = hd
    D = dev("ladder 33..1025", dtype)
    X, Y, ref = ladder_reference(k, dtype)
    same_numbers(run(bh, D, X, -2.0, 1.0, Y, gap=gap, what="ladder"), ref, ("ladder", k, gap))
    if k == 1:                                                      # the matrix call with one column is the vector call
        for vector_call in (False, True):
            same_numbers(run(bh, D, X, -2.0, 1.0, Y, gap=0, vector_call=vector_call, what="ladder"), ref, ("ladder", vector_call))


# ---------------------------------------------------------------- real values within the bound
@pytest.mark.parametrize("name", ("ladder 33..1025", "ladder 1025..33", "rectangular", "one row"))
def test_real_values_within_the_bound(hd, name):
    bh, dtype = hd
    m, n, A = MATRICES[name]()
    rng = np.random.default_rng(53)
    rounded = lambda v: np.ascontiguousarray(v, dtype).astype(np.float64)   # noqa: E731  (the values as the build holds them)
    D = Dev(m, n, (A[0], A[1], rounded(wide_values(len(A[1]), rng))), dtype)
    mode = "f64" if dtype == np.float64 else "f32_once"
    for k in (1, 5, 17):
        X, Y = rounded(wide_values(n * k, rng)).reshape(n, k), rounded(wide_values(m * k, rng)).reshape(m, k)
        for alpha, beta in ((1.0, 0.0), (-0.75, 1.5)):
            ref, S, K = sr.spmm(m, n, D.Ap, D.Aj, D.Ax.astype(np.float64), X, alpha, beta, Y, np.float64)
            got = run(bh, D, X, alpha, beta, Y if beta else None, gap=3 if k == 5 else 0, what=name)
            worst = check_values(ref, S, K, got, mode, "%s k %d alpha %g beta %g: " % (name, k, alpha, beta))
            print("%s k %d alpha %g beta %g %s: worst err/bound %.3g" % (name, k, alpha, beta, mode, worst))


# ---------------------------------------------------------------- non-finite values
def special_values(count, rng):
    v = rng.standard_normal(count)
    pick = rng.random(count)
    v[pick < 0.01] = np.nan
    v[(pick >= 0.01) & (pick < 0.03)] = np.inf
    v[(pick >= 0.03) & (pick < 0.05)] = -np.inf
    v[(pick >= 0.05) & (pick < 0.15)] = 0.0
    v[(pick >= 0.15) & (pick < 0.25)] = -0.0
    return v


@pytest.mark.parametrize("name", ("rectangular", "ladder 33..1025"))
def test_nan_and_infinities_keep_class_and_place(hd, name):
    bh, dtype = hd
    m, n, A = MATRICES[name]()
    rng = np.random.default_rng(61)
    D = Dev(m, n, (A[0], A[1], special_values(len(A[1]), rng)), dtype)
    mode = "f64" if dtype == np.float64 else "f32_once"
    for k in (1, 5):
        X, Y = special_values(n * k, rng).reshape(n, k), special_values(m * k, rng).reshape(m, k)
        X, Y = X.astype(dtype).astype(np.float64), Y.astype(dtype).astype(np.float64)
        for alpha, beta in ((1.0, 0.0), (-2.0, 1.0), (0.0, 1.0)):
            ref, S, K = sr.spmm(m, n, D.Ap, D.Aj, D.Ax.astype(np.float64), X, alpha, beta, Y, np.float64)
            assert np.isnan(ref).any() and (name != "rectangular" or np.isfinite(ref).any())
            got = run(bh, D, X, alpha, beta, Y if beta else None, what=name + " special")
            check_values(ref, S, K, got, mode, "%s special k %d alpha %g beta %g: " % (name, k, alpha, beta))


def test_alpha_zero_takes_no_shortcut_and_beta_zero_never_reads_y(hd):
    bh, dtype = hd
    Ap, Aj = np.array([0, 2, 4, 4]), np.array([0, 1, 1, 2])
    D = Dev(3, 3, (Ap, Aj, np.array([1.0, np.inf, 2.0, 3.0])), dtype)
    x = np.array([[1.0], [1.0], [1.0]])
    got = run(bh, D, x, 0.0, 0.0)                                   # (the output is prefilled with NaN)
    assert np.isnan(got[0, 0]) and got[1, 0] == 0.0 and got[2, 0] == 0.0, got
    got = run(bh, D, x, 1.0, 0.0)
    assert got[0, 0] == np.inf and got[1, 0] == 5.0 and got[2, 0] == 0.0, got
    got = run(bh, D, np.array([[1.0], [0.0], [1.0]]), 1.0, 0.0)     # Inf * 0
    assert np.isnan(got[0, 0]) and got[1, 0] == 3.0, got


# ---------------------------------------------------------------- repeatable
@pytest.mark.parametrize("k", (1, 5))
def test_two_calls_give_the_same_bits(hd, k):
    bh, dtype = hd
    m, n, A = MATRICES["ladder 33..1025"]()
    rng = np.random.default_rng(70 + k)
    D = Dev(m, n, (A[0], A[1], wide_values(len(A[1]), rng)), dtype)
    X, Y = wide_values(n * k, rng).reshape(n, k), wide_values(m * k, rng).reshape(m, k)
    a = run(bh, D, X, -0.75, 1.5, Y)
    b = run(bh, D, X, -0.75, 1.5, Y)
    assert np.array_equal(bits(a), bits(b))
    assert np.array_equal(bits(run(bh, D, X)), bits(run(bh, D, X)))


# ---------------------------------------------------------------- refusals
def bad_inputs():
    """(the word spmvref gives, Ap, Aj): inputs the device's checks must refuse; every array keeps the size the call is
    told, so nothing is read out of bounds whatever the check does"""
    m, n, (Ap, Aj, Ax) = MATRICES["ladder 33..1025"]()
    nnz = len(Aj)
    p0 = Ap.copy(); p0[0] = 1
    pm = Ap.copy(); pm[-1] = nnz - 1
    pd = Ap.copy(); pd[10], pd[11] = Ap[11], Ap[10]
    assert pd[10] > pd[11]
    lens = np.diff(Ap)
    cases = [("rowPtrA[0] != 0", p0, Aj), ("rowPtrA[m] != nnzA", pm, Aj), ("decreasing rowPtrA", pd, Aj)]
    for L, col in ((17, -1), (17, n), (65, n), (65, -1), (5000, n), (5000, -1)):   # a bad column in every bin
        j = Aj.copy()
        j[Ap[int(np.flatnonzero(lens == L)[0])] + L // 2] = col
        cases.append(("column of A out of range", Ap, j))
    return m, n, Ax, cases


def test_invalid_inputs_are_refused(hd):
    bh, dtype = hd
    m, n, Ax, cases = bad_inputs()
    good = dev("ladder 33..1025", dtype)
    for word, Ap, Aj in cases:
        assert sr.invalid(m, n, Ap, Aj) == word and word in sr.DEVICE_REFUSALS
        D = Dev(m, n, (Ap, Aj, Ax), dtype)
        for k, gap in ((1, 0), (5, 3)):
            X, Y = int_dense(n, k, 21), int_dense(m, k, 22)
            run(bh, D, X, 1.0, 1.0, Y, gap=gap, want=INV, what=word)   # (y may be partly written; never outside its m x k elements)
            # the handle still answers a valid call
            X, Y, ref = ladder_reference(k, dtype)
            same_numbers(run(bh, good, X, -2.0, 1.0, Y, gap=gap, what="after " + word), ref, ("after", word, k))


def test_host_side_refusals_leave_y_untouched(hd):
    bh, dtype = hd
    D = dev("rectangular", dtype)
    m, n, k, ld = D.m, D.n, 4, 6
    t = tdt(dtype)
    X = torch.ones((n, ld), dtype=t).cuda()
    Y = torch.full((m * ld + PAD,), SENTINEL, dtype=t).cuda()
    torch.cuda.synchronize()
    Ap, Aj, Ax = D.d

    def mm(m=m, n=n, nnz=D.nnz, Ax=Ax, Ap=Ap, Aj=Aj, k=k, X=X, ldX=ld, Y=Y, ldY=ld):
        return dense.csr_spmm_raw_device(bh, m, n, nnz, Ax, Ap, Aj, k, 1.0, X, ldX, 1.0, Y, ldY)

    def mv(m=m, n=n, nnz=D.nnz, Ax=Ax, Ap=Ap, Aj=Aj, x=X, y=Y):
        return dense.csr_spmv_raw_device(bh, m, n, nnz, Ax, Ap, Aj, 1.0, x, 1.0, y)

    refused = {
        "negative size": (mm(m=-1), mm(n=-1), mm(nnz=-1), mv(m=-1), mv(n=-1), mv(nnz=-1)),
        "k < 1": (mm(k=0), mm(k=-3)),
        "ldX < k": (mm(ldX=k - 1),),
        "ldY < k": (mm(ldY=k - 1),),
        "NULL rowPtrA": (mm(Ap=None), mv(Ap=None)),
        "NULL colIndA": (mm(Aj=None), mv(Aj=None)),
        "NULL x": (mm(X=None), mv(x=None)),
        "NULL y": (mm(Y=None), mv(y=None)),
        "y overlaps an input": (mm(Y=X), mm(Y=Ax), mv(y=X), mv(y=Ax), mm(X=Y[k:]), mv(x=Y[m - 1:])),
    }
    assert sorted(refused) == sorted(sr.HOST_REFUSALS)
    for word, codes in refused.items():
        assert all(c == INV for c in codes), (word, codes)
    assert bool((Y == SENTINEL).all()), "y written by a refused call"
    # NULL arrays that are legal: no entries, no rows
    E = dev("empty rows", dtype)
    assert dense.csr_spmv_raw_device(bh, E.m, E.n, 0, None, E.d[0], None, 1.0, None, 0.0, Y) == 0
    assert bool((Y[:E.m] == 0).all()) and bool((Y[E.m:] == SENTINEL).all())
    Z = dev("no rows", dtype)
    assert dense.csr_spmv_raw_device(bh, 0, Z.n, 0, None, Z.d[0], None, 1.0, X, 0.0, None) == 0
    assert dense.csr_spmv_raw_device(bhsparse(dtype), 0, 0, 0, None, None, None, 1.0, None, 0.0, None) == _lib.BHS_ERR_NOT_READY
    assert dense.csr_spmm_raw_device(bhsparse(dtype), 0, 0, 0, None, None, None, 1, 1.0, None, 1, 0.0, None, 1) == _lib.BHS_ERR_NOT_READY


def test_refused_between_symbolic_and_finish():
    m = n = 300
    A = random_csr(m, n, 0.05, np.random.default_rng(34))
    D = Dev(m, n, A, np.float64)
    x = int_dense(n, 1, 35)
    dx = up(x, np.float64)
    y = torch.full((m + PAD,), SENTINEL, dtype=torch.float64).cuda()
    bh = new_handle()
    try:
        assert bh.initData_device(m, n, n, D.nnz, D.d[2], D.d[0], D.d[1], D.nnz, D.d[2], D.d[0], D.d[1]) == 0
        assert bh.spgemm_symbolic() == 0
        assert dense.csr_spmv_raw_device(bh, m, n, D.nnz, D.d[2], D.d[0], D.d[1], 1.0, dx, 0.0, y) == INV
        assert dense.csr_spmm_raw_device(bh, m, n, D.nnz, D.d[2], D.d[0], D.d[1], 1, 1.0, dx, 1, 0.0, y, 1) == INV
        assert bool((y == SENTINEL).all())
        assert bh.spgemm_numeric(0, m) == 0 and bh.spgemm_finish() == 0
        assert dense.csr_spmv_raw_device(bh, m, n, D.nnz, D.d[2], D.d[0], D.d[1], 1.0, dx, 0.0, y) == 0
        same_numbers(y[:m].cpu().numpy(), sr.spmv(m, n, D.Ap, D.Aj, D.Ax, x)[0], "after finish")
        assert bool((y[m:] == SENTINEL).all())
        bh.free_mem()
    finally:
        bh.freePlatform()


# ---------------------------------------------------------------- the handle is left alone
@pytest.mark.parametrize("dtype", DTYPES)
def test_products_leave_the_handle_alone_and_apply_its_C(dtype, oracle):
    g = load_golden("p9_12.npz")
    m, kk, n = int(g["m"]), int(g["k"]), int(g["n"])
    rng = np.random.default_rng(15)
    Ap, Aj, Bp, Bj = (np.ascontiguousarray(g[key], np.int32) for key in ("Ap", "Aj", "Bp", "Bj"))
    Ax, Bx = (np.ascontiguousarray(rng.integers(1, 5, len(j)), dtype) for j in (Aj, Bj))
    L = dev("ladder 33..1025", dtype)
    keys = ("class_state", "mixed_rows", "spec_launches", "spec_refuted", "b_sorted", "max_row_a", "max_row_b",
            "select_dropped", "add_inplace_used", "extract_reordered_rows")

    def multiply(bh):
        Cp = np.zeros(m + 1, np.int32)
        assert bh.initData(m, kk, n, len(Aj), Ax, Ap, Aj, len(Bj), Bx, Bp, Bj, Cp) == 0
        assert bh.spgemm() == 0 and bh.spgemm() == 0                # (the second one launches speculatively where the class path runs)
        return Cp, state(bh)

    def state(bh):
        """what the last multiply reports: the handle's figures and the kernels that ran"""
        return {key: bh.get_info(key) for key in keys}, sorted((s["name"], s["launches"]) for s in bh.kernel_stats() if s["launches"])

    fresh = new_handle(dtype, {"class_path": 2})
    try:
        multiply(fresh)
        assert fresh.spgemm() == 0
        fresh_third = state(fresh)
        fresh.free_mem()
    finally:
        fresh.freePlatform()
    bh = new_handle(dtype, {"class_path": 2})
    try:
        Cp, (before, _) = multiply(bh)
        nnzC, ptrs = bh.get_nnzC(), bh.get_C_device()
        Cj, Cx = np.empty(nnzC, np.int32), np.empty(nnzC, dtype)
        assert bh.get_C(Cj, Cx) == 0
        ref = oracle.spgemm(m, kk, n, Ap, Aj, Ax.astype(np.float64), Bp, Bj, Bx.astype(np.float64))
        assert np.array_equal(Cp, ref[0]) and np.array_equal(Cj, ref[1]) and np.array_equal(Cx, ref[2].astype(dtype))

        def unchanged(what):
            assert {key: bh.get_info(key) for key in keys} == before, what
            assert bh.get_nnzC() == nnzC and bh.get_C_device() == ptrs, what
            j2, x2 = np.empty(nnzC, np.int32), np.empty(nnzC, dtype)
            assert bh.get_C(j2, x2) == 0
            assert np.array_equal(j2, Cj) and np.array_equal(bits(x2), bits(Cx)) and np.array_equal(bh.get_rowptrC(), Cp), what
        for k in (1, 5):
            X, Y, want = ladder_reference(k, dtype)
            same_numbers(run(bh, L, X, -2.0, 1.0, Y, what="beside a multiply"), want, ("beside a multiply", k))
            unchanged("after k = %d" % k)
        # the product itself, straight from the device pointers and without a copy: C x == A (B x)
        x = int_dense(n, 1, 16)
        y = torch.full((m + PAD,), SENTINEL, dtype=tdt(dtype)).cuda()
        dx = up(x, dtype)
        torch.cuda.synchronize()
        assert dense.csr_spmv_raw_device(bh, m, n, nnzC, ptrs[2], ptrs[0], ptrs[1], 1.0, dx, 0.0, y) == 0
        Bx_ = sr.spmv(kk, n, Bp, Bj, Bx, x, dtype=dtype)[0]
        ABx = sr.spmv(m, kk, Ap, Aj, Ax, Bx_, dtype=dtype)[0]
        same_numbers(y[:m].cpu().numpy(), ABx, "C x against A (B x)")
        assert bool((y[m:] == SENTINEL).all())
        unchanged("after applying C")
        assert bh.spgemm() == 0                                     # and the next multiply is what a fresh handle's third is
        assert state(bh) == fresh_third and bh.get_nnzC() == nnzC
        bh.free_mem()
    finally:
        bh.freePlatform()


# ---------------------------------------------------------------- the tensor calls and the conveniences
@pytest.mark.parametrize("dtype", DTYPES)
def test_tensor_calls_take_the_leading_dimension_from_the_stride(dtype):
    D = dev("rectangular", dtype)
    k = 5
    X, Y = int_dense(D.n, k, 81), int_dense(D.m, k, 82)
    wideX = torch.full((D.n, k + 3), float("nan"), dtype=tdt(dtype)).cuda()
    wideX[:, :k] = up(X, dtype)
    wideY = torch.full((D.m, k + 2), SENTINEL, dtype=tdt(dtype)).cuda()
    wideY[:, :k] = up(Y, dtype)
    bh = new_handle(dtype)
    try:
        out = dense.csr_spmm_device(bh, D.m, D.n, D.d, wideX[:, :k], 2.0, -1.0, wideY[:, :k])
        assert out.data_ptr() == wideY.data_ptr()
        same_numbers(wideY[:, :k].cpu().numpy(), sr.spmm(D.m, D.n, D.Ap, D.Aj, D.Ax, X, 2.0, -1.0, Y, dtype)[0], "strided")
        assert bool((wideY[:, k:] == SENTINEL).all())
        out = dense.csr_spmm_device(bh, D.m, D.n, D.d, wideX[:, :k])
        assert out.shape == (D.m, k) and out.is_contiguous()
        same_numbers(out.cpu().numpy(), sr.spmm(D.m, D.n, D.Ap, D.Aj, D.Ax, X, dtype=dtype)[0], "allocated")
        y = dense.csr_spmv_device(bh, D.m, D.n, (D.d[0], D.d[1], None), up(X[:, 0], dtype))
        same_numbers(y.cpu().numpy(), sr.spmv(D.m, D.n, D.Ap, D.Aj, None, X[:, 0], dtype=dtype)[0], "pattern")
        bad = D.Aj.copy()
        bad[7] = D.n
        with pytest.raises(BhsparseError) as ei:
            dense.csr_spmv_device(bh, D.m, D.n, (D.d[0], up(bad, np.int32), D.d[2]), up(X[:, 0], dtype))
        assert ei.value.code == INV
        with pytest.raises(ValueError):
            dense.csr_spmm_device(bh, D.m, D.n, D.d, torch.zeros((k, D.n), dtype=tdt(dtype)).cuda().t())   # (column-major)
    finally:
        bh.freePlatform()


@pytest.mark.parametrize("dtype", DTYPES)
def test_conveniences_on_host_arrays(dtype):
    m, n, A = MATRICES["ladder 1025..33"]()
    k = 3
    X, Y = int_dense(n, k, 91), int_dense(m, k, 92)
    got, info = dense.spmm_csr(m, n, A[0], A[1], A[2], X, 2.0, -1.0, Y, value_dtype=dtype)
    same_numbers(got, sr.spmm(m, n, A[0], A[1], A[2], X, 2.0, -1.0, Y, dtype)[0], "spmm_csr")
    assert {s["name"] for s in info["kernels"] if s["launches"] > 0} == {"spmm_short", "spmm_wave", "spmm_long"} and info["ms"] >= 0
    got, info = dense.spmv_csr(m, n, A[0], A[1], A[2], X[:, 0], value_dtype=dtype)
    same_numbers(got, sr.spmv(m, n, A[0], A[1], A[2], X[:, 0], dtype=dtype)[0], "spmv_csr")
    assert {s["name"] for s in info["kernels"] if s["launches"] > 0} == {"spmv_short", "spmv_wave", "spmv_long"}
    b = int_dense(m, 1, 93)[:, 0]
    got, _ = dense.residual_csr(m, n, A[0], A[1], A[2], X[:, 0], b, value_dtype=dtype)
    same_numbers(got, sr.spmv(m, n, A[0], A[1], A[2], X[:, 0], -1.0, 1.0, b, dtype)[0], "residual_csr")
    # the residual of an exact integer solution is all zeros
    exact = sr.spmv(m, n, A[0], A[1], A[2], X[:, 0])[0]
    got, _ = dense.residual_csr(m, n, A[0], A[1], A[2], X[:, 0], exact, value_dtype=dtype)
    assert got.dtype == np.dtype(dtype) and got.shape == (m,) and not got.any()


def test_cpp_demo_runs():
    demo_dir = os.path.join(ROOT, "tests", "spmv")
    subprocess.check_call(["make", "-C", demo_dir, "-s"])
    out = subprocess.run([os.path.join(demo_dir, "spmv_demo")], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "spmv / spmm 5 x 7, 12 entries: PASS" in out.stdout
