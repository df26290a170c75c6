"""bhs_csr_sddmm_device on the GPU, both builds, and amg.affinity_strength_device on top of it.

Reference: tests/sddmmref.py, the rule of include/bhsparse_hip.h ("sampled dense-dense product") restated in numpy.  The
rule fixes the order of every operation, so the comparison is of the value bits (sddmmref.same_bits: equal bits, NaN in
the same places -- which NaN an operation returns is the machine's choice, not the rule's).  Every array the call reads
carries NaN (or a column that is none) in its gap columns and behind its end, Z carries sentinels behind its nnz values."""
import functools
import os
import subprocess

import numpy as np
import pytest
import torch

import matchref
import sddmmref as sd
from conftest import ROOT
from helpers import real_values, wide_values
from test_spmv_gpu import bits, new_handle, rows_matrix, tdt, up

from benchmark_spgemm_using_csr_amd import _lib, amg, dense
from benchmark_spgemm_using_csr_amd.facade import bhsparse

pytestmark = pytest.mark.gpu

DTYPES = (np.float64, np.float32)
INV = _lib.BHS_ERR_INVALID_ARG
SENTINEL = -7.0
PAD = 64
NO_COLUMN = 0x7fffffff
KS = (1, 2, 3, 4, 5, 16, 17, 63, 64, 65, 100, 129)
EDGES = (0, 1, 2, 31, 32, 33, 1023, 1024, 1025, 3000)    # the bins' borders, and a workgroup's row
N = 3001


@pytest.fixture(scope="module", params=DTYPES, ids=("f64", "f32"))
def hd(request):
    bh = new_handle(request.param)
    yield bh, request.param
    bh.freePlatform()


def families(bh):
    return {s["name"] for s in bh.kernel_stats() if s["launches"] > 0}


def expected_families(Mp):
    lens = np.diff(np.asarray(Mp, np.int64))
    fam = {"sddmm_short"}
    if len(lens) and lens.sum() > 32:
        if np.any((lens > 32) & (lens <= 1024)):
            fam.add("sddmm_wave")
        if np.any(lens > 1024):
            fam.add("sddmm_long")
    return fam


@functools.lru_cache(maxsize=None)
def edge_matrix(m):
    """m x N: the lengths of EDGES on both sides of the 256-row border of the first workgroup (and of the next where m
    allows it) among rows of 0 .. 8 entries; columns in no order, duplicate pairs in the rows of 16 entries and more;
    wide real values"""
    rng = np.random.default_rng(100 + m)
    lens = rng.integers(0, 9, m)
    at = list(range(247, 247 + len(EDGES)))                      # rows 247 .. 256: the last of m = 257
    if m >= 600:
        at += list(range(507, 507 + len(EDGES)))
    for r, L in zip(at, EDGES + EDGES):
        if r < m:
            lens[r] = L
    lens[:4] = (3000, 1025, 33, 0)                                # every bin whatever m is
    _, _, (Mp, Mj, _) = rows_matrix(lens, N, 200 + m)
    _, (_, _, Mx), _ = real_values("wide", N, (Mp, Mj, None), (Mp, Mj, None), rng)
    return Mp, Mj, Mx


@functools.lru_cache(maxsize=None)
def dense_pair(m, k, kind="real"):
    rng = np.random.default_rng(1000 * m + k)
    if kind == "int":
        return rng.integers(-4, 5, (m, k)).astype(np.float64), rng.integers(-4, 5, (N, k)).astype(np.float64)
    return wide_values(m * k, rng).reshape(m, k), wide_values(N * k, rng).reshape(N, k)


def padded(a, rows, k, gap, dtype):
    """a (rows x k) in a device array of leading dimension k + gap: NaN in the gap columns and behind the end"""
    ld = k + gap
    buf = torch.full((rows * ld + PAD,), float("nan"), dtype=tdt(dtype)).cuda()
    if rows:
        buf[:rows * ld].view(rows, ld)[:, :k] = up(np.asarray(a).reshape(rows, k), dtype)
    return buf, ld


def run(bh, dtype, m, n, M, X, Y, alpha=1.0, beta=0.0, Z=None, times_m=False, gap=0, in_place=False, same_xy=False, want=0,
        check_families=True):
    """The device's Z (numpy, nnz values) for host arrays.  Z None (beta == 0): the output starts as NaN.  in_place: d_valZ
    is d_valM.  same_xy: d_X is d_Y (X must be Y's first m rows).  The sentinels behind Z's nnz values are checked."""
    Mp, Mj, Mx = M
    nnz = len(Mj)
    k = np.asarray(Y).shape[1]
    dMp = up(Mp, np.int32)
    dMj = up(np.concatenate([Mj, np.full(PAD, NO_COLUMN)]), np.int32)
    dY, ldY = padded(Y, n, k, gap, dtype)
    dX, ldX = (dY, ldY) if same_xy else padded(X, m, k, gap, dtype)
    t = tdt(dtype)
    tail = torch.full((PAD,), SENTINEL, dtype=t).cuda()
    dMx = None
    if times_m or in_place:
        dMx = torch.cat([up(Mx, dtype), tail if in_place else torch.full((PAD,), float("nan"), dtype=t).cuda()])
    if in_place:
        dZ = dMx
    else:
        dZ = torch.cat([torch.full((nnz,), float("nan"), dtype=t).cuda() if Z is None else up(Z, dtype), tail])
    torch.cuda.synchronize()
    err = dense.csr_sddmm_raw_device(bh, m, n, nnz, dMx, dMp, dMj, k, alpha, dX, ldX, dY, ldY, beta, dZ,
                                     _lib.BHS_SDDMM_TIMES_M if times_m else 0)
    assert err == want, (err, want)
    assert bool((dZ[nnz:] == SENTINEL).all()), "written past nnzM"
    if not want:
        assert bh.sddmm_ms >= 0.0
        if check_families:
            assert families(bh) == expected_families(Mp), (families(bh), expected_families(Mp))
    return dZ[:nnz].cpu().numpy()


def agree(got, ref, what):
    assert sd.same_bits(got, ref), (what, np.argwhere(bits(np.nan_to_num(got)) != bits(np.nan_to_num(ref)))[:5])


# ---------------------------------------------------------------- the widths on the bins' borders
def test_the_matrices_hold_every_bin_edge():
    for m in (257, 600):
        Mp, Mj, _ = edge_matrix(m)
        lens = np.diff(Mp)
        assert set(EDGES) <= set(lens.tolist()) and len(Mp) == m + 1 and Mj.max() < N
        assert lens[255] > 0 and lens[256] > 0                    # entries on both sides of the workgroup's border
        assert expected_families(Mp) == {"sddmm_short", "sddmm_wave", "sddmm_long"}
        r = int(np.argmax(lens == 33))                            # unsorted, with a pair twice
        assert np.any(np.diff(Mj[Mp[r]:Mp[r + 1]]) < 0) and len(set(Mj[Mp[r]:Mp[r + 1]].tolist())) < 33


@pytest.mark.parametrize("m", (257, 600))
@pytest.mark.parametrize("k", KS)
def test_every_width_on_the_bin_edges(hd, k, m):
    bh, dtype = hd
    M = edge_matrix(m)
    X, Y = dense_pair(m, k)
    ref = sd.sddmm(m, N, M[0], M[1], None, X, Y, dtype=dtype)
    got = run(bh, dtype, m, N, M, X, Y, gap=3)                    # beta == 0 over a Z of NaN, poisoned gaps
    assert not np.isnan(ref).any()
    agree(got, ref, (k, m))
    agree(run(bh, dtype, m, N, M, X, Y, gap=0), ref, (k, m, "ld == k"))


@pytest.mark.parametrize("alpha", (0.0, 1.0, -0.5))
@pytest.mark.parametrize("beta", (0.0, 1.0, -0.5))
def test_coefficients_and_times_m(hd, alpha, beta):
    bh, dtype = hd
    m, k = 257, 17
    M = edge_matrix(m)
    X, Y = dense_pair(m, k)
    Z = wide_values(len(M[1]), np.random.default_rng(7))
    for times_m in (False, True):
        ref = sd.sddmm(m, N, M[0], M[1], M[2], X, Y, alpha, beta, Z, times_m, dtype)
        got = run(bh, dtype, m, N, M, X, Y, alpha, beta, None if beta == 0.0 else Z, times_m, gap=2)
        agree(got, ref, (alpha, beta, times_m))


@pytest.mark.parametrize("k", (5, 100))
def test_in_place_on_the_values_of_m(hd, k):
    bh, dtype = hd
    m = 257
    M = edge_matrix(m)
    X, Y = dense_pair(m, k)
    ref = sd.sddmm(m, N, M[0], M[1], M[2], X, Y, -0.5, 1.0, M[2], True, dtype)
    agree(run(bh, dtype, m, N, M, X, Y, -0.5, 1.0, times_m=True, in_place=True, gap=1), ref, k)
    ref = sd.sddmm(m, N, M[0], M[1], None, X, Y, 1.0, -0.5, M[2], False, dtype)
    agree(run(bh, dtype, m, N, M, X, Y, 1.0, -0.5, in_place=True), ref, (k, "without TIMES_M"))


@pytest.mark.parametrize("k", (3, 65))
def test_x_and_y_may_be_one_array(hd, k):
    bh, dtype = hd
    m = 257
    M = edge_matrix(m)
    _, Y = dense_pair(m, k)
    ref = sd.sddmm(m, N, M[0], M[1], None, Y[:m], Y, dtype=dtype)
    agree(run(bh, dtype, m, N, M, Y[:m], Y, same_xy=True, gap=2), ref, k)


@pytest.mark.parametrize("k", (4, 129))
def test_small_integers_are_exact(hd, k):
    bh, dtype = hd
    m = 257
    Mp, Mj, _ = edge_matrix(m)
    Mx = np.random.default_rng(3).integers(-3, 4, len(Mj)).astype(np.float64)
    X, Y = dense_pair(m, k, "int")
    rows = np.repeat(np.arange(m), np.diff(Mp))
    exact = (2.0 * np.einsum("ij,ij->i", X[rows], Y[Mj]) * Mx + Mx).astype(dtype)
    ref = sd.sddmm(m, N, Mp, Mj, Mx, X, Y, 2.0, 1.0, Mx, True, dtype)
    assert np.array_equal(ref, exact)
    got = run(bh, dtype, m, N, (Mp, Mj, Mx), X, Y, 2.0, 1.0, Mx, True)
    assert np.array_equal(got, exact)


def test_nan_and_infinities_propagate_as_the_rule_says(hd):
    bh, dtype = hd
    m, k = 257, 17
    Mp, Mj, Mx = edge_matrix(m)
    X, Y = (a.copy() for a in dense_pair(m, k))
    Mx = Mx.copy()
    rng = np.random.default_rng(11)
    for a in (X, Y):
        flat = a.reshape(-1)
        at = rng.choice(flat.size, 12, replace=False)
        flat[at] = np.tile([np.inf, -np.inf, np.nan, 0.0], 3)
    Mx[rng.choice(len(Mx), 40, replace=False)] = np.tile([np.inf, -np.inf, np.nan, 0.0], 10)
    for alpha, times_m in ((1.0, False), (0.0, True), (-0.5, True)):   # alpha == 0 takes no shortcut: 0 * Inf is NaN
        ref = sd.sddmm(m, N, Mp, Mj, Mx, X, Y, alpha, 0.0, None, times_m, dtype)
        assert np.isnan(ref).any() and np.isinf(ref).any() == (alpha != 0.0)
        agree(run(bh, dtype, m, N, (Mp, Mj, Mx), X, Y, alpha, 0.0, None, times_m), ref, (alpha, times_m))


# ---------------------------------------------------------------- the same bits everywhere
@pytest.mark.parametrize("k", (3, 16, 100))
def test_one_pair_has_the_same_bits_in_every_bin_and_place(hd, k):
    bh, dtype = hd
    lens = (5, 100, 2000, 1, 33)
    m = len(lens)
    rng = np.random.default_rng(17)
    _, _, (Mp, Mj, _) = rows_matrix(lens, N, 18)
    where = [int(Mp[i] + rng.integers(0, L)) for i, L in enumerate(lens)]
    Mj[where] = 77                                                # the pair's column, somewhere in every row
    X, Y = wide_values(m * k, rng).reshape(m, k), wide_values(N * k, rng).reshape(N, k)
    X[:] = X[0]                                                   # ... and every row of X the same
    ref = sd.sddmm(m, N, Mp, Mj, None, X, Y, dtype=dtype)
    got = run(bh, dtype, m, N, (Mp, Mj, None), X, Y, gap=1)
    agree(got, ref, k)
    assert len(set(bits(got[where]).tolist())) == 1 and len(set(bits(ref[where]).tolist())) == 1


def test_two_runs_and_two_handles_give_the_same_arrays(hd):
    bh, dtype = hd
    m, k = 600, 65
    M = edge_matrix(m)
    X, Y = dense_pair(m, k)
    first = run(bh, dtype, m, N, M, X, Y, -0.5, 1.0, M[2], True)
    again = run(bh, dtype, m, N, M, X, Y, -0.5, 1.0, M[2], True)
    other = new_handle(dtype)
    try:
        third = run(other, dtype, m, N, M, X, Y, -0.5, 1.0, M[2], True)
    finally:
        other.freePlatform()
    assert np.array_equal(bits(first), bits(again)) and np.array_equal(bits(first), bits(third))


# ---------------------------------------------------------------- the smallest shapes
def test_one_by_one_no_entries_no_rows(hd):
    bh, dtype = hd
    one = (np.array([0, 1]), np.array([0]), np.array([3.0]))
    for k in (1, 5):
        X, Y = np.arange(1, k + 1, dtype=np.float64).reshape(1, k), np.full((1, k), 0.5)
        ref = sd.sddmm(1, 1, one[0], one[1], one[2], X, Y, 2.0, 0.0, None, True, dtype)
        agree(run(bh, dtype, 1, 1, one, X, Y, 2.0, 0.0, None, True, gap=1), ref, k)
        assert ref[0] == 3.0 * k * (k + 1) / 2
    empty = (np.zeros(6, np.int64), np.zeros(0, np.int64), np.zeros(0))
    X, Y = np.ones((5, 3)), np.ones((4, 3))
    assert len(run(bh, dtype, 5, 4, empty, X, Y)) == 0 and families(bh) == {"sddmm_short"}
    none = (np.zeros(1, np.int64), np.zeros(0, np.int64), np.zeros(0))
    assert len(run(bh, dtype, 0, 4, none, np.zeros((0, 3)), Y)) == 0
    assert len(run(bh, dtype, 0, 0, none, np.zeros((0, 3)), np.zeros((0, 3)))) == 0
    # NULL arrays that are legal without entries
    t = torch.zeros(8, dtype=torch.int32).cuda()
    assert dense.csr_sddmm_raw_device(bh, 5, 4, 0, None, t, None, 3, 1.0, None, 3, None, 3, 0.0, None, 0) == 0
    assert dense.csr_sddmm_raw_device(bhsparse(dtype), 0, 0, 0, None, None, None, 1, 1.0, None, 1, None, 1, 0.0, None, 0) == _lib.BHS_ERR_NOT_READY


# ---------------------------------------------------------------- refusals
def bad_patterns():
    """(word, Mp, Mj) for every refusal of the device, on a 300 x 50 pattern with rows in every bin of a small matrix"""
    m, n = 300, 50
    lens = np.random.default_rng(23).integers(0, 9, m)
    lens[[3, 200, 299]] = (40, 33, 5)
    _, _, (Mp, Mj, _) = rows_matrix(lens, n, 24)
    out = []
    p = Mp.copy(); p[0] = 1
    out.append(("rowPtrM[0] != 0", p, Mj))
    out.append(("rowPtrM[m] != nnzM", Mp, np.concatenate([Mj, [0]]).astype(np.int32)))
    p = Mp.copy(); p[150], p[151] = Mp[151], Mp[150]
    if p[150] == p[151]:
        p[150] += 1
    out.append(("decreasing rowPtrM", p, Mj))
    for col in (n, -1, NO_COLUMN):
        j = Mj.copy(); j[int(Mp[200]) + 7] = col
        out.append(("column of M out of range", Mp, j))
    return m, n, (Mp, Mj), out


def test_the_device_refuses_bad_patterns_and_writes_nothing_outside(hd):
    bh, dtype = hd
    m, n, (Gp, Gj), cases = bad_patterns()
    assert sorted({w for w, _, _ in cases}) == sorted(sd.DEVICE_REFUSALS)
    k = 5
    rng = np.random.default_rng(25)
    X, Y = wide_values(m * k, rng).reshape(m, k), wide_values(n * k, rng).reshape(n, k)
    for word, Mp, Mj in cases:
        assert sd.invalid(m, n, Mp, Mj, k) == word
        Mx = np.ones(len(Mj))
        run(bh, dtype, m, n, (Mp, Mj, Mx), X, Y, 1.0, 1.0, Mx, True, gap=2, want=INV)   # (run checks the guards behind nnzM)
        # the handle still answers a valid call
        ref = sd.sddmm(m, n, Gp, Gj, None, X, Y, dtype=dtype)
        agree(run(bh, dtype, m, n, (Gp, Gj, None), X, Y, gap=2), ref, ("after", word))


def test_host_side_refusals_leave_z_untouched(hd):
    bh, dtype = hd
    m, n, (Mp, Mj), _ = bad_patterns()
    nnz, k, ld = len(Mj), 4, 6
    t = tdt(dtype)
    dMp, dMj = up(Mp, np.int32), up(Mj, np.int32)
    Mx = torch.ones(nnz, dtype=t).cuda()
    X, Y = torch.ones((m, ld), dtype=t).cuda(), torch.ones((n + nnz, ld), dtype=t).cuda()
    Z = torch.full((nnz + PAD,), SENTINEL, dtype=t).cuda()
    torch.cuda.synchronize()

    def call(m=m, n=n, nnz=nnz, Mx=Mx, Mp=dMp, Mj=dMj, k=k, X=X, ldX=ld, Y=Y, ldY=ld, Z=Z, flags=_lib.BHS_SDDMM_TIMES_M):
        return dense.csr_sddmm_raw_device(bh, m, n, nnz, Mx, Mp, Mj, k, 1.0, X, ldX, Y, ldY, 1.0, Z, flags)

    refused = {
        "negative size": (call(m=-1), call(n=-1), call(nnz=-1)),
        "k < 1": (call(k=0), call(k=-3)),
        "ldX < k": (call(ldX=k - 1),),
        "ldY < k": (call(ldY=k - 1),),
        "NULL rowPtrM": (call(Mp=None),),
        "NULL colIndM": (call(Mj=None),),
        "NULL X": (call(X=None),),
        "NULL Y": (call(Y=None),),
        "NULL valZ": (call(Z=None),),
        "NULL valM under TIMES_M": (call(Mx=None),),
        "unknown flag bits": (call(flags=2), call(flags=3), call(flags=0x80000000)),
        "valZ overlaps an input": (call(Z=X.view(-1)), call(Z=Y.view(-1)), call(Z=Mx[1:]), call(Mx=Z[1:]), call(X=Z), call(Y=Z[nnz - 1:]),
                                   call(Mp=Z.view(torch.int32)), call(Mj=Z.view(torch.int32))),
    }
    assert sorted(refused) == sorted(sd.HOST_REFUSALS)
    words = {
        "negative size": sd.invalid(-1, n, Mp, Mj, k), "k < 1": sd.invalid(m, n, Mp, Mj, 0), "ldX < k": sd.invalid(m, n, Mp, Mj, k, ldX=k - 1),
        "ldY < k": sd.invalid(m, n, Mp, Mj, k, ldY=k - 1), "NULL rowPtrM": sd.invalid(m, n, None, Mj, k),
        "NULL colIndM": sd.invalid(m, n, Mp, None, k, nnz=nnz),
        "NULL X": sd.invalid(m, n, Mp, Mj, k, has_x=False), "NULL Y": sd.invalid(m, n, Mp, Mj, k, has_y=False),
        "NULL valZ": sd.invalid(m, n, Mp, Mj, k, has_z=False),
        "NULL valM under TIMES_M": sd.invalid(m, n, Mp, Mj, k, flags=1, has_valm=False),
        "unknown flag bits": sd.invalid(m, n, Mp, Mj, k, flags=2), "valZ overlaps an input": sd.invalid(m, n, Mp, Mj, k, overlap=True),
    }
    for word, codes in refused.items():
        assert words[word] == word, (word, words[word])
        assert all(c == INV for c in codes), (word, codes)
    assert bool((Z == SENTINEL).all()), "Z written by a refused call"
    assert sd.invalid(m, n, Mp, Mj, k, flags=0, has_valm=False) is None and call(Mx=None, flags=0) == 0   # (no values without TIMES_M)
    assert bool((Z[nnz:] == SENTINEL).all())


def test_refused_between_symbolic_and_finish():
    m, n, (Mp, Mj), _ = bad_patterns()
    k = 3
    X, Y = np.ones((m, k)), np.ones((n, k))
    sq = (np.arange(n + 1), np.arange(n), np.ones(n))                # the identity, as A and B of a multiply
    dA = (up(sq[0], np.int32), up(sq[1], np.int32), up(sq[2], np.float64))
    bh = new_handle()
    try:
        assert bh.initData_device(n, n, n, n, dA[2], dA[0], dA[1], n, dA[2], dA[0], dA[1]) == 0
        assert bh.spgemm_symbolic() == 0
        run(bh, np.float64, m, n, (Mp, Mj, None), X, Y, want=INV)
        assert bh.spgemm_numeric(0, n) == 0 and bh.spgemm_finish() == 0
        got = run(bh, np.float64, m, n, (Mp, Mj, None), X, Y, check_families=False)
        assert np.array_equal(got, np.full(len(Mj), float(k)))
        bh.free_mem()
    finally:
        bh.freePlatform()


# ---------------------------------------------------------------- the handle is left as it was
@pytest.mark.parametrize("dtype", DTYPES)
def test_the_call_leaves_the_last_multiply_alone(dtype):
    from helpers import random_csr
    mm = 300
    Ap, Aj, Ax = random_csr(mm, mm, 0.03, np.random.default_rng(31))
    Ap, Aj, Ax = np.ascontiguousarray(Ap, np.int32), np.ascontiguousarray(Aj, np.int32), np.ascontiguousarray(Ax, dtype)
    m, k = 257, 17
    M = edge_matrix(m)
    X, Y = dense_pair(m, k)
    bh = new_handle(dtype)
    try:
        Cp = np.zeros(mm + 1, np.int32)
        assert bh.initData(mm, mm, mm, len(Aj), Ax, Ap, Aj, len(Aj), Ax, Ap, Aj, Cp) == 0
        assert bh.spgemm() == 0
        nnzC, ptrs = bh.get_nnzC(), bh.get_C_device()
        Cj, Cx = np.empty(nnzC, np.int32), np.empty(nnzC, dtype)
        assert bh.get_C(Cj, Cx) == 0 and nnzC > 0
        agree(run(bh, dtype, m, N, M, X, Y, gap=1), sd.sddmm(m, N, M[0], M[1], None, X, Y, dtype=dtype), "beside a multiply")
        assert bh.get_nnzC() == nnzC and bh.get_C_device() == ptrs
        j2, x2 = np.empty(nnzC, np.int32), np.empty(nnzC, dtype)
        assert bh.get_C(j2, x2) == 0
        assert np.array_equal(j2, Cj) and np.array_equal(bits(x2), bits(Cx)) and np.array_equal(bh.get_rowptrC(), Cp)
        # C itself as the pattern, straight from the device pointers: the row sums of X Y^T .* C
        dX, dY = up(np.ones((mm, 2)), dtype), up(np.full((mm, 2), 0.5), dtype)
        Z = torch.full((nnzC + PAD,), SENTINEL, dtype=tdt(dtype)).cuda()
        torch.cuda.synchronize()
        assert dense.csr_sddmm_raw_device(bh, mm, mm, nnzC, ptrs[2], ptrs[0], ptrs[1], 2, 1.0, dX, 2, dY, 2, 0.0, Z,
                                          _lib.BHS_SDDMM_TIMES_M) == 0
        assert np.array_equal(Z[:nnzC].cpu().numpy(), Cx) and bool((Z[nnzC:] == SENTINEL).all())
        bh.free_mem()
    finally:
        bh.freePlatform()


# ---------------------------------------------------------------- the tensor call and the convenience
@pytest.mark.parametrize("dtype", DTYPES)
def test_tensor_call_and_convenience(dtype):
    m, k = 257, 5
    Mp, Mj, Mx = edge_matrix(m)
    X, Y = dense_pair(m, k)
    ref = sd.sddmm(m, N, Mp, Mj, Mx, X, Y, -0.5, 0.0, None, True, dtype)
    dM = (up(Mp, np.int32), up(Mj, np.int32), up(Mx, dtype))
    wideX, wideY = up(np.full((m, k + 3), np.nan), dtype), up(np.full((N, k + 2), np.nan), dtype)
    wideX[:, :k], wideY[:, :k] = up(X, dtype), up(Y, dtype)
    bh = new_handle(dtype)
    try:
        Z = dense.csr_sddmm_device(bh, m, N, dM, wideX[:, :k], wideY[:, :k], alpha=-0.5, times_m=True)   # (the stride is the leading dimension)
        agree(Z.cpu().numpy(), ref, "tensor call")
        assert bh.sddmm_ms >= 0.0 and Z.dtype == tdt(dtype) and Z.shape == (len(Mj),)
        with pytest.raises(ValueError):
            dense.csr_sddmm_device(bh, m, N, dM, wideX[:, :k], wideY[:, :k + 1])
    finally:
        bh.freePlatform()
    got, info = dense.sddmm_csr(m, N, Mp, Mj, Mx, X, Y, alpha=-0.5, times_m=True, value_dtype=dtype)
    agree(got, ref, "convenience")
    assert {s["name"] for s in info["kernels"] if s["launches"] > 0} == expected_families(Mp) and info["ms"] >= 0.0


# ---------------------------------------------------------------- affinity strength of connection
@pytest.mark.parametrize("scaled", (False, True), ids=("aniso", "D.A.D"))
def test_affinity_strength_finds_the_x_neighbours(hd, scaled):
    bh, dtype = hd
    nx = ny = 32
    n = nx * ny
    A = matchref.aniso(nx, ny, 1.0 / 64)
    if scaled:
        A = sd.scaled(A)
    dA = (up(A.indptr, np.int32), up(A.indices, np.int32), up(A.data, dtype))
    for seed in (0, 5, 15):
        Sp, Sj = amg.affinity_strength_device(bh, n, dA, theta=0.5, vectors=16, sweeps=8, omega=2.0 / 3.0, seed=seed)
        Sp, Sj = Sp.cpu().numpy(), Sj.cpu().numpy()
        share = sd.not_x_neighbours(Sp, Sj, nx, ny)
        print("affinity %s seed %d: %.4f of the rows keep another set" % ("D.A.D" if scaled else "aniso", seed, share))
        assert share <= 0.05, (seed, share)
        # symmetric, a full diagonal, strictly ascending rows
        import scipy.sparse as sp
        S = sp.csr_matrix((np.ones(len(Sj)), Sj, Sp), shape=(n, n))
        assert Sp[0] == 0 and Sp[-1] == len(Sj) and (S != S.T).nnz == 0 and np.all(S.diagonal() == 1)
        for i in range(n):
            assert np.all(np.diff(Sj[Sp[i]:Sp[i + 1]]) > 0), i
        assert bh.affinity_ms >= 0.0
    agg, nagg, roots = amg.aggregate_device(bh, n, (up(Sp, np.int32), up(Sj, np.int32)), seed=0)[:3]
    assert 0 < int(nagg) < n


# ---------------------------------------------------------------- the demo
def test_cpp_demo_runs():
    demo_dir = os.path.join(ROOT, "tests", "sddmm")
    subprocess.check_call(["make", "-C", demo_dir, "-s"])
    out = subprocess.run([os.path.join(demo_dir, "sddmm_demo")], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "sddmm 5 x 7, 52 entries, k = 5: PASS" in out.stdout
