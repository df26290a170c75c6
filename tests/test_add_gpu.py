"""C = alpha A·B + beta D (bhs_spgemm_add[_device]) and the stand-alone sparse add (bhs_csr_add_*_device) on the GPU.

References.  The stand-alone add: numpy on keys row·n + col (np_add below).  bhs_spgemm_add: the oracle on the augmented
operands A' = [alpha·A, beta·I] (m x (k+m)), B' = [B; D] -- oracle.spgemm(m, k+m, n, A', B') has exactly the wanted pattern
(the union, explicit zeros kept) and values.  rowPtrC / colIndC are compared bit for bit; integer values bit for bit too."""
import os
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN, ROOT
from helpers import check_csr_invariants, poisson_case, random_csr, real_values, wide_values
import valuecheck

from benchmark_spgemm_using_csr_amd import _lib, gallery
from benchmark_spgemm_using_csr_amd.facade import (BHSPARSE_HIP, NUM_PLATFORMS, BhsparseError, bhsparse, csr_add,
                                                   spgemm_add_csr)

pytestmark = pytest.mark.gpu

FILL = ("add_short", "add_wave", "add_long")
INT_COEFFS = ((1, 1), (1, -1), (2, 1), (-1, 2), (1, 0), (0, 1), (2, -1))


# ---------------------------------------------------------------- reference side
def rows_of(p):
    return np.repeat(np.arange(len(p) - 1, dtype=np.int64), np.diff(np.asarray(p, np.int64)))


def np_add(m, n, alpha, X, beta, Y):
    """Z = alpha X + beta Y with the union of the patterns.  Returns (Zp, Zj, Zx float64, mag) with mag = |alpha x| + |beta y|."""
    (Xp, Xj, Xx), (Yp, Yj, Yx) = X, Y
    kx = rows_of(Xp) * n + np.asarray(Xj, np.int64)
    ky = rows_of(Yp) * n + np.asarray(Yj, np.int64)
    kz = np.union1d(kx, ky)
    ax = np.zeros(len(kz))
    by = np.zeros(len(kz))
    inx = np.zeros(len(kz), bool)
    iny = np.zeros(len(kz), bool)
    px, py = np.searchsorted(kz, kx), np.searchsorted(kz, ky)
    ax[px] = alpha * np.asarray(Xx, np.float64)
    by[py] = beta * np.asarray(Yx, np.float64)
    inx[px] = True
    iny[py] = True
    Zx = np.where(inx & iny, ax + by, np.where(inx, ax, by))
    r = kz // max(n, 1)
    Zp = np.zeros(m + 1, np.int64)
    np.cumsum(np.bincount(r, minlength=m)[:m] if m else np.zeros(0, np.int64), out=Zp[1:])
    return Zp.astype(np.int32), (kz - r * n).astype(np.int32), Zx, np.abs(ax) + np.abs(by)


def augmented(m, k, A, B, D, alpha, beta):
    """A' = [alpha A, beta I], B' = [B; D]."""
    (Ap, Aj, Ax), (Bp, Bj, Bx), (Dp, Dj, Dx) = A, B, D
    Ap64 = np.asarray(Ap, np.int64)
    r = rows_of(Ap)
    order = np.argsort(np.concatenate((r, np.arange(m, dtype=np.int64))), kind="stable")   # row i: A's entries, then column k + i
    Aj2 = np.concatenate((np.asarray(Aj, np.int64), k + np.arange(m, dtype=np.int64)))[order].astype(np.int32)
    Ax2 = np.concatenate((alpha * np.asarray(Ax, np.float64), np.full(m, float(beta))))[order]
    Ap2 = (Ap64 + np.arange(m + 1)).astype(np.int32)
    Bp2 = np.concatenate((np.asarray(Bp, np.int64), Bp[-1] + np.asarray(Dp, np.int64)[1:])).astype(np.int32)
    Bj2 = np.concatenate((Bj, Dj)).astype(np.int32)
    Bx2 = np.concatenate((np.asarray(Bx, np.float64), np.asarray(Dx, np.float64)))
    return (Ap2, Aj2, Ax2), (Bp2, Bj2, Bx2)


def reference(oracle, m, k, n, A, B, D, alpha, beta):
    A2, B2 = augmented(m, k, A, B, D, alpha, beta)
    return oracle.spgemm(m, k + m, n, *A2, *B2)


def pattern_with_extras(rng, m, n, inside, frac_in=0.5, extra_per_row=3, empty_rows=(), values="int"):
    """Part of the pattern `inside` = (Cp, Cj) plus random entries per row: a D whose rows reach outside A·B."""
    Cp, Cj = inside
    keep = rng.random(len(Cj)) < frac_in
    rr = [rows_of(Cp)[keep]]
    cc = [np.asarray(Cj, np.int64)[keep]]
    if n > 0 and extra_per_row:
        r = np.repeat(np.arange(m), extra_per_row)
        rr.append(r)
        cc.append(rng.integers(0, n, len(r)))
    rr, cc = np.concatenate(rr).astype(np.int64), np.concatenate(cc).astype(np.int64)
    for e in empty_rows:
        sel = rr != e
        rr, cc = rr[sel], cc[sel]
    Dp, Dj = gallery._csr_from_pairs(m, n, rr, cc)
    return Dp, Dj, int_values(rng, len(Dj), values)


def int_values(rng, count, kind="int"):
    if kind == "signed":
        v = rng.integers(-4, 5, count).astype(np.float64)
        v[v == 0] = 1.0
        return v
    return rng.integers(1, 10, count).astype(np.float64)


# ---------------------------------------------------------------- device side
def new_handle(dtype=np.float64, options=None):
    plats = [False] * NUM_PLATFORMS
    plats[BHSPARSE_HIP] = True
    bh = bhsparse(value_dtype=dtype)
    assert bh.initPlatform(plats) == 0
    for key, val in (options or {}).items():
        assert bh.set_option(key, val) == 0, key
    return bh


def bind(bh, m, k, n, A, B, dtype=np.float64):
    Ap, Aj, Ax = A
    Bp, Bj, Bx = B
    arrs = [np.ascontiguousarray(x, t) for x, t in ((Ax, dtype), (Ap, np.int32), (Aj, np.int32),
                                                    (Bx, dtype), (Bp, np.int32), (Bj, np.int32))]
    Cp = np.zeros(m + 1, np.int32)
    assert bh.initData(m, k, n, len(arrs[2]), arrs[0], arrs[1], arrs[2], len(arrs[5]), arrs[3], arrs[4], arrs[5], Cp) == 0
    return Cp


def result(bh):
    nnz = bh.get_nnzC()
    Cj = np.empty(nnz, np.int32)
    Cx = np.empty(nnz, bh._vdt)
    assert bh.get_C(Cj, Cx) == 0
    return bh._rowptrC.copy(), Cj, Cx


def run_add(bh, alpha, beta, D):
    Dp, Dj, Dx = D
    assert bh.spgemm_add(alpha, beta, Dp, Dj, Dx) == 0
    Cp, Cj, Cx = result(bh)
    assert bh.nnzC == len(Cj) == Cp[-1]
    assert np.array_equal(bh.get_rowptrC(), Cp)
    return Cp, Cj, Cx


def families(bh):
    return {s["name"]: s for s in bh.kernel_stats() if s["launches"]}


def assert_same_pattern(m, n, ref, got):
    assert np.array_equal(np.asarray(got[0], np.int64), np.asarray(ref[0], np.int64)), "rowPtrC differs"
    assert np.array_equal(np.asarray(got[1], np.int32), np.asarray(ref[1], np.int32)), "colIndC differs"
    check_csr_invariants(m, n, np.asarray(got[0]), np.asarray(got[1]))


def assert_exact(m, n, ref, got):
    assert_same_pattern(m, n, ref, got)
    assert np.array_equal(np.asarray(got[2], np.float64), ref[2]), "values differ"


def square(m, rp, col, val):
    return m, m, m, (rp, col, val), (rp, col, val)


# ---------------------------------------------------------------- integer values: D = A, in place and through the second arrays
STENCILS = {
    "p5_16": lambda: square(*poisson_case("poisson5pt", 16, 16)),
    "p27_6": lambda: square(*poisson_case("poisson27pt", 6, 6, 6)),
    "p27_8": lambda: square(*poisson_case("poisson27pt", 8, 8, 8)),
}


@pytest.mark.parametrize("class_path", [2, 0])
@pytest.mark.parametrize("values", ["int", "signed"])
@pytest.mark.parametrize("case", sorted(STENCILS))
def test_product_plus_a_in_place_and_through_second_arrays(case, values, class_path, oracle):
    m, k, n, A, B = STENCILS[case]()
    rng = np.random.default_rng(5)
    if values == "signed":
        A = (A[0], A[1], int_values(rng, len(A[1]), "signed"))
        B = A
    D = (A[0], A[1], int_values(rng, len(A[1]), values))
    got = {}
    for inplace in (1, 0):
        bh = new_handle(options={"class_path": class_path, "add_inplace": inplace})
        try:
            bind(bh, m, k, n, A, B)
            for alpha, beta in INT_COEFFS:
                C = run_add(bh, alpha, beta, D)
                assert bh.get_info("add_inplace_used") == inplace
                fam = families(bh)
                adds = {nm for nm in fam if nm.startswith("add_")}
                if inplace:
                    assert adds <= {"add_count", "add_inplace"} and "add_inplace" in adds, adds
                else:
                    assert "add_count" in adds and "add_scan" in adds and adds & set(FILL), adds
                assert any(not nm.startswith("add_") for nm in fam), fam       # beside the multiply's families, not instead
                assert bh.add_ms > 0
                got[(inplace, alpha, beta)] = C
        finally:
            bh.freePlatform()
    for alpha, beta in INT_COEFFS:
        ref = reference(oracle, m, k, n, A, B, D, alpha, beta)
        assert_exact(m, n, ref, got[(1, alpha, beta)])
        assert_exact(m, n, ref, got[(0, alpha, beta)])
    if values == "signed":
        assert np.count_nonzero(got[(1, 1, -1)][2] == 0) + np.count_nonzero(got[(1, 1, 1)][2] == 0) > 0   # sums that cancel stay


# ---------------------------------------------------------------- integer values: rows that grow, empty rows, edge cases
def _rect(oracle, values="int"):
    rng = np.random.default_rng(7)
    m, k, n = 300, 200, 250
    A = random_csr(m, k, 0.03, rng, empty_rows=(0, 5, 77), values=values)
    B = random_csr(k, n, 0.04, rng, empty_rows=(3,), values=values)
    Cp, Cj, _ = oracle.spgemm(m, k, n, *A, *B)
    D = pattern_with_extras(rng, m, n, (Cp, Cj), 0.5, 3, empty_rows=(5, 6, 200), values=values)   # row 5: empty in A and in D
    return m, k, n, A, B, D


@pytest.mark.parametrize("values", ["int", "signed"])
def test_rows_grow_rectangular(values, oracle):
    m, k, n, A, B, D = _rect(oracle, values)
    nnzAB = int(oracle.spgemm(m, k, n, *A, *B)[0][-1])
    bh = new_handle()
    try:
        bind(bh, m, k, n, A, B)
        for alpha, beta in INT_COEFFS:
            C = run_add(bh, alpha, beta, D)
            assert bh.get_info("add_inplace_used") == 0
            assert_exact(m, n, reference(oracle, m, k, n, A, B, D, alpha, beta), C)
            assert C[0][-1] > nnzAB                                            # the rows grew
    finally:
        bh.freePlatform()


def test_empty_d_and_empty_matrix(oracle):
    rng = np.random.default_rng(9)
    m, k, n = 60, 50, 40
    A = random_csr(m, k, 0.1, rng)
    B = random_csr(k, n, 0.1, rng)
    D0 = (np.zeros(m + 1, np.int32), np.zeros(0, np.int32), np.zeros(0))
    for inplace in (1, 0):
        Cp, Cj, Cx, info = spgemm_add_csr(m, k, n, *A, *B, *D0, alpha=2, beta=1, options={"add_inplace": inplace})
        assert info["add_inplace_used"] == inplace
        assert_exact(m, n, reference(oracle, m, k, n, A, B, D0, 2, 1), (Cp, Cj, Cx))
    z = (np.zeros(1, np.int32), np.zeros(0, np.int32), np.zeros(0))
    Cp, Cj, Cx, info = spgemm_add_csr(0, k, n, *z, *B, *z)
    assert len(Cp) == 1 and Cp[0] == 0 and len(Cj) == 0 and info["nnzC"] == 0
    # an empty product with a D: the sum is D
    Ae = (np.zeros(m + 1, np.int32), np.zeros(0, np.int32), np.zeros(0))
    D = random_csr(m, n, 0.1, rng)
    Cp, Cj, Cx, info = spgemm_add_csr(m, k, n, *Ae, *B, *D, alpha=1, beta=3)
    assert_exact(m, n, reference(oracle, m, k, n, Ae, B, D, 1, 3), (Cp, Cj, Cx))


def _every_bin(oracle):
    """A D whose rows reach every fill bin: one row of 5000 entries, a block of rows with 100-600, the rest short."""
    rng = np.random.default_rng(13)
    m, k, n = 300, 200, 8000
    A = random_csr(m, k, 0.03, rng)
    B = random_csr(k, n, 0.002, rng)
    lens = np.full(m, 3)
    lens[0] = 5000
    lens[10:40] = rng.integers(100, 601, 30)
    Dp = np.zeros(m + 1, np.int32)
    np.cumsum(lens, out=Dp[1:])
    Dj = np.concatenate([np.sort(rng.choice(n, int(ln), replace=False)) for ln in lens]).astype(np.int32)
    return m, k, n, A, B, (Dp, Dj, int_values(rng, len(Dj), "signed"))


def test_every_fill_family_is_reached(oracle):
    m, k, n, A, B, D = _every_bin(oracle)
    Cp, Cj, Cx, info = spgemm_add_csr(m, k, n, *A, *B, *D, alpha=-1, beta=2)
    fam = {s["name"]: s for s in info["kernels"]}
    for name in FILL:
        assert name in fam and fam[name]["launches"] >= 1 and fam[name]["rows"] >= 1, (name, sorted(fam))
    assert fam["add_long"]["rows"] >= 1 and fam["add_wave"]["rows"] >= 30
    assert info["add_inplace_used"] == 0
    assert_exact(m, n, reference(oracle, m, k, n, A, B, D, -1, 2), (Cp, Cj, Cx))


def test_powerlaw_golden_plus_a(oracle):
    z = np.load(os.path.join(GOLDEN, "ref_opencl_powerlaw_3k.npz"))
    A = (z["Ap"], z["Aj"], z["Ax"])
    B = (z["Bp"], z["Bj"], z["Bx"])
    m, k = len(A[0]) - 1, len(B[0]) - 1
    n = m
    assert m == k and int(B[1].max()) < n
    assert np.array_equal(A[2], np.round(A[2])) and np.array_equal(B[2], np.round(B[2]))    # (integer values: bit-exact)
    ref = reference(oracle, m, k, n, A, B, A, 1, -2)
    for inplace in (1, 0):
        Cp, Cj, Cx, info = spgemm_add_csr(m, k, n, *A, *B, *A, alpha=1, beta=-2, options={"add_inplace": inplace})
        assert info["add_inplace_used"] == 0              # (A has entries outside A·B here: rows grow)
        assert_exact(m, n, ref, (Cp, Cj, Cx))


# ---------------------------------------------------------------- the stand-alone add
def _long_pair(rng, m, n, lens_x, lens_y, shared=0.5):
    """X and Y whose row i has lens_x[i] / lens_y[i] entries, about `shared` of Y's entries also in X."""
    Xr, Xc, Yr, Yc = [], [], [], []
    for i in range(m):
        cx = np.sort(rng.choice(n, int(lens_x[i]), replace=False))
        take = cx[rng.random(len(cx)) < shared][: int(lens_y[i])]
        rest = rng.choice(n, max(int(lens_y[i]) - len(take), 0), replace=False)
        cy = np.unique(np.concatenate((take, rest)))
        Xr.append(np.full(len(cx), i)); Xc.append(cx); Yr.append(np.full(len(cy), i)); Yc.append(cy)
    Xp, Xj = gallery._csr_from_pairs(m, n, np.concatenate(Xr), np.concatenate(Xc))
    Yp, Yj = gallery._csr_from_pairs(m, n, np.concatenate(Yr), np.concatenate(Yc))
    return (Xp, Xj, int_values(rng, len(Xj), "signed")), (Yp, Yj, int_values(rng, len(Yj), "signed"))


def _standalone_cases():
    rng = np.random.default_rng(23)
    out = {}
    m, n = 400, 350
    out["dense_sparse"] = (m, n, random_csr(m, n, 0.08, rng, empty_rows=(0, 9)), random_csr(m, n, 0.01, rng, empty_rows=(9, 10)))
    m, n = 40, 6000
    lx = rng.integers(0, 40, m); ly = rng.integers(0, 40, m)
    lx[:4] = (3000, 2500, 5000, 10); ly[:4] = (3500, 2600, 30, 4000)          # long rows on both sides: chunks with pairs at the cuts
    lx[4:12] = rng.integers(100, 600, 8); ly[4:12] = rng.integers(100, 400, 8)
    out["long_rows"] = (m, n) + _long_pair(rng, m, n, lx, ly)
    m, n = 64, 6200                                # rows 0-2 full in X; Y's row 0 lacks column 0 (every cut of the merge falls between an x
    xrows = [np.arange(n) if i < 3 else np.sort(rng.choice(n, 5, replace=False)) for i in range(m)]   # and its equal y), row 1 is full too,
    yrows = [np.arange(1, n), np.arange(n), np.arange(0, n, 3)] + xrows[3:]                            # row 2 holds every third column
    Xp = np.zeros(m + 1, np.int32); Xp[1:] = np.cumsum([len(r) for r in xrows])
    Yp = np.zeros(m + 1, np.int32); Yp[1:] = np.cumsum([len(r) for r in yrows])
    Xj, Yj = np.concatenate(xrows).astype(np.int32), np.concatenate(yrows).astype(np.int32)
    out["full_rows"] = (m, n, (Xp, Xj, int_values(rng, len(Xj))), (Yp, Yj, int_values(rng, len(Yj), "signed")))
    return out


@pytest.mark.parametrize("case", ["dense_sparse", "long_rows", "full_rows"])
def test_standalone_add_on_a_fresh_handle(case):
    m, n, X, Y = _standalone_cases()[case]
    for alpha, beta in ((1, 1), (2, -1), (0, 1), (1, 0), (0.75, -1.5)):
        Zp, Zj, Zx, info = csr_add(m, n, alpha, *X, beta, *Y)
        rp, rj, rx, _ = np_add(m, n, alpha, X, beta, Y)
        assert_exact(m, n, (rp, rj, rx), (Zp, Zj, Zx))                        # (integer values, dyadic coefficients: exact)
        inside = int(np.array_equal(rp, X[0]))
        assert info["y_inside_x"] == inside
        fam = {s["name"] for s in info["kernels"]}
        assert "add_bin" in fam and fam & set(FILL) and all(nm.startswith("add_") for nm in fam), fam
        assert info["ms"] > 0
    if case == "long_rows":
        assert "add_long" in fam and "add_wave" in fam and "add_short" in fam


def test_standalone_y_inside_x_and_chaining():
    import torch
    rng = np.random.default_rng(29)
    m, n = 500, 450
    X = random_csr(m, n, 0.05, rng)
    keep = rng.random(len(X[1])) < 0.4
    r = rows_of(X[0])[keep]
    Yp, Yj = gallery._csr_from_pairs(m, n, r, X[1][keep].astype(np.int64))
    Y = (Yp, Yj, int_values(rng, len(Yj), "signed"))
    W = random_csr(m, n, 0.02, rng, values="signed")
    dev = torch.device("cuda")
    up = lambda M: (torch.from_numpy(np.ascontiguousarray(M[0], np.int32)).to(dev),          # noqa: E731
                    torch.from_numpy(np.ascontiguousarray(M[1], np.int32)).to(dev),
                    torch.from_numpy(np.ascontiguousarray(M[2], np.float64)).to(dev))
    bh = new_handle()                                                         # (no data is ever bound)
    try:
        dX, dY, dW = up(X), up(Y), up(W)
        Zp, Zj, Zx, inside = bh.csr_add_device(m, n, 1, dX, 3, dY)
        assert inside == 1 and np.array_equal(Zp.cpu().numpy(), X[0])
        ref1 = np_add(m, n, 1, X, 3, Y)
        assert_exact(m, n, ref1[:3], (Zp.cpu().numpy(), Zj.cpu().numpy(), Zx.cpu().numpy()))
        Z2p, Z2j, Z2x, inside2 = bh.csr_add_device(m, n, 2, (Zp, Zj, Zx), -1, dW)           # the result as X of a second add
        assert inside2 == 0
        ref2 = np_add(m, n, 2, ref1[:3], -1, W)
        assert_exact(m, n, ref2[:3], (Z2p.cpu().numpy(), Z2j.cpu().numpy(), Z2x.cpu().numpy()))
        Z3p, _, _, inside3 = bh.csr_add_device(m, n, 1, dY, 1, dX)                          # X inside Y is not Y inside X
        assert inside3 == 0 and np.array_equal(Z3p.cpu().numpy(), X[0])
    finally:
        bh.freePlatform()


# ---------------------------------------------------------------- invalid input
def _bad_versions(m, n, P, J):
    i = int(np.argmax(np.diff(P) >= 2))
    s = P[i]
    unsorted = J.copy()
    unsorted[s], unsorted[s + 1] = unsorted[s + 1], unsorted[s]
    dup = J.copy()
    dup[s + 1] = dup[s]
    big = J.copy()
    big[-1] = n
    nonmono = P.copy()
    nonmono[m // 2] = nonmono[m // 2 + 1] + 1
    return {"unsorted_row": (P, unsorted, len(J)), "duplicate": (P, dup, len(J)), "column_eq_n": (P, big, len(J)),
            "wrong_nnz": (P, J, len(J) - 1), "decreasing_rowptr": (nonmono, J, len(J))}


def test_invalid_x_and_y_are_rejected_and_nothing_is_written():
    import torch
    rng = np.random.default_rng(31)
    m, n = 200, 180
    X = random_csr(m, n, 0.05, rng)
    Y = random_csr(m, n, 0.05, rng)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.int32)).cuda()                # noqa: E731
    bh = new_handle()
    try:
        good = (t(X[0]), t(X[1]), len(X[1])), (t(Y[0]), t(Y[1]), len(Y[1]))
        for side in (0, 1):
            src = (X, Y)[side]
            for name, (p, j, nnz) in _bad_versions(m, n, src[0], src[1]).items():
                ops = list(good)
                ops[side] = (t(p), t(j), nnz)
                Zp = torch.full((m + 1,), -77, dtype=torch.int32, device="cuda")
                torch.cuda.synchronize()
                err, _, _ = bh.csr_add_symbolic_device(m, n, ops[0][2], ops[0][0], ops[0][1], ops[1][2], ops[1][0], ops[1][1], Zp)
                assert err == _lib.BHS_ERR_INVALID_ARG, (side, name)
                assert torch.all(Zp == -77).item(), (side, name)
        Zp = torch.full((m + 1,), -77, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        err, nnzZ, _ = bh.csr_add_symbolic_device(m, n, good[0][2], good[0][0], good[0][1], good[1][2], good[1][0], good[1][1], Zp)
        assert err == 0 and nnzZ == np_add(m, n, 1, X, 1, Y)[0][-1]             # the handle still works
        # the numeric call refuses a row pointer that cannot belong to these operands, and writes nothing
        Zj = torch.full((nnzZ,), -5, dtype=torch.int32, device="cuda")
        Zx = torch.full((nnzZ,), -5.0, dtype=torch.float64, device="cuda")
        vx, vy = torch.ones(len(X[1]), dtype=torch.float64, device="cuda"), torch.ones(len(Y[1]), dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        err = bh.csr_add_numeric_device(m, n, 1, good[0][2], vx, good[0][0], good[0][1], 1, good[1][2], vy, good[1][0], good[1][1],
                                        good[0][0], Zj, Zx)                    # rowPtrX for rowPtrZ: rows too short
        assert err == _lib.BHS_ERR_INVALID_ARG
        assert torch.all(Zj == -5).item() and torch.all(Zx == -5.0).item()
    finally:
        bh.freePlatform()


def test_invalid_d_is_rejected_before_the_multiply(oracle):
    m, k, n, A, B = square(*poisson_case("poisson5pt", 12, 12))
    bh = new_handle()
    try:
        bind(bh, m, k, n, A, B)
        assert bh.spgemm() == 0
        Cp, Cj, Cx = result(bh)
        for name, (p, j, nnz) in _bad_versions(m, n, A[0], A[1]).items():
            vals = np.ones(len(j))
            err = bh._lib.bhs_spgemm_add(bh._h, 1.0, 1.0, nnz, vals.ctypes.data, np.ascontiguousarray(p, np.int32).ctypes.data,
                                         np.ascontiguousarray(j, np.int32).ctypes.data, None, None, None, None)
            assert err == _lib.BHS_ERR_INVALID_ARG, name
            Cp2, Cj2, Cx2 = result(bh)                                        # the C of the earlier bhs_spgemm
            assert np.array_equal(Cj2, Cj) and np.array_equal(Cx2, Cx) and np.array_equal(bh.get_rowptrC(), Cp), name
        C = run_add(bh, 1, 1, A)                                              # the handle still works
        assert_exact(m, n, reference(oracle, m, k, n, A, B, A, 1, 1), C)
    finally:
        bh.freePlatform()


def test_bound_output_arrays_split_multiply_and_no_data(oracle):
    import torch
    m, k, n, A, B = square(*poisson_case("poisson5pt", 12, 12))
    bh = new_handle()
    try:
        assert bh.spgemm_add(1, 1, *A) == _lib.BHS_ERR_NOT_READY
        bind(bh, m, k, n, A, B)
        assert bh.spgemm_symbolic() == 0
        assert bh.spgemm_add(1, 1, *A) == _lib.BHS_ERR_INVALID_ARG
        Zp = torch.zeros(m + 1, dtype=torch.int32, device="cuda")
        dp, dj = torch.from_numpy(A[0].astype(np.int32)).cuda(), torch.from_numpy(A[1].astype(np.int32)).cuda()
        torch.cuda.synchronize()
        assert bh.csr_add_symbolic_device(m, n, len(A[1]), dp, dj, len(A[1]), dp, dj, Zp)[0] == _lib.BHS_ERR_INVALID_ARG
        assert bh.spgemm_numeric(0, m) == 0 and bh.spgemm_finish() == 0
        cj = torch.zeros(bh.nnzC + 64, dtype=torch.int32, device="cuda")
        cx = torch.zeros(bh.nnzC + 64, dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        assert bh.set_output_device(cj, cx, bh.nnzC + 64) == 0
        assert bh.spgemm_add(1, 1, *A) == _lib.BHS_ERR_INVALID_ARG
        assert bh.set_output_device(None, None, 0) == 0
        C = run_add(bh, 1, 1, A)
        assert_exact(m, n, reference(oracle, m, k, n, A, B, A, 1, 1), C)
    finally:
        bh.freePlatform()


# ---------------------------------------------------------------- the handle's state
def test_spgemm_after_add_and_add_twice(oracle):
    m, k, n, A, B = square(*poisson_case("poisson27pt", 24, 24, 24))
    rng = np.random.default_rng(37)
    AB = oracle.spgemm(m, k, n, *A, *B)
    Dout = pattern_with_extras(rng, m, n, (AB[0], AB[1]), 0.3, 2)
    for D, inplace in ((A, 1), (Dout, 0)):
        bh = new_handle(options={"class_path": 2})
        try:
            bind(bh, m, k, n, A, B)
            ref = reference(oracle, m, k, n, A, B, D, 1, 2)
            first = run_add(bh, 1, 2, D)
            state = bh.get_info("class_state")
            second = run_add(bh, 1, 2, D)                                     # (the class path's second multiply goes out speculatively)
            assert bh.get_info("add_inplace_used") == inplace
            assert bh.get_info("spec_launches") >= 1 and bh.get_info("class_state") == state
            assert_exact(m, n, ref, first)
            assert_exact(m, n, ref, second)
            assert bh.spgemm() == 0                                           # plain A·B again
            assert_exact(m, n, AB, result(bh))
            third = run_add(bh, 1, 2, D)
            assert_exact(m, n, ref, third)
        finally:
            bh.freePlatform()


def test_masked_multiply_leaves_the_sum(oracle):
    m, k, n, A, B, D = _rect(oracle)
    bh = new_handle()
    try:
        bind(bh, m, k, n, A, B)
        C = run_add(bh, 2, 1, D)
        ptrs = bh.get_C_device()
        AB = oracle.spgemm(m, k, n, *A, *B)
        valM = bh.spgemm_masked(AB[0].astype(np.int32), AB[1])
        assert np.array_equal(valM, AB[2])
        C2 = result(bh)
        assert bh.get_C_device() == ptrs
        assert all(np.array_equal(x, y) for x, y in zip(C, C2))
        assert_exact(m, n, reference(oracle, m, k, n, A, B, D, 2, 1), C2)
        assert bh.free_mem() == 0
        assert bh.get_nnzC() == 0
    finally:
        bh.freePlatform()


def test_device_entry(oracle):
    import torch
    m, k, n, A, B, D = _rect(oracle)
    dev = torch.device("cuda")
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dt)).to(dev)   # noqa: E731
    dA = (t(A[2], np.float64), t(A[0], np.int32), t(A[1], np.int32))
    dB = (t(B[2], np.float64), t(B[0], np.int32), t(B[1], np.int32))
    dD = (t(D[2], np.float64), t(D[0], np.int32), t(D[1], np.int32))
    bh = new_handle()
    try:
        assert bh.initData_device(m, k, n, len(A[1]), *dA, len(B[1]), *dB) == 0
        assert bh.spgemm_add_device(-1, 2, len(D[1]), *dD) == 0
        nnz = bh.get_nnzC()
        assert nnz == bh.nnzC
        Cj, Cx = np.empty(nnz, np.int32), np.empty(nnz, np.float64)
        assert bh.get_C(Cj, Cx) == 0
        assert_exact(m, n, reference(oracle, m, k, n, A, B, D, -1, 2), (bh.get_rowptrC(), Cj, Cx))
        assert bh.free_mem() == 0
    finally:
        bh.freePlatform()


# ---------------------------------------------------------------- real values against the derived bound
def _class_mismatch(ref, got):
    for r, g in zip(valuecheck._classes(ref), valuecheck._classes(got)):
        if np.any(r != g):
            return True
    return False


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("kind", ["wide", "cancel"])
@pytest.mark.parametrize("inside", [1, 0])
def test_real_values(inside, kind, dtype, oracle):
    """Bound, derived (not measured).  The sum is fl_out(alpha c~ + beta d): c~ is the multiply's entry, within
    b = valuecheck.bound(mode, ref_AB, S, K) of the exact (A·B)(i, j) (mode "f64"; "f32_atomic" for the float build, the
    looser of the two float modes: the add does not care which family produced c~), and |c~| <= S up to the same gamma.
    alpha and beta are powers of two, so alpha c~ and beta d are exact; their sum is formed in double (one rounding, or
    one fused rounding: u = 2^-53) and rounded once to the output format (u_out = 2^-53 or 2^-24).  The oracle's own sum of
    the augmented product carries up to two more roundings of the same two terms.  Hence
        |got - ref| <= |alpha| b + (u_out + 3·2^-53) (|alpha| S + |beta d|).
    Stand-alone add (any real alpha, beta): (u_out + 3·2^-53) (|alpha x| + |beta y|) -- two products, one sum, one
    rounding to the output format.  Non-finite entries must match the reference in class."""
    f32 = dtype == np.float32
    mode = "f32_atomic" if f32 else "f64"
    u_out = 2.0 ** -24 if f32 else 2.0 ** -53
    rng = np.random.default_rng(41 + inside)
    m, k0, n = 350, 300, 320
    A0 = random_csr(m, k0, 0.03, rng)
    B0 = random_csr(k0, n, 0.03, rng)
    k, A, B = real_values(kind, k0, A0, B0, rng, f32=f32)
    AB = oracle.spgemm(m, k, n, A[0], A[1], np.ones(len(A[1])), B[0], B[1], np.ones(len(B[1])))
    if inside:
        keep = rng.random(len(AB[1])) < 0.5
        Dp, Dj = gallery._csr_from_pairs(m, n, rows_of(AB[0])[keep], AB[1][keep].astype(np.int64))
    else:
        Dp, Dj, _ = pattern_with_extras(rng, m, n, (AB[0], AB[1]), 0.5, 3)
    Dx = wide_values(len(Dj), rng)
    rnd = (lambda x: np.asarray(x, np.float32).astype(np.float64)) if f32 else (lambda x: np.asarray(x, np.float64))
    A, B, D = (A[0], A[1], rnd(A[2])), (B[0], B[1], rnd(B[2])), (Dp, Dj, rnd(Dx))
    for alpha, beta in ((1.0, 1.0), (0.5, -4.0)):
        for planted in (False, True):
            Ax, Dxp = A[2].copy(), D[2].copy()
            if planted:
                Ax[len(Ax) // 3] = np.nan
                Dxp[len(Dxp) // 4] = np.inf
                Dxp[len(Dxp) // 2] = np.nan
            Ap_, Dp_ = (A[0], A[1], Ax), (D[0], D[1], Dxp)
            with np.errstate(invalid="ignore"):
                ref = reference(oracle, m, k, n, Ap_, B, Dp_, alpha, beta)
                r, S, K = valuecheck.references(oracle, m, k, n, Ap_, B, mode)
            Cp, Cj, Cx, info = spgemm_add_csr(m, k, n, *Ap_, *B, *Dp_, alpha=alpha, beta=beta, value_dtype=dtype)
            assert info["add_inplace_used"] == inside
            assert Cx.dtype == dtype
            assert_same_pattern(m, n, ref, (Cp, Cj, Cx))
            pat = lambda x: valuecheck.on_pattern((r[0], r[1], x), n, ref[0], ref[1])   # noqa: E731
            rv, Sv, Kv = pat(r[2]), pat(S), pat(K)
            d = valuecheck.on_pattern(Dp_, n, ref[0], ref[1])
            got = np.asarray(Cx, np.float64)
            assert not _class_mismatch(ref[2], got), "non-finite entries differ in class"
            fin = np.isfinite(ref[2])
            assert planted == (not np.all(fin))
            with np.errstate(invalid="ignore"):
                lim = abs(alpha) * valuecheck.bound(mode, rv, Sv, Kv) + (u_out + 3 * 2.0 ** -53) * (abs(alpha) * Sv + np.abs(beta * d))
                err = np.abs(got - ref[2])
            worst = float(np.max(err[fin] / np.maximum(lim[fin], 1e-300)))
            print("real %s %s inside=%d alpha=%g planted=%d: worst err/bound %.3g" % (kind, mode, inside, alpha, planted, worst))
            assert np.all(err[fin] <= lim[fin]), worst


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_standalone_real_values(dtype):
    f32 = dtype == np.float32
    u_out = 2.0 ** -24 if f32 else 2.0 ** -53
    rng = np.random.default_rng(43)
    m, n = 600, 500
    X = random_csr(m, n, 0.04, rng)
    Y = random_csr(m, n, 0.03, rng)
    rnd = (lambda x: np.asarray(x, np.float32).astype(np.float64)) if f32 else (lambda x: x)
    X = (X[0], X[1], rnd(wide_values(len(X[1]), rng)))
    Y = (Y[0], Y[1], rnd(wide_values(len(Y[1]), rng)))
    Y[2][len(Y[2]) // 2] = np.inf
    X[2][len(X[2]) // 3] = np.nan
    for alpha, beta in ((1.0, 1.0), (0.3, -1.7), (-2.5e-3, 7.1e2)):
        Zp, Zj, Zx, _ = csr_add(m, n, alpha, *X, beta, *Y, value_dtype=dtype)
        with np.errstate(invalid="ignore"):
            rp, rj, rx, mag = np_add(m, n, alpha, X, beta, Y)
        assert Zx.dtype == dtype
        assert_same_pattern(m, n, (rp, rj, rx), (Zp, Zj, Zx))
        got = np.asarray(Zx, np.float64)
        assert not _class_mismatch(rx, got)
        fin = np.isfinite(rx)
        assert not np.all(fin)
        err = np.abs(got[fin] - rx[fin])
        lim = (u_out + 3 * 2.0 ** -53) * mag[fin]
        print("stand-alone real %s alpha=%g: worst err/bound %.3g" % (np.dtype(dtype).name, alpha, float(np.max(err / np.maximum(lim, 1e-300)))))
        assert np.all(err <= lim)


def test_f32_integer_values_exact(oracle):
    m, k, n, A, B = square(*poisson_case("poisson27pt", 6, 6, 6))
    for inplace in (1, 0):
        Cp, Cj, Cx, info = spgemm_add_csr(m, k, n, *A, *B, *A, alpha=2, beta=-1, options={"add_inplace": inplace},
                                          value_dtype=np.float32)
        assert Cx.dtype == np.float32 and info["add_inplace_used"] == inplace
        assert_exact(m, n, reference(oracle, m, k, n, A, B, A, 2, -1), (Cp, Cj, Cx))


# ---------------------------------------------------------------- the C++ facade's extension
def test_cpp_facade_add_demo():
    demo_dir = os.path.join(ROOT, "tests", "add")
    subprocess.check_call(["make", "-C", demo_dir, "-s"])
    r = subprocess.run([os.path.join(demo_dir, "add_demo")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "add OK" in r.stdout and "nnz(C) = " in r.stdout
