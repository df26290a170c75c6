"""Shared helpers for the parity tests (test infrastructure)."""
import numpy as np

from benchmark_spgemm_using_csr_amd import gallery


def poisson_case(name, nx, ny, nz=1):
    rp, col = gallery.poisson_csr(name, nx, ny, nz)
    val = gallery.fill_values(len(col))
    m = len(rp) - 1
    return m, rp, col, val


def random_csr(m, n, density, rng, empty_rows=(), values="int", max_row=None):
    """Random CSR with sorted duplicate-free rows."""
    lens = rng.binomial(n, density, size=m)
    if max_row is not None:
        lens = np.minimum(lens, max_row)
    for r in empty_rows:
        if r < m:
            lens[r] = 0
    rp = np.zeros(m + 1, np.int64)
    np.cumsum(lens, out=rp[1:])
    cols = np.empty(rp[-1], np.int32)
    for i in range(m):
        cols[rp[i]:rp[i + 1]] = np.sort(rng.choice(n, lens[i], replace=False))
    if values == "int":
        val = rng.integers(1, 10, rp[-1]).astype(np.float64)
    elif values == "signed":
        val = rng.integers(-4, 5, rp[-1]).astype(np.float64)
        val[val == 0] = 1.0
    else:
        val = rng.standard_normal(rp[-1])
    return rp.astype(np.int32), cols, val


VALUE_KINDS = ("wide", "cancel")


def wide_values(count, rng):
    """sign x (1 + U[0,1)) x 2^U{-20..20}: real values over twelve decades, no product or sum near under- or overflow."""
    sign = np.where(rng.random(count) < 0.5, -1.0, 1.0)
    return sign * (1.0 + rng.random(count)) * np.exp2(rng.integers(-20, 21, count).astype(np.float64))


def real_values(kind, k, A, B, rng, f32=False):
    """The pattern of A (m x k) and B (k x n) with real values.  Returns (k', A', B'), A' B' of the same m x n shape.
    "wide": wide_values on A and B as they are.
    "cancel": A' = [A A], B' = [B; -B o (1 + eps r)], r in U[0,1), so that C' = -eps A (B o r): most entries of C'
    are eps times the sum of their products' magnitudes.  eps = 2^-30, or 2^-12 for the float build (a 2^-30
    perturbation vanishes when the inputs are rounded to float).  Every row of A' holds A's row twice, every product
    of A B lands twice."""
    Ap, Aj, _ = A
    Bp, Bj, _ = B
    Ap, Bp = np.asarray(Ap, np.int64), np.asarray(Bp, np.int64)
    Ax, Bx = wide_values(len(Aj), rng), wide_values(len(Bj), rng)
    if kind == "wide":
        return k, (A[0], A[1], Ax), (B[0], B[1], Bx)
    assert kind == "cancel", kind
    eps = 2.0 ** -12 if f32 else 2.0 ** -30
    rows = np.repeat(np.arange(len(Ap) - 1), np.diff(Ap))
    o = np.argsort(np.concatenate((rows, rows)), kind="stable")           # row i: its entries, then the same + k
    Aj2 = np.concatenate((Aj, np.asarray(Aj) + k)).astype(np.int32)[o]
    Ax2 = np.concatenate((Ax, Ax))[o]
    Ap2 = (2 * Ap).astype(np.int32)
    Bp2 = np.concatenate((Bp, Bp[-1] + Bp[1:])).astype(np.int32)
    Bj2 = np.concatenate((Bj, Bj)).astype(np.int32)
    Bx2 = np.concatenate((Bx, -Bx * (1.0 + eps * rng.random(len(Bx)))))
    return 2 * k, (Ap2, Aj2, Ax2), (Bp2, Bj2, Bx2)


def check_csr_invariants(m, n, Cp, Cj):
    """Output postconditions of SURVEY.md §8b: rowPtr monotone from 0, rows strictly ascending."""
    assert Cp[0] == 0 and np.all(np.diff(Cp) >= 0)
    if len(Cj):
        assert Cj.min() >= 0 and Cj.max() < n
        d = np.diff(Cj.astype(np.int64))
        starts = np.zeros(len(Cj), bool)
        starts[Cp[1:-1][Cp[1:-1] < len(Cj)]] = True
        assert np.all((d > 0) | starts[1:]), "rows must be strictly ascending by column"
