"""bhs_csr_relax_device, bhs_chebyshev_coefficients and the reductions of bhs_csr_spmv_dots_device of
include/bhsparse_hip.h ("relaxation and fused products") restated in numpy: the reference of their tests.

A step: inputs rounded to the build's value type, everything after that float64 -- sum_i the row's products as
tests/spmvref.py sums them (the correctly rounded sum), r = b - sum, q = r / diag, dn = c q, dn = dn + a d only where
a != 0, d <- round(dn), x <- round(x + dn).  relax() also returns, for its LAST step, S = |x| + |c / diag| (|b| + |A| |x|)
+ |a d| and K = entries of the row + 5 (the products' additions, the subtraction from b, the division, the scaling by c,
the addition of a d, the addition to x): what tests/valuecheck.py bounds the error of any summation order with."""
import numpy as np

import spmvref as sr

ZERO_GUESS = 1


def chebyshev_coefficients(lmin, lmax, steps):
    """(steps, 2) float64: Saad, Iterative Methods for Sparse Linear Systems, Algorithm 12.1"""
    lmin, lmax = np.float64(lmin), np.float64(lmax)
    theta, delta = (lmax + lmin) / 2, (lmax - lmin) / 2
    sigma = theta / delta
    rho = 1 / sigma
    out = [(0.0, 1 / theta)]
    for _ in range(1, steps):
        nxt = 1 / (2 * sigma - rho)
        out.append((nxt * rho, 2 * nxt / delta))
        rho = nxt
    return np.array(out, np.float64)


def chebyshev_value(s, t):
    """T_s(t) for any real t, float64: the three-term recurrence"""
    t = np.asarray(t, np.float64)
    a, b = np.ones_like(t), t.copy()
    if s == 0:
        return a
    for _ in range(s - 1):
        a, b = b, 2 * t * b - a
    return b


def relax(n, Ap, Aj, Ax, diag, coef, b, x, d=None, zero_guess=False, dtype=np.float64):
    """Returns (x, d, S, K): x and d in `dtype` after len(coef) steps (d None where none is kept); S float64 and K int64 of
    the last step's x.  d None: every a must be 0."""
    r_ = lambda v: np.ascontiguousarray(v, dtype).astype(np.float64)   # noqa: E731
    coef = np.asarray(coef, np.float64).reshape(-1, 2)
    diag, b = r_(diag), r_(b)
    x = np.zeros(n) if zero_guess else r_(x)
    keep = d is not None
    d = r_(d) if keep else None
    assert keep or not coef[:, 0].any()
    a_ = np.ones(len(Aj)) if Ax is None else r_(Ax)
    S, K = np.zeros(n), np.zeros(n, np.int64)
    with np.errstate(all="ignore"):
        for s, (a, c) in enumerate(coef):
            if s == 0 and zero_guess:
                total, St = np.zeros(n), np.zeros(n)
            else:
                total, St, _ = sr.spmv(n, n, Ap, Aj, a_, x, dtype=np.float64)
            q = (b - total) / diag
            dn = c * q
            S = np.abs(x) + np.abs(c / diag) * (np.abs(b) + St)
            if a != 0.0:
                dn = dn + a * d
                S = S + np.abs(a * d)
            if keep:
                d = r_(dn.astype(dtype))
            x = r_((x + dn).astype(dtype))
        S = np.where(np.isnan(S), np.inf, S)
        K = (np.diff(np.asarray(Ap, np.int64)) + 5).astype(np.int64)
    return x.astype(dtype), (d.astype(dtype) if keep else None), S, K


def dots(z, w=None):
    """(zz, wz, Szz, Swz): the sums in float64 (math.fsum's correctly rounded value where finite) and their magnitudes"""
    import math
    z = np.asarray(z).astype(np.float64)
    out = []
    for v in (z * z, None if w is None else np.asarray(w).astype(np.float64) * z):
        if v is None:
            out.append((None, None))
        elif np.isfinite(v).all():
            out.append((math.fsum(v), float(np.abs(v).sum())))
        else:
            with np.errstate(invalid="ignore"):
                out.append((float(v.sum()), np.inf))
    return out[0][0], out[1][0], out[0][1], out[1][1]
