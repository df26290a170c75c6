"""bhs_csr_spmv_device and bhs_csr_spmm_device of include/bhsparse_hip.h ("CSR x dense") restated in numpy: the reference
of their tests.

A is an m x n CSR matrix whose rows need not be ascending and may hold duplicate (row, column) pairs, which add up; X is
n x k, Y m x k.  Inputs are rounded to the build's value type first and everything after that is float64: s = the sum of
double(a) * double(x) over a row's entries from +0 (math.fsum of the products where they are finite: the correctly rounded
sum), t = alpha * s, t = t + beta * y only where beta != 0 (y is then never looked at), one rounding to the value type.
alpha == 0 takes no shortcut.  spmm() also returns S = |alpha| (|A| |X|) + |beta| |Y| and K = entries of the row + 2 (the
products' additions, the scaling by alpha, the addition of beta y): what tests/valuecheck.py bounds the error of any
summation order with."""
import math

import numpy as np

# the arguments bhs_csr_spmm_device refuses on the host (each BHS_ERR_INVALID_ARG, y untouched), by the word invalid() gives
HOST_REFUSALS = ("negative size", "k < 1", "ldX < k", "ldY < k", "NULL rowPtrA", "NULL colIndA", "NULL x", "NULL y",
                 "y overlaps an input")
# what the device's validation refuses
DEVICE_REFUSALS = ("rowPtrA[0] != 0", "rowPtrA[m] != nnzA", "decreasing rowPtrA", "column of A out of range")


def invalid(m, n, Ap, Aj, k=1, ldX=None, ldY=None, has_x=True, has_y=True, overlap=False):
    """What the calls must refuse: a word for the first reason found (one of HOST_REFUSALS, then DEVICE_REFUSALS), or None
    for a legal call.  Ap / Aj None stand for NULL pointers; nnzA is len(Aj)."""
    nnz = 0 if Aj is None else len(Aj)
    ldX, ldY = (k if ldX is None else ldX), (k if ldY is None else ldY)
    if m < 0 or n < 0:
        return "negative size"
    if k < 1:
        return "k < 1"
    if ldX < k:
        return "ldX < k"
    if ldY < k:
        return "ldY < k"
    if Ap is None:
        return "NULL rowPtrA"
    if Aj is None and nnz > 0:
        return "NULL colIndA"
    if not has_x and nnz > 0:
        return "NULL x"
    if not has_y and m > 0:
        return "NULL y"
    if overlap:
        return "y overlaps an input"
    Ap = np.asarray(Ap, np.int64)
    if len(Ap) != m + 1 or Ap[0] != 0:
        return "rowPtrA[0] != 0"
    if Ap[-1] != nnz:
        return "rowPtrA[m] != nnzA"
    if np.any(np.diff(Ap) < 0) or np.any(Ap < 0) or np.any(Ap > nnz):
        return "decreasing rowPtrA"
    Aj = np.asarray(Aj, np.int64)
    if nnz and (Aj.min() < 0 or Aj.max() >= n):
        return "column of A out of range"
    return None


def _rowsum(P):
    """the sum over axis 0 of the (entries x k) products, from +0: fsum where a column is finite, numpy's class otherwise"""
    out = np.zeros(P.shape[1], np.float64)
    for c in range(P.shape[1]):
        g = P[:, c]
        if np.isfinite(g).all():
            out[c] = math.fsum(g) + 0.0
        else:
            with np.errstate(invalid="ignore"):
                out[c] = g.sum()
    return out


def spmm(m, n, Ap, Aj, Ax, X, alpha=1.0, beta=0.0, Y=None, dtype=np.float64):
    """Returns (out, S, K): out (m x k) in `dtype`; S float64 and K int64 of the same shape.  Ax None: every entry counts
    as 1.  Y may be None when beta == 0."""
    X = np.asarray(X)
    X = X.reshape(n, -1) if X.ndim != 2 else X
    k = X.shape[1]
    assert invalid(m, n, Ap, Aj, k) is None and X.shape[0] == n
    Ap, Aj = np.asarray(Ap, np.int64), np.asarray(Aj, np.int64)
    a = np.ones(len(Aj), np.float64) if Ax is None else np.ascontiguousarray(Ax, dtype).astype(np.float64)
    x = np.ascontiguousarray(X, dtype).astype(np.float64)
    alpha, beta = np.float64(alpha), np.float64(beta)
    s = np.zeros((m, k), np.float64)
    S = np.zeros((m, k), np.float64)
    with np.errstate(all="ignore"):
        for i in range(m):
            lo, hi = Ap[i], Ap[i + 1]
            if hi > lo:
                P = a[lo:hi, None] * x[Aj[lo:hi]]
                s[i] = _rowsum(P)
                S[i] = np.abs(P).sum(axis=0)
        t = alpha * s
        S = np.abs(alpha) * S
        if beta != 0.0:
            y = np.ascontiguousarray(np.asarray(Y).reshape(m, k), dtype).astype(np.float64)
            t = t + beta * y
            S = S + np.abs(beta) * np.abs(y)
        S = np.where(np.isnan(S), np.inf, S)
        K = np.repeat((np.diff(Ap) + 2)[:, None], k, axis=1).astype(np.int64)
        return t.astype(dtype), S, K


def spmv(m, n, Ap, Aj, Ax, x, alpha=1.0, beta=0.0, y=None, dtype=np.float64):
    """the k = 1 case on vectors: (out[m], S[m], K[m])"""
    out, S, K = spmm(m, n, Ap, Aj, Ax, np.asarray(x).reshape(n, 1), alpha, beta, None if y is None else np.asarray(y).reshape(m, 1),
                     dtype)
    return out[:, 0], S[:, 0], K[:, 0]
