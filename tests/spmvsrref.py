"""bhs_csr_spmv_semiring_device and bhs_csr_spmm_semiring_device of include/bhsparse_hip.h ("semiring CSR x dense") restated
in numpy: the reference of their tests.

A is an m x n CSR matrix whose rows need not be ascending and may hold duplicate (row, column) pairs, each of them an entry;
X is n x k, the mask M and Y are m x k.  Inputs are rounded to the build's value type first and everything after that is
float64.  For element (i, c): t = (+) over the row's entries of a (x) X(col, c) from the (+)-identity -- min and max on the
order-preserving keys of tests/semiringref.py (-0 below +0, a NaN product takes the key that wins), the PLUS_TIMES sum as
the correctly rounded sum (math.fsum) where the products are finite --, then double(y_old) (+) t with `accumulate`, one
rounding to the value type.  An element is selected where its mask value is non-zero (NaN is, -0 is not), or is NOT with
`complement`; what is not selected keeps what Y held (NaN where no Y is given: nothing is written there).  `changed` counts
the selected elements whose stored value differs as a number from y_old (accumulate) or from the identity (+0 == -0, NaN
over NaN unchanged)."""
import math

import numpy as np

import semiringref as srf

SEMIRINGS = srf.SEMIRINGS
ACCUM, COMPLEMENT = 1, 2

# the arguments the calls refuse on the host (each BHS_ERR_INVALID_ARG, Y untouched), by the word invalid() gives
HOST_REFUSALS = ("negative size", "k < 1", "ldX < k", "ldY < k", "NULL rowPtrA", "NULL colIndA", "NULL x", "NULL y",
                 "unknown semiring", "unknown flag", "ldM < k", "complement without a mask", "y overlaps an input")
# what the device's validation refuses
DEVICE_REFUSALS = ("rowPtrA[0] != 0", "rowPtrA[m] != nnzA", "decreasing rowPtrA", "column of A out of range")


def selected(mask, complement, m, k):
    """the m x k elements the mask selects (None: all of them)"""
    if mask is None:
        return np.ones((m, k), bool)
    with np.errstate(invalid="ignore"):
        return (np.asarray(mask).reshape(m, k) != 0) != bool(complement)


def invalid(m, n, Ap, Aj, k=1, ldX=None, ldY=None, has_x=True, has_y=True, overlap=False, semiring=0, flags=0, has_mask=False,
            ldM=None, rows_read=None):
    """What the calls must refuse: a word for the first reason found (one of HOST_REFUSALS, then DEVICE_REFUSALS), or None
    for a legal call.  Ap / Aj None stand for NULL pointers; nnzA is len(Aj).  rows_read: which rows hold a selected
    element (None: all) -- columns are checked where they are read, the row pointer everywhere."""
    nnz = 0 if Aj is None else len(Aj)
    ldX, ldY, ldM = (k if ldX is None else ldX), (k if ldY is None else ldY), (k if ldM is None else ldM)
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
    if semiring not in SEMIRINGS.values():
        return "unknown semiring"
    if flags & ~(ACCUM | COMPLEMENT):
        return "unknown flag"
    if has_mask and ldM < k:
        return "ldM < k"
    if not has_mask and flags & COMPLEMENT:
        return "complement without a mask"
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
    read = np.ones(m, bool) if rows_read is None else np.asarray(rows_read, bool)
    per_entry = np.repeat(read, np.diff(Ap))
    if nnz and np.any(per_entry & ((Aj < 0) | (Aj >= n))):
        return "column of A out of range"
    return None


def _keys(p, is_max):
    return np.where(np.isnan(p), srf.ALL1 if is_max else np.uint64(0), srf.encode(p))


def _fsum_columns(P):
    """the sum over axis 0 of the (entries x k) products from +0: fsum where a column is finite, numpy's class otherwise"""
    out = np.zeros(P.shape[1], np.float64)
    for c in range(P.shape[1]):
        g = P[:, c]
        if np.isfinite(g).all():
            out[c] = math.fsum(g) + 0.0
        else:
            with np.errstate(invalid="ignore"):
                out[c] = g.sum()
    return out


def products(name, a, x):
    """a (x) x for a (entries) against x (entries x k), float64"""
    a = a[:, None]
    with np.errstate(all="ignore"):
        if name in ("min_plus", "max_plus"):
            return a + x
        if name in ("max_times", "plus_times"):
            return a * x
        if name == "min_max":
            return srf.ordered(np.broadcast_to(a, x.shape), x, True)
        if name == "max_min":
            return srf.ordered(np.broadcast_to(a, x.shape), x, False)
        if name == "or_and":
            return ((a != 0) & (x != 0)).astype(np.float64)
        return np.ones(x.shape)


def reduce_rows(name, m, n, Ap, Aj, Ax, X, dtype=np.float64):
    """t (m x k, float64, not rounded): the row's reduction from the identity.  Also S = sum |products| (PLUS_ semirings;
    what tests/valuecheck.py bounds the error of a summation order with)."""
    Ap, Aj = np.asarray(Ap, np.int64), np.asarray(Aj, np.int64)
    x = np.ascontiguousarray(X, dtype).astype(np.float64)
    k = x.shape[1]
    a = np.ones(len(Aj), np.float64) if Ax is None else np.ascontiguousarray(Ax, dtype).astype(np.float64)
    t = np.full((m, k), srf.identity(name), np.float64)
    S = np.zeros((m, k), np.float64)
    is_max = name.startswith("max") or name == "or_and"
    for i in range(m):
        lo, hi = Ap[i], Ap[i + 1]
        if hi == lo:
            continue
        P = products(name, a[lo:hi], x[Aj[lo:hi]])
        if name == "plus_times":
            t[i] = _fsum_columns(P)
            with np.errstate(all="ignore"):
                S[i] = np.abs(P).sum(axis=0)
        elif name == "plus_pair":
            t[i] = float(hi - lo)
            S[i] = float(hi - lo)
        else:
            K = _keys(P, is_max)
            t[i] = srf.decode(K.max(axis=0) if is_max else K.min(axis=0))
    return t, S


def spmm_semiring(name, m, n, Ap, Aj, Ax, X, Y=None, mask=None, accumulate=False, complement=False, dtype=np.float64,
                  with_bound=False):
    """Returns (out, changed): out (m x k) in `dtype`, changed an int.  Ax None: every entry counts as 1.  Y may be None
    without `accumulate`: what the mask does not select then comes back as NaN (nothing is written there).  with_bound:
    returns (out, changed, ref64, S, K) -- the unrounded result, sum |terms| and the number of operations per element, for
    the PLUS_ semirings' error bound."""
    X = np.asarray(X)
    X = X.reshape(n, -1) if X.ndim != 2 else X
    k = X.shape[1]
    sel = selected(mask, complement, m, k)
    flags = (ACCUM if accumulate else 0) | (COMPLEMENT if complement else 0)
    assert invalid(m, n, Ap, Aj, k, semiring=SEMIRINGS[name], flags=flags, has_mask=mask is not None,
                   rows_read=sel.any(axis=1)) is None and X.shape[0] == n
    # rows that are not read may hold columns that are no index: give them none
    Ap_ = np.asarray(Ap, np.int64)
    read = np.repeat(sel.any(axis=1), np.diff(Ap_))
    Aj_ = np.where(read, np.asarray(Aj, np.int64), 0)
    t, S = reduce_rows(name, m, n, Ap_, Aj_, Ax, X, dtype)
    ident = np.asarray(srf.identity(name), dtype)
    with np.errstate(all="ignore"):
        if Y is None:
            assert not accumulate
            old = np.full((m, k), np.nan, dtype)
        else:
            old = np.ascontiguousarray(np.asarray(Y).reshape(m, k), dtype).copy()
        if accumulate:
            y = old.astype(np.float64)
            if name == "or_and":
                y = (y != 0).astype(np.float64)
            if name in ("plus_times", "plus_pair"):
                t = y + t
                S = S + np.abs(y)
            else:
                is_max = name.startswith("max") or name == "or_and"
                ky, kt = _keys(y, is_max), _keys(t, is_max)
                t = srf.decode(np.maximum(ky, kt) if is_max else np.minimum(ky, kt))
        new = t.astype(dtype)                                       # the one rounding
        was = old if accumulate else np.broadcast_to(ident, new.shape)
        same = (new == was) | (np.isnan(new) & np.isnan(was))
        changed = int(np.count_nonzero(sel & ~same))
        out = np.where(sel, new, old)
    if with_bound:
        K = np.repeat((np.diff(Ap_) + 1 + (1 if accumulate else 0))[:, None], k, axis=1).astype(np.int64)
        S = np.where(np.isnan(S), np.inf, S)
        return out, changed, np.where(sel, t, old.astype(np.float64)), S, K
    return out, changed


def spmv_semiring(name, m, n, Ap, Aj, Ax, x, y=None, mask=None, accumulate=False, complement=False, dtype=np.float64):
    """the k = 1 case on vectors: (out[m], changed)"""
    out, changed = spmm_semiring(name, m, n, Ap, Aj, Ax, np.asarray(x).reshape(n, 1), None if y is None else np.asarray(y).reshape(m, 1),
                                 None if mask is None else np.asarray(mask).reshape(m, 1), accumulate, complement, dtype)
    return out[:, 0], changed
