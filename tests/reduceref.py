"""bhs_csr_reduce_device and bhs_csr_scale_device of include/bhsparse_hip.h ("reduce / scale") restated in numpy: the
reference of their tests.

X is an m x n CSR matrix whose rows need not be ascending and may hold duplicate (row, column) pairs.  Every entry is
converted to double; min and max order values as numbers with -0 below +0 and hand a NaN through; the sums are math.fsum of
the terms (the correctly rounded sum), rounded once to the value type, a zero sum being +0.  For the sum operators reduce()
also returns S = sum |term| and K = number of terms per output: what tests/valuecheck.py bounds the error of any summation
order with."""
import math

import numpy as np

ROWS, COLS, ALL, DIAG = 0, 1, 2, 3
PLUS, MIN, MAX, ABS_PLUS, ABS_MAX, SQ_PLUS, COUNT = range(7)
OFFDIAG = 1
LEFT_DIV, RIGHT_DIV = 1, 2
SUM_OPS = (PLUS, ABS_PLUS, SQ_PLUS, COUNT)


def _rowptr_invalid(m, Xp, nnz):
    Xp = np.asarray(Xp, np.int64)
    if len(Xp) != m + 1 or Xp[0] != 0:
        return "rowPtrX[0] != 0"
    if Xp[-1] != nnz:
        return "rowPtrX[m] != nnzX"
    if np.any(np.diff(Xp) < 0) or np.any(Xp < 0) or np.any(Xp > nnz):
        return "decreasing rowPtrX"
    return None


def reads_columns(axis, flags):
    return axis in (COLS, DIAG) or bool(flags & OFFDIAG)


def invalid(m, n, Xp, Xj, axis, op, flags=0):
    """What bhs_csr_reduce_device must refuse: a word for the first reason found, or None for a legal call.  X's columns
    count only in the calls that read them, and for the diagonal only in the rows below min(m, n)."""
    if axis not in (ROWS, COLS, ALL, DIAG):
        return "unknown axis"
    if op not in range(7):
        return "unknown op"
    if flags & ~OFFDIAG:
        return "unknown flag"
    if (flags & OFFDIAG) and axis == DIAG:
        return "OFFDIAG with DIAG"
    Xj = np.asarray(Xj, np.int64)
    bad = _rowptr_invalid(m, Xp, len(Xj))
    if bad:
        return bad
    if reads_columns(axis, flags):
        Xp = np.asarray(Xp, np.int64)
        seg = Xj[:Xp[min(m, n)]] if axis == DIAG else Xj
        if len(seg) and (seg.min() < 0 or seg.max() >= n):
            return "column of X out of range"
    return None


def invalid_scale(m, n, Xp, Xj, has_left, has_right, flags=0):
    """The same for bhs_csr_scale_device: X's columns count only with a right vector."""
    if flags & ~(LEFT_DIV | RIGHT_DIV):
        return "unknown flag"
    if ((flags & LEFT_DIV) and not has_left) or ((flags & RIGHT_DIV) and not has_right):
        return "DIV without its vector"
    Xj = np.asarray(Xj, np.int64)
    bad = _rowptr_invalid(m, Xp, len(Xj))
    if bad:
        return bad
    if has_right and len(Xj) and (Xj.min() < 0 or Xj.max() >= n):
        return "column of X out of range"
    return None


def identity(op):
    return {MIN: np.inf, MAX: -np.inf}.get(op, 0.0)


def reduce(m, n, Xp, Xj, Xx, axis, op, flags=0, dtype=np.float64):
    """Returns (out, S, K): out in `dtype` (m, n, 1 or min(m, n) values); S and K float64 / int64 arrays of the same length
    for the sum operators (COUNT included), None otherwise.  Xx None: every entry counts as 1."""
    assert invalid(m, n, Xp, Xj, axis, op, flags) is None
    Xp = np.asarray(Xp, np.int64)
    Xj = np.asarray(Xj, np.int64)
    nnz = len(Xj)
    x = np.ones(nnz, np.float64) if (Xx is None or op == COUNT) else np.ascontiguousarray(Xx, dtype).astype(np.float64)
    row = np.repeat(np.arange(m, dtype=np.int64), np.diff(Xp))
    keep = np.ones(nnz, bool)
    if flags & OFFDIAG:
        keep &= Xj != row
    if axis == DIAG:
        keep &= Xj == row
    dest = {ROWS: row, COLS: Xj, ALL: np.zeros(nnz, np.int64), DIAG: row}[axis]
    nOut = {ROWS: m, COLS: n, ALL: 1, DIAG: min(m, n)}[axis]
    with np.errstate(over="ignore", invalid="ignore"):
        term = {PLUS: x, MIN: x, MAX: x, ABS_PLUS: np.abs(x), ABS_MAX: np.abs(x), SQ_PLUS: x * x, COUNT: x}[op]
    dest, term = dest[keep], term[keep]
    order = np.argsort(dest, kind="stable")
    dest, term = dest[order], term[order]
    cuts = np.searchsorted(dest, np.arange(nOut + 1))
    out = np.full(nOut, identity(op), np.float64)
    sums = op in SUM_OPS
    S = np.zeros(nOut, np.float64) if sums else None
    K = np.diff(cuts).astype(np.int64) if sums else None
    full = np.flatnonzero(np.diff(cuts))                            # the outputs with an entry; their terms lie back to back
    if len(full) and not sums:
        starts = cuts[full]
        with np.errstate(invalid="ignore"):
            v = (np.minimum if op == MIN else np.maximum).reduceat(term, starts)      # (hands a NaN through)
        # a zero result: -0 below +0
        loses = np.signbit(term) if op == MIN else ~np.signbit(term)
        any_loser = np.logical_or.reduceat((term == 0.0) & loses, starts)
        zero = v == 0.0
        v[zero] = np.where(any_loser[zero], -0.0 if op == MIN else 0.0, 0.0 if op == MIN else -0.0)
        out[full] = v
    for i in (full if sums else ()):
        g = term[cuts[i]:cuts[i + 1]]
        if np.isfinite(g).all():
            out[i] = math.fsum(g) + 0.0
            S[i] = math.fsum(np.abs(g))
        else:                                                       # (fsum raises on Inf - Inf: the class is numpy's)
            with np.errstate(invalid="ignore"):
                out[i] = g.sum()
            S[i] = np.inf
    with np.errstate(over="ignore"):
        return out.astype(dtype), S, K


def scale(m, n, Xp, Xj, Xx, alpha=1.0, left=None, right=None, flags=0, dtype=np.float64):
    """valZ of Z = alpha Dl X Dr in `dtype`: t = double(x), (*|/) l[i], (*|/) r[j], * alpha, one rounding."""
    assert invalid_scale(m, n, Xp, Xj, left is not None, right is not None, flags) is None
    Xp = np.asarray(Xp, np.int64)
    Xj = np.asarray(Xj, np.int64)
    t = np.ascontiguousarray(Xx, dtype).astype(np.float64)
    row = np.repeat(np.arange(m, dtype=np.int64), np.diff(Xp))
    with np.errstate(all="ignore"):
        if left is not None:
            l = np.ascontiguousarray(left, dtype).astype(np.float64)[row]
            t = t / l if flags & LEFT_DIV else t * l
        if right is not None:
            r = np.ascontiguousarray(right, dtype).astype(np.float64)[Xj]
            t = t / r if flags & RIGHT_DIV else t * r
        t = t * np.float64(alpha)
        return t.astype(dtype)
