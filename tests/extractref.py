"""Z = X(rows, cols) of include/bhsparse_hip.h ("extract") restated in numpy: the reference of the extraction's tests.

X is an m x n CSR matrix whose rows need not be ascending and may hold duplicate (row, column) pairs.  Row i of Z holds the
entries of X's row rows[i] whose column is named by cols, relabelled to their place in cols, in ascending order of that
place; ties keep the order of their position in X (a stable argsort)."""
import numpy as np


def invalid(m, n, Xp, Xj, rows=None, cols=None, mI=None, nJ=None):
    """What the validation must refuse: a word for the first reason found, or None for a legal call.  X's columns count only
    in the rows that `rows` names (the others are never read); its row pointer counts everywhere."""
    Xp = np.asarray(Xp, np.int64)
    Xj = np.asarray(Xj, np.int64)
    nnz = len(Xj)
    if len(Xp) != m + 1 or Xp[0] != 0:
        return "rowPtrX[0] != 0"
    if Xp[-1] != nnz:
        return "rowPtrX[m] != nnzX"
    if np.any(np.diff(Xp) < 0) or np.any(Xp < 0) or np.any(Xp > nnz):
        return "decreasing rowPtrX"
    if rows is None:
        if (m if mI is None else mI) != m:
            return "rows NULL with mI != m"
        r = np.arange(m, dtype=np.int64)
    else:
        r = np.asarray(rows, np.int64)
        if np.any(r < 0) or np.any(r >= m):
            return "row index out of range"
    if cols is None:
        if (n if nJ is None else nJ) != n:
            return "cols NULL with nJ != n"
    else:
        c = np.asarray(cols, np.int64)
        if np.any(c < 0) or np.any(c >= n):
            return "column index out of range"
        if len(np.unique(c)) != len(c):
            return "repeated column index"
    for i in np.unique(r):
        seg = Xj[Xp[i]:Xp[i + 1]]
        if len(seg) and (seg.min() < 0 or seg.max() >= n):
            return "column of X out of range"
    return None


def extract(m, n, Xp, Xj, Xx=None, rows=None, cols=None):
    """Returns (Zp int32[mI+1], Zj int32[nnzZ], Zx (Xx's dtype, or None), perm int32[nnzZ], reordered_rows); perm[p] is the
    position in X of entry p of Z, so Zx == Xx[perm] bit for bit; reordered_rows counts the Z rows whose relabelled entries
    were not already ascending."""
    assert invalid(m, n, Xp, Xj, rows, cols) is None
    Xp = np.asarray(Xp, np.int64)
    Xj = np.asarray(Xj, np.int64)
    r = np.arange(m, dtype=np.int64) if rows is None else np.asarray(rows, np.int64)
    if cols is None:
        inv = np.arange(n, dtype=np.int64)
    else:
        inv = np.full(n, -1, np.int64)
        inv[np.asarray(cols, np.int64)] = np.arange(len(cols), dtype=np.int64)
    lens = (Xp[r + 1] - Xp[r]) if len(r) else np.zeros(0, np.int64)
    zrow = np.repeat(np.arange(len(r), dtype=np.int64), lens)       # the Z row of every gathered entry
    start = np.zeros(len(r) + 1, np.int64)
    np.cumsum(lens, out=start[1:])
    q = np.arange(int(start[-1]), dtype=np.int64) - np.repeat(start[:-1], lens) + np.repeat(Xp[r], lens)
    j = inv[Xj[q]] if len(q) else np.zeros(0, np.int64)
    keep = j >= 0
    zrow, q, j = zrow[keep], q[keep], j[keep]
    seq = np.arange(len(q), dtype=np.int64)                         # (ties by position in the gathered sequence: q's order inside a row)
    order = np.lexsort((seq, j, zrow))
    moved = order != seq
    reordered = len(np.unique(zrow[moved])) if len(q) else 0
    Zp = np.zeros(len(r) + 1, np.int64)
    np.cumsum(np.bincount(zrow, minlength=len(r))[:len(r)] if len(q) else np.zeros(len(r), np.int64), out=Zp[1:])
    perm = q[order]
    Zx = None if Xx is None else np.ascontiguousarray(Xx)[perm]
    return Zp.astype(np.int32), j[order].astype(np.int32), Zx, perm.astype(np.int32), int(reordered)
