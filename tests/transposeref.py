"""The stable transpose of include/bhsparse_hip.h ("transpose") restated in numpy: the reference of the transpose's tests.

T = X^T for an m x n CSR matrix X whose rows need not be ascending and may hold duplicate (row, column) pairs.  Row j of T
holds the entries of X with column j in the order of their position in X's arrays: a stable argsort of colIndX."""
import numpy as np


def transpose(m, n, Xp, Xj, Xx=None):
    """Returns (Tp int32[n+1], Tj int32[nnz], Tx (Xx's dtype, or None), perm int32[nnz]); perm[q] is the position in X of
    entry q of T, so Tx == Xx[perm] bit for bit."""
    Xp = np.asarray(Xp, np.int64)
    Xj = np.asarray(Xj, np.int64)
    nnz = len(Xj)
    assert len(Xp) == m + 1 and Xp[0] == 0 and Xp[-1] == nnz and np.all(np.diff(Xp) >= 0)
    assert nnz == 0 or (Xj.min() >= 0 and Xj.max() < n)
    order = np.argsort(Xj, kind="stable")
    rows = np.repeat(np.arange(m, dtype=np.int64), np.diff(Xp))
    Tp = np.zeros(n + 1, np.int64)
    np.cumsum(np.bincount(Xj, minlength=n)[:n] if nnz else np.zeros(n, np.int64), out=Tp[1:])
    Tx = None if Xx is None else np.ascontiguousarray(Xx)[order]
    return Tp.astype(np.int32), rows[order].astype(np.int32), Tx, order.astype(np.int32)


def sort_rows(m, Xp, Xj, Xx):
    """X with every row stably sorted by column: what (X^T)^T is."""
    Xp = np.asarray(Xp, np.int64)
    rows = np.repeat(np.arange(m, dtype=np.int64), np.diff(Xp))
    order = np.lexsort((np.arange(len(Xj)), np.asarray(Xj, np.int64), rows))
    return np.asarray(Xj, np.int32)[order], np.ascontiguousarray(Xx)[order]
