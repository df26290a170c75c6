"""The selection rule of include/bhsparse_hip.h ("entry selection") restated in plain numpy, row by row (test
infrastructure: the reference of tests/test_select_*.py -- the code under test is never its own reference).

    stage 1  position: BAND keeps band_lo <= col - row <= band_hi, DROP_DIAG drops col == row
    stage 2  ABS: keep unless |v| <= abs_tol
    stage 3  REL: keep unless |v| < rel_tol * rowmax      (rowmax over what stage 1 left, highest in rank order)
    stage 4  TOPK: the top_k entries of largest |v| of what is left, ties to the entry that comes first
    KEEP_DIAG: col == row that passed stage 1 passes 2-4, is not counted in top_k, does not enter rowmax

|v| is abs(float64(v)); rank order is the order of its bit pattern as uint64 (NaN above Inf).  The survivors keep their
order and their bits."""
import numpy as np

BAND, DROP_DIAG, KEEP_DIAG, ABS, REL, TOPK = 1, 2, 4, 8, 16, 32


class Spec(object):
    """The fields of bhs_select."""

    def __init__(self, flags=0, top_k=0, band_lo=0, band_hi=0, abs_tol=0.0, rel_tol=0.0):
        self.flags, self.top_k, self.band_lo, self.band_hi = int(flags), int(top_k), int(band_lo), int(band_hi)
        self.abs_tol, self.rel_tol = float(abs_tol), float(rel_tol)


def select_row(row, cols, vals, spec):
    """Indices (ascending: input order) of the entries of one row that survive."""
    cols = [int(c) for c in cols]                                   # (python ints: col - row cannot overflow)
    mag = np.abs(np.asarray(vals, np.float64)) if vals is not None else np.zeros(len(cols))
    key = mag.view(np.uint64)
    f = spec.flags
    stage1 = []
    for i, c in enumerate(cols):
        if f & BAND and not (spec.band_lo <= c - row <= spec.band_hi):
            continue
        if f & DROP_DIAG and c == row:
            continue
        stage1.append(i)
    always = [i for i in stage1 if f & KEEP_DIAG and cols[i] == row]
    rest = [i for i in stage1 if not (f & KEEP_DIAG and cols[i] == row)]
    rowmax = 0.0
    if rest:
        rowmax = float(np.array([key[rest].max()], np.uint64).view(np.float64)[0])
    if f & ABS:
        rest = [i for i in rest if not (mag[i] <= spec.abs_tol)]
    if f & REL:
        with np.errstate(invalid="ignore"):
            thr = np.float64(spec.rel_tol) * np.float64(rowmax)
        rest = [i for i in rest if not (mag[i] < thr)]
    if f & TOPK and len(rest) > spec.top_k:
        order = _stable_desc(key[rest])
        rest = [rest[j] for j in order[:spec.top_k]]
    return sorted(always + rest)


def _stable_desc(k):
    """Stable descending order of uint64 keys: np.argsort(-key, kind="stable") with the negation taken in uint64 (it wraps,
    and reverses the order of all keys but 0, which no |v| > 0 has; +0 is mapped apart so that it stays last)."""
    k = np.asarray(k, np.uint64)
    neg = np.where(k == 0, np.uint64(0xFFFFFFFFFFFFFFFF), (~k) + np.uint64(1))   # -key mod 2^64; key 0 ranks last
    return np.argsort(neg, kind="stable")


def select(m, n, Xp, Xj, Xx, spec):
    """Z = select(X).  Returns (Zp int32[m+1], Zj int32, Zx of Xx's dtype or None)."""
    Xp = np.asarray(Xp, np.int64)
    keep = []
    Zp = np.zeros(m + 1, np.int64)
    for r in range(m):
        a, b = int(Xp[r]), int(Xp[r + 1])
        idx = select_row(r, Xj[a:b], None if Xx is None else Xx[a:b], spec)
        keep.extend(a + i for i in idx)
        Zp[r + 1] = Zp[r] + len(idx)
    keep = np.asarray(keep, np.int64)
    Zj = np.asarray(Xj, np.int32)[keep]
    Zx = None if Xx is None else np.asarray(Xx)[keep]
    return Zp.astype(np.int32), Zj, Zx
