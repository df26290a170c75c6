"""The assembly's reference (test infrastructure): include/bhsparse_hip.h's "assembly" restated in numpy, the sums as a loop.

assemble(m, n, rows, cols, vals, flags) returns (Zp, Zj, Zx, entryPtr, perm, nkept), or raises Refused where the contract
refuses the triplets.  vals may be None (Zx is None then) and has the value type of the build under test: the sum runs in
double in the stable order, starting FROM the run's first value, and is rounded once to that type."""
import numpy as np

SUM, FIRST, LAST, KEEP, IGNORE_NEGATIVE = 0, 1, 2, 3, 4


class Refused(ValueError):
    pass


def kept_positions(m, n, rows, cols, flags):
    rows, cols = np.asarray(rows, np.int64), np.asarray(cols, np.int64)
    if np.any(rows >= m) or np.any(cols >= n):
        raise Refused("an index >= m or >= n")
    neg = (rows < 0) | (cols < 0)
    if np.any(neg) and not flags & IGNORE_NEGATIVE:
        raise Refused("a negative index without IGNORE_NEGATIVE")
    return np.flatnonzero(~neg)


def run_sums(vals, perm, entryPtr):
    """s = double(first); s += double(next) ... in perm's order, one rounding to vals' type -- a loop over the place in the
    run, every run that reaches the place at once: each run's additions happen one after the other"""
    v = np.asarray(vals)[perm].astype(np.float64)
    start, length = entryPtr[:-1], np.diff(entryPtr)
    s = v[start].copy() if len(start) else np.zeros(0)
    with np.errstate(all="ignore"):
        for k in range(1, int(length.max()) if len(length) else 0):
            live = np.flatnonzero(length > k)
            s[live] = s[live] + v[start[live] + k]
        return s.astype(np.asarray(vals).dtype)


def values(vals, entryPtr, perm, flags):
    """what bhs_coo_assemble_values_device computes from a map"""
    mode = flags & 3
    entryPtr, perm = np.asarray(entryPtr, np.int64), np.asarray(perm, np.int64)
    if mode == SUM:
        return run_sums(vals, perm, entryPtr)
    vals = np.asarray(vals)
    return vals[perm[entryPtr[:-1]]] if mode in (FIRST, KEEP) else vals[perm[entryPtr[1:] - 1]]


def assemble(m, n, rows, cols, vals, flags):
    rows, cols = np.asarray(rows, np.int64), np.asarray(cols, np.int64)
    kept = kept_positions(m, n, rows, cols, flags)
    perm = kept[np.lexsort((kept, cols[kept], rows[kept]))]           # by (row, column, position)
    nkept = len(perm)
    r, c = rows[perm], cols[perm]
    if (flags & 3) == KEEP:
        head = np.ones(nkept, bool)
    else:
        head = np.ones(nkept, bool)
        head[1:] = (r[1:] != r[:-1]) | (c[1:] != c[:-1])
    first = np.flatnonzero(head)
    entryPtr = np.append(first, nkept).astype(np.int64)
    Zj = c[first].astype(np.int32)
    Zp = np.zeros(m + 1, np.int64)
    np.cumsum(np.bincount(r[first], minlength=m), out=Zp[1:])
    Zx = None if vals is None else values(vals, entryPtr, perm, flags)
    return Zp.astype(np.int32), Zj, Zx, entryPtr.astype(np.int32), perm.astype(np.int32), nkept


def raw_lengths(m, n, rows, cols, flags):
    """the kept triplets per row: what the library's bins (up to 32, up to 1024, beyond; in LDS up to 4096) go by"""
    kept = kept_positions(m, n, rows, cols, flags)
    return np.bincount(np.asarray(rows, np.int64)[kept], minlength=m)
