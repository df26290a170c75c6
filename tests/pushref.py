"""bhs_csr_push_semiring_device of include/bhsparse_hip.h ("sparse frontier x CSR") restated in numpy: the reference of its
tests.

G is an m x n CSR matrix of out-edges whose rows need not be ascending and may hold duplicate (row, column) pairs, each of
them an entry; fidx lists nf rows of G, repeats allowed, each listing an operand of its own; F is nf x k, the mask M and Y
are n x k.  Inputs are rounded to the build's value type first and everything after that is float64.  For every list
position p, every entry e of row fidx[p] and every column c, the selected element Y(col_e, c) takes double(Y) (+) (g_e (x)
F(p, c)): min and max on the order-preserving keys of tests/semiringref.py (-0 below +0, a NaN product takes the key that
wins), or as max over {0, 1} with a reached Y counting as 1 where it is not zero; one rounding to the value type -- which
equals a rounding per update, rounding being monotone.  PLUS_PAIR adds 1 per entry, with a rounding each.  An element that
no product reaches, or that the mask does not select, keeps its bits.  `changed` counts the elements whose value differs as
a number from what Y held (+0 == -0, NaN over NaN unchanged); `next` lists the rows that hold one, ascending."""
import numpy as np

import semiringref as srf
import spmvsrref as sr

SEMIRINGS = {k: v for k, v in srf.SEMIRINGS.items() if k != "plus_times"}     # the seven the call accepts
COMPLEMENT = sr.COMPLEMENT

# the arguments the call refuses on the host (each BHS_ERR_INVALID_ARG, Y untouched), by the word invalid() gives
HOST_REFUSALS = ("negative size", "k < 1", "ldF < k", "ldY < k", "NULL rowPtrG", "NULL colIndG", "NULL fidx", "NULL F", "NULL Y",
                 "unknown semiring", "plus_times", "unknown flag", "ldM < k", "complement without a mask",
                 "an output overlaps an input")
# what the device's validation refuses
DEVICE_REFUSALS = ("fidx out of range", "bad row pointer in a pushed row", "column out of range in a pushed row")


def invalid(m, n, Gp, Gj, nf, fidx, k=1, ldF=None, ldY=None, has_F=True, has_Y=True, overlap=False, semiring=1, flags=0,
            has_mask=False, ldM=None, nnzG=None):
    """What the call must refuse: a word for the first reason found (one of HOST_REFUSALS, then DEVICE_REFUSALS), or None
    for a legal call.  Gp / Gj / fidx None stand for NULL pointers; nnzG defaults to len(Gj).  Rows of G that are not
    listed are not looked at: whatever their row pointer and columns hold is legal."""
    nnz = (0 if Gj is None else len(Gj)) if nnzG is None else nnzG
    ldF, ldY, ldM = (k if ldF is None else ldF), (k if ldY is None else ldY), (k if ldM is None else ldM)
    if m < 0 or n < 0 or nnz < 0 or nf < 0:
        return "negative size"
    if k < 1:
        return "k < 1"
    if ldF < k:
        return "ldF < k"
    if ldY < k:
        return "ldY < k"
    if Gp is None and m > 0:
        return "NULL rowPtrG"
    if Gj is None and nnz > 0:
        return "NULL colIndG"
    if fidx is None and nf > 0:
        return "NULL fidx"
    if not has_F and nf > 0:
        return "NULL F"
    if not has_Y and n > 0:
        return "NULL Y"
    if semiring == srf.SEMIRINGS["plus_times"]:
        return "plus_times"
    if semiring not in SEMIRINGS.values():
        return "unknown semiring"
    if flags & ~COMPLEMENT:
        return "unknown flag"
    if has_mask and ldM < k:
        return "ldM < k"
    if not has_mask and flags & COMPLEMENT:
        return "complement without a mask"
    if overlap:
        return "an output overlaps an input"
    f = np.asarray(fidx, np.int64)[:nf] if nf else np.zeros(0, np.int64)
    if np.any((f < 0) | (f >= m)):
        return "fidx out of range"
    Gp = np.asarray(Gp, np.int64) if m > 0 else np.zeros(1, np.int64)
    a, b = Gp[f], Gp[f + 1]
    if np.any((a > b) | (a < 0) | (b > nnz)):
        return "bad row pointer in a pushed row"
    Gj = np.zeros(0, np.int64) if Gj is None else np.asarray(Gj, np.int64)
    for lo, hi in zip(a, b):
        if np.any((Gj[lo:hi] < 0) | (Gj[lo:hi] >= n)):
            return "column out of range in a pushed row"
    return None


def push_semiring(name, m, n, Gp, Gj, Gx, fidx, F, Y, mask=None, complement=False, dtype=np.float64):
    """Returns (out, changed, next): out (n x k) in `dtype`, changed an int, next the int32 rows of Y that hold a changed
    element, ascending.  Gx None: every entry counts as 1.  F: nf x k (or nf values: k = 1), Y and mask: n x k."""
    fidx = np.asarray(fidx, np.int64).reshape(-1)
    nf = len(fidx)
    Y = np.asarray(Y)
    flat = Y.ndim == 1
    k = 1 if flat else Y.shape[1]
    old = np.ascontiguousarray(Y.reshape(n, k), dtype).copy()
    f = np.ascontiguousarray(np.asarray(F).reshape(nf, k), dtype).astype(np.float64)
    sel = sr.selected(mask, complement, n, k)
    assert invalid(m, n, Gp, Gj, nf, fidx, k, semiring=SEMIRINGS[name], flags=COMPLEMENT if complement else 0,
                   has_mask=mask is not None) is None
    Gp, Gj = np.asarray(Gp, np.int64), np.asarray(Gj, np.int64)
    g = np.ones(len(Gj), np.float64) if Gx is None else np.ascontiguousarray(Gx, dtype).astype(np.float64)
    is_max = name.startswith("max") or name == "or_and"
    reached = np.zeros((n, k), bool)
    count = np.zeros(n, np.int64)                                   # plus_pair: entries that land on the row
    key = np.full((n, k), sr._keys(np.full(1, srf.identity(name)), is_max)[0], np.uint64)
    for p in range(nf):
        lo, hi = Gp[fidx[p]], Gp[fidx[p] + 1]
        if hi == lo:
            continue
        cols = Gj[lo:hi]
        reached[cols] = True
        if name == "plus_pair":
            np.add.at(count, cols, 1)
            continue
        K = sr._keys(sr.products(name, g[lo:hi], np.broadcast_to(f[p], (hi - lo, k))), is_max)
        (np.maximum if is_max else np.minimum).at(key, cols, K)
    with np.errstate(all="ignore"):
        y = old.astype(np.float64)
        if name == "plus_pair":
            new = old.copy()
            left = np.repeat(count[:, None], k, axis=1)
            while left.any():                                        # a rounding per add (exact in double below 2^53)
                new = np.where(left > 0, (new.astype(np.float64) + 1.0).astype(dtype), new)
                left = np.maximum(left - 1, 0)
        else:
            if name == "or_and":
                y = (y != 0).astype(np.float64)
            ky = sr._keys(y, is_max)
            new = srf.decode(np.maximum(ky, key) if is_max else np.minimum(ky, key)).astype(dtype)   # the one rounding
        hit = sel & reached
        out = np.where(hit, new, old)
        same = (out == old) | (np.isnan(out) & np.isnan(old))
    changed_at = hit & ~same
    res = out[:, 0] if flat else out
    return res, int(np.count_nonzero(changed_at)), np.flatnonzero(changed_at.any(axis=1)).astype(np.int32)
