"""bhs_csr_cfsplit_device and bhs_csr_interp_{symbolic,numeric}_device of include/bhsparse_hip.h ("C/F splitting and
interpolation") restated in vectorised numpy: the reference of their tests, and the scipy restatement of the classical
hierarchy that benchmark_spgemm_using_csr_amd/amg.py builds on top of them (rs_setup, pcg).

Neighbours, the hash and the keys are the aggregation's (aggref.hash32, aggref.keys); BHS_CF_DEGREE puts the row's length in
front of the hash.  Restated independently of each other: the synchronous rounds the library runs (`split`) and the greedy
maximal independent set in descending key order by its definition (`greedy`).  `interp` follows the header's expression
order; its sums follow the SpMV's rule (`row_sums`: entry k of a row to lane k mod L, a lane adds in row order, the lanes
meet in a butterfly), so that it gives the device's bits on any values, not only where the sums are exact."""
import numpy as np

import aggref as ar

DEGREE = 1                                           # BHS_CF_DEGREE
UNDECIDED, IN = ar.UNDECIDED, ar.IN
KEY_MASK = np.uint64((1 << 62) - 1)


def keys(n, Sp, seed=0, prio=None, degree=False):
    """the n distinct 62-bit keys as uint64; degree: prio31 = min(row length, 1023) << 21 | hash >> 11"""
    if not degree:
        return ar.keys(n, seed, prio)
    assert prio is None, "BHS_CF_DEGREE with caller priorities is refused"
    i = np.arange(n, dtype=np.uint64)
    deg = np.minimum(np.diff(np.asarray(Sp, np.int64)[:n + 1]), 1023).astype(np.uint64)
    p31 = (deg << np.uint64(21)) | (ar.hash32(i, seed) >> np.uint64(11))
    return (p31 << np.uint64(31)) | i


def _near_max(n, Sp, c, w):
    """max of w over i and N(i): a segmented maximum over the rows that have entries"""
    out = w.copy()
    if len(c):
        has = np.diff(Sp) > 0
        out[has] = np.maximum(out[has], np.maximum.reduceat(w[c], Sp[:-1][has]))
    return out


def rounds(n, Sp, Sj, key, counts=None):
    """The library's algorithm: (is_c bool[n], number of rounds).  For every undecided i, m = the greatest word over i and
    N(i): m's state is in -> i is out; m is i's own word -> i is in; else i stays.  counts: a list that gets the number of
    undecided vertices every round starts from."""
    Sp = np.asarray(Sp, np.int64)[:n + 1]
    c = np.asarray(Sj, np.int64)[Sp[0]:Sp[n]]
    Sp = Sp - Sp[0]
    w = UNDECIDED | key
    nrounds = 0
    while True:
        und = (w >> np.uint64(62)) == 1
        if not und.any():
            break
        assert nrounds <= n, "a round decides at least one vertex"
        if counts is not None:
            counts.append(int(und.sum()))
        m = _near_max(n, Sp, c, w)
        goes_out = und & ((m >> np.uint64(62)) == 2)
        goes_in = und & (m == w)
        assert goes_in.any() or goes_out.any()
        w = np.where(goes_in, IN | key, np.where(goes_out, key, w))
        nrounds += 1
    return (w >> np.uint64(62)) == 2, nrounds


def greedy(n, Sp, Sj, key):
    """The definition, for a structurally symmetric S: vertices in descending key order, a vertex is C unless an
    off-diagonal neighbour chosen earlier is C.  is_c bool[n]."""
    Sp = np.asarray(Sp, np.int64)
    Sj = np.asarray(Sj, np.int64)
    blocked = np.zeros(n, bool)
    is_c = np.zeros(n, bool)
    for v in np.argsort(key)[::-1]:
        if blocked[v]:
            continue
        is_c[v] = True
        blocked[Sj[Sp[v]:Sp[v + 1]]] = True
    return is_c


def number(is_c):
    """(cf int32[n], nc, cpts int32[nc]): the C points numbered in ascending vertex order, -1 at an F point"""
    cpts = np.flatnonzero(is_c).astype(np.int32)
    cf = np.full(len(is_c), -1, np.int32)
    cf[cpts] = np.arange(len(cpts), dtype=np.int32)
    return cf, len(cpts), cpts


def split(n, Sp, Sj, seed=0, prio=None, degree=False, counts=None):
    """(cf int32[n], nc, rounds): what bhs_csr_cfsplit_device returns (the C points are flatnonzero(cf >= 0))"""
    if n == 0:
        return np.zeros(0, np.int32), 0, 0
    is_c, nrounds = rounds(n, Sp, Sj, keys(n, Sp, seed, prio, degree), counts)
    cf, nc, _ = number(is_c)
    return cf, nc, nrounds


def check_split(n, Sp, Sj, cf, nc, cpts=None):
    """on a symmetric S: independent, maximal, numbered in ascending vertex order"""
    r, c = ar.edges(n, Sp, Sj)
    off = r != c
    r, c = r[off], c[off]
    is_c = cf >= 0
    assert not np.any(is_c[r] & is_c[c]), "two C points are neighbours"
    covered = np.zeros(n, bool)
    covered[r[is_c[c]]] = True
    assert np.all(covered | is_c), "an F point without a C neighbour"
    assert np.array_equal(cf[is_c], np.arange(nc)) and np.all(cf[~is_c] == -1)
    if cpts is not None:
        assert np.array_equal(cpts, np.flatnonzero(is_c))


# ---------------------------------------------------------------- direct interpolation
def lanes(n, nnz):
    """lanes a row from the mean row length (ag_lanes)"""
    mean = nnz / n if n else 0.0
    return 1 if mean <= 4 else 4 if mean <= 16 else 16 if mean <= 64 else 64


def row_sums(n, Ap, vals, L):
    """The rows' sums of vals (0 where an entry does not count) by the SpMV's rule: entry k of a row goes to lane k mod L, a
    lane adds its entries in row order from +0, the L lanes meet in a butterfly of steps 1, 2, 4, .. (both partners add the
    same two numbers)."""
    Ap = np.asarray(Ap, np.int64)
    lens = np.diff(Ap)
    r = np.repeat(np.arange(n), lens)
    k = np.arange(len(vals)) - np.repeat(Ap[:-1], lens)
    T = np.zeros((n, L))
    for turn in range(int(-(-lens.max() // L)) if n and len(vals) else 0):
        sel = k // L == turn
        T[r[sel], k[sel] % L] += vals[sel]                           # (a row and lane once a turn)
    lane = np.arange(L)
    step = 1
    while step < L:
        T = T + T[:, lane ^ step]
        step *= 2
    return T[:, 0].copy()


def interp(n, Ap, Aj, Ax, Sp, Sj, cf, L=None):
    """(rowPtrP int32[n+1], colIndP int32, valP float64): the direct interpolation in double; rows of A and S strictly
    ascending.  L: the lanes a row of the sums (default: from A's mean row length, as the library takes them)."""
    Ap, Sp = np.asarray(Ap, np.int64)[:n + 1], np.asarray(Sp, np.int64)[:n + 1]
    j = np.asarray(Aj, np.int64)[:Ap[n]]
    a = np.asarray(Ax, np.float64)[:Ap[n]]
    cf = np.asarray(cf, np.int64)
    L = lanes(n, len(j)) if L is None else L
    r = np.repeat(np.arange(n, dtype=np.int64), np.diff(Ap))
    sr = np.repeat(np.arange(n, dtype=np.int64), np.diff(Sp))
    in_s = np.isin(r * n + j, sr * n + np.asarray(Sj, np.int64)[:Sp[n]])
    off = j != r
    d = np.zeros(n)
    d[r[~off]] = a[~off]                                             # a_ii, 0 where it is not stored
    coarse = off & in_s & (cf[j] >= 0)
    with np.errstate(all="ignore"):
        t = a * d[r]
        neg, pos = off & (t < 0), off & (t > 0)
        Nn, Np_ = row_sums(n, Ap, np.where(neg, a, 0.0), L), row_sums(n, Ap, np.where(pos, a, 0.0), L)
        Cn, Cp = row_sums(n, Ap, np.where(neg & coarse, a, 0.0), L), row_sums(n, Ap, np.where(pos & coarse, a, 0.0), L)
        dp = d.copy()
        dp = np.where(Cp == 0, dp + Np_, dp)
        dp = np.where(Cn == 0, dp + Nn, dp)
        fn, fp = Nn / Cn, Np_ / Cp
        w = np.where(neg, -(fn[r] * a) / dp[r], np.where(pos, -(fp[r] * a) / dp[r], -(0.0 * a) / dp[r]))
    kept = coarse & (cf[r] < 0)
    cpts = np.flatnonzero(cf >= 0)
    rows = np.concatenate([r[kept], cpts])
    cols = np.concatenate([cf[j[kept]], cf[cpts]])
    vals = np.concatenate([w[kept], np.ones(len(cpts))])
    o = np.argsort(rows, kind="stable")                              # (a row's kept entries stay in ascending j)
    Pp = np.zeros(n + 1, np.int32)
    np.cumsum(np.bincount(rows, minlength=n), out=Pp[1:])
    return Pp, cols[o].astype(np.int32), vals[o]


def invalid_split(n, nnzS, Sp, Sj, flags=0, has_prio=False, has_cf=True, overlap=False):
    """the reason bhs_csr_cfsplit_device refuses its arguments with BHS_ERR_INVALID_ARG, or None"""
    if flags & ~DEGREE and n >= 0 and nnzS >= 0:
        return "unknown flag"
    if flags & DEGREE and has_prio and n >= 0 and nnzS >= 0:
        return "degree keys with caller priorities"
    return ar.invalid(n, nnzS, Sp, Sj, 0, has_cf, overlap)


def invalid_interp(n, nnzA, Ap, Aj, nnzS, Sp, Sj, cf, nc, Pp=None, nnzP=None, flags=0, overlap=False, null=False):
    """the reason the interpolation calls refuse their arguments with BHS_ERR_INVALID_ARG, or None; Pp and nnzP: the numeric
    call's row pointer, compared with this module's"""
    if min(n, nnzA, nnzS, nc) < 0 or (nnzP is not None and nnzP < 0):
        return "negative size"
    if nc > n or (nnzP is not None and nnzP > 0x7FFFFFFF):
        return "size out of range"
    if flags != 0:
        return "unknown flag"
    if null:
        return "NULL array"
    if overlap:
        return "an output overlaps an input"
    for p, jj, nnz in ((Ap, Aj, nnzA), (Sp, Sj, nnzS)):
        why = ar.invalid(n, nnz, p, jj)
        if why:
            return why
        p = np.asarray(p, np.int64)
        jj = np.asarray(jj, np.int64)
        inner = np.ones(len(jj), bool)
        inner[p[:n][np.diff(p[:n + 1]) > 0]] = False                 # a row's first entry has no predecessor
        if np.any(inner[1:] & (np.diff(jj) <= 0)):
            return "a row that does not ascend strictly"
    cf = np.asarray(cf, np.int64)
    if n and (cf.min() < -1 or cf.max() >= nc):
        return "cf out of range"
    if Pp is not None:
        want = interp(n, Ap, Aj, np.ones(nnzA), Sp, Sj, cf)[0]
        if nnzP != want[n] or not np.array_equal(np.asarray(Pp)[:n + 1], want):
            return "rowPtrP is not this splitting's"
    return None


# ---------------------------------------------------------------- the hierarchy, in scipy
def rs_setup(A, theta=0.25, max_levels=10, min_coarse=40, seed=0):
    """levels [(A_l, P_l, R_l)], the last with P = R = None, and the coarse sizes: strength (aggref.strength) -> split with
    the degree keys and seed + 8 * level -> interp -> the Galerkin product on its structural pattern (aggref.on_pattern)"""
    import scipy.sparse as sp
    A = sp.csr_matrix(A, dtype=np.float64)
    A.sort_indices()
    levels, sizes = [], []
    while len(levels) + 1 < max_levels and A.shape[0] > min_coarse:
        n = A.shape[0]
        S = ar.strength(A, theta)
        cf, nc, _ = split(n, S.indptr, S.indices, seed + 8 * len(levels), None, True)
        if nc >= n:
            break
        Pp, Pj, Px = interp(n, A.indptr, A.indices, A.data, S.indptr, S.indices, cf)
        P = sp.csr_matrix((Px, Pj, Pp), shape=(n, nc))
        R = P.T.tocsr()
        R.sort_indices()
        levels.append((A, P, R))
        sizes.append(nc)
        A = ar.on_pattern(R @ (A @ P), ar._ones(R) @ (ar._ones(A) @ ar._ones(P)))
    levels.append((A, None, None))
    return levels, sizes


def pcg(levels, b, tol=1e-8, maxiter=200):
    """(x, iterations, residual norms): CG preconditioned with one Jacobi V(1,1) cycle from zero (aggref.vcycle), as
    amg.pcg_device runs it with smoother="jacobi" """
    A = levels[0][0]
    x = np.zeros_like(b)
    r = b.copy()
    res = [np.linalg.norm(r)]
    p, rz, its = None, 0.0, 0
    while res[-1] > tol * res[0] and its < maxiter:
        z = ar.vcycle(levels, r, np.zeros_like(r))
        rz_new = float(r @ z)
        p = z if p is None else z + (rz_new / rz) * p
        rz = rz_new
        q = A @ p
        alpha = rz / float(p @ q)
        x = x + alpha * p
        r = r - alpha * q
        res.append(np.linalg.norm(r))
        its += 1
    return x, its, res
