"""bhs_csr_levels_device, bhs_csr_trsv_device and bhs_csr_ilu0_device of include/bhsparse_hip.h ("triangular solve and
ILU(0)") restated in numpy: the reference of their tests, and the ILU(0)-preconditioned CG that
benchmark_spgemm_using_csr_amd/amg.py builds on top of them.

The levels come from the definition, row by row.  The solve sums a row as the device does: L lanes (1, 4, 16 or 64 by the
mean row length, as the colouring chooses them), lane `sub` the entries a + sub, a + sub + L, ... in double from +0, the L
sums meeting pairwise (lanes 0 and 1, 2 and 3, then those pairs, ...).  ILU(0) runs in the value type with double
intermediates, row by row, the entries k < i ascending."""
import numpy as np

import gsref as gr

LOWER, UPPER = "lower", "upper"


def lanes_per_row(n, nnz):
    """the library's choice from the mean row length (ag_lanes)"""
    mean = nnz / n if n else 0.0
    return 1 if mean <= 4.0 else 4 if mean <= 16.0 else 16 if mean <= 64.0 else 64


def levels(n, Ap, Aj, upper=False):
    """(level int32[n], nlevels, order int32[n], levelPtr int32[nlevels + 1]): level(i) = 0 without a counted entry (j < i for
    the lower triangle, j > i for the upper), else 1 + the greatest level among them; the rows by (level, index)"""
    Ap = np.asarray(Ap, np.int64)
    Aj = np.asarray(Aj, np.int64)
    level = np.zeros(n, np.int64)
    for i in (range(n - 1, -1, -1) if upper else range(n)):
        j = Aj[Ap[i]:Ap[i + 1]]
        j = j[j > i] if upper else j[j < i]
        if len(j):
            level[i] = 1 + level[j].max()
    if n == 0:
        return np.zeros(0, np.int32), 0, np.zeros(0, np.int32), np.zeros(1, np.int32)
    order, ptr = gr.order_of(level)
    return level.astype(np.int32), len(ptr) - 1, order, ptr


def lane_sum(terms, L):
    """the sum of `terms` (a row's products, 0 where an entry is not counted) as L lanes make it"""
    part = [0.0] * L
    for q, t in enumerate(terms):
        part[q % L] = part[q % L] + t
    while len(part) > 1:
        part = [part[2 * k] + part[2 * k + 1] for k in range(len(part) // 2)]
    return part[0]


def trsv(n, Ap, Aj, Ax, levelPtr, order, b, x, alpha=1.0, upper=False, unit_diag=False, dtype=np.float64, lanes=None):
    """The solve of the header on a copy of x (the caller's x where a row is not listed): for every level in turn and every
    listed row, s over the triangle's off-diagonal entries, t = (alpha b_i - s) / a_ii (the row's first diagonal entry; no
    division for a unit diagonal), one rounding to `dtype`.  Raises ValueError where a listed row lacks a diagonal entry."""
    Ap = np.asarray(Ap, np.int64)
    Aj = np.asarray(Aj, np.int64)
    Ax = np.asarray(Ax, dtype).astype(np.float64)
    b = np.asarray(b, dtype).astype(np.float64)
    x = np.array(x, dtype)
    L = lanes_per_row(n, len(Aj)) if lanes is None else lanes
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        for c in range(len(levelPtr) - 1):
            for i in order[levelPtr[c]:levelPtr[c + 1]]:
                j = Aj[Ap[i]:Ap[i + 1]]
                v = Ax[Ap[i]:Ap[i + 1]]
                take = (j > i) if upper else (j < i)
                xs = x[j].astype(np.float64)
                s = lane_sum([float(v[q] * xs[q]) if take[q] else 0.0 for q in range(len(j))], L)
                t = np.float64(alpha) * b[i] - np.float64(s)
                if not unit_diag:
                    dq = np.flatnonzero(j == i)
                    if len(dq) == 0:
                        raise ValueError("row %d has no diagonal entry" % i)
                    t = t / v[dq[0]]
                x[i] = dtype(t)
    return x


def ilu0(n, Ap, Aj, Ax, dtype=np.float64):
    """(values of L and U on A's pattern in `dtype`, pivot): rows strictly ascending, a diagonal entry in every row; row by
    row, for each entry k < i ascending l_ik = dtype(a_ik / u_kk) and a_ij = dtype(a_ij - l_ik u_kj) for every entry j > k of
    row i that row k also holds, the intermediates in double.  pivot: the smallest row whose u_ii is 0 or not finite, or -1."""
    Ap = np.asarray(Ap, np.int64)
    Aj = np.asarray(Aj, np.int64)
    val = np.array(Ax, dtype)
    pivot = -1
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        for i in range(n):
            a, e = Ap[i], Ap[i + 1]
            cols = Aj[a:e]
            assert np.all(np.diff(cols) > 0) and i in cols, "row %d" % i
            where = {int(j): a + q for q, j in enumerate(cols)}
            for q in range(a, e):
                k = int(Aj[q])
                if k >= i:
                    break
                ka, ke = Ap[k], Ap[k + 1]
                kd = ka + int(np.searchsorted(Aj[ka:ke], k))
                l = dtype(np.float64(val[q]) / np.float64(val[kd]))
                val[q] = l
                for p in range(kd + 1, ke):
                    at = where.get(int(Aj[p]))
                    if at is not None:
                        val[at] = dtype(np.float64(val[at]) - np.float64(l) * np.float64(val[p]))
            u = np.float64(val[where[i]])
            if pivot < 0 and (u == 0.0 or not np.isfinite(u)):
                pivot = i
    return val, pivot


def split(n, Ap, Aj, val):
    """(L with its unit diagonal, U) of ilu0's values as scipy CSR matrices in float64"""
    import scipy.sparse as sp
    r = np.repeat(np.arange(n), np.diff(Ap))
    v = np.asarray(val, np.float64)
    low = r > Aj
    Lm = sp.csr_matrix((v[low], (r[low], np.asarray(Aj)[low])), shape=(n, n)) + sp.identity(n, format="csr")
    Um = sp.csr_matrix((v[~low], (r[~low], np.asarray(Aj)[~low])), shape=(n, n))
    return Lm.tocsr(), Um.tocsr()


def identity_error(n, Ap, Aj, Ax, val):
    """max over the pattern of |(L U)_ij - a_ij| / ((m_ij + 2) (sum_k |l_ik| |u_kj| + |a_ij|)), m_ij the updates of the entry
    (the k < min(i, j) that row i holds and whose row holds j): what the factorisation lost, in units of the rounding unit"""
    import scipy.sparse as sp
    Lm, Um = split(n, Ap, Aj, val)
    r = np.repeat(np.arange(n), np.diff(Ap))
    c = np.asarray(Aj)
    a = np.asarray(Ax, np.float64)
    LU = (Lm @ Um).tocsr()
    mag = (abs(Lm) @ abs(Um)).tocsr()
    onesL = sp.csr_matrix((np.ones(int((r > c).sum())), (r[r > c], c[r > c])), shape=(n, n))
    onesU = sp.csr_matrix((np.ones(int((r < c).sum())), (r[r < c], c[r < c])), shape=(n, n))
    m = (onesL @ onesU).tocsr()
    got = np.asarray(LU[r, c]).ravel()
    scale = np.asarray(mag[r, c]).ravel() + np.abs(a)
    cnt = np.asarray(m[r, c]).ravel()
    return float(np.max(np.abs(got - a) / ((cnt + 2.0) * scale))), int(cnt.max())


# ---------------------------------------------------------------- ILU(0)-preconditioned CG, in scipy
def ilu0_setup(A, ordering="natural", seed=0):
    """what amg.ilu0_setup_device makes, on the host: (LU values' matrix parts, permutation or None, levels, colours)"""
    import scipy.sparse as sp
    import aggref as ar
    A = sp.csr_matrix(A)
    A.sort_indices()
    n = A.shape[0]
    perm, ncolors = None, 0
    if ordering == "colour":
        S = ar.strength(A, 0.0)
        _, ncolors, order, _, _ = gr.colouring(n, S.indptr, S.indices, seed)
        perm = order.astype(np.int64)
        A = A[perm][:, perm].tocsr()
        A.sort_indices()
    val, pivot = ilu0(n, A.indptr, A.indices, A.data)
    Lm, Um = split(n, A.indptr, A.indices, val)
    nlow = levels(n, A.indptr, A.indices)[1]
    nup = levels(n, A.indptr, A.indices, upper=True)[1]
    return {"L": Lm, "U": Um, "perm": perm, "nlevels": (nlow, nup), "ncolors": ncolors, "pivot": pivot}


def ilu0_apply(M, r):
    from scipy.sparse.linalg import spsolve_triangular
    y = r if M["perm"] is None else r[M["perm"]]
    y = spsolve_triangular(M["L"], y, lower=True, unit_diagonal=True)
    y = spsolve_triangular(M["U"], y, lower=False)
    if M["perm"] is None:
        return y
    z = np.empty_like(y)
    z[M["perm"]] = y
    return z


def pcg(A, b, precond=None, tol=1e-8, maxiter=100):
    """(x, iterations, residual norms of the recurrence): CG from x = 0, z = precond(r) (None: plain CG)"""
    x = np.zeros_like(b)
    r = b.copy()
    res = [np.linalg.norm(r)]
    p, rz, its = None, 0.0, 0
    while res[-1] > tol * res[0] and its < maxiter:
        z = r if precond is None else precond(r)
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


def ilu0_pcg(A, b, tol=1e-8, maxiter=100, ordering="colour", seed=0):
    M = ilu0_setup(A, ordering, seed)
    return pcg(A, b, lambda r: ilu0_apply(M, r), tol, maxiter)
