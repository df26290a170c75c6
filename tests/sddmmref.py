"""bhs_csr_sddmm_device of include/bhsparse_hip.h ("sampled dense-dense product") restated in numpy, bit for bit, and the
affinity strength of connection built on it (amg.affinity_strength_device) with numpy products: the reference of their
tests.

M is an m x n CSR pattern whose rows need not be ascending and may hold duplicate (row, column) pairs, each with a value of
its own; X is m x k, Y n x k.  Inputs are rounded to the build's value type first and everything after that is float64,
every operation rounded by itself (numpy never contracts): with T = min(64, the smallest power of two >= k), T partial
sums from +0, sequential over the tiles of T columns (s_l = s_l + x * y); then the adjacent-pair tree over the T sums --
what the butterfly xor 1, 2, .. T / 2 computes in every lane, an IEEE addition being commutative --; s = s * m under
times_m; t = alpha * s; t = t + beta * z only where beta != 0 (z is then never looked at); one rounding to the value
type."""
import numpy as np

# the arguments bhs_csr_sddmm_device refuses on the host (each BHS_ERR_INVALID_ARG, valZ untouched), by the word invalid() gives
HOST_REFUSALS = ("negative size", "k < 1", "ldX < k", "ldY < k", "NULL rowPtrM", "NULL colIndM", "NULL X", "NULL Y", "NULL valZ",
                 "NULL valM under TIMES_M", "unknown flag bits", "valZ overlaps an input")
# what the device's validation refuses
DEVICE_REFUSALS = ("rowPtrM[0] != 0", "rowPtrM[m] != nnzM", "decreasing rowPtrM", "column of M out of range")

TIMES_M = 1


def tile(k):
    """T = min(64, the smallest power of two >= k)"""
    T = 1
    while T < k and T < 64:
        T *= 2
    return T


def invalid(m, n, Mp, Mj, k=1, ldX=None, ldY=None, flags=0, has_x=True, has_y=True, has_z=True, has_valm=True, overlap=False,
            nnz=None):
    """What the call must refuse: a word for the first reason found (one of HOST_REFUSALS, then DEVICE_REFUSALS), or None
    for a legal call.  Mp / Mj None stand for NULL pointers; nnzM is len(Mj), or `nnz` where it is given (a NULL colIndM
    has no length)."""
    if nnz is None:
        nnz = 0 if Mj is None else len(Mj)
    ldX, ldY = (k if ldX is None else ldX), (k if ldY is None else ldY)
    if m < 0 or n < 0 or nnz < 0:
        return "negative size"
    if k < 1:
        return "k < 1"
    if ldX < k:
        return "ldX < k"
    if ldY < k:
        return "ldY < k"
    if flags & ~TIMES_M:
        return "unknown flag bits"
    if Mp is None:
        return "NULL rowPtrM"
    if Mj is None and nnz > 0:
        return "NULL colIndM"
    if not has_x and nnz > 0:
        return "NULL X"
    if not has_y and nnz > 0:
        return "NULL Y"
    if not has_z and nnz > 0:
        return "NULL valZ"
    if (flags & TIMES_M) and not has_valm and nnz > 0:
        return "NULL valM under TIMES_M"
    if overlap:
        return "valZ overlaps an input"
    Mp = np.asarray(Mp, np.int64)
    if len(Mp) != m + 1 or Mp[0] != 0:
        return "rowPtrM[0] != 0"
    if Mp[-1] != nnz:
        return "rowPtrM[m] != nnzM"
    if np.any(np.diff(Mp) < 0) or np.any(Mp < 0) or np.any(Mp > nnz):
        return "decreasing rowPtrM"
    Mj = np.asarray([] if Mj is None else Mj, np.int64)
    if nnz and (Mj.min() < 0 or Mj.max() >= n):
        return "column of M out of range"
    return None


def _dense(X, rows, dtype):
    X = np.asarray(X)
    X = X.reshape(rows, -1) if X.ndim != 2 else X
    return np.ascontiguousarray(X, dtype).astype(np.float64)


def sddmm(m, n, Mp, Mj, Mx, X, Y, alpha=1.0, beta=0.0, Z=None, times_m=False, dtype=np.float64):
    """Z's values (len(Mj) of them) in `dtype`.  Mx may be None without times_m, Z may be None when beta == 0."""
    x, y = _dense(X, m, dtype), _dense(Y, n, dtype)
    k = x.shape[1]
    assert invalid(m, n, Mp, Mj, k) is None and x.shape[0] == m and y.shape == (n, k)
    Mp, Mj = np.asarray(Mp, np.int64), np.asarray(Mj, np.int64)
    rows = np.repeat(np.arange(m, dtype=np.int64), np.diff(Mp))
    T = tile(k)
    alpha, beta = np.float64(alpha), np.float64(beta)
    with np.errstate(all="ignore"):
        s = np.zeros((len(Mj), T), np.float64)
        for t0 in range(0, k, T):                                    # sequential over the tiles: product rounded, sum rounded
            w = min(T, k - t0)
            p = x[rows, t0:t0 + w] * y[Mj, t0:t0 + w]
            s[:, :w] = s[:, :w] + p
        while s.shape[1] > 1:                                        # the adjacent-pair tree
            s = s[:, 0::2] + s[:, 1::2]
        s = s[:, 0]
        if times_m:
            s = s * np.ascontiguousarray(Mx, dtype).astype(np.float64)
        t = alpha * s
        if beta != 0.0:
            bz = beta * np.ascontiguousarray(Z, dtype).astype(np.float64)
            t = t + bz
        return t.astype(dtype)


def same_bits(a, b):
    """the same value bits, NaN in the same places (a NaN's sign and payload are the machine's, not the rule's)"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    u = np.uint32 if a.dtype == np.float32 else np.uint64
    return bool(np.array_equal(na, nb) and np.array_equal(a[~na].view(u), b[~nb].view(u)))


# ---------------------------------------------------------------- the affinity strength of connection
def affinity_values(A, vectors=16, sweeps=8, omega=2.0 / 3.0, seed=0):
    """c_ij = (x_i . x_j)^2 / ((x_i . x_i) (x_j . x_j)) on pattern(A) from `vectors` start vectors after `sweeps` weighted
    Jacobi sweeps on A x = 0 (Livne and Brandt's affinity): the steps of amg.affinity_strength_device, the product A X in
    numpy.  A: scipy CSR with sorted rows.  Returns c in A's entry order."""
    from benchmark_spgemm_using_csr_amd.amg import _start_vector
    n = A.shape[0]
    Ap, Aj = A.indptr.astype(np.int64), A.indices.astype(np.int64)
    X = np.stack([_start_vector(n, seed + c) for c in range(vectors)], axis=1)
    d = A.diagonal()
    for _ in range(sweeps):
        X = X - omega * ((A @ X) / d[:, None])
    g = sddmm(n, n, Ap, Aj, None, X, X)
    g2 = sddmm(n, n, Ap, Aj, g, X, X, times_m=True)
    dd = sddmm(n, n, np.arange(n + 1), np.arange(n), None, X, X)
    rows = np.repeat(np.arange(n), np.diff(Ap))
    return g2 / dd[rows] / dd[Aj] * 1.0


def kept(A, theta):
    """what the strength rule itself keeps, before its union with the transpose: the diagonal and every a_ij unless
    |a_ij| < theta * max_{k != i} |a_ik| (scipy CSR of ones)"""
    import scipy.sparse as sp
    A = sp.csr_matrix(A)
    n = A.shape[0]
    r = np.repeat(np.arange(n), np.diff(A.indptr))
    diag = r == A.indices
    rowmax = np.zeros(n)
    np.maximum.at(rowmax, r[~diag], np.abs(A.data[~diag]))
    keep = ~(np.abs(A.data) < theta * rowmax[r]) | diag
    S = sp.csr_matrix((np.ones(int(keep.sum())), (r[keep], A.indices[keep])), shape=(n, n))
    S.sort_indices()
    return S


def affinity_matrix(A, vectors=16, sweeps=8, omega=2.0 / 3.0, seed=0):
    """affinity_values on A's pattern as a scipy CSR matrix"""
    import scipy.sparse as sp
    A = sp.csr_matrix(A)
    A.sort_indices()
    return sp.csr_matrix((affinity_values(A, vectors, sweeps, omega, seed), A.indices, A.indptr), shape=A.shape)


def affinity_strength(A, theta=0.5, vectors=16, sweeps=8, omega=2.0 / 3.0, seed=0):
    """the symmetric pattern of strong connections by affinity: aggref.strength's rule (kept(), united with its transpose)
    on affinity_matrix (scipy CSR)"""
    import aggref
    return aggref.strength(affinity_matrix(A, vectors, sweeps, omega, seed), theta)


def scaled(A, seed=5):
    """D A D with D = 2 ** default_rng(seed).integers(-3, 4, n): a symmetric diagonal scaling by powers of two"""
    import scipy.sparse as sp
    n = A.shape[0]
    D = sp.diags(2.0 ** np.random.default_rng(seed).integers(-3, 4, n))
    B = (D @ sp.csr_matrix(A) @ D).tocsr()
    B.sort_indices()
    return B


def not_x_neighbours(Sp, Sj, nx, ny):
    """the share of the rows of an nx x ny grid's pattern whose off-diagonal set is anything but the row's x-neighbours"""
    n = nx * ny
    differ = 0
    for i in range(n):
        got = set(int(j) for j in Sj[Sp[i]:Sp[i + 1]]) - {i}
        want = set(j for j in (i - 1, i + 1) if 0 <= j < n and j // nx == i // nx)
        differ += got != want
    return differ / float(n)
