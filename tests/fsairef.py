"""bhs_csr_fsai_device of include/bhsparse_hip.h ("approximate inverse") restated in numpy, bit for bit: the reference of
its tests, the matrices they share, the backward-error bound of a row, and the FSAI-preconditioned CG that
benchmark_spgemm_using_csr_amd/amg.py builds on top of it (on iluref.pcg).

A row of G is restated as the contract words it: the lower triangle of M = A(J, J) gathered from the examined part of A's
rows, the Cholesky factor column by column -- a column's update of the trailing triangle is ONE outer-product statement:
every element still takes one rounded product and one rounded difference per column, in ascending columns, so the bits
are those of any sharing of the work --, the solve of L^T g = e_d from the last unknown to the first, one rounding."""
import functools

import numpy as np

MAX_ROW = 128
SHORT_D, WAVE_D = 16, 64                                   # the bins' upper ends: fsai_short, fsai_wave (fsai_long: MAX_ROW)

# what bhs_csr_fsai_device refuses on the host (each BHS_ERR_INVALID_ARG, valG untouched), by the word invalid() gives
HOST_REFUSALS = ("negative size", "flags != 0", "NULL array", "nnzG < n", "valG overlaps an input")
# ... and on the device
DEVICE_REFUSALS = ("rowPtrG", "empty row of G", "row of G longer than 128", "column of G outside [0, i]", "row of G not ascending",
                   "row of G does not end in i", "rowPtrA", "column of A out of range", "row of A not ascending")


def examined(n, Ap, Aj, nnzA, j):
    """(word or None, positions) of row j of A: the entries up to and including the first whose column is >= j, each checked
    against its predecessor and the range"""
    ra, re = int(Ap[j]), int(Ap[j + 1])
    if ra < 0 or re < ra or re > nnzA:
        return "rowPtrA", range(0)
    for q in range(ra, re):
        c = int(Aj[q])
        if c < 0 or c >= n:
            return "column of A out of range", range(0)
        if q > ra and c <= int(Aj[q - 1]):
            return "row of A not ascending", range(0)
        if c >= j:
            return None, range(ra, q + 1)
    return None, range(ra, re)


def row_of_g_wrong(i, cols):
    """the word for row i of G with these columns, or None"""
    d = len(cols)
    if d < 1:
        return "empty row of G"
    if d > MAX_ROW:
        return "row of G longer than 128"
    cols = np.asarray(cols, np.int64)
    if np.any(cols < 0) or np.any(cols > i):
        return "column of G outside [0, i]"
    if np.any(np.diff(cols) <= 0):
        return "row of G not ascending"
    if cols[-1] != i:
        return "row of G does not end in i"
    return None


def invalid(n, Ap, Aj, Gp, Gj, flags=0, nnzA=None, nnzG=None, null=False, overlap=False):
    """the word of the first refusal of the call (the host's, then the device's by row), or None for a call that succeeds"""
    nnzA = (len(Aj) if Aj is not None else 0) if nnzA is None else nnzA
    nnzG = (len(Gj) if Gj is not None else 0) if nnzG is None else nnzG
    if n < 0 or nnzA < 0 or nnzG < 0:
        return "negative size"
    if flags != 0:
        return "flags != 0"
    if nnzG < n:
        return "nnzG < n"
    if n > 0 and (null or any(a is None for a in (Ap, Aj, Gp, Gj))):
        return "NULL array"
    if overlap:
        return "valG overlaps an input"
    if n == 0:
        return None
    Gp = np.asarray(Gp, np.int64)
    if Gp[0] != 0 or Gp[n] != nnzG or np.any(Gp[:n + 1] < 0) or np.any(np.diff(Gp[:n + 1]) < 0) or np.any(Gp[:n + 1] > nnzG):
        return "rowPtrG"
    for i in range(n):
        word = row_of_g_wrong(i, Gj[Gp[i]:Gp[i + 1]])
        if word:
            return word
    for i in range(n):
        for j in Gj[Gp[i]:Gp[i + 1]]:
            word, _ = examined(n, Ap, Aj, nnzA, int(j))
            if word:
                return word
    return None


def row_matrix(n, Ap, Aj, Ax64, J):
    """the lower triangle of M = A(J, J) as a dense d x d array of doubles (+0 where A holds no entry; the upper triangle 0)"""
    d = len(J)
    where = {int(j): q for q, j in enumerate(J)}
    M = np.zeros((d, d))
    for p, j in enumerate(J):
        word, at = examined(n, Ap, Aj, len(Aj), int(j))
        if word:
            raise ValueError(word)
        for k in at:
            q = where.get(int(Aj[k]))
            if q is not None and q <= p:
                M[p, q] = Ax64[k]
    return M


def row_solve(M):
    """(L, g, bad) of one row: steps 1 and 2 of the contract on the lower triangle of M, all in double; bad: some pivot was
    not > 0 or not finite when its root was taken"""
    d = M.shape[0]
    L = np.tril(M).astype(np.float64)
    bad = False
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        for c in range(d):
            mcc = L[c, c]
            if not (mcc > 0.0) or not np.isfinite(mcc):
                bad = True
            lcc = np.sqrt(mcc)
            col = L[c + 1:, c] / lcc
            L[c + 1:, c] = col
            L[c, c] = lcc
            if c + 1 < d:
                prod = np.outer(col, col)                       # l_rc * l_c'c, rounded
                L[c + 1:, c + 1:] = L[c + 1:, c + 1:] - np.tril(prod)   # (the upper triangle takes - 0: it stays +0)
        t = np.zeros(d)
        t[d - 1] = 1.0
        g = np.zeros(d)
        for q in range(d - 1, -1, -1):
            g[q] = t[q] / L[q, q]
            prod = L[q, :q] * g[q]
            t[:q] = t[:q] - prod
    return L, g, bad


def fsai(n, Ap, Aj, Ax, Gp, Gj, dtype=np.float64, keep=False):
    """(valG in `dtype`, bad_row) -- and, with keep, the rows' (J, M, L) -- of the call on valid arrays (ValueError with the
    refusal's word otherwise)"""
    Ap, Aj = np.asarray(Ap, np.int64), np.asarray(Aj, np.int64)
    Gp, Gj = np.asarray(Gp, np.int64), np.asarray(Gj, np.int64)
    Ax64 = np.asarray(Ax, dtype).astype(np.float64)
    word = invalid(n, Ap, Aj, Gp, Gj)
    if word:
        raise ValueError(word)
    val = np.zeros(len(Gj), dtype)
    bad_row, kept = -1, []
    for i in range(n):
        J = Gj[Gp[i]:Gp[i + 1]]
        M = row_matrix(n, Ap, Aj, Ax64, J)
        L, g, bad = row_solve(M)
        with np.errstate(over="ignore", invalid="ignore"):
            val[Gp[i]:Gp[i + 1]] = g.astype(dtype)
        if bad and bad_row < 0:
            bad_row = i
        if keep:
            kept.append((J, M, L))
    return (val, bad_row, kept) if keep else (val, bad_row)


def same_bits(a, b):
    """equal bits, NaN in the same places (which NaN an operation returns is the machine's choice, not the rule's)"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    u = np.uint32 if a.dtype == np.float32 else np.uint64
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(a.view(u)[~na], b.view(u)[~nb]))


def ulp_distance(a, b):
    """the largest distance of two arrays of one float type in units of the last place (finite values of one sign pattern)"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    s = np.int32 if a.dtype == np.float32 else np.int64
    ka, kb = a.view(s).astype(np.int64), b.view(s).astype(np.int64)
    lo = np.int64(np.iinfo(s).min)
    ka = np.where(ka < 0, lo - ka, ka)
    kb = np.where(kb < 0, lo - kb, kb)
    return int(np.abs(ka - kb).max()) if len(ka) else 0


# ---------------------------------------------------------------- the backward-error bound of a row
def row_error_over_bound(M, L, g, dtype=np.float64):
    """max over the components of |M g - e_d / g_d| / bound, in np.longdouble, for a computed row g (values of `dtype`) of
    the symmetric M given by its lower triangle and the restatement's factor L:
        bound = (2 d + 3) 2^-53 (|L| |L^T| |g|) + 2^-53 |1 / g_d| e_d      [+ 2^-24 (|M| |g| + |1 / g_d| e_d) in float]
    -- the backward error of a Cholesky factorisation (d + 1 units on |L| |L^T|) plus one triangular solve (d + 2 units)
    carried to the product, and the rounding of the right side's division."""
    ld = np.longdouble
    d = M.shape[0]
    Ms = np.tril(M) + np.tril(M, -1).T
    g = np.asarray(g, np.float64).astype(ld)
    e = np.zeros(d, ld)
    e[d - 1] = 1
    rhs = e / g[d - 1]
    resid = np.abs(Ms.astype(ld) @ g - rhs)
    aL = np.abs(np.tril(L)).astype(ld)
    u = ld(2.0) ** -53
    lim = (2 * d + 3) * u * (aL @ (aL.T @ np.abs(g))) + u * np.abs(rhs)
    if np.dtype(dtype) == np.dtype(np.float32):
        lim = lim + ld(2.0) ** -24 * (np.abs(Ms).astype(ld) @ np.abs(g) + np.abs(rhs))
    return float((resid / lim).max())


def worst_error_over_bound(Gp, val, kept, dtype=np.float64):
    """the largest row_error_over_bound over the rows of a call: val the computed values, kept what fsai(keep=True) returned"""
    return max(row_error_over_bound(M, L, val[Gp[i]:Gp[i + 1]], dtype) for i, (_, M, L) in enumerate(kept))


# ---------------------------------------------------------------- the matrices of the tests
BLOCKS = (1, 2, 15, 16, 17, 63, 64, 65, 127, 128)          # every bin's two ends


def block_patterns(orders=BLOCKS):
    """(n, Ap, Aj, Gp, Gj, starts): block diagonal with dense blocks of these orders -- A full, G the blocks' lower triangles"""
    n = int(sum(orders))
    Ap, Aj, Gp, Gj, starts = [0], [], [0], [], []
    s = 0
    for k in orders:
        starts.append(s)
        for r in range(k):
            Aj.extend(range(s, s + k))
            Ap.append(len(Aj))
            Gj.extend(range(s, s + r + 1))
            Gp.append(len(Gj))
        s += k
    return n, np.array(Ap, np.int32), np.array(Aj, np.int32), np.array(Gp, np.int32), np.array(Gj, np.int32), starts


@functools.lru_cache(maxsize=None)
def exact_family(seed=0):
    """(n, Ap, Aj, Ax, Gp, Gj, starts): A = L0 L0^T on block_patterns(), L0 with 1, 2 or 4 on its diagonal and multiples of
    1/8 in [-3/8, 3/8] below.  Every entry of A is a multiple of 1/64 below 2^11, every root and every division of the
    factorisation is by a power of two, and the factor comes back exactly -- in double and in float."""
    rng = np.random.default_rng(seed)
    n, Ap, Aj, Gp, Gj, starts = block_patterns()
    Ax = []
    for k in BLOCKS:
        L0 = np.tril(rng.integers(-3, 4, (k, k)) / 8.0, -1) + np.diag(2.0 ** rng.integers(0, 3, k))
        Ax.append((L0 @ L0.T).ravel())
    return n, Ap, Aj, np.concatenate(Ax), Gp, Gj, starts


def grid(name):
    """(n, Ap, Aj, Ax) of poisson5pt_33, poisson27pt_9 or aniso_33 (eps = 1/64), rows ascending"""
    import aggref
    import matchref
    if name == "aniso_33":
        A = matchref.aniso(33, 33, 1.0 / 64)
        return A.shape[0], A.indptr.astype(np.int32), A.indices.astype(np.int32), A.data.astype(np.float64)
    return aggref.poisson(*{"poisson5pt_33": ("poisson5pt", 33, 33), "poisson27pt_9": ("poisson27pt", 9, 9, 9)}[name])


def csr(n, Ap, Aj, Ax):
    import scipy.sparse as sp
    return sp.csr_matrix((np.asarray(Ax, np.float64), np.asarray(Aj), np.asarray(Ap)), shape=(n, n))


def tril_pattern(n, Ap, Aj, power=1):
    """(Gp, Gj) int32: the pattern of tril(A^power), rows ascending"""
    import scipy.sparse as sp
    P = sp.csr_matrix((np.ones(len(Aj)), np.asarray(Aj), np.asarray(Ap)), shape=(n, n))
    Q = P
    for _ in range(power - 1):
        Q = (Q @ P).tocsr()
    Q = sp.tril(Q).tocsr()
    Q.sort_indices()
    return Q.indptr.astype(np.int32), Q.indices.astype(np.int32)


@functools.lru_cache(maxsize=None)
def random_spd(seed=1):
    """(n, Ap, Aj, Ax) on the pattern of poisson27pt_9: symmetric off-diagonals drawn in (-1, 0), diagonal = the sum of
    their magnitudes + 1 (strictly diagonally dominant: SPD)"""
    import scipy.sparse as sp
    n, Ap, Aj, _ = grid("poisson27pt_9")
    rng = np.random.default_rng(seed)
    r = np.repeat(np.arange(n), np.diff(Ap))
    low = r > Aj
    v = -rng.uniform(0.0, 1.0, int(low.sum()))
    v[v == 0.0] = -0.5
    Lw = sp.csr_matrix((v, (r[low], Aj[low])), shape=(n, n))
    S = (Lw + Lw.T).tocsr()
    S = (S + sp.diags(np.asarray(abs(S).sum(axis=1)).ravel() + 1.0)).tocsr()
    S.sort_indices()
    assert np.array_equal(S.indptr, Ap) and np.array_equal(S.indices, Aj)
    return n, Ap, Aj, S.data.copy()


def with_extra_lower(n, Gp, Gj, seed, per_row=3):
    """(Gp, Gj) with up to per_row more columns below the diagonal in every row, ascending, no row beyond MAX_ROW"""
    rng = np.random.default_rng(seed)
    p, j = [0], []
    for i in range(n):
        cols = set(int(c) for c in Gj[Gp[i]:Gp[i + 1]])
        room = MAX_ROW - len(cols)
        if i > 0 and room > 0:
            cols |= set(int(c) for c in rng.integers(0, i, min(per_row, room)))
        j.extend(sorted(cols))
        p.append(len(j))
    return np.array(p, np.int32), np.array(j, np.int32)


# ---------------------------------------------------------------- FSAI-preconditioned CG, in scipy
def fsai_matrix(n, Gp, Gj, val):
    return csr(n, Gp, Gj, val)


def fsai_pcg(A, b, tol=1e-8, maxiter=100, pattern=None):
    """what amg.fsai_pcg_device does, on the host: G from the restatement on `pattern` (None: tril(A)), z = G^T (G r)"""
    import scipy.sparse as sp
    import iluref
    A = sp.csr_matrix(A)
    A.sort_indices()
    n = A.shape[0]
    Gp, Gj = tril_pattern(n, A.indptr, A.indices) if pattern is None else pattern
    val, _ = fsai(n, A.indptr, A.indices, A.data, Gp, Gj)
    G = fsai_matrix(n, Gp, Gj, val)
    Gt = G.T.tocsr()
    return iluref.pcg(A, b, lambda r: Gt @ (G @ r), tol, maxiter)


def jacobi_pcg(A, b, tol=1e-8, maxiter=100):
    import iluref
    d = A.diagonal()
    return iluref.pcg(A, b, lambda r: r / d, tol, maxiter)
