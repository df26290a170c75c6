"""bhs_csr_color_device and bhs_csr_gs_device of include/bhsparse_hip.h ("colouring and relaxation") restated in numpy: the
reference of their tests, and the Gauss-Seidel V-cycle and the preconditioned CG that benchmark_spgemm_using_csr_amd/amg.py
builds on top of them, in scipy.

The keys are the aggregation's (aggref.keys).  Three things are restated independently of each other: the first-fit greedy
colouring in descending key order by its definition (`greedy`), the synchronous rounds the library runs (`rounds`), and the
sweep, row by row in float64 (`sweep`; `sweep_by_colour` is the same map a colour at a time, for the cycles)."""
import numpy as np

import aggref as ar

FORWARD, BACKWARD, SYMMETRIC = "forward", "backward", "symmetric"


def neighbours(n, Sp, Sj):
    """per vertex the off-diagonal columns of its row (repeats kept: they make no difference)"""
    Sp = np.asarray(Sp, np.int64)
    Sj = np.asarray(Sj, np.int64)
    return [Sj[Sp[i]:Sp[i + 1]][Sj[Sp[i]:Sp[i + 1]] != i] for i in range(n)]


def first_free(taken):
    """the smallest colour >= 0 not among `taken`"""
    taken = set(int(t) for t in taken)
    c = 0
    while c in taken:
        c += 1
    return c


def greedy(n, Sp, Sj, key):
    """The definition: vertices from the greatest key down, each the smallest colour no off-diagonal neighbour coloured
    before it holds.  color int32[n]."""
    nb = neighbours(n, Sp, Sj)
    color = np.full(n, -1, np.int64)
    for v in np.argsort(key)[::-1]:
        near = color[nb[v]]
        color[v] = first_free(near[near >= 0])
    return color.astype(np.int32)


def rounds(n, Sp, Sj, key, counts=None):
    """The library's algorithm: (color int32[n], number of rounds).  A round colours every uncoloured vertex whose key
    exceeds that of each uncoloured off-diagonal neighbour, from the colours of the round before.  counts: a list that gets
    the number of uncoloured vertices every round starts from."""
    nb = neighbours(n, Sp, Sj)
    color = np.full(n, -1, np.int64)
    nrounds = 0
    while np.any(color < 0):
        assert nrounds <= n, "a round colours at least one vertex"
        new = color.copy()
        if counts is not None:
            counts.append(int((color < 0).sum()))
        for v in np.flatnonzero(color < 0):
            near = color[nb[v]]
            if np.any(key[nb[v]][near < 0] > key[v]):
                continue
            new[v] = first_free(near[near >= 0])
        assert np.any(new != color)
        color = new
        nrounds += 1
    return color.astype(np.int32), nrounds


def order_of(color):
    """(order int32[n], colorPtr int32[ncolors + 1]): the vertices by (colour, index) and every colour's first place"""
    color = np.asarray(color, np.int64)
    ncolors = int(color.max()) + 1 if len(color) else 0
    order = np.argsort(color, kind="stable").astype(np.int32)
    ptr = np.zeros(ncolors + 1, np.int32)
    np.cumsum(np.bincount(color, minlength=ncolors), out=ptr[1:])
    return order, ptr


def colouring(n, Sp, Sj, seed=0, prio=None, counts=None):
    """(color, ncolors, order, colorPtr, rounds): what bhs_csr_color_device returns (counts: see `rounds`)"""
    if n == 0:
        return np.zeros(0, np.int32), 0, np.zeros(0, np.int32), np.zeros(1, np.int32), 0
    color, nrounds = rounds(n, Sp, Sj, ar.keys(n, seed, prio), counts)
    order, ptr = order_of(color)
    return color, len(ptr) - 1, order, ptr, nrounds


def is_proper(n, Sp, Sj, color):
    r, c = ar.edges(n, Sp, Sj)
    off = r != c
    return not np.any(color[r[off]] == color[c[off]])


def passes(ncolors, direction):
    """the colours one sweep goes through, in order"""
    fwd = list(range(ncolors))
    return fwd if direction == FORWARD else fwd[::-1] if direction == BACKWARD else fwd + fwd[::-1]


def sweep(Ap, Aj, Ax, diag, colorPtr, order, b, x, omega=1.0, sweeps=1, direction=SYMMETRIC):
    """The update of the header, row by row in float64, on a copy of x: for every colour in turn and every listed row i of it
    s = sum_{j != i} a_ij x_j, t = (b_i - s) / d_i, x_i = t or x_i + omega (t - x_i)."""
    Ap = np.asarray(Ap, np.int64)
    Aj = np.asarray(Aj, np.int64)
    Ax = np.asarray(Ax, np.float64)
    x = np.array(x, np.float64)
    ncolors = len(colorPtr) - 1
    with np.errstate(divide="ignore", invalid="ignore"):
        for _ in range(sweeps):
            for c in passes(ncolors, direction):
                for i in order[colorPtr[c]:colorPtr[c + 1]]:
                    j = Aj[Ap[i]:Ap[i + 1]]
                    keep = j != i
                    s = float(np.sum(Ax[Ap[i]:Ap[i + 1]][keep] * x[j[keep]])) if keep.any() else 0.0
                    t = (np.float64(b[i]) - s) / np.float64(diag[i])
                    x[i] = t if omega == 1.0 else x[i] + omega * (t - x[i])
    return x


def sweep_by_colour(A, diag, colorPtr, order, b, x, omega=1.0, sweeps=1, direction=SYMMETRIC):
    """The same map a colour at a time (the rows of a colour of a proper colouring share no entry): A a scipy CSR matrix"""
    x = np.array(x, np.float64)
    ncolors = len(colorPtr) - 1
    for _ in range(sweeps):
        for c in passes(ncolors, direction):
            rows = order[colorPtr[c]:colorPtr[c + 1]]
            if len(rows) == 0:
                continue
            t = (b[rows] - (A[rows] @ x - A.diagonal()[rows] * x[rows])) / diag[rows]
            x[rows] = t if omega == 1.0 else x[rows] + omega * (t - x[rows])
    return x


def error_bound(Ap, Aj, Ax, diag, b, xs, steps, u):
    """steps * (maxrowlen + 4) * u * scale, scale = max_i (|b_i| + sum_j |a_ij| |x_j|) / |d_i| over the iterates xs: each
    update commits at most (len + 4) roundings of relative size u on terms bounded by scale, and a weakly diagonally dominant
    Gauss-Seidel map does not amplify what the updates before it committed"""
    import scipy.sparse as sp
    n = len(Ap) - 1
    absA = sp.csr_matrix((np.abs(np.asarray(Ax, np.float64)), Aj, Ap), shape=(n, n))
    scale = max(float(np.max((np.abs(b) + absA @ np.abs(x)) / np.abs(diag))) for x in xs)
    return steps * (int(np.diff(Ap).max()) + 4) * u * scale


# ---------------------------------------------------------------- the hierarchy's smoother, cycle and PCG, in scipy
def smoother_setup(levels, seed=0):
    """per level but the last: (diagonal, order, colorPtr) from the colouring of pattern(A) U pattern(A^T)"""
    out = []
    for A, P, _ in levels:
        if P is None:
            continue
        S = ar.strength(A, 0.0)
        n = A.shape[0]
        _, _, order, ptr, _ = colouring(n, S.indptr, S.indices, seed)
        out.append((A.diagonal(), order, ptr))
    return out


def vcycle_gs(levels, smoothers, b, x, pre=1, post=1, lvl=0):
    A, P, R = levels[lvl]
    if P is None:
        return np.linalg.solve(A.toarray(), b)
    d, order, ptr = smoothers[lvl]
    x = sweep_by_colour(A, d, ptr, order, b, x, 1.0, pre, FORWARD)
    xc = vcycle_gs(levels, smoothers, R @ (b - A @ x), np.zeros(P.shape[1]), pre, post, lvl + 1)
    x = x + P @ xc
    return sweep_by_colour(A, d, ptr, order, b, x, 1.0, post, BACKWARD)


def solve_gs(levels, smoothers, b, tol=1e-8, maxiter=100):
    """(x, cycles, residual norms)"""
    A = levels[0][0]
    x = np.zeros_like(b)
    res = [np.linalg.norm(b)]
    cycles = 0
    while res[-1] > tol * res[0] and cycles < maxiter:
        x = vcycle_gs(levels, smoothers, b, x)
        res.append(np.linalg.norm(b - A @ x))
        cycles += 1
    return x, cycles, res


def pcg(levels, smoothers, b, tol=1e-8, maxiter=100):
    """(x, iterations, residual norms of the recurrence): CG preconditioned with one Gauss-Seidel V(1,1) cycle from zero"""
    A = levels[0][0]
    x = np.zeros_like(b)
    r = b.copy()
    res = [np.linalg.norm(r)]
    p, rz, its = None, 0.0, 0
    while res[-1] > tol * res[0] and its < maxiter:
        z = vcycle_gs(levels, smoothers, r, np.zeros_like(r))
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
