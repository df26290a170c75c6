"""bhs_csr_match_device of include/bhsparse_hip.h ("matching") restated in numpy: the reference of its tests, and the scipy
restatement of the pairwise aggregation and the hierarchy that benchmark_spgemm_using_csr_amd/amg.py builds on top of it.

An entry (i, j) of row i is an edge seen from i where j != i, w = |a_ij| > 0 and w is not NaN; without values every weight is
1.  The key of an edge is (w, h(lo, hi), lo, hi), lo = min(i, j), hi = max(i, j), h = mix(mix(lo ^ seed) ^ hi) with the
aggregation's finaliser (aggref.hash32(x, seed) is mix(x ^ seed)).  Three things are restated independently of each other:
the synchronous rounds the library runs (`rounds`), the greedy matching in descending key order by its definition
(`greedy`), and the numbering (`number`)."""
import numpy as np

import aggref as ar


def edge_hash(lo, hi, seed):
    return ar.hash32(ar.hash32(lo, seed) ^ np.asarray(hi, np.uint64), 0)


def weight_bits(w):
    """a non-negative IEEE number's bit pattern read as an unsigned integer preserves order (+Inf above every finite one)"""
    return np.ascontiguousarray(w, np.float64).view(np.uint64)


def seen_edges(n, Ap, Aj, Ax):
    """(row, column, weight) of every entry that is an edge seen from its row"""
    r, c = ar.edges(n, Ap, Aj)
    Ap = np.asarray(Ap, np.int64)
    w = np.ones(len(c)) if Ax is None else np.abs(np.asarray(Ax, np.float64)[Ap[0]:Ap[n]])
    with np.errstate(invalid="ignore"):
        keep = (r != c) & (w > 0)                                    # (NaN > 0 is false)
    return r[keep], c[keep], w[keep]


def rounds(n, Ap, Aj, Ax=None, seed=0, counts=None):
    """The library's algorithm: (mate int32[n], npairs, productive rounds).  mate is -1 undecided, i finally unmatched, j
    matched with j.  The entries are sorted once by (row, key seen from the row); a round takes, per undecided row, the last
    entry whose other end is undecided -- its proposal -- and accepts the mutual ones.  Entries with a decided end never
    come back and are dropped from the list as the rounds go.  counts: a list that gets the number of undecided vertices
    every round starts from (no round starts from none) and, where the last round leaves some, their number."""
    if n == 0:
        return np.zeros(0, np.int32), 0, 0
    r, c, w = seen_edges(n, Ap, Aj, Ax)
    h = edge_hash(np.minimum(r, c), np.maximum(r, c), seed)
    order = np.lexsort((c, h, weight_bits(w), r))                    # within a row: (w, h, the greater other endpoint)
    r, c = r[order], c[order]
    mate = np.full(n, -1, np.int64)
    me = np.arange(n)
    npairs = nrounds = 0
    while True:
        assert nrounds <= n // 2, "a productive round makes a pair"
        und = mate < 0
        if counts is not None and und.any():
            counts.append(int(und.sum()))
        live = und[r] & und[c]
        r, c = r[live], c[live]
        cand = np.full(n, -1, np.int64)
        if len(r):
            last = np.flatnonzero(np.append(r[1:] != r[:-1], True))  # the last live entry of every row that has one
            cand[r[last]] = c[last]
        alone = und & (cand < 0)
        mutual = und & (cand >= 0)
        mutual[mutual] = cand[cand[mutual]] == me[mutual]
        mate[alone] = me[alone]
        mate[mutual] = cand[mutual]
        made = int(mutual.sum()) // 2
        if made == 0:
            break
        npairs += made
        nrounds += 1
    left = mate < 0                                                  # (only where pattern or weights are not symmetric)
    if counts is not None and left.any():
        counts.append(int(left.sum()))
    mate[left] = me[left]
    return mate.astype(np.int32), npairs, nrounds


def greedy(n, Ap, Aj, Ax=None, seed=0):
    """The definition, for a symmetric input: the undirected edges (of a repeated one the greatest weight) in descending key
    order, an edge is taken where both its ends are free.  mate int32[n]."""
    r, c, w = seen_edges(n, Ap, Aj, Ax)
    lo, hi = np.minimum(r, c), np.maximum(r, c)
    heaviest = {}
    for a, b, x in zip(lo.tolist(), hi.tolist(), w.tolist()):
        if x > heaviest.get((a, b), 0.0):
            heaviest[(a, b)] = x
    keyed = sorted(((x, int(edge_hash(a, b, seed)), a, b) for (a, b), x in heaviest.items()), reverse=True)
    mate = np.arange(n, dtype=np.int32)
    free = np.ones(n, bool)
    for _, _, a, b in keyed:
        if free[a] and free[b]:
            mate[a], mate[b] = b, a
            free[a] = free[b] = False
    return mate


def number(mate):
    """(agg int32[n], nagg): pairs and singletons numbered by ascending leader min(i, mate[i])"""
    mate = np.asarray(mate, np.int64)
    me = np.arange(len(mate))
    leads = mate >= me
    rank = np.cumsum(leads) - 1
    return rank[np.minimum(me, mate)].astype(np.int32), int(leads.sum())


def match(n, Ap, Aj, Ax=None, seed=0, counts=None):
    """(mate, agg, nagg, npairs, rounds): what bhs_csr_match_device returns (counts: see `rounds`)"""
    mate, npairs, nrounds = rounds(n, Ap, Aj, Ax, seed, counts)
    agg, nagg = number(mate)
    assert nagg == n - npairs
    return mate, agg, nagg, npairs, nrounds


def is_matching(mate):
    mate = np.asarray(mate, np.int64)
    return bool(np.all((mate >= 0) & (mate < len(mate))) and np.array_equal(mate[mate], np.arange(len(mate))))


# ---------------------------------------------------------------- pairwise aggregation and its hierarchy, in scipy
def pairwise(A, passes=2, seed=0):
    """(agg int32[n], nagg): pass p matches the current matrix with seed + p, the matrix is coarsened with the unit tentative
    prolongator of the pairs (T^T A T) and the aggregates are composed; stops early where a pass matches nothing"""
    import scipy.sparse as sp
    if not 1 <= passes <= 4:
        raise ValueError("passes is 1, 2, 3 or 4")
    A = sp.csr_matrix(A, dtype=np.float64)
    n = m = A.shape[0]
    agg = np.arange(n, dtype=np.int32)
    for p in range(passes):
        _, agg_p, nagg, npairs, _ = match(m, A.indptr, A.indices, A.data, seed + p)
        if npairs == 0:
            break
        agg = agg_p[agg]
        if p + 1 < passes:
            T = sp.csr_matrix((np.ones(m), agg_p, np.arange(m + 1)), shape=(m, nagg))
            A = (T.T @ A @ T).tocsr()
        m = nagg
    return agg.astype(np.int32), m


def numbered_by_smallest_member(agg, nagg):
    """are the aggregates numbered by ascending smallest member"""
    first = np.full(nagg, len(agg), np.int64)
    np.minimum.at(first, agg, np.arange(len(agg)))
    return bool(np.all(first < len(agg)) and np.all(np.diff(first) > 0))


def pa_setup(A, passes=2, omega=2.0 / 3.0, max_levels=10, min_coarse=40, seed=0):
    """aggref.sa_setup with pairwise aggregation, level l with seed + 8 l: (levels, aggregate counts, the levels'
    aggregates)"""
    import scipy.sparse as sp
    A = sp.csr_matrix(A, dtype=np.float64)
    levels, sizes, aggs = [], [], []
    while len(levels) + 1 < max_levels and A.shape[0] > min_coarse:
        n = A.shape[0]
        agg, nagg = pairwise(A, passes, seed + 8 * len(levels))
        if nagg >= n:
            break
        T, _ = ar.tentative(n, np.asarray(agg, np.int64), nagg)
        Dinv = sp.diags(1.0 / A.diagonal())
        P = ar.on_pattern(T - omega * (Dinv @ A @ T), ar._ones(T) + ar._ones(A) @ ar._ones(T))
        R = P.T.tocsr()
        R.sort_indices()
        levels.append((A, P, R))
        sizes.append(nagg)
        aggs.append(agg)
        A = ar.on_pattern(R @ (A @ P), ar._ones(R) @ (ar._ones(A) @ ar._ones(P)))
    levels.append((A, None, None))
    return levels, sizes, aggs


def pcg(levels, b, tol=1e-8, maxiter=500):
    """CG on A_0 x = b preconditioned with one Jacobi V(1,1) cycle (aggref.vcycle): (x, iterations)"""
    A = levels[0][0]
    x = np.zeros_like(b)
    r = b.copy()
    nb = np.linalg.norm(b)
    p, rz, its = None, 0.0, 0
    while np.linalg.norm(r) > tol * nb and its < maxiter:
        z = ar.vcycle(levels, r, np.zeros_like(r))
        rz_new = float(r @ z)
        p = z if p is None else z + (rz_new / rz) * p
        rz = rz_new
        q = A @ p
        alpha = rz / float(p @ q)
        x = x + alpha * p
        r = r - alpha * q
        its += 1
    return x, its


# ---------------------------------------------------------------- the test inputs
def increasing_path(n=200):
    """a path whose edge {k, k + 1} weighs k + 1: one pair a round from the heavy end, n / 2 rounds"""
    import scipy.sparse as sp
    k = np.arange(n - 1)
    A = sp.coo_matrix((np.r_[k + 1.0, k + 1.0], (np.r_[k, k + 1], np.r_[k + 1, k])), shape=(n, n)).tocsr()
    return n, A.indptr.astype(np.int32), A.indices.astype(np.int32), A.data.copy()


def by_hand():
    """rows {(0,1) NaN, (0,2) 0, (0,3) +Inf}, {(1,0) NaN, (1,2) -2}, {(2,0) -0, (2,1) 2}, {(3,0) -Inf}: 0 -- 3 through the
    infinite weight, 1 -- 2 through |-2| = 2, in one round; NaN and the zeros are no connections"""
    Ap = np.array([0, 3, 5, 7, 8], np.int32)
    Aj = np.array([1, 2, 3, 0, 2, 0, 1, 0], np.int32)
    Ax = np.array([np.nan, 0.0, np.inf, np.nan, -2.0, -0.0, 2.0, -np.inf])
    return 4, Ap, Aj, Ax


def directed_triangle():
    """0 -> 1 -> 2 -> 0: every vertex proposes, nobody is proposed to by its candidate"""
    return 3, np.array([0, 1, 2, 3], np.int32), np.array([1, 2, 0], np.int32), None


def integer_weights(n, Ap, Aj, seed=5, top=4):
    """symmetric integer weights 1 .. top on a symmetric pattern: a function of the unordered pair"""
    r, c = ar.edges(n, Ap, Aj)
    return (1 + edge_hash(np.minimum(r, c), np.maximum(r, c), 1000 + seed) % np.uint64(top)).astype(np.float64)


def asymmetric_weights(n, Ap, Aj, seed=9):
    """weights 1 .. 8 drawn per ENTRY on a symmetric pattern: the two ends of an edge disagree"""
    return np.random.default_rng(seed).integers(1, 9, len(Aj)).astype(np.float64)


def unsorted_with_repeats(n, Ap, Aj, Ax, seed=3):
    """the same matrix with every row shuffled and every entry stored a second time with a smaller weight"""
    rng = np.random.default_rng(seed)
    r, c = ar.edges(n, Ap, Aj)
    r2, c2, x2 = np.r_[r, r], np.r_[c, c], np.r_[Ax, Ax * 0.5]
    order = np.lexsort((rng.random(len(r2)), r2))
    Bp = np.zeros(n + 1, np.int32)
    np.cumsum(np.bincount(r2, minlength=n), out=Bp[1:])
    return n, Bp, c2[order].astype(np.int32), x2[order]


def aniso(nx, ny, eps):
    """the 5-point operator with the y-coupling scaled by eps (dyadic eps: every value exact in float): scipy CSR"""
    import scipy.sparse as sp
    ex, ey = np.ones(nx), np.ones(ny)
    Tx = sp.diags([-ex[:-1], 2 * ex, -ex[:-1]], [-1, 0, 1])
    Ty = sp.diags([-ey[:-1], 2 * ey, -ey[:-1]], [-1, 0, 1])
    A = (sp.kron(sp.identity(ny), Tx) + eps * sp.kron(Ty, sp.identity(nx))).tocsr()
    A.sort_indices()
    return A
