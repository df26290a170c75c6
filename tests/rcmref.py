"""The contract of bhs_csr_rcm_device (include/bhsparse_hip.h, "bandwidth-reducing ordering") restated in numpy: the checks,
the starts with and without the George-Liu refinement, the levels and the level-by-level Cuthill-McKee order, vectorised per
level (`rcm`).  Beside it an independent restatement from the textbook (`serial_rcm`): per component, a queue in which a
dequeued vertex appends its unnumbered neighbours by ascending (degree, index), and SPARSPAK's FNROOT loop as the contract
words it.  tests/test_rcm_abi.py holds the two against each other; tests/test_rcm_gpu.py compares the device with `rcm`.
The input generators of both are here too."""
from collections import deque

import numpy as np
import scipy.sparse as sp
from scipy.sparse.csgraph import connected_components

PERIPHERAL, NO_REVERSE = 1, 2


# ---------------------------------------------------------------- the checks
def refusal(n, Sp, Sj, nnz=None):
    """None where the device accepts (n, Sp, Sj), else which of its four checks refuses it"""
    Sp, Sj = np.asarray(Sp, np.int64), np.asarray(Sj, np.int64)
    nnz = len(Sj) if nnz is None else nnz
    if Sp[0] < 0 or np.any(np.diff(Sp) < 0) or Sp[n] > nnz or Sp[n] != nnz:
        return "row pointer"
    Sj = Sj[:Sp[n]]
    if np.any(Sj < 0) or np.any(Sj >= n):
        return "column"
    r = np.repeat(np.arange(n), np.diff(Sp))
    inner = np.ones(len(Sj), bool)
    inner[Sp[:-1][np.diff(Sp) > 0]] = False                           # a row's first entry has none before it
    if np.any(inner[1:] & (Sj[1:] <= Sj[:-1])):
        return "ascending"
    if not np.array_equal(np.sort(r * n + Sj), np.sort(Sj * n + r)):  # (no repeats: the entries and their mirrors are one set)
        return "symmetric"
    return None


def degrees(n, Sp, Sj):
    r = np.repeat(np.arange(n), np.diff(Sp))
    return np.bincount(r[r != Sj], minlength=n).astype(np.int64)


def matrix(n, Sp, Sj):
    return sp.csr_matrix((np.ones(len(Sj), np.int8), np.asarray(Sj), np.asarray(Sp)), shape=(n, n))


def components(n, Sp, Sj):
    """(root, comp, ncomp): the smallest vertex of every vertex's component, the components numbered by ascending root"""
    k, lab = connected_components(matrix(n, Sp, Sj), directed=False)
    first = np.full(k, n, np.int64)
    np.minimum.at(first, lab, np.arange(n))
    root = first[lab]
    comp = (np.cumsum(root == np.arange(n)) - 1)[root]
    return root, comp, k


# ---------------------------------------------------------------- the sweeps
def sweep(S, n, start):
    """the levels of one breadth-first search from every start at once"""
    level = np.full(n, -1, np.int64)
    level[start] = 0
    front = np.zeros(n, np.int8)
    front[start] = 1
    cur = 0
    while True:
        reach = (S @ front) > 0
        new = reach & (level < 0)
        if not new.any():
            return level
        cur += 1
        level[new] = cur
        front = new.astype(np.int8)


def far(n, level, comp, ncomp, key):
    """per component: e, its greatest level, and x, the vertex of smallest key on that level"""
    e = np.zeros(ncomp, np.int64)
    np.maximum.at(e, comp, level)
    last = level == e[comp]
    x = np.full(ncomp, np.iinfo(np.int64).max, np.int64)
    np.minimum.at(x, comp[last], key[last])
    return e, x & 0xffffffff


def starts(n, Sp, Sj, peripheral):
    """(start per component, level, sweeps, comp, ncomp, deg)"""
    S = matrix(n, Sp, Sj)
    deg = degrees(n, Sp, Sj)
    key = (deg << 32) | np.arange(n)
    _, comp, ncomp = components(n, Sp, Sj)
    start = np.full(ncomp, np.iinfo(np.int64).max, np.int64)
    np.minimum.at(start, comp, key)
    start &= 0xffffffff
    level = sweep(S, n, start)
    if not peripheral:
        return start, level, 1, comp, ncomp, deg
    e, x = far(n, level, comp, ncomp, key)
    done = np.zeros(ncomp, bool)
    start = x.copy()                                                  # after sweep 0 every start moves
    for sweeps in range(2, n + 2):
        level = sweep(S, n, start)
        e2, x2 = far(n, level, comp, ncomp, key)
        grew = ~done & (e2 > e)
        done |= ~grew
        if not grew.any():
            return start, level, sweeps, comp, ncomp, deg
        e[grew] = e2[grew]
        start[grew] = x2[grew]
    raise AssertionError("more than n + 1 sweeps")


# ---------------------------------------------------------------- the order
def forest_order(n, Sp, Sj, level, start, comp, deg):
    """pos of every vertex in the forest order: level by level, a level ordered by (pos of the parent, degree, index)"""
    Sp = np.asarray(Sp, np.int64)
    r = np.repeat(np.arange(n), np.diff(Sp))
    c = np.asarray(Sj, np.int64)
    down = level[c] == level[r] - 1                                   # the entries towards the level before
    r, c = r[down], c[down]
    by = np.argsort(level[r], kind="stable")
    r, c = r[by], c[by]
    depth = int(level.max()) + 1
    eptr = np.searchsorted(level[r], np.arange(depth + 1))
    verts = np.argsort(level, kind="stable")
    vptr = np.searchsorted(level[verts], np.arange(depth + 1))
    pos = np.full(n, -1, np.int64)
    pos[start] = comp[start]
    par = np.full(n, n, np.int64)
    for l in range(1, depth):
        rr, cc = r[eptr[l]:eptr[l + 1]], c[eptr[l]:eptr[l + 1]]
        np.minimum.at(par, rr, pos[cc])
        v = verts[vptr[l]:vptr[l + 1]]
        o = np.lexsort((v, deg[v], par[v]))
        pos[v[o]] = vptr[l] + np.arange(len(v))
    return pos


def rcm(n, Sp, Sj, flags=PERIPHERAL):
    """(perm, level, start, ncomp, depth, sweeps) as the device gives them, int32 arrays; raises ValueError on an input it
    refuses"""
    why = refusal(n, Sp, Sj)
    if why:
        raise ValueError(why)
    if n == 0:
        z = np.zeros(0, np.int32)
        return z, z, z, 0, 0, 0
    start, level, sweeps, comp, ncomp, deg = starts(n, Sp, Sj, bool(flags & PERIPHERAL))
    pos = forest_order(n, Sp, Sj, level, start, comp, deg)
    forest = np.argsort(pos)
    cm = forest[np.argsort(comp[forest], kind="stable")]              # stably regrouped by component
    perm = cm if flags & NO_REVERSE else cm[::-1]
    return perm.astype(np.int32), level.astype(np.int32), start.astype(np.int32), ncomp, int(level.max()) + 1, sweeps


# ---------------------------------------------------------------- the textbook, independently
def serial_rcm(n, Sp, Sj, flags=PERIPHERAL):
    """(perm, start, ncomp, depth, sweeps) by per-component loops: the queue algorithm and FNROOT's loop"""
    Sp, Sj = np.asarray(Sp).tolist(), np.asarray(Sj).tolist()
    nb = [[j for j in Sj[Sp[i]:Sp[i + 1]] if j != i] for i in range(n)]
    deg = [len(x) for x in nb]

    def structure(s):
        lev = {s: 0}
        q = deque([s])
        while q:
            u = q.popleft()
            for w in nb[u]:
                if w not in lev:
                    lev[w] = lev[u] + 1
                    q.append(w)
        e = max(lev.values())
        return e, min((deg[v], v) for v in lev if lev[v] == e)[1], lev

    seen = [False] * n
    cm, begin, depth, sweeps = [], [], 0, 0
    for r in range(n):                                                # ascending smallest vertex
        if seen[r]:
            continue
        members, q = [r], deque([r])
        seen[r] = True
        while q:
            u = q.popleft()
            for w in nb[u]:
                if not seen[w]:
                    seen[w] = True
                    members.append(w)
                    q.append(w)
        s = min((deg[v], v) for v in members)[1]
        e, x, _ = structure(s)
        mine = 1
        if flags & PERIPHERAL:
            while True:
                s = x
                e2, x, _ = structure(s)
                mine += 1
                if e2 <= e:
                    e = e2
                    break
                e = e2
        sweeps, depth = max(sweeps, mine), max(depth, e + 1)
        begin.append(s)
        numbered, q = {s}, deque([s])
        while q:
            u = q.popleft()
            cm.append(u)
            for w in sorted((w for w in nb[u] if w not in numbered), key=lambda w: (deg[w], w)):
                numbered.add(w)
                q.append(w)
    perm = cm if flags & NO_REVERSE else cm[::-1]
    return np.array(perm, np.int32), np.array(begin, np.int32), len(begin), depth, sweeps


# ---------------------------------------------------------------- what an ordering is for
def bandwidth_profile(n, Sp, Sj, perm=None):
    """(bandwidth, profile) of S(perm, perm): max |i - j|, and the sum over the rows of i - (the first column <= i)"""
    if n == 0:
        return 0, 0
    new = np.arange(n) if perm is None else np.empty(n, np.int64)
    if perm is not None:
        new[np.asarray(perm, np.int64)] = np.arange(n)
    r = new[np.repeat(np.arange(n), np.diff(Sp))]
    c = new[np.asarray(Sj, np.int64)]
    first = np.arange(n)
    np.minimum.at(first, r, c)
    return int(np.abs(r - c).max()) if len(c) else 0, int((np.arange(n) - first).sum())


# ---------------------------------------------------------------- the inputs
def from_pairs(n, a, b, diag=False):
    """the symmetric pattern with the entries (a, b) and (b, a), rows ascending, without repeats"""
    a, b = np.asarray(a, np.int64), np.asarray(b, np.int64)
    r, c = np.concatenate([a, b]), np.concatenate([b, a])
    if diag:
        r, c = np.concatenate([r, np.arange(n)]), np.concatenate([c, np.arange(n)])
    X = sp.csr_matrix((np.ones(len(r)), (r, c)), shape=(n, n))       # (repeats are summed)
    X.sort_indices()
    return n, X.indptr.astype(np.int32), X.indices.astype(np.int32)


def canonical(n, Sp, Sj):
    """pattern(S) U pattern(S^T), rows ascending, without repeats: what a pattern that does not qualify is turned into"""
    r = np.repeat(np.arange(n), np.diff(Sp))
    keep = r != np.asarray(Sj)
    has_diag = bool((~keep).any())
    return from_pairs(n, r[keep], np.asarray(Sj)[keep], diag=has_diag)


def shuffled(n, Sp, Sj, seed):
    """the pattern under a seeded relabelling of its vertices"""
    p = np.random.default_rng(seed).permutation(n)
    r = np.repeat(np.arange(n), np.diff(Sp))
    X = sp.csr_matrix((np.ones(len(Sj)), (p[r], p[np.asarray(Sj)])), shape=(n, n))
    X.sort_indices()
    return n, X.indptr.astype(np.int32), X.indices.astype(np.int32)


def path(n):
    return from_pairs(n, np.arange(n - 1), np.arange(1, n))


def grid(nx, ny, diag=True):
    """the five-point grid of nx x ny vertices, x fastest"""
    i = np.arange(nx * ny)
    right, up = i[i % nx < nx - 1], i[i < nx * (ny - 1)]
    return from_pairs(nx * ny, np.concatenate([right, up]), np.concatenate([right + 1, up + nx]), diag)


def star(n):
    """n vertices: vertex 0 joined to every other"""
    return from_pairs(n, np.zeros(n - 1, np.int64), np.arange(1, n))


def random_symmetric(n, draws, seed):
    rng = np.random.default_rng(seed)
    a, b = rng.integers(0, n, draws), rng.integers(0, n, draws)
    return from_pairs(n, a[a != b], b[a != b])


def two_cliques(k=40):
    X = sp.block_diag([np.ones((k, k)), np.ones((k, k))]).tocsr()
    X.sort_indices()
    return 2 * k, X.indptr.astype(np.int32), X.indices.astype(np.int32)


def no_entries(n=1000):
    return n, np.zeros(n + 1, np.int32), np.zeros(0, np.int32)


def tree(a=100, b=100):
    """1 -> a -> b each -> 1 each: n = 1 + a + 2 a b; the third level's a b child counts are scanned in one go"""
    mid = 1 + np.arange(a)
    low = 1 + a + np.arange(a * b)
    leaf = 1 + a + a * b + np.arange(a * b)
    src = np.concatenate([np.zeros(a, np.int64), np.repeat(mid, b), low])
    dst = np.concatenate([mid, low, leaf])
    return from_pairs(1 + a + 2 * a * b, src, dst)


def disjoint_paths3(n, seed=77):
    """floor(n / 3) paths of 3 vertices, and n % 3 single ones, under a seeded relabelling"""
    a = 3 * np.arange(n // 3)
    return shuffled(*from_pairs(n, np.concatenate([a, a + 1]), np.concatenate([a + 1, a + 2])), seed)


def disjoint_cliques(n, q=27, seed=78):
    """floor(n / q) cliques of q vertices with their diagonals, and n % q single ones, under a seeded relabelling"""
    i = np.arange(n // q * q)
    src = np.concatenate([i] * (q - 1))
    dst = np.concatenate([i - i % q + (i % q + s) % q for s in range(1, q)])
    return shuffled(*from_pairs(n, src, dst, diag=True), seed)


# seeds at which the facts asserted by tests/test_rcm_abi.py hold (found by trying 1, 2, ...)
SEED_PATH, SEED_GRID33, SEED_GRID20x50, SEED_RANDOM = 1, 1, 7, 4


def qualified(n, Sp, Sj):
    """the pattern itself where the device accepts it, else pattern U pattern^T with ascending rows"""
    return (n, Sp, Sj) if refusal(n, Sp, Sj) is None else canonical(n, Sp, Sj)


def patterns():
    """name -> (n, Sp, Sj): every pattern of tests/test_rcm_gpu.py that does not depend on the device's size"""
    import aggref as ar
    cases = {name: qualified(*c) for name, c in ar.gpu_cases().items()}
    cases["two_cliques"] = two_cliques()
    cases["no_entries"] = no_entries()
    cases["shuffled_path"] = shuffled(*path(2000), SEED_PATH)
    cases["shuffled_grid33"] = shuffled(*grid(33, 33), SEED_GRID33)
    cases["shuffled_grid20x50"] = shuffled(*grid(20, 50), SEED_GRID20x50)
    cases["random3000"] = random_symmetric(3000, 4000, SEED_RANDOM)
    cases["tree"] = tree()
    return cases
