"""The k-core decomposition restated in numpy, as include/bhsparse_hip.h words it ("k-core decomposition"): the reference of
tests/test_kcore_gpu.py, held against networkx and against an independent bucket peel by tests/test_kcore_abi.py; the k-truss
restated the way graph.ktruss_device iterates; and the makers of the inputs both files share.

A pattern is (n, Sp, Sj): int32 CSR, rows strictly ascending, structurally symmetric; a diagonal entry is allowed and ignored."""
import functools

import numpy as np
import scipy.sparse as sp

import gridpass as gp


# ---------------------------------------------------------------- patterns
def from_pairs(n, r, c, diag=False):
    """(n, Sp, Sj) of the undirected edges (r[t], c[t]), each stored both ways once, with every diagonal entry under diag"""
    r, c = np.asarray(r, np.int64), np.asarray(c, np.int64)
    keep = r != c
    r, c = r[keep], c[keep]
    rr, cc = np.concatenate([r, c]), np.concatenate([c, r])
    if diag:
        rr, cc = np.concatenate([rr, np.arange(n)]), np.concatenate([cc, np.arange(n)])
    key = np.unique(rr * n + cc)
    rr, cc = key // n, key % n
    Sp = np.zeros(n + 1, np.int32)
    np.cumsum(np.bincount(rr, minlength=n), out=Sp[1:])
    return n, Sp, cc.astype(np.int32)


def pairs_of(n, Sp, Sj):
    r = np.repeat(np.arange(n, dtype=np.int64), np.diff(Sp))
    return r, np.asarray(Sj, np.int64)


def relabel(pattern, seed):
    """the same graph under a random relabelling of its vertices: (pattern, perm) with perm[old] = new"""
    n, Sp, Sj = pattern
    perm = np.random.default_rng(seed).permutation(n)
    r, c = pairs_of(n, Sp, Sj)
    d = r == c
    out = from_pairs(n, perm[r[~d]], perm[c[~d]])
    if d.any():                                                       # the diagonal entries follow their vertices
        rr, cc = pairs_of(*out)
        key = np.unique(np.concatenate([rr * n + cc, perm[r[d]] * n + perm[r[d]]]))
        Sp2 = np.zeros(n + 1, np.int32)
        np.cumsum(np.bincount(key // n, minlength=n), out=Sp2[1:])
        out = (n, Sp2, (key % n).astype(np.int32))
    return out, perm


def path(n):
    return from_pairs(n, np.arange(n - 1), np.arange(1, n))


def star(n):
    """vertex 0 and n - 1 leaves"""
    return from_pairs(n, np.zeros(n - 1, np.int64), np.arange(1, n))


def grid5(nx):
    """the 5-point grid of nx x nx vertices, with its diagonal"""
    idx = np.arange(nx * nx).reshape(nx, nx)
    r = np.concatenate([idx[:, :-1].ravel(), idx[:-1, :].ravel()])
    c = np.concatenate([idx[:, 1:].ravel(), idx[1:, :].ravel()])
    return from_pairs(nx * nx, r, c, diag=True)


def cliques(sizes, diag=False):
    """disjoint cliques of the given sizes, one after the other"""
    r, c, at = [], [], 0
    for q in sizes:
        i, j = np.triu_indices(q, 1)
        r.append(i + at)
        c.append(j + at)
        at += q
    return from_pairs(at, np.concatenate(r), np.concatenate(c), diag=diag)


def cliques35(n):
    """n >= 8 vertices in disjoint cliques of 3 (about 85 in a hundred vertices, first) and of 5, vectorised, none left over.
    Returns (pattern, core before relabelling): core 2 in round 1, core 4 in round 2"""
    n5 = (15 * n // 100) // 5
    n5 += (2 * n - n5) % 3                                            # so that 3 divides what the cliques of 5 leave
    n3 = (n - 5 * n5) // 3
    assert n3 >= 0 and 3 * n3 + 5 * n5 == n
    core = np.zeros(n, np.int32)
    r, c = [], []
    for q, cnt, at in ((3, n3, 0), (5, n5, 3 * n3)):
        i, j = np.triu_indices(q, 1)
        base = at + q * np.arange(cnt, dtype=np.int64)[:, None]
        r.append((base + i[None, :]).ravel())
        c.append((base + j[None, :]).ravel())
        core[at:at + q * cnt] = q - 1
    return from_pairs(n, np.concatenate(r), np.concatenate(c)), core


def hub():
    """a hub with 1000 pendant leaves that is also one corner of a triangle, and two isolated vertices: vertex 0 the hub, 1 and
    2 the triangle's other corners, 3 .. 1002 the leaves, 1003 and 1004 isolated"""
    r = np.concatenate([[0, 0, 1], np.zeros(1000, np.int64)])
    c = np.concatenate([[1, 2, 2], np.arange(3, 1003)])
    return from_pairs(1005, r, c)


def leaves3():
    """a vertex with 3 pendant leaves and nothing else: its degree falls from 3 to 0, BELOW k = 1, in one round"""
    return from_pairs(4, [0, 0, 0], [1, 2, 3])


def uniform(n, per_row, seed):
    """about per_row entries a row: n * per_row / 2 random pairs, symmetrised"""
    rng = np.random.default_rng(seed)
    m = n * per_row // 2
    return from_pairs(n, rng.integers(0, n, m), rng.integers(0, n, m))


def rmat(scale, edge_factor, seed, a=0.57, b=0.19, c=0.19):
    """an R-MAT-like skewed graph of 2^scale vertices: edge_factor 2^scale pairs drawn bit by bit with the quadrant
    probabilities (a, b, c, 1 - a - b - c), symmetrised"""
    rng = np.random.default_rng(seed)
    m = edge_factor << scale
    r, col = np.zeros(m, np.int64), np.zeros(m, np.int64)
    for _ in range(scale):
        u = rng.random(m)
        r = 2 * r + (u >= a + b)
        col = 2 * col + (((u >= a) & (u < a + b)) | (u >= a + b + c))
    return from_pairs(1 << scale, r, col)


def band_pieces(n, w, piece=512):
    """disjoint bands of half-width w with their diagonals, of at most `piece` vertices each"""
    i = np.arange(n, dtype=np.int64)[:, None]
    j = i + np.arange(1, w + 1, dtype=np.int64)[None, :]
    ok = (j < n) & (j // piece == i // piece)
    return from_pairs(n, np.repeat(np.arange(n), ok.sum(axis=1)), j[ok], diag=True)


def planted(n, per_row, sizes, seed):
    """uniform(n, per_row) with cliques of the given sizes planted on random vertices"""
    rng = np.random.default_rng(seed)
    _, Sp, Sj = uniform(n, per_row, seed + 1)
    r, c = pairs_of(n, Sp, Sj)
    rs, cs = [r], [c]
    members = rng.permutation(n)
    at = 0
    for q in sizes:
        v = members[at:at + q]
        at += q
        i, j = np.triu_indices(q, 1)
        rs.append(v[i])
        cs.append(v[j])
    return from_pairs(n, np.concatenate(rs), np.concatenate(cs))


def lanes(n, nnz):
    """side_lanes: the lanes a row gets from the mean row length"""
    mean = nnz / n if n else 0.0
    return 1 if mean <= 4 else 4 if mean <= 16 else 16 if mean <= 64 else 64


# name: (maker, {core values}, kmax, rounds) -- the closed forms
CLOSED = {
    "path4096": (lambda: path(4096), {1}, 1, 2048),
    "path4097": (lambda: path(4097), {1}, 1, 2049),
    "star1024": (lambda: star(1024), {1}, 1, 2),
    "grid32": (lambda: grid5(32), {2}, 2, 31),
    "grid64": (lambda: grid5(64), {2}, 2, 63),
    "grid31": (lambda: grid5(31), {2}, 2, 31),
    "cliques": (lambda: cliques((3, 7, 7, 20)), {2, 6, 19}, 19, 3),
    "hub": (hub, {0, 1, 2}, 2, 3),
}
OTHERS = {
    "uniform4096": lambda: uniform(4096, 8, 11),
    "rmat12": lambda: rmat(12, 16, 12),
    "leaves3": leaves3,
}
BAND_N = 3000                                                         # six pieces: five of 512 and one of 440 vertices


@functools.lru_cache(maxsize=None)
def case(name):
    """the input `name` of the GPU tests, under a random relabelling (the bands as they are: band<L>)"""
    if name.startswith("band"):
        L = int(name[4:])
        return relabel(band_pieces(BAND_N, gp.HALF_WIDTH[L]), 500 + L)[0]
    maker = CLOSED[name][0] if name in CLOSED else OTHERS[name]
    return relabel(maker(), 100 + sorted(list(CLOSED) + list(OTHERS)).index(name))[0]


CASES = tuple(CLOSED) + tuple(OTHERS) + tuple("band%d" % L for L in gp.LANES)


# ---------------------------------------------------------------- the definition
def refusal(n, Sp, Sj, nnz=None):
    """None, or why the device refuses the pattern"""
    Sp, Sj = np.asarray(Sp, np.int64), np.asarray(Sj, np.int64)
    nnz = len(Sj) if nnz is None else nnz
    if Sp[0] < 0 or np.any(np.diff(Sp) < 0) or Sp[n] != nnz or Sp[n] > len(Sj):
        return "row pointer"
    if np.any(Sj < 0) or np.any(Sj >= n):
        return "column"
    r, c = pairs_of(n, Sp, Sj)
    key = r * n + c
    if np.any(np.diff(key) <= 0):
        return "ascending"
    if not np.array_equal(np.sort(c * n + r), key):
        return "symmetric"
    return None


@functools.lru_cache(maxsize=None)
def _answer(name):
    return peel(*case(name))


def answer(name):
    """peel(case(name)), computed once"""
    return _answer(name)


def peel(n, Sp, Sj):
    """the definition, round by round: (core int32[n], round int32[n], kmax, rounds)"""
    if refusal(n, Sp, Sj) is not None:
        raise ValueError("not a symmetric pattern with ascending rows")
    Sp = np.asarray(Sp, np.int64)
    r, c = pairs_of(n, Sp, Sj)
    deg = np.bincount(r[r != c], minlength=n).astype(np.int64)
    present = np.ones(n, bool)
    core, rnd = np.zeros(n, np.int32), np.zeros(n, np.int32)
    k, rounds = 0, 0
    cand = np.arange(n)                                               # where to look for the vertices that leave
    left = n
    while left:
        rounds += 1
        leave = cand[deg[cand] <= k] if len(cand) else cand
        if len(leave) == 0:                                           # nothing at or below k: the level jumps
            alive = np.flatnonzero(present)
            k = max(k, int(deg[alive].min()))
            leave = alive[deg[alive] <= k]
        core[leave], rnd[leave] = k, rounds
        present[leave] = False
        left -= len(leave)
        lens = Sp[leave + 1] - Sp[leave]                              # the neighbours of those that left, with repeats
        at = np.repeat(Sp[leave] - np.concatenate([[0], np.cumsum(lens)[:-1]]), lens) + np.arange(lens.sum())
        nb = np.asarray(Sj, np.int64)[at]
        nb = nb[nb != np.repeat(leave, lens)]
        np.subtract.at(deg, nb, 1)
        cand = np.unique(nb[present[nb]])
    return core, rnd, (int(core.max()) if n else 0), rounds


def bucket_peel(n, Sp, Sj):
    """Batagelj-Zaversnik: the core numbers by the serial bucket algorithm, one vertex at a time (int32[n])"""
    r, c = pairs_of(n, Sp, Sj)
    deg = np.bincount(r[r != c], minlength=n).astype(np.int64)
    order = np.argsort(deg, kind="stable")
    pos = np.empty(n, np.int64)
    pos[order] = np.arange(n)
    md = int(deg.max()) if n else 0
    start = np.zeros(md + 2, np.int64)
    np.cumsum(np.bincount(deg, minlength=md + 1), out=start[1:])
    start = start[:-1].copy()                                         # the first place of every degree's bucket
    deg, order, pos, start = deg.tolist(), order.tolist(), pos.tolist(), start.tolist()
    Spl, Sjl = np.asarray(Sp).tolist(), np.asarray(Sj).tolist()
    for i in range(n):
        v = order[i]
        for q in range(Spl[v], Spl[v + 1]):
            u = Sjl[q]
            if u != v and deg[u] > deg[v]:
                du, pu = deg[u], pos[u]
                pw = start[du]                                        # swap u with the first vertex of its bucket
                w = order[pw]
                if u != w:
                    order[pu], order[pw] = w, u
                    pos[u], pos[w] = pw, pu
                start[du] += 1
                deg[u] -= 1
    return np.asarray(deg, np.int32)


def later_neighbours(n, Sp, Sj, order):
    """per vertex the number of its neighbours that stand behind it in `order`"""
    place = np.empty(n, np.int64)
    place[np.asarray(order, np.int64)] = np.arange(n)
    r, c = pairs_of(n, Sp, Sj)
    return np.bincount(r[place[c] > place[r]], minlength=n)


# ---------------------------------------------------------------- the k-truss
def supports(n, Tp, Tj):
    """per entry of the symmetric pattern T without a diagonal: the common neighbours of its two ends"""
    T = sp.csr_matrix((np.ones(len(Tj)), Tj, Tp), shape=(n, n))
    r, c = pairs_of(n, Tp, Tj)
    if not len(Tj):
        return np.zeros(0, np.int64)
    return np.asarray((T @ T)[r, c]).ravel().round().astype(np.int64)


def ktruss(n, Sp, Sj, k):
    """as graph.ktruss_device iterates: the diagonal dropped, then products and selections until nnz stops falling:
    (Tp, Tj, support, iterations)"""
    r, c = pairs_of(n, Sp, Sj)
    _, Tp, Tj = from_pairs(n, r, c)
    iterations = 0
    while True:
        if not len(Tj):
            return Tp, Tj, np.zeros(0, np.int64), iterations
        sup = supports(n, Tp, Tj)
        iterations += 1
        keep = sup >= k - 2
        if k <= 2 or keep.all():
            return Tp, Tj, sup, iterations
        r, c = pairs_of(n, Tp, Tj)
        Tp = np.zeros(n + 1, np.int32)
        np.cumsum(np.bincount(r[keep], minlength=n), out=Tp[1:])
        Tj = Tj[keep]
