"""The definition of include/bhsparse_hip.h, "betweenness centrality" (bhs_csr_betweenness_device), restated on the host in
numpy: what tests/test_bc_abi.py holds against networkx and closed forms and tests/test_bc_gpu.py compares the device with,
bit for bit.

G = (n, Gp, Gj) holds the OUT-EDGES: an entry G(i, j) is an edge i -> j.  T = (Tp, Tj) holds the in-edges, G^T; for an
undirected graph T is G.  For each source s, in list order:

  level[s] = 0, level[v] the breadth-first depth over G, -1 where v is not reached;
  sigma[s] = 1, sigma[v] = the sum of sigma[u] over the entries u of ROW v OF T with level[u] == level[v] - 1, 0 where v
    is not reached;
  delta[u] = 0 on the deepest level, else sigma[u] * S with S the sum of (1 + delta[v]) / sigma[v] over the entries v of ROW u
    OF G with level[v] == level[u] + 1;
  bc[u] = fl(bc[u] + delta[u]) for every reached u != s with 0 < level[u] < the deepest level.

The summation rule (`row_sums`): L = lanes(n, nnz) of the matrix whose row is walked; a row of more than 32 L entries takes
L_row = 64, any other L_row = L; the entry at position p belongs to lane p mod L_row; a lane adds its qualifying terms in
ascending p from +0; the lane sums fold by the xor butterfly t[l] = t[l] + t[l ^ off], off = L_row / 2, ..., 1.  An entry
that does not qualify contributes nothing -- here it adds +0, which changes no sum that starts at +0 and has no negative
term.  Every NaN is stored as the one word 0x7FF8000000000000 (`canon`)."""
import numpy as np

BATCH = 8
LONG = 32                                                             # kBcLong: a row of more entries a lane takes a wave
NAN_WORD = np.uint64(0x7FF8000000000000)


def lanes(n, nnz):
    """side_lanes: the lanes a row gets from the mean row length"""
    mean = nnz / n if n else 0.0
    return 1 if mean <= 4.0 else 4 if mean <= 16.0 else 16 if mean <= 64.0 else 64


def canon(x):
    """every NaN as the one word the call stores"""
    x = np.asarray(x, np.float64).copy()
    x.view(np.uint64)[np.isnan(x)] = NAN_WORD
    return x


def refusal(n, Gp, Gj, Tp, Tj, sources):
    """what the device refuses, or None"""
    for P, J in ((Gp, Gj), (Tp, Tj)):
        P = np.asarray(P, np.int64)
        if P[0] != 0 or P[n] != len(J) or np.any(np.diff(P[:n + 1]) < 0):
            return "row pointer"
        if len(J) and (np.min(J) < 0 or np.max(J) >= n):
            return "column"
    s = np.asarray(sources)
    if s.min() < 0 or s.max() >= n:
        return "source"
    return None


def _fold(t):
    """the xor butterfly over the last axis; every lane ends with the same word, lane 0's is returned"""
    W = t.shape[-1]
    idx = np.arange(W)
    off = W // 2
    while off >= 1:
        t = t + t[..., idx ^ off]
        off //= 2
    return t[..., 0]


def row_sums(verts, Xp, Xj, L, qualifies, value):
    """the rule's sum for every vertex of `verts` over its row of X: entry q adds value[Xj[q]] where qualifies[Xj[q]]"""
    verts = np.asarray(verts, np.int64)
    out = np.zeros(len(verts))
    lo, hi = Xp[verts].astype(np.int64), Xp[verts + 1].astype(np.int64)
    cnt = hi - lo
    with np.errstate(over="ignore", invalid="ignore"):
        short = np.flatnonzero(cnt <= LONG * L)
        if len(short):
            c = cnt[short]
            K = max(int(-(-c.max() // L)), 1)
            pad = np.zeros((len(short), K * L))
            row = np.repeat(np.arange(len(short)), c)
            p = np.arange(int(c.sum())) - np.repeat(np.cumsum(c) - c, c)
            col = Xj[np.repeat(lo[short], c) + p]
            pad[row, p] = np.where(qualifies[col], value[col], 0.0)
            pad = pad.reshape(len(short), K, L)
            acc = np.zeros((len(short), L))
            for k in range(K):                                        # ascending p, from +0
                acc = acc + pad[:, k, :]
            out[short] = _fold(acc)
        for i in np.flatnonzero(cnt > LONG * L):                      # a wave a row
            col = Xj[lo[i]:hi[i]]
            K = -(-len(col) // 64)
            pad = np.zeros(K * 64)
            pad[:len(col)] = np.where(qualifies[col], value[col], 0.0)
            out[i] = _fold(np.add.accumulate(pad.reshape(K, 64), axis=0)[-1])   # (accumulate adds left to right, from the first row: +0 + x = x)
    return out


def bfs(n, Gp, Gj, s):
    """(level, slices): the breadth-first depths from s over G and every level's vertices, ascending"""
    level = np.full(n, -1, np.int32)
    level[s] = 0
    slices = [np.array([s], np.int64)]
    while True:
        v = slices[-1]
        c = (Gp[v + 1] - Gp[v]).astype(np.int64)
        q = np.repeat(Gp[v].astype(np.int64) - (np.cumsum(c) - c), c) + np.arange(int(c.sum()))
        new = np.unique(Gj[q])
        new = new[level[new] == -1]
        if len(new) == 0:
            return level, slices
        level[new] = len(slices)
        slices.append(new.astype(np.int64))


def source(n, Gp, Gj, Tp, Tj, s, bc):
    """one source added to bc in place: (level, sigma, deepest, overflowed)"""
    LG, LT = lanes(n, len(Gj)), lanes(n, len(Tj))
    level, slices = bfs(n, Gp, Gj, s)
    sigma = np.zeros(n)
    sigma[s] = 1.0
    for l in range(1, len(slices)):
        sigma[slices[l]] = row_sums(slices[l], Tp, Tj, LT, level == l - 1, sigma)
    delta = np.zeros(n)
    deepest = len(slices) - 1
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        for l in range(deepest - 1, 0, -1):
            u = slices[l]
            term = (1.0 + delta) / np.where(level == l + 1, sigma, 1.0)
            S = row_sums(u, Gp, Gj, LG, level == l + 1, term)
            delta[u] = canon(sigma[u] * S)
            bc[u] = canon(bc[u] + delta[u])
    return level, sigma, deepest, not np.all(np.isfinite(sigma))


def launched(deepest):
    """the forward passes a source launches: those that have a slice, deepest + 1, rounded up to the batch"""
    return BATCH * -(-(deepest + 1) // BATCH)


def answer(n, Gp, Gj, Tp, Tj, sources, start=None):
    """everything the call reports: bc (from `start` under ACCUMULATE), level and sigma of the last source, reached, passes
    (launched), levels, overflow, work (the passes that had a slice) and backs (the backward launches)"""
    Gp, Gj, Tp, Tj = (np.asarray(a) for a in (Gp, Gj, Tp, Tj))
    bc = np.zeros(n) if start is None else np.array(start, np.float64)
    out = {"reached": 0, "passes": 0, "levels": 0, "overflow": 0, "backs": 0}
    for s in np.asarray(sources, np.int64):
        level, sigma, deepest, over = source(n, Gp, Gj, Tp, Tj, int(s), bc)
        out["reached"] += int((level >= 0).sum())
        out["passes"] += launched(deepest)
        out["levels"] += deepest + 1
        out["overflow"] += int(over)
        out["backs"] += max(deepest - 1, 0)
    out.update(bc=bc, level=level, sigma=sigma, work=out["levels"])
    return out


# ---------------------------------------------------------------- inputs
def csr(n, r, c):
    """the edges in the order given, grouped by row (a stable sort: rows stay as unsorted as they come)"""
    r = np.asarray(r, np.int64)
    o = np.argsort(r, kind="stable")
    Gp = np.zeros(n + 1, np.int32)
    np.cumsum(np.bincount(r, minlength=n), out=Gp[1:])
    return n, Gp, np.asarray(c, np.int32)[o]


def transposed(n, Gp, Gj):
    """the in-edges (Tp, Tj): rows ascending by source, parallel edges kept -- what the device transpose gives"""
    r = np.repeat(np.arange(n, dtype=np.int64), np.diff(np.asarray(Gp, np.int64)))
    o = np.lexsort((r, Gj))
    Tp = np.zeros(n + 1, np.int32)
    np.cumsum(np.bincount(Gj, minlength=n), out=Tp[1:])
    return Tp, r[o].astype(np.int32)


def shuffled(n, Gp, Gj, seed):
    """the same rows with their entries in a random order"""
    rng = np.random.default_rng(seed)
    key = np.repeat(np.arange(n), np.diff(Gp)) + rng.random(len(Gj))
    return n, Gp, Gj[np.argsort(key)]


def path(n):
    """the directed path 0 -> 1 -> ... -> n - 1: from 0 the deepest level is n - 1"""
    r = np.arange(n - 1)
    return csr(n, r, r + 1)


def star(n):
    """vertex 0 and n - 1 leaves, edges both ways"""
    leaves = np.arange(1, n)
    return csr(n, np.r_[np.zeros(n - 1, np.int64), leaves], np.r_[leaves, np.zeros(n - 1, np.int64)])


def diamond():
    """0 -> {1, 2} -> 3 -> 4: two shortest paths meet at 3"""
    return csr(5, [0, 0, 1, 2, 3], [1, 2, 3, 3, 4])


def stages(widths, seed=None, drop=0.0):
    """a chain of stages of the given widths, every vertex of a stage joined to every vertex of the next: sigma of a stage
    is the product of the widths before it.  Vertex 0 is a source ahead of stage 0.  drop: that share of the edges is left
    out at random (never one from a stage's first vertex, so the levels stay), and the path counts inside a stage differ;
    seed: the entries inside rows in a random order"""
    at, r, c, prev = 1, [], [], np.array([0])
    for w in widths:
        cur = np.arange(at, at + w)
        r.append(np.repeat(prev, w))
        c.append(np.tile(cur, len(prev)))
        prev, at = cur, at + w
    r, c = np.concatenate(r), np.concatenate(c)
    if drop:
        first = np.r_[0, 1 + np.cumsum(widths)[:-1]]
        keep = (np.random.default_rng(0 if seed is None else seed).random(len(r)) >= drop) | np.isin(r, first)
        r, c = r[keep], c[keep]
    g = csr(at, r, c)
    return g if seed is None else shuffled(*g, seed)


def diamonds(count):
    """a chain of `count` diamonds a -> {b, c} -> a': sigma doubles a diamond, vertex 3 k is the k-th joint"""
    k = np.arange(count, dtype=np.int64)
    a, b, c = 3 * k, 3 * k + 1, 3 * k + 2
    return csr(3 * count + 1, np.r_[a, a, b, c], np.r_[b, c, a + 3, a + 3])


def fan(m):
    """source 0 -> m middle vertices -> one sink: depth 2, the source's row and the sink's in-row are hub rows"""
    mid = np.arange(1, m + 1, dtype=np.int64)
    return csr(m + 2, np.r_[np.zeros(m, np.int64), mid], np.r_[mid, np.full(m, m + 1)])


def grid_with_diagonals(nx=24, ny=19):
    """tests/bc/bc_demo.cpp's graph, entry for entry: a grid, edges both ways to the four neighbours and, where
    (x + y) % 3 == 0, along the diagonal to (x + 1, y + 1); rows in the order the demo joins them"""
    rows = [[] for _ in range(nx * ny)]

    def join(a, b):
        rows[a].append(b)
        rows[b].append(a)
    for y in range(ny):
        for x in range(nx):
            if x + 1 < nx:
                join(y * nx + x, y * nx + x + 1)
            if y + 1 < ny:
                join(y * nx + x, (y + 1) * nx + x)
            if (x + y) % 3 == 0 and x + 1 < nx and y + 1 < ny:
                join(y * nx + x, (y + 1) * nx + x + 1)
    n = nx * ny
    return csr(n, np.repeat(np.arange(n), [len(r) for r in rows]), np.concatenate(rows))


def fnv(data):
    """FNV-1a, 64 bits, over the bytes"""
    h = 1469598103934665603
    for b in bytes(data):
        h = ((h ^ b) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    return h
