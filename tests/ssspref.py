"""The definition of include/bhsparse_hip.h, "shortest paths" (bhs_csr_sssp_device), restated on the host: what
tests/test_sssp_abi.py holds against scipy and networkx and tests/test_sssp_gpu.py compares the device with, bit for bit.

G = (Gp, Gj, Gx or None) is the OUT-EDGE matrix: an entry G(i, j) is an edge i -> j of weight Gx (1 without values).  The
distances are the least fixed point of d[s] = 0, d[v] = min over the edges (u, v) of fl(d[u] + w), fl one rounding to the
value type: `dijkstra` is the textbook heap loop on numpy scalars of that type.  `parents` is the parent rule, `simulate` the
synchronous bucket passes for a delta -- the passes that have a slice and the buckets that are not empty."""
import heapq

import numpy as np

INV_PARENT = np.iinfo(np.int32).max
BATCH = 8


def weights(Gx, nnz, dtype):
    """the weights in the value type, 1 without values, -0 as 0"""
    if Gx is None:
        return np.ones(nnz, dtype)
    return np.ascontiguousarray(Gx, dtype) + dtype(0)


def refusal(n, Gp, Gj, Gx, sources):
    """what the device refuses, or None"""
    Gp = np.asarray(Gp, np.int64)
    if Gp[0] != 0 or Gp[n] != len(Gj) or np.any(np.diff(Gp) < 0):
        return "row pointer"
    if len(Gj) and (np.min(Gj) < 0 or np.max(Gj) >= n):
        return "column"
    if Gx is not None and len(Gx) and (np.any(np.isnan(Gx)) or np.any(np.signbit(Gx) & (np.asarray(Gx) != 0))):
        return "weight"
    s = np.asarray(sources)
    if s.min() < 0 or s.max() >= n:
        return "source"
    return None


def dijkstra(n, Gp, Gj, Gx, sources, dtype=np.float64):
    """a heap Dijkstra in the value type: one rounding an edge"""
    dtype = np.dtype(dtype).type
    w = weights(Gx, len(Gj), dtype)
    dist = np.full(n, np.inf, dtype)
    heap = []
    for s in np.unique(np.asarray(sources, np.int64)):
        dist[s] = dtype(0)
        heap.append((dtype(0), int(s)))
    heapq.heapify(heap)
    settled = np.zeros(n, bool)
    with np.errstate(over="ignore"):
        while heap:
            du, u = heapq.heappop(heap)
            if settled[u]:
                continue
            settled[u] = True
            for q in range(int(Gp[u]), int(Gp[u + 1])):
                v = int(Gj[q])
                nd = dtype(du + w[q])
                if nd < dist[v]:
                    dist[v] = nd
                    heapq.heappush(heap, (nd, v))
    return dist


def parents(n, Gp, Gj, Gx, sources, dist):
    """(parent int32[n], loose): the smallest u with an edge (u, v), fl(d[u] + w) == d[v] and d[u] < d[v]; -1 a source or
    not reached, -2 reached with no such edge"""
    dtype = dist.dtype.type
    w = weights(Gx, len(Gj), dtype)
    rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(np.asarray(Gp, np.int64)))
    v = np.asarray(Gj, np.int64)
    with np.errstate(over="ignore", invalid="ignore"):
        du = dist[rows]
        nd = (du + w).astype(dtype)
        ok = np.isfinite(du) & (nd == dist[v]) & (du < dist[v])
    par = np.full(n, INV_PARENT, np.int64)
    np.minimum.at(par, v[ok], rows[ok])
    out = np.where(~np.isfinite(dist), -1, np.where(par == INV_PARENT, -2, par)).astype(np.int32)
    out[np.asarray(sources, np.int64)] = -1
    return out, int((out == -2).sum())


def bound_of(m, delta):
    """the bound of the bucket that holds m: (floor(m / delta) + 1) delta in double"""
    with np.errstate(over="ignore", invalid="ignore"):
        return float((np.floor(np.float64(m) / np.float64(delta)) + np.float64(1.0)) * np.float64(delta))


def simulate(n, Gp, Gj, Gx, sources, delta, dtype=np.float64):
    """(dist, passes, buckets) of the synchronous passes: a pass relaxes its slice from the distances the pass before left;
    a vertex it lowers and leaves below the bound is in the next slice; where it appends nothing the next slice is the
    pending vertices below the bound of the bucket that holds their minimum, or equal to that minimum.  passes: those that
    have a slice; buckets: those that are not empty"""
    dtype = np.dtype(dtype).type
    Gp = np.asarray(Gp, np.int64)
    Gj = np.asarray(Gj, np.int64)
    w = weights(Gx, len(Gj), dtype)
    dist = np.full(n, np.inf, dtype)
    done = np.full(n, np.inf, dtype)
    sv = np.unique(np.asarray(sources, np.int64))
    dist[sv] = dtype(0)
    sd = dist[sv].copy()
    bound, buckets, passes = bound_of(0.0, delta), 1, 0
    while len(sv):
        passes += 1
        act = sd < done[sv]
        v, dv = sv[act], sd[act]
        done[v] = dv
        cnt = Gp[v + 1] - Gp[v]
        idx = np.repeat(Gp[v] - np.r_[0, np.cumsum(cnt)[:-1]], cnt) + np.arange(int(cnt.sum()))
        u = Gj[idx]
        with np.errstate(over="ignore"):
            nd = (np.repeat(dv, cnt) + w[idx]).astype(dtype)
        app = np.zeros(0, np.int64)
        if len(u):
            o = np.argsort(u, kind="stable")
            us = u[o]
            starts = np.flatnonzero(np.r_[True, us[1:] != us[:-1]])
            touched, low = us[starts], np.minimum.reduceat(nd[o], starts)
            lowered = low < dist[touched]
            touched, low = touched[lowered], low[lowered]
            dist[touched] = low
            app = touched[low.astype(np.float64) < bound]
        if len(app) == 0:
            pend = np.flatnonzero(dist < done)
            if len(pend) == 0:
                break
            m = dist[pend].min()
            bound = bound_of(m, delta)
            buckets += 1
            app = pend[(dist[pend].astype(np.float64) < bound) | (dist[pend] == m)]
        sv, sd = app, dist[app].copy()
    return dist, passes, buckets


def launched(passes):
    """what *passes_out reports: the passes that have a slice, rounded up to the batch"""
    return BATCH * -(-passes // BATCH)


def answer(n, Gp, Gj, Gx, sources, delta, dtype=np.float64, heap=True):
    """everything the call reports for this input: dist, parent, reached, loose, buckets, passes (those with a slice).  The
    distances are the heap loop's, and the simulation must give the same bits (heap=False: the simulation's alone, where
    the heap loop would run for minutes)"""
    dist, passes, buckets = simulate(n, Gp, Gj, Gx, sources, delta, dtype)
    if heap:
        want = dijkstra(n, Gp, Gj, Gx, sources, dtype)
        assert want.tobytes() == dist.tobytes()
    parent, loose = parents(n, Gp, Gj, Gx, sources, dist)
    return {"dist": dist, "parent": parent, "reached": int(np.isfinite(dist).sum()), "loose": loose, "buckets": buckets,
            "passes": passes}


def lanes(n, nnz):
    """side_lanes: the lanes a row gets from the mean row length"""
    mean = nnz / n if n else 0.0
    return 1 if mean <= 4.0 else 4 if mean <= 16.0 else 16 if mean <= 64.0 else 64


# ---------------------------------------------------------------- inputs
def csr(n, r, c, x=None):
    """the edges in the order given, grouped by row (a stable sort: rows stay as unsorted as they come)"""
    r = np.asarray(r, np.int64)
    o = np.argsort(r, kind="stable")
    Gp = np.zeros(n + 1, np.int32)
    np.cumsum(np.bincount(r, minlength=n), out=Gp[1:])
    return n, Gp, np.asarray(c, np.int32)[o], None if x is None else np.asarray(x)[o]


def path(n, weight=None):
    """the directed path 0 -> 1 -> ... -> n - 1"""
    r = np.arange(n - 1)
    return csr(n, r, r + 1, None if weight is None else np.full(n - 1, float(weight)))


def star(hub_row=5000, long_row=300, seed=3):
    """vertex 0 with hub_row out-edges to 1 .. hub_row in a random order, vertex 1 with long_row out-edges to vertices
    behind them, and a chain from there: a row beyond 32 entries a lane at every lane width, and a second one"""
    rng = np.random.default_rng(seed)
    n = 1 + hub_row + long_row + 8
    r = np.r_[np.zeros(hub_row, np.int64), np.ones(long_row, np.int64), np.arange(hub_row + 1, n - 1)]
    c = np.r_[rng.permutation(hub_row) + 1, rng.permutation(long_row) + hub_row + 1, np.arange(hub_row + 2, n)]
    x = rng.integers(1, 9, len(r)).astype(np.float64) / 4.0
    return csr(n, r, c, x)


def star_padded(L, seed=4):
    """the star with so many short rows behind it that the mean row length gives L lanes a row"""
    n0, Gp, Gj, Gx = star(seed=seed)
    per, extra = {1: (2, 4000), 4: (10, 3000), 16: (150, 1500), 64: (600, 800)}[L]
    rng = np.random.default_rng(seed + L)
    r0 = np.repeat(np.arange(n0), np.diff(Gp))
    r1 = np.repeat(np.arange(n0, n0 + extra), per)
    c1 = rng.integers(0, n0 + extra, len(r1))
    x1 = rng.integers(1, 9, len(r1)).astype(np.float64) / 4.0
    link_r, link_c, link_x = np.array([n0 - 1]), np.array([n0]), np.array([0.5])
    # the extra vertices hang off the chain's end and off each other
    chain_r, chain_c = np.arange(n0, n0 + extra - 1), np.arange(n0 + 1, n0 + extra)
    return csr(n0 + extra, np.r_[r0, link_r, r1, chain_r], np.r_[Gj, link_c, c1, chain_c],
               np.r_[Gx, link_x, x1, np.full(extra - 1, 3.0)])


def uniform(n=3000, per_row=8, seed=11):
    """per_row random columns a row as they come -- unsorted, repeated entries, loops -- with weights over 16 decades, a
    tenth of them zero (some -0) and a fiftieth +Inf"""
    rng = np.random.default_rng(seed)
    r = np.repeat(np.arange(n), per_row)
    c = rng.integers(0, n, len(r))
    c[::97] = r[::97]                                                 # loops
    c[1::per_row] = c[0::per_row]                                     # a repeated entry a row
    x = 10.0 ** rng.uniform(-8.0, 8.0, len(r))
    kind = rng.random(len(r))
    x[kind < 0.10] = 0.0
    x[kind < 0.02] = -0.0
    x[kind > 0.98] = np.inf
    return csr(n, r, c, x)


def positive(n=600, per_row=5, seed=5):
    """distinct columns a row, no loops, strictly positive finite weights: what scipy reads as it is written"""
    rng = np.random.default_rng(seed)
    r = np.repeat(np.arange(n), per_row)
    c = np.concatenate([rng.choice(np.delete(np.arange(n), i), per_row, replace=False) for i in range(n)])
    x = 10.0 ** rng.uniform(-6.0, 6.0, len(r))
    return csr(n, r, c, x)


def grid(n, width):
    """the road-like grid: vertex i at (i // width, i % width), edges both ways to the four neighbours that exist, the
    last line partial; unit weights (no values)"""
    i = np.arange(n, dtype=np.int64)
    right = i[(i % width != width - 1) & (i + 1 < n)]
    down = i[i + width < n]
    r = np.r_[right, right + 1, down, down + width]
    c = np.r_[right + 1, right, down + width, down]
    o = np.lexsort((c, r))
    return csr(n, r[o], c[o])


def zero_cycle():
    """source 0 -> 1 (weight 2), and the cycle 1 -> 2 -> 1 of weight 0: 1 takes the source as its parent, 2 takes -2"""
    return csr(3, [0, 1, 2], [1, 2, 1], [2.0, 0.0, 0.0])


def transposed(n, Gp, Gj, Gx):
    """the in-edge matrix (rows ascending by source, parallel edges kept): what graph.sssp_frontier_device pulls from"""
    r = np.repeat(np.arange(n, dtype=np.int64), np.diff(np.asarray(Gp, np.int64)))
    o = np.lexsort((r, Gj))
    Tp = np.zeros(n + 1, np.int32)
    np.cumsum(np.bincount(Gj, minlength=n), out=Tp[1:])
    return Tp, r[o].astype(np.int32), None if Gx is None else np.asarray(Gx)[o]
