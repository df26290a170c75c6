"""The contract of bhs_csr_components_device (include/bhsparse_hip.h, "connected components") restated in numpy, and the
patterns that tests/test_components_abi.py and tests/test_components_gpu.py share.

components(n, Ap, Aj) is the definition: i and j are joined where the pattern stores (i, j) or (j, i); root[i] is the smallest
vertex of i's component, comp[i] the rank of root[i] among the roots, sizes[c] the number of vertices with comp == c.  It is a
union-find with nothing of scipy in it, so that scipy can be the yardstick.

sync_passes(n, Ap, Aj) is the pass of csrc/bhs_components.hip.h as synchronous rounds -- every read of a round sees the
array as the round found it: both ends of every entry are lowered to the smaller of the two parents, the old parent of i is
lowered to the minimum over row i (hooking), parent = parent[parent] twice (pointer jumping).  It returns the number of
rounds up to and including the first that changes nothing.  (The device hooks one step further up, at the grandparent, which
measured faster; the restatement is the yardstick for "a pass that jumps", not a copy of the kernel.)"""
import functools

import numpy as np

REPEATS = 170                                      # how often a leaf of star_centre_last lists the centre


def components(n, Ap, Aj):
    """(root int32[n], comp int32[n], sizes int32[ncomp], ncomp)"""
    Ap, Aj = np.asarray(Ap, np.int64), np.asarray(Aj, np.int64)
    up = np.arange(n, dtype=np.int64)
    r = np.repeat(np.arange(n, dtype=np.int64), np.diff(Ap))
    # union by minimum, vectorised: every set's representative is lowered to the smallest representative an edge shows it,
    # paths are halved until nothing moves (exact whatever the order: the fixed point is the definition)
    while True:
        a, b = up[r], up[Aj]
        lo = np.minimum(a, b)
        nxt = up.copy()
        np.minimum.at(nxt, a, lo)
        np.minimum.at(nxt, b, lo)
        nxt = nxt[nxt]
        if np.array_equal(nxt, up):
            break
        up = nxt
    root = up.astype(np.int32)
    assert np.array_equal(root[root], root) and np.all(root <= np.arange(n))
    is_root = root == np.arange(n)
    rank = np.cumsum(is_root) - 1
    comp = rank[root].astype(np.int32)
    ncomp = int(is_root.sum())
    sizes = np.bincount(comp, minlength=ncomp).astype(np.int32)
    return root, comp, sizes, ncomp


def sync_passes(n, Ap, Aj):
    Ap, Aj = np.asarray(Ap, np.int64), np.asarray(Aj, np.int64)
    r = np.repeat(np.arange(n, dtype=np.int64), np.diff(Ap))
    parent = np.arange(n, dtype=np.int64)
    passes = 0
    while True:
        passes += 1
        old = parent
        a, b = old[r], old[Aj]
        lo = np.minimum(a, b)
        nxt = old.copy()
        np.minimum.at(nxt, r, lo)                                    # both ends of every entry
        np.minimum.at(nxt, Aj, lo)
        m = old.copy()
        np.minimum.at(m, r, lo)                                      # the row's minimum ...
        np.minimum.at(nxt, old, m)                                   # ... hooks the old parent
        nxt = np.minimum(nxt, nxt[nxt])                              # two shortcuts
        nxt = np.minimum(nxt, nxt[nxt])
        if np.array_equal(nxt, old):
            return passes
        parent = nxt


def from_edges(n, src, dst):
    """(Ap, Aj) with entry (src, dst) for every pair, in the order given inside a row"""
    src, dst = np.asarray(src, np.int64), np.asarray(dst, np.int64)
    order = np.argsort(src, kind="stable")
    Ap = np.zeros(n + 1, np.int32)
    np.cumsum(np.bincount(src, minlength=n), out=Ap[1:])
    return Ap, dst[order].astype(np.int32)


@functools.lru_cache(maxsize=None)
def relabelled_path(n=32768, seed=1):
    """(n, Ap, Aj): the path 0 - 1 - ... - n-1 under default_rng(seed).permutation, both directions stored"""
    p = np.random.default_rng(seed).permutation(n)
    a, b = p[:-1], p[1:]
    return (n,) + from_edges(n, np.concatenate([a, b]), np.concatenate([b, a]))


@functools.lru_cache(maxsize=None)
def random_directed(n=20000, m=12000, seed=5):
    """(n, Ap, Aj): m random directed entries, the last 200 of them repeats of the first 200: not symmetric, thousands of
    components"""
    rng = np.random.default_rng(seed)
    src, dst = rng.integers(0, n, m - 200), rng.integers(0, n, m - 200)
    return (n,) + from_edges(n, np.concatenate([src, src[:200]]), np.concatenate([dst, dst[:200]]))


@functools.lru_cache(maxsize=None)
def no_entries(n=1000):
    return n, np.zeros(n + 1, np.int32), np.zeros(0, np.int32)


@functools.lru_cache(maxsize=None)
def star_centre_last(leaves=1023, isolated=500):
    """(n, Ap, Aj): a star of leaves + 1 vertices whose centre is the LAST index, stored both ways, its leaves scattered
    among `isolated` vertices without an entry.  The lanes per row follow the MEAN row length, so every leaf lists the centre
    REPEATS times (repeated columns make no difference to the answer): the mean is above 64, a row takes a whole wave, and
    the minimum, the smallest leaf, has to travel through the centre against the row order."""
    n = leaves + isolated + 1
    centre = n - 1
    leaf = np.sort(np.random.default_rng(9).choice(n - 1, leaves, replace=False))
    src = np.concatenate([np.repeat(leaf, REPEATS), np.full(leaves, centre)])
    dst = np.concatenate([np.full(REPEATS * leaves, centre), leaf])
    n, Ap, Aj = (n,) + from_edges(n, src, dst)
    assert len(Aj) > 64 * n
    return n, Ap, Aj


def by_hand():
    """seven vertices: 5 -> 2 and 2 -> 6 stored one way only, a self-loop on 3, 0 -> 1 twice (a repeated column)"""
    rows = [[1, 1], [], [6], [3], [], [2], []]
    Ap = np.zeros(8, np.int32)
    np.cumsum([len(r) for r in rows], out=Ap[1:])
    return 7, Ap, np.array([c for r in rows for c in r], np.int32)
