"""The contract of bhs_csr_spanning_forest_device (include/bhsparse_hip.h, "spanning forest") restated in numpy, and the inputs
that tests/test_forest_abi.py and tests/test_forest_gpu.py share.

kruskal(n, Ap, Aj, Ax, flags) is the definition: a union-find over the distinct edges sorted by the integer key (k(w), lo, hi),
both words complemented under MAXIMUM.  It returns the forest's edges sorted by (lo, hi).

sync_rounds(n, Ap, Aj, Ax, flags) is the device's synchronous rounds -- pick, hook, flatten -- and predicts what the call
returns beyond the forest itself: the labels, the slot order of the edge list and the number of rounds that hooked.  It also
counts the doublings the deepest hook chain of any round needed against ceil(log2 R), the launches the host issues.

The weight makers are seeded and give small integers and dyadic fractions: exact in float, so both builds see one input."""
import functools

import numpy as np

MAXIMUM, ABS = 1, 2
FLAGS = (0, MAXIMUM, ABS, MAXIMUM | ABS)
NONE = np.uint64(0xFFFFFFFFFFFFFFFF)
SIGN = np.uint64(1 << 63)


def weight_key(w):
    """rd_key(x, false) of csrc/bhs_reduce.hip.h on float64 (no NaN): unsigned order == order of the numbers, -0 below +0"""
    b = np.ascontiguousarray(w, np.float64).view(np.uint64)
    return np.where(b >> np.uint64(63) != 0, ~b, b | SIGN)


def weight_unkey(k):
    k = np.ascontiguousarray(k, np.uint64)
    return np.where(k >> np.uint64(63) != 0, k & ~SIGN, ~k).view(np.float64)


def edges(n, Ap, Aj, Ax=None, flags=0):
    """(r, c, kw, ke) of every entry that is an edge: j != i and the weight not NaN; the two key words as the device compares them"""
    Ap, Aj = np.asarray(Ap, np.int64), np.asarray(Aj, np.int64)
    r = np.repeat(np.arange(n, dtype=np.int64), np.diff(Ap))
    w = np.ones(len(Aj)) if Ax is None else np.asarray(Ax, np.float64).copy()
    if flags & ABS:
        w = np.abs(w)
    ok = (r != Aj) & ~np.isnan(w)
    r, c, w = r[ok], Aj[ok], w[ok]
    kw = weight_key(w)
    ke = (np.minimum(r, c).astype(np.uint64) << np.uint64(32)) | np.maximum(r, c).astype(np.uint64)
    if flags & MAXIMUM:
        kw, ke = ~kw, ~ke
    return r, c, kw, ke


def decode(kw, ke, flags):
    """(lo, hi, w) of key words"""
    if flags & MAXIMUM:
        kw, ke = ~kw, ~ke
    return (ke >> np.uint64(32)).astype(np.int64), (ke & np.uint64(0xFFFFFFFF)).astype(np.int64), weight_unkey(kw)


def by_lo_hi(lo, hi, w):
    order = np.lexsort((hi, lo))
    return lo[order].astype(np.int32), hi[order].astype(np.int32), w[order]


def kruskal(n, Ap, Aj, Ax=None, flags=0):
    """(lo int32[m], hi int32[m], w float64[m]) sorted by (lo, hi): THE forest"""
    _, _, kw, ke = edges(n, Ap, Aj, Ax, flags)
    both = np.unique(np.stack([kw, ke], axis=1), axis=0)              # ascending (kw, ke); equal tuples are one edge
    lo, hi, w = decode(both[:, 0], both[:, 1], flags)
    up = list(range(n))

    def find(x):
        while up[x] != x:
            up[x] = up[up[x]]
            x = up[x]
        return x
    take = []
    for t, (a, b) in enumerate(zip(lo.tolist(), hi.tolist())):
        ra, rb = find(a), find(b)
        if ra != rb:
            up[ra] = rb
            take.append(t)
    take = np.asarray(take, np.int64)
    return by_lo_hi(lo[take], hi[take], w[take])


def sync_rounds(n, Ap, Aj, Ax=None, flags=0):
    """(label int32[n], lo, hi, w in slot order, nedges, rounds, info): info["jumps"] the doublings every round needed,
    info["allowed"] ceil(log2 R) of that round, info["hooks"] the trees it hooked"""
    r, c, kw, ke = edges(n, Ap, Aj, Ax, flags)
    label = np.arange(n, dtype=np.int64)
    slot_lo = np.full(n, -1, np.int64)
    slot_hi = np.full(n, -1, np.int64)
    slot_w = np.zeros(n)
    info = {"jumps": [], "allowed": [], "hooks": []}
    roots, nrounds = n, 0
    while True:
        lr, lc = label[r], label[c]
        cross = lr != lc
        if not cross.any():
            break
        # pick: the least (kw, ke) over the entries that cross a tree's boundary, seen from both ends
        t = np.concatenate([lr[cross], lc[cross]])
        w2, e2 = np.concatenate([kw[cross]] * 2), np.concatenate([ke[cross]] * 2)
        order = np.lexsort((e2, w2, t))
        t, w2, e2 = t[order], w2[order], e2[order]
        first = np.concatenate([[True], t[1:] != t[:-1]])
        bestW, bestE = np.full(n, NONE), np.full(n, NONE)
        pick = t[first]
        bestW[pick], bestE[pick] = w2[first], e2[first]
        # hook
        lo, hi, w = decode(bestW[pick], bestE[pick], flags)
        llo, lhi = label[lo], label[hi]
        assert np.all((llo == pick) != (lhi == pick))
        far = np.where(llo == pick, lhi, llo)
        stay = (bestW[far] == bestW[pick]) & (bestE[far] == bestE[pick]) & (pick < far)
        parent = np.arange(n, dtype=np.int64)
        hook = ~stay
        assert hook.any() and np.all(slot_lo[pick[hook]] == -1)
        parent[pick[hook]] = far[hook]
        slot_lo[pick[hook]], slot_hi[pick[hook]], slot_w[pick[hook]] = lo[hook], hi[hook], w[hook]
        # flatten
        jumps = 0
        while True:
            nxt = parent[parent]
            if np.array_equal(nxt, parent):
                break
            parent = nxt
            jumps += 1
            assert jumps <= 64, "a cycle in the hook graph"
        allowed = int(np.ceil(np.log2(roots))) if roots > 1 else 0
        assert jumps <= allowed
        info["jumps"].append(jumps)
        info["allowed"].append(allowed)
        info["hooks"].append(int(hook.sum()))
        label = parent[label]
        nrounds += 1
        roots -= int(hook.sum())
    used = slot_lo >= 0
    assert np.array_equal(label[label], label)
    return (label.astype(np.int32), slot_lo[used].astype(np.int32), slot_hi[used].astype(np.int32), slot_w[used], int(used.sum()),
            nrounds, info)


def same_partition(a, b):
    """do two labellings put the same vertices together"""
    a, b = np.asarray(a, np.int64), np.asarray(b, np.int64)
    if len(a) != len(b):
        return False
    pairs = np.unique(np.stack([a, b], axis=1), axis=0)
    return len(pairs) == len(np.unique(a)) == len(np.unique(b))


def bits(w, dtype=np.float64):
    return np.ascontiguousarray(w, dtype).tobytes()


# ---------------------------------------------------------------- weights
def _pairs(n, Ap, Aj):
    """(index of every entry's undirected pair among the distinct pairs, their number)"""
    Ap, Aj = np.asarray(Ap, np.int64), np.asarray(Aj, np.int64)
    r = np.repeat(np.arange(n, dtype=np.int64), np.diff(Ap))
    key = np.minimum(r, Aj) * n + np.maximum(r, Aj)
    uniq, inv = np.unique(key, return_inverse=True)
    return inv.reshape(-1), len(uniq)


def w_distinct(n, Ap, Aj, seed=3):
    """symmetric, a different weight for every pair: quarters"""
    inv, m = _pairs(n, Ap, Aj)
    return (np.random.default_rng(seed).permutation(m)[inv] + 1) * 0.25


def w_ties(n, Ap, Aj, seed=4):
    """symmetric, 1 .. 3"""
    inv, m = _pairs(n, Ap, Aj)
    return np.random.default_rng(seed).integers(1, 4, m)[inv].astype(np.float64)


def w_asymmetric(n, Ap, Aj, seed=5):
    """an independent draw per stored entry: halves in [-4, 4]"""
    return np.random.default_rng(seed).integers(-8, 9, len(Aj)) * 0.5


def w_specials(n, Ap, Aj, seed=6):
    """w_asymmetric with NaN, +-Inf, +-0 and negatives over 10 % of the entries"""
    rng = np.random.default_rng(seed)
    w = w_asymmetric(n, Ap, Aj, seed + 100)
    at = rng.random(len(Aj)) < 0.10
    w[at] = rng.choice(np.array([np.nan, np.inf, -np.inf, 0.0, -0.0, -1.5, -3.0]), int(at.sum()))
    return w


MAKERS = {"distinct": w_distinct, "ties": w_ties, "asymmetric": w_asymmetric, "specials": w_specials, "none": None}


# ---------------------------------------------------------------- inputs
def by_hand():
    """the case of the header's tests: (0,1) 2, (1,0) 5, (1,2) 2, (2,3) NaN, (3,2) -0, (2,4) +0, (3,4) 1, (0,4) 2, (5,5) -7"""
    rows = [[(1, 2.0), (4, 2.0)], [(0, 5.0), (2, 2.0)], [(3, np.nan), (4, 0.0)], [(2, -0.0), (4, 1.0)], [], [(5, -7.0)]]
    Ap = np.zeros(7, np.int32)
    np.cumsum([len(r) for r in rows], out=Ap[1:])
    return (6, Ap, np.array([c for r in rows for c, _ in r], np.int32), np.array([v for r in rows for _, v in r], np.float64))


def increasing_path(n=300):
    """(n, Ap, Aj, Ax): the path with edge {i, i + 1} of weight i + 1, stored both ways, with the diagonal"""
    import aggref
    m, Ap, Aj = aggref.gpu_cases()["path300"]
    assert m == n
    r = np.repeat(np.arange(n), np.diff(Ap))
    return n, Ap, Aj, (np.minimum(r, Aj) + 1).astype(np.float64)


PATTERNS = ("one_with_diag", "two_one_edge", "path300", "poisson5pt_33", "poisson27pt_9", "uniform2048", "powerlaw3000", "star1024",
            "two_k70", "random_directed", "no_entries", "star_centre_last")


@functools.lru_cache(maxsize=None)
def pattern(name):
    import aggref
    import ccref
    if name in ("random_directed", "no_entries", "star_centre_last"):
        n, Ap, Aj = getattr(ccref, name).__wrapped__()                # arrays of this module's own: ccref's cached ones are shared
        Ap.setflags(write=False)
        Aj.setflags(write=False)
        return n, Ap, Aj
    return aggref.gpu_cases()[name]


@functools.lru_cache(maxsize=None)
def weights(name, maker):
    f = MAKERS[maker]
    return None if f is None else f(*pattern(name))


@functools.lru_cache(maxsize=None)
def reference(name, maker, flags):
    n, Ap, Aj = pattern(name)
    return sync_rounds(n, Ap, Aj, weights(name, maker), flags)


def random_multigraph(rng):
    """(n, Ap, Aj, Ax): n < 60, asymmetric, repeated columns, diagonals, heavily tied weights with specials"""
    n = int(rng.integers(1, 60))
    m = int(rng.integers(0, 4 * n + 1))
    src, dst = rng.integers(0, n, m), rng.integers(0, n, m)
    order = np.argsort(src, kind="stable")
    Ap = np.zeros(n + 1, np.int32)
    np.cumsum(np.bincount(src, minlength=n), out=Ap[1:])
    pool = np.array([np.nan, np.inf, -np.inf, 0.0, -0.0, -2.0, -0.5, 0.5, 1.0, 1.0, 1.0, 2.0, 2.0, 3.0])
    return n, Ap, dst[order].astype(np.int32), rng.choice(pool, m)
