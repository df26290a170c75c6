"""The contract of bhs_csr_scc_device (include/bhsparse_hip.h, "strongly connected components") restated in numpy, and the
inputs that tests/test_scc_abi.py and tests/test_scc_gpu.py share.

scc(n, Ap, Aj) follows the header's round as synchronous fixed points, with nothing of scipy in it, so that scipy can be the
yardstick: an entry (i, j), j != i, is the edge i -> j; an edge is valid where both ends are live and of one class.  A round
trims to a fixed point (a live vertex without a valid out-edge or without a valid in-edge is a component by itself), lowers
lab[j] to lab[i] over the valid edges from lab[v] = v until nothing moves (with the shortcut lab = lab[lab], which the
contract allows: the fixed point is the same), marks from the vertices with lab[v] == v backwards over the valid edges between
equal labels until nothing moves, decides the marked ones (root = lab) and leaves every other live vertex in the class of its
label.  A round whose trim leaves nobody ends there and counts.  Every phase's fixed point is unique, so root, comp, the
sizes, nscc AND the rounds are functions of the pattern."""
import numpy as np

import ccref
import scantiles as st


def scc(n, Ap, Aj):
    """(root int32[n], comp int32[n], sizes int32[nscc], nscc, rounds)"""
    Ap = np.asarray(Ap, np.int64)
    Aj = np.asarray(Aj, np.int64)[:Ap[n]]                            # (entries behind rowPtr[n] are not the pattern's)
    idx = np.arange(n, dtype=np.int64)
    r = np.repeat(idx, np.diff(Ap))
    off = r != Aj
    src, dst = r[off], Aj[off]
    part = np.zeros(n, np.int64)
    root = np.full(n, -1, np.int64)
    rounds = 0
    while n and np.any(part >= 0):
        rounds += 1
        while True:                                                   # 1. trim
            live = part >= 0
            valid = live[src] & live[dst] & (part[src] == part[dst])
            both = (np.bincount(src[valid], minlength=n) > 0) & (np.bincount(dst[valid], minlength=n) > 0)
            kill = live & ~both
            if not kill.any():
                break
            root[kill] = idx[kill]
            part[kill] = -1
        if not live.any():
            break
        s, t = src[valid], dst[valid]
        lab = idx.copy()                                              # 2. forward labels (a decided vertex keeps its own: it is on no valid edge)
        while True:
            nxt = lab.copy()
            np.minimum.at(nxt, t, lab[s])
            nxt = np.minimum(nxt, nxt[nxt])
            if np.array_equal(nxt, lab):
                break
            lab = nxt
        same = lab[s] == lab[t]                                       # 3. backward reach
        s, t = s[same], t[same]
        reach = live & (lab == idx)
        while True:
            nxt = reach.copy()
            nxt[s[reach[t]]] = True
            if np.array_equal(nxt, reach):
                break
            reach = nxt
        root[reach] = lab[reach]                                      # 4. decide
        part[reach] = -1
        rest = live & ~reach
        part[rest] = lab[rest]
    root = root.astype(np.int32)
    assert np.array_equal(root[root], root) and np.all(root <= idx)
    is_root = root == idx
    rank = np.cumsum(is_root) - 1
    comp = rank[root].astype(np.int32)
    nscc = int(is_root.sum())
    return root, comp, np.bincount(comp, minlength=nscc).astype(np.int32), nscc, rounds


def transposed(n, Ap, Aj):
    """(n, Ap, Aj) of the transposed pattern, repeats kept"""
    r = np.repeat(np.arange(n, dtype=np.int64), np.diff(np.asarray(Ap, np.int64)))
    return (n,) + ccref.from_edges(n, np.asarray(Aj, np.int64)[:len(r)], r)


def ring_chain(q, c, ascending):
    """(n, Ap, Aj): c one-way rings of q vertices, ring k on the vertices k q .. k q + q - 1, and a one-way bridge from ring
    k to ring k + 1 (ascending) or to ring k - 1.  root[v] = q (v // q), nscc = c, every size q.  Ascending, every ring
    behind the smallest live one takes its label and one ring is decided a round: c rounds.  Descending, every ring keeps
    its own smallest vertex: 1 round.  A weak-components answer is one component."""
    n = q * c
    v = np.arange(n, dtype=np.int64)
    k = v // q
    src, dst = v, k * q + (v - k * q + 1) % q
    heads = np.arange(c - 1, dtype=np.int64) * q
    bs, bd = (heads + q - 1, heads + q) if ascending else (heads + q, heads + q - 1)
    return (n,) + ccref.from_edges(n, np.concatenate([src, bs]), np.concatenate([dst, bd]))


def ring_chain_answer(q, c, ascending):
    """(root, comp, sizes, nscc, rounds) of ring_chain"""
    v = np.arange(q * c)
    return (q * (v // q)).astype(np.int32), (v // q).astype(np.int32), np.full(c, q, np.int32), c, c if ascending else 1


def ring_pairs(q, c, repeats=1):
    """(n, Ap, Aj, members, clique_of): scantiles.cliques(q, c)'s randomly relabelled member lists, every clique replaced by
    a one-way ring over its members in member order (q >= 2), and a one-way bridge from the smallest member of clique 2 k to
    the smallest member of clique 2 k + 1.  The depth is q and a constant whatever c.  repeats: how often a row lists its
    ring edge -- repeated columns make no difference to the answer, and the lanes a row gets follow the MEAN row length."""
    n, _, _, members, clique_of = st.cliques(q, c)
    if n == 0:
        return 0, np.zeros(1, np.int32), np.zeros(0, np.int32), members, clique_of
    assert q >= 2
    src, dst = np.repeat(members.ravel(), repeats), np.repeat(np.roll(members, -1, axis=1).ravel(), repeats)
    pairs = c // 2
    bs, bd = members[0:2 * pairs:2, 0], members[1:2 * pairs:2, 0]
    return (n,) + ccref.from_edges(n, np.concatenate([src, bs]), np.concatenate([dst, bd])) + (members, clique_of)


def ring_pairs_answer(q, c):
    """(root, comp, sizes, nscc, rounds): the root is the ring's smallest member, the number its rank among them, every size
    q; a second round where the ring a bridge leaves holds a smaller vertex than the ring it enters, whose label that ring
    then takes"""
    n, _, _, members, clique_of = st.cliques(q, c)
    if n == 0:
        return np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros(0, np.int32), 0, 0
    rank = np.empty(c, np.int64)
    rank[np.argsort(members[:, 0])] = np.arange(c)
    pairs = c // 2
    two = bool(np.any(members[0:2 * pairs:2, 0] < members[1:2 * pairs:2, 0]))
    return members[clique_of, 0].astype(np.int32), rank[clique_of].astype(np.int32), np.full(c, q, np.int32), c, 2 if two else 1


def one_way_ring(n=2048, seed=3):
    """(n, Ap, Aj): one ring of n vertices, every edge one way, under default_rng(seed).permutation: one component of depth n"""
    p = np.random.default_rng(seed).permutation(n)
    return (n,) + ccref.from_edges(n, p, np.roll(p, -1))


def one_way_path(n=3000):
    """(n, Ap, Aj): 0 -> 1 -> ... -> n - 1: n components, trimmed from both ends"""
    v = np.arange(n - 1, dtype=np.int64)
    return (n,) + ccref.from_edges(n, v, v + 1)


def random_graph(n, m, seed):
    """(n, Ap, Aj): m random directed entries"""
    rng = np.random.default_rng(seed)
    return (n,) + ccref.from_edges(n, rng.integers(0, n, m), rng.integers(0, n, m))


BY_HAND_ROOT = [0, 0, 0, 3, 3, 5, 6, 7, 8]
BY_HAND_COMP = [0, 0, 0, 1, 1, 2, 3, 4, 5]
BY_HAND_SIZES = [3, 2, 1, 1, 1, 1]


def by_hand():
    """nine vertices: the 3-cycle 0 -> 1 -> 2 -> 0 (0 -> 1 stored twice: a repeated column) feeds the 2-cycle 3 <-> 4 through
    2 -> 3, so that {3, 4} takes the label 0 in the first round and is decided in the second; 5 has a self-loop and an edge
    into the 2-cycle and nothing enters it; 6 is isolated; 4 -> 7 -> 8 is a one-way tail"""
    rows = [[1, 1], [2], [0, 3], [4], [3, 7], [5, 3], [], [8], []]
    Ap = np.zeros(10, np.int32)
    np.cumsum([len(r) for r in rows], out=Ap[1:])
    return 9, Ap, np.array([c for r in rows for c in r], np.int32)
