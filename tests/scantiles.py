"""The inputs and the numpy references of tests/test_scan_tiles_gpu.py, and what tests/test_scan_tiles_shapes.py asserts of
them on the CPU: the shapes at which the five scans of the graph and solver families (the push product's two, the
aggregation's, the colouring's and the level sets' order) cover more than one 8192-count tile, none, one count, exactly a
tile, several tiles and a remainder, and just under a tile -- in that order, on one handle.

Everything is made once per session (`cached`) and shared by both builds: the values are small integers or dyadic numbers
that both value types hold exactly, so one float64 reference serves float and double.  `SECONDS` books the CPU time of the
references per family."""
import time

import numpy as np
import scipy.sparse as sp

import aggref as ar
import gsref as gr
import iluref as ir
import pushref as pr
import spmvref
import spmvsrref

SCAN_TILE = 8192                                   # kScan1Tile (csrc/bhs_kernels.hip.h)
ROLES = ("above", "empty", "one", "exact", "several", "under")
COUNTS = (SCAN_TILE + 1, 0, 1, SCAN_TILE, 3 * SCAN_TILE + 5, SCAN_TILE - 1)   # T of the aggregation's and of the push's scans
# c disjoint cliques K_q: ncolors = nlevels = q, T = q * ceil(q c / 64); a seventh step regrows past a tile with an n that is
# no multiple of 64
CLIQUES = ((64, 129), (0, 0), (1, 1), (64, 128), (64, 385), (64, 127), (65, 126))
CLIQUE_ROLES = ROLES + ("above",)
REFUSE_AFTER = ROLES.index("exact")                # the refused calls come between this step and the next
COLOURINGS = ((0, False), (1, False), (99, True))  # (seed, caller priorities): the sweep runs on the last one's arrays
GREEDY_AT = (64, 129)                              # where the closed form is compared with gsref.colouring
OMEGA = 0.5
N_COLS = 1500                                      # columns of the CSR x dense products' matrix
PUSH_M = 3000                                      # rows of the push product's G, and its columns in the frontier series
PUSH_SHORT = 100                                   # the frontier of the row-map series

_CACHE = {}
SECONDS = {}


def cached(key, make, family=None):
    """make() once per session; its time is booked under `family` (a reference) or not at all (an input)"""
    if key not in _CACHE:
        t0 = time.perf_counter()
        _CACHE[key] = make()
        if family:
            SECONDS[family] = SECONDS.get(family, 0.0) + time.perf_counter() - t0
    return _CACHE[key]


def words(n):
    return (n + 63) // 64


def role_of(T):
    """where a scanned count lies against the tile multiples"""
    if T == 0:
        return "empty"
    if T == 1:
        return "one"
    if T == SCAN_TILE:
        return "exact"
    if SCAN_TILE - 64 <= T < SCAN_TILE:
        return "under"
    if SCAN_TILE < T < 2 * SCAN_TILE:
        return "above"
    if T > 2 * SCAN_TILE and T % SCAN_TILE:
        return "several"
    return None


# ---------------------------------------------------------------- cliques: the colouring, the levels, the sweep, the solve
def cliques(q, c):
    """(n, Sp, Sj, members, clique_of): c disjoint K_q with their diagonals under a random relabelling, rows ascending;
    members[k] the sorted vertices of clique k"""
    def make():
        n = q * c
        if n == 0:
            return 0, np.zeros(1, np.int32), np.zeros(0, np.int32), np.zeros((0, 0), np.int64), np.zeros(0, np.int64)
        perm = np.random.default_rng(7000 + n).permutation(n)
        members = np.sort(perm.reshape(c, q), axis=1)
        clique_of = np.empty(n, np.int64)
        clique_of[perm] = np.arange(n) // q
        return n, (np.arange(n + 1) * q).astype(np.int32), members[clique_of].ravel().astype(np.int32), members, clique_of
    return cached(("cliques", q, c), make)


def clique_T(q, c):
    return q * words(q * c)


def priorities(n):
    return np.random.default_rng(5).integers(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32)


def closed_form_colouring(q, c, seed, prio=None):
    """On disjoint cliques first fit in descending key order gives a vertex its rank by descending key inside its clique, a
    round colours one vertex a clique: (color, ncolors, order, colorPtr, rounds) as gsref.colouring returns them"""
    n, Sp, Sj, _, clique_of = cliques(q, c)
    if n == 0:
        return gr.colouring(0, Sp, Sj)
    by_clique_and_key = np.lexsort((ar.keys(n, seed, prio), clique_of))
    color = np.empty(n, np.int32)
    color[by_clique_and_key] = q - 1 - np.arange(n) % q
    order, ptr = gr.order_of(color)
    return color, q, order, ptr, q


def colouring(step, which):
    q, c = CLIQUES[step]
    seed, with_prio = COLOURINGS[which]
    prio = priorities(q * c) if with_prio else None
    return prio, cached(("colouring", step, which), lambda: closed_form_colouring(q, c, seed, prio), "colouring")


def greedy_colouring():
    """gsref.colouring itself at GREEDY_AT, seed 0"""
    n, Sp, Sj, _, _ = cliques(*GREEDY_AT)
    return cached("greedy", lambda: gr.colouring(n, Sp, Sj, COLOURINGS[0][0]), "colouring")


def levels(step, upper):
    n, Sp, Sj, _, _ = cliques(*CLIQUES[step])
    return cached(("levels", step, upper), lambda: ir.levels(n, Sp, Sj, upper), "levels")


def sweep_case(step):
    """(Ax, diag, b, x0, x after one symmetric sweep with OMEGA on the last colouring of COLOURINGS).  The pattern is the
    cliques'; off the diagonal only a matching holds values that are not zero (the vertices at places 2 t and 2 t + 1 of a
    clique, integers of magnitude 1 .. 3 each way), the diagonal is 1, 2 or 4, b and x0 are integers in [-8, 8].  A row's
    sum is one product among zeros and a row depends on its partner alone, so after the four updates of a pair every value
    is an integer over 1024 of fewer than 24 bits: exact in both value types in whatever order the device sums."""
    q, c = CLIQUES[step]
    n, Sp, Sj, members, clique_of = cliques(q, c)

    def make():
        rng = np.random.default_rng(1000 + step)
        r = np.repeat(np.arange(n), q)
        place = np.empty(n, np.int64)
        place[members.ravel()] = np.arange(n) % q
        other = place ^ 1
        partner = np.where(other < q, members[clique_of, np.minimum(other, q - 1)], -1) if n else np.zeros(0, np.int64)
        Ax = np.zeros(len(Sj))
        on_diag, on_pair = r == Sj, Sj == partner[r]
        Ax[on_diag] = rng.choice([1.0, 2.0, 4.0], n)
        Ax[on_pair] = rng.integers(1, 4, int(on_pair.sum())) * rng.choice([-1.0, 1.0], int(on_pair.sum()))
        diag = Ax[on_diag].copy()
        b = rng.integers(-8, 9, n).astype(np.float64)
        x0 = rng.integers(-8, 9, n).astype(np.float64)
        _, (_, _, order, ptr, _) = colouring(step, len(COLOURINGS) - 1)
        want = gr.sweep(Sp, Sj, Ax, diag, ptr, order, b, x0, OMEGA, 1, gr.SYMMETRIC)
        assert np.array_equal(want * 1024.0, np.round(want * 1024.0)) and np.all(np.abs(want) * 1024.0 < 2.0 ** 24)
        assert n < 2 or not np.array_equal(want, x0)
        return Ax, diag, b, x0, want
    return cached(("sweep", step), make, "sweep")


def solve_case(step):
    """(Ax, x*, b of the lower solve, b of the upper solve with a unit diagonal) for alpha = 1/2, chosen as
    test_trsv_gpu.exact_case chooses them: off-diagonal entries integers in [-3, 3], diagonals 1/2, 1, 2 or 4, x* integers in
    [-8, 8], b = 2 T x* -- iluref.trsv returns x* (asserted here), and so must the device, bit for bit in both builds"""
    q, c = CLIQUES[step]
    n, Sp, Sj, _, _ = cliques(q, c)

    def make():
        rng = np.random.default_rng(2000 + step)
        r = np.repeat(np.arange(n), q)
        Ax = rng.integers(-3, 4, len(Sj)).astype(np.float64)
        Ax[r == Sj] = rng.choice([0.5, 1.0, 2.0, 4.0], n)
        xs = rng.integers(-8, 9, n).astype(np.float64)
        A = sp.csr_matrix((Ax, Sj, Sp), shape=(n, n))
        bl, bu = 2.0 * (sp.tril(A) @ xs), 2.0 * (sp.triu(A, 1) @ xs + xs)
        for upper, b in ((False, bl), (True, bu)):
            _, _, order, ptr = levels(step, upper)
            assert np.array_equal(ir.trsv(n, Sp, Sj, Ax, ptr, order, b, np.zeros(n), 0.5, upper, unit_diag=upper), xs)
        return Ax, xs, bl, bu
    return cached(("solve", step), make, "solve")


# ---------------------------------------------------------------- the aggregation
def band(n, w):
    """(n, Sp, Sj): every vertex joined to those within w of it, with the diagonal: the path for w = 1 (mean degree 3),
    mean degree 2 w + 1"""
    def make():
        j = np.arange(n, dtype=np.int64)[:, None] + np.arange(-w, w + 1)[None, :]
        ok = (j >= 0) & (j < n)
        Sp = np.zeros(n + 1, np.int32)
        np.cumsum(ok.sum(axis=1), out=Sp[1:])
        return n, Sp, j[ok].astype(np.int32)
    return cached(("band", n, w), make)


def agg_n(step):
    T = COUNTS[step]
    return 64 * T - (3 if T and T != SCAN_TILE else 0)


# (step, half band width): the path at every step, and at the first one a band of mean degree 7 -- four lanes a row
AGG_CASES = tuple((s, 1) for s in range(len(COUNTS))) + ((0, 3),)


def agg_reference(step, w, seed):
    n, Sp, Sj = band(agg_n(step), w)
    return cached(("agg", step, w, seed), lambda: ar.aggregate(n, Sp, Sj, seed), "aggregation")


# ---------------------------------------------------------------- the push product
def push_graph(n, seed):
    """(m, n, Gp, Gj, Gx): PUSH_M rows of 0 .. 5 entries at random columns, in no order and with repeats; values 1 .. 9
    (30 empty rows for n = 0)"""
    def make():
        rng = np.random.default_rng(seed)
        m = PUSH_M if n else 30
        lens = rng.integers(0, 6, m) if n else np.zeros(m, np.int64)
        Gp = np.zeros(m + 1, np.int32)
        np.cumsum(lens, out=Gp[1:])
        Gj = rng.integers(0, max(n, 1), Gp[-1]).astype(np.int32)
        return m, n, Gp, Gj, rng.integers(1, 10, len(Gj)).astype(np.float64)
    return cached(("G", n, seed), make)


def push_cases():
    """(series, step, n, nf, semiring, k): the frontier series -- nf takes COUNTS on PUSH_M columns, one tile of row-map words
    -- and the row-map series -- n = 64 T (less 3 off the exact size) under a frontier of PUSH_SHORT"""
    out = []
    for step, T in enumerate(COUNTS):
        out.append(("frontier", step, PUSH_M, T, "min_plus", 1))
        if T <= SCAN_TILE + 1:
            out.append(("frontier", step, PUSH_M, T, "or_and", 4))
    for step, T in enumerate(COUNTS):
        n = agg_n(step)
        out.append(("rowmap", step, n, PUSH_SHORT if n else 3, "min_plus", 1))
        out.append(("rowmap", step, n, PUSH_SHORT if n else 3, "or_and", 4 if T in (1, SCAN_TILE - 1) else 1))
    return out


def push_inputs(case):
    """(G, fidx, F, Y): the list names rows more than once; min_plus on integers and +Inf, or_and on 0, 1 and 2"""
    series, step, n, nf, name, k = case

    def make():
        G = push_graph(n, 300 + (step if series == "rowmap" else 0))
        rng = np.random.default_rng(400 + 10 * step + (series == "rowmap") + 2 * (name == "or_and"))
        fidx = rng.integers(0, G[0], nf).astype(np.int32)
        if nf > 3:
            fidx[nf // 2] = fidx[0]
        if name == "min_plus":
            F = rng.integers(0, 20, (nf, k)).astype(np.float64)
            Y = np.where(rng.random((n, k)) < 0.7, np.inf, rng.integers(0, 30, (n, k)).astype(np.float64))
        else:
            F = rng.integers(0, 3, (nf, k)).astype(np.float64)
            Y = (rng.random((n, k)) < 0.2).astype(np.float64)
        return G, fidx, F, Y
    return cached(("push inputs",) + tuple(case), make)


def push_reference(case):
    G, fidx, F, Y = push_inputs(case)
    m, n, Gp, Gj, Gx = G
    return cached(("push",) + tuple(case), lambda: pr.push_semiring(case[4], m, n, Gp, Gj, Gx, fidx, F, Y), "push")


def push_scan_rows(case, want_next):
    """what the record push_scan books: the frontier's degrees, and the row map's words where a list is asked for"""
    return case[3] + (words(case[2]) if want_next else 0)


# ---------------------------------------------------------------- CSR x dense, plain and over a semiring
def dense_case(step):
    """(m, A, x, X of three columns, y): m the step's clique vertices, 0 .. 5 entries a row, integers"""
    m = CLIQUES[step][0] * CLIQUES[step][1]

    def make():
        rng = np.random.default_rng(500 + step)
        lens = rng.integers(0, 6, m)
        Ap = np.zeros(m + 1, np.int32)
        np.cumsum(lens, out=Ap[1:])
        Aj = rng.integers(0, N_COLS, Ap[-1]).astype(np.int32)
        Ax = rng.integers(1, 10, len(Aj)).astype(np.float64)
        return (m, (Ap, Aj, Ax), rng.integers(-9, 10, (N_COLS, 1)).astype(np.float64),
                rng.integers(-9, 10, (N_COLS, 3)).astype(np.float64), rng.integers(-9, 10, (m, 1)).astype(np.float64))
    return cached(("dense", step), make)


def dense_references(step):
    """(2 A x - y, 2 A X, y min= A min.+ x with its count of changed elements)"""
    m, (Ap, Aj, Ax), x, X, y = dense_case(step)

    def make():
        return (spmvref.spmm(m, N_COLS, Ap, Aj, Ax, x, 2.0, -1.0, y)[0], spmvref.spmm(m, N_COLS, Ap, Aj, Ax, X, 2.0)[0],
                spmvsrref.spmm_semiring("min_plus", m, N_COLS, Ap, Aj, Ax, x, y, None, True))
    return cached(("dense references", step), make, "CSR x dense")
