"""The inputs and the numpy references of tests/test_grid_pass_gpu.py, and what tests/test_grid_pass_shapes.py asserts of them
on the CPU: the sizes at which a workgroup of a capped grid takes a second turn in its block loop
(`for (t = blockIdx.x; t < nBlocks; t += gridDim.x)`).

A. The graph and solver families give a row L = 1, 4, 16 or 64 lanes (ag_lanes, from the mean row length), a workgroup
256 / L rows, and cap the grid at 16 workgroups a CU: `cap_rows(numCU, L)` is an n whose block count is 1.3 times the cap and
whose last block is partial.  The inputs are disjoint bands under a random relabelling (half-width 1, 2, 8, 33: mean row
lengths 3, 5, 17, 67); where the restatement is a Python loop over the vertices that would run for more than about ten
seconds (the colouring at L = 1 and 4, the levels at L = 1) they are scantiles.cliques(q, c) with q = 3, 5 and a closed form.

B. The long-row kernels take one workgroup a row of more than 1024 entries and cap the grid at 8 workgroups a CU:
`long_rows(numCU)` is a matrix with 8 numCU + 37 such rows.  The sampled dense-dense product takes it as its pattern at the
widths SDDMM_KS (restated SDDMM_SLICE rows at a time), the relaxation runs RELAX_CASES on `long_square`, the matrix with empty
rows behind its own, and the fused product's two reductions are those of `long_dots`.

C. k_dot_finish, one workgroup, adds the partials of the fused product's reductions DOT_TURN a turn: `dots_case(DOTS_M)` has
DOT_TURN + 1 of them, the last from a partial workgroup, and `dots_case(DOTS_M_AFTER)` two.

Everything is made once per session (`cached`, scantiles' own cache) and shared by both builds: the values are small integers
or dyadic numbers that both value types hold exactly.  `SECONDS` (scantiles') books the CPU time of the references per
family: at 256 CUs "sddmm" 2.1 to 5.8 s (1.8 s of it each at k = 64, k = 65 and k = 65 in place on the slower machine),
"relax" 1.5 to 3 s (five cases, each restated in both value types), "dots" under 0.1 s."""
import numpy as np
import scipy.sparse as sp

import aggref as ar
import ccref
import extractref as ex
import forestref as fr
import gsref as gr
import iluref as ir
import matchref as mr
import reduceref as rr
import relaxref as rx
import scantiles as st
import sddmmref as sd
import selectref as sr
import spmvref
import spmvsrref
import transposeref as tr
from scantiles import SECONDS, cached

CAP_A, CAP_B = 16, 8                               # workgroups a CU: the graph families' block loops, the long-row queues
LANES = (1, 4, 16, 64)
HALF_WIDTH = {1: 1, 4: 2, 16: 8, 64: 33}           # of the band that gives L lanes a row
CLIQUE_Q = {1: 3, 4: 5, 16: 33, 64: 65}            # of the cliques that do
PARTS = 5                                          # disjoint bands: the components
OVER = 13                                          # block count / cap, in tenths
COLOUR_ON_CLIQUES = (1, 4)                         # where gsref.colouring would run for a minute and more
LEVELS_ON_CLIQUES = (1,)                           # where iluref.levels would run for 7 s a triangle
SOLVE_AT = 16                                      # the sweep and the solves run on this L's orders
OMEGA = 0.5
LONG = 1024                                        # kSpmvWaveL, kRdWaveL, kTrWaveL, kExWaveL, kSelWaveL: a longer row is a long row
LDS_KEYS = 4096                                    # kTrLdsMax, kExLdsMax: a longer row sorts in global memory
N_COLS = 6007                                      # columns of the long-row matrix
EXTRA = 37                                         # long rows beyond the cap
SDDMM_KS = (1, 2, 3, 16, 64, 65)                   # tiles 1, 2, 4 (sd_owner's three cases), 16 and 64, and a second tile in a lane
SDDMM_IN_PLACE_KS = (3, 65)                        # ... of them under TIMES_M in place on M's values, with
SDDMM_IN_PLACE = (2.0, -1.0)                       # alpha, beta: a row done twice gives m, done once 2 s m - m
SDDMM_GAP = 3                                      # columns of NaN behind X's and Y's k
SDDMM_SLICE = 64                                   # rows of M a call of the restatement
DOT_PER = 4096                                     # kDotPer: elements a workgroup of k_dot_part, one partial each
DOT_TURN = 256                                     # partials a turn of k_dot_finish's loop: its one workgroup's threads
DOTS_M = (DOT_TURN + 1) * DOT_PER - 1000           # 257 partials, the last of a partial workgroup
DOTS_M_AFTER = DOT_PER + 1                         # two partials, with the stale ones of DOTS_M behind them
RELAX_COEF = ((0.0, 1.0), (0.5, 0.5), (0.25, 2.0), (0.5, 1.0))      # test_relax_gpu.COEF
# name: (sparse values, the steps' (a, c), is d kept, BHS_RELAX_ZERO_GUESS)
RELAX_CASES = {"one step": (False, ((0.5, 2.0),), True, False), "one step, no d": (False, ((0.0, 1.0),), False, False),
               "four steps": (True, RELAX_COEF, True, False), "four steps, zero guess": (True, RELAX_COEF, True, True),
               "jacobi": (True, ((0.0, 0.5),) * 4, False, False)}
# per L the weight makers of the matching, and (maker, flags) of the forest: every maker and both flag words are met, and the
# inputs of a million vertices twice each
MATCH_MAKERS = {1: ("ties", "specials"), 4: ("asymmetric",), 16: ("ties",), 64: ("specials",)}
FOREST_CASES = {1: (("ties", 0), ("specials", fr.MAXIMUM | fr.ABS)), 4: (("asymmetric", 0),),
                16: (("ties", 0), ("specials", fr.MAXIMUM | fr.ABS)), 64: (("asymmetric", fr.MAXIMUM | fr.ABS),)}


def blocks(n, L):
    return -(-n // (256 // L))


def cap_rows(numCU, L):
    """an n with ceil(n / (256 / L)) = ceil(1.3 * 16 numCU) whose last block is half full"""
    per = 256 // L
    return -(-OVER * CAP_A * numCU // 10) * per - (per // 2 + 1)


def clique_count(numCU, L):
    """c for scantiles.cliques(CLIQUE_Q[L], c): the smallest c with at least cap_rows vertices and a partial last block"""
    q, per = CLIQUE_Q[L], 256 // L
    c = -(-cap_rows(numCU, L) // q)
    while q * c % per == 0:
        c += 1
    return c


def sizes(numCU):
    """{L: (n of the band, (q, c) of the cliques)}, and under "long" the number of long rows"""
    out = {L: (cap_rows(numCU, L), (CLIQUE_Q[L], clique_count(numCU, L))) for L in LANES}
    out["long"] = CAP_B * numCU + EXTRA
    return out


# ---------------------------------------------------------------- A: the patterns
def relabelled_band(n, w, parts, seed):
    """(n, Sp, Sj): `parts` disjoint bands of half-width w with their diagonals under a random relabelling, rows ascending"""
    perm = np.random.default_rng(seed).permutation(n)
    size = -(-n // parts)
    i = np.arange(n, dtype=np.int64)[:, None]
    j = i + np.arange(-w, w + 1, dtype=np.int64)[None, :]
    ok = (j >= 0) & (j < n) & (j // size == i // size)
    r, c = perm[np.repeat(np.arange(n), ok.sum(axis=1))], perm[j[ok]]
    o = np.lexsort((c, r))
    Sp = np.zeros(n + 1, np.int32)
    np.cumsum(np.bincount(r, minlength=n), out=Sp[1:])
    return n, Sp, c[o].astype(np.int32)


def band(numCU, L):
    n = cap_rows(numCU, L)
    return cached(("gp band", n, L), lambda: relabelled_band(n, HALF_WIDTH[L], PARTS, 9000 + L))


def cliques(numCU, L):
    """scantiles.cliques at this L's size: (n, Sp, Sj, members, clique_of)"""
    return st.cliques(CLIQUE_Q[L], clique_count(numCU, L))


def colour_pattern(numCU, L):
    return cliques(numCU, L)[:3] if L in COLOUR_ON_CLIQUES else band(numCU, L)


def level_pattern(numCU, L):
    return cliques(numCU, L)[:3] if L in LEVELS_ON_CLIQUES else band(numCU, L)


def closed_form_levels(q, c, upper):
    """On disjoint cliques a vertex's level is its rank among its clique's members, from the other end for the upper
    triangle: (level, nlevels, order, levelPtr) as iluref.levels returns them"""
    n, _, _, members, clique_of = st.cliques(q, c)
    rank = np.empty(n, np.int64)
    rank[members.ravel()] = np.arange(n) % q
    level = q - 1 - rank if upper else rank
    order, ptr = gr.order_of(level)
    return level.astype(np.int32), q, order, ptr


# ---------------------------------------------------------------- A: the references
def counted(f, *args):
    """(f(*args), the sum of the counts f's rounds start from: the rows its round kernel's record books)"""
    counts = []
    out = f(*args, counts=counts)
    return out, sum(counts)


def aggregation(numCU, L, seed=0, rows=False):
    """the reference; rows: what agg_decide books instead -- the undecided vertices every round starts from"""
    n, Sp, Sj = band(numCU, L)
    return cached(("gp agg", n, L, seed), lambda: counted(ar.aggregate, n, Sp, Sj, seed), "aggregation")[int(rows)]


def colouring(numCU, L, seed=0, rows=False):
    """the reference; rows: what color_round books instead -- the uncoloured vertices every round starts from (on cliques a
    round colours one vertex a clique)"""
    n, Sp, Sj = colour_pattern(numCU, L)
    if L in COLOUR_ON_CLIQUES:
        q, c = CLIQUE_Q[L], clique_count(numCU, L)
        return cached(("gp colouring", n, L, seed), lambda: (st.closed_form_colouring(q, c, seed), c * q * (q + 1) // 2),
                      "colouring")[int(rows)]
    return cached(("gp colouring", n, L, seed), lambda: counted(gr.colouring, n, Sp, Sj, seed, None), "colouring")[int(rows)]


def levels(numCU, L, upper):
    n, Sp, Sj = level_pattern(numCU, L)
    if L in LEVELS_ON_CLIQUES:
        return cached(("gp levels", n, L, upper), lambda: closed_form_levels(CLIQUE_Q[L], clique_count(numCU, L), upper), "levels")
    return cached(("gp levels", n, L, upper), lambda: ir.levels(n, Sp, Sj, upper), "levels")


def components(numCU, L):
    n, Sp, Sj = band(numCU, L)
    return cached(("gp components", n, L), lambda: ccref.components(n, Sp, Sj), "components")


def weights(numCU, L, maker):
    n, Sp, Sj = band(numCU, L)
    return cached(("gp weights", n, L, maker), lambda: fr.MAKERS[maker](n, Sp, Sj))


def match_makers(L):
    return MATCH_MAKERS[L]


def forest_cases(L):
    return FOREST_CASES[L]


def matching(numCU, L, maker, seed=0, rows=False):
    """the reference; rows: what match_round books instead -- the undecided vertices every round starts from and those the
    last one leaves to k_mt_finish"""
    n, Sp, Sj = band(numCU, L)
    return cached(("gp match", n, L, maker, seed), lambda: counted(mr.match, n, Sp, Sj, weights(numCU, L, maker), seed),
                  "matching")[int(rows)]


def forest(numCU, L, maker, flags):
    n, Sp, Sj = band(numCU, L)
    return cached(("gp forest", n, L, maker, flags), lambda: fr.sync_rounds(n, Sp, Sj, weights(numCU, L, maker), flags), "forest")


def sweep_case(numCU, L):
    """(Ax, diag, b, x0, x after one symmetric sweep with OMEGA on colouring(numCU, L)'s order), chosen as
    scantiles.sweep_case chooses them: on the band's pattern only a matching holds off-diagonal values that are not zero
    (the vertices at places 2 t and 2 t + 1 of a band, integers of magnitude 1 .. 3 each way), the diagonal is 1, 2 or 4, b
    and x0 are integers in [-8, 8] -- every value an integer over 1024 of fewer than 24 bits, in whatever order the device
    sums."""
    n, Sp, Sj = band(numCU, L)

    def make():
        rng = np.random.default_rng(1000 + L)
        perm = np.random.default_rng(9000 + L).permutation(n)         # (relabelled_band's)
        size = -(-n // PARTS)
        place = np.empty(n, np.int64)
        place[perm] = np.arange(n)
        other = place ^ 1
        paired = (other < n) & (other // size == place // size)
        partner = np.where(paired, perm[np.minimum(other, n - 1)], -1)
        r = np.repeat(np.arange(n), np.diff(Sp))
        Ax = np.zeros(len(Sj))
        on_diag, on_pair = r == Sj, Sj == partner[r]
        assert on_diag.sum() == n and on_pair.sum() == paired.sum()
        Ax[on_diag] = rng.choice([1.0, 2.0, 4.0], n)
        Ax[on_pair] = rng.integers(1, 4, int(on_pair.sum())) * rng.choice([-1.0, 1.0], int(on_pair.sum()))
        diag = Ax[on_diag].copy()
        b = rng.integers(-8, 9, n).astype(np.float64)
        x0 = rng.integers(-8, 9, n).astype(np.float64)
        _, _, order, ptr, _ = colouring(numCU, L)
        want = gr.sweep(Sp, Sj, Ax, diag, ptr, order, b, x0, OMEGA, 1, gr.SYMMETRIC)
        assert np.array_equal(want * 1024.0, np.round(want * 1024.0)) and np.all(np.abs(want) * 1024.0 < 2.0 ** 24)
        assert not np.array_equal(want, x0)
        return Ax, diag, b, x0, want
    return cached(("gp sweep", n, L), make, "sweep")


def solve_case(numCU, L):
    """(Ax, x*, b of the lower solve, b of the upper solve with a unit diagonal) for alpha = 1/2, chosen as
    scantiles.solve_case chooses them: off-diagonal entries integers in [-3, 3], diagonals 1/2, 1, 2 or 4, x* integers in
    [-8, 8], b = 2 T x* -- iluref.trsv returns x* (asserted here), and so must the device, bit for bit in both builds"""
    n, Sp, Sj = band(numCU, L)

    def make():
        rng = np.random.default_rng(2000 + L)
        r = np.repeat(np.arange(n), np.diff(Sp))
        Ax = rng.integers(-3, 4, len(Sj)).astype(np.float64)
        Ax[r == Sj] = rng.choice([0.5, 1.0, 2.0, 4.0], n)
        xs = rng.integers(-8, 9, n).astype(np.float64)
        A = sp.csr_matrix((Ax, Sj, Sp), shape=(n, n))
        bl, bu = 2.0 * (sp.tril(A) @ xs), 2.0 * (sp.triu(A, 1) @ xs + xs)
        for upper, b in ((False, bl), (True, bu)):
            _, _, order, ptr = levels(numCU, L, upper)
            got = ir.trsv(n, Sp, Sj, Ax, ptr, order, b, np.zeros(n), 0.5, upper, unit_diag=upper)
            assert np.array_equal(got, xs)
        return Ax, xs, bl, bu
    return cached(("gp solve", n, L), make, "solve")


# ---------------------------------------------------------------- B: the long rows
def long_lens(numCU):
    """the row lengths: 8 numCU + 37 long rows of 1025 .. 1100 entries, about every 200th of them 4100 .. 4200 (beyond the
    keys a workgroup sorts in LDS), and 300 short and wave-bin rows (0 .. 1024 entries) scattered among them"""
    nq = CAP_B * numCU + EXTRA
    rng = np.random.default_rng(70 + numCU)
    lens = rng.integers(LONG + 1, 1101, nq)
    step = min(200, (nq - 97) // 5)                                   # (at least five of them on a small device)
    lens[97::step] = rng.integers(LDS_KEYS + 4, 4201, len(lens[97::step]))
    few = np.r_[rng.integers(0, 33, 200), rng.integers(33, LONG + 1, 96), [0, 1, 32, LONG]]
    at = np.sort(rng.choice(nq, len(few), replace=False))
    return np.insert(lens, at, few)


def long_rows(numCU):
    """(m, n, (Ap, Aj, Ax)): rows of long_lens in random column order with a duplicate pair side by side and one at the two
    ends of every row that has room, values integers in [-4, 4] (what test_spmv_gpu.rows_matrix builds)"""
    def make():
        rng = np.random.default_rng(71 + numCU)
        lens = long_lens(numCU)
        m = len(lens)
        Ap = np.zeros(m + 1, np.int32)
        np.cumsum(lens, out=Ap[1:])
        Aj = np.argsort(rng.random((m, N_COLS)), axis=1)              # a row's columns: the head of a permutation
        Aj = Aj[np.arange(N_COLS)[None, :] < lens[:, None]].astype(np.int32)
        a, ln = Ap[:-1][lens >= 16].astype(np.int64), lens[lens >= 16]
        Aj[a + 5] = Aj[a + 4]
        Aj[a + ln - 1] = Aj[a]
        return m, N_COLS, (Ap, Aj, rng.integers(-4, 5, Ap[-1]).astype(np.float64))
    return cached(("gp long", numCU), make)


def long_transposed(numCU):
    """(n, m, (Tp, Tj, Tx)): the long-row matrix transposed by scipy (rows ascending, the duplicates kept): the transpose's
    input, so that ITS transpose has the long rows"""
    def make():
        m, n, (Ap, Aj, Ax) = long_rows(numCU)
        r = np.repeat(np.arange(m), np.diff(Ap))
        o = np.lexsort((r, Aj))                                       # by column, then row; a duplicate pair stays a pair
        Tp = np.zeros(n + 1, np.int32)
        np.cumsum(np.bincount(Aj, minlength=n), out=Tp[1:])
        T = sp.csr_matrix((Ax[o], r[o], Tp), shape=(n, m))
        assert (abs(T - sp.csr_matrix((Ax, Aj, Ap), shape=(m, n)).T)).nnz == 0
        return n, m, (Tp, r[o].astype(np.int32), Ax[o])
    return cached(("gp long T", numCU), make)


def long_vectors(numCU):
    """(x, X of three columns, y, left, right): integers in [-9, 9]; the scaling vectors in [1, 4]"""
    def make():
        m, n, _ = long_rows(numCU)
        rng = np.random.default_rng(72 + numCU)
        return (rng.integers(-9, 10, (n, 1)).astype(np.float64), rng.integers(-9, 10, (n, 3)).astype(np.float64),
                rng.integers(-9, 10, (m, 1)).astype(np.float64), rng.integers(1, 5, m).astype(np.float64),
                rng.integers(1, 5, n).astype(np.float64))
    return cached(("gp long vectors", numCU), make)


def long_bound(numCU):
    """the greatest sum of magnitudes any of the references below adds up exactly: it must stay below 2^24"""
    m, n, (Ap, Aj, Ax) = long_rows(numCU)
    x, X, y, left, right = long_vectors(numCU)
    absA = sp.csr_matrix((np.abs(Ax), Aj, Ap), shape=(m, n))
    return float(max((2.0 * (absA @ np.abs(X)) + 9.0).max(), (2.0 * (absA @ np.abs(x)) + np.abs(y)).max(), np.abs(Ax).max() * 16.0))


def long_references(numCU):
    """{name: the reference}: 2 A x - y, 2 A X, min_plus and plus_times A x, the row sums and the rows' greatest
    magnitudes, Dl A Dr"""
    m, n, (Ap, Aj, Ax) = long_rows(numCU)
    x, X, y, left, right = long_vectors(numCU)

    def make():
        return {"spmv": spmvref.spmm(m, n, Ap, Aj, Ax, x, 2.0, -1.0, y)[0],
                "spmm": spmvref.spmm(m, n, Ap, Aj, Ax, X, 2.0)[0],
                "min_plus": spmvsrref.spmm_semiring("min_plus", m, n, Ap, Aj, Ax, x, y, None, True),
                "plus_times": spmvsrref.spmm_semiring("plus_times", m, n, Ap, Aj, Ax, x),
                "plus": rr.reduce(m, n, Ap, Aj, Ax, rr.ROWS, rr.PLUS)[0],
                "abs_max": rr.reduce(m, n, Ap, Aj, Ax, rr.ROWS, rr.ABS_MAX)[0],
                "scale": rr.scale(m, n, Ap, Aj, Ax, 1.0, left, right, 0)}
    return cached(("gp long references", numCU), make, "long rows")


def long_transpose(numCU):
    n, m, (Tp, Tj, Tx) = long_transposed(numCU)
    return cached(("gp long transpose", numCU), lambda: tr.transpose(n, m, Tp, Tj, Tx), "long rows")


def long_extract_lists(numCU):
    """(rows, cols): every row once in a random order and a permutation of the columns: every Z row is reordered and keeps
    all its entries, so the rows beyond LDS_KEYS stay beyond them"""
    m, n, _ = long_rows(numCU)
    rng = np.random.default_rng(73 + numCU)
    return rng.permutation(m).astype(np.int32), rng.permutation(n).astype(np.int32)


def long_extract(numCU):
    m, n, (Ap, Aj, Ax) = long_rows(numCU)
    rows, cols = long_extract_lists(numCU)
    return cached(("gp long extract", numCU), lambda: ex.extract(m, n, Ap, Aj, Ax, rows, cols), "long rows")


# two selections: the entries off the diagonal whose magnitude exceeds 1/2 (eight ninths of a row), and a row's 700 greatest
SELECT_SPECS = {"most": sr.Spec(flags=sr.ABS | sr.DROP_DIAG, abs_tol=0.5), "topk": sr.Spec(flags=sr.TOPK, top_k=700)}


def select_vectorised(m, n, Xp, Xj, Xx, spec):
    """selectref.select for the two specs above, all rows at once: (Zp, Zj, Zx)"""
    Xp = np.asarray(Xp, np.int64)
    row = np.repeat(np.arange(m, dtype=np.int64), np.diff(Xp))
    mag = np.abs(np.asarray(Xx, np.float64))
    assert spec.flags in (sr.ABS | sr.DROP_DIAG, sr.TOPK)
    if spec.flags & sr.ABS:
        keep = ~(mag <= spec.abs_tol) & (np.asarray(Xj, np.int64) != row)
    else:                                                             # by (row, magnitude descending, position): a row's first top_k
        order = np.lexsort((np.arange(len(Xj)), -mag, row))
        rank = np.empty(len(Xj), np.int64)
        rank[order] = np.arange(len(Xj)) - np.repeat(Xp[:-1], np.diff(Xp))
        keep = rank < spec.top_k
    Zp = np.zeros(m + 1, np.int32)
    np.cumsum(np.bincount(row[keep], minlength=m), out=Zp[1:])
    return Zp, np.asarray(Xj, np.int32)[keep], np.asarray(Xx)[keep]


def long_select(numCU, which, dtype=np.float64):
    m, n, (Ap, Aj, Ax) = long_rows(numCU)
    return cached(("gp long select", numCU, which, np.dtype(dtype).name),
                  lambda: select_vectorised(m, n, Ap, Aj, np.ascontiguousarray(Ax, dtype), SELECT_SPECS[which]), "long rows")


# ---------------------------------------------------------------- B: the sampled dense-dense product on the long rows
def sddmm_dense(numCU, k):
    """(X, Y): m x k and N_COLS x k, integers in [-4, 4], drawn per k"""
    def make():
        m, n, _ = long_rows(numCU)
        rng = np.random.default_rng(7500 + 100 * k + numCU)
        return rng.integers(-4, 5, (m, k)).astype(np.float64), rng.integers(-4, 5, (n, k)).astype(np.float64)
    return cached(("gp sddmm dense", numCU, k), make)


def sddmm_sliced(m, n, M, X, Y, alpha=1.0, beta=0.0, times_m=False, rows=SDDMM_SLICE):
    """sddmmref.sddmm with Z = M's values (in place), `rows` rows of M at a time: its temporaries are entries x T doubles"""
    Mp, Mj, Mx = M
    out = [np.zeros(0)]
    for r0 in range(0, m, rows):
        r1 = min(m, r0 + rows)
        a, b = int(Mp[r0]), int(Mp[r1])
        out.append(sd.sddmm(r1 - r0, n, np.asarray(Mp[r0:r1 + 1], np.int64) - a, Mj[a:b], Mx[a:b], X[r0:r1], Y, alpha, beta, Mx[a:b],
                            times_m))
    return np.concatenate(out)


def sddmm_reference(numCU, k, in_place=False):
    """Z in float64 -- integers below 2^24 in magnitude (asserted), so both builds hold it, and the rule's bits are the
    same in both: X Y^T on M's pattern, or under in_place 2 (X Y^T) .* M - M"""
    m, n, M = long_rows(numCU)
    X, Y = sddmm_dense(numCU, k)

    def make():
        alpha, beta = SDDMM_IN_PLACE if in_place else (1.0, 0.0)
        Z = sddmm_sliced(m, n, M, X, Y, alpha, beta, in_place)
        assert np.array_equal(Z, np.round(Z)) and np.abs(Z).max() < 2.0 ** 24 and len(Z) == len(M[1])
        return Z
    return cached(("gp sddmm", numCU, k, in_place), make, "sddmm")


# ---------------------------------------------------------------- B: the relaxation on the long rows
def long_square(numCU, sparse_values):
    """(n, (Ap, Aj, Ax), diag): the long-row matrix made square by N_COLS - m empty rows behind its own, diag = 1, 2 or 4;
    sparse_values: all but four values a row are zero, the rest +-1 (what test_relax_gpu.square does), so that the row sums
    of several steps stay exact"""
    def make():
        m, n, (Ap, Aj, Ax) = long_rows(numCU)
        assert m <= n
        Sp = np.concatenate([Ap, np.full(n - m, Ap[-1], np.int32)])
        rng = np.random.default_rng(74 + numCU)
        diag = 2.0 ** rng.integers(0, 3, n)
        vals = Ax
        if sparse_values:
            rows = np.repeat(np.arange(m), np.diff(Ap))
            order = np.lexsort((rng.random(len(Aj)), rows))           # every row's entries in a random order
            rank = np.arange(len(Aj)) - np.repeat(Ap[:-1].astype(np.int64), np.diff(Ap))
            keep = np.zeros(len(Aj), bool)
            keep[order[rank < 4]] = True
            vals = np.where(keep, np.sign(Ax) + (Ax == 0), 0.0)
        return n, (Sp, Aj, vals), diag
    return cached(("gp long square", numCU, sparse_values), make)


def relax_vectors(numCU):
    """(b, x, d): integers in [-3, 3], as test_relax_gpu.vectors draws them"""
    def make():
        rng = np.random.default_rng(75 + numCU)
        return tuple(rng.integers(-3, 4, N_COLS).astype(np.float64) for _ in range(3))
    return cached(("gp relax vectors", numCU), make)


def relax_reference(numCU, case):
    """(x, d) of RELAX_CASES[case] in float64 (d None where none is kept).  The restatement run in float32 gives the same
    numbers (asserted): no step's x or d rounds in either build, so the sums are exact in whatever order the device adds"""
    sparse, coef, with_d, zero = RELAX_CASES[case]
    n, (Ap, Aj, Ax), diag = long_square(numCU, sparse)
    b, x, d = relax_vectors(numCU)

    def make():
        both = [rx.relax(n, Ap, Aj, Ax, diag, coef, b, x, d if with_d else None, zero_guess=zero, dtype=t)[:2]
                for t in (np.float64, np.float32)]
        for wide, narrow in zip(*both):
            assert (wide is None and narrow is None) or np.array_equal(wide, narrow.astype(np.float64)), case
        assert not np.array_equal(both[0][0], x)
        return both[0]
    return cached(("gp relax", numCU, case), make, "relax")


# ---------------------------------------------------------------- B and C: the reductions beside a product
def exact_dots(z, w):
    """(z.z, w.z) in integer arithmetic; every sum of magnitudes stays below `2^53`: any order of additions is exact"""
    assert np.array_equal(z, np.round(z)) and np.array_equal(w, np.round(w))
    zi, wi = z.astype(np.int64), w.astype(np.int64)
    assert int((zi * zi).sum()) < 2 ** 53 and int(np.abs(wi * zi).sum()) < 2 ** 53
    return int((zi * zi).sum()), int((wi * zi).sum())


def long_dots(numCU):
    """(w, z.z, w.z) for z = long_references()["spmv"] = 2 A x - y: w integers in [-9, 9]"""
    def make():
        m, _, _ = long_rows(numCU)
        w = np.random.default_rng(76 + numCU).integers(-9, 10, m).astype(np.float64)
        return (w,) + exact_dots(long_references(numCU)["spmv"][:, 0], w)
    return cached(("gp long dots", numCU), make, "long rows")


def dots_case(m):
    """(A, x, y, w, z, z.z, w.z) for section C: A is m x m with one entry a row, its columns a permutation, its values in
    {-2, -1, 1, 2}; x, y and w integers in [-3, 3]; z = A x + y, so |z| <= 9 and both sums stay below 2^27; the last
    workgroup of k_dot_part has a share in both sums that is not zero"""
    def make():
        rng = np.random.default_rng(77)
        Aj = rng.permutation(m).astype(np.int32)
        Ax = rng.choice([-2.0, -1.0, 1.0, 2.0], m)
        x, y, w = (rng.integers(-3, 4, m).astype(np.float64) for _ in range(3))
        z = Ax * x[Aj] + y
        zz, wz = exact_dots(z, w)
        assert np.abs(z).max() <= 9 and zz < 2 ** 27 and int(np.abs(w * z).sum()) < 2 ** 27
        last = (-(-m // DOT_PER) - 1) * DOT_PER
        assert exact_dots(z[last:], w[last:])[0] != 0 and exact_dots(z[last:], w[last:])[1] != 0
        return (np.arange(m + 1, dtype=np.int32), Aj, Ax), x, y, w, z, zz, wz
    return cached(("gp dots", m), make, "dots")
