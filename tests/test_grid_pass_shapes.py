"""The shapes of tests/test_grid_pass_gpu.py, from the references alone (no GPU), for devices of 256, 64 and 304 CUs: every
graph input gets the lanes a row it is listed under and a block count between 1.25 and 2 times the cap of 16 workgroups a CU
with a partial last block, has several components, and its references take several rounds and levels -- so that what a
second turn of a block loop computes depends on the turn before; the long-row matrix has more long rows than 8 workgroups a
CU, rows beyond the keys a workgroup sorts in LDS among them, and sums that both value types hold exactly -- those of the
relaxation's steps on its square pattern, of the sampled dense-dense product (whose sliced restatement is the unsliced one)
and of the fused product's reductions too; the input of k_dot_finish's second turn has 257 partials, the last from a partial
workgroup.  The closed forms that stand in for a slow restatement are compared with it at a small size."""
import numpy as np
import pytest

import forestref as fr
import gridpass as gp
import gsref as gr
import iluref as ir
import scantiles as st
import sddmmref as sd
import selectref as sr

CUS = (256, 64, 304)


def test_the_thresholds_are_the_host_codes():
    """a workgroup holds 256 / L rows and the grid is capped at 16 numCU: on 256 CUs the loop turns twice above these n"""
    assert [16 * 256 * (256 // L) for L in gp.LANES] == [1048576, 262144, 65536, 16384]
    assert gp.sizes(256) == {1: (1363071, (3, 454357)), 4: (340767, (5, 68154)), 16: (85191, (33, 2582)), 64: (21297, (65, 329)),
                             "long": 2085}
    for numCU in CUS:
        for L in gp.LANES:
            n, (q, c) = gp.sizes(numCU)[L]
            for size in (n, q * c):
                assert 1.25 * gp.CAP_A * numCU < gp.blocks(size, L) <= 2 * gp.CAP_A * numCU, (numCU, L, size)
                assert size % (256 // L) != 0, (numCU, L, size)
                assert (gp.blocks(size, L) - 1) % (gp.CAP_A * numCU) != 0  # (the partial block is a second turn's, not a first's)
        assert gp.sizes(numCU)["long"] > gp.CAP_B * numCU


@pytest.mark.parametrize("numCU", CUS)
def test_graph_inputs(numCU):
    for L in gp.LANES:
        patterns = {"band": gp.band(numCU, L), "colouring": gp.colour_pattern(numCU, L), "levels": gp.level_pattern(numCU, L)}
        for what, (n, Sp, Sj) in patterns.items():
            assert len(Sp) == n + 1 and Sp[-1] == len(Sj) and 0 <= Sj.min() and Sj.max() < n, (numCU, L, what)
            assert ir.lanes_per_row(n, len(Sj)) == L, (numCU, L, what, len(Sj) / n)
            assert 1.25 * gp.CAP_A * numCU < gp.blocks(n, L) <= 2 * gp.CAP_A * numCU and n % (256 // L) != 0, (numCU, L, what)
        n, Sp, Sj = patterns["band"]
        rows = np.repeat(np.arange(n), np.diff(Sp))
        assert np.diff(Sp).max() == 2 * gp.HALF_WIDTH[L] + 1 and int((Sj == rows).sum()) == n      # the diagonal is kept
        assert np.all(np.diff(Sj.astype(np.int64))[rows[1:] == rows[:-1]] > 0)                     # rows strictly ascending
        assert np.mean(np.abs(Sj - rows)) > 0.2 * n                                                # no index locality
        assert gp.components(numCU, L)[3] == gp.PARTS >= 2, (numCU, L)
        for maker in gp.match_makers(L):
            want, booked = gp.matching(numCU, L, maker), gp.matching(numCU, L, maker, rows=True)
            assert want[4] >= 2 and n < booked <= n * (want[4] + 2), (numCU, L, maker, want[4], booked)  # (a closing round, the finish)
        for maker, flags in gp.forest_cases(L):
            want = gp.forest(numCU, L, maker, flags)
            assert want[5] >= 3 and len(want[6]["hooks"]) == want[5], (numCU, L, maker, flags, want[5])
        for upper in (False, True):
            level, nlevels, order, ptr = gp.levels(numCU, L, upper)
            assert nlevels >= 3 and len(level) == patterns["levels"][0] and ptr[-1] == len(order), (numCU, L, upper, nlevels)
    assert {m for L in gp.LANES for m in gp.match_makers(L)} == {"ties", "asymmetric", "specials"}
    assert {m for L in gp.LANES for m, _ in gp.forest_cases(L)} == {"ties", "asymmetric", "specials"}
    assert all({f for m, f in gp.forest_cases(L)} <= {0, fr.MAXIMUM | fr.ABS} for L in gp.LANES)
    assert {f for L in gp.LANES for m, f in gp.forest_cases(L)} == {0, fr.MAXIMUM | fr.ABS}
    print("%d CUs, reference CPU seconds: %s" % (numCU, {k: round(v, 2) for k, v in sorted(gp.SECONDS.items())}))


@pytest.mark.parametrize("numCU", CUS)
def test_long_rows(numCU):
    m, n, (Ap, Aj, Ax) = gp.long_rows(numCU)
    lens = np.diff(Ap)
    nq = gp.sizes(numCU)["long"]
    assert int((lens > gp.LONG).sum()) == nq > gp.CAP_B * numCU
    assert int((lens > gp.LDS_KEYS).sum()) >= 5 and lens.max() < n
    assert int(((lens > 32) & (lens <= gp.LONG)).sum()) >= 90 and int((lens <= 32).sum()) >= 190 and (lens == 0).any()
    # a row beyond the LDS keys lies between two that sort in LDS in one workgroup's turns: it is neither first nor last
    beyond = np.flatnonzero(lens[lens > gp.LONG] > gp.LDS_KEYS)
    assert beyond[0] >= 1 and beyond[-1] < nq - 1 and np.any(beyond >= gp.CAP_B * numCU - 200)
    assert np.array_equal(Ax, np.round(Ax)) and np.abs(Ax).max() <= 4 and gp.long_bound(numCU) < 2.0 ** 24
    rows = np.repeat(np.arange(m), lens)
    key = rows * n + Aj
    assert len(np.unique(key)) < len(key) and np.any(np.diff(Aj)[np.diff(rows) == 0] < 0)   # duplicate pairs; no order in a row
    # the transposed input's transpose is the matrix with every row sorted
    tn, tm, (Tp, Tj, Tx) = gp.long_transposed(numCU)
    assert (tn, tm) == (n, m) and np.diff(Tp).max() <= gp.LONG
    back = gp.long_transpose(numCU)
    assert np.array_equal(back[0], Ap) and int((np.diff(back[0]) > gp.LONG).sum()) == nq
    # the extraction keeps every entry and reorders every row; in the order of Z's rows (the order its long queue is filled
    # in, 256 rows of Z at a time) a row beyond the LDS keys lies between two long rows that sort in LDS
    rows_list, cols = gp.long_extract_lists(numCU)
    assert np.array_equal(np.sort(rows_list), np.arange(m)) and np.array_equal(np.sort(cols), np.arange(n))
    Zp, _, _, _, reordered = gp.long_extract(numCU)
    zlens = np.diff(Zp)
    assert np.array_equal(zlens, lens[rows_list]) and reordered >= nq
    zlong = zlens[zlens > gp.LONG]
    zbeyond = np.flatnonzero(zlong > gp.LDS_KEYS)
    assert len(zbeyond) >= 5 and zbeyond[0] >= 1 and zbeyond[-1] < nq - 1 and np.all(np.diff(zbeyond) > 1), (numCU, zbeyond)
    # the vectorised selection is the restatement's on the first 40 rows, long ones among them
    assert int((lens[:40] > gp.LONG).sum()) >= 20
    for which, spec in gp.SELECT_SPECS.items():
        got = gp.long_select(numCU, which)
        want = sr.select(40, n, Ap[:41], Aj[:Ap[40]], Ax[:Ap[40]], spec)
        assert np.array_equal(got[0][:41], want[0]), which
        assert np.array_equal(got[1][:want[0][-1]], want[1]) and np.array_equal(got[2][:want[0][-1]], want[2]), which
        kept = np.diff(got[0])[lens > gp.LONG]
        assert np.all(kept > 0.8 * lens[lens > gp.LONG]) if which == "most" else np.all(kept == spec.top_k), which


def test_the_thresholds_of_the_relaxation_the_sampled_product_and_the_fused_dots():
    """k_rx_long and k_sd_long get min(nq, 8 numCU) workgroups (rx_run, sd_run), as spmv_long does in dots_run; k_dot_part
    makes a partial per 4096 elements and k_dot_finish's 256 threads add them 256 a turn: a second turn needs m > 1 048 576"""
    assert (gp.CAP_B, gp.DOT_PER, gp.DOT_TURN, gp.DOT_TURN * gp.DOT_PER) == (8, 4096, 256, 1048576)
    assert gp.DOTS_M == 1051672 and -(-gp.DOTS_M // gp.DOT_PER) == 257 == gp.DOT_TURN + 1 and gp.DOTS_M % gp.DOT_PER != 0
    assert -(-gp.DOTS_M_AFTER // gp.DOT_PER) == 2
    assert sorted({sd.tile(k) for k in gp.SDDMM_KS}) == [1, 2, 4, 16, 64] and max(gp.SDDMM_KS) > 64
    assert set(gp.SDDMM_IN_PLACE_KS) <= set(gp.SDDMM_KS) and gp.SDDMM_IN_PLACE[1] != 0.0
    for numCU in CUS:
        assert gp.sizes(numCU)["long"] > gp.CAP_B * numCU


@pytest.mark.parametrize("numCU", CUS)
def test_long_rows_relaxation(numCU):
    """the square pattern keeps every long row; no step of any case rounds in float32, x and d alike"""
    m, _, (Ap, Aj, Ax) = gp.long_rows(numCU)
    b, x, d = gp.relax_vectors(numCU)
    for sparse in (False, True):
        n, (Sp, Sj, Sx), diag = gp.long_square(numCU, sparse)
        lens = np.diff(Sp)
        assert n == gp.N_COLS == len(lens) == len(diag) and Sp[-1] == len(Sj) == len(Sx) and Sj is Aj
        assert np.array_equal(lens[:m], np.diff(Ap)) and not lens[m:].any() and n > m
        assert int((lens > gp.LONG).sum()) == gp.sizes(numCU)["long"] > gp.CAP_B * numCU
        assert set(np.unique(diag).tolist()) == {1.0, 2.0, 4.0}
        if sparse:
            rows = np.repeat(np.arange(n), lens)
            assert np.array_equal(np.bincount(rows[Sx != 0], minlength=n), np.minimum(lens, 4)) and set(np.unique(Sx).tolist()) == {-1.0, 0.0, 1.0}
        else:
            assert Sx is Ax
    for case, (sparse, coef, with_d, zero) in gp.RELAX_CASES.items():
        gx, gd = gp.relax_reference(numCU, case)
        assert (gd is not None) == with_d and len(coef) in (1, 4) and sparse == (len(coef) > 1)
        for v in (gx,) + ((gd,) if with_d else ()):
            assert v.dtype == np.float64 and np.isfinite(v).all() and np.array_equal(v, v.astype(np.float32).astype(np.float64)), (numCU, case)
        assert not np.array_equal(gx[m:], x[m:])                     # an empty row's x moves by c b / diag
    assert np.array_equal(np.array(gp.RELAX_CASES["four steps"][1]), np.array(gp.RELAX_COEF))
    print("%d CUs: max |x| %.1f after the full step, %.1f after the four sparse ones" % (
        numCU, np.abs(gp.relax_reference(numCU, "one step")[0]).max(), np.abs(gp.relax_reference(numCU, "four steps")[0]).max()))


@pytest.mark.parametrize("numCU", CUS)
def test_long_rows_sampled_product_and_reductions(numCU):
    m, n, (Ap, Aj, Ax) = gp.long_rows(numCU)
    k, rows = 65, 40
    X, Y = gp.sddmm_dense(numCU, k)
    assert X.shape == (m, k) and Y.shape == (n, k) and np.abs(np.r_[X.ravel(), Y.ravel()]).max() == 4
    alpha, beta = gp.SDDMM_IN_PLACE
    head = (Ap[:rows + 1], Aj[:Ap[rows]], Ax[:Ap[rows]])
    assert int((np.diff(head[0]) > gp.LONG).sum()) >= 20
    sliced = gp.sddmm_sliced(rows, n, head, X[:rows], Y, alpha, beta, True, rows=16)      # 16 + 16 + 8 rows
    whole = sd.sddmm(rows, n, head[0], head[1], head[2], X[:rows], Y, alpha, beta, head[2], True)
    assert sd.same_bits(sliced, whole) and np.abs(whole).max() < 2.0 ** 24 and np.array_equal(whole, np.round(whole))
    r = np.repeat(np.arange(rows), np.diff(head[0]))
    s = np.einsum("ij,ij->i", X[r], Y[head[1]])
    assert np.array_equal(whole, 2.0 * s * head[2] - head[2]) and np.mean(whole != head[2]) > 0.5   # (a row done twice: m instead)
    assert k * 16 * 4 * 2 + 4 < 2 ** 24                              # the bound of any entry at any of the widths
    # the reductions of the fused product: z = 2 A x - y on the long rows, and section C's
    w, zz, wz = gp.long_dots(numCU)
    z = gp.long_references(numCU)["spmv"][:, 0]
    assert len(w) == m == len(z) and np.abs(w).max() == 9 and np.abs(z).max() < 2 ** 19
    assert 0 < zz < 2 ** 53 and abs(wz) < 2 ** 53 and zz == int((z * z).sum()) and wz == int((w * z).sum())
    if numCU == CUS[0]:                                              # (it does not depend on the CU count)
        for mm in (gp.DOTS_M, gp.DOTS_M_AFTER):
            A, x, y, w, z, zz, wz = gp.dots_case(mm)
            assert len(z) == mm and np.array_equal(np.sort(A[1]), np.arange(mm)) and np.abs(z).max() <= 9 and 0 < zz < 2 ** 27
            assert wz == int((w * z).sum()) and zz == int((z * z).sum())
    print("%d CUs, reference CPU seconds: %s" % (numCU, {k_: round(v, 2) for k_, v in sorted(gp.SECONDS.items())}))


def test_closed_forms_are_the_restatements():
    """at q = 3 and 5 (the cliques of L = 1 and 4) with 40 cliques, seed 0"""
    for q in (gp.CLIQUE_Q[1], gp.CLIQUE_Q[4]):
        n, Sp, Sj, _, _ = st.cliques(q, 40)
        got, want = st.closed_form_colouring(q, 40, 0), gr.colouring(n, Sp, Sj, 0)
        assert got[1] == want[1] == q == got[4] == want[4]
        counts = []
        gr.colouring(n, Sp, Sj, 0, counts=counts)                    # a round colours one vertex a clique: what color_round books
        assert counts == [40 * k for k in range(q, 0, -1)] and sum(counts) == 40 * q * (q + 1) // 2
        assert all(a.dtype == b.dtype and np.array_equal(a, b) for a, b in zip((got[0], got[2], got[3]), (want[0], want[2], want[3])))
        for upper in (False, True):
            got, want = gp.closed_form_levels(q, 40, upper), ir.levels(n, Sp, Sj, upper)
            assert got[1] == want[1] == q
            assert all(a.dtype == b.dtype and np.array_equal(a, b) for a, b in zip((got[0], got[2], got[3]), (want[0], want[2], want[3])))


def test_values_of_the_sweep_and_the_solve_are_exact():
    """the builders assert it as they go (on the smallest device: the restatements are Python loops over the rows)"""
    numCU, L = 64, gp.SOLVE_AT
    assert L not in gp.COLOUR_ON_CLIQUES and L not in gp.LEVELS_ON_CLIQUES      # the orders are the band's
    Ax, diag, b, x0, want = gp.sweep_case(numCU, L)
    assert np.array_equal(want, want.astype(np.float32).astype(np.float64))
    Ax, xs, bl, bu = gp.solve_case(numCU, L)
    assert np.array_equal(bl, np.round(bl)) and np.array_equal(bu, np.round(bu)) and np.abs(np.r_[bl, bu]).max() < 2.0 ** 24
