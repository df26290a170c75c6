"""The block loops of the capped grids, past their first turn, both builds, one handle per build.

Many kernels get a grid with a ceiling and let a workgroup loop over the blocks that are left
(`for (t = blockIdx.x; t < nBlocks; t += gridDim.x)`).  The families' own tests stay under the ceilings, so what a workgroup
does after its first turn -- the per-row state it sets up again, the LDS it reuses behind a trailing barrier, the counts it
adds once per workgroup, the reversed block order of the upper triangle -- is run here, at tests/gridpass.py's sizes, which
follow from the device's CU count (torch's multi_processor_count: the number bhs_create reads).

A. The graph and solver families (a row over L = 1, 4, 16 or 64 lanes, 256 / L rows a workgroup, the grid capped at 16
workgroups a CU): k_agg_decide, the colouring's round kernel, k_lev_pass for both triangles, k_cc_pass, k_mt_accept, and
k_sf_weight, k_sf_edge and k_sf_hook, each at every L through its family's own `run` and `check` -- everything a call
returns compared exactly with the numpy restatement (or, where tests/gridpass.py says so, the closed form on cliques),
sentinels included.  k_mt_accept and k_sf_hook take 256 vertices a workgroup whatever L: they pass the cap on the L = 1
input alone.  At L = 16 one Gauss-Seidel sweep runs on the colouring's device arrays and the two solves on the levels':
those kernels are not capped, but they consume orders made past the cap.  The aggregation at L = 1 and L = 4 is left to
tests/test_scan_tiles_gpu.py (a path of 1.57 M vertices, a band of 524 k: over the cap on devices of up to 384 and 512
CUs); every other combination is run here, L = 4 of the components, the matching and the forest too.

B. The long-row queues (one workgroup a row of more than 1024 entries, the grid capped at 8 workgroups a CU): spmv, spmm,
the semiring products, the row reductions, the scaling, the transpose, the extraction and the selection on one matrix with
8 numCU + 37 long rows, about every 200th of them beyond the 4096 keys a workgroup sorts in LDS; integer values, so every
result is compared exactly.  On the same matrix the kernels whose second turn carries state: k_sd_long<T> (it keeps `bad`
across rows) at the tiles T = 1, 2, 4, 16 and 64 and at k = 65, also in place with beta != 0, where a row done twice is wrong;
k_rx_long (sW behind a trailing barrier, ctl[RD_ERR] read once a workgroup) once per product pass of one and of four steps
on the matrix made square by empty rows, where a skipped row keeps the x of two steps before; and spmv_long as the fused
product launches it, on its own workspace's queues, with both reductions exact.

C. The partials of the fused reductions: k_dot_finish, one workgroup, adds them 256 a turn.  m = 257 x 4096 - 1000 gives 257
(whatever the CU count: k_dot_part's grid has no cap), the last from a partial workgroup, so thread 0 adds two; m = 4097
afterwards leaves 255 stale partials behind the two that count.

The references of these families took 3.7 s of CPU a session beside a 256-CU device (the sampled product 2.1 s, most of it
at k = 64 and 65; the relaxation 1.5 s for its five cases in both value types; section C's 0.02 s), on a slower CPU 9 s.

Before a call the test asserts that its block count exceeds the cap, after it that the kernel record books the rows n
implies, and prints both: it cannot pass without reaching the second turn."""
import numpy as np
import pytest
import torch

import forestref as fr
import gridpass as gp
import reduceref as rr
import scantiles as st
import sddmmref as sd
import test_aggregate_gpu as aggt
import test_components_gpu as cct
import test_extract_gpu as ext
import test_forest_gpu as ft
import test_gs_gpu as gst
import test_match_gpu as mt
import test_reduce_gpu as rdt
import test_relax_gpu as rxt
import test_scan_tiles_gpu as tiles
import test_sddmm_gpu as sdt
import test_select_gpu as selt
import test_spmv_dots_gpu as dt
import test_spmv_gpu as spmvt
import test_spmv_sr_gpu as srt
import test_transpose_gpu as trt
import test_trsv_gpu as trsvt

from benchmark_spgemm_using_csr_amd import _lib, amg
from benchmark_spgemm_using_csr_amd import dense as bhdense
from benchmark_spgemm_using_csr_amd import facade as bhmod

pytestmark = pytest.mark.gpu

BUILDS = {"f64": np.float64, "f32": np.float32}
LOWER, UPPER, UNIT = _lib.BHS_TRI_LOWER, _lib.BHS_TRI_UPPER, _lib.BHS_TRI_UNIT_DIAG
up, padded, exactly = tiles.up, tiles.padded, tiles.exactly


def num_cu():
    return torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count


@pytest.fixture(scope="module", params=sorted(BUILDS))
def hd(request):
    dtype = BUILDS[request.param]
    plats = [False] * bhmod.NUM_PLATFORMS
    plats[bhmod.BHSPARSE_HIP] = True
    bh = bhmod.bhsparse(value_dtype=dtype)
    assert bh.initPlatform(plats) == 0
    yield bh, dtype, request.param
    print("%s reference CPU seconds: %s" % (request.param, {k: round(v, 2) for k, v in sorted(gp.SECONDS.items())}))
    assert bh.free_mem() == 0
    bh.freePlatform()


def stats(bh):
    return {s["name"]: s for s in bh.kernel_stats() if s["launches"] > 0}


def over_the_cap(n, L, what, per=None):
    """before a call: the block loop of a kernel with 256 / L rows (or `per` vertices) a workgroup turns twice"""
    per = per or 256 // L
    nblocks, cap = -(-n // per), gp.CAP_A * num_cu()
    assert nblocks > cap and (nblocks - 1) % cap != 0, (what, n, nblocks, cap)
    return "%d blocks of %d over a grid of %d" % (nblocks, per, cap)


def reached(bh, build, what, L, reach, record, rows):
    """after a call: the record books exactly the rows n and the reference's rounds imply -- a count that a workgroup added
    once a turn instead of once would show here"""
    got = stats(bh)[record]
    assert got["rows"] == rows, (what, record, got["rows"], rows)
    print("%s %s L=%d: %s; %s booked %d rows in %d launches" % (build, what, L, reach, record, got["rows"], got["launches"]))


class Pattern(object):
    """a pattern on the device, as tests/test_scan_tiles_gpu.py's calls want it"""

    def __init__(self, n, Sp, Sj, nlabels):
        self.n, self.Sp, self.Sj, self.nnz = n, Sp, Sj, len(Sj)
        self.T = nlabels * st.words(n)                               # the order's table: labels x ceil(n / 64) counts
        self.dSp, self.dSj = up(Sp, np.int32), up(Sj, np.int32)


# ---------------------------------------------------------------- A: the graph and solver families
@pytest.mark.parametrize("L", (16, 64))
def test_aggregation(hd, L):
    bh, dtype, build = hd
    n, Sp, Sj = gp.band(num_cu(), L)
    want = gp.aggregation(num_cu(), L)
    reach = over_the_cap(n, L, "aggregation")
    aggt.check(aggt.run(bh, n, Sp, Sj, 0, what=("aggregation", L)), want, ("aggregation", L))
    rounds = want[3]
    assert rounds >= 2 and stats(bh)["agg_decide"]["launches"] == rounds and stats(bh)["agg_near"]["rows"] == n * rounds
    reached(bh, build, "aggregation", L, reach, "agg_decide", rows=gp.aggregation(num_cu(), L, rows=True))


def sweep_on(bh, P, dtype, coloring, case, what):
    """one symmetric sweep with omega = 1/2 on the colouring's device arrays, without and with BHS_GS_VERIFY"""
    color, ncolors, order, hptr = coloring
    Ax, diag, b, x0, want = case
    dAx, ddiag, db = up(Ax, dtype), up(diag, dtype), up(b, dtype)
    for flags, dcolor in ((_lib.BHS_GS_SYMMETRIC, None), (_lib.BHS_GS_SYMMETRIC | _lib.BHS_GS_VERIFY, color)):
        x = padded(x0, dtype)
        torch.cuda.synchronize()
        err = amg.gs_raw_device(bh, P.n, P.nnz, P.dSp, P.dSj, dAx, ddiag, ncolors, hptr, order, dcolor, db, x, gp.OMEGA, 1, flags)
        assert err == 0, (what, flags, err)
        assert bool((x[P.n:] == tiles.XSENT).all()), (what, "written past the end of d_x")
        exactly(x[:P.n], want, (what, flags))
        got = stats(bh)
        assert set(got) == gst.GS_FAMILIES and all(got[f]["launches"] == ncolors for f in got), (what, got)


@pytest.mark.parametrize("L", gp.LANES)
def test_colouring(hd, L):
    bh, dtype, build = hd
    n, Sp, Sj = gp.colour_pattern(num_cu(), L)
    want = gp.colouring(num_cu(), L)
    reach = over_the_cap(n, L, "colouring")
    gst.color_check(gst.color_run(bh, n, Sp, Sj, 0, what=("colouring", L)), want, ("colouring", L))
    rounds = want[4]
    assert rounds >= 3 and stats(bh)["color_round"]["launches"] == rounds
    reached(bh, build, "colouring", L, reach, "color_round", rows=gp.colouring(num_cu(), L, rows=True))
    if L != gp.SOLVE_AT:
        return
    P = Pattern(n, Sp, Sj, want[1])

    def call(color, order, ptr):
        bh.color_ncolors = bh.color_rounds = -1
        return amg.color_raw_device(bh, n, P.nnz, P.dSp, P.dSj, None, 0, 0, color, order, ptr), bh.color_ncolors
    color, ncolors, order, ptr = tiles.ordered_on_device(bh, P, call, "color_order", gst.COLOR_FAMILIES, "colouring kept on the device")
    gst.color_check((color[:n].cpu().numpy(), ncolors, order[:n].cpu().numpy(), ptr, bh.color_rounds), want, "colouring kept on the device")
    sweep_on(bh, P, dtype, (color, ncolors, order, ptr), gp.sweep_case(num_cu(), L), "sweep on the order made past the cap")


def solves_on(bh, P, dtype, lev, case, what):
    """the lower solve in place, the upper one with a unit diagonal into an array of its own, on the levels' device arrays"""
    Ax, xs, bl, bu = case
    dAx = up(Ax, dtype)
    for upper, b, flags in ((False, bl, LOWER), (True, bu, UPPER | UNIT)):
        nlevels, order, hptr = lev[upper]
        db = padded(b, dtype)
        dx = padded(np.full(P.n, 77.0), dtype) if upper else db
        torch.cuda.synchronize()
        err = amg.trsv_raw_device(bh, P.n, P.nnz, P.dSp, P.dSj, dAx, nlevels, hptr, order, 0.5, db, dx, flags)
        assert err == 0, (what, upper, err)
        assert bool((dx[P.n:] == tiles.XSENT).all()) and bool((db[P.n:] == tiles.XSENT).all()), (what, "written past the end")
        exactly(dx[:P.n], xs, (what, upper))
        if upper:
            exactly(db[:P.n], bu, (what, "d_b was written"))
        assert {k: v["launches"] for k, v in stats(bh).items()} == {"trsv_level": nlevels}, (what, stats(bh))


@pytest.mark.parametrize("L", gp.LANES)
def test_levels(hd, L):
    bh, dtype, build = hd
    n, Sp, Sj = gp.level_pattern(num_cu(), L)
    reach = over_the_cap(n, L, "levels")
    lev = {}
    for upper in (False, True):
        what = "upper levels" if upper else "lower levels"
        want = gp.levels(num_cu(), L, upper)
        assert want[1] >= 3
        got = trsvt.levels_run(bh, n, Sp, Sj, UPPER if upper else LOWER, what=(what, L))
        trsvt.levels_check(got, want, (what, L))
        assert got[4] >= 1 and stats(bh)["levels_pass"]["launches"] == got[4]
        reached(bh, build, what, L, reach, "levels_pass", rows=n * got[4])
        if L == gp.SOLVE_AT:
            P = Pattern(n, Sp, Sj, want[1])

            def call(level, order, ptr):
                bh.levels_nlevels = bh.levels_passes = -1
                err = amg.levels_raw_device(bh, n, P.nnz, P.dSp, P.dSj, UPPER if upper else LOWER, level, order, ptr)
                return err, bh.levels_nlevels
            level, nlevels, order, ptr = tiles.ordered_on_device(bh, P, call, "levels_order", trsvt.LEVEL_FAMILIES, what + " kept on the device")
            trsvt.levels_check((level[:n].cpu().numpy(), nlevels, order[:n].cpu().numpy(), ptr, bh.levels_passes), want, what)
            lev[upper] = (nlevels, order, ptr)
    if L == gp.SOLVE_AT:
        solves_on(bh, P, dtype, lev, gp.solve_case(num_cu(), L), "solves on the orders made past the cap")


@pytest.mark.parametrize("L", gp.LANES)
def test_components(hd, L):
    bh, dtype, build = hd
    n, Sp, Sj = gp.band(num_cu(), L)
    want = gp.components(num_cu(), L)
    assert want[3] >= 2
    reach = over_the_cap(n, L, "components")
    got = cct.run(bh, n, Sp, Sj, what=("components", L))
    cct.check(got, want, ("components", L))
    reached(bh, build, "components", L, reach, "components_pass", rows=n * got[4])
    assert stats(bh)["components_number"]["rows"] == n + st.words(n)


@pytest.mark.parametrize("L", gp.LANES)
def test_matching(hd, L):
    """k_mt_accept takes 256 vertices a workgroup whatever L: its loop turns twice on the L = 1 input, whose n alone exceeds
    256 x the cap; the other inputs run the proposals of their L on rounds whose count the accept kernel makes"""
    bh, dtype, build = hd
    n, Sp, Sj = gp.band(num_cu(), L)
    reach = over_the_cap(n, L, "matching")
    if L == 1:
        reach += "; k_mt_accept: " + over_the_cap(n, L, "matching: k_mt_accept", per=256)
    dev = (up(Sp, np.int32), up(Sj, np.int32))
    for maker in gp.match_makers(L):
        want = gp.matching(num_cu(), L, maker)
        assert want[4] >= 2
        what = ("matching", L, maker)
        got = mt.run(bh, dtype, n, Sp, Sj, what=what, dev=dev + (up(gp.weights(num_cu(), L, maker), dtype),))
        mt.check(got, want, what)
        assert mt.mr.is_matching(got[0])
        assert stats(bh)["match_init"]["rows"] == n and stats(bh)["match_number"]["rows"] == n + st.words(n)
        reached(bh, build, "matching %s" % maker, L, reach, "match_round", rows=gp.matching(num_cu(), L, maker, rows=True))


def forest_rows(n, hooks):
    """what forest_pick and forest_hook book: the roots every round started from, the closing round's too unless one tree is left"""
    roots = [n]
    for k in hooks:
        roots.append(roots[-1] - k)
    return sum(roots[:-1]) if hooks and roots[-1] == 1 else sum(roots)


@pytest.mark.parametrize("L", gp.LANES)
def test_forest(hd, L):
    """k_sf_weight and k_sf_edge take 256 / L rows a workgroup, k_sf_hook 256 vertices whatever L: its loop turns twice on the
    L = 1 input"""
    bh, dtype, build = hd
    n, Sp, Sj = gp.band(num_cu(), L)
    reach = over_the_cap(n, L, "forest")
    if L == 1:
        reach += "; k_sf_hook: " + over_the_cap(n, L, "forest: k_sf_hook", per=256)
    dAp, dAj = up(Sp, np.int32), up(Sj, np.int32)
    for maker, flags in gp.forest_cases(L):
        want = gp.forest(num_cu(), L, maker, flags)
        assert want[5] >= 3 and flags in (0, fr.MAXIMUM | fr.ABS)
        what = ("forest", L, maker, flags)
        got = ft.run(bh, dtype, n, Sp, Sj, flags=flags, what=what, dev=(dAp, dAj, up(gp.weights(num_cu(), L, maker), dtype)))
        ft.check(got, want, what, n, bh)
        rows = forest_rows(n, want[6]["hooks"])
        assert stats(bh)["forest_hook"]["rows"] == rows and stats(bh)["forest_list"]["rows"] == n + st.words(n) + got[4]
        reached(bh, build, "forest %s flags %d" % (maker, flags), L, reach, "forest_pick", rows=rows)


# ---------------------------------------------------------------- B: the long-row queues
def long_reached(bh, build, record):
    """after a call: the long queue held more rows than the grid has workgroups"""
    nq, cap = gp.sizes(num_cu())["long"], gp.CAP_B * num_cu()
    rows = stats(bh)[record]["rows"]
    assert rows == nq > cap, (record, rows, nq, cap)
    print("%s %s: %d rows over a grid of %d" % (build, record, rows, cap))


def test_long_rows_spmv_and_spmm(hd):
    bh, dtype, build = hd
    m, n, A = gp.long_rows(num_cu())
    x, X, y, _, _ = gp.long_vectors(num_cu())
    want = gp.long_references(num_cu())
    D = spmvt.Dev(m, n, A, dtype)
    exactly(spmvt.run(bh, D, x, 2.0, -1.0, y, what="long rows"), want["spmv"], "2 A x - y")
    long_reached(bh, build, "spmv_long")
    exactly(spmvt.run(bh, D, X, 2.0, gap=2, what="long rows"), want["spmm"], "2 A X, three columns in a leading dimension of five")
    long_reached(bh, build, "spmm_long")


def test_long_rows_semiring(hd):
    bh, dtype, build = hd
    m, n, A = gp.long_rows(num_cu())
    x, X, y, _, _ = gp.long_vectors(num_cu())
    want = gp.long_references(num_cu())
    D = srt.Dev(m, n, A, dtype)
    got = srt.run(bh, "min_plus", D, x, y, None, True, what="long rows")
    exactly(got[0], want["min_plus"][0], "y min= A min.+ x", bits=True)
    assert got[1] == want["min_plus"][1] > gp.CAP_B * num_cu(), (got[1], want["min_plus"][1])
    long_reached(bh, build, "srmv_long")
    got = srt.run(bh, "plus_times", D, x, what="long rows")
    exactly(got[0], want["plus_times"][0], "A +.x x")
    long_reached(bh, build, "srmv_long")


def test_long_rows_reduce_and_scale(hd):
    bh, dtype, build = hd
    m, n, A = gp.long_rows(num_cu())
    _, _, _, left, right = gp.long_vectors(num_cu())
    want = gp.long_references(num_cu())
    D = rdt.Dev(m, n, A, dtype)
    exactly(rdt.run_reduce(bh, D, rr.ROWS, rr.PLUS, what="long rows"), want["plus"], "row sums")
    long_reached(bh, build, "reduce_long")
    exactly(rdt.run_reduce(bh, D, rr.ROWS, rr.ABS_MAX, what="long rows"), want["abs_max"], "the rows' greatest magnitudes")
    long_reached(bh, build, "reduce_long")
    exactly(rdt.run_scale(bh, D, 1.0, left, right, 0, False, "long rows"), want["scale"], "Dl A Dr", bits=True)
    long_reached(bh, build, "scale_long")


def test_long_rows_transpose(hd):
    """the input is the long-row matrix transposed: ITS transpose has the long rows, those beyond the LDS keys among them"""
    bh, dtype, build = hd
    n, m, T = gp.long_transposed(num_cu())
    ref = trt.check_transpose(bh, n, m, T, dtype, what="long rows")
    assert np.array_equal(ref[0], gp.long_rows(num_cu())[2][0])       # T's row pointer is the long-row matrix's own
    long_reached(bh, build, "transpose_long")


def test_long_rows_extract(hd):
    """every row once in a random order under a permutation of the columns: every long row is reordered and keeps its
    entries, so those of more than 4096 sort in global memory between rows that sort in LDS"""
    bh, dtype, build = hd
    m, n, A = gp.long_rows(num_cu())
    rows, cols = gp.long_extract_lists(num_cu())
    Zp, Zj, Zx, perm, reordered = gp.long_extract(num_cu())
    assert reordered > gp.CAP_B * num_cu() and int((np.diff(Zp) > gp.LDS_KEYS).sum()) >= 5
    ext.check_extract(bh, m, n, A, rows, cols, dtype, what="long rows", ref=(Zp, Zj, np.ascontiguousarray(Zx, dtype), perm, reordered))
    long_reached(bh, build, "extract_long")


@pytest.mark.parametrize("which", sorted(gp.SELECT_SPECS))
def test_long_rows_select(hd, which):
    """"most": off the diagonal and above 1/2 in magnitude, eight ninths of every long row; "topk": a row's 700 greatest, ties
    to the front"""
    bh, dtype, build = hd
    m, n, A = gp.long_rows(num_cu())
    ref = gp.long_select(num_cu(), which, dtype)
    selt.check_select(bh, m, n, A, gp.SELECT_SPECS[which], dtype, what=("long rows", which), ref=ref)
    long_reached(bh, build, "select_long")


def test_long_rows_sddmm(hd):
    """k_sd_long<T> at T = 1, 2, 4, 16 and 64 and, at k = 65, with a second tile in a lane: X Y^T on the long-row pattern over
    a Z of NaN; at k = 3 and 65 also 2 (X Y^T) .* M - M in place on M's values, where a row done twice would end as M"""
    bh, dtype, build = hd
    m, n, M = gp.long_rows(num_cu())
    for k in gp.SDDMM_KS:
        X, Y = gp.sddmm_dense(num_cu(), k)
        cases = [(1.0, 0.0, False)] + ([gp.SDDMM_IN_PLACE + (True,)] if k in gp.SDDMM_IN_PLACE_KS else [])
        for alpha, beta, in_place in cases:
            want = np.ascontiguousarray(gp.sddmm_reference(num_cu(), k, in_place), dtype)
            got = sdt.run(bh, dtype, m, n, M, X, Y, alpha, beta, times_m=in_place, in_place=in_place, gap=gp.SDDMM_GAP)
            assert sd.same_bits(got, want), (k, in_place, np.argwhere(got != want)[:5])
            assert sdt.families(bh) == {"sddmm_short", "sddmm_wave", "sddmm_long"}
            print("k = %d%s:" % (k, " in place" if in_place else ""), end=" ")
            long_reached(bh, build, "sddmm_long")


@pytest.mark.parametrize("case", sorted(gp.RELAX_CASES))
def test_long_rows_relax(hd, case):
    """k_rx_long once per product pass on the square long-row pattern: one step on full integer values (the call ends in
    relax_finish), four steps on sparse values from the caller's x and from the zero guess over an x of NaN (the queues of
    k_rx_short<true> and of k_rx_zero, the ping-pong of the two scratch x and the caller's, d from scratch to the
    caller's), and four Jacobi steps without d.  A row that a pass skipped keeps an x that is two steps old."""
    bh, dtype, build = hd
    sparse, coef, with_d, zero = gp.RELAX_CASES[case]
    n, A, diag = gp.long_square(num_cu(), sparse)
    b, x, d = gp.relax_vectors(num_cu())
    wx, wd = gp.relax_reference(num_cu(), case)
    coef = np.array(coef)
    assert case != "four steps" or np.array_equal(coef, rxt.COEF)
    gx, gd = rxt.call(bh, dtype, n, A, diag, coef, b, x, d if with_d else None, zero=zero, nan_x=zero)
    exactly(gx, wx, (case, "x"))
    assert (gd is None) == (wd is None)
    if with_d:
        exactly(gd, wd, (case, "d"))
    passes = len(coef) - (1 if zero else 0)
    lens = np.diff(A[0])
    nq, nq_wave, cap = gp.sizes(num_cu())["long"], int(((lens > 32) & (lens <= gp.LONG)).sum()), gp.CAP_B * num_cu()
    got = stats(bh)
    assert got["relax_long"]["launches"] == passes == got["relax_wave"]["launches"], (case, got)
    assert got["relax_wave"]["rows"] == nq_wave * passes and got["relax_short"]["rows"] == n * passes, (case, got)
    assert got["relax_long"]["rows"] == nq * passes and nq > cap, (case, got["relax_long"], nq, passes, cap)
    print("%s relax %s: %d rows over a grid of %d in each of %d launches" % (build, case, nq, cap, passes))


def fused_records(bh, D, x, alpha, beta, y, w, z, dots, what):
    """tests/test_spmv_dots_gpu.py's call ends in the plain product, whose records replace the fused call's: the fused call
    once more, out of place -- the same bits in z and in both reductions --, and ITS records"""
    dx, dy, dw = up(x, D.dtype), up(y, D.dtype), up(w, D.dtype)
    dz = padded(np.full(D.m, np.nan), D.dtype)
    again = np.full(2, dt.UNTOUCHED)
    torch.cuda.synchronize()
    err = bhdense.csr_spmv_dots_raw_device(bh, D.m, D.n, D.nnz, D.d[2], D.d[0], D.d[1], alpha, dx, beta, dy, dz, dw, again)
    assert err == 0, (what, err)
    assert bool((dz[D.m:] == tiles.XSENT).all()), (what, "written past the end of z")
    assert np.array_equal(spmvt.bits(dz[:D.m].cpu().numpy()), spmvt.bits(z)) and np.array_equal(spmvt.bits(again), spmvt.bits(dots)), what
    return stats(bh)


def test_long_rows_spmv_dots(hd):
    """spmv_long as dots_run launches it, on the queues of its own workspace: z = 2 A x - y out of place and in place, with
    the bits of the plain product, and both reductions exact"""
    bh, dtype, build = hd
    m, n, A = gp.long_rows(num_cu())
    x, _, y, _, _ = gp.long_vectors(num_cu())
    w, zz, wz = gp.long_dots(num_cu())
    want = gp.long_references(num_cu())["spmv"][:, 0]
    D = spmvt.Dev(m, n, A, dtype)
    for in_place in (False, True):
        z, dots, plain = dt.call(bh, D, x[:, 0], 2.0, -1.0, y[:, 0], w, in_place)
        assert np.array_equal(spmvt.bits(z), spmvt.bits(plain)), in_place
        exactly(z, want, ("2 A x - y beside its reductions", in_place))
        assert dots[0] == zz and dots[1] == wz, (in_place, dots, zz, wz)
        long_reached(bh, build, "spmv_long")                          # (the plain product's)
    got = fused_records(bh, D, x[:, 0], 2.0, -1.0, y[:, 0], w, z, dots, "long rows")
    assert got["dots_part"]["rows"] == m and got["dots_finish"]["rows"] == -(-m // gp.DOT_PER)
    long_reached(bh, build, "spmv_long")                              # (the fused call's)


# ---------------------------------------------------------------- C: the partials of the fused reductions
def test_dots_finish_second_turn(hd):
    """k_dot_finish adds 257 partials, thread 0 those of workgroups 0 and 256, the last from a partial workgroup whose share
    in both sums is not zero; then two partials on the same handle, with the 255 stale ones behind them"""
    bh, dtype, build = hd
    for m, nparts in ((gp.DOTS_M, gp.DOT_TURN + 1), (gp.DOTS_M_AFTER, 2)):
        A, x, y, w, want, zz, wz = gp.dots_case(m)
        assert -(-m // gp.DOT_PER) == nparts and m % gp.DOT_PER != 0
        D = spmvt.Dev(m, m, A, dtype)
        z, dots, plain = dt.call(bh, D, x, 1.0, 1.0, y, w)
        assert np.array_equal(spmvt.bits(z), spmvt.bits(plain)), m
        exactly(z, want, ("A x + y", m))
        assert dots[0] == zz and dots[1] == wz, (m, dots, zz, wz)
        got = fused_records(bh, D, x, 1.0, 1.0, y, w, z, dots, ("dots", m))
        assert got["dots_finish"]["rows"] == nparts and got["dots_part"]["rows"] == m, (m, got["dots_finish"], got["dots_part"])
        print("%s dots_finish: %d partials over %d threads" % (build, got["dots_finish"]["rows"], gp.DOT_TURN))
