"""The graph and solver families on one long-lived handle, across the tile boundary of their scans.

The push product, the MIS(2) aggregation, the colouring with its Gauss-Seidel sweep and the level sets with the triangular
solve and ILU(0) each keep a workspace on the handle (csrc/bhs_host_side.inc.h) and build an order or a list with the
library's one-pass scan over 8192-count tiles: the push product twice a call (the frontier's degrees, then the row map's
words, on one set of tile words and one epoch), the aggregation over ceil(n / 64) words, the colouring and the levels over a
label-major table of labels x ceil(n / 64) counts whose offsets go to one shared buffer.  Their own tests stay inside one
tile.  Here one handle per build is taken through tests/scantiles.py's sizes -- every scanned count above a tile, empty, 1,
exactly a tile, several tiles and a remainder, just under a tile, in that order -- and at every size all the families run
one after another, with the CSR x dense products between them, before the next size; a seventh step regrows the colouring's
and the levels' tables past a tile on an n that is no multiple of 64.  The colouring and the levels
alternate, so that the shared offsets pass from one to the other; the sweep and the solves read the device arrays the
colouring and the levels have just written.  Everything is compared exactly with the numpy restatements of tests/: integer
outputs as arrays, values on small integers and dyadic numbers bit for bit.  Sentinels behind every output are checked as
the families' own tests check them (their helpers are used where they fit).

After each call the scan's work is read from kernel_stats(): the record color_order / levels_order books n + T rows,
agg_scan n + ceil(n / 64), push_scan nf + ceil(n / 64) (nf alone where no list is asked for) -- the test cannot pass without
reaching the tiles it names.

Between the exact size and the next a refused call on device arrays of the colouring (a column out of range, met by its
round kernel), of the levels (the same, met by their pass) and of the push product (a frontier index out of range) must
return BHS_ERR_INVALID_ARG, leave what the families' refusal tests say it leaves, and the next call must be exact."""
import numpy as np
import pytest
import torch

import scantiles as st
import semiringref as srf
import test_aggregate_gpu as aggt
import test_gs_gpu as gst
import test_push_sr_gpu as pusht
import test_spmv_gpu as spmvt
import test_spmv_sr_gpu as srt
import test_trsv_gpu as trsvt

from benchmark_spgemm_using_csr_amd import _lib, amg
from benchmark_spgemm_using_csr_amd import facade as bhmod

pytestmark = pytest.mark.gpu

BUILDS = {"f64": np.float64, "f32": np.float32}
INV = _lib.BHS_ERR_INVALID_ARG
PAD, SENT, XSENT = 64, -7, -123.5
LOWER, UPPER, UNIT = _lib.BHS_TRI_LOWER, _lib.BHS_TRI_UPPER, _lib.BHS_TRI_UNIT_DIAG
REACHED = {}                                       # record -> the scanned counts read from kernel_stats(), in order


def up(a, dt):
    """A device copy (of an empty array: an empty tensor, which the calls take for an array without entries)."""
    a = np.ascontiguousarray(a, dt)
    t = torch.empty(max(a.size, 1), dtype=torch.from_numpy(np.zeros(1, dt)).dtype).cuda()
    t[:a.size].copy_(torch.from_numpy(a.copy()))
    return t[:a.size]


def padded(values, dtype):
    x = torch.full((len(values) + PAD,), XSENT, dtype=trsvt.tdt(dtype)).cuda()
    x[:len(values)] = up(values, dtype)
    return x


def stats(bh):
    return {s["name"]: s for s in bh.kernel_stats() if s["launches"] > 0}


def scanned(bh, record, other_rows, want, what):
    """the scan's count from the rows the record booked: exactly `want`"""
    rows = stats(bh)[record]["rows"] if record in stats(bh) else 0
    assert rows == other_rows + want, (what, record, rows, other_rows, want)
    REACHED.setdefault(record, []).append(rows - other_rows)


def exactly(got, want, what, bits=False):
    """equal as numbers in every element (the references hold no NaN); bits: the same bits, the sign of a zero included, as
    the semiring calls promise them"""
    got = got.cpu().numpy() if hasattr(got, "cpu") else np.asarray(got)
    assert got.shape == np.shape(want), (what, got.shape, np.shape(want))
    got, want = got.astype(np.float64), np.asarray(want, np.float64)
    assert np.array_equal(got, want), (what, np.argwhere(got != want)[:5])
    assert not bits or srf.same_bits(got, want), (what, "the sign of a zero")


class Cliques(object):
    """a step's clique pattern on the device"""

    def __init__(self, step):
        self.step = step
        self.q, self.c = st.CLIQUES[step]
        self.n, self.Sp, self.Sj, _, _ = st.cliques(self.q, self.c)
        self.nnz, self.T = len(self.Sj), st.clique_T(self.q, self.c)
        self.dSp, self.dSj = up(self.Sp, np.int32), up(self.Sj, np.int32)


# ---------------------------------------------------------------- the colouring and the levels, their outputs kept on the device
def ordered_on_device(bh, P, call, record, families, what):
    """call(label, order, ptr) -> (error, labels in use); the sentinels behind the three outputs as gst.color_run and
    trsvt.levels_run check them; (label, count, order, ptr) as device tensors"""
    n = P.n
    label, order = (torch.full((n + PAD,), SENT, dtype=torch.int32).cuda() for _ in range(2))
    ptr = torch.full((n + 1 + PAD,), SENT, dtype=torch.int32).cuda()
    torch.cuda.synchronize()
    err, count = call(label, order, ptr)
    assert err == 0, (what, err)
    assert bool((label[n:] == SENT).all()) and bool((order[n:] == SENT).all()), (what, "written past the end")
    assert bool((ptr[n + 1:] == SENT).all()), (what, "written past the end of the offsets")
    if n:
        assert bool((ptr[count + 1:] == SENT).all()), (what, "written behind the last offset")
        assert set(stats(bh)) <= families, (what, sorted(stats(bh)))
        scanned(bh, record, n, P.T, what)
    else:
        assert count == 0
    # (label and order with their padding, never an empty tensor; the offsets on the host, where the sweep and the solve want them)
    return label, count, order, ptr[:count + 1].cpu().numpy() if n else np.zeros(1, np.int32)


def run_colouring(bh, P, which, what):
    prio, want = st.colouring(P.step, which)
    dprio = None if prio is None else up(prio.view(np.int32), np.int32)

    def call(color, order, ptr):
        bh.color_ncolors = bh.color_rounds = -1
        err = amg.color_raw_device(bh, P.n, P.nnz, P.dSp, P.dSj if P.nnz else None, dprio, st.COLOURINGS[which][0], 0, color, order, ptr)
        return err, bh.color_ncolors if P.n else 0
    color, ncolors, order, ptr = ordered_on_device(bh, P, call, "color_order", gst.COLOR_FAMILIES, what)
    gst.color_check((color[:P.n].cpu().numpy(), ncolors, order[:P.n].cpu().numpy(), ptr, bh.color_rounds if P.n else 0), want, what)
    return color, ncolors, order, ptr


def run_levels(bh, P, upper, what):
    def call(level, order, ptr):
        bh.levels_nlevels = bh.levels_passes = -1
        err = amg.levels_raw_device(bh, P.n, P.nnz, P.dSp, P.dSj if P.nnz else None, UPPER if upper else LOWER, level, order, ptr)
        return err, bh.levels_nlevels if P.n else 0
    level, nlevels, order, ptr = ordered_on_device(bh, P, call, "levels_order", trsvt.LEVEL_FAMILIES, what)
    trsvt.levels_check((level[:P.n].cpu().numpy(), nlevels, order[:P.n].cpu().numpy(), ptr, bh.levels_passes if P.n else 0),
                       st.levels(P.step, upper), what)
    return nlevels, order, ptr


def run_sweep(bh, P, dtype, coloring, what):
    """one symmetric sweep with omega = 1/2 on the colouring's device arrays, without and with BHS_GS_VERIFY"""
    color, ncolors, order, hptr = coloring
    Ax, diag, b, x0, want = st.sweep_case(P.step)
    dAx, ddiag, db = up(Ax, dtype), up(diag, dtype), up(b, dtype)
    for flags, dcolor in ((_lib.BHS_GS_SYMMETRIC, None), (_lib.BHS_GS_SYMMETRIC | _lib.BHS_GS_VERIFY, color)):
        x = padded(x0, dtype)
        torch.cuda.synchronize()
        err = amg.gs_raw_device(bh, P.n, P.nnz, P.dSp, P.dSj, dAx, ddiag, ncolors, hptr, order, dcolor, db, x, st.OMEGA,
                                1, flags)
        assert err == 0, (what, flags, err)
        assert bool((x[P.n:] == XSENT).all()), (what, "written past the end of d_x")
        exactly(x[:P.n], want, (what, flags))
        if P.n:
            got = stats(bh)
            assert set(got) == gst.GS_FAMILIES and all(got[f]["launches"] == P.q for f in got), (what, got)


def run_ilu0(bh, dtype, what):
    """tridiagonal300's integer factors: between a levels call and a solve on the workspace the three share"""
    n, Ap, Aj, Ax, want = trsvt.factor_case("tridiagonal300")
    T = st.cached(("tridiagonal300", np.dtype(dtype).name), lambda: trsvt.Tri(n, Ap, Aj, Ax, dtype))
    got, pivot = trsvt.ilu_run(bh, T, what=what)
    assert pivot == -1 and np.array_equal(got, want), (what, pivot)


def run_solves(bh, P, dtype, lev, what):
    """the lower solve in place, the upper one with a unit diagonal into an array of its own, on the levels' device arrays"""
    Ax, xs, bl, bu = st.solve_case(P.step)
    dAx = up(Ax, dtype)
    for upper, b, flags in ((False, bl, LOWER), (True, bu, UPPER | UNIT)):
        nlevels, order, hptr = lev[upper]
        db = padded(b, dtype)
        dx = padded(np.full(P.n, 77.0), dtype) if upper else db
        torch.cuda.synchronize()
        err = amg.trsv_raw_device(bh, P.n, P.nnz, P.dSp, P.dSj, dAx, nlevels, hptr, order, 0.5, db, dx, flags)
        assert err == 0, (what, upper, err)
        assert bool((dx[P.n:] == XSENT).all()) and bool((db[P.n:] == XSENT).all()), (what, "written past the end")
        exactly(dx[:P.n], xs, (what, upper))
        if upper:
            exactly(db[:P.n], bu, (what, "d_b was written"))
        if P.n:
            assert {k: v["launches"] for k, v in stats(bh).items()} == {"trsv_level": P.q}, (what, stats(bh))


def run_cliques(bh, step, dtype, what):
    """colouring, levels, colouring, levels, colouring: the shared offsets change hands at every call; then what consumes them"""
    P = Cliques(step)
    run_colouring(bh, P, 0, what + " colouring 0")
    lev = {False: run_levels(bh, P, False, what + " lower levels")}
    run_colouring(bh, P, 1, what + " colouring 1")
    lev[True] = run_levels(bh, P, True, what + " upper levels")
    coloring = run_colouring(bh, P, 2, what + " colouring with priorities")
    run_ilu0(bh, dtype, what + " ilu0")
    run_sweep(bh, P, dtype, coloring, what + " sweep")
    run_solves(bh, P, dtype, lev, what + " solve")
    return P


# ---------------------------------------------------------------- the aggregation
def run_aggregation(bh, step, dtype, what):
    for s, w in st.AGG_CASES:
        if s != step:
            continue
        n, Sp, Sj = st.band(st.agg_n(step), w)
        if n == 0:                                                   # nothing is launched: the records are the last call's
            agg = torch.full((PAD,), aggt.SENT_AGG, dtype=torch.int32).cuda()
            torch.cuda.synchronize()
            assert amg.aggregate_raw_device(bh, 0, 0, up(Sp, np.int32), None, None, step, 0, agg, None) == 0
            assert bh.aggregate_nagg == 0 and bh.aggregate_rounds == 0 and bool((agg == aggt.SENT_AGG).all()), what
            continue
        aggt.check(aggt.run(bh, n, Sp, Sj, step, what=(what, w)), st.agg_reference(step, w, step), (what, w))
        scanned(bh, "agg_scan", n, st.words(n), (what, w))


# ---------------------------------------------------------------- the push product
def check_push(bh, case, dtype, what):
    (m, n, Gp, Gj, Gx), fidx, F, Y = st.push_inputs(case)
    want, changed, nxt = st.push_reference(case)
    D = pusht.Dev(m, n, (Gp, Gj, Gx), dtype)
    for asked in (True, False):                                      # d_next and changed_out both asked for, both omitted
        got = pusht.run(bh, case[4], D, fidx, F, Y, want_next=asked, want_changed=asked, what=what)
        exactly(got[0], want, (what, asked), bits=True)
        if asked:
            assert got[1] == changed and got[2].dtype == np.int32 and np.array_equal(got[2], nxt), (what, got[1], changed)
        scanned(bh, "push_scan", 0, st.push_scan_rows(case, asked), (what, asked))


def run_push(bh, step, dtype, what):
    for case in st.push_cases():
        if case[1] == step:
            check_push(bh, case, dtype, "%s %s" % (what, case))


# ---------------------------------------------------------------- CSR x dense: no scan, other workspaces
def run_dense(bh, step, dtype, what):
    m, A, x, X, y = st.dense_case(step)
    spmv, spmm, (srmv, changed) = st.dense_references(step)
    D = spmvt.Dev(m, st.N_COLS, A, dtype)
    exactly(spmvt.run(bh, D, x, 2.0, -1.0, y, what=what), spmv, what + " spmv")
    exactly(spmvt.run(bh, D, X, 2.0, what=what), spmm, what + " spmm")
    got = srt.run(bh, "min_plus", D, x, y, None, True, what=what)
    exactly(got[0], srmv, what + " semiring spmv", bits=True)
    assert got[1] == changed, (what, got[1], changed)


# ---------------------------------------------------------------- the refused calls
def refusals(bh, P, step, dtype, what):
    bad = P.Sj.copy()
    bad[P.nnz // 2] = P.n
    gst.color_run(bh, P.n, P.Sp, bad, want=INV, what=what + ": a column equal to n, colouring")
    run_colouring(bh, P, 0, what + ": the colouring after its refusal")
    trsvt.levels_run(bh, P.n, P.Sp, bad, LOWER, want=INV, what=what + ": a column equal to n, levels")
    run_levels(bh, P, False, what + ": the levels after their refusal")
    case = [c for c in st.push_cases() if c[1] == step and c[0] == "frontier"][0]
    (m, n, Gp, Gj, Gx), fidx, F, Y = st.push_inputs(case)
    off = fidx.copy()
    off[len(off) - 5] = m                                            # near the end of the list
    pusht.run(bh, case[4], pusht.Dev(m, n, (Gp, Gj, Gx), dtype), off, F, Y, want=INV, what=what + ": a frontier index equal to m")
    check_push(bh, case, dtype, what + ": the push after its refusal")


# ---------------------------------------------------------------- the tour
@pytest.mark.parametrize("build", sorted(BUILDS))
def test_one_handle_through_the_scan_sizes(build):
    dtype = BUILDS[build]
    plats = [False] * bhmod.NUM_PLATFORMS
    plats[bhmod.BHSPARSE_HIP] = True
    bh = bhmod.bhsparse(value_dtype=dtype)
    assert bh.initPlatform(plats) == 0
    REACHED.clear()
    try:
        for step in range(len(st.CLIQUES)):
            what = "%s, %s (%s)" % (step, st.CLIQUE_ROLES[step], build)
            P = run_cliques(bh, step, dtype, what)
            if step < len(st.COUNTS):
                run_aggregation(bh, step, dtype, what + " aggregation")
                run_push(bh, step, dtype, what + " push")
            run_dense(bh, step, dtype, what)
            if step == st.REFUSE_AFTER:
                refusals(bh, P, step, dtype, what + " refused")
        for record in sorted(REACHED):
            print("%s %s scanned: %s" % (build, record, REACHED[record]))
        print("%s reference CPU seconds: %s" % (build, {k: round(v, 2) for k, v in sorted(st.SECONDS.items())}))
        assert bh.free_mem() == 0
    finally:
        bh.freePlatform()
