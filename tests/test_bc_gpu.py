"""The betweenness centrality (bhs_csr_betweenness_device) and what benchmark_spgemm_using_csr_amd/graph.py builds on it, on
the GPU, both builds -- which run the same code on doubles and must give the same bits.

Reference: tests/bcref.py, the definition of include/bhsparse_hip.h ("betweenness centrality") restated on the host, which
tests/test_bc_abi.py holds against networkx and closed forms.  Every output and count is a function of the input, so all of
them are compared EXACTLY: the bytes of d_bc, d_sigma and d_level, reached, passes, and the three bhs_get_info keys; no
tolerance, no entry left out.  Sentinels sit behind every output and, after a refused call, in it; they must be intact.  The
launch counts of the kernel records are checked against the reference's: one check, a seed a source, an expand and two count
launches a forward pass (8 passes a control round trip, so a multiple of 8 a source), max(deepest - 1, 0) backward launches a
source, one finish."""
import os
import re
import subprocess

import networkx as nx
import numpy as np
import pytest
import torch

from conftest import ROOT
import bcref as R
import coreref as cr
import gridpass as gp
import scantiles as st

from benchmark_spgemm_using_csr_amd import _lib, graph
from benchmark_spgemm_using_csr_amd.facade import BHSPARSE_HIP, NUM_PLATFORMS, bhsparse

pytestmark = pytest.mark.gpu

DTYPES = (np.float64, np.float32)
INV = _lib.BHS_ERR_INVALID_ARG
ACC = _lib.BHS_BC_ACCUMULATE
PAD = 64
SENT = -7
KEYS = ("bc_levels", "bc_overflow", "bc_work_passes")


def new_handle(dtype=np.float64):
    plats = [False] * NUM_PLATFORMS
    plats[BHSPARSE_HIP] = True
    bh = bhsparse(value_dtype=dtype)
    assert bh.initPlatform(plats) == 0
    return bh


@pytest.fixture(scope="module", params=DTYPES, ids=("f64", "f32"))
def hd(request):
    bh = new_handle(request.param)
    yield bh
    bh.freePlatform()


def up(a, dt=np.int32):
    return torch.from_numpy(np.ascontiguousarray(a, dt).copy()).cuda()


def launches(bh):
    return {s["name"]: s["launches"] for s in bh.kernel_stats() if s["launches"] > 0}


def num_cu():
    return torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count


def device_graph(g, T=None):
    """(dGp, dGj, dTp, dTj): T None is the undirected case, the SAME arrays"""
    n, Gp, Gj = g
    dGp, dGj = up(Gp), up(Gj) if len(Gj) else None
    if T is None:
        return dGp, dGj, dGp, dGj
    return dGp, dGj, up(T[0]), up(T[1]) if len(T[1]) else None


def run(bh, g, T, sources, want=0, what="", start=None, last=True, dev=None, nnzG=None, nnzT=None, nsrc=None, flags=None, src=None):
    """The device's answer as bcref.answer gives it; the sentinels behind the outputs are checked, the launch counts against
    the counts, and after a refusal that the outputs and the handle's attributes stayed.  start: the sums d_bc holds, added to
    under BHS_BC_ACCUMULATE"""
    n, Gp, Gj = g
    dGp, dGj, dTp, dTj = dev if dev is not None else device_graph(g, T)
    if src is None:
        src = up(np.asarray(sources, np.int32)) if len(sources) else torch.zeros(1, dtype=torch.int32).cuda()
    room = max(n, 0)
    bc = torch.full((room + PAD,), float(SENT), dtype=torch.float64).cuda()
    if start is not None:
        bc[:n] = torch.from_numpy(np.asarray(start, np.float64)).cuda()
    before = bc.clone()
    sigma = torch.full((room + PAD,), float(SENT), dtype=torch.float64).cuda()
    level = torch.full((room + PAD,), SENT, dtype=torch.int32).cuda()
    torch.cuda.synchronize()
    bh.bc_reached = bh.bc_passes = -1
    bh.bc_ms = -1.0
    info = [bh.get_info(k) for k in KEYS]
    nT = (len(Gj) if T is None else len(T[1])) if nnzT is None else nnzT
    err = graph.betweenness_raw_device(bh, n, len(Gj) if nnzG is None else nnzG, dGp, dGj, nT, dTp, dTj,
                                       len(sources) if nsrc is None else nsrc, src, (ACC if start is not None else 0) if flags is None else flags,
                                       bc, level if last else None, sigma if last else None)
    assert err == want, (what, err)
    torch.cuda.synchronize()
    assert bool((bc[room:] == SENT).all()) and bool((sigma[room:] == SENT).all()) and bool((level[room:] == SENT).all()), (what, "written past the end")
    if not last:
        assert bool((sigma == SENT).all()) and bool((level == SENT).all()), (what, "d_level and d_sigma were not given")
    if want != 0:
        assert bc.cpu().numpy().tobytes() == before.cpu().numpy().tobytes(), (what, "a refused call wrote d_bc")
        assert bool((sigma == SENT).all()) and bool((level == SENT).all()), (what, "a refused call wrote an output")
        assert bh.bc_reached == -1 and bh.bc_passes == -1 and bh.bc_ms == -1.0, what
        assert [bh.get_info(k) for k in KEYS] == info, (what, "a refused call changed the counts")
        return None
    got = {"bc": bc[:n].cpu().numpy(), "level": level[:n].cpu().numpy() if last else None, "sigma": sigma[:n].cpu().numpy() if last else None,
           "reached": bh.bc_reached, "passes": bh.bc_passes}
    got["levels"], got["overflow"], got["work"] = (bh.get_info(k) for k in KEYS)
    got["launches"] = launches(bh) if n else {}
    assert bh.bc_ms >= 0.0, what
    return got


def check(got, want, what):
    print("%s: reached %d (reference %d), passes %d (%d), levels %d (%d), overflow %d (%d), work %d (%d)"
          % (what, got["reached"], want["reached"], got["passes"], want["passes"], got["levels"], want["levels"], got["overflow"],
             want["overflow"], got["work"], want["work"]))
    for name in ("bc", "sigma"):
        if got[name] is None:
            continue
        bad = np.flatnonzero(got[name].view(np.uint64) != want[name].view(np.uint64))
        assert got[name].tobytes() == want[name].tobytes(), (what, name, len(bad), bad[:5], got[name][bad[:5]], want[name][bad[:5]])
    if got["level"] is not None:
        assert got["level"].dtype == np.int32 and np.array_equal(got["level"], want["level"]), (what, "level")
    for name in ("reached", "passes", "levels", "overflow", "work"):
        assert got[name] == want[name], (what, name, got[name], want[name])
    if len(want["bc"]):
        nsrc = want["nsrc"]
        expect = {"bc_check": 1, "bc_seed": nsrc, "bc_expand": want["passes"], "bc_count": 2 * want["passes"], "bc_finish": 1}
        if want["backs"]:
            expect["bc_back"] = want["backs"]
        assert got["launches"] == expect, (what, got["launches"], expect)


def answer(key, g, T, sources, start=None):
    def make():
        n, Gp, Gj = g
        a = R.answer(n, Gp, Gj, *((Gp, Gj) if T is None else T), sources, start)
        a["nsrc"] = len(sources)
        return a
    return st.cached(("bc", key, tuple(int(s) for s in sources) if len(sources) < 8 else len(sources), start is not None), make, "bc")


def both(bh, key, g, T, sources):
    """with d_level and d_sigma and without"""
    want = answer(key, g, T, sources)
    check(run(bh, g, T, sources, what=key), want, key)
    check(run(bh, g, T, sources, what=key, last=False), want, key + ", bc alone")
    return want


def directed(g):
    return R.transposed(*g)


# ---------------------------------------------------------------- exact equality: tiny graphs
def test_tiny_graphs(hd):
    bh = hd
    empty = (0, np.zeros(1, np.int32), np.zeros(0, np.int32))
    got = run(bh, empty, None, [], what="n = 0")
    assert (got["reached"], got["passes"], got["levels"], got["overflow"], got["work"]) == (0,) * 5 and bh.bc_ms == 0.0 and len(got["bc"]) == 0
    one = (1, np.zeros(2, np.int32), np.zeros(0, np.int32))
    want = both(bh, "n = 1", one, None, [0])
    assert want["bc"].tolist() == [0.0] and (want["reached"], want["passes"], want["levels"]) == (1, 8, 1)
    edge = R.csr(2, [0], [1])
    want = both(bh, "one edge", edge, directed(edge), [0, 1])
    assert want["bc"].tolist() == [0.0, 0.0] and want["reached"] == 3 and want["level"].tolist() == [-1, 0]
    g = R.path(5)
    want = both(bh, "a path of 5", g, directed(g), range(5))
    assert want["bc"].tolist() == [0.0, 3.0, 4.0, 3.0, 0.0]
    g = R.star(9)
    want = both(bh, "a star", g, None, range(9))
    assert want["bc"].tolist() == [56.0] + [0.0] * 8
    g = R.diamond()
    want = both(bh, "a diamond", g, directed(g), range(5))
    assert want["bc"].tolist() == [0.0, 1.0, 1.0, 3.0, 0.0] and want["backs"] == 2 + 1 + 1
    g = R.csr(3, [0, 1, 2], [1, 2, 0])
    want = both(bh, "a directed 3-cycle", g, directed(g), range(3))
    assert want["bc"].tolist() == [1.0, 1.0, 1.0]
    g = R.csr(6, [1, 2, 4], [2, 3, 5])                               # 0 has no out-edge; from 1, 4 and 5 are not reached
    want = both(bh, "a source with no out-edge", g, directed(g), [0])
    assert (want["reached"], want["levels"], want["backs"]) == (1, 1, 0) and want["level"].tolist() == [0] + [-1] * 5
    want = both(bh, "unreached vertices", g, directed(g), [1, 4])
    assert want["bc"].tolist() == [0.0, 0.0, 1.0, 0.0, 0.0, 0.0] and want["level"].tolist() == [-1, -1, -1, -1, 0, 1]
    g = R.csr(5, [0, 0, 0, 1, 1, 2, 3, 3], [0, 1, 2, 1, 3, 3, 3, 4])                      # loops at 0, 1 and 3
    want = both(bh, "loops", g, directed(g), range(5))
    assert want["bc"].tobytes() == answer("a diamond", R.diamond(), directed(R.diamond()), range(5))["bc"].tobytes()   # they never qualify
    g = R.csr(5, [0, 0, 0, 1, 2, 3], [1, 1, 2, 3, 3, 4])                                  # 0 -> 1 twice
    want = both(bh, "parallel edges", g, directed(g), [0])
    assert want["sigma"].tolist() == [1.0, 2.0, 1.0, 3.0, 3.0] and want["bc"][3] == 1.0 and want["bc"][1] == 2.0 * ((1.0 + 1.0) / 3.0)
    g = R.csr(7, [0, 0, 0, 0, 3, 1, 2, 4, 5], [4, 2, 3, 1, 5, 5, 5, 6, 6])                # row 0 descends, T's rows as they come
    T = directed(g)
    T = (T[0], np.concatenate([T[1][a:b][::-1] for a, b in zip(T[0][:-1], T[0][1:])]).astype(np.int32))
    want = both(bh, "unsorted rows", g, T, [0, 3])
    assert want["sigma"].tolist()[5] == 1.0 and answer("sorted", g, directed(g), [0, 3])["bc"].tobytes() == want["bc"].tobytes()
    g = R.diamond()
    want = both(bh, "repeated sources", g, directed(g), [0, 1, 0, 0])
    assert want["bc"].tolist() == [0.0, 3.0, 3.0, 4.0, 0.0] and want["reached"] == 3 * 5 + 3


@pytest.mark.parametrize("deepest", (6, 7, 8, 15, 16, 17))
def test_depth_against_the_batch(hd, deepest):
    """deepest + 1 passes have a slice: 7 and 8 fill one batch, 9 opens a second, 16 fills two, 17 and 18 open a third"""
    g = R.path(deepest + 1)
    want = both(hd, "path, deepest level %d" % deepest, g, directed(g), [0])
    assert want["passes"] == 8 * -(-(deepest + 1) // 8) and want["levels"] == deepest + 1 and want["backs"] == deepest - 1
    assert want["bc"].tolist() == [0.0] + [float(deepest - i) for i in range(1, deepest)] + [0.0]
    want = both(hd, "path, deepest level %d, two sources" % deepest, g, directed(g), [2, 0])
    assert want["passes"] == 8 * -(-(deepest - 1) // 8) + 8 * -(-(deepest + 1) // 8)


# ---------------------------------------------------------------- lanes
def lanes_graph(per_row):
    return st.cached(("bc uniform", per_row), lambda: cr.relabel(cr.uniform(2000, per_row, 40 + per_row), 7)[0])


@pytest.mark.parametrize("per_row,L", ((3, 1), (8, 4), (32, 16), (80, 64)))
def test_every_lane_width(hd, per_row, L):
    """an undirected graph at every lane width, T the SAME arrays; then a directed part of it, T by the handle's transpose"""
    g = lanes_graph(per_row)
    assert R.lanes(g[0], len(g[2])) == L and g[0] == 2000
    want = both(hd, "uniform, L = %d" % L, g, None, [11, 1999, 640])
    assert want["reached"] > 3 * 1500
    n, Gp, Gj = g
    r = np.repeat(np.arange(n), np.diff(Gp))
    keep = (r * 7 + Gj) % 8 != 0
    d = R.shuffled(*R.csr(n, r[keep], Gj[keep]), 9)
    T = directed(d)
    assert R.lanes(n, len(d[2])) == L and not np.array_equal(T[1], d[2])
    want = answer("uniform directed, L = %d" % L, d, T, [11, 640])
    G = (up(d[1]), up(d[2]))
    Tp, Tj, _, _ = hd.csr_transpose_device(n, n, (G[0], G[1], None), values=False)
    assert np.array_equal(Tp.cpu().numpy(), T[0]) and np.array_equal(Tj.cpu().numpy(), T[1])   # the stable transpose
    bc, level, sigma, reached, passes = graph.betweenness_device(hd, n, G, [11, 640], last=True)
    assert bc.cpu().numpy().tobytes() == want["bc"].tobytes() and sigma.cpu().numpy().tobytes() == want["sigma"].tobytes()
    assert np.array_equal(level.cpu().numpy(), want["level"]) and (reached, passes) == (want["reached"], want["passes"])
    check(run(hd, d, T, [11, 640], what="directed"), want, "uniform directed, L = %d" % L)


def test_a_hub_row_goes_to_a_wave(hd):
    """coreref.hub(): a row of 1002 entries at one lane a row, past 32 entries a lane"""
    g = st.cached(("bc hub",), cr.hub)
    assert R.lanes(g[0], len(g[2])) == 1 and np.diff(g[1])[0] == 1002 > 32
    want = both(hd, "hub", g, None, [0, 3, 1003, 1])
    assert want["bc"][0] > 1000.0 and want["reached"] == 3 * 1003 + 1


# ---------------------------------------------------------------- inexact sums, overflow
def test_inexact_sums_follow_the_stated_order(hd):
    """a chain of 45 stages of widths 3, 5, 7, each fully joined to the next, entries shuffled inside rows: sigma passes 2^53
    around stage 30.  Then the same with edges left out, where a stage's path counts differ and another ORDER gives other bits"""
    for drop in (0.0, 0.15):
        g = st.cached(("bc stages", drop), lambda: R.stages([3, 5, 7] * 15, seed=5, drop=drop))
        T = directed(g)
        T = R.shuffled(g[0], T[0], T[1], 8)[1:]
        want = both(hd, "stages, drop %g" % drop, g, T, [0, 1, 17])
        assert want["sigma"].max() > 2.0 ** 53 and want["overflow"] == 0 and np.isfinite(want["bc"]).all()
        frac = want["bc"] != np.floor(want["bc"])
        assert frac.any()


def test_overflow_to_infinity(hd):
    """1030 diamonds: sigma doubles a diamond and reaches +Inf; Inf * 0 is NaN, and every NaN is the one word"""
    g = st.cached(("bc diamonds",), lambda: R.diamonds(1030))
    want = both(hd, "diamonds", g, directed(g), [0])
    assert want["overflow"] == 1 and np.isinf(want["sigma"]).sum() == 19 and np.isnan(want["bc"]).any() and want["levels"] == 2061
    want = both(hd, "diamonds, two sources", g, directed(g), [0, 3 * 20])
    assert want["overflow"] == 1                                      # from the 20th joint only 1010 diamonds lie ahead


# ---------------------------------------------------------------- capped grids
def test_the_block_loops_of_capped_grids(hd):
    """a fan: source 0 -> gridpass.cap_rows(numCU, 1) middle vertices -> one sink, one lane a row; the middle slice is more
    than 16 workgroups a CU hold, the last one partial, so the expand, the count and the backward launch take a second turn
    of their block loops; the source's row and the sink's in-row are hub rows"""
    cus = num_cu()
    m = gp.cap_rows(cus, 1)
    g = st.cached(("bc fan", m), lambda: R.fan(m))
    assert R.lanes(g[0], len(g[2])) == 1 and gp.blocks(m, 1) > gp.CAP_A * cus and m % 256 != 0
    T = st.cached(("bc fan T", m), lambda: directed(g))
    dev = device_graph(g, T)
    want = answer("fan", g, T, [0])
    assert (want["reached"], want["levels"], want["backs"]) == (m + 2, 3, 1) and want["sigma"][-1] == float(m)
    assert np.all(want["bc"][1:m + 1] == 1.0 / m)
    check(run(hd, g, T, [0], what="fan", dev=dev), want, "fan")
    want = answer("fan", g, T, [0, 5])
    check(run(hd, g, T, [0, 5], what="fan, two sources", dev=dev), want, "fan, two sources")
    print("reference seconds: %.2f" % st.SECONDS["bc"])


# ---------------------------------------------------------------- contracts
def test_accumulate_chains_to_the_bits_of_one_call(hd):
    g = lanes_graph(8)
    sources = [11, 1999, 640, 11, 5]
    want = answer("uniform, five sources", g, None, sources)
    check(run(hd, g, None, sources, what="one call"), want, "one call")
    dev = device_graph(g)
    bc = np.zeros(g[0])
    reached = 0
    for k, s in enumerate(sources):                                   # k chained single-source calls
        got = run(hd, g, None, [s], what="chained", start=bc, dev=dev)
        bc, reached = got["bc"], reached + got["reached"]
    assert bc.tobytes() == want["bc"].tobytes() and reached == want["reached"]
    assert got["sigma"].tobytes() == want["sigma"].tobytes() and np.array_equal(got["level"], want["level"])
    start = np.r_[np.nan, -np.nan, np.inf, np.arange(g[0] - 3, dtype=np.float64) / 3.0]   # what the caller passes in is added to
    check(run(hd, g, None, [640], what="onto a caller's sums", start=start, dev=dev), answer("uniform, onto", g, None, [640], start), "onto a caller's sums")


def test_runs_handles_and_builds_agree():
    g = st.cached(("bc stages", 0.15), lambda: R.stages([3, 5, 7] * 15, seed=5, drop=0.15))
    T = directed(g)
    want = answer("stages, handles", g, T, [0, 2])
    outs = []
    for dtype in DTYPES:
        bh = new_handle(dtype)
        try:
            outs += [run(bh, g, T, [0, 2]) for _ in range(2)]        # the same handle twice
        finally:
            bh.freePlatform()
        bh = new_handle(dtype)                                        # and a fresh one
        try:
            outs.append(run(bh, g, T, [0, 2]))
        finally:
            bh.freePlatform()
    for got in outs:
        check(got, want, "handles")
        assert got["bc"].tobytes() == outs[0]["bc"].tobytes() and got["sigma"].tobytes() == outs[0]["sigma"].tobytes()


def test_refusals(hd):
    bh = hd
    n, Gp, Gj = g = lanes_graph(8)
    r = np.repeat(np.arange(n), np.diff(Gp))
    keep = (r * 7 + Gj) % 8 != 0
    n, Gp, Gj = g = R.csr(n, r[keep], Gj[keep])
    Tp, Tj = T = directed(g)
    assert R.refusal(n, Gp, Gj, Tp, Tj, [3]) is None
    refused = {"bc_check": 1, "bc_seed": 1, "bc_expand": 8, "bc_count": 16}   # the first batch left at once
    start = np.arange(n, dtype=np.float64)
    bad = Gj.copy(); bad[len(bad) // 3] = n                          # noqa: E702
    for st_ in (None, start):                                         # ... under ACCUMULATE too
        run(bh, (n, Gp, bad), T, [3], want=INV, what="a column of G equal to n", start=st_)
        assert launches(bh) == refused, launches(bh)
    bad = Tj.copy(); bad[7] = -1                                     # noqa: E702
    run(bh, g, (Tp, bad), [3], want=INV, what="a negative column of T")
    assert launches(bh) == refused
    p = Gp.copy(); p[100] = p[101] + 1                               # noqa: E702
    run(bh, (n, p, Gj), T, [3], want=INV, what="a falling rowPtr of G")
    p = Tp.copy(); p[100] = p[101] + 1                               # noqa: E702
    run(bh, g, (p, Tj), [3], want=INV, what="a falling rowPtr of T")
    p = Gp.copy(); p[0] = 1                                          # noqa: E702
    run(bh, (n, p, Gj), T, [3], want=INV, what="rowPtr of G starts at 1")
    run(bh, g, T, [3], want=INV, what="rowPtrG[n] != nnzG", nnzG=len(Gj) - 3)
    run(bh, g, T, [3], want=INV, what="rowPtrT[n] != nnzT", nnzT=len(Tj) - 3)
    assert launches(bh) == refused
    run(bh, g, T, [3, n], want=INV, what="a source equal to n")
    assert launches(bh) == refused
    run(bh, g, T, [3, 5, -1], want=INV, what="a negative source", start=start)
    # by the host: nothing is launched
    dev = device_graph(g, T)
    run(bh, g, T, [3], want=INV, what="nsrc = 0", nsrc=0, dev=dev)
    run(bh, g, T, [3], want=INV, what="a negative nsrc", nsrc=-1, dev=dev)
    run(bh, g, T, [3], want=INV, what="a negative nnzT", nnzT=-1, dev=dev)
    run(bh, (-1, Gp, Gj), T, [3], want=INV, what="a negative n", dev=dev)
    run(bh, g, T, [3], want=INV, what="unknown flags", flags=2, dev=dev)
    run(bh, g, T, [3], want=INV, what="unknown flags beside ACCUMULATE", flags=ACC | 4, dev=dev)
    run(bh, g, T, [3], want=INV, what="a NULL rowPtr of G", dev=(None,) + dev[1:])
    run(bh, g, T, [3], want=INV, what="a NULL colInd of G", dev=(dev[0], None) + dev[2:])
    run(bh, g, T, [3], want=INV, what="a NULL rowPtr of T", dev=(dev[0], dev[1], None, dev[3]))
    run(bh, g, T, [3], want=INV, what="a NULL colInd of T", dev=dev[:3] + (None,))
    src = up(np.array([3], np.int32))
    room = torch.zeros(n + 8, dtype=torch.float64).cuda()
    torch.cuda.synchronize()
    bh.bc_reached = -1
    raw = lambda *out: graph.betweenness_raw_device(bh, n, len(Gj), dev[0], dev[1], len(Tj), dev[2], dev[3], 1, src, 0, *out)   # noqa: E731
    assert raw(None, None, None) == INV                               # no d_bc
    assert raw(room, dev[3][8:], None) == INV                         # d_level over T's columns
    assert raw(room, None, room[4:]) == INV                           # d_sigma over d_bc
    assert raw(dev[1][:len(Gj) // 2 * 2].view(torch.float64), None, None) == INV         # d_bc over G's columns
    assert graph.betweenness_raw_device(bh, n, len(Gj), dev[0], dev[1], len(Tj), dev[2], dev[3], 1, None, 0, room, None, None) == INV
    assert bh.bc_reached == -1 and np.array_equal(dev[1].cpu().numpy(), Gj) and np.array_equal(dev[3].cpu().numpy(), Tj)
    assert float(room.abs().sum()) == 0.0
    check(run(bh, g, T, [3, 5], what="after the refusals", dev=dev), answer("refusals", g, T, [3, 5]), "after the refusals")
    check(run(bh, g, None, [3], what="inputs alias each other", dev=dev[:2] + dev[:2]), answer("refusals, T = G", g, None, [3]), "T = G")
    with pytest.raises(ValueError):
        graph.betweenness_device(bh, n, dev[:2], [n], Gt=dev[2:])


def test_refused_between_symbolic_and_finish():
    n, Gp, Gj = g = lanes_graph(3)
    dGp, dGj = up(Gp), up(Gj)
    vals = torch.ones(len(Gj), dtype=torch.float64).cuda()
    bh = new_handle()
    try:
        assert bh.initData_device(n, n, n, len(Gj), vals, dGp, dGj, len(Gj), vals, dGp, dGj) == 0
        assert bh.spgemm_symbolic() == 0
        run(bh, g, None, [3], want=INV, what="a multiply is open")
        assert bh.spgemm_numeric(0, n) == 0 and bh.spgemm_finish() == 0
        check(run(bh, g, None, [3], what="after finish"), answer("after finish", g, None, [3]), "after finish")
        bh.free_mem()
    finally:
        bh.freePlatform()


# ---------------------------------------------------------------- graph.py on top
def test_betweenness_csr_has_networkx_conventions():
    n, Gp, Gj = g = st.cached(("bc small",), lambda: cr.relabel(cr.uniform(120, 4, 3), 2)[0])
    r = np.repeat(np.arange(n), np.diff(Gp))
    G = nx.Graph()
    G.add_nodes_from(range(n))
    G.add_edges_from(zip(r.tolist(), Gj.tolist()))
    rel = (3 * len(Gj) + n) * 2.0 ** -52                              # tests/test_bc_abi.py's bound
    raw = R.answer(n, Gp, Gj, Gp, Gj, np.arange(n))["bc"]
    for normalized in (False, True):
        bc, info = graph.betweenness_csr(n, Gp, Gj, directed=False, normalized=normalized)
        want = nx.betweenness_centrality(G, normalized=normalized)
        want = np.array([want[v] for v in range(n)])
        assert bc.tobytes() == (raw * (1.0 / ((n - 1) * (n - 2))) if normalized else raw * 0.5).tobytes()
        assert np.all(np.abs(bc - want) <= 2 * rel * np.maximum(bc, want))   # (the scaling's rounding on both sides)
        assert info["passes"] % 8 == 0 and info["overflow"] == 0 and info["reached"] == int(sum(len(c) ** 2 for c in nx.connected_components(G)))
    bc, info = graph.betweenness_csr(n, Gp, Gj, sources=[5, 9])
    assert bc.tobytes() == R.answer(n, Gp, Gj, *directed(g), [5, 9])["bc"].tobytes()   # directed: the transpose is the handle's
    est, info = graph.betweenness_sample_csr(n, Gp, Gj, 30, seed=4, directed=False)
    piv = np.sort(np.random.default_rng(4).choice(n, 30, replace=False))
    assert np.array_equal(info["pivots"], piv)
    assert est.tobytes() == (R.answer(n, Gp, Gj, Gp, Gj, piv)["bc"] * 0.5 * (n / 30.0)).tobytes()
    for directed_ in (True, False):                                   # all vertices as pivots: the exact value, whatever the convention
        for normalized in (True, False):
            exact, _ = graph.betweenness_csr(n, Gp, Gj, directed=directed_, normalized=normalized)
            est, _ = graph.betweenness_sample_csr(n, Gp, Gj, n, seed=1, directed=directed_, normalized=normalized)
            assert est.tobytes() == exact.tobytes(), (directed_, normalized)
    want = nx.betweenness_centrality(G, normalized=True)
    est, _ = graph.betweenness_sample_csr(n, Gp, Gj, n, directed=False, normalized=True)
    assert np.all(np.abs(est - [want[v] for v in range(n)]) <= 2 * rel * est)


def test_closeness(hd):
    n, Gp, Gj = g = st.cached(("bc small",), lambda: cr.relabel(cr.uniform(120, 4, 3), 2)[0])
    G = (up(Gp), up(Gj))
    src = [0, 17, 119]
    classic, harmonic = graph.closeness_device(hd, n, G, src)
    H = nx.Graph()
    H.add_nodes_from(range(n))
    H.add_edges_from(zip(np.repeat(np.arange(n), np.diff(Gp)).tolist(), Gj.tolist()))
    for k, s in enumerate(src):
        assert abs(classic[k] - nx.closeness_centrality(H, u=s, wf_improved=True)) <= 4 * 2.0 ** -52 * classic[k]
        assert abs(harmonic[k] - nx.harmonic_centrality(H, nbunch=[s])[s]) <= n * 2.0 ** -52 * harmonic[k]
    lonely = R.csr(4, [1], [2])
    classic, harmonic = graph.closeness_device(hd, 4, (up(lonely[1]), up(lonely[2])), [0, 1])
    assert classic.tolist() == [0.0, 1.0 / 3.0] and harmonic.tolist() == [0.0, 1.0]


# ---------------------------------------------------------------- the demo
def test_cpp_demo_runs():
    demo_dir = os.path.join(ROOT, "tests", "bc")
    subprocess.check_call(["make", "-C", demo_dir, "-s"])
    out = subprocess.run([os.path.join(demo_dir, "bc_demo")], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "betweenness of 456 vertices" in out.stdout and "PASS" in out.stdout
    n, Gp, Gj = g = R.grid_with_diagonals()
    want = R.answer(n, Gp, Gj, Gp, Gj, (np.arange(n) * 7) % n)
    m = re.search(r"(\d+) entries, (\d+) lanes from all sources: levels (\d+), passes (\d+); the most central vertex (\d+) at (\S+); hash ([0-9a-f]{16})",
                  out.stdout)
    assert m, out.stdout
    top = int(np.argmax(want["bc"]))
    assert (int(m.group(1)), int(m.group(2)), int(m.group(3)), int(m.group(4))) == (len(Gj), 4, want["levels"], want["passes"])
    assert int(m.group(5)) == top and float.fromhex(m.group(6)) == want["bc"][top]
    assert int(m.group(7), 16) == R.fnv(want["bc"].tobytes())
