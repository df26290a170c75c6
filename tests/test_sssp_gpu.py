"""The shortest paths (bhs_csr_sssp_device) and what benchmark_spgemm_using_csr_amd/graph.py builds on them, on the GPU, both
builds.

Reference: tests/ssspref.py, the definition of include/bhsparse_hip.h ("shortest paths") restated on the host, which
tests/test_sssp_abi.py holds against scipy and networkx.  dist, parent, reached, loose, the buckets and the passes are
functions of the input and delta, so all of them are compared EXACTLY: the bits of every distance, no tolerance, no entry left
out.  Sentinels sit behind every output and, after a refused call, in it; they must be intact.  The launch counts of the kernel
records are checked against the passes: 8 passes a control round trip, so the relax's launches are the passes that have a slice
rounded up to a multiple of 8 -- which is also what *passes_out reports."""
import os
import subprocess

import numpy as np
import pytest
import torch

from conftest import ROOT
import gridpass as gp
import scantiles as st
import ssspref as R

from benchmark_spgemm_using_csr_amd import _lib, graph
from benchmark_spgemm_using_csr_amd.facade import BHSPARSE_HIP, NUM_PLATFORMS, bhsparse

pytestmark = pytest.mark.gpu

DTYPES = (np.float64, np.float32)
INV = _lib.BHS_ERR_INVALID_ARG
PAD = 64
SENT = -7
INF = float("inf")
UNIFORM_SOURCES = (5, 77, 5)


def new_handle(dtype=np.float64):
    plats = [False] * NUM_PLATFORMS
    plats[BHSPARSE_HIP] = True
    bh = bhsparse(value_dtype=dtype)
    assert bh.initPlatform(plats) == 0
    return bh


@pytest.fixture(scope="module", params=DTYPES, ids=("f64", "f32"))
def hd(request):
    bh = new_handle(request.param)
    yield bh, request.param
    bh.freePlatform()


def up(a, dt):
    return torch.from_numpy(np.ascontiguousarray(a, dt).copy()).cuda()


def launches(bh):
    return {s["name"]: s["launches"] for s in bh.kernel_stats() if s["launches"] > 0}


def num_cu():
    return torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count


def device_graph(g, dtype):
    n, Gp, Gj, Gx = g
    return (up(Gp, np.int32) if len(Gp) else torch.zeros(1, dtype=torch.int32).cuda(), up(Gj, np.int32) if len(Gj) else None,
            None if Gx is None or not len(Gj) else up(Gx, dtype))


def run(bh, dtype, g, sources, delta, want=0, what="", parents=True, dev=None, nnz=None, nsrc=None, alias=None):
    """The device's answer as ssspref.answer gives it (parent None where it is not asked for), with "launched" beside it; the
    sentinels behind the outputs are checked, the launch counts against the passes, and after a refusal that the outputs and
    the handle's attributes stayed"""
    n, Gp, Gj, Gx = g
    dGp, dGj, dGx = dev if dev is not None else device_graph(g, dtype)
    src = up(np.asarray(sources, np.int32), np.int32) if len(sources) else torch.zeros(1, dtype=torch.int32).cuda()
    room = max(n, 0)
    tdt = torch.float64 if dtype == np.float64 else torch.float32
    dist = torch.full((room + PAD,), float(SENT), dtype=tdt).cuda()
    par = torch.full((room + PAD,), SENT, dtype=torch.int32).cuda()
    torch.cuda.synchronize()
    bh.sssp_reached = bh.sssp_passes = -1
    bh.sssp_ms = -1.0
    out_dist = dGx if alias == "valG" else dist
    err = graph.sssp_delta_raw_device(bh, n, len(Gj) if nnz is None else nnz, dGp, dGj, dGx, len(sources) if nsrc is None else nsrc, src,
                                      delta, 0, out_dist, par if parents else None)
    assert err == want, (what, err)
    torch.cuda.synchronize()
    assert bool((dist[room:] == SENT).all()) and bool((par[room:] == SENT).all()), (what, "written past the end")
    if not parents:
        assert bool((par == SENT).all()), (what, "d_parent was not given")
    if want != 0:
        assert bool((dist == SENT).all()) and bool((par == SENT).all()), (what, "a refused call wrote an output")
        assert bh.sssp_reached == -1 and bh.sssp_passes == -1 and bh.sssp_ms == -1.0, what
        return None
    got = {"dist": dist[:n].cpu().numpy(), "parent": par[:n].cpu().numpy() if parents else None, "reached": bh.sssp_reached,
           "launched": bh.sssp_passes}
    assert bh.sssp_ms >= 0.0, what
    if n:
        got["loose"], got["buckets"], got["passes"] = (bh.get_info(k) for k in ("sssp_loose", "sssp_buckets", "sssp_work_passes"))
        la = launches(bh)
        ran = R.launched(got["passes"])
        expect = {"sssp_check": 1, "sssp_seed": 1, "sssp_relax": ran, "sssp_advance": 3 * ran, "sssp_finish": 1}
        if parents:
            expect["sssp_parents"] = 2
        assert la == expect and got["launched"] == ran, (what, got["passes"], la)
    return got


def check(got, want, what):
    print("%s: passes %d (reference %d), buckets %d (reference %d), reached %d (reference %d), loose %d (reference %d)"
          % (what, got["passes"], want["passes"], got["buckets"], want["buckets"], got["reached"], want["reached"], got["loose"],
             want["loose"] if got["parent"] is not None else 0))
    assert got["dist"].dtype == want["dist"].dtype and len(got["dist"]) == len(want["dist"]), what
    word = np.uint64 if got["dist"].itemsize == 8 else np.uint32
    bad = np.flatnonzero(got["dist"].view(word) != want["dist"].view(word))
    assert got["dist"].tobytes() == want["dist"].tobytes(), (what, "dist", bad[:5], got["dist"][bad[:5]], want["dist"][bad[:5]])
    assert (got["reached"], got["buckets"], got["passes"]) == (want["reached"], want["buckets"], want["passes"]), what
    assert got["launched"] == R.launched(want["passes"]), what
    if got["parent"] is None:
        assert got["loose"] == 0, what
    else:
        assert np.array_equal(got["parent"], want["parent"]), (what, "parent", np.flatnonzero(got["parent"] != want["parent"])[:5])
        assert got["loose"] == want["loose"], what


def answer(key, g, sources, delta, dtype, heap=True):
    return st.cached(("sssp", key, tuple(sources) if len(sources) < 8 else len(sources), float(delta), np.dtype(dtype).name),
                     lambda: R.answer(*g, np.asarray(sources, np.int64), delta, dtype, heap), "sssp")


def both(bh, dtype, key, g, sources, delta, heap=True):
    """with the parents and without"""
    want = answer(key, g, sources, delta, dtype, heap)
    what = "%s, delta %g" % (key, delta)
    check(run(bh, dtype, g, sources, delta, what=what), want, what)
    check(run(bh, dtype, g, sources, delta, what=what, parents=False), want, what + ", without the parents")
    return want


# ---------------------------------------------------------------- exact equality
def test_smallest_sizes(hd):
    bh, dtype = hd
    empty = (0, np.zeros(1, np.int32), np.zeros(0, np.int32), None)
    got = run(bh, dtype, empty, [], 1.0, what="n = 0")
    assert got["reached"] == 0 and got["launched"] == 0 and len(got["dist"]) == 0 and bh.sssp_ms == 0.0
    one = (1, np.zeros(2, np.int32), np.zeros(0, np.int32), None)
    want = both(bh, dtype, "n = 1", one, [0], 1.0)
    assert want["dist"].tolist() == [0.0] and want["parent"].tolist() == [-1] and (want["passes"], want["buckets"]) == (1, 1)
    lonely = R.csr(5, [1, 2], [2, 3], [1.5, 2.5])                    # the source 0 has no edge; 4 neither
    want = both(bh, dtype, "a source with no edges", lonely, [0], 1.0)
    assert want["reached"] == 1 and np.isinf(want["dist"][1:]).all()
    want = both(bh, dtype, "two sources, one repeated", lonely, [1, 4, 1], INF)
    assert want["dist"].tolist() == [INF, 0.0, 1.5, 4.0, 0.0] and want["parent"].tolist() == [-1, -1, 1, 2, -1]


@pytest.mark.parametrize("delta", (1.0, INF, 0.25))
def test_unit_path_across_the_batches(hd, delta):
    """2049 passes, one vertex each: 257 batches.  At delta = 1/4 three of every four buckets are empty and add no pass"""
    bh, dtype = hd
    want = both(bh, dtype, "unit path", R.path(2049), [0], delta)
    assert want["passes"] == 2049 and want["buckets"] == (1 if delta == INF else 2049)
    assert np.array_equal(want["dist"], np.arange(2049)) and np.array_equal(want["parent"], np.arange(-1, 2048))


def test_path_of_weight_1000_jumps_the_empty_buckets(hd):
    bh, dtype = hd
    want = both(bh, dtype, "path of weight 1000", R.path(2049, 1000.0), [0], 1.0)
    assert (want["passes"], want["buckets"]) == (2049, 2049) and want["dist"][-1] == 2048000.0


@pytest.mark.parametrize("L", (1, 4, 16, 64))
def test_long_rows_go_to_a_wave(hd, L):
    """a hub row of 5000 entries and a row of 300 at every lane width"""
    bh, dtype = hd
    g = st.cached(("sssp star", L), lambda: R.star_padded(L))
    assert R.lanes(g[0], len(g[2])) == L and np.diff(g[1])[0] == 5000 > 32 * L
    for delta in (1.0, INF):
        want = both(bh, dtype, "star, L = %d" % L, g, [0], delta, heap=L <= 4)
        assert want["reached"] > 5300


def test_uniform_graph_at_three_deltas(hd):
    """unsorted rows, repeated entries, loops, weights over 16 decades with zeros, -0 and +Inf; absorbed additions"""
    bh, dtype = hd
    g = st.cached(("sssp uniform",), R.uniform)
    wants = [both(bh, dtype, "uniform", g, UNIFORM_SOURCES, delta) for delta in (1e-3, 1.0, 1e4)]
    assert all(w["dist"].tobytes() == wants[0]["dist"].tobytes() for w in wants)
    assert wants[0]["loose"] > 0 and len({(w["passes"], w["buckets"]) for w in wants}) == 3
    assert all(np.array_equal(w["parent"], wants[0]["parent"]) for w in wants)


# ---------------------------------------------------------------- capped grids
def test_the_block_loops_of_capped_grids(hd):
    """the road-like grid with unit weights at gridpass.cap_rows(numCU, 1): more blocks than 16 workgroups a CU hold, the
    last one partial, so that the check, the minimum, the gather, the parents and the finish take a second turn of their
    block loops; from 64 sources the passes stay in the hundreds.  Then from all vertices but every sixteenth: a first slice
    that is itself more than the cap's workgroups take in one turn, for the seeds and the relax"""
    bh, dtype = hd
    cus = num_cu()
    n = gp.cap_rows(cus, 1)
    width = int(np.sqrt(n)) | 1
    g = st.cached(("sssp grid", n), lambda: R.grid(n, width))
    assert R.lanes(n, len(g[2])) == 1 and gp.blocks(n, 1) > gp.CAP_A * cus and n % 256 != 0
    dev = device_graph(g, dtype)
    few = np.arange(100, n, n // 64)
    want = answer("grid", g, few, 4.0, dtype, heap=False)
    assert 100 < want["passes"] < 1000 and want["reached"] == n and want["loose"] == 0
    check(run(bh, dtype, g, few, 4.0, what="grid", dev=dev), want, "grid")
    most = np.flatnonzero(np.arange(n) % 16 != 0)
    assert len(most) > 256 * gp.CAP_A * cus
    want = answer("grid, most", g, most, 1.0, dtype, heap=False)
    assert want["passes"] == 2 and want["dist"].max() == 1.0
    check(run(bh, dtype, g, most, 1.0, what="grid from most vertices", dev=dev), want, "grid from most vertices")


# ---------------------------------------------------------------- parents and paths
def test_parents_are_tight_and_strictly_closer(hd):
    bh, dtype = hd
    n, Gp, Gj, Gx = g = st.cached(("sssp uniform",), R.uniform)
    got = run(bh, dtype, g, UNIFORM_SOURCES, 1.0, what="parents")
    dist, par = got["dist"], got["parent"]
    w = R.weights(Gx, len(Gj), dtype)
    rows = np.repeat(np.arange(n), np.diff(Gp))
    has = np.flatnonzero(par >= 0)
    assert len(has) > n // 4 and np.all(dist[par[has]] < dist[has])
    with np.errstate(over="ignore"):
        tight = (dist[rows] + w).astype(dtype) == dist[Gj]
    edges = set(zip(rows[tight].tolist(), Gj[tight].tolist()))
    assert all((int(par[v]), int(v)) in edges for v in has)
    assert set(np.flatnonzero(par == -1).tolist()) == set(np.flatnonzero(np.isinf(dist)).tolist()) | set(UNIFORM_SOURCES)
    assert np.all(np.isfinite(dist[par == -2])) and (par == -2).sum() == got["loose"] > 0


def test_parents_on_a_zero_weight_cycle(hd):
    bh, dtype = hd
    for delta in (1.0, INF):
        want = both(bh, dtype, "zero cycle", R.zero_cycle(), [0], delta)
        assert want["parent"].tolist() == [-1, 0, -2] and want["dist"].tolist() == [0.0, 2.0, 2.0] and want["loose"] == 1


def test_path_from_parents_sums_to_the_distance(hd):
    bh, dtype = hd
    n, Gp, Gj, Gx = g = st.cached(("sssp positive",), lambda: R.positive(600, 5, 5))
    G = device_graph(g, dtype)
    dist, par, reached, passes = graph.sssp_delta_device(bh, n, G, [3], parents=True)   # delta: the default
    assert dist.dtype == (torch.float64 if dtype == np.float64 else torch.float32) and par.dtype == torch.int32
    want = answer("positive", g, [3], 1.0, dtype)
    assert dist.cpu().numpy().tobytes() == want["dist"].tobytes() and np.array_equal(par.cpu().numpy(), want["parent"])
    assert reached == want["reached"] and passes % 8 == 0 and bh.get_info("sssp_loose") == want["loose"]
    dist, par = dist.cpu().numpy(), par.cpu().numpy()
    w = R.weights(Gx, len(Gj), dtype)
    walked = 0
    for target in np.flatnonzero(np.isfinite(dist))[::37]:
        chain = [int(target)]
        while par[chain[-1]] >= 0:
            chain.append(int(par[chain[-1]]))
        if par[chain[-1]] == -2:                                      # (in float a weight can be absorbed: no path to walk)
            with pytest.raises(ValueError):
                graph.path_from_parents(par, int(target))
            continue
        walked += 1
        walk = graph.path_from_parents(par, int(target))
        assert walk[0] == 3 and walk[-1] == target
        total = dtype(0)
        for a, b in zip(walk[:-1], walk[1:]):                         # left to right, one rounding an edge
            q = np.arange(Gp[a], Gp[a + 1])
            q = q[Gj[q] == b]
            total = min(dtype(total + w[k]) for k in q)
        assert total == dist[target], (target, walk)
    assert walked >= 10
    only = graph.sssp_delta_device(bh, n, G, [3], delta=INF)
    assert len(only) == 3 and only[0].cpu().numpy().tobytes() == want["dist"].tobytes()


def test_agrees_with_the_frontier_route(hd):
    """graph.sssp_frontier_device pulls from the in-edge matrix and pushes along G: the same bits"""
    bh, dtype = hd
    n, Gp, Gj, Gx = g = st.cached(("sssp uniform",), R.uniform)
    G = device_graph(g, dtype)
    Tp, Tj, Tx = R.transposed(n, Gp, Gj, Gx)
    A = (up(Tp, np.int32), up(Tj, np.int32), up(Tx, dtype))
    D = graph.sssp_frontier_device(bh, n, A, [5], At=G)
    dist, reached, passes = graph.sssp_delta_device(bh, n, G, [5])
    assert dist.cpu().numpy().tobytes() == D[:, 0].contiguous().cpu().numpy().tobytes()
    assert dist.cpu().numpy().tobytes() == answer("uniform one", g, [5], 1.0, dtype)["dist"].tobytes()


def test_bfs_levels_by_the_queue(hd):
    bh, dtype = hd
    n, Gp, Gj, Gx = g = st.cached(("sssp uniform",), R.uniform)
    G = device_graph(g, dtype)
    levels = graph.bfs_levels_queue_device(bh, n, G, [5, 77])
    want = answer("uniform bfs", (n, Gp, Gj, None), [5, 77], 1.0, dtype)
    assert levels.dtype == torch.int32
    assert np.array_equal(levels.cpu().numpy(), np.where(np.isinf(want["dist"]), 0, want["dist"] + 1).astype(np.int32))
    assert bh.get_info("sssp_work_passes") == want["passes"] == int(want["dist"][np.isfinite(want["dist"])].max()) + 1   # a pass a level


def test_sssp_delta_csr():
    n, Gp, Gj, Gx = R.positive(600, 5, 5)
    dist, par, info = graph.sssp_delta_csr(n, Gp, Gj, Gx, [3], delta=1.0, parents=True)
    want = answer("positive", (n, Gp, Gj, Gx), [3], 1.0, np.float64)
    assert dist.tobytes() == want["dist"].tobytes() and np.array_equal(par, want["parent"])
    assert (info["reached"], info["buckets"], info["loose"], info["passes"]) == (want["reached"], want["buckets"], want["loose"], R.launched(want["passes"]))


# ---------------------------------------------------------------- repeatability
def test_runs_and_handles_agree():
    g = st.cached(("sssp uniform",), R.uniform)
    for dtype in DTYPES:
        outs = []
        bh = new_handle(dtype)
        try:
            outs += [run(bh, dtype, g, UNIFORM_SOURCES, 1.0) for _ in range(2)]   # the same handle twice
        finally:
            bh.freePlatform()
        bh = new_handle(dtype)                                       # and a fresh one
        try:
            outs.append(run(bh, dtype, g, UNIFORM_SOURCES, 1.0))
        finally:
            bh.freePlatform()
        for got in outs:
            check(got, answer("uniform", g, UNIFORM_SOURCES, 1.0, dtype), "handles")
            assert got["dist"].tobytes() == outs[0]["dist"].tobytes() and got["parent"].tobytes() == outs[0]["parent"].tobytes()


# ---------------------------------------------------------------- refusals
def test_refusals(hd):
    bh, dtype = hd
    n, Gp, Gj, Gx = g = st.cached(("sssp positive",), lambda: R.positive(600, 5, 5))
    refused = {"sssp_check": 1, "sssp_seed": 1, "sssp_relax": 8, "sssp_advance": 24}   # the first batch left at once
    bad = Gx.copy(); bad[len(bad) // 2] = -1e-300 if dtype == np.float64 else -1e-30   # noqa: E702
    assert R.refusal(n, Gp, Gj, bad, [3]) == "weight"
    run(bh, dtype, (n, Gp, Gj, bad), [3], 1.0, want=INV, what="a negative weight")
    assert launches(bh) == refused, launches(bh)
    bad = Gx.copy(); bad[7] = np.nan                                 # noqa: E702
    run(bh, dtype, (n, Gp, Gj, bad), [3], 1.0, want=INV, what="a NaN weight")
    assert launches(bh) == refused
    bad = Gj.copy(); bad[len(bad) // 3] = n                          # noqa: E702
    run(bh, dtype, (n, Gp, bad, Gx), [3], 1.0, want=INV, what="a column equal to n")
    assert launches(bh) == refused
    p = Gp.copy(); p[100] = p[101] + 1                               # noqa: E702
    run(bh, dtype, (n, p, Gj, Gx), [3], 1.0, want=INV, what="a falling rowPtr")
    run(bh, dtype, g, [3], 1.0, want=INV, what="rowPtr[n] != nnz", nnz=len(Gj) - 3)
    run(bh, dtype, g, [3, n], 1.0, want=INV, what="a source equal to n")
    assert launches(bh) == refused
    run(bh, dtype, g, [-1], 1.0, want=INV, what="a negative source")
    for delta in (0.0, -1.0, float("nan"), -INF):
        run(bh, dtype, g, [3], delta, want=INV, what="delta %r" % delta)
    run(bh, dtype, g, [3], 1.0, want=INV, what="nsrc = 0", nsrc=0)
    run(bh, dtype, g, [3], 1.0, want=INV, what="a negative nsrc", nsrc=-1)
    run(bh, dtype, (-1, Gp, Gj, Gx), [3], 1.0, want=INV, what="a negative n")
    dev = device_graph(g, dtype)
    run(bh, dtype, g, [3], 1.0, want=INV, what="d_dist is d_valG", dev=dev, alias="valG")
    assert dev[2].cpu().numpy().tobytes() == np.ascontiguousarray(Gx, dtype).tobytes()
    run(bh, dtype, g, [3], 1.0, want=INV, what="a NULL rowPtr", dev=(None, dev[1], dev[2]))
    run(bh, dtype, g, [3], 1.0, want=INV, what="a NULL colInd", dev=(dev[0], None, dev[2]))
    src = up(np.array([3], np.int32), np.int32)
    torch.cuda.synchronize()
    bh.sssp_reached = -1                                              # d_parent over the columns; flags; no d_dist
    assert graph.sssp_delta_raw_device(bh, n, len(Gj), dev[0], dev[1], dev[2], 1, src, 1.0, 0, torch.zeros(n, dtype=dev[2].dtype).cuda(), dev[1][8:]) == INV
    assert graph.sssp_delta_raw_device(bh, n, len(Gj), dev[0], dev[1], dev[2], 1, src, 1.0, 1, torch.zeros(n, dtype=dev[2].dtype).cuda(), None) == INV
    assert graph.sssp_delta_raw_device(bh, n, len(Gj), dev[0], dev[1], dev[2], 1, src, 1.0, 0, None, None) == INV
    assert bh.sssp_reached == -1 and np.array_equal(dev[1].cpu().numpy(), Gj) and np.array_equal(dev[0].cpu().numpy(), Gp)
    check(run(bh, dtype, g, [3], 1.0, what="after the refusals"), answer("positive", g, [3], 1.0, dtype), "after the refusals")
    with pytest.raises(ValueError):
        graph.sssp_delta_device(bh, n, dev, [n])


def test_refused_between_symbolic_and_finish():
    n, Gp, Gj, Gx = g = R.positive(600, 5, 5)
    dGp, dGj, dGx = device_graph(g, np.float64)
    bh = new_handle()
    try:
        assert bh.initData_device(n, n, n, len(Gj), dGx, dGp, dGj, len(Gj), dGx, dGp, dGj) == 0
        assert bh.spgemm_symbolic() == 0
        run(bh, np.float64, g, [3], 1.0, want=INV, what="a multiply is open")
        assert bh.spgemm_numeric(0, n) == 0 and bh.spgemm_finish() == 0
        check(run(bh, np.float64, g, [3], 1.0, what="after finish"), answer("positive", g, [3], 1.0, np.float64), "after finish")
        bh.free_mem()
    finally:
        bh.freePlatform()


# ---------------------------------------------------------------- the demo
def test_cpp_demo_runs():
    demo_dir = os.path.join(ROOT, "tests", "sssp")
    subprocess.check_call(["make", "-C", demo_dir, "-s"])
    out = subprocess.run([os.path.join(demo_dir, "sssp_demo")], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "shortest paths of 1776 vertices" in out.stdout and "PASS" in out.stdout
