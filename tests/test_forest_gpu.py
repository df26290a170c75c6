"""The spanning forest (bhs_csr_spanning_forest_device) and what benchmark_spgemm_using_csr_amd/graph.py builds on it, on the
GPU, both builds.

Reference: tests/forestref.py, the contract of include/bhsparse_hip.h ("spanning forest") restated in numpy; its rounds are
checked against Kruskal's algorithm in tests/test_forest_abi.py.  Everything the call returns is a function of the input --
the slot order of the edge list, the labels and the number of hooking rounds included -- so all of it is compared exactly, the
weights by their bits, and so are the launches of the three kernel records, which follow from the trees every round hooked.
Sentinels sit behind every output and behind the edges written; they must be intact, also after a refused call, and a
refusal by the host leaves the outputs themselves untouched.

The edge list scans ONE COUNT PER 64 VERTICES (the written slots among them) with the library's one-pass scan over tiles of
scantiles.SCAN_TILE counts: the clique sizes of test_components_abi.CLIQUES put ceil(n / 64) above a tile, at none, at one
count, at exactly a tile, at several tiles and a remainder and just under a tile, and one handle goes through them in that
order."""
import os
import subprocess

import numpy as np
import pytest
import torch

from conftest import ROOT
import ccref
import forestref as fr
import scantiles as st
from test_components_abi import CLIQUES, scanned

from benchmark_spgemm_using_csr_amd import _lib, facade, graph
from benchmark_spgemm_using_csr_amd.facade import BHSPARSE_HIP, NUM_PLATFORMS, bhsparse

pytestmark = pytest.mark.gpu

DTYPES = (np.float64, np.float32)
INV = _lib.BHS_ERR_INVALID_ARG
PAD = 64
SENT = -7
FAMILIES = {"forest_pick", "forest_hook", "forest_list"}
LANES = {"path300": 1, "poisson5pt_33": 4, "poisson27pt_9": 16, "two_k70": 64, "star_centre_last": 64}


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


def expected_launches(n, nedges, hooks):
    """the three records' launches from the trees every hooking round hooked: a round is clear, weight and edge, then the
    hook, ceil(log2 R) jumps from its R roots and the relabel; after the hooking rounds one more finds nothing, unless a
    single tree is left; the start and the list's three come on top"""
    roots = [n]
    for k in hooks:
        roots.append(roots[-1] - k)
    if not (hooks and roots[-1] == 1):
        roots.append(None)                                           # (the closing round: its roots are roots[-2])
    runs = [r for r in roots[:-1]]
    jumps = sum(int(np.ceil(np.log2(r))) if r > 1 else 0 for r in runs)
    return {"forest_pick": 1 + 3 * len(runs), "forest_hook": 2 * len(runs) + jumps, "forest_list": 3}


def run(bh, dtype, n, Ap, Aj, Ax=None, flags=0, want=0, what="", nnz=None, dev=None, alias=None, valued=True, by_host=True):
    """The device's answer (label, lo, hi, val, nedges, rounds) as numpy (val None where it is not asked for); the sentinels
    behind the outputs and behind the edges written are checked, and after a refusal that the handle's attributes stayed --
    and, where the host refuses, the outputs"""
    if dev is None:
        dev = (up(Ap, np.int32) if len(Ap) else torch.zeros(1, dtype=torch.int32).cuda(), up(Aj, np.int32) if len(Aj) else None,
               up(Ax, dtype) if Ax is not None and len(Aj) else None)
    dAp, dAj, dAx = dev
    room = max(n, 0)
    label, lo, hi = (torch.full((room + PAD,), SENT, dtype=torch.int32).cuda() for _ in range(3))
    val = torch.full((room + PAD,), float(SENT), dtype=torch.float64 if dtype == np.float64 else torch.float32).cuda()
    torch.cuda.synchronize()
    bh.forest_nedges = bh.forest_rounds = -1
    bh.forest_ms = -1.0
    outs = {"label": label, "lo": lo, "hi": hi, "val": val if valued else None}
    if alias:
        outs[alias[0]] = outs[alias[1]]
    err = graph.spanning_forest_raw_device(bh, n, len(Aj) if nnz is None else nnz, dAp, dAj, dAx, flags, outs["label"], outs["lo"],
                                           outs["hi"], outs["val"])
    assert err == want, (what, err)
    for t in (label, lo, hi):
        assert bool((t[room:] == SENT).all()), (what, "written past the end")
    assert bool((val[room:] == SENT).all()), (what, "written past the end")
    if not valued:
        assert bool((val == SENT).all()), (what, "d_edgeVal was not given")
    if want != 0:
        assert bh.forest_nedges == -1 and bh.forest_rounds == -1 and bh.forest_ms == -1.0, what
        if by_host:
            assert all(bool((t == SENT).all()) for t in (label, lo, hi, val)), (what, "an output was touched")
        return None
    m = bh.forest_nedges
    assert 0 <= m <= max(n - 1, 0) and bh.forest_ms >= 0.0, what
    assert bool((lo[m:] == SENT).all()) and bool((hi[m:] == SENT).all()) and bool((val[m:] == SENT).all()), (what, "written behind nedges")
    if n:
        assert set(launches(bh)) == FAMILIES, (what, launches(bh))
    else:
        assert bh.forest_ms == 0.0
    return (label[:n].cpu().numpy(), lo[:m].cpu().numpy(), hi[:m].cpu().numpy(), val[:m].cpu().numpy() if valued else None, m,
            bh.forest_rounds)


def check(got, want, what, n=None, bh=None):
    label, lo, hi, val, nedges, nrounds = got
    wlabel, wlo, whi, ww, wnedges, wrounds, info = want
    assert (nedges, nrounds) == (wnedges, wrounds), (what, nedges, nrounds, wnedges, wrounds)
    assert np.array_equal(lo, wlo) and np.array_equal(hi, whi), (what, "edges", np.flatnonzero((lo != wlo) | (hi != whi))[:5])
    assert val is None or fr.bits(val) == fr.bits(ww), (what, "weights")
    assert np.array_equal(label, wlabel), (what, "labels", np.flatnonzero(label != wlabel)[:5])
    if bh is not None and n:
        assert launches(bh) == expected_launches(n, nedges, info["hooks"]), (what, launches(bh), info)


# ---------------------------------------------------------------- the patterns
def test_empty():
    """n == 0 on a fresh handle: nothing is launched, so no kernel record exists"""
    for dtype in DTYPES:
        bh = new_handle(dtype)
        try:
            got = run(bh, dtype, 0, np.zeros(1, np.int32), np.zeros(0, np.int32), what="n = 0")
            assert got[4:] == (0, 0) and len(got[0]) == 0 and bh.forest_ms == 0.0 and launches(bh) == {}
        finally:
            bh.freePlatform()
    assert fr.sync_rounds(0, np.zeros(1, np.int32), np.zeros(0, np.int32))[4:6] == (0, 0)


@pytest.mark.parametrize("name", fr.PATTERNS)
def test_against_the_restatement(hd, name):
    """every weight maker and no values, under the four flag combinations: edge list in slot order, weights by their bits,
    nedges, rounds, labels, launches; the labels' partition is the components'"""
    bh, dtype = hd
    n, Ap, Aj = fr.pattern(name)
    if name in LANES:                                                # the lanes a row of bhs_host_aggregate.inc.h's ag_lanes
        mean = len(Aj) / n
        assert (1 if mean <= 4 else 4 if mean <= 16 else 16 if mean <= 64 else 64) == LANES[name], (name, mean)
    dAp, dAj = up(Ap, np.int32), up(Aj, np.int32) if len(Aj) else None
    root = ccref.components(n, Ap, Aj)[0]
    for maker in fr.MAKERS:
        Ax = fr.weights(name, maker)
        dAx = up(Ax, dtype) if Ax is not None and len(Aj) else None
        for flags in fr.FLAGS:
            what = (name, maker, flags)
            got = run(bh, dtype, n, Ap, Aj, Ax, flags, what=what, dev=(dAp, dAj, dAx))
            check(got, fr.reference(name, maker, flags), what, n, bh)
            assert np.array_equal(got[0][got[0]], got[0]) and np.all(got[1] < got[2]), what
            if maker != "specials":                                  # (a NaN is no edge: there the partition is the restatement's)
                assert fr.same_partition(got[0], root) and got[4] == n - len(np.unique(root)), what
    got = run(bh, dtype, n, Ap, Aj, fr.weights(name, "ties"), 0, what=(name, "no d_edgeVal"), valued=False)
    check(got, fr.reference(name, "ties", 0), (name, "no d_edgeVal"))
    if name == "powerlaw3000":
        assert np.diff(Ap).max() > 512                               # a hub row beyond every lanes-per-row
    if name == "random_directed":
        assert fr.reference(name, "none", 0)[5] >= 4                 # several rounds, thousands of trees left


def test_the_increasing_path_is_one_round_and_a_deep_chain(hd):
    bh, dtype = hd
    n, Ap, Aj, Ax = fr.increasing_path()
    want = fr.sync_rounds(n, Ap, Aj, Ax, 0)
    got = run(bh, dtype, n, Ap, Aj, Ax, what="increasing path")
    check(got, want, "increasing path", n, bh)
    assert got[4:] == (299, 1) and np.all(got[0] == 0) and want[6]["jumps"] == [9]
    assert launches(bh)["forest_hook"] == 2 + 9                      # one tree is left: no closing round
    want = fr.sync_rounds(n, Ap, Aj, Ax, fr.MAXIMUM)                 # from the other end
    got = run(bh, dtype, n, Ap, Aj, Ax, fr.MAXIMUM, what="decreasing path")
    check(got, want, "decreasing path", n, bh)
    assert got[4:] == (299, 1) and np.all(got[0] == got[0][0])


def test_the_case_by_hand(hd):
    bh, dtype = hd
    n, Ap, Aj, Ax = fr.by_hand()
    label, lo, hi, val, nedges, nrounds = run(bh, dtype, n, Ap, Aj, Ax, what="by hand")
    assert (nedges, nrounds) == (4, 2) and label.tolist() == [0, 0, 0, 0, 0, 5]
    assert list(zip(lo.tolist(), hi.tolist(), val.tolist())) == [(0, 1, 2.0), (0, 4, 2.0), (2, 3, 0.0), (2, 4, 0.0)]
    assert np.signbit(val).tolist() == [False, False, True, False]
    assert launches(bh) == {"forest_pick": 1 + 3 * 3, "forest_hook": 3 * 2 + 3 + 2 + 1, "forest_list": 3}   # R = 6, 3, 2
    label, lo, hi, val, nedges, nrounds = run(bh, dtype, n, Ap, Aj, Ax, fr.MAXIMUM, what="by hand, maximum")
    assert sorted(zip(lo.tolist(), hi.tolist(), val.tolist())) == [(0, 1, 5.0), (0, 4, 2.0), (1, 2, 2.0), (3, 4, 1.0)]
    assert label[5] == 5 and len(set(label[:5].tolist())) == 1
    for flags in fr.FLAGS:
        check(run(bh, dtype, n, Ap, Aj, Ax, flags, what=("by hand", flags)), fr.sync_rounds(n, Ap, Aj, Ax, flags), ("by hand", flags), n, bh)


def clique_answer(q, c):
    """disjoint K_q with unit weights, members m0 < m1 < ...: every vertex picks its edge of least (lo, hi) -- m0 picks
    {m0, m1}, every other mk picks {m0, mk} -- so the pair (m0, m1) is mutual, m0 stays and every other member hooks to it in
    slot mk: one round"""
    n, Sp, Sj, members, clique_of = st.cliques(q, c)
    if n == 0:
        return (np.zeros(0, np.int32),) * 3 + (np.zeros(0), 0, 0, {"hooks": []})
    first = members[clique_of, 0]
    other = np.flatnonzero(first != np.arange(n))
    return (first.astype(np.int32), first[other].astype(np.int32), other.astype(np.int32), np.ones(len(other)), len(other),
            1 if q > 1 else 0, {"hooks": [len(other)] if q > 1 else []})


def test_one_handle_through_the_scan_sizes(hd):
    """the edge list's scan over ceil(n / 64) counts: above a tile, none, one count, exactly a tile, several tiles and a
    remainder, just under a tile, in that order on one handle"""
    bh, dtype = hd
    assert tuple(st.role_of(scanned(q, c)) for q, c in CLIQUES) == st.ROLES
    n, Sp, Sj, _, _ = st.cliques(3, 7)
    want, closed = fr.sync_rounds(n, Sp, Sj), clique_answer(3, 7)
    assert all(np.array_equal(a, b) for a, b in zip(want[:4], closed[:4])) and want[4:6] == closed[4:6]
    for role, (q, c) in zip(st.ROLES, CLIQUES):
        n, Sp, Sj, _, _ = st.cliques(q, c)
        got = run(bh, dtype, n, Sp, Sj, what=role)
        check(got, clique_answer(q, c), role, n, bh)
        if n:
            rows = {s["name"]: s["rows"] for s in bh.kernel_stats()}["forest_list"]
            assert rows == n + scanned(q, c) + got[4], (role, rows)


# ---------------------------------------------------------------- repeatability
def test_runs_handles_and_libraries_agree():
    n, Ap, Aj = fr.pattern("uniform2048")
    Ax = fr.weights("uniform2048", "specials")
    outs = []
    for dtype in DTYPES:
        bh = new_handle(dtype)
        try:
            outs += [run(bh, dtype, n, Ap, Aj, Ax, fr.ABS) for _ in range(2)]   # the same handle twice
        finally:
            bh.freePlatform()
        bh = new_handle(dtype)                                       # and a fresh one
        try:
            outs.append(run(bh, dtype, n, Ap, Aj, Ax, fr.ABS))
        finally:
            bh.freePlatform()
    for got in outs:
        check(got, fr.reference("uniform2048", "specials", fr.ABS), "handles")
        for a, b in zip(got[:3], outs[0][:3]):
            assert a.tobytes() == b.tobytes()
        assert fr.bits(got[3]) == fr.bits(outs[0][3])                # the float build's weights widen to the double build's


# ---------------------------------------------------------------- refusals
def test_refusals(hd):
    bh, dtype = hd
    n, Ap, Aj = fr.pattern("poisson5pt_33")
    Ax = fr.weights("poisson5pt_33", "ties")
    bad = Aj.copy(); bad[len(bad) // 2] = n                          # noqa: E702
    run(bh, dtype, n, Ap, bad, Ax, want=INV, what="a column equal to n", by_host=False)
    bad = Aj.copy(); bad[7] = -1                                     # noqa: E702
    run(bh, dtype, n, Ap, bad, Ax, want=INV, what="a negative column", by_host=False)
    p = Ap.copy(); p[100] = p[101] + 1                               # noqa: E702
    run(bh, dtype, n, p, Aj, Ax, want=INV, what="a decreasing rowPtr", by_host=False)
    run(bh, dtype, n, Ap, Aj, Ax, want=INV, what="nnzA below rowPtr[n]", nnz=len(Aj) - 3, by_host=False)
    for pair in (("lo", "label"), ("hi", "lo"), ("hi", "label")):
        run(bh, dtype, n, Ap, Aj, Ax, want=INV, what="%s is %s" % pair, alias=pair)
    run(bh, dtype, n, Ap, Aj, Ax, 4, want=INV, what="flags = 4")
    run(bh, dtype, n, Ap, Aj, Ax, -1, want=INV, what="flags = -1")
    run(bh, dtype, -1, Ap, Aj, Ax, want=INV, what="a negative n")
    run(bh, dtype, n, Ap, Aj, Ax, want=INV, what="a negative nnzA", nnz=-1)
    dAp, dAj, dAx = up(Ap, np.int32), up(Aj, np.int32), up(Ax, dtype)
    run(bh, dtype, n, Ap, Aj, want=INV, what="a NULL rowPtr", dev=(None, dAj, dAx))
    run(bh, dtype, n, Ap, Aj, want=INV, what="a NULL colInd", dev=(dAp, None, dAx))
    # outputs inside A: the labels over the columns, the weights over the values, the edges over the row pointer; no label
    torch.cuda.synchronize()
    bh.forest_nedges = -1
    spare = [torch.full((n + PAD,), SENT, dtype=torch.int32).cuda() for _ in range(3)]
    raw = graph.spanning_forest_raw_device
    assert raw(bh, n, len(Aj), dAp, dAj, dAx, 0, dAj[8:], spare[0], spare[1], None) == INV and bh.forest_nedges == -1
    assert raw(bh, n, len(Aj), dAp, dAj, dAx, 0, spare[0], spare[1], spare[2], dAx[4:]) == INV and bh.forest_nedges == -1
    assert raw(bh, n, len(Aj), dAp, dAj, dAx, 0, spare[0], dAp[1:], spare[2], None) == INV and bh.forest_nedges == -1
    assert raw(bh, n, len(Aj), dAp, dAj, dAx, 0, None, spare[1], spare[2], None) == INV and bh.forest_nedges == -1
    assert raw(bh, n, len(Aj), dAp, dAj, dAx, 0, spare[0], None, spare[2], None) == INV and bh.forest_nedges == -1
    assert raw(bhsparse(value_dtype=dtype), n, len(Aj), dAp, dAj, dAx, 0, spare[0], spare[1], spare[2], None) == _lib.BHS_ERR_NOT_READY
    assert np.array_equal(dAj.cpu().numpy(), Aj) and np.array_equal(dAp.cpu().numpy(), Ap)
    assert np.array_equal(dAx.cpu().numpy(), Ax.astype(dtype)) and all(bool((s == SENT).all()) for s in spare)
    check(run(bh, dtype, n, Ap, Aj, Ax, what="after the refusals"), fr.reference("poisson5pt_33", "ties", 0), "after the refusals", n, bh)


def test_refused_between_symbolic_and_finish():
    n, Ap, Aj = fr.pattern("poisson5pt_33")
    dAp, dAj, dAx = up(Ap, np.int32), up(Aj, np.int32), up(np.ones(len(Aj)), np.float64)
    bh = new_handle()
    try:
        assert bh.initData_device(n, n, n, len(Aj), dAx, dAp, dAj, len(Aj), dAx, dAp, dAj) == 0
        assert bh.spgemm_symbolic() == 0
        run(bh, np.float64, n, Ap, Aj, want=INV, what="a multiply is open")
        assert bh.spgemm_numeric(0, n) == 0 and bh.spgemm_finish() == 0
        check(run(bh, np.float64, n, Ap, Aj, what="after finish"), fr.reference("poisson5pt_33", "none", 0), "after finish")
        bh.free_mem()
    finally:
        bh.freePlatform()


# ---------------------------------------------------------------- the handle's state
def test_a_multiply_before_and_after_matches_the_oracle(hd):
    """A · A with unit values (integer sums: exact in both builds) through the handle, the forest, the same multiply again:
    both results are the oracle's"""
    from oracle import oracle
    bh, dtype = hd
    n, Ap, Aj = fr.pattern("poisson5pt_33")
    ones = np.ones(len(Aj))
    ref = oracle.spgemm(n, n, n, Ap, Aj, ones, Ap, Aj, ones)
    bh.quiet = True
    for leg in ("before", "after"):
        facade._bind(bh, n, n, n, Ap, Aj, ones, Ap, Aj, ones, np.zeros(n + 1, np.int32))
        assert bh.spgemm() == 0
        Cp, Cj, Cx = facade._fetch(bh)
        assert oracle.compare(ref, (Cp, Cj, Cx.astype(np.float64)), rel_tol=1e-6)["ok"] and np.array_equal(Cx.astype(np.float64), ref[2]), leg
        if leg == "before":
            m, mp, mj = fr.pattern("random_directed")
            got = run(bh, dtype, m, mp, mj, fr.weights("random_directed", "asymmetric"), fr.MAXIMUM, what="between two multiplies")
            check(got, fr.reference("random_directed", "asymmetric", fr.MAXIMUM), "between two multiplies", m, bh)
            Cj2, Cx2 = np.empty(len(Cj), np.int32), np.empty(len(Cx), dtype)
            assert bh.get_nnzC() == len(Cj) and bh.get_C(Cj2, Cx2) == 0 and np.array_equal(Cj, Cj2) and np.array_equal(Cx, Cx2)
        assert bh.free_mem() == 0


# ---------------------------------------------------------------- the Python layer
def test_spanning_forest_device_and_csr(hd):
    bh, dtype = hd
    name = "powerlaw3000"
    n, Ap, Aj = fr.pattern(name)
    Ax = fr.weights(name, "asymmetric")
    A = (up(Ap, np.int32), up(Aj, np.int32), up(Ax, dtype))
    for maximum, absolute in ((False, False), (True, True)):
        flags = (fr.MAXIMUM if maximum else 0) | (fr.ABS if absolute else 0)
        lo, hi, w, label = graph.spanning_forest_device(bh, n, A, maximum, absolute)
        klo, khi, kw = fr.kruskal(n, Ap, Aj, Ax, flags)
        assert lo.dtype == torch.int32 and (bh.forest_nedges, bh.forest_rounds) == fr.reference(name, "asymmetric", flags)[4:6]
        assert np.array_equal(lo.cpu().numpy(), klo) and np.array_equal(hi.cpu().numpy(), khi) and fr.bits(w.cpu().numpy()) == fr.bits(kw)
        assert np.array_equal(label.cpu().numpy(), fr.reference(name, "asymmetric", flags)[0])
    Fp, Fj, Fx = (t.cpu().numpy() for t in graph.forest_csr_device(n, lo, hi, w))
    r = np.repeat(np.arange(n), np.diff(Fp))
    assert Fp.dtype == np.int32 and Fp[0] == 0 and Fp[-1] == 2 * len(klo) == len(Fj)
    order = np.lexsort((np.concatenate([khi, klo]), np.concatenate([klo, khi])))
    assert np.array_equal(r, np.concatenate([klo, khi])[order]) and np.array_equal(Fj, np.concatenate([khi, klo])[order])
    assert fr.bits(Fx) == fr.bits(np.concatenate([kw, kw])[order])
    assert fr.same_partition(ccref.components(n, Fp, Fj)[0], ccref.components(n, Ap, Aj)[0])   # the forest spans what A joins
    lo, hi, w, label = graph.spanning_forest_csr(n, Ap, Aj, None, value_dtype=dtype)
    klo, khi, kw = fr.kruskal(n, Ap, Aj, None, 0)
    assert np.array_equal(lo, klo) and np.array_equal(hi, khi) and fr.bits(w) == fr.bits(kw) and w.dtype == dtype
    assert np.array_equal(label, fr.reference(name, "none", 0)[0])


def blobs():
    """three blobs of 40 points with integer coordinates around (0, 0), (1000, 0) and (0, 1000): every point lists its 4
    nearest neighbours and the next point of its blob (one way only), three entries bridge the blobs; weights are squared
    distances, exact in float"""
    rng = np.random.default_rng(12)
    pts = np.concatenate([rng.integers(-30, 31, (40, 2)) + np.array(c) for c in ((0, 0), (1000, 0), (0, 1000))]).astype(np.int64)
    n = len(pts)
    d2 = ((pts[:, None, :] - pts[None, :, :]) ** 2).sum(axis=2)
    src, dst = [], []
    for i in range(n):
        near = [j for j in np.argsort(d2[i], kind="stable").tolist() if j != i][:4]
        if (i + 1) % 40:
            near.append(i + 1)
        src += [i] * len(near)
        dst += near
    src += [5, 45, 85]
    dst += [45, 85, 5]
    Ap, Aj = ccref.from_edges(n, src, dst)
    r = np.repeat(np.arange(n), np.diff(Ap))
    return n, Ap, Aj, d2[r, Aj].astype(np.float64)


def test_single_linkage_on_three_blobs(hd):
    bh, dtype = hd
    n, Ap, Aj, Ax = blobs()
    assert len(np.unique(ccref.components(n, Ap, Aj)[0])) == 1 and Ax.max() < 2 ** 24
    A = (up(Ap, np.int32), up(Aj, np.int32), up(Ax, dtype))
    comp = graph.single_linkage_device(bh, n, A, 3)
    assert comp.dtype == torch.int32 and np.array_equal(comp.cpu().numpy(), np.arange(n) // 40)
    assert np.all(graph.single_linkage_device(bh, n, A, 1).cpu().numpy() == 0)
    assert np.array_equal(graph.single_linkage_device(bh, n, A, n).cpu().numpy(), np.arange(n))
    two = graph.single_linkage_device(bh, n, A, 2).cpu().numpy()
    assert len(np.unique(two)) == 2 and all(len(np.unique(two[b * 40:(b + 1) * 40])) == 1 for b in range(3))
    with pytest.raises(ValueError):
        graph.single_linkage_device(bh, n, A, 0)
    with pytest.raises(ValueError):
        graph.single_linkage_device(bh, n, A, n + 1)
    m, mp, mj = fr.pattern("two_k70")
    with pytest.raises(ValueError):                                  # two components: one cluster cannot be
        graph.single_linkage_device(bh, m, (up(mp, np.int32), up(mj, np.int32), None), 1)
    assert np.array_equal(graph.single_linkage_device(bh, m, (up(mp, np.int32), up(mj, np.int32), None), 2).cpu().numpy(),
                          np.arange(m) // 70)


# ---------------------------------------------------------------- the demo
def test_cpp_demo_runs():
    demo_dir = os.path.join(ROOT, "tests", "forest")
    subprocess.check_call(["make", "-C", demo_dir, "-s"])
    out = subprocess.run([os.path.join(demo_dir, "forest_demo")], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "spanning forest of 1200 vertices" in out.stdout and "PASS" in out.stdout
