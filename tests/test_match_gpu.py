"""The heavy-edge matching (bhs_csr_match_device) and what benchmark_spgemm_using_csr_amd/amg.py builds on it -- the pairwise
aggregation, its hierarchy, the preconditioned solve -- on the GPU, both builds.

Reference: tests/matchref.py, the contract of include/bhsparse_hip.h ("matching") restated in numpy.  The result is a function
of the input, the number of productive rounds included, so d_mate, d_agg, npairs and rounds are compared exactly.  Sentinels
sit behind every output; they must be intact, also after a refused call, and a refusal by the host leaves the outputs
themselves untouched.

The numbering scans ONE COUNT PER 64 VERTICES (the leaders among them) with the library's one-pass scan over tiles of
scantiles.SCAN_TILE counts: the bands of scantiles.AGG_CASES put ceil(n / 64) above a tile, at none, at one count, at exactly
a tile, at several tiles and a remainder and just under a tile, and one handle goes through them in that order."""
import functools
import os
import subprocess

import numpy as np
import pytest
import scipy.sparse as sp
from scipy.sparse.csgraph import connected_components
import torch

from conftest import ROOT
import aggref as ar
import ccref
import matchref as mr
import scantiles as st

from benchmark_spgemm_using_csr_amd import _lib, amg
from benchmark_spgemm_using_csr_amd.facade import BHSPARSE_HIP, NUM_PLATFORMS, bhsparse

pytestmark = pytest.mark.gpu

DTYPES = (np.float64, np.float32)
INV = _lib.BHS_ERR_INVALID_ARG
PAD = 64
SENT = -7
PATTERNS = tuple(ar.gpu_cases()) + ("star_centre_last",)
LANES = {"path300": 1, "poisson5pt_33": 4, "poisson27pt_9": 16, "two_k70": 64, "star_centre_last": 64}
GRIDS = ("poisson5pt_33", "poisson27pt_9", "aniso64")               # the pairwise aggregation's inputs
SOLVES = ("poisson5pt_64", "aniso64", "poisson27pt_16")             # the hierarchy's


def new_handle(dtype=np.float64):
    plats = [False] * NUM_PLATFORMS
    plats[BHSPARSE_HIP] = True
    bh = bhsparse(value_dtype=dtype)
    assert bh.initPlatform(plats) == 0
    return bh


@pytest.fixture(scope="module", params=DTYPES, ids=("f64", "f32"))
def hd(request):
    """(h1, h2, value type): the module's handles; the matching runs on the first, the Galerkin products use both"""
    h1, h2 = new_handle(request.param), new_handle(request.param)
    yield h1, h2, request.param
    h2.freePlatform()
    h1.freePlatform()


def up(a, dt):
    return torch.from_numpy(np.ascontiguousarray(a, dt).copy()).cuda()


def launches(bh):
    return {s["name"]: s["launches"] for s in bh.kernel_stats() if s["launches"] > 0}


@functools.lru_cache(maxsize=None)
def pattern(name):
    return ccref.star_centre_last() if name == "star_centre_last" else ar.gpu_cases()[name]


@functools.lru_cache(maxsize=None)
def weights(name):
    return mr.integer_weights(*pattern(name))


@functools.lru_cache(maxsize=None)
def reference(name, weighted, seed):
    n, Ap, Aj = pattern(name)
    return mr.match(n, Ap, Aj, weights(name) if weighted else None, seed)


def run(bh, dtype, n, Ap, Aj, Ax=None, seed=0, want=0, what="", nnz=None, numbered=True, flags=0, dev=None, alias=False,
        by_host=True):
    """The device's answer (mate, agg, npairs, rounds) as numpy (agg None where it is not asked for); the sentinels behind the
    outputs are checked, and after a refusal that the handle's attributes stayed -- and, where the host refuses, the outputs"""
    if dev is None:
        dev = (up(Ap, np.int32) if len(Ap) else torch.zeros(1, dtype=torch.int32).cuda(), up(Aj, np.int32) if len(Aj) else None,
               up(Ax, dtype) if Ax is not None and len(Aj) else None)
    dAp, dAj, dAx = dev
    room = max(n, 0)
    mate, agg = (torch.full((room + PAD,), SENT, dtype=torch.int32).cuda() for _ in range(2))
    torch.cuda.synchronize()
    bh.match_npairs = bh.match_rounds = -1
    bh.match_ms = -1.0
    err = amg.match_raw_device(bh, n, len(Aj) if nnz is None else nnz, dAp, dAj, dAx, seed, flags, mate,
                               mate if alias else agg if numbered else None)
    assert err == want, (what, err)
    assert bool((mate[room:] == SENT).all()) and bool((agg[room:] == SENT).all()), (what, "written past the end")
    if not numbered:
        assert bool((agg == SENT).all()), (what, "d_agg was not given")
    if want != 0:
        assert bh.match_npairs == -1 and bh.match_rounds == -1 and bh.match_ms == -1.0, what
        if by_host:
            assert bool((mate == SENT).all()) and bool((agg == SENT).all()), (what, "an output was touched")
        return None
    assert bh.match_ms >= 0.0, what
    if n:
        assert set(launches(bh)) == {"match_init", "match_round"} | ({"match_number"} if numbered else set()), (what, launches(bh))
        assert launches(bh)["match_init"] == 1 and launches(bh)["match_round"] >= 2 * max(bh.match_rounds, 1), (what, launches(bh))
    else:
        assert bh.match_ms == 0.0
    return mate[:n].cpu().numpy(), agg[:n].cpu().numpy() if numbered else None, bh.match_npairs, bh.match_rounds


def check(got, want, what):
    mate, agg, npairs, nrounds = got
    wmate, wagg, wnagg, wnpairs, wrounds = want
    assert (npairs, nrounds) == (wnpairs, wrounds), (what, npairs, nrounds, wnpairs, wrounds)
    assert np.array_equal(mate, wmate), (what, "mates", np.flatnonzero(mate != wmate)[:5])
    assert agg is None or np.array_equal(agg, wagg), (what, "numbers", np.flatnonzero(agg != wagg)[:5])


# ---------------------------------------------------------------- the patterns
def test_empty(hd):
    bh, _, dtype = hd
    got = run(bh, dtype, 0, np.zeros(1, np.int32), np.zeros(0, np.int32), what="n = 0")
    assert got[2] == 0 and got[3] == 0 and len(got[0]) == 0 and bh.match_ms == 0.0
    assert mr.match(0, np.zeros(1, np.int32), np.zeros(0, np.int32))[2:] == (0, 0, 0)


@pytest.mark.parametrize("name", PATTERNS)
def test_against_the_restatement(hd, name):
    bh, _, dtype = hd
    n, Ap, Aj = pattern(name)
    if name in LANES:                                                # the lanes a row of bhs_host_aggregate.inc.h's ag_lanes
        mean = len(Aj) / n
        assert (1 if mean <= 4 else 4 if mean <= 16 else 16 if mean <= 64 else 64) == LANES[name], (name, mean)
    dev = (up(Ap, np.int32), up(Aj, np.int32) if len(Aj) else None)
    dAx = up(weights(name), dtype) if len(Aj) else None
    for weighted in (False, True):
        for seed in (0, 1):
            for numbered in (True, False):
                what = (name, weighted, seed, numbered)
                got = run(bh, dtype, n, Ap, Aj, seed=seed, what=what, numbered=numbered, dev=dev + (dAx if weighted else None,))
                check(got, reference(name, weighted, seed), what)
    if name == "powerlaw3000":
        assert np.diff(Ap).max() > 512                               # a hub row beyond every lanes-per-row
    if name == "uniform2048":
        assert not np.array_equal(reference(name, True, 0)[0], reference(name, False, 0)[0])   # the weights count
        assert not np.array_equal(reference(name, False, 0)[0], reference(name, False, 1)[0])  # and the seed


def test_the_increasing_path_takes_n_over_2_rounds(hd):
    bh, _, dtype = hd
    n, Ap, Aj, Ax = mr.increasing_path(200)
    got = run(bh, dtype, n, Ap, Aj, Ax, what="increasing path")
    check(got, mr.match(n, Ap, Aj, Ax, 0), "increasing path")
    assert got[2:] == (100, 100) and np.array_equal(got[0], np.arange(200) ^ 1)
    assert launches(bh)["match_round"] == 200                        # the hundredth round leaves nobody: no empty round


def test_special_values_by_hand(hd):
    bh, _, dtype = hd
    n, Ap, Aj, Ax = mr.by_hand()
    for seed in (0, 1):
        got = run(bh, dtype, n, Ap, Aj, Ax, seed=seed, what="by hand")
        assert got[0].tolist() == [3, 2, 1, 0] and got[1].tolist() == [0, 1, 1, 0] and got[2:] == (2, 1)
    n, Ap, Aj, _ = mr.directed_triangle()
    got = run(bh, dtype, n, Ap, Aj, what="directed triangle")
    assert got[0].tolist() == [0, 1, 2] and got[1].tolist() == [0, 1, 2] and got[2:] == (0, 0)
    assert launches(bh)["match_round"] == 3                          # one round that matched nothing, and its closing


def test_asymmetric_weights_and_unsorted_rows(hd):
    bh, _, dtype = hd
    n, Ap, Aj = pattern("poisson5pt_33")
    Ax = mr.asymmetric_weights(n, Ap, Aj)
    got = run(bh, dtype, n, Ap, Aj, Ax, what="asymmetric weights")
    check(got, mr.match(n, Ap, Aj, Ax, 0), "asymmetric weights")
    assert mr.is_matching(got[0])
    Ax = weights("poisson5pt_33")
    m2, Bp, Bj, Bx = mr.unsorted_with_repeats(n, Ap, Aj, Ax)
    got = run(bh, dtype, m2, Bp, Bj, Bx, seed=1, what="unsorted rows with repeats")
    check(got, mr.match(m2, Bp, Bj, Bx, 1), "unsorted rows with repeats")
    check(got, reference("poisson5pt_33", True, 1), "the same matrix, stored once")


def test_one_handle_through_the_scan_sizes(hd):
    """the numbering's scan over ceil(n / 64) counts: above a tile, none, one count, exactly a tile, several tiles and a
    remainder, just under a tile, then the band of half-width 3 (four lanes a row), in that order on one handle"""
    bh, _, dtype = hd
    assert tuple(st.role_of(st.words(st.agg_n(s))) for s in range(len(st.COUNTS))) == st.ROLES
    assert [st.agg_n(s) for s in range(6)] == [524349, 0, 61, 524288, 1573181, 524221]
    for step, w in st.AGG_CASES:
        n, Sp, Sj = st.band(st.agg_n(step), w)
        want = st.cached(("match", step, w), lambda: mr.match(n, Sp, Sj, None, 0), "matching")
        got = run(bh, dtype, n, Sp, Sj, what=(step, w))
        check(got, want, (step, w))
        if n:
            rows = {s["name"]: s["rows"] for s in bh.kernel_stats()}["match_number"]
            assert rows == n + st.words(n), (step, w, rows)
            assert got[3] <= 7, (step, w, got[3])


# ---------------------------------------------------------------- repeatability
def test_runs_handles_and_libraries_agree():
    n, Ap, Aj = pattern("uniform2048")
    Ax = weights("uniform2048")
    outs = []
    for dtype in DTYPES:
        bh = new_handle(dtype)
        try:
            outs += [run(bh, dtype, n, Ap, Aj, Ax) for _ in range(3)]   # the same handle three times
        finally:
            bh.freePlatform()
        bh = new_handle(dtype)                                       # and a fresh one
        try:
            outs.append(run(bh, dtype, n, Ap, Aj, Ax))
            outs.append(run(bh, dtype, n, Ap, Aj, None))
        finally:
            bh.freePlatform()
    for got in outs:
        weighted = got is not outs[4] and got is not outs[9]
        check(got, reference("uniform2048", weighted, 0), "handles")
        first = outs[0] if weighted else outs[4]
        assert got[0].tobytes() == first[0].tobytes() and got[1].tobytes() == first[1].tobytes()


# ---------------------------------------------------------------- refusals
def test_refusals(hd):
    bh, _, dtype = hd
    n, Ap, Aj = pattern("poisson5pt_33")
    Ax = weights("poisson5pt_33")
    bad = Aj.copy(); bad[len(bad) // 2] = n                          # noqa: E702
    run(bh, dtype, n, Ap, bad, Ax, want=INV, what="a column equal to n", by_host=False)
    bad = Aj.copy(); bad[7] = -1                                     # noqa: E702
    run(bh, dtype, n, Ap, bad, Ax, want=INV, what="a negative column", by_host=False)
    p = Ap.copy(); p[100] = p[101] + 1                               # noqa: E702
    run(bh, dtype, n, p, Aj, Ax, want=INV, what="a decreasing rowPtr", by_host=False)
    run(bh, dtype, n, Ap, Aj, Ax, want=INV, what="nnzA below rowPtr[n]", nnz=len(Aj) - 3, by_host=False)
    run(bh, dtype, n, Ap, Aj, Ax, want=INV, what="d_agg is d_mate", alias=True)
    run(bh, dtype, n, Ap, Aj, Ax, want=INV, what="flags = 1", flags=1)
    run(bh, dtype, -1, Ap, Aj, Ax, want=INV, what="a negative n")
    run(bh, dtype, n, Ap, Aj, Ax, want=INV, what="a negative nnzA", nnz=-1)
    dAp, dAj, dAx = up(Ap, np.int32), up(Aj, np.int32), up(Ax, dtype)
    run(bh, dtype, n, Ap, Aj, want=INV, what="a NULL rowPtr", dev=(None, dAj, dAx))
    run(bh, dtype, n, Ap, Aj, want=INV, what="a NULL colInd", dev=(dAp, None, dAx))
    # outputs inside A: d_mate over the columns, d_agg over the values; no d_mate at all
    torch.cuda.synchronize()
    bh.match_npairs = -1
    spare = torch.full((n + PAD,), SENT, dtype=torch.int32).cuda()
    assert amg.match_raw_device(bh, n, len(Aj), dAp, dAj, dAx, 0, 0, dAj[8:], None) == INV and bh.match_npairs == -1
    assert amg.match_raw_device(bh, n, len(Aj), dAp, dAj, dAx, 0, 0, spare, dAx[4:]) == INV and bh.match_npairs == -1
    assert amg.match_raw_device(bh, n, len(Aj), dAp, dAj, dAx, 0, 0, None, spare) == INV and bh.match_npairs == -1
    assert amg.match_raw_device(bhsparse(value_dtype=dtype), n, len(Aj), dAp, dAj, dAx, 0, 0, spare, None) == _lib.BHS_ERR_NOT_READY
    assert np.array_equal(dAj.cpu().numpy(), Aj) and np.array_equal(dAp.cpu().numpy(), Ap) and bool((spare == SENT).all())
    assert np.array_equal(dAx.cpu().numpy(), Ax.astype(dtype))
    check(run(bh, dtype, n, Ap, Aj, Ax, what="after the refusals"), reference("poisson5pt_33", True, 0), "after the refusals")


def test_refused_between_symbolic_and_finish():
    n, Ap, Aj = pattern("poisson5pt_33")
    dAp, dAj, dAx = up(Ap, np.int32), up(Aj, np.int32), up(np.ones(len(Aj)), np.float64)
    bh = new_handle()
    try:
        assert bh.initData_device(n, n, n, len(Aj), dAx, dAp, dAj, len(Aj), dAx, dAp, dAj) == 0
        assert bh.spgemm_symbolic() == 0
        run(bh, np.float64, n, Ap, Aj, want=INV, what="a multiply is open")
        assert bh.spgemm_numeric(0, n) == 0 and bh.spgemm_finish() == 0
        check(run(bh, np.float64, n, Ap, Aj, what="after finish"), reference("poisson5pt_33", False, 0), "after finish")
        bh.free_mem()
    finally:
        bh.freePlatform()


# ---------------------------------------------------------------- pairwise aggregation
@functools.lru_cache(maxsize=None)
def matrix(name):
    """scipy CSR, rows ascending; integers, or dyadic numbers for "aniso64_dyadic": every Galerkin sum is exact in both builds"""
    if name == "aniso64":
        return mr.aniso(64, 64, 1e-2)
    if name == "aniso64_dyadic":
        return mr.aniso(64, 64, 1.0 / 64)
    kind, size = name.split("_")
    n, Ap, Aj, Ax = ar.poisson(kind, *([int(size)] * (3 if kind == "poisson27pt" else 2)))
    return sp.csr_matrix((Ax, Aj, Ap), shape=(n, n))


def device_matrix(A, dtype):
    return up(A.indptr, np.int32), up(A.indices, np.int32), up(A.data, dtype)


@functools.lru_cache(maxsize=None)
def pairwise_reference(name, passes):
    return mr.pairwise(matrix(name), passes, 0)


def check_aggregates(A, agg, nagg, passes, what):
    """sizes <= 2^passes, numbered by ascending smallest member, every aggregate connected in A's graph"""
    n = A.shape[0]
    sizes = np.bincount(agg, minlength=nagg)
    assert len(agg) == n and agg.min() >= 0 and agg.max() == nagg - 1 and sizes.min() >= 1 and sizes.max() <= 2 ** passes, what
    assert mr.numbered_by_smallest_member(agg, nagg), what
    r, c, _ = mr.seen_edges(n, A.indptr, A.indices, A.data)
    same = agg[r] == agg[c]
    inside = sp.csr_matrix((np.ones(int(same.sum())), (r[same], c[same])), shape=(n, n))
    assert connected_components(inside, directed=False)[0] == nagg, (what, "an aggregate is not connected")


@pytest.mark.parametrize("name", GRIDS)
def test_pairwise_aggregation(hd, name):
    h1, h2, dtype = hd
    A = matrix("aniso64_dyadic" if name == "aniso64" else name)
    n = A.shape[0]
    dA = device_matrix(A, dtype)
    for passes in (1, 2, 3):
        agg, nagg, info = amg.pairwise_aggregate_device((h1, h2), n, dA, passes, 0)
        wagg, wnagg = pairwise_reference("aniso64_dyadic" if name == "aniso64" else name, passes)
        assert agg.dtype == torch.int32 and nagg == wnagg and np.array_equal(agg.cpu().numpy(), wagg), (name, passes)
        check_aggregates(A, wagg, wnagg, passes, (name, passes))
        assert len(info) == passes and info[0]["n"] == n and all(r["npairs"] > 0 and r["rounds"] >= 1 for r in info)
        assert nagg == n - sum(r["npairs"] for r in info)
    for passes in (0, 5):
        with pytest.raises(ValueError):
            amg.pairwise_aggregate_device((h1, h2), n, dA, passes, 0)
        with pytest.raises(ValueError):
            amg.pa_setup_device((h1, h2), n, dA, passes)


def test_match_device_and_csr(hd):
    bh, _, dtype = hd
    n, Ap, Aj = pattern("poisson27pt_9")
    Ax = weights("poisson27pt_9")
    mate, agg, nagg, npairs = amg.match_device(bh, n, (up(Ap, np.int32), up(Aj, np.int32), up(Ax, dtype)), 1)
    want = reference("poisson27pt_9", True, 1)
    assert (nagg, npairs) == (want[2], want[3]) and np.array_equal(mate.cpu().numpy(), want[0]) and np.array_equal(agg.cpu().numpy(), want[1])
    mate, agg, nagg, npairs = amg.match_csr(n, Ap, Aj, None, seed=0, value_dtype=dtype)
    want = reference("poisson27pt_9", False, 0)
    assert (nagg, npairs) == (want[2], want[3]) and np.array_equal(mate, want[0]) and np.array_equal(agg, want[1])


# ---------------------------------------------------------------- the hierarchy and the solve
def true_residual(A, x, b):
    return float(np.linalg.norm(b - A @ x.cpu().numpy().astype(np.float64)) / np.linalg.norm(b))


@pytest.mark.parametrize("name", SOLVES)
def test_hierarchy_and_pcg(hd, name):
    """pa_setup_device(passes = 2): every level's aggregates are what pairwise_aggregate_device gives on that level's matrix
    with the level's seed (checked structurally; the first level's against the restatement, exactly, in the double build --
    deeper levels hold sums that scipy may round in another order).  Double build: CG preconditioned with the Jacobi V-cycle
    reaches 1e-8 in no more iterations on the pairwise hierarchy than on sa_setup_device's MIS(2) hierarchy in this same
    test (CPU prototype: 12 against 22, 33 against 70, 8 against 15), and the true residual, in float64 on the host, is
    within 10 x of the MIS(2) solve's: both stop at the same tolerance, the factor covers the last step's overshoot.  The
    Gauss-Seidel counts are printed, not asserted."""
    h1, h2, dtype = hd
    A = matrix(name)
    n = A.shape[0]
    dA = device_matrix(A, dtype)
    levels, info = amg.pa_setup_device((h1, h2), n, dA, passes=2)
    assert len(levels) == len(info) >= 3 and levels[-1][1] is None and levels[-1][2] is None and set(info[-1]) == {"n", "nnz"}
    assert info[-1]["n"] <= 40 and info[0]["n"] == n
    for lvl, (Al, P, R) in enumerate(levels[:-1]):
        rows = info[lvl]["n"]
        assert set(info[lvl]) == {"n", "nnz", "nagg", "passes", "aggregate_ms", "prolongator_ms", "galerkin_ms"}
        assert info[lvl]["nagg"] == info[lvl + 1]["n"] and int(Al[0].numel()) == rows + 1
        assert int(P[0].numel()) == rows + 1 and int(R[0].numel()) == info[lvl]["nagg"] + 1
        agg, nagg, _ = amg.pairwise_aggregate_device((h1, h2), rows, Al, 2, 8 * lvl)
        assert nagg == info[lvl]["nagg"], (name, lvl)
        Ah = sp.csr_matrix((Al[2].cpu().numpy().astype(np.float64), Al[1].cpu().numpy(), Al[0].cpu().numpy()), shape=(rows, rows))
        check_aggregates(Ah, agg.cpu().numpy(), nagg, 2, (name, lvl))
        if lvl == 0 and dtype == np.float64:
            wagg, wnagg = mr.pairwise(A, 2, 0)
            assert nagg == wnagg and np.array_equal(agg.cpu().numpy(), wagg), name
    sizes = [r["n"] for r in info]
    complexity = sum(r["nnz"] for r in info) / info[0]["nnz"]
    print("%s %s: pairwise(2) levels %s, operator complexity %.2f" % (name, np.dtype(dtype).name, sizes, complexity))
    if dtype != np.float64:
        return
    b = torch.from_numpy(np.random.default_rng(4).standard_normal(n)).cuda()
    sa_levels, sa_info = amg.sa_setup_device((h1, h2), n, dA)
    its = {}
    for smoother in ("jacobi", "gs"):
        x, its["pa", smoother], res = amg.pcg_device(h1, levels, b, 1e-8, 200, smoother)
        xs, its["sa", smoother], res_sa = amg.pcg_device(h1, sa_levels, b, 1e-8, 200, smoother)
        assert res[-1] <= 1e-8 * res[0] and res_sa[-1] <= 1e-8 * res_sa[0], (name, smoother, its)
        rel, rel_sa = true_residual(A, x, b.cpu().numpy()), true_residual(A, xs, b.cpu().numpy())
        print("%s %s: pairwise %d iterations (true residual %.2e), MIS(2) %s %d iterations (%.2e)"
              % (name, smoother, its["pa", smoother], rel, [r["n"] for r in sa_info], its["sa", smoother], rel_sa))
        if smoother == "jacobi":
            assert its["pa", "jacobi"] <= its["sa", "jacobi"], (name, its)
            assert rel <= 10.0 * rel_sa, (name, rel, rel_sa)


# ---------------------------------------------------------------- the demo
def test_cpp_demo_runs():
    demo_dir = os.path.join(ROOT, "tests", "match")
    subprocess.check_call(["make", "-C", demo_dir, "-s"])
    out = subprocess.run([os.path.join(demo_dir, "match_demo")], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "matching of 1200 vertices" in out.stdout and "PASS" in out.stdout
