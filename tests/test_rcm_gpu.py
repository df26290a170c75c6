"""The reverse Cuthill-McKee ordering (bhs_csr_rcm_device) and what benchmark_spgemm_using_csr_amd/ordering.py and amg.py
build on it, on the GPU, both builds.

Reference: tests/rcmref.py, the contract of include/bhsparse_hip.h ("bandwidth-reducing ordering") restated in numpy, which
tests/test_rcm_abi.py holds against an independent serial queue algorithm.  Everything but the number of passes is a function
of the pattern, so d_perm, d_level, d_start, ncomp, depth AND the sweeps are compared exactly.  Sentinels sit behind every
output; they must be intact, also after a refused call.  The launch counts of every kernel record are checked against the
depth, the sweeps and the passes."""
import functools
import os
import subprocess

import numpy as np
import pytest
import scipy.sparse as sp
import torch

from conftest import ROOT
import aggref as ar
import gridpass as gp
import iluref as ir
import rcmref as R
import scantiles as st

from benchmark_spgemm_using_csr_amd import _lib, amg, ordering
from benchmark_spgemm_using_csr_amd.facade import BHSPARSE_HIP, NUM_PLATFORMS, bhsparse

pytestmark = pytest.mark.gpu

DTYPES = (np.float64, np.float32)
INV = _lib.BHS_ERR_INVALID_ARG
PAD = 64
SENT = -7
BATCH = 8
FAMILIES = {"rcm_check", "rcm_components", "rcm_level", "rcm_far", "rcm_order", "rcm_number", "rcm_group"}
P, NR = R.PERIPHERAL, R.NO_REVERSE
FLAGS = (P, 0, NR, P | NR)
PATTERNS = ("one_with_diag", "one_without_diag", "two_one_edge", "path300", "poisson5pt_33", "poisson9pt_20", "poisson27pt_9",
            "uniform2048", "powerlaw3000", "roadlike40", "star1024", "two_k70", "two_cliques", "no_entries", "shuffled_path",
            "shuffled_grid33", "shuffled_grid20x50", "random3000", "tree")


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


def lanes(n, nnz):
    """side_lanes: the lanes a row gets from the mean row length"""
    mean = nnz / n if n else 0.0
    return 1 if mean <= 4 else 4 if mean <= 16 else 16 if mean <= 64 else 64


@functools.lru_cache(maxsize=None)
def patterns():
    return R.patterns()


def pattern(name):
    return patterns()[name]


@functools.lru_cache(maxsize=None)
def reference(name, flags):
    return R.rcm(*pattern(name), flags)


def run(bh, n, Sp, Sj, flags=P, want=0, what="", nnz=None, levelled=True, started=True, dev=None, alias=False):
    """The device's answer (perm, level, start, ncomp, depth, sweeps, passes) as numpy (level and start None where they are
    not asked for); the sentinels behind the outputs are checked, the launch counts against the depth, the sweeps and the
    passes, and after a refusal that the handle's attributes stayed"""
    dSp, dSj = dev if dev is not None else (up(Sp, np.int32) if len(Sp) else torch.zeros(1, dtype=torch.int32).cuda(),
                                            up(Sj, np.int32) if len(Sj) else None)
    room = max(n, 0)
    perm, level, start = (torch.full((room + PAD,), SENT, dtype=torch.int32).cuda() for _ in range(3))
    torch.cuda.synchronize()
    bh.rcm_ncomp = bh.rcm_depth = bh.rcm_sweeps = bh.rcm_passes = -1
    bh.rcm_ms = -1.0
    err = ordering.rcm_raw_device(bh, n, len(Sj) if nnz is None else nnz, dSp, dSj, flags, perm,
                                  perm if alias else level if levelled else None, start if started else None)
    assert err == want, (what, err)
    torch.cuda.synchronize()
    assert bool((perm[room:] == SENT).all()) and bool((level[room:] == SENT).all()), (what, "written past the end")
    assert bool((start[room:] == SENT).all()), (what, "written past the end of d_start")
    if not levelled:
        assert bool((level == SENT).all()), (what, "d_level was not given")
    if not started:
        assert bool((start == SENT).all()), (what, "d_start was not given")
    if want != 0:
        assert bh.rcm_ncomp == -1 and bh.rcm_depth == -1 and bh.rcm_sweeps == -1 and bh.rcm_passes == -1 and bh.rcm_ms == -1.0, what
        return None
    ncomp, depth, sweeps, passes = bh.rcm_ncomp, bh.rcm_depth, bh.rcm_sweeps, bh.rcm_passes
    assert bh.rcm_ms >= 0.0, what
    if n:
        la = launches(bh)
        assert set(la) == FAMILIES, (what, la)
        assert la["rcm_check"] == 1 and la["rcm_order"] == 3 and la["rcm_group"] == 2, (what, la)
        # the components: the start, the passes, the flags, the scan, the sizes' clearing and the numbering
        pc = la["rcm_components"] - 5
        # a sweep: the levels' start and its passes; the far step's three launches; the starts' two once
        pl = la["rcm_level"] - sweeps
        assert pc >= BATCH and pc % BATCH == 0 and pl % BATCH == 0 and pl >= BATCH * sweeps and pl >= depth, (what, sweeps, depth, la)
        assert passes == pc + pl and passes % BATCH == 0, (what, passes, la)
        assert la["rcm_far"] == 2 + 3 * sweeps, (what, sweeps, la)
        # the numbering: level 0, then the parents, the scan and the places of every further level
        assert la["rcm_number"] == 1 + 3 * (depth - 1), (what, depth, la)
        assert sweeps == 1 or flags & P, (what, sweeps)
        if started:
            assert bool((start[ncomp:] == SENT).all()), (what, "written behind d_start[ncomp]")
    return (perm[:n].cpu().numpy(), level[:n].cpu().numpy() if levelled else None, start[:ncomp].cpu().numpy() if started else None,
            ncomp, depth, sweeps, passes)


def check(got, want, what):
    perm, level, start, ncomp, depth, sweeps, _ = got
    wperm, wlevel, wstart, wncomp, wdepth, wsweeps = want
    assert (ncomp, depth, sweeps) == (wncomp, wdepth, wsweeps), (what, (ncomp, depth, sweeps), (wncomp, wdepth, wsweeps))
    assert level is None or np.array_equal(level, wlevel), (what, "levels", np.flatnonzero(level != wlevel)[:5])
    assert start is None or np.array_equal(start, wstart), (what, "starts")
    assert np.array_equal(perm, wperm), (what, "perm", np.flatnonzero(perm != wperm)[:5])


# ---------------------------------------------------------------- the patterns
def test_empty(hd):
    bh, _ = hd
    got = run(bh, 0, np.zeros(1, np.int32), np.zeros(0, np.int32), what="n = 0")
    assert got[3:] == (0, 0, 0, 0) and len(got[0]) == 0 and bh.rcm_ms == 0.0


def test_the_patterns_qualify_and_cover_the_lanes():
    """every pattern is ascending and symmetric as it is used; lanes 1, 4, 16 and 64 and a hub row above 512 all occur"""
    seen = set()
    for name in PATTERNS:
        n, Sp, Sj = pattern(name)
        assert R.refusal(n, Sp, Sj) is None, name
        seen.add(lanes(n, len(Sj)))
    assert seen == {1, 4, 16, 64}
    of = lambda name: lanes(pattern(name)[0], len(pattern(name)[2]))   # noqa: E731
    assert (of("path300"), of("poisson5pt_33"), of("poisson27pt_9"), of("two_k70")) == (1, 4, 16, 64)
    assert np.diff(pattern("powerlaw3000")[1]).max() > 512            # a hub row beyond every lanes-per-row
    assert set(ar.gpu_cases()) <= set(PATTERNS)


@pytest.mark.parametrize("name", PATTERNS)
def test_against_the_restatement(hd, name):
    """one module-wide handle through all patterns in order, each flag combination"""
    bh, _ = hd
    n, Sp, Sj = pattern(name)
    for flags in FLAGS:
        check(run(bh, n, Sp, Sj, flags, what=(name, flags)), reference(name, flags), (name, flags))
    check(run(bh, n, Sp, Sj, P, what=name, levelled=False), reference(name, P), (name, "without the levels"))
    check(run(bh, n, Sp, Sj, P, what=name, started=False), reference(name, P), (name, "without the starts"))
    check(run(bh, n, Sp, Sj, 0, what=name, levelled=False, started=False), reference(name, 0), (name, "the permutation alone"))
    if name == "no_entries":
        assert reference(name, P)[3:] == (1000, 1, 2) and reference(name, 0)[3:] == (1000, 1, 1)
    if name in ("one_with_diag", "one_without_diag"):
        assert reference(name, P)[0].tolist() == [0] and reference(name, P)[3:] == (1, 1, 2)
    if name == "shuffled_path":
        got = run(bh, n, Sp, Sj, P, what=name)
        assert got[4] == 2000 and got[5] == 2 and R.bandwidth_profile(n, Sp, Sj, got[0]) == (1, 1999)
    if name == "shuffled_grid20x50":
        assert R.bandwidth_profile(n, Sp, Sj, run(bh, n, Sp, Sj, P)[0])[0] == 20 and R.bandwidth_profile(n, Sp, Sj, run(bh, n, Sp, Sj, 0)[0])[0] == 21
    if name == "random3000":
        assert reference(name, P)[3] > 200 and reference(name, P)[5] == 3
    if name == "tree":
        assert n == 20101 and np.bincount(reference(name, P)[1])[:-1].max() > st.SCAN_TILE   # a level's child counts: more than a tile


# ---------------------------------------------------------------- capped grids
@pytest.mark.parametrize("L", (1, 16), ids=("L1", "L16"))
def test_the_block_loops_of_capped_grids(hd, L):
    """disjoint paths of 3 (L = 1) and disjoint cliques of 27 with diagonals (L = 16) at gridpass.cap_rows: more blocks than
    16 workgroups a CU, the last one partial, so that every row kernel takes a second turn of its block loop"""
    bh, _ = hd
    cus = num_cu()
    n = gp.cap_rows(cus, L)
    n, Sp, Sj = st.cached(("rcm capped", n, L), lambda: R.disjoint_paths3(n) if L == 1 else R.disjoint_cliques(n))
    assert lanes(n, len(Sj)) == L and gp.blocks(n, L) > gp.CAP_A * cus and n % (256 // L) != 0, (n, len(Sj), L, cus)
    want = st.cached(("rcm capped answer", n, L), lambda: R.rcm(n, Sp, Sj, P))
    check(run(bh, n, Sp, Sj, P, what=("capped", L)), want, ("capped", L))
    assert want[3] == (n // 3 + n % 3 if L == 1 else n // 27 + n % 27)


# ---------------------------------------------------------------- repeatability
def test_runs_handles_and_libraries_agree():
    n, Sp, Sj = pattern("random3000")
    outs = []
    for dtype in DTYPES:
        bh = new_handle(dtype)
        try:
            outs += [run(bh, n, Sp, Sj) for _ in range(3)]           # the same handle three times
        finally:
            bh.freePlatform()
        bh = new_handle(dtype)                                       # and a fresh one
        try:
            outs.append(run(bh, n, Sp, Sj))
        finally:
            bh.freePlatform()
    for got in outs:
        check(got, reference("random3000", P), "handles")
        assert got[3:6] == outs[0][3:6]
        for a, b in zip(got[:3], outs[0][:3]):
            assert a.tobytes() == b.tobytes()


# ---------------------------------------------------------------- refusals
def test_refusals(hd):
    bh, dtype = hd
    n, Sp, Sj = pattern("poisson5pt_33")
    bad = Sj.copy(); bad[len(bad) // 2] = n                          # noqa: E702
    run(bh, n, Sp, bad, want=INV, what="a column equal to n")
    assert launches(bh) == {"rcm_check": 1}                           # refused by the first kernel: nothing else ran
    bad = Sj.copy(); bad[7] = -1                                     # noqa: E702
    run(bh, n, Sp, bad, want=INV, what="a negative column")
    p = Sp.copy(); p[100] = p[101] + 1                               # noqa: E702
    run(bh, n, p, Sj, want=INV, what="a falling rowPtr")
    run(bh, n, Sp, Sj, want=INV, what="nnzS below rowPtr[n]", nnz=len(Sj) - 3)
    bad = Sj.copy(); q = Sp[200]; bad[q], bad[q + 1] = bad[q + 1], bad[q]   # noqa: E702
    run(bh, n, Sp, bad, want=INV, what="an unsorted row")
    assert R.refusal(n, Sp, bad) == "ascending"
    bad = Sj.copy(); bad[q + 1] = bad[q]                             # noqa: E702
    run(bh, n, Sp, bad, want=INV, what="a repeated entry")
    q = int(np.flatnonzero(Sj[Sp[300]:Sp[301]] != 300)[0]) + Sp[300]
    p, bad = np.where(np.arange(n + 1) > 300, Sp - 1, Sp).astype(np.int32), np.delete(Sj, q)
    assert R.refusal(n, p, bad) == "symmetric"
    run(bh, n, p, bad, want=INV, what="one mirror entry missing")
    assert launches(bh) == {"rcm_check": 1}
    run(bh, n, Sp, Sj, want=INV, what="d_level is d_perm", alias=True)
    run(bh, n, Sp, Sj, 4, want=INV, what="flags = 4")
    run(bh, n, Sp, Sj, -1, want=INV, what="flags = -1")
    run(bh, -1, Sp, Sj, want=INV, what="a negative n")
    dSp, dSj = up(Sp, np.int32), up(Sj, np.int32)
    run(bh, n, Sp, Sj, want=INV, what="a NULL rowPtr", dev=(None, dSj))
    run(bh, n, Sp, Sj, want=INV, what="a NULL colInd", dev=(dSp, None))
    torch.cuda.synchronize()
    bh.rcm_ncomp = -1                                                 # an output inside S: d_perm over the columns; no d_perm
    assert ordering.rcm_raw_device(bh, n, len(Sj), dSp, dSj, 0, dSj[8:], None, None) == INV and bh.rcm_ncomp == -1
    assert ordering.rcm_raw_device(bh, n, len(Sj), dSp, dSj, 0, None, None, None) == INV
    assert np.array_equal(dSj.cpu().numpy(), Sj) and np.array_equal(dSp.cpu().numpy(), Sp)
    check(run(bh, n, Sp, Sj, what="after the refusals"), reference("poisson5pt_33", P), "after the refusals")


def operands(n, Ap, Aj, dtype):
    return up(Ap, np.int32), up(Aj, np.int32), up(np.ones(len(Aj)), dtype)


def test_refused_between_symbolic_and_finish():
    n, Ap, Aj = pattern("poisson5pt_33")
    dAp, dAj, dAx = operands(n, Ap, Aj, np.float64)
    bh = new_handle()
    try:
        assert bh.initData_device(n, n, n, len(Aj), dAx, dAp, dAj, len(Aj), dAx, dAp, dAj) == 0
        assert bh.spgemm_symbolic() == 0
        run(bh, n, Ap, Aj, want=INV, what="a multiply is open")
        assert bh.spgemm_numeric(0, n) == 0 and bh.spgemm_finish() == 0
        check(run(bh, n, Ap, Aj, what="after finish"), reference("poisson5pt_33", P), "after finish")
        bh.free_mem()
    finally:
        bh.freePlatform()


# ---------------------------------------------------------------- the handle's state
def test_a_multiply_stays_as_it_was(hd):
    bh, dtype = hd
    n, Ap, Aj = pattern("poisson5pt_33")
    dAp, dAj, dAx = operands(n, Ap, Aj, dtype)
    assert bh.initData_device(n, n, n, len(Aj), dAx, dAp, dAj, len(Aj), dAx, dAp, dAj) == 0
    bh.quiet = True
    assert bh.spgemm() == 0
    nnzC = bh.get_nnzC()
    Cj, Cx = np.empty(nnzC, np.int32), np.empty(nnzC, dtype)
    assert nnzC > len(Aj) and bh.get_C(Cj, Cx) == 0
    m, mp, mj = pattern("random3000")
    check(run(bh, m, mp, mj, what="after a multiply"), reference("random3000", P), "after a multiply")
    Cj2, Cx2 = np.empty(nnzC, np.int32), np.empty(nnzC, dtype)
    assert bh.get_nnzC() == nnzC and bh.get_C(Cj2, Cx2) == 0
    assert np.array_equal(Cj, Cj2) and np.array_equal(Cx, Cx2)
    assert bh.free_mem() == 0


# ---------------------------------------------------------------- the Python layer
def valued(name, dtype, seed=5):
    """(n, Ap, Aj, Ax, scipy matrix): the pattern with seeded integer values"""
    n, Ap, Aj = pattern(name)
    Ax = np.random.default_rng(seed).integers(1, 9, len(Aj)).astype(dtype)
    return n, Ap, Aj, Ax, sp.csr_matrix((Ax, Aj, Ap), shape=(n, n))


def test_bandwidth_profile_and_permute_match_scipy(hd):
    bh, dtype = hd
    for name in ("shuffled_grid33", "random3000", "powerlaw3000", "no_entries"):
        n, Ap, Aj, Ax, A = valued(name, dtype)
        dA = (up(Ap, np.int32), up(Aj, np.int32), up(Ax, dtype))
        perm = ordering.rcm_device(bh, n, dA)
        want = reference(name, P)[0]
        assert perm.dtype == torch.int32 and np.array_equal(perm.cpu().numpy(), want), name
        assert np.array_equal(ordering.rcm_device(bh, n, dA, peripheral=False, reverse=False).cpu().numpy(), reference(name, NR)[0]), name
        for p in (None, want):
            B = (A if p is None else A[p][:, p]).tocoo()
            first = np.arange(n)
            np.minimum.at(first, B.row, B.col)
            scipy_answer = (int(np.abs(B.row - B.col).max()) if B.nnz else 0, int((np.arange(n) - first).sum()))
            got = ordering.bandwidth_profile_device(n, dA, None if p is None else up(p, np.int32))
            assert got == scipy_answer == R.bandwidth_profile(n, Ap, Aj, p), (name, got, scipy_answer)
        if not len(Aj):
            continue
        Zp, Zj, Zx = ordering.permute_device(bh, n, dA, perm)
        Z = sp.csr_matrix((Zx.cpu().numpy(), Zj.cpu().numpy(), Zp.cpu().numpy()), shape=(n, n))
        assert (Z != A[want][:, want]).nnz == 0 and Z.nnz == A.nnz and Z.has_sorted_indices, name
        Sp, Sj = ordering.symmetric_pattern_device(bh, n, dA)
        assert np.array_equal(Sp.cpu().numpy(), Ap) and np.array_equal(Sj.cpu().numpy(), Aj), name   # symmetric already


def test_rcm_csr():
    n, Ap, Aj, Ax, A = valued("shuffled_grid33", np.float64)
    perm, (Zp, Zj, Zx), info = ordering.rcm_csr(n, Ap, Aj, Ax)
    want = reference("shuffled_grid33", P)
    assert np.array_equal(perm, want[0]) and (info["ncomp"], info["depth"], info["sweeps"]) == want[3:]
    assert info["bandwidth"] == (R.bandwidth_profile(n, Ap, Aj)[0], 33) and info["profile"][1] < info["profile"][0]
    assert (sp.csr_matrix((Zx, Zj, Zp), shape=(n, n)) != A[perm][:, perm]).nnz == 0


def spd_cases():
    """name -> (n, Ap, Aj, Ax): poisson27pt 9^3, and the Laplacian (4 on the diagonal, -1 off it) on the shuffled 33 x 33 grid"""
    n, Sp, Sj = pattern("shuffled_grid33")
    r = np.repeat(np.arange(n), np.diff(Sp))
    return {"poisson27pt_9": ar.poisson("poisson27pt", 9, 9, 9), "shuffled_grid33": (n, Sp, Sj, np.where(r == Sj, 4.0, -1.0))}


@pytest.mark.parametrize("name", ("poisson27pt_9", "shuffled_grid33"))
def test_ilu0_pcg_in_rcm_order(name):
    """double: to 1e-8, the iterations within 1 of iluref.ilu0_pcg in natural order on the system permuted on the host with
    the restated permutation (the margin of tests/test_trsv_gpu.py)"""
    n, Ap, Aj, Ax = spd_cases()[name]
    A = sp.csr_matrix((Ax, Aj, Ap), shape=(n, n))
    b = np.random.default_rng(17).standard_normal(n)
    perm = R.rcm(n, Ap, Aj, P)[0]
    _, want_its, want_res = ir.ilu0_pcg(A[perm][:, perm].tocsr(), b[perm], 1e-8, 200, "natural")
    bh = new_handle(np.float64)
    try:
        dA = (up(Ap, np.int32), up(Aj, np.int32), up(Ax, np.float64))
        x, its, res = amg.ilu0_pcg_rcm_device(bh, dA, up(b, np.float64), 1e-8, 200)
        x = x.cpu().numpy()
        print("%s: %d iterations on the device, %d on the host; residual %.3e" % (name, its, want_its, res[-1] / res[0]))
        assert res[-1] <= 1e-8 * res[0] and want_res[-1] <= 1e-8 * want_res[0] and want_its < 200
        assert np.linalg.norm(b - A @ x) <= 1e-7 * np.linalg.norm(b)
        assert abs(its - want_its) <= 1, (its, want_its)
        M = amg.ilu0_setup_permuted_device(bh, dA, up(perm, np.int32))
        assert sorted(M) == ["LU", "lower", "ncolors", "perm", "pivot", "upper"] and M["perm"].dtype == torch.int64
        assert M["ncolors"] == 0 and M["pivot"] == -1 and np.array_equal(M["perm"].cpu().numpy(), perm)
        with pytest.raises(ValueError):
            amg.ilu0_setup_device(bh, dA, ordering="rcm")             # as it was
    finally:
        bh.freePlatform()


# ---------------------------------------------------------------- the demo
def test_cpp_demo_runs():
    demo_dir = os.path.join(ROOT, "tests", "rcm")
    subprocess.check_call(["make", "-C", demo_dir, "-s"])
    out = subprocess.run([os.path.join(demo_dir, "rcm_demo")], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "reverse Cuthill-McKee of 2317 vertices" in out.stdout and "bandwidths 40 and 1 PASS" in out.stdout
