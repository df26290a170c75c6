"""The k-core decomposition (bhs_csr_kcore_device) and what benchmark_spgemm_using_csr_amd/graph.py builds on it -- the
degeneracy ordering, the k-core as a submatrix, the k-truss -- on the GPU, both builds.

Reference: tests/coreref.py, the definition of include/bhsparse_hip.h ("k-core decomposition") restated in numpy, which
tests/test_kcore_abi.py holds against networkx and an independent bucket peel.  core, round, kmax and rounds are functions of
the pattern, so all four are compared exactly.  Sentinels sit behind every output and, after a refused call, in it; they must
be intact.  The launch counts of the kernel records are checked against the rounds: 8 passes a control round trip, so the
peel's launches are the rounds rounded up to a multiple of 8, and the trips are that over 8 plus the close."""
import os
import subprocess

import numpy as np
import pytest
import torch

from conftest import ROOT
import coreref as R
import gridpass as gp
import scantiles as st

from benchmark_spgemm_using_csr_amd import _lib, graph
from benchmark_spgemm_using_csr_amd.facade import BHSPARSE_HIP, NUM_PLATFORMS, bhsparse

pytestmark = pytest.mark.gpu

DTYPES = (np.float64, np.float32)
INV = _lib.BHS_ERR_INVALID_ARG
PAD = 64
SENT = -7
BATCH = 8
FAMILIES = {"kcore_check", "kcore_peel", "kcore_advance"}


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


def run(bh, n, Sp, Sj, flags=0, want=0, what="", nnz=None, rounded=True, dev=None, alias=False):
    """The device's answer (core, round, kmax, rounds) as numpy (round None where it is not asked for); the sentinels behind
    the outputs are checked, the launch counts against the rounds, and after a refusal that the outputs and the handle's
    attributes stayed"""
    dSp, dSj = dev if dev is not None else (up(Sp, np.int32) if len(Sp) else torch.zeros(1, dtype=torch.int32).cuda(),
                                            up(Sj, np.int32) if len(Sj) else None)
    room = max(n, 0)
    core, rnd = (torch.full((room + PAD,), SENT, dtype=torch.int32).cuda() for _ in range(2))
    torch.cuda.synchronize()
    bh.kcore_kmax = bh.kcore_rounds = -1
    bh.kcore_ms = -1.0
    err = graph.kcore_raw_device(bh, n, len(Sj) if nnz is None else nnz, dSp, dSj, flags, core, core if alias else rnd if rounded else None)
    assert err == want, (what, err)
    torch.cuda.synchronize()
    assert bool((core[room:] == SENT).all()) and bool((rnd[room:] == SENT).all()), (what, "written past the end")
    if not rounded:
        assert bool((rnd == SENT).all()), (what, "d_round was not given")
    if want != 0:
        assert bool((core == SENT).all()) and bool((rnd == SENT).all()), (what, "a refused call wrote an output")
        assert bh.kcore_kmax == -1 and bh.kcore_rounds == -1 and bh.kcore_ms == -1.0, what
        return None
    kmax, rounds = bh.kcore_kmax, bh.kcore_rounds
    assert bh.kcore_ms >= 0.0, what
    if n:
        la = launches(bh)
        passes = BATCH * -(-rounds // BATCH)                          # ceil(rounds / 8) control round trips, and the close
        assert set(la) == FAMILIES, (what, la)
        assert la["kcore_check"] == 1 and la["kcore_peel"] == passes and la["kcore_advance"] == 1 + 3 * passes, (what, rounds, la)
    return core[:n].cpu().numpy(), rnd[:n].cpu().numpy() if rounded else None, kmax, rounds


def check(got, want, what):
    core, rnd, kmax, rounds = got
    wcore, wrnd, wkmax, wrounds = want
    print("%s: kmax %d (reference %d), rounds %d (reference %d)" % (what, kmax, wkmax, rounds, wrounds))
    assert (kmax, rounds) == (wkmax, wrounds), (what, (kmax, rounds), (wkmax, wrounds))
    assert np.array_equal(core, wcore), (what, "core", np.flatnonzero(core != wcore)[:5])
    assert rnd is None or np.array_equal(rnd, wrnd), (what, "round", np.flatnonzero(rnd != wrnd)[:5])


# ---------------------------------------------------------------- exact equality
def test_empty(hd):
    bh, _ = hd
    got = run(bh, 0, np.zeros(1, np.int32), np.zeros(0, np.int32), what="n = 0")
    assert got[2:] == (0, 0) and len(got[0]) == 0 and bh.kcore_ms == 0.0


@pytest.mark.parametrize("name", R.CASES)
def test_against_the_restatement(hd, name):
    """one module-wide handle through all inputs in order: the closed forms, the uniform and the skewed graph, the vertex
    whose degree falls below k, and one band per lane width"""
    bh, _ = hd
    n, Sp, Sj = R.case(name)
    want = R.answer(name)
    check(run(bh, n, Sp, Sj, what=name), want, name)
    check(run(bh, n, Sp, Sj, what=name, rounded=False), want, (name, "without the rounds"))
    if name in R.CLOSED:
        assert (set(want[0].tolist()), want[2], want[3]) == R.CLOSED[name][1:], name
    if name.startswith("band"):
        assert R.lanes(n, len(Sj)) == int(name[4:]), name             # the lane width this input is for
    if name == "rmat12":
        assert len(np.unique(want[0])) > 30 and np.diff(Sp).max() > 1024   # level jumps; a hub row beyond every lane width
    if name == "leaves3":
        assert want[0].tolist() == [1, 1, 1, 1] and sorted(want[1].tolist()) == [1, 1, 1, 2]


# ---------------------------------------------------------------- capped grids
def test_the_block_loops_of_capped_grids(hd):
    """disjoint cliques of 3 and of 5 under a random relabelling at gridpass.cap_rows(numCU, 1): more blocks than 16
    workgroups a CU hold, the last one partial, and a first frontier -- the cliques of 3 -- that is itself more than the
    cap's workgroups take in one turn, so that the check, the peel, the minimum and the gather all take a second turn of
    their block loops; a second level follows.  The closed form: core q - 1, rounds 1 and 2"""
    bh, _ = hd
    cus = num_cu()
    n = gp.cap_rows(cus, 1)

    def make():
        pattern, core = R.cliques35(n)
        pattern, perm = R.relabel(pattern, 77)
        out = np.empty(n, np.int32)
        out[perm] = core
        return pattern, out
    (n, Sp, Sj), core = st.cached(("kcore capped", n), make)
    assert R.lanes(n, len(Sj)) == 1 and gp.blocks(n, 1) > gp.CAP_A * cus and n % 256 != 0, (n, len(Sj), cus)
    assert (core == 2).sum() > 256 * gp.CAP_A * cus and (core == 4).sum() > 0
    check(run(bh, n, Sp, Sj, what="capped"), (core, core // 2, 4, 2), "capped")


# ---------------------------------------------------------------- repeatability
def test_runs_handles_and_libraries_agree():
    n, Sp, Sj = R.case("rmat12")
    outs = []
    for dtype in DTYPES:
        bh = new_handle(dtype)
        try:
            outs += [run(bh, n, Sp, Sj) for _ in range(2)]           # the same handle twice
        finally:
            bh.freePlatform()
        bh = new_handle(dtype)                                       # and a fresh one
        try:
            outs.append(run(bh, n, Sp, Sj))
        finally:
            bh.freePlatform()
    for got in outs:
        check(got, R.answer("rmat12"), "handles")
        assert got[2:] == outs[0][2:]
        for a, b in zip(got[:2], outs[0][:2]):
            assert a.tobytes() == b.tobytes()


# ---------------------------------------------------------------- refusals
def test_refusals(hd):
    bh, dtype = hd
    n, Sp, Sj = R.case("grid32")
    bad = Sj.copy(); bad[len(bad) // 2] = n                          # noqa: E702
    run(bh, n, Sp, bad, want=INV, what="a column equal to n")
    la = launches(bh)                                                 # refused by the first kernel: the first batch left at once
    assert la == {"kcore_check": 1, "kcore_peel": BATCH, "kcore_advance": 1 + 3 * BATCH}, la
    bad = Sj.copy(); bad[7] = -1                                     # noqa: E702
    run(bh, n, Sp, bad, want=INV, what="a negative column")
    p = Sp.copy(); p[100] = p[101] + 1                               # noqa: E702
    run(bh, n, p, Sj, want=INV, what="a falling rowPtr")
    run(bh, n, Sp, Sj, want=INV, what="rowPtr[n] != nnz", nnz=len(Sj) - 3)
    bad = Sj.copy(); q = Sp[200]; bad[q], bad[q + 1] = bad[q + 1], bad[q]   # noqa: E702
    assert R.refusal(n, Sp, bad) == "ascending"
    run(bh, n, Sp, bad, want=INV, what="a row not strictly ascending")
    bad = Sj.copy(); bad[q + 1] = bad[q]                             # noqa: E702
    run(bh, n, Sp, bad, want=INV, what="a repeated entry")
    q = int(np.flatnonzero(Sj[Sp[300]:Sp[301]] != 300)[0]) + Sp[300]
    p, bad = np.where(np.arange(n + 1) > 300, Sp - 1, Sp).astype(np.int32), np.delete(Sj, q)
    assert R.refusal(n, p, bad) == "symmetric"
    run(bh, n, p, bad, want=INV, what="an asymmetric pattern")
    run(bh, n, Sp, Sj, want=INV, what="d_round is d_core", alias=True)
    run(bh, n, Sp, Sj, 1, want=INV, what="flags = 1")
    run(bh, n, Sp, Sj, -1, want=INV, what="flags = -1")
    run(bh, -1, Sp, Sj, want=INV, what="a negative n")
    dSp, dSj = up(Sp, np.int32), up(Sj, np.int32)
    run(bh, n, Sp, Sj, want=INV, what="a NULL rowPtr", dev=(None, dSj))
    run(bh, n, Sp, Sj, want=INV, what="a NULL colInd", dev=(dSp, None))
    torch.cuda.synchronize()
    bh.kcore_kmax = -1                                                # an output inside S: d_core over the columns; no d_core
    assert graph.kcore_raw_device(bh, n, len(Sj), dSp, dSj, 0, dSj[8:], None) == INV and bh.kcore_kmax == -1
    assert graph.kcore_raw_device(bh, n, len(Sj), dSp, dSj, 0, None, None) == INV
    assert np.array_equal(dSj.cpu().numpy(), Sj) and np.array_equal(dSp.cpu().numpy(), Sp)
    check(run(bh, n, Sp, Sj, what="after the refusals"), R.answer("grid32"), "after the refusals")


def test_refused_between_symbolic_and_finish():
    n, Ap, Aj = R.case("grid32")
    dAp, dAj, dAx = up(Ap, np.int32), up(Aj, np.int32), up(np.ones(len(Aj)), np.float64)
    bh = new_handle()
    try:
        assert bh.initData_device(n, n, n, len(Aj), dAx, dAp, dAj, len(Aj), dAx, dAp, dAj) == 0
        assert bh.spgemm_symbolic() == 0
        run(bh, n, Ap, Aj, want=INV, what="a multiply is open")
        assert bh.spgemm_numeric(0, n) == 0 and bh.spgemm_finish() == 0
        check(run(bh, n, Ap, Aj, what="after finish"), R.answer("grid32"), "after finish")
        bh.free_mem()
    finally:
        bh.freePlatform()


# ---------------------------------------------------------------- the Python layer
@pytest.mark.parametrize("name", ("uniform4096", "rmat12", "hub"))
def test_degeneracy_order_and_subgraph(hd, name):
    bh, dtype = hd
    n, Sp, Sj = R.case(name)
    wcore, wrnd, wkmax, wrounds = R.answer(name)
    A = (up(Sp, np.int32), up(Sj, np.int32), up(np.arange(1, len(Sj) + 1) % 7 + 1, dtype))
    core, rnd, kmax, rounds = graph.kcore_device(bh, n, A)
    assert core.dtype == rnd.dtype == torch.int32 and (kmax, rounds) == (wkmax, wrounds)
    assert np.array_equal(core.cpu().numpy(), wcore) and np.array_equal(rnd.cpu().numpy(), wrnd)
    order = graph.degeneracy_order_device(rnd)
    assert order.dtype == torch.int32 and np.array_equal(order.cpu().numpy(), np.lexsort((np.arange(n), wrnd)))
    later = R.later_neighbours(n, Sp, Sj, order.cpu().numpy())
    assert np.all(later <= wcore) and later.max() <= kmax             # at most core[v] <= kmax neighbours behind every vertex
    V, (Zp, Zj, Zx) = graph.kcore_subgraph_device(bh, n, A, core, kmax)
    V, Zp, Zj = V.cpu().numpy(), Zp.cpu().numpy(), Zj.cpu().numpy()
    assert np.array_equal(V, np.flatnonzero(wcore >= kmax)) and len(V) > kmax and len(Zp) == len(V) + 1
    off = np.bincount(np.repeat(np.arange(len(V)), np.diff(Zp))[Zj != np.repeat(np.arange(len(V)), np.diff(Zp))], minlength=len(V))
    assert off.min() >= kmax, (name, off.min(), kmax)                 # the kmax-core: minimum degree >= kmax
    assert Zx is not None and len(Zx) == len(Zj)
    none = graph.kcore_subgraph_device(bh, n, A, core, kmax + 1)
    assert none[0].numel() == 0 and none[1][1].numel() == 0


def test_kcore_csr():
    n, Sp, Sj = R.case("cliques")
    core, rnd, kmax, rounds = graph.kcore_csr(n, Sp, Sj)
    check((core, rnd, kmax, rounds), R.answer("cliques"), "kcore_csr")


# ---------------------------------------------------------------- the k-truss
def truss_equals(T, iterations, want, n, what):
    Tp, Tj, Tx = (t.cpu().numpy() for t in T)
    wp, wj, wsup, wit = want
    print("%s: nnz %d (reference %d), iterations %d (reference %d)" % (what, len(Tj), len(wj), iterations, wit))
    assert np.array_equal(Tp, wp) and np.array_equal(Tj, wj), what
    assert np.array_equal(Tx, wsup.astype(Tx.dtype)), what            # the values: the triangle counts inside T
    assert np.array_equal(wsup, R.supports(n, Tp, Tj)) and iterations == wit, what
    assert R.refusal(n, Tp, Tj) is None, what                         # T is symmetric, rows ascending, no diagonal kept below
    r, c = R.pairs_of(n, Tp, Tj)
    assert not np.any(r == c), what


def test_ktruss_of_a_clique(hd):
    bh, dtype = hd
    n, Sp, Sj = R.cliques((8,), diag=True)
    A = (up(Sp, np.int32), up(Sj, np.int32), None)
    T, iterations = graph.ktruss_device(bh, n, A, 8)
    truss_equals(T, iterations, R.ktruss(n, Sp, Sj, 8), n, "K8, k = 8")
    assert T[1].numel() == 56 and bool((T[2] == 6).all()) and T[2].dtype == (torch.float64 if dtype == np.float64 else torch.float32)
    T, iterations = graph.ktruss_device(bh, n, A, 9)
    assert T[1].numel() == 0 and T[2].numel() == 0 and iterations == 1 and T[0].cpu().numpy().tolist() == [0] * 9
    T, iterations = graph.ktruss_device(bh, n, A, 2)                  # k <= 2: the off-diagonal pattern with its supports
    truss_equals(T, iterations, R.ktruss(n, Sp, Sj, 2), n, "K8, k = 2")
    assert iterations == 1 and T[1].numel() == 56


@pytest.mark.parametrize("k", (3, 4, 5, 9))
def test_ktruss_of_planted_cliques(hd, k):
    bh, _ = hd
    n, Sp, Sj = st.cached(("kcore planted",), lambda: R.planted(1024, 8, (6, 9, 12), 21))
    want = st.cached(("kcore planted truss", k), lambda: R.ktruss(n, Sp, Sj, k))
    T, iterations = graph.ktruss_device(bh, n, (up(Sp, np.int32), up(Sj, np.int32), None), k)
    truss_equals(T, iterations, want, n, "planted, k = %d" % k)
    assert T[1].numel() > 0 and float(T[2].min()) >= k - 2


def test_ktruss_csr():
    n, Sp, Sj = R.planted(1024, 8, (6, 9, 12), 21)
    (Tp, Tj, Tx), iterations = graph.ktruss_csr(n, Sp, Sj, 5)
    wp, wj, wsup, wit = R.ktruss(n, Sp, Sj, 5)
    assert np.array_equal(Tp, wp) and np.array_equal(Tj, wj) and np.array_equal(Tx, wsup.astype(np.float64)) and iterations == wit


# ---------------------------------------------------------------- the demo
def test_cpp_demo_runs():
    demo_dir = os.path.join(ROOT, "tests", "kcore")
    subprocess.check_call(["make", "-C", demo_dir, "-s"])
    out = subprocess.run([os.path.join(demo_dir, "kcore_demo")], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "k-core decomposition of 1443 vertices" in out.stdout and "kmax 15" in out.stdout and "PASS" in out.stdout
