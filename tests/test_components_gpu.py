"""The connected components (bhs_csr_components_device) and what benchmark_spgemm_using_csr_amd/graph.py builds on them, on
the GPU, both builds.

Reference: tests/ccref.py, the contract of include/bhsparse_hip.h ("connected components") restated in numpy, and on disjoint
cliques the closed form from tests/scantiles.py's `members`.  Everything but the number of passes is a function of the
pattern, so d_root, d_comp, the sizes and ncomp are compared exactly.  Sentinels sit behind every output; they must be intact,
also after a refused call.

The numbering scans ONE COUNT PER 64 VERTICES (the roots among them) with the library's one-pass scan over tiles of
scantiles.SCAN_TILE counts: the clique sizes of test_components_abi.CLIQUES put ceil(n / 64) above a tile, at none, at one
count, at exactly a tile, at several tiles and a remainder and just under a tile, and one handle goes through them in that
order."""
import functools
import os
import subprocess

import numpy as np
import pytest
import scipy.sparse as sp
import torch

from conftest import ROOT
import aggref as ar
import ccref
import scantiles as st
from test_components_abi import CLIQUES, scanned

from benchmark_spgemm_using_csr_amd import _lib, amg, graph
from benchmark_spgemm_using_csr_amd.facade import BHSPARSE_HIP, NUM_PLATFORMS, bhsparse

pytestmark = pytest.mark.gpu

DTYPES = (np.float64, np.float32)
INV = _lib.BHS_ERR_INVALID_ARG
PAD = 64
SENT = -7
FAMILIES = {"components_pass", "components_number"}
PATTERNS = ("one_with_diag", "one_without_diag", "two_one_edge", "path300", "poisson5pt_33", "poisson27pt_9", "uniform2048",
            "powerlaw3000", "star1024", "two_k70", "random_directed", "no_entries", "star_centre_last", "by_hand")


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


@functools.lru_cache(maxsize=None)
def pattern(name):
    own = {"random_directed": ccref.random_directed, "no_entries": ccref.no_entries, "star_centre_last": ccref.star_centre_last,
           "by_hand": ccref.by_hand, "relabelled_path": ccref.relabelled_path}
    return own[name]() if name in own else ar.gpu_cases()[name]


@functools.lru_cache(maxsize=None)
def reference(name):
    return ccref.components(*pattern(name))


def run(bh, n, Ap, Aj, want=0, what="", nnz=None, numbered=True, sized=True, flags=0, dev=None, alias=False):
    """The device's answer (root, comp, sizes, ncomp, passes) as numpy (comp and sizes None where they are not asked for); the
    sentinels behind the outputs are checked, and after a refusal that the handle's attributes stayed"""
    dAp, dAj = dev if dev is not None else (up(Ap, np.int32) if len(Ap) else torch.zeros(1, dtype=torch.int32).cuda(),
                                            up(Aj, np.int32) if len(Aj) else None)
    room = max(n, 0)
    root, comp, size = (torch.full((room + PAD,), SENT, dtype=torch.int32).cuda() for _ in range(3))
    torch.cuda.synchronize()
    bh.components_ncomp = bh.components_passes = -1
    bh.components_ms = -1.0
    err = graph.components_raw_device(bh, n, len(Aj) if nnz is None else nnz, dAp, dAj, flags, root,
                                      root if alias else comp if numbered else None, size if sized else None)
    assert err == want, (what, err)
    assert bool((root[room:] == SENT).all()) and bool((comp[room:] == SENT).all()), (what, "written past the end")
    assert bool((size[room:] == SENT).all()), (what, "written past the end of d_compSize")
    if not numbered:
        assert bool((comp == SENT).all()), (what, "d_comp was not given")
    if not sized:
        assert bool((size == SENT).all()), (what, "d_compSize was not given")
    if want != 0:
        assert bh.components_ncomp == -1 and bh.components_passes == -1 and bh.components_ms == -1.0, what
        return None
    ncomp, passes = bh.components_ncomp, bh.components_passes
    assert bh.components_ms >= 0.0, what
    if n:
        assert set(launches(bh)) == (FAMILIES if numbered else {"components_pass"}), (what, launches(bh))
        assert passes >= 8 and passes % 8 == 0 and launches(bh)["components_pass"] == passes + 1, (what, passes, launches(bh))
        if sized:
            assert bool((size[ncomp:] == SENT).all()), (what, "written behind d_compSize[ncomp]")
    return (root[:n].cpu().numpy(), comp[:n].cpu().numpy() if numbered else None, size[:ncomp].cpu().numpy() if sized else None,
            ncomp, passes)


def check(got, want, what):
    root, comp, sizes, ncomp, passes = got
    wroot, wcomp, wsizes, wncomp = want
    assert ncomp == wncomp, (what, ncomp, wncomp)
    assert np.array_equal(root, wroot), (what, "roots", np.flatnonzero(root != wroot)[:5])
    assert comp is None or np.array_equal(comp, wcomp), (what, "numbers")
    assert sizes is None or np.array_equal(sizes, wsizes), (what, "sizes")


# ---------------------------------------------------------------- the patterns
def test_empty(hd):
    bh, _ = hd
    got = run(bh, 0, np.zeros(1, np.int32), np.zeros(0, np.int32), what="n = 0")
    assert got[3] == 0 and got[4] == 0 and len(got[0]) == 0 and bh.components_ms == 0.0


@pytest.mark.parametrize("name", PATTERNS)
def test_against_the_restatement(hd, name):
    bh, _ = hd
    n, Ap, Aj = pattern(name)
    check(run(bh, n, Ap, Aj, what=name), reference(name), name)
    check(run(bh, n, Ap, Aj, what=name, sized=False), reference(name), (name, "without the sizes"))
    check(run(bh, n, Ap, Aj, what=name, numbered=False, sized=False), reference(name), (name, "the roots alone"))
    if name == "no_entries":
        assert reference(name)[3] == n == 1000                      # the sizes fill their capacity exactly
    if name == "random_directed":
        assert 7500 < reference(name)[3] < 8500
    if name == "star_centre_last":
        assert len(Aj) > 64 * n                                      # a whole wave a row
    if name == "powerlaw3000":
        assert np.diff(Ap).max() > 512                               # a hub row beyond every lanes-per-row
    if name == "by_hand":
        got = run(bh, n, Ap, Aj, what=name)
        assert got[0].tolist() == [0, 0, 2, 3, 4, 2, 2] and got[1].tolist() == [0, 0, 1, 2, 3, 1, 1] and got[2].tolist() == [2, 3, 1, 1]


def clique_answer(q, c):
    """on disjoint cliques: the root is the clique's smallest member, the number its rank among them, every size q"""
    n, Sp, Sj, members, clique_of = st.cliques(q, c)
    if n == 0:
        return np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros(0, np.int32), 0
    rank = np.empty(c, np.int64)
    rank[np.argsort(members[:, 0])] = np.arange(c)
    return members[clique_of, 0].astype(np.int32), rank[clique_of].astype(np.int32), np.full(c, q, np.int32), c


def test_one_handle_through_the_scan_sizes(hd):
    """the numbering's scan over ceil(n / 64) counts: above a tile, none, one count, exactly a tile, several tiles and a
    remainder, just under a tile, in that order on one handle; the record components_number books n + that count of rows"""
    bh, _ = hd
    assert tuple(st.role_of(scanned(q, c)) for q, c in CLIQUES) == st.ROLES
    for role, (q, c) in zip(st.ROLES, CLIQUES):
        n, Sp, Sj, _, _ = st.cliques(q, c)
        got = run(bh, n, Sp, Sj, what=role)
        check(got, clique_answer(q, c), role)
        if n:
            rows = {s["name"]: s["rows"] for s in bh.kernel_stats()}["components_number"]
            assert rows == n + scanned(q, c), (role, rows, n, scanned(q, c))
            assert got[4] == 8, (role, got[4])                       # a clique is one hop wide: the first batch ends it


# ---------------------------------------------------------------- depth
def test_the_relabelled_path_takes_few_passes(hd):
    """a path of 32 768 vertices under a random relabelling: diameter 32 767.  The cap is 8 times the synchronous pass count of
    ccref.sync_passes (11; a batch is 8 passes and in-place passes see fresher values than synchronous ones, never staler
    ones than the previous launch's), where plain minimum-label propagation needs thousands.  Measured: 16 passes
    (profiles/components_case.md)."""
    bh, _ = hd
    n, Ap, Aj = pattern("relabelled_path")
    cap = 8 * ccref.sync_passes(n, Ap, Aj)
    got = run(bh, n, Ap, Aj, what="relabelled path")
    print("relabelled path of %d: %d passes, cap %d, %.3f ms" % (n, got[4], cap, bh.components_ms))
    check(got, reference("relabelled_path"), "relabelled path")
    assert got[3] == 1 and got[4] % 8 == 0 and got[4] <= cap, (got[4], cap)


# ---------------------------------------------------------------- repeatability
def test_runs_handles_and_libraries_agree():
    n, Ap, Aj = pattern("random_directed")
    outs = []
    for dtype in DTYPES:
        bh = new_handle(dtype)
        try:
            outs += [run(bh, n, Ap, Aj) for _ in range(3)]           # the same handle three times
        finally:
            bh.freePlatform()
        bh = new_handle(dtype)                                       # and a fresh one
        try:
            outs.append(run(bh, n, Ap, Aj))
        finally:
            bh.freePlatform()
    for got in outs:
        check(got, reference("random_directed"), "handles")
        for a, b in zip(got[:3], outs[0][:3]):
            assert a.tobytes() == b.tobytes()


# ---------------------------------------------------------------- refusals
def test_refusals(hd):
    bh, dtype = hd
    n, Ap, Aj = pattern("poisson5pt_33")
    bad = Aj.copy(); bad[len(bad) // 2] = n                          # noqa: E702
    run(bh, n, Ap, bad, want=INV, what="a column equal to n")
    bad = Aj.copy(); bad[7] = -1                                     # noqa: E702
    run(bh, n, Ap, bad, want=INV, what="a negative column")
    p = Ap.copy(); p[100] = p[101] + 1                               # noqa: E702
    run(bh, n, p, Aj, want=INV, what="a decreasing rowPtr")
    run(bh, n, Ap, Aj, want=INV, what="nnzS below rowPtr[n]", nnz=len(Aj) - 3)
    run(bh, n, Ap, Aj, want=INV, what="d_comp is d_root", alias=True)
    run(bh, n, Ap, Aj, want=INV, what="sizes without numbers", numbered=False, sized=True)
    run(bh, n, Ap, Aj, want=INV, what="flags = 1", flags=1)
    run(bh, -1, Ap, Aj, want=INV, what="a negative n")
    dAp, dAj = up(Ap, np.int32), up(Aj, np.int32)
    run(bh, n, Ap, Aj, want=INV, what="a NULL rowPtr", dev=(None, dAj))
    run(bh, n, Ap, Aj, want=INV, what="a NULL colInd", dev=(dAp, None))
    # an output inside S: d_root over the columns
    torch.cuda.synchronize()
    bh.components_ncomp = -1
    assert graph.components_raw_device(bh, n, len(Aj), dAp, dAj, 0, dAj[8:], None, None) == INV and bh.components_ncomp == -1
    assert graph.components_raw_device(bh, n, len(Aj), dAp, dAj, 0, None, None, None) == INV
    assert np.array_equal(dAj.cpu().numpy(), Aj) and np.array_equal(dAp.cpu().numpy(), Ap)
    check(run(bh, n, Ap, Aj, what="after the refusals"), reference("poisson5pt_33"), "after the refusals")


def dense_operands(n, Ap, Aj, dtype):
    return up(Ap, np.int32), up(Aj, np.int32), up(np.ones(len(Aj)), dtype)


def test_refused_between_symbolic_and_finish():
    n, Ap, Aj = pattern("poisson5pt_33")
    dAp, dAj, dAx = dense_operands(n, Ap, Aj, np.float64)
    bh = new_handle()
    try:
        assert bh.initData_device(n, n, n, len(Aj), dAx, dAp, dAj, len(Aj), dAx, dAp, dAj) == 0
        assert bh.spgemm_symbolic() == 0
        run(bh, n, Ap, Aj, want=INV, what="a multiply is open")
        assert bh.spgemm_numeric(0, n) == 0 and bh.spgemm_finish() == 0
        check(run(bh, n, Ap, Aj, what="after finish"), reference("poisson5pt_33"), "after finish")
        bh.free_mem()
    finally:
        bh.freePlatform()


# ---------------------------------------------------------------- the handle's state
def test_a_multiply_stays_as_it_was(hd):
    bh, dtype = hd
    n, Ap, Aj = pattern("poisson5pt_33")
    dAp, dAj, dAx = dense_operands(n, Ap, Aj, dtype)
    assert bh.initData_device(n, n, n, len(Aj), dAx, dAp, dAj, len(Aj), dAx, dAp, dAj) == 0
    bh.quiet = True
    assert bh.spgemm() == 0
    nnzC = bh.get_nnzC()
    Cj, Cx = np.empty(nnzC, np.int32), np.empty(nnzC, dtype)
    assert nnzC > len(Aj) and bh.get_C(Cj, Cx) == 0
    m, mp, mj = pattern("random_directed")
    check(run(bh, m, mp, mj, what="after a multiply"), reference("random_directed"), "after a multiply")
    assert set(launches(bh)) == FAMILIES
    run(bh, m, mp, mj, what="after a multiply", numbered=False, sized=False)
    assert set(launches(bh)) == {"components_pass"}
    Cj2, Cx2 = np.empty(nnzC, np.int32), np.empty(nnzC, dtype)
    assert bh.get_nnzC() == nnzC and bh.get_C(Cj2, Cx2) == 0
    assert np.array_equal(Cj, Cj2) and np.array_equal(Cx, Cx2)
    assert bh.free_mem() == 0


# ---------------------------------------------------------------- the Python layer
def test_component_lists(hd):
    bh, _ = hd
    for name in ("random_directed", "two_k70", "no_entries"):
        n, Ap, Aj = pattern(name)
        _, wcomp, wsizes, ncomp = reference(name)
        root, comp, sizes = graph.components_device(bh, n, (up(Ap, np.int32), up(Aj, np.int32)))
        assert bh.components_ncomp == ncomp and np.array_equal(comp.cpu().numpy(), wcomp) and np.array_equal(sizes.cpu().numpy(), wsizes)
        order, ptr = graph.component_lists_device(bh, n, comp, ncomp)
        assert order.dtype == torch.int32 and ptr.dtype == torch.int32
        assert np.array_equal(order.cpu().numpy(), np.lexsort((np.arange(n), wcomp))), name
        assert np.array_equal(ptr.cpu().numpy(), np.concatenate([[0], np.cumsum(wsizes)])), name


def test_the_largest_component():
    """two_k70 and a pendant path of 30 on the SECOND clique: 100 vertices against 70"""
    n0, Ap, Aj = pattern("two_k70")
    n = n0 + 30
    S = sp.lil_matrix((n, n))
    S[:n0, :n0] = sp.csr_matrix((np.ones(len(Aj)), Aj, Ap), shape=(n0, n0))
    for k in range(30):
        a, b = (n0 - 1 if k == 0 else n0 + k - 1), n0 + k
        S[a, b] = S[b, a] = 1.0
    S = S.tocsr()
    S.data = np.random.default_rng(3).integers(1, 9, S.nnz).astype(np.float64)
    vertices, (Zp, Zj, Zx) = graph.largest_component_csr(n, S.indptr, S.indices, S.data)
    want = np.arange(70, 170)
    assert vertices.dtype == np.int32 and np.array_equal(vertices, want)
    Z = sp.csr_matrix((Zx, Zj, Zp), shape=(100, 100))
    assert (Z != S[want][:, want]).nnz == 0
    # a tie goes to the smaller root
    vertices, _ = graph.largest_component_csr(n0, Ap, Aj, np.ones(len(Aj)))
    assert np.array_equal(vertices, np.arange(70))


def test_aggregates_are_connected(hd):
    """poisson5pt_33: every aggregate of aggregate_device induces a connected subgraph -- the pattern restricted to the edges
    inside an aggregate has as many components as there are aggregates"""
    bh, _ = hd
    n, Ap, Aj = pattern("poisson5pt_33")
    agg, nagg, _ = amg.aggregate_device(bh, n, (up(Ap, np.int32), up(Aj, np.int32)))
    agg = agg.cpu().numpy()
    r = np.repeat(np.arange(n), np.diff(Ap))
    keep = agg[r] == agg[Aj]
    Rp = np.zeros(n + 1, np.int32)
    np.cumsum(np.bincount(r[keep], minlength=n), out=Rp[1:])
    root, comp, sizes = graph.components_csr(n, Rp, Aj[keep])
    assert len(sizes) == nagg and 1 < nagg < n
    assert np.array_equal(sizes, np.bincount(comp)) and np.all(agg[root] == agg)


# ---------------------------------------------------------------- the demo
def test_cpp_demo_runs():
    demo_dir = os.path.join(ROOT, "tests", "components")
    subprocess.check_call(["make", "-C", demo_dir, "-s"])
    out = subprocess.run([os.path.join(demo_dir, "components_demo")], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "components of 3000 vertices" in out.stdout and "PASS" in out.stdout
