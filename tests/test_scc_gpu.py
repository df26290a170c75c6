"""The strongly connected components (bhs_csr_scc_device) and what benchmark_spgemm_using_csr_amd/graph.py builds on them, on
the GPU, both builds.

Reference: tests/sccref.py, the contract of include/bhsparse_hip.h ("strongly connected components") restated in numpy, and
on ring chains and ring pairs their closed forms.  Everything but the number of passes is a function of the pattern, so
d_root, d_comp, the sizes, nscc AND the rounds are compared exactly.  Sentinels sit behind every output; they must be intact,
also after a refused call.

The numbering scans ONE COUNT PER 64 VERTICES (the roots among them) with the library's one-pass scan over tiles of
scantiles.SCAN_TILE counts: the ring sizes of test_scc_abi.RINGS put ceil(n / 64) above a tile, at none, at one count, at
exactly a tile, at several tiles and a remainder and just under a tile, and one handle goes through them in that order."""
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
import gridpass as gp
import scantiles as st
import sccref
from test_scc_abi import RINGS, scanned

from benchmark_spgemm_using_csr_amd import _lib, graph
from benchmark_spgemm_using_csr_amd.facade import BHSPARSE_HIP, NUM_PLATFORMS, bhsparse

pytestmark = pytest.mark.gpu

DTYPES = (np.float64, np.float32)
INV = _lib.BHS_ERR_INVALID_ARG
PAD = 64
SENT = -7
BATCH = 8
ROUND_FAMILIES = {"scc_trim", "scc_forward", "scc_backward", "scc_decide"}
PATTERNS = ("by_hand", "ring_chain_up", "ring_chain_down", "ring_chain_70", "one_with_diag", "one_without_diag", "two_one_edge",
            "path300", "poisson5pt_33", "poisson9pt_20", "poisson27pt_9", "uniform2048", "powerlaw3000", "roadlike40", "star1024",
            "two_k70", "random_directed", "star_centre_last", "no_entries", "random_30000", "random_60000")
TRANSPOSED = ("by_hand", "ring_chain_up", "ring_chain_down", "powerlaw3000", "random_directed", "random_30000", "star_centre_last")
CAPPED = ((3, 1, 1), (33, 16, 20))                 # (q, lanes a row, repeats of a ring edge): ring_pairs at gridpass.cap_rows


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
def pattern(name):
    own = {"by_hand": sccref.by_hand, "ring_chain_up": lambda: sccref.ring_chain(5, 6, True),
           "ring_chain_down": lambda: sccref.ring_chain(5, 6, False), "ring_chain_70": lambda: sccref.ring_chain(70, 3, True),
           "random_directed": ccref.random_directed, "star_centre_last": ccref.star_centre_last, "no_entries": ccref.no_entries,
           "random_30000": lambda: sccref.random_graph(20000, 30000, 21), "random_60000": lambda: sccref.random_graph(20000, 60000, 22),
           "one_way_ring": sccref.one_way_ring}
    return own[name]() if name in own else ar.gpu_cases()[name]


@functools.lru_cache(maxsize=None)
def reference(name):
    return sccref.scc(*pattern(name))


def run(bh, n, Ap, Aj, want=0, what="", nnz=None, numbered=True, sized=True, flags=0, dev=None, alias=False):
    """The device's answer (root, comp, sizes, nscc, rounds, passes) as numpy (comp and sizes None where they are not asked
    for); the sentinels behind the outputs are checked, the launch counts against the rounds and passes, and after a refusal
    that the handle's attributes stayed"""
    dAp, dAj = dev if dev is not None else (up(Ap, np.int32) if len(Ap) else torch.zeros(1, dtype=torch.int32).cuda(),
                                            up(Aj, np.int32) if len(Aj) else None)
    room = max(n, 0)
    root, comp, size = (torch.full((room + PAD,), SENT, dtype=torch.int32).cuda() for _ in range(3))
    torch.cuda.synchronize()
    bh.scc_nscc = bh.scc_rounds = bh.scc_passes = -1
    bh.scc_ms = -1.0
    err = graph.scc_raw_device(bh, n, len(Aj) if nnz is None else nnz, dAp, dAj, flags, root,
                               root if alias else comp if numbered else None, size if sized else None)
    assert err == want, (what, err)
    assert bool((root[room:] == SENT).all()) and bool((comp[room:] == SENT).all()), (what, "written past the end")
    assert bool((size[room:] == SENT).all()), (what, "written past the end of d_compSize")
    if not numbered:
        assert bool((comp == SENT).all()), (what, "d_comp was not given")
    if not sized:
        assert bool((size == SENT).all()), (what, "d_compSize was not given")
    if want != 0:
        assert bh.scc_nscc == -1 and bh.scc_rounds == -1 and bh.scc_passes == -1 and bh.scc_ms == -1.0, what
        return None
    nscc, rounds, passes = bh.scc_nscc, bh.scc_rounds, bh.scc_passes
    assert bh.scc_ms >= 0.0, what
    if n:
        la = launches(bh)
        assert set(la) - ROUND_FAMILIES == ({"scc_number"} if numbered else set()) and "scc_trim" in la, (what, la)
        # a trim pass is two launches; a round that goes on starts its labels and its flags once and decides once
        decides = la.get("scc_decide", 0)
        trim, fwd, bwd = la["scc_trim"], la.get("scc_forward", 0) - decides, la.get("scc_backward", 0) - decides
        assert rounds >= 1 and rounds - 1 <= decides <= rounds, (what, rounds, la)
        assert trim % (2 * BATCH) == 0 and fwd % BATCH == 0 and bwd % BATCH == 0 and passes % BATCH == 0, (what, passes, la)
        assert trim // 2 >= BATCH * rounds and fwd >= BATCH * decides and bwd >= BATCH * decides, (what, rounds, la)
        assert passes == trim // 2 + fwd + bwd, (what, passes, la)
        if numbered:
            assert la["scc_number"] == (4 if sized else 3), (what, la)
        if sized:
            assert bool((size[nscc:] == SENT).all()), (what, "written behind d_compSize[nscc]")
    return (root[:n].cpu().numpy(), comp[:n].cpu().numpy() if numbered else None, size[:nscc].cpu().numpy() if sized else None,
            nscc, rounds, passes)


def check(got, want, what):
    root, comp, sizes, nscc, rounds, _ = got
    wroot, wcomp, wsizes, wnscc, wrounds = want
    assert nscc == wnscc, (what, nscc, wnscc)
    assert np.array_equal(root, wroot), (what, "roots", np.flatnonzero(root != wroot)[:5])
    assert comp is None or np.array_equal(comp, wcomp), (what, "numbers")
    assert sizes is None or np.array_equal(sizes, wsizes), (what, "sizes")
    assert rounds == wrounds, (what, "rounds", rounds, wrounds)


# ---------------------------------------------------------------- the patterns
def test_empty(hd):
    bh, _ = hd
    got = run(bh, 0, np.zeros(1, np.int32), np.zeros(0, np.int32), what="n = 0")
    assert got[3] == 0 and got[4] == 0 and got[5] == 0 and len(got[0]) == 0 and bh.scc_ms == 0.0


@pytest.mark.parametrize("name", PATTERNS)
def test_against_the_restatement(hd, name):
    bh, _ = hd
    n, Ap, Aj = pattern(name)
    check(run(bh, n, Ap, Aj, what=name), reference(name), name)
    check(run(bh, n, Ap, Aj, what=name, sized=False), reference(name), (name, "without the sizes"))
    check(run(bh, n, Ap, Aj, what=name, numbered=False, sized=False), reference(name), (name, "the roots alone"))
    if name == "by_hand":
        got = run(bh, n, Ap, Aj, what=name)
        assert got[0].tolist() == [0, 0, 0, 3, 3, 5, 6, 7, 8] and got[1].tolist() == [0, 0, 0, 1, 1, 2, 3, 4, 5]
        assert got[2].tolist() == [3, 2, 1, 1, 1, 1] and got[3:5] == (6, 2)
        assert got[3] > ccref.components(n, Ap, Aj)[3]               # not the weak components' answer
    if name.startswith("ring_chain"):
        q, c, ascending = {"ring_chain_up": (5, 6, True), "ring_chain_down": (5, 6, False), "ring_chain_70": (70, 3, True)}[name]
        want = sccref.ring_chain_answer(q, c, ascending)
        assert all(np.array_equal(a, b) for a, b in zip(reference(name), want)), name
        assert reference(name)[4] == (c if ascending else 1) and ccref.components(n, Ap, Aj)[3] == 1
    if name == "no_entries":
        assert reference(name)[3] == n == 1000 and launches(bh) == {"scc_trim": 2 * BATCH}   # the sizes fill their capacity; trimmed at once
    if name in ("random_30000", "random_60000"):
        assert 1000 < reference(name)[3] < n and reference(name)[2].max() > 1000             # thousands of SCCs and a giant one
    if name == "star_centre_last":
        assert len(Aj) > 64 * n and lanes(n, len(Aj)) == 64          # a whole wave a row
    if name == "poisson27pt_9":
        assert lanes(n, len(Aj)) == 16
    if name == "poisson5pt_33":
        assert lanes(n, len(Aj)) == 4 and reference(name)[3:] == (1, 1)   # symmetric and connected: one SCC, one round
    if name == "powerlaw3000":
        assert np.diff(Ap).max() > 512                               # a hub row beyond every lanes-per-row


@pytest.mark.parametrize("name", TRANSPOSED)
def test_the_direction_does_not_matter(hd, name):
    """the same pattern transposed on the host: identical roots, numbers and sizes"""
    bh, _ = hd
    n, Ap, Aj = pattern(name)
    a = run(bh, n, Ap, Aj, what=name)
    b = run(bh, *sccref.transposed(n, Ap, Aj), what=(name, "transposed"))
    check(a, reference(name), name)
    assert a[3] == b[3], (name, a[3], b[3])
    for x, y in zip(a[:3], b[:3]):
        assert x.tobytes() == y.tobytes(), name


def test_one_handle_through_the_scan_sizes(hd):
    """the numbering's scan over ceil(n / 64) counts: above a tile, none, one count, exactly a tile, several tiles and a
    remainder, just under a tile, in that order on one handle; the record scc_number books n + that count of rows"""
    bh, _ = hd
    assert tuple(st.role_of(scanned(q, c)) for q, c in RINGS) == st.ROLES
    for role, (q, c) in zip(st.ROLES, RINGS):
        n, Sp, Sj, _, _ = sccref.ring_pairs(q, c)
        got = run(bh, n, Sp, Sj, what=role)
        check(got, sccref.ring_pairs_answer(q, c), role)
        if n:
            rows = {s["name"]: s["rows"] for s in bh.kernel_stats()}["scc_number"]
            assert rows == n + scanned(q, c), (role, rows, n, scanned(q, c))


# ---------------------------------------------------------------- capped grids
@pytest.mark.parametrize("q,L,repeats", CAPPED, ids=("L1", "L16"))
def test_the_block_loops_of_capped_grids(hd, q, L, repeats):
    """ring pairs at gridpass.cap_rows: more blocks than 16 workgroups a CU, the last one partial, so that the workgroups of
    every pass take a second turn in the block loop; against the closed form"""
    bh, _ = hd
    cus = num_cu()
    per = 256 // L
    c = -(-gp.cap_rows(cus, L) // q)
    while q * c % per == 0:
        c += 1
    n, Sp, Sj, _, _ = sccref.ring_pairs(q, c, repeats)
    assert lanes(n, len(Sj)) == L and gp.blocks(n, L) > gp.CAP_A * cus and n % per != 0, (n, len(Sj), L, cus)
    check(run(bh, n, Sp, Sj, what=("capped", L)), sccref.ring_pairs_answer(q, c), ("capped", L))


# ---------------------------------------------------------------- depth
def test_a_one_way_ring_stays_inside_the_bound(hd):
    """a one-way ring of 2048 vertices under a seeded relabelling: one SCC in one round, every phase inside the contract's own
    n + 1 passes and a batch.  Measured: 2016 and 2024 passes in the two builds (profiles/scc_case.md): the backward reach
    moves one hop a pass."""
    bh, _ = hd
    n, Ap, Aj = pattern("one_way_ring")
    got = run(bh, n, Ap, Aj, what="one-way ring")
    print("one-way ring of %d: %d passes in %d round, %.3f ms" % (n, got[5], got[4], bh.scc_ms))
    check(got, reference("one_way_ring"), "one-way ring")
    assert got[3] == 1 and got[4] == 1 and got[5] % BATCH == 0 and got[5] <= 3 * (n + 1) + 24, got[5]


# ---------------------------------------------------------------- repeatability
def test_runs_handles_and_libraries_agree():
    n, Ap, Aj = pattern("random_30000")
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
        check(got, reference("random_30000"), "handles")
        assert got[4] == outs[0][4]
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
    bh.scc_nscc = -1
    assert graph.scc_raw_device(bh, n, len(Aj), dAp, dAj, 0, dAj[8:], None, None) == INV and bh.scc_nscc == -1
    assert graph.scc_raw_device(bh, n, len(Aj), dAp, dAj, 0, None, None, None) == INV
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
    m, mp, mj = pattern("random_30000")
    check(run(bh, m, mp, mj, what="after a multiply"), reference("random_30000"), "after a multiply")
    assert set(launches(bh)) == ROUND_FAMILIES | {"scc_number"}
    run(bh, m, mp, mj, what="after a multiply", numbered=False, sized=False)
    assert set(launches(bh)) == ROUND_FAMILIES
    Cj2, Cx2 = np.empty(nnzC, np.int32), np.empty(nnzC, dtype)
    assert bh.get_nnzC() == nnzC and bh.get_C(Cj2, Cx2) == 0
    assert np.array_equal(Cj, Cj2) and np.array_equal(Cx, Cx2)
    assert bh.free_mem() == 0


# ---------------------------------------------------------------- the Python layer
def test_scc_device_and_the_lists(hd):
    bh, _ = hd
    for name in ("random_30000", "by_hand", "no_entries"):
        n, Ap, Aj = pattern(name)
        _, wcomp, wsizes, nscc, rounds = reference(name)
        root, comp, sizes = graph.scc_device(bh, n, (up(Ap, np.int32), up(Aj, np.int32)))
        assert bh.scc_nscc == nscc and bh.scc_rounds == rounds
        assert np.array_equal(comp.cpu().numpy(), wcomp) and np.array_equal(sizes.cpu().numpy(), wsizes), name
        order, ptr = graph.component_lists_device(bh, n, comp, nscc)
        assert order.dtype == torch.int32 and ptr.dtype == torch.int32
        assert np.array_equal(order.cpu().numpy(), np.lexsort((np.arange(n), wcomp))), name
        assert np.array_equal(ptr.cpu().numpy(), np.concatenate([[0], np.cumsum(wsizes)])), name


def dense_condensation(n, Ap, Aj, comp, nscc):
    D = np.zeros((nscc, nscc))
    r = np.repeat(np.arange(n), np.diff(Ap))
    off = comp[r] != comp[Aj]
    np.add.at(D, (comp[r][off], comp[Aj][off]), 1.0)
    return D


def test_the_condensation(hd):
    bh, dtype = hd
    # six rings in a chain: the path DAG 0 -> 1 -> ... -> 5, every value 1
    n, Ap, Aj = pattern("ring_chain_up")
    A = (up(Ap, np.int32), up(Aj, np.int32))
    _, comp, _ = graph.scc_device(bh, n, A)
    Zp, Zj, Zx = graph.condensation_device(bh, n, A, comp, bh.scc_nscc)
    assert Zp.cpu().numpy().tolist() == [0, 1, 2, 3, 4, 5, 5] and Zj.cpu().numpy().tolist() == [1, 2, 3, 4, 5]
    assert Zx.cpu().numpy().dtype == dtype and Zx.cpu().numpy().tolist() == [1.0] * 5
    # by hand, against a dense host computation; a value counts the entries between two SCCs
    n, Ap, Aj = pattern("by_hand")
    _, wcomp, _, nscc, _ = reference("by_hand")
    A = (up(Ap, np.int32), up(Aj, np.int32))
    _, comp, _ = graph.scc_device(bh, n, A)
    Zp, Zj, Zx = graph.condensation_device(bh, n, A, comp, nscc)
    Zp, Zj, Zx = Zp.cpu().numpy(), Zj.cpu().numpy(), Zx.cpu().numpy()
    Z = sp.csr_matrix((Zx, Zj, Zp), shape=(nscc, nscc)).toarray()
    want = dense_condensation(n, Ap, Aj, wcomp, nscc)
    assert np.array_equal(Z, want) and want.sum() == 4 and len(Zj) == 4
    # a DAG: every vertex of it is a component by itself
    root, _, sizes = graph.scc_csr(nscc, Zp, Zj)
    assert np.array_equal(root, np.arange(nscc)) and len(sizes) == nscc and np.all(sizes == 1)


def test_the_largest_scc():
    """a ring of 5, a ring of 8 behind a bridge and a tail of 2: the ring of 8; two rings of 5: a tie goes to the smaller root"""
    ring = lambda a, k: (np.arange(a, a + k), a + (np.arange(k) + 1) % k)   # noqa: E731
    (s1, d1), (s2, d2) = ring(0, 5), ring(5, 8)
    src, dst = np.concatenate([s1, s2, [4, 12, 13]]), np.concatenate([d1, d2, [5, 13, 14]])
    n = 15
    Ap, Aj = ccref.from_edges(n, src, dst)
    Ax = np.random.default_rng(3).integers(1, 9, len(Aj)).astype(np.float64)
    vertices, (Zp, Zj, Zx) = graph.largest_scc_csr(n, Ap, Aj, Ax)
    want = np.arange(5, 13)
    assert vertices.dtype == np.int32 and np.array_equal(vertices, want)
    S = sp.csr_matrix((Ax, Aj, Ap), shape=(n, n))
    Z = sp.csr_matrix((Zx, Zj, Zp), shape=(8, 8))
    assert (Z != S[want][:, want]).nnz == 0 and Z.nnz == 8
    m, Bp, Bj = sccref.ring_chain(5, 2, True)
    vertices, _ = graph.largest_scc_csr(m, Bp, Bj, np.ones(len(Bj)))
    assert np.array_equal(vertices, np.arange(5))


# ---------------------------------------------------------------- the demo
def test_cpp_demo_runs():
    demo_dir = os.path.join(ROOT, "tests", "scc")
    subprocess.check_call(["make", "-C", demo_dir, "-s"])
    out = subprocess.run([os.path.join(demo_dir, "scc_demo")], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "strongly connected components of 3000 vertices" in out.stdout and "PASS" in out.stdout
