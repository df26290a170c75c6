"""MIS(2) aggregation (bhs_csr_aggregate_device) on the GPU, both builds.

Reference: tests/aggref.py, the contract of include/bhsparse_hip.h ("aggregation") restated in numpy.  The result is a
function of (pattern, priorities or seed) alone, so d_agg and d_roots are compared as arrays and nagg exactly, in every case.
Sentinels sit behind d_agg[n] and behind d_roots[nagg]; they must be intact, also after a refused call."""
import functools
import os
import subprocess

import numpy as np
import pytest
import torch

from conftest import ROOT
import aggref as ar

from benchmark_spgemm_using_csr_amd import _lib, amg, gallery
from benchmark_spgemm_using_csr_amd.facade import BHSPARSE_HIP, NUM_PLATFORMS, bhsparse

pytestmark = pytest.mark.gpu

DTYPES = (np.float64, np.float32)
INV = _lib.BHS_ERR_INVALID_ARG
PAD = 64
SENT_AGG, SENT_ROOT = -7, -5
FAMILIES = {"agg_init", "agg_near", "agg_decide", "agg_scan", "agg_join"}
SEEDS = (0, 1, 12345)


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


def families(bh):
    return {s["name"] for s in bh.kernel_stats() if s["launches"] > 0}


@functools.lru_cache(maxsize=None)
def cases():
    return ar.gpu_cases()


@functools.lru_cache(maxsize=None)
def reference(name, seed):
    n, Sp, Sj = cases()[name]
    return ar.aggregate(n, Sp, Sj, seed)


def run(bh, n, Sp, Sj, seed=0, prio=None, flags=0, want=0, with_roots=True, what="", nnz=None, agg_arg="own"):
    """The device's answer (agg, nagg, roots, rounds) as numpy; the sentinels behind both outputs are checked.  agg_arg:
    "own" a buffer made here, None a NULL pointer, or a tensor to pass as d_agg."""
    dSp = up(Sp, np.int32) if len(Sp) else torch.zeros(1, dtype=torch.int32).cuda()
    dSj = up(Sj, np.int32) if len(Sj) else torch.zeros(1, dtype=torch.int32).cuda()
    dprio = None if prio is None else up(np.asarray(prio, np.uint32).view(np.int32), np.int32)
    room = max(n, 0)
    agg = torch.full((room + PAD,), SENT_AGG, dtype=torch.int32).cuda()
    roots = torch.full((room + PAD,), SENT_ROOT, dtype=torch.int32).cuda() if with_roots else None
    torch.cuda.synchronize()
    bh.aggregate_nagg = bh.aggregate_rounds = -1
    d_agg = agg if isinstance(agg_arg, str) else agg_arg
    err = amg.aggregate_raw_device(bh, n, len(Sj) if nnz is None else nnz, dSp, dSj if len(Sj) else None, dprio, seed, flags,
                                   d_agg, roots)
    assert err == want, (what, err)
    assert bool((agg[room:] == SENT_AGG).all()), (what, "written past the end of d_agg")
    if roots is not None:
        assert bool((roots[room:] == SENT_ROOT).all()), (what, "written past the end of d_roots")
    if want != 0:
        assert bh.aggregate_nagg == -1
        return None
    nagg = bh.aggregate_nagg
    assert bh.aggregate_ms >= 0.0 and families(bh) <= FAMILIES, (what, families(bh))
    if roots is not None:
        assert bool((roots[nagg:] == SENT_ROOT).all()), (what, "written behind d_roots[nagg]")
    return agg[:n].cpu().numpy(), nagg, (None if roots is None else roots[:nagg].cpu().numpy()), bh.aggregate_rounds


def check(got, want, what):
    agg, nagg, roots, rounds = got
    wagg, wnagg, wroots, wrounds = want
    assert nagg == wnagg, (what, nagg, wnagg)
    assert np.array_equal(agg, wagg), what
    if roots is not None:
        assert np.array_equal(roots, wroots), what
    assert rounds == wrounds and (rounds >= 1 or len(wagg) == 0), (what, rounds, wrounds)


# ---------------------------------------------------------------- patterns x seeds
def test_empty(hd):
    bh, _ = hd
    got = run(bh, 0, np.zeros(1, np.int32), np.zeros(0, np.int32), what="n = 0")
    assert got[1] == 0 and got[3] == 0 and len(got[0]) == 0


@pytest.mark.parametrize("name", ("one_with_diag", "one_without_diag", "two_one_edge", "path300", "poisson5pt_33", "poisson9pt_20",
                                  "poisson27pt_9", "uniform2048", "powerlaw3000", "roadlike40", "star1024", "two_k70"))
def test_patterns_and_seeds(hd, name):
    bh, _ = hd
    n, Sp, Sj = cases()[name]
    for seed in SEEDS:
        check(run(bh, n, Sp, Sj, seed, what=(name, seed)), reference(name, seed), (name, seed))
    if name == "star1024":
        assert reference(name, 0)[1] == 1
    if name == "two_k70":
        assert reference(name, 0)[1] == 2
    if name == "roadlike40":
        agg, nagg, roots, _ = reference(name, 0)
        assert (np.bincount(agg, minlength=nagg) == 1).any()          # isolated vertices: singleton aggregates


def test_without_roots(hd):
    bh, _ = hd
    n, Sp, Sj = cases()["poisson5pt_33"]
    check(run(bh, n, Sp, Sj, 1, with_roots=False), reference("poisson5pt_33", 1), "d_roots NULL")


def test_caller_priorities(hd):
    bh, _ = hd
    n, Sp, Sj = cases()["uniform2048"]
    rng = np.random.default_rng(5)
    prio = rng.integers(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32)
    prio[:7] = (0, 1, 0xFFFFFFFF, 0xFFFFFFFE, 0x80000000, 2, 3)   # the lowest bit is dropped: ties, broken by index
    check(run(bh, n, Sp, Sj, 99, prio=prio, what="prio"), ar.aggregate(n, Sp, Sj, 99, prio), "caller priorities")


def test_equal_priorities_on_a_path(hd):
    """ties are broken by index: the greatest index wins, the chain of decisions runs down the path -- about n / 3 rounds"""
    bh, _ = hd
    Ap, Aj = gallery.poisson_csr("poisson5pt", 64, 1)
    want = ar.aggregate(64, Ap, Aj, 0, np.full(64, 12, np.uint32))
    assert want[3] >= 20 and want[2].tolist() == list(range(0, 64, 3))
    check(run(bh, 64, Ap, Aj, 0, prio=np.full(64, 12, np.uint32), what="equal priorities"), want, "equal priorities")


# ---------------------------------------------------------------- invariances
@pytest.mark.parametrize("name", ("poisson9pt_20", "powerlaw3000"))
def test_invariances_of_the_pattern(hd, name):
    bh, _ = hd
    n, Sp, Sj = cases()[name]
    want = reference(name, 1)
    Sp64 = np.asarray(Sp, np.int64)
    r = np.repeat(np.arange(n), np.diff(Sp64))
    # the diagonal removed
    keep = r != Sj
    p = np.zeros(n + 1, np.int64)
    np.cumsum(np.bincount(r[keep], minlength=n), out=p[1:])
    check(run(bh, n, p, Sj[keep], 1, what="no diagonal"), want, (name, "no diagonal"))
    # every entry twice
    check(run(bh, n, 2 * Sp64, np.repeat(Sj, 2), 1, what="duplicates"), want, (name, "duplicates"))
    # rows shuffled inside
    rng = np.random.default_rng(3)
    order = np.lexsort((rng.random(len(Sj)), r))
    check(run(bh, n, Sp, Sj[order], 1, what="shuffled"), want, (name, "shuffled"))
    assert not np.array_equal(Sj[order], Sj)


def test_both_libraries_handles_and_repeats_agree():
    n, Sp, Sj = cases()["uniform2048"]
    want = reference("uniform2048", 12345)
    outs = []
    for dtype in DTYPES:
        bh = new_handle(dtype)
        try:
            outs.append(run(bh, n, Sp, Sj, 12345))
            outs.append(run(bh, n, Sp, Sj, 12345))                   # the same handle again
        finally:
            bh.freePlatform()
    for got in outs:
        check(got, want, "handles")


def test_a_handle_that_has_just_multiplied(hd):
    bh, dtype = hd
    n, Sp, Sj = cases()["poisson5pt_33"]
    A = (up(Sp, np.int32), up(Sj, np.int32), up(np.ones(len(Sj)), dtype))
    torch.cuda.synchronize()
    assert bh.initData_device(n, n, n, len(Sj), A[2], A[0], A[1], len(Sj), A[2], A[0], A[1]) == 0
    assert bh.spgemm() == 0
    nnzC, ptrs = bh.get_nnzC(), bh.get_C_device()
    check(run(bh, n, Sp, Sj, 0, what="after a multiply"), reference("poisson5pt_33", 0), "after a multiply")
    assert bh.get_nnzC() == nnzC and bh.get_C_device() == ptrs      # the multiply's result stays where it is
    assert bh.free_mem() == 0


# ---------------------------------------------------------------- a non-symmetric pattern
def test_non_symmetric(hd):
    bh, _ = hd
    Ap, Aj = gallery.uniform_csr(2048, 4, seed=9)
    agg, nagg, roots, rounds = run(bh, 2048, Ap, Aj, 0, what="non-symmetric")
    assert 1 <= nagg <= 2048 and rounds >= 1
    assert agg.min() >= 0 and agg.max() < nagg
    assert np.array_equal(agg[roots], np.arange(nagg)) and np.all(np.diff(roots) > 0)
    check((agg, nagg, roots, rounds), ar.aggregate(2048, Ap, Aj, 0), "non-symmetric against the restatement")


# ---------------------------------------------------------------- refusals
def test_refusals(hd):
    bh, _ = hd
    n, Sp, Sj = cases()["poisson5pt_33"]
    nnz = len(Sj)
    bad = Sj.copy(); bad[nnz // 2] = n                               # noqa: E702
    assert ar.invalid(n, nnz, Sp, bad) == "column out of range"
    run(bh, n, Sp, bad, want=INV, what="a column equal to n")
    bad = Sj.copy(); bad[5] = -1                                     # noqa: E702
    run(bh, n, Sp, bad, want=INV, what="a column of -1")
    p = Sp.copy(); p[100] = p[99] - 1                                # noqa: E702
    assert ar.invalid(n, nnz, p, Sj) == "bad row pointer"
    run(bh, n, p, Sj, want=INV, what="a decreasing row pointer")
    p = Sp.copy(); p[n] = nnz + 3                                    # noqa: E702
    run(bh, n, p, Sj, want=INV, what="a last row pointer above nnzS", nnz=nnz)
    run(bh, n, Sp, Sj, flags=1, want=INV, what="flags = 1")
    run(bh, n, Sp, Sj, want=INV, what="NULL d_agg", agg_arg=None)
    run(bh, -1, Sp, Sj, want=INV, what="negative n")
    # d_agg aliasing d_colIndS
    dSp, dSj = up(Sp, np.int32), up(Sj, np.int32)
    torch.cuda.synchronize()
    assert amg.aggregate_raw_device(bh, n, nnz, dSp, dSj, None, 0, 0, dSj, None) == INV
    assert np.array_equal(dSj.cpu().numpy(), Sj)
    # d_roots overlapping d_agg: a path of 8 vertices, two views into one tensor shifted by one element
    Pp = np.array([0, 1, 3, 5, 7, 9, 11, 13, 14], np.int32)
    Pj = np.array([1, 0, 2, 1, 3, 2, 4, 3, 5, 4, 6, 5, 7, 6], np.int32)
    assert ar.invalid(8, 14, Pp, Pj) is None
    dPp, dPj = up(Pp, np.int32), up(Pj, np.int32)
    both = torch.full((9,), SENT_AGG, dtype=torch.int32).cuda()
    torch.cuda.synchronize()
    assert amg.aggregate_raw_device(bh, 8, 14, dPp, dPj, None, 0, 0, both[:8], both[1:]) == INV
    assert amg.aggregate_raw_device(bh, 8, 14, dPp, dPj, None, 0, 0, both[:8], both[:8]) == INV
    assert bool((both == SENT_AGG).all())
    # the next valid call on the same handle is correct
    check(run(bh, n, Sp, Sj, 0, what="after the refusals"), reference("poisson5pt_33", 0), "after the refusals")


def test_cpp_demo_runs():
    demo_dir = os.path.join(ROOT, "tests", "aggregate")
    subprocess.check_call(["make", "-C", demo_dir, "-s"])
    out = subprocess.run([os.path.join(demo_dir, "aggregate_demo")], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    _, nagg, _, rounds = reference("poisson5pt_33", 0)
    assert "aggregate poisson5pt 33x33 seed 0: nagg %d rounds %d PASS" % (nagg, rounds) in out.stdout
