"""Sparse frontier x CSR (bhs_csr_push_semiring_device) and the frontier traversals on top of it (graph.py) on the GPU, both
builds.

Reference: tests/pushref.py, the contract of include/bhsparse_hip.h ("sparse frontier x CSR") restated in numpy.  All seven
semirings give the same bits in any order, so Y is compared bit for bit (a NaN in class and place), `changed` exactly and
`next` as an array, in every case.  Y carries sentinels behind its end and in the gaps of its leading dimension, the gaps of F
and M hold NaN, d_next carries sentinels behind the list: none of it may reach a result, nothing may be written there, and
what the mask does not select or no product reaches must still hold the bits it held."""
import functools
import os
import subprocess

import numpy as np
import pytest
import torch

from conftest import ROOT, load_golden
import pushref as pr
import semiringref as srf

from benchmark_spgemm_using_csr_amd import _lib, dense, gallery, graph
from benchmark_spgemm_using_csr_amd.facade import BHSPARSE_HIP, NUM_PLATFORMS, BhsparseError, bhsparse

pytestmark = pytest.mark.gpu

DTYPES = (np.float64, np.float32)
INV = _lib.BHS_ERR_INVALID_ARG
SENTINEL = -7.0
PAD = 64
NAMES = tuple(pr.SEMIRINGS)
CMP = _lib.BHS_MV_MASK_COMPLEMENT
FAMILIES = {"push_degrees", "push_scan", "push_edges", "push_compact"}


# ---------------------------------------------------------------- helpers
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


def bits(x):
    x = np.ascontiguousarray(x)
    return x.view(np.uint64 if x.dtype == np.float64 else np.uint32)


def up(a, dt):
    return torch.from_numpy(np.ascontiguousarray(a, dt).copy()).cuda()


def tdt(dtype):
    return torch.float32 if np.dtype(dtype) == np.dtype(np.float32) else torch.float64


def families(bh):
    return {s["name"] for s in bh.kernel_stats() if s["launches"] > 0}


class Dev:
    """G on the device, uploaded once per (matrix, dtype)"""

    def __init__(self, m, n, G, dtype):
        self.m, self.n, self.dtype = m, n, dtype
        self.Gp, self.Gj = np.ascontiguousarray(G[0], np.int32), np.ascontiguousarray(G[1], np.int32)
        self.Gx = None if G[2] is None else np.ascontiguousarray(G[2], dtype)
        self.nnz = len(self.Gj)
        self.d = (up(self.Gp, np.int32), up(self.Gj, np.int32), None if self.Gx is None else up(self.Gx, dtype))


def run(bh, name, D, fidx, F, Y, mask=None, complement=False, gap=0, values=True, want_next=True, want_changed=True, want=0,
        what=""):
    """The device's answer (Y as numpy n x k, changed, next as numpy or None) to the list fidx, F (numpy nf x k), Y (numpy
    n x k) and mask (numpy n x k or None).  gap: ld = k + gap for F, M and Y.  The sentinels behind Y, in its gaps and behind
    the list are checked; the gaps of F and M hold NaN."""
    n, k = D.n, Y.shape[1]
    nf = len(fidx)
    ld = k + gap
    t = tdt(D.dtype)
    dF = torch.full((max(nf, 1), ld), float("nan"), dtype=t).cuda()
    dF[:nf, :k] = up(F, D.dtype)
    dM = None
    if mask is not None:
        dM = torch.full((max(n, 1), ld), float("nan"), dtype=t).cuda()
        dM[:n, :k] = up(mask, D.dtype)
    buf = torch.full((n * ld + PAD,), SENTINEL, dtype=t).cuda()
    view = buf[:n * ld].view(n, ld)
    view[:, :k] = up(Y, D.dtype)
    dfidx = up(np.asarray(fidx, np.int64), np.int32) if nf else torch.zeros(1, dtype=torch.int32).cuda()
    nxt = torch.full((n + PAD,), -5, dtype=torch.int32).cuda() if want_next else None
    torch.cuda.synchronize()
    bh.spmv_changed, bh.push_next = -1, -1
    err = dense.csr_push_semiring_raw_device(bh, name, D.m, n, D.nnz, D.d[2] if values else None, D.d[0], D.d[1], nf, dfidx, k, dF, ld,
                                             CMP if complement else 0, dM, ld, buf, ld, nxt, want_changed=want_changed)
    assert err == want, (what, name, k, gap, err)
    assert bool((buf[n * ld:] == SENTINEL).all()), (what, name, k, gap, "written past the end of Y")
    assert bool((view[:, k:] == SENTINEL).all()), (what, name, k, gap, "written into the gaps of Y's leading dimension")
    if want != 0:
        assert bh.spmv_changed == -1 and bh.push_next == -1
        return view[:, :k].cpu().numpy(), None, None
    assert bh.spmv_ms >= 0.0 and families(bh) <= FAMILIES
    got_next = None
    if want_next:
        assert 0 <= bh.push_next <= n and bool((nxt[bh.push_next:] == -5).all()), (what, name, "written behind the list")
        got_next = nxt[:bh.push_next].cpu().numpy()
    else:
        assert bh.push_next == 0
    return view[:, :k].cpu().numpy(), bh.spmv_changed if want_changed else None, got_next


def check(bh, name, D, fidx, F, Y, mask=None, complement=False, gap=0, values=True, ref=None, optional=False, what=""):
    """one call against the reference (computed here unless given): Y's bits, the count, the list; with `optional` also
    with each of the optional outputs left out"""
    if ref is None:
        ref = pr.push_semiring(name, D.m, D.n, D.Gp, D.Gj, D.Gx if values else None, fidx, F, Y, mask, complement, D.dtype)
    tag = (what, name, Y.shape[1], gap, complement)
    for want_next, want_changed in ((True, True), (False, True), (True, False), (False, False)) if optional else ((True, True),):
        got, changed, nxt = run(bh, name, D, fidx, F, Y, mask, complement, gap, values, want_next, want_changed, what=what)
        assert srf.same_bits(got, ref[0]), (tag, np.argwhere(bits(got) != bits(ref[0]))[:5])
        if want_changed:
            assert changed == ref[1], (tag, changed, ref[1])
        if want_next:
            assert nxt.dtype == np.int32 and np.array_equal(nxt, ref[2]), (tag, nxt[:8], ref[2][:8])
    return ref


def values_for(name, count, rng):
    """edge values (zeros of both signs, infinities) a semiring can take without turning everything into NaN; NaNs are
    placed by hand by the tests that want them"""
    if name == "plus_pair":
        return rng.integers(-4, 5, count).astype(np.float64)
    return srf.edge_values(rng, count, plus_safe=name in ("min_plus", "max_plus"))


def random_mask(n, k, seed):
    """per element: 0, -0 (not set); a number, NaN (set)"""
    rng = np.random.default_rng(seed)
    return rng.choice(np.array([0.0, -0.0, 2.0, np.nan, -1.0, 0.0]), (n, k))


# ---------------------------------------------------------------- the matrices
DEGREES = (0, 1, 2, 31, 32, 33, 64, 65, 1024, 1025, 5000)
N_COLS = 1100                                                       # not a multiple of 64: the row map's last word


@functools.lru_cache(maxsize=None)
def ladder():
    """G with n = 1100 columns and 40 rows: every special degree once among short rows that are not pushed.  The 5000-entry
    row draws all its columns from three targets (the contention case, exact duplicates included); the other rows' columns
    are in no order, with duplicates where there is room.  (rows, n, Gp, Gj, the special rows in DEGREES' order)"""
    rng = np.random.default_rng(141)
    lens = rng.integers(0, 9, 40)
    special = rng.choice(40, len(DEGREES), replace=False)
    lens[special] = DEGREES
    Gp = np.zeros(41, np.int32)
    np.cumsum(lens, out=Gp[1:])
    Gj = np.concatenate([rng.integers(0, N_COLS, L) for L in lens]).astype(np.int32)
    hub = special[-1]
    Gj[Gp[hub]:Gp[hub + 1]] = rng.choice(np.array([3, 700, N_COLS - 1]), 5000)
    Gj[Gp[special[8]]] = N_COLS - 1                                 # the last column from another row as well
    return 40, N_COLS, Gp, Gj, tuple(int(s) for s in special)


@functools.lru_cache(maxsize=None)
def ladder_dev(name, dtype):
    m, n, Gp, Gj, special = ladder()
    Gx = values_for(name, len(Gj), np.random.default_rng(143))
    return Dev(m, n, (Gp, Gj, Gx), dtype)


@functools.lru_cache(maxsize=None)
def random_dev(name, dtype):
    """2000 x 2000, 0 .. 12 entries a row: the whole of it is the frontier (8 workgroups of the degree pass)"""
    rng = np.random.default_rng(151)
    m = n = 2000
    lens = rng.integers(0, 13, m)
    Gp = np.zeros(m + 1, np.int32)
    np.cumsum(lens, out=Gp[1:])
    Gj = rng.integers(0, n, Gp[-1]).astype(np.int32)
    return Dev(m, n, (Gp, Gj, values_for(name, len(Gj), np.random.default_rng(152))), dtype)


def dense_for(name, rows, k, seed, nan_at=None):
    rng = np.random.default_rng(seed)
    V = values_for(name, rows * k, rng).reshape(rows, k)
    if nan_at is not None and V.size > nan_at and name != "plus_pair":
        V.flat[nan_at] = np.nan
    return V


def y_for(name, n, k, seed):
    """Y on entry: identities, numbers, infinities, zeros of both signs and a few NaNs"""
    rng = np.random.default_rng(seed)
    pick = rng.integers(0, 8, (n, k))
    base = values_for(name, n * k, rng).reshape(n, k)
    return np.select([pick <= 2, pick == 3, pick == 4], [np.full((n, k), srf.identity(name)), np.full((n, k), -0.0),
                                                         np.full((n, k), np.nan if name != "plus_pair" else 3.0)], base)


def test_the_ladder_holds_every_degree():
    m, n, Gp, Gj, special = ladder()
    lens = np.diff(Gp)
    assert [int(lens[s]) for s in special] == list(DEGREES) and n % 64 != 0
    hub = Gj[Gp[special[-1]]:Gp[special[-1] + 1]]
    assert set(hub) == {3, 700, n - 1} and len(hub) == 5000
    assert 5000 + 4 < 2 ** 24                                        # plus_pair's counts are exact in both builds


# ---------------------------------------------------------------- every semiring, every k
@pytest.mark.parametrize("k", (1, 3, 4, 16))
@pytest.mark.parametrize("name", NAMES)
def test_the_ladder_against_the_reference(hd, name, k):
    bh, dtype = hd
    D = ladder_dev(name, dtype)
    special = list(ladder()[4])
    fidx = special[::-1] + [special[3]]                              # every special row, the 31-entry one twice
    F = dense_for(name, len(fidx), k, 160 + k, nan_at=2 * k)
    Y, M = y_for(name, D.n, k, 170 + k), random_mask(D.n, k, 180 + k)
    gap = 0 if k == 1 else 3
    optional = k in (1, 3)
    check(bh, name, D, fidx, F, Y, gap=gap, optional=optional, what="ladder")
    assert families(bh) == (FAMILIES - {"push_compact"} if optional else FAMILIES)   # (optional: the last call asked for no list)
    check(bh, name, D, fidx, F, Y, M, False, gap=3, what="ladder masked")       # (k = 1 with leading dimensions above k too)
    assert families(bh) == FAMILIES
    check(bh, name, D, fidx, F, Y, M, True, gap=3, values=(k != 3), what="ladder complement")


@pytest.mark.parametrize("name", NAMES)
def test_a_whole_matrix_as_the_frontier(hd, name):
    bh, dtype = hd
    D = random_dev(name, dtype)
    rng = np.random.default_rng(190)
    fidx = rng.permutation(D.m)                                      # nf = m, in no order
    for k in (1, 4):
        F, Y = dense_for(name, D.m, k, 191 + k, nan_at=5), y_for(name, D.n, k, 193 + k)
        ref = check(bh, name, D, fidx, F, Y, gap=k - 1, what="whole matrix")
        assert ref[1] > 0 and 0 < len(ref[2]) <= D.n


def test_small_frontiers(hd):
    bh, dtype = hd
    name = "min_plus"
    D = ladder_dev(name, dtype)
    special = ladder()[4]
    Y = y_for(name, D.n, 2, 201)
    # nf = 0: nothing runs but the compaction of an empty map; Y keeps its bits
    ref = check(bh, name, D, [], np.zeros((0, 2)), Y, optional=True, what="nf = 0")
    assert ref[1] == 0 and len(ref[2]) == 0
    # nf = 1: the empty row, a single entry, the hub
    for s in (special[0], special[1], special[-1]):
        check(bh, name, D, [s], dense_for(name, 1, 2, 202), Y, optional=True, what="nf = 1")
    # one vertex many times
    check(bh, "plus_pair", ladder_dev("plus_pair", dtype), [special[4]] * 70, np.zeros((70, 2)), y_for("plus_pair", D.n, 2, 203),
          what="one vertex 70 times")
    # empty matrices
    Z = Dev(0, 50, (np.zeros(1, np.int32), np.zeros(0, np.int32), np.zeros(0)), dtype)
    check(bh, name, Z, [], np.zeros((0, 1)), y_for(name, 50, 1, 204), what="m = 0")
    Z = Dev(30, 0, (np.zeros(31, np.int32), np.zeros(0, np.int32), np.zeros(0)), dtype)
    check(bh, name, Z, [3, 4, 3], np.ones((3, 1)), np.zeros((0, 1)), what="n = 0")


# ---------------------------------------------------------------- special values
@pytest.mark.parametrize("name", NAMES)
def test_special_values(hd, name):
    """+-0, NaN and +-Inf in G, F and Y, each against each, for every semiring (Inf - Inf and 0 * Inf are NaN products)"""
    bh, dtype = hd
    vals = np.array([0.0, -0.0, np.nan, np.inf, -np.inf, 1.5, -2.0])
    nv = len(vals)
    # G: row a holds one entry per value of Y, all of value vals[a]: row a pushes vals[a] (x) f onto every kind of Y
    Gp = np.arange(nv + 1, dtype=np.int32) * nv
    Gj = np.tile(np.arange(nv, dtype=np.int32), nv)
    Gx = np.repeat(vals, nv)
    D = Dev(nv, nv, (Gp, Gj, Gx), dtype)
    Y = np.repeat(vals[:, None], nv, axis=1)                        # Y(v, c) = vals[v]; column c pushes F = vals[c]
    for a in range(nv):
        F = vals[None, :].copy()
        check(bh, name, D, [a], F, Y, what="special values, g = %r" % vals[a])
    check(bh, name, D, list(range(nv)), np.repeat(vals[None, :], nv, axis=0), Y, what="special values, all at once")


# ---------------------------------------------------------------- repeatable
@pytest.mark.parametrize("name", ("min_plus", "max_times", "or_and", "plus_pair"))
def test_the_contention_case_twice(hd, name):
    bh, dtype = hd
    D = ladder_dev(name, dtype)
    special = ladder()[4]
    fidx = [special[-1], special[8], special[-1]]                    # the hub twice: 10000 updates of three rows of Y
    k = 4
    F, Y = dense_for(name, 3, k, 211), y_for(name, D.n, k, 212)
    a = run(bh, name, D, fidx, F, Y)
    b = run(bh, name, D, fidx, F, Y)
    assert np.array_equal(bits(a[0]), bits(b[0])) and a[1] == b[1] and np.array_equal(a[2], b[2])
    ref = pr.push_semiring(name, D.m, D.n, D.Gp, D.Gj, D.Gx, fidx, F, Y, dtype=dtype)
    assert srf.same_bits(a[0], ref[0]) and a[1] == ref[1] and np.array_equal(a[2], ref[2])


# ---------------------------------------------------------------- refusals
def test_device_refusals_come_before_the_dependent_read(hd):
    bh, dtype = hd
    name = "min_plus"
    m, n, Gp, Gj, special = ladder()
    good = ladder_dev(name, dtype)
    k = 3
    Y = y_for(name, n, k, 221)
    pushed, other = special[5], special[6]                           # 33 and 64 entries
    F = dense_for(name, 2, k, 222)
    # fidx = m and -1: never an index into the row pointer
    for bad in (m, -1):
        assert pr.invalid(m, n, Gp, Gj, 2, [pushed, bad]) == "fidx out of range"
        run(bh, name, good, [pushed, bad], F, Y, gap=2, want=INV, what="fidx %d" % bad)
    # a decreasing pointer pair, a pointer beyond nnzG, a column = n and -1: refused in a pushed row, not looked at elsewhere
    pd = Gp.copy()
    pd[other], pd[other + 1] = Gp[other + 1], Gp[other]
    pb = Gp.copy()
    pb[other + 1] = len(Gj) + 5
    for word, p, j in (("bad row pointer in a pushed row", pd, Gj), ("bad row pointer in a pushed row", pb, Gj)):
        D = Dev(m, n, (p, j, good.Gx), dtype)
        assert pr.invalid(m, n, p, j, 2, [pushed, other]) == word and pr.invalid(m, n, p, j, 1, [pushed]) is None
        run(bh, name, D, [pushed, other], F, Y, gap=2, want=INV, what=word)
        check(bh, name, D, [pushed], F[:1], Y, gap=2, what=word + ", row not pushed")
    for col in (n, -1):
        j = Gj.copy()
        j[Gp[other] + 40] = col
        D = Dev(m, n, (Gp, j, good.Gx), dtype)
        assert pr.invalid(m, n, Gp, j, 2, [pushed, other]) == "column out of range in a pushed row"
        run(bh, name, D, [pushed, other], F, Y, gap=2, want=INV, what="column %d" % col)
        check(bh, name, D, [pushed], F[:1], Y, gap=2, what="column %d, row not pushed" % col)
    # the handle still answers a valid call
    check(bh, name, good, [pushed, other], F, Y, what="after the refusals")


def test_host_side_refusals_leave_y_untouched(hd):
    bh, dtype = hd
    D = ladder_dev("min_plus", dtype)
    m, n, k, ld = D.m, D.n, 4, 6
    t = tdt(dtype)
    nf = 5
    fidx = up(np.arange(nf), np.int32)
    F = torch.ones((nf, ld), dtype=t).cuda()
    M = torch.ones((n, ld), dtype=t).cuda()
    Y = torch.full((n * ld + PAD,), SENTINEL, dtype=t).cuda()
    nxt = torch.full((n + PAD,), -5, dtype=torch.int32).cuda()
    torch.cuda.synchronize()
    Gp, Gj, Gx = D.d

    def push(sr_=1, m=m, n=n, nnz=D.nnz, Gx=Gx, Gp=Gp, Gj=Gj, nf=nf, fidx=fidx, k=k, F=F, ldF=ld, flags=0, M=M, ldM=ld, Y=Y, ldY=ld,
             nxt=nxt):
        return dense.csr_push_semiring_raw_device(bh, sr_, m, n, nnz, Gx, Gp, Gj, nf, fidx, k, F, ldF, flags, M, ldM, Y, ldY, nxt)

    refused = {
        "negative size": (push(m=-1), push(n=-1), push(nnz=-1), push(nf=-1)),
        "k < 1": (push(k=0), push(k=-3)),
        "ldF < k": (push(ldF=k - 1),),
        "ldY < k": (push(ldY=k - 1),),
        "NULL rowPtrG": (push(Gp=None),),
        "NULL colIndG": (push(Gj=None),),
        "NULL fidx": (push(fidx=None),),
        "NULL F": (push(F=None),),
        "NULL Y": (push(Y=None),),
        "unknown semiring": (push(sr_=8), push(sr_=-1), push(sr_=100)),
        "plus_times": (push(sr_=_lib.BHS_SR_PLUS_TIMES), push(sr_="plus_times")),
        "unknown flag": (push(flags=_lib.BHS_MV_ACCUM), push(flags=4), push(flags=CMP | 8), push(flags=-1)),
        "ldM < k": (push(ldM=k - 1),),
        "complement without a mask": (push(flags=CMP, M=None),),
        "an output overlaps an input": (push(Y=F), push(Y=Gx), push(Y=M), push(F=Y[k:]), push(M=Y[k:]), push(nxt=Gj), push(nxt=Gp),
                                        push(nxt=fidx), push(fidx=nxt[3:]), push(nxt=Y.view(torch.int32)[:n])),
    }
    assert sorted(refused) == sorted(pr.HOST_REFUSALS)
    for word, codes in refused.items():
        assert all(c == INV for c in codes), (word, codes)
    assert bool((Y == SENTINEL).all()) and bool((nxt == -5).all()), "an output written by a refused call"
    # what is legal: a leading dimension of M below k without a mask, a NULL list and a NULL F for an empty frontier
    assert push(M=None, ldM=0) == 0 and push(nf=0, fidx=None, F=None) == 0 and bh.spmv_changed == 0 and bh.push_next == 0
    assert dense.csr_push_semiring_raw_device(bhsparse(dtype), 1, 0, 0, 0, None, None, None, 0, None, 1, None, 1, 0, None, 1, None, 1,
                                              None) == _lib.BHS_ERR_NOT_READY


def test_refused_between_symbolic_and_finish():
    from helpers import random_csr
    m = n = 300
    A = random_csr(m, n, 0.05, np.random.default_rng(34))
    D = Dev(m, n, A, np.float64)
    fidx, F = up(np.arange(10), np.int32), torch.ones(10, dtype=torch.float64).cuda()
    y = torch.full((n + PAD,), SENTINEL, dtype=torch.float64).cuda()
    bh = new_handle()
    try:
        assert bh.initData_device(m, n, n, D.nnz, D.d[2], D.d[0], D.d[1], D.nnz, D.d[2], D.d[0], D.d[1]) == 0
        assert bh.spgemm_symbolic() == 0
        call = lambda: dense.csr_push_semiring_raw_device(bh, "min_plus", m, n, D.nnz, D.d[2], D.d[0], D.d[1], 10, fidx, 1, F, 1, 0,   # noqa: E731
                                                          None, 1, y, 1, None)
        assert call() == INV and bool((y == SENTINEL).all())
        assert bh.spgemm_numeric(0, m) == 0 and bh.spgemm_finish() == 0
        y[:n] = float("inf")
        torch.cuda.synchronize()
        assert call() == 0
        ref = pr.push_semiring("min_plus", m, n, D.Gp, D.Gj, D.Gx, np.arange(10), np.ones((10, 1)), np.full((n, 1), np.inf))
        assert srf.same_bits(y[:n].cpu().numpy(), ref[0][:, 0]) and bh.spmv_changed == ref[1] and bool((y[n:] == SENTINEL).all())
        bh.free_mem()
    finally:
        bh.freePlatform()


# ---------------------------------------------------------------- the handle is left alone
@pytest.mark.parametrize("dtype", DTYPES)
def test_a_push_call_leaves_the_handle_alone(dtype, oracle):
    g = load_golden("p9_12.npz")
    m, kk, n = int(g["m"]), int(g["k"]), int(g["n"])
    rng = np.random.default_rng(15)
    Ap, Aj, Bp, Bj = (np.ascontiguousarray(g[key], np.int32) for key in ("Ap", "Aj", "Bp", "Bj"))
    Ax, Bx = (np.ascontiguousarray(rng.integers(1, 5, len(j)), dtype) for j in (Aj, Bj))
    bh = new_handle(dtype)
    try:
        Cp = np.zeros(m + 1, np.int32)
        assert bh.initData(m, kk, n, len(Aj), Ax, Ap, Aj, len(Bj), Bx, Bp, Bj, Cp) == 0
        assert bh.spgemm() == 0
        nnzC, ptrs, state = bh.get_nnzC(), bh.get_C_device(), bh.get_info("class_state")
        Cj, Cx = np.empty(nnzC, np.int32), np.empty(nnzC, dtype)
        assert bh.get_C(Cj, Cx) == 0
        ref = oracle.spgemm(m, kk, n, Ap, Aj, Ax.astype(np.float64), Bp, Bj, Bx.astype(np.float64))
        assert np.array_equal(Cp, ref[0]) and np.array_equal(Cj, ref[1]) and np.array_equal(Cx, ref[2].astype(dtype))
        D = ladder_dev("min_plus", dtype)
        special = list(ladder()[4])
        check(bh, "min_plus", D, special, dense_for("min_plus", len(special), 3, 231), y_for("min_plus", D.n, 3, 232), what="after a multiply")
        assert bh.get_nnzC() == nnzC and bh.get_C_device() == ptrs and bh.get_info("class_state") == state
        j2, x2 = np.empty(nnzC, np.int32), np.empty(nnzC, dtype)
        assert bh.get_C(j2, x2) == 0
        assert np.array_equal(j2, Cj) and np.array_equal(bits(x2), bits(Cx)) and np.array_equal(bh.get_rowptrC(), Cp)
        # the product itself as G, straight from the device pointers: its first rows push
        fidx = up(np.arange(7), np.int32)
        F = up(np.arange(7.0), dtype)
        y = torch.full((n + PAD,), float("inf"), dtype=tdt(dtype)).cuda()
        torch.cuda.synchronize()
        assert dense.csr_push_semiring_raw_device(bh, "min_plus", m, n, nnzC, ptrs[2], ptrs[0], ptrs[1], 7, fidx, 1, F, 1, 0, None, 1, y, 1,
                                                  None) == 0
        want = pr.push_semiring("min_plus", m, n, Cp, Cj, Cx, np.arange(7), np.arange(7.0), np.full(n, np.inf), dtype=dtype)
        assert srf.same_bits(y[:n].cpu().numpy(), want[0]) and bh.spmv_changed == want[1]
        assert bh.spgemm() == 0 and bh.get_nnzC() == nnzC and bh.get_info("class_state") == state   # a multiply after it: the same C
        assert np.array_equal(bh.get_rowptrC(), ref[0])
        j2, x2 = np.empty(nnzC, np.int32), np.empty(nnzC, dtype)
        assert bh.get_C(j2, x2) == 0 and np.array_equal(j2, ref[1]) and np.array_equal(bits(x2), bits(ref[2].astype(dtype)))
        bh.free_mem()
    finally:
        bh.freePlatform()


# ---------------------------------------------------------------- the tensor call
@pytest.mark.parametrize("dtype", DTYPES)
def test_tensor_call_takes_the_leading_dimensions_from_the_strides(dtype):
    name, k = "max_min", 3
    D = ladder_dev(name, dtype)
    special = list(ladder()[4])
    F, Y, M = dense_for(name, len(special), k, 241), y_for(name, D.n, k, 242), random_mask(D.n, k, 243)
    t = tdt(dtype)
    wideF = torch.full((len(special), k + 3), float("nan"), dtype=t).cuda()
    wideF[:, :k] = up(F, dtype)
    wideM = torch.full((D.n, k + 1), float("nan"), dtype=t).cuda()
    wideM[:, :k] = up(M, dtype)
    wideY = torch.full((D.n, k + 2), SENTINEL, dtype=t).cuda()
    wideY[:, :k] = up(Y, dtype)
    bh = new_handle(dtype)
    try:
        fidx = up(np.array(special), np.int32)
        out, changed, nxt = dense.csr_push_semiring_device(bh, name, D.m, D.n, D.d, fidx, wideF[:, :k], wideY[:, :k], wideM[:, :k], True)
        ref = pr.push_semiring(name, D.m, D.n, D.Gp, D.Gj, D.Gx, special, F, Y, M, True, dtype)
        assert out.data_ptr() == wideY.data_ptr() and changed == ref[1] and nxt.dtype == torch.int32
        assert np.array_equal(nxt.cpu().numpy(), ref[2]) and bh.push_next == len(ref[2])
        assert srf.same_bits(wideY[:, :k].cpu().numpy(), ref[0]) and bool((wideY[:, k:] == SENTINEL).all())
        # vectors are k = 1; without want_list no list comes back
        y = up(Y[:, 0], dtype)
        out, changed, nxt = dense.csr_push_semiring_device(bh, _lib.BHS_SR_MAX_MIN, D.m, D.n, D.d, fidx, up(F[:, 0], dtype), y, want_list=False)
        ref = pr.push_semiring(name, D.m, D.n, D.Gp, D.Gj, D.Gx, special, F[:, 0], Y[:, 0], dtype=dtype)
        assert out.shape == (D.n,) and nxt is None and srf.same_bits(out.cpu().numpy(), ref[0]) and changed == ref[1]
        with pytest.raises(BhsparseError) as ei:
            dense.csr_push_semiring_device(bh, "plus_times", D.m, D.n, D.d, fidx, up(F[:, 0], dtype), y)
        assert ei.value.code == INV
        with pytest.raises(BhsparseError) as ei:
            dense.csr_push_semiring_device(bh, name, D.m, D.n, D.d, up(np.array([D.m]), np.int32), up(F[:1, 0], dtype), y)
        assert ei.value.code == INV
    finally:
        bh.freePlatform()


# ---------------------------------------------------------------- traversals against the pull loops and scipy.sparse.csgraph
def scipy_answers(n, A, sources):
    import scipy.sparse as sp
    from scipy.sparse import csgraph
    G = sp.csr_matrix((A[2], A[1], A[0]), shape=(n, n)).T.tocsr()   # (csgraph reads G[i, j] as an edge i -> j)
    hops = csgraph.shortest_path(G, method="D", unweighted=True, indices=list(sources)).T
    return np.where(np.isfinite(hops), hops + 1, 0.0), csgraph.bellman_ford(G, indices=list(sources)).T


def weighted(Ap, Aj, seed, symmetric=False):
    """weights 1 .. 9 on a pattern without duplicates (symmetric: the same weight both ways)"""
    import scipy.sparse as sp
    n = len(Ap) - 1
    rng = np.random.default_rng(seed)
    G = sp.csr_matrix((rng.integers(1, 10, len(Aj)).astype(np.float64), Aj, Ap), shape=(n, n))
    G.sum_duplicates()
    G.data = np.minimum(G.data, 9.0)
    if symmetric:
        G = G.maximum(G.T).tocsr()
    G.sort_indices()
    return G.indptr.astype(np.int32), G.indices.astype(np.int32), G.data.astype(np.float64)


@functools.lru_cache(maxsize=None)
def graphs():
    """name -> (n, A in the pull form, is A symmetric)"""
    out = {}
    n = 600
    Ap = np.concatenate([[0], np.arange(n)]).astype(np.int32)       # row v pulls from v - 1: the directed path 0 -> 1 -> ..
    out["directed path"] = (n, (Ap, np.arange(n - 1, dtype=np.int32), 1.0 + (np.arange(n - 1) % 7)), False)
    rows = np.concatenate([np.arange(n - 1), np.arange(1, n)])
    cols = np.concatenate([np.arange(1, n), np.arange(n - 1)])
    order = np.lexsort((cols, rows))
    Sp = np.zeros(n + 1, np.int32)
    np.cumsum(np.bincount(rows, minlength=n), out=Sp[1:])
    out["symmetric path"] = (n, weighted(Sp, cols[order].astype(np.int32), 251, True), True)
    Rp, Rj = gallery.roadlike_csr(64, 64)[:2]
    out["roadlike"] = (len(Rp) - 1, weighted(Rp, Rj, 252, True), True)
    n = 3000
    rng = np.random.default_rng(253)
    pairs = np.unique(np.stack([rng.integers(0, n, 3 * n), rng.integers(0, n, 3 * n)], axis=1), axis=0)
    Dp = np.zeros(n + 1, np.int32)
    np.cumsum(np.bincount(pairs[:, 0], minlength=n), out=Dp[1:])
    out["random digraph"] = (n, weighted(Dp, pairs[:, 1].astype(np.int32), 254), False)
    Mp, Mj = gallery.rmat_csr(scale=10)
    out["rmat"] = (1 << 10, weighted(Mp, Mj, 255), False)
    return out


@functools.lru_cache(maxsize=None)
def answers(which, nsrc):
    n, A, sym = graphs()[which]
    sources = [0] if nsrc == 1 else [0, n // 5, n // 2, n - 7, n - 1]
    return sources, scipy_answers(n, A, sources)


@pytest.mark.parametrize("dtype", DTYPES, ids=("f64", "f32"))
@pytest.mark.parametrize("nsrc", (1, 5))
@pytest.mark.parametrize("which", ("directed path", "symmetric path", "roadlike", "random digraph", "rmat"))
def test_frontier_traversals(which, nsrc, dtype):
    n, A, sym = graphs()[which]
    sources, (levels, dist) = answers(which, nsrc)
    dA = (up(A[0], np.int32), up(A[1], np.int32), up(A[2], dtype))
    bh = new_handle(dtype)
    try:
        pull_levels, pull_dist = graph.bfs_levels_device(bh, n, dA, sources), graph.sssp_device(bh, n, dA, sources)
        assert np.array_equal(pull_levels.cpu().numpy(), levels.astype(dtype)) and np.array_equal(pull_dist.cpu().numpy(), dist.astype(dtype))
        At = dA if sym else None                                     # (None: the handle transposes)
        for push_below in (0, 4, float("inf")):
            got, steps, ms, pushes = graph._bfs_frontier(bh, n, dA, sources, At, push_below)
            assert torch.equal(got, pull_levels), (which, push_below)
            assert (pushes == 0) if push_below == 0 else (pushes == steps) if push_below == float("inf") else pushes > 0
            if push_below == float("inf") and which.endswith("path") and nsrc == 1:
                assert steps == int(levels.max()) == 600             # a library call a level: the last one finds nothing
            got, rounds, ms, pushes = graph._sssp_frontier(bh, n, dA, sources, At, None, push_below)
            assert torch.equal(got, pull_dist), (which, push_below)
            assert (pushes == 0) if push_below == 0 else (pushes == rounds) if push_below == float("inf") else pushes > 0
        assert torch.equal(graph.bfs_levels_frontier_device(bh, n, dA, sources), pull_levels)      # the defaults
        assert torch.equal(graph.sssp_frontier_device(bh, n, dA, sources), pull_dist)
    finally:
        bh.freePlatform()


def test_a_negative_cycle_raises_and_the_conveniences_run():
    Ap, Aj, Ax = np.array([0, 1, 2, 3], np.int32), np.array([2, 0, 1], np.int32), np.array([1.0, 1.0, -3.0])
    for push_below in (0, float("inf")):
        with pytest.raises(BhsparseError):
            graph.sssp_frontier_csr(3, Ap, Aj, Ax, 0, push_below=push_below)
    dist, info = graph.sssp_frontier_csr(3, Ap, Aj, np.abs(Ax), 0, push_below=float("inf"), value_dtype=np.float32)
    assert dist[:, 0].tolist() == [0.0, 1.0, 4.0] and info["steps"] == 3 == info["push_steps"] and info["ms"] > 0
    levels, info = graph.bfs_levels_frontier_csr(3, Ap, Aj, None, [1, 2], push_below=float("inf"))
    assert levels.tolist() == [[3.0, 2.0], [1.0, 3.0], [2.0, 1.0]] and info["steps"] == 3 == info["push_steps"]
    assert {s["name"] for s in info["kernels"] if s["launches"] > 0} == FAMILIES


def test_cpp_demo_runs():
    demo_dir = os.path.join(ROOT, "tests", "push")
    subprocess.check_call(["make", "-C", demo_dir, "-s"])
    out = subprocess.run([os.path.join(demo_dir, "push_demo")], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "push bfs / sssp on a path of 12 vertices, 22 entries: PASS" in out.stdout
