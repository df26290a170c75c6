"""The transpose (bhs_csr_transpose_device, bhs_csr_transpose_values_device) and the Galerkin product built on it, on the GPU,
both builds.

Reference: tests/transposeref.py, the stable transpose of include/bhsparse_hip.h restated in numpy.  The transpose moves
values and computes nothing, so rowPtrT, colIndT, perm and the values' bit patterns are compared bit for bit.  The Galerkin
product is compared bit for bit with the oracle's (P^T·A)·P on integer values whose partial sums stay below 2^24: exact in
float and double whatever the association."""
import os
import subprocess

import numpy as np
import pytest
import torch

from conftest import ROOT, load_golden
from helpers import random_csr
import transposeref as tr

from benchmark_spgemm_using_csr_amd import _lib, gallery
from benchmark_spgemm_using_csr_amd.facade import (BHSPARSE_HIP, NUM_PLATFORMS, BhsparseError, bhsparse, csr_transpose,
                                                   galerkin_csr, select_spec)

pytestmark = pytest.mark.gpu

DTYPES = (np.float64, np.float32)
INV = _lib.BHS_ERR_INVALID_ARG
FILL = ("transpose_short", "transpose_wave", "transpose_long")


# ---------------------------------------------------------------- helpers
def new_handle(dtype=np.float64, options=None):
    plats = [False] * NUM_PLATFORMS
    plats[BHSPARSE_HIP] = True
    bh = bhsparse(value_dtype=dtype)
    assert bh.initPlatform(plats) == 0
    for key, val in (options or {}).items():
        assert bh.set_option(key, val) == 0, key
    return bh


def bits(x):
    x = np.ascontiguousarray(x)
    return x.view(np.uint64 if x.dtype == np.float64 else np.uint32)


def up(a, dt):
    return torch.from_numpy(np.ascontiguousarray(a, dt).copy()).cuda()


def expected_families(Tp, nnz):
    """What bhs_get_kernel_stats must name after a transpose whose T has this row pointer."""
    if nnz == 0 or len(Tp) <= 1:
        return {"transpose_count"}
    lens = np.diff(np.asarray(Tp, np.int64))
    fam = {"transpose_count", "transpose_scan", "transpose_scatter"}
    if np.any((lens >= 1) & (lens <= 32)):
        fam.add("transpose_short")
    if np.any((lens > 32) & (lens <= 1024)):
        fam.add("transpose_wave")
    if np.any(lens > 1024):
        fam.add("transpose_long")
    return fam


def check_transpose(bh, m, n, X, dtype, what="", values=True):
    """The transpose of X on the device against transposeref: bit for bit, nothing written past the end of T, the kernel
    families that must have run did.  Returns the reference."""
    Xp, Xj, Xx = X
    Xx = np.ascontiguousarray(Xx, dtype) if values else None
    nnz = len(Xj)
    ref = tr.transpose(m, n, Xp, Xj, Xx)
    dXp, dXj = up(Xp, np.int32), up(Xj, np.int32)
    dXx = up(Xx, dtype) if values else None
    tdt = torch.float32 if np.dtype(dtype) == np.dtype(np.float32) else torch.float64
    Tp = torch.full((n + 1 + 16,), -7, dtype=torch.int32).cuda()
    Tj = torch.full((nnz + 64,), -7, dtype=torch.int32).cuda()
    pm = torch.full((nnz + 64,), -7, dtype=torch.int32).cuda()
    Tx = torch.full((nnz + 64,), -7.0, dtype=tdt).cuda() if values else None
    torch.cuda.synchronize()
    err = bh.csr_transpose_raw_device(m, n, nnz, dXx, dXp, dXj, Tp, Tj, Tx, pm)
    assert err == 0, (what, err)
    fam = {s["name"] for s in bh.kernel_stats() if s["launches"] > 0}
    assert bool((Tp[n + 1:] == -7).all()) and bool((Tj[nnz:] == -7).all()) and bool((pm[nnz:] == -7).all()), (what, "written past the end")
    assert np.array_equal(Tp[:n + 1].cpu().numpy(), ref[0]), (what, "rowPtrT differs")
    assert np.array_equal(Tj[:nnz].cpu().numpy(), ref[1]), (what, "colIndT differs")
    assert np.array_equal(pm[:nnz].cpu().numpy(), ref[3]), (what, "perm differs")
    if values:
        assert bool((Tx[nnz:] == -7).all()), (what, "written past the end of valT")
        got = Tx[:nnz].cpu().numpy()
        assert got.dtype == np.dtype(dtype) and np.array_equal(bits(got), bits(ref[2])), (what, "valT differs")
    assert fam == expected_families(ref[0], nnz), (what, fam)
    assert bh.transpose_ms >= 0.0
    return ref


def shuffled_rows(Xp, Xj, rng):
    """the same rows, every row's entries in a random order"""
    Xj = np.array(Xj, np.int32)
    for i in range(len(Xp) - 1):
        rng.shuffle(Xj[Xp[i]:Xp[i + 1]])
    return Xj


def special_values(count, rng):
    v = rng.standard_normal(count)
    pick = rng.random(count)
    v[pick < 0.08] = np.nan
    v[(pick >= 0.08) & (pick < 0.14)] = np.inf
    v[(pick >= 0.14) & (pick < 0.20)] = -np.inf
    v[(pick >= 0.20) & (pick < 0.30)] = 0.0
    v[(pick >= 0.30) & (pick < 0.40)] = -0.0
    return v


# ---------------------------------------------------------------- shapes
@pytest.mark.parametrize("dtype", DTYPES)
def test_stencils_take_the_lds_window(dtype):
    bh = new_handle(dtype)
    try:
        for name, dims in (("poisson27pt", (12, 12, 12)), ("poisson5pt", (64, 64, 1))):
            rp, col = gallery.poisson_csr(name, *dims)
            m = len(rp) - 1
            # 256 consecutive rows reach nx + 1 (2-D) or nx ny + nx + 1 columns to either side: inside the window of 8192
            reach = dims[0] + 1 if dims[2] == 1 else dims[0] * dims[1] + dims[0] + 1
            assert 2 * reach + 256 <= 8192
            ref = check_transpose(bh, m, m, (rp, col, gallery.fill_values(len(col))), dtype, name)
            assert np.array_equal(ref[0], rp) and np.array_equal(ref[1], col)      # (a symmetric pattern)
    finally:
        bh.freePlatform()


@pytest.mark.parametrize("dtype", DTYPES)
def test_rectangular_and_cage4(dtype):
    g = load_golden("rect_rand.npz")
    c4 = load_golden("cage4_sq.npz")
    bh = new_handle(dtype)
    try:
        check_transpose(bh, int(g["m"]), int(g["k"]), (g["Ap"], g["Aj"], g["Ax"]), dtype, "rect A")
        check_transpose(bh, int(g["k"]), int(g["n"]), (g["Bp"], g["Bj"], g["Bx"]), dtype, "rect B")
        m = int(c4["m"])
        check_transpose(bh, m, m, (c4["Ap"], c4["Aj"], c4["Ax"]), dtype, "cage4")
        check_transpose(bh, 1, 5000, (np.array([0, 3], np.int32), np.array([4999, 0, 17], np.int32), np.array([1.0, 2.0, 3.0])),
                        dtype, "one wide row")
    finally:
        bh.freePlatform()


@pytest.mark.parametrize("dtype", DTYPES)
def test_uniform_random_overflows_the_window(dtype):
    rp, col = gallery.uniform_csr(n=1 << 16, per_row=8)
    m = len(rp) - 1
    span = np.array([col[rp[i]:rp[min(i + 256, m)]].max() - col[rp[i]:rp[min(i + 256, m)]].min() for i in range(0, m, 256)])
    assert np.all(span >= 8192)                                     # every workgroup is on the global-atomic path
    rng = np.random.default_rng(5)
    bh = new_handle(dtype)
    try:
        check_transpose(bh, m, m, (rp, col, rng.standard_normal(len(col))), dtype, "uniform")
    finally:
        bh.freePlatform()


@pytest.mark.parametrize("dtype", DTYPES)
def test_power_law_reaches_every_bin(dtype):
    rp, col = gallery.powerlaw_csr(30000, 30000, 300000, 6000)
    m = len(rp) - 1
    rng = np.random.default_rng(6)
    val = rng.standard_normal(len(col))
    bh = new_handle(dtype)
    try:
        ref = check_transpose(bh, m, m, (rp, col, val), dtype, "powerlaw")
        # its transpose as X: T is the gallery matrix itself, hub rows of 6000 entries (keys beyond the LDS, in scratch)
        Yp, Yj, Yx = ref[0], ref[1], np.asarray(ref[2], np.float64)
        ref2 = check_transpose(bh, m, m, (Yp, Yj, Yx), dtype, "powerlaw^T")
        lens = np.diff(ref2[0].astype(np.int64))
        assert lens.max() > 4096 and np.any(lens <= 32) and np.any((lens > 32) & (lens <= 1024))
        assert np.array_equal(ref2[0], rp) and np.array_equal(ref2[1], col)
    finally:
        bh.freePlatform()


@pytest.mark.parametrize("dtype", DTYPES)
def test_a_hub_column_of_200000_entries(dtype):
    m, n = 200000, 64
    rng = np.random.default_rng(7)
    other = rng.integers(1, n, m).astype(np.int32)
    first = rng.random(m) < 0.5                                     # the hub entry first or second in its row
    col = np.empty(2 * m, np.int32)
    col[0::2] = np.where(first, 0, other)
    col[1::2] = np.where(first, other, 0)
    rp = (2 * np.arange(m + 1)).astype(np.int32)
    bh = new_handle(dtype)
    try:
        ref = check_transpose(bh, m, n, (rp, col, rng.standard_normal(2 * m)), dtype, "hub column")
        assert ref[0][1] == m
    finally:
        bh.freePlatform()


@pytest.mark.parametrize("dtype", DTYPES)
def test_unsorted_rows_duplicates_and_special_values(dtype):
    rng = np.random.default_rng(8)
    m, n = 3000, 700
    lens = rng.integers(0, 90, m)
    lens[::97] = 1500                                               # rows longer than n columns: duplicates for certain
    rp = np.zeros(m + 1, np.int64)
    np.cumsum(lens, out=rp[1:])
    col = rng.integers(0, n, rp[-1]).astype(np.int32)               # (with replacement: duplicate pairs, no order)
    col[rng.random(len(col)) < 0.3] = 5                             # a long T row full of duplicates
    val = special_values(len(col), rng)
    bh = new_handle(dtype)
    try:
        ref = check_transpose(bh, m, n, (rp.astype(np.int32), col, val), dtype, "unsorted + duplicates")
        # stable: inside a T row the positions ascend
        starts = np.zeros(len(col), bool)
        starts[ref[0][:-1][ref[0][:-1] < len(col)]] = True
        assert np.all((np.diff(ref[3].astype(np.int64)) > 0) | starts[1:])
    finally:
        bh.freePlatform()


@pytest.mark.parametrize("dtype", DTYPES)
def test_empty_matrices(dtype):
    z = np.zeros(0)
    zi = np.zeros(0, np.int32)
    bh = new_handle(dtype)
    try:
        for m, n in ((0, 0), (0, 5), (5, 0), (7, 3), (3, 20000)):
            check_transpose(bh, m, n, (np.zeros(m + 1, np.int32), zi, z), dtype, "empty %d x %d" % (m, n))
        check_transpose(bh, 4, 4, (np.array([0, 0, 2, 2, 2], np.int32), np.array([3, 0], np.int32), np.array([1.0, 2.0])), dtype,
                        "mostly empty")
    finally:
        bh.freePlatform()


def test_pattern_only():
    rng = np.random.default_rng(9)
    rp, col, _ = random_csr(500, 300, 0.05, rng)
    bh = new_handle(np.float64)
    try:
        check_transpose(bh, 500, 300, (rp, shuffled_rows(rp, col, rng), None), np.float64, "pattern only", values=False)
        Tp, Tj, Tx, pm = bh.csr_transpose_device(500, 300, (up(rp, np.int32), up(col, np.int32), None))
        assert Tx is None and pm is None
        ref = tr.transpose(500, 300, rp, col)
        assert np.array_equal(Tp.cpu().numpy(), ref[0]) and np.array_equal(Tj.cpu().numpy(), ref[1])
        # values asked for without values given
        t = torch.zeros(len(col), dtype=torch.float64).cuda()
        ti = torch.zeros(len(col) + 301, dtype=torch.int32).cuda()
        assert bh.csr_transpose_raw_device(500, 300, len(col), None, up(rp, np.int32), up(col, np.int32), ti[:301], ti[301:], t,
                                           None) == INV
    finally:
        bh.freePlatform()


# ---------------------------------------------------------------- perm and the values-only call
@pytest.mark.parametrize("dtype", DTYPES)
def test_perm_revalues_the_pattern(dtype):
    rng = np.random.default_rng(10)
    bh = new_handle(dtype)
    try:
        for what, (m, n, rp, col) in (("random", (2000, 1500) + random_csr(2000, 1500, 0.01, rng)[:2]),
                                      ("p27", (1728, 1728) + tuple(gallery.poisson_csr("poisson27pt", 12, 12, 12))),
                                      ("odd", (3, 4, np.array([0, 2, 3, 5], np.int32), np.array([3, 1, 1, 0, 3], np.int32)))):
            nnz = len(col)
            v1 = np.ascontiguousarray(special_values(nnz, rng), dtype)
            dX = (up(rp, np.int32), up(col, np.int32), up(v1, dtype))
            Tp, Tj, Tx, pm = bh.csr_transpose_device(m, n, dX, perm=True)
            assert bool((dX[2][pm.long()].view(torch.int64 if dtype == np.float64 else torch.int32) ==
                         Tx.view(torch.int64 if dtype == np.float64 else torch.int32)).all()), what
            v2 = np.ascontiguousarray(special_values(nnz, rng), dtype)
            dX[2].copy_(torch.from_numpy(v2))
            for offset in (0, 1):                                   # (valT 16-byte aligned, and not)
                buf = torch.full((nnz + 8,), -7.0, dtype=dX[2].dtype).cuda()
                out = bh.csr_transpose_values_device(dX[2], pm, buf[offset:offset + nnz])
                assert {s["name"] for s in bh.kernel_stats() if s["launches"] > 0} == {"transpose_values"}
                fresh = tr.transpose(m, n, rp, col, v2)
                assert np.array_equal(bits(out.cpu().numpy()), bits(fresh[2])), (what, offset)
                assert bool((buf[:offset] == -7).all()) and bool((buf[offset + nnz:] == -7).all()), (what, offset)
            Tp2, Tj2, Tx2, _ = bh.csr_transpose_device(m, n, dX)
            assert torch.equal(Tp, Tp2) and torch.equal(Tj, Tj2)
            assert np.array_equal(bits(Tx2.cpu().numpy()), bits(out.cpu().numpy())), what
    finally:
        bh.freePlatform()


@pytest.mark.parametrize("dtype", DTYPES)
def test_out_of_range_perm_is_rejected(dtype):
    nnz = 5000
    rng = np.random.default_rng(11)
    val = up(rng.standard_normal(nnz), dtype)
    bh = new_handle(dtype)
    try:
        good = rng.permutation(nnz).astype(np.int32)
        out = bh.csr_transpose_values_device(val, up(good, np.int32))
        assert torch.equal(out, val[torch.from_numpy(good).long().cuda()])
        for where, bad in ((0, nnz), (nnz - 1, -1), (1234, 2 ** 31 - 1), (77, -2 ** 31)):
            p = good.copy()
            p[where] = bad
            with pytest.raises(BhsparseError) as e:
                bh.csr_transpose_values_device(val, up(p, np.int32))
            assert e.value.code == INV
        # the handle works on
        out = bh.csr_transpose_values_device(val, up(good, np.int32))
        assert torch.equal(out, val[torch.from_numpy(good).long().cuda()])
        assert bh._lib.bhs_csr_transpose_values_device(bh._h, 0, None, None, None, None) == 0
    finally:
        bh.freePlatform()


# ---------------------------------------------------------------- invalid input
@pytest.mark.parametrize("dtype", DTYPES)
def test_invalid_x_is_rejected_and_nothing_is_written(dtype):
    rng = np.random.default_rng(12)
    m, n = 900, 400
    rp, col, val = random_csr(m, n, 0.03, rng)
    nnz = len(col)
    cases = {}
    p = rp.copy(); p[0] = 1
    cases["rowPtrX[0] != 0"] = (p, col)
    p = rp.copy(); p[300], p[301] = rp[301] + 2, rp[300]
    cases["decreasing rowPtrX"] = (p, col)
    p = rp.copy(); p[-1] = nnz - 1
    cases["rowPtrX[m] != nnzX"] = (p, col)
    p = rp.copy(); p[-1] = nnz + 5
    cases["rowPtrX[m] beyond nnzX"] = (p, col)
    c = col.copy(); c[nnz // 2] = n
    cases["column == n"] = (rp, c)
    c = col.copy(); c[7] = -1
    cases["column < 0"] = (rp, c)
    bh = new_handle(dtype)
    try:
        tdt = torch.float32 if dtype == np.float32 else torch.float64
        for what, (P, J) in cases.items():
            Tp = torch.full((n + 1,), -7, dtype=torch.int32).cuda()
            Tj = torch.full((nnz,), -7, dtype=torch.int32).cuda()
            pm = torch.full((nnz,), -7, dtype=torch.int32).cuda()
            Tx = torch.full((nnz,), -7.0, dtype=tdt).cuda()
            torch.cuda.synchronize()
            err = bh.csr_transpose_raw_device(m, n, nnz, up(val, dtype), up(P, np.int32), up(J, np.int32), Tp, Tj, Tx, pm)
            assert err == INV, (what, err)
            assert bool((Tp == -7).all()) and bool((Tj == -7).all()) and bool((pm == -7).all()) and bool((Tx == -7).all()), what
        check_transpose(bh, m, n, (rp, col, val), dtype, "after the refusals")
        dX = (up(rp, np.int32), up(col, np.int32), up(val, dtype))
        Tp = torch.zeros(n + 1, dtype=torch.int32).cuda()
        Tj = torch.zeros(nnz, dtype=torch.int32).cuda()
        assert bh.csr_transpose_raw_device(-1, n, nnz, None, dX[0], dX[1], Tp, Tj, None, None) == INV
        assert bh.csr_transpose_raw_device(m, n, nnz, None, dX[0], dX[1], None, Tj, None, None) == INV
        assert bh.csr_transpose_raw_device(m, n, nnz, None, dX[0], dX[1], Tp, dX[1], None, None) == INV      # (T on top of X)
    finally:
        bh.freePlatform()


def test_refused_between_symbolic_and_finish():
    rp, col = gallery.poisson_csr("poisson5pt", 16, 16)
    m = len(rp) - 1
    val = gallery.fill_values(len(col))
    dA = (up(rp, np.int32), up(col, np.int32), up(val, np.float64))
    Tp = torch.zeros(m + 1, dtype=torch.int32).cuda()
    Tj = torch.zeros(len(col), dtype=torch.int32).cuda()
    bh = new_handle()
    try:
        assert bh.initData_device(m, m, m, len(col), dA[2], dA[0], dA[1], len(col), dA[2], dA[0], dA[1]) == 0
        assert bh.spgemm_symbolic() == 0
        assert bh.csr_transpose_raw_device(m, m, len(col), None, dA[0], dA[1], Tp, Tj, None, None) == INV
        assert bh.spgemm_numeric(0, m) == 0 and bh.spgemm_finish() == 0
        assert bh.csr_transpose_raw_device(m, m, len(col), None, dA[0], dA[1], Tp, Tj, None, None) == 0
        assert np.array_equal(Tj.cpu().numpy(), col)
        bh.free_mem()
    finally:
        bh.freePlatform()


# ---------------------------------------------------------------- the handle is left alone
@pytest.mark.parametrize("dtype", DTYPES)
def test_transpose_leaves_the_handle_alone(dtype, oracle):
    rp, col = (np.ascontiguousarray(a, np.int32) for a in gallery.poisson_csr("poisson27pt", 12, 12, 12))
    m = len(rp) - 1
    val = np.ascontiguousarray(np.random.default_rng(13).integers(1, 10, len(col)), dtype)
    rng = np.random.default_rng(14)
    Yp, Yj, Yx = random_csr(700, 900, 0.02, rng)
    bh = new_handle(dtype, {"class_path": 2})
    try:
        Cp = np.zeros(m + 1, np.int32)
        assert bh.initData(m, m, m, len(col), val, rp, col, len(col), val, rp, col, Cp) == 0
        assert bh.spgemm() == 0 and bh.spgemm() == 0                # (the second one launches speculatively where the class path runs)
        keys = ("class_state", "mixed_rows", "spec_launches", "spec_refuted", "b_sorted", "max_row_a", "max_row_b",
                "select_dropped", "add_inplace_used")
        before = {k: bh.get_info(k) for k in keys}
        nnzC, ptrs = bh.get_nnzC(), bh.get_C_device()
        Cj, Cx = np.empty(nnzC, np.int32), np.empty(nnzC, dtype)
        assert bh.get_C(Cj, Cx) == 0
        ref = oracle.spgemm(m, m, m, rp, col, val, rp, col, val)
        assert np.array_equal(Cp, ref[0]) and np.array_equal(Cj, ref[1]) and np.array_equal(Cx, ref[2].astype(dtype))

        def unchanged(what):
            assert {k: bh.get_info(k) for k in keys} == before, what
            assert bh.get_nnzC() == nnzC and bh.get_C_device() == ptrs, what
            j2, x2 = np.empty(nnzC, np.int32), np.empty(nnzC, dtype)
            assert bh.get_C(j2, x2) == 0
            assert np.array_equal(j2, Cj) and np.array_equal(bits(x2), bits(Cx)) and np.array_equal(bh.get_rowptrC(), Cp), what
        check_transpose(bh, 700, 900, (Yp, Yj, Yx), dtype, "beside a multiply")
        unchanged("after a transpose")
        pm = up(rng.permutation(len(Yj)).astype(np.int32), np.int32)
        bh.csr_transpose_values_device(up(Yx, dtype), pm)
        unchanged("after the values call")
        # the product itself, straight from the device pointers
        Tp = torch.zeros(m + 1, dtype=torch.int32).cuda()
        Tj = torch.zeros(nnzC, dtype=torch.int32).cuda()
        Tx = torch.zeros(nnzC, dtype=torch.float32 if dtype == np.float32 else torch.float64).cuda()
        assert bh.csr_transpose_raw_device(m, m, nnzC, ptrs[2], ptrs[0], ptrs[1], Tp, Tj, Tx, None) == 0
        rt = tr.transpose(m, m, Cp, Cj, Cx)
        assert np.array_equal(Tp.cpu().numpy(), rt[0]) and np.array_equal(Tj.cpu().numpy(), rt[1])
        assert np.array_equal(bits(Tx.cpu().numpy()), bits(rt[2]))
        unchanged("after transposing C")
        assert bh.spgemm() == 0                                     # and the next multiply is what it was
        assert bh.get_info("class_state") == before["class_state"] and bh.get_nnzC() == nnzC
        # a selected C served by the getters stays as well
        assert bh.spgemm_select(select_spec(band=(None, -1))) == 0
        nnzL = bh.get_nnzC()
        assert 0 < nnzL < nnzC and bh.get_info("select_dropped") == nnzC - nnzL
        Lj, Lx = np.empty(nnzL, np.int32), np.empty(nnzL, dtype)
        assert bh.get_C(Lj, Lx) == 0
        check_transpose(bh, 700, 900, (Yp, Yj, Yx), dtype, "beside a selection")
        L2j, L2x = np.empty(nnzL, np.int32), np.empty(nnzL, dtype)
        assert bh.get_nnzC() == nnzL and bh.get_C(L2j, L2x) == 0
        assert np.array_equal(Lj, L2j) and np.array_equal(bits(Lx), bits(L2x))
        bh.free_mem()
    finally:
        bh.freePlatform()


# ---------------------------------------------------------------- algebra
@pytest.mark.parametrize("dtype", DTYPES)
def test_involution(dtype):
    rng = np.random.default_rng(15)
    bh = new_handle(dtype)
    try:
        for m, n, dens in ((1200, 800, 0.02), (50, 4000, 0.1), (4000, 50, 0.1)):
            rp, col, val = random_csr(m, n, dens, rng, values="real")
            val = np.ascontiguousarray(val, dtype)
            T = bh.csr_transpose_device(m, n, (up(rp, np.int32), up(col, np.int32), up(val, dtype)))
            U = bh.csr_transpose_device(n, m, T[:3])
            assert np.array_equal(U[0].cpu().numpy(), rp) and np.array_equal(U[1].cpu().numpy(), col)
            assert np.array_equal(bits(U[2].cpu().numpy()), bits(val))
    finally:
        bh.freePlatform()


@pytest.mark.parametrize("dtype", DTYPES)
def test_symmetrise_with_the_add(dtype):
    rng = np.random.default_rng(16)
    n = 3000
    rp, col, val = random_csr(n, n, 0.004, rng)
    val = np.ascontiguousarray(val, dtype)
    bh = new_handle(dtype)
    try:
        X = (up(rp, np.int32), up(col, np.int32), up(val, dtype))
        T = bh.csr_transpose_device(n, n, X)
        Zp, Zj, Zx, _ = bh.csr_add_device(n, n, 1.0, X, 1.0, T[:3])
        Zp, Zj, Zx = Zp.cpu().numpy(), Zj.cpu().numpy(), Zx.cpu().numpy()
        zt = tr.transpose(n, n, Zp, Zj, Zx)
        assert np.array_equal(zt[0], Zp) and np.array_equal(zt[1], Zj) and np.array_equal(zt[2], Zx)     # Z == Z^T, values too
        import scipy.sparse as sp
        S = sp.csr_matrix((val.astype(np.float64), col, rp), shape=(n, n))
        S = (S + S.T).tocsr()
        S.sort_indices()
        assert np.array_equal(S.indptr, Zp) and np.array_equal(S.indices, Zj) and np.array_equal(S.data.astype(dtype), Zx)
    finally:
        bh.freePlatform()


@pytest.mark.parametrize("dtype", DTYPES)
def test_random_property(dtype):
    """100 seeded draws of shape, density, row order and duplicates."""
    bh = new_handle(dtype)
    try:
        for seed in range(100):
            rng = np.random.default_rng(1000 + seed)
            m, n = int(rng.integers(1, 1500)), int(rng.integers(1, 1500))
            mean = float(rng.choice([0.5, 3.0, 20.0, 120.0]))
            lens = rng.poisson(mean, m)
            if seed % 7 == 0:
                lens[rng.integers(0, m)] = int(rng.integers(1000, 5000))
            rp = np.zeros(m + 1, np.int64)
            np.cumsum(lens, out=rp[1:])
            nnz = int(rp[-1])
            if seed % 3 == 0:
                col = np.minimum(n - 1, (rng.random(nnz) ** 3 * n).astype(np.int64)).astype(np.int32)   # skewed: long T rows
            else:
                col = rng.integers(0, n, nnz).astype(np.int32)
            if seed % 2 == 0:                                       # ascending rows (duplicates stay)
                rows = np.repeat(np.arange(m), lens)
                col = col[np.lexsort((col, rows))]
            check_transpose(bh, m, n, (rp.astype(np.int32), col, special_values(nnz, rng)), dtype, "seed %d" % seed)
    finally:
        bh.freePlatform()


def test_csr_transpose_convenience():
    rng = np.random.default_rng(17)
    rp, col, val = random_csr(300, 500, 0.03, rng)
    for dtype in DTYPES:
        Tp, Tj, Tx, info = csr_transpose(300, 500, rp, col, val, value_dtype=dtype)
        ref = tr.transpose(300, 500, rp, col, val.astype(dtype))
        assert np.array_equal(Tp, ref[0]) and np.array_equal(Tj, ref[1]) and np.array_equal(bits(Tx), bits(ref[2]))
        assert np.array_equal(info["perm"], ref[3]) and info["ms"] > 0.0
        assert {"transpose_count", "transpose_scan", "transpose_scatter"} <= {s["name"] for s in info["kernels"]}


# ---------------------------------------------------------------- the Galerkin product
def galerkin_reference(oracle, m, nc, P, A):
    Pp, Pj, Px = P
    Ap, Aj, Ax = A
    Tp, Tj, Tx, _ = tr.transpose(m, nc, Pp, Pj, np.asarray(Px, np.float64))
    PtA = oracle.spgemm(nc, m, m, Tp, Tj, Tx, Ap, Aj, Ax)
    ref = oracle.spgemm(nc, m, nc, PtA[0].astype(np.int32), PtA[1], PtA[2], Pp, Pj, np.asarray(Px, np.float64))
    # every partial sum of either association is bounded by the same product on the magnitudes
    PtA_abs = oracle.spgemm(nc, m, m, Tp, Tj, np.abs(Tx), Ap, Aj, np.abs(Ax))
    bound = oracle.spgemm(nc, m, nc, PtA_abs[0].astype(np.int32), PtA_abs[1], PtA_abs[2], Pp, Pj, np.abs(np.asarray(Px, np.float64)))
    assert bound[2].max() < 2 ** 24, "the float build would round"
    return ref


@pytest.mark.parametrize("dtype", DTYPES)
def test_galerkin_aggregation_on_poisson27pt(dtype, oracle):
    nx = 16
    rp, col = gallery.poisson_csr("poisson27pt", nx, nx, nx)
    m = len(rp) - 1
    rng = np.random.default_rng(18)
    Ax = rng.integers(1, 10, len(col)).astype(np.float64)
    i = np.arange(m)
    x, y, z = i % nx, (i // nx) % nx, i // (nx * nx)
    nc = (nx // 2) ** 3
    Pj = ((z // 2) * (nx // 2) ** 2 + (y // 2) * (nx // 2) + x // 2).astype(np.int32)          # 2 x 2 x 2 aggregates
    Pp = np.arange(m + 1, dtype=np.int32)
    Px = rng.integers(1, 10, m).astype(np.float64)
    ref = galerkin_reference(oracle, m, nc, (Pp, Pj, Px), (rp, col, Ax))
    Cp, Cj, Cx, info = galerkin_csr(m, nc, Pp, Pj, Px, rp, col, Ax, options={"class_path": 2}, value_dtype=dtype)
    ran = [sorted(s["name"] for s in info[key] if s["launches"] > 0) for key in ("kernels_AP", "kernels")]
    print("galerkin p27 16^3 %s: class_state %d / %d, ms %.3f + %.3f + %.3f, A·P ran %s, P^T·(AP) ran %s" %
          (np.dtype(dtype).name, info["class_state_AP"], info["class_state"], info["transpose_ms"], info["ap_ms"], info["ptap_ms"],
           ran[0], ran[1]))
    assert np.array_equal(Cp, ref[0]) and np.array_equal(Cj, ref[1])
    assert Cx.dtype == np.dtype(dtype) and np.array_equal(Cx, ref[2].astype(dtype))
    assert info["nnzC"] == len(ref[1])
    assert info["nnzCt_AP"] == len(col) and info["nnzCt"] > 0 and info["nnzC_AP"] > 0
    assert min(info["transpose_ms"], info["ap_ms"], info["ptap_ms"]) > 0.0


@pytest.mark.parametrize("dtype", DTYPES)
def test_galerkin_random_prolongator(dtype, oracle):
    rng = np.random.default_rng(19)
    m, nc = 2500, 400
    Ap, Aj, Ax = random_csr(m, m, 0.004, rng, empty_rows=(3, 999), values="signed")
    lens = rng.integers(0, 4, m)
    Pp = np.zeros(m + 1, np.int64)
    np.cumsum(lens, out=Pp[1:])
    Pj = np.concatenate([np.sort(rng.choice(nc, L, replace=False)) for L in lens] + [np.zeros(0, np.int64)]).astype(np.int32)
    Px = rng.integers(-3, 4, len(Pj)).astype(np.float64)
    Px[Px == 0] = 2.0
    ref = galerkin_reference(oracle, m, nc, (Pp.astype(np.int32), Pj, Px), (Ap, Aj, Ax))
    Cp, Cj, Cx, info = galerkin_csr(m, nc, Pp.astype(np.int32), Pj, Px, Ap, Aj, Ax, options={"class_path": 0}, value_dtype=dtype)
    # class_path = 0: both multiplies ran the general pipeline ("class_state" only says the data set was never refused the
    # class path; which kernels ran is what bhs_get_kernel_stats names)
    for key in ("kernels_AP", "kernels"):
        ran = {s["name"] for s in info[key] if s["launches"] > 0}
        assert ran and not any("class" in nm for nm in ran), (key, ran)
    assert np.array_equal(Cp, ref[0]) and np.array_equal(Cj, ref[1])
    assert Cx.dtype == np.dtype(dtype) and np.array_equal(Cx, ref[2].astype(dtype))
    assert info["nnzC"] == len(ref[1])


# ---------------------------------------------------------------- the C++ facade
def test_cpp_facade_transpose_demo():
    demo_dir = os.path.join(ROOT, "tests", "transpose")
    subprocess.check_call(["make", "-C", demo_dir, "-s"])
    r = subprocess.run([os.path.join(demo_dir, "transpose_demo")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "PASS" in r.stdout
