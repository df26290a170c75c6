"""Submatrix extraction and permutation (bhs_csr_extract_symbolic_device, bhs_csr_extract_numeric_device) on the GPU, both
builds.

Reference: tests/extractref.py, Z = X(rows, cols) of include/bhsparse_hip.h restated in numpy.  The extraction moves values
and computes nothing, so rowPtrZ, colIndZ, perm and the values' bit patterns are compared bit for bit.  Outputs carry a
sentinel behind their end: nothing may be written there.  The kernel families that ran are compared with what the lengths of
the touched X rows predict."""
import functools
import os
import subprocess

import numpy as np
import pytest
import torch

from conftest import ROOT, load_golden
from helpers import random_csr
import extractref as ex
import transposeref as tr

from benchmark_spgemm_using_csr_amd import _lib, gallery
from benchmark_spgemm_using_csr_amd.facade import (BHSPARSE_HIP, NUM_PLATFORMS, bhsparse, extract_csr,
                                                   permute_csr, select_spec)

pytestmark = pytest.mark.gpu

DTYPES = (np.float64, np.float32)
INV = _lib.BHS_ERR_INVALID_ARG


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


def upi(a):
    return None if a is None else up(a, np.int32)


def tdt(dtype):
    return torch.float32 if np.dtype(dtype) == np.dtype(np.float32) else torch.float64


def families(bh):
    return {s["name"] for s in bh.kernel_stats() if s["launches"] > 0}


def expected_families(Xp, rows, cols, m):
    """(after the symbolic call, after the numeric call) for a legal extraction"""
    r = np.arange(m) if rows is None else np.asarray(rows, np.int64)
    lens = np.diff(np.asarray(Xp, np.int64))[r] if len(r) else np.zeros(0, np.int64)
    base = {"extract_count"} | ({"extract_map"} if (rows is not None or cols is not None) else set())
    sym = base | ({"extract_scan"} if len(r) else set())
    num = set(base)
    if np.any((lens >= 1) & (lens <= 32)):
        num.add("extract_short")
    if np.any((lens > 32) & (lens <= 1024)):
        num.add("extract_wave")
    if np.any(lens > 1024):
        num.add("extract_long")
    return sym, num


def check_extract(bh, m, n, X, rows, cols, dtype, what="", values=True, ref=None):
    """X(rows, cols) on the device against extractref: bit for bit, nothing written past the end of Z, the kernel families
    that must have run did, the reordered rows counted.  Returns the reference."""
    Xp, Xj, Xx = X
    Xx = np.ascontiguousarray(Xx, dtype) if values else None
    nnz = len(Xj)
    if ref is None:
        ref = ex.extract(m, n, Xp, Xj, Xx, rows, cols)
    mI = m if rows is None else len(rows)
    nJ = n if cols is None else len(cols)
    nnzZ = len(ref[1])
    dXp, dXj, dXx = up(Xp, np.int32), up(Xj, np.int32), (up(Xx, dtype) if values else None)
    dR, dC = upi(rows), upi(cols)
    Zp = torch.full((mI + 1 + 16,), -7, dtype=torch.int32).cuda()
    Zj = torch.full((nnzZ + 64,), -7, dtype=torch.int32).cuda()
    pm = torch.full((nnzZ + 64,), -7, dtype=torch.int32).cuda()
    Zx = torch.full((nnzZ + 64,), -7.0, dtype=tdt(dtype)).cuda() if values else None
    torch.cuda.synchronize()
    want_sym, want_num = expected_families(Xp, rows, cols, m)
    err, got = bh.csr_extract_symbolic_device(m, n, nnz, dXp, dXj, mI, dR, nJ, dC, Zp)
    assert err == 0 and got == nnzZ, (what, err, got, nnzZ)
    assert families(bh) == want_sym, (what, families(bh))
    assert bool((Zp[mI + 1:] == -7).all()), (what, "written past the end of rowPtrZ")
    assert np.array_equal(Zp[:mI + 1].cpu().numpy(), ref[0]), (what, "rowPtrZ differs")
    err = bh.csr_extract_numeric_device(m, n, nnz, dXx, dXp, dXj, mI, dR, nJ, dC, nnzZ, Zp, Zj, Zx, pm)
    assert err == 0, (what, err)
    assert families(bh) == want_num, (what, families(bh))
    assert bool((Zj[nnzZ:] == -7).all()) and bool((pm[nnzZ:] == -7).all()), (what, "written past the end")
    assert np.array_equal(Zj[:nnzZ].cpu().numpy(), ref[1]), (what, "colIndZ differs")
    assert np.array_equal(pm[:nnzZ].cpu().numpy(), ref[3]), (what, "perm differs")
    if values:
        assert bool((Zx[nnzZ:] == -7).all()), (what, "written past the end of valZ")
        g = Zx[:nnzZ].cpu().numpy()
        assert g.dtype == np.dtype(dtype) and np.array_equal(bits(g), bits(ref[2])), (what, "valZ differs")
    assert bh.get_info("extract_reordered_rows") == ref[4], (what, bh.get_info("extract_reordered_rows"), ref[4])
    assert bh.extract_ms >= 0.0
    return ref


def shuffled_rows(Xp, Xj, rng):
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


def nan_payloads(v, rng):
    """every NaN of v (float64) gets a payload of its own"""
    v = np.array(v, np.float64)
    w = v.view(np.uint64)
    isn = np.isnan(v)
    w[isn] = np.uint64(0x7FF8000000000000) | rng.integers(1, 1 << 20, int(isn.sum())).astype(np.uint64) << np.uint64(30)
    return v


# ---------------------------------------------------------------- shapes
@pytest.mark.parametrize("dtype", DTYPES)
def test_cf_split_of_stencils_needs_no_sort(dtype):
    bh = new_handle(dtype)
    try:
        for name, dims in (("poisson27pt", (12, 12, 12)), ("poisson5pt", (64, 64, 1))):
            rp, col = gallery.poisson_csr(name, *dims)
            m = len(rp) - 1
            ref = check_extract(bh, m, m, (rp, col, gallery.fill_values(len(col))), np.arange(1, m, 2), np.arange(0, m, 2), dtype, name)
            assert ref[4] == 0 and bh.get_info("extract_reordered_rows") == 0
            ref = check_extract(bh, m, m, (rp, col, gallery.fill_values(len(col))), np.random.default_rng(1).permutation(m), None,
                                dtype, name + " row gather")
            assert ref[4] == 0
    finally:
        bh.freePlatform()


@pytest.mark.parametrize("dtype", DTYPES)
def test_rectangular_and_cage4(dtype):
    g = load_golden("rect_rand.npz")
    c4 = load_golden("cage4_sq.npz")
    rng = np.random.default_rng(2)
    bh = new_handle(dtype)
    try:
        for what, m, n, X in (("rect A", int(g["m"]), int(g["k"]), (g["Ap"], g["Aj"], g["Ax"])),
                              ("rect B", int(g["k"]), int(g["n"]), (g["Bp"], g["Bj"], g["Bx"])),
                              ("cage4", int(c4["m"]), int(c4["m"]), (c4["Ap"], c4["Aj"], c4["Ax"]))):
            rows = rng.integers(0, m, m + 3)                        # (with repeats)
            cols = rng.permutation(n)[:max(1, (2 * n) // 3)]
            check_extract(bh, m, n, X, rows, cols, dtype, what)
    finally:
        bh.freePlatform()


@functools.lru_cache(maxsize=None)
def powerlaw_case():
    rp, col = gallery.powerlaw_csr(30000, 30000, 300000, 6000)
    m = len(rp) - 1
    rng = np.random.default_rng(3)
    val = rng.standard_normal(len(col))
    T = tr.transpose(m, m, rp, col, val)
    cols = rng.permutation(m)[:m // 2]
    rows = rng.permutation(m)
    out = []
    for Xp, Xj, Xx in ((rp, col, val), (T[0], T[1], T[2])):
        out.append((Xp, Xj, Xx, rows, cols, {dt: ex.extract(m, m, Xp, Xj, Xx.astype(dt), rows, cols) for dt in DTYPES}))
    return m, out


@pytest.mark.parametrize("dtype", DTYPES)
def test_power_law_reaches_every_bin(dtype):
    m, cases = powerlaw_case()
    bh = new_handle(dtype)
    try:
        most, ran = 0, set()
        for k, (Xp, Xj, Xx, rows, cols, refs) in enumerate(cases):
            ref = check_extract(bh, m, m, (Xp, Xj, Xx), rows, cols, dtype, "powerlaw %d" % k, ref=refs[dtype])
            ran |= families(bh)
            lens = np.diff(Xp.astype(np.int64))
            most = max(most, int(lens.max()))
            assert np.any(lens <= 32) and np.any((lens > 32) & (lens <= 1024))
            assert ref[4] > 0                                       # (cols is a shuffled half: rows are put in order)
        assert most > 4096                                          # (hub rows of X beyond 4096 entries)
        assert {"extract_short", "extract_wave", "extract_long"} <= ran
    finally:
        bh.freePlatform()


@pytest.mark.parametrize("dtype", DTYPES)
def test_one_row_of_5000_entries(dtype):
    rng = np.random.default_rng(4)
    n = 9000
    col = rng.permutation(n)[:5000].astype(np.int32)                # (not ascending)
    rp = np.array([0, 0, 5000, 5000], np.int32)
    val = special_values(5000, rng)
    bh = new_handle(dtype)
    try:
        ref = check_extract(bh, 3, n, (rp, col, val), None, rng.permutation(n)[:8000], dtype, "5000 -> ~4400, keys in scratch")
        assert ref[0][2] > 4096
        ref = check_extract(bh, 3, n, (rp, col, val), [1, 1], rng.permutation(n)[:3000], dtype, "5000 -> ~1700, keys in LDS")
        assert 1024 < ref[0][1] <= 4096
        ref = check_extract(bh, 3, n, (rp, np.sort(col), val), [1], np.arange(0, n, 2), dtype, "ascending: straight through")
        assert ref[4] == 0
        check_extract(bh, 3, n, (rp, col, val), [1, 0, 1], None, dtype, "row gather of a long unsorted row")
    finally:
        bh.freePlatform()


@functools.lru_cache(maxsize=None)
def wide_case():
    rp, col = gallery.uniform_csr(n=1 << 20, per_row=8)
    n = len(rp) - 1
    rng = np.random.default_rng(5)
    rows = rng.integers(0, n, 200000)
    cols = rng.permutation(n)[:n // 2]
    val = rng.standard_normal(len(col))
    return n, rp, col, val, rows, cols, {dt: ex.extract(n, n, rp, col, val.astype(dt), rows, cols) for dt in DTYPES}


@pytest.mark.parametrize("dtype", DTYPES)
def test_a_map_of_a_million_columns(dtype):
    n, rp, col, val, rows, cols, refs = wide_case()
    bh = new_handle(dtype)
    try:
        check_extract(bh, n, n, (rp, col, val), rows, cols, dtype, "n = 2^20", ref=refs[dtype])
    finally:
        bh.freePlatform()


# ---------------------------------------------------------------- order
@pytest.mark.parametrize("dtype", DTYPES)
def test_reversed_columns_flip_the_matrix(dtype):
    rng = np.random.default_rng(6)
    m, n = 1500, 1100
    rp, col, val = random_csr(m, n, 0.02, rng)
    rp = rp.copy()
    bh = new_handle(dtype)
    try:
        ref = check_extract(bh, m, n, (rp, col, val), None, np.arange(n - 1, -1, -1), dtype, "reversed")
        import scipy.sparse as sp
        S = sp.csr_matrix((val.astype(dtype), col, rp), shape=(m, n))[:, ::-1].tocsr()
        S.sort_indices()
        assert np.array_equal(S.indptr, ref[0]) and np.array_equal(S.indices, ref[1]) and np.array_equal(bits(S.data), bits(ref[2]))
        assert ref[4] == int(np.sum(np.diff(rp) >= 2)) == bh.get_info("extract_reordered_rows")
    finally:
        bh.freePlatform()


@pytest.mark.parametrize("dtype", DTYPES)
def test_all_rows_all_columns_sorts_the_rows(dtype):
    rng = np.random.default_rng(7)
    m, n = 2000, 300
    lens = rng.integers(0, 90, m)
    lens[::211] = 1500                                              # longer than n: duplicates for certain
    rp = np.zeros(m + 1, np.int64)
    np.cumsum(lens, out=rp[1:])
    col = rng.integers(0, n, rp[-1]).astype(np.int32)
    val = np.ascontiguousarray(nan_payloads(special_values(len(col), rng), rng), dtype)
    bh = new_handle(dtype)
    try:
        ref = check_extract(bh, m, n, (rp.astype(np.int32), col, val), None, None, dtype, "NULL, NULL")
        Sj, Sx = tr.sort_rows(m, rp, col, val)
        assert np.array_equal(ref[0], rp) and np.array_equal(ref[1], Sj) and np.array_equal(bits(ref[2]), bits(Sx))
        assert "extract_map" not in families(bh)
    finally:
        bh.freePlatform()


@pytest.mark.parametrize("dtype", DTYPES)
def test_permutation_and_its_inverse(dtype):
    rng = np.random.default_rng(8)
    n = 3000
    rp, col, val = random_csr(n, n, 0.004, rng, values="real")
    val = np.ascontiguousarray(val, dtype)
    p = rng.permutation(n).astype(np.int32)
    pinv = np.empty(n, np.int32)
    pinv[p] = np.arange(n, dtype=np.int32)
    bh = new_handle(dtype)
    try:
        X = (up(rp, np.int32), up(col, np.int32), up(val, dtype))
        Y = bh.csr_extract_device(n, n, X, rows=up(p, np.int32), cols=up(p, np.int32))
        Z = bh.csr_extract_device(n, n, Y[:3], rows=up(pinv, np.int32), cols=up(pinv, np.int32))
        assert np.array_equal(Z[0].cpu().numpy(), rp) and np.array_equal(Z[1].cpu().numpy(), col)
        assert np.array_equal(bits(Z[2].cpu().numpy()), bits(val))
    finally:
        bh.freePlatform()


# ---------------------------------------------------------------- special values, pattern only
@pytest.mark.parametrize("dtype", DTYPES)
def test_special_values_go_through_unchanged(dtype):
    rng = np.random.default_rng(9)
    m, n = 800, 600
    rp, col, _ = random_csr(m, n, 0.05, rng)
    val = np.ascontiguousarray(nan_payloads(special_values(len(col), rng), rng), dtype)
    bh = new_handle(dtype)
    try:
        ref = check_extract(bh, m, n, (rp, shuffled_rows(rp, col, rng), val), rng.integers(0, m, 1000), rng.permutation(n)[:400],
                            dtype, "special values")
        assert np.isnan(ref[2]).any() and np.isinf(ref[2]).any() and np.signbit(ref[2][ref[2] == 0]).any()
    finally:
        bh.freePlatform()


def test_pattern_only():
    rng = np.random.default_rng(10)
    m, n = 500, 300
    rp, col, _ = random_csr(m, n, 0.05, rng)
    col = shuffled_rows(rp, col, rng)
    rows, cols = rng.integers(0, m, 300), rng.permutation(n)[:200]
    bh = new_handle(np.float64)
    try:
        check_extract(bh, m, n, (rp, col, None), rows, cols, np.float64, "pattern only", values=False)
        Z = bh.csr_extract_device(m, n, (up(rp, np.int32), up(col, np.int32), None), rows=upi(rows), cols=upi(cols))
        assert Z[2] is None and Z[3] is None
        ref = ex.extract(m, n, rp, col, None, rows, cols)
        assert np.array_equal(Z[0].cpu().numpy(), ref[0]) and np.array_equal(Z[1].cpu().numpy(), ref[1])
        # values asked for without values given
        nz = len(ref[1])
        Zj = torch.full((nz,), -7, dtype=torch.int32).cuda()
        Zx = torch.full((nz,), -7.0, dtype=torch.float64).cuda()
        assert bh.csr_extract_numeric_device(m, n, len(col), None, up(rp, np.int32), up(col, np.int32), len(rows), upi(rows), len(cols),
                                             upi(cols), nz, Z[0], Zj, Zx, None) == INV
        assert bool((Zj == -7).all()) and bool((Zx == -7).all())
    finally:
        bh.freePlatform()


# ---------------------------------------------------------------- perm and the values-only call
@pytest.mark.parametrize("dtype", DTYPES)
def test_perm_revalues_the_pattern(dtype):
    rng = np.random.default_rng(11)
    rp, col = gallery.poisson_csr("poisson27pt", 12, 12, 12)
    n = len(rp) - 1
    nnz = len(col)
    p = rng.permutation(n).astype(np.int32)
    it = torch.int64 if dtype == np.float64 else torch.int32
    bh = new_handle(dtype)
    try:
        for what, rows, cols in (("X(p, p)", p, p), ("rows twice", np.concatenate([p, p[:100]]), None), ("sub-matrix", p[:900], p[:700])):
            v1 = np.ascontiguousarray(special_values(nnz, rng), dtype)
            dX = (up(rp, np.int32), up(col, np.int32), up(v1, dtype))
            Zp, Zj, Zx, pm = bh.csr_extract_device(n, n, dX, rows=upi(rows), cols=upi(cols), perm=True)
            assert bool((dX[2][pm.long()].view(it) == Zx.view(it)).all()), what
            v2 = np.ascontiguousarray(special_values(nnz, rng), dtype)
            dX[2].copy_(torch.from_numpy(v2))
            fresh = ex.extract(n, n, rp, col, v2, rows, cols)
            if len(fresh[1]) >= nnz:                                # (the values call bounds perm by the count it is given)
                out = bh.csr_transpose_values_device(dX[2], pm)
                assert families(bh) == {"transpose_values"}
                assert np.array_equal(bits(out.cpu().numpy()), bits(fresh[2])), what
            Z2 = bh.csr_extract_device(n, n, dX, rows=upi(rows), cols=upi(cols), perm=True)
            assert torch.equal(Zp, Z2[0]) and torch.equal(Zj, Z2[1]) and torch.equal(pm, Z2[3])
            assert np.array_equal(bits(Z2[2].cpu().numpy()), bits(fresh[2])), what
    finally:
        bh.freePlatform()


# ---------------------------------------------------------------- empty cases
@pytest.mark.parametrize("dtype", DTYPES)
def test_empty_cases(dtype):
    z, zi = np.zeros(0), np.zeros(0, np.int32)
    rng = np.random.default_rng(12)
    rp, col, val = random_csr(40, 30, 0.2, rng)
    bh = new_handle(dtype)
    try:
        check_extract(bh, 0, 0, (np.zeros(1, np.int32), zi, z), None, None, dtype, "0 x 0")
        check_extract(bh, 0, 0, (np.zeros(1, np.int32), zi, z), zi, zi, dtype, "0 x 0, empty lists")
        check_extract(bh, 0, 5, (np.zeros(1, np.int32), zi, z), None, [4, 0], dtype, "m = 0")
        check_extract(bh, 5, 0, (np.zeros(6, np.int32), zi, z), [4, 4, 0], None, dtype, "n = 0")
        check_extract(bh, 40, 30, (rp, col, val), zi, [3, 1], dtype, "mI = 0")
        check_extract(bh, 40, 30, (rp, col, val), [7, 7, 2], zi, dtype, "nJ = 0")
        check_extract(bh, 7, 3, (np.zeros(8, np.int32), zi, z), [6, 0], [2, 0, 1], dtype, "nnzX = 0")
        # rows naming only empty rows, cols naming only empty columns
        rp2 = np.array([0, 0, 3, 3, 5, 5], np.int32)
        col2 = np.array([0, 2, 4, 4, 0], np.int32)
        check_extract(bh, 5, 6, (rp2, col2, np.arange(5.0)), [0, 2, 4, 2], [4, 0], dtype, "only empty rows")
        check_extract(bh, 5, 6, (rp2, col2, np.arange(5.0)), None, [5, 1, 3], dtype, "only empty columns")
    finally:
        bh.freePlatform()


# ---------------------------------------------------------------- refusals
@pytest.mark.parametrize("dtype", DTYPES)
def test_invalid_input_is_refused_and_nothing_is_written(dtype):
    rng = np.random.default_rng(13)
    m, n = 900, 400
    rp, col, val = random_csr(m, n, 0.03, rng)
    nnz = len(col)
    rows = rng.integers(0, m, 1000).astype(np.int32)
    cols = rng.permutation(n)[:250].astype(np.int32)
    good = ex.extract(m, n, rp, col, val, rows, cols)
    nz = len(good[1])
    touched = int(rows[17])
    assert rp[touched + 1] > rp[touched]
    cases = {}
    p = rp.copy(); p[0] = 1
    cases["rowPtrX[0] != 0"] = (p, col, rows, cols)
    p = rp.copy(); p[300], p[301] = rp[301] + 2, rp[300]
    cases["decreasing rowPtrX"] = (p, col, rows, cols)
    p = rp.copy(); p[-1] = nnz - 1
    cases["rowPtrX[m] != nnzX"] = (p, col, rows, cols)
    c = col.copy(); c[rp[touched]] = n
    cases["column of X == n"] = (rp, c, rows, cols)
    c = col.copy(); c[rp[touched + 1] - 1] = -1
    cases["column of X < 0"] = (rp, c, rows, cols)
    r = rows.copy(); r[500] = m
    cases["row index == m"] = (rp, col, r, cols)
    r = rows.copy(); r[0] = -1
    cases["row index < 0"] = (rp, col, r, cols)
    c = cols.copy(); c[100] = n
    cases["column index == n"] = (rp, col, rows, c)
    c = cols.copy(); c[3] = c[240]
    cases["a repeat far apart"] = (rp, col, rows, c)
    c = cols.copy(); c[61] = c[60]
    cases["an adjacent repeat"] = (rp, col, rows, c)
    bh = new_handle(dtype)
    try:
        dZpGood = up(good[0], np.int32)
        for what, (P, J, R, Cc) in cases.items():
            assert ex.invalid(m, n, P, J, R, Cc) is not None, what
            Zp = torch.full((len(R) + 1,), -7, dtype=torch.int32).cuda()
            Zj = torch.full((nz,), -7, dtype=torch.int32).cuda()
            pm = torch.full((nz,), -7, dtype=torch.int32).cuda()
            Zx = torch.full((nz,), -7.0, dtype=tdt(dtype)).cuda()
            dP, dJ, dR, dC = up(P, np.int32), up(J, np.int32), up(R, np.int32), up(Cc, np.int32)
            torch.cuda.synchronize()
            err, _ = bh.csr_extract_raw_device(m, n, nnz, up(val, dtype), dP, dJ, len(R), dR, len(Cc), dC, Zp, Zj, Zx, pm)
            assert err == INV, (what, err)
            assert bool((Zp == -7).all()), what
            err = bh.csr_extract_numeric_device(m, n, nnz, up(val, dtype), dP, dJ, len(R), dR, len(Cc), dC, nz, dZpGood, Zj, Zx, pm)
            assert err == INV, (what, "numeric", err)
            assert bool((Zj == -7).all()) and bool((pm == -7).all()) and bool((Zx == -7).all()), what
        check_extract(bh, m, n, (rp, col, val), rows, cols, dtype, "after the refusals")
        # an invalid column of X in a row that is never read does not count
        c = col.copy()
        unread = np.setdiff1d(np.arange(m), rows)
        unread = unread[np.diff(rp)[unread] > 0][0]
        c[rp[unread]] = n + 5
        Z = bh.csr_extract_device(m, n, (up(rp, np.int32), up(c, np.int32), up(val, dtype)), rows=upi(rows), cols=upi(cols))
        assert np.array_equal(Z[1].cpu().numpy(), good[1])
        # on the host: NULL with a wrong count, bad sizes, aliasing
        dX = (up(rp, np.int32), up(col, np.int32), up(val, dtype))
        dR, dC = upi(rows), upi(cols)
        Zp = torch.full((m + 1001,), -7, dtype=torch.int32).cuda()
        Zj = torch.full((nz,), -7, dtype=torch.int32).cuda()
        Zx = torch.full((nz,), -7.0, dtype=tdt(dtype)).cuda()
        sym, num = bh.csr_extract_symbolic_device, bh.csr_extract_numeric_device
        assert sym(m, n, nnz, dX[0], dX[1], m - 1, None, len(cols), dC, Zp)[0] == INV          # rows NULL, mI != m
        assert sym(m, n, nnz, dX[0], dX[1], len(rows), dR, n - 1, None, Zp)[0] == INV          # cols NULL, nJ != n
        assert sym(-1, n, nnz, dX[0], dX[1], len(rows), dR, len(cols), dC, Zp)[0] == INV
        assert sym(m, n, nnz, dX[0], dX[1], len(rows), dR, len(cols), dC, None)[0] == INV
        assert sym(m, n, nnz, dX[0], dX[1], len(rows), dR, len(cols), dC, dX[0])[0] == INV     # rowPtrZ on top of rowPtrX
        assert sym(m, n, nnz, dX[0], dX[1], len(rows), dR, len(cols), dC, dR[:])[0] == INV     # ... on top of rows
        assert sym(m, n, nnz, dX[0], dX[1], len(rows), dR, len(cols), dC, dX[1][5:])[0] == INV  # ... inside colIndX
        assert bool((Zp == -7).all())
        args = (m, n, nnz, dX[2], dX[0], dX[1], len(rows), dR, len(cols), dC, nz, dZpGood)
        assert num(*args, dX[1], Zx, None) == INV                                               # colIndZ on top of colIndX
        assert num(*args, Zj, dX[2], None) == INV                                               # valZ on top of valX
        assert num(*args, Zj, Zx, Zj) == INV                                                    # perm on top of colIndZ
        assert num(*args, Zj, Zx, dZpGood) == INV                                               # perm on top of rowPtrZ
        assert num(*args, None, Zx, None) == INV
        assert num(m, n, nnz, dX[2], dX[0], dX[1], m - 1, None, len(cols), dC, nz, dZpGood, Zj, Zx, None) == INV
        assert bool((Zj == -7).all()) and bool((Zx == -7).all())
        check_extract(bh, m, n, (rp, col, val), rows, cols, dtype, "after the host's refusals")
    finally:
        bh.freePlatform()


@pytest.mark.parametrize("dtype", DTYPES)
def test_numeric_call_checks_the_row_pointer_it_is_given(dtype):
    rng = np.random.default_rng(14)
    m, n = 700, 500
    rp, col, val = random_csr(m, n, 0.04, rng)
    rp, col = rp.copy(), col.copy()
    rp_long = np.concatenate([rp, [rp[-1] + 2000]]).astype(np.int32)         # a long row at the end: every bin checks
    col_long = np.concatenate([col, rng.integers(0, n, 2000).astype(np.int32)])
    val_long = np.concatenate([val, rng.standard_normal(2000)])
    m += 1
    nnz = len(col_long)
    rows = rng.integers(0, m, 600).astype(np.int32)
    rows[5] = m - 1
    cols1 = rng.permutation(n)[:300].astype(np.int32)
    cols2 = np.roll(cols1, 1)                                        # the same columns: the same counts, another order
    cols3 = np.concatenate([cols1[:299], np.setdiff1d(np.arange(n), cols1)[:1]]).astype(np.int32)   # one column swapped
    ref1 = ex.extract(m, n, rp_long, col_long, val_long, rows, cols1)
    ref3 = ex.extract(m, n, rp_long, col_long, val_long, rows, cols3)
    assert not np.array_equal(ref1[0], ref3[0])
    nz = len(ref1[1])
    bh = new_handle(dtype)
    try:
        dX = (up(rp_long, np.int32), up(col_long, np.int32), up(val_long, dtype))
        dR = upi(rows)
        Zp1 = up(ref1[0], np.int32)

        def fresh():
            return (torch.full((nz + 64,), -7, dtype=torch.int32).cuda(), torch.full((nz + 64,), -7.0, dtype=tdt(dtype)).cuda(),
                    torch.full((nz + 64,), -7, dtype=torch.int32).cuda())
        Zj, Zx, pm = fresh()
        err = bh.csr_extract_numeric_device(m, n, nnz, dX[2], dX[0], dX[1], len(rows), dR, 300, upi(cols3), nz, Zp1, Zj, Zx, pm)
        assert err == INV
        assert bool((Zj[nz:] == -7).all()) and bool((Zx[nz:] == -7).all()) and bool((pm[nz:] == -7).all())
        assert bool((Zj == -7).all()) and bool((Zx == -7).all()) and bool((pm == -7).all())     # (refused before the fill)
        # rowPtrZ[mI] != nnzZ
        Zj, Zx, pm = fresh()
        assert bh.csr_extract_numeric_device(m, n, nnz, dX[2], dX[0], dX[1], len(rows), dR, 300, upi(cols1), nz - 1, Zp1, Zj, Zx,
                                             pm) == INV
        assert bool((Zj == -7).all())
        # the same counts in another order: legal, and it is cols2's result
        ref2 = ex.extract(m, n, rp_long, col_long, np.ascontiguousarray(val_long, dtype), rows, cols2)
        assert np.array_equal(ref2[0], ref1[0])
        Zj, Zx, pm = fresh()
        assert bh.csr_extract_numeric_device(m, n, nnz, dX[2], dX[0], dX[1], len(rows), dR, 300, upi(cols2), nz, Zp1, Zj, Zx, pm) == 0
        assert np.array_equal(Zj[:nz].cpu().numpy(), ref2[1]) and np.array_equal(bits(Zx[:nz].cpu().numpy()), bits(ref2[2]))
        assert bool((Zj[nz:] == -7).all())
    finally:
        bh.freePlatform()


def test_refused_between_symbolic_and_finish():
    rp, col = gallery.poisson_csr("poisson5pt", 16, 16)
    m = len(rp) - 1
    val = gallery.fill_values(len(col))
    dA = (up(rp, np.int32), up(col, np.int32), up(val, np.float64))
    Zp = torch.zeros(m + 1, dtype=torch.int32).cuda()
    Zj = torch.zeros(len(col), dtype=torch.int32).cuda()
    bh = new_handle()
    try:
        assert bh.initData_device(m, m, m, len(col), dA[2], dA[0], dA[1], len(col), dA[2], dA[0], dA[1]) == 0
        assert bh.spgemm_symbolic() == 0
        assert bh.csr_extract_symbolic_device(m, m, len(col), dA[0], dA[1], m, None, m, None, Zp)[0] == INV
        assert bh.csr_extract_numeric_device(m, m, len(col), None, dA[0], dA[1], m, None, m, None, len(col), dA[0], Zj, None, None) == INV
        assert bh.spgemm_numeric(0, m) == 0 and bh.spgemm_finish() == 0
        assert bh.csr_extract_raw_device(m, m, len(col), None, dA[0], dA[1], m, None, m, None, Zp, Zj, None, None) == (0, len(col))
        assert np.array_equal(Zj.cpu().numpy(), col) and np.array_equal(Zp.cpu().numpy(), rp)
        bh.free_mem()
    finally:
        bh.freePlatform()


# ---------------------------------------------------------------- overflow
def test_nnz_beyond_int32_is_an_overflow():
    L, times = 70000, 31000
    assert L * times > 2 ** 31 - 1
    dXp = up(np.array([0, L], np.int32), np.int32)
    dXj = torch.arange(L, dtype=torch.int32).cuda()
    both = torch.full((2 * times + 1,), -7, dtype=torch.int32).cuda()       # rows, then rowPtrZ: the test's only other allocation
    both[:times] = 0
    torch.cuda.synchronize()
    bh = new_handle()
    try:
        err, _ = bh.csr_extract_symbolic_device(1, L, L, dXp, dXj, times, both[:times], L, None, both[times:])
        assert err == _lib.BHS_ERR_NNZ_OVERFLOW
        assert bool((both[times:] == -7).all())
        err, nz = bh.csr_extract_symbolic_device(1, L, L, dXp, dXj, 30000, both[:30000], L, None, both[times:])
        assert err == 0 and nz == 30000 * L and int(both[times + 30000]) == nz
    finally:
        bh.freePlatform()


# ---------------------------------------------------------------- the handle is left alone
@pytest.mark.parametrize("dtype", DTYPES)
def test_extraction_leaves_the_handle_alone(dtype, oracle):
    rp, col = (np.ascontiguousarray(a, np.int32) for a in gallery.poisson_csr("poisson27pt", 12, 12, 12))
    m = len(rp) - 1
    val = np.ascontiguousarray(np.random.default_rng(15).integers(1, 10, len(col)), dtype)
    rng = np.random.default_rng(16)
    Yp, Yj, Yx = random_csr(700, 900, 0.02, rng)
    yr, yc = rng.integers(0, 700, 800), rng.permutation(900)[:500]
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
        check_extract(bh, 700, 900, (Yp, Yj, Yx), yr, yc, dtype, "beside a multiply")
        unchanged("after an extraction")
        # the product itself, straight from the device pointers
        p = rng.permutation(m).astype(np.int32)
        rc = ex.extract(m, m, Cp, Cj, Cx, p, p)
        Zp = torch.zeros(m + 1, dtype=torch.int32).cuda()
        Zj = torch.zeros(nnzC, dtype=torch.int32).cuda()
        Zx = torch.zeros(nnzC, dtype=tdt(dtype)).cuda()
        dp = up(p, np.int32)
        assert bh.csr_extract_raw_device(m, m, nnzC, ptrs[2], ptrs[0], ptrs[1], m, dp, m, dp, Zp, Zj, Zx, None) == (0, nnzC)
        assert np.array_equal(Zp.cpu().numpy(), rc[0]) and np.array_equal(Zj.cpu().numpy(), rc[1])
        assert np.array_equal(bits(Zx.cpu().numpy()), bits(rc[2]))
        unchanged("after extracting from C")
        assert bh.spgemm() == 0                                     # and the next multiply is what it was
        assert bh.get_info("class_state") == before["class_state"] and bh.get_nnzC() == nnzC
        # a selected C served by the getters stays as well
        assert bh.spgemm_select(select_spec(band=(None, -1))) == 0
        nnzL = bh.get_nnzC()
        assert 0 < nnzL < nnzC
        Lj, Lx = np.empty(nnzL, np.int32), np.empty(nnzL, dtype)
        assert bh.get_C(Lj, Lx) == 0
        check_extract(bh, 700, 900, (Yp, Yj, Yx), yr, yc, dtype, "beside a selection")
        L2j, L2x = np.empty(nnzL, np.int32), np.empty(nnzL, dtype)
        assert bh.get_nnzC() == nnzL and bh.get_C(L2j, L2x) == 0
        assert np.array_equal(Lj, L2j) and np.array_equal(bits(Lx), bits(L2x))
        bh.free_mem()
    finally:
        bh.freePlatform()


# ---------------------------------------------------------------- with the multiply
@pytest.mark.parametrize("dtype", DTYPES)
def test_permuted_product_is_the_product_of_the_permuted(dtype, oracle):
    rp, col = (np.ascontiguousarray(a, np.int32) for a in gallery.poisson_csr("poisson27pt", 12, 12, 12))
    m = len(rp) - 1
    nnz = len(col)
    val = np.ascontiguousarray(np.random.default_rng(17).integers(1, 10, nnz), dtype)
    p = np.random.default_rng(18).permutation(m).astype(np.int32)
    h1, h2 = new_handle(dtype), new_handle(dtype)
    try:
        dX = (up(rp, np.int32), up(col, np.int32), up(val, dtype))
        dp = up(p, np.int32)
        # (X·X)(p, p): the oracle-checked C, extracted on the device
        assert h1.initData_device(m, m, m, nnz, dX[2], dX[0], dX[1], nnz, dX[2], dX[0], dX[1]) == 0
        assert h1.spgemm() == 0
        nnzC, ptrs = h1.get_nnzC(), h1.get_C_device()
        ref = oracle.spgemm(m, m, m, rp, col, val, rp, col, val)
        Cj, Cx = np.empty(nnzC, np.int32), np.empty(nnzC, dtype)
        assert h1.get_C(Cj, Cx) == 0
        assert np.array_equal(h1.get_rowptrC(), ref[0]) and np.array_equal(Cj, ref[1]) and np.array_equal(Cx, ref[2].astype(dtype))
        Zp = torch.zeros(m + 1, dtype=torch.int32).cuda()
        Zj = torch.zeros(nnzC, dtype=torch.int32).cuda()
        Zx = torch.zeros(nnzC, dtype=tdt(dtype)).cuda()
        assert h1.csr_extract_raw_device(m, m, nnzC, ptrs[2], ptrs[0], ptrs[1], m, dp, m, dp, Zp, Zj, Zx, None) == (0, nnzC)
        # X(p, p)·X(p, p): the extracted arrays handed over on the device (rows strictly ascending: "b_sorted" holds)
        Y = h2.csr_extract_device(m, m, dX, rows=dp, cols=dp)
        torch.cuda.synchronize()
        assert h2.initData_device(m, m, m, nnz, Y[2], Y[0], Y[1], nnz, Y[2], Y[0], Y[1]) == 0
        assert h2.get_info("b_sorted") == 1
        assert h2.spgemm() == 0 and h2.get_nnzC() == nnzC
        Dj, Dx = np.empty(nnzC, np.int32), np.empty(nnzC, dtype)
        assert h2.get_C(Dj, Dx) == 0
        assert np.array_equal(h2.get_rowptrC(), Zp.cpu().numpy()) and np.array_equal(Dj, Zj.cpu().numpy())
        assert np.array_equal(bits(Dx), bits(Zx.cpu().numpy()))     # (integers below 2^24: exact in any order)
        h1.free_mem(); h2.free_mem()
    finally:
        h1.freePlatform(); h2.freePlatform()


@pytest.mark.parametrize("dtype", DTYPES)
def test_four_blocks_of_a_cf_split_give_the_matrix_back(dtype):
    import scipy.sparse as sp
    rng = np.random.default_rng(19)
    n = 2500
    rp, col, val = random_csr(n, n, 0.004, rng, values="real")
    val = np.ascontiguousarray(val, dtype)
    F, Cc = np.arange(0, n, 2, dtype=np.int32), np.arange(1, n, 2, dtype=np.int32)
    bh = new_handle(dtype)
    try:
        X = (up(rp, np.int32), up(col, np.int32), up(val, dtype))
        ri, ci, vv = [], [], []
        for R in (F, Cc):
            for K in (F, Cc):
                Zp, Zj, Zx, _ = bh.csr_extract_device(n, n, X, rows=up(R, np.int32), cols=up(K, np.int32))
                assert bh.get_info("extract_reordered_rows") == 0
                Zp, Zj = Zp.cpu().numpy(), Zj.cpu().numpy()
                ri.append(R[np.repeat(np.arange(len(R)), np.diff(Zp))]); ci.append(K[Zj]); vv.append(Zx.cpu().numpy())
        S = sp.coo_matrix((np.concatenate(vv), (np.concatenate(ri), np.concatenate(ci))), shape=(n, n)).tocsr()
        S.sort_indices()
        assert np.array_equal(S.indptr, rp) and np.array_equal(S.indices, col) and np.array_equal(bits(S.data.astype(dtype)), bits(val))
    finally:
        bh.freePlatform()


# ---------------------------------------------------------------- random property
@pytest.mark.parametrize("dtype", DTYPES)
def test_random_property(dtype):
    """60 seeded draws of shape, row lengths, row order, duplicates, rows and cols."""
    bh = new_handle(dtype)
    try:
        for seed in range(60):
            rng = np.random.default_rng(2000 + seed)
            m, n = int(rng.integers(1, 1500)), int(rng.integers(1, 1500))
            mean = float(rng.choice([0.5, 3.0, 20.0, 120.0]))
            lens = rng.poisson(mean, m)
            if seed % 7 == 0:
                lens[rng.integers(0, m)] = int(rng.integers(1000, 5000))
            if seed % 4 < 2:                                        # without duplicates: no row longer than n
                lens = np.minimum(lens, n)
            rp = np.zeros(m + 1, np.int64)
            np.cumsum(lens, out=rp[1:])
            nnz = int(rp[-1])
            if seed % 4 < 2:
                col = np.concatenate([rng.permutation(n)[:k] for k in lens] + [np.zeros(0, np.int64)]).astype(np.int32)
            else:
                col = rng.integers(0, n, nnz).astype(np.int32)      # (with replacement: duplicate pairs)
            if seed % 2 == 0:                                       # ascending rows (duplicates stay)
                rws = np.repeat(np.arange(m), lens)
                col = col[np.lexsort((col, rws))]
            rows = (None, rng.permutation(m), rng.permutation(m)[:max(1, m // 3)], rng.integers(0, m, m + 5))[seed % 4 if seed % 5 else 0]
            k = int(rng.integers(0, n + 1))
            cols = (None, np.sort(rng.permutation(n)[:k]), rng.permutation(n)[:k])[seed % 3]
            check_extract(bh, m, n, (rp.astype(np.int32), col, special_values(nnz, rng)), rows, cols, dtype, "seed %d" % seed)
    finally:
        bh.freePlatform()


# ---------------------------------------------------------------- convenience, C++ facade
def test_extract_csr_and_permute_csr():
    rng = np.random.default_rng(20)
    rp, col, val = random_csr(300, 300, 0.03, rng)
    rows, cols = rng.integers(0, 300, 200), rng.permutation(300)[:120]
    p = rng.permutation(300)
    for dtype in DTYPES:
        Zp, Zj, Zx, info = extract_csr(300, 300, rp, col, val, rows=rows, cols=cols, value_dtype=dtype)
        ref = ex.extract(300, 300, rp, col, val.astype(dtype), rows, cols)
        assert np.array_equal(Zp, ref[0]) and np.array_equal(Zj, ref[1]) and np.array_equal(bits(Zx), bits(ref[2]))
        assert np.array_equal(info["perm"], ref[3]) and info["ms"] > 0.0 and info["reordered_rows"] == ref[4]
        assert {"extract_map", "extract_count"} <= {s["name"] for s in info["kernels"]}
        Zp, Zj, Zx, info = permute_csr(300, rp, col, val, p, value_dtype=dtype)
        ref = ex.extract(300, 300, rp, col, val.astype(dtype), p, p)
        assert np.array_equal(Zp, ref[0]) and np.array_equal(Zj, ref[1]) and np.array_equal(bits(Zx), bits(ref[2]))
        assert np.array_equal(info["perm"], ref[3]) and info["reordered_rows"] == ref[4]


def test_cpp_facade_extract_demo():
    demo_dir = os.path.join(ROOT, "tests", "extract")
    subprocess.check_call(["make", "-C", demo_dir, "-s"])
    out = subprocess.run([os.path.join(demo_dir, "extract_demo")], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "PASS" in out.stdout, (out.returncode, out.stdout, out.stderr)
