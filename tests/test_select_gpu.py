"""The entry selection (bhs_csr_select_*_device) and the pruned multiply (bhs_spgemm_select[_device]) on the GPU, both builds.

Reference: tests/selectref.py, the rule of include/bhsparse_hip.h restated in numpy.  The selection does no arithmetic on
values, so rowPtr, colInd and the values' bit patterns are compared bit for bit.  bhs_spgemm_select is compared against
selectref applied to the oracle's product."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

from conftest import ROOT
from helpers import poisson_case, random_csr, real_values, wide_values
import selectref as sr
import valuecheck

from benchmark_spgemm_using_csr_amd import _lib, gallery
from benchmark_spgemm_using_csr_amd.facade import BHSPARSE_HIP, NUM_PLATFORMS, bhsparse, csr_select, spgemm_select_csr

pytestmark = pytest.mark.gpu

FILL = ("select_short", "select_wave", "select_long")
DTYPES = (np.float64, np.float32)
I64MIN, I64MAX = -2 ** 63, 2 ** 63 - 1
INV = _lib.BHS_ERR_INVALID_ARG


# ---------------------------------------------------------------- helpers
def cspec(s):
    """selectref.Spec -> the C structure"""
    c = _lib.Select()
    c.flags, c.top_k, c.band_lo, c.band_hi, c.abs_tol, c.rel_tol = s.flags, s.top_k, s.band_lo, s.band_hi, s.abs_tol, s.rel_tol
    return c


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


def expected_families(Xp):
    lens = np.diff(np.asarray(Xp, np.int64))
    fam = set()
    if np.any((lens >= 1) & (lens <= 32)):
        fam.add("select_short")
    if np.any((lens > 32) & (lens <= 1024)):
        fam.add("select_wave")
    if np.any(lens > 1024):
        fam.add("select_long")
    return fam


def check_select(bh, m, n, X, spec, dtype, what="", ref=None):
    """The stand-alone selection of X on the device against selectref (or `ref`, where the caller has it): bit for bit; the
    kernel families that must have run did."""
    Xp, Xj, Xx = X
    Xx = np.ascontiguousarray(Xx, dtype)
    if ref is None:
        ref = sr.select(m, n, Xp, Xj, Xx, spec)
    dX = (up(Xp, np.int32), up(Xj, np.int32), up(Xx, dtype))
    Zp = torch.full((m + 1,), -7, dtype=torch.int32).cuda()
    torch.cuda.synchronize()
    err, nnzZ = bh.csr_select_symbolic_device(m, n, len(Xj), dX[2], dX[0], dX[1], cspec(spec), Zp)
    assert err == 0, (what, err)
    fam = {s["name"] for s in bh.kernel_stats()}                    # (the records are per call: symbolic, then numeric)
    assert fam == ({"select_count", "select_scan"} if m > 0 else {"select_count"}), (what, fam)
    Zj = torch.full((nnzZ + 64,), -7, dtype=torch.int32).cuda()
    Zx = torch.full((nnzZ + 64,), -7.0, dtype=dX[2].dtype).cuda()
    torch.cuda.synchronize()
    assert bh.csr_select_numeric_device(m, n, len(Xj), dX[2], dX[0], dX[1], cspec(spec), Zp, Zj, Zx) == 0, what
    fam |= {s["name"] for s in bh.kernel_stats()}
    assert bool((Zj[nnzZ:] == -7).all()) and bool((Zx[nnzZ:] == -7).all()), (what, "written past the end of Z")
    Zp, Zj, Zx = Zp.cpu().numpy(), Zj[:nnzZ].cpu().numpy(), Zx[:nnzZ].cpu().numpy()
    assert np.array_equal(Zp, ref[0]), (what, "rowPtrZ differs")
    assert np.array_equal(Zj, ref[1]), (what, "colIndZ differs")
    assert Zx.dtype == np.dtype(dtype) and np.array_equal(bits(Zx), bits(ref[2])), (what, "valZ differs")
    assert "select_count" in fam and all(nm.startswith("select_") for nm in fam), (what, fam)
    assert fam & set(FILL) == expected_families(Xp), (what, fam)
    return ref, fam


def values_of(kind, count, rng):
    if kind == "int":
        return rng.integers(1, 10, count).astype(np.float64) * np.where(rng.random(count) < 0.5, -1.0, 1.0)
    if kind == "wide":                                              # helpers.wide_values: twelve decades
        return wide_values(count, rng)
    if kind == "cancel":                                            # what helpers' "cancel" products look like: 2^-30 of "wide"
        return wide_values(count, rng) * 2.0 ** -30 * rng.random(count)
    if kind == "ties":
        return np.where(rng.random(count) < 0.5, -3.0, 3.0)
    if kind == "fewvalues":                                         # many ties at every cut
        return rng.integers(-3, 4, count).astype(np.float64)
    assert kind == "special", kind
    v = wide_values(count, rng)
    pick = rng.random(count)
    v[pick < 0.05] = np.nan
    v[(pick >= 0.05) & (pick < 0.10)] = np.inf
    v[(pick >= 0.10) & (pick < 0.15)] = -np.inf
    v[(pick >= 0.15) & (pick < 0.22)] = 0.0
    v[(pick >= 0.22) & (pick < 0.29)] = -0.0
    return v


KINDS = ("int", "wide", "cancel", "ties", "fewvalues", "special")


def matrix_of_lengths(lens, n, kind, rng, ascending=True, diag=True):
    """CSR with the given row lengths, columns without duplicates, the diagonal present where it fits and diag is set."""
    m = len(lens)
    Xp = np.zeros(m + 1, np.int64)
    np.cumsum(lens, out=Xp[1:])
    Xj = np.empty(Xp[-1], np.int32)
    for i, L in enumerate(lens):
        c = rng.choice(n, int(L), replace=False) if L < n else rng.permutation(n)
        if diag and L > 0 and i < n and i not in c:
            c[rng.integers(0, L)] = i
        Xj[Xp[i]:Xp[i + 1]] = np.sort(c) if ascending else c
    return Xp.astype(np.int32), Xj, values_of(kind, int(Xp[-1]), rng)


def specs_for(top_ks):
    out = [sr.Spec(flags=sr.BAND, band_lo=I64MIN, band_hi=I64MAX),
           sr.Spec(flags=sr.BAND, band_lo=I64MIN, band_hi=-1),
           sr.Spec(flags=sr.BAND, band_lo=1, band_hi=I64MAX),
           sr.Spec(flags=sr.BAND, band_lo=-40, band_hi=0),
           sr.Spec(flags=sr.BAND, band_lo=0, band_hi=0),
           sr.Spec(flags=sr.BAND, band_lo=-700, band_hi=300),
           sr.Spec(flags=sr.DROP_DIAG),
           sr.Spec(flags=sr.ABS, abs_tol=0.0),
           sr.Spec(flags=sr.ABS, abs_tol=2.5),
           sr.Spec(flags=sr.REL, rel_tol=0.25),
           sr.Spec(flags=sr.REL | sr.KEEP_DIAG, rel_tol=0.25),
           sr.Spec(flags=sr.ABS | sr.REL | sr.DROP_DIAG, abs_tol=2.0 ** -25, rel_tol=1e-3),
           sr.Spec(flags=sr.BAND | sr.ABS | sr.REL | sr.KEEP_DIAG, band_lo=-5000, band_hi=I64MAX, abs_tol=0.0, rel_tol=0.01)]
    for k in top_ks:
        out.append(sr.Spec(flags=sr.TOPK, top_k=k))
    out.append(sr.Spec(flags=sr.TOPK | sr.KEEP_DIAG, top_k=top_ks[len(top_ks) // 2]))
    out.append(sr.Spec(flags=sr.BAND | sr.ABS | sr.REL | sr.TOPK | sr.KEEP_DIAG, band_lo=-3000, band_hi=3000, abs_tol=0.0, rel_tol=1e-4,
                       top_k=top_ks[-2]))
    return out


TOP_KS = (0, 1, 7, 32, 33, 1000, 10 ** 6)


# ---------------------------------------------------------------- the stand-alone selection
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("family", ("short", "wave", "long"))
def test_every_flag_on_every_family(family, dtype):
    """Every flag alone and in combinations on rows of one bin, its edges +-1 included, with and without TOPK."""
    rng = np.random.default_rng({"short": 11, "wave": 12, "long": 13}[family])
    lens, n = {"short": ([1, 2, 15, 16, 17, 31, 32, 0, 32, 9] * 3, 64),
               "wave": ([33, 34, 63, 64, 65, 500, 1023, 1024, 0, 33], 2000),
               "long": ([1025, 1026, 2049, 5000, 0, 1025], 6000)}[family]
    bh = new_handle(dtype)
    try:
        for kind in ("int", "special", "fewvalues"):
            X = matrix_of_lengths(lens, n, kind, rng)
            for spec in specs_for(TOP_KS):
                _, fam = check_select(bh, len(lens), n, X, spec, dtype, (family, kind, vars(spec)))
                assert fam & set(FILL) == {"select_" + family}
    finally:
        bh.freePlatform()


@pytest.mark.parametrize("dtype", DTYPES)
def test_bin_edges_mixed_and_value_ranges(dtype):
    """All three bins in one matrix, rows at each bin edge +-1; the "wide" and "cancel" value ranges; rectangular."""
    rng = np.random.default_rng(21)
    lens = [31, 32, 33, 1023, 1024, 1025, 0, 5, 700, 3000]
    for (n, kind) in ((4000, "wide"), (3500, "cancel"), (4000, "special")):
        X = matrix_of_lengths(lens, n, kind, rng)
        bh = new_handle(dtype)
        try:
            for spec in specs_for((0, 1, 7, 32, 33, 1000, 5000)):
                _, fam = check_select(bh, len(lens), n, X, spec, dtype, (kind, vars(spec)))
                assert fam & set(FILL) == set(FILL)
        finally:
            bh.freePlatform()


@pytest.mark.parametrize("dtype", DTYPES)
def test_unsorted_rows_keep_their_order_and_ties_go_to_the_front(dtype):
    rng = np.random.default_rng(31)
    lens = [30, 32, 200, 1024, 2500, 7]
    bh = new_handle(dtype)
    try:
        for kind in ("ties", "fewvalues", "wide"):
            X = matrix_of_lengths(lens, 3000, kind, rng, ascending=False)
            for spec in specs_for((1, 7, 32, 33, 100, 1000)):
                check_select(bh, len(lens), 3000, X, spec, dtype, (kind, vars(spec)))
    finally:
        bh.freePlatform()


@pytest.mark.parametrize("dtype", DTYPES)
def test_a_row_of_200000_entries(dtype):
    rng = np.random.default_rng(41)
    lens = [5, 200003, 40, 1500]
    n = 250000
    bh = new_handle(dtype)
    try:
        for kind in ("wide", "fewvalues", "special"):
            X = matrix_of_lengths(lens, n, kind, rng)
            for spec in (sr.Spec(flags=sr.BAND, band_lo=I64MIN, band_hi=I64MAX), sr.Spec(flags=sr.ABS | sr.REL, abs_tol=0.0, rel_tol=1e-3),
                         sr.Spec(flags=sr.TOPK, top_k=32), sr.Spec(flags=sr.TOPK, top_k=1000), sr.Spec(flags=sr.TOPK, top_k=150000),
                         sr.Spec(flags=sr.TOPK | sr.REL | sr.KEEP_DIAG, top_k=33, rel_tol=1e-6)):
                _, fam = check_select(bh, len(lens), n, X, spec, dtype, (kind, vars(spec)))
                assert "select_long" in fam
    finally:
        bh.freePlatform()


@pytest.mark.parametrize("dtype", DTYPES)
def test_empty_matrices_and_no_rows(dtype):
    bh = new_handle(dtype)
    try:
        for m, n in ((0, 0), (0, 5), (7, 0), (7, 9)):
            X = (np.zeros(m + 1, np.int32), np.zeros(0, np.int32), np.zeros(0))
            for spec in (sr.Spec(flags=sr.BAND, band_lo=-1, band_hi=1), sr.Spec(flags=sr.TOPK | sr.ABS, top_k=3)):
                dX = (up(X[0], np.int32), up(X[1], np.int32), up(X[2], dtype))
                Zp, Zj, Zx = bh.csr_select_device(m, n, dX, cspec(spec))
                assert np.array_equal(Zp.cpu().numpy(), np.zeros(m + 1, np.int32)) and Zj.numel() == 0
    finally:
        bh.freePlatform()


def test_pattern_only_selection_without_values():
    """d_valX NULL with position flags only; d_valZ NULL: the pattern alone."""
    rng = np.random.default_rng(51)
    Xp, Xj, Xx = random_csr(300, 400, 0.05, rng)
    spec = sr.Spec(flags=sr.BAND | sr.DROP_DIAG, band_lo=-50, band_hi=20)
    ref = sr.select(300, 400, Xp, Xj, None, spec)
    bh = new_handle()
    try:
        Zp, Zj, Zx = bh.csr_select_device(300, 400, (up(Xp, np.int32), up(Xj, np.int32), None), cspec(spec))
        assert Zx is None
        assert np.array_equal(Zp.cpu().numpy(), ref[0]) and np.array_equal(Zj.cpu().numpy(), ref[1])
        # values present, none wanted back
        Zp, Zj, Zx = bh.csr_select_device(300, 400, (up(Xp, np.int32), up(Xj, np.int32), up(Xx, np.float64)), cspec(spec), values=False)
        assert Zx is None and np.array_equal(Zj.cpu().numpy(), ref[1])
        # a value flag without values is refused
        dZp = torch.full((301,), -7, dtype=torch.int32).cuda()
        err, _ = bh.csr_select_symbolic_device(300, 400, len(Xj), None, up(Xp, np.int32), up(Xj, np.int32),
                                               cspec(sr.Spec(flags=sr.ABS)), dZp)
        assert err == INV and bool((dZp == -7).all())
    finally:
        bh.freePlatform()


def random_spec(rng, n):
    f = 0
    kw = {}
    if rng.random() < 0.5:
        f |= sr.BAND
        lo = int(rng.integers(-n, n))
        kw["band_lo"], kw["band_hi"] = (I64MIN if rng.random() < 0.2 else lo), (I64MAX if rng.random() < 0.2 else lo + int(rng.integers(0, n + 1)))
    d = rng.random()
    if d < 0.25:
        f |= sr.DROP_DIAG
    elif d < 0.6:
        f |= sr.KEEP_DIAG
    if rng.random() < 0.5:
        f |= sr.ABS
        kw["abs_tol"] = float(rng.choice([0.0, 1.0, 3.0, 2.0 ** -18, 2.0 ** -45]))
    if rng.random() < 0.5:
        f |= sr.REL
        kw["rel_tol"] = float(rng.choice([0.0, 1.0, 0.5, 1e-3, 2.0]))
    if rng.random() < 0.6:
        f |= sr.TOPK
        kw["top_k"] = int(rng.choice([0, 1, 2, 5, 16, 31, 32, 33, 64, 200, 2000]))
    return sr.Spec(flags=f, **kw)


@pytest.mark.parametrize("seed", range(120))
def test_random_property(seed):
    """Seeded draws of shape, density, value kind and rule, bit-exact against selectref."""
    rng = np.random.default_rng(7000 + seed)
    dtype = DTYPES[seed % 2]
    m, n = int(rng.integers(1, 400)), int(rng.integers(1, 3000))
    shape = rng.random()
    if shape < 0.4:
        lens = rng.binomial(n, min(1.0, rng.choice([2, 8, 30, 60]) / n), m)
    elif shape < 0.8:
        lens = np.minimum(n, rng.zipf(1.5, m))
    else:
        lens = rng.integers(0, n + 1, m) if n < 1500 else np.minimum(n, rng.zipf(1.3, m))
    if m * int(np.max(lens, initial=0)) > 400000:
        lens = np.minimum(lens, 400000 // m)
    X = matrix_of_lengths(lens, n, KINDS[int(rng.integers(0, len(KINDS)))], rng, ascending=bool(rng.random() < 0.7),
                          diag=bool(rng.random() < 0.7))
    bh = new_handle(dtype)
    try:
        for _ in range(3):
            spec = random_spec(rng, n)
            check_select(bh, m, n, X, spec, dtype, (seed, vars(spec)))
    finally:
        bh.freePlatform()


def test_csr_select_convenience():
    rng = np.random.default_rng(61)
    Xp, Xj, Xx = random_csr(200, 300, 0.1, rng, values="real")
    spec = sr.Spec(flags=sr.TOPK | sr.DROP_DIAG, top_k=4)
    Zp, Zj, Zx, info = csr_select(200, 300, Xp, Xj, Xx, cspec(spec))
    ref = sr.select(200, 300, Xp, Xj, Xx, spec)
    assert np.array_equal(Zp, ref[0]) and np.array_equal(Zj, ref[1]) and np.array_equal(bits(Zx), bits(ref[2]))
    assert {s["name"] for s in info["kernels"]} == {"select_count"} | expected_families(Xp)   # (the numeric call's records)
    assert "select_short" in expected_families(Xp)


# ---------------------------------------------------------------- validation
BAD_SPECS = (dict(flags=sr.DROP_DIAG | sr.KEEP_DIAG), dict(flags=sr.TOPK, top_k=-1), dict(flags=sr.ABS, abs_tol=-1.0),
             dict(flags=sr.ABS, abs_tol=float("nan")), dict(flags=sr.ABS, abs_tol=float("inf")), dict(flags=sr.REL, rel_tol=-0.5),
             dict(flags=sr.REL, rel_tol=float("nan")), dict(flags=sr.REL, rel_tol=float("inf")), dict(flags=sr.BAND, band_lo=1, band_hi=0),
             dict(flags=64), dict(flags=sr.BAND | 1024, band_lo=0, band_hi=1))


@pytest.mark.parametrize("dtype", DTYPES)
def test_invalid_input_is_rejected_and_nothing_is_written(dtype):
    rng = np.random.default_rng(71)
    m, n = 50, 60
    Xp, Xj, Xx = random_csr(m, n, 0.2, rng)
    nnz = len(Xj)
    good = sr.Spec(flags=sr.ABS | sr.TOPK, abs_tol=1.0, top_k=3)
    bad = []
    p = Xp.copy(); p[0] = 1; bad.append(("rowPtr[0] != 0", p, Xj, nnz))
    p = Xp.copy(); p[10], p[11] = Xp[11], Xp[10]; assert p[10] > p[11]; bad.append(("decreasing rowPtr", p, Xj, nnz))
    bad.append(("rowPtr[m] != nnz", Xp, Xj, nnz - 1))
    j = Xj.copy(); j[5] = n; bad.append(("column == n", Xp, j, nnz))
    j = Xj.copy(); j[nnz - 1] = -1; bad.append(("column < 0", Xp, j, nnz))
    p = Xp.copy(); p[20] = nnz + 5; bad.append(("rowPtr beyond nnz", p, Xj, nnz))
    bh = new_handle(dtype)
    try:
        dXx = up(Xx, dtype)
        for what, p, j, z in bad:
            dZp = torch.full((m + 1,), -7, dtype=torch.int32).cuda()
            err, _ = bh.csr_select_symbolic_device(m, n, z, dXx, up(p, np.int32), up(j, np.int32), cspec(good), dZp)
            assert err == INV, what
            assert bool((dZp == -7).all()), what
        dXp, dXj = up(Xp, np.int32), up(Xj, np.int32)
        for kw in BAD_SPECS:
            c = _lib.Select()
            c.flags, c.top_k = kw.get("flags", 0), kw.get("top_k", 0)
            c.band_lo, c.band_hi, c.abs_tol, c.rel_tol = kw.get("band_lo", 0), kw.get("band_hi", 0), kw.get("abs_tol", 0.0), kw.get("rel_tol", 0.0)
            dZp = torch.full((m + 1,), -7, dtype=torch.int32).cuda()
            dZj = torch.full((nnz,), -7, dtype=torch.int32).cuda()
            dZx = torch.full((nnz,), -7.0, dtype=dXx.dtype).cuda()
            err, _ = bh.csr_select_symbolic_device(m, n, nnz, dXx, dXp, dXj, c, dZp)
            assert err == INV and bool((dZp == -7).all()), kw
            assert bh.csr_select_numeric_device(m, n, nnz, dXx, dXp, dXj, c, dXp, dZj, dZx) == INV, kw
            assert bool((dZj == -7).all()) and bool((dZx == -7).all()), kw
        # the handle still works
        check_select(bh, m, n, (Xp, Xj, Xx), good, dtype)
    finally:
        bh.freePlatform()


@pytest.mark.parametrize("dtype", DTYPES)
def test_x_changed_between_symbolic_and_numeric(dtype):
    rng = np.random.default_rng(81)
    lens = [20, 32, 300, 1024, 3000, 12]
    m, n = len(lens), 4000
    Xp, Xj, Xx = matrix_of_lengths(lens, n, "int", rng)
    bh = new_handle(dtype)
    try:
        for spec, change in ((sr.Spec(flags=sr.ABS, abs_tol=4.5), 100.0), (sr.Spec(flags=sr.ABS | sr.TOPK, abs_tol=4.5, top_k=2000), 100.0),
                             (sr.Spec(flags=sr.ABS, abs_tol=0.5), 0.0)):
            for row in range(m):                                     # one row of every family grows or shrinks
                dXp, dXj, dXx = up(Xp, np.int32), up(Xj, np.int32), up(Xx, dtype)
                dZp = torch.empty(m + 1, dtype=torch.int32).cuda()
                err, nnzZ = bh.csr_select_symbolic_device(m, n, len(Xj), dXx, dXp, dXj, cspec(spec), dZp)
                assert err == 0
                x2 = np.ascontiguousarray(Xx, dtype).copy()
                x2[Xp[row]:Xp[row + 1]] = change
                ref2 = sr.select(m, n, Xp, Xj, x2, spec)
                assert ref2[0][-1] != nnzZ
                pad = 4096
                dZj = torch.full((nnzZ + pad,), -7, dtype=torch.int32).cuda()
                dZx = torch.full((nnzZ + pad,), -7.0, dtype=dXx.dtype).cuda()
                torch.cuda.synchronize()
                assert bh.csr_select_numeric_device(m, n, len(Xj), up(x2, dtype), dXp, dXj, cspec(spec), dZp, dZj, dZx) == INV, (vars(spec), row)
                assert bool((dZj[nnzZ:] == -7).all()) and bool((dZx[nnzZ:] == -7).all()), (vars(spec), row)
                # unchanged X: the same arrays are filled
                assert bh.csr_select_numeric_device(m, n, len(Xj), dXx, dXp, dXj, cspec(spec), dZp, dZj, dZx) == 0
                ref = sr.select(m, n, Xp, Xj, np.ascontiguousarray(Xx, dtype), spec)
                assert np.array_equal(dZj[:nnzZ].cpu().numpy(), ref[1]) and bool((dZj[nnzZ:] == -7).all())
    finally:
        bh.freePlatform()


# ---------------------------------------------------------------- bhs_spgemm_select
def bind(bh, m, k, n, A, B, dtype=np.float64):
    Ap, Aj, Ax = A
    Bp, Bj, Bx = B
    arrs = [np.ascontiguousarray(x, t) for x, t in ((Ax, dtype), (Ap, np.int32), (Aj, np.int32),
                                                    (Bx, dtype), (Bp, np.int32), (Bj, np.int32))]
    Cp = np.zeros(m + 1, np.int32)
    assert bh.initData(m, k, n, len(arrs[2]), arrs[0], arrs[1], arrs[2], len(arrs[5]), arrs[3], arrs[4], arrs[5], Cp) == 0
    return Cp


def result(bh):
    nnz = bh.get_nnzC()
    Cj, Cx = np.empty(nnz, np.int32), np.empty(nnz, bh._vdt)
    assert bh.get_C(Cj, Cx) == 0
    return bh.get_rowptrC(), Cj, Cx


def int_case(kind):
    rng = np.random.default_rng({"stencil": 1, "perturbed": 2, "powerlaw": 3, "general": 4}[kind])
    if kind in ("stencil", "general"):
        m, rp, col, _ = poisson_case("poisson27pt", 12, 12, 12)
        opts = {} if kind == "stencil" else {"class_path": 0}
    elif kind == "perturbed":
        m, rp, col, _ = poisson_case("poisson9pt", 64, 64)
        rp, col = gallery.perturb_rows_csr(rp, col, m, fraction=0.01, seed=5)
        opts = {}
    else:
        m = 3000
        rp, col = gallery.powerlaw_csr(m, m, 24000, 1500, seed=9, hubs=3)
        opts = {}
    val = rng.integers(1, 10, len(col)).astype(np.float64)
    return m, (rp, col, val), opts


PRODUCT_SPECS = (sr.Spec(flags=sr.BAND, band_lo=I64MIN, band_hi=-1), sr.Spec(flags=sr.TOPK | sr.KEEP_DIAG, top_k=7),
                 sr.Spec(flags=sr.ABS | sr.REL | sr.TOPK, abs_tol=20.0, rel_tol=0.1, top_k=33))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kind", ("stencil", "perturbed", "powerlaw", "general"))
def test_spgemm_select_integer_values_bit_exact(kind, dtype, oracle):
    m, A, opts = int_case(kind)
    ref = oracle.spgemm(m, m, m, *A, *A)
    bh = new_handle(dtype, opts)
    try:
        Cp = bind(bh, m, m, m, A, A, dtype)
        for spec in PRODUCT_SPECS:
            want = sr.select(m, m, ref[0], ref[1], np.asarray(ref[2], dtype), spec)
            assert bh.spgemm_select(cspec(spec)) == 0
            fam = {s["name"] for s in bh.kernel_stats()}
            assert "select_count" in fam and fam & set(FILL) and any(not nm.startswith("select_") for nm in fam), fam
            if kind == "powerlaw":
                assert "select_long" in fam, fam
            gp, gj, gx = result(bh)
            assert np.array_equal(Cp, want[0]) and np.array_equal(gp, want[0])          # rowPtrC_out and the getter
            assert np.array_equal(gj, want[1]) and np.array_equal(bits(gx), bits(want[2]))
            assert bh.nnzC == bh.get_nnzC() == len(want[1]) and bh.nnzCt == int(np.diff(A[0])[A[1]].sum())
            assert bh.get_info("select_dropped") == len(ref[1]) - len(want[1]) > 0
            dp, dj, dx = bh.get_C_device()
            assert dp and dj and dx
            # a following plain multiply returns the full product again
            assert bh.spgemm() == 0
            gp, gj, gx = result(bh)
            assert np.array_equal(gp, ref[0]) and np.array_equal(gj, ref[1]) and np.array_equal(gx, np.asarray(ref[2], dtype))
    finally:
        bh.freePlatform()


@pytest.mark.parametrize("dtype", DTYPES)
def test_spgemm_select_device_row_pointer_and_convenience(dtype, oracle):
    m, A, _ = int_case("perturbed")
    ref = oracle.spgemm(m, m, m, *A, *A)
    spec = PRODUCT_SPECS[1]
    want = sr.select(m, m, ref[0], ref[1], np.asarray(ref[2], dtype), spec)
    bh = new_handle(dtype)
    try:
        bind(bh, m, m, m, A, A, dtype)
        dCp = torch.full((m + 1,), -7, dtype=torch.int32).cuda()
        assert bh.spgemm_select_device(cspec(spec), dCp) == 0
        assert np.array_equal(dCp.cpu().numpy(), want[0])
        gp, gj, gx = result(bh)
        assert np.array_equal(gj, want[1]) and np.array_equal(bits(gx), bits(want[2]))
    finally:
        bh.freePlatform()
    Cp, Cj, Cx, info = spgemm_select_csr(m, m, m, *A, *A, cspec(spec), value_dtype=dtype)
    assert np.array_equal(Cp, want[0]) and np.array_equal(Cj, want[1]) and np.array_equal(bits(Cx), bits(want[2]))
    assert info["select_dropped"] == len(ref[1]) - len(want[1])


@pytest.mark.parametrize("dtype,mode", ((np.float64, "f64"), (np.float32, "f32_once")))
def test_spgemm_select_real_values(dtype, mode, oracle):
    """abs_tol at the midpoint of a gap (>= 1e-3 relative) in the oracle's sorted |C|: the pattern does not depend on the order
    of the additions; values within valuecheck's bound for the mode."""
    rng = np.random.default_rng(91)
    m, rp, col, _ = poisson_case("poisson27pt", 10, 10, 10)
    k, A, B = real_values("wide", m, (rp, col, None), (rp, col, None), rng)
    ref, S, K = valuecheck.references(oracle, m, k, m, A, B, mode)
    mags = np.sort(np.abs(ref[2]))
    lo, hi = mags[:-1], mags[1:]
    gaps = np.flatnonzero((hi - lo) >= 1e-3 * hi)
    assert len(gaps)
    g = gaps[np.argmin(np.abs(gaps - len(mags) // 2))]              # the gap nearest the median
    tol = 0.5 * (lo[g] + hi[g])
    spec = sr.Spec(flags=sr.ABS, abs_tol=tol)
    keep = np.abs(ref[2]) > tol
    rows = np.repeat(np.arange(m), np.diff(ref[0]))
    wantp = np.zeros(m + 1, np.int64)
    np.cumsum(np.bincount(rows[keep], minlength=m), out=wantp[1:])
    bh = new_handle(dtype)
    try:
        bind(bh, m, k, m, A, B, dtype)
        assert bh.spgemm_select(cspec(spec)) == 0
        gp, gj, gx = result(bh)
        assert np.array_equal(gp, wantp.astype(np.int32)) and np.array_equal(gj, ref[1][keep])
        assert 0 < len(gj) < len(ref[1])
        worst = valuecheck.check_values(ref[2][keep], S[keep], K[keep], gx, mode, "spgemm_select ")
        print("worst err/bound %.3g" % worst)
    finally:
        bh.freePlatform()


def test_spgemm_select_with_speculative_launches(oracle):
    m, A, _ = int_case("stencil")
    ref = oracle.spgemm(m, m, m, *A, *A)
    spec = PRODUCT_SPECS[2]
    want = sr.select(m, m, ref[0], ref[1], ref[2], spec)
    bh = new_handle(np.float64, {"spec_numeric": 1})
    try:
        bind(bh, m, m, m, A, A)
        for rep in range(3):
            assert bh.spgemm_select(cspec(spec)) == 0
            gp, gj, gx = result(bh)
            assert np.array_equal(gp, want[0]) and np.array_equal(gj, want[1]) and np.array_equal(bits(gx), bits(want[2])), rep
        assert bh.get_info("spec_refuted") == 0
    finally:
        bh.freePlatform()


def test_keep_everything_makes_no_second_set_of_arrays(oracle):
    m, A, _ = int_case("stencil")
    ref = oracle.spgemm(m, m, m, *A, *A)
    bh = new_handle()
    try:
        bind(bh, m, m, m, A, A)
        assert bh.spgemm() == 0
        plain = bh.get_C_device()
        for spec in (sr.Spec(flags=sr.ABS, abs_tol=0.0), sr.Spec(flags=sr.BAND, band_lo=I64MIN, band_hi=I64MAX), sr.Spec(flags=0)):
            assert bh.spgemm_select(cspec(spec)) == 0
            assert bh.get_info("select_dropped") == 0 and bh.nnzC == len(ref[1])
            assert bh.get_C_device() == plain
            fam = {s["name"] for s in bh.kernel_stats()}
            assert "select_count" in fam and not fam & set(FILL), fam
            gp, gj, gx = result(bh)
            assert np.array_equal(gp, ref[0]) and np.array_equal(gj, ref[1]) and np.array_equal(gx, ref[2])
        assert bh.spgemm_select(cspec(sr.Spec(flags=sr.TOPK, top_k=2))) == 0
        assert bh.get_C_device() != plain
        assert bh.spgemm() == 0
        assert bh.get_C_device() == plain
    finally:
        bh.freePlatform()


def test_spgemm_select_refusals(oracle):
    m, A, _ = int_case("stencil")
    spec = cspec(PRODUCT_SPECS[0])
    bh = new_handle()
    try:
        assert bh.spgemm_select(spec) == _lib.BHS_ERR_NOT_READY            # no data
        assert bh.spgemm_select_device(spec) == _lib.BHS_ERR_NOT_READY
        bind(bh, m, m, m, A, A)
        assert bh.spgemm() == 0
        nnz = bh.get_nnzC()
        for kw in BAD_SPECS:                                             # the rule is checked before the multiply starts
            c = _lib.Select()
            c.flags, c.top_k = kw.get("flags", 0), kw.get("top_k", 0)
            c.band_lo, c.band_hi, c.abs_tol, c.rel_tol = kw.get("band_lo", 0), kw.get("band_hi", 0), kw.get("abs_tol", 0.0), kw.get("rel_tol", 0.0)
            assert bh.spgemm_select(c) == INV, kw
        assert bh.get_nnzC() == nnz
        # inside a split multiply
        assert bh.spgemm_symbolic() == 0
        nnzC = bh.nnzC
        assert bh.spgemm_select(spec) == INV
        dZp = torch.full((m + 1,), -7, dtype=torch.int32).cuda()
        e2, _ = bh.csr_select_symbolic_device(m, m, 0, None, dZp, None, cspec(sr.Spec(flags=0)), dZp)
        assert e2 == INV
        assert bh.spgemm_numeric(0, m) == 0
        assert bh.spgemm_finish() == 0
        # bound output arrays
        dj = torch.empty(nnzC, dtype=torch.int32).cuda()
        dx = torch.empty(nnzC, dtype=torch.float64).cuda()
        assert bh.set_output_device(dj, dx, nnzC) == 0
        assert bh.spgemm_select(spec) == INV
        assert bh.set_output_device(None, None, 0) == 0
        assert bh.spgemm_select(spec) == 0
    finally:
        bh.freePlatform()


# ---------------------------------------------------------------- end to end
def test_triangle_count_entirely_on_the_device(oracle):
    """L = the selection with band_hi = -1 of a symmetrised R-MAT graph, then the masked multiply L·L on L."""
    rp, col = gallery.rmat_csr(scale=11, edge_factor=8, seed=123)
    n = len(rp) - 1
    r = np.repeat(np.arange(n), np.diff(rp))
    rows = np.concatenate([r, col]).astype(np.int64)
    cols = np.concatenate([col, r]).astype(np.int64)
    Sp, Sj = gallery._csr_from_pairs(n, n, rows, cols)             # the symmetrised graph, diagonal and all
    Sx = np.ones(len(Sj))
    bh = new_handle()
    try:
        dS = (up(Sp, np.int32), up(Sj, np.int32), up(Sx, np.float64))
        Lp, Lj, Lx = bh.csr_select_device(n, n, dS, cspec(sr.Spec(flags=sr.BAND, band_lo=I64MIN, band_hi=-1)))
        Lj, Lx = Lj.contiguous(), Lx.contiguous()
        nnzL = Lj.numel()
        assert bh.initData_device(n, n, n, nnzL, Lx, Lp, Lj, nnzL, Lx, Lp, Lj) == 0
        dC = torch.empty(nnzL, dtype=torch.float64).cuda()
        assert bh.spgemm_masked_device(Lp, Lj, nnzL, dC) == 0
        count = int(dC.sum().item())
    finally:
        bh.freePlatform()
    low = Sj < np.repeat(np.arange(n), np.diff(Sp))
    hp, hj = gallery._csr_from_pairs(n, n, np.repeat(np.arange(n), np.diff(Sp))[low], Sj[low])
    assert np.array_equal(Lp.cpu().numpy(), hp) and np.array_equal(Lj.cpu().numpy(), hj)
    ones = np.ones(len(hj))
    P = oracle.spgemm(n, n, n, hp, hj, ones, hp, hj, ones)          # L·L by the oracle, summed over L's pattern
    want = int(round(valuecheck.on_pattern(P, n, hp, hj).sum()))
    assert want > 0 and count == want


def test_cpp_facade_select_demo():
    demo_dir = os.path.join(ROOT, "tests", "select")
    subprocess.check_call(["make", "-C", demo_dir, "-s"])
    r = subprocess.run([os.path.join(demo_dir, "select_demo")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "select OK" in r.stdout, r.stdout + r.stderr
