"""The multiply over a semiring (bhs_spgemm_semiring[_masked[_device]]) on the GPU.

Reference: tests/semiringref.py, the header's rule in numpy (pinned against a dense triple loop in
tests/test_semiring_abi.py).  Every comparison is bit for bit, NaNs compared as NaNs: min, max and or do not depend on the
order of their operands, and plus-pair counts in integers."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from helpers import poisson_case, random_csr
import semiringref as sr

from benchmark_spgemm_using_csr_amd import _lib, gallery
from benchmark_spgemm_using_csr_amd.facade import (BHSPARSE_HIP, NUM_PLATFORMS, BhsparseError, bhsparse,
                                                   spgemm_masked_csr, spgemm_semiring_csr, spgemm_semiring_masked_csr)

pytestmark = pytest.mark.gpu

NEW = sorted(sr.NEW)
BIN_SEMIRINGS = ["min_plus", "max_min", "or_and", "plus_pair"]
HUB_MIN = 10000                                           # "masked_hub_min_products" of the hub cases


def code(name):
    return sr.SEMIRINGS[name]


def values_for(name, rng, count, integers=False):
    return sr.edge_values(rng, count, plus_safe=name in ("min_plus", "max_plus"), integers=integers)


def revalue(name, rng, A, B, dtype=np.float64):
    """The patterns of A and B with edge-case values, rounded to the build's value type."""
    Ax = values_for(name, rng, len(A[1])).astype(dtype)
    Bx = values_for(name, rng, len(B[1])).astype(dtype)
    return (A[0], A[1], Ax), (B[0], B[1], Bx)


def new_handle(dtype=np.float64, options=None):
    plats = [False] * NUM_PLATFORMS
    plats[BHSPARSE_HIP] = True
    bh = bhsparse(value_dtype=dtype)
    assert bh.initPlatform(plats) == 0
    for key, val in (options or {}).items():
        assert bh.set_option(key, val) == 0, key
    return bh


def bind(bh, m, k, n, A, B, dtype=np.float64):
    Ap, Aj, Ax = A
    Bp, Bj, Bx = B
    arrs = [np.ascontiguousarray(x, t) for x, t in ((Ax, dtype), (Ap, np.int32), (Aj, np.int32),
                                                    (Bx, dtype), (Bp, np.int32), (Bj, np.int32))]
    Cp = np.zeros(m + 1, np.int32)
    assert bh.initData(m, k, n, len(arrs[2]), arrs[0], arrs[1], arrs[2], len(arrs[5]), arrs[3], arrs[4], arrs[5], Cp) == 0
    return Cp


def get_c(bh):
    nnz = bh.get_nnzC()
    Cj = np.empty(nnz, np.int32)
    Cx = np.empty(nnz, bh._vdt)
    assert bh.get_C(Cj, Cx) == 0
    return bh.get_rowptrC(), Cj, Cx


def families(kernels):
    return {s["name"]: s for s in kernels}


def square(m, rp, col, val):
    return m, m, m, (rp, col, val), (rp, col, val)


def mask_from_pairs(m, n, rows, cols):
    key = np.unique(np.asarray(rows, np.int64) * n + np.asarray(cols, np.int64))
    Mp = np.concatenate([[0], np.cumsum(np.bincount(key // n, minlength=m))]).astype(np.int32)
    return Mp, (key % n).astype(np.int32)


def random_mask(rng, m, n, inside, frac_in=0.5, extra_per_row=3, empty_rows=()):
    """Part of pattern(A·B) (inside = (Cp, Cj)) plus random entries, rows strictly ascending."""
    Cp, Cj = inside
    keep = rng.random(len(Cj)) < frac_in
    rr = np.concatenate([np.repeat(np.arange(m), np.diff(Cp.astype(np.int64)))[keep], np.repeat(np.arange(m), extra_per_row)])
    cc = np.concatenate([Cj[keep].astype(np.int64), rng.integers(0, n, m * extra_per_row)])
    sel = ~np.isin(rr, list(empty_rows))
    return mask_from_pairs(m, n, rr[sel], cc[sel])


def run_and_check(name, m, k, n, A, B, Mp, Mj, options=None, dtype=np.float64):
    """The masked semiring multiply once; asserts it equals the reference bit for bit; returns (valC, reference, info)."""
    valC, info = spgemm_semiring_masked_csr(m, k, n, *A, *B, Mp, Mj, code(name), options=options, value_dtype=dtype)
    want = sr.semiring_masked(name, m, n, A, B, Mp, Mj, dtype=dtype)
    assert valC.dtype == np.dtype(dtype)
    assert sr.same_bits(valC, want), (name, int(np.count_nonzero(~((valC == want) | (np.isnan(valC) & np.isnan(want))))))
    fam = families(info["kernels"])
    assert fam["sr_scan"]["launches"] == 1 and fam["sr_scan"]["rows"] == m
    assert not any(nm.startswith(("masked", "numeric", "symbolic")) for nm in fam), fam
    return valC, want, info


# ---------------------------------------------------------------- 1. M = pattern(A·B)
def _rect():
    rng = np.random.default_rng(7)
    A = random_csr(300, 200, 0.03, rng, empty_rows=(0, 5, 77))
    B = random_csr(200, 250, 0.04, rng, empty_rows=(3,))
    return 300, 200, 250, A, B


PATTERN_CASES = {
    "p5_16_class": (lambda: square(*poisson_case("poisson5pt", 16, 16)), {"class_path": 2}),
    "p5_16_general": (lambda: square(*poisson_case("poisson5pt", 16, 16)), {"class_path": 0}),
    "rect_rand": (_rect, {}),
}


@pytest.mark.parametrize("name", NEW)
@pytest.mark.parametrize("case", sorted(PATTERN_CASES))
def test_semiring_on_pattern_of_product(case, name):
    make, opts = PATTERN_CASES[case]
    m, k, n, A, B = make()
    A, B = revalue(name, np.random.default_rng(100 + code(name)), A, B)
    Mp, Mj = sr.pattern(m, n, A, B)
    valC, want, info = run_and_check(name, m, k, n, A, B, Mp, Mj, options=opts)
    fam = families(info["kernels"])
    assert sum(s["rows"] for nm, s in fam.items() if nm != "sr_scan") == int(np.count_nonzero(np.diff(Mp)))
    assert info["ms"] > 0 and info["nnzCt"] == int(np.diff(B[0])[A[1]].sum())
    if name == "plus_pair":
        assert valC.min() >= 1                            # every entry of the pattern has a product


# ---------------------------------------------------------------- 2. a random mask: inside, outside, empty rows
@pytest.mark.parametrize("name", NEW)
def test_semiring_random_mask_reads_the_identity_where_nothing_lands(name):
    rng = np.random.default_rng(3)
    m, k, n = 500, 400, 450
    A = random_csr(m, k, 0.02, rng, empty_rows=(1, 2, 3, 100))
    B = random_csr(k, n, 0.02, rng, empty_rows=(7,))
    A, B = revalue(name, rng, A, B)
    inside = sr.pattern(m, n, A, B)
    Mp, Mj = random_mask(rng, m, n, inside, frac_in=0.5, extra_per_row=3, empty_rows=(0, 10, 499))
    assert Mp[1] == 0 and Mp[11] == Mp[10]
    valC, want, _ = run_and_check(name, m, k, n, A, B, Mp, Mj)
    # the entries of M outside pattern(A·B) read the identity (+Inf for min-plus)
    ikey = np.repeat(np.arange(m, dtype=np.int64), np.diff(inside[0])) * n + inside[1]
    mkey = np.repeat(np.arange(m, dtype=np.int64), np.diff(Mp)) * n + Mj
    outside = ~np.isin(mkey, ikey)
    assert outside.any() and (~outside).any()
    ident = np.float64(sr.identity(name))
    assert np.all(valC[outside] == ident)
    if ident == 0:
        assert not np.signbit(valC[outside]).any()
    if name == "min_plus":
        assert np.all(np.isposinf(valC[outside]))


# ---------------------------------------------------------------- 3. every bin
def _one_row(rng, nA, k, n, b_len):
    """Row 0 of A has nA entries (on the first nA rows of B, each of b_len entries), rows 1.. are small."""
    m = 4
    Ap = np.array([0, nA, nA + 1, nA + 1, nA + 3], np.int32)
    Aj = np.concatenate([np.arange(nA), [k - 3], [k - 2, k - 1]]).astype(np.int32)   # (k - 3 >= nA: the small rows of B)
    Bp = np.zeros(k + 1, np.int64)
    cols = []
    for i in range(k):
        c = np.sort(rng.choice(n, b_len if i < nA else min(b_len, 30), replace=False))
        cols.append(c)
        Bp[i + 1] = Bp[i] + len(c)
    Bj = np.concatenate(cols).astype(np.int32)
    return m, k, n, (Ap, Aj, np.ones(len(Aj))), (Bp.astype(np.int32), Bj, np.ones(len(Bj)))


def _bin_case(kind):
    """((m, k, n, A, B), (Mp, Mj) or None for pattern(A·B), options, the family that must run, its least products)"""
    rng = np.random.default_rng({"short": 1, "wave256": 2, "wave2048": 3, "long": 4, "hub_5x4000": 5, "hub_slice_lds": 5,
                                 "hub_slice_big": 5, "hub_entries_lds": 6, "hub_entries_big": 6}[kind])
    if kind == "short":
        return square(*poisson_case("poisson5pt", 20, 20)), None, {}, "sr_short", 1
    if kind == "wave256":                                 # mask rows of up to 125 entries, 729 products
        return square(*poisson_case("poisson27pt", 7, 7, 7)), None, {}, "sr_wave", 1
    if kind == "wave2048":                                # mask rows of ~550 entries: the 2048-entry table
        m, k, n = 64, 400, 3000
        return (m, k, n, random_csr(m, k, 30 / k, rng), random_csr(k, n, 20 / n, rng)), None, {}, "sr_wave", 1
    if kind == "long":                                    # table capped at 16: mask rows of 17 .. 40 entries take k_sr_long
        m, k, n = 50, 60, 120
        A, B = random_csr(m, k, 0.1, rng), random_csr(k, n, 0.1, rng)
        lens = rng.integers(17, 41, m)
        rows = np.repeat(np.arange(m), lens)
        cols = np.concatenate([rng.choice(n, ln, replace=False) for ln in lens])
        M = mask_from_pairs(m, n, rows, cols)
        assert np.diff(M[0]).min() >= 17 and np.diff(M[0]).max() <= 40
        return (m, k, n, A, B), M, {"masked_max_table_log2": 4}, "sr_long", 1
    if kind == "hub_5x4000":                              # 5 A entries on B rows of 4000 entries, ~20 000 products: 3 parts of
        #                                                   8192 products <= 5 entries, so this row is split BY A ENTRIES
        case = _one_row(rng, 5, 8, 6000, 4000)
        lens = 1500
    elif kind in ("hub_slice_lds", "hub_slice_big"):      # ONE A entry on a B row of 20 000: 3 parts > 1 entry, every part
        #                                                   takes a SLICE OF THE B ROW (the only cases on that split)
        case = _one_row(rng, 1, 8, 30000, 20000)
        lens = 1500
    else:                                                 # 300 A entries on B rows of ~70 entries: the split by A entries
        case = _one_row(rng, 300, 400, 3000, 70)
        lens = 1500
    m, k, n, A, B = case
    inside = sr.pattern(m, n, A, B)
    row0 = inside[1][:inside[0][1]]
    pick = np.concatenate([rng.choice(row0, min(lens - 200, len(row0)), replace=False), rng.integers(0, n, 200)])
    rr = np.concatenate([np.zeros(len(pick), np.int64), np.repeat(np.arange(1, m), np.diff(inside[0])[1:])])
    cc = np.concatenate([pick, inside[1][inside[0][1]:]])
    M = mask_from_pairs(m, n, rr, cc)
    opts = {"masked_hub_min_products": HUB_MIN}
    if kind in ("hub_slice_big", "hub_entries_big"):
        opts["masked_max_table_log2"] = 8                 # the mask row (> 256 entries) is beyond the LDS cap
    assert 256 < M[0][1] <= 2048
    return case, M, opts, "sr_hub", HUB_MIN


BIN_KINDS = ["short", "wave256", "wave2048", "long", "hub_5x4000", "hub_slice_lds", "hub_slice_big", "hub_entries_lds",
             "hub_entries_big"]


@pytest.mark.parametrize("name", BIN_SEMIRINGS)
@pytest.mark.parametrize("kind", BIN_KINDS)
def test_every_bin(kind, name):
    (m, k, n, A, B), M, opts, family, least = _bin_case(kind)
    A, B = revalue(name, np.random.default_rng(200 + code(name)), A, B)
    Mp, Mj = M if M is not None else sr.pattern(m, n, A, B)
    valC, want, info = run_and_check(name, m, k, n, A, B, Mp, Mj, options=opts)
    fam = families(info["kernels"])
    assert family in fam and fam[family]["launches"] >= 1, fam
    assert fam[family]["rows"] >= 1 and fam[family]["products"] >= least, fam
    if kind == "wave256":
        assert fam["sr_wave"]["launches"] == 1 and np.diff(Mp).max() <= 256
    if kind == "wave2048":
        assert np.diff(Mp).max() > 256
    if kind == "long":
        assert fam["sr_long"]["rows"] == m
    if family == "sr_hub":
        assert fam["sr_hub"]["rows"] == 1 and fam["sr_hub"]["launches"] == 3


# ---------------------------------------------------------------- 4. NaN propagates, -0 is below +0
def _signed_zero_case():
    """Row 0: products (+0, +0), (-0, -0) and (1, 5) in each of 20 columns -- and a NaN in column 3.  Row 1 has no NaN."""
    n = 20
    Ap = np.array([0, 3, 5], np.int32)
    Aj = np.array([0, 1, 2, 0, 1], np.int32)
    Ax = np.array([0.0, -0.0, 1.0, 0.0, -0.0])
    Bp = np.array([0, n, 2 * n, 3 * n], np.int32)
    Bj = np.tile(np.arange(n), 3).astype(np.int32)
    Bx = np.concatenate([np.full(n, 0.0), np.full(n, -0.0), np.full(n, 5.0)])
    Bx[2 * n + 3] = np.nan
    return 2, 3, n, (Ap, Aj, Ax), (Bp, Bj, Bx)


@pytest.mark.parametrize("opts", [{}, {"masked_max_table_log2": 4}], ids=["lds", "long"])
@pytest.mark.parametrize("name", NEW)
def test_nan_propagates_and_minus_zero_is_below_plus_zero(name, opts):
    m, k, n, A, B = _signed_zero_case()
    Mp, Mj = sr.pattern(m, n, A, B)
    valC, want, info = run_and_check(name, m, k, n, A, B, Mp, Mj, options=opts)
    fam = families(info["kernels"])
    assert ("sr_long" if opts else "sr_short") in fam
    row0, row1 = valC[:n], valC[n:]
    if name in ("or_and", "plus_pair"):
        assert np.all(row0 == (1.0 if name == "or_and" else 3.0))   # or-and: NaN and 5 are non-zero; the zeros are not
        assert np.all(row1 == (0.0 if name == "or_and" else 2.0))
        return
    assert np.isnan(row0[3]) and not np.isnan(np.delete(row0, 3)).any() and not np.isnan(row1).any()
    # row 1 reduces (+0) and (-0) alone: min gives -0, max gives +0
    assert np.all(row1 == 0) and np.all(np.signbit(row1) == name.startswith("min"))
    expect0 = {"min_plus": -0.0, "max_plus": 6.0, "max_times": 5.0, "min_max": -0.0, "max_min": 1.0}[name]
    rest = np.delete(row0, 3)
    assert np.all(rest == expect0) and np.all(np.signbit(rest) == np.signbit(expect0))


# ---------------------------------------------------------------- 5. the float build
@pytest.mark.parametrize("name", NEW)
def test_f32_pattern_of_product(name):
    m, k, n, A, B = _rect()
    A, B = revalue(name, np.random.default_rng(300 + code(name)), A, B, dtype=np.float32)
    Mp, Mj = sr.pattern(m, n, A, B)
    run_and_check(name, m, k, n, A, B, Mp, Mj, dtype=np.float32)


@pytest.mark.parametrize("name", BIN_SEMIRINGS)
@pytest.mark.parametrize("kind", ["long", "hub_entries_lds", "hub_slice_big"])
def test_f32_bins_that_reduce_in_valc(kind, name):
    (m, k, n, A, B), M, opts, family, least = _bin_case(kind)
    A, B = revalue(name, np.random.default_rng(400 + code(name)), A, B, dtype=np.float32)
    Mp, Mj = M
    valC, want, info = run_and_check(name, m, k, n, A, B, Mp, Mj, options=opts, dtype=np.float32)
    assert families(info["kernels"])[family]["products"] >= least


# ---------------------------------------------------------------- 6. the full product
def _int_values(A, B, rng):
    return ((A[0], A[1], rng.integers(-6, 7, len(A[1])).astype(np.float64)),
            (B[0], B[1], rng.integers(-6, 7, len(B[1])).astype(np.float64)))


FULL_CASES = {
    "p27_6_class": (lambda: square(*poisson_case("poisson27pt", 6, 6, 6)), {"class_path": 2}),
    "p27_16_class": (lambda: square(*poisson_case("poisson27pt", 16, 16, 16)), {"class_path": 2}),
    "rect_general": (_rect, {"class_path": 0}),
}


@pytest.mark.parametrize("case", sorted(FULL_CASES))
def test_full_product_and_the_multiplies_after_it(case, oracle):
    """bhs_spgemm_semiring: the oracle's pattern, the reference's values; a plain spgemm() after it is the oracle's C bit
    for bit (integer values), also as the data set's second and later multiply -- the ones the class path launches
    speculatively on the figures of the multiply before."""
    make, opts = FULL_CASES[case]
    m, k, n, A, B = make()
    A, B = _int_values(A, B, np.random.default_rng(11))
    ref = oracle.spgemm(m, k, n, *A, *B)
    rCp, rCj, rCx = np.asarray(ref[0], np.int32), np.asarray(ref[1], np.int32), np.asarray(ref[2], np.float64)
    bh = new_handle(options=opts)
    try:
        Cp = bind(bh, m, k, n, A, B)
        names = ["min_plus", "plus_pair"] if case == "p27_16_class" else ["min_plus", "max_min", "plus_pair", "or_and"]
        for step, name in enumerate(names):
            assert bh.spgemm_semiring(code(name)) == 0
            assert np.array_equal(Cp, rCp) and bh.nnzC == len(rCj) and bh.nnzCt == oracle.nnzCt(A[0], A[1], B[0])
            gCp, gCj, gCx = get_c(bh)
            assert np.array_equal(gCp, rCp) and np.array_equal(gCj, rCj)
            assert sr.same_bits(gCx, sr.semiring_masked(name, m, n, A, B, rCp, rCj)), name
            fam = families(bh.kernel_stats())
            assert fam["sr_scan"]["launches"] == 1 and any(nm.startswith("numeric") for nm in fam)
            assert bh.semiring_ms > 0 and bh.multiply_ms > 0
            ptrs = bh.get_C_device()
            assert bh.spgemm() == 0                       # the data set's multiply number 2, 4, ..
            gCp, gCj, gCx = get_c(bh)
            assert np.array_equal(gCp, rCp) and np.array_equal(gCj, rCj) and np.array_equal(gCx, rCx), (name, step)
            assert bh.get_C_device() == ptrs              # the pipeline's arrays have not moved
        print("spec_launches", case, bh.get_info("spec_launches"), "refuted", bh.get_info("spec_refuted"),
              "class_state", bh.get_info("class_state"))
        assert bh.get_info("spec_refuted") == 0
        if case.endswith("_class"):                       # the second and later multiplies were launched speculatively
            assert bh.get_info("class_state") == 1 and bh.get_info("spec_launches") >= 1
        # PLUS_TIMES forwards to the ordinary multiply
        assert bh.spgemm_semiring(_lib.BHS_SR_PLUS_TIMES) == 0
        gCp, gCj, gCx = get_c(bh)
        assert np.array_equal(gCj, rCj) and np.array_equal(gCx, rCx)
        assert "sr_scan" not in families(bh.kernel_stats())
    finally:
        bh.freePlatform()


def test_full_product_convenience_on_real_values():
    m, k, n, A, B = _rect()
    A, B = revalue("max_times", np.random.default_rng(13), A, B)
    Cp, Cj, Cx, info = spgemm_semiring_csr(m, k, n, *A, *B, _lib.BHS_SR_MAX_TIMES)
    rCp, rCj = sr.pattern(m, n, A, B)
    assert np.array_equal(Cp, rCp) and np.array_equal(Cj, rCj)
    assert sr.same_bits(Cx, sr.semiring_masked("max_times", m, n, A, B, rCp, rCj))
    assert np.isnan(Cx).any()                             # 0 * Inf among the products


def test_full_product_refusals(oracle):
    import torch
    m, k, n, A, B = square(*poisson_case("poisson5pt", 12, 12))
    ref = oracle.spgemm(m, k, n, *A, *B)
    bh = new_handle()
    try:
        assert bh.spgemm_semiring(_lib.BHS_SR_MIN_PLUS) == _lib.BHS_ERR_NOT_READY
        bind(bh, m, k, n, A, B)
        assert bh.spgemm() == 0
        Cp, Cj, Cx = get_c(bh)
        assert np.array_equal(Cx, ref[2])
        # an unknown semiring: nothing is started, the last C stands
        for bad in (-1, 8, 1000):
            assert bh.spgemm_semiring(bad) == _lib.BHS_ERR_INVALID_ARG
        Cp2, Cj2, Cx2 = get_c(bh)
        assert np.array_equal(Cp2, Cp) and np.array_equal(Cj2, Cj) and np.array_equal(Cx2, Cx)
        # inside a split multiply
        assert bh.spgemm_symbolic() == 0
        assert bh.spgemm_semiring(_lib.BHS_SR_MIN_PLUS) == _lib.BHS_ERR_INVALID_ARG
        assert bh.spgemm_numeric(0, m) == 0 and bh.spgemm_finish() == 0
        # with bound output arrays
        dCj = torch.empty(len(Cj), dtype=torch.int32, device="cuda")
        dCx = torch.empty(len(Cj), dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        assert bh.set_output_device(dCj, dCx, len(Cj)) == 0
        assert bh.spgemm_semiring(_lib.BHS_SR_MIN_PLUS) == _lib.BHS_ERR_INVALID_ARG
        assert bh.set_output_device(None, None, 0) == 0
        assert bh.spgemm_semiring(_lib.BHS_SR_MIN_PLUS) == 0
        gCp, gCj, gCx = get_c(bh)
        assert np.array_equal(gCj, Cj) and sr.same_bits(gCx, sr.semiring_masked("min_plus", m, n, A, B, Cp, Cj))
        assert bh.free_mem() == 0
        assert bh.spgemm_semiring(_lib.BHS_SR_MIN_PLUS) == _lib.BHS_ERR_NOT_READY
    finally:
        bh.freePlatform()


# ---------------------------------------------------------------- 7. PLUS_TIMES forwards
def test_plus_times_forwards_to_the_masked_multiply():
    rng = np.random.default_rng(17)
    m, k, n = 300, 200, 250
    A = random_csr(m, k, 0.03, rng, values="signed")
    B = random_csr(k, n, 0.04, rng, values="signed")
    Mp, Mj = random_mask(rng, m, n, sr.pattern(m, n, A, B))
    want, _ = spgemm_masked_csr(m, k, n, *A, *B, Mp, Mj)
    got, info = spgemm_semiring_masked_csr(m, k, n, *A, *B, Mp, Mj, _lib.BHS_SR_PLUS_TIMES)
    assert np.array_equal(got, want)
    fam = families(info["kernels"])
    assert "masked_scan" in fam and not any(nm.startswith("sr_") for nm in fam)
    assert sr.same_bits(got, sr.semiring_masked("plus_times", m, n, A, B, Mp, Mj))


# ---------------------------------------------------------------- 8. uses
def test_triangle_count_rmat_plus_pair():
    rp, col = gallery.rmat_csr(scale=12, edge_factor=8, seed=123)
    n = len(rp) - 1
    r = np.repeat(np.arange(n), np.diff(rp))
    rows = np.concatenate([r, col]).astype(np.int64)
    cols = np.concatenate([col, r]).astype(np.int64)
    low = rows > cols                                     # symmetrised, strict lower triangle
    Lp, Lj = mask_from_pairs(n, n, rows[low], cols[low])
    ones = np.ones(len(Lj))
    junk = np.random.default_rng(1).standard_normal(len(Lj))   # plus-pair never reads a value
    junk[::7] = np.nan
    junk[::5] = 0.0
    pair, info = spgemm_semiring_masked_csr(n, n, n, Lp, Lj, junk, Lp, Lj, junk, Lp, Lj, _lib.BHS_SR_PLUS_PAIR)
    masked, _ = spgemm_masked_csr(n, n, n, Lp, Lj, ones, Lp, Lj, ones, Lp, Lj)
    assert np.array_equal(pair, masked)
    assert int(pair.sum()) == int(masked.sum()) > 0
    assert info["nnzCt"] == int(np.diff(Lp)[Lj].sum())


def test_shortest_paths_by_min_plus_squaring():
    """Three min-plus squarings of W (edge weights, 0 on the diagonal) hold the best path of up to 8 edges.  On a 64-node ring
    with chords of 8 every pair is within 7 hops; with weights in [4, 5) a path of 7 hops costs less than 35 and any path of
    9 edges or more at least 36: every shortest path has at most 8 edges, so the third squaring is Floyd-Warshall's answer.
    Weights are multiples of 1/64: every path length is exact, whatever the association."""
    rng = np.random.default_rng(23)
    n = 64
    W = np.full((n, n), np.inf)
    for i in range(n):
        for j in ((i + 1) % n, (i + 8) % n):
            W[i, j] = W[j, i] = 4.0 + float(rng.integers(0, 64)) / 64.0
    np.fill_diagonal(W, 0.0)

    def floyd_warshall(D):
        D = D.copy()
        for kk in range(n):
            D = np.minimum(D, D[:, kk:kk + 1] + D[kk:kk + 1, :])
        return D
    D = floyd_warshall(W)
    hops = np.where(np.isfinite(W), 1.0, np.inf)
    np.fill_diagonal(hops, 0.0)
    H = floyd_warshall(hops)
    assert H.max() == 7

    def csr(dense):
        has = np.isfinite(dense)
        rr, cc = np.nonzero(has)
        return np.concatenate([[0], np.cumsum(has.sum(1))]).astype(np.int32), cc.astype(np.int32), dense[rr, cc]
    X = csr(W)
    for step in (1, 2, 3):
        Cp, Cj, Cx, _info = spgemm_semiring_csr(n, n, n, *X, *X, _lib.BHS_SR_MIN_PLUS)
        X = (Cp, Cj, Cx)
        got = np.full((n, n), np.inf)
        got[np.repeat(np.arange(n), np.diff(Cp)), Cj] = Cx
        reach = H <= 2 ** step                            # the pairs this squaring reaches
        assert np.array_equal(np.isfinite(got), reach) and len(Cj) == int(reach.sum())
        assert np.all(got[reach] >= D[reach])
    assert reach.all() and np.array_equal(got, D)


# ---------------------------------------------------------------- 9. repeatability
def test_hub_bin_is_bit_exact_from_run_to_run():
    (m, k, n, A, B), (Mp, Mj), opts, family, least = _bin_case("hub_entries_big")
    rng = np.random.default_rng(29)
    A = (A[0], A[1], rng.standard_normal(len(A[1])))
    B = (B[0], B[1], rng.standard_normal(len(B[1])))
    bh = new_handle(options=opts)
    try:
        bind(bh, m, k, n, A, B)
        for name in ("max_plus", "min_max"):
            first = bh.spgemm_semiring_masked(code(name), Mp, Mj)
            assert families(bh.kernel_stats())["sr_hub"]["products"] >= least
            second = bh.spgemm_semiring_masked(code(name), Mp, Mj)
            assert first.tobytes() == second.tobytes()
            assert sr.same_bits(first, sr.semiring_masked(name, m, n, A, B, Mp, Mj))
    finally:
        bh.freePlatform()


# ---------------------------------------------------------------- 10. the handle's state, invalid masks
@pytest.mark.parametrize("opts", [{"class_path": 2}, {"class_path": 0}])
def test_handle_state_untouched(opts):
    m, k, n, A, B = square(*poisson_case("poisson27pt", 8, 8, 8))
    rng = np.random.default_rng(41)
    Mp, Mj = random_mask(rng, m, n, sr.pattern(m, n, A, B))
    bh = new_handle(options=opts)
    try:
        bind(bh, m, k, n, A, B)
        assert bh.spgemm() == 0
        Cp, Cj, Cx = get_c(bh)
        state = bh.get_info("class_state")
        ptrs = bh.get_C_device()
        valC = bh.spgemm_semiring_masked(_lib.BHS_SR_MIN_PLUS, Mp, Mj)
        Cp2, Cj2, Cx2 = get_c(bh)
        assert np.array_equal(Cj2, Cj) and np.array_equal(Cx2, Cx) and np.array_equal(Cp2, Cp)
        assert bh.get_C_device() == ptrs
        assert bh.get_info("class_state") == state
        assert bh.spgemm() == 0
        Cp3, Cj3, Cx3 = get_c(bh)
        assert np.array_equal(Cp3, Cp) and np.array_equal(Cj3, Cj) and np.array_equal(Cx3, Cx)
        assert bh.get_info("class_state") == state
    finally:
        bh.freePlatform()
    assert sr.same_bits(valC, sr.semiring_masked("min_plus", m, n, A, B, Mp, Mj))


def _bad_masks(m, n, Mp, Mj):
    i = int(np.argmax(np.diff(Mp) >= 2))
    s = Mp[i]
    unsorted = Mj.copy()
    unsorted[s], unsorted[s + 1] = unsorted[s + 1], unsorted[s]
    dup = Mj.copy()
    dup[s + 1] = dup[s]
    big = Mj.copy()
    big[-1] = n
    neg = Mj.copy()
    neg[0] = -1
    nonmono = Mp.copy()
    nonmono[m // 2] = nonmono[m // 2 + 1] + 1
    first = Mp.copy()
    first[0] = 1
    return {"unsorted_row": (Mp, unsorted, len(Mj)), "duplicate": (Mp, dup, len(Mj)), "column_ge_n": (Mp, big, len(Mj)),
            "negative_column": (Mp, neg, len(Mj)), "non_monotone": (nonmono, Mj, len(Mj)),
            "rowptr0": (first, Mj, len(Mj)), "wrong_nnz": (Mp, Mj, len(Mj) - 1)}


def test_invalid_masks_and_semirings_are_rejected_and_leave_valc_alone():
    import torch
    m, k, n, A, B = square(*poisson_case("poisson5pt", 12, 12))
    Mp, Mj = sr.pattern(m, n, A, B)
    S = _lib.BHS_SR_MAX_MIN
    bh = new_handle()
    try:
        with pytest.raises(BhsparseError) as e:
            bh.spgemm_semiring_masked(S, Mp, Mj)
        assert e.value.code == _lib.BHS_ERR_NOT_READY
        bind(bh, m, k, n, A, B)
        cases = {nm: (S,) + v for nm, v in _bad_masks(m, n, Mp, Mj).items()}
        cases["semiring_8"] = (8, Mp, Mj, len(Mj))
        cases["semiring_neg"] = (-1, Mp, Mj, len(Mj))
        for name, (s, p, j, nnz) in cases.items():
            sentinel = np.full(len(Mj), 12345.0)
            out = sentinel.copy()
            with pytest.raises(BhsparseError) as e:
                if nnz == len(j):
                    bh.spgemm_semiring_masked(s, p, j, out)
                else:
                    raise BhsparseError("x", bh._lib.bhs_spgemm_semiring_masked(bh._h, s, p.ctypes.data, j.ctypes.data, nnz,
                                                                                out.ctypes.data, None, None))
            assert e.value.code == _lib.BHS_ERR_INVALID_ARG, name
            assert np.array_equal(out, sentinel), name
            dC = torch.full((len(Mj),), 12345.0, dtype=torch.float64, device="cuda")
            rc = bh.spgemm_semiring_masked_device(s, torch.from_numpy(np.ascontiguousarray(p)).cuda(),
                                                  torch.from_numpy(np.ascontiguousarray(j)).cuda(), nnz, dC)
            assert rc == _lib.BHS_ERR_INVALID_ARG, name
            assert torch.all(dC == 12345.0).item(), name
        # inside a split multiply
        assert bh.spgemm_symbolic() == 0
        with pytest.raises(BhsparseError) as e:
            bh.spgemm_semiring_masked(S, Mp, Mj)
        assert e.value.code == _lib.BHS_ERR_INVALID_ARG
        assert bh.spgemm_numeric(0, m) == 0 and bh.spgemm_finish() == 0
        good = bh.spgemm_semiring_masked(S, Mp, Mj)       # the handle still works
        assert sr.same_bits(good, sr.semiring_masked("max_min", m, n, A, B, Mp, Mj))
        dMp, dMj = torch.from_numpy(Mp).cuda(), torch.from_numpy(Mj).cuda()
        dC = torch.zeros(len(Mj), dtype=torch.float64, device="cuda")
        assert bh.spgemm_semiring_masked_device(S, dMp, dMj, len(Mj), dC) == 0
        assert sr.same_bits(dC.cpu().numpy(), good)
    finally:
        bh.freePlatform()


# ---------------------------------------------------------------- 11. the C++ facade's extension
def test_cpp_facade_semiring_demo():
    demo_dir = os.path.join(ROOT, "tests", "semiring")
    subprocess.check_call(["make", "-C", demo_dir, "-s"])
    r = subprocess.run([os.path.join(demo_dir, "semiring_demo")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "PASS" in r.stdout
