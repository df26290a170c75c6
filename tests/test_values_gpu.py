"""Real and non-finite values through every kernel family, against the a-priori error bound of tests/valuecheck.py.

The parity tests multiply small integers, whose products and sums are exact in any order and in either precision: they
cannot see a product or a sum formed in float in the double library, nor the float build's promise of INTEGRATION.md §7
(products and sums in double, one rounding per entry, except the long-row and hub bins' float atomics).  Here every
family runs on two generators of real values (helpers.real_values: "wide" and the cancelling "cancel"), on both builds,
and its values must stay within the bound of its mode; then on inputs holding NaN, +-Inf and explicit zeros, whose
non-finite entries must come out in the same places and classes as the oracle's."""
import os
import zlib

import numpy as np
import pytest

import test_masked_gpu as masked
import test_parity_gpu as parity
from helpers import VALUE_KINDS, poisson_case, random_csr, real_values
from valuecheck import check_bounded, on_pattern

from benchmark_spgemm_using_csr_amd import facade as bhmod
from benchmark_spgemm_using_csr_amd import gallery
from benchmark_spgemm_using_csr_amd.facade import spgemm_masked_csr

pytestmark = pytest.mark.gpu

# families whose float build adds rounded products with float global atomics (include/bhsparse_hip.h)
F32_ATOMIC = {"numeric_long_rows", "numeric_hub_rows", "masked_long", "masked_hub"}
BUILDS = {"f64": np.float64, "f32": np.float32}


# ---------------------------------------------------------------- shapes (the parity tests' builders)
def _quarter_wave():
    """test_quarter_wave_rows (5, 5, 1): rows of 5 A entries x 5-entry B rows, neighbouring B rows overlapping."""
    rng = np.random.default_rng(505)
    nA, lenB, k, n, m = 5, 5, 400, 5000, 203
    Bp = np.arange(k + 1, dtype=np.int32) * lenB
    Bj = np.concatenate([(j // 2) * 3 % (n - 4 * lenB) + np.sort(rng.choice(2 * lenB, lenB, replace=False))
                         for j in range(k)]).astype(np.int32)
    lens = np.full(m, nA)
    lens[::7] = 0
    lens[3::11] = nA - 1
    Ap = np.zeros(m + 1, np.int32)
    Ap[1:] = np.cumsum(lens)
    Aj = np.concatenate([np.sort(rng.choice(k, L, replace=False)) for L in lens]).astype(np.int32)
    return m, k, n, (Ap, Aj, None), (Bp, Bj, None)


def _ladder():
    """Rows of A of 1 .. 150 entries on B rows of ~40 random columns out of 200 000: rows of C from ~40 to ~6000 entries,
    one or more rows in every numeric bin up to numeric_wg<8192>; and rows of 20 entries on 200 narrow B rows (3 of the
    first 40 columns each), too many A entries for the quarter-wave kernel: numeric_wave<64>."""
    rng = np.random.default_rng(77)
    k, n = 3000, 200000
    Bp, Bj, _ = random_csr(k, n, 40 / n, rng)
    narrow = [np.sort(rng.choice(40, 3, replace=False)) for _ in range(200)]
    Bp = np.concatenate((Bp, Bp[-1] + np.cumsum([len(r) for r in narrow]))).astype(np.int32)
    Bj = np.concatenate([Bj] + narrow).astype(np.int32)
    rows = [np.sort(rng.choice(np.arange(k, k + 200), 20, replace=False)) for _ in range(8)]
    k += 200
    for L in (1, 2, 3, 4, 6, 8, 10, 13, 16, 20, 25, 30, 36, 42, 50, 60, 70, 85, 100, 120, 150):
        rows += [np.sort(rng.choice(k - 200, L, replace=False)) for _ in range(4)]
    Ap = np.zeros(len(rows) + 1, np.int32)
    Ap[1:] = np.cumsum([len(r) for r in rows])
    return len(rows), k, n, (Ap, np.concatenate(rows).astype(np.int32), None), (Bp, Bj, None)


def _long_rows():
    """test_long_rows_bitmap_accumulators at n = 200 000: rows of C beyond every LDS table, columns hit once and many times."""
    n, k = 200000, 2000
    rng = np.random.default_rng(n % 1000)
    pool = np.sort(rng.choice(n, 5000, replace=False))
    rowsB = [np.sort(rng.choice(pool, int(rng.integers(20, 60)), replace=False) if j < k // 2 else
                     rng.choice(n, int(rng.integers(20, 60)), replace=False)) for j in range(k)]
    rowsB[k - 1] = np.array([0, 15, 16, 31, 32, n - 2, n - 1])
    Bp = np.zeros(k + 1, np.int32); Bp[1:] = np.cumsum([len(r) for r in rowsB])
    rowsA = [np.sort(rng.choice(k, 1500, replace=False)), np.sort(rng.choice(k, 10, replace=False)), np.empty(0, np.int64),
             np.sort(rng.choice(k // 2, 600, replace=False)), np.arange(k - 700, k)]
    Ap = np.zeros(len(rowsA) + 1, np.int32); Ap[1:] = np.cumsum([len(r) for r in rowsA])
    return len(rowsA), k, n, (Ap, np.concatenate(rowsA).astype(np.int32), None), (Bp, np.concatenate(rowsB).astype(np.int32), None)


def _windows():
    """test_wave_per_row_column_windows at n = 70 000 (B's columns skewed like an R-MAT graph's)."""
    n, k = 70000, 3000
    rng = np.random.default_rng(n % 977)
    skewed = lambda cnt: np.unique(np.minimum((n * rng.random(cnt) ** 3).astype(np.int64), n - 1))   # noqa: E731
    rowsB = [skewed(int(rng.integers(150, 500))) for _ in range(k)]
    rowsB[5] = np.empty(0, np.int64)
    rowsB[6] = np.array([0, n - 1])
    Bp = np.zeros(k + 1, np.int32); Bp[1:] = np.cumsum([len(r) for r in rowsB])
    free = np.setdiff1d(np.arange(40, k), [5, 6])
    rowsA = [np.sort(rng.choice(free, int(rng.integers(8, 30)), replace=False)) for _ in range(150)]
    rowsA += [np.sort(rng.choice(free, L, replace=False)) for L in (64, 65, 128, 129)] + [np.array([5, 6, 50, 51]), np.empty(0, np.int64)]
    Ap = np.zeros(len(rowsA) + 1, np.int32); Ap[1:] = np.cumsum([len(r) for r in rowsA])
    return len(rowsA), k, n, (Ap, np.concatenate(rowsA).astype(np.int32), None), (Bp, np.concatenate(rowsB).astype(np.int32), None)


def _hub():
    """test_hub_rows_split_across_workgroups, "dense_rows": three rows of 16 000 entries in a sparse 40 000^2 matrix."""
    rng = np.random.default_rng(11)
    n = 40000
    rp, col = parity._dense_row_case(n, 9, {5, 17000, n - 1}, 16000, rng)
    return n, n, n, (rp, col, None), (rp, col, None)


def _stencil(name, *dims):
    m, rp, col, _ = poisson_case(name, *dims)
    return m, m, m, (rp, col, None), (rp, col, None)


def _fem4():
    """poisson9pt (x) ones(4, 4): 36 entries a row, 1296 products -- beyond the register kernels' tables, the big-class kernel."""
    _, rp0, col0, _ = poisson_case("poisson9pt", 23, 19, 1)
    m, rp, col = parity._kron_ones(rp0, col0, 4)
    return m, m, m, (rp, col, None), (rp, col, None)


def _p9_perturbed():
    """test_row_class_path_mixed_mode, "p9_extra_entries": a stencil with a few rows holding extra entries (mixed mode)."""
    rp, col = gallery.poisson_csr("poisson9pt", 120, 90, 1)
    m = len(rp) - 1
    rp, col = gallery.perturb_rows_csr(rp, col, m, 0.003, seed=9)
    return m, m, m, (rp, col, None), (rp, col, None)


# name: (shape, options, kernels that must have run, multiply in row ranges, float build's mode)
GENERAL = {
    "lane": (lambda: _stencil("poisson5pt", 37, 41), {"class_path": 0, "lane_rows": 2, "lane_numeric": 1}, {"numeric_lane"}, False, "f32_once"),
    "quad": (_quarter_wave, {"class_path": 0, "lane_rows": 0, "wave_first": 0}, {"numeric_quad<64>"}, False, "f32_once"),
    # (the double build's LDS-bitmap kernel takes the rows of numeric_wg<4096> and numeric_wg<8192> in one launch, named
    # after the latter; the float build keeps both bins' tables: run_general asks for numeric_wg<4096> there)
    "wave_wg": (_ladder, {"class_path": 0}, {"numeric_wave<64>", "numeric_wave<128>", "numeric_wave<256>", "numeric_wave<512>",
                                             "numeric_wave<1024>", "numeric_wg<2048>", "numeric_wg<8192>"},
                False, "f32_once"),
    "long_rows_lds": (_long_rows, {"class_path": 0}, {"numeric_long_rows"}, False, "f32_atomic"),
    "long_rows_hbm": (_long_rows, {"class_path": 0, "lds_bitmap": 0}, {"numeric_long_rows"}, False, "f32_atomic"),
    "column_windows": (_windows, {"class_path": 0, "window_bitmap": 2}, {"b_windows", "numeric_long_rows"}, False, "f32_atomic"),
    "hub_rows": (_hub, {"class_path": 0}, {"numeric_hub_rows"}, False, "f32_atomic"),
    "class_numeric_0": (lambda: _stencil("poisson7pt", 17, 16, 15), {"class_path": 2, "class_numeric": 0},
                        {"classify_rows", "class_patterns", "numeric_class"}, False, "f32_once"),
    "class_numeric_1": (lambda: _stencil("poisson7pt", 17, 16, 15), {"class_path": 2, "class_numeric": 1},
                        {"classify_rows", "class_patterns", "numeric_class"}, False, "f32_once"),
    "class_numeric_2": (lambda: _stencil("poisson7pt", 17, 16, 15), {"class_path": 2, "class_numeric": 2},
                        {"classify_rows", "class_patterns", "numeric_class"}, False, "f32_once"),
    "big_class": (_fem4, {"class_path": 2}, {"numeric_class"}, False, "f32_once"),
    "mixed": (_p9_perturbed, {"class_path": 2}, {"numeric_class"}, False, "f32_once"),
    "row_ranges_general": (_ladder, {"class_path": 0}, {"numeric_wave<256>", "numeric_wg<2048>"}, True, "f32_once"),
    "row_ranges_mixed": (_p9_perturbed, {"class_path": 2}, {"numeric_class"}, True, "f32_once"),
}

# name: (test_masked_gpu._fam_case's kind, the kernel that must have run, float build's mode)
MASKED = {"masked_short": ("short", "masked_short", "f32_once"), "masked_wave": ("wave", "masked_wave", "f32_once"),
          "masked_wave_big": ("wave_big", "masked_wave", "f32_once"), "masked_long": ("long", "masked_long", "f32_atomic"),
          "masked_hub": ("hub", "masked_hub", "f32_atomic"), "masked_hub_lds": ("hub_lds", "masked_hub", "f32_atomic"),
          "masked_hub_slice": ("hub_slice", "masked_hub", "f32_atomic")}


# ---------------------------------------------------------------- runners
def multiply(m, k, n, A, B, options, vd, ranges=False):
    """One multiply on a fresh handle (in row ranges: symbolic half, numeric half on a few ranges, finish).  Returns
    ((Cp, Cj, Cx), names of the kernels that ran, facts from the handle)."""
    plats = [False] * bhmod.NUM_PLATFORMS
    plats[bhmod.BHSPARSE_HIP] = True
    bh = bhmod.bhsparse(value_dtype=vd)
    assert bh.initPlatform(plats) == 0
    try:
        for key, val in options.items():
            assert bh.set_option(key, val) == 0, key
        Ax, Bx = np.ascontiguousarray(A[2], vd), np.ascontiguousarray(B[2], vd)
        Ap, Aj, Bp, Bj = (np.ascontiguousarray(x, np.int32) for x in (A[0], A[1], B[0], B[1]))
        Cp = np.zeros(m + 1, np.int32)
        assert bh.initData(m, k, n, len(Aj), Ax, Ap, Aj, len(Bj), Bx, Bp, Bj, Cp) == 0
        if ranges:
            cuts = [0, m // 5, m // 5, m // 2 + 3, m]
            assert bh.spgemm_symbolic() == 0
            for a, b in zip(cuts[:-1], cuts[1:]):
                assert bh.spgemm_numeric(min(a, m), min(b, m)) == 0
            assert bh.spgemm_finish() == 0
        else:
            assert bh.spgemm() == 0
        Cj = np.empty(bh.get_nnzC(), np.int32)
        Cx = np.empty(bh.get_nnzC(), vd)
        assert bh.get_C(Cj, Cx) == 0
        names = {s["name"] for s in bh.kernel_stats() if s["launches"]}
        facts = {"mixed_rows": bh.get_info("mixed_rows"), "class_state": bh.get_info("class_state")}
        if "numeric_class" in names:
            facts["class_tables_usable"] = bh.class_tables_device()[-1]
        assert bh.free_mem() == 0
    finally:
        bh.freePlatform()
    return (Cp, Cj, Cx), names, facts


def f32_mode(names, declared=None):
    mode = "f32_atomic" if names & F32_ATOMIC else "f32_once"
    if declared is not None:
        assert mode == declared, ("the kernels that ran do not match the float mode §7 gives this family", sorted(names))
    return mode


def _report(what, worst):
    print("%-44s worst err/bound %.3g" % (what, worst))


def run_general(oracle, family, A, B, shape, build, what):
    make, opts, want, ranges, declared = GENERAL[family]
    m, k, n = shape
    vd = BUILDS[build]
    got, names, facts = multiply(m, k, n, A, B, opts, vd, ranges=ranges)
    if family == "wave_wg" and build == "f32":
        want = want | {"numeric_wg<4096>"}
    assert want <= names, (family, sorted(want - names), sorted(names))
    if family.startswith("class_numeric") or family == "big_class":
        assert "upper_bound" not in names and facts["mixed_rows"] == 0, (family, sorted(names), facts)
    if family == "big_class":
        assert facts["class_tables_usable"] is False, facts             # (the big kernel's lists: no rebuildable tables)
    if family.endswith("mixed"):
        assert facts["mixed_rows"] > 0 and facts["class_state"] == 2, facts
    mode = "f64" if build == "f64" else f32_mode(names, declared)
    worst = check_bounded(oracle, m, k, n, A, B, got, mode, what=what + ": ")
    _report(what + " " + mode, worst)
    return got


def run_masked(oracle, family, A, B, shape, Mp, Mj, opts, build, what):
    m, k, n = shape
    vd = BUILDS[build]
    valC, info = spgemm_masked_csr(m, k, n, *A, *B, Mp, Mj, options=opts, value_dtype=vd)
    names = {s["name"] for s in info["kernels"] if s["launches"]}
    _, fam, declared = MASKED[family]
    assert fam in names, (family, sorted(names))
    mode = "f64" if build == "f64" else f32_mode(names, declared)
    worst = check_bounded(oracle, m, k, n, A, B, valC, mode, mask=(Mp, Mj), what=what + ": ")
    _report(what + " " + mode, worst)
    return valC


def _masked_shape(family, oracle):
    (m, k, n, A, B), opts = masked._fam_case(MASKED[family][0])
    rng = np.random.default_rng(99)
    Mp, Mj = masked.random_mask(rng, m, n, masked.pattern_of(oracle, m, k, n, A, B), frac_in=0.9, extra_per_row=5)
    return (m, k, n), A, B, Mp, Mj, opts


# ---------------------------------------------------------------- the family table on real values
@pytest.mark.parametrize("build", sorted(BUILDS))
@pytest.mark.parametrize("kind", VALUE_KINDS)
@pytest.mark.parametrize("family", sorted(GENERAL))
def test_family_real_values(oracle, family, kind, build):
    m, k, n, A, B = GENERAL[family][0]()
    k2, A, B = real_values(kind, k, A, B, np.random.default_rng(zlib.crc32((family + kind).encode())), f32=build == "f32")
    run_general(oracle, family, A, B, (m, k2, n), build, "%s %s %s" % (family, kind, build))


@pytest.mark.parametrize("build", sorted(BUILDS))
@pytest.mark.parametrize("kind", VALUE_KINDS)
@pytest.mark.parametrize("family", sorted(MASKED))
def test_masked_family_real_values(oracle, family, kind, build):
    (m, k, n), A, B, Mp, Mj, opts = _masked_shape(family, oracle)
    k2, A, B = real_values(kind, k, A, B, np.random.default_rng(len(family) * 7 + len(kind)), f32=build == "f32")
    run_masked(oracle, family, A, B, (m, k2, n), Mp, Mj, opts, build, "%s %s %s" % (family, kind, build))


# ---------------------------------------------------------------- non-finite inputs
def poison(X, rng, nan=0, pinf=0, ninf=0, zero=0):
    """X's values with a few NaN, +Inf, -Inf and explicitly stored zeros at random entries (0 x Inf gives NaN)."""
    x = np.array(X[2], np.float64)
    idx = rng.choice(len(x), nan + pinf + ninf + zero, replace=False)
    x[idx[:nan]] = np.nan
    x[idx[nan:nan + pinf]] = np.inf
    x[idx[nan + pinf:nan + pinf + ninf]] = -np.inf
    x[idx[nan + pinf + ninf:]] = 0.0
    return (X[0], X[1], x)


def _non_finite_inputs(k, A, B, rng):
    _, A, B = real_values("wide", k, A, B, rng)
    if len(A[1]) < 8:                                               # (a hub row of two A entries: one NaN, one zero)
        A = poison(A, rng, nan=1, zero=1)
    else:
        A = poison(A, rng, nan=2, pinf=1, ninf=1, zero=max(2, len(A[1]) // 50))
    B = poison(B, rng, nan=1, pinf=2, ninf=2, zero=max(2, len(B[1]) // 50))
    return A, B


@pytest.mark.parametrize("build", sorted(BUILDS))
@pytest.mark.parametrize("family", sorted(GENERAL))
def test_family_non_finite_inputs(oracle, family, build):
    m, k, n, A, B = GENERAL[family][0]()
    A, B = _non_finite_inputs(k, A, B, np.random.default_rng(zlib.crc32(family.encode())))
    ref = oracle.spgemm(m, k, n, *A, *B)[2]
    assert np.isnan(ref).any() and np.isinf(ref).any(), family        # (the draw did put non-finite values into C)
    run_general(oracle, family, A, B, (m, k, n), build, "%s non-finite %s" % (family, build))


@pytest.mark.parametrize("build", sorted(BUILDS))
@pytest.mark.parametrize("family", sorted(MASKED))
def test_masked_family_non_finite_inputs(oracle, family, build):
    """... and in the masked multiply, where a NaN whose products all fall outside M must not reach valC: every other
    entry of A·B that the NaNs reach is taken out of the mask."""
    (m, k, n), A, B, Mp, Mj, opts = _masked_shape(family, oracle)
    A, B = _non_finite_inputs(k, A, B, np.random.default_rng(len(family)))
    full = oracle.spgemm(m, k, n, *A, *B)
    onM = on_pattern(full, n, Mp, Mj)
    ckeys = np.repeat(np.arange(m, dtype=np.int64), np.diff(full[0])) * n + full[1]
    drop = set(ckeys[np.isnan(full[2]) | np.isinf(full[2])][::2].tolist())
    mkeys = np.repeat(np.arange(m, dtype=np.int64), np.diff(np.asarray(Mp, np.int64))) * n + Mj
    keep = np.array([key not in drop for key in mkeys.tolist()], bool)
    if drop:
        Mp, Mj = gallery._csr_from_pairs(m, n, (mkeys // n)[keep], (mkeys % n)[keep])
        onM = on_pattern(full, n, Mp, Mj)
    assert np.isnan(full[2]).sum() + np.isinf(full[2]).sum() > np.isnan(onM).sum() + np.isinf(onM).sum(), family
    run_masked(oracle, family, A, B, (m, k, n), Mp, Mj, opts, build, "%s non-finite %s" % (family, build))


# ---------------------------------------------------------------- real-valued draws of the soaks (seeds of their own)
SOAK = os.environ.get("BHS_SOAK") == "1"
GENERAL_SEEDS = [8000, 8001, 8002, 8003, 8004, 8005, 8006, 8007, 8008, 8009] + (list(range(8010, 8100)) if SOAK else [])
MIXED_SEEDS = [8005, 8008, 8009, 8012, 8017, 8019, 8021, 8022, 8023, 8028] + (list(range(8030, 8080)) if SOAK else [])
MASKED_SEEDS = list(range(5000, 5010)) + (list(range(5010, 5200)) if SOAK else [])
SOAK_PRODUCTS = 3000000 if not SOAK else 30000000       # (the oracle runs three times on up to twice this many products)


def _soak_values(seed, k, A, B):
    kind = VALUE_KINDS[seed % 2]
    build = "f32" if seed % 3 == 2 else "f64"
    k2, A, B = real_values(kind, k, A, B, np.random.default_rng(seed), f32=build == "f32")
    return kind, build, k2, A, B


def _products(A, B):
    return int(np.diff(np.asarray(B[0], np.int64))[np.asarray(A[1])].sum())


@pytest.mark.parametrize("seed", GENERAL_SEEDS)
def test_general_pipeline_real_value_draws(oracle, seed):
    (m, k, n, how), A, B = parity._general_soak_inputs(seed)
    if _products(A, B) > SOAK_PRODUCTS:                        # (the first rows of A that hold that many products)
        ends = np.cumsum(np.diff(np.asarray(B[0], np.int64))[A[1]])[np.maximum(np.asarray(A[0][1:], np.int64) - 1, 0)]
        m = max(1, int(np.searchsorted(ends, SOAK_PRODUCTS)))
        A = (A[0][:m + 1].copy(), A[1][:A[0][m]].copy(), A[2][:A[0][m]].copy())
    kind, build, k2, A, B = _soak_values(seed, k, A, B)
    for opts, ranges in (({}, False), ({"class_path": 0}, True)):
        got, names, _ = multiply(m, k2, n, A, B, opts, BUILDS[build], ranges=ranges)
        mode = "f64" if build == "f64" else f32_mode(names)
        worst = check_bounded(oracle, m, k2, n, A, B, got, mode, what="general draw %d (%s): " % (seed, how))
        _report("general draw %d %s %s%s" % (seed, kind, mode, " ranges" if ranges else ""), worst)


@pytest.mark.parametrize("seed", MIXED_SEEDS)
def test_mixed_mode_real_value_draws(oracle, seed):
    (m, k, n, sa, sb, na, nb, noise), A, B = parity._mixed_soak_inputs(seed)
    kind, build, k2, A, B = _soak_values(seed, k, A, B)
    for ranges in (False, True):
        got, names, facts = multiply(m, k2, n, A, B, {"class_path": 2}, BUILDS[build], ranges=ranges)
        mode = "f64" if build == "f64" else f32_mode(names)
        worst = check_bounded(oracle, m, k2, n, A, B, got, mode, what="mixed draw %d: " % seed)
        _report("mixed draw %d %s %s%s (class_state %d)" % (seed, kind, mode, " ranges" if ranges else "", facts["class_state"]), worst)


@pytest.mark.parametrize("seed", MASKED_SEEDS)
def test_masked_real_value_draws(oracle, seed):
    (m, k, n), A, B, Mp, Mj, opts = masked._soak_inputs(seed, oracle)
    kind, build, k2, A, B = _soak_values(seed, k, A, B)
    valC, info = spgemm_masked_csr(m, k2, n, *A, *B, Mp, Mj, options=opts, value_dtype=BUILDS[build])
    names = {s["name"] for s in info["kernels"] if s["launches"]}
    mode = "f64" if build == "f64" else f32_mode(names)
    worst = check_bounded(oracle, m, k2, n, A, B, valC, mode, mask=(Mp, Mj), what="masked draw %d: " % seed)
    _report("masked draw %d %s %s" % (seed, kind, mode), worst)
