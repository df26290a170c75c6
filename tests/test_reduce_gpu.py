"""Reductions and the diagonal scaling (bhs_csr_reduce_device, bhs_csr_scale_device) on the GPU, both builds.

Reference: tests/reduceref.py, the contract of include/bhsparse_hip.h ("reduce / scale") restated in numpy.  MIN, MAX,
ABS_MAX, COUNT and every form of the scale are compared bit for bit (NaN in class and place); the sum operators bit for bit
on small integers, and on real values against the bound of tests/valuecheck.py for ANY order of a sum's K terms (Higham
§3.1; K + 1 for SQ_PLUS, whose squares are rounded as well) -- a derived bound, no entry excluded.  Outputs carry sentinels
behind their end: nothing may be written there, and nothing at all by a refused reduction.  The kernel families that ran are
compared with what the axis and the row lengths predict."""
import functools
import os
import subprocess

import numpy as np
import pytest
import torch

from conftest import ROOT
from helpers import random_csr, real_values
import reduceref as rr
from valuecheck import bound, check_values

from benchmark_spgemm_using_csr_amd import _lib
from benchmark_spgemm_using_csr_amd.facade import (BHSPARSE_HIP, NUM_PLATFORMS, bhsparse, diagonal_csr, normalize_csr,
                                                   reduce_csr, scale_csr, smoothed_prolongator_csr,
                                                   spgemm_semiring_masked_csr)

pytestmark = pytest.mark.gpu

DTYPES = (np.float64, np.float32)
INV = _lib.BHS_ERR_INVALID_ARG
AXES = (rr.ROWS, rr.COLS, rr.ALL, rr.DIAG)
EXACT_OPS = (rr.MIN, rr.MAX, rr.ABS_MAX, rr.COUNT)
SUM_OPS = (rr.PLUS, rr.ABS_PLUS, rr.SQ_PLUS)
SENTINEL = -7.0
PAD = 64


# ---------------------------------------------------------------- helpers
def new_handle(dtype=np.float64, options=None):
    plats = [False] * NUM_PLATFORMS
    plats[BHSPARSE_HIP] = True
    bh = bhsparse(value_dtype=dtype)
    assert bh.initPlatform(plats) == 0
    for key, val in (options or {}).items():
        assert bh.set_option(key, val) == 0, key
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


def n_out(m, n, axis):
    return {rr.ROWS: m, rr.COLS: n, rr.ALL: 1, rr.DIAG: min(m, n)}[axis]


def row_families(Xp, m, n_read, prefix):
    lens = np.diff(np.asarray(Xp, np.int64))[:n_read]
    fam = {prefix + "_short"}
    if np.any((lens > 32) & (lens <= 1024)):
        fam.add(prefix + "_wave")
    if np.any(lens > 1024):
        fam.add(prefix + "_long")
    return fam


def expected_families(Xp, m, n, axis, op, flags, has_values):
    if axis == rr.COLS:
        return {"reduce_cols", "reduce_finish"}
    if axis == rr.ALL and not flags:
        return {"reduce_all", "reduce_finish"}
    if axis == rr.ROWS and not flags and (op == rr.COUNT or (not has_values and op == rr.PLUS)):
        return {"reduce_short", "reduce_finish"}                    # (the row pointer alone)
    fam = row_families(Xp, m, min(m, n) if axis == rr.DIAG else m, "reduce") | {"reduce_finish"}
    return fam | ({"reduce_all"} if axis == rr.ALL else set())


def same_exactly(got, ref, what):
    """bit for bit; a NaN in class and place"""
    assert got.dtype == ref.dtype and got.shape == ref.shape, (what, got.dtype, got.shape, ref.shape)
    gn, rn = np.isnan(got), np.isnan(ref)
    assert np.array_equal(gn, rn), (what, "NaN in other places", np.flatnonzero(gn != rn)[:5])
    bad = np.flatnonzero(bits(got)[~rn] != bits(ref)[~rn])
    assert len(bad) == 0, (what, len(bad), got[~rn][bad[:5]], ref[~rn][bad[:5]])


class Dev:
    """X on the device, uploaded once per (matrix, dtype)"""

    def __init__(self, m, n, X, dtype):
        self.m, self.n, self.dtype = m, n, dtype
        self.Xp, self.Xj = np.ascontiguousarray(X[0], np.int32), np.ascontiguousarray(X[1], np.int32)
        self.Xx = None if X[2] is None else np.ascontiguousarray(X[2], dtype)
        self.nnz = len(self.Xj)
        self.d = (up(self.Xp, np.int32), up(self.Xj, np.int32), None if self.Xx is None else up(self.Xx, dtype))


def run_reduce(bh, D, axis, op, flags=0, values=True, check_families=True, what=""):
    """the device's answer (numpy, nOut values); sentinels behind the end are checked"""
    count = n_out(D.m, D.n, axis)
    out = torch.full((count + PAD,), SENTINEL, dtype=tdt(D.dtype)).cuda()
    torch.cuda.synchronize()
    dXx = D.d[2] if values else None
    err = bh.csr_reduce_raw_device(D.m, D.n, D.nnz, dXx, D.d[0], D.d[1], axis, op, flags, out)
    assert err == 0, (what, axis, op, flags, err)
    assert bool((out[count:] == SENTINEL).all()), (what, "written past the end of d_out")
    if check_families:
        want = expected_families(D.Xp, D.m, D.n, axis, op, flags, dXx is not None)
        assert families(bh) == want, (what, axis, op, flags, families(bh), want)
    assert bh.reduce_ms >= 0.0
    return out[:count].cpu().numpy()


def check_exact(bh, D, axis, op, flags=0, values=True, what=""):
    ref, _, _ = rr.reduce(D.m, D.n, D.Xp, D.Xj, D.Xx if values else None, axis, op, flags, D.dtype)
    same_exactly(run_reduce(bh, D, axis, op, flags, values, what=what), ref, (what, axis, op, flags))


def check_bounded(bh, D, axis, op, flags=0, what=""):
    ref64, S, K = rr.reduce(D.m, D.n, D.Xp, D.Xj, D.Xx.astype(np.float64), axis, op, flags, np.float64)   # (of the values as the build holds them)
    got = run_reduce(bh, D, axis, op, flags, what=what)
    mode = "f64" if D.dtype == np.float64 else "f32_once"
    worst = check_values(ref64, S, K + (1 if op == rr.SQ_PLUS else 0), got, mode, "%s axis %d op %d flags %d: " % (what, axis, op, flags))
    print("%s axis %d op %d flags %d %s: worst err/bound %.3g" % (what, axis, op, flags, mode, worst))


# ---------------------------------------------------------------- the matrices
def shuffled(Xp, Xj, Xx, rng):
    Xj, Xx = np.array(Xj, np.int32), np.array(Xx, np.float64)
    for i in range(len(Xp) - 1):
        o = rng.permutation(Xp[i + 1] - Xp[i]) + Xp[i]
        Xj[Xp[i]:Xp[i + 1]], Xx[Xp[i]:Xp[i + 1]] = Xj[o], Xx[o]
    return Xj, Xx


@functools.lru_cache(maxsize=None)
def random_matrix(m, n, seed):
    """a few hundred rows, rows in a random order, a diagonal entry in every third row"""
    rng = np.random.default_rng(seed)
    Xp, Xj, Xx = random_csr(m, n, 0.05, rng, empty_rows=(3, m - 1))
    for i in range(0, min(m, n), 3):
        if Xp[i + 1] > Xp[i]:
            Xj[Xp[i]] = i                                           # (may repeat a column of the row: a duplicate pair)
    Xj, Xx = shuffled(Xp, Xj, Xx, rng)
    return m, n, (Xp, Xj, Xx)


LADDER = (0, 1, 16, 17, 32, 33, 64, 65, 1024, 1025, 5000)


@functools.lru_cache(maxsize=None)
def ladder_matrix():
    """row lengths on both sides of every bin boundary, twice, in a random order; rows not ascending; duplicate pairs and
    diagonal entries (some of them twice) in the rows that have room"""
    rng = np.random.default_rng(41)
    lens = rng.permutation(np.array(LADDER + LADDER))
    m, n = len(lens), 6000
    Xp = np.zeros(m + 1, np.int32)
    np.cumsum(lens, out=Xp[1:])
    Xj = np.concatenate([rng.choice(n, L, replace=False) for L in lens]).astype(np.int32)
    for i in range(m):
        a, L = Xp[i], lens[i]
        if L >= 16:
            Xj[a + 3] = i                                           # a diagonal entry ...
            Xj[a + 9] = i                                           # ... twice
            Xj[a + 5] = Xj[a + 4]                                   # a duplicate off-diagonal pair
        elif L == 1 and i % 2:
            Xj[a] = i
    Xx = rng.integers(1, 10, Xp[-1]).astype(np.float64)
    return m, n, (Xp, Xj, Xx)


@functools.lru_cache(maxsize=None)
def hub_matrix():
    """3000 x 40, column 0 in every row"""
    rng = np.random.default_rng(42)
    m, n = 3000, 40
    Xj = np.concatenate([np.concatenate(([0], 1 + rng.choice(n - 1, 3, replace=False))) for _ in range(m)]).astype(np.int32)
    Xp = (4 * np.arange(m + 1)).astype(np.int32)
    Xx = rng.integers(1, 10, 4 * m).astype(np.float64)
    return m, n, (Xp, Xj, Xx)


MATRICES = {
    "random": lambda: random_matrix(300, 300, 31),
    "wide": lambda: random_matrix(90, 400, 32),
    "tall": lambda: random_matrix(400, 90, 33),
    "ladder": ladder_matrix,
    "hub": hub_matrix,
}


def special_values(count, rng):
    v = rng.standard_normal(count)
    pick = rng.random(count)
    v[pick < 0.02] = np.nan
    v[(pick >= 0.02) & (pick < 0.05)] = np.inf
    v[(pick >= 0.05) & (pick < 0.08)] = -np.inf
    v[(pick >= 0.08) & (pick < 0.30)] = 0.0
    v[(pick >= 0.30) & (pick < 0.52)] = -0.0
    return v


def with_values(mat, vals):
    m, n, (Xp, Xj, _) = mat
    return m, n, (Xp, Xj, vals)


# ---------------------------------------------------------------- min, max, count: bit for bit
@pytest.mark.parametrize("name", sorted(MATRICES))
def test_exact_operators_on_every_axis(hd, name):
    bh, dtype = hd
    m, n, X = MATRICES[name]()
    vals = np.random.default_rng(50).standard_normal(len(X[1]))
    D = Dev(m, n, (X[0], X[1], vals), dtype)
    for axis in AXES:
        for op in EXACT_OPS:
            check_exact(bh, D, axis, op, what=name)
            if axis != rr.DIAG:
                check_exact(bh, D, axis, op, rr.OFFDIAG, what=name + " offdiag")


@pytest.mark.parametrize("name", ("random", "ladder"))
def test_signed_zeros_nan_and_infinities(hd, name):
    """-0 below +0 under min and max, a NaN comes out (under ABS_MAX too), +-Inf in class and place -- for the sums as well,
    whose class does not depend on the order"""
    bh, dtype = hd
    m, n, X = MATRICES[name]()
    D = Dev(m, n, (X[0], X[1], special_values(len(X[1]), np.random.default_rng(51))), dtype)
    for axis in AXES:
        for op in (rr.MIN, rr.MAX, rr.ABS_MAX):
            check_exact(bh, D, axis, op, what=name + " special")
        for op in SUM_OPS:
            ref, _, _ = rr.reduce(m, n, D.Xp, D.Xj, D.Xx, axis, op, 0, dtype)
            got = run_reduce(bh, D, axis, op, what=name + " special")
            for cls in (np.isnan, np.isposinf, np.isneginf):
                assert np.array_equal(cls(got), cls(ref)), (name, axis, op, cls.__name__)
    # only zeros: every order of -0 and +0
    zeros = np.where(np.random.default_rng(52).random(len(X[1])) < 0.5, -0.0, 0.0)
    Z = Dev(m, n, (X[0], X[1], zeros), dtype)
    for axis in AXES:
        for op in (rr.MIN, rr.MAX, rr.ABS_MAX):
            check_exact(bh, Z, axis, op, what=name + " zeros")


def test_without_values_every_entry_counts_as_one(hd):
    bh, dtype = hd
    m, n, X = MATRICES["ladder"]()
    D = Dev(m, n, X, dtype)
    for axis in AXES:
        for op in (rr.PLUS, rr.MAX, rr.SQ_PLUS, rr.COUNT):
            check_exact(bh, D, axis, op, values=False, what="no values")
    check_exact(bh, D, rr.ROWS, rr.PLUS, rr.OFFDIAG, values=False, what="no values offdiag")


# ---------------------------------------------------------------- the sums
@pytest.mark.parametrize("name", sorted(MATRICES))
def test_sums_of_small_integers_are_exact(hd, name):
    """values 1..9: every sum (the squares' total of the ladder: 13 k entries x 81) stays below 2^24, so every order of the
    additions gives the same bits in both builds"""
    bh, dtype = hd
    m, n, X = MATRICES[name]()
    assert len(X[1]) <= 10 ** 5 and 81 * len(X[1]) < 2 ** 24
    D = Dev(m, n, X, dtype)
    for axis in AXES:
        for op in SUM_OPS:
            check_exact(bh, D, axis, op, what=name + " integers")
            if axis != rr.DIAG:
                check_exact(bh, D, axis, op, rr.OFFDIAG, what=name + " integers offdiag")


@pytest.mark.parametrize("name", sorted(MATRICES))
def test_sums_of_real_values_within_the_bound(hd, name):
    bh, dtype = hd
    m, n, X = MATRICES[name]()
    _, A, _ = real_values("wide", n, X, X, np.random.default_rng(53), f32=dtype == np.float32)
    D = Dev(m, n, (X[0], X[1], A[2]), dtype)
    for axis in AXES:
        for op in SUM_OPS:
            check_bounded(bh, D, axis, op, what=name)
        if axis != rr.DIAG:
            check_bounded(bh, D, axis, rr.PLUS, rr.OFFDIAG, what=name + " offdiag")


@pytest.mark.parametrize("name", ("random", "ladder"))
def test_sums_repeat_bit_for_bit_on_rows_diag_and_all(hd, name):
    bh, dtype = hd
    m, n, X = MATRICES[name]()
    _, A, _ = real_values("wide", n, X, X, np.random.default_rng(54), f32=dtype == np.float32)
    D = Dev(m, n, (X[0], X[1], A[2]), dtype)
    for axis in (rr.ROWS, rr.DIAG, rr.ALL):
        for op in SUM_OPS:
            for flags in ((0,) if axis == rr.DIAG else (0, rr.OFFDIAG)):
                a = run_reduce(bh, D, axis, op, flags)
                b = run_reduce(bh, D, axis, op, flags)
                assert np.array_equal(bits(a), bits(b)), (name, axis, op, flags)


# ---------------------------------------------------------------- empty shapes
@pytest.mark.parametrize("shape", ((0, 0), (0, 5), (5, 0), (5, 7)))
def test_empty_matrices_give_the_identities(hd, shape):
    bh, dtype = hd
    m, n = shape
    D = Dev(m, n, (np.zeros(m + 1, np.int32), np.zeros(0, np.int32), np.zeros(0)), dtype)
    for axis in AXES:
        for op in range(7):
            check_exact(bh, D, axis, op, what="empty %d x %d" % shape)
    ident = {rr.MIN: np.inf, rr.MAX: -np.inf}
    for op in range(7):
        got = run_reduce(bh, D, rr.ALL, op)
        assert got.shape == (1,) and got[0] == ident.get(op, 0.0) and bool(np.signbit(got[0])) == (op == rr.MAX), op
    Zx = torch.full((PAD,), SENTINEL, dtype=tdt(dtype)).cuda()
    torch.cuda.synchronize()
    assert bh.csr_scale_raw_device(m, n, 0, Zx, D.d[0], D.d[1], 2.0, None, None, 0, Zx) == 0
    assert bool((Zx == SENTINEL).all())


# ---------------------------------------------------------------- the scale
SCALE_FORMS = (
    ("alpha", 3.5, False, False, 0),
    ("left", 1.0, True, False, 0),
    ("right", 1.0, False, True, 0),
    ("both", -0.75, True, True, 0),
    ("left div", 1.0, True, False, rr.LEFT_DIV),
    ("right div", 2.0, False, True, rr.RIGHT_DIV),
    ("both div", -3.0, True, True, rr.LEFT_DIV | rr.RIGHT_DIV),
    ("mixed", 1.0, True, True, rr.RIGHT_DIV),
)


def scale_families(Xp, m, has_left):
    return row_families(Xp, m, m, "scale") if has_left else {"scale"}


def run_scale(bh, D, alpha, left, right, flags, inplace, what):
    dl = None if left is None else up(left, D.dtype)
    dr = None if right is None else up(right, D.dtype)
    src = torch.full((D.nnz + PAD,), SENTINEL, dtype=tdt(D.dtype)).cuda()
    src[:D.nnz] = D.d[2]
    dst = src if inplace else torch.full((D.nnz + PAD,), SENTINEL, dtype=tdt(D.dtype)).cuda()
    torch.cuda.synchronize()
    err = bh.csr_scale_raw_device(D.m, D.n, D.nnz, src, D.d[0], D.d[1], alpha, dl, dr, flags, dst)
    assert err == 0, (what, err)
    assert bool((dst[D.nnz:] == SENTINEL).all()), (what, "written past the end of d_valZ")
    assert families(bh) == scale_families(D.Xp, D.m, left is not None), (what, families(bh))
    assert bh.scale_ms >= 0.0
    if not inplace:
        assert np.array_equal(bits(src[:D.nnz].cpu().numpy()), bits(D.Xx)), (what, "valX changed")
    return dst[:D.nnz].cpu().numpy()


@pytest.mark.parametrize("name", ("random", "wide", "tall", "ladder"))
def test_scale_bit_for_bit(hd, name):
    bh, dtype = hd
    m, n, X = MATRICES[name]()
    rng = np.random.default_rng(60)
    _, A, _ = real_values("wide", n, X, X, rng, f32=dtype == np.float32)
    D = Dev(m, n, (X[0], X[1], A[2]), dtype)
    left, right = rng.standard_normal(m) * 3.0, rng.standard_normal(n) * 0.2
    for form, alpha, hl, hr, flags in SCALE_FORMS:
        for inplace in (False, True):
            what = "%s %s%s" % (name, form, " in place" if inplace else "")
            ref = rr.scale(m, n, D.Xp, D.Xj, D.Xx, alpha, left if hl else None, right if hr else None, flags, dtype)
            got = run_scale(bh, D, alpha, left if hl else None, right if hr else None, flags, inplace, what)
            same_exactly(got, ref, what)


def test_scale_division_by_zero_and_non_finite_values(hd):
    bh, dtype = hd
    m, n, X = MATRICES["random"]()
    rng = np.random.default_rng(61)
    D = Dev(m, n, (X[0], X[1], special_values(len(X[1]), rng)), dtype)
    left, right = special_values(m, rng), special_values(n, rng)
    for form, alpha, hl, hr, flags in SCALE_FORMS:
        ref = rr.scale(m, n, D.Xp, D.Xj, D.Xx, alpha, left if hl else None, right if hr else None, flags, dtype)
        assert np.isinf(ref).any() and np.isnan(ref).any()
        same_exactly(run_scale(bh, D, alpha, left if hl else None, right if hr else None, flags, True, form), ref, form)


# ---------------------------------------------------------------- refusals
def bad_inputs():
    """(name the reference gives, Xp, Xj, nnzX): inputs the library's own checks must refuse; every array keeps the size the
    call is told, so nothing is read out of bounds whatever the check does"""
    m, n, (Xp, Xj, Xx) = MATRICES["random"]()
    nnz = len(Xj)
    p0 = Xp.copy(); p0[0] = 1
    pm = Xp.copy(); pm[-1] = nnz - 1
    pd = Xp.copy(); pd[10], pd[11] = Xp[11], Xp[10]
    assert pd[10] > pd[11]
    jn = Xj.copy(); jn[Xp[5]] = -1
    jb = Xj.copy(); jb[Xp[200]] = n
    return m, n, Xx, (("rowPtrX[0] != 0", p0, Xj), ("rowPtrX[m] != nnzX", pm, Xj), ("decreasing rowPtrX", pd, Xj),
                      ("column of X out of range", Xp, jn), ("column of X out of range", Xp, jb))


def test_invalid_inputs_are_refused_with_the_output_untouched(hd):
    bh, dtype = hd
    m, n, Xx, cases = bad_inputs()
    for word, Xp, Xj in cases:
        D = Dev(m, n, (Xp, Xj, Xx), dtype)
        for axis in AXES:
            for op, flags in ((rr.PLUS, 0), (rr.MAX, 0), (rr.COUNT, 0), (rr.PLUS, rr.OFFDIAG)):
                if axis == rr.DIAG and flags:
                    continue
                want = rr.invalid(m, n, Xp, Xj, axis, op, flags)
                assert want in (None, word), (want, word)
                out = torch.full((n_out(m, n, axis) + PAD,), SENTINEL, dtype=tdt(dtype)).cuda()
                torch.cuda.synchronize()
                err = bh.csr_reduce_raw_device(m, n, D.nnz, D.d[2], D.d[0], D.d[1], axis, op, flags, out)
                if want is None:                                    # a bad column in a call that reads no column
                    assert word == "column of X out of range" and not rr.reads_columns(axis, flags)
                    assert err == 0, (word, axis, op, flags, err)
                    ok = Dev(m, n, (Xp, np.zeros_like(Xj), Xx), dtype)
                    ref, _, _ = rr.reduce(m, n, Xp, ok.Xj, ok.Xx, axis, op, flags, dtype)
                    same_exactly(out[:len(ref)].cpu().numpy(), ref, (word, axis, op))
                else:
                    assert err == INV, (word, axis, op, flags, err)
                    assert bool((out == SENTINEL).all()), (word, axis, op, flags, "d_out written by a refused call")
        # the scale: the row pointer before anything is written; a bad column only with a right vector, and never outside [0, nnzX)
        left, right = up(np.ones(m), dtype), up(np.ones(n), dtype)
        for hl, hr in ((True, False), (False, True), (True, True), (False, False)):
            want = rr.invalid_scale(m, n, Xp, Xj, hl, hr, 0)
            Zx = torch.full((D.nnz + PAD,), SENTINEL, dtype=tdt(dtype)).cuda()
            torch.cuda.synchronize()
            err = bh.csr_scale_raw_device(m, n, D.nnz, D.d[2], D.d[0], D.d[1], 2.0, left if hl else None, right if hr else None, 0, Zx)
            assert err == (0 if want is None else INV), (word, hl, hr, err)
            assert bool((Zx[D.nnz:] == SENTINEL).all()), (word, hl, hr, "written outside [0, nnzX)")
            if want is not None and want != "column of X out of range":
                assert bool((Zx == SENTINEL).all()), (word, hl, hr, "d_valZ written although the row pointer was refused")


def test_host_side_refusals(hd):
    bh, dtype = hd
    m, n, X = MATRICES["random"]()
    D = Dev(m, n, X, dtype)
    out = torch.full((m + n + PAD,), SENTINEL, dtype=tdt(dtype)).cuda()
    torch.cuda.synchronize()
    red = lambda axis, op, flags, o=out, v=D.d[2]: bh.csr_reduce_raw_device(m, n, D.nnz, v, D.d[0], D.d[1], axis, op, flags, o)   # noqa: E731
    for axis, op, flags in ((4, 0, 0), (-1, 0, 0), (0, 7, 0), (0, -1, 0), (0, 0, 2), (0, 0, 3), (rr.DIAG, 0, rr.OFFDIAG)):
        assert rr.invalid(m, n, D.Xp, D.Xj, axis, op, flags) is not None
        assert red(axis, op, flags) == INV, (axis, op, flags)
    assert red(rr.ROWS, rr.PLUS, 0, o=D.d[2]) == INV                 # d_out overlapping an input
    assert red(rr.ROWS, rr.PLUS, 0, o=None) == INV
    assert bool((out == SENTINEL).all())
    sc = lambda l, r, flags, z: bh.csr_scale_raw_device(m, n, D.nnz, D.d[2], D.d[0], D.d[1], 1.0, l, r, flags, z)   # noqa: E731
    Zx = torch.full((D.nnz + PAD,), SENTINEL, dtype=tdt(dtype)).cuda()
    left, right = up(np.ones(m), dtype), up(np.ones(n), dtype)
    torch.cuda.synchronize()
    assert sc(left, right, 4, Zx) == INV
    assert sc(None, right, rr.LEFT_DIV, Zx) == INV and sc(left, None, rr.RIGHT_DIV, Zx) == INV
    assert sc(left, right, 0, D.d[2][1:]) == INV                    # overlapping valX without being it
    assert sc(left, right, 0, left) == INV and sc(left, right, 0, None) == INV
    assert bool((Zx == SENTINEL).all())
    assert bhsparse(dtype).csr_reduce_raw_device(m, n, D.nnz, None, None, None, 0, 0, 0, None) == _lib.BHS_ERR_NOT_READY
    assert bhsparse(dtype).csr_scale_raw_device(m, n, D.nnz, None, None, None, 1.0, None, None, 0, None) == _lib.BHS_ERR_NOT_READY


def test_refused_between_symbolic_and_finish():
    m = n = 300
    D = Dev(m, n, random_csr(m, n, 0.05, np.random.default_rng(34)), np.float64)
    out = torch.full((m,), SENTINEL, dtype=torch.float64).cuda()
    bh = new_handle()
    try:
        assert bh.initData_device(m, n, n, D.nnz, D.d[2], D.d[0], D.d[1], D.nnz, D.d[2], D.d[0], D.d[1]) == 0
        assert bh.spgemm_symbolic() == 0
        assert bh.csr_reduce_raw_device(m, n, D.nnz, D.d[2], D.d[0], D.d[1], rr.ROWS, rr.PLUS, 0, out) == INV
        assert bh.csr_scale_raw_device(m, n, D.nnz, D.d[2], D.d[0], D.d[1], 2.0, None, None, 0, out) == INV
        assert bool((out == SENTINEL).all())
        assert bh.spgemm_numeric(0, m) == 0 and bh.spgemm_finish() == 0
        assert bh.csr_reduce_raw_device(m, n, D.nnz, D.d[2], D.d[0], D.d[1], rr.ROWS, rr.PLUS, 0, out) == 0
        same_exactly(out.cpu().numpy(), rr.reduce(m, n, D.Xp, D.Xj, D.Xx, rr.ROWS, rr.PLUS)[0], "after finish")
        bh.free_mem()
    finally:
        bh.freePlatform()


# ---------------------------------------------------------------- the handle is left alone
@pytest.mark.parametrize("dtype", DTYPES)
def test_reduce_and_scale_leave_the_handle_alone(dtype, oracle):
    from benchmark_spgemm_using_csr_amd import gallery
    rp, col = (np.ascontiguousarray(a, np.int32) for a in gallery.poisson_csr("poisson27pt", 12, 12, 12))
    m = len(rp) - 1
    val = np.ascontiguousarray(np.random.default_rng(15).integers(1, 10, len(col)), dtype)
    ym, yn, Y = MATRICES["ladder"]()
    D = Dev(ym, yn, Y, dtype)
    bh = new_handle(dtype, {"class_path": 2})
    try:
        Cp = np.zeros(m + 1, np.int32)
        assert bh.initData(m, m, m, len(col), val, rp, col, len(col), val, rp, col, Cp) == 0
        assert bh.spgemm() == 0 and bh.spgemm() == 0                # (the second one launches speculatively where the class path runs)
        keys = ("class_state", "mixed_rows", "spec_launches", "spec_refuted", "b_sorted", "max_row_a", "max_row_b",
                "select_dropped", "add_inplace_used", "extract_reordered_rows")
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
        for axis in AXES:
            check_exact(bh, D, axis, rr.PLUS, what="beside a multiply")
        unchanged("after reductions")
        left = np.random.default_rng(16).integers(1, 5, ym).astype(np.float64)
        same_exactly(run_scale(bh, D, 2.0, left, None, rr.LEFT_DIV, False, "beside a multiply"),
                     rr.scale(ym, yn, D.Xp, D.Xj, D.Xx, 2.0, left, None, rr.LEFT_DIV, dtype), "beside a multiply")
        unchanged("after a scale")
        # the product itself, straight from the device pointers: its row sums and its total
        T = torch.full((m + 1,), SENTINEL, dtype=tdt(dtype)).cuda()
        torch.cuda.synchronize()
        assert bh.csr_reduce_raw_device(m, m, nnzC, ptrs[2], ptrs[0], ptrs[1], rr.ROWS, rr.PLUS, 0, T) == 0
        same_exactly(T[:m].cpu().numpy(), rr.reduce(m, m, Cp, Cj, Cx, rr.ROWS, rr.PLUS, 0, dtype)[0], "row sums of C")
        unchanged("after reducing C")
        assert bh.spgemm() == 0                                     # and the next multiply is what it was
        assert bh.get_info("class_state") == before["class_state"] and bh.get_nnzC() == nnzC
        bh.free_mem()
    finally:
        bh.freePlatform()


# ---------------------------------------------------------------- compositions
@pytest.mark.parametrize("dtype", DTYPES)
def test_normalize_makes_the_columns_stochastic(dtype):
    m, n, X = MATRICES["tall"]()
    n += 3                                                          # (three columns without an entry)
    rng = np.random.default_rng(70)
    vals = np.abs(real_values("wide", n, X, X, rng, f32=dtype == np.float32)[1][2])
    Zx, norms = normalize_csr(m, n, X[0], X[1], vals, _lib.BHS_AXIS_COLS, 1, value_dtype=dtype)
    ref_n, S, K = rr.reduce(m, n, X[0], X[1], vals, rr.COLS, rr.ABS_PLUS, 0, dtype)
    mode = "f64" if dtype == np.float64 else "f32_once"
    check_values(ref_n.astype(np.float64), S, K, norms, mode, "column norms: ")
    div = np.where(norms == 0, 1, norms).astype(dtype)
    same_exactly(Zx, rr.scale(m, n, X[0], X[1], vals, 1.0, None, div, rr.RIGHT_DIV, dtype), "normalised values")
    # the column sums of the result: 1 where the column has an entry -- K quotients of relative error u each (S = sum = 1
    # up to u), then K additions: the bound of K + 1 terms with the value type's u --, 0 where it has none
    sums, _, Kz = rr.reduce(m, n, X[0], X[1], Zx, rr.COLS, rr.PLUS, 0, np.float64)
    assert 0 in Kz and np.all(sums[Kz == 0] == 0.0)
    u = 2.0 ** -53 if dtype == np.float64 else 2.0 ** -24
    assert np.all(np.abs(sums[Kz > 0] - 1.0) <= 2.0 * (Kz[Kz > 0] + 1) * u)
    # rows, the other norms
    for norm, op in ((2, rr.SQ_PLUS), ("inf", rr.ABS_MAX)):
        Zx, norms = normalize_csr(m, n, X[0], X[1], vals, _lib.BHS_AXIS_ROWS, norm, value_dtype=dtype)
        ref_n = rr.reduce(m, n, X[0], X[1], vals, rr.ROWS, op, 0, dtype)[0]
        if norm == 2:
            assert np.allclose(norms, np.sqrt(ref_n.astype(np.float64)), rtol=1e-6 if dtype == np.float32 else 1e-14)
        else:
            same_exactly(norms, ref_n, "row inf-norms")
        div = np.where(norms == 0, 1, norms).astype(dtype)
        same_exactly(Zx, rr.scale(m, n, X[0], X[1], vals, 1.0, div, None, rr.LEFT_DIV, dtype), "row-normalised values")


@pytest.mark.parametrize("dtype", DTYPES)
def test_smoothed_prolongator_against_scipy(dtype):
    import scipy.sparse as sp
    from benchmark_spgemm_using_csr_amd import gallery
    rp, col = gallery.poisson_csr("poisson5pt", 12, 12)
    n = len(rp) - 1
    rng = np.random.default_rng(71)
    # (1 + U[0,1)) x 2^U{-3..3}, diagonal included: no product or sum near under- or overflow, no zero on the diagonal
    val = ((1.0 + rng.random(len(col))) * np.exp2(rng.integers(-3, 4, len(col)))).astype(dtype)
    nc = n // 4
    Tj = (np.arange(n) // 4).astype(np.int32)                       # piecewise constant: four fine points an aggregate
    Tp = np.arange(n + 1, dtype=np.int32)
    Tx = np.ones(n, dtype)
    omega = 2.0 / 3.0
    Pp, Pj, Px, info = smoothed_prolongator_csr(n, nc, rp, col, val, Tp, Tj, Tx, omega, value_dtype=dtype)
    A = sp.csr_matrix((val.astype(np.float64), col, rp), shape=(n, n))
    T = sp.csr_matrix((Tx.astype(np.float64), Tj, Tp), shape=(n, nc))
    d = A.diagonal()
    same_exactly(diagonal_csr(n, n, rp, col, val, value_dtype=dtype), d.astype(dtype), "diag(A)")
    # the library rounds -omega D^-1 A to the value type before the multiply: the reference does the same
    Sx = rr.scale(n, n, rp, col, val, -omega, d.astype(dtype), None, rr.LEFT_DIV, dtype)
    S = sp.csr_matrix((Sx.astype(np.float64), col, rp), shape=(n, n))
    ST = (S @ T).tocsr()
    absST = (abs(S) @ abs(T)).tocsr()
    ones = lambda M: sp.csr_matrix((np.ones(M.nnz), M.indices, M.indptr), shape=M.shape)   # noqa: E731
    P = (ST + T).tocsr()
    # (scipy drops nothing here: no product cancels to an exact zero pattern entry, the pattern is the union)
    pat = (ones(S) @ ones(T) + ones(T)).tocsr()
    pat.sort_indices()
    assert np.array_equal(Pp, pat.indptr) and np.array_equal(Pj, pat.indices), "the pattern differs"
    dense = lambda M: np.asarray(M.todense())[np.repeat(np.arange(n), np.diff(pat.indptr)), pat.indices]   # noqa: E731
    # the bound of bhs_spgemm_add with alpha = beta = 1, as tests/test_add_gpu.py derives it: the product's entry within
    # valuecheck.bound of the exact one, then one sum in double and one rounding to the output format
    mode = "f64" if dtype == np.float64 else "f32_atomic"
    u_out = 2.0 ** -53 if dtype == np.float64 else 2.0 ** -24
    Sv, t = dense(absST), dense(T)
    lim = bound(mode, dense(ST), Sv, dense(ones(S) @ ones(T))) + (u_out + 3 * 2.0 ** -53) * (Sv + np.abs(t))
    err = np.abs(Px.astype(np.float64) - dense(P))
    print("P = T - omega D^-1 A T %s: worst err/bound %.3g" % (mode, float(np.max(err / np.maximum(lim, 1e-300)))))
    assert np.all(err <= lim)
    assert info["nnzC"] == pat.nnz and info["reduce_ms"] >= 0 and info["scale_ms"] >= 0


@pytest.mark.parametrize("dtype", DTYPES)
def test_triangle_count_is_the_total_of_the_pair_product(dtype):
    import scipy.sparse as sp
    rng = np.random.default_rng(72)
    nodes = 200
    G = sp.random(nodes, nodes, density=0.08, format="csr", random_state=np.random.RandomState(7))
    G = ((G + G.T) != 0).astype(np.float64)
    L = sp.tril(G, -1).tocsr()
    L.sort_indices()
    want = int(round(((L @ L).multiply(L)).sum()))
    assert want > 0 and rng is not None
    Lp, Lj, Lx = L.indptr.astype(np.int32), L.indices.astype(np.int32), np.ones(L.nnz)
    valC, _ = spgemm_semiring_masked_csr(nodes, nodes, nodes, Lp, Lj, Lx, Lp, Lj, Lx, Lp, Lj, _lib.BHS_SR_PLUS_PAIR, value_dtype=dtype)
    total, info = reduce_csr(nodes, nodes, Lp, Lj, valC, _lib.BHS_AXIS_ALL, _lib.BHS_RED_PLUS, value_dtype=dtype)
    assert total.dtype == np.dtype(dtype) and total.shape == (1,) and float(total[0]) == float(want), (total, want)
    assert {s["name"] for s in info["kernels"] if s["launches"] > 0} == {"reduce_all", "reduce_finish"}
    Zx, _ = scale_csr(nodes, nodes, Lp, Lj, valC, alpha=0.5, value_dtype=dtype)
    assert np.array_equal(Zx, (valC * 0.5).astype(dtype))


def test_cpp_demo_runs():
    demo_dir = os.path.join(ROOT, "tests", "reduce")
    subprocess.check_call(["make", "-C", demo_dir, "-s"])
    out = subprocess.run([os.path.join(demo_dir, "reduce_demo")], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "reduce / scale 5 x 7, 12 entries: PASS" in out.stdout
