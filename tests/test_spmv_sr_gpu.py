"""Semiring CSR x dense with mask and accumulate (bhs_csr_spmv_semiring_device, bhs_csr_spmm_semiring_device) and the
traversals on top of it (graph.py) on the GPU, both builds.

Reference: tests/spmvsrref.py, the contract of include/bhsparse_hip.h ("semiring CSR x dense") restated in numpy.  The seven
semirings whose result does not depend on an order are compared bit for bit (a NaN in class and place); PLUS_TIMES on small
integers as numbers and on real values against the bound of tests/valuecheck.py for ANY order of an element's K = entries
+ 1 operations (one more with ACCUM) -- a derived bound, no entry excluded.  `changed` equals the reference's count exactly,
in every case.  Every output array carries sentinels behind its end and in the gaps of its leading dimension, the gaps of X
and M hold NaN, and wherever ACCUM is off the output is prefilled with NaN: none of it may reach a result, nothing may be
written there, and what the mask does not select must still hold what it held.  The kernel families that ran are compared
with what the row lengths and the mask predict."""
import functools
import os
import subprocess

import numpy as np
import pytest
import torch

from conftest import ROOT, load_golden
from helpers import wide_values
import semiringref as srf
import spmvsrref as sr
from valuecheck import check_values

from benchmark_spgemm_using_csr_amd import _lib, dense, gallery, graph
from benchmark_spgemm_using_csr_amd.facade import BHSPARSE_HIP, NUM_PLATFORMS, BhsparseError, bhsparse, select_spec

pytestmark = pytest.mark.gpu

DTYPES = (np.float64, np.float32)
INV = _lib.BHS_ERR_INVALID_ARG
SENTINEL = -7.0
PAD = 64
KS = (1, 2, 3, 4, 5, 8, 9, 16, 17, 32, 33, 64, 65, 130)
NAMES = tuple(srf.SEMIRINGS)
ALL_K = ("min_plus", "max_min", "plus_times")
FEW_K = tuple(s for s in NAMES if s not in ALL_K)
ACC, CMP = _lib.BHS_MV_ACCUM, _lib.BHS_MV_MASK_COMPLEMENT


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


def expected_families(Ap, sel):
    """srmv_short always; the other two where a row of their bin holds a selected element"""
    lens = np.diff(np.asarray(Ap, np.int64))
    read = sel.any(axis=1) if len(lens) else np.zeros(0, bool)
    fam = {"srmv_short"}
    if np.any(read & (lens > 32) & (lens <= 1024)):
        fam.add("srmv_wave")
    if np.any(read & (lens > 1024)):
        fam.add("srmv_long")
    return fam


def same_numbers(got, ref, what):
    """equal as numbers: +-0 compare equal, a NaN in class and place"""
    assert got.dtype == ref.dtype and got.shape == ref.shape, (what, got.dtype, got.shape, ref.shape)
    gn, rn = np.isnan(got), np.isnan(ref)
    assert np.array_equal(gn, rn), (what, "NaN in other places", np.argwhere(gn != rn)[:5])
    bad = np.argwhere(~rn & (got != ref))
    assert len(bad) == 0, (what, len(bad), bad[:5], got[tuple(bad[0])], ref[tuple(bad[0])])


def agrees(name, got, ref, what):
    if name == "plus_times":                                        # (the sign of a zero sum is not specified)
        same_numbers(got, ref, what)
    else:
        assert srf.same_bits(got, ref), (what, np.argwhere(bits(got) != bits(ref))[:5])


class Dev:
    """A on the device, uploaded once per (matrix, dtype)"""

    def __init__(self, m, n, A, dtype):
        self.m, self.n, self.dtype = m, n, dtype
        self.Ap, self.Aj = np.ascontiguousarray(A[0], np.int32), np.ascontiguousarray(A[1], np.int32)
        self.Ax = None if A[2] is None else np.ascontiguousarray(A[2], dtype)
        self.nnz = len(self.Aj)
        self.d = (up(self.Ap, np.int32), up(self.Aj, np.int32), None if self.Ax is None else up(self.Ax, dtype))


def run(bh, name, D, X, Y=None, mask=None, accumulate=False, complement=False, gap=0, values=True, vector_call=None, want=0,
        what=""):
    """The device's answer (numpy m x k, changed) to X (numpy n x k), Y (numpy m x k; None without accumulate: the output is
    then prefilled with NaN) and mask (numpy m x k or None).  gap: ld = k + gap for X, M and Y.  The sentinels behind Y and in
    its gaps are checked, the gaps of X and M hold NaN; with want == 0 the families that ran too.  vector_call:
    bhs_csr_spmv_semiring_device (default where k == 1 and gap == 0)."""
    m, n, k = D.m, D.n, X.shape[1]
    ld = k + gap
    t = tdt(D.dtype)
    dX = torch.full((max(n, 1), ld), float("nan"), dtype=t).cuda()
    dX[:n, :k] = up(X, D.dtype)
    dM = None
    if mask is not None:
        dM = torch.full((max(m, 1), ld), float("nan"), dtype=t).cuda()
        dM[:m, :k] = up(mask, D.dtype)
    buf = torch.full((m * ld + PAD,), SENTINEL, dtype=t).cuda()
    view = buf[:m * ld].view(m, ld)
    view[:, :k] = float("nan") if Y is None else up(Y, D.dtype)
    assert Y is not None or not accumulate
    torch.cuda.synchronize()
    dAx = D.d[2] if values else None
    flags = (ACC if accumulate else 0) | (CMP if complement else 0)
    if vector_call is None:
        vector_call = k == 1 and gap == 0
    bh.spmv_changed = -1
    if vector_call:
        err = dense.csr_spmv_semiring_raw_device(bh, name, m, n, D.nnz, dAx, D.d[0], D.d[1], dX, flags, dM, buf)
    else:
        err = dense.csr_spmm_semiring_raw_device(bh, name, m, n, D.nnz, dAx, D.d[0], D.d[1], k, dX, ld, flags, dM, ld, buf, ld)
    assert err == want, (what, name, k, gap, err)
    assert bool((buf[m * ld:] == SENTINEL).all()), (what, name, k, gap, "written past the end of Y")
    assert bool((view[:, k:] == SENTINEL).all()), (what, name, k, gap, "written into the gaps of Y's leading dimension")
    if want == 0:
        fam = expected_families(D.Ap, sr.selected(mask, complement, m, k))
        assert families(bh) == fam, (what, name, k, families(bh), fam)
        assert bh.spmv_ms >= 0.0 and bh.spmv_changed >= 0
    else:
        assert bh.spmv_changed == -1
    return view[:, :k].cpu().numpy(), bh.spmv_changed


def check(bh, name, D, X, Y=None, mask=None, accumulate=False, complement=False, gap=0, values=True, vector_call=None, ref=None,
          what=""):
    """one call against the reference (computed here unless given): the values, what was not selected, the count"""
    if ref is None:
        ref = sr.spmm_semiring(name, D.m, D.n, D.Ap, D.Aj, D.Ax if values else None, X, Y, mask, accumulate, complement, D.dtype)
    got, changed = run(bh, name, D, X, Y, mask, accumulate, complement, gap, values, vector_call, what=what)
    agrees(name, got, ref[0], (what, name, X.shape[1], gap, accumulate, complement))
    assert changed == ref[1], (what, name, X.shape[1], gap, accumulate, complement, changed, ref[1])
    return got


# ---------------------------------------------------------------- the matrices
SPECIAL = (0, 1, 2, 16, 17, 32, 33, 64, 1024, 1025, 2500)
N_ROWS = 2803


def rows_matrix(lens, n, seed):
    """rows of these lengths in this order: columns in no order, duplicate pairs in the rows that have room"""
    rng = np.random.default_rng(seed)
    lens = np.asarray(lens, np.int64)
    m = len(lens)
    Ap = np.zeros(m + 1, np.int32)
    np.cumsum(lens, out=Ap[1:])
    Aj = np.concatenate([rng.choice(n, L, replace=False) for L in lens] + [np.zeros(0, np.int64)]).astype(np.int32)
    for i in range(m):
        a, L = Ap[i], lens[i]
        if L >= 16:
            Aj[a + 5] = Aj[a + 4]                                   # a duplicate pair, side by side ...
            Aj[a + L - 1] = Aj[a]                                   # ... and at the row's two ends
    return m, n, Ap, Aj


@functools.lru_cache(maxsize=None)
def ladder():
    """m = 300: every special length once among short random rows -- every bin, both bin boundaries, two workgroups of the
    short kernel; the longest rows in the second one"""
    rng = np.random.default_rng(41)
    lens = rng.integers(0, 9, 300)
    lens[rng.choice(256, 8, replace=False)] = SPECIAL[:8]
    lens[256 + rng.choice(44, 3, replace=False)] = SPECIAL[8:]
    return rows_matrix(lens, N_ROWS, 42)


def values_for(name, count, rng, integers=False):
    """edge values (zeros of both signs, infinities) a semiring can take without turning everything into NaN; NaNs are
    placed by hand by the tests that want them"""
    if name in ("plus_times", "plus_pair") or integers:
        return rng.integers(-4, 5, count).astype(np.float64)
    return srf.edge_values(rng, count, plus_safe=name in ("min_plus", "max_plus"))


@functools.lru_cache(maxsize=None)
def ladder_dev(name, dtype):
    m, n, Ap, Aj = ladder()
    Ax = values_for(name, len(Aj), np.random.default_rng(43))
    if name not in ("plus_times", "plus_pair"):
        Ax[Ap[5]:Ap[5] + 1] = np.nan                                # a NaN by hand (where row 5 has an entry)
    return Dev(m, n, (Ap, Aj, Ax), dtype)


def dense_for(name, rows, k, seed):
    rng = np.random.default_rng(seed)
    V = values_for(name, rows * k, rng).reshape(rows, k)
    if name not in ("plus_times", "plus_pair") and rows * k > 7:
        V.flat[7] = np.nan
    return V


def random_mask(m, k, seed):
    """per element: 0, -0 (not set); a number, NaN (set)"""
    rng = np.random.default_rng(seed)
    return rng.choice(np.array([0.0, -0.0, 2.0, np.nan, -1.0, 0.0]), (m, k))


@functools.lru_cache(maxsize=None)
def ladder_case(name, k, dtype):
    """X, Y, M and the two references on the ladder, computed once per (semiring, k, build): no mask and no accumulation;
    a random mask (complemented for odd k) with accumulation"""
    D = ladder_dev(name, dtype)
    X, Y, M = dense_for(name, D.n, k, 100 + k), dense_for(name, D.m, k, 200 + k), random_mask(D.m, k, 300 + k)
    plain = sr.spmm_semiring(name, D.m, D.n, D.Ap, D.Aj, D.Ax, X, dtype=dtype)
    masked = sr.spmm_semiring(name, D.m, D.n, D.Ap, D.Aj, D.Ax, X, Y, M, True, bool(k & 1), dtype)
    return X, Y, M, plain, masked


def on_the_ladder(bh, dtype, name, k, gap):
    D = ladder_dev(name, dtype)
    X, Y, M, plain, masked = ladder_case(name, k, dtype)
    check(bh, name, D, X, gap=gap, ref=plain, what="ladder")
    check(bh, name, D, X, Y, M, True, bool(k & 1), gap=gap, ref=masked, what="ladder masked")
    if k == 1 and gap == 0:                                         # the matrix call with one column is the vector call
        for vector_call in (False, True):
            check(bh, name, D, X, Y, M, True, True, vector_call=vector_call, ref=masked, what="ladder vector")


def test_the_ladder_holds_every_bin_edge():
    m, n, Ap, Aj = ladder()
    lens = np.diff(Ap)
    assert m == 300 and set(SPECIAL) <= set(lens) and (lens[256:] > 1024).any() and (lens[:256] > 32).any()
    # every PLUS_TIMES sum of the exact tests stays an integer below 2^24: exact in both builds whatever the order
    assert 2500 * 4 * 4 + 4 < 2 ** 24


@pytest.mark.parametrize("gap", (0, 3))
@pytest.mark.parametrize("k", KS)
def test_every_column_count_on_the_ladder(hd, k, gap):
    bh, dtype = hd
    for name in ALL_K:
        on_the_ladder(bh, dtype, name, k, gap)


@pytest.mark.parametrize("gap", (0, 3))
@pytest.mark.parametrize("k", (1, 3, 64, 65))
@pytest.mark.parametrize("name", FEW_K)
def test_the_other_semirings_on_the_ladder(hd, name, k, gap):
    bh, dtype = hd
    on_the_ladder(bh, dtype, name, k, gap)


# ---------------------------------------------------------------- masks
@pytest.mark.parametrize("name", ("min_plus", "or_and", "plus_pair"))
def test_masks_plain_and_complemented(hd, name):
    bh, dtype = hd
    D = ladder_dev(name, dtype)
    lens = np.diff(D.Ap)
    for k in (1, 5):
        X, Y = dense_for(name, D.n, k, 11), dense_for(name, D.m, k, 12)
        rows = np.arange(D.m)[:, None] + np.zeros(k, np.int64)
        masks = {"all set": np.ones((D.m, k)), "none set": np.zeros((D.m, k)), "alternate rows": (rows & 1) * 3.0,
                 "NaN and -0": np.where(rows % 3 == 0, np.nan, -0.0)}
        if k > 1:
            masks["per element"] = random_mask(D.m, k, 13)
        one = np.zeros((D.m, k))
        one[int(np.flatnonzero(lens == 1025)[0]), k // 2] = 1.0     # exactly one element of a 1025-entry row
        masks["one element of a long row"] = one
        for what, M in masks.items():
            for complement in (False, True):
                check(bh, name, D, X, None, M, False, complement, gap=3 if k == 5 else 0, what=what)
                check(bh, name, D, X, Y, M, True, complement, what=what + " accumulate")
        # nothing selected: the row pointer is still checked, nothing else runs, nothing changes
        assert run(bh, name, D, X, None, masks["none set"])[1] == 0 and families(bh) == {"srmv_short"}
        assert run(bh, name, D, X, None, one)[1] <= 1 and families(bh) == {"srmv_short", "srmv_long"}


# ---------------------------------------------------------------- accumulate
@pytest.mark.parametrize("name", NAMES)
def test_accumulate_into_identity_nan_infinities_winners_and_losers(hd, name):
    bh, dtype = hd
    D = ladder_dev(name, dtype)
    k = 3
    X = dense_for(name, D.n, k, 21)
    t = sr.spmm_semiring(name, D.m, D.n, D.Ap, D.Aj, D.Ax, X, dtype=dtype)[0].astype(np.float64)
    rng = np.random.default_rng(22)
    finite = np.where(np.isfinite(t), t, 0.0)
    pick = rng.integers(0, 7, t.shape)
    Y = np.select([pick == 0, pick == 1, pick == 2, pick == 3, pick == 4, pick == 5],
                  [np.full(t.shape, srf.identity(name)), np.full(t.shape, np.nan), np.full(t.shape, np.inf),
                   np.full(t.shape, -np.inf), finite + 1.0, finite - 1.0], finite)        # (6: y_old equals t)
    if name in ("plus_times", "plus_pair"):
        Y = np.where(np.isfinite(Y), np.round(Y), Y)
    out = check(bh, name, D, X, Y, None, True, what="accumulate")
    ref_changed = sr.spmm_semiring(name, D.m, D.n, D.Ap, D.Aj, D.Ax, X, Y, None, True, dtype=dtype)[1]
    assert 0 < ref_changed < t.size and np.isnan(out[pick == 1]).all() == (name != "or_and")
    # accumulating a second time changes nothing more (min, max, or: idempotent)
    if name not in ("plus_times", "plus_pair"):
        assert run(bh, name, D, X, out, None, True)[1] == 0


def test_without_values_every_entry_counts_as_one(hd):
    bh, dtype = hd
    for name in ("min_plus", "max_times", "or_and", "plus_times", "plus_pair"):
        D = ladder_dev(name, dtype)
        X = dense_for(name, D.n, 3, 31)
        check(bh, name, D, X, values=False, what="pattern")
        check(bh, name, D, X[:, :1], values=False, what="pattern")


# ---------------------------------------------------------------- shapes at the edge
@pytest.mark.parametrize("name", ("max_plus", "min_max", "plus_times", "plus_pair"))
def test_degenerate_shapes(hd, name):
    bh, dtype = hd
    rng = np.random.default_rng(51)
    shapes = {
        "one row": (1, 40, np.array([0, 7]), rng.integers(0, 40, 7)),
        "no rows": (0, 40, np.array([0]), np.zeros(0, np.int64)),
        "no columns": (40, 0, np.zeros(41, np.int64), np.zeros(0, np.int64)),
        "one pair many times": (3, 5, np.array([0, 0, 70, 70]), np.full(70, 2)),
        "descending columns": (2, 50, np.array([0, 40, 50]), np.concatenate([np.arange(40)[::-1], np.arange(10)[::-1]])),
    }
    for what, (m, n, Ap, Aj) in shapes.items():
        D = Dev(m, n, (Ap, Aj, values_for(name, len(Aj), rng)), dtype)
        for k in (1, 4):
            X, Y, M = dense_for(name, n, k, 52), dense_for(name, m, k, 53), random_mask(m, k, 54)
            check(bh, name, D, X, what=what)
            check(bh, name, D, X, Y, M, True, True, gap=3, what=what)
        if what == "one row":
            # 7 entries in all: one family.  (That the host then skips the queue lengths' round trip -- smv_run's
            # nnzA > 32 branch -- is not observable from here and is not asserted.)
            assert families(bh) == {"srmv_short"}


# ---------------------------------------------------------------- PLUS_TIMES on real values: within the bound
def test_plus_times_real_values_within_the_bound(hd):
    bh, dtype = hd
    m, n, Ap, Aj = ladder()
    rng = np.random.default_rng(61)
    rounded = lambda v: np.ascontiguousarray(v, dtype).astype(np.float64)   # noqa: E731  (the values as the build holds them)
    D = Dev(m, n, (Ap, Aj, rounded(wide_values(len(Aj), rng))), dtype)
    mode = "f64" if dtype == np.float64 else "f32_once"
    for k in (1, 5, 17):
        X, Y = rounded(wide_values(n * k, rng)).reshape(n, k), rounded(wide_values(m * k, rng)).reshape(m, k)
        M = random_mask(m, k, 62)
        for accumulate, mask in ((False, None), (True, None), (True, M)):
            _, _, ref, S, K = sr.spmm_semiring("plus_times", m, n, Ap, Aj, D.Ax.astype(np.float64), X, Y if accumulate else None,
                                                     mask, accumulate, False, np.float64, with_bound=True)
            assert np.array_equal(K[:, 0], np.diff(Ap) + 1 + accumulate)
            got, got_changed = run(bh, "plus_times", D, X, Y if accumulate else None, mask, accumulate, gap=3 if k == 5 else 0)
            sel = sr.selected(mask, False, m, k)
            worst = check_values(ref[sel], S[sel], K[sel], got[sel], mode, "plus_times k %d accumulate %d: " % (k, accumulate))
            print("plus_times k %d accumulate %d mask %d %s: worst err/bound %.3g" % (k, accumulate, mask is not None, mode, worst))
            assert np.array_equal(bits(got[~sel]), bits(np.ascontiguousarray(Y, dtype)[~sel]))
            # the count from the reference in the build's own value type: what is stored is compared with what was there
            assert got_changed == sr.spmm_semiring("plus_times", m, n, Ap, Aj, D.Ax, X, Y if accumulate else None, mask, accumulate,
                                                   False, dtype)[1]


# ---------------------------------------------------------------- repeatable
@pytest.mark.parametrize("name", NAMES)
def test_two_calls_give_the_same_bits(hd, name):
    bh, dtype = hd
    m, n, Ap, Aj = ladder()
    rng = np.random.default_rng(70)
    D = Dev(m, n, (Ap, Aj, wide_values(len(Aj), rng)), dtype)
    k = 5
    X, Y, M = wide_values(n * k, rng).reshape(n, k), wide_values(m * k, rng).reshape(m, k), random_mask(m, k, 71)
    a, ca = run(bh, name, D, X, Y, M, True, True)
    b, cb = run(bh, name, D, X, Y, M, True, True)
    assert np.array_equal(bits(a), bits(b)) and ca == cb
    a, ca = run(bh, name, D, X)
    b, cb = run(bh, name, D, X)
    assert np.array_equal(bits(a), bits(b)) and ca == cb


def test_a_null_changed_out_leaves_the_values_as_they_are(hd):
    """the C-ABI with a NULL changed_out (the Python calls always pass one): the same bits in Y.  (That the kernels then skip
    the count cannot be seen through the ABI and is not asserted; tools/srmv_case.py times it.)"""
    import ctypes as C
    bh, dtype = hd
    name, k = "min_plus", 5
    D = ladder_dev(name, dtype)
    X, Y, M, plain, masked = ladder_case(name, k, dtype)
    dX, dM = up(X, dtype), up(M, dtype)
    for ref, flags, mask in ((plain, 0, None), (masked, ACC | CMP, dM)):
        dY = up(Y, dtype)
        torch.cuda.synchronize()
        ms = C.c_double(-1.0)
        err = bh._lib.bhs_csr_spmm_semiring_device(bh._h, _lib.SEMIRINGS[name], D.m, D.n, D.nnz, D.d[2].data_ptr(), D.d[0].data_ptr(),
                                                   D.d[1].data_ptr(), k, dX.data_ptr(), k, flags, mask.data_ptr() if mask is not None else None,
                                                   k, dY.data_ptr(), k, None, C.byref(ms))
        assert err == 0 and ms.value >= 0.0
        got = dY.cpu().numpy()
        assert srf.same_bits(got, ref[0])                            # (what the mask does not select still holds Y)


# ---------------------------------------------------------------- refusals
def bad_inputs():
    """(the word spmvsrref gives, Ap, Aj): inputs the device's checks must refuse; every array keeps the size the call is
    told, so nothing is read out of bounds whatever the check does"""
    m, n, Ap, Aj = ladder()
    nnz = len(Aj)
    p0 = Ap.copy(); p0[0] = 1
    pm = Ap.copy(); pm[-1] = nnz - 1
    pd = Ap.copy()
    r = int(np.flatnonzero(np.diff(Ap) > 0)[3])
    pd[r], pd[r + 1] = Ap[r + 1], Ap[r]
    assert pd[r] > pd[r + 1]
    lens = np.diff(Ap)
    cases = [("rowPtrA[0] != 0", p0, Aj, None), ("rowPtrA[m] != nnzA", pm, Aj, None), ("decreasing rowPtrA", pd, Aj, None)]
    for L, col in ((17, -1), (17, n), (64, n), (64, -1), (2500, n), (2500, -1)):   # a bad column in every bin
        j = Aj.copy()
        row = int(np.flatnonzero(lens == L)[0])
        j[Ap[row] + L // 2] = col
        cases.append(("column of A out of range", Ap, j, row))
    return m, n, cases


def test_invalid_inputs_are_refused(hd):
    bh, dtype = hd
    m, n, cases = bad_inputs()
    name = "min_plus"
    good = ladder_dev(name, dtype)
    for word, Ap, Aj, row in cases:
        assert sr.invalid(m, n, Ap, Aj) == word and word in sr.DEVICE_REFUSALS
        D = Dev(m, n, (Ap, Aj, good.Ax), dtype)
        for k, gap in ((1, 0), (5, 3)):
            X, Y = dense_for(name, n, k, 81), dense_for(name, m, k, 82)
            run(bh, name, D, X, Y, None, True, gap=gap, want=INV, what=word)   # (Y may be partly written; never outside its m x k elements)
            unread = np.ones((m, k))
            if row is None:
                # the row pointer is checked in every row, selected or not
                run(bh, name, D, X, Y, np.zeros((m, k)), True, gap=gap, want=INV, what=word + ", nothing selected")
            else:
                # a column is checked where it is read: not in a row the mask does not select ...
                unread[row] = 0.0
                assert sr.invalid(m, n, Ap, Aj, k, has_mask=True, rows_read=unread.any(axis=1)) is None
                check(bh, name, D, X, Y, unread, True, gap=gap, what=word + ", row not selected")
                # ... and it is, as soon as one element of that row is selected
                unread[row, k - 1] = 1.0
                run(bh, name, D, X, Y, unread, True, gap=gap, want=INV, what=word + ", one element selected")
            # the handle still answers a valid call
            Xg, Yg, Mg, plain, masked = ladder_case(name, k, dtype)
            check(bh, name, good, Xg, gap=gap, ref=plain, what="after " + word)


def test_host_side_refusals_leave_y_untouched(hd):
    bh, dtype = hd
    D = ladder_dev("min_plus", dtype)
    m, n, k, ld = D.m, D.n, 4, 6
    t = tdt(dtype)
    X = torch.ones((n, ld), dtype=t).cuda()
    M = torch.ones((m, ld), dtype=t).cuda()
    Y = torch.full((m * ld + PAD,), SENTINEL, dtype=t).cuda()
    torch.cuda.synchronize()
    Ap, Aj, Ax = D.d

    def mm(sr_=1, m=m, n=n, nnz=D.nnz, Ax=Ax, Ap=Ap, Aj=Aj, k=k, X=X, ldX=ld, flags=ACC, M=M, ldM=ld, Y=Y, ldY=ld):
        return dense.csr_spmm_semiring_raw_device(bh, sr_, m, n, nnz, Ax, Ap, Aj, k, X, ldX, flags, M, ldM, Y, ldY)

    def mv(sr_=1, m=m, n=n, nnz=D.nnz, Ax=Ax, Ap=Ap, Aj=Aj, x=X, flags=ACC, mask=M, y=Y):
        return dense.csr_spmv_semiring_raw_device(bh, sr_, m, n, nnz, Ax, Ap, Aj, x, flags, mask, y)

    refused = {
        "negative size": (mm(m=-1), mm(n=-1), mm(nnz=-1), mv(m=-1), mv(n=-1), mv(nnz=-1)),
        "k < 1": (mm(k=0), mm(k=-3)),
        "ldX < k": (mm(ldX=k - 1),),
        "ldY < k": (mm(ldY=k - 1),),
        "NULL rowPtrA": (mm(Ap=None), mv(Ap=None)),
        "NULL colIndA": (mm(Aj=None), mv(Aj=None)),
        "NULL x": (mm(X=None), mv(x=None)),
        "NULL y": (mm(Y=None), mv(y=None)),
        "unknown semiring": (mm(sr_=8), mm(sr_=-1), mv(sr_=8), mv(sr_=100)),
        "unknown flag": (mm(flags=4), mm(flags=ACC | 8), mv(flags=-1)),
        "ldM < k": (mm(ldM=k - 1),),
        "complement without a mask": (mm(flags=CMP, M=None), mv(flags=ACC | CMP, mask=None)),
        "y overlaps an input": (mm(Y=X), mm(Y=Ax), mm(Y=M), mv(y=X), mv(y=Ax), mv(y=M), mm(X=Y[k:]), mv(x=Y[m - 1:]), mm(M=Y[k:]),
                                mv(mask=Y[m - 1:])),
    }
    assert sorted(refused) == sorted(sr.HOST_REFUSALS)
    for word, codes in refused.items():
        assert all(c == INV for c in codes), (word, codes)
    assert bool((Y == SENTINEL).all()), "y written by a refused call"
    # what is legal: the mask overlapping X, a leading dimension of M below k without a mask, NULL arrays without entries or rows
    assert mm(M=X[:m], ldM=ld) == 0 and mm(M=None, ldM=0) == 0
    Y.fill_(SENTINEL)
    torch.cuda.synchronize()
    Z = torch.zeros(41, dtype=torch.int32).cuda()
    assert dense.csr_spmv_semiring_raw_device(bh, "min_plus", 40, 0, 0, None, Z, None, None, 0, None, Y) == 0
    assert bool((Y[:40] == float("inf")).all()) and bool((Y[40:] == SENTINEL).all()) and bh.spmv_changed == 0
    assert dense.csr_spmv_semiring_raw_device(bh, "min_plus", 0, 40, 0, None, Z, None, X, 0, None, None) == 0
    nr = _lib.BHS_ERR_NOT_READY
    assert dense.csr_spmv_semiring_raw_device(bhsparse(dtype), 1, 0, 0, 0, None, None, None, None, 0, None, None) == nr


def test_refused_between_symbolic_and_finish():
    from helpers import random_csr
    m = n = 300
    A = random_csr(m, n, 0.05, np.random.default_rng(34))
    D = Dev(m, n, A, np.float64)
    x = dense_for("min_plus", n, 1, 35)
    dx = up(x, np.float64)
    y = torch.full((m + PAD,), SENTINEL, dtype=torch.float64).cuda()
    bh = new_handle()
    try:
        assert bh.initData_device(m, n, n, D.nnz, D.d[2], D.d[0], D.d[1], D.nnz, D.d[2], D.d[0], D.d[1]) == 0
        assert bh.spgemm_symbolic() == 0
        assert dense.csr_spmv_semiring_raw_device(bh, "min_plus", m, n, D.nnz, D.d[2], D.d[0], D.d[1], dx, 0, None, y) == INV
        assert dense.csr_spmm_semiring_raw_device(bh, "min_plus", m, n, D.nnz, D.d[2], D.d[0], D.d[1], 1, dx, 1, 0, None, 1, y, 1) == INV
        assert bool((y == SENTINEL).all())
        assert bh.spgemm_numeric(0, m) == 0 and bh.spgemm_finish() == 0
        assert dense.csr_spmv_semiring_raw_device(bh, "min_plus", m, n, D.nnz, D.d[2], D.d[0], D.d[1], dx, 0, None, y) == 0
        ref, changed = sr.spmv_semiring("min_plus", m, n, D.Ap, D.Aj, D.Ax, x[:, 0])
        assert srf.same_bits(y[:m].cpu().numpy(), ref) and bh.spmv_changed == changed and bool((y[m:] == SENTINEL).all())
        bh.free_mem()
    finally:
        bh.freePlatform()


# ---------------------------------------------------------------- the handle is left alone
@pytest.mark.parametrize("dtype", DTYPES)
def test_a_semiring_call_leaves_the_handle_alone(dtype, oracle):
    g = load_golden("p9_12.npz")
    m, kk, n = int(g["m"]), int(g["k"]), int(g["n"])
    rng = np.random.default_rng(15)
    Ap, Aj, Bp, Bj = (np.ascontiguousarray(g[key], np.int32) for key in ("Ap", "Aj", "Bp", "Bj"))
    Ax, Bx = (np.ascontiguousarray(rng.integers(1, 5, len(j)), dtype) for j in (Aj, Bj))
    keys = ("class_state", "mixed_rows", "spec_launches", "spec_refuted", "b_sorted", "max_row_a", "max_row_b",
            "select_dropped", "add_inplace_used", "extract_reordered_rows")

    def multiply(bh):
        Cp = np.zeros(m + 1, np.int32)
        assert bh.initData(m, kk, n, len(Aj), Ax, Ap, Aj, len(Bj), Bx, Bp, Bj, Cp) == 0
        assert bh.spgemm() == 0 and bh.spgemm() == 0                # (the second one launches speculatively where the class path runs)
        return Cp, state(bh)

    def state(bh):
        """what the last multiply reports: the handle's figures and the kernels that ran"""
        return {key: bh.get_info(key) for key in keys}, sorted((s["name"], s["launches"]) for s in bh.kernel_stats() if s["launches"])

    fresh = new_handle(dtype, {"class_path": 2})
    try:
        multiply(fresh)
        assert fresh.spgemm() == 0
        fresh_third = state(fresh)
        fresh.free_mem()
    finally:
        fresh.freePlatform()
    bh = new_handle(dtype, {"class_path": 2})
    try:
        Cp, (before, _) = multiply(bh)
        nnzC, ptrs = bh.get_nnzC(), bh.get_C_device()
        Cj, Cx = np.empty(nnzC, np.int32), np.empty(nnzC, dtype)
        assert bh.get_C(Cj, Cx) == 0
        ref = oracle.spgemm(m, kk, n, Ap, Aj, Ax.astype(np.float64), Bp, Bj, Bx.astype(np.float64))
        assert np.array_equal(Cp, ref[0]) and np.array_equal(Cj, ref[1]) and np.array_equal(Cx, ref[2].astype(dtype))
        for name, k in (("min_plus", 1), ("or_and", 5)):
            on_the_ladder(bh, dtype, name, k, 0)
            assert {key: bh.get_info(key) for key in keys} == before, name
            assert bh.get_nnzC() == nnzC and bh.get_C_device() == ptrs, name
            j2, x2 = np.empty(nnzC, np.int32), np.empty(nnzC, dtype)
            assert bh.get_C(j2, x2) == 0
            assert np.array_equal(j2, Cj) and np.array_equal(bits(x2), bits(Cx)) and np.array_equal(bh.get_rowptrC(), Cp), name
        # the product itself, straight from the device pointers: one relaxation step through C
        x = dense_for("min_plus", n, 1, 16)
        y = torch.full((m + PAD,), SENTINEL, dtype=tdt(dtype)).cuda()
        dx = up(x, dtype)
        torch.cuda.synchronize()
        assert dense.csr_spmv_semiring_raw_device(bh, "min_plus", m, n, nnzC, ptrs[2], ptrs[0], ptrs[1], dx, 0, None, y) == 0
        want, changed = sr.spmv_semiring("min_plus", m, n, Cp, Cj, Cx, x[:, 0], dtype=dtype)
        assert srf.same_bits(y[:m].cpu().numpy(), want) and bh.spmv_changed == changed and bool((y[m:] == SENTINEL).all())
        assert bh.spgemm() == 0                                     # and the next multiply is what a fresh handle's third is
        assert state(bh) == fresh_third and bh.get_nnzC() == nnzC
        assert np.array_equal(bh.get_rowptrC(), ref[0])
        j2, x2 = np.empty(nnzC, np.int32), np.empty(nnzC, dtype)
        assert bh.get_C(j2, x2) == 0 and np.array_equal(j2, ref[1]) and np.array_equal(bits(x2), bits(ref[2].astype(dtype)))

        def served():
            """what the getters serve: the count, the row pointer, the columns, the values' bits, the device pointers"""
            nnz = bh.get_nnzC()
            j, x = np.empty(nnz, np.int32), np.empty(nnz, dtype)
            assert bh.get_C(j, x) == 0
            return nnz, bh.get_rowptrC().copy(), j, bits(x).copy(), bh.get_C_device()

        def same_served(a, b, what):
            assert a[0] == b[0] and a[4] == b[4], what
            assert all(np.array_equal(u, v) for u, v in zip(a[1:4], b[1:4])), what
        # a selected C served by the getters survives semiring calls (with and without a mask, both entry points) ...
        assert bh.spgemm_select(select_spec(band=(None, -1))) == 0
        sel = served()
        dropped = bh.get_info("select_dropped")
        assert 0 < sel[0] < nnzC and dropped > 0
        for name, k in (("min_plus", 1), ("or_and", 5)):
            on_the_ladder(bh, dtype, name, k, 0)
            same_served(served(), sel, "a served selection after " + name)
            assert bh.get_info("select_dropped") == dropped
        # ... and so does a served sum C = 2 A B - D, D the diagonal
        nd = min(m, n)
        Dp = np.minimum(np.arange(m + 1), nd).astype(np.int32)
        Dj, Dx = np.arange(nd, dtype=np.int32), np.ascontiguousarray(rng.integers(1, 5, nd), dtype)
        assert bh.spgemm_add(2.0, -1.0, Dp, Dj, Dx) == 0
        added = served()
        assert added[0] >= nnzC and not np.array_equal(added[3], bits(Cx))
        for name, k in (("min_plus", 1), ("or_and", 5)):
            on_the_ladder(bh, dtype, name, k, 0)
            same_served(served(), added, "a served sum after " + name)
        bh.free_mem()
    finally:
        bh.freePlatform()


# ---------------------------------------------------------------- the tensor call and the convenience
@pytest.mark.parametrize("dtype", DTYPES)
def test_tensor_call_takes_the_leading_dimensions_from_the_strides(dtype):
    name, k = "max_min", 5
    D = ladder_dev(name, dtype)
    X, Y, M = dense_for(name, D.n, k, 91), dense_for(name, D.m, k, 92), random_mask(D.m, k, 93)
    t = tdt(dtype)
    wideX = torch.full((D.n, k + 3), float("nan"), dtype=t).cuda()
    wideX[:, :k] = up(X, dtype)
    wideM = torch.full((D.m, k + 1), float("nan"), dtype=t).cuda()
    wideM[:, :k] = up(M, dtype)
    wideY = torch.full((D.m, k + 2), SENTINEL, dtype=t).cuda()
    wideY[:, :k] = up(Y, dtype)
    bh = new_handle(dtype)
    try:
        out, changed = dense.csr_spmm_semiring_device(bh, name, D.m, D.n, D.d, wideX[:, :k], wideY[:, :k], wideM[:, :k], True, True)
        ref = sr.spmm_semiring(name, D.m, D.n, D.Ap, D.Aj, D.Ax, X, Y, M, True, True, dtype)
        assert out.data_ptr() == wideY.data_ptr() and changed == ref[1]
        assert srf.same_bits(wideY[:, :k].cpu().numpy(), ref[0]) and bool((wideY[:, k:] == SENTINEL).all())
        y, changed = dense.csr_spmm_semiring_device(bh, _lib.BHS_SR_MAX_MIN, D.m, D.n, D.d, up(X[:, 0], dtype))
        ref = sr.spmv_semiring(name, D.m, D.n, D.Ap, D.Aj, D.Ax, X[:, 0], dtype=dtype)
        assert y.shape == (D.m,) and srf.same_bits(y.cpu().numpy(), ref[0]) and changed == ref[1]
        bad = D.Aj.copy()
        bad[D.Ap[np.flatnonzero(np.diff(D.Ap) > 0)[0]]] = D.n
        with pytest.raises(BhsparseError) as ei:
            dense.csr_spmm_semiring_device(bh, name, D.m, D.n, (D.d[0], up(bad, np.int32), D.d[2]), up(X[:, 0], dtype))
        assert ei.value.code == INV
    finally:
        bh.freePlatform()
    got, info = dense.spmm_semiring_csr(name, D.m, D.n, D.Ap, D.Aj, D.Ax, X, Y, M, True, False, value_dtype=dtype)
    ref = sr.spmm_semiring(name, D.m, D.n, D.Ap, D.Aj, D.Ax, X, Y, M, True, False, dtype)
    assert srf.same_bits(got, ref[0]) and info["changed"] == ref[1] and info["ms"] >= 0
    assert {s["name"] for s in info["kernels"] if s["launches"] > 0} == {"srmv_short", "srmv_wave", "srmv_long"}
    assert expected_families(D.Ap, sr.selected(M, False, D.m, k)) == {"srmv_short", "srmv_wave", "srmv_long"}


# ---------------------------------------------------------------- traversals against scipy.sparse.csgraph
def symmetric(n, pairs, weights):
    """the undirected graph of these edges as CSR (both directions, no duplicates), weights small positive integers"""
    import scipy.sparse as sp
    r, c = np.asarray(pairs).T
    G = sp.coo_matrix((weights, (r, c)), shape=(n, n)).tocsr()
    G = G.maximum(G.T).tocsr()
    G.sort_indices()
    return G.indptr.astype(np.int32), G.indices.astype(np.int32), G.data.astype(np.float64)


def scipy_answers(n, A, sources):
    import scipy.sparse as sp
    from scipy.sparse import csgraph
    G = sp.csr_matrix((A[2], A[1], A[0]), shape=(n, n)).T.tocsr()   # (csgraph reads G[i, j] as an edge i -> j)
    hops = csgraph.shortest_path(G, method="D", unweighted=True, indices=list(sources)).T
    return np.where(np.isfinite(hops), hops + 1, 0.0), csgraph.bellman_ford(G, indices=list(sources)).T


@functools.lru_cache(maxsize=None)
def graphs():
    rng = np.random.default_rng(7)
    out = {}
    n = 70
    out["path"] = (n, symmetric(n, [(i, i + 1) for i in range(n - 1)], rng.integers(1, 6, n - 1)), [0])
    n = 1101
    out["star"] = (n, symmetric(n, [(0, i) for i in range(1, n)], rng.integers(1, 6, n - 1)), [5])
    n = 60
    out["two components"] = (n, symmetric(n, [(i, i + 1) for i in range(29)] + [(i, i + 1) for i in range(30, 59)],
                                          rng.integers(1, 6, 58)), [3])
    Rp, Rj = gallery.rmat_csr(scale=10)
    rows = np.repeat(np.arange(1 << 10), np.diff(Rp))
    out["rmat"] = (1 << 10, symmetric(1 << 10, np.stack([rows, Rj], axis=1), rng.integers(1, 10, len(Rj))), [0, 17, 1000])
    return out


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("which", ("path", "star", "two components", "rmat"))
def test_traversals_against_scipy(which, dtype):
    n, A, sources = graphs()[which]
    levels, dist = scipy_answers(n, A, sources)
    dA = (up(A[0], np.int32), up(A[1], np.int32), up(A[2], dtype))
    bh = new_handle(dtype)
    try:
        got, steps, ms = graph._bfs(bh, n, dA, sources)
        assert np.array_equal(got.cpu().numpy(), levels.astype(dtype)) and steps == int(levels.max()) and ms > 0
        lens = np.diff(A[0])
        assert families(bh) <= {"srmv_short", "srmv_wave", "srmv_long"} and (lens.max() <= 1024 or which == "star")
        gotd, sweeps, ms = graph._sssp(bh, n, dA, sources, None)
        assert np.array_equal(gotd.cpu().numpy(), dist.astype(dtype)) and 1 <= sweeps <= n
        if which == "path":
            assert steps == 70 and sweeps == 70
        if which == "two components":
            assert (levels == 0).sum() == 30 and np.isinf(dist).sum() == 30
        if len(sources) > 1:                                        # k sources at once: the single-source runs, bit for bit
            for c, s in enumerate(sources):
                assert np.array_equal(bits(graph.bfs_levels_device(bh, n, dA, s).cpu().numpy()[:, 0]), bits(got.cpu().numpy()[:, c]))
                assert np.array_equal(bits(graph.sssp_device(bh, n, dA, [s]).cpu().numpy()[:, 0]), bits(gotd.cpu().numpy()[:, c]))
        # the pattern alone: every edge weighs 1, distances are the levels minus one
        hop = graph.sssp_device(bh, n, (dA[0], dA[1], None), sources).cpu().numpy()
        assert np.array_equal(np.where(np.isfinite(hop), hop + 1, 0.0), levels.astype(dtype))
    finally:
        bh.freePlatform()


def test_a_negative_cycle_raises_after_n_sweeps():
    Ap, Aj, Ax = np.array([0, 1, 2, 3], np.int32), np.array([2, 0, 1], np.int32), np.array([1.0, 1.0, -3.0])
    with pytest.raises(BhsparseError):
        graph.sssp_csr(3, Ap, Aj, Ax, 0)
    dist, info = graph.sssp_csr(3, Ap, Aj, np.abs(Ax), 0, value_dtype=np.float32)
    assert dist[:, 0].tolist() == [0.0, 1.0, 4.0] and info["steps"] == 3 and info["ms"] > 0
    levels, info = graph.bfs_levels_csr(3, Ap, Aj, None, [1, 2])
    assert levels.tolist() == [[3.0, 2.0], [1.0, 3.0], [2.0, 1.0]] and info["steps"] == 3


def test_cpp_demo_runs():
    demo_dir = os.path.join(ROOT, "tests", "srmv")
    subprocess.check_call(["make", "-C", demo_dir, "-s"])
    out = subprocess.run([os.path.join(demo_dir, "srmv_demo")], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "bfs / sssp on a path of 12 vertices, 22 entries: PASS" in out.stdout
