"""The workspaces of the operations beside the multiply, reused from call to call, and their scan's tile boundary.

Every family -- the add, the selection, the transpose, the extraction, the reductions, the masked multiply -- keeps one
workspace on the handle (csrc/bhs_host_side.inc.h: control block, queues, counts, tile words, epoch) that only grows, and
the four with a row pointer to make share one scan over 8192-count tiles.  One long-lived handle per build is taken through
SIZES of the scanned dimension (m of the add and the selection, n of the transpose, mI of the extraction): it grows, empties,
regrows across one tile, lands exactly on a tile, covers several tiles and stops just under one.  At every size all the
families run one after another before the next size, so that a workspace crossed with another's, sized for the last call,
or a tile word left from it shows as a wrong result.  Integer values: every result is compared exactly, against the numpy
references of tests/ and, for the add and the masked multiply, the oracle.

Between two sizes a refused call on device arrays (a column of X out of range, met by the selection's count kernel) and one on
host arrays (an invalid mask, met behind the masked multiply's staging copies) must return BHS_ERR_INVALID_ARG, write
nothing caller-owned and leave the handle to give the exact result at the next call."""
import numpy as np
import pytest
import torch

import extractref
import reduceref as rr
import selectref as sr
import test_add_gpu as addt
import transposeref
from valuecheck import on_pattern

from benchmark_spgemm_using_csr_amd import _lib, gallery
from benchmark_spgemm_using_csr_amd import facade as bhmod

pytestmark = pytest.mark.gpu

BUILDS = {"f64": np.float64, "f32": np.float32}
SCAN_TILE = 8192                                   # kScan1Tile (csrc/bhs_kernels.hip.h)
SIZES = (SCAN_TILE + 1, 0, 1, SCAN_TILE, 3 * SCAN_TILE + 5, SCAN_TILE - 1)
REFUSE_AFTER = SCAN_TILE                           # the refused calls come between this size and the next
N_COLS = 1500                                      # columns of the add's / selection's / reductions' X, rows of the transpose's
EX_M, EX_N = 3000, 2000                            # the matrix rows and columns are extracted from
MK, MN = 300, 400                                  # the masked multiply: A is size x MK, B is MK x MN
SENT_J, SENT_X = -7, -7.0
SPEC = sr.Spec(flags=sr.TOPK | sr.DROP_DIAG, top_k=2)

_CACHE = {}                                        # inputs and references, made once and shared by both builds


def _cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def ragged(seed, m, n):
    """m x n CSR, 0-5 entries a row at random columns (ascending, no duplicates), values 1 .. 9."""
    rng = np.random.default_rng(seed)
    rows = np.repeat(np.arange(m, dtype=np.int64), rng.integers(0, 6, m))
    Xp, Xj = gallery._csr_from_pairs(m, n, rows, rng.integers(0, n, len(rows)))
    return Xp, Xj, rng.integers(1, 10, len(Xj)).astype(np.float64)


def matrix(which, size):
    return _cached((which, size), lambda: ragged({"X": 1, "Y": 2, "A": 3}[which] * 100003 + size, size,
                                                 MK if which == "A" else N_COLS))


def up(a, dt):
    """A device copy; an empty array as an empty slice of a one-element tensor (its address is not NULL)."""
    a = np.ascontiguousarray(a, dt)
    t = torch.empty(max(a.size, 1), dtype=torch.from_numpy(np.zeros(1, dt)).dtype).cuda()
    t[:a.size].copy_(torch.from_numpy(a.copy()))
    return t[:a.size]


def dev(X, vd):
    return up(X[0], np.int32), up(X[1], np.int32), up(X[2], vd)


def same(got, want, what):
    got = got.cpu().numpy() if hasattr(got, "cpu") else np.asarray(got)
    want = np.asarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
    assert np.array_equal(got, want), what


def select_struct():
    c = _lib.Select()
    c.flags, c.top_k, c.band_lo, c.band_hi, c.abs_tol, c.rel_tol = (SPEC.flags, SPEC.top_k, SPEC.band_lo, SPEC.band_hi,
                                                                   SPEC.abs_tol, SPEC.rel_tol)
    return c


# ---------------------------------------------------------------- the families, one call each
def run_add(oracle, bh, size, what):
    X, Y = matrix("X", size), matrix("Y", size)

    def reference():                                                # 2 X - Y = [2 I, -I] [X; Y] by the oracle
        eye = (np.arange(size + 1, dtype=np.int32), np.arange(size, dtype=np.int32), np.ones(size))
        return addt.reference(oracle, size, size, N_COLS, eye, X, Y, 2, -1)
    want = _cached(("add", size), reference)
    Zp, Zj, Zx, _ = bh.csr_add_device(size, N_COLS, 2, dev(X, bh._vdt), -1, dev(Y, bh._vdt))
    same(Zp, want[0].astype(np.int32), what)
    same(Zj, want[1], what)
    same(Zx, want[2].astype(bh._vdt), what)


def run_select(oracle, bh, size, what):
    X = matrix("X", size)
    want = _cached(("select", size), lambda: sr.select(size, N_COLS, X[0], X[1], X[2], SPEC))
    Zp, Zj, Zx = bh.csr_select_device(size, N_COLS, dev(X, bh._vdt), select_struct())
    same(Zp, want[0], what)
    same(Zj, want[1], what)
    same(Zx, want[2].astype(bh._vdt), what)


def run_transpose(oracle, bh, size, what):
    X = matrix("X", size)
    W = _cached(("W", size), lambda: transposeref.transpose(size, N_COLS, X[0], X[1], X[2])[:3])   # N_COLS x size: n = size is scanned
    want = _cached(("transpose", size), lambda: transposeref.transpose(N_COLS, size, W[0], W[1], W[2]))
    Tp, Tj, Tx, pm = bh.csr_transpose_device(N_COLS, size, dev(W, bh._vdt), perm=True)
    same(Tp, want[0], what)
    same(Tj, want[1], what)
    same(Tx, want[2].astype(bh._vdt), what)
    same(pm, want[3], what)


def run_extract(oracle, bh, size, what):
    X = _cached("EX", lambda: ragged(7, EX_M, EX_N))
    rng = np.random.default_rng(900 + size)
    rows = rng.integers(0, EX_M, size).astype(np.int32)             # mI = size rows of Z, rows of X taken more than once
    cols = rng.permutation(EX_N)[:2 * EX_N // 3].astype(np.int32)
    want = _cached(("extract", size), lambda: extractref.extract(EX_M, EX_N, X[0], X[1], X[2], rows, cols))
    Zp, Zj, Zx, pm = bh.csr_extract_device(EX_M, EX_N, dev(X, bh._vdt), up(rows, np.int32), up(cols, np.int32), perm=True)
    same(Zp, want[0], what)
    same(Zj, want[1], what)
    same(Zx, want[2].astype(bh._vdt), what)
    same(pm, want[3], what)


def run_reduce(oracle, bh, size, what):
    X = matrix("X", size)
    for axis in (rr.ROWS, rr.ALL):
        want = _cached(("reduce", size, axis), lambda: rr.reduce(size, N_COLS, X[0], X[1], X[2], axis, rr.PLUS)[0])
        same(bh.csr_reduce_device(size, N_COLS, dev(X, bh._vdt), axis, rr.PLUS), want.astype(bh._vdt), (what, axis))


def masked_case(oracle, size):
    """(A, B, the mask's row pointer and columns, the oracle's A·B on the mask)"""
    def make():
        A, B = matrix("A", size), _cached("B", lambda: ragged(11, MK, MN))
        ref = oracle.spgemm(size, MK, MN, *A, *B)
        if size == 0:
            Mp, Mj = np.zeros(1, np.int32), np.zeros(0, np.int32)
        else:
            Mp, Mj, _ = addt.pattern_with_extras(np.random.default_rng(5000 + size), size, MN, (ref[0], ref[1]), 0.5, 1)
        return A, B, Mp, Mj, on_pattern(ref, MN, Mp, Mj)
    return _cached(("masked", size), make)


def bind(bh, size, A, B):
    arrs = [np.ascontiguousarray(x, t) for x, t in ((A[2], bh._vdt), (A[0], np.int32), (A[1], np.int32),
                                                    (B[2], bh._vdt), (B[0], np.int32), (B[1], np.int32))]
    assert bh.initData(size, MK, MN, len(arrs[2]), arrs[0], arrs[1], arrs[2], len(arrs[5]), arrs[3], arrs[4], arrs[5],
                       np.zeros(size + 1, np.int32)) == 0


def run_masked(oracle, bh, size, what):
    A, B, Mp, Mj, want = masked_case(oracle, size)
    bind(bh, size, A, B)
    valC = torch.full((len(Mj) + 8,), SENT_X, dtype=torch.from_numpy(np.zeros(1, bh._vdt)).dtype).cuda()
    assert bh.spgemm_masked_device(up(Mp, np.int32), up(Mj, np.int32), len(Mj), valC) == 0, what
    got = valC.cpu().numpy()
    assert np.all(got[len(Mj):] == SENT_X), what
    same(got[:len(Mj)], want.astype(bh._vdt), what)


FAMILIES = (run_add, run_select, run_transpose, run_extract, run_reduce, run_masked)


# ---------------------------------------------------------------- the refused calls
def refused_on_device(oracle, bh, size, what):
    """A column of X out of range: the selection's count kernel refuses, rowPtrZ stays as it was, the next call is exact."""
    X = matrix("X", size)
    Xj = X[1].copy()
    Xj[len(Xj) // 2] = N_COLS
    Zp = torch.full((size + 1,), SENT_J, dtype=torch.int32).cuda()
    torch.cuda.synchronize()
    err, _ = bh.csr_select_symbolic_device(size, N_COLS, len(Xj), up(X[2], bh._vdt), up(X[0], np.int32), up(Xj, np.int32),
                                           select_struct(), Zp)
    assert err == _lib.BHS_ERR_INVALID_ARG, what
    torch.cuda.synchronize()
    assert bool((Zp == SENT_J).all()), (what, "rowPtrZ was written by a refused call")
    run_select(oracle, bh, size, what + ", the call after it")


def refused_on_host(oracle, bh, size, what):
    """A mask with a column out of range through the host-array entry: refused behind the staging copies, valC stays as it
    was, the next call through the same entry is exact."""
    A, B, Mp, Mj, want = masked_case(oracle, size)                  # (the data set of this size is still bound)
    bad = Mj.copy()
    bad[len(bad) // 2] = MN
    valC = np.full(len(Mj), SENT_X, bh._vdt)
    with pytest.raises(bhmod.BhsparseError) as e:
        bh.spgemm_masked(Mp, bad, valC)
    assert e.value.code == _lib.BHS_ERR_INVALID_ARG, what
    assert np.all(valC == SENT_X), (what, "valC was written by a refused call")
    same(bh.spgemm_masked(Mp, Mj, valC), want.astype(bh._vdt), what + ", the call after it")


@pytest.mark.parametrize("build", sorted(BUILDS))
def test_one_handle_through_the_scan_sizes(oracle, build):
    plats = [False] * bhmod.NUM_PLATFORMS
    plats[bhmod.BHSPARSE_HIP] = True
    bh = bhmod.bhsparse(value_dtype=BUILDS[build])
    assert bh.initPlatform(plats) == 0
    try:
        for size in SIZES:
            for family in FAMILIES:
                family(oracle, bh, size, "%s at %d (%s)" % (family.__name__, size, build))
            if size == REFUSE_AFTER:
                refused_on_device(oracle, bh, size, "refused selection at %d (%s)" % (size, build))
                refused_on_host(oracle, bh, size, "refused masked multiply at %d (%s)" % (size, build))
        assert bh.free_mem() == 0
    finally:
        bh.freePlatform()
