"""The smoothed-aggregation setup and cycle of benchmark_spgemm_using_csr_amd/amg.py on the GPU, both builds.

Reference: tests/aggref.py -- the aggregation restated in numpy, the hierarchy in scipy.  A matrix is compared pattern for
pattern (columns ascending on both sides) and value for value; "relative" is relative to the largest magnitude of the
reference matrix, the measure the project's parity tests use for chained products."""
import functools

import numpy as np
import pytest
import scipy.sparse as sp
import torch

import aggref as ar

from benchmark_spgemm_using_csr_amd import amg, gallery
from benchmark_spgemm_using_csr_amd.facade import BHSPARSE_HIP, NUM_PLATFORMS, bhsparse

pytestmark = pytest.mark.gpu

DTYPES = (np.float64, np.float32)


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


def host_csr(M, shape):
    p, j, x = (t.cpu().numpy() if hasattr(t, "cpu") else np.asarray(t) for t in M)
    X = sp.csr_matrix((x.astype(np.float64), j, p), shape=shape)
    Y = X.copy()
    Y.sort_indices()
    assert np.array_equal(Y.indices, X.indices), "columns ascending in every row"
    return X


def same_matrix(got, want, tol, what):
    want = sp.csr_matrix(want)
    want.sort_indices()
    assert got.shape == want.shape, what
    assert np.array_equal(got.indptr, want.indptr) and np.array_equal(got.indices, want.indices), (what, "pattern")
    scale = np.abs(want.data).max() if want.nnz else 1.0
    err = np.abs(got.data - want.data).max() / scale if want.nnz else 0.0
    print("%s: relative error %.3g (bound %.1g)" % (what, err, tol))
    assert err <= tol, (what, err)


@functools.lru_cache(maxsize=None)
def problem(name):
    args = {"poisson5pt_33": ("poisson5pt", 33, 33), "poisson27pt_9": ("poisson27pt", 9, 9, 9)}[name]
    return ar.poisson(*args)


@functools.lru_cache(maxsize=None)
def reference_hierarchy(name, seed=0):
    n, Ap, Aj, Ax = problem(name)
    return ar.sa_setup(sp.csr_matrix((Ax, Aj, Ap), shape=(n, n)), seed=seed)


# ---------------------------------------------------------------- the pieces
def test_tentative(hd):
    bh, dtype = hd
    n, Ap, Aj, _ = problem("poisson5pt_33")
    agg, nagg, _, _ = ar.aggregate(n, Ap, Aj, 0)
    rng = np.random.default_rng(2)
    for cand in (None, rng.random(n) + 0.5):
        cand_r = None if cand is None else cand.astype(dtype).astype(np.float64)
        T, cc = amg.tentative_device(bh, n, up(agg, np.int32), nagg, None if cand is None else up(cand, dtype))
        wantT, wantcc = ar.tentative(n, agg.astype(np.int64), nagg, cand_r)
        assert np.array_equal(T[0].cpu().numpy(), np.arange(n + 1)) and np.array_equal(T[1].cpu().numpy(), agg)
        tol = 1e-14 if dtype == np.float64 else 4 * np.finfo(np.float32).eps     # (a sum of squares, a root, a quotient, a rounding each)
        assert np.allclose(T[2].cpu().numpy().astype(np.float64), wantT.data, rtol=tol, atol=0)
        assert np.allclose(cc.cpu().numpy().astype(np.float64), wantcc, rtol=tol, atol=0)
        T2, cc2 = amg.tentative_device(bh, n, up(agg, np.int32), nagg, None if cand is None else up(cand, dtype))
        assert torch.equal(T2[2], T[2]) and torch.equal(cc2, cc)       # bit for bit
        colnorm = np.sqrt(np.bincount(agg, weights=T[2].cpu().numpy().astype(np.float64) ** 2, minlength=nagg))
        assert np.allclose(colnorm, 1.0, rtol=0, atol=1e-13 if dtype == np.float64 else 1e-6)


@pytest.mark.parametrize("theta", (0.0, 0.25))
def test_strength(hd, theta):
    bh, dtype = hd
    n, Ap, Aj, _ = problem("poisson5pt_33")
    Ax = gallery.fill_values(len(Aj))
    Sp, Sj = amg.strength_device(bh, n, (up(Ap, np.int32), up(Aj, np.int32), up(Ax, dtype)), theta)
    want = ar.strength(sp.csr_matrix((Ax, Aj, Ap), shape=(n, n)), theta)
    assert np.array_equal(Sp.cpu().numpy(), want.indptr) and np.array_equal(Sj.cpu().numpy(), want.indices)
    if theta == 0.0:
        assert want.nnz == len(Aj)                                   # pattern(A) U pattern(A^T) of a symmetric pattern
    else:
        assert n < want.nnz < len(Aj)
    assert bh.strength_ms >= 0.0


# ---------------------------------------------------------------- the setup
@pytest.mark.parametrize("name", ("poisson5pt_33", "poisson27pt_9"))
@pytest.mark.parametrize("dtype", DTYPES, ids=("f64", "f32"))
def test_sa_setup_csr(name, dtype):
    """Level sizes are the reference's; every P_l and A_l matches the scipy hierarchy built from the same aggregates: the
    pattern exactly, the values to 1e-10 relative in double and 1e-4 in float."""
    n, Ap, Aj, Ax = problem(name)
    levels, info = amg.sa_setup_csr(n, Ap, Aj, Ax, value_dtype=dtype)
    ref_levels, ref_sizes = reference_hierarchy(name)
    assert [rec["n"] for rec in info] == [n] + ref_sizes
    assert [rec["nagg"] for rec in info[:-1]] == ref_sizes and len(levels) == len(ref_levels) >= 2
    tol = 1e-10 if dtype == np.float64 else 1e-4
    for lvl, ((A, P, R), (wA, wP, wR)) in enumerate(zip(levels, ref_levels)):
        rows = wA.shape[0]
        same_matrix(host_csr(A, (rows, rows)), wA, tol, "%s %s A_%d" % (name, np.dtype(dtype).name, lvl))
        assert info[lvl]["nnz"] == wA.nnz
        if wP is None:
            assert P is None and R is None
            continue
        same_matrix(host_csr(P, wP.shape), wP, tol, "%s %s P_%d" % (name, np.dtype(dtype).name, lvl))
        same_matrix(host_csr(R, wR.shape), wR, tol, "%s %s R_%d" % (name, np.dtype(dtype).name, lvl))
        rec = info[lvl]
        assert rec["rounds"] >= 1 and all(rec[k] >= 0.0 for k in ("strength_ms", "aggregate_ms", "prolongator_ms", "galerkin_ms"))


def test_sa_setup_device_with_a_handle_factory():
    n, Ap, Aj, Ax = problem("poisson27pt_9")
    A = (up(Ap, np.int32), up(Aj, np.int32), up(Ax, np.float64))
    made = []

    def factory():
        made.append(new_handle())
        return made[-1]
    levels, info = amg.sa_setup_device(factory, n, A, seed=1)
    assert len(made) == 2 and all(h._h is None for h in made)        # destroyed by the setup
    assert [rec["n"] for rec in info] == [n] + reference_hierarchy("poisson27pt_9", 1)[1]
    assert levels[0][0][0].is_cuda and levels[-1][1] is None


# ---------------------------------------------------------------- the cycle
def test_solve_device():
    """1e-8 relative residual on poisson5pt 33^2 in double, within the cycles the CPU restatement needs plus 2"""
    n, Ap, Aj, Ax = problem("poisson5pt_33")
    b = np.random.default_rng(0).standard_normal(n)
    ref_levels, _ = reference_hierarchy("poisson5pt_33")
    _, ref_cycles, ref_res = ar.solve(ref_levels, b, 1e-8, 100)
    assert ref_res[-1] <= 1e-8 * ref_res[0]
    A = (up(Ap, np.int32), up(Aj, np.int32), up(Ax, np.float64))
    h1, h2 = new_handle(), new_handle()
    try:
        levels, _ = amg.sa_setup_device((h1, h2), n, A)
        x, cycles, res = amg.solve_device(h1, levels, up(b, np.float64), 1e-8, 100)
    finally:
        h1.freePlatform()
        h2.freePlatform()
    print("solve: %d cycles on the device, %d in the restatement; residuals %.3g -> %.3g" % (cycles, ref_cycles, res[0], res[-1]))
    assert res[-1] <= 1e-8 * res[0] and cycles <= ref_cycles + 2
    Amat = sp.csr_matrix((Ax, Aj, Ap), shape=(n, n))
    assert np.linalg.norm(b - Amat @ x.cpu().numpy()) <= 1.01e-8 * np.linalg.norm(b)
