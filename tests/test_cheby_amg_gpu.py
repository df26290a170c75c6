"""The Chebyshev smoother in the multigrid cycle on the GPU: the Lanczos estimate of rho(D^-1 A) against the dense
eigenvalues, the symmetry of the cycle against the Jacobi cycle's, PCG with it, and the omega estimate of the setup.
Inputs and the host restatement of the estimate: tests/chebyref.py."""
import numpy as np
import pytest
import scipy.sparse as sp
import torch

import aggref as ar
import chebyref as cr
from test_spmv_gpu import bits, new_handle, tdt, up

from benchmark_spgemm_using_csr_amd import amg

pytestmark = pytest.mark.gpu

DTYPES = (np.float64, np.float32)


def device_matrix(M, dtype):
    n, Ap, Aj, Ax = M
    return n, (up(Ap, np.int32), up(Aj, np.int32), up(Ax, dtype))


@pytest.mark.parametrize("dtype", DTYPES, ids=("f64", "f32"))
def test_spectral_radius(dtype):
    """A Ritz value never exceeds lambda_max (64 eps of the build for the rounding of the products); 10 steps from the
    start vector of seed 0 reach 0.95 of it (the host restatement reaches 0.984 .. 0.997 on these inputs:
    tests/test_relax_abi.py)"""
    eps = float(np.finfo(dtype).eps)
    bh = new_handle(dtype)
    try:
        for name, M in cr.matrices().items():
            n, A = device_matrix(M, dtype)
            lam = cr.lambda_max(*M)
            est = amg.spectral_radius_device(bh, n, A)
            host = cr.lanczos(*M, amg._start_vector(n, 0), 10)
            print("%s %s: estimate %.6f, host restatement %.6f, lambda_max %.6f (%.4f)" % (name, np.dtype(dtype).name, est, host, lam, est / lam))
            assert est <= lam * (1 + 64 * eps), (name, est, lam)
            assert est >= 0.95 * lam, (name, est, lam)
            assert est == amg.spectral_radius_device(bh, n, A, steps=10, seed=0)        # seeded: the same bits
            assert bh.lanczos_ms >= 0.0
        n, A = device_matrix(cr.matrices()["poisson5pt 16^2"], dtype)
        with pytest.raises(ValueError):
            amg.spectral_radius_device(bh, n, A, diag=torch.zeros(n, dtype=tdt(dtype)).cuda())
        with pytest.raises(ValueError):
            amg.spectral_radius_device(bh, n, A, diag=-torch.ones(n, dtype=tdt(dtype)).cuda())
    finally:
        bh.freePlatform()


def hierarchy(name, dtype, h1, h2, **kw):
    M = ar.poisson(*{"poisson5pt_32": ("poisson5pt", 32, 32), "poisson27pt_8": ("poisson27pt", 8, 8, 8)}[name])
    n, A = device_matrix(M, dtype)
    levels, info = amg.sa_setup_device((h1, h2), n, A, min_coarse=40, **kw)
    return M, n, A, levels, info


def test_cheby_setup_and_symmetric_cycle():
    """|<u, M v> - <v, M u>| / (||u|| ||M v||) of the V(1,1) cycle from zero: rounding only, so the Jacobi cycle of the same
    hierarchy is the yardstick -- ten times its figure is allowed"""
    h1, h2 = new_handle(), new_handle()
    try:
        M, n, A, levels, _ = hierarchy("poisson5pt_32", np.float64, h1, h2)
        assert len(levels) >= 2
        smoothers = amg.cheby_setup_device(h1, levels)
        assert len(smoothers) == len(levels) - 1
        for lvl, ((d, coef), (Al, _, _)) in enumerate(zip(smoothers, levels)):
            assert d.is_cuda and coef.shape == (2, 2) and coef[0, 0] == 0.0
            if lvl:
                continue                                            # (the estimate's lower bound is checked on the finest level's matrix only)
            theta = 1 / coef[0, 1]                                  # (lmax + lmin) / 2 with lmin = 0.3 lmax
            lmax = theta / 0.65
            nl = int(Al[0].numel()) - 1
            Ah = sp.csr_matrix((Al[2].cpu().numpy(), Al[1].cpu().numpy(), Al[0].cpu().numpy()), shape=(nl, nl))
            lam = cr.lambda_max(nl, Ah.indptr, Ah.indices, Ah.data)
            assert 0.95 * 1.1 * lam <= lmax * (1 + 1e-12) and lmax <= 1.1 * lam * (1 + 1e-12), (lmax, lam)
        assert amg.cheby_setup_device(h1, levels, degree=3)[0][1].shape == (3, 2)
        rng = np.random.default_rng(3)
        u, v = up(rng.standard_normal(n), np.float64), up(rng.standard_normal(n), np.float64)
        zero = torch.zeros_like(u)
        asym = {}
        for smoother, sm in (("jacobi", None), ("chebyshev", smoothers)):
            Mu = amg.vcycle_device(h1, levels, u, zero, smoother=smoother, smoothers=sm)
            Mv = amg.vcycle_device(h1, levels, v, zero, smoother=smoother, smoothers=sm)
            asym[smoother] = abs(float(torch.dot(u, Mv)) - float(torch.dot(v, Mu))) / float(torch.linalg.norm(u) * torch.linalg.norm(Mv))
        assert bool((zero == 0).all())                              # the guess is the caller's: not written
        # with the setup made inside: the same cycle
        Mu2 = amg.vcycle_device(h1, levels, u, zero, smoother="chebyshev")
        assert torch.equal(Mu2, amg.vcycle_device(h1, levels, u, zero, smoother="chebyshev", smoothers=smoothers))
    finally:
        h1.freePlatform()
        h2.freePlatform()
    assert asym["chebyshev"] <= 10 * asym["jacobi"], "asymmetry: chebyshev %.3g, jacobi %.3g" % (asym["chebyshev"], asym["jacobi"])
    print("asymmetry of the cycle: chebyshev %.3g, jacobi %.3g" % (asym["chebyshev"], asym["jacobi"]))


@pytest.mark.parametrize("dtype", DTYPES, ids=("f64", "f32"))
@pytest.mark.parametrize("name", ("poisson5pt_32", "poisson27pt_8"))
def test_pcg_converges(name, dtype):
    """to 1e-8 in double as tests/test_gs_gpu.py asks of the other smoothers (true residual within 1.01e-8 ||b||); in float to
    1e-4, the true residual within 2e-4 ||b||: the recurrence's residual drifts from it by eps ||A|| ||x||, and
    ||x|| / ||b|| reaches 1 / lambda_min, about 100 here -- 6e-8 * 8 * 100 = 5e-5, twice that allowed"""
    tol, true_tol = (1e-8, 1.01e-8) if dtype == np.float64 else (1e-4, 2e-4)
    h1, h2 = new_handle(dtype), new_handle(dtype)
    try:
        M, n, A, levels, info = hierarchy(name, dtype, h1, h2)
        b = np.random.default_rng(0).standard_normal(n).astype(dtype)
        x, its, res = amg.pcg_device(h1, levels, up(b, dtype), tol, 100, smoother="chebyshev")
        xj, its_j, _ = amg.pcg_device(h1, levels, up(b, dtype), tol, 100, smoother="jacobi")
    finally:
        h1.freePlatform()
        h2.freePlatform()
    Amat = sp.csr_matrix((M[3], M[2], M[1]), shape=(n, n))
    true = np.linalg.norm(b.astype(np.float64) - Amat @ x.cpu().numpy().astype(np.float64)) / np.linalg.norm(b.astype(np.float64))
    print("%s %s: levels %s, chebyshev %d iterations (jacobi %d), true residual %.3g" % (name, np.dtype(dtype).name, [r["n"] for r in info], its, its_j, true))
    assert its < 100 and len(res) == its + 1 and res[-1] <= tol * res[0], (its, res[-1] / res[0])
    assert true <= true_tol, true


def test_omega_estimate():
    h1, h2 = new_handle(), new_handle()
    try:
        M, n, A, levels, info = hierarchy("poisson5pt_32", np.float64, h1, h2, omega="estimate")
        assert len(levels) >= 2 and all("omega" in r and r["lanczos_ms"] >= 0 for r in info[:-1])
        lam = cr.lambda_max(*M)
        assert 4 / (3 * lam) * (1 - 1e-12) <= info[0]["omega"] <= 4 / (3 * 0.95 * lam)
        b = up(np.random.default_rng(0).standard_normal(n), np.float64)
        x, its, res = amg.pcg_device(h1, levels, b, 1e-8, 100, smoother="chebyshev")
        assert its < 100 and res[-1] <= 1e-8 * res[0]
        # a number for omega is the setup it was: the default call's levels, bit for bit
        _, _, _, dflt, _ = hierarchy("poisson5pt_32", np.float64, h1, h2)
        _, _, _, given, _ = hierarchy("poisson5pt_32", np.float64, h1, h2, omega=2.0 / 3.0)
        assert len(dflt) == len(given)
        for a, g in zip(dflt, given):
            for Ma, Mg in zip(a, g):
                assert (Ma is None) == (Mg is None)
                if Ma is not None:
                    assert torch.equal(Ma[0], Mg[0]) and torch.equal(Ma[1], Mg[1])
                    assert np.array_equal(bits(Ma[2].cpu().numpy()), bits(Mg[2].cpu().numpy()))
        with pytest.raises(ValueError):
            hierarchy("poisson5pt_32", np.float64, h1, h2, omega="guess")
    finally:
        h1.freePlatform()
        h2.freePlatform()
