"""CPU tests of "relaxation and fused products" (include/bhsparse_hip.h): bhs_chebyshev_coefficients against the numpy
restatement tests/relaxref.py and against the closed form of the Chebyshev iteration, and what the two device calls
refuse without a device."""
import ctypes as C
import inspect

import numpy as np
import pytest

import relaxref as rr

from benchmark_spgemm_using_csr_amd import _lib, amg, dense

EPS = np.finfo(np.float64).eps
INTERVALS = ((0.3, 1.1), (0.6, 2.2), (2.2 / 30, 2.2))
STEPS = (1, 2, 3, 4, 5, 6)


def ulps(a, b):
    return np.abs(a - b) / np.spacing(np.maximum(np.abs(a), np.abs(b)))


@pytest.mark.parametrize("interval", INTERVALS)
def test_coefficients_against_the_restatement(hiplib, interval):
    """the same few double operations on both sides: 4 ulp"""
    for steps in STEPS:
        got = amg.chebyshev_coefficients(interval[0], interval[1], steps)
        want = rr.chebyshev_coefficients(interval[0], interval[1], steps)
        assert got.shape == (steps, 2) and got.dtype == np.float64
        assert got[0, 0] == 0.0 and np.all(got[:, 1] > 0) and np.all(got[1:, 0] > 0)
        worst = float(ulps(got[:, 1], want[:, 1]).max()), float(ulps(got[1:, 0], want[1:, 0]).max()) if steps > 1 else 0.0
        print("%s steps %d: worst ulp distance c %.2f, a %.2f" % (interval, steps, worst[0], worst[1]))
        assert max(worst) <= 4.0, (interval, steps, worst)
        # a longer list starts with the shorter one
        assert np.array_equal(got, amg.chebyshev_coefficients(interval[0], interval[1], 6)[:steps])


def test_coefficients_refusals(hiplib):
    out = (C.c_double * 12)(*([-7.0] * 12))
    f = hiplib.bhs_chebyshev_coefficients
    inf, nan = float("inf"), float("nan")
    for lmin, lmax, steps in ((0.0, 1.0, 2), (-0.5, 1.0, 2), (1.0, 1.0, 2), (2.0, 1.0, 2), (0.5, inf, 2), (nan, 1.0, 2),
                              (0.5, nan, 2), (-inf, 1.0, 2), (0.3, 1.1, 0), (0.3, 1.1, -1)):
        assert f(lmin, lmax, steps, out) == _lib.BHS_ERR_INVALID_ARG, (lmin, lmax, steps)
        with pytest.raises(ValueError):
            amg.chebyshev_coefficients(lmin, lmax, steps)
    assert f(0.3, 1.1, 2, None) == _lib.BHS_ERR_INVALID_ARG
    assert list(out) == [-7.0] * 12                                 # nothing written by a refused call
    assert f(0.3, 1.1, 2, out) == 0 and list(out)[4:] == [-7.0] * 8


@pytest.mark.parametrize("interval", INTERVALS)
def test_the_iteration_is_the_chebyshev_polynomial(hiplib, interval):
    """x = 1, b = 0 on the scalar lambda: after s steps x = T_s((theta - lambda) / delta) / T_s(sigma), within 64 s eps;
    inside the interval |x| <= 1 / T_s(sigma)"""
    lmin, lmax = interval
    theta, delta = (lmax + lmin) / 2, (lmax - lmin) / 2
    sigma = theta / delta
    lam = np.concatenate([np.linspace(lmin, lmax, 257), [lmin / 2, 1.02 * lmax]])
    inside = np.arange(len(lam)) < 257
    for steps in STEPS:
        coef = amg.chebyshev_coefficients(lmin, lmax, steps)
        x, d = np.ones_like(lam), np.zeros_like(lam)
        for a, c in coef:
            d = c * (0.0 - lam * x) + a * d
            x = x + d
        top = float(rr.chebyshev_value(steps, sigma))
        want = rr.chebyshev_value(steps, (theta - lam) / delta) / top
        err = float(np.abs(x - want).max())
        print("%s steps %d: closed form off by %.2f eps, max |x| inside %.6g (1 / T_s(sigma) = %.6g)"
              % (interval, steps, err / EPS, np.abs(x[inside]).max(), 1 / top))
        assert err <= 64 * steps * EPS, (interval, steps, err / EPS)
        assert np.abs(x[inside]).max() <= 1 / top + 64 * steps * EPS


def test_null_handle_is_refused(hiplib):
    coef = (C.c_double * 2)(0.0, 1.0)
    dots = (C.c_double * 2)(-7.0, -7.0)
    assert hiplib.bhs_csr_relax_device(None, 0, 0, None, None, None, None, 1, coef, None, None, None, 0, None) == _lib.BHS_ERR_INVALID_ARG
    assert hiplib.bhs_csr_spmv_dots_device(None, 0, 0, 0, None, None, None, 1.0, None, 0.0, None, None, None, dots, None) == _lib.BHS_ERR_INVALID_ARG
    assert list(dots) == [-7.0, -7.0]
    f32 = _lib.load(f32=True)
    assert f32.bhs_csr_relax_device(None, 0, 0, None, None, None, None, 1, coef, None, None, None, 0, None) == _lib.BHS_ERR_INVALID_ARG
    assert f32.bhs_csr_spmv_dots_device(None, 0, 0, 0, None, None, None, 1.0, None, 0.0, None, None, None, dots, None) == _lib.BHS_ERR_INVALID_ARG


def test_python_layers():
    sig = lambda f: list(inspect.signature(f).parameters)           # noqa: E731
    assert _lib.BHS_RELAX_ZERO_GUESS == 1 == rr.ZERO_GUESS
    assert sig(amg.relax_raw_device) == ["bh", "n", "nnzA", "d_valA", "d_rowPtrA", "d_colIndA", "d_diag", "steps", "coef", "d_b",
                                         "d_x", "d_d", "flags"]
    assert sig(amg.relax_device) == ["bh", "A", "diag", "b", "x", "coef", "d", "zero_guess"]
    assert sig(amg.jacobi_device) == ["bh", "A", "diag", "b", "x", "omega", "sweeps", "zero_guess"]
    assert sig(amg.spectral_radius_device) == ["bh", "n", "A", "diag", "steps", "seed"]
    assert sig(amg.cheby_setup_device) == ["bh", "levels", "degree", "lanczos_steps", "upper", "lower_ratio"]
    assert inspect.signature(amg.cheby_setup_device).parameters["upper"].default == 1.1
    assert inspect.signature(amg.cheby_setup_device).parameters["lower_ratio"].default == 0.3
    assert sig(dense.csr_spmv_dots_raw_device) == ["bh", "m", "n", "nnzA", "d_valA", "d_rowPtrA", "d_colIndA", "alpha", "d_x", "beta",
                                                   "d_y", "d_z", "d_w", "dots"]
    assert sig(dense.csr_spmv_dots_device) == ["bh", "m", "n", "A", "x", "alpha", "beta", "y", "w"]
    for name in ("bhs_relax.hip.h", "bhs_host_relax.inc.h"):
        assert name in _lib.SOURCES


def test_start_vector_and_lanczos_on_the_host():
    """The estimate spectral_radius_device returns, restated with numpy products on the inputs of the GPU test: at 10 steps
    the start vector of (index, seed 0) reaches 0.95 of the largest eigenvalue of D^-1/2 A D^-1/2 on each, and never
    exceeds it."""
    import chebyref as cr
    for name, (n, Ap, Aj, Ax) in cr.matrices().items():
        lam = cr.lambda_max(n, Ap, Aj, Ax)
        est = cr.lanczos(n, Ap, Aj, Ax, amg._start_vector(n, 0), 10)
        print("%s: Lanczos(10) %.6f of lambda_max %.6f = %.4f" % (name, est, lam, est / lam))
        assert 0.95 * lam <= est <= lam * (1 + 64 * EPS), (name, est, lam)
    v = amg._start_vector(1000, 0)
    assert v.dtype == np.float64 and v.min() >= -1.0 and v.max() < 1.0 and abs(v.mean()) < 0.1 and len(np.unique(v)) == 1000
    assert not np.array_equal(v, amg._start_vector(1000, 1)) and np.array_equal(v[:10], amg._start_vector(10, 0))
