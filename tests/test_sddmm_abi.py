"""CPU tests of the "sampled dense-dense product" (include/bhsparse_hip.h): what bhs_csr_sddmm_device refuses without a
device, the Python layers' signatures, the numpy restatement tests/sddmmref.py against an independent sum and against
itself wherever an entry is placed, and the affinity strength of connection (amg.affinity_strength_device, restated with
numpy products) on the anisotropic operator and on its symmetric diagonal scaling."""
import inspect

import numpy as np
import pytest

import aggref
import matchref
import sddmmref as sd
from helpers import wide_values
from valuecheck import bound

from benchmark_spgemm_using_csr_amd import _lib, amg, dense


def test_null_handle_is_refused(hiplib):
    args = (None, 0, 0, 0, None, None, None, 1, 1.0, None, 1, None, 1, 0.0, None, 0, None)
    assert hiplib.bhs_csr_sddmm_device(*args) == _lib.BHS_ERR_INVALID_ARG
    assert _lib.load(f32=True).bhs_csr_sddmm_device(*args) == _lib.BHS_ERR_INVALID_ARG


def test_python_layers():
    sig = lambda f: list(inspect.signature(f).parameters)           # noqa: E731
    default = lambda f, name: inspect.signature(f).parameters[name].default   # noqa: E731
    assert _lib.BHS_SDDMM_TIMES_M == 1 == sd.TIMES_M
    assert "bhs_csr_sddmm_device" in _lib.SYMBOLS and len(_lib.SYMBOLS["bhs_csr_sddmm_device"][1]) == 17
    assert sig(dense.csr_sddmm_raw_device) == ["bh", "m", "n", "nnzM", "d_valM", "d_rowPtrM", "d_colIndM", "k", "alpha", "d_X", "ldX",
                                               "d_Y", "ldY", "beta", "d_valZ", "flags"]
    assert sig(dense.csr_sddmm_device) == ["bh", "m", "n", "M", "X", "Y", "alpha", "beta", "Z", "times_m"]
    assert [default(dense.csr_sddmm_device, p) for p in ("alpha", "beta", "Z", "times_m")] == [1.0, 0.0, None, False]
    assert sig(dense.sddmm_csr) == ["m", "n", "Mp", "Mj", "Mx", "X", "Y", "alpha", "beta", "Z", "times_m", "value_dtype", "device"]
    assert [default(dense.sddmm_csr, p) for p in ("alpha", "beta", "Z", "times_m", "value_dtype", "device")] == [1.0, 0.0, None, False,
                                                                                                               np.float64, 0]
    assert sig(amg.affinity_strength_device) == ["bh", "n", "A", "theta", "vectors", "sweeps", "omega", "seed"]
    assert [default(amg.affinity_strength_device, p) for p in ("theta", "vectors", "sweeps", "omega", "seed")] == [0.5, 16, 8, 2.0 / 3.0, 0]
    for name in ("bhs_sddmm.hip.h", "bhs_host_sddmm.inc.h"):
        assert name in _lib.SOURCES


def test_the_refusal_words():
    Mp, Mj = np.array([0, 2, 3]), np.array([1, 0, 2])
    assert sd.invalid(2, 3, Mp, Mj, 4) is None and sd.invalid(2, 3, Mp, Mj, 4, flags=1) is None
    assert sd.invalid(0, 0, [0], [], 1) is None and sd.invalid(2, 3, [0, 0, 0], None, 1, has_x=False, has_y=False, has_z=False) is None
    got = [sd.invalid(-1, 3, Mp, Mj), sd.invalid(2, 3, Mp, Mj, 0), sd.invalid(2, 3, Mp, Mj, 4, ldX=3), sd.invalid(2, 3, Mp, Mj, 4, ldY=3),
           sd.invalid(2, 3, None, Mj), sd.invalid(2, 3, Mp, None, nnz=3), sd.invalid(2, 3, Mp, Mj, has_x=False),
           sd.invalid(2, 3, Mp, Mj, has_y=False), sd.invalid(2, 3, Mp, Mj, has_z=False), sd.invalid(2, 3, Mp, Mj, flags=1, has_valm=False),
           sd.invalid(2, 3, Mp, Mj, flags=2), sd.invalid(2, 3, Mp, Mj, overlap=True)]
    assert tuple(got) == sd.HOST_REFUSALS
    got = [sd.invalid(2, 3, [1, 2, 3], Mj), sd.invalid(2, 3, [0, 2, 2], Mj), sd.invalid(3, 3, [0, 2, 1, 3], Mj),
           sd.invalid(2, 2, Mp, Mj)]
    assert tuple(got) == sd.DEVICE_REFUSALS


@pytest.mark.parametrize("k", (1, 2, 3, 4, 5, 16, 17, 63, 64, 65, 100, 129))
def test_the_restatement_against_einsum(k):
    """any order of an entry's k products and k - 1 additions, the factor m and the two operations of alpha and beta:
    valuecheck's bound with K = k + 2 on S = |alpha| |m| (|x| . |y|) + |beta| |z|"""
    rng = np.random.default_rng(k)
    m, n = 37, 41
    lens = rng.integers(0, 9, m)
    Mp = np.concatenate([[0], np.cumsum(lens)])
    Mj = rng.integers(0, n, Mp[-1])
    X, Y = wide_values(m * k, rng).reshape(m, k), wide_values(n * k, rng).reshape(n, k)
    Mx, Z = wide_values(len(Mj), rng), wide_values(len(Mj), rng)
    rows = np.repeat(np.arange(m), lens)
    for alpha, beta, times_m in ((1.0, 0.0, False), (-0.5, 1.0, True), (0.0, -0.5, True)):
        got = sd.sddmm(m, n, Mp, Mj, Mx, X, Y, alpha, beta, Z, times_m)
        f = Mx if times_m else 1.0
        ref = alpha * (np.einsum("ij,ij->i", X[rows], Y[Mj]) * f) + beta * Z
        S = abs(alpha) * np.abs(f) * np.einsum("ij,ij->i", np.abs(X[rows]), np.abs(Y[Mj])) + abs(beta) * np.abs(Z)
        lim = bound("f64", ref, S, np.full(len(Mj), k + 2))
        worst = float((np.abs(got - ref) / np.where(lim > 0, lim, 1.0)).max())
        print("k = %d alpha %g beta %g times_m %d: worst error / bound %.3f" % (k, alpha, beta, times_m, worst))
        assert np.all(np.abs(got - ref) <= lim), (k, alpha, beta, times_m, worst)
    # float inputs: the products are exact, one rounding at the end
    got = sd.sddmm(m, n, Mp, Mj, None, X, Y, dtype=np.float32)
    x32, y32 = X.astype(np.float32).astype(np.float64), Y.astype(np.float32).astype(np.float64)
    assert got.dtype == np.float32 and np.allclose(got, np.einsum("ij,ij->i", x32[rows], y32[Mj]), rtol=1e-6, atol=0)


@pytest.mark.parametrize("k", (3, 16, 100))
def test_one_pair_gives_the_same_bits_wherever_it_stands(k):
    rng = np.random.default_rng(50 + k)
    n = 64
    lens = (5, 40, 1100, 1)
    m = len(lens)
    Mp = np.concatenate([[0], np.cumsum(lens)])
    Mj = rng.integers(0, n, Mp[-1])
    where = [int(Mp[i] + rng.integers(0, L)) for i, L in enumerate(lens)]
    Mj[where] = 9
    X, Y = wide_values(m * k, rng).reshape(m, k), wide_values(n * k, rng).reshape(n, k)
    X[:] = X[0]
    Mx = wide_values(len(Mj), rng)
    Mx[where] = Mx[where[0]]
    for dtype in (np.float64, np.float32):
        got = sd.sddmm(m, n, Mp, Mj, Mx, X, Y, -0.5, 1.0, Mx, True, dtype)
        u = np.uint32 if dtype == np.float32 else np.uint64
        assert len(set(got[where].view(u).tolist())) == 1
        alone = sd.sddmm(1, n, [0, 1], [9], Mx[where[:1]], X[:1], Y, -0.5, 1.0, Mx[where[:1]], True, dtype)
        assert alone.view(u)[0] == got[where[0]].view(u)
    # the rule's order, spelled out for k = 3: T = 4, ((p0 + p1) + (p2 + 0))
    if k == 3:
        x, y = X[0], Y[9]
        want = ((0.0 + x[0] * y[0]) + (0.0 + x[1] * y[1])) + ((0.0 + x[2] * y[2]) + 0.0)
        assert sd.sddmm(1, n, [0, 1], [9], None, X[:1], Y)[0] == want and sd.tile(3) == 4
    assert [sd.tile(q) for q in (1, 2, 5, 64, 65, 1000)] == [1, 2, 8, 64, 64, 64]


def test_affinity_sees_through_a_diagonal_scaling():
    """aniso(32, 32, 1/64) and D A D, D = 2 ** default_rng(5).integers(-3, 4, n): the share of the rows whose kept
    off-diagonal set is anything but the row's x-neighbours.  Measured: affinity (theta 0.5, 16 vectors, 8 sweeps) at most
    1.0 % on A and 3.3 % on D A D over the seeds 0 .. 15 (0.0 % and 1.6 % at seed 0), the classical rule at theta 0.25
    0 % on A and 47.4 % on D A D."""
    nx = ny = 32
    A = matchref.aniso(nx, ny, 1.0 / 64)
    B = sd.scaled(A, 5)
    share = lambda S: sd.not_x_neighbours(S.indptr, S.indices, nx, ny)   # noqa: E731
    classical = share(sd.kept(A, 0.25)), share(sd.kept(B, 0.25))
    print("classical rule, theta 0.25: %.4f on A, %.4f on D A D" % classical)
    assert classical[0] == 0.0 and classical[1] > 0.40
    for name, M in (("A", A), ("D A D", B)):
        worst = 0.0
        for seed in range(16):
            C = sd.affinity_matrix(M, 16, 8, 2.0 / 3.0, seed)
            rule, united = share(sd.kept(C, 0.5)), share(sd.affinity_strength(M, 0.5, 16, 8, 2.0 / 3.0, seed))
            worst = max(worst, rule, united)
            assert rule <= 0.05 and united <= 0.05, (name, seed, rule, united)
            assert np.all(np.abs(C.diagonal() - 1.0) <= 4 * np.finfo(np.float64).eps)
        print("affinity, theta 0.5 on %s: at most %.4f over the seeds 0 .. 15" % (name, worst))
    S = sd.affinity_strength(B, 0.5, 16, 8, 2.0 / 3.0, 0)
    assert (S != S.T).nnz == 0 and np.all(S.diagonal() == 1) and (aggref.strength(S, 0.0) != S).nnz == 0
