"""CPU tests of the inputs tests/test_fsai_gpu.py uses (tests/fsairef.py): they reach every bin of bhs_csr_fsai_device and
the bins' two ends, the numpy restatement itself stays inside the backward-error bound the device is held to, and its
FSAI-preconditioned CG needs fewer iterations than Jacobi-preconditioned CG on the two grids."""
import numpy as np
import pytest

import fsairef as fr


def lengths(Gp):
    return np.diff(np.asarray(Gp, np.int64))


def test_the_exact_family_holds_every_length_and_comes_back_exactly():
    n, Ap, Aj, Ax, Gp, Gj, starts = fr.exact_family()
    assert n == 498 == sum(fr.BLOCKS) and len(Gj) == sum(k * (k + 1) // 2 for k in fr.BLOCKS)
    d = lengths(Gp)
    assert set(d.tolist()) == set(range(1, fr.MAX_ROW + 1))          # every length, so every bin and both ends of each
    for edge in (1, fr.SHORT_D, fr.SHORT_D + 1, fr.WAVE_D, fr.WAVE_D + 1, fr.MAX_ROW):
        assert edge in d
    assert fr.invalid(n, Ap, Aj, Gp, Gj) is None
    assert np.array_equal(Ax, Ax.astype(np.float32).astype(np.float64))   # exact in float too
    # the factor of every block's last row is L0: roots and divisions by powers of two only
    val, bad, kept = fr.fsai(n, Ap, Aj, Ax, Gp, Gj, keep=True)
    assert bad == -1 and np.all(np.isfinite(val))
    for s, k in zip(starts, fr.BLOCKS):
        J, M, L = kept[s + k - 1]
        assert len(J) == k and np.array_equal(L @ L.T, np.tril(M) + np.tril(M, -1).T)
        diag = np.diag(L)
        assert np.all((diag == 1) | (diag == 2) | (diag == 4)) and np.all(np.abs(np.tril(L, -1) * 8) <= 3)
        assert np.array_equal(np.tril(L, -1) * 8, np.round(np.tril(L, -1) * 8))
    # (G A G^T)_ii = 1 up to rounding, whatever the row's length
    G, A = fr.fsai_matrix(n, Gp, Gj, val), fr.csr(n, Ap, Aj, Ax)
    assert np.allclose((G @ A @ G.T).diagonal(), 1.0, rtol=0, atol=1e-9)


def test_the_grid_and_the_random_patterns_reach_their_bins():
    n, Ap, Aj, _ = fr.grid("poisson5pt_33")
    Gp, _ = fr.tril_pattern(n, Ap, Aj)
    assert n == 1089 and lengths(Gp).max() == 3 and n > 16 * 16    # short rows over many workgroups
    n, Ap, Aj, Ax = fr.random_spd()
    assert n == 729 and np.all(Ax[np.repeat(np.arange(n), np.diff(Ap)) != Aj] < 0)
    d1, d2 = lengths(fr.tril_pattern(n, Ap, Aj)[0]), lengths(fr.tril_pattern(n, Ap, Aj, 2)[0])
    assert d1.max() == 14 and d2.max() == 63                        # the short bin alone; the short and the wave bin
    assert np.any(d2 <= fr.SHORT_D) and np.any(d2 > fr.SHORT_D) and d2.max() <= fr.WAVE_D
    A = fr.csr(n, Ap, Aj, Ax)
    assert (A != A.T).nnz == 0 and np.linalg.eigvalsh(A.toarray()).min() > 0
    Ep, Ej = fr.with_extra_lower(n, *fr.tril_pattern(n, Ap, Aj), seed=3)
    assert fr.invalid(n, Ap, Aj, Ep, Ej) is None and len(Ej) > len(fr.tril_pattern(n, Ap, Aj)[1])


@pytest.mark.parametrize("power", (1, 2), ids=("tril(A)", "tril(A^2)"))
def test_the_restatement_stays_inside_the_bound(power):
    n, Ap, Aj, Ax = fr.random_spd()
    Gp, Gj = fr.tril_pattern(n, Ap, Aj, power)
    for dtype in (np.float64, np.float32):
        val, bad, kept = fr.fsai(n, Ap, Aj, Ax, Gp, Gj, dtype, keep=True)
        worst = fr.worst_error_over_bound(Gp, val, kept, dtype)
        print("random SPD, tril(A^%d), %s: the restatement's worst error / bound %.3f" % (power, np.dtype(dtype).name, worst))
        assert bad == -1 and worst <= 1.0


def test_the_restatement_stays_inside_the_bound_on_dense_blocks():
    n, Ap, Aj, Ax, Gp, Gj, _ = fr.exact_family()
    rng = np.random.default_rng(5)
    B = fr.csr(n, Ap, Aj, rng.uniform(-1.0, 0.0, len(Aj)))
    B = (B + B.T).tocsr()
    B.setdiag(0)
    B = (B + fr.csr(n, np.arange(n + 1), np.arange(n), np.asarray(abs(B).sum(axis=1)).ravel() + 1.0)).tocsr()
    B.sort_indices()
    val, bad, kept = fr.fsai(n, B.indptr, B.indices, B.data, Gp, Gj, keep=True)
    worst = fr.worst_error_over_bound(Gp, val, kept)
    print("dense blocks up to 128: the restatement's worst error / bound %.3f" % worst)
    assert bad == -1 and worst <= 1.0


@pytest.mark.parametrize("name", ("poisson27pt_9", "poisson5pt_33"))
def test_fsai_pcg_needs_fewer_iterations_than_jacobi_pcg(name):
    n, Ap, Aj, Ax = fr.grid(name)
    A = fr.csr(n, Ap, Aj, Ax)
    b = np.random.default_rng(0).standard_normal(n)
    x, its, res = fr.fsai_pcg(A, b, 1e-8, 300)
    _, jac, _ = fr.jacobi_pcg(A, b, 1e-8, 300)
    print("%s: FSAI-PCG %d iterations, Jacobi-PCG %d" % (name, its, jac))
    assert its < jac < 300 and res[-1] <= 1e-8 * res[0]
    assert np.linalg.norm(b - A @ x) <= 1.01e-8 * np.linalg.norm(b)
