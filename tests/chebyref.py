"""The inputs of the Chebyshev smoother's tests and amg.spectral_radius_device restated on the host: Lanczos on
D^-1/2 A D^-1/2 with numpy products (Paige's order: z = S v - beta v_prev, alpha = <v, z>, z -= alpha v), the largest
eigenvalue of the tridiagonal matrix."""
import functools

import numpy as np
import scipy.sparse as sp

import aggref as ar
import matchref as mr


def _csr(A):
    A = sp.csr_matrix(A)
    A.sort_indices()
    return A.shape[0], A.indptr.astype(np.int32), A.indices.astype(np.int32), A.data.astype(np.float64)


@functools.lru_cache(maxsize=None)
def matrices():
    """name -> (n, Ap, Aj, Ax): symmetric, positive diagonal, rows ascending"""
    rng = np.random.default_rng(7)
    R = sp.random(300, 300, 0.03, random_state=rng, data_rvs=lambda k: -rng.random(k))
    R = sp.triu(R, 1)
    R = R + R.T
    R = R + sp.diags(np.asarray(abs(R).sum(axis=1)).ravel() * (1.0 + rng.random(300)) + 0.1)
    return {
        "poisson5pt 16^2": ar.poisson("poisson5pt", 16, 16),
        "poisson5pt 32^2": ar.poisson("poisson5pt", 32, 32),
        "aniso 16^2": _csr(mr.aniso(16, 16, 0.01)),
        "poisson27pt 8^3": ar.poisson("poisson27pt", 8, 8, 8),
        "random 300": _csr(R),
    }


def scaled(n, Ap, Aj, Ax):
    A = sp.csr_matrix((Ax, Aj, Ap), shape=(n, n))
    s = 1.0 / np.sqrt(A.diagonal())
    return sp.diags(s) @ A @ sp.diags(s)


def lambda_max(n, Ap, Aj, Ax):
    return float(np.linalg.eigvalsh(scaled(n, Ap, Aj, Ax).toarray())[-1])


def lanczos(n, Ap, Aj, Ax, v, steps):
    S = scaled(n, Ap, Aj, Ax)
    v = v / np.linalg.norm(v)
    prev, beta, alphas, betas = np.zeros(n), 0.0, [], []
    for _ in range(min(steps, n)):
        z = S @ v - beta * prev
        alpha = float(v @ z)
        alphas.append(alpha)
        z = z - alpha * v
        nrm = float(np.linalg.norm(z))
        if not nrm > 1e-12 * max(abs(a) for a in alphas):
            break
        betas.append(nrm)
        prev, v, beta = v, z / nrm, nrm
    k = len(alphas)
    T = np.diag(alphas) + np.diag(betas[:k - 1], 1) + np.diag(betas[:k - 1], -1)
    return float(np.linalg.eigvalsh(T)[-1])
