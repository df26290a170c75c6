"""CPU tests of the "approximate inverse" (include/bhsparse_hip.h): what bhs_csr_fsai_device refuses without a device, the
Python layers' signatures, the refusal words of the numpy restatement tests/fsairef.py, and the restatement against
numpy's own Cholesky factorisation and inverse."""
import inspect

import numpy as np

import fsairef as fr

from benchmark_spgemm_using_csr_amd import _lib, amg


def test_null_handle_is_refused(hiplib):
    args = (None, 0, 0, None, None, None, 0, None, None, None, 0, None, None)
    assert hiplib.bhs_csr_fsai_device(*args) == _lib.BHS_ERR_INVALID_ARG
    assert _lib.load(f32=True).bhs_csr_fsai_device(*args) == _lib.BHS_ERR_INVALID_ARG


def test_python_layers():
    sig = lambda f: list(inspect.signature(f).parameters)           # noqa: E731
    default = lambda f, name: inspect.signature(f).parameters[name].default   # noqa: E731
    assert _lib.BHS_FSAI_MAX_ROW == 128 == fr.MAX_ROW
    assert "bhs_csr_fsai_device" in _lib.SYMBOLS and len(_lib.SYMBOLS["bhs_csr_fsai_device"][1]) == 13
    assert "#define BHS_FSAI_MAX_ROW 128" in open(_lib.HEADER).read()
    assert sig(amg.fsai_raw_device) == ["bh", "n", "nnzA", "d_rowPtrA", "d_colIndA", "d_valA", "nnzG", "d_rowPtrG", "d_colIndG",
                                        "d_valG", "flags"]
    assert sig(amg.fsai_device) == ["bh", "A", "pattern"] == sig(amg.fsai_setup_device)
    assert default(amg.fsai_device, "pattern") is None and default(amg.fsai_setup_device, "pattern") is None
    assert sig(amg.fsai_apply_device) == ["bh", "M", "r", "z"] == sig(amg.ilu0_apply_device)
    assert sig(amg.fsai_pcg_device) == ["bh", "A", "b", "tol", "maxiter", "pattern"]
    assert [default(amg.fsai_pcg_device, p) for p in ("tol", "maxiter", "pattern")] == [1e-8, 100, None]
    assert sig(amg.ilu0_pcg_device) == ["bh", "A", "b", "tol", "maxiter", "ordering"]
    assert [default(amg.ilu0_pcg_device, p) for p in ("tol", "maxiter", "ordering")] == [1e-8, 100, "colour"]
    for name in ("bhs_fsai.hip.h", "bhs_host_fsai.inc.h"):
        assert name in _lib.SOURCES


def test_the_refusal_words():
    Ap, Aj = np.array([0, 1, 3, 6]), np.array([0, 0, 1, 0, 1, 2])
    Gp, Gj = np.array([0, 1, 3, 5]), np.array([0, 0, 1, 1, 2])
    assert fr.invalid(3, Ap, Aj, Gp, Gj) is None and fr.invalid(0, None, None, None, None) is None
    got = [fr.invalid(-1, Ap, Aj, Gp, Gj), fr.invalid(3, Ap, Aj, Gp, Gj, flags=1), fr.invalid(3, Ap, Aj, Gp, None, nnzG=5),
           fr.invalid(3, Ap, Aj, Gp, Gj, nnzG=2), fr.invalid(3, Ap, Aj, Gp, Gj, overlap=True)]
    assert tuple(got) == fr.HOST_REFUSALS
    got = [fr.invalid(3, Ap, Aj, [1, 1, 3, 5], Gj),
           fr.invalid(3, Ap, Aj, [0, 1, 1, 3], [0, 1, 2]),
           fr.invalid(130, np.arange(131), np.arange(130), np.concatenate([np.arange(129), [130, 259]]),
                      np.concatenate([np.arange(128), [127, 128], np.arange(129)])),
           fr.invalid(3, Ap, Aj, Gp, [0, 2, 1, 1, 2]),
           fr.invalid(3, Ap, Aj, Gp, [0, 1, 1, 1, 2]),
           fr.invalid(3, Ap, Aj, Gp, [0, 0, 1, 0, 1]),
           fr.invalid(3, [0, 1, 7, 6], Aj, Gp, Gj),
           fr.invalid(3, Ap, [0, 0, 1, 0, -1, 2], Gp, Gj),
           fr.invalid(3, Ap, [0, 0, 1, 1, 0, 2], Gp, Gj)]
    assert tuple(got) == fr.DEVICE_REFUSALS
    # what lies behind the first entry at or beyond the diagonal of a row of A is not looked at
    assert fr.invalid(3, [0, 3, 5, 8], [0, 2, 1, 0, 1, 0, 1, 2], Gp, Gj) is None


def test_the_restatement_against_numpy():
    """row i of G is the last row of inv(chol(A(J, J))); a diagonal pattern gives 1 / sqrt(a_ii) by the two operations"""
    n, Ap, Aj, Ax = fr.random_spd()
    A = fr.csr(n, Ap, Aj, Ax).toarray()
    Gp, Gj = fr.with_extra_lower(n, *fr.tril_pattern(n, Ap, Aj), seed=3)
    val, bad = fr.fsai(n, Ap, Aj, Ax, Gp, Gj)
    assert bad == -1
    for i in (0, 1, 100, 400, n - 1):
        J = Gj[Gp[i]:Gp[i + 1]]
        want = np.linalg.inv(np.linalg.cholesky(A[np.ix_(J, J)]))[-1]
        assert np.allclose(val[Gp[i]:Gp[i + 1]], want, rtol=1e-12, atol=0)
    G = fr.fsai_matrix(n, Gp, Gj, val)
    assert np.allclose((G @ A @ G.T).diagonal(), 1.0, rtol=0, atol=1e-13)
    # tril(A) in place of A: the same bits (entries beyond the diagonal are never used)
    T = np.tril(A)
    import scipy.sparse as sp
    Tl = sp.csr_matrix(T)
    Tl.sort_indices()
    assert fr.same_bits(fr.fsai(n, Tl.indptr, Tl.indices, Tl.data, Gp, Gj)[0], val)
    dp, dj = np.arange(n + 1), np.arange(n)
    dv, _ = fr.fsai(n, Ap, Aj, Ax, dp, dj)
    assert np.array_equal(dv, 1.0 / np.sqrt(A.diagonal()))
    dv32, _ = fr.fsai(n, Ap, Aj, Ax, dp, dj, np.float32)
    a32 = A.diagonal().astype(np.float32).astype(np.float64)
    assert dv32.dtype == np.float32 and np.array_equal(dv32, (1.0 / np.sqrt(a32)).astype(np.float32))


def test_pivots_of_the_restatement():
    n, Ap, Aj, Ax, Gp, Gj, starts = fr.exact_family()
    clean, bad = fr.fsai(n, Ap, Aj, Ax, Gp, Gj)
    assert bad == -1
    r = np.repeat(np.arange(n), np.diff(Ap))
    x = Ax.copy()
    at = starts[3] + 5                                              # a diagonal entry in the block of order 16
    x[(r == at) & (Aj == at)] *= -1
    val, bad = fr.fsai(n, Ap, Aj, x, Gp, Gj)
    assert bad == at                                               # the first row whose J holds the entry
    keep = np.repeat(np.arange(n) < starts[3], np.diff(Gp)) | np.repeat(np.arange(n) >= starts[4], np.diff(Gp))
    assert fr.same_bits(val[keep], clean[keep]) and np.isnan(val[~keep]).any()
