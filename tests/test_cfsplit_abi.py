"""CPU tests of the C/F splitting and the direct interpolation (bhs_csr_cfsplit_device, bhs_csr_interp_symbolic_device,
bhs_csr_interp_numeric_device): the header, the binding and the libraries agree, and tests/cfref.py -- the reference of the
GPU tests -- is checked against the definitions it restates: the rounds against the sequential greedy set, independence and
maximality, colour 0 of the colouring's restatement, the interpolation on a case worked out by hand and on the Poisson
matrices' zero row sums."""
import ctypes as C
import re

import numpy as np
import pytest
import scipy.sparse as sp

import aggref as ar
import ccref
import cfref as cr
import gsref as gr
import matchref as mr

from benchmark_spgemm_using_csr_amd import _lib, amg

NAMES = ("bhs_csr_cfsplit_device", "bhs_csr_interp_symbolic_device", "bhs_csr_interp_numeric_device")
PATTERNS = tuple(ar.gpu_cases()) + ("star_centre_last",)


def pattern(name):
    return ccref.star_centre_last() if name == "star_centre_last" else ar.gpu_cases()[name]


# ---------------------------------------------------------------- the interface
def test_header_declares_the_entry_points():
    txt = open(_lib.HEADER).read()
    assert "C/F splitting and interpolation" in txt and re.search(r"#define\s+BHS_CF_DEGREE\s+1\b", txt)
    for name in NAMES:
        assert re.search(r"BHS_API\s+int\s+%s\s*\(" % name, txt), name
        assert name in _lib.SYMBOLS
    for stat in ("cf_init", "cf_round", "cf_number", "interp_count", "interp_fill"):
        assert stat in txt, stat
    assert _lib.BHS_CF_DEGREE == cr.DEGREE == 1
    assert len(_lib.SYMBOLS["bhs_csr_cfsplit_device"][1]) == 13
    assert len(_lib.SYMBOLS["bhs_csr_interp_symbolic_device"][1]) == 13
    assert len(_lib.SYMBOLS["bhs_csr_interp_numeric_device"][1]) == 17


def test_both_libraries_export_the_entry_points(hiplib):
    for path in (_lib.SO_PATH, _lib.SO_PATH_F32):
        raw = C.CDLL(path)
        for name in NAMES:
            assert getattr(raw, name) is not None
    blob = open(_lib.SO_PATH, "rb").read()
    for kern in (b"k_cf_init", b"k_cf_round", b"k_cf_number", b"k_ip_count", b"k_ip_fill"):
        assert kern in blob, kern


def test_null_handle_is_refused(hiplib):
    assert hiplib.bhs_csr_cfsplit_device(None, 0, 0, None, None, None, 0, 0, None, None, None, None, None) == _lib.BHS_ERR_INVALID_ARG
    assert hiplib.bhs_csr_interp_symbolic_device(None, 0, 0, None, None, 0, None, None, None, 0, None, None, None) == _lib.BHS_ERR_INVALID_ARG
    assert hiplib.bhs_csr_interp_numeric_device(None, 0, 0, None, None, None, 0, None, None, None, 0, None, 0, None, None, 0,
                                                None) == _lib.BHS_ERR_INVALID_ARG


def test_python_module_has_the_calls():
    for f in ("cfsplit_raw_device", "cfsplit_device", "interp_symbolic_raw_device", "interp_numeric_raw_device",
              "interp_direct_device", "interp_values_device", "rs_setup_device", "rs_setup_csr"):
        assert callable(getattr(amg, f)), f
    from benchmark_spgemm_using_csr_amd.facade import bhsparse
    bh = bhsparse()                                                  # no platform: every raw call says so
    assert amg.cfsplit_raw_device(bh, 0, 0, None, None, None, 0, 0, None, None) == _lib.BHS_ERR_NOT_READY
    assert amg.interp_symbolic_raw_device(bh, 0, 0, None, None, 0, None, None, None, 0, None) == _lib.BHS_ERR_NOT_READY
    assert amg.interp_numeric_raw_device(bh, 0, 0, None, None, None, 0, None, None, None, 0, None, 0, None, None) == _lib.BHS_ERR_NOT_READY


# ---------------------------------------------------------------- the splitting
def test_degree_keys_by_hand():
    Sp = np.array([0, 0, 3, 2000], np.int64)
    key = cr.keys(3, Sp, seed=5, degree=True)
    h = ar.hash32(np.arange(3), 5)
    for i, deg in enumerate((0, 3, 1023)):                           # (a row of 1997 entries counts as 1023)
        assert int(key[i]) == ((deg << 21 | int(h[i]) >> 11) << 31) | i
    assert np.array_equal(cr.keys(3, Sp, seed=5), ar.keys(3, 5))
    assert int(key.max()) < 1 << 62


@pytest.mark.parametrize("name", PATTERNS)
def test_rounds_equal_greedy_and_the_structure_holds(name):
    n, Sp, Sj = pattern(name)
    prio = np.random.default_rng(3).integers(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32)
    for seed, p, degree in ((0, None, False), (1, None, False), (0, prio, False), (0, None, True), (1, None, True)):
        key = cr.keys(n, Sp, seed, p, degree)
        assert len(np.unique(key)) == n
        cf, nc, nrounds = cr.split(n, Sp, Sj, seed, p, degree)
        assert np.array_equal(cf >= 0, cr.greedy(n, Sp, Sj, key)), (name, seed, degree)
        cr.check_split(n, Sp, Sj, cf, nc)
        assert 1 <= nrounds <= n
        if not degree:                                               # colour 0 of the first-fit colouring under the same keys
            assert np.array_equal(cf >= 0, gr.greedy(n, Sp, Sj, key) == 0), (name, seed)
    deg = np.diff(Sp)
    isolated = np.array([set(Sj[Sp[i]:Sp[i + 1]]) <= {i} for i in range(n)])
    assert np.all(cr.split(n, Sp, Sj, 0, None, True)[0][isolated] >= 0)
    if name == "star1024":                                           # the hub has the greatest degree: it alone is C
        assert deg[0] == deg.max() and cr.split(n, Sp, Sj, 0, None, True)[1] == 1


def test_a_path_with_ascending_keys_takes_n_rounds():
    n, Sp, Sj = ar.gpu_cases()["path300"]
    prio = (np.arange(n, dtype=np.uint64) * 2).astype(np.uint32)
    cf, nc, nrounds = cr.split(n, Sp, Sj, 0, prio)
    assert nrounds == n and nc == n // 2 and np.array_equal(np.flatnonzero(cf >= 0), np.arange(n - 1, -1, -2)[::-1])


def test_a_directed_triangle_ends():
    n, Ap, Aj, _ = mr.directed_triangle()
    for seed in range(4):
        cf, nc, nrounds = cr.split(n, Ap, Aj, seed)
        assert 1 <= nc <= n and nrounds <= n and np.array_equal(np.sort(cf[cf >= 0]), np.arange(nc))


def test_empty_and_counts():
    assert cr.split(0, np.zeros(1, np.int32), np.zeros(0, np.int32))[1:] == (0, 0)
    n, Sp, Sj = ar.gpu_cases()["poisson5pt_33"]
    counts = []
    _, _, nrounds = cr.split(n, Sp, Sj, 0, None, True, counts)
    assert len(counts) == nrounds and counts[0] == n and all(a > b for a, b in zip(counts, counts[1:]))


# ---------------------------------------------------------------- the interpolation
def by_hand():
    """C points 1 and 2.  Row 0: two negative-type coarse neighbours and a positive-type fine one, which goes to the
    diagonal.  Row 3: a weak negative-type neighbour (0 is not in S's row) that goes to the diagonal, a positive-type coarse
    neighbour and an explicit zero at a coarse one."""
    A = np.array([[4.0, -1.0, -2.0, 2.0], [-1.0, 4.0, 0.0, 1.0], [-2.0, 0.0, 4.0, 0.0], [-1.0, 1.0, 0.0, 2.0]])
    Ap = np.array([0, 4, 7, 9, 13], np.int32)
    Aj = np.array([0, 1, 2, 3, 0, 1, 3, 0, 2, 0, 1, 2, 3], np.int32)
    Ax = np.array([A[i, j] for i in range(4) for j in Aj[Ap[i]:Ap[i + 1]]])
    Sp = np.array([0, 4, 7, 9, 12], np.int32)
    Sj = np.array([0, 1, 2, 3, 0, 1, 3, 0, 2, 1, 2, 3], np.int32)
    return 4, Ap, Aj, Ax, Sp, Sj, np.array([-1, 0, 1, -1], np.int32)


def test_interp_by_hand():
    n, Ap, Aj, Ax, Sp, Sj, cf = by_hand()
    for L in (None, 1, 4, 16, 64):
        Pp, Pj, Px = cr.interp(n, Ap, Aj, Ax, Sp, Sj, cf, L)
        assert Pp.tolist() == [0, 2, 3, 4, 6] and Pj.tolist() == [0, 1, 0, 1, 0, 1]
        # row 0: d' = 4 + 2, weights -((-3 / -3) a) / 6; row 3: d' = 2 - 1, weight -((1 / 1) 1) / 1 and a zero
        assert Px.tolist() == [-(1.0 * -1.0) / 6.0, -(1.0 * -2.0) / 6.0, 1.0, 1.0, -1.0, 0.0]
    assert cr.invalid_interp(n, len(Aj), Ap, Aj, len(Sj), Sp, Sj, cf, 2) is None
    P = cr.interp(n, Ap, Aj, Ax, Sp, Sj, cf)
    assert cr.invalid_interp(n, len(Aj), Ap, Aj, len(Sj), Sp, Sj, cf, 2, P[0], 6) is None


def test_interp_without_a_diagonal_gives_the_ieee_results():
    n, Ap, Aj, Ax, Sp, Sj, cf = by_hand()
    keep = ~((np.repeat(np.arange(n), np.diff(Ap)) == Aj) & (Aj == 0))   # row 0 loses its diagonal
    Bp = np.array([0, 3, 6, 8, 12], np.int32)
    Pp, Pj, Px = cr.interp(n, Bp, Aj[keep], Ax[keep], Sp, Sj, cf)
    assert Pp.tolist() == [0, 2, 3, 4, 6] and np.isnan(Px[:2]).all() and Px[2:].tolist() == [1.0, 1.0, -1.0, 0.0]


def test_row_sums_follow_the_lanes():
    rng = np.random.default_rng(8)
    Ap = np.array([0, 0, 1, 6, 23, 24], np.int64)
    v = rng.standard_normal(24)
    for L in (1, 4, 16, 64):
        got = cr.row_sums(5, Ap, v, L)
        for i in range(5):
            row = v[Ap[i]:Ap[i + 1]]
            lane = [0.0] * L
            for k, x in enumerate(row):
                lane[k % L] += x
            while len(lane) > 1:                                     # the butterfly: neighbours at distance 1, 2, 4, ..
                lane = [lane[2 * t] + lane[2 * t + 1] for t in range(len(lane) // 2)]
            assert got[i] == lane[0], (L, i)


@pytest.mark.parametrize("name", ("poisson5pt_33", "poisson27pt_9", "poisson9pt_20"))
def test_interpolation_reproduces_constants_where_rows_sum_to_zero(name):
    """Where A's row sums to 0 the weights of an F row sum to -(N- + N+) / d' = 1, whichever sign went to the diagonal: each
    weight carries three roundings and a row adds at most 26 of them, all of one sign here: within 30 u < 1e-14."""
    kind, size = name.split("_")
    n, Ap, Aj, Ax = ar.poisson(kind, *([int(size)] * (3 if kind == "poisson27pt" else 2)))
    A = sp.csr_matrix((Ax, Aj, Ap), shape=(n, n))
    S = ar.strength(A, 0.25)
    cf, nc, _ = cr.split(n, S.indptr, S.indices, 0, None, True)
    Pp, Pj, Px = cr.interp(n, Ap, Aj, Ax, S.indptr, S.indices, cf)
    P = sp.csr_matrix((Px, Pj, Pp), shape=(n, nc))
    assert np.all(np.diff(Pp)[cf >= 0] == 1) and np.array_equal(Pj[Pp[:-1][cf >= 0]], cf[cf >= 0]) and np.all(Px[Pp[:-1][cf >= 0]] == 1.0)
    assert np.all(np.diff(Pp)[cf < 0] >= 1)                          # every F point has a strong C neighbour
    rows = np.repeat(np.arange(n), np.diff(Pp))
    inner = np.ones(len(Pj), bool)
    inner[Pp[:-1]] = False
    assert np.all(np.diff(Pj)[inner[1:]] > 0), "P's rows ascend strictly"
    zero = np.asarray(A.sum(axis=1)).ravel() == 0
    assert zero.sum() > n // 3 and np.all(np.abs(np.asarray(P.sum(axis=1)).ravel()[zero] - 1.0) < 1e-14)
    assert rows.max() == n - 1


def test_invalid_names_what_is_refused():
    n, Sp, Sj = ar.gpu_cases()["poisson5pt_33"]
    nnz = len(Sj)
    assert cr.invalid_split(n, nnz, Sp, Sj) is None and cr.invalid_split(0, 0, None, None) is None
    assert cr.invalid_split(n, nnz, Sp, Sj, flags=cr.DEGREE) is None
    assert cr.invalid_split(-1, 0, Sp, Sj) == "negative size" and cr.invalid_split(n, nnz, Sp, Sj, flags=2) == "unknown flag"
    assert cr.invalid_split(n, nnz, Sp, Sj, flags=cr.DEGREE, has_prio=True) == "degree keys with caller priorities"
    assert cr.invalid_split(n, nnz, Sp, Sj, has_cf=False) == "NULL array"
    assert cr.invalid_split(n, nnz, Sp, Sj, overlap=True) == "an output overlaps an input"
    j = Sj.copy(); j[7] = n                                          # noqa: E702
    assert cr.invalid_split(n, nnz, Sp, j) == "column out of range"
    p = Sp.copy(); p[100] = p[99] - 1                                # noqa: E702
    assert cr.invalid_split(n, nnz, p, Sj) == "bad row pointer"
    cf, nc, _ = cr.split(n, Sp, Sj)
    args = (n, nnz, Sp, Sj, nnz, Sp, Sj)
    Pp = cr.interp(n, Sp, Sj, np.ones(nnz), Sp, Sj, cf)[0]
    assert cr.invalid_interp(*args, cf, nc) is None and cr.invalid_interp(*args, cf, nc, Pp, int(Pp[n])) is None
    assert cr.invalid_interp(*args, cf, -1) == "negative size" and cr.invalid_interp(*args, cf, n + 1) == "size out of range"
    assert cr.invalid_interp(*args, cf, nc, flags=1) == "unknown flag" and cr.invalid_interp(*args, cf, nc, null=True) == "NULL array"
    assert cr.invalid_interp(*args, cf, nc, overlap=True) == "an output overlaps an input"
    assert cr.invalid_interp(*args, cf, nc - 1) == "cf out of range"
    bad = cf.copy(); bad[5] = -2                                     # noqa: E702
    assert cr.invalid_interp(*args, bad, nc) == "cf out of range"
    j = Sj.copy(); j[[Sp[40], Sp[40] + 1]] = j[[Sp[40] + 1, Sp[40]]]   # noqa: E702
    assert cr.invalid_interp(n, nnz, Sp, j, nnz, Sp, Sj, cf, nc) == "a row that does not ascend strictly"
    assert cr.invalid_interp(n, nnz, Sp, Sj, nnz, Sp, j, cf, nc) == "a row that does not ascend strictly"
    other = cr.split(n, Sp, Sj, 1)[0]
    assert cr.invalid_interp(*args, other, cr.split(n, Sp, Sj, 1)[1], Pp, int(Pp[n])) == "rowPtrP is not this splitting's"
    assert cr.invalid_interp(*args, cf, nc, Pp, int(Pp[n]) - 1) == "rowPtrP is not this splitting's"


# ---------------------------------------------------------------- the hierarchy on the restatements
def test_the_hierarchy_converges():
    """cfref.rs_setup and cfref.pcg, the references of the GPU test's iteration counts: theta 0.25, min_coarse 40, PCG to
    1e-8 with the Jacobi cycle from a random right-hand side"""
    for name, A in (("poisson5pt_33", None), ("aniso32", mr.aniso(32, 32, 1e-2))):
        if A is None:
            n, Ap, Aj, Ax = ar.poisson("poisson5pt", 33, 33)
            A = sp.csr_matrix((Ax, Aj, Ap), shape=(n, n))
        n = A.shape[0]
        levels, sizes = cr.rs_setup(A)
        assert len(levels) >= 3 and levels[-1][0].shape[0] <= 40 and sizes[0] < n // 2 + 1
        for Al, P, R in levels[:-1]:
            assert P.shape == (Al.shape[0], R.shape[0]) and abs(R - P.T).nnz == 0
        b = np.random.default_rng(4).standard_normal(n)
        x, its, res = cr.pcg(levels, b)
        assert its <= 30 and np.linalg.norm(b - A @ x) <= 1e-7 * np.linalg.norm(b), (name, its)
