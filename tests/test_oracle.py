"""CPU tests (-m "not gpu"): pin the oracle against the golden vectors.

The reference holds no expected outputs.  Since round 3 the first pin is the REFERENCE ITSELF:
tests/golden/ref_opencl_*.npz and ref_opencl_digests.json are outputs of its OpenCL branch (compiled unmodified,
oracle/Makefile `_ref`, run on an MI355X by oracle/make_ref_golden.py).  Beside them: the hand-derived answers for
the reference's two fixed inputs, scipy-generated fixtures (tests/golden/make_golden.py), the Poisson closed forms.
"""
import json
import os

import numpy as np
import pytest

from conftest import GOLDEN, load_golden
from benchmark_spgemm_using_csr_amd import gallery


def _run(oracle, g, nthreads=0):
    return oracle.spgemm(int(g["m"]), int(g["k"]), int(g["n"]), g["Ap"], g["Aj"], g["Ax"],
                         g["Bp"], g["Bj"], g["Bx"], nthreads=nthreads)


def test_small_test_known_answer(oracle):
    # inputs: SpGEMM_cuda/main.cu:153-205; expected: SURVEY.md §4
    g = load_golden("small_test.npz")
    Cp, Cj, Cx = _run(oracle, g)
    assert Cp.tolist() == [0, 1, 4, 4, 6]
    assert Cj.tolist() == [0, 0, 1, 3, 1, 3]
    assert Cx.tolist() == [10, 120, 190, 60, 120, 180]
    assert oracle.nnzCt(g["Ap"], g["Aj"], g["Bp"]) == 7


def test_cage4_known_answer(oracle):
    g = load_golden("cage4_sq.npz")
    Ap, Aj, Ax = g["Ap"], g["Aj"], g["Ax"]
    Cp, Cj, Cx = oracle.spgemm(9, 9, 9, Ap, Aj, Ax, Ap, Aj, Ax)
    assert oracle.nnzCt(Ap, Aj, Ap) == 269 and Cp[-1] == 81
    assert Cp.tolist() == list(range(0, 82, 9))
    assert np.array_equal(Cj, g["Cj"]) and np.allclose(Cx, g["Cx"], rtol=1e-13, atol=0)
    ones = np.ones_like(Ax)
    _, _, C1 = oracle.spgemm(9, 9, 9, Ap, Aj, ones, Ap, Aj, ones)
    assert C1[:9].tolist() == [5, 3, 2, 3, 3, 3, 3, 3, 2] and C1.sum() == 269
    # per-row upper bounds of the survey: {27,27,27,27,33,33,33,33,29}
    _, ub = oracle.nnzCt(Ap, Aj, Ap, want_ub=True)
    assert ub.tolist() == [27, 27, 27, 27, 33, 33, 33, 33, 29]


@pytest.mark.parametrize("name", ["p5_16.npz", "p27_6.npz", "p9_12.npz", "p7_7.npz", "rect_rand.npz"])
@pytest.mark.parametrize("nthreads", [1, 4])
def test_scipy_fixtures(oracle, name, nthreads):
    g = load_golden(name)
    Cp, Cj, Cx = _run(oracle, g, nthreads)
    assert np.array_equal(Cp, g["Cp"]) and np.array_equal(Cj, g["Cj"]) and np.array_equal(Cx, g["Cx"])
    assert oracle.nnzCt(g["Ap"], g["Aj"], g["Bp"]) == int(g["nnzCt"])


@pytest.mark.parametrize("tag", ["p5_256", "p27_51"])
def test_reference_default_sizes_checksums(oracle, tag):
    # the reference's default benchmark sizes (main.cu:32-51), digests from scipy
    ref = json.load(open(os.path.join(GOLDEN, "checksums.json")))[tag]
    rp, col = gallery.poisson_csr(ref["stencil"], *ref["dims"])
    val = gallery.fill_values(len(col))
    m = len(rp) - 1
    assert m == ref["m"] and len(col) == ref["nnzA"]
    Cp, Cj, Cx = oracle.spgemm(m, m, m, rp, col, val, rp, col, val)
    d = oracle.digest(Cp, Cj, Cx)
    assert d[0] == ref["nnzC"] and d[1] == ref["sum_rowptr"] and d[2] == ref["wsum_col"]
    assert np.array([d[3]], np.uint64).view(np.float64)[0] == ref["sum_val"]
    assert oracle.nnzCt(rp, col, rp) == ref["nnzCt"]


def test_poisson27_closed_forms(oracle):
    # nnzA=(3N-2)^3, nnzCt=(9N-10)^3, nnzC=(5N-6)^3
    for N in (4, 9, 16):
        rp, col = gallery.poisson_csr("poisson27pt", N, N, N)
        assert len(col) == (3 * N - 2) ** 3
        assert oracle.nnzCt(rp, col, rp) == (9 * N - 10) ** 3
        val = np.ones(len(col))
        Cp, _, _ = oracle.spgemm(N ** 3, N ** 3, N ** 3, rp, col, val, rp, col, val)
        assert Cp[-1] == (5 * N - 6) ** 3


def test_structural_zero_is_kept(oracle):
    # [[1,-1],[0,0]] * [[1,0],[1,0]]: the products cancel; the reference keeps the entry
    Ap = np.array([0, 2, 2], np.int32); Aj = np.array([0, 1], np.int32); Ax = np.array([1.0, -1.0])
    Bp = np.array([0, 1, 2], np.int32); Bj = np.array([0, 0], np.int32); Bx = np.array([1.0, 1.0])
    Cp, Cj, Cx = oracle.spgemm(2, 2, 2, Ap, Aj, Ax, Bp, Bj, Bx)
    assert Cp.tolist() == [0, 1, 1] and Cj.tolist() == [0] and Cx.tolist() == [0.0]


def test_csr_sort_indices(oracle):
    rng = np.random.default_rng(3)
    rp = np.array([0, 5, 5, 45, 46], np.int32)
    col = np.concatenate([rng.permutation(50)[:5], rng.permutation(100)[:40], [7]]).astype(np.int32)
    val = col.astype(np.float64) * 2 + 1
    oracle.csr_sort_indices(rp, col, val)
    for i in range(4):
        seg = col[rp[i]:rp[i + 1]]
        assert np.all(np.diff(seg) > 0)
    assert np.array_equal(val, col * 2.0 + 1)


def test_compare_reports_like_compData(oracle):
    g = load_golden("p5_16.npz")
    ref = (g["Cp"], g["Cj"], g["Cx"])
    good = (g["Cp"].astype(np.int32), g["Cj"].copy(), g["Cx"].copy())
    assert oracle.compare(ref, good)["ok"]
    bad = (good[0], good[1], good[2].copy()); bad[2][5] *= 1 + 1e-4
    r = oracle.compare(ref, bad)
    assert not r["ok"] and r["stage"] == 2 and r["val_err"] == 1
    bad = (good[0], good[1].copy(), good[2]); bad[1][3] += 1
    assert oracle.compare(ref, bad)["col_err"] == 1
    badp = good[0].copy(); badp[4] += 1
    assert oracle.compare(ref, (badp, good[1], good[2]))["stage"] == 1


@pytest.mark.parametrize("rel_tol", [0.0, 1e-6])
def test_compare_sees_non_finite_values(oracle, rel_tol):
    """compData's |ref - got| > tol*|ref| is false for a NaN result: compare() must still count it."""
    g = load_golden("p5_16.npz")
    ref = (g["Cp"], g["Cj"], g["Cx"].copy())
    got = lambda x: (g["Cp"].astype(np.int32), g["Cj"], x)              # noqa: E731
    # NaN where the reference is finite fails
    x = ref[2].copy(); x[7] = np.nan
    r = oracle.compare(ref, got(x), rel_tol=rel_tol)
    assert not r["ok"] and r["stage"] == 2 and r["val_err"] == 1 and r["col_err"] == 0
    # NaN where the reference is NaN passes
    ref[2][7] = np.nan
    assert oracle.compare(ref, got(x), rel_tol=rel_tol)["ok"]
    # ... a finite value where the reference is NaN fails
    assert not oracle.compare(ref, got(g["Cx"].copy()), rel_tol=rel_tol)["ok"]
    # +Inf against -Inf fails, +Inf against +Inf passes, a finite value against Inf fails either way round
    ref[2][7] = np.inf
    x[7] = -np.inf
    r = oracle.compare(ref, got(x), rel_tol=rel_tol)
    assert not r["ok"] and r["val_err"] == 1
    x[7] = np.inf
    assert oracle.compare(ref, got(x), rel_tol=rel_tol)["ok"]
    x[7] = 1.0
    r = oracle.compare(ref, got(x), rel_tol=rel_tol)
    assert not r["ok"] and r["val_err"] == 1
    r = oracle.compare((g["Cp"], g["Cj"], g["Cx"]), got(np.where(np.arange(len(x)) == 3, -np.inf, g["Cx"])), rel_tol=rel_tol)
    assert not r["ok"] and r["val_err"] == 1
    # finite results behave as before: equal passes, one entry off beyond the tolerance is one error, within it none
    y = g["Cx"].copy()
    assert oracle.compare((g["Cp"], g["Cj"], g["Cx"]), got(y), rel_tol=rel_tol)["ok"]
    y[5] *= 1 + 1e-4
    r = oracle.compare((g["Cp"], g["Cj"], g["Cx"]), got(y), rel_tol=rel_tol)
    assert not r["ok"] and r["stage"] == 2 and r["val_err"] == 1
    y = g["Cx"].copy(); y[5] *= 1 + 1e-9
    assert oracle.compare((g["Cp"], g["Cj"], g["Cx"]), got(y), rel_tol=rel_tol)["ok"] == (rel_tol > 0)


def test_value_fill_is_deterministic_and_shardable():
    a = gallery.fill_values(1000)
    assert a.min() >= 1 and a.max() <= 9 and np.all(a == np.round(a))
    b = np.concatenate([gallery.fill_values(400), gallery.fill_values(600, offset=400)])
    assert np.array_equal(a, b)
    assert a[:5].tolist() == [3.0, 9.0, 4.0, 9.0, 6.0]


def test_poisson_row_blocks_concatenate():
    rp, col = gallery.poisson_csr("poisson27pt", 5, 6, 7)
    m = 5 * 6 * 7
    parts = [gallery.poisson_csr("poisson27pt", 5, 6, 7, r0, r1) for r0, r1 in ((0, 70), (70, 150), (150, m))]
    assert np.array_equal(np.concatenate([p[1] for p in parts]), col)
    assert sum(len(p[0]) - 1 for p in parts) == m
    for name, dims in (("poisson5pt", (7, 9, 1)), ("poisson9pt", (8, 5, 1)), ("poisson7pt", (4, 5, 6))):
        rp, col = gallery.poisson_csr(name, *dims)
        assert (len(rp) - 1, len(col)) == gallery.poisson_closed_form(name, *dims)


def test_webbase_standin_matches_published_shape():
    """configs[3] stand-in (the SuiteSparse file is not in the image): same dimensions as Williams/webbase-1M
    (m = n = 1 000 005, nnz = 3 105 536, longest row ~4.7 k) within a few per cent, power-law row lengths."""
    from benchmark_spgemm_using_csr_amd import gallery
    rp, col = gallery.powerlaw_csr(1000005, 1000005, 3105536, 4700)
    lens = np.diff(rp)
    assert len(rp) - 1 == 1000005
    assert abs(int(rp[-1]) - 3105536) <= 0.04 * 3105536            # duplicates removed: slightly below target
    assert 4600 <= lens.max() <= 4700 and 4600 <= np.sort(lens)[-8] <= 4700   # 8 hub rows of ~4.7 k (webbase: 4700)
    assert (lens <= 3).mean() > 0.7                                 # most rows are tiny (webbase: ~70 % with <= 3)
    assert (lens > 100).sum() < 5000                                # a thin tail carries the long rows
    d = np.diff(col.astype(np.int64))
    starts = np.zeros(len(col), bool); starts[rp[1:-1][rp[1:-1] < len(col)]] = True
    assert np.all((d > 0) | starts[1:])                             # rows sorted, duplicate-free


def test_weblike_standin_has_webbase_shape_and_compression(oracle):
    """The second configs[3] stand-in (gallery.weblike_csr): webbase-1M's dimensions AND its duplicate accumulation --
    published (Liu & Vinter): 3 105 536 entries, longest row 4700, ~69.5 M products ->
    ~51.1 M entries of A^2 (1.36).  The oracle's A^2 must reproduce the digest scipy computed (checksums.json)."""
    rp, col = gallery.weblike_csr()
    lens = np.diff(rp)
    m = len(rp) - 1
    assert m == 1000005 and abs(len(col) - 3105536) <= 0.01 * 3105536 and 4600 <= lens.max() <= 4800
    assert lens.min() >= 1 and (lens <= 3).mean() > 0.6
    ref = json.load(open(os.path.join(GOLDEN, "checksums.json")))["weblike_1m"]
    val = gallery.fill_values(len(col))
    ct = oracle.nnzCt(rp, col, rp)
    Cp, Cj, Cx = oracle.spgemm(m, m, m, rp, col, val, rp, col, val)
    assert ct == ref["nnzCt"] and len(Cj) == ref["nnzC"]
    assert 1.30 <= ct / len(Cj) <= 1.42                              # (webbase-1M: 1.36; the round 1-3 stand-in: 1.007)
    assert abs(ct - 69.5e6) <= 0.03 * 69.5e6 and abs(len(Cj) - 51.1e6) <= 0.03 * 51.1e6
    t = np.arange(len(Cj), dtype=np.uint64) % np.uint64(8191) + np.uint64(1)
    assert int(Cp.astype(np.uint64).sum()) == ref["sum_rowptr"] and int((Cj.astype(np.uint64) * t).sum()) == ref["wsum_col"]
    assert float(Cx.sum()) == ref["sum_val"] and float((Cx * t.astype(np.float64)).sum()) == ref["wsum_val"]
    # long rows WITH duplicates: rows of more than 3072 products compress too
    _, ub = oracle.nnzCt(rp, col, rp, want_ub=True)
    big = ub > 3072
    assert big.sum() > 1500 and ub[big].sum() / np.diff(Cp)[big].sum() > 1.3


# ---------------------------------------------------------------------------------------------------------------
# Pins against outputs of the reference itself (SpGEMM_opencl on MI355X; generator: oracle/make_ref_golden.py).
# Structure bit-exact; values bit-exact for the integer-valued inputs, 1e-6 relative (north_star) for cage4's reals.
# ---------------------------------------------------------------------------------------------------------------
REF_FULL = ["small_test", "p5_16", "p27_6", "p9_12", "p7_7", "rect_rand", "cage4", "cage4_ones", "p27_12",
            "rand_bins", "cancel", "powerlaw_3k"]


def _sorted_rows(Cp, Cj, Cx):
    row = np.repeat(np.arange(len(Cp) - 1, dtype=np.int64), np.diff(Cp.astype(np.int64)))
    order = np.lexsort((Cj, row))
    return Cj[order], Cx[order]


@pytest.mark.parametrize("tag", REF_FULL)
def test_oracle_equals_reference_opencl_output(oracle, tag):
    g = load_golden("ref_opencl_%s.npz" % tag)
    Cp, Cj, Cx = _run(oracle, g)
    rCj, rCx = _sorted_rows(g["Cp"], g["Cj"], g["Cx"])
    assert bool(g["rows_sorted"])                      # the reference's kernels leave every row ascending
    assert np.array_equal(Cp, g["Cp"].astype(np.int64))
    assert np.array_equal(Cj, rCj)
    if tag == "cage4":
        assert np.all(np.abs(Cx - rCx) <= 1e-6 * np.abs(rCx))
    else:
        assert np.array_equal(Cx, rCx)
    assert oracle.nnzCt(g["Ap"], g["Aj"], g["Bp"]) == int(g["nnzCt"])


def test_reference_keeps_structural_zeros(oracle):
    # SURVEY.md §8b "explicit zeros retained": pinned by the reference's own output for the cancellation case
    g = load_golden("ref_opencl_cancel.npz")
    assert int((g["Cx"] == 0.0).sum()) == 168
    _, _, Cx = _run(oracle, g)
    assert int((Cx == 0.0).sum()) == 168


def test_reference_bins_are_all_exercised(oracle):
    # rand_bins / powerlaw_3k were built to reach every bin of bhsparse.h:373-406 incl. the EM re-queue rounds
    for tag, need in (("rand_bins", (0, 1, 2, 32, 33, 128, 129, 256, 257, 512, 513)), ("powerlaw_3k", (513, 2305, 9217))):
        g = load_golden("ref_opencl_%s.npz" % tag)
        _, ub = oracle.nnzCt(g["Ap"], g["Aj"], g["Bp"], want_ub=True)
        for lo in need:
            assert (ub >= lo).any(), (tag, lo)
        if tag == "rand_bins":
            assert (ub == 0).any() and ((ub >= 2) & (ub <= 32)).any() and ((ub >= 33) & (ub <= 512)).any()


@pytest.mark.parametrize("tag,gen", [
    ("p5_256", lambda: gallery.poisson_csr("poisson5pt", 256, 256, 1)),
    ("p27_51", lambda: gallery.poisson_csr("poisson27pt", 51, 51, 51)),
    ("powerlaw_20k", lambda: gallery.powerlaw_csr(20000, 20000, 90000, 3000)),
])
def test_oracle_equals_reference_opencl_digests(oracle, tag, gen):
    # the reference's default benchmark sizes (main.cu:32-51) and a power-law case with rows of up to 67 k products:
    # digests of the reference's C (the full comparison ran beside the reference on the GPU box: *_equal flags)
    ref = json.load(open(os.path.join(GOLDEN, "ref_opencl_digests.json")))[tag]
    assert ref["oracle_rowptr_equal"] and ref["oracle_col_equal"] and ref["oracle_val_bit_equal"]
    rp, col = gen()
    val = gallery.fill_values(len(col))
    m = len(rp) - 1
    assert m == ref["m"] and len(col) == ref["nnzA"]
    Cp, Cj, Cx = oracle.spgemm(m, m, m, rp, col, val, rp, col, val)
    t = np.arange(len(Cj), dtype=np.uint64) % np.uint64(8191) + np.uint64(1)
    assert len(Cj) == ref["nnzC"] and int(Cp.astype(np.uint64).sum()) == ref["sum_rowptr"]
    assert int((Cj.astype(np.uint64) * t).sum()) == ref["wsum_col"]
    assert float(Cx.sum()) == ref["sum_val"] and float((Cx * t.astype(np.float64)).sum()) == ref["wsum_val"]
    assert oracle.nnzCt(rp, col, rp) == ref["nnzCt"]


@pytest.mark.parametrize("dof", [1, 2, 3, 4])
def test_block_expand_is_the_kronecker_product_with_ones(oracle, dof):
    """gallery.block_expand_csr (the 3-dof FEM stand-in of bench.py and tools/) == scipy's kron(P, ones(dof, dof)),
    and its square through the oracle has dof^2 entries for every entry of the node-level square."""
    import scipy.sparse as sp
    rp, col = gallery.poisson_csr("poisson27pt", 5, 4, 3)
    m0 = len(rp) - 1
    rpb, colb = gallery.block_expand_csr(rp, col, dof)
    P = sp.csr_matrix((np.ones(len(col)), col, rp), shape=(m0, m0))
    M = sp.kron(P, np.ones((dof, dof)), format="csr")
    M.sort_indices()
    assert np.array_equal(rpb, M.indptr) and np.array_equal(colb, M.indices)
    val = gallery.fill_values(len(colb))
    m = m0 * dof
    Cp, Cj, Cx = oracle.spgemm(m, m, m, rpb, colb, val, rpb, colb, val)
    node = oracle.spgemm(m0, m0, m0, rp, col, np.ones(len(col)), rp, col, np.ones(len(col)))
    assert Cp[-1] == node[0][-1] * dof * dof
