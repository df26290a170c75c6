"""CPU tests of the assembly's reference and of the GPU tests' inputs.

tests/cooref.py against scipy (coo_matrix.tocsr(): sorted, duplicates summed) on integer values and against
gallery._csr_from_pairs on patterns, and against a case written out by hand; then tests/asminputs.py's inputs: the raw row
lengths sit on both sides of the library's bin limits, the runs sit where the docstring says, the scanned counts take
scantiles' roles (as tests/test_scan_tiles_shapes.py asserts its own)."""
import numpy as np
import pytest
import scipy.sparse as sp

import asminputs as ai
import cooref as cr
import gridpass as gp
import scantiles as st

from benchmark_spgemm_using_csr_amd import gallery


# ---------------------------------------------------------------- the reference
def test_cooref_by_hand():
    #           e:  0    1    2     3    4    5    6     7
    rows = [2, 0, 2, -1, 0, 2, 3, 2]
    cols = [1, 3, 1, 0, 3, 0, -5, 1]
    vals = np.array([1.0, -0.0, 2.0, 9.0, 0.0, 5.0, 9.0, 4.0])
    with pytest.raises(cr.Refused):
        cr.assemble(4, 4, rows, cols, vals, cr.SUM)
    with pytest.raises(cr.Refused):
        cr.assemble(3, 4, rows, cols, vals, cr.SUM | cr.IGNORE_NEGATIVE)      # row 3 >= m: with or without the flag
    Zp, Zj, Zx, ent, perm, nkept = cr.assemble(4, 4, rows, cols, vals, cr.SUM | cr.IGNORE_NEGATIVE)
    assert nkept == 6 and perm.tolist() == [1, 4, 5, 0, 2, 7]
    assert Zp.tolist() == [0, 1, 1, 3, 3] and Zj.tolist() == [3, 0, 1] and ent.tolist() == [0, 2, 3, 6]
    assert Zx.tolist() == [0.0, 5.0, 7.0] and not np.signbit(Zx[0])            # -0 + 0 = +0
    for flags, want in ((cr.FIRST, [-0.0, 5.0, 1.0]), (cr.LAST, [0.0, 5.0, 4.0])):
        got = cr.assemble(4, 4, rows, cols, vals, flags | cr.IGNORE_NEGATIVE)[2]
        assert got.tolist() == want and np.signbit(got[0]) == np.signbit(want[0])
    Zp, Zj, Zx, ent, perm, nkept = cr.assemble(4, 4, rows, cols, vals, cr.KEEP | cr.IGNORE_NEGATIVE)
    assert Zp.tolist() == [0, 2, 2, 6, 6] and Zj.tolist() == [3, 3, 0, 1, 1, 1] and ent.tolist() == list(range(7))
    assert Zx.tolist() == [-0.0, 0.0, 5.0, 1.0, 2.0, 4.0] and np.signbit(Zx[0])
    assert cr.assemble(4, 4, rows, cols, None, cr.IGNORE_NEGATIVE)[2] is None


def test_cooref_sums_in_order_and_rounds_once():
    big = np.array([1e16, 1.0, 1.0, -1e16, np.inf, -0.0], np.float64)
    rows, cols = [0, 0, 0, 0, 1, 2], [0, 0, 0, 0, 0, 0]
    Zx = cr.assemble(3, 1, rows, cols, big, cr.SUM)[2]
    assert Zx[0] == 0.0 and Zx[1] == np.inf and Zx[2] == 0.0 and np.signbit(Zx[2])   # ((1e16 + 1) + 1) - 1e16 = 0; a lone -0 stays
    f = np.array([16777216.0, 1.0, 1.0], np.float32)                  # in float each + 1 is lost; in double both stay
    Zx = cr.assemble(1, 1, [0, 0, 0], [0, 0, 0], f, cr.SUM)[2]
    assert Zx.dtype == np.float32 and Zx[0] == np.float32(16777218.0)
    nan = cr.assemble(1, 1, [0, 0], [0, 0], np.array([np.inf, -np.inf]), cr.SUM)[2]
    assert np.isnan(nan[0])


@pytest.mark.parametrize("seed", range(4))
def test_cooref_equals_scipy_and_the_gallery(seed):
    rng = np.random.default_rng(seed)
    m, n, nnz = 37, 29, 900
    rows, cols = rng.integers(0, m, nnz), rng.integers(0, n, nnz)
    vals = rng.integers(-4, 5, nnz).astype(np.float64)
    Zp, Zj, Zx, ent, perm, nkept = cr.assemble(m, n, rows, cols, vals, cr.SUM)
    S = sp.coo_matrix((vals, (rows, cols)), shape=(m, n)).tocsr()     # (sums duplicates, keeps explicit zeros)
    S.sort_indices()
    assert np.array_equal(Zp, S.indptr) and np.array_equal(Zj, S.indices) and np.array_equal(Zx, S.data)
    assert nkept == nnz and ent[0] == 0 and ent[-1] == nkept and np.all(np.diff(ent) > 0)
    assert np.array_equal(np.sort(perm), np.arange(nnz))
    Gp, Gj = gallery._csr_from_pairs(m, n, rows, cols)
    assert np.array_equal(Zp, Gp) and np.array_equal(Zj, Gj)
    assert np.array_equal(cr.values(vals, ent, perm, cr.SUM), Zx)
    assert np.array_equal(cr.raw_lengths(m, n, rows, cols, 0), np.bincount(rows, minlength=m))


def test_cooref_nothing():
    for m, n in ((5, 3), (0, 3), (5, 0)):
        Zp, Zj, Zx, ent, perm, nkept = cr.assemble(m, n, [], [], np.zeros(0), cr.SUM)
        assert Zp.tolist() == [0] * (m + 1) and len(Zj) == len(Zx) == len(perm) == nkept == 0 and ent.tolist() == [0]
    Zp, Zj, Zx, ent, perm, nkept = cr.assemble(5, 3, [-1, 2, -7], [0, -1, -1], np.ones(3), cr.IGNORE_NEGATIVE)
    assert Zp.tolist() == [0] * 6 and nkept == 0 and ent.tolist() == [0]


# ---------------------------------------------------------------- the inputs' roles
def test_bins_input_has_its_roles():
    m, n, rows, cols, vals, shuffle = ai.bins()
    assert m % 64 != 0 and m == len(ai.BIN_LENS)
    lens = cr.raw_lengths(m, n, rows, cols, 0)
    assert lens.tolist() == list(ai.BIN_LENS)
    assert lens[0] == 0 and lens[-1] == 0 and 0 in lens[1:-1].tolist()          # empty rows first, last and in between
    for limit in (ai.SHORT, ai.WAVE, ai.LDS_KEYS):                              # both sides of every limit
        assert limit in lens.tolist() and np.any((lens > limit) & (lens <= limit + 4))
    assert 1 in lens.tolist()
    assert np.sum((lens > 0) & (lens <= ai.SHORT)) == 2 and np.sum((lens > ai.SHORT) & (lens <= ai.WAVE)) == 3
    assert np.sum(lens > ai.WAVE) == 3 and np.sum(lens > ai.LDS_KEYS) == 1      # the rows a bin's kernel meets
    Zp, Zj, Zx, ent, perm, nkept = cr.assemble(m, n, rows, cols, vals, cr.SUM)
    run = np.diff(ent)
    assert np.array_equal(perm, np.arange(len(rows)))                 # generation order is the sorted order
    at = np.concatenate(([0], np.cumsum(lens)))
    for i, L in enumerate(ai.BIN_LENS):
        c = cols[at[i]:at[i + 1]]
        if i == ai.SINGLE_RUN_ROW:
            assert L > ai.SHORT and Zp[i + 1] - Zp[i] == 1 and run[Zp[i]] == L
            continue
        places = ai.pair_places(L)
        assert (L < 2) == (not places)
        for p in places:                                              # a run of two begins at p
            assert c[p] == c[p + 1] and (p == 0 or c[p - 1] != c[p]) and (p + 2 >= L or c[p + 2] != c[p]), (i, p)
        if L > 64:
            assert {0, 15, 63, L - 2} <= set(places)                  # start, 16-lane boundary, wave boundary, end
        assert np.all(np.diff(c) >= 0)
    a, b = ai.TOUCHING
    assert b == a + 1 and cols[at[a + 1] - 1] == cols[at[b]]          # the last column of a row is the first of the next
    assert Zj[Zp[a + 1] - 1] == Zj[Zp[b]] and Zp[b] == Zp[a + 1]      # ... and they stay two entries
    assert np.abs(vals).max() <= 4 and np.abs(Zx).max() < 2 ** 24
    for name, o in ai.orders(len(rows), shuffle).items():
        assert np.array_equal(np.sort(o), np.arange(len(rows))), name
    assert not np.array_equal(shuffle, np.arange(len(rows)))


def test_tiles_inputs_have_scantiles_roles():
    seen = []
    for step, T in enumerate(st.COUNTS):
        m, nkept = ai.tile_sizes(step)
        assert m == T and st.words(nkept) == T
        assert st.role_of(m) == st.ROLES[step] and st.role_of(st.words(nkept)) == st.ROLES[step]
        seen.append(st.role_of(T))
    assert tuple(seen) == st.ROLES
    m, nkept = ai.tile_sizes(st.ROLES.index("several"))
    assert 1_500_000 < nkept < 1_700_000                              # about 1.6 M triplets
    m, n, rows, cols, vals = ai.tiles(st.ROLES.index("one"))
    assert len(rows) == 61 and m == 1 and n == ai.N_TILE_COLS
    m, n, rows, cols, vals = ai.tiles(st.ROLES.index("above"))
    lens = cr.raw_lengths(m, n, rows, cols, 0)
    assert len(lens) == st.SCAN_TILE + 1 and lens.max() > ai.SHORT and lens.min() <= ai.SHORT    # short and wave rows side by side
    assert len(np.unique(rows.astype(np.int64) * n + cols)) < len(rows)                          # duplicates


@pytest.mark.parametrize("num_cu", (64, 256, 304))
def test_long_rows_pass_the_cap(num_cu):
    """k_as_sort_long is the assembly's one kernel with a capped grid (8 workgroups a CU): gridpass' long-row matrix has
    8 numCU + 37 rows beyond 1024 entries, so the block loop turns twice, with a partial second turn"""
    lens = gp.long_lens(num_cu)
    nlong, cap = int(np.sum(lens > gp.LONG)), 8 * num_cu
    assert nlong == cap + gp.EXTRA and nlong > cap and nlong % cap != 0
    assert np.any(lens > gp.LDS_KEYS)
