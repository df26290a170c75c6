"""The shapes of tests/test_scan_tiles_gpu.py, from the references alone (no GPU): every size has the scanned count T it is
listed under, T lies over, on or under the tile multiples in the order the GPU test relies on, the clique patterns give as
many colours and levels as a clique has vertices, and the closed-form colouring of disjoint cliques is gsref.colouring's."""
import numpy as np

import gsref as gr
import scantiles as st


def test_counts_lie_where_they_are_listed():
    assert st.ROLES == ("above", "empty", "one", "exact", "several", "under")
    assert [st.role_of(T) for T in st.COUNTS] == list(st.ROLES)
    # the aggregation and the row-map series of the push product: ceil(n / 64) = T, n a multiple of 64 at the exact size only
    for step, T in enumerate(st.COUNTS):
        n = st.agg_n(step)
        assert st.words(n) == T and (n % 64 == 0) == (T in (0, st.SCAN_TILE)), (step, n)
    assert st.AGG_CASES[-1] == (0, 3) and all(w == 1 for _, w in st.AGG_CASES[:-1])
    for step, w in st.AGG_CASES:
        n, Sp, Sj = st.band(st.agg_n(step), w)
        mean = len(Sj) / max(n, 1)
        assert (mean <= 4.0) if w == 1 else (4.0 < mean <= 16.0), (step, w, mean)
        assert n == 0 or (len(Sp) == n + 1 and Sp[-1] == len(Sj) and 0 <= Sj.min() and Sj.max() < n)


def test_push_cases_reach_both_scans():
    cases = st.push_cases()
    for series in ("frontier", "rowmap"):
        for name in ("min_plus", "or_and"):
            steps = [c for c in cases if c[0] == series and c[4] == name]
            counts = [c[3] if series == "frontier" else st.words(c[2]) for c in steps]
            want = [T for T in st.COUNTS if series == "rowmap" or name == "min_plus" or T <= st.SCAN_TILE + 1]
            assert counts == want, (series, name, counts)
    assert {c[5] for c in cases} == {1, 4}
    # a call whose first scan spans several tiles and whose second spans one, and one the other way round
    assert any(c[3] > 2 * st.SCAN_TILE and st.words(c[2]) <= st.SCAN_TILE for c in cases)
    assert any(c[3] <= st.SCAN_TILE and st.words(c[2]) > 2 * st.SCAN_TILE for c in cases)
    for case in cases:
        (m, n, Gp, Gj, Gx), fidx, F, Y = st.push_inputs(case)
        assert len(fidx) == case[3] and F.shape == (case[3], case[5]) and Y.shape == (n, case[5])
        assert np.diff(Gp).max(initial=0) <= 5 and (case[3] < 4 or len(np.unique(fidx)) < len(fidx))
        assert st.push_scan_rows(case, True) == case[3] + st.words(n) and st.push_scan_rows(case, False) == case[3]


def test_cliques_give_q_colours_and_q_levels():
    assert [st.role_of(st.clique_T(q, c)) for q, c in st.CLIQUES] == list(st.CLIQUE_ROLES)
    assert [st.clique_T(q, c) for q, c in st.CLIQUES] == [8256, 0, 1, 8192, 3 * 8192 + 64, 8128, 8320]
    assert st.CLIQUES[-1][0] * st.CLIQUES[-1][1] % 64 != 0 and max(q for q, _ in st.CLIQUES) <= 70
    for step, (q, c) in enumerate(st.CLIQUES):
        n, Sp, Sj, members, clique_of = st.cliques(q, c)
        assert n == q * c and len(Sj) == n * q
        if n > 64:                                                   # the relabelling mixes cliques inside a 64-vertex word
            assert len(np.unique(clique_of[:64])) > 1
        for which in range(len(st.COLOURINGS)):
            _, (color, ncolors, order, ptr, rounds) = st.colouring(step, which)
            assert ncolors == q == rounds and len(ptr) == q + 1 and np.all(np.diff(ptr) == c)
            assert gr.is_proper(n, Sp, Sj, color)
            assert ncolors * st.words(n) == st.clique_T(q, c)
        for upper in (False, True):
            level, nlevels, order, ptr = st.levels(step, upper)
            assert nlevels == q and nlevels * st.words(n) == st.clique_T(q, c) and np.all(np.diff(ptr) == c)
    assert not np.array_equal(st.colouring(0, 0)[1][0], st.colouring(0, 1)[1][0])


def test_closed_form_colouring_is_the_restatements():
    step = st.CLIQUES.index(st.GREEDY_AT)
    want = st.greedy_colouring()
    got = st.colouring(step, 0)[1]
    assert got[1] == want[1] and got[4] == want[4]
    for a, b in zip((got[0], got[2], got[3]), (want[0], want[2], want[3])):
        assert a.dtype == b.dtype and np.array_equal(a, b)
    # with caller priorities, on a size the restatement does in no time
    n, Sp, Sj, _, _ = st.cliques(5, 40)
    prio = st.priorities(n)
    got, want = st.closed_form_colouring(5, 40, 99, prio), gr.colouring(n, Sp, Sj, 99, prio)
    assert got[1] == want[1] == 5 == got[4] == want[4] and all(np.array_equal(a, b) for a, b in zip(got[:4:2], want[:4:2]))


def test_values_of_the_sweep_and_the_solve_are_exact():
    """the builders assert it as they go: the sweep's result a 24-bit integer over 1024, the restated solve the integer x*"""
    for step in (0, 2, 6):
        Ax, diag, b, x0, want = st.sweep_case(step)
        assert np.array_equal(want, want.astype(np.float32).astype(np.float64))
        Ax, xs, bl, bu = st.solve_case(step)
        assert np.array_equal(bl, np.round(bl)) and np.array_equal(bu, np.round(bu))
