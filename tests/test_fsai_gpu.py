"""bhs_csr_fsai_device on the GPU, both builds, and amg's FSAI-preconditioned CG on top of it.

Reference: tests/fsairef.py, the rule of include/bhsparse_hip.h ("approximate inverse") restated in numpy.  The rule fixes
the order of every operation, so the comparison is of the value bits (fsairef.same_bits: equal bits, NaN in the same
places); on random SPD values the requirement is the backward-error bound of a row (fsairef.row_error_over_bound), with
the bits compared on top.  Every array the call reads carries NaN (or a column that is none) behind its end, valG carries
sentinels behind its nnzG values."""
import functools
import os
import subprocess

import numpy as np
import pytest
import scipy.sparse as sp
import torch

import fsairef as fr
import iluref as ir
from conftest import ROOT
from test_spmv_gpu import bits, new_handle, tdt, up

from benchmark_spgemm_using_csr_amd import _lib, amg

pytestmark = pytest.mark.gpu

DTYPES = (np.float64, np.float32)
INV = _lib.BHS_ERR_INVALID_ARG
SENTINEL = -7.0
PAD = 64
NO_COLUMN = 0x7fffffff


@pytest.fixture(scope="module", params=DTYPES, ids=("f64", "f32"))
def hd(request):
    bh = new_handle(request.param)
    yield bh, request.param
    bh.freePlatform()


def families(bh):
    return {s["name"] for s in bh.kernel_stats() if s["launches"] > 0}


def expected_families(Gp):
    d = np.diff(np.asarray(Gp, np.int64))
    fam = {"fsai_short"}
    if np.any((d > fr.SHORT_D) & (d <= fr.WAVE_D)):
        fam.add("fsai_wave")
    if np.any(d > fr.WAVE_D):
        fam.add("fsai_long")
    return fam


def run(bh, dtype, n, A, G, want=0, flags=0, nnzA=None, nnzG=None, check_families=True):
    """(the device's valG as numpy, bad_row) for host arrays; NaN and columns that are none behind the inputs' ends, the
    sentinels behind valG's nnzG values checked, valG wholly unchanged after a refusal that `want` names as the host's"""
    Ap, Aj, Ax = A
    Gp, Gj = G
    nnzA = len(Aj) if nnzA is None else nnzA
    nnzG = len(Gj) if nnzG is None else nnzG
    t = tdt(dtype)
    dAp, dGp = up(Ap, np.int32), up(Gp, np.int32)
    dAj = up(np.concatenate([Aj, np.full(PAD, NO_COLUMN)]), np.int32)
    dGj = up(np.concatenate([Gj, np.full(PAD, NO_COLUMN)]), np.int32)
    dAx = torch.cat([up(Ax, dtype), torch.full((PAD,), float("nan"), dtype=t).cuda()])
    dG = torch.cat([torch.full((max(nnzG, 0),), float("nan"), dtype=t).cuda(), torch.full((PAD,), SENTINEL, dtype=t).cuda()])
    torch.cuda.synchronize()
    err = amg.fsai_raw_device(bh, n, nnzA, dAp, dAj, dAx, nnzG, dGp, dGj, dG, flags)
    assert err == want, (err, want)
    assert bool((dG[max(nnzG, 0):] == SENTINEL).all()), "written past nnzG"
    if want:
        return None, None
    assert bh.fsai_ms >= 0.0
    if check_families and n > 0:
        assert families(bh) == expected_families(Gp), (families(bh), expected_families(Gp))
    return dG[:nnzG].cpu().numpy(), bh.fsai_bad_row


def agree(got, ref, what):
    assert fr.same_bits(got, ref), (what, np.argwhere(bits(np.nan_to_num(got)) != bits(np.nan_to_num(ref)))[:5].ravel())


@functools.lru_cache(maxsize=None)
def exact_reference(dtype):
    n, Ap, Aj, Ax, Gp, Gj, _ = fr.exact_family()
    return fr.fsai(n, Ap, Aj, Ax, Gp, Gj, dtype)


@functools.lru_cache(maxsize=None)
def random_reference(power, dtype):
    n, Ap, Aj, Ax = fr.random_spd()
    Gp, Gj = fr.tril_pattern(n, Ap, Aj, power)
    return (Gp, Gj) + fr.fsai(n, Ap, Aj, Ax, Gp, Gj, dtype, keep=True)


# ---------------------------------------------------------------- 1. the exact family, bit for bit
def test_exact_family_in_every_bin(hd):
    bh, dtype = hd
    n, Ap, Aj, Ax, Gp, Gj, _ = fr.exact_family()
    ref, ref_bad = exact_reference(dtype)
    got, bad = run(bh, dtype, n, (Ap, Aj, Ax), (Gp, Gj))
    assert families(bh) == {"fsai_short", "fsai_wave", "fsai_long"}
    assert bad == ref_bad == -1 and np.all(np.isfinite(ref))
    agree(got, ref, "exact family")
    launches = {s["name"]: (s["launches"], s["rows"]) for s in bh.kernel_stats() if s["launches"] > 0}
    d = np.diff(Gp)
    assert launches == {"fsai_short": (1, n), "fsai_wave": (1, int(((d > 16) & (d <= 64)).sum())), "fsai_long": (1, int((d > 64).sum()))}


def test_short_rows_over_many_workgroups_and_the_default_pattern(hd):
    bh, dtype = hd
    n, Ap, Aj, Ax = fr.grid("poisson5pt_33")
    Gp, Gj = fr.tril_pattern(n, Ap, Aj)
    ref, _ = fr.fsai(n, Ap, Aj, Ax, Gp, Gj, dtype)
    got, bad = run(bh, dtype, n, (Ap, Aj, Ax), (Gp, Gj))
    assert bad == -1 and families(bh) == {"fsai_short"}
    agree(got, ref, "poisson5pt_33")
    # the tensor call: its default pattern is tril(A), made by the selection
    A = (up(Ap, np.int32), up(Aj, np.int32), up(Ax, dtype))
    dGp, dGj, dGx = amg.fsai_device(bh, A)
    assert np.array_equal(dGp.cpu().numpy(), Gp) and np.array_equal(dGj.cpu().numpy(), Gj) and dGx.dtype == tdt(dtype)
    agree(dGx.cpu().numpy(), ref, "fsai_device")
    assert bh.fsai_bad_row == -1 and bh.fsai_ms >= 0.0
    M = amg.fsai_setup_device(bh, A, (dGp, dGj))
    Gm = fr.fsai_matrix(n, Gp, Gj, ref.astype(np.float64)).T.tocsr()
    Gm.sort_indices()
    assert M["bad_row"] == -1 and np.array_equal(M["Gt"][1].cpu().numpy(), Gm.indices)
    assert np.array_equal(M["Gt"][2].cpu().numpy(), Gm.data.astype(dtype))


# ---------------------------------------------------------------- 2. random SPD values: the bound, then the bits
@pytest.mark.parametrize("power", (1, 2), ids=("tril(A)", "tril(A^2)"))
def test_random_spd_values_within_the_backward_error_bound(hd, power):
    """componentwise in np.longdouble, |M g - e_d / g_d| <= (2 d + 3) 2^-53 (|L| |L^T| |g|) + 2^-53 |1 / g_d| e_d, L the
    restatement's; the float build adds 2^-24 (|M| |g| + |1 / g_d| e_d) for its final rounding"""
    bh, dtype = hd
    n, Ap, Aj, Ax = fr.random_spd()
    Gp, Gj, ref, ref_bad, kept = random_reference(power, dtype)
    got, bad = run(bh, dtype, n, (Ap, Aj, Ax), (Gp, Gj))
    assert bad == ref_bad == -1 and np.all(np.isfinite(got))
    worst = fr.worst_error_over_bound(Gp, got, kept, dtype)
    ulps = fr.ulp_distance(got, ref)
    print("random SPD tril(A^%d) %s: worst error / bound %.3f, %d ulp from the restatement" % (power, np.dtype(dtype).name, worst, ulps))
    assert worst <= 1.0
    agree(got, ref, ("random SPD", power))


# ---------------------------------------------------------------- 3. patterns outside A's
def test_patterns_outside_the_pattern_of_a(hd):
    bh, dtype = hd
    n, Ap, Aj, Ax, Gp, Gj, _ = fr.exact_family()
    Ep, Ej = fr.with_extra_lower(n, Gp, Gj, seed=11)
    assert len(Ej) > len(Gj) and np.diff(Ep).max() == fr.MAX_ROW
    ref, ref_bad = fr.fsai(n, Ap, Aj, Ax, Ep, Ej, dtype)
    got, bad = run(bh, dtype, n, (Ap, Aj, Ax), (Ep, Ej))
    assert bad == ref_bad
    agree(got, ref, "extra lower entries")
    # the diagonal alone: 1 / sqrt(a_ii) by the contract's two operations
    dp, dj = np.arange(n + 1, dtype=np.int32), np.arange(n, dtype=np.int32)
    got, bad = run(bh, dtype, n, (Ap, Aj, Ax), (dp, dj))
    a = fr.csr(n, Ap, Aj, Ax).diagonal().astype(dtype).astype(np.float64)
    assert bad == -1 and np.array_equal(got, (1.0 / np.sqrt(a)).astype(dtype))
    agree(got, fr.fsai(n, Ap, Aj, Ax, dp, dj, dtype)[0], "the diagonal alone")
    # tril(A) in place of A: entries beyond the diagonal are never used
    T = sp.tril(fr.csr(n, Ap, Aj, Ax)).tocsr()
    T.sort_indices()
    got, _ = run(bh, dtype, n, (T.indptr, T.indices, T.data), (Gp, Gj))
    agree(got, exact_reference(dtype)[0], "tril(A) as A")


# ---------------------------------------------------------------- 4. pivots
@pytest.mark.parametrize("case", ("negated", "zero"))
def test_bad_pivots_are_reported_and_stay_in_their_blocks(hd, case):
    bh, dtype = hd
    n, Ap, Aj, Ax, Gp, Gj, starts = fr.exact_family()
    r = np.repeat(np.arange(n), np.diff(Ap))
    x = Ax.copy()
    if case == "negated":
        hit = {4: starts[4] + 9, 8: starts[8] + 100}                # in the blocks of order 17 and 127
        for at in hit.values():
            x[(r == at) & (Aj == at)] *= -1
    else:
        hit = {6: starts[6]}                                        # the first pivot of the block of order 64: a root of 0,
        x[(r == hit[6]) & (Aj == hit[6])] = 0.0                     # divisions by it
    ref, ref_bad = fr.fsai(n, Ap, Aj, x, Gp, Gj, dtype)
    assert ref_bad == min(hit.values())
    got, bad = run(bh, dtype, n, (Ap, Aj, x), (Gp, Gj))
    assert bad == ref_bad
    agree(got, ref, case)
    clean = exact_reference(dtype)[0]
    rows = np.ones(n, bool)
    for b in hit:
        rows[starts[b]:starts[b] + fr.BLOCKS[b]] = False
    keep = np.repeat(rows, np.diff(Gp))
    assert np.array_equal(bits(got[keep]), bits(clean[keep])) and not np.array_equal(bits(got[~keep]), bits(clean[~keep]))


# ---------------------------------------------------------------- 5. refusals
def bad_inputs():
    """(word, Ap, Aj, Gp, Gj, nnzA, nnzG) for every refusal of the device, on poisson5pt_33 with tril(A) as G"""
    n, Ap, Aj, Ax = fr.grid("poisson5pt_33")
    Gp, Gj = fr.tril_pattern(n, Ap, Aj)
    out = []

    def rebuilt(i, cols):
        """G with row i replaced by cols"""
        j = np.concatenate([Gj[:Gp[i]], cols, Gj[Gp[i + 1]:]]).astype(np.int32)
        p = Gp.copy()
        p[i + 1:] += len(cols) - (Gp[i + 1] - Gp[i])
        return p, j

    for word, i, cols in (("empty row of G", 500, []), ("row of G not ascending", 500, [499, 467, 500]),
                          ("row of G not ascending", 500, [467, 467, 500]), ("column of G outside [0, i]", 500, [467, 499, 501]),
                          ("column of G outside [0, i]", 500, [-1, 499, 500]), ("row of G does not end in i", 500, [467, 499]),
                          ("row of G longer than 128", 500, list(range(372, 501))), ("row of G longer than 128", 1088, list(range(100, 1089)))):
        p, j = rebuilt(i, cols)
        out.append((word, Ap, Aj, p, j, len(Aj), len(j)))
    p = Gp.copy(); p[0] = 1
    out.append(("rowPtrG", Ap, Aj, p, Gj, len(Aj), len(Gj)))
    out.append(("rowPtrG", Ap, Aj, Gp, np.concatenate([Gj, [0]]).astype(np.int32), len(Aj), len(Gj) + 1))
    p = Gp.copy(); p[600], p[601] = Gp[601], Gp[600]
    out.append(("rowPtrG", Ap, Aj, p, Gj, len(Aj), len(Gj)))
    p = Ap.copy(); p[700] = len(Aj) + 5
    out.append(("rowPtrA", p, Aj, Gp, Gj, len(Aj), len(Gj)))
    p = Ap.copy(); p[700], p[701] = Ap[701], Ap[700]
    out.append(("rowPtrA", p, Aj, Gp, Gj, len(Aj), len(Gj)))
    j = Aj.copy(); a = Ap[800]; j[a], j[a + 1] = Aj[a + 1], Aj[a]     # two columns below the diagonal of row 800
    assert Aj[a + 1] < 800
    out.append(("row of A not ascending", Ap, j, Gp, Gj, len(Aj), len(Gj)))
    j = Aj.copy(); j[Ap[800]] = -3
    out.append(("column of A out of range", Ap, j, Gp, Gj, len(Aj), len(Gj)))
    return n, (Ap, Aj, Ax), (Gp, Gj), out


def test_the_device_refuses_bad_inputs_and_writes_nothing_outside(hd):
    bh, dtype = hd
    n, A, G, cases = bad_inputs()
    assert {w for w, *_ in cases} == set(fr.DEVICE_REFUSALS)
    for word, Ap, Aj, Gp, Gj, nnzA, nnzG in cases:
        assert fr.invalid(n, Ap, Aj, Gp, Gj, nnzA=nnzA, nnzG=nnzG) == word, word
        run(bh, dtype, n, (Ap, Aj, A[2]), (Gp, Gj), want=INV, nnzA=nnzA, nnzG=nnzG)   # (run checks the guards behind nnzG)
    # a disorder behind the diagonal of a row of A is not looked at, and the handle still answers
    Ap, Aj, Ax = A
    j = Aj.copy()
    e = Ap[401] - 1
    assert Aj[e - 1] > 400
    j[e], j[e - 1] = Aj[e - 1], Aj[e]
    ref, _ = fr.fsai(n, Ap, Aj, Ax, G[0], G[1], dtype)
    got, bad = run(bh, dtype, n, (Ap, j, Ax), G)
    assert bad == -1
    agree(got, ref, "after the refusals")


def test_host_side_refusals_leave_valg_untouched(hd):
    bh, dtype = hd
    n, (Ap, Aj, Ax), (Gp, Gj), _ = bad_inputs()
    nnzA, nnzG = len(Aj), len(Gj)
    t = tdt(dtype)
    dAp, dAj, dAx, dGp, dGj = up(Ap, np.int32), up(Aj, np.int32), up(Ax, dtype), up(Gp, np.int32), up(Gj, np.int32)
    Z = torch.full((nnzA + nnzG + PAD,), SENTINEL, dtype=t).cuda()
    torch.cuda.synchronize()

    def call(n=n, nnzA=nnzA, Ap=dAp, Aj=dAj, Ax=dAx, nnzG=nnzG, Gp=dGp, Gj=dGj, G=Z, flags=0):
        return amg.fsai_raw_device(bh, n, nnzA, Ap, Aj, Ax, nnzG, Gp, Gj, G, flags)

    refused = {
        "negative size": (call(n=-1), call(nnzA=-1), call(nnzG=-1)),
        "flags != 0": (call(flags=1), call(flags=2), call(flags=-1)),
        "NULL array": (call(Ap=None), call(Aj=None), call(Ax=None), call(Gp=None), call(Gj=None), call(G=None)),
        "nnzG < n": (call(nnzG=n - 1),),
        "valG overlaps an input": (call(G=dAx), call(G=dAx[nnzA - 1:]), call(Ax=Z[nnzG - 1:]), call(Gj=Z.view(torch.int32)),
                                   call(G=dGj.view(t)) if dtype == np.float32 else call(Gj=Z[1:].view(torch.int32)),
                                   call(Ap=Z.view(torch.int32)), call(Gp=Z.view(torch.int32)), call(Aj=Z.view(torch.int32))),
    }
    assert sorted(refused) == sorted(fr.HOST_REFUSALS)
    for word, codes in refused.items():
        assert all(c == INV for c in codes), (word, codes)
    assert bool((Z == SENTINEL).all()), "valG written by a refused call"
    assert np.array_equal(dAx.cpu().numpy(), Ax.astype(dtype))
    # n == 0 succeeds, launches nothing and writes nothing
    assert call(n=0, nnzA=0, nnzG=0) == 0 and bh.fsai_bad_row == -1 and bh.fsai_ms == 0.0
    assert call(n=0, nnzA=0, nnzG=0, Ap=None, Aj=None, Ax=None, Gp=None, Gj=None, G=None) == 0
    assert bool((Z == SENTINEL).all())


def test_refused_between_symbolic_and_finish():
    n, A, G, _ = bad_inputs()
    k = 50
    sq = (np.arange(k + 1), np.arange(k), np.ones(k))                # the identity, as A and B of a multiply
    dA = (up(sq[0], np.int32), up(sq[1], np.int32), up(sq[2], np.float64))
    bh = new_handle()
    try:
        assert bh.initData_device(k, k, k, k, dA[2], dA[0], dA[1], k, dA[2], dA[0], dA[1]) == 0
        assert bh.spgemm_symbolic() == 0
        run(bh, np.float64, n, A, G, want=INV)
        assert bh.spgemm_numeric(0, k) == 0 and bh.spgemm_finish() == 0
        got, _ = run(bh, np.float64, n, A, G, check_families=False)
        agree(got, fr.fsai(n, *A, *G)[0], "after finish")
        bh.free_mem()
    finally:
        bh.freePlatform()


# ---------------------------------------------------------------- 6. repeatability
def test_two_calls_two_handles_and_a_multiply_between_give_the_same_bits(hd):
    from helpers import random_csr
    bh, dtype = hd
    n, Ap, Aj, Ax = fr.random_spd()
    Gp, Gj = random_reference(2, dtype)[:2]
    first, _ = run(bh, dtype, n, (Ap, Aj, Ax), (Gp, Gj))
    again, _ = run(bh, dtype, n, (Ap, Aj, Ax), (Gp, Gj))
    other = new_handle(dtype)
    try:
        third, _ = run(other, dtype, n, (Ap, Aj, Ax), (Gp, Gj))
        mm = 300
        Bp, Bj, Bx = random_csr(mm, mm, 0.03, np.random.default_rng(31))
        Bp, Bj, Bx = np.ascontiguousarray(Bp, np.int32), np.ascontiguousarray(Bj, np.int32), np.ascontiguousarray(Bx, dtype)
        Cp = np.zeros(mm + 1, np.int32)
        assert other.initData(mm, mm, mm, len(Bj), Bx, Bp, Bj, len(Bj), Bx, Bp, Bj, Cp) == 0 and other.spgemm() == 0
        nnzC = other.get_nnzC()
        fourth, _ = run(other, dtype, n, (Ap, Aj, Ax), (Gp, Gj), check_families=False)
        assert other.get_nnzC() == nnzC > 0                         # the multiply's result stays
        other.free_mem()
    finally:
        other.freePlatform()
    for what, arr in (("again", again), ("another handle", third), ("after a multiply", fourth)):
        assert np.array_equal(bits(first), bits(arr)), what


# ---------------------------------------------------------------- 7. FSAI-PCG
@pytest.mark.parametrize("name", ("poisson27pt_9", "poisson5pt_33"))
def test_fsai_pcg_and_ilu_pcg_beside_it(name):
    """1e-8 relative residual in double: the restatement's iterations +- 1 (the margin test_trsv_gpu gives ILU-PCG), fewer
    than the restatement's Jacobi-PCG; ilu0_pcg_device, whose loop FSAI-PCG shares, still agrees with its restatement"""
    n, Ap, Aj, Ax = fr.grid(name)
    Amat = fr.csr(n, Ap, Aj, Ax)
    b = np.random.default_rng(0).standard_normal(n)
    A = (up(Ap, np.int32), up(Aj, np.int32), up(Ax, np.float64))
    db = up(b, np.float64)
    _, want, _ = fr.fsai_pcg(Amat, b, 1e-8, 100)
    _, jac, _ = fr.jacobi_pcg(Amat, b, 1e-8, 300)
    bh = new_handle()
    try:
        x, its, res = amg.fsai_pcg_device(bh, A, db, 1e-8, 100)
        print("%s: FSAI-PCG %d iterations, the restatement %d, Jacobi-PCG %d" % (name, its, want, jac))
        assert abs(its - want) <= 1 and len(res) == its + 1 and res[-1] <= 1e-8 * res[0]
        assert np.linalg.norm(b - Amat @ x.cpu().numpy()) <= 1.01e-8 * np.linalg.norm(b)
        assert its < jac
        # a caller's pattern: tril(A^2) needs no more iterations than tril(A)
        Gp, Gj = fr.tril_pattern(n, Ap, Aj, 2)
        _, want2, _ = fr.fsai_pcg(Amat, b, 1e-8, 100, (Gp, Gj))
        _, its2, res2 = amg.fsai_pcg_device(bh, A, db, 1e-8, 100, (up(Gp, np.int32), up(Gj, np.int32)))
        print("%s: FSAI-PCG on tril(A^2) %d iterations, the restatement %d" % (name, its2, want2))
        assert abs(its2 - want2) <= 1 and its2 <= its and res2[-1] <= 1e-8 * res2[0]
        for ordering in ("natural", "colour") if name == "poisson27pt_9" else ("natural",):
            _, want, _ = ir.ilu0_pcg(Amat, b, 1e-8, 100, ordering)
            x, its, res = amg.ilu0_pcg_device(bh, A, db, 1e-8, 100, ordering)
            print("%s ILU-PCG %s: %d iterations, the restatement %d" % (name, ordering, its, want))
            assert abs(its - want) <= 1 and len(res) == its + 1 and res[-1] <= 1e-8 * res[0]
            assert np.linalg.norm(b - Amat @ x.cpu().numpy()) <= 1.01e-8 * np.linalg.norm(b)
    finally:
        bh.freePlatform()


# ---------------------------------------------------------------- 8. the demo
def test_cpp_demo_runs():
    demo_dir = os.path.join(ROOT, "tests", "fsai")
    subprocess.check_call(["make", "-C", demo_dir, "-s"])
    out = subprocess.run([os.path.join(demo_dir, "fsai_demo")], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "fsai 48 rows, 798 entries of G, rows of up to 21: PASS" in out.stdout
