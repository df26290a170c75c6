"""The assembly from triplets (bhs_coo_assemble_device, bhs_coo_assemble_values_device) on the GPU, both builds.

Reference: tests/cooref.py, include/bhsparse_hip.h's "assembly" restated in numpy with the sums as a loop.  Every output is
a function of the input alone, so rowPtrZ, colIndZ, entryPtr, perm and the values' bit patterns are compared bit for bit
(NaNs by class); behind every capacity lie guard words that must stay, and what lies between what a call writes (nnzZ,
nnzZ + 1, nkept) and the capacity must stay as well.  The inputs and the roles they play -- the bins' limits, the scan's
tiles, the capped grid of the long-row sort, the one kernel of the family that caps its grid -- are tests/asminputs.py's,
asserted on the CPU by tests/test_assemble_shapes.py.  Every refusal here is an invalid ARGUMENT the contract refuses
cleanly."""
import os
import subprocess

import numpy as np
import pytest
import scipy.sparse as sp
import torch

from conftest import ROOT
import asminputs as ai
import cooref as cr
import gridpass as gp
import helpers
import scantiles as st

from benchmark_spgemm_using_csr_amd import _lib, amg, assemble as asm, gallery, graph
from benchmark_spgemm_using_csr_amd.facade import BHSPARSE_HIP, NUM_PLATFORMS, BhsparseError, bhsparse

pytestmark = pytest.mark.gpu

BUILDS = {"f64": np.float64, "f32": np.float32}
INV = _lib.BHS_ERR_INVALID_ARG
GUARD = 16
SENT = -7
SUM, FIRST, LAST, KEEP, IGN = cr.SUM, cr.FIRST, cr.LAST, cr.KEEP, cr.IGNORE_NEGATIVE


# ---------------------------------------------------------------- helpers
def new_handle(dtype=np.float64, options=None):
    plats = [False] * NUM_PLATFORMS
    plats[BHSPARSE_HIP] = True
    bh = bhsparse(value_dtype=dtype)
    assert bh.initPlatform(plats) == 0
    for key, val in (options or {}).items():
        assert bh.set_option(key, val) == 0, key
    return bh


@pytest.fixture(scope="module", params=sorted(BUILDS))
def hd(request):
    dtype = BUILDS[request.param]
    bh = new_handle(dtype)
    yield bh, dtype, request.param
    bh.freePlatform()


def num_cu():
    return torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count


def bits(x):
    x = np.ascontiguousarray(x)
    return x.view(np.uint64 if x.dtype == np.float64 else np.uint32)


def same_values(got, want):
    """bit for bit; NaNs by class"""
    got, want = np.asarray(got), np.asarray(want)
    if got.dtype != want.dtype or got.shape != want.shape:
        return False
    nan = np.isnan(want)
    return np.array_equal(np.isnan(got), nan) and np.array_equal(bits(got)[~nan], bits(want)[~nan])


def up(a, dt):
    """on the device; for an empty array one element of room, so that its pointer is not null (the calls take the count)"""
    a = np.ascontiguousarray(a, dt)
    return torch.from_numpy(a.copy() if a.size else np.zeros(1, dt)).cuda()


def typed(ref, dtype):
    """a reference made once in double on small integers (every sum below 2^24: exact in both types) for this build"""
    assert np.abs(ref[2]).max(initial=0) < 2 ** 24 and np.array_equal(ref[2], np.round(ref[2]))
    return ref[:2] + (ref[2].astype(dtype),) + ref[3:]


def tdt(dtype):
    return torch.float32 if np.dtype(dtype) == np.dtype(np.float32) else torch.float64


def stats(bh):
    return {s["name"]: s for s in bh.kernel_stats() if s["launches"] > 0}


class Outputs(object):
    """the five output arrays filled with the sentinel, GUARD words behind every capacity"""

    def __init__(self, dtype, m, nnz, val=True, ent=True, perm=True):
        self.m, self.nnz = m, nnz
        self.Zp = torch.full((m + 1 + GUARD,), SENT, dtype=torch.int32).cuda()
        self.Zj = torch.full((nnz + GUARD,), SENT, dtype=torch.int32).cuda()
        self.Zx = torch.full((nnz + GUARD,), float(SENT), dtype=tdt(dtype)).cuda() if val else None
        self.ent = torch.full((nnz + 1 + GUARD,), SENT, dtype=torch.int32).cuda() if ent else None
        self.pm = torch.full((nnz + GUARD,), SENT, dtype=torch.int32).cuda() if perm else None
        torch.cuda.synchronize()

    def untouched_from(self, zp, zj, ent, pm):
        for a, k in ((self.Zp, zp), (self.Zj, zj), (self.Zx, zj), (self.ent, ent), (self.pm, pm)):
            if a is not None and not bool((a[k:] == SENT).all()):
                return False
        return True


def raw(bh, dtype, m, n, rows, cols, vals, flags, out):
    nnz = len(rows)
    torch.cuda.synchronize()
    return asm.coo_assemble_raw_device(bh, m, n, nnz, up(rows, np.int32), up(cols, np.int32),
                                       None if vals is None else up(vals, dtype), flags, out.Zp, out.Zj, out.Zx, out.ent, out.pm)


def expected_families(lens, nnz, values):
    if nnz == 0:
        return set()
    if lens.sum() == 0:
        return {"assemble_count"}
    fam = {"assemble_count", "assemble_scan", "assemble_scatter", "assemble_dedupe"}
    if np.any((lens >= 1) & (lens <= ai.SHORT)):
        fam.add("assemble_short")
    if np.any((lens > ai.SHORT) & (lens <= ai.WAVE)):
        fam.add("assemble_wave")
    if np.any(lens > ai.WAVE):
        fam.add("assemble_long")
    if values:
        fam.add("assemble_values")
    return fam


def check(bh, dtype, m, n, rows, cols, vals, flags, what, val=True, ent=True, perm=True, ref=None):
    """one full call against cooref: everything it returns and writes, and nothing else.  Returns (reference, Outputs)."""
    vals = None if vals is None else np.ascontiguousarray(vals, dtype)
    ref = ref or cr.assemble(m, n, rows, cols, vals, flags)
    Zp, Zj, Zx, rent, rperm, nkept = ref
    out = Outputs(dtype, m, len(rows), val and vals is not None, ent, perm)
    err = raw(bh, dtype, m, n, rows, cols, vals, flags, out)
    assert err == 0, (what, err)
    nz = len(Zj)
    assert (bh.assemble_nnz, bh.assemble_nkept) == (nz, nkept), (what, bh.assemble_nnz, bh.assemble_nkept, nz, nkept)
    assert out.untouched_from(m + 1, nz, nz + 1, nkept), (what, "written beyond what the call returns")
    assert np.array_equal(out.Zp[:m + 1].cpu().numpy(), Zp), (what, "rowPtrZ differs")
    assert np.array_equal(out.Zj[:nz].cpu().numpy(), Zj), (what, "colIndZ differs")
    if ent:
        assert np.array_equal(out.ent[:nz + 1].cpu().numpy(), rent), (what, "entryPtr differs")
    if perm:
        assert np.array_equal(out.pm[:nkept].cpu().numpy(), rperm), (what, "perm differs")
    if out.Zx is not None:
        assert same_values(out.Zx[:nz].cpu().numpy(), Zx), (what, "valZ differs")
    lens = cr.raw_lengths(m, n, rows, cols, flags)
    fam = set(stats(bh))
    assert fam == expected_families(lens, len(rows), out.Zx is not None), (what, fam)
    assert bh.assemble_ms >= 0.0
    return ref, out


# ---------------------------------------------------------------- 1. nothing
def test_nothing(hd):
    bh, dtype, build = hd
    none = np.zeros(0, np.int32)
    for m, n in ((5, 3), (0, 3), (5, 0), (0, 0)):
        check(bh, dtype, m, n, none, none, np.zeros(0), SUM, "nnzIn = 0, %d x %d" % (m, n))
    rows, cols = np.array([-1, 2, -7, -1], np.int32), np.array([0, -1, -1, 2], np.int32)
    ref, out = check(bh, dtype, 5, 3, rows, cols, np.ones(4), SUM | IGN, "all negative")
    assert ref[5] == 0 and ref[0].tolist() == [0] * 6 and out.ent[0].item() == 0


# ---------------------------------------------------------------- 2. the bins
@pytest.mark.parametrize("order", ("shuffled", "sorted", "reversed"))
def test_bins(hd, order):
    bh, dtype, build = hd
    m, n, rows, cols, vals, shuffle = ai.bins()
    o = ai.orders(len(rows), shuffle)[order]
    ref, _ = check(bh, dtype, m, n, rows[o], cols[o], vals[o], SUM, "bins " + order)
    got = stats(bh)
    assert {"assemble_short", "assemble_wave", "assemble_long"} <= set(got)
    assert (got["assemble_short"]["rows"], got["assemble_wave"]["rows"], got["assemble_long"]["rows"]) == (2, 3, 3)
    # the same matrix whatever the order the triplets came in; under FIRST and LAST the order shows
    base = st.cached("asm bins ref", lambda: cr.assemble(m, n, rows, cols, vals, SUM))
    assert np.array_equal(ref[0], base[0]) and np.array_equal(ref[1], base[1]) and np.array_equal(ref[2], base[2].astype(dtype))
    check(bh, dtype, m, n, rows[o], cols[o], vals[o], LAST, "bins LAST " + order)


# ---------------------------------------------------------------- 3. one run only
def test_one_run_longer_than_the_lds_keys(hd):
    bh, dtype, build = hd
    k = 5000
    assert k > ai.LDS_KEYS
    ref, out = check(bh, dtype, 5, 9, np.full(k, 3, np.int32), np.full(k, 7, np.int32), np.ones(k), SUM, "one run")
    assert bh.assemble_nnz == 1 and out.Zx[0].item() == 5000.0 and out.Zp[:6].tolist() == [0, 0, 0, 0, 1, 1]
    assert out.pm[:k].cpu().tolist() == list(range(k))
    assert stats(bh)["assemble_long"]["rows"] == 1


# ---------------------------------------------------------------- 4. the scan's tiles, one handle
def test_one_handle_through_the_scan_sizes(hd):
    bh, dtype, build = hd
    for step, role in enumerate(st.ROLES):                            # above, empty, one, exact, several, under
        m, n, rows, cols, vals = ai.tiles(step)
        ref = st.cached(("asm tiles ref", step), lambda: cr.assemble(m, n, rows, cols, vals, SUM), "assembly")
        check(bh, dtype, m, n, rows, cols, vals, SUM, "tiles " + role, ref=typed(ref, dtype))
        got = stats(bh)
        if len(rows):
            assert got["assemble_scan"]["launches"] == 2
            assert got["assemble_scan"]["rows"] == m + st.words(len(rows)), (role, got["assemble_scan"])
        print("%s tiles %s: m = %d, %d triplets, %d entries, %.3f ms" % (build, role, m, len(rows), bh.assemble_nnz, bh.assemble_ms))


# ---------------------------------------------------------------- 5. the capped grid
def test_long_rows_past_the_cap(hd):
    """k_as_sort_long is the family's one kernel with a capped grid (8 workgroups a CU; every flat kernel takes one lane an
    element and as many workgroups as that needs -- 1.57 M triplets in the test above): 8 numCU + 37 raw rows beyond 1024
    triplets, about every 200th beyond the keys a workgroup holds in LDS"""
    bh, dtype, build = hd
    m, n, (Ap, Aj, Ax) = gp.long_rows(num_cu())
    rows, cols, vals = st.cached(("asm long", num_cu()), lambda: ai.csr_triplets(Ap, Aj, Ax, 77))
    nlong, cap = int(np.sum(np.diff(Ap) > gp.LONG)), 8 * num_cu()
    assert nlong > cap and nlong % cap != 0
    ref = st.cached(("asm long ref", num_cu()), lambda: cr.assemble(m, n, rows, cols, vals, SUM), "assembly")
    check(bh, dtype, m, n, rows, cols, vals, SUM, "long rows", ref=typed(ref, dtype))
    got = stats(bh)["assemble_long"]
    assert got["rows"] == nlong and got["launches"] == 1
    print("%s long rows: %d rows over a grid of %d; %d triplets in %.3f ms" % (build, nlong, cap, len(rows), bh.assemble_ms))


# ---------------------------------------------------------------- 6. the flags
def flag_input():
    def make():
        rng = np.random.default_rng(606)
        m, n, nnz = 70, 50, 6000
        rows, cols = rng.integers(0, m, nnz).astype(np.int32), rng.integers(0, n, nnz).astype(np.int32)
        rows[rng.random(nnz) < 0.3] = 11                              # a long row among wave rows
        return m, n, rows, cols, rng.integers(-4, 5, nnz).astype(np.float64)
    return st.cached("asm flags", make)


def test_what_happens_to_duplicates(hd):
    bh, dtype, build = hd
    m, n, rows, cols, vals = flag_input()
    seen = {}
    for name, flags in (("SUM", SUM), ("FIRST", FIRST), ("LAST", LAST), ("KEEP", KEEP)):
        ref, _ = check(bh, dtype, m, n, rows, cols, vals, flags, name)
        seen[name] = ref
    assert len(seen["KEEP"][1]) == len(rows) and seen["KEEP"][3].tolist() == list(range(len(rows) + 1))
    assert len(seen["SUM"][1]) < len(rows) and not np.array_equal(seen["FIRST"][2], seen["LAST"][2])
    assert not np.array_equal(seen["SUM"][2], seen["FIRST"][2])


@pytest.mark.parametrize("where", ("row", "column", "both"))
def test_ignore_negative(hd, where):
    bh, dtype, build = hd
    m, n, rows, cols, vals = flag_input()
    rows, cols = rows.copy(), cols.copy()
    hit = np.random.default_rng(607).random(len(rows)) < 0.2
    hit[0] = hit[-1] = True
    if where in ("row", "both"):
        rows[hit] = -1 - rows[hit]
    if where in ("column", "both"):
        cols[hit] = -3
    for flags in (SUM | IGN, KEEP | IGN):
        ref, out = check(bh, dtype, m, n, rows, cols, vals, flags, "negative " + where)
        nkept = bh.assemble_nkept
        assert nkept == int(np.sum(~hit))
        named = out.pm[:nkept].cpu().numpy()
        assert not np.any(hit[named]) and len(np.unique(named)) == nkept       # perm names kept positions only, each once
    out = Outputs(dtype, m, len(rows))
    assert raw(bh, dtype, m, n, rows, cols, vals, SUM, out) == INV and out.untouched_from(0, 0, 0, 0)


def test_pattern_only_and_optional_outputs(hd):
    bh, dtype, build = hd
    m, n, rows, cols, vals = flag_input()
    ref, _ = check(bh, dtype, m, n, rows, cols, None, SUM, "pattern only")
    assert ref[2] is None
    check(bh, dtype, m, n, rows, cols, vals, SUM, "no valZ", val=False)
    check(bh, dtype, m, n, rows, cols, vals, SUM, "no entryPtr", ent=False)
    check(bh, dtype, m, n, rows, cols, vals, LAST, "no perm", perm=False)
    check(bh, dtype, m, n, rows, cols, vals, SUM, "pattern and nothing else", val=False, ent=False, perm=False)


# ---------------------------------------------------------------- 7. real and special values
def special_input(dtype):
    rng = np.random.default_rng(707)
    m, n = 40, 64
    runs = rng.integers(1, 10, 900)                                   # runs of 1 to 9
    pair = rng.choice(m * n, len(runs), replace=False)
    key = np.repeat(pair, runs)
    count = len(key)
    p, j = np.array([0, count], np.int32), np.zeros(count, np.int32)
    _, (_, _, vals), _ = helpers.real_values("wide", 1, (p, j, None), (np.zeros(2, np.int32), np.zeros(0, np.int32), None), rng)
    vals = vals.astype(dtype)                                         # the float build's inputs ARE floats
    pick = rng.random(count)
    for lo, v in ((0.00, np.nan), (0.04, np.inf), (0.08, -np.inf), (0.12, 0.0), (0.18, -0.0)):
        vals[(pick >= lo) & (pick < lo + 0.04)] = v
    lone = np.flatnonzero(runs == 1)[:5]
    vals[np.concatenate(([0], np.cumsum(runs)))[lone]] = -0.0         # five lone -0
    o = rng.permutation(count)
    return m, n, (key // n).astype(np.int32)[o], (key % n).astype(np.int32)[o], vals[o], [divmod(int(pair[i]), n) for i in lone]


def test_real_and_special_values(hd):
    bh, dtype, build = hd
    m, n, rows, cols, vals, lone = special_input(dtype)
    assert vals.dtype == np.dtype(dtype) and np.isnan(vals).any() and np.isinf(vals).any() and np.signbit(vals[vals == 0]).any()
    for name, flags in (("SUM", SUM), ("FIRST", FIRST), ("LAST", LAST), ("KEEP", KEEP)):
        ref, out = check(bh, dtype, m, n, rows, cols, vals, flags, "special values " + name)
    Zp, Zj, Zx = check(bh, dtype, m, n, rows, cols, vals, SUM, "special values")[0][:3]
    assert np.isnan(Zx).any() and np.isinf(Zx).any()
    for i, j in lone:                                                 # a lone -0 stays -0
        q = Zp[i] + int(np.searchsorted(Zj[Zp[i]:Zp[i + 1]], j))
        assert Zj[q] == j and Zx[q] == 0 and np.signbit(Zx[q])


# ---------------------------------------------------------------- 8. reuse
def test_values_through_the_map(hd):
    bh, dtype, build = hd
    m, n, rows, cols, vals, _ = special_input(dtype)
    nnz = len(rows)
    d_rows, d_cols, d_vals = up(rows, np.int32), up(cols, np.int32), up(vals, dtype)
    for combine, flags in (("sum", SUM), ("first", FIRST), ("last", LAST)):
        Zp, Zj, Zx, zmap = asm.coo_assemble_device(bh, m, n, d_rows, d_cols, d_vals, combine, want_map=True)
        assert Zx.numel() == bh.assemble_nnz and zmap[0].numel() == Zx.numel() + 1 and zmap[1].numel() == bh.assemble_nkept
        again = asm.coo_values_device(bh, d_vals, zmap, combine)
        assert np.array_equal(bits(again.cpu().numpy()), bits(Zx.cpu().numpy())), combine      # the full call's bits, NaN payloads too
        assert set(stats(bh)) == {"assemble_check", "assemble_values"}
        new = np.ascontiguousarray(np.random.default_rng(808).standard_normal(nnz), dtype)
        fresh = cr.assemble(m, n, rows, cols, new, flags)
        got = asm.coo_values_device(bh, up(new, dtype), zmap, combine)
        assert same_values(got.cpu().numpy(), fresh[2]), combine
        assert np.array_equal(Zp.cpu().numpy(), fresh[0]) and np.array_equal(Zj.cpu().numpy(), fresh[1])
    # a tampered map is refused, valZ untouched
    ent, pm, _ = zmap
    nz = ent.numel() - 1

    def refused(e, p, what):
        Zx = torch.full((nz + GUARD,), float(SENT), dtype=tdt(dtype)).cuda()
        torch.cuda.synchronize()
        assert asm.coo_values_raw_device(bh, nnz, d_vals, nz, e, p, SUM, Zx) == INV, what
        assert bool((Zx == SENT).all()), what
    bad = pm.clone()
    bad[nnz // 2] = nnz
    refused(ent, bad, "a perm entry of nnzIn")
    bad = pm.clone()
    bad[nnz - 1] = -1
    refused(ent, bad, "a negative perm entry")
    bad = ent.clone()
    bad[5] = bad[6] + 1
    refused(bad, pm, "a decreasing entryPtr")
    bad = ent.clone()
    bad[nz] = nnz + 1
    refused(bad, pm, "entryPtr[nnzZ] = nnzIn + 1")
    bad = ent.clone()
    bad[0] = 1
    refused(bad, pm, "entryPtr[0] = 1")
    Zx = torch.full((nz + GUARD,), float(SENT), dtype=tdt(dtype)).cuda()
    torch.cuda.synchronize()
    assert asm.coo_values_raw_device(bh, nnz, d_vals, nz, ent, pm, SUM, Zx) == 0 and bool((Zx[nz:] == SENT).all())
    with pytest.raises(BhsparseError):
        asm.coo_values_device(bh, d_vals, zmap, "keep")


# ---------------------------------------------------------------- 9. refusals
@pytest.mark.parametrize("at", ("first", "last"))
def test_bad_indices_are_refused_with_the_outputs_untouched(hd, at):
    bh, dtype, build = hd
    m, n, rows, cols, vals = flag_input()
    e = 0 if at == "first" else len(rows) - 1
    for what, r, c, flags in (("row == m", m, 0, SUM | IGN), ("column == n", 0, n, SUM | IGN), ("a negative row", -1, 0, SUM),
                              ("a negative column", 0, -1, KEEP), ("row == m beside a negative column", m, -1, SUM | IGN)):
        rows2, cols2 = rows.copy(), cols.copy()
        rows2[e], cols2[e] = r, c
        out = Outputs(dtype, m, len(rows))
        assert raw(bh, dtype, m, n, rows2, cols2, vals, flags, out) == INV, (what, at)
        assert out.untouched_from(0, 0, 0, 0), (what, at, "an output or a guard word was written")
    check(bh, dtype, m, n, rows, cols, vals, SUM, "after the refusals")


def test_host_refusals(hd):
    bh, dtype, build = hd
    m, n, rows, cols, vals = flag_input()
    nnz = len(rows)
    d_rows, d_cols, d_vals = up(rows, np.int32), up(cols, np.int32), up(vals, dtype)
    out = Outputs(dtype, m, nnz)

    def call(m_=m, n_=n, nnz_=nnz, r=d_rows, c=d_cols, v=d_vals, flags=SUM, Zp=out.Zp, Zj=out.Zj, Zx=out.Zx, ent=out.ent, pm=out.pm):
        torch.cuda.synchronize()
        return asm.coo_assemble_raw_device(bh, m_, n_, nnz_, r, c, v, flags, Zp, Zj, Zx, ent, pm)
    assert call(m_=-1) == INV and call(n_=-1) == INV and call(nnz_=-1) == INV
    assert call(flags=8) == INV and call(flags=SUM | 16) == INV
    assert call(r=None) == INV and call(c=None) == INV and call(Zp=None) == INV and call(Zj=None) == INV
    assert call(v=None) == INV                                         # d_valZ without d_valIn
    # an output's footprint over an input or another output: the capacities count, not what would be written
    assert call(Zj=d_rows) == INV and call(pm=d_cols) == INV and call(Zx=d_vals) == INV and call(ent=d_rows[8:]) == INV
    assert call(pm=out.Zj) == INV and call(ent=out.Zj[nnz - 1:]) == INV and call(Zp=out.pm[nnz - 1:]) == INV
    big = torch.full((2 * nnz + 2,), SENT, dtype=torch.int32).cuda()
    assert call(Zj=big[:nnz], pm=big[nnz - 1:]) == INV and call(Zj=big[:nnz], ent=big[nnz:], pm=big[2 * nnz:]) == INV
    assert out.untouched_from(0, 0, 0, 0) and bool((big == SENT).all())
    lib = bh._lib
    assert lib.bhs_coo_assemble_device(None, m, n, 0, None, None, None, 0, None, None, None, None, None, None, None, None) == INV
    # the values call
    Zp, Zj, Zx, (ent, pm, _) = asm.coo_assemble_device(bh, m, n, d_rows, d_cols, d_vals, want_map=True)
    nz = Zx.numel()
    Zx2 = torch.full((nz,), float(SENT), dtype=tdt(dtype)).cuda()

    def vcall(nnz_=nnz, v=d_vals, nz_=nz, e=ent, p=pm, flags=SUM, z=Zx2):
        torch.cuda.synchronize()
        return asm.coo_values_raw_device(bh, nnz_, v, nz_, e, p, flags, z)
    assert vcall(nnz_=-1) == INV and vcall(nz_=-1) == INV and vcall(flags=KEEP) == INV and vcall(flags=IGN) == INV and vcall(flags=8) == INV
    assert vcall(v=None) == INV and vcall(e=None) == INV and vcall(p=None) == INV and vcall(z=None) == INV
    assert vcall(z=d_vals) == INV
    assert bool((Zx2 == SENT).all())
    assert lib.bhs_coo_assemble_values_device(None, 0, None, 0, None, None, 0, None, None) == INV
    # between bhs_spgemm_symbolic and bhs_spgemm_finish
    rp, col = (np.ascontiguousarray(a, np.int32) for a in gallery.poisson_csr("poisson5pt", 8, 8, 1))
    k = len(rp) - 1
    val = np.ones(len(col), dtype)
    Cp = np.zeros(k + 1, np.int32)
    assert bh.initData(k, k, k, len(col), val, rp, col, len(col), val, rp, col, Cp) == 0
    assert bh.spgemm_symbolic() == 0
    assert call() == INV and vcall() == INV
    assert out.untouched_from(0, 0, 0, 0) and bool((Zx2 == SENT).all())
    assert bh.spgemm_numeric(0, k) == 0 and bh.spgemm_finish() == 0
    assert call() == 0 and vcall() == 0
    assert bh.free_mem() == 0


# ---------------------------------------------------------------- 10. the handle
@pytest.mark.parametrize("build", sorted(BUILDS))
def test_assembly_leaves_the_handle_alone(build, oracle):
    dtype = BUILDS[build]
    rp, col = (np.ascontiguousarray(a, np.int32) for a in gallery.poisson_csr("poisson27pt", 12, 12, 12))
    k = len(rp) - 1
    val = np.ascontiguousarray(np.random.default_rng(13).integers(1, 10, len(col)), dtype)
    ref = oracle.spgemm(k, k, k, rp, col, val, rp, col, val)
    keys = ("class_state", "mixed_rows", "spec_launches", "spec_refuted", "b_sorted", "max_row_a", "max_row_b", "select_dropped",
            "add_inplace_used")
    m, n, rows, cols, vals = flag_input()
    d_rows, d_cols, d_vals = up(rows, np.int32), up(cols, np.int32), up(vals, dtype)

    def multiply(bh, Cp):
        assert bh.spgemm() == 0
        nnzC = bh.get_nnzC()
        Cj, Cx = np.empty(nnzC, np.int32), np.empty(nnzC, dtype)
        assert bh.get_C(Cj, Cx) == 0
        assert np.array_equal(Cp, ref[0]) and np.array_equal(Cj, ref[1]) and np.array_equal(Cx, ref[2].astype(dtype))

    seen = {}
    for with_assemblies in (False, True):
        bh = new_handle(dtype, {"class_path": 2})
        try:
            Cp = np.zeros(k + 1, np.int32)
            assert bh.initData(k, k, k, len(col), val, rp, col, len(col), val, rp, col, Cp) == 0
            multiply(bh, Cp)
            before = {key: bh.get_info(key) for key in keys}
            if with_assemblies:
                for combine in ("sum", "first", "last", "keep"):
                    out = asm.coo_assemble_device(bh, m, n, d_rows, d_cols, d_vals, combine, want_map=combine != "keep")
                    if combine != "keep":
                        asm.coo_values_device(bh, d_vals, out[3], combine)
                    assert {key: bh.get_info(key) for key in keys} == before, combine
                    assert bh.get_nnzC() == len(ref[1]) and np.array_equal(bh.get_rowptrC(), ref[0])
            multiply(bh, Cp)
            multiply(bh, Cp)
            seen[with_assemblies] = {key: bh.get_info(key) for key in keys}
            assert bh.free_mem() == 0
        finally:
            bh.freePlatform()
    assert seen[True] == seen[False], seen                            # the speculative-launch counters of a fresh handle
    print("%s: %s" % (build, seen[True]))


# ---------------------------------------------------------------- 11. on top
def test_canonical_csr_is_what_the_strict_calls_accept(hd):
    """A CSR with shuffled rows and repeats: the calls that check the order of a row on the device -- the interpolation and
    the add -- refuse the raw arrays and accept the canonical ones.  (bhs_csr_cfsplit_device validates the row pointer and
    the columns' range, not the order inside a row: it is shown to accept the canonical arrays and to feed the
    interpolation.)"""
    bh, dtype, build = hd
    rng = np.random.default_rng(1111)
    Sp, Sj = (np.ascontiguousarray(a, np.int32) for a in gallery.poisson_csr("poisson5pt", 20, 15, 1))
    n = len(Sp) - 1
    lens = np.diff(Sp.astype(np.int64))
    # every row: its entries and a repeat of its first, shuffled
    rows = np.repeat(np.arange(n), lens)
    r2, c2 = np.concatenate((rows, np.arange(n))), np.concatenate((Sj, Sj[Sp[:-1]]))
    o = np.lexsort((rng.random(len(r2)), r2))
    Xp = np.concatenate(([0], np.cumsum(np.bincount(r2, minlength=n)))).astype(np.int32)
    Xj = c2[o].astype(np.int32)
    Xx = rng.integers(-4, 5, len(Xj)).astype(dtype)
    dX = (up(Xp, np.int32), up(Xj, np.int32), up(Xx, dtype))
    Zp, Zj, Zx = asm.canonical_csr_device(bh, n, n, dX)
    want = cr.assemble(n, n, r2[o], Xj, Xx, SUM)
    assert np.array_equal(Zp.cpu().numpy(), want[0]) and np.array_equal(Zj.cpu().numpy(), want[1])
    assert same_values(Zx.cpu().numpy(), want[2])
    assert np.array_equal(want[0], Sp) and np.array_equal(want[1], Sj)                                 # the matrix it was made from
    helpers.check_csr_invariants(n, n, want[0], want[1])
    Kp, Kj, Kx = asm.canonical_csr_device(bh, n, n, dX, "keep")
    assert torch.equal(Kp, dX[0]) and np.array_equal(Kj.cpu().numpy(), cr.assemble(n, n, r2[o], Xj, Xx, KEEP)[1])
    cf, nc, cpts = amg.cfsplit_device(bh, n, (Zp, Zj))
    assert 0 < nc < n and bool((cf[cpts.to(torch.int64)] == torch.arange(nc, device=cf.device)).all())
    Pp = torch.full((n + 1,), SENT, dtype=torch.int32).cuda()
    torch.cuda.synchronize()
    assert amg.interp_symbolic_raw_device(bh, n, len(Xj), dX[0], dX[1], len(Xj), dX[0], dX[1], cf, nc, Pp) == INV      # the raw arrays
    assert amg.interp_symbolic_raw_device(bh, n, Zj.numel(), Zp, Zj, Zj.numel(), Zp, Zj, cf, nc, Pp) == 0
    assert bh.interp_nnzP > 0
    Ap2 = torch.full((n + 1,), SENT, dtype=torch.int32).cuda()
    torch.cuda.synchronize()
    assert bh.csr_add_symbolic_device(n, n, len(Xj), dX[0], dX[1], len(Xj), dX[0], dX[1], Ap2)[0] == INV
    assert bh.csr_add_symbolic_device(n, n, Zj.numel(), Zp, Zj, Zj.numel(), Zp, Zj, Ap2)[:2] == (0, Zj.numel())
    assert torch.equal(Ap2, Zp)


def test_symmetric_from_edges_is_the_forest_csr(hd):
    bh, dtype, build = hd
    rp, col = (np.ascontiguousarray(a, np.int32) for a in gallery.poisson_csr("poisson5pt", 40, 30, 1))
    n = len(rp) - 1
    w = np.random.default_rng(1112).integers(1, 6, len(col)).astype(dtype)
    lo, hi, fw, _ = graph.spanning_forest_device(bh, n, (up(rp, np.int32), up(col, np.int32), up(w, dtype)))
    assert lo.numel() == n - 1
    want = graph.forest_csr_device(n, lo, hi, fw)
    got = asm.symmetric_from_edges_device(bh, n, lo, hi, fw)
    for a, b in zip(got, want):
        assert a.dtype == b.dtype and np.array_equal(bits(a.cpu().numpy()) if a.is_floating_point() else a.cpu().numpy(),
                                                     bits(b.cpu().numpy()) if b.is_floating_point() else b.cpu().numpy())
    Pp, Pj, none = asm.symmetric_from_edges_device(bh, n, lo, hi)
    assert none is None and torch.equal(Pp, want[0]) and torch.equal(Pj, want[1])


@pytest.mark.parametrize("build", sorted(BUILDS))
def test_coo_to_csr_equals_scipy(build):
    dtype = BUILDS[build]
    m, n, rows, cols, vals = flag_input()
    Zp, Zj, Zx = asm.coo_to_csr(m, n, rows, cols, vals, value_dtype=dtype)
    S = sp.coo_matrix((vals, (rows, cols)), shape=(m, n)).tocsr()
    S.sort_indices()
    assert np.array_equal(Zp, S.indptr) and np.array_equal(Zj, S.indices) and np.array_equal(Zx, S.data.astype(dtype))
    assert Zx.dtype == np.dtype(dtype)
    Pp, Pj, none = asm.coo_to_csr(m, n, rows, cols, None, value_dtype=dtype)
    assert none is None and np.array_equal(Pp, Zp) and np.array_equal(Pj, Zj)


def test_cpp_demo_runs():
    demo_dir = os.path.join(ROOT, "tests", "assemble")
    subprocess.check_call(["make", "-C", demo_dir, "-s"])
    out = subprocess.run([os.path.join(demo_dir, "assemble_demo")], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "assembly of 6528 contributions" in out.stdout and "PASS" in out.stdout
