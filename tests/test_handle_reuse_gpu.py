"""One long-lived handle across every kernel family and data set.

Nearly every other GPU test multiplies on a fresh handle; the library's users keep one and hand it data set after data
set.  The handle carries a grow-only pool of buffers (a small data set runs inside buffers sized by, and still filled
with, a large one), bitmaps that kernels must leave all-zero, epoch-tagged scan words, per-data-set verdicts and
speculation figures, the output pool and sticky options from one multiply and one data set to the next
("What a handle keeps between data sets").  Here one handle is taken through a catalogue of STATIONS --
the smallest shapes at which each kernel family is reached, from tests/test_values_gpu.py's GENERAL table and the parity
tests' builders -- in orders chosen for a hazard each.  At every station the product must be the oracle's (integers bit
for bit, "wide" reals within valuecheck's bound), and what the data set's first multiply decides -- the kernels it
launches, class_state, mixed_rows, b_sorted, compress_b_used, the longest rows -- must be what a fresh handle with the
same options decides.

Options: every station's FULL dictionary (the station's values over the library's defaults, DEFAULTS below) holds at
every station.  The fresh control handle is given all of it; the touring handle is sent only the keys whose value
differs from what it already holds: options persist, and a bhs_set_option("class_path") or ("compress_b") call itself
drops a verdict -- sent at every station it would hide one that survives bhs_set_data.  A wrong DEFAULTS table shows in
the kernel-set comparison.

Every oracle product is computed once per session (MemoOracle)."""
import hashlib
import zlib

import numpy as np
import pytest
import torch

import aggref
import extractref
import gsref
import pushref
import reduceref as rr
import selectref as sr
import semiringref
import spmvref
import spmvsrref
import test_add_gpu as addt
import test_aggregate_gpu as aggt
import test_gs_gpu as gst
import test_push_sr_gpu as pusht
import test_spmv_gpu as spmvt
import test_spmv_sr_gpu as srt
import test_trsv_gpu as trsvt
import test_values_gpu as vals
import transposeref
from helpers import poisson_case, random_csr, real_values
from valuecheck import check_bounded, on_pattern

from benchmark_spgemm_using_csr_amd import _lib, amg, gallery
from benchmark_spgemm_using_csr_amd import facade as bhmod

pytestmark = pytest.mark.gpu

BUILDS = vals.BUILDS
PAD = 64
SENT_J, SENT_X = -7, -7.0
# the library's defaults (the initialisers of struct bhs_handle, csrc/bhsparse_hip.hip) of every key a station sets
DEFAULTS = {"class_path": 1, "class_numeric": 2, "lane_rows": 1, "lane_numeric": 2, "wave_first": 1, "lds_bitmap": 1,
            "window_bitmap": 1, "sort_b": 1, "compress_b": 1}
FACTS = ("class_state", "mixed_rows", "b_sorted", "compress_b_used", "max_row_a", "max_row_b")


# ---------------------------------------------------------------- the catalogue
def _one_by_one():
    one = np.array([0, 1], np.int32)
    return 1, 1, 1, (one, np.zeros(1, np.int32), None), (one, np.zeros(1, np.int32), None)


def _unsorted_b():
    """test_unsorted_B_rows_still_correct: the entries of B shuffled inside their rows."""
    rng = np.random.default_rng(11)
    A = random_csr(300, 200, 0.05, rng)
    Bp, Bj, _ = random_csr(200, 5000, 0.02, rng)
    for j in range(200):
        Bj[Bp[j]:Bp[j + 1]] = Bj[Bp[j]:Bp[j + 1]][rng.permutation(Bp[j + 1] - Bp[j])]
    return 300, 200, 5000, (A[0], A[1], None), (Bp, Bj, None)


def _banded_long_rows():
    """test_compressed_symbolic_pass, "banded_long_rows": A rows beyond 64 entries, B rows of 70..90 adjacent columns."""
    rng = np.random.default_rng(77)
    m, k, n = 200, 400, 3000
    A = random_csr(m, k, 0.3, rng)
    lens = rng.integers(70, 91, k)
    starts = rng.integers(0, n - 100, k)
    Bp = np.zeros(k + 1, np.int32); np.cumsum(lens, out=Bp[1:])
    Bj = np.concatenate([np.arange(s0, s0 + l0) for s0, l0 in zip(starts, lens)]).astype(np.int32)
    return m, k, n, (A[0], A[1], None), (Bp, Bj, None)


LONG_ROWS_OTHER_N = 300007


def _long_rows_other_n():
    """test_values_gpu._long_rows (m, k and the pattern's shape unchanged) in a wider column space: the upper half of the
    columns moved up, so that the rows' bitmaps are laid out with other strides."""
    m, k, n, A, B = vals._long_rows()
    Bj = B[1].copy()
    Bj[Bj >= n // 2] += LONG_ROWS_OTHER_N - n
    return m, k, LONG_ROWS_OTHER_N, A, (B[0], Bj, None)


CLASS2 = vals.GENERAL["class_numeric_2"]
# name: (shape, options, kernels that must have run, float build's mode); "empty" is made on the spot (its rows depend on
# the station before it)
STATIONS = {name: (g[0], g[1], g[2], g[4]) for name, g in vals.GENERAL.items() if not name.startswith("row_ranges")}
STATIONS.update({
    "one_by_one": (_one_by_one, {}, set(), "f32_once"),
    "unsorted_b": (_unsorted_b, {"sort_b": 1}, set(), "f32_once"),
    "banded_long_rows": (_banded_long_rows, {"class_path": 0, "compress_b": 1}, set(), "f32_once"),
    # class_numeric_2's m, k, nnzA and nnzB, the stencil's grid turned: other strides, other classes
    "class_other_pattern": (lambda: vals._stencil("poisson7pt", 15, 16, 17), CLASS2[1], CLASS2[2], "f32_once"),
    "long_rows_other_n": (_long_rows_other_n, {"class_path": 0}, {"numeric_long_rows"}, "f32_atomic"),
})
assert all(set(s[1]) <= set(DEFAULTS) for s in STATIONS.values())


def full_options(name):
    return dict(DEFAULTS, **(STATIONS[name][1] if name != "empty" else {}))


class MemoOracle(object):
    """The oracle with every product remembered by its inputs' bytes: a product is computed once per session."""

    def __init__(self, oracle):
        self._oracle, self._memo = oracle, {}

    def spgemm(self, m, k, n, *arrs):
        key = (m, k, n) + tuple(hashlib.sha1(np.ascontiguousarray(a).tobytes()).digest() + str(np.asarray(a).dtype).encode()
                                for a in arrs)
        if key not in self._memo:
            self._memo[key] = self._oracle.spgemm(m, k, n, *arrs)
        return self._memo[key]

    def __getattr__(self, name):
        return getattr(self._oracle, name)


_CACHE = {}         # station inputs, the memoising oracle, the fresh handles' answers, the operations' references


def memo(oracle):
    if "oracle" not in _CACHE:
        _CACHE["oracle"] = MemoOracle(oracle)
    return _CACHE["oracle"]


def inputs(name, kind, build, draw=0):
    """(m, k, n, A, B) of a station with integer ("int") or helpers.real_values' "wide" values, as float64 arrays."""
    key = ("inputs", name, kind, build if kind == "wide" else "", draw)
    if key not in _CACHE:
        if ("shape", name) not in _CACHE:
            _CACHE[("shape", name)] = STATIONS[name][0]()
        m, k, n, A, B = _CACHE[("shape", name)]
        rng = np.random.default_rng(zlib.crc32(("%s %s %d" % (name, kind, draw)).encode()))
        if kind == "int":
            if draw == 0:
                A = (A[0], A[1], gallery.fill_values(len(A[1])))
                B = (B[0], B[1], gallery.fill_values(len(B[1]), offset=len(A[1])))
            else:
                A = (A[0], A[1], rng.integers(1, 10, len(A[1])).astype(np.float64))
                B = (B[0], B[1], rng.integers(1, 10, len(B[1])).astype(np.float64))
        else:
            _, A, B = real_values("wide", k, A, B, rng, f32=build == "f32")
        _CACHE[key] = (m, k, n, tuple(np.ascontiguousarray(x) for x in A), tuple(np.ascontiguousarray(x) for x in B))
    return _CACHE[key]


def empty_inputs(rows):
    """An empty product of `rows` rows: all-empty A on a small B (test_empty_multiply_after_nonempty_on_one_handle)."""
    k, rp, col, val = poisson_case("poisson5pt", 6, 6)
    return rows, k, k, (np.zeros(rows + 1, np.int32), np.empty(0, np.int32), np.empty(0)), (rp, col, val)


# ---------------------------------------------------------------- the handle
def new_handle(build):
    plats = [False] * bhmod.NUM_PLATFORMS
    plats[bhmod.BHSPARSE_HIP] = True
    bh = bhmod.bhsparse(value_dtype=BUILDS[build])
    assert bh.initPlatform(plats) == 0
    bh.held = dict(DEFAULTS)                  # what the handle holds of the stations' keys
    bh.bound_rows = 0
    bh.transitions = 0
    bh.last_bind = None
    return bh


def apply_options(bh, full, everything=False):
    for key in sorted(full):
        if everything or bh.held[key] != full[key]:
            assert bh.set_option(key, full[key]) == 0, key
            bh.held[key] = full[key]


def up(a, dt):
    return torch.from_numpy(np.ascontiguousarray(a, dt).copy()).cuda()


def bind(bh, data, via="host"):
    """bhs_set_data ("host") or bhs_set_data_device on torch tensors the handle borrows ("device")."""
    m, k, n, A, B = data
    vd = bh._vdt
    if via == "host":
        arrs = [np.ascontiguousarray(x, t) for x, t in ((A[2], vd), (A[0], np.int32), (A[1], np.int32),
                                                        (B[2], vd), (B[0], np.int32), (B[1], np.int32))]
        bh.Cp = np.full(m + 1, -9, np.int32)
        bh.borrowed = None
        bh.last_bind = lambda: bh.initData(m, k, n, len(arrs[2]), arrs[0], arrs[1], arrs[2], len(arrs[5]), arrs[3], arrs[4], arrs[5], bh.Cp)
    else:
        t = [up(x, dt) for x, dt in ((A[2], vd), (A[0], np.int32), (A[1], np.int32), (B[2], vd), (B[0], np.int32), (B[1], np.int32))]
        bh.Cp = None
        bh.borrowed = t
        bh.last_bind = lambda: bh.initData_device(m, k, n, len(A[1]), t[0], t[1], t[2], len(B[1]), t[3], t[4], t[5])
    assert bh.last_bind() == 0
    bh.bound_rows = m


def leave(bh):
    """Between two data sets, in turn: bhs_free_data; nothing; the old data set handed over once more, straight over
    itself (no multiply between two bhs_set_data calls)."""
    how = bh.transitions % 3
    bh.transitions += 1
    if bh.last_bind is None:
        return
    if how == 0:
        assert bh.free_mem() == 0
    elif how == 2:
        assert bh.last_bind() == 0


def ran(bh):
    return {s["name"] for s in bh.kernel_stats() if s["launches"] > 0}


def facts(bh):
    return {key: bh.get_info(key) for key in FACTS}


def fetch(bh, m):
    """(rowPtrC, colIndC, valC) as the getters serve them; nothing may land behind nnzC."""
    nnzC = bh.get_nnzC()
    Cj = np.full(nnzC + PAD, SENT_J, np.int32)
    Cx = np.full(nnzC + PAD, SENT_X, bh._vdt)
    assert bh.get_C(Cj, Cx) == 0
    assert np.all(Cj[nnzC:] == SENT_J) and np.all(Cx[nnzC:] == SENT_X), "get_C served more than nnzC entries"
    Cp = bh.get_rowptrC()
    assert len(Cp) == m + 1
    if bh.Cp is not None:
        assert np.array_equal(bh.Cp, Cp), "the caller's csrRowPtrC differs from bhs_get_rowptrC"
    return Cp, Cj[:nnzC], Cx[:nnzC]


def check_product(oracle, bh, data, kind, mode, what):
    """The handle's last product against the oracle: integers bit for bit, reals within check_bounded's bound of `mode`."""
    m, k, n, A, B = data
    got = fetch(bh, m)
    if m and len(A[1]) == 0:                                        # (an empty product needs no oracle)
        assert bh.get_nnzC() == 0 and not got[0].any(), what
        return
    if kind == "int":
        ref = oracle.spgemm(m, k, n, *A, *B)
        assert bh.get_nnzC() == ref[0][-1], (what, bh.get_nnzC(), int(ref[0][-1]))
        assert np.array_equal(got[0].astype(np.int64), ref[0]), (what, "rowPtrC differs")
        assert np.array_equal(got[1], ref[1]), (what, "colIndC differs")
        assert np.array_equal(got[2], ref[2].astype(bh._vdt)), (what, "valC differs")
    else:
        worst = check_bounded(oracle, m, k, n, A, B, got, mode, what=what + ": ")
        print("%-60s %-10s worst err/bound %.3g" % (what, mode, worst))


def multiply_in_ranges(bh, m):
    cuts = [0, m // 5, m // 5, m // 2 + 3, m]                       # (test_values_gpu.multiply's)
    assert bh.spgemm_symbolic() == 0
    for a, b in zip(cuts[:-1], cuts[1:]):
        assert bh.spgemm_numeric(min(a, m), min(b, m)) == 0
    assert bh.spgemm_finish() == 0


def fresh_answer(name, data, kind, build, via):
    """What a fresh handle given the station's full dictionary decides on its first multiply: (kernels, facts)."""
    key = ("fresh", name, data[0], kind, build, via)
    if key not in _CACHE:
        bh = new_handle(build)
        try:
            apply_options(bh, full_options(name), everything=True)
            bind(bh, data, via)
            assert bh.spgemm() == 0
            _CACHE[key] = (ran(bh), facts(bh))
            assert bh.free_mem() == 0
        finally:
            bh.freePlatform()
    return _CACHE[key]


def must_run(name, build):
    want = set(STATIONS[name][2]) if name != "empty" else set()
    if name == "wave_wg" and build == "f32":
        want |= {"numeric_wg<4096>"}                                # (test_values_gpu.run_general)
    return want


def visit(oracle, bh, name, build, via="host", between=None, what=""):
    """One station on the touring handle, with integer values and then with "wide" ones: the data set handed over, two
    multiplies, a third in row ranges.  between(data, kind): called after the first multiply and its checks; the
    multiply after it is checked like the others."""
    for kind in ("int", "wide"):
        if name == "empty":
            if kind == "wide":
                continue
            data = empty_inputs(2 * bh.bound_rows + 7)
        else:
            data = inputs(name, kind, build)
        m = data[0]
        tag = "%s%s %s %s" % (what, name, kind, build)
        leave(bh)
        apply_options(bh, full_options(name))
        bind(bh, data, via)
        assert bh.spgemm() == 0, tag
        names, seen = ran(bh), facts(bh)
        want_names, want_facts = fresh_answer(name, data, kind, build, via)
        assert names == want_names, (tag, "kernels differ from a fresh handle's", sorted(names ^ want_names))
        assert must_run(name, build) <= names, (tag, sorted(must_run(name, build) - names))
        assert seen == want_facts, (tag, "get_info differs from a fresh handle's", seen, want_facts)
        if name == "banded_long_rows":
            assert seen["compress_b_used"] == 1, tag
        if name in ("unsorted_b",):
            assert seen["b_sorted"] == 1, tag
        mode = "f64" if build == "f64" else vals.f32_mode(names, STATIONS[name][3] if name != "empty" else None)
        check_product(oracle, bh, data, kind, mode, tag + " first")
        if between is not None:
            between(data, kind)
        assert bh.spgemm() == 0, tag
        check_product(oracle, bh, data, kind, mode, tag + " second")
        multiply_in_ranges(bh, m)
        check_product(oracle, bh, data, kind, mode, tag + " ranges")
        if bh.borrowed is not None:
            torch.cuda.synchronize()
            A, B = data[3], data[4]
            for t, x in zip(bh.borrowed, (A[2], A[0], A[1], B[2], B[0], B[1])):
                assert np.array_equal(t.cpu().numpy(), np.asarray(x).astype(t.cpu().numpy().dtype)), (tag, "a borrowed array was written")


# ---------------------------------------------------------------- the orders
DESCENDING = ["hub_rows", "long_rows_lds", "column_windows", "wave_wg", "big_class", "class_numeric_2", "quad", "lane",
              "one_by_one", "empty"]
CATALOGUE = sorted(STATIONS) + ["empty"]
ORDERS = {
    # every later station runs in buffers larger than it needs, the earlier contents behind its own
    "descending_pool": DESCENDING,
    # every ensure reallocates: the zero-initialisation of new tile-word, spa and hub buffers at every step
    "ascending_pool": DESCENDING[::-1],
    # class path -> general pipeline -> mixed mode -> clean classes again -> lane kernels -> other class kernels
    "path_flips": ["class_numeric_2", "wave_wg", "mixed", "class_numeric_2", "lane", "class_numeric_0", "class_other_pattern",
                   "big_class", "class_numeric_1"],
    # the bitmaps of the long-row, window and hub kernels, re-laid-out when n changes and left all-zero by each
    "bitmaps": ["long_rows_hbm", "long_rows_other_n", "hub_rows", "long_rows_hbm", "column_windows", "long_rows_lds", "hub_rows"],
    # B borrowed or copied, as it is or sorted on the handle's private copy
    "b_ownership": [("banded_long_rows", "device"), ("unsorted_b", "device"), ("banded_long_rows", "host"), ("unsorted_b", "host"),
                    ("banded_long_rows", "device")],
    "shuffle_1": [CATALOGUE[i] for i in np.random.default_rng(1).permutation(len(CATALOGUE))],
    "shuffle_2": [CATALOGUE[i] for i in np.random.default_rng(2).permutation(len(CATALOGUE))],
}
TOURS = [(o, "f64") for o in ORDERS] + [(o, "f32") for o in ("descending_pool", "path_flips", "bitmaps")]


@pytest.mark.parametrize("order,build", TOURS, ids=["%s-%s" % t for t in TOURS])
def test_tour(oracle, order, build):
    oracle = memo(oracle)
    bh = new_handle(build)
    try:
        for i, stop in enumerate(ORDERS[order]):
            name, via = stop if isinstance(stop, tuple) else (stop, "host")
            visit(oracle, bh, name, build, via, what="%s[%d] " % (order, i))
            if order == "path_flips" and name == "class_numeric_2":
                assert bh.get_info("class_state") == 1                  # (clean again after the mixed station)
            if order == "path_flips" and name == "mixed":
                assert bh.get_info("class_state") == 2 and bh.get_info("mixed_rows") > 0
        assert bh.free_mem() == 0
        assert bh.get_nnzC() == 0
    finally:
        bh.freePlatform()


# ---------------------------------------------------------------- other operations between the multiplies
def _ragged(seed, m, n, lens):
    rng = np.random.default_rng(seed)
    lens = np.asarray(lens)
    Xp = np.zeros(m + 1, np.int32); np.cumsum(lens, out=Xp[1:])
    Xj = np.concatenate([np.sort(rng.choice(n, L, replace=False)) for L in lens] + [np.empty(0, np.int64)]).astype(np.int32)
    return Xp, Xj, rng.integers(1, 10, len(Xj)).astype(np.float64)


def _unrelated(size, which=0):
    """A matrix unrelated to any station: "large" 1500 x 2600 with rows of 0 .. 1500 entries (every row family of the
    operations' kernels), "small" 37 x 50."""
    key = ("unrelated", size, which)
    if key not in _CACHE:
        if size == "large":
            rng = np.random.default_rng(40 + which)
            lens = rng.integers(0, 30, 1500)
            lens[::97] = rng.integers(40, 900, len(lens[::97]))
            lens[[3, 777]] = (1500, 1100)
            _CACHE[key] = (1500, 2600) + (_ragged(50 + which, 1500, 2600, lens),)
        else:
            _CACHE[key] = (37, 50) + (_ragged(60 + which, 37, 50, np.random.default_rng(70 + which).integers(0, 9, 37)),)
    return _CACHE[key]


def _cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def _same_exactly(got, ref, what):
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.dtype == ref.dtype and got.shape == ref.shape, (what, got.dtype, ref.dtype, got.shape, ref.shape)
    assert np.array_equal(got, ref), what


def _dev(X, vd):
    return (up(X[0], np.int32), up(X[1], np.int32), up(X[2], vd))


def op_masked(oracle, bh, data, size, what):
    m, k, n, A, B = data
    ref = oracle.spgemm(m, k, n, *A, *B)
    Mp, Mj, _ = _cached(("M", what, size), lambda: addt.pattern_with_extras(
        np.random.default_rng(5), m, n, (ref[0], ref[1]), 0.9 if size == "large" else 0.05, 5 if size == "large" else 1))
    valC = torch.full((len(Mj) + PAD,), SENT_X, dtype=vals_tdt(bh)).cuda()
    assert bh.spgemm_masked_device(up(Mp, np.int32), up(Mj, np.int32), len(Mj), valC) == 0
    got = valC.cpu().numpy()
    assert np.all(got[len(Mj):] == SENT_X), what
    _same_exactly(got[:len(Mj)], on_pattern(ref, n, Mp, Mj).astype(bh._vdt), what)


def op_semiring_masked(oracle, bh, data, size, what):
    m, k, n, A, B = data
    ref = oracle.spgemm(m, k, n, *A, *B)
    Mp, Mj, _ = _cached(("M", what, size), lambda: addt.pattern_with_extras(
        np.random.default_rng(6), m, n, (ref[0], ref[1]), 0.9 if size == "large" else 0.05, 5 if size == "large" else 1))
    want = _cached(("min_plus", what, size, bh._vdt), lambda: semiringref.semiring_masked("min_plus", m, n, A, B, Mp, Mj, bh._vdt))
    valC = torch.full((len(Mj) + PAD,), SENT_X, dtype=vals_tdt(bh)).cuda()
    assert bh.spgemm_semiring_masked_device(_lib.SEMIRINGS["min_plus"], up(Mp, np.int32), up(Mj, np.int32), len(Mj), valC) == 0
    got = valC.cpu().numpy()
    assert np.all(got[len(Mj):] == SENT_X), what
    assert semiringref.same_bits(got[:len(Mj)], want), what


def op_spgemm_add(oracle, bh, data, size, what):
    m, k, n, A, B = data
    ref = oracle.spgemm(m, k, n, *A, *B)
    D = _cached(("D", what, size), lambda: addt.pattern_with_extras(
        np.random.default_rng(7), m, n, (ref[0], ref[1]), 0.5 if size == "large" else 0.02, 3 if size == "large" else 1))
    want = addt.reference(oracle, m, k, n, A, B, D, 2, -1)
    assert bh.spgemm_add_device(2, -1, len(D[1]), up(D[2], bh._vdt), up(D[0], np.int32), up(D[1], np.int32)) == 0
    assert bh.get_info("add_inplace_used") == 0, what                # (D reaches outside A·B: the sum lives in arrays of its own)
    got = fetch(bh, m)
    assert bh.get_nnzC() == want[0][-1], what
    assert np.array_equal(got[0].astype(np.int64), want[0]) and np.array_equal(got[1], want[1]), what
    _same_exactly(got[2], want[2].astype(bh._vdt), what)


def op_spgemm_select(oracle, bh, data, size, what):
    m, k, n, A, B = data
    ref = oracle.spgemm(m, k, n, *A, *B)
    spec = sr.Spec(flags=sr.TOPK, top_k=40 if size == "large" else 2)
    want = _cached(("topk", what, size, bh._vdt), lambda: sr.select(m, n, ref[0], ref[1], np.asarray(ref[2], bh._vdt), spec))
    c = _lib.Select()
    c.flags, c.top_k, c.band_lo, c.band_hi, c.abs_tol, c.rel_tol = spec.flags, spec.top_k, spec.band_lo, spec.band_hi, spec.abs_tol, spec.rel_tol
    assert bh.spgemm_select(c) == 0
    got = fetch(bh, m)
    assert bh.get_nnzC() == len(want[1]), what
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), what
    _same_exactly(got[2], want[2], what)


def vals_tdt(bh):
    return torch.float32 if bh._vdt == np.dtype(np.float32) else torch.float64


def op_csr_add(oracle, bh, data, size, what):
    m, n, X = _unrelated(size)
    _, _, Y = _unrelated(size, 1)
    want = _cached(("np_add", size), lambda: addt.np_add(m, n, 2, X, -1, Y))
    Zp, Zj, Zx, _ = bh.csr_add_device(m, n, 2, _dev(X, bh._vdt), -1, _dev(Y, bh._vdt))
    assert np.array_equal(Zp.cpu().numpy(), want[0]) and np.array_equal(Zj.cpu().numpy(), want[1]), what
    _same_exactly(Zx.cpu().numpy(), want[2].astype(bh._vdt), what)


def op_csr_select(oracle, bh, data, size, what):
    m, n, X = _unrelated(size)
    spec = sr.Spec(flags=sr.TOPK | sr.DROP_DIAG, top_k=7)
    want = _cached(("select", size, bh._vdt), lambda: sr.select(m, n, X[0], X[1], np.asarray(X[2], bh._vdt), spec))
    c = _lib.Select()
    c.flags, c.top_k, c.band_lo, c.band_hi, c.abs_tol, c.rel_tol = spec.flags, spec.top_k, spec.band_lo, spec.band_hi, spec.abs_tol, spec.rel_tol
    Zp, Zj, Zx = bh.csr_select_device(m, n, _dev(X, bh._vdt), c)
    assert np.array_equal(Zp.cpu().numpy(), want[0]) and np.array_equal(Zj.cpu().numpy(), want[1]), what
    _same_exactly(Zx.cpu().numpy(), want[2], what)


def op_csr_transpose(oracle, bh, data, size, what):
    m, n, X = _unrelated(size)
    want = _cached(("transpose", size, bh._vdt), lambda: transposeref.transpose(m, n, X[0], X[1], np.asarray(X[2], bh._vdt)))
    Tp, Tj, Tx, pm = bh.csr_transpose_device(m, n, _dev(X, bh._vdt), perm=True)
    assert np.array_equal(Tp.cpu().numpy(), want[0]) and np.array_equal(Tj.cpu().numpy(), want[1]), what
    _same_exactly(Tx.cpu().numpy(), want[2], what)
    assert np.array_equal(pm.cpu().numpy(), want[3]), what


def op_csr_extract(oracle, bh, data, size, what):
    m, n, X = _unrelated(size)
    rng = np.random.default_rng(8)
    rows = rng.choice(m, m // 2, replace=False).astype(np.int32)
    cols = rng.permutation(n)[:2 * n // 3].astype(np.int32)
    want = _cached(("extract", size, bh._vdt), lambda: extractref.extract(m, n, X[0], X[1], np.asarray(X[2], bh._vdt), rows, cols))
    Zp, Zj, Zx, _ = bh.csr_extract_device(m, n, _dev(X, bh._vdt), up(rows, np.int32), up(cols, np.int32))
    assert np.array_equal(Zp.cpu().numpy(), want[0]) and np.array_equal(Zj.cpu().numpy(), want[1]), what
    _same_exactly(Zx.cpu().numpy(), want[2], what)


def op_csr_reduce(oracle, bh, data, size, what):
    m, n, X = _unrelated(size)
    for axis in (rr.ROWS, rr.COLS):
        want = rr.reduce(m, n, X[0], X[1], np.asarray(X[2], bh._vdt), axis, rr.PLUS, 0, bh._vdt)[0]
        _same_exactly(bh.csr_reduce_device(m, n, _dev(X, bh._vdt), axis, rr.PLUS).cpu().numpy(), want, what)


def op_csr_scale(oracle, bh, data, size, what):
    m, n, X = _unrelated(size)
    rng = np.random.default_rng(9)
    left, right = rng.integers(1, 5, m).astype(np.float64), rng.integers(1, 5, n).astype(np.float64)
    want = rr.scale(m, n, X[0], X[1], np.asarray(X[2], bh._vdt), 2.0, left, right, 0, bh._vdt)
    got = bh.csr_scale_device(m, n, _dev(X, bh._vdt), 2.0, up(left, bh._vdt), up(right, bh._vdt))
    _same_exactly(got.cpu().numpy(), want, what)


# the CSR x dense products, the push product, the aggregation, the colouring with its sweep and the levels with the solve
# and ILU(0): workspaces of their own on the handle, each exact against its numpy restatement of tests/
def _same_bits(got, ref, what):
    assert semiringref.same_bits(np.asarray(got).astype(np.float64), np.asarray(ref, np.float64)), what


def _dense_ints(rows, k, seed):
    return np.random.default_rng(seed).integers(-9, 10, (rows, k)).astype(np.float64)


def op_spmv_spmm(oracle, bh, data, size, what):
    m, n, X = _unrelated(size)
    D = _cached(("spmv dev", size, bh._vdt), lambda: spmvt.Dev(m, n, X, bh._vdt))
    for k in (1, 3):
        V, Y = _dense_ints(n, k, 20 + k), _dense_ints(m, k, 30 + k)
        want = _cached(("spmm", size, k), lambda: spmvref.spmm(m, n, X[0], X[1], X[2], V, 2.0, -1.0, Y)[0])
        _same_exactly(spmvt.run(bh, D, V, 2.0, -1.0, Y, what=what), want.astype(bh._vdt), (what, k))


def op_spmv_semiring(oracle, bh, data, size, what):
    m, n, X = _unrelated(size)
    D = _cached(("spmv dev", size, bh._vdt), lambda: spmvt.Dev(m, n, X, bh._vdt))
    k = 4 if size == "large" else 1
    V, Y = _dense_ints(n, k, 41), np.where(_dense_ints(m, k, 42) < 0, np.inf, _dense_ints(m, k, 43))
    want = _cached(("srmv", size), lambda: spmvsrref.spmm_semiring("min_plus", m, n, X[0], X[1], X[2], V, Y, None, True))
    got, changed = srt.run(bh, "min_plus", D, V, Y, None, True, what=what)
    _same_bits(got, want[0], what)
    assert changed == want[1], (what, changed, want[1])


def op_push(oracle, bh, data, size, what):
    m, n, G = _unrelated(size)
    D = _cached(("push dev", size, bh._vdt), lambda: pusht.Dev(m, n, G, bh._vdt))
    rng = np.random.default_rng(44)
    k, nf = (4, 200) if size == "large" else (1, 10)
    fidx = rng.integers(0, m, nf)
    fidx[:3] = (3, 3, m - 1)                                          # (the large shape's 1500-entry row, twice)
    F = rng.integers(0, 20, (nf, k)).astype(np.float64)
    Y = np.where(rng.random((n, k)) < 0.5, np.inf, rng.integers(0, 30, (n, k)).astype(np.float64))
    want = _cached(("push", size), lambda: pushref.push_semiring("min_plus", m, n, G[0], G[1], G[2], fidx, F, Y))
    got, changed, nxt = pusht.run(bh, "min_plus", D, fidx, F, Y, what=what)
    _same_bits(got, want[0], what)
    assert changed == want[1] and np.array_equal(nxt, want[2]), (what, changed, want[1])


def op_aggregate(oracle, bh, data, size, what):
    name = "uniform2048" if size == "large" else "two_one_edge"
    n, Sp, Sj = aggt.cases()[name]
    aggt.check(aggt.run(bh, n, Sp, Sj, 1, what=what), aggt.reference(name, 1), what)


def _poisson_sweep(size):
    """(n, Ap, Aj, Ax, b, x0, the restatement's colouring with seed 0 and its forward sweep): poisson5pt (diagonal 4, -1 beside
    it) on integers, every value an integer over 4^colours of fewer than 24 bits -- exact in both builds
    (test_gs_gpu.test_sweep_bit_for_bit_on_dyadic_values)"""
    def make():
        n, Ap, Aj, Ax = aggref.poisson("poisson5pt", *((33, 33) if size == "large" else (7, 5)))
        rng = np.random.default_rng(45)
        b, x0 = rng.integers(-8, 9, n).astype(np.float64), rng.integers(-8, 9, n).astype(np.float64)
        col = gsref.colouring(n, Ap, Aj, 0)
        want = gsref.sweep(Ap, Aj, Ax, np.full(n, 4.0), col[3], col[2], b, x0, 1.0, 1, gsref.FORWARD)
        scaled = want * 4.0 ** col[1]
        assert col[1] <= 5 and np.array_equal(scaled, np.round(scaled)) and np.abs(scaled).max() < 2.0 ** 24
        return n, Ap, Aj, Ax, b, x0, col, want
    return _cached(("poisson sweep", size), make)


def op_color_sweep(oracle, bh, data, size, what):
    """the sweep runs on the device arrays the colouring has just returned"""
    n, Ap, Aj, Ax, b, x0, col, want = _poisson_sweep(size)
    A = (up(Ap, np.int32), up(Aj, np.int32), up(Ax, bh._vdt))
    color, ncolors, order, cptr = amg.color_device(bh, n, A, 0)
    gst.color_check((color.cpu().numpy(), ncolors, order.cpu().numpy(), cptr, bh.color_rounds), col, what)
    x = amg.gs_device(bh, A, up(np.full(n, 4.0), bh._vdt), (color, ncolors, order, cptr), up(b, bh._vdt), up(x0, bh._vdt),
                      direction="forward", verify=True)
    _same_exactly(x.cpu().numpy(), want.astype(bh._vdt), what)


def op_levels_solve_ilu(oracle, bh, data, size, what):
    """the levels of both triangles, the lower solve on the device arrays the levels call returned, ILU(0)"""
    name = "uniform2048" if size == "large" else "path300"
    n, Ap, Aj, Ax, xs, bl, bu = trsvt.exact_case(name)
    A = (up(Ap, np.int32), up(Aj, np.int32), up(Ax, bh._vdt))
    lev = amg.levels_device(bh, n, A)
    want = trsvt.level_reference(name, False, True)
    trsvt.levels_check((lev[0].cpu().numpy(), lev[1], lev[2].cpu().numpy(), lev[3], bh.levels_passes), want, what)
    trsvt.levels_check(trsvt.levels_run(bh, n, Ap, Aj, _lib.BHS_TRI_UPPER, what=what), trsvt.level_reference(name, True, True), what)
    x = amg.trsv_device(bh, A, lev, up(bl, bh._vdt), up(np.zeros(n), bh._vdt), alpha=0.5)
    _same_exactly(x.cpu().numpy(), xs.astype(bh._vdt), what)
    fname = "two_dense70" if size == "large" else "arrow200"
    fn, Fp, Fj, Fx, factors = trsvt.factor_case(fname)
    T = _cached(("tri", fname, bh._vdt), lambda: trsvt.Tri(fn, Fp, Fj, Fx, bh._vdt))
    got, pivot = trsvt.ilu_run(bh, T, what=what)
    assert pivot == -1 and np.array_equal(got, factors), (what, pivot)


OPERATIONS = [op_masked, op_semiring_masked, op_spgemm_add, op_spgemm_select, op_csr_add, op_csr_select, op_csr_transpose,
              op_csr_extract, op_csr_reduce, op_csr_scale, op_spmv_spmm, op_spmv_semiring, op_push, op_aggregate, op_color_sweep,
              op_levels_solve_ilu]
OPS_A_STATION = 4


@pytest.mark.parametrize("build", sorted(BUILDS))
def test_tour_with_operations(oracle, build):
    """The path_flips order with other operations of the handle after each data set's first multiply: station i runs the
    four operations from 4 i on (of sixteen, in a circle), each operation on a large shape at one call and a small one at
    its next, so that its own pool grows and is then reused oversized; the multiplies after them are checked like every
    other.  Nine stations: every operation runs at least twice, once large and once small."""
    oracle = memo(oracle)
    bh = new_handle(build)
    calls, sizes = {}, {}
    nops = len(OPERATIONS)
    try:
        for i, name in enumerate(ORDERS["path_flips"]):
            def between(data, kind, i=i, name=name):
                if kind != "int":                                       # (the operations' references are exact on integers)
                    return
                for j in [(OPS_A_STATION * i + t) % nops for t in range(OPS_A_STATION)]:
                    op = OPERATIONS[j]
                    calls[j] = calls.get(j, j) + 1                      # (even operations start large, odd ones small)
                    size = "large" if calls[j] % 2 else "small"
                    sizes.setdefault(j, set()).add(size)
                    op(oracle, bh, data, size, "%s %s after %s[%d] %s" % (op.__name__, size, name, i, build))
                    torch.cuda.synchronize()
            visit(oracle, bh, name, build, between=between, what="operations[%d] " % i)
        assert set(calls) == set(range(nops))
        assert all(sizes[j] == {"large", "small"} for j in range(nops)), sizes
        assert bh.free_mem() == 0
    finally:
        bh.freePlatform()


# ---------------------------------------------------------------- values rewritten in place, pattern unchanged
def _rewrite(bh, data):
    A, B = data[3], data[4]
    bh.borrowed[0].copy_(up(A[2], bh._vdt))
    bh.borrowed[3].copy_(up(B[2], bh._vdt))
    torch.cuda.synchronize()


def _bind_and_check_first(oracle, bh, name, build):
    data = inputs(name, "int", build)
    apply_options(bh, full_options(name))
    bind(bh, data, "device")
    before = bh.get_info("spec_launches")
    assert bh.spgemm() == 0
    assert bh.get_info("spec_launches") == before, (name, "a data set's first multiply went out on another's figures")
    names, seen = ran(bh), facts(bh)
    want_names, want_facts = fresh_answer(name, data, "int", build, "device")
    assert names == want_names and must_run(name, build) <= names and seen == want_facts, (name, sorted(names ^ want_names), seen, want_facts)
    check_product(oracle, bh, data, "int", "f64", name + " first")
    return names


@pytest.mark.parametrize("build", ["f64"])
def test_values_rewritten_in_place(oracle, build):
    """Borrowed device arrays whose values change between the multiplies (the pattern does not): the speculative openings
    of the class and lane paths run on the last multiply's figures and must serve the new values."""
    oracle = memo(oracle)
    bh = new_handle(build)
    try:
        for name in ("class_numeric_2", "lane", "wave_wg"):
            spec0 = bh.get_info("spec_launches") if bh.last_bind else 0
            names = _bind_and_check_first(oracle, bh, name, build)
            mode = "f64" if build == "f64" else vals.f32_mode(names, STATIONS[name][3])
            for kind, draw in (("int", 1), ("wide", 0), ("wide", 1)):
                data = inputs(name, kind, build, draw)
                _rewrite(bh, data)
                assert bh.spgemm() == 0
                check_product(oracle, bh, data, kind, mode, "%s rewritten %s %d" % (name, kind, draw))
            if name != "wave_wg":
                assert bh.get_info("spec_launches") > spec0, name       # (the speculative openings ran, and what they wrote was checked)
            assert bh.get_info("spec_refuted") == 0, name
        # the same sizes, another pattern: first after wave_wg, then straight after class_numeric_2 with no option changed between
        for before in (None, "class_numeric_2"):
            if before:
                _bind_and_check_first(oracle, bh, before, build)
                spec0 = bh.get_info("spec_launches")
                assert bh.spgemm() == 0 and bh.get_info("spec_launches") == spec0 + 1
            _bind_and_check_first(oracle, bh, "class_other_pattern", build)
            assert bh.spgemm() == 0
            check_product(oracle, bh, inputs("class_other_pattern", "int", build), "int", "f64", "other pattern second")
        assert bh.get_info("spec_refuted") == 0
        assert bh.free_mem() == 0
    finally:
        bh.freePlatform()


# ---------------------------------------------------------------- recovery after a refused multiply
@pytest.mark.parametrize("form", ["whole", "split"])
def test_recovery_after_refused_multiply(oracle, form):
    """Bound output arrays one entry too small: the multiply (or the numeric half) answers BHS_ERR_ALLOC and writes nothing
    behind the arrays' end; bound large enough it is right, and so are the long-row and hub kernels after it (the refusal
    marks the bitmaps for re-zeroing)."""
    oracle = memo(oracle)
    build = "f64"
    bh = new_handle(build)
    try:
        for name in ("wave_wg", "mixed"):
            data = inputs(name, "int", build)
            m, k, n, A, B = data
            nnzC = int(oracle.spgemm(m, k, n, *A, *B)[0][-1])
            cj = torch.full((nnzC + PAD,), SENT_J, dtype=torch.int32).cuda()
            cx = torch.full((nnzC + PAD,), SENT_X, dtype=torch.float64).cuda()
            torch.cuda.synchronize()
            leave(bh)
            apply_options(bh, full_options(name))
            bind(bh, data)                                          # (the first multiply of the data set: no speculation figures)
            assert bh.set_output_device(cj, cx, nnzC - 1) == 0
            if form == "whole":
                assert bh.spgemm() == _lib.BHS_ERR_ALLOC, name
            else:
                assert bh.spgemm_symbolic() == 0 and bh.nnzC == nnzC
                assert bh.spgemm_numeric(0, m) == _lib.BHS_ERR_ALLOC, name
            torch.cuda.synchronize()
            assert bool((cj[nnzC:] == SENT_J).all()) and bool((cx[nnzC:] == SENT_X).all()), (name, "written behind the bound arrays")
            assert bh.set_output_device(cj, cx, nnzC) == 0
            if form == "whole":
                assert bh.spgemm() == 0
            else:
                multiply_in_ranges(bh, m)
            check_product(oracle, bh, data, "int", "f64", "%s %s after the refusal" % (name, form))
            torch.cuda.synchronize()
            assert bool((cj[nnzC:] == SENT_J).all()) and bool((cx[nnzC:] == SENT_X).all()), (name, "written behind the bound arrays")
            ref = oracle.spgemm(m, k, n, *A, *B)
            assert np.array_equal(cj[:nnzC].cpu().numpy(), ref[1]) and np.array_equal(cx[:nnzC].cpu().numpy(), ref[2]), name
            assert bh.set_output_device(None, None, 0) == 0
            for after in ("long_rows_hbm", "hub_rows"):
                visit(oracle, bh, after, build, what="after the refusal on %s (%s): " % (name, form))
        assert bh.free_mem() == 0
    finally:
        bh.freePlatform()
