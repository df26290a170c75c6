"""CPU tests of the semiring multiply's interfaces (bhs_spgemm_semiring[_masked[_device]]): the header declares the entry
points and the constants, both libraries export them and carry the new kernels, the facades have the methods, the C++ demo
builds -- and the numpy restatement of the rule (tests/semiringref.py), the reference of tests/test_semiring_gpu.py, is
pinned against a dense triple loop."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT
import semiringref as sr

from benchmark_spgemm_using_csr_amd import _lib

ENTRY = ("bhs_spgemm_semiring_masked_device", "bhs_spgemm_semiring_masked", "bhs_spgemm_semiring")
CONSTANTS = ("BHS_SR_PLUS_TIMES", "BHS_SR_MIN_PLUS", "BHS_SR_MAX_PLUS", "BHS_SR_MAX_TIMES", "BHS_SR_MIN_MAX", "BHS_SR_MAX_MIN",
             "BHS_SR_OR_AND", "BHS_SR_PLUS_PAIR")
DEMO_DIR = os.path.join(ROOT, "tests", "semiring")


def test_header_declares_the_entry_points_and_the_constants():
    txt = open(_lib.HEADER).read()
    decl = set(re.findall(r"BHS_API\s+[\w\s\*]+?\b(bhs_\w+)\s*\(", txt))
    for name in ENTRY:
        assert name in decl
        assert name in _lib.SYMBOLS
    for value, name in enumerate(CONSTANTS):
        m = re.search(r"\b%s\s*=\s*(\d+)" % name, txt)
        assert m and int(m.group(1)) == value, name
        assert getattr(_lib, name) == value
    assert "semiring multiply" in txt
    for fam in ("sr_scan", "sr_short", "sr_wave", "sr_long", "sr_hub"):
        assert fam in txt


def test_both_libraries_export_the_entry_points(hiplib):
    for path in (_lib.SO_PATH, _lib.SO_PATH_F32):
        raw = C.CDLL(path)
        for name in ENTRY:
            assert getattr(raw, name) is not None
        blob = open(path, "rb").read()
        for kern in (b"k_sr_lds", b"k_sr_long", b"k_sr_hub", b"k_sr_init", b"k_sr_decode"):
            assert kern in blob


def test_sources_are_tracked_by_the_build():
    assert "bhs_semiring.hip.h" in _lib.SOURCES and "bhs_host_semiring.inc.h" in _lib.SOURCES
    mk = open(os.path.join(_lib.CSRC, "Makefile")).read()
    assert "bhs_semiring.hip.h" in mk and "bhs_host_semiring.inc.h" in mk
    for f in ("bhs_semiring.hip.h", "bhs_host_semiring.inc.h"):
        assert os.path.exists(os.path.join(_lib.CSRC, f))


def test_null_handle_is_rejected(hiplib):
    nnzct = C.c_int64(0)
    for s in range(8):
        assert hiplib.bhs_spgemm_semiring_masked(None, s, None, None, 0, None, C.byref(nnzct), None) == _lib.BHS_ERR_INVALID_ARG
        assert hiplib.bhs_spgemm_semiring_masked_device(None, s, None, None, 0, None, None, None) == _lib.BHS_ERR_INVALID_ARG
        assert hiplib.bhs_spgemm_semiring(None, s, None, None, None, None) == _lib.BHS_ERR_INVALID_ARG


def test_python_facade_has_the_semiring_multiply():
    from benchmark_spgemm_using_csr_amd import facade
    for name in ("spgemm_semiring", "spgemm_semiring_masked", "spgemm_semiring_masked_device"):
        assert callable(getattr(facade.bhsparse, name, None)), name
    assert callable(getattr(facade, "spgemm_semiring_csr", None))
    assert callable(getattr(facade, "spgemm_semiring_masked_csr", None))
    assert facade.bhsparse().semiring_ms == 0.0
    assert sorted(_lib.SEMIRINGS.values()) == list(range(8))


def test_cpp_facade_semiring_extension_builds(hiplib):
    src = open(os.path.join(ROOT, "benchmark_spgemm_using_csr_amd", "host", "bhsparse.h")).read()
    flat = re.sub(r"\s+", " ", src)
    assert "int spgemm_semiring(int semiring);" in flat
    assert ("int spgemm_semiring_masked(int semiring, int *csrRowPtrM, int *csrColIndM, int nnzM, value_type *csrValC);"
            in flat)
    subprocess.check_call(["make", "-C", DEMO_DIR, "-s"])
    demo = os.path.join(DEMO_DIR, "semiring_demo")
    assert os.access(demo, os.X_OK)
    out = subprocess.run(["nm", "-D", "--undefined-only", demo], capture_output=True, text=True).stdout
    assert "bhs_spgemm_semiring" in out


def test_cpp_facade_header_can_be_included_twice(tmp_path):
    """Every inline definition of host/bhsparse.h sits inside its include guard: a translation unit that meets the header
    through two of its own headers still compiles."""
    hdr = os.path.join(ROOT, "benchmark_spgemm_using_csr_amd", "host", "bhsparse.h")
    src = tmp_path / "twice.cpp"
    src.write_text('#include "%s"\n#include "%s"\nint main() { bhsparse b; return b.spgemm_semiring(BHS_SR_MIN_PLUS) == 0; }\n'
                   % (hdr, hdr))
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    r = subprocess.run([hipcc, "-std=c++17", "-fsyntax-only", str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


# ---------------------------------------------------------------- the reference against a dense triple loop
def _below(a, b):
    """a before b in the rule's order: as numbers, -0 below +0"""
    if a == b:
        return math.copysign(1.0, a) < math.copysign(1.0, b)
    return a < b


def _omax(a, b):
    if math.isnan(a) or math.isnan(b):
        return math.nan
    return b if _below(a, b) else a


def _omin(a, b):
    if math.isnan(a) or math.isnan(b):
        return math.nan
    return a if _below(a, b) else b


def _times(a, b):
    return a * b                                                   # (Python floats: 0 * Inf = NaN, no exception)


def _plus(a, b):
    return a + b


MUL = {"plus_times": _times, "min_plus": _plus, "max_plus": _plus, "max_times": _times, "min_max": _omax, "max_min": _omin,
       "or_and": lambda a, b: 1.0 if (a != 0 and b != 0) else 0.0, "plus_pair": lambda a, b: 1.0}
ADD = {"plus_times": _plus, "plus_pair": _plus, "or_and": lambda x, y: 1.0 if (x != 0 or y != 0) else 0.0,
       "min_plus": _omin, "min_max": _omin, "max_plus": _omax, "max_times": _omax, "max_min": _omax}


def _dense_case():
    """40 x 30 x 50, dyadic values (every plus-times sum is exact, so its order does not matter) with +-0, +-Inf, one NaN
    and explicit zeros among the entries."""
    rng = np.random.default_rng(2024)
    m, k, n = 40, 30, 50

    def draw(rows, cols, density):
        has = rng.random((rows, cols)) < density
        val = rng.integers(-12, 13, (rows, cols)) / 4.0
        u = rng.random((rows, cols))
        val[u < 0.06] = 0.0
        val[(u >= 0.06) & (u < 0.12)] = -0.0
        val[(u >= 0.12) & (u < 0.15)] = np.inf
        val[(u >= 0.15) & (u < 0.18)] = -np.inf
        return has, val
    hasA, valA = draw(m, k, 0.2)
    hasB, valB = draw(k, n, 0.2)
    i, j = np.argwhere(hasA)[7]
    valA[i, j] = np.nan

    def csr(has, val):
        rp = np.concatenate([[0], np.cumsum(has.sum(1))]).astype(np.int32)
        rr, cc = np.nonzero(has)
        return rp, cc.astype(np.int32), val[rr, cc]
    return m, k, n, hasA, valA, hasB, valB, csr(hasA, valA), csr(hasB, valB)


@pytest.fixture(scope="module")
def dense_case():
    return _dense_case()


@pytest.mark.parametrize("name", sorted(sr.SEMIRINGS))
def test_reference_matches_a_dense_triple_loop(name, dense_case):
    m, k, n, hasA, valA, hasB, valB, A, B = dense_case
    rng = np.random.default_rng(5)
    Mp, Mj = sr.pattern(m, n, A, B)
    # the mask: the product's pattern and, in every row, a few entries more (some of them land outside it)
    rows = np.concatenate([np.repeat(np.arange(m), np.diff(Mp)), np.repeat(np.arange(m), 3)])
    cols = np.concatenate([Mj, rng.integers(0, n, 3 * m)])
    key = np.unique(rows.astype(np.int64) * n + cols)
    Mp = np.concatenate([[0], np.cumsum(np.bincount(key // n, minlength=m))]).astype(np.int32)
    Mj = (key % n).astype(np.int32)
    want = np.empty(len(Mj))
    mul, add = MUL[name], ADD[name]
    p = 0
    misses = 0
    for i in range(m):
        for q in range(Mp[i], Mp[i + 1]):
            j = Mj[q]
            acc = None
            for kk in range(k):
                if hasA[i, kk] and hasB[kk, j]:
                    v = mul(float(valA[i, kk]), float(valB[kk, j]))
                    acc = v if acc is None else add(acc, v)
            if acc is None:
                acc = sr.identity(name)
                misses += 1
            want[p] = acc
            p += 1
    assert misses > 0
    got = sr.semiring_masked(name, m, n, A, B, Mp, Mj)
    assert np.array_equal(got, want, equal_nan=True)
    ok = ~np.isnan(want)
    assert np.array_equal(np.signbit(got[ok]), np.signbit(want[ok]))
    assert sr.same_bits(got, want)
    if name not in ("or_and", "plus_pair"):
        assert np.isnan(want).any()
    if name in ("min_plus", "min_max", "max_min", "max_times", "plus_times"):
        z = want[ok] == 0
        assert np.signbit(want[ok][z]).any()                       # a -0 came out somewhere
    # the float build's rounding: the reduction commutes with it
    got32 = sr.semiring_masked(name, m, n, A, B, Mp, Mj, dtype=np.float32)
    assert sr.same_bits(got32, want.astype(np.float32))
