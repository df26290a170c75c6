"""CPU tests of the reverse Cuthill-McKee ordering (bhs_csr_rcm_device): the header declares the entry point and the ctypes
list matches it, both libraries export it, the build tracks the new sources and the handle keeps and releases the workspace, a
NULL handle and a handle without a platform are refused, the C++ facade's method compiles and links (tests/rcm;
tests/test_rcm_gpu.py runs the same binary on a GPU), ordering.py and amg.py have the calls; the numpy restatement
(tests/rcmref.py) agrees with an independent serial queue algorithm on every pattern of the GPU tests, refuses what the device
refuses, and shows what the ordering is for on seeded inputs.

The issue's list of facts names "depth 2" for the star of 1024 vertices beside a bandwidth of 1022.  The bandwidth says the
start is a leaf, so the levels are leaf, centre, leaves: 2 is the greatest LEVEL, and the depth as the contract defines it
(the number of levels; 1 for a vertex by itself) is 3.  Both are asserted.  The random graph's figures are this file's seeded
graph's (776 with the refinement, 795 without, 2939 natural), not the issue's 780, 796 and 2976, whose seed is not known."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT
import gridpass as gp
import rcmref as R
import scantiles as st
from test_gs_abi import kinds_of

from benchmark_spgemm_using_csr_amd import _lib

ENTRY = "bhs_csr_rcm_device"
FAMILIES = ("rcm_check", "rcm_components", "rcm_level", "rcm_far", "rcm_order", "rcm_number", "rcm_group")
KERNELS = (b"k_rcm_check", b"k_rcm_start", b"k_rcm_seed", b"k_rcm_init", b"k_rcm_level", b"k_rcm_far_max", b"k_rcm_far_min",
           b"k_rcm_decide", b"k_rcm_roots", b"k_rcm_parent", b"k_rcm_place", b"k_rcm_perm")
FILES = ("bhs_rcm.hip.h", "bhs_host_rcm.inc.h")
DEMO_DIR = os.path.join(ROOT, "tests", "rcm")
FLAGS = (0, R.PERIPHERAL, R.NO_REVERSE, R.PERIPHERAL | R.NO_REVERSE)


# ---------------------------------------------------------------- the interfaces
def test_header_declares_the_entry_point():
    txt = open(_lib.HEADER).read()
    decl = set(re.findall(r"BHS_API\s+[\w\s\*]+?\b(bhs_\w+)\s*\(", txt))
    vp, i = C.c_void_p, C.c_int
    assert ENTRY in decl and ENTRY in _lib.SYMBOLS
    res, args = _lib.SYMBOLS[ENTRY]
    want = ["int" if t is i else "double" if t is C.c_double else "ptr" for t in args]
    assert res is i and kinds_of(txt, ENTRY) == want and len(want) == 14
    assert args[:9] == [vp, i, i, vp, vp, i, vp, vp, vp]
    assert txt.count("/* ---- bandwidth-reducing ordering -") == 1
    at = txt.index("---- bandwidth-reducing ordering")
    sect = txt[at:txt.index("/* ----", at + 1)]
    assert ENTRY in sect
    for fam in FAMILIES:
        assert fam in sect, fam
    assert re.search(r"#define BHS_RCM_PERIPHERAL\s+1\b", sect) and re.search(r"#define BHS_RCM_NO_REVERSE\s+2\b", sect)
    flat = re.sub(r"\s*\n \*\s*", " ", sect)                          # (the comment's line breaks)
    for words in ("alues are NOT TAKEN", "STRICTLY ASCENDING", "STRUCTURALLY SYMMETRIC", "allowed and ignored", "binary search",
                  "nothing stays queued", "George-Liu", "FNROOT", "lockstep", "BHS_ERR_INTERNAL after n + 1 sweeps", "smallest pos",
                  "(pos(p(v)), deg(v), v)", "FOREST ORDER", "stably regrouped by comp", "serial queue algorithm", "OLD index of new row k",
                  "function of the pattern alone", "Only *passes_out is exempt", "A MULTIPLE OF THE BATCH", "never cur", "64-bit atomic maximum",
                  "64-bit atomic minimum", "BHS_ERR_ALLOC", "quadratic in a hub's degree", "profiles/rcm_case.md", "Nothing spins",
                  "n == 0 succeeds", "CAPACITY"):
        assert words in flat, words
    host = open(os.path.join(_lib.CSRC, FILES[1])).read()
    for fam in FAMILIES:
        assert '"%s"' % fam in host, fam


def test_both_libraries_export_the_entry_point(hiplib):
    for path in (_lib.SO_PATH, _lib.SO_PATH_F32):
        raw = C.CDLL(path)
        assert getattr(raw, ENTRY) is not None
        blob = open(path, "rb").read()
        for kern in KERNELS:
            assert kern in blob, (path, kern)


def test_sources_are_tracked_by_the_build():
    mk = open(os.path.join(_lib.CSRC, "Makefile")).read()
    for f in FILES:
        assert f in _lib.SOURCES and f in mk, f
    unit = open(os.path.join(_lib.CSRC, "bhsparse_hip.hip")).read()
    incs = re.findall(r'#include "(bhs_host_\w+\.inc\.h)"', unit)
    assert incs.count("bhs_host_rcm.inc.h") == 1
    assert incs.index("bhs_host_rcm.inc.h") > max(incs.index("bhs_host_components.inc.h"), incs.index("bhs_host_color.inc.h"))
    assert "SideWs rcmWs;" in unit
    cabi = open(os.path.join(_lib.CSRC, "bhs_host_cabi.inc.h")).read()
    assert "release(h->rcmWs)" in cabi
    host = open(os.path.join(_lib.CSRC, FILES[1])).read()
    assert '#include "bhs_rcm.hip.h"' in host and host.count("guarded(h,") == 1 and "BHS_ERR_INTERNAL" in host
    assert "kRcmBatch = 8" in host and host.count("side_passes(") == 2 and host.count("co_order(h,") == 1 and host.count("side_scan(") == 3
    assert "side_open(" in host and "side_aliased(" in host and "side_nothing(" in host and host.count("with_lanes(") == 4
    for kern in ("k_cc_init", "k_cc_pass<L>", "k_cc_flag", "k_cc_clear", "k_cc_number"):
        assert host.count(kern + ",") == 1, kern                     # the components' kernels, launched under this call's record
    assert "ccWs" not in host and "colWs" not in host               # a workspace of its own
    raw = open(os.path.join(_lib.CSRC, FILES[0])).read()
    assert '#include "bhs_components.hip.h"' in raw
    code = re.sub(r"//.*", "", raw)
    assert "asm" not in code
    assert not re.search(r"\bwhile\s*\(|for\s*\(\s*;\s*;\s*\)", code)   # nothing spins: no while at all
    assert len(re.findall(r"__global__", code)) == len(re.findall(r"__global__ __launch_bounds__\(256\)", code)) == len(KERNELS)
    assert "k_cc_pass" not in code and "k_cc_number" not in code and "k_col_count" not in code   # included, not copied
    assert code.count("+= gridDim.x") == len(KERNELS)               # every kernel loops over its blocks: the grids are capped
    assert sorted(set(re.findall(r"\batomic\w+", code))) == ["atomicAdd", "atomicMax", "atomicMin"]
    level = code[code.index("void k_rcm_level"):code.index("void k_rcm_far_max")]
    assert "level[i] = cur + 1;" in level and "atomic" not in level  # plain stores of one value


def test_null_handle_and_missing_platform(hiplib):
    inv = _lib.BHS_ERR_INVALID_ARG
    assert hiplib.bhs_csr_rcm_device(None, 0, 0, None, None, 0, None, None, None, None, None, None, None, None) == inv
    one = (C.c_int * 2)(0, 0)
    out = (C.c_int * 1)(-5)
    counts = (C.c_int * 4)(-5, -5, -5, -5)
    at = lambda k: C.cast(C.byref(counts, 4 * k), C.POINTER(C.c_int))   # noqa: E731
    assert hiplib.bhs_csr_rcm_device(None, 1, 0, one, None, 1, out, None, None, at(0), at(1), at(2), at(3), None) == inv
    assert out[0] == -5 and list(counts) == [-5] * 4
    from benchmark_spgemm_using_csr_amd import facade, ordering
    bh = facade.bhsparse()
    assert ordering.rcm_raw_device(bh, 0, 0, None, None, 0, None, None, None) == _lib.BHS_ERR_NOT_READY
    assert ordering.rcm_raw_device(bh, 1, 0, None, None, 7, None, None, None) == _lib.BHS_ERR_NOT_READY
    for name in ("rcm_ncomp", "rcm_depth", "rcm_sweeps", "rcm_passes", "rcm_ms"):
        assert not hasattr(bh, name), name


def test_python_modules_have_the_calls():
    from benchmark_spgemm_using_csr_amd import amg, ordering
    sig = lambda f: list(inspect.signature(f).parameters)           # noqa: E731
    assert sig(ordering.rcm_raw_device) == ["bh", "n", "nnz", "dSp", "dSj", "flags", "perm", "level", "start"]
    assert sig(ordering.rcm_device) == ["bh", "n", "S", "peripheral", "reverse"]
    assert inspect.signature(ordering.rcm_device).parameters["peripheral"].default is True
    assert inspect.signature(ordering.rcm_device).parameters["reverse"].default is True
    assert sig(ordering.symmetric_pattern_device) == ["bh", "n", "A"]
    assert sig(ordering.bandwidth_profile_device) == ["n", "A", "perm"]
    assert sig(ordering.permute_device) == ["bh", "n", "A", "perm"]
    assert sig(ordering.rcm_csr)[:4] == ["n", "Ap", "Aj", "Ax"]
    assert (ordering.BHS_RCM_PERIPHERAL, ordering.BHS_RCM_NO_REVERSE) == (R.PERIPHERAL, R.NO_REVERSE) == (1, 2)
    assert sig(amg.ilu0_setup_permuted_device) == ["bh", "A", "perm"]
    assert sig(amg.ilu0_pcg_rcm_device) == ["bh", "A", "b", "tol", "maxiter"]
    with pytest.raises(ValueError):                                   # as it was: no "rcm" in ilu0_setup_device
        amg.ilu0_setup_device(None, None, ordering="rcm")


def test_cpp_facade_extension_builds(hiplib):
    src = open(os.path.join(ROOT, "benchmark_spgemm_using_csr_amd", "host", "bhsparse.h")).read()
    flat = re.sub(r"\s+", " ", src)
    assert ("int csr_rcm_device(int n, int nnzS, const index_type *d_rowPtrS, const index_type *d_colIndS, int flags, "
            "index_type *d_perm, index_type *d_level, index_type *d_start, int *ncomp_out, int *depth_out, int *sweeps_out, "
            "int *passes_out);") in flat
    subprocess.check_call(["make", "-C", DEMO_DIR, "-s"])
    demo = os.path.join(DEMO_DIR, "rcm_demo")
    assert os.access(demo, os.X_OK)
    out = subprocess.run(["nm", "-D", "--undefined-only", demo], capture_output=True, text=True).stdout
    assert ENTRY in out
    assert "tests/rcm/rcm_demo" in open(os.path.join(ROOT, ".gitignore")).read().split()
    main = open(os.path.join(DEMO_DIR, "rcm_demo.cpp")).read()
    assert "2317" in main and "PASS" in main and "queue" in main    # a host queue algorithm of its own


# ---------------------------------------------------------------- the restatement
@pytest.fixture(scope="module")
def cases():
    out = dict(R.patterns())
    out["paths3_capped"] = R.disjoint_paths3(gp.cap_rows(1, 1))       # the capped cases of the GPU tests at one CU
    out["cliques_capped"] = R.disjoint_cliques(gp.cap_rows(1, 16))
    return out


@pytest.fixture(scope="module")
def answers(cases):
    return {(name, f): R.rcm(*c, f) for name, c in cases.items() for f in FLAGS}


def test_every_pattern_qualifies(cases):
    import aggref as ar
    for name, c in cases.items():
        assert R.refusal(*c) is None, name
    for name, c in ar.gpu_cases().items():                            # taken as they are, or made canonical
        n, Sp, Sj = cases[name]
        assert n == c[0] and (R.refusal(*c) is not None or (np.array_equal(Sp, c[1]) and np.array_equal(Sj, c[2]))), name


def test_the_restatement_equals_the_serial_queue(cases, answers):
    for name, c in cases.items():
        for f in FLAGS:
            perm, level, start, ncomp, depth, sweeps = answers[name, f]
            sperm, sstart, sncomp, sdepth, ssweeps = R.serial_rcm(*c, f)
            assert np.array_equal(perm, sperm), (name, f)
            assert np.array_equal(start, sstart) and (ncomp, depth, sweeps) == (sncomp, sdepth, ssweeps), (name, f)
            assert perm.dtype == level.dtype == start.dtype == np.int32 and depth == level.max() + 1, (name, f)
            assert np.all(level[start] == 0) and sweeps == (1 if not f & R.PERIPHERAL else sweeps) and sweeps >= 1, (name, f)
            assert sweeps >= 2 or not f & R.PERIPHERAL, (name, f)


def test_every_perm_is_a_permutation_with_contiguous_components(cases, answers):
    for name, (n, Sp, Sj) in cases.items():
        root, comp, ncomp = R.components(n, Sp, Sj)
        for f in FLAGS:
            perm = answers[name, f][0]
            assert np.array_equal(np.sort(perm), np.arange(n)), (name, f)
            c = comp[perm] if f & R.NO_REVERSE else comp[perm[::-1]]
            assert np.all(np.diff(c) >= 0) and answers[name, f][3] == ncomp, (name, f)   # contiguous, ascending by root


def test_the_direction_flag_only_reverses(cases, answers):
    for name in cases:
        for p in (0, R.PERIPHERAL):
            a, b = answers[name, p], answers[name, p | R.NO_REVERSE]
            assert np.array_equal(a[0], b[0][::-1]), (name, p)
            assert np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2]) and a[3:] == b[3:], (name, p)


def test_the_restatement_refuses_what_the_device_refuses():
    n, Sp, Sj = R.grid(5, 4)
    assert R.refusal(n, Sp, Sj) is None
    bad = Sj.copy(); bad[Sp[3]], bad[Sp[3] + 1] = bad[Sp[3] + 1], bad[Sp[3]]   # noqa: E702
    assert R.refusal(n, Sp, bad) == "ascending"
    rep = Sj.copy(); rep[Sp[3] + 1] = rep[Sp[3]]                     # noqa: E702
    assert R.refusal(n, Sp, rep) == "ascending"
    q = int(np.flatnonzero(Sj[Sp[7]:Sp[8]] != 7)[0]) + Sp[7]          # one mirror entry missing
    assert R.refusal(n, np.where(np.arange(n + 1) > 7, Sp - 1, Sp), np.delete(Sj, q)) == "symmetric"
    far = Sj.copy(); far[4] = n                                      # noqa: E702
    assert R.refusal(n, Sp, far) == "column"
    p = Sp.copy(); p[5] = p[6] + 1                                   # noqa: E702
    assert R.refusal(n, p, Sj) == "row pointer" and R.refusal(n, Sp, Sj, nnz=len(Sj) - 1) == "row pointer"
    for broken in ((n, Sp, bad), (n, Sp, rep), (n, Sp, far)):
        with pytest.raises(ValueError):
            R.rcm(*broken)


def band(c, ans):
    return R.bandwidth_profile(*c, ans[0])[0]


def test_what_the_ordering_is_for(cases, answers):
    """the issue's facts, from rcmref (see the module's docstring for the star's depth and the random graph's figures)"""
    P, N = R.PERIPHERAL, 0
    c = cases["shuffled_path"]
    assert c[0] == 2000 and band(c, answers["shuffled_path", P]) == band(c, answers["shuffled_path", N]) == 1
    assert answers["shuffled_path", P][5] == 2 and R.bandwidth_profile(*c)[0] > 1000
    c = cases["shuffled_grid33"]
    assert band(c, answers["shuffled_grid33", P]) == 33 and R.bandwidth_profile(*c)[0] > 900
    c = cases["shuffled_grid20x50"]
    assert band(c, answers["shuffled_grid20x50", P]) == 20 and band(c, answers["shuffled_grid20x50", N]) == 21
    c = R.star(1024)
    perm, level, start, ncomp, depth, sweeps = R.rcm(*c)
    assert c[0] == 1024 and band(c, (perm,)) == 1022 and level.max() == 2 and depth == 3 and level[0] == 1
    c = cases["random3000"]
    a, b = answers["random3000", P], answers["random3000", N]
    natural = R.bandwidth_profile(*c)[0]
    assert a[3] > 200 and a[5] == 3 and 3 * band(c, a) < natural and 3 * band(c, b) < natural
    assert (band(c, a), band(c, b), natural) == (776, 795, 2939)
    c = cases["tree"]
    for f in (P, N):                                                  # from a leaf: 1, 1, 1, 100, 198, 9900, 9900 -- a level that has
        width = np.bincount(answers["tree", f][1])                    # children holds more child counts than one tile of the scan
        assert c[0] == 20101 and answers["tree", f][4] == 7 and width[:-1].max() == 9900 > st.SCAN_TILE, width
    assert R.rcm(0, np.zeros(1, np.int32), np.zeros(0, np.int32))[3:] == (0, 0, 0)
    assert answers["no_entries", P][3:] == (1000, 1, 2) and answers["no_entries", N][3:] == (1000, 1, 1)


def test_bandwidth_and_profile_by_hand():
    """0 - 2, 1 - 2 with diagonals: rows {0, 2}, {1, 2}, {0, 1, 2}: bandwidth 2, profile 0 + 0 + 2; under the order 0, 2, 1
    the rows are {0, 1}, {1, 2} -> new 1 = old 2 holds {0, 1, 2}: bandwidth 1, profile 0 + 1 + 1"""
    n, Sp, Sj = R.from_pairs(3, [0, 1], [2, 2], diag=True)
    assert R.bandwidth_profile(n, Sp, Sj) == (2, 2)
    assert R.bandwidth_profile(n, Sp, Sj, np.array([0, 2, 1])) == (1, 2)
    assert R.bandwidth_profile(0, np.zeros(1, np.int32), np.zeros(0, np.int32)) == (0, 0)
