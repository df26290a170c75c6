"""CPU tests of the heavy-edge matching (bhs_csr_match_device) and the pairwise aggregation on it: the header declares the entry
point in its place and the ctypes list matches it, both libraries export it and hold the kernels, the build tracks the new
sources and the handle keeps and releases the workspace, a NULL handle and a handle without a platform are refused, amg.py
has the calls and every earlier signature as it was, the C++ facade's method compiles and links (tests/match;
tests/test_match_gpu.py runs the same binary on a GPU); the numpy restatement's synchronous rounds (tests/matchref.py) give
the greedy matching of the definition on every pattern of the GPU tests, and the cases written out by hand."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import scipy.sparse as sp

from conftest import ROOT
import aggref as ar
import matchref as mr
from test_gs_abi import kinds_of

from benchmark_spgemm_using_csr_amd import _lib

ENTRY = "bhs_csr_match_device"
FAMILIES = ("match_init", "match_round", "match_number")
FILES = ("bhs_match.hip.h", "bhs_host_match.inc.h")
KERNELS = (b"k_mt_init", b"k_mt_propose", b"k_mt_accept", b"k_mt_finish", b"k_mt_flag", b"k_mt_number")
DEMO_DIR = os.path.join(ROOT, "tests", "match")


# ---------------------------------------------------------------- the interfaces
def test_header_declares_the_entry_point():
    txt = open(_lib.HEADER).read()
    decl = set(re.findall(r"BHS_API\s+[\w\s\*]+?\b(bhs_\w+)\s*\(", txt))
    vp, i = C.c_void_p, C.c_int
    assert ENTRY in decl and ENTRY in _lib.SYMBOLS
    res, args = _lib.SYMBOLS[ENTRY]
    assert res is i and args == [vp, i, i, vp, vp, vp, C.c_uint, i, vp, vp, C.POINTER(i), C.POINTER(i), C.POINTER(C.c_double)]
    want = ["uint" if t is C.c_uint else "int" if t is i else "ptr" for t in args]
    assert kinds_of(txt, ENTRY) == want and len(want) == 13
    sections = re.findall(r"/\* ---- ([^-]+?) -+", txt)
    at = sections.index("matching")
    assert sections[at - 1] == "connected components" and sections[at + 1] == "sparse frontier x CSR"
    start = txt.index("---- matching")
    sect = txt[start:txt.index("/* ----", start + 1)]
    assert ENTRY in sect
    for fam in FAMILIES:
        assert fam in sect, fam
    for words in ("greater than 0", "not NaN", "every weight is 1", "+Inf is a legal weight", "explicit zero", "greatest weight counts",
                  "0x9e3779b9", "0x85ebca6b", "0xc2b2ae35", "mix(mix(lo ^ seed) ^ hi)", "the greater other endpoint wins",
                  "n / 2 rounds", "PROPOSE", "ACCEPT", "eligibility only shrinks", "no atomics touch a result",
                  "function of the input", "n / 2 + 1 rounds", "BHS_ERR_INTERNAL", "mate[mate[i]] == i", "SYMMETRIC", "unique, maximal",
                  "need not be maximal", "ascending leader", "n == 0 succeeds", "Nothing spins", "profiles/match_case.md"):
        assert words in sect, words
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
    assert list(_lib.SOURCES[1:]) == sorted(_lib.SOURCES[1:])
    hdrs = re.search(r"^HDRS = \\\n((?:.*\\\n)*.*)\n", mk, re.M).group(1).replace("\\", " ").split()
    assert hdrs == list(_lib.SOURCES[1:])
    unit = open(os.path.join(_lib.CSRC, "bhsparse_hip.hip")).read()
    incs = re.findall(r'#include "(bhs_host_\w+\.inc\.h)"', unit)
    assert incs[incs.index("bhs_host_components.inc.h") + 1] == "bhs_host_match.inc.h"
    assert incs[-4:] == ["bhs_host_transpose.inc.h", "bhs_host_reduce.inc.h", "bhs_host_semiring.inc.h", "bhs_host_extract.inc.h"]
    assert "SideWs mtWs;" in unit
    cabi = open(os.path.join(_lib.CSRC, "bhs_host_cabi.inc.h")).read()
    assert "release(h->mtWs)" in cabi
    host = open(os.path.join(_lib.CSRC, FILES[1])).read()
    assert '#include "bhs_match.hip.h"' in host and host.count("guarded(h,") == 1 and "BHS_ERR_INTERNAL" in host
    assert host.count("side_scan(") == 1 and "d.n / 2 + 1" in host    # the library's scan, called; the cap on the rounds
    code = re.sub(r"//.*", "", open(os.path.join(_lib.CSRC, FILES[0])).read())
    assert "asm" not in code and "__shared__ rd_u64 sCount;" in code and code.count("__shared__") == 1
    assert not re.search(r"\bwhile\s*\(|for\s*\(\s*;\s*;\s*\)", code)    # nothing spins
    assert len(re.findall(r"__global__", code)) == len(re.findall(r"__global__ __launch_bounds__\(256\)", code)) == len(KERNELS)
    assert "lane_xor64<S>" in code and "atomic" not in code           # (the count's adds are smv_count's)
    # propose reads the mates and writes the candidates, accept reads the candidates and writes the vertex's own mate
    propose = code[code.index("void k_mt_propose"):code.index("void k_mt_accept")]
    accept = code[code.index("void k_mt_accept"):code.index("void k_mt_finish")]
    assert "const int* __restrict__ mate" in propose and not re.search(r"mate\s*\[[^\]]*\]\s*=[^=]", propose)
    assert "const int* __restrict__ cand" in accept and re.findall(r"mate\s*\[([^\]]*)\]\s*=[^=]", accept) == ["i", "i"]
    assert propose.index("(unsigned)j >= (unsigned)d.n") < propose.index("mate[j]")   # the range check comes first


def test_null_handle_and_missing_platform(hiplib):
    inv = _lib.BHS_ERR_INVALID_ARG
    assert hiplib.bhs_csr_match_device(None, 0, 0, None, None, None, 0, 0, None, None, None, None, None) == inv
    one = (C.c_int * 2)(0, 0)
    out = (C.c_int * 1)(-5)
    assert hiplib.bhs_csr_match_device(None, 1, 0, one, None, None, 0, 0, out, None, None, None, None) == inv and out[0] == -5
    from benchmark_spgemm_using_csr_amd import amg, facade
    bh = facade.bhsparse()
    assert amg.match_raw_device(bh, 0, 0, None, None, None, 0, 0, None, None) == _lib.BHS_ERR_NOT_READY
    assert amg.match_raw_device(bh, 1, 0, None, None, None, 0, 1, None, None) == _lib.BHS_ERR_NOT_READY
    assert not hasattr(bh, "match_npairs") and not hasattr(bh, "match_rounds") and not hasattr(bh, "match_ms")


def test_python_module_has_the_calls():
    from benchmark_spgemm_using_csr_amd import amg, graph
    sig = lambda f: list(inspect.signature(f).parameters)           # noqa: E731
    defaults = lambda f: {k: v.default for k, v in inspect.signature(f).parameters.items()   # noqa: E731
                          if v.default is not inspect.Parameter.empty}
    assert sig(amg.match_raw_device) == ["bh", "n", "nnzA", "d_rowPtrA", "d_colIndA", "d_valA", "seed", "flags", "d_mate", "d_agg"]
    assert sig(amg.match_device) == ["bh", "n", "A", "seed"] and defaults(amg.match_device) == {"seed": 0}
    assert sig(amg.match_csr) == ["n", "Ap", "Aj", "Ax", "seed", "value_dtype", "device"]
    assert sig(amg.pairwise_aggregate_device) == ["handles", "n", "A", "passes", "seed"]
    assert defaults(amg.pairwise_aggregate_device) == {"passes": 2, "seed": 0}
    assert sig(amg.pa_setup_device) == ["handles", "n", "A", "passes", "omega", "max_levels", "min_coarse", "seed"]
    assert defaults(amg.pa_setup_device) == {"passes": 3, "omega": 2.0 / 3.0, "max_levels": 10, "min_coarse": 40, "seed": 0}
    assert sig(amg.pa_setup_csr) == ["n", "Ap", "Aj", "Ax", "passes", "omega", "max_levels", "min_coarse", "seed", "value_dtype", "device"]
    # as they were
    assert sig(amg.sa_setup_device) == ["handles", "n", "A", "theta", "omega", "max_levels", "min_coarse", "seed"]
    assert defaults(amg.sa_setup_device) == {"theta": 0.0, "omega": 2.0 / 3.0, "max_levels": 10, "min_coarse": 40, "seed": 0}
    assert sig(amg.aggregate_device) == ["bh", "n", "S", "seed", "prio"] and sig(amg.galerkin_device) == ["h1", "h2", "n", "nc", "A", "P"]
    assert sig(amg.pcg_device) == ["bh", "levels", "b", "tol", "maxiter", "smoother"]
    assert sig(graph.components_device) == ["bh", "n", "A"]
    assert "_setup_levels(" in inspect.getsource(amg.sa_setup_device) and "_setup_levels(" in inspect.getsource(amg.pa_setup_device)
    assert "pairwise" in amg.__doc__ and "bhs_csr_match_device" in amg.__doc__


def test_cpp_facade_extension_builds(hiplib):
    src = open(os.path.join(ROOT, "benchmark_spgemm_using_csr_amd", "host", "bhsparse.h")).read()
    flat = re.sub(r"\s+", " ", src)
    assert ("int csr_match_device(int n, int nnzA, const index_type *d_rowPtrA, const index_type *d_colIndA, "
            "const value_type *d_valA, unsigned seed, int flags, index_type *d_mate, index_type *d_agg, int *npairs_out, "
            "int *rounds_out);") in flat
    subprocess.check_call(["make", "-C", DEMO_DIR, "-s"])
    demo = os.path.join(DEMO_DIR, "match_demo")
    assert os.access(demo, os.X_OK)
    out = subprocess.run(["nm", "-D", "--undefined-only", demo], capture_output=True, text=True).stdout
    assert ENTRY in out
    assert "tests/match/match_demo" in open(os.path.join(ROOT, ".gitignore")).read().split()


# ---------------------------------------------------------------- the restatement
def check_greedy(name, n, Ap, Aj, Ax, seed):
    mate, npairs, nrounds = mr.rounds(n, Ap, Aj, Ax, seed)
    assert mr.is_matching(mate) and np.array_equal(mate, mr.greedy(n, Ap, Aj, Ax, seed)), (name, seed)
    assert npairs == int((mate > np.arange(n)).sum()) and nrounds <= 7, (name, seed, nrounds)
    # maximal: no edge with both ends unmatched
    r, c, _ = mr.seen_edges(n, Ap, Aj, Ax)
    alone = mate == np.arange(n)
    assert not np.any(alone[r] & alone[c]), (name, seed)
    agg, nagg = mr.number(mate)
    assert nagg == n - npairs and mr.numbered_by_smallest_member(agg, nagg) and np.bincount(agg, minlength=nagg).max(initial=0) <= 2
    return nrounds


def test_the_rounds_give_the_greedy_matching():
    """on every pattern of aggref.gpu_cases() with unit weights and on uniform2048 with integer weights 1 .. 4, seeds 0 and 1:
    at most 7 productive rounds"""
    cases = ar.gpu_cases()
    assert len(cases) == 12
    for name, (n, Ap, Aj) in cases.items():
        for seed in (0, 1):
            check_greedy(name, n, Ap, Aj, None, seed)
    n, Ap, Aj = cases["uniform2048"]
    Ax = mr.integer_weights(n, Ap, Aj)
    assert set(np.unique(Ax)) == {1.0, 2.0, 3.0, 4.0}
    A = sp.csr_matrix((Ax, Aj, Ap), shape=(n, n))
    assert (A != A.T).nnz == 0
    for seed in (0, 1):
        check_greedy("uniform2048 weighted", n, Ap, Aj, Ax, seed)
    assert not np.array_equal(mr.rounds(n, Ap, Aj, Ax, 0)[0], mr.rounds(n, Ap, Aj, None, 0)[0])   # the weights count


def test_the_increasing_path_is_the_worst_case():
    n, Ap, Aj, Ax = mr.increasing_path(200)
    mate, npairs, nrounds = mr.rounds(n, Ap, Aj, Ax, 0)
    assert (npairs, nrounds) == (100, 100) and np.array_equal(mate, np.arange(200) ^ 1)
    assert np.array_equal(mate, mr.greedy(n, Ap, Aj, Ax, 0))
    # equal weights: the hash in front of the indices keeps the rounds few
    assert mr.rounds(n, Ap, Aj, None, 0)[2] <= 7


def test_four_vertices_by_hand():
    """rows {(0,1) NaN, (0,2) 0, (0,3) +Inf}, {(1,0) NaN, (1,2) -2}, {(2,0) -0, (2,1) 2}, {(3,0) -Inf}"""
    n, Ap, Aj, Ax = mr.by_hand()
    assert Ap.tolist() == [0, 3, 5, 7, 8] and Aj.tolist() == [1, 2, 3, 0, 2, 0, 1, 0]
    assert np.isnan(Ax[0]) and Ax[1] == 0 and Ax[2] == np.inf and np.isnan(Ax[3]) and Ax[4] == -2 and np.signbit(Ax[5]) and Ax[5] == 0
    for seed in (0, 1, 77):
        mate, agg, nagg, npairs, nrounds = mr.match(n, Ap, Aj, Ax, seed)
        assert mate.tolist() == [3, 2, 1, 0] and (npairs, nrounds, nagg) == (2, 1, 2) and agg.tolist() == [0, 1, 1, 0]
    assert mr.match(0, np.zeros(1, np.int32), np.zeros(0, np.int32))[2:] == (0, 0, 0)


def test_the_directed_triangle_matches_nothing():
    n, Ap, Aj, Ax = mr.directed_triangle()
    mate, agg, nagg, npairs, nrounds = mr.match(n, Ap, Aj, Ax, 0)
    assert mate.tolist() == [0, 1, 2] and agg.tolist() == [0, 1, 2] and (nagg, npairs, nrounds) == (3, 0, 0)


def test_asymmetric_weights_give_a_valid_matching():
    n, Ap, Aj = ar.gpu_cases()["poisson5pt_33"]
    Ax = mr.asymmetric_weights(n, Ap, Aj)
    A = sp.csr_matrix((Ax, Aj, Ap), shape=(n, n))
    assert (A != A.T).nnz > 0
    mate, npairs, nrounds = mr.rounds(n, Ap, Aj, Ax, 0)
    assert mr.is_matching(mate) and npairs > n // 4 and nrounds >= 1
    assert np.all((A[np.arange(n), mate.astype(np.int64)] != 0) | (mate == np.arange(n)))   # a partner is a neighbour
    # stored twice and shuffled: of a repeated entry the greatest weight counts, the order inside a row does not
    Ax = mr.integer_weights(n, Ap, Aj)
    m2, Bp, Bj, Bx = mr.unsorted_with_repeats(n, Ap, Aj, Ax)
    assert len(Bj) == 2 * len(Aj) and np.any(np.diff(Bj[Bp[5]:Bp[6]]) < 0)
    assert np.array_equal(mr.rounds(m2, Bp, Bj, Bx, 0)[0], mr.rounds(n, Ap, Aj, Ax, 0)[0])


def test_pairs_follow_the_strong_direction():
    """anisotropic 64 x 64 (eps = 1e-2): with the entries below 0.25 zeroed every pair is along x; two passes on the unfiltered
    matrix give aggregates of at most 4, numbered by ascending smallest member"""
    A = mr.aniso(64, 64, 1e-2)
    n = A.shape[0]
    F = A.copy()
    F.data[np.abs(F.data) < 0.25] = 0.0                              # explicit zeros: no connection
    assert F.nnz == A.nnz
    mate, npairs, _ = mr.rounds(n, F.indptr, F.indices, F.data, 0)
    paired = mate != np.arange(n)
    assert npairs > 0.4 * n and np.all(np.abs(mate[paired] - np.arange(n)[paired]) == 1)
    assert np.all(mate[paired] // 64 == np.arange(n)[paired] // 64)
    for passes in (1, 2, 3):
        agg, nagg = mr.pairwise(A, passes, 0)
        sizes = np.bincount(agg, minlength=nagg)
        assert sizes.min() >= 1 and sizes.max() <= 2 ** passes and mr.numbered_by_smallest_member(agg, nagg), passes
    agg, nagg = mr.pairwise(A, 2, 0)
    assert np.bincount(agg).max() == 4 and nagg < 0.32 * n
