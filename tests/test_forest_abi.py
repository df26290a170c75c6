"""CPU tests of the spanning forest (bhs_csr_spanning_forest_device): the header declares the entry point and the two flags in
its section and the ctypes list matches it, both libraries export it and hold the kernels, the build tracks the new sources
and the handle keeps and releases the workspace, a NULL handle and a handle without a platform are refused with the outputs
untouched, graph.py has the calls and every earlier signature as it was, the C++ facade's method compiles and links
(tests/forest; tests/test_forest_gpu.py runs the same binary on a GPU); the numpy restatement's synchronous rounds
(tests/forestref.py) give Kruskal's forest on every input of the GPU tests and on 200 random multigraphs, Kruskal's total
weight is scipy's, and the case written out by hand holds."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import scipy.sparse as sp
from scipy.sparse.csgraph import minimum_spanning_tree

from conftest import ROOT
import ccref
import forestref as fr
from test_gs_abi import kinds_of

from benchmark_spgemm_using_csr_amd import _lib

ENTRY = "bhs_csr_spanning_forest_device"
FAMILIES = ("forest_pick", "forest_hook", "forest_list")
FILES = ("bhs_forest.hip.h", "bhs_host_forest.inc.h")
KERNELS = (b"k_sf_init", b"k_sf_clear", b"k_sf_weight", b"k_sf_edge", b"k_sf_hook", b"k_sf_jump", b"k_sf_relabel", b"k_sf_flag",
           b"k_sf_write")
DEMO_DIR = os.path.join(ROOT, "tests", "forest")


# ---------------------------------------------------------------- the interfaces
def test_header_declares_the_entry_point():
    txt = open(_lib.HEADER).read()
    decl = set(re.findall(r"BHS_API\s+[\w\s\*]+?\b(bhs_\w+)\s*\(", txt))
    vp, i = C.c_void_p, C.c_int
    assert ENTRY in decl and ENTRY in _lib.SYMBOLS
    res, args = _lib.SYMBOLS[ENTRY]
    assert res is i and args == [vp, i, i, vp, vp, vp, i, vp, vp, vp, vp, C.POINTER(i), C.POINTER(i), C.POINTER(C.c_double)]
    want = ["int" if t is i else "ptr" for t in args]
    assert kinds_of(txt, ENTRY) == want and len(want) == 14
    sections = re.findall(r"/\* ---- ([^-]+?) -+", txt)
    at = sections.index("spanning forest")
    assert sections[at + 1] == "connected components" and sections[at + 2] == "matching"
    start = txt.index("---- spanning forest")
    sect = txt[start:txt.index("/* ----", start + 1)]
    assert ENTRY in sect and "enum { BHS_FOREST_MAXIMUM = 1, BHS_FOREST_ABS = 2 };" in sect
    assert (_lib.BHS_FOREST_MAXIMUM, _lib.BHS_FOREST_ABS) == (1, 2)
    for fam in FAMILIES:
        assert fam in sect, fam
    for words in ("not NaN", "multigraph","|a_ij| under BHS_FOREST_ABS", "1 where d_valA == NULL", "explicit zeros are legal",
                  "how often, an edge is stored", "(k(w), lo, hi)", "rd_key(x, false)", "-0 below +0", "widened exactly",
                  "complement of both words", "Kruskal's algorithm", "unique for ANY input", "the lightest weight counts",
                  "n - (number of weak components)", "atomicMin", "label[i] != label[j]", "lo << 32 | hi", "agent-scope relaxed load",
                  "a mutual pair", "the smaller of c and d stays a root", "SLOT c", "hooked at most once",
                  "ceil(log2 R)", "parent[parent[l]] != parent[l]", "BHS_ERR_INTERNAL", "floor(log2 n)", "33rd round",
                  "Nothing spins", "no floating atomics", "label[label[i]] == label[i]", "ascending slot order", "lo < hi",
                  "the weight as compared", "n == 0 succeeds", "profiles/forest_case.md"):
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
    assert incs[incs.index("bhs_host_match.inc.h") + 1] == "bhs_host_forest.inc.h"
    assert incs[-4:] == ["bhs_host_transpose.inc.h", "bhs_host_reduce.inc.h", "bhs_host_semiring.inc.h", "bhs_host_extract.inc.h"]
    assert "SideWs sfWs;" in unit
    cabi = open(os.path.join(_lib.CSRC, "bhs_host_cabi.inc.h")).read()
    assert "release(h->sfWs)" in cabi
    host = open(os.path.join(_lib.CSRC, FILES[1])).read()
    assert '#include "bhs_forest.hip.h"' in host and host.count("guarded(h,") == 1 and "BHS_ERR_INTERNAL" in host
    assert host.count("side_scan(") == 1 and "kSfMaxRounds = 32" in host   # the library's scan, called; the cap on the rounds
    code = re.sub(r"//.*", "", open(os.path.join(_lib.CSRC, FILES[0])).read())
    assert '#include "bhs_components.hip.h"' in code and "asm" not in code
    assert "__shared__ rd_u64 sCount;" in code and code.count("__shared__") == 1
    assert not re.search(r"\bwhile\s*\(|for\s*\(\s*;\s*;\s*\)", code)    # nothing spins
    assert len(re.findall(r"__global__", code)) == len(re.findall(r"__global__ __launch_bounds__\(256\)", code)) == len(KERNELS)
    # the only atomics: the 64-bit minimum behind its guard, and the relaxed loads (the count's adds are smv_count's)
    assert re.findall(r"\batomic\w+", code) == ["atomicMin"] and "if (sf_load(p) > v) (void)atomicMin(p, v);" in code
    assert "(double*)" not in code and "atomicAdd" not in code
    # the picks read the labels and lower the trees' words; the hook writes parent and the slots, never a label; the relabel
    # writes the vertex's own label
    weight = code[code.index("void k_sf_weight"):code.index("void k_sf_edge")]
    edge = code[code.index("void k_sf_edge"):code.index("void k_sf_hook")]
    hook = code[code.index("void k_sf_hook"):code.index("void k_sf_jump")]
    relabel = code[code.index("void k_sf_relabel"):code.index("void k_sf_flag")]
    for part in (weight, edge, hook):
        assert "const int* __restrict__ label" in part and not re.search(r"label\s*\[[^\]]*\]\s*=[^=]", part)
    assert "const rd_u64* __restrict__ bestW" in edge and "const rd_u64* __restrict__ bestE" in hook
    assert re.findall(r"parent\s*\[([^\]]*)\]\s*=[^=]", hook) == ["c"] and re.findall(r"slotLo\s*\[([^\]]*)\]\s*=[^=]", hook) == ["c"]
    assert re.findall(r"label\s*\[([^\]]*)\]\s*=[^=]", relabel) == ["i"] and "const int* __restrict__ parent" in relabel
    for part in (weight, edge):
        assert part.index("(unsigned)j >= (unsigned)d.n") < part.index("label[j]")   # the range check comes first


def test_null_handle_and_missing_platform(hiplib):
    inv = _lib.BHS_ERR_INVALID_ARG
    fn = hiplib.bhs_csr_spanning_forest_device
    assert fn(None, 0, 0, None, None, None, 0, None, None, None, None, None, None, None) == inv
    one = (C.c_int * 2)(0, 0)
    outs = [(C.c_int * 1)(-5) for _ in range(3)]
    val = (C.c_double * 1)(-5.0)
    cnt, rounds, ms = C.c_int(-5), C.c_int(-5), C.c_double(-5.0)
    assert fn(None, 1, 0, one, None, None, 0, outs[0], outs[1], outs[2], val, C.byref(cnt), C.byref(rounds), C.byref(ms)) == inv
    assert [o[0] for o in outs] == [-5] * 3 and val[0] == -5.0 and (cnt.value, rounds.value, ms.value) == (-5, -5, -5.0)
    from benchmark_spgemm_using_csr_amd import facade, graph
    bh = facade.bhsparse()
    assert graph.spanning_forest_raw_device(bh, 0, 0, None, None, None, 0, None, None, None, None) == _lib.BHS_ERR_NOT_READY
    assert graph.spanning_forest_raw_device(bh, 1, 0, None, None, None, 4, None, None, None, None) == _lib.BHS_ERR_NOT_READY
    assert not hasattr(bh, "forest_nedges") and not hasattr(bh, "forest_rounds") and not hasattr(bh, "forest_ms")


def test_python_module_has_the_calls():
    from benchmark_spgemm_using_csr_amd import amg, graph
    sig = lambda f: list(inspect.signature(f).parameters)           # noqa: E731
    defaults = lambda f: {k: v.default for k, v in inspect.signature(f).parameters.items()   # noqa: E731
                          if v.default is not inspect.Parameter.empty}
    assert sig(graph.spanning_forest_raw_device) == ["bh", "n", "nnzA", "d_rowPtrA", "d_colIndA", "d_valA", "flags", "d_label",
                                                     "d_edgeLo", "d_edgeHi", "d_edgeVal"]
    assert sig(graph.spanning_forest_device) == ["bh", "n", "A", "maximum", "absolute"]
    assert defaults(graph.spanning_forest_device) == {"maximum": False, "absolute": False}
    assert sig(graph.forest_csr_device) == ["n", "lo", "hi", "w"]
    assert sig(graph.spanning_forest_csr) == ["n", "Ap", "Aj", "Ax", "maximum", "absolute", "value_dtype", "device"]
    assert sig(graph.single_linkage_device) == ["bh", "n", "A", "nclusters"]
    # as they were
    assert sig(graph.components_raw_device) == ["bh", "n", "nnz", "dAp", "dAj", "flags", "root", "comp", "size"]
    assert sig(graph.components_device) == ["bh", "n", "A"] and sig(graph.components_csr) == ["n", "Ap", "Aj", "device"]
    assert sig(graph.component_lists_device) == ["bh", "n", "comp", "ncomp"]
    assert sig(graph.bfs_levels_frontier_device) == ["bh", "n", "A", "sources", "At", "push_below"]
    assert sig(amg.match_device) == ["bh", "n", "A", "seed"]
    assert "spanning forest" in graph.__doc__ and ENTRY in graph.__doc__
    assert "components_device(" in inspect.getsource(graph.single_linkage_device)
    assert "torch.argsort" in inspect.getsource(graph.spanning_forest_device)


def test_cpp_facade_extension_builds(hiplib):
    src = open(os.path.join(ROOT, "benchmark_spgemm_using_csr_amd", "host", "bhsparse.h")).read()
    flat = re.sub(r"\s+", " ", src)
    assert ("int csr_spanning_forest_device(int n, int nnzA, const index_type *d_rowPtrA, const index_type *d_colIndA, "
            "const value_type *d_valA, int flags, index_type *d_label, index_type *d_edgeLo, index_type *d_edgeHi, "
            "value_type *d_edgeVal, int *nedges_out, int *rounds_out);") in flat
    subprocess.check_call(["make", "-C", DEMO_DIR, "-s"])
    demo = os.path.join(DEMO_DIR, "forest_demo")
    assert os.access(demo, os.X_OK)
    out = subprocess.run(["nm", "-D", "--undefined-only", demo], capture_output=True, text=True).stdout
    assert ENTRY in out
    assert "tests/forest/forest_demo" in open(os.path.join(ROOT, ".gitignore")).read().split()


# ---------------------------------------------------------------- the restatement
def log2_floor(n):
    return int(n).bit_length() - 1 if n > 1 else 0


def check_forest(what, n, Ap, Aj, Ax, flags):
    """the rounds give Kruskal's forest, weights bit for bit; the labels are its trees; the rounds stay below the bound"""
    label, lo, hi, w, nedges, nrounds, info = fr.sync_rounds(n, Ap, Aj, Ax, flags)
    klo, khi, kw = fr.kruskal(n, Ap, Aj, Ax, flags)
    glo, ghi, gw = fr.by_lo_hi(lo.astype(np.int64), hi.astype(np.int64), w)
    assert np.array_equal(glo, klo) and np.array_equal(ghi, khi) and fr.bits(gw) == fr.bits(kw), what
    assert nedges == len(klo) and np.all(lo < hi) and nrounds <= log2_floor(n), (what, nrounds)
    assert np.array_equal(label[label], label), what
    root = ccref.components(n, *_edge_pattern(n, Ap, Aj, Ax, flags))[0] if n else np.zeros(0, np.int32)
    assert fr.same_partition(label, root) and nedges == n - len(np.unique(root)), what
    assert all(j <= a for j, a in zip(info["jumps"], info["allowed"])), (what, info)
    return nrounds, info


def _edge_pattern(n, Ap, Aj, Ax, flags):
    """the pattern of the entries that are edges (a NaN is none)"""
    r, c, _, _ = fr.edges(n, Ap, Aj, Ax, flags)
    return ccref.from_edges(n, r, c)


def test_the_rounds_give_kruskals_forest_on_the_gpu_inputs():
    for name in fr.PATTERNS:
        n, Ap, Aj = fr.pattern(name)
        for maker in fr.MAKERS:
            for flags in fr.FLAGS:
                check_forest((name, maker, flags), n, Ap, Aj, fr.weights(name, maker), flags)
    n, Ap, Aj = fr.pattern("uniform2048")
    A = sp.csr_matrix((fr.weights("uniform2048", "distinct"), Aj, Ap), shape=(n, n))
    assert (A != A.T).nnz == 0
    A = sp.csr_matrix((fr.weights("uniform2048", "asymmetric"), Aj, Ap), shape=(n, n))
    assert (A != A.T).nnz > 0
    w = fr.weights("uniform2048", "specials")
    assert np.isnan(w).any() and np.isinf(w).any() and np.any((w == 0) & np.signbit(w)) and np.any((w == 0) & ~np.signbit(w))
    for maker in ("distinct", "ties", "asymmetric", "specials"):      # exact in float
        w = fr.weights("powerlaw3000", maker)
        assert fr.bits(w.astype(np.float32).astype(np.float64)) == fr.bits(w), maker
    # the flags count
    assert len({fr.reference("uniform2048", "specials", f)[1].tobytes() for f in fr.FLAGS}) == 4


def test_the_rounds_give_kruskals_forest_on_random_multigraphs():
    rng = np.random.default_rng(2024)
    seen = 0
    for t in range(200):
        n, Ap, Aj, Ax = fr.random_multigraph(rng)
        for flags in fr.FLAGS:
            seen += check_forest((t, flags), n, Ap, Aj, Ax, flags)[0]
        check_forest((t, "no values"), n, Ap, Aj, None, 0)
    assert seen > 800                                                # (most of them take more than one round)


def test_kruskal_agrees_with_scipy():
    """total weight on symmetric inputs with distinct positive weights (scipy's csgraph takes an explicit zero for no edge and
    breaks ties its own way, so only the weight of a forest with distinct positive weights is comparable)"""
    for name in ("poisson5pt_33", "poisson27pt_9", "uniform2048", "powerlaw3000", "two_k70"):
        n, Ap, Aj = fr.pattern(name)
        w = fr.weights(name, "distinct")
        assert w.min() > 0
        A = sp.csr_matrix((w.copy(), Aj.copy(), Ap.copy()), shape=(n, n))   # (setdiag works in place: not on the shared arrays)
        A.setdiag(0)
        A.eliminate_zeros()
        T = minimum_spanning_tree(A)
        lo, hi, kw = fr.kruskal(n, Ap, Aj, w, 0)
        assert len(lo) == T.nnz and kw.sum() == T.sum(), name
        Tmax = minimum_spanning_tree(-A)
        assert fr.kruskal(n, Ap, Aj, w, fr.MAXIMUM)[2].sum() == -Tmax.sum(), name


def test_the_case_by_hand():
    n, Ap, Aj, Ax = fr.by_hand()
    assert n == 6 and Ap.tolist() == [0, 2, 4, 6, 8, 8, 9] and Aj.tolist() == [1, 4, 0, 2, 3, 4, 2, 4, 5]
    assert np.isnan(Ax[4]) and Ax[5] == 0 and not np.signbit(Ax[5]) and Ax[6] == 0 and np.signbit(Ax[6]) and Ax[8] == -7
    label, lo, hi, w, nedges, nrounds, info = fr.sync_rounds(n, Ap, Aj, Ax, 0)
    assert (nedges, nrounds) == (4, 2) and info["hooks"] == [3, 1]   # 1 -> 0, 3 -> 2, 4 -> 2; then 2 -> 0
    assert list(zip(lo.tolist(), hi.tolist(), w.tolist())) == [(0, 1, 2.0), (0, 4, 2.0), (2, 3, 0.0), (2, 4, 0.0)]
    assert np.signbit(w).tolist() == [False, False, True, False]      # (2, 3, -0) before (2, 4, +0)
    assert label.tolist() == [0, 0, 0, 0, 0, 5]
    label, lo, hi, w, nedges, nrounds, _ = fr.sync_rounds(n, Ap, Aj, Ax, fr.MAXIMUM)
    assert sorted(zip(lo.tolist(), hi.tolist(), w.tolist())) == [(0, 1, 5.0), (0, 4, 2.0), (1, 2, 2.0), (3, 4, 1.0)]
    assert label.tolist()[5] == 5 and len(set(label.tolist()[:5])) == 1
    for flags in fr.FLAGS:
        check_forest(("by hand", flags), n, Ap, Aj, Ax, flags)
    empty = fr.sync_rounds(0, np.zeros(1, np.int32), np.zeros(0, np.int32))
    assert empty[4:6] == (0, 0) and len(empty[0]) == 0


def test_the_increasing_path_is_one_round_and_a_deep_chain():
    n, Ap, Aj, Ax = fr.increasing_path()
    label, lo, hi, w, nedges, nrounds, info = fr.sync_rounds(n, Ap, Aj, Ax, 0)
    assert (n, nedges, nrounds) == (300, 299, 1) and info["jumps"] == [9] and info["allowed"] == [9]
    assert np.all(label == 0) and np.array_equal(lo, np.arange(299)) and np.array_equal(hi, np.arange(1, 300))
    check_forest("increasing path", n, Ap, Aj, Ax, 0)
    # the key: -0 below +0, the order of the numbers, and back
    x = np.array([-np.inf, -3.0, -0.0, 0.0, 0.25, 7.0, np.inf])
    k = fr.weight_key(x)
    assert np.all(k[1:] > k[:-1]) and fr.bits(fr.weight_unkey(k)) == fr.bits(x)
