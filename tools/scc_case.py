"""The strongly connected components (bhs_csr_scc_device) beside the connected components on the same pattern
(bhs_csr_components_device: the floor, it reads the same entries and answers the weaker question) and beside scipy's strong
components on the CPU with the copies a user of the device arrays needs; measured in one process on the same arrays; prints one
JSON line per case.

    python tools/scc_case.py [case ...]
        cases: rmat20 weblike uniform roadlike_oneway poisson5pt_1024 ring2048 (default: all six)

Double build (BHSPARSE_HIP_LIB names another build of the same library: the variants of the forward pass's shortcut,
-DBHS_SCC_JUMPS=0 and =2, that profiles/scc_case.md compares).  Per case:
  (a) the call with the numbering and the sizes, and for the roots alone: nscc, rounds, passes, device ms of the call from its
      event pair (every round trip included) after a warm-up, median and minimum of REPS runs, and the kernel records' ms and
      launches per phase of one further run with the timers on;
  (b) bhs_csr_components_device with the numbering on the same arrays, the same way;
  (c) scipy.sparse.csgraph.connected_components(connection="strong") once: the copy of the pattern to the host, the canonical
      matrix (sum_duplicates: scipy does not return on repeated entries), the call, and the copy of the labels back, as wall ms.
The one-way road-like graph keeps every road of gallery.roadlike_csr() and stores ONEWAY of them in one direction only."""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from benchmark_spgemm_using_csr_amd import _lib, facade, gallery, graph  # noqa: E402

REPS = int(os.environ.get("REPS", "5"))
ONEWAY = 0.3
CASES = ("rmat20", "weblike", "uniform", "roadlike_oneway", "poisson5pt_1024", "ring2048")


def from_pairs(n, src, dst):
    order = np.argsort(src, kind="stable")
    rp = np.zeros(n + 1, np.int64)
    np.cumsum(np.bincount(src, minlength=n), out=rp[1:])
    return rp, dst[order]


def make(case):
    """(rowPtr, colInd)"""
    if case == "rmat20":
        return gallery.rmat_csr(scale=20)
    if case == "weblike":
        return gallery.weblike_csr()
    if case == "uniform":
        return gallery.uniform_csr(1 << 20, 8)
    if case == "roadlike_oneway":
        rp, col = gallery.roadlike_csr()
        n = len(rp) - 1
        r = np.repeat(np.arange(n, dtype=np.int64), np.diff(rp))
        col = np.asarray(col, np.int64)
        lo, hi = np.minimum(r, col), np.maximum(r, col)
        h = (lo * 0x9E3779B1 + hi * 0x85EBCA77) & 0xFFFFFFFF         # a road's own number, the same from both ends
        h ^= h >> 15
        h = (h * 0x2C1B3C6D) & 0xFFFFFFFF
        h ^= h >> 12
        oneway = (h & 0xFFFF) < int(ONEWAY * 65536)
        forward = ((h >> 16) & 1) == 1                                # which way a one-way road points
        keep = (r != col) & (~oneway | (forward == (r < col)))
        return from_pairs(n, r[keep], col[keep])
    if case == "poisson5pt_1024":
        return gallery.poisson_csr("poisson5pt", 1024, 1024)
    if case == "ring2048":                                           # the one-way ring of tests/sccref.py
        p = np.random.default_rng(3).permutation(2048)
        return from_pairs(2048, p, np.roll(p, -1))
    raise SystemExit("unknown case %s" % case)


def stat(xs):
    return {"median": float(np.median(xs)), "min": float(np.min(xs))}


def records(bh):
    return {k["name"]: {"ms": round(k["ms"], 4), "launches": k["launches"]} for k in bh.kernel_stats() if k["launches"] > 0}


def run(case, bh, dev):
    rp, col = make(case)
    n, nnz = len(rp) - 1, len(col)
    up = lambda x, dt: torch.from_numpy(np.ascontiguousarray(x, dt)).to(dev)   # noqa: E731
    A = (up(rp, np.int32), up(col, np.int32))
    out = {"case": case, "n": n, "nnz": nnz, "mean_row": nnz / n, "library": os.path.basename(_lib.SO_PATH),
           "source_digest": _lib.source_digest()}
    root, comp, size = (torch.empty(n, dtype=torch.int32, device=dev) for _ in range(3))
    torch.cuda.synchronize()
    for name, c, s in (("numbered", comp, size), ("roots_alone", None, None)):
        ms, passes = [], []
        assert bh.set_option("kernel_stats", 0) == 0                  # (no event pair a launch inside the timed span)
        for rep in range(REPS + 1):
            assert graph.scc_raw_device(bh, n, nnz, A[0], A[1], 0, root, c, s) == 0
            if rep >= 1:
                ms.append(bh.scc_ms)
                passes.append(bh.scc_passes)
        assert bh.set_option("kernel_stats", 1) == 0
        assert graph.scc_raw_device(bh, n, nnz, A[0], A[1], 0, root, c, s) == 0
        out[name] = {"nscc": bh.scc_nscc, "rounds": bh.scc_rounds, "passes": sorted(set(passes)), "ms": stat(ms), "kernels": records(bh)}
    sizes = size[:bh.scc_nscc].cpu().numpy()
    out["largest"] = int(sizes.max())
    out["singletons"] = int((sizes == 1).sum())
    scc_root = root.cpu().numpy().copy()

    # (b) the connected components on the same arrays
    ms, passes = [], []
    assert bh.set_option("kernel_stats", 0) == 0
    for rep in range(REPS + 1):
        assert graph.components_raw_device(bh, n, nnz, A[0], A[1], 0, root, comp, size) == 0
        if rep >= 1:
            ms.append(bh.components_ms)
            passes.append(bh.components_passes)
    out["components"] = {"ncomp": bh.components_ncomp, "passes": sorted(set(passes)), "ms": stat(ms)}

    # (c) scipy on the CPU, with the copies
    import scipy.sparse as sp
    from scipy.sparse.csgraph import connected_components
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    hp, hj = A[0].cpu().numpy(), A[1].cpu().numpy()
    S = sp.csr_matrix((np.ones(len(hj), np.int8), hj, hp), shape=(n, n))
    S.sum_duplicates()
    t1 = time.perf_counter()
    k, lab = connected_components(S, directed=True, connection="strong")
    t2 = time.perf_counter()
    back = torch.from_numpy(lab).to(dev)
    torch.cuda.synchronize()
    t3 = time.perf_counter()
    first = np.full(k, n, np.int64)
    np.minimum.at(first, lab, np.arange(n))
    out["scipy"] = {"nscc": int(k), "copy_and_canonical_ms": (t1 - t0) * 1e3, "call_ms": (t2 - t1) * 1e3, "copy_back_ms": (t3 - t2) * 1e3,
                    "wall_ms": (t3 - t0) * 1e3, "agrees": bool(k == out["numbered"]["nscc"] and np.array_equal(first[lab], scc_root))}
    del back
    return out


def main():
    cases = sys.argv[1:] or CASES
    dev = torch.device("cuda", 0)
    with facade._handle(np.float64, 0, None) as bh:
        for case in cases:
            print(json.dumps(run(case, bh, dev)), flush=True)


if __name__ == "__main__":
    main()
