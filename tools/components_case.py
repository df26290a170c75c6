"""The connected components (bhs_csr_components_device) beside what a user had before it: one frontier BFS from vertex 0
(graph.bfs_levels_frontier_device) and, on the road-like graph, plain minimum-label propagation through the MIN_PLUS
semiring SpMV; measured in one process on the same arrays; prints one JSON line per case.

    python tools/components_case.py [case ...]
        cases: roadlike delaunay uniform tri_rmat20 poisson27pt_128 path32768 (default: all six)

Double build (BHSPARSE_HIP_LIB names another build of the same library: the variants of the pass that
profiles/components_case.md compares).  Per case:
  (a) the call with the numbering and the sizes, and for the roots alone: ncomp, passes, device ms of the call from its
      event pair (the batches' round trips included) after 2 warm-ups, median and minimum of REPS runs, and the kernel
      records' ms of one run;
  (b) one BFS from vertex 0 with a direction per level, the out-edges (the transpose) made beforehand and outside the time:
      levels reached, steps, steps by push, the summed device ms of the steps and the wall ms of the loop;
  (c) roadlike only: PROPAGATION_CALLS calls of y = min(y, A min.+ y) on the labels 0 .. n-1 with zero weights, the device ms
      per call, and its extrapolation to the calls that propagation needs -- vertex 0 is the smallest label, so its component
      is labelled after exactly as many calls as the BFS from vertex 0 has levels.  The loop is STOPPED after
      PROPAGATION_CALLS calls; the total is calls x ms per call, not a measurement."""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from benchmark_spgemm_using_csr_amd import _lib, dense, facade, gallery, graph  # noqa: E402

REPS = int(os.environ.get("REPS", "7"))
PROPAGATION_CALLS = 200
CASES = ("roadlike", "delaunay", "uniform", "tri_rmat20", "poisson27pt_128", "path32768")


def make(case):
    """(rowPtr, colInd)"""
    if case == "roadlike":
        return gallery.roadlike_csr()
    if case == "delaunay":
        return gallery.mesh2d_csr(1 << 20)
    if case == "uniform":
        return gallery.uniform_csr(1 << 20, 8)
    if case == "tri_rmat20":
        from tools.reduce_case import make as other
        return other(case)
    if case == "poisson27pt_128":
        return gallery.poisson_csr("poisson27pt", 128, 128, 128)
    if case == "path32768":                                          # the relabelled path of tests/ccref.py
        n = 32768
        p = np.random.default_rng(1).permutation(n)
        src, dst = np.concatenate([p[:-1], p[1:]]), np.concatenate([p[1:], p[:-1]])
        order = np.argsort(src, kind="stable")
        rp = np.zeros(n + 1, np.int64)
        np.cumsum(np.bincount(src, minlength=n), out=rp[1:])
        return rp, dst[order]
    raise SystemExit("unknown case %s" % case)


def stat(xs):
    return {"median": float(np.median(xs)), "min": float(np.min(xs))}


def run(case, bh, dev):
    rp, col = make(case)
    n, nnz = len(rp) - 1, len(col)
    up = lambda x, dt: torch.from_numpy(np.ascontiguousarray(x, dt)).to(dev)   # noqa: E731
    A = (up(rp, np.int32), up(col, np.int32), None)
    out = {"case": case, "n": n, "nnz": nnz, "mean_row": nnz / n, "library": os.path.basename(_lib.SO_PATH),
           "source_digest": _lib.source_digest()}
    root, comp, size = (torch.empty(n, dtype=torch.int32, device=dev) for _ in range(3))
    torch.cuda.synchronize()
    for name, c, s in (("numbered", comp, size), ("roots_alone", None, None)):
        ms, passes = [], []
        assert bh.set_option("kernel_stats", 0) == 0                  # (no event pair a launch inside the timed span)
        for rep in range(REPS + 2):
            assert graph.components_raw_device(bh, n, nnz, A[0], A[1], 0, root, c, s) == 0
            if rep >= 2:
                ms.append(bh.components_ms)
                passes.append(bh.components_passes)
        assert bh.set_option("kernel_stats", 1) == 0
        assert graph.components_raw_device(bh, n, nnz, A[0], A[1], 0, root, c, s) == 0
        out[name] = {"ncomp": bh.components_ncomp, "passes": sorted(set(passes)), "ms": stat(ms),
                     "kernels_ms": {k["name"]: round(k["ms"], 4) for k in bh.kernel_stats() if k["launches"] > 0}}
    sizes = size[:bh.components_ncomp].cpu().numpy()
    out["largest"] = int(sizes.max())
    out["singletons"] = int((sizes == 1).sum())
    assert bh.set_option("kernel_stats", 0) == 0

    # (b) one traversal from vertex 0
    Tp, Tj, _, _ = bh.csr_transpose_device(n, n, A, values=False)
    At = (Tp, Tj, None)
    graph._bfs_frontier(bh, n, A, [0], At)                            # warm-up
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    levels, steps, ms, pushes = graph._bfs_frontier(bh, n, A, [0], At)
    torch.cuda.synchronize()
    out["bfs_from_0"] = {"levels": int(levels.max().item()), "reached": int((levels != 0).sum().item()), "steps": steps,
                         "push_steps": pushes, "device_ms": ms, "wall_ms": (time.perf_counter() - t0) * 1e3}

    # (c) plain minimum-label propagation, stopped and extrapolated
    if case == "roadlike":
        W = (A[0], A[1], torch.zeros(nnz, dtype=torch.float64, device=dev))
        D = torch.arange(n, dtype=torch.float64, device=dev).reshape(n, 1)
        per_call = []
        changed = -1
        for _ in range(PROPAGATION_CALLS):
            D2 = D.clone()
            D2, changed = dense.csr_spmm_semiring_device(bh, "min_plus", n, n, W, D, D2, accumulate=True)
            per_call.append(bh.spmv_ms)
            D = D2
        need = out["bfs_from_0"]["levels"]
        out["min_label_propagation"] = {"calls_run": PROPAGATION_CALLS, "still_changing": int(changed), "ms_per_call": stat(per_call),
                                        "calls_needed_at_least": need, "extrapolated_ms": need * float(np.median(per_call)),
                                        "note": "stopped after calls_run calls; extrapolated_ms = calls_needed_at_least x median ms per call"}
    return out


def main():
    cases = sys.argv[1:] or CASES
    dev = torch.device("cuda", 0)
    with facade._handle(np.float64, 0, None) as bh:
        for case in cases:
            print(json.dumps(run(case, bh, dev)), flush=True)


if __name__ == "__main__":
    main()
