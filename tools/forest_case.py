"""The spanning forest (bhs_csr_spanning_forest_device) beside the connected components on the same pattern
(bhs_csr_components_device: the floor, it reads the same entries) and one frontier BFS from vertex 0
(graph.bfs_levels_frontier_device: a spanning tree of one component as a user had it before); measured in one process on the
same arrays; prints one JSON line per case.

    python tools/forest_case.py [case ...]
        cases: poisson27pt_128 poisson5pt_1024 uniform roadlike (default: all four)

Double build.  Per case:
  (a) the call with seeded symmetric weights (a hash of the pair (lo, hi), multiples of 1/1024 below 1024) and with NULL
      values, minimum forest, with and without d_edgeVal: nedges, rounds, device ms of the call from its event pair (the
      rounds' round trips included) after 2 warm-ups, median and minimum of REPS runs, and the kernel records' launches and
      ms of one run;
  (b) the components with the numbering on the same pattern: ncomp, passes, ms the same way;
  (c) one BFS from vertex 0 with a direction per level, the out-edges (the transpose) made beforehand and outside the time:
      levels, steps, the summed device ms of the steps and the wall ms of the loop."""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from benchmark_spgemm_using_csr_amd import _lib, facade, gallery, graph  # noqa: E402

REPS = int(os.environ.get("REPS", "7"))
CASES = ("poisson27pt_128", "poisson5pt_1024", "uniform", "roadlike")


def make(case):
    """(rowPtr, colInd)"""
    if case == "poisson27pt_128":
        return gallery.poisson_csr("poisson27pt", 128, 128, 128)
    if case == "poisson5pt_1024":
        return gallery.poisson_csr("poisson5pt", 1024, 1024)
    if case == "uniform":
        return gallery.uniform_csr(1 << 20, 8)
    if case == "roadlike":
        return gallery.roadlike_csr()
    raise SystemExit("unknown case %s" % case)


def pair_weights(Ap, Aj, n, seed=1):
    """a weight per entry that depends on the unordered pair alone: ((lo * 2654435761 + hi * 40503 + seed) mod 1048573 + 1) / 1024"""
    r = torch.repeat_interleave(torch.arange(n, dtype=torch.int64, device=Ap.device), (Ap[1:] - Ap[:-1]).to(torch.int64))
    c = Aj.to(torch.int64)
    lo, hi = torch.minimum(r, c), torch.maximum(r, c)
    h = (lo * 2654435761 + hi * 40503 + seed) % 1048573
    return (h + 1).to(torch.float64) / 1024.0


def stat(xs):
    return {"median": float(np.median(xs)), "min": float(np.min(xs))}


def run(case, bh, dev):
    rp, col = make(case)
    n, nnz = len(rp) - 1, len(col)
    up = lambda x, dt: torch.from_numpy(np.ascontiguousarray(x, dt)).to(dev)   # noqa: E731
    Ap, Aj = up(rp, np.int32), up(col, np.int32)
    Ax = pair_weights(Ap, Aj, n)
    out = {"case": case, "n": n, "nnz": nnz, "mean_row": nnz / n, "library": os.path.basename(_lib.SO_PATH),
           "source_digest": _lib.source_digest()}
    label, lo, hi = (torch.empty(n, dtype=torch.int32, device=dev) for _ in range(3))
    val = torch.empty(n, dtype=torch.float64, device=dev)
    torch.cuda.synchronize()
    for name, x, v in (("weighted", Ax, val), ("weighted_no_edgeval", Ax, None), ("null_values", None, val)):
        ms, rounds = [], []
        assert bh.set_option("kernel_stats", 0) == 0                  # (no event pair a launch inside the timed span)
        for rep in range(REPS + 2):
            assert graph.spanning_forest_raw_device(bh, n, nnz, Ap, Aj, x, 0, label, lo, hi, v) == 0
            if rep >= 2:
                ms.append(bh.forest_ms)
                rounds.append(bh.forest_rounds)
        assert bh.set_option("kernel_stats", 1) == 0
        assert graph.spanning_forest_raw_device(bh, n, nnz, Ap, Aj, x, 0, label, lo, hi, v) == 0
        ks = [k for k in bh.kernel_stats() if k["launches"] > 0]
        out[name] = {"nedges": bh.forest_nedges, "rounds": sorted(set(rounds)), "ms": stat(ms),
                     "launches": {k["name"]: k["launches"] for k in ks}, "kernels_ms": {k["name"]: round(k["ms"], 4) for k in ks}}
    assert bh.set_option("kernel_stats", 0) == 0

    # (b) the components on the same pattern
    root, comp, size = (torch.empty(n, dtype=torch.int32, device=dev) for _ in range(3))
    ms, passes = [], []
    for rep in range(REPS + 2):
        assert graph.components_raw_device(bh, n, nnz, Ap, Aj, 0, root, comp, size) == 0
        if rep >= 2:
            ms.append(bh.components_ms)
            passes.append(bh.components_passes)
    out["components"] = {"ncomp": bh.components_ncomp, "passes": sorted(set(passes)), "ms": stat(ms)}
    assert out["weighted"]["nedges"] == n - bh.components_ncomp == out["null_values"]["nedges"]

    # (c) one traversal from vertex 0
    A = (Ap, Aj, None)
    Tp, Tj, _, _ = bh.csr_transpose_device(n, n, A, values=False)
    At = (Tp, Tj, None)
    graph._bfs_frontier(bh, n, A, [0], At)                            # warm-up
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    levels, steps, ms, pushes = graph._bfs_frontier(bh, n, A, [0], At)
    torch.cuda.synchronize()
    out["bfs_from_0"] = {"levels": int(levels.max().item()), "reached": int((levels != 0).sum().item()), "steps": steps,
                         "push_steps": pushes, "device_ms": ms, "wall_ms": (time.perf_counter() - t0) * 1e3}
    return out


def main():
    cases = sys.argv[1:] or CASES
    dev = torch.device("cuda", 0)
    with facade._handle(np.float64, 0, None) as bh:
        for case in cases:
            print(json.dumps(run(case, bh, dev)), flush=True)


if __name__ == "__main__":
    main()
