"""The betweenness centrality (bhs_csr_betweenness_device) case by case: what the call costs from 1 and from 64 sources, how
that splits into the forward and the backward half, beside as many graph.sssp_delta_device breadth-first calls (the forward
half alone: unit weights, one bucket) on the same device and networkx's betweenness_centrality_subset on the host; prints one
JSON line per case.

    python tools/bc_case.py [--no-bfs] [--networkx] [--host-only] [case ...]
        cases: roadlike uniform tri_rmat20 p27_128 (default: all four; tools/sssp_case.py's inputs and the 27-point grid)

Double build (the float build runs the same code).  Per case:
  (a) the matrix holds the in-edges T (an entry (i, j) an edge j -> i, tools/sssp_case.py's reading), G = its transpose by
      the handle; the sources: the first 64 vertices with an out-edge, the first of them alone for the single-source rows;
  (b) the call from 1 source: reached, levels, passes launched, device ms of the call from its event pair (every round trip
      included) and wall ms, median and minimum of REPS runs behind a warm-up with the per-launch timers off; the kernel
      records of one further run with the timers on, and from them the split: forward = bc_seed + bc_expand + bc_count,
      backward = bc_back;
  (c) the call from 64 sources: the same, ONE run behind the warm-up of (b) (a deep graph takes seconds); the records only
      where the sources' levels stay below 4096, since every launch would take an event pair;
  (d) unless --no-bfs: 1 and 64 calls of graph.sssp_delta_device with unit weights and one bucket on the same arrays:
      device ms summed, wall ms;
  (e) with --networkx: networkx.betweenness_centrality_subset from the first source on the host (the graph's construction
      not counted), wall ms, and the greatest relative difference from the call's sums.  --host-only does nothing else and
      needs no GPU."""
import functools
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

from benchmark_spgemm_using_csr_amd import gallery  # noqa: E402
from tools.reduce_case import make as make_other  # noqa: E402

REPS = int(os.environ.get("REPS", "3"))
CASES = ("roadlike", "uniform", "tri_rmat20", "p27_128")
NSRC = 64
RECORD_LEVELS = 4096


@functools.lru_cache(maxsize=None)
def make(case):
    if case not in CASES:
        raise SystemExit("unknown case %s" % case)
    return gallery.roadlike_csr() if case == "roadlike" else make_other(case)


def stat(xs):
    return {"median": float(np.median(xs)), "min": float(np.min(xs))}


def records(bh):
    return {k["name"]: {"ms": round(k["ms"], 4), "launches": k["launches"]} for k in bh.kernel_stats() if k["launches"] > 0}


def split(recs):
    ms = lambda *names: round(sum(recs.get(k, {}).get("ms", 0.0) for k in names), 4)   # noqa: E731
    return {"forward_ms": ms("bc_seed", "bc_expand", "bc_count"), "backward_ms": ms("bc_back"), "check_ms": ms("bc_check")}


def sources_of(n, col):
    """the first NSRC vertices with an out-edge: those that occur as a column"""
    return np.flatnonzero(np.bincount(col, minlength=n) > 0)[:NSRC].astype(np.int32)


def host_networkx(case, got=None):
    import networkx as nx
    rp, col = make(case)
    n = len(rp) - 1
    G = nx.DiGraph()
    G.add_nodes_from(range(n))
    G.add_edges_from(zip(col.tolist(), np.repeat(np.arange(n), np.diff(rp)).tolist()))
    s = int(sources_of(n, col)[0])
    t0 = time.perf_counter()
    want = nx.betweenness_centrality_subset(G, [s], list(range(n)), normalized=False)
    out = {"wall_ms": (time.perf_counter() - t0) * 1e3, "source": s}
    if got is not None:
        want = np.array([want[v] for v in range(n)])
        out["max_rel_diff"] = float(np.max(np.abs(got - want) / np.maximum(np.maximum(got, want), 1e-300)))
    return out


def run(case, bh, dev, opts):
    import torch
    from benchmark_spgemm_using_csr_amd import _lib, graph
    rp, col = make(case)
    n, nnz = len(rp) - 1, len(col)
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)   # noqa: E731
    Tp, Tj = up(rp.astype(np.int32)), up(col.astype(np.int32))
    assert bh.set_option("kernel_stats", 0) == 0
    G = bh.csr_transpose_device(n, n, (Tp, Tj, None), values=False)[:2]
    srcs = sources_of(n, col)
    out = {"case": case, "n": n, "nnz": nnz, "longest_row": int((G[0][1:] - G[0][:-1]).max()), "sources": [int(srcs[0]), len(srcs)],
           "library": os.path.basename(_lib.SO_PATH), "source_digest": _lib.source_digest()}
    src = up(srcs)
    bc = torch.empty(n, dtype=torch.float64, device=dev)
    call = lambda k: graph.betweenness_raw_device(bh, n, nnz, G[0], G[1], nnz, Tp, Tj, k, src, 0, bc, None, None)   # noqa: E731

    def timed(k, reps, warm):
        dev_ms, wall_ms = [], []
        for rep in range(reps + warm):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            assert call(k) == 0
            wall = (time.perf_counter() - t0) * 1e3
            if rep >= warm:
                dev_ms.append(bh.bc_ms)
                wall_ms.append(wall)
        return {"reached": bh.bc_reached, "levels": bh.get_info("bc_levels"), "launched": bh.bc_passes,
                "overflow": bh.get_info("bc_overflow"), "device_ms": stat(dev_ms), "wall_ms": stat(wall_ms)}

    for k, reps, warm in ((1, REPS, 1), (len(srcs), 1, 0)):
        res = timed(k, reps, warm)
        if res["levels"] < RECORD_LEVELS:
            assert bh.set_option("kernel_stats", 1) == 0
            assert call(k) == 0
            res["kernels"] = records(bh)
            res.update(split(res["kernels"]))
            assert bh.set_option("kernel_stats", 0) == 0
        out["sources_%d" % k] = res
        if k == 1:
            first = bc.cpu().numpy()
    if opts["bfs"]:
        Gu = (G[0], G[1], None)
        graph.sssp_delta_device(bh, n, Gu, [int(srcs[0])])            # the warm-up
        for k in (1, len(srcs)):
            torch.cuda.synchronize()
            t0, ms, passes = time.perf_counter(), 0.0, 0
            for s in srcs[:k]:
                graph.sssp_delta_device(bh, n, Gu, [int(s)])
                ms += bh.sssp_ms
                passes += bh.get_info("sssp_work_passes")
            out["bfs_%d" % k] = {"device_ms": ms, "wall_ms": (time.perf_counter() - t0) * 1e3, "passes": passes}
    if opts["networkx"]:
        out["networkx"] = host_networkx(case, first)
    return out


def main():
    args = sys.argv[1:]
    opts = {"bfs": "--no-bfs" not in args, "networkx": "--networkx" in args}
    cases = [a for a in args if not a.startswith("--")] or CASES
    if "--host-only" in args:
        for case in cases:
            print(json.dumps({"case": case, "networkx": host_networkx(case)}), flush=True)
        return
    import torch
    from benchmark_spgemm_using_csr_amd import facade
    dev = torch.device("cuda", 0)
    with facade._handle(np.float64, 0, None) as bh:
        for case in cases:
            print(json.dumps(run(case, bh, dev, opts)), flush=True)


if __name__ == "__main__":
    main()
