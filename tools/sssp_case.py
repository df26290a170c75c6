"""The shortest paths in one call (bhs_csr_sssp_device) case by case: what the call costs at five bucket widths, beside
graph.sssp_frontier_device (a Python loop of semiring calls, one host round trip a round) on the same device and scipy's
dijkstra on the host; measured in one process on the same arrays; prints one JSON line per (case, weights).

    python tools/sssp_case.py [--no-frontier] [--no-scipy] [case ...]
        cases: roadlike uniform tri_rmat20 (default: all three; tools/push_case.py's inputs)

Double build.  Per case, once with seeded real weights (1 + uniform[0, 1), tools/push_case.py's) and once with unit weights:
  (a) G = the out-edge matrix (the matrix's transpose by the handle, as the push call takes it), one source: the first vertex
      with an out-edge;
  (b) the call at delta in {mean / 2, mean, 2 mean, 4 mean, +Inf} (mean: the mean weight; 1 for unit weights): reached, the
      passes that had a slice, the buckets, device ms of the call from its event pair (every round trip included) and wall ms,
      median and minimum of REPS runs behind a warm-up with the per-launch timers off, and the kernel records of one further
      run with the timers on; that the distances are the same bits at every delta;
  (c) once more at delta = mean with the parents: device ms, and the vertices given -2;
  (d) unless --no-frontier: graph.sssp_frontier_device on the same arrays -- rounds, pushes, device ms, wall ms of one run
      behind a warm-up -- and that it gives the same bits;
  (e) unless --no-scipy: scipy.sparse.csgraph.dijkstra on the host, wall ms, and the greatest relative difference (scipy
      sums repeated entries and drops explicit zeros; these inputs have neither)."""
import functools
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from benchmark_spgemm_using_csr_amd import _lib, facade, gallery, graph  # noqa: E402
from benchmark_spgemm_using_csr_amd.facade import BhsparseError  # noqa: E402
from tools.reduce_case import make as make_other  # noqa: E402

REPS = int(os.environ.get("REPS", "5"))
CASES = ("roadlike", "uniform", "tri_rmat20")


@functools.lru_cache(maxsize=None)
def make(case):
    """tools/push_case.py's inputs"""
    if case not in CASES:
        raise SystemExit("unknown case %s" % case)
    return gallery.roadlike_csr() if case == "roadlike" else make_other(case)


def stat(xs):
    return {"median": float(np.median(xs)), "min": float(np.min(xs))}


def records(bh):
    return {k["name"]: {"ms": round(k["ms"], 4), "launches": k["launches"]} for k in bh.kernel_stats() if k["launches"] > 0}


def timed_call(bh, call):
    """device and wall ms, median and minimum of REPS runs behind a warm-up with the per-launch timers off; then the records
    of one run with them on"""
    dev_ms, wall_ms = [], []
    assert bh.set_option("kernel_stats", 0) == 0
    for rep in range(REPS + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        assert call() == 0
        wall = (time.perf_counter() - t0) * 1e3
        if rep >= 1:
            dev_ms.append(bh.sssp_ms)
            wall_ms.append(wall)
    assert bh.set_option("kernel_stats", 1) == 0
    assert call() == 0
    return stat(dev_ms), stat(wall_ms), records(bh)


def run(case, unit, bh, dev, opts):
    rp, col = make(case)
    n, nnz = len(rp) - 1, len(col)
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)   # noqa: E731
    vals = np.ones(nnz) if unit else 1.0 + np.random.default_rng(1).random(nnz)
    A = (up(rp.astype(np.int32)), up(col.astype(np.int32)), up(vals))    # A(i, j): an edge j -> i
    assert bh.set_option("kernel_stats", 0) == 0
    Tp, Tj, Tx, _ = bh.csr_transpose_device(n, n, A)
    G = (Tp, Tj, None if unit else Tx)                                # G(i, j): an edge i -> j
    out_deg = (Tp[1:] - Tp[:-1]).cpu().numpy()
    source = int(np.flatnonzero(out_deg > 0)[0])
    mean = 1.0 if unit else float(vals.mean())
    out = {"case": case, "weights": "unit" if unit else "1 + uniform", "n": n, "nnz": nnz, "longest_row": int(out_deg.max()),
           "source": source, "mean_weight": mean, "library": os.path.basename(_lib.SO_PATH), "source_digest": _lib.source_digest()}
    src = up(np.array([source], np.int32))
    dist = torch.empty(n, dtype=torch.float64, device=dev)
    par = torch.empty(n, dtype=torch.int32, device=dev)
    first = None
    out["delta"] = {}
    for name, delta in (("mean/2", mean / 2), ("mean", mean), ("2 mean", 2 * mean), ("4 mean", 4 * mean), ("inf", float("inf"))):
        call = lambda: graph.sssp_delta_raw_device(bh, n, nnz, G[0], G[1], G[2], 1, src, delta, 0, dist, None)   # noqa: E731
        dev_ms, wall_ms, recs = timed_call(bh, call)
        bits = dist.cpu().numpy().tobytes()
        first = bits if first is None else first
        out["delta"][name] = {"delta": delta, "reached": bh.sssp_reached, "passes": bh.get_info("sssp_work_passes"),
                              "launched": bh.sssp_passes, "buckets": bh.get_info("sssp_buckets"), "device_ms": dev_ms,
                              "wall_ms": wall_ms, "kernels": recs, "same_bits": bits == first}
    call = lambda: graph.sssp_delta_raw_device(bh, n, nnz, G[0], G[1], G[2], 1, src, mean, 0, dist, par)   # noqa: E731
    dev_ms, wall_ms, recs = timed_call(bh, call)
    out["with_parents"] = {"device_ms": dev_ms, "wall_ms": wall_ms, "loose": bh.get_info("sssp_loose"),
                           "parents_ms": recs.get("sssp_parents", {}).get("ms")}
    got = dist.cpu().numpy()
    if opts["frontier"]:
        try:                                                          # the warm-up: 64 rounds of it
            graph._sssp_frontier(bh, n, A, [source], G if not unit else (Tp, Tj, Tx), 64)
        except BhsparseError:
            pass
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        D, rounds, ms, pushes = graph._sssp_frontier(bh, n, A, [source], G if not unit else (Tp, Tj, Tx))
        torch.cuda.synchronize()
        out["frontier"] = {"rounds": rounds, "pushes": pushes, "device_ms": ms, "wall_ms": (time.perf_counter() - t0) * 1e3,
                           "same_bits": D[:, 0].contiguous().cpu().numpy().tobytes() == got.tobytes()}
    if opts["scipy"]:
        import scipy.sparse as sp
        from scipy.sparse.csgraph import dijkstra
        M = sp.csr_matrix((Tx.cpu().numpy(), Tj.cpu().numpy(), Tp.cpu().numpy()), shape=(n, n))
        t0 = time.perf_counter()
        want = dijkstra(M, indices=source)
        wall = (time.perf_counter() - t0) * 1e3
        fin = np.isfinite(want)
        rel = float(np.max(np.abs(got[fin] - want[fin]) / np.maximum(want[fin], 1.0))) if fin.any() else 0.0
        out["scipy"] = {"wall_ms": wall, "same_reached": bool(np.array_equal(fin, np.isfinite(got))), "max_rel_diff": rel,
                        "same_bits": got.tobytes() == want.tobytes()}
    return out


def main():
    args = sys.argv[1:]
    opts = {"frontier": "--no-frontier" not in args, "scipy": "--no-scipy" not in args}
    cases = [a for a in args if not a.startswith("--")] or CASES
    dev = torch.device("cuda", 0)
    with facade._handle(np.float64, 0, None) as bh:
        for case in cases:
            for unit in (False, True):
                print(json.dumps(run(case, unit, bh, dev, opts)), flush=True)


if __name__ == "__main__":
    main()
