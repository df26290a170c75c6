"""MIS(2) aggregation (bhs_csr_aggregate_device) and the smoothed-aggregation setup on top of it (amg.sa_setup_device),
measured in one process on the same arrays; prints one JSON line per case.

    python tools/aggregate_case.py [case ...]      cases: poisson27pt_128 poisson5pt_1024 uniform roadlike (default: all four)

Double build.  Per case, on the symmetric pattern of the input:
  (a) the aggregation: rounds, aggregates, device ms per call (the event pair around the whole call: validation, every
      round's round trip, the scan and the joins included) and ms per round, after 2 warm-ups, median and minimum of REPS
      runs; the kernels' records of one call with the per-kernel timers on;
  (b) beside it, in the same run: one bhs_csr_spmv_semiring_device MAX_PLUS pull on the same pattern with zero values (a
      round is two such pulls without the values), and the device copy of the pattern's arrays (torch clone, event-timed):
      the floor for anything that reads the pattern once;
  (c) the whole amg.sa_setup_device on Poisson-like values (the pattern's entries -1, the diagonal the row's length): per
      level n, nnz, nagg, rounds and the device ms of strength / aggregate / prolongator / galerkin, their totals and the
      aggregation's share of the setup."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import scipy.sparse as sp  # noqa: E402
import torch  # noqa: E402

from benchmark_spgemm_using_csr_amd import amg, dense, facade, gallery  # noqa: E402

REPS = int(os.environ.get("REPS", "9"))
CASES = ("poisson27pt_128", "poisson5pt_1024", "uniform", "roadlike")


def make(case):
    """(n, rowPtr, colInd) of a structurally symmetric pattern that holds its diagonal"""
    if case == "poisson27pt_128":
        rp, col = gallery.poisson_csr("poisson27pt", 128, 128, 128)
    elif case == "poisson5pt_1024":
        rp, col = gallery.poisson_csr("poisson5pt", 1024, 1024)
    elif case == "roadlike":
        rp, col = gallery.roadlike_csr()
    elif case == "uniform":
        rp, col = gallery.uniform_csr(1 << 20, 4)
    else:
        raise SystemExit("unknown case %s" % case)
    n = len(rp) - 1
    if case == "uniform":                                            # symmetrised, with the diagonal
        X = sp.csr_matrix((np.ones(len(col)), col, rp), shape=(n, n))
        X = ((X + X.T + sp.identity(n)) > 0).astype(np.float64).tocsr()
        X.sort_indices()
        rp, col = X.indptr, X.indices
    return n, np.asarray(rp, np.int32), np.asarray(col, np.int32)


def stat(xs):
    return {"median": float(np.median(xs)), "min": float(np.min(xs))}


def run(case, h1, h2, dev):
    n, rp, col = make(case)
    nnz = len(col)
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)   # noqa: E731
    S = (up(rp), up(col))
    lens = np.diff(rp.astype(np.int64))
    out = {"case": case, "n": n, "nnz": nnz, "mean_row": nnz / n, "longest_row": int(lens.max())}

    # ---- (a) the aggregation
    assert h1.set_option("kernel_stats", 0) == 0
    ms = []
    for rep in range(REPS + 2):
        agg, nagg, roots = amg.aggregate_device(h1, n, S, seed=0)
        if rep >= 2:
            ms.append(h1.aggregate_ms)
    rounds = h1.aggregate_rounds
    out["aggregate"] = {"nagg": nagg, "rounds": rounds, "ms": stat(ms), "ms_per_round": float(np.median(ms)) / rounds,
                        "rows_per_aggregate": n / nagg}
    assert h1.set_option("kernel_stats", 1) == 0
    again = amg.aggregate_device(h1, n, S, seed=0)
    assert torch.equal(again[0], agg) and torch.equal(again[2], roots)
    out["aggregate"]["kernels"] = {s["name"]: {"launches": s["launches"], "ms": round(s["ms"], 4)} for s in h1.kernel_stats()
                                   if s["launches"] > 0}
    assert h1.set_option("kernel_stats", 0) == 0

    # ---- (b) one MAX_PLUS pull on the pattern with zero values; the copy of the pattern
    zeros = torch.zeros(nnz, dtype=torch.float64, device=dev)
    x = torch.rand(n, dtype=torch.float64, device=dev)
    y = torch.empty(n, dtype=torch.float64, device=dev)
    ms = []
    for rep in range(REPS + 2):
        dense.csr_spmm_semiring_device(h1, "max_plus", n, n, (S[0], S[1], zeros), x, y)
        if rep >= 2:
            ms.append(h1.spmv_ms)
    out["max_plus_pull_ms"] = stat(ms)
    ms = []
    for rep in range(REPS + 2):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        keep = (S[0].clone(), S[1].clone())
        b.record()
        torch.cuda.synchronize()
        if rep >= 2:
            ms.append(a.elapsed_time(b))
        del keep
    out["pattern_copy_ms"] = stat(ms)
    out["round_over_two_pulls"] = out["aggregate"]["ms_per_round"] / (2 * out["max_plus_pull_ms"]["median"])

    # ---- (c) the whole setup
    r = np.repeat(np.arange(n), lens)
    val = np.where(r == col, (lens[r] - 1).clip(min=1).astype(np.float64), -1.0)
    A = (S[0], S[1], up(val))
    runs = []
    # (the uniform graph's second level is all but dense: one coarsening there)
    for rep in range(2):                                             # the second of two: the handles' workspaces are in place
        levels, info = amg.sa_setup_device((h1, h2), n, A, max_levels=2 if case == "uniform" else 10)
        runs.append(info)
    info = runs[-1]
    parts = ("strength_ms", "aggregate_ms", "prolongator_ms", "galerkin_ms")
    total = {k: float(sum(rec.get(k, 0.0) for rec in info)) for k in parts}
    whole = sum(total.values())
    out["setup"] = {"levels": info, "total_ms": total, "setup_ms": whole,
                    "aggregate_share": total["aggregate_ms"] / whole if whole else 0.0,
                    "first_run_setup_ms": float(sum(rec.get(k, 0.0) for rec in runs[0] for k in parts))}
    return out


def main():
    cases = sys.argv[1:] or CASES
    dev = torch.device("cuda", 0)
    with facade._handle(np.float64, 0, None) as h1, facade._handle(np.float64, 0, None) as h2:
        for case in cases:
            print(json.dumps(run(case, h1, h2, dev)), flush=True)


if __name__ == "__main__":
    main()
