"""The heavy-edge matching (bhs_csr_match_device) beside the MIS(2) aggregation (bhs_csr_aggregate_device) on the same device
arrays, and the pairwise-aggregation hierarchy (amg.pa_setup_device) beside the MIS(2) one (amg.sa_setup_device) through
setup and solve; measured in one process; prints one JSON line per case.

    python tools/match_case.py [match|solve] [case ...]
        match cases: poisson27pt_128 poisson5pt_1024 uniform roadlike    (default: all four)
        solve cases: poisson27pt_128 poisson5pt_1024 aniso_1024          (default: all three)

Double build.  Part one, per pattern (symmetrised on the device: pattern(A) U pattern(A^T)):
  the matching without values (every weight 1) and with symmetric integer weights 1 .. 4, with the numbering: pairs, rounds,
  the share of unmatched vertices, device ms of the call from its event pair (the rounds' round trips included) after 2
  warm-ups, median and minimum of REPS runs, the kernel records' ms of one further run; and the aggregation on the same
  arrays in the same way: aggregates, rounds, ms.
Part two, per matrix (the Poisson stencils with -1 off the diagonal, the 5-point operator with the y-coupling scaled by
  1e-2), for MIS(2) and for pairwise aggregation with 2 and with 3 passes: the wall ms of the second of two setups (ending in
  a device synchronise), the level sizes, the operator complexity (the levels' entries over the finest's), the summed device
  ms of the setup's aggregation steps, the wall ms of the Gauss-Seidel smoother's setup (diagonals, colourings), and the
  iterations and wall ms of pcg_device to 1e-8 with the Gauss-Seidel V(1,1) cycle, the smoother's setup inside it
  included -- the second of two solves."""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from benchmark_spgemm_using_csr_amd import _lib, amg, facade, gallery  # noqa: E402

REPS = int(os.environ.get("REPS", "7"))
MATCH_CASES = ("poisson27pt_128", "poisson5pt_1024", "uniform", "roadlike")
SOLVE_CASES = ("poisson27pt_128", "poisson5pt_1024", "aniso_1024")
MAXITER = 1000


def pattern(case):
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


def matrix(case):
    """(rowPtr, colInd, val), rows ascending"""
    if case == "aniso_1024":
        import scipy.sparse as sp
        e = np.ones(1024)
        T = sp.diags([-e[:-1], 2 * e, -e[:-1]], [-1, 0, 1])
        A = (sp.kron(sp.identity(1024), T) + 1e-2 * sp.kron(T, sp.identity(1024))).tocsr()
        A.sort_indices()
        return A.indptr, A.indices, A.data
    rp, col = pattern(case)
    rows = np.repeat(np.arange(len(rp) - 1), np.diff(rp))
    full = len(gallery.stencil_offsets(case.split("_")[0]))
    return rp, col, np.where(rows == col, float(full - 1), -1.0)


def stat(xs):
    return {"median": float(np.median(xs)), "min": float(np.min(xs))}


def kernels_ms(bh):
    return {k["name"]: [k["launches"], round(k["ms"], 4)] for k in bh.kernel_stats() if k["launches"] > 0}


def pair_weights(n, Sp, Sj):
    """symmetric integer weights 1 .. 4: a function of the unordered pair"""
    rows = torch.repeat_interleave(torch.arange(n, device=Sj.device), (Sp[1:] - Sp[:-1]).long())
    lo, hi = torch.minimum(rows, Sj.long()), torch.maximum(rows, Sj.long())
    return (1 + ((lo * 2654435761 + hi * 40503) >> 16) % 4).to(torch.float64)


def timed_calls(bh, call, read):
    ms = []
    assert bh.set_option("kernel_stats", 0) == 0                      # (no event pair a launch inside the timed span)
    for rep in range(REPS + 2):
        assert call() == 0
        if rep >= 2:
            ms.append(read())
    assert bh.set_option("kernel_stats", 1) == 0
    assert call() == 0
    records = kernels_ms(bh)
    assert bh.set_option("kernel_stats", 0) == 0
    return stat(ms), records


def run_match(case, bh, dev):
    rp, col = pattern(case)
    n = len(rp) - 1
    up = lambda x, dt: torch.from_numpy(np.ascontiguousarray(x, dt)).to(dev)   # noqa: E731
    ones = torch.ones(len(col), dtype=torch.float64, device=dev)
    Sp, Sj = amg.strength_device(bh, n, (up(rp, np.int32), up(col, np.int32), ones), 0.0)
    nnz = int(Sj.numel())
    out = {"part": "match", "case": case, "n": n, "nnz": nnz, "mean_row": nnz / n, "library": os.path.basename(_lib.SO_PATH),
           "source_digest": _lib.source_digest()}
    mate, agg, roots = (torch.empty(n, dtype=torch.int32, device=dev) for _ in range(3))
    torch.cuda.synchronize()
    for name, vals in (("unit", None), ("weighted", pair_weights(n, Sp, Sj))):
        torch.cuda.synchronize()
        ms, records = timed_calls(bh, lambda: amg.match_raw_device(bh, n, nnz, Sp, Sj, vals, 0, 0, mate, agg), lambda: bh.match_ms)
        out["match_" + name] = {"npairs": bh.match_npairs, "rounds": bh.match_rounds, "unmatched_share": 1.0 - 2.0 * bh.match_npairs / n,
                                "ms": ms, "kernels": records}
    ms, records = timed_calls(bh, lambda: amg.aggregate_raw_device(bh, n, nnz, Sp, Sj, None, 0, 0, agg, roots), lambda: bh.aggregate_ms)
    out["aggregate"] = {"nagg": bh.aggregate_nagg, "rounds": bh.aggregate_rounds, "ms": ms, "kernels": records}
    return out


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    got = fn()
    torch.cuda.synchronize()
    return got, (time.perf_counter() - t0) * 1e3


def run_solve(case, h1, h2, dev):
    rp, col, val = matrix(case)
    n = len(rp) - 1
    up = lambda x, dt: torch.from_numpy(np.ascontiguousarray(x, dt)).to(dev)   # noqa: E731
    A = (up(rp, np.int32), up(col, np.int32), up(val, np.float64))
    b = torch.from_numpy(np.random.default_rng(4).standard_normal(n)).to(dev)
    out = {"part": "solve", "case": case, "n": n, "nnz": len(col), "library": os.path.basename(_lib.SO_PATH),
           "source_digest": _lib.source_digest()}
    setups = (("mis2", lambda: amg.sa_setup_device((h1, h2), n, A)),
              ("pairwise2", lambda: amg.pa_setup_device((h1, h2), n, A, passes=2)),
              ("pairwise3", lambda: amg.pa_setup_device((h1, h2), n, A, passes=3)))
    for name, setup in setups:
        setup()
        (levels, info), setup_ms = wall(setup)
        _, smoother_ms = wall(lambda: amg.smoother_setup_device(h1, levels))
        amg.pcg_device(h1, levels, b, 1e-8, 3, "gs")
        (x, its, res), solve_ms = wall(lambda: amg.pcg_device(h1, levels, b, 1e-8, MAXITER, "gs"))
        out[name] = {"levels": [r["n"] for r in info], "operator_complexity": sum(r["nnz"] for r in info) / info[0]["nnz"],
                     "setup_wall_ms": setup_ms, "aggregate_device_ms": sum(r.get("aggregate_ms", 0.0) for r in info),
                     "strength_device_ms": sum(r.get("strength_ms", 0.0) for r in info),
                     "prolongator_device_ms": sum(r.get("prolongator_ms", 0.0) for r in info),
                     "galerkin_device_ms": sum(r.get("galerkin_ms", 0.0) for r in info),
                     "smoother_setup_wall_ms": smoother_ms, "pcg_iterations": its, "converged": bool(res[-1] <= 1e-8 * res[0]),
                     "solve_wall_ms": solve_ms, "setup_plus_solve_ms": setup_ms + solve_ms}
        del levels, x
    return out


def main():
    args = sys.argv[1:]
    parts = [a for a in args if a in ("match", "solve")] or ["match", "solve"]
    cases = [a for a in args if a not in ("match", "solve")]
    dev = torch.device("cuda", 0)
    with facade._handle(np.float64, 0, None) as h1, facade._handle(np.float64, 0, None) as h2:
        if "match" in parts:
            for case in [c for c in (cases or MATCH_CASES) if c in MATCH_CASES]:
                print(json.dumps(run_match(case, h1, dev)), flush=True)
        if "solve" in parts:
            for case in [c for c in (cases or SOLVE_CASES) if c in SOLVE_CASES]:
                print(json.dumps(run_solve(case, h1, h2, dev)), flush=True)


if __name__ == "__main__":
    main()
