"""The C/F splitting (bhs_csr_cfsplit_device) beside the MIS(2) aggregation and the heavy-edge matching on the same device
arrays, the direct interpolation (bhs_csr_interp_{symbolic,numeric}_device) beside the SpMV on the same matrix, and the
classical hierarchy (amg.rs_setup_device) beside the MIS(2) one (amg.sa_setup_device) and ILU(0)-PCG in colour order through
setup and solve; measured in one process; prints one JSON line per case.

    python tools/cf_case.py [split|interp|solve] [case ...]
        split cases:  poisson27pt_128 poisson5pt_1024 uniform roadlike    (default: all four)
        interp cases: poisson27pt_128 poisson5pt_1024 aniso_1024          (default: all three)
        solve cases:  poisson27pt_128 poisson5pt_1024 aniso_1024          (default: all three)

Double build.  Part one, per pattern (symmetrised on the device: pattern(A) U pattern(A^T)): the splitting with the degree
  keys and with the plain hash: C points, rounds, device ms of the call from its event pair (the rounds' round trips
  included) after 2 warm-ups, median and minimum of REPS runs, the kernel records' ms of one further run; the aggregation and
  the matching (every weight 1) on the same arrays in the same way.
Part two, per matrix (the Poisson stencils with -1 off the diagonal, the 5-point operator with the y-coupling scaled by
  1e-2): strength at theta 0.25, the splitting, then the symbolic and the numeric interpolation and y = A x, each timed by
  its own ms_out in the same way.
Part three, per matrix, for the classical hierarchy (theta 0.25) and for MIS(2): the wall ms of the second of two setups
  (ending in a device synchronise), the level sizes, the operator complexity (the levels' entries over the finest's), the
  summed device ms of the setup's steps, the wall ms of the Gauss-Seidel smoother's setup, and the iterations and wall ms of
  pcg_device to 1e-8 with the Gauss-Seidel V(1,1) cycle, the smoother's setup inside it included -- the second of two
  solves; and ilu0_pcg_device in colour order to the same tolerance, its setup inside the solve."""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from benchmark_spgemm_using_csr_amd import _lib, amg, facade, gallery  # noqa: E402
from benchmark_spgemm_using_csr_amd.dense import csr_spmv_device  # noqa: E402

REPS = int(os.environ.get("REPS", "7"))
SPLIT_CASES = ("poisson27pt_128", "poisson5pt_1024", "uniform", "roadlike")
SOLVE_CASES = ("poisson27pt_128", "poisson5pt_1024", "aniso_1024")
MAXITER = 1000
THETA = 0.25


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


def head(part, case, n, nnz):
    return {"part": part, "case": case, "n": n, "nnz": nnz, "mean_row": nnz / n, "library": os.path.basename(_lib.SO_PATH),
            "source_digest": _lib.source_digest()}


def run_split(case, bh, dev):
    rp, col = pattern(case)
    n = len(rp) - 1
    up = lambda x, dt: torch.from_numpy(np.ascontiguousarray(x, dt)).to(dev)   # noqa: E731
    ones = torch.ones(len(col), dtype=torch.float64, device=dev)
    Sp, Sj = amg.strength_device(bh, n, (up(rp, np.int32), up(col, np.int32), ones), 0.0)
    nnz = int(Sj.numel())
    out = head("split", case, n, nnz)
    a, b = (torch.empty(n, dtype=torch.int32, device=dev) for _ in range(2))
    torch.cuda.synchronize()
    for name, flags in (("degree", _lib.BHS_CF_DEGREE), ("hashed", 0)):
        ms, records = timed_calls(bh, lambda: amg.cfsplit_raw_device(bh, n, nnz, Sp, Sj, None, 0, flags, a, b), lambda: bh.cfsplit_ms)
        out["cfsplit_" + name] = {"nc": bh.cfsplit_nc, "rounds": bh.cfsplit_rounds, "ms": ms, "kernels": records}
    ms, records = timed_calls(bh, lambda: amg.aggregate_raw_device(bh, n, nnz, Sp, Sj, None, 0, 0, a, b), lambda: bh.aggregate_ms)
    out["aggregate"] = {"nagg": bh.aggregate_nagg, "rounds": bh.aggregate_rounds, "ms": ms, "kernels": records}
    ms, records = timed_calls(bh, lambda: amg.match_raw_device(bh, n, nnz, Sp, Sj, None, 0, 0, a, b), lambda: bh.match_ms)
    out["match_unit"] = {"npairs": bh.match_npairs, "rounds": bh.match_rounds, "ms": ms, "kernels": records}
    return out


def run_interp(case, bh, dev):
    rp, col, val = matrix(case)
    n = len(rp) - 1
    up = lambda x, dt: torch.from_numpy(np.ascontiguousarray(x, dt)).to(dev)   # noqa: E731
    A = (up(rp, np.int32), up(col, np.int32), up(val, np.float64))
    nnz = len(col)
    S = amg.strength_device(bh, n, A, THETA)
    cf, nc, _ = amg.cfsplit_device(bh, n, S)
    out = head("interp", case, n, nnz)
    out.update({"nnzS": int(S[1].numel()), "nc": nc, "split_rounds": bh.cfsplit_rounds, "split_ms": bh.cfsplit_ms})
    Pp = torch.empty(n + 1, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    sym = lambda: amg.interp_symbolic_raw_device(bh, n, nnz, A[0], A[1], S[1].numel(), S[0], S[1], cf, nc, Pp)   # noqa: E731
    ms, records = timed_calls(bh, sym, lambda: bh.interp_symbolic_ms)
    nnzP = bh.interp_nnzP
    out["symbolic"] = {"nnzP": nnzP, "ms": ms, "kernels": records}
    Pj = torch.empty(nnzP, dtype=torch.int32, device=dev)
    Px = torch.empty(nnzP, dtype=torch.float64, device=dev)
    torch.cuda.synchronize()
    num = lambda: amg.interp_numeric_raw_device(bh, n, nnz, A[0], A[1], A[2], S[1].numel(), S[0], S[1], cf, nc, Pp, nnzP, Pj, Px)   # noqa: E731
    ms, records = timed_calls(bh, num, lambda: bh.interp_numeric_ms)
    out["numeric"] = {"ms": ms, "kernels": records}
    x = torch.ones(n, dtype=torch.float64, device=dev)

    def spmv():
        csr_spmv_device(bh, n, n, A, x)
        return 0
    ms, records = timed_calls(bh, spmv, lambda: bh.spmv_ms)
    out["spmv"] = {"ms": ms, "kernels": records}
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
    out = head("solve", case, n, len(col))
    setups = (("classical", lambda: amg.rs_setup_device((h1, h2), n, A, THETA)), ("mis2", lambda: amg.sa_setup_device((h1, h2), n, A)))
    for name, setup in setups:
        setup()
        (levels, info), setup_ms = wall(setup)
        _, smoother_ms = wall(lambda: amg.smoother_setup_device(h1, levels))
        amg.pcg_device(h1, levels, b, 1e-8, 3, "gs")
        (x, its, res), solve_ms = wall(lambda: amg.pcg_device(h1, levels, b, 1e-8, MAXITER, "gs"))
        steps = ("strength_ms", "split_ms", "interp_ms", "aggregate_ms", "prolongator_ms", "galerkin_ms")
        out[name] = {"levels": [r["n"] for r in info], "operator_complexity": sum(r["nnz"] for r in info) / info[0]["nnz"],
                     "rounds": [r["rounds"] for r in info if "rounds" in r], "setup_wall_ms": setup_ms,
                     "device_ms": {s: sum(r.get(s, 0.0) for r in info) for s in steps if any(s in r for r in info)},
                     "smoother_setup_wall_ms": smoother_ms, "pcg_iterations": its, "converged": bool(res[-1] <= 1e-8 * res[0]),
                     "solve_wall_ms": solve_ms, "setup_plus_solve_ms": setup_ms + solve_ms}
        del levels, x
    amg.ilu0_pcg_device(h1, A, b, 1e-8, 3, "colour")
    (x, its, res), ilu_ms = wall(lambda: amg.ilu0_pcg_device(h1, A, b, 1e-8, MAXITER, "colour"))
    out["ilu0_colour"] = {"pcg_iterations": its, "converged": bool(res[-1] <= 1e-8 * res[0]), "setup_plus_solve_ms": ilu_ms}
    return out


def main():
    args = sys.argv[1:]
    names = ("split", "interp", "solve")
    parts = [a for a in args if a in names] or list(names)
    cases = [a for a in args if a not in names]
    dev = torch.device("cuda", 0)
    with facade._handle(np.float64, 0, None) as h1, facade._handle(np.float64, 0, None) as h2:
        if "split" in parts:
            for case in [c for c in (cases or SPLIT_CASES) if c in SPLIT_CASES]:
                print(json.dumps(run_split(case, h1, dev)), flush=True)
        if "interp" in parts:
            for case in [c for c in (cases or SOLVE_CASES) if c in SOLVE_CASES]:
                print(json.dumps(run_interp(case, h1, dev)), flush=True)
        if "solve" in parts:
            for case in [c for c in (cases or SOLVE_CASES) if c in SOLVE_CASES]:
                print(json.dumps(run_solve(case, h1, h2, dev)), flush=True)


if __name__ == "__main__":
    main()
