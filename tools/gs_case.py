"""The colouring (bhs_csr_color_device), the multicolour Gauss-Seidel sweep (bhs_csr_gs_device) and the solvers on top of them
(amg.vcycle_device with smoother="gs", amg.pcg_device), measured in one process on the same arrays; prints one JSON line per
case.

    python tools/gs_case.py [case ...]      cases: poisson27pt_128 uniform poisson5pt_1024 (default: all three)

Double build.  Per case, on a matrix with the symmetric pattern of the input (Poisson cases: -1 beside the diagonal, the
stencil's size - 1 on it; uniform: random values made strictly diagonally dominant):
  (a) the colouring: colours, rounds, device ms per call (the event pair around the whole call: every round's round trip, the
      scan and the numbering included), after 2 warm-ups, median and minimum of REPS runs; the kernels' records of one call
      with the per-kernel timers on; the colours' sizes;
  (b) one forward sweep (device ms of the call, launches) beside one bhs_csr_spmv_device call on the same arrays;
  (c) one symmetric sweep beside one weighted-Jacobi sweep as amg._jacobi does it (an SpMV and three torch kernels), both as
      wall time around a synchronised call, and the symmetric sweep's device ms;
  (d) Poisson cases only: the hierarchy of amg.sa_setup_device, the smoothers' setup, then whole solves to 1e-8 from a random
      right-hand side: Jacobi cycles (amg.solve_device), Gauss-Seidel cycles and amg.pcg_device -- cycles or iterations and
      wall ms (every step is a synchronous library call, so wall time is device time plus the calls' round trips).
      The uniform graph's second level is all but dense (profiles/aggregate_case.md): no solve there."""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import scipy.sparse as sp  # noqa: E402
import torch  # noqa: E402

from benchmark_spgemm_using_csr_amd import _lib, amg, dense, facade, gallery  # noqa: E402

REPS = int(os.environ.get("REPS", "9"))
CASES = ("poisson27pt_128", "uniform", "poisson5pt_1024")


def make(case):
    """(n, rowPtr, colInd, val, solvable)"""
    rng = np.random.default_rng(1)
    if case == "poisson27pt_128":
        rp, col = gallery.poisson_csr("poisson27pt", 128, 128, 128)
    elif case == "poisson5pt_1024":
        rp, col = gallery.poisson_csr("poisson5pt", 1024, 1024)
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
    rp, col = np.asarray(rp, np.int32), np.asarray(col, np.int32)
    lens = np.diff(rp.astype(np.int64))
    r = np.repeat(np.arange(n), lens)
    if case == "uniform":
        val = rng.uniform(-1.0, 1.0, len(col))
        off = np.bincount(r[r != col], weights=np.abs(val[r != col]), minlength=n)
        val[r == col] = off[r[r == col]] + 1.0
    else:
        full = int(lens.max())
        val = np.where(r == col, float(full - 1), -1.0)
    return n, rp, col, val, case != "uniform"


def stat(xs):
    return {"median": float(np.median(xs)), "min": float(np.min(xs))}


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, (time.perf_counter() - t0) * 1e3


def run(case, h1, h2, dev):
    n, rp, col, val, solvable = make(case)
    nnz = len(col)
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)   # noqa: E731
    A = (up(rp), up(col), up(val))
    out = {"case": case, "n": n, "nnz": nnz, "mean_row": nnz / n, "longest_row": int(np.diff(rp).max()),
           "source_digest": _lib.source_digest()}
    rng = np.random.default_rng(2)
    b = up(rng.standard_normal(n))
    x0 = up(rng.standard_normal(n))
    diag = h1.csr_reduce_device(n, n, A, _lib.BHS_AXIS_DIAG, _lib.BHS_RED_PLUS)

    # ---- (a) the colouring
    assert h1.set_option("kernel_stats", 0) == 0
    ms = []
    for rep in range(REPS + 2):
        coloring = amg.color_device(h1, n, A, seed=0)
        if rep >= 2:
            ms.append(h1.color_ms)
    color, ncolors, order, cptr = coloring
    rounds = h1.color_rounds
    out["color"] = {"ncolors": ncolors, "rounds": rounds, "ms": stat(ms), "ms_per_round": float(np.median(ms)) / rounds,
                    "sizes": np.diff(cptr).tolist()}
    assert h1.set_option("kernel_stats", 1) == 0
    again = amg.color_device(h1, n, A, seed=0)
    assert torch.equal(again[0], color) and torch.equal(again[2], order) and np.array_equal(again[3], cptr)
    out["color"]["kernels"] = {s["name"]: {"launches": s["launches"], "ms": round(s["ms"], 4)} for s in h1.kernel_stats()
                               if s["launches"] > 0}
    assert h1.set_option("kernel_stats", 0) == 0

    # ---- (b) a forward sweep beside one SpMV
    fwd, spmv = [], []
    for rep in range(REPS + 2):
        x = x0.clone()
        amg.gs_device(h1, A, diag, coloring, b, x, direction="forward")
        t = h1.gs_ms
        dense.csr_spmv_device(h1, n, n, A, x0)
        if rep >= 2:
            fwd.append(t)
            spmv.append(h1.spmv_ms)
    out["forward_ms"] = stat(fwd)
    out["spmv_ms"] = stat(spmv)
    out["forward_over_spmv"] = out["forward_ms"]["median"] / out["spmv_ms"]["median"]
    out["forward_launches"] = int(np.count_nonzero(np.diff(cptr)))
    x = x0.clone()
    amg.gs_device(h1, A, diag, coloring, b, x, direction="forward", verify=True)     # the colouring is proper for A
    out["forward_verified_ms"] = h1.gs_ms

    # ---- (c) a symmetric sweep beside one Jacobi sweep
    sym_dev, sym_wall, jac_wall = [], [], []
    for rep in range(REPS + 2):
        x = x0.clone()
        _, t = wall(lambda: amg.gs_device(h1, A, diag, coloring, b, x, direction="symmetric"))
        d = h1.gs_ms
        _, tj = wall(lambda: amg._jacobi(h1, A, diag, b, x0, 2.0 / 3.0, 1))
        if rep >= 2:
            sym_dev.append(d)
            sym_wall.append(t)
            jac_wall.append(tj)
    out["symmetric_ms"] = stat(sym_dev)
    out["symmetric_wall_ms"] = stat(sym_wall)
    out["jacobi_wall_ms"] = stat(jac_wall)
    out["symmetric_over_jacobi_wall"] = out["symmetric_wall_ms"]["median"] / out["jacobi_wall_ms"]["median"]

    # ---- (d) whole solves
    if solvable:
        levels, info = amg.sa_setup_device((h1, h2), n, A)
        smoothers, t_sm = wall(lambda: amg.smoother_setup_device(h1, levels))
        out["levels"] = [rec["n"] for rec in info]
        out["smoother_setup_wall_ms"] = t_sm
        out["level_colours"] = [s[1][1] for s in smoothers]
        (xj, cj, rj), tj = wall(lambda: amg.solve_device(h1, levels, b, 1e-8, 200))

        def gs_solve():
            x = torch.zeros_like(b)
            res, cycles = [float(torch.linalg.norm(b))], 0
            while res[-1] > 1e-8 * res[0] and cycles < 200:
                x = amg.vcycle_device(h1, levels, b, x, smoother="gs", smoothers=smoothers)
                res.append(float(torch.linalg.norm(dense.csr_spmv_device(h1, n, n, A, x, alpha=-1.0, beta=1.0, y=b.clone()))))
                cycles += 1
            return x, cycles, res
        (xg, cg, rg), tg = wall(gs_solve)
        (xp, ip, rp_), tp = wall(lambda: amg.pcg_device(h1, levels, b, 1e-8, 200))
        true = lambda x: float(torch.linalg.norm(dense.csr_spmv_device(h1, n, n, A, x, alpha=-1.0, beta=1.0, y=b.clone())) / torch.linalg.norm(b))   # noqa: E731
        out["solve"] = {"jacobi": {"cycles": cj, "wall_ms": tj, "residual": true(xj)},
                        "gs": {"cycles": cg, "wall_ms": tg, "residual": true(xg)},
                        "pcg": {"iterations": ip, "wall_ms": tp, "residual": true(xp), "includes_smoother_setup": True}}
    return out


def main():
    cases = sys.argv[1:] or CASES
    dev = torch.device("cuda", 0)
    with facade._handle(np.float64, 0, None) as h1, facade._handle(np.float64, 0, None) as h2:
        for case in cases:
            print(json.dumps(run(case, h1, h2, dev)), flush=True)


if __name__ == "__main__":
    main()
