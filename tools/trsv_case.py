"""The level sets (bhs_csr_levels_device), the sparse triangular solve (bhs_csr_trsv_device), ILU(0) (bhs_csr_ilu0_device) and
the ILU(0)-preconditioned CG on top of them (amg.ilu0_pcg_device), measured in one process on the same arrays; prints one
JSON line per case.

    python tools/trsv_case.py [case ...]      cases: poisson27pt_128 poisson5pt_1024 uniform (default: all three)

Double build.  Per case, on a matrix with ascending rows and a diagonal entry in every row (Poisson cases: -1 beside the
diagonal, the stencil's size - 1 on it; uniform: 2^20 rows of 4 random columns and the diagonal, random values made strictly
diagonally dominant), in natural order and permuted by (colour, index) of the colouring of pattern(A) U pattern(A^T):
  (a) the analysis of both triangles: levels, passes, device ms per call after 2 warm-ups (median and minimum of REPS runs),
      the sizes of the thinnest and the widest level and how many levels hold at most 1024 rows;
  (b) ILU(0) in place on a copy of the values: device ms, launches, pivot;
  (c) the unit lower solve and the upper solve with the factors, in place: device ms and launches, beside one forward
      Gauss-Seidel sweep on the colouring and one bhs_csr_spmv_device call on the same arrays;
  (d) Poisson cases only: whole solves to 1e-8 from a random right-hand side -- amg.ilu0_pcg_device in both orderings beside
      amg.pcg_device on the smoothed-aggregation hierarchy: iterations and wall ms (every step is a synchronous library
      call, so wall time is device time plus the calls' round trips); the setups are inside the times."""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import scipy.sparse as sp  # noqa: E402
import torch  # noqa: E402

from benchmark_spgemm_using_csr_amd import _lib, amg, dense, facade, gallery  # noqa: E402

REPS = int(os.environ.get("REPS", "7"))
SOLVE = int(os.environ.get("SOLVE", "1"))             # 0: without the whole solves of (d)
CASES = ("poisson27pt_128", "poisson5pt_1024", "uniform")


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
    if case == "uniform":                                            # with the diagonal, rows ascending
        X = sp.csr_matrix((np.ones(len(col)), col, rp), shape=(n, n))
        X = ((X + sp.identity(n)) > 0).astype(np.float64).tocsr()
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
        val = np.where(r == col, float(int(lens.max()) - 1), -1.0)
    return n, rp, col, val, case != "uniform"


def stat(xs):
    return {"median": float(np.median(xs)), "min": float(np.min(xs))}


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, (time.perf_counter() - t0) * 1e3


def launches(bh):
    return {s["name"]: s["launches"] for s in bh.kernel_stats() if s["launches"] > 0}


def ordering(bh, n, A, b, coloring=None):
    """the measurements (a) .. (c) of one matrix"""
    out = {}
    levels = {}
    for upper in (False, True):
        ms = []
        for rep in range(REPS + 2):
            lev = amg.levels_device(bh, n, A, upper=upper)
            if rep >= 2:
                ms.append(bh.levels_ms)
        levels[upper] = lev
        sizes = np.diff(lev[3])
        out["upper" if upper else "lower"] = {"levels": lev[1], "passes": bh.levels_passes, "ms": stat(ms), "thinnest": int(sizes.min()),
                                              "widest": int(sizes.max()), "thin_levels": int((sizes <= 1024).sum())}
    ms = []
    for rep in range(REPS + 2):
        LU = (A[0], A[1], A[2].clone())
        amg.ilu0_device(bh, LU, levels[False])
        if rep >= 2:
            ms.append(bh.ilu0_ms)
    out["ilu0"] = {"ms": stat(ms), "launches": launches(bh).get("ilu0_level", 0), "pivot": bh.ilu0_pivot}
    low, upp = [], []
    for rep in range(REPS + 2):
        y = b.clone()
        amg.trsv_device(bh, LU, levels[False], y, y, unit_diag=True)
        t, ran_low = bh.trsv_ms, launches(bh)
        amg.trsv_device(bh, LU, levels[True], y, y, upper=True)
        if rep >= 2:
            low.append(t)
            upp.append(bh.trsv_ms)
    out["trsv"] = {"lower_ms": stat(low), "upper_ms": stat(upp), "lower_launches": ran_low, "upper_launches": launches(bh)}
    if coloring is not None:
        diag = bh.csr_reduce_device(n, n, A, _lib.BHS_AXIS_DIAG, _lib.BHS_RED_PLUS)
        fwd, spmv = [], []
        for rep in range(REPS + 2):
            x = b.clone()
            amg.gs_device(bh, A, diag, coloring, b, x, direction="forward")
            t = bh.gs_ms
            dense.csr_spmv_device(bh, n, n, A, b)
            if rep >= 2:
                fwd.append(t)
                spmv.append(bh.spmv_ms)
        out["gs_forward_ms"] = stat(fwd)
        out["spmv_ms"] = stat(spmv)
    return out


def run(case, h1, h2, dev):
    n, rp, col, val, solvable = make(case)
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)   # noqa: E731
    A = (up(rp), up(col), up(val))
    out = {"case": case, "n": n, "nnz": len(col), "mean_row": len(col) / n, "source_digest": _lib.source_digest()}
    b = up(np.random.default_rng(2).standard_normal(n))
    coloring = amg.color_device(h1, n, amg.strength_device(h1, n, A, 0.0), 0)
    out["ncolors"] = coloring[1]
    out["natural"] = ordering(h1, n, A, b, coloring)
    Ac = amg._permuted_device(h1, n, A, coloring[2])
    out["colour"] = ordering(h1, n, Ac, b)
    if solvable and SOLVE:
        true = lambda x: float(torch.linalg.norm(dense.csr_spmv_device(h1, n, n, A, x, alpha=-1.0, beta=1.0, y=b.clone())) / torch.linalg.norm(b))   # noqa: E731
        out["solve"] = {}
        for o in ("natural", "colour"):
            (x, its, _), t = wall(lambda: amg.ilu0_pcg_device(h1, A, b, 1e-8, 2000, ordering=o))
            out["solve"]["ilu0_pcg_" + o] = {"iterations": its, "wall_ms": t, "residual": true(x)}

        def amg_pcg():
            levels, _ = amg.sa_setup_device((h1, h2), n, A)
            return amg.pcg_device(h1, levels, b, 1e-8, 200)
        (x, its, _), t = wall(amg_pcg)
        out["solve"]["amg_pcg"] = {"iterations": its, "wall_ms": t, "residual": true(x)}
    return out


def main():
    cases = sys.argv[1:] or CASES
    dev = torch.device("cuda", 0)
    with facade._handle(np.float64, 0, None) as h1, facade._handle(np.float64, 0, None) as h2:
        for case in cases:
            print(json.dumps(run(case, h1, h2, dev)), flush=True)


if __name__ == "__main__":
    main()
