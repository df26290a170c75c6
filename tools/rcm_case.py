"""The reverse Cuthill-McKee ordering (bhs_csr_rcm_device) case by case: what the call costs per kernel record, what it does
to the bandwidth and the profile, and what ILU(0)-PCG makes of it beside the natural and the colour ordering; measured in one
process on the same arrays; prints one JSON line per case.

    python tools/rcm_case.py [--no-pcg] [case ...]
        cases: poisson27pt_128 roadlike rmat20 (default: all three)

Double build.  Per case:
  (a) the pattern: the matrix's own where it is symmetric, pattern U pattern^T through ordering.symmetric_pattern_device
      for R-MAT; poisson27pt 128^3 under a seeded relabelling of its vertices (a mesh as a mesher hands it over);
  (b) the call with BHS_RCM_PERIPHERAL and without: ncomp, depth, sweeps, passes, device ms of the call from its event
      pair (every round trip included) after a warm-up, median and minimum of REPS runs with the per-launch timers off, and
      the kernel records' ms and launches of one further run with the timers on;
  (c) bandwidth and profile of the matrix before and after (ordering.bandwidth_profile_device);
  (d) unless --no-pcg: ILU(0)-PCG to 1e-8 on A = the pattern's Laplacian plus SHIFT on the diagonal (poisson27pt: the
      stencil's own values), in natural, colour and RCM order: iterations, the levels of the two triangles, setup and solve
      wall ms."""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from benchmark_spgemm_using_csr_amd import _lib, amg, facade, gallery, ordering  # noqa: E402

REPS = int(os.environ.get("REPS", "5"))
SHIFT = 0.05
MAXITER = 1000
CASES = ("poisson27pt_128", "roadlike", "rmat20")


def shuffled(rp, col, seed):
    import scipy.sparse as sp
    n = len(rp) - 1
    p = np.random.default_rng(seed).permutation(n)
    X = sp.csr_matrix((np.ones(len(col), np.int8), col, rp), shape=(n, n))[p][:, p].tocsr()
    X.sort_indices()
    return X.indptr, X.indices


def make(case):
    """(rowPtr, colInd, symmetric already)"""
    if case == "poisson27pt_128":
        return shuffled(*gallery.poisson_csr("poisson27pt", 128, 128, 128), 128) + (True,)
    if case == "roadlike":
        return gallery.roadlike_csr() + (True,)
    if case == "rmat20":
        return gallery.rmat_csr(scale=20) + (False,)
    raise SystemExit("unknown case %s" % case)


def stat(xs):
    return {"median": float(np.median(xs)), "min": float(np.min(xs))}


def records(bh):
    return {k["name"]: {"ms": round(k["ms"], 4), "launches": k["launches"]} for k in bh.kernel_stats() if k["launches"] > 0}


def pcg(bh, A, b, ordering_name, S):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    if ordering_name == "rcm":
        M = amg.ilu0_setup_permuted_device(bh, A, ordering.rcm_device(bh, A[0].numel() - 1, S))
    else:
        M = amg.ilu0_setup_device(bh, A, ordering_name)
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    _, its, res = amg._pcg_with(bh, A, b, 1e-8, MAXITER, lambda r, z: amg.ilu0_apply_device(bh, M, r, z))
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    return {"iterations": its, "converged": bool(res[-1] <= 1e-8 * res[0]), "levels": [int(M["lower"][1]), int(M["upper"][1])],
            "pivot": int(M["pivot"]), "setup_ms": (t1 - t0) * 1e3, "solve_ms": (t2 - t1) * 1e3}


def run(case, bh, dev, with_pcg):
    rp, col, symmetric = make(case)
    n = len(rp) - 1
    up = lambda x, dt: torch.from_numpy(np.ascontiguousarray(x, dt)).to(dev)   # noqa: E731
    S = (up(rp, np.int32), up(col, np.int32))
    if not symmetric:
        S = ordering.symmetric_pattern_device(bh, n, S + (torch.ones(len(col), dtype=torch.float64, device=dev),))
    nnz = S[1].numel()
    out = {"case": case, "n": n, "nnz": nnz, "mean_row": nnz / n, "longest_row": int((S[0][1:] - S[0][:-1]).max()),
           "library": os.path.basename(_lib.SO_PATH), "source_digest": _lib.source_digest()}
    perm = torch.empty(n, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    before = ordering.bandwidth_profile_device(n, S)
    for name, flags in (("peripheral", ordering.BHS_RCM_PERIPHERAL), ("plain", 0)):
        ms, passes = [], []
        assert bh.set_option("kernel_stats", 0) == 0                  # (no event pair a launch inside the timed span)
        for rep in range(REPS + 1):
            err = ordering.rcm_raw_device(bh, n, nnz, S[0], S[1], flags, perm, None, None)
            if err:
                break
            if rep >= 1:
                ms.append(bh.rcm_ms)
                passes.append(bh.rcm_passes)
        if err:
            out[name] = {"error": err}
            continue
        assert bh.set_option("kernel_stats", 1) == 0
        assert ordering.rcm_raw_device(bh, n, nnz, S[0], S[1], flags, perm, None, None) == 0
        after = ordering.bandwidth_profile_device(n, S, perm)
        out[name] = {"ncomp": bh.rcm_ncomp, "depth": bh.rcm_depth, "sweeps": bh.rcm_sweeps, "passes": sorted(set(passes)), "ms": stat(ms),
                     "kernels": records(bh), "bandwidth": [before[0], after[0]], "profile": [before[1], after[1]]}
    if with_pcg:
        lens = (S[0][1:] - S[0][:-1]).to(torch.int64)
        rows = torch.repeat_interleave(torch.arange(n, dtype=torch.int64, device=dev), lens, output_size=nnz)
        diag = rows == S[1].long()
        if case == "poisson27pt_128":
            val = torch.where(diag, 26.0, -1.0).to(torch.float64)
        else:                                                         # the Laplacian plus SHIFT: every row needs its diagonal entry
            assert int(diag.sum()) == n, "a row without its diagonal entry"
            deg = (lens - 1).to(torch.float64)
            val = torch.where(diag, deg[rows] + SHIFT, torch.full_like(deg[rows], -1.0))
        A = (S[0], S[1], val)
        b = torch.from_numpy(np.random.default_rng(1).standard_normal(n)).to(dev)
        out["ilu0_pcg"] = {name: pcg(bh, A, b, name, S) for name in ("natural", "colour", "rcm")}
    return out


def main():
    args = sys.argv[1:]
    with_pcg = "--no-pcg" not in args
    cases = [a for a in args if not a.startswith("--")] or CASES
    dev = torch.device("cuda", 0)
    with facade._handle(np.float64, 0, None) as bh:
        for case in cases:
            print(json.dumps(run(case, bh, dev, with_pcg)), flush=True)


if __name__ == "__main__":
    main()
