"""C = A·B + D (bhs_spgemm_add_device) and the stand-alone sparse add against the multiply alone (bhs_spgemm) on the same
device-resident data; prints one JSON line.

    python tools/add_case.py [case ...]      cases: p27_128 uniform rmat uniform_grow rmat_grow (default: all)

Per case, in one process: bhs_spgemm alone, bhs_spgemm_add_device in place (alpha = beta = 1; where D is inside A·B), the
same with add_inplace=0 (the sum in a second set of arrays), and the stand-alone add Z = (A·B) + D on the product's own
device arrays.  D = A, or for the *_grow cases a random pattern of nnz(A) entries so that rows grow.  After warm-ups,
medians and minima of REPS (default 12) runs with per-kernel timers off: device time of the multiply (its four stages) and
of the add (its own events).  One extra run of each with kernel_stats=1 gives the add's kernel families.  Achieved
bandwidth is computed on the add's algorithmic bytes: in place, alpha == 1: 12·nnz(D) read + 16·nnz(D) (valC lines read
and written, counted per entry) -- the count pass's read of C's columns (4·nnz(AB)) is listed beside it; two-array path:
12·(nnz(AB) + nnz(D)) read, 12·nnz(C) + 4·(m+1) written."""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from benchmark_spgemm_using_csr_amd import facade, gallery  # noqa: E402

REPS = int(os.environ.get("REPS", "12"))
WARM = 3


def make(case):
    grow = case.endswith("_grow")
    base = case[:-5] if grow else case
    if base == "p27_128":
        rp, col = gallery.poisson_csr("poisson27pt", 128, 128, 128)
    elif base == "uniform":
        rp, col = gallery.uniform_csr()
    elif base == "rmat":
        rp, col = gallery.rmat_csr(scale=18, edge_factor=8)
    else:
        raise ValueError(case)
    m = len(rp) - 1
    if grow:
        rng = np.random.default_rng(1)
        drp, dcol = gallery._csr_from_pairs(m, m, rng.integers(0, m, len(col)), rng.integers(0, m, len(col)))
    else:
        drp, dcol = rp, col
    return rp, col, drp, dcol


def stat(xs):
    return {"median_ms": float(np.median(xs)), "min_ms": float(np.min(xs))}


def families(bh):
    return {s["name"]: {"launches": s["launches"], "ms": round(s["ms"], 4), "rows": s["rows"]} for s in bh.kernel_stats()
            if s["name"].startswith("add_")}


def run(case):
    rp, col, drp, dcol = make(case)
    m = len(rp) - 1
    val = gallery.fill_values(len(col))
    dval = gallery.fill_values(len(dcol))
    dev = torch.device("cuda", 0)
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)   # noqa: E731
    Ap, Aj, Ax = up(rp.astype(np.int32)), up(col.astype(np.int32)), up(val)
    Bp, Bj, Bx = Ap.clone(), Aj.clone(), Ax.clone()
    Dp, Dj, Dx = up(drp.astype(np.int32)), up(dcol.astype(np.int32)), up(dval)
    nnzD = int(Dj.numel())
    plats = [False] * facade.NUM_PLATFORMS
    plats[facade.BHSPARSE_HIP] = True
    bh = facade.bhsparse()
    assert bh.initPlatform(plats) == 0
    assert bh.initData_device(m, m, m, Aj.numel(), Ax, Ap, Aj, Bj.numel(), Bx, Bp, Bj) == 0
    out = {"case": case, "m": m, "nnzA": int(Aj.numel()), "nnzD": nnzD}
    assert bh.set_option("kernel_stats", 0) == 0
    dms = []
    for i in range(WARM + REPS):
        assert bh.spgemm() == 0
        if i >= WARM:
            dms.append(sum(bh.stage_ms))
    nnzAB = bh.nnzC
    out["spgemm"] = dict(stat(dms), nnzCt=bh.nnzCt, nnzC=nnzAB, class_state=bh.get_info("class_state"))
    for label, inplace in (("add_inplace", 1), ("add_two_arrays", 0)):
        assert bh.set_option("add_inplace", inplace) == 0
        mul, add, wall = [], [], []
        for i in range(WARM + REPS):
            t0 = time.perf_counter()
            assert bh.spgemm_add_device(1.0, 1.0, nnzD, Dx, Dp, Dj) == 0
            w = (time.perf_counter() - t0) * 1e3
            if i >= WARM:
                add.append(bh.add_ms)
                wall.append(w)
        used = bh.get_info("add_inplace_used")
        nnzC = bh.nnzC
        assert bh.set_option("kernel_stats", 1) == 0
        assert bh.spgemm_add_device(1.0, 1.0, nnzD, Dx, Dp, Dj) == 0
        fam = families(bh)
        assert bh.set_option("kernel_stats", 0) == 0
        if used:
            nbytes = 12 * nnzD + 16 * nnzD
        else:
            nbytes = 12 * (nnzAB + nnzD) + 12 * nnzC + 4 * (m + 1)
        a = stat(add)
        out[label] = {"add": a, "wall": stat(wall), "inplace_used": used, "nnzC": nnzC, "kernels": fam,
                      "algorithmic_bytes": nbytes, "count_pass_column_bytes": 4 * nnzAB,
                      "achieved_GBps": nbytes / (a["median_ms"] * 1e6),
                      "add_over_spgemm": a["median_ms"] / out["spgemm"]["median_ms"]}
    # the stand-alone add on the product's device arrays
    assert bh.set_option("add_inplace", 1) == 0
    assert bh.spgemm() == 0
    pCp, pCj, pCx = bh.get_C_device()
    Zp = torch.empty(m + 1, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    sym, num = [], []
    nnzZ = 0
    for i in range(WARM + REPS):
        t0 = time.perf_counter()
        err, nnzZ, inside = bh.csr_add_symbolic_device(m, m, nnzAB, pCp, pCj, nnzD, Dp, Dj, Zp)
        assert err == 0
        if i >= WARM:
            sym.append((time.perf_counter() - t0) * 1e3)
    Zj = torch.empty(max(nnzZ, 1), dtype=torch.int32, device=dev)
    Zx = torch.empty(max(nnzZ, 1), dtype=torch.float64, device=dev)
    torch.cuda.synchronize()
    for i in range(WARM + REPS):
        assert bh.csr_add_numeric_device(m, m, 1.0, nnzAB, pCx, pCp, pCj, 1.0, nnzD, Dx, Dp, Dj, Zp, Zj, Zx) == 0
        if i >= WARM:
            num.append(bh.add_ms)
    nbytes = 12 * (nnzAB + nnzD) + 12 * nnzZ + 4 * (m + 1)
    out["standalone"] = {"symbolic_wall": stat(sym), "numeric": stat(num), "nnzZ": nnzZ,
                         "numeric_achieved_GBps": nbytes / (float(np.median(num)) * 1e6)}
    bh.free_mem()
    bh.freePlatform()
    return out


if __name__ == "__main__":
    cases = sys.argv[1:] or ["p27_128", "uniform", "rmat", "uniform_grow", "rmat_grow"]
    res = []
    for c in cases:
        res.append(run(c))
        torch.cuda.empty_cache()
    print(json.dumps({"tool": "add_case", "reps": REPS, "results": res}))
