"""The masked multiply (bhs_spgemm_masked_device) against the full multiply (bhs_spgemm) on the same device-resident data;
prints one JSON line.

    python tools/masked_case.py [case ...]      cases: p27_128_class p27_128_general uniform banded tri_rmat20 (default: all)

Per case: the full multiply timed first (its C's pattern is then the mask for "M = pattern(A^2)" cases; the triangle
count uses M = L), then the masked multiply on that mask.  Both after warm-ups, medians of REPS (default 20) runs with
per-kernel timers off; device time (stage timers / the masked call's own events) and host wall time.  One extra run of
each with kernel_stats=1 gives the kernel-family breakdown.  The masked values are checked against the full product's
where M = pattern(A^2) (bit for bit: integer values)."""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from benchmark_spgemm_using_csr_amd import facade, gallery  # noqa: E402

REPS = int(os.environ.get("REPS", "20"))
WARM = 3


def lower_triangle(rp, col):
    n = len(rp) - 1
    r = np.repeat(np.arange(n), np.diff(rp))
    rows = np.concatenate([r, col]).astype(np.int64)
    cols = np.concatenate([col, r]).astype(np.int64)
    low = rows > cols
    return gallery._csr_from_pairs(n, n, rows[low], cols[low])


def make(case):
    if case.startswith("p27_128"):
        rp, col = gallery.poisson_csr("poisson27pt", 128, 128, 128)
        return rp, col, {"class_path": 1 if case.endswith("class") else 0}
    if case == "uniform":
        rp, col = gallery.uniform_csr()
        return rp, col, {}
    if case == "banded":
        rp, col = gallery.banded_csr()
        return rp, col, {}
    if case == "tri_rmat20":
        rp, col = lower_triangle(*gallery.rmat_csr(scale=20))
        return rp, col, {}
    raise ValueError(case)


def families(bh):
    return {s["name"]: {"launches": s["launches"], "ms": round(s["ms"], 4), "rows": s["rows"], "products": s["products"]}
            for s in bh.kernel_stats()}


def run(case):
    rp, col, opts = make(case)
    m = len(rp) - 1
    val = gallery.fill_values(len(col)) if case != "tri_rmat20" else np.ones(len(col))
    dev = torch.device("cuda", 0)
    Ap, Aj, Ax = (torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in (rp.astype(np.int32), col.astype(np.int32), val))
    Bp, Bj, Bx = Ap.clone(), Aj.clone(), Ax.clone()
    plats = [False] * facade.NUM_PLATFORMS
    plats[facade.BHSPARSE_HIP] = True
    bh = facade.bhsparse()
    assert bh.initPlatform(plats) == 0
    for k, v in opts.items():
        assert bh.set_option(k, v) == 0
    assert bh.initData_device(m, m, m, Aj.numel(), Ax, Ap, Aj, Bj.numel(), Bx, Bp, Bj) == 0
    out = {"case": case, "m": m, "nnzA": int(Aj.numel()), "options": opts}
    # the full multiply
    assert bh.set_option("kernel_stats", 0) == 0
    dms, wms = [], []
    for i in range(WARM + REPS):
        t0 = time.perf_counter()
        assert bh.spgemm() == 0
        w = (time.perf_counter() - t0) * 1e3
        if i >= WARM:
            dms.append(sum(bh.stage_ms))
            wms.append(w)
    out["full"] = {"device_ms": float(np.median(dms)), "wall_ms": float(np.median(wms)), "nnzCt": bh.nnzCt, "nnzC": bh.nnzC,
                   "class_state": bh.get_info("class_state")}
    assert bh.set_option("kernel_stats", 1) == 0
    assert bh.spgemm() == 0
    out["full"]["kernels"] = families(bh)
    dCp, dCj, dCx = bh.get_C_device()
    nnzC = bh.nnzC
    if case == "tri_rmat20":
        Mp, Mj, nnzM = Ap, Aj, int(Aj.numel())
    else:
        Mp, Mj, nnzM = dCp, dCj, nnzC                       # the library's own C pattern: no multiply runs from here on
    valC = torch.empty(nnzM, dtype=torch.float64, device=dev)
    assert bh.set_option("kernel_stats", 0) == 0
    dms, wms = [], []
    for i in range(WARM + REPS):
        t0 = time.perf_counter()
        assert bh.spgemm_masked_device(Mp, Mj, nnzM, valC) == 0
        w = (time.perf_counter() - t0) * 1e3
        if i >= WARM:
            dms.append(bh.masked_ms)
            wms.append(w)
    out["masked"] = {"device_ms": float(np.median(dms)), "wall_ms": float(np.median(wms)), "nnzM": nnzM, "nnzCt": bh.nnzCt,
                     "device_ms_range": [float(np.min(dms)), float(np.max(dms))]}
    if case == "tri_rmat20":
        out["masked"]["triangles"] = int(round(float(valC.sum().item())))
    else:
        Cj_h = np.empty(nnzC, np.int32)
        Cx_h = np.empty(nnzC, np.float64)
        assert bh.get_C(Cj_h, Cx_h) == 0                    # (the full product's C, still there after the masked calls)
        out["masked"]["equal_to_full"] = bool(np.array_equal(Cx_h, valC.cpu().numpy()))
    assert bh.set_option("kernel_stats", 1) == 0
    assert bh.spgemm_masked_device(Mp, Mj, nnzM, valC) == 0
    out["masked"]["kernels"] = families(bh)
    out["speedup_device"] = out["full"]["device_ms"] / out["masked"]["device_ms"]
    bh.free_mem()
    bh.freePlatform()
    return out


if __name__ == "__main__":
    cases = sys.argv[1:] or ["p27_128_class", "p27_128_general", "uniform", "banded", "tri_rmat20"]
    res = []
    for c in cases:
        res.append(run(c))
        torch.cuda.empty_cache()
    print(json.dumps({"tool": "masked_case", "reps": REPS, "results": res}))
