"""The entry selection (bhs_csr_select_*_device, bhs_spgemm_select_device) on the product's own device arrays against the
sparse add with an empty Y on the same X (the same bytes: count 4·nnz read, fill 12·nnz read + 12·nnz written); prints
one JSON line.

    python tools/select_case.py [case ...]      cases: p27_128 uniform powerlaw (default: all)

Per case, in one process, X = the C of A·A: the add Z = X + 0 (symbolic + numeric), the keep-everything selection
(BHS_SEL_BAND over the whole int64 range), the selection with top_k = 32, and -- p27_128 only -- bhs_spgemm_select_device
with ABS 0 (nothing dropped: the count pass alone) beside bhs_spgemm.  After 3 warm-ups, medians and minima of REPS
(default 12) runs with per-kernel timers off: wall time of the symbolic calls (they have no device timer of their own),
device time of the numeric calls.  One extra run of each with kernel_stats=1 gives the kernel families."""
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
    if case == "p27_128":
        return gallery.poisson_csr("poisson27pt", 128, 128, 128)
    if case == "uniform":
        return gallery.uniform_csr()
    if case == "powerlaw":
        return gallery.powerlaw_csr(1000005, 1000005, 3105536, 4700)
    raise ValueError(case)


def stat(xs):
    return {"median_ms": float(np.median(xs)), "min_ms": float(np.min(xs))}


def families(bh, prefix):
    return {s["name"]: {"launches": s["launches"], "ms": round(s["ms"], 4), "rows": s["rows"]} for s in bh.kernel_stats()
            if s["name"].startswith(prefix)}


def timed(fn, after=None):
    wall, dev = [], []
    for i in range(WARM + REPS):
        t0 = time.perf_counter()
        fn()
        w = (time.perf_counter() - t0) * 1e3
        if i >= WARM:
            wall.append(w)
            if after:
                dev.append(after())
    return wall, dev


def run(case):
    rp, col = make(case)
    m = len(rp) - 1
    val = gallery.fill_values(len(col))
    dev = torch.device("cuda", 0)
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)   # noqa: E731
    Ap, Aj, Ax = up(rp.astype(np.int32)), up(col.astype(np.int32)), up(val)
    Bp, Bj, Bx = Ap.clone(), Aj.clone(), Ax.clone()
    plats = [False] * facade.NUM_PLATFORMS
    plats[facade.BHSPARSE_HIP] = True
    bh = facade.bhsparse()
    assert bh.initPlatform(plats) == 0
    assert bh.initData_device(m, m, m, Aj.numel(), Ax, Ap, Aj, Bj.numel(), Bx, Bp, Bj) == 0
    assert bh.set_option("kernel_stats", 0) == 0
    out = {"case": case, "m": m, "nnzA": int(Aj.numel())}

    def plain():
        assert bh.spgemm() == 0
    _, mul = timed(plain, lambda: sum(bh.stage_ms))
    nnzX = bh.nnzC
    out["spgemm"] = dict(stat(mul), nnzCt=bh.nnzCt, nnzC=nnzX)
    if case == "p27_128":
        zero = facade.select_spec(abs_tol=0.0)

        def fused():
            assert bh.spgemm_select_device(zero) == 0
        wall, sel = timed(fused, lambda: bh.select_ms)
        assert bh.get_info("select_dropped") == 0
        out["spgemm_select_abs0"] = {"select": stat(sel), "wall": stat(wall)}
        assert bh.spgemm() == 0
    pCp, pCj, pCx = bh.get_C_device()
    Zp = torch.empty(m + 1, dtype=torch.int32, device=dev)
    Zj = torch.empty(max(nnzX, 1), dtype=torch.int32, device=dev)
    Zx = torch.empty(max(nnzX, 1), dtype=torch.float64, device=dev)
    Yp = torch.zeros(m + 1, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    lens = np.diff(bh.get_rowptrC().astype(np.int64))
    out["longest_row"] = int(lens.max())

    # the yardstick: Z = X + 0
    def add_sym():
        assert bh.csr_add_symbolic_device(m, m, nnzX, pCp, pCj, 0, Yp, None, Zp)[0] == 0

    def add_num():
        assert bh.csr_add_numeric_device(m, m, 1.0, nnzX, pCx, pCp, pCj, 1.0, 0, None, Yp, None, Zp, Zj, Zx) == 0
    sym, _ = timed(add_sym)
    _, num = timed(add_num, lambda: bh.add_ms)
    assert bh.set_option("kernel_stats", 1) == 0
    add_sym()
    fam = families(bh, "add_")
    add_num()
    fam.update(families(bh, "add_"))
    assert bh.set_option("kernel_stats", 0) == 0
    out["add_empty_y"] = {"symbolic_wall": stat(sym), "numeric": stat(num), "kernels": fam,
                          "total_median_ms": float(np.median(sym) + np.median(num))}

    for label, spec in (("select_keep_all", facade.select_spec(band=(None, None))), ("select_top32", facade.select_spec(top_k=32))):
        nz = [0]

        def sel_sym():
            err, nz[0] = bh.csr_select_symbolic_device(m, m, nnzX, pCx, pCp, pCj, spec, Zp)
            assert err == 0

        def sel_num():
            assert bh.csr_select_numeric_device(m, m, nnzX, pCx, pCp, pCj, spec, Zp, Zj, Zx) == 0
        sym, _ = timed(sel_sym)
        _, num = timed(sel_num, lambda: bh.select_ms)
        assert bh.set_option("kernel_stats", 1) == 0
        sel_sym()
        fam = families(bh, "select_")
        sel_num()
        fam2 = families(bh, "select_")
        assert bh.set_option("kernel_stats", 0) == 0
        count_bytes = (12 if label == "select_top32" else 4) * nnzX + 8 * m
        fill_bytes = 12 * nnzX + 12 * nz[0] + 8 * m
        total = float(np.median(sym) + np.median(num))
        out[label] = {"symbolic_wall": stat(sym), "numeric": stat(num), "nnzZ": nz[0], "symbolic_kernels": fam, "numeric_kernels": fam2,
                      "total_median_ms": total, "count_bytes": count_bytes, "fill_bytes": fill_bytes,
                      "count_achieved_GBps": count_bytes / (float(np.median(sym)) * 1e6),
                      "fill_achieved_GBps": fill_bytes / (float(np.median(num)) * 1e6),
                      "over_add": total / out["add_empty_y"]["total_median_ms"]}
    out["top32_over_keep_all"] = out["select_top32"]["total_median_ms"] / out["select_keep_all"]["total_median_ms"]
    bh.free_mem()
    bh.freePlatform()
    return out


if __name__ == "__main__":
    cases = sys.argv[1:] or ["p27_128", "uniform", "powerlaw"]
    res = []
    for c in cases:
        res.append(run(c))
        torch.cuda.empty_cache()
    print(json.dumps({"tool": "select_case", "reps": REPS, "results": res}))
