"""The transpose (bhs_csr_transpose_device with pattern, values and perm; bhs_csr_transpose_values_device) on device-resident
inputs against two yardsticks that do not depend on it: the sparse add with an empty Y on the same X (a streaming pass over
the same arrays) and a device-to-device copy; prints one JSON line.

    python tools/transpose_case.py [case ...]      cases: p27_128 uniform banded powerlaw (default: all)

Per case, in one process: after 3 warm-ups, medians and minima of REPS (default 12) runs with per-kernel timers off --
device time of the transpose, of the values-only call and of the add's numeric call, wall time of the add's symbolic call
(it has no device timer of its own).  One extra transpose with kernel_stats=1 gives the kernel families.  Achieved bytes per
second are over the compulsory bytes: 4(m+1) + 12 nnz read, 4(n+1) + 12 nnz written (the perm's 4 nnz on top are named)."""
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
    if case == "banded":
        return gallery.banded_csr()
    if case == "powerlaw":
        return gallery.powerlaw_csr(1000005, 1000005, 3105536, 4700)
    raise ValueError(case)


def stat(xs):
    return {"median_ms": float(np.median(xs)), "min_ms": float(np.min(xs))}


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


def stream_copy_GBs(dev, nbytes=1 << 28):
    src = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    dst = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    src.zero_()
    ms = []
    for i in range(WARM + REPS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        dst.copy_(src)
        b.record()
        torch.cuda.synchronize()
        if i >= WARM:
            ms.append(a.elapsed_time(b))
    return 2.0 * nbytes / (float(np.median(ms)) * 1e6)


def run(case, bh, dev):
    rp, col = make(case)
    m = n = len(rp) - 1
    nnz = len(col)
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)   # noqa: E731
    Xp, Xj, Xx = up(rp.astype(np.int32)), up(col.astype(np.int32)), up(gallery.fill_values(nnz))
    Tp = torch.empty(n + 1, dtype=torch.int32, device=dev)
    Tj = torch.empty(nnz, dtype=torch.int32, device=dev)
    Tx = torch.empty(nnz, dtype=torch.float64, device=dev)
    pm = torch.empty(nnz, dtype=torch.int32, device=dev)
    Zp = torch.empty(m + 1, dtype=torch.int32, device=dev)
    Zj = torch.empty(nnz, dtype=torch.int32, device=dev)
    Zx = torch.empty(nnz, dtype=torch.float64, device=dev)
    Yp = torch.zeros(m + 1, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    assert bh.set_option("kernel_stats", 0) == 0
    out = {"case": case, "m": m, "nnz": nnz}

    def full():
        assert bh.csr_transpose_raw_device(m, n, nnz, Xx, Xp, Xj, Tp, Tj, Tx, pm) == 0
    _, tr_ms = timed(full, lambda: bh.transpose_ms)
    out["longest_T_row"] = int(np.diff(Tp.cpu().numpy().astype(np.int64)).max())

    def vals():
        bh.csr_transpose_values_device(Xx, pm, Tx)
    _, val_ms = timed(vals, lambda: bh.transpose_ms)

    def add_sym():
        assert bh.csr_add_symbolic_device(m, n, nnz, Xp, Xj, 0, Yp, None, Zp)[0] == 0

    def add_num():
        assert bh.csr_add_numeric_device(m, n, 1.0, nnz, Xx, Xp, Xj, 1.0, 0, None, Yp, None, Zp, Zj, Zx) == 0
    sym, _ = timed(add_sym)
    _, num = timed(add_num, lambda: bh.add_ms)
    assert bh.set_option("kernel_stats", 1) == 0
    full()
    fam = {s["name"]: {"launches": s["launches"], "ms": round(s["ms"], 4), "rows": s["rows"]} for s in bh.kernel_stats()
           if s["name"].startswith("transpose_") and s["launches"]}
    assert bh.set_option("kernel_stats", 0) == 0
    compulsory = 4 * (m + 1) + 12 * nnz + 4 * (n + 1) + 12 * nnz
    t_med, v_med = float(np.median(tr_ms)), float(np.median(val_ms))
    add_total = float(np.median(sym) + np.median(num))
    out["transpose"] = dict(stat(tr_ms), kernels=fam, compulsory_bytes=compulsory, perm_bytes=4 * nnz,
                            achieved_GBps=compulsory / (t_med * 1e6))
    out["values_only"] = dict(stat(val_ms), bytes=20 * nnz, achieved_GBps=20 * nnz / (v_med * 1e6))
    out["add_empty_y"] = {"symbolic_wall": stat(sym), "numeric": stat(num), "total_median_ms": add_total}
    out["transpose_over_add"] = t_med / add_total
    out["values_over_transpose"] = v_med / t_med
    return out


if __name__ == "__main__":
    cases = sys.argv[1:] or ["p27_128", "uniform", "banded", "powerlaw"]
    dev = torch.device("cuda", 0)
    plats = [False] * facade.NUM_PLATFORMS
    plats[facade.BHSPARSE_HIP] = True
    bh = facade.bhsparse()
    assert bh.initPlatform(plats) == 0
    res = []
    for c in cases:
        res.append(run(c, bh, dev))
        torch.cuda.empty_cache()
    copy = stream_copy_GBs(dev)
    bh.freePlatform()
    print(json.dumps({"tool": "transpose_case", "reps": REPS, "stream_copy_GBs": copy, "results": res}))
