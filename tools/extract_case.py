"""The extraction Z = X(rows, cols) (bhs_csr_extract_{symbolic,numeric}_device) on device-resident inputs against two
yardsticks that do not depend on it, in the same process and on the same arrays: a device-to-device copy of X's three arrays
and the entry selection (bhs_csr_select_*) with a rule that keeps a comparable number of entries; prints one JSON line.

    python tools/extract_case.py [case ...]      cases: p27_128 uniform (default: both)

Three extractions per case:
    gather   the row gather X(p, :) for a random permutation p (no column map)
    cf       a C/F split: rows = the odd indices, cols = the even indices ascending (about a quarter of the entries survive)
    permute  X(p, p) for a random p: every row with two entries or more is put in order
Per extraction, after 3 warm-ups, medians and minima of REPS (default 12) runs with per-kernel timers off: device time of
the numeric call (event pair around the whole call, validation and count pass included), wall time of the symbolic call (it
has no device timer of its own).  The selection is timed the same way: abs_tol 0.5 keeps every entry (beside gather and
permute), abs_tol 7.5 keeps the values 8 and 9, two in nine (beside cf).  Achieved bytes per second of a numeric call are
over its compulsory bytes: 12 B read per entry of a touched X row, 4 B of map gather per such entry where cols is given,
16 B (colIndZ, valZ, perm) written per survivor, 4 B per row index and 8 B per Z row of row pointers."""
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
        return gallery.uniform_csr(1 << 20, 8)
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


def copy_ms(pairs):
    ms = []
    for i in range(WARM + REPS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for dst, src in pairs:
            dst.copy_(src)
        b.record()
        torch.cuda.synchronize()
        if i >= WARM:
            ms.append(a.elapsed_time(b))
    return ms


def run(case, bh, dev):
    rp, col = make(case)
    m = n = len(rp) - 1
    nnz = len(col)
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)   # noqa: E731
    Xp, Xj, Xx = up(rp.astype(np.int32)), up(col.astype(np.int32)), up(gallery.fill_values(nnz))
    rng = np.random.default_rng(1)
    p = up(rng.permutation(n).astype(np.int32))
    odd, even = up(np.arange(1, n, 2, dtype=np.int32)), up(np.arange(0, n, 2, dtype=np.int32))
    Zp = torch.empty(m + 1, dtype=torch.int32, device=dev)
    Zj = torch.empty(nnz, dtype=torch.int32, device=dev)
    Zx = torch.empty(nnz, dtype=torch.float64, device=dev)
    pm = torch.empty(nnz, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    assert bh.set_option("kernel_stats", 0) == 0
    out = {"case": case, "m": m, "nnz": nnz}
    cp = copy_ms([(Zp, Xp), (Zj, Xj), (Zx, Xx)])
    out["device_copy"] = dict(stat(cp), bytes=2 * (4 * (m + 1) + 12 * nnz), achieved_GBps=2 * (4 * (m + 1) + 12 * nnz) / (np.median(cp) * 1e6))

    lens = np.diff(rp.astype(np.int64))
    for name, rows, cols in (("gather", p, None), ("cf", odd, even), ("permute", p, p)):
        mI = rows.numel()
        nJ = n if cols is None else cols.numel()
        got = {}

        def sym():
            err, got["nnzZ"] = bh.csr_extract_symbolic_device(m, n, nnz, Xp, Xj, mI, rows, nJ, cols, Zp)
            assert err == 0

        def num():
            assert bh.csr_extract_numeric_device(m, n, nnz, Xx, Xp, Xj, mI, rows, nJ, cols, got["nnzZ"], Zp, Zj, Zx, pm) == 0
        s_wall, _ = timed(sym)
        _, n_dev = timed(num, lambda: bh.extract_ms)
        reordered = bh.get_info("extract_reordered_rows")
        assert bh.set_option("kernel_stats", 1) == 0
        num()
        fam = {s["name"]: {"launches": s["launches"], "ms": round(s["ms"], 4), "rows": s["rows"]} for s in bh.kernel_stats()
               if s["name"].startswith("extract_") and s["launches"]}
        assert bh.set_option("kernel_stats", 0) == 0
        touched = int(lens[rows.cpu().numpy()].sum())
        compulsory = 12 * touched + (4 * touched if cols is not None else 0) + 16 * got["nnzZ"] + 4 * mI + 8 * (mI + 1)
        med = float(np.median(n_dev))
        out[name] = {"mI": mI, "nJ": nJ, "nnzZ": got["nnzZ"], "touched_entries": touched, "reordered_rows": int(reordered),
                     "symbolic_wall": stat(s_wall), "numeric": stat(n_dev), "kernels": fam, "compulsory_bytes": compulsory,
                     "achieved_GBps": compulsory / (med * 1e6), "numeric_over_copy": med / float(np.median(cp))}

    for name, tol in (("select_keep_all", 0.5), ("select_two_in_nine", 7.5)):
        spec = facade.select_spec(abs_tol=tol)
        got = {}

        def ssym():
            err, got["nnzZ"] = bh.csr_select_symbolic_device(m, n, nnz, Xx, Xp, Xj, spec, Zp)
            assert err == 0

        def snum():
            assert bh.csr_select_numeric_device(m, n, nnz, Xx, Xp, Xj, spec, Zp, Zj, Zx) == 0
        s_wall, _ = timed(ssym)
        _, n_dev = timed(snum, lambda: bh.select_ms)
        compulsory = 12 * nnz + 12 * got["nnzZ"] + 8 * (m + 1)
        med = float(np.median(n_dev))
        out[name] = {"nnzZ": got["nnzZ"], "symbolic_wall": stat(s_wall), "numeric": stat(n_dev), "compulsory_bytes": compulsory,
                     "achieved_GBps": compulsory / (med * 1e6)}
    out["gather_over_select_keep_all"] = out["gather"]["numeric"]["median_ms"] / out["select_keep_all"]["numeric"]["median_ms"]
    out["permute_over_select_keep_all"] = out["permute"]["numeric"]["median_ms"] / out["select_keep_all"]["numeric"]["median_ms"]
    out["cf_over_select_two_in_nine"] = out["cf"]["numeric"]["median_ms"] / out["select_two_in_nine"]["numeric"]["median_ms"]
    return out


if __name__ == "__main__":
    cases = sys.argv[1:] or ["p27_128", "uniform"]
    dev = torch.device("cuda", 0)
    plats = [False] * facade.NUM_PLATFORMS
    plats[facade.BHSPARSE_HIP] = True
    bh = facade.bhsparse()
    assert bh.initPlatform(plats) == 0
    res = []
    for c in cases:
        res.append(run(c, bh, dev))
        torch.cuda.empty_cache()
    bh.freePlatform()
    print(json.dumps({"tool": "extract_case", "reps": REPS, "results": res}))
