"""The masked multiply over a semiring (bhs_spgemm_semiring_masked_device) beside the plus-times masked multiply
(bhs_spgemm_masked_device) on the same device-resident data in the same run, and bhs_spgemm_semiring beside bhs_spgemm;
prints one JSON line.

    python tools/semiring_case.py [case ...]      cases: uniform tri_rmat20 (default: both)

uniform: 2^20 rows of 8 uniformly random columns, M = pattern(A^2) (the library's own C arrays).  tri_rmat20: the R-MAT 2^20
graph symmetrised and made strictly lower, M = L (triangle counting).  Unit values, so that every result can be checked
against the plus-times masked values c (the products landing on an entry): plus-pair = c, or-and = (c > 0),
min-plus = 2 where c > 0 and +Inf elsewhere.  Per call: WARM (3) warm-ups, then the median and the minimum of REPS
(default 12) device times with per-kernel timers off; one extra run with kernel_stats=1 gives the family breakdown.  The
yardstick is the plus-times masked call measured beside the others -- never the new code against itself."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from benchmark_spgemm_using_csr_amd import _lib, facade, gallery  # noqa: E402

REPS = int(os.environ.get("REPS", "12"))
WARM = 3
SEMIRINGS = (("min_plus", _lib.BHS_SR_MIN_PLUS), ("or_and", _lib.BHS_SR_OR_AND), ("plus_pair", _lib.BHS_SR_PLUS_PAIR))


def lower_triangle(rp, col):
    n = len(rp) - 1
    r = np.repeat(np.arange(n), np.diff(rp))
    rows = np.concatenate([r, col]).astype(np.int64)
    cols = np.concatenate([col, r]).astype(np.int64)
    key = np.unique(rows[rows > cols] * n + cols[rows > cols])    # strictly lower, duplicates collapsed, rows ascending
    rp = np.zeros(n + 1, np.int64)
    np.cumsum(np.bincount(key // n, minlength=n), out=rp[1:])
    return rp, key % n


def families(bh):
    return {s["name"]: {"launches": s["launches"], "ms": round(s["ms"], 4), "rows": s["rows"], "products": s["products"]}
            for s in bh.kernel_stats()}


def timed(bh, call, read_ms):
    assert bh.set_option("kernel_stats", 0) == 0
    ms = []
    for i in range(WARM + REPS):
        assert call() == 0
        if i >= WARM:
            ms.append(read_ms())
    assert bh.set_option("kernel_stats", 1) == 0
    assert call() == 0
    return {"device_ms": float(np.median(ms)), "device_ms_min": float(np.min(ms)), "device_ms_max": float(np.max(ms)),
            "kernels": families(bh)}


def run(case):
    if case == "uniform":
        rp, col = gallery.uniform_csr()
    elif case == "tri_rmat20":
        rp, col = lower_triangle(*gallery.rmat_csr(scale=20))
    else:
        raise ValueError(case)
    m = len(rp) - 1
    dev = torch.device("cuda", 0)
    Ap, Aj, Ax = (torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in (rp.astype(np.int32), col.astype(np.int32),
                                                                               np.ones(len(col))))
    Bp, Bj, Bx = Ap.clone(), Aj.clone(), Ax.clone()
    plats = [False] * facade.NUM_PLATFORMS
    plats[facade.BHSPARSE_HIP] = True
    bh = facade.bhsparse()
    assert bh.initPlatform(plats) == 0
    assert bh.initData_device(m, m, m, Aj.numel(), Ax, Ap, Aj, Bj.numel(), Bx, Bp, Bj) == 0
    out = {"case": case, "m": m, "nnzA": int(Aj.numel())}
    if case == "uniform":
        # the full product: bhs_spgemm, then bhs_spgemm_semiring(MIN_PLUS) with both parts of its ms_out
        full = timed(bh, bh.spgemm, lambda: sum(bh.stage_ms))
        parts = []
        sr_full = timed(bh, lambda: bh.spgemm_semiring(_lib.BHS_SR_MIN_PLUS),
                        lambda: parts.append((bh.multiply_ms, bh.semiring_ms)) or bh.multiply_ms + bh.semiring_ms)
        sr_full["multiply_ms"] = float(np.median([p[0] for p in parts]))
        sr_full["revalue_ms"] = float(np.median([p[1] for p in parts]))
        out["spgemm"] = full
        out["spgemm_semiring_min_plus"] = sr_full
        out["nnzCt"], out["nnzC"] = bh.nnzCt, bh.nnzC
        Mp, Mj, _ = bh.get_C_device()                       # the library's own C pattern
        nnzM = bh.nnzC
    else:
        Mp, Mj, nnzM = Ap, Aj, int(Aj.numel())
    out["nnzM"] = nnzM
    valC = torch.empty(nnzM, dtype=torch.float64, device=dev)
    out["masked_plus_times"] = timed(bh, lambda: bh.spgemm_masked_device(Mp, Mj, nnzM, valC), lambda: bh.masked_ms)
    out["nnzCt"] = bh.nnzCt
    count = valC.clone()
    if case == "tri_rmat20":
        out["triangles"] = int(round(float(count.sum().item())))
    want = {"plus_pair": count, "or_and": (count > 0).to(torch.float64),
            "min_plus": torch.where(count > 0, torch.full_like(count, 2.0), torch.full_like(count, float("inf")))}
    for name, code in SEMIRINGS:
        valC.fill_(-7.0)
        r = timed(bh, lambda: bh.spgemm_semiring_masked_device(code, Mp, Mj, nnzM, valC), lambda: bh.semiring_ms)
        r["agrees_with_plus_times"] = bool(torch.equal(valC, want[name]))
        r["ratio_to_plus_times"] = r["device_ms"] / out["masked_plus_times"]["device_ms"]
        out["masked_" + name] = r
    bh.free_mem()
    bh.freePlatform()
    return out


if __name__ == "__main__":
    cases = sys.argv[1:] or ["uniform", "tri_rmat20"]
    res = []
    for c in cases:
        res.append(run(c))
        torch.cuda.empty_cache()
    print(json.dumps({"tool": "semiring_case", "reps": REPS, "results": res}))
