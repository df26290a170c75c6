"""CSR x dense (bhs_csr_spmv_device, bhs_csr_spmm_device) on device-resident inputs against two yardsticks that do not
depend on it, in the same process and on the same arrays: a device-to-device copy of A's three arrays, and the row sums
(bhs_csr_reduce_device, PLUS on ROWS), which read the row pointer and the values -- everything the vector product reads
but the column indices -- and gather nothing; prints one JSON line.

    python tools/spmv_case.py [case ...]      cases: p27_128 uniform tri_rmat20 (default: all three)

Both builds (double, float), k = 1 (the vector call), 4 and 16 (row-major X and Y, ld = k), alpha = 1, beta = 0.  Per case,
after 3 warm-ups, medians and minima of REPS (default 12) runs with per-kernel timers off, device time from the event pair
around the whole call (validation and the queue lengths' round trip included).  Achieved bytes per second are over the
compulsory bytes -- 4 B per row of row pointer, 4 B + one value per entry, one value per element of X and of Y; the row
sums: 4 B per row, one value per entry and per row -- and are set beside the copy's rate of the same run.  "rows_plus_scaled"
is the row sums' time times (4 + V) / V, V the value's bytes: what the vector product would take at the row sums' rate if
the gathers of x were free."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from benchmark_spgemm_using_csr_amd import _lib, dense, facade  # noqa: E402
from tools.extract_case import REPS, copy_ms, stat, timed  # noqa: E402
from tools.reduce_case import make  # noqa: E402

KS = (1, 4, 16)


def run(case, bh, dev, dtype):
    rp, col = make(case)
    m = n = len(rp) - 1
    nnz = len(col)
    V = np.dtype(dtype).itemsize
    tdt = torch.float32 if V == 4 else torch.float64
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)   # noqa: E731
    rng = np.random.default_rng(1)
    Ap, Aj, Ax = up(rp.astype(np.int32)), up(col.astype(np.int32)), up((1.0 + rng.random(nnz)).astype(dtype))
    Zp, Zj, Zx = torch.empty_like(Ap), torch.empty_like(Aj), torch.empty_like(Ax)
    kmax = max(KS)
    X = up((1.0 + rng.random(n * kmax)).astype(dtype))
    Y = torch.empty(m * kmax, dtype=tdt, device=dev)
    torch.cuda.synchronize()
    assert bh.set_option("kernel_stats", 0) == 0
    lens = np.diff(rp.astype(np.int64))
    out = {"case": case, "value_bytes": V, "m": m, "nnz": nnz, "longest_row": int(lens.max()),
           "rows_beyond_32": int(np.count_nonzero(lens > 32)), "rows_beyond_1024": int(np.count_nonzero(lens > 1024))}
    cp = copy_ms([(Zp, Ap), (Zj, Aj), (Zx, Ax)])
    copy_bytes = 2 * (4 * (m + 1) + (4 + V) * nnz)
    copy_rate = copy_bytes / (np.median(cp) * 1e6)
    out["device_copy"] = dict(stat(cp), bytes=copy_bytes, achieved_GBps=copy_rate)

    def families(prefix):
        return {s["name"]: {"launches": s["launches"], "ms": round(s["ms"], 4)} for s in bh.kernel_stats()
                if s["name"].startswith(prefix) and s["launches"]}

    def measure(name, call, ms, prefix, compulsory):
        _, d = timed(call, ms)
        assert bh.set_option("kernel_stats", 1) == 0
        call()
        fam = families(prefix)
        assert bh.set_option("kernel_stats", 0) == 0
        med = float(np.median(d))
        out[name] = dict(stat(d), kernels=fam, compulsory_bytes=compulsory, achieved_GBps=compulsory / (med * 1e6),
                         share_of_copy_rate=compulsory / (med * 1e6) / copy_rate)
        return med

    def rows_plus():
        assert bh.csr_reduce_raw_device(m, n, nnz, Ax, Ap, Aj, _lib.BHS_AXIS_ROWS, _lib.BHS_RED_PLUS, 0, Y) == 0
    med = measure("rows_plus", rows_plus, lambda: bh.reduce_ms, "reduce_", 4 * (m + 1) + V * nnz + V * m)
    out["rows_plus_scaled"] = {"median_ms": med * (4 + V) / V}
    for k in KS:
        def product(k=k):
            if k == 1:
                assert dense.csr_spmv_raw_device(bh, m, n, nnz, Ax, Ap, Aj, 1.0, X, 0.0, Y) == 0
            else:
                assert dense.csr_spmm_raw_device(bh, m, n, nnz, Ax, Ap, Aj, k, 1.0, X, k, 0.0, Y, k) == 0
        measure("spmv" if k == 1 else "spmm_k%d" % k, product, lambda: bh.spmv_ms, "spmv_" if k == 1 else "spmm_",
                4 * (m + 1) + (4 + V) * nnz + V * k * (n + m))
    # a spot check of what was timed: row 0 and the last row of the k = 16 product against numpy
    Yh = Y.view(m, kmax).cpu().numpy()
    Xh, Axh = X.view(n, kmax).cpu().numpy().astype(np.float64), Ax.cpu().numpy().astype(np.float64)
    for i in (0, m - 1):
        ref = (Axh[rp[i]:rp[i + 1], None] * Xh[col[rp[i]:rp[i + 1]]]).sum(axis=0)
        assert np.allclose(Yh[i], ref, rtol=1e-5 if V == 4 else 1e-12), (case, i)
    return out


if __name__ == "__main__":
    cases = sys.argv[1:] or ["p27_128", "uniform", "tri_rmat20"]
    dev = torch.device("cuda", 0)
    plats = [False] * facade.NUM_PLATFORMS
    plats[facade.BHSPARSE_HIP] = True
    res = []
    for dtype in (np.float64, np.float32):
        bh = facade.bhsparse(value_dtype=dtype)
        assert bh.initPlatform(plats) == 0
        for c in cases:
            res.append(run(c, bh, dev, dtype))
            torch.cuda.empty_cache()
        bh.freePlatform()
    print(json.dumps({"tool": "spmv_case", "reps": REPS, "device": torch.cuda.get_device_name(0), "source_digest": _lib.source_digest(),
                      "results": res}))
