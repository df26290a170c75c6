"""The sampled dense-dense product (bhs_csr_sddmm_device) on device-resident inputs against three yardsticks in the same
process and on the same arrays: a device-to-device copy of M's three arrays, bhs_csr_spmm_device at the same k on the same
pattern -- the same gathers of a dense row per entry, summed in the other direction --, and the torch route
(X[rows] * Y[cols]).sum(1), which materialises both gathers; then amg.affinity_strength_device beside amg.strength_device
on two operators.  Prints one JSON line.

    python tools/sddmm_case.py [case ...]      cases: p27_128 uniform tri_rmat20 affinity (default: all four)

Both builds (double, float), k = 1, 4, 16, 64 (row-major X and Y, ld = k), alpha = 1, beta = 0, no TIMES_M.  Per case, after
3 warm-ups, medians and minima of REPS (default 12) runs with per-kernel timers off, device time from the event pair around
the whole call (validation and the queue lengths' round trip included); the torch route between two torch events.
Achieved bytes per second are over the compulsory bytes -- 4 B per row of row pointer, 4 B and one value written per entry,
one value per element of X and of Y -- and are set beside the copy's rate of the same run.  Where torch cannot allocate
its intermediates the route is reported as not measured."""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from benchmark_spgemm_using_csr_amd import _lib, amg, dense, facade, gallery  # noqa: E402
from tools.extract_case import REPS, WARM, copy_ms, stat, timed  # noqa: E402
from tools.reduce_case import make  # noqa: E402

KS = (1, 4, 16, 64)


def run(case, bh, dev, dtype):
    rp, col = make(case)
    m = n = len(rp) - 1
    nnz = len(col)
    V = np.dtype(dtype).itemsize
    tdt = torch.float32 if V == 4 else torch.float64
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)   # noqa: E731
    rng = np.random.default_rng(1)
    Mp, Mj, Mx = up(rp.astype(np.int32)), up(col.astype(np.int32)), up((1.0 + rng.random(nnz)).astype(dtype))
    Cp, Cj, Cx = torch.empty_like(Mp), torch.empty_like(Mj), torch.empty_like(Mx)
    rows = torch.repeat_interleave(torch.arange(m, device=dev), (Mp[1:] - Mp[:-1]).long())
    cols = Mj.long()
    kmax = max(KS)
    Xall, Yall = up((1.0 + rng.random(m * kmax)).astype(dtype)), up((1.0 + rng.random(n * kmax)).astype(dtype))
    Z = torch.empty(nnz, dtype=tdt, device=dev)
    Out = torch.empty(m * kmax, dtype=tdt, device=dev)
    torch.cuda.synchronize()
    assert bh.set_option("kernel_stats", 0) == 0
    lens = np.diff(rp.astype(np.int64))
    out = {"case": case, "value_bytes": V, "m": m, "nnz": nnz, "longest_row": int(lens.max()),
           "rows_beyond_32": int(np.count_nonzero(lens > 32)), "rows_beyond_1024": int(np.count_nonzero(lens > 1024))}
    cp = copy_ms([(Cp, Mp), (Cj, Mj), (Cx, Mx)])
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

    for k in KS:
        X, Y = Xall[:m * k].view(m, k), Yall[:n * k].view(n, k)

        def sddmm(k=k, X=X, Y=Y):
            assert dense.csr_sddmm_raw_device(bh, m, n, nnz, None, Mp, Mj, k, 1.0, X, k, Y, k, 0.0, Z, 0) == 0

        def spmm(k=k, Y=Y):
            assert dense.csr_spmm_raw_device(bh, m, n, nnz, Mx, Mp, Mj, k, 1.0, Y, k, 0.0, Out, k) == 0
        sd = measure("sddmm_k%d" % k, sddmm, lambda: bh.sddmm_ms, "sddmm_", 4 * (m + 1) + (4 + V) * nnz + V * k * (n + m))
        mm = measure("spmm_k%d" % k, spmm, lambda: bh.spmv_ms, "spm", 4 * (m + 1) + (4 + V) * nnz + V * k * (n + m))
        try:
            ms = []
            for i in range(WARM + REPS):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                T = (X[rows] * Y[cols]).sum(1)
                b.record()
                torch.cuda.synchronize()
                if i >= WARM:
                    ms.append(a.elapsed_time(b))
            out["torch_k%d" % k] = stat(ms)
            tm = float(np.median(ms))
            sddmm()
            torch.cuda.synchronize()
            assert torch.allclose(Z, T, rtol=1e-5 if V == 4 else 1e-12), (case, k)   # what was timed is the product
            del T
        except torch.cuda.OutOfMemoryError:
            out["torch_k%d" % k] = "not measured: torch could not allocate the gathered rows"
            tm = None
        torch.cuda.empty_cache()
        out["ratios_k%d" % k] = {"sddmm_over_spmm": sd / mm, "sddmm_over_torch": None if tm is None else sd / tm}
    return out


def aniso(nx, ny, eps):
    """the 5-point operator with the y-coupling scaled by eps: (rowPtr, colInd, val) with sorted rows"""
    import scipy.sparse as sp
    Tx = sp.diags([-np.ones(nx - 1), 2 * np.ones(nx), -np.ones(nx - 1)], [-1, 0, 1])
    Ty = sp.diags([-np.ones(ny - 1), 2 * np.ones(ny), -np.ones(ny - 1)], [-1, 0, 1])
    A = (sp.kron(sp.identity(ny), Tx) + eps * sp.kron(Ty, sp.identity(nx))).tocsr()
    A.sort_indices()
    return A.indptr, A.indices, A.data


def poisson27(nx):
    rp, col = gallery.poisson_csr("poisson27pt", nx, nx, nx)
    r = np.repeat(np.arange(len(rp) - 1), np.diff(rp))
    return rp, col, np.where(col == r, 26.0, -1.0)


def run_affinity(bh, dev, dtype):
    out = {"case": "affinity", "value_bytes": np.dtype(dtype).itemsize}
    up = lambda x, dt: torch.from_numpy(np.ascontiguousarray(x, dt)).to(dev)   # noqa: E731
    for name, (rp, col, val) in (("aniso_1024", aniso(1024, 1024, 1.0 / 64)), ("p27_128", poisson27(128))):
        n = len(rp) - 1
        A = (up(rp, np.int32), up(col, np.int32), up(val, dtype))
        res = {"n": n, "nnz": len(col)}
        for what, call, ms in (("affinity_strength", lambda: amg.affinity_strength_device(bh, n, A), lambda: bh.affinity_ms),
                               ("strength", lambda: amg.strength_device(bh, n, A, 0.25), lambda: bh.strength_ms)):
            wall, devms = [], []
            for i in range(1 + 3):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                S = call()
                torch.cuda.synchronize()
                if i >= 1:
                    wall.append((time.perf_counter() - t0) * 1e3)
                    devms.append(ms())
            res[what] = {"wall_median_ms": float(np.median(wall)), "library_calls_device_median_ms": float(np.median(devms)),
                         "nnz_S": int(S[1].numel())}
        out[name] = res
        torch.cuda.empty_cache()
    return out


if __name__ == "__main__":
    cases = sys.argv[1:] or ["p27_128", "uniform", "tri_rmat20", "affinity"]
    dev = torch.device("cuda", 0)
    plats = [False] * facade.NUM_PLATFORMS
    plats[facade.BHSPARSE_HIP] = True
    res = []
    for dtype in (np.float64, np.float32):
        bh = facade.bhsparse(value_dtype=dtype)
        assert bh.initPlatform(plats) == 0
        for c in cases:
            res.append(run_affinity(bh, dev, dtype) if c == "affinity" else run(c, bh, dev, dtype))
            torch.cuda.empty_cache()
        bh.freePlatform()
    print(json.dumps({"tool": "sddmm_case", "reps": REPS, "device": torch.cuda.get_device_name(0), "source_digest": _lib.source_digest(),
                      "results": res}))
