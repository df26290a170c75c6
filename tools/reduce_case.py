"""The reductions and the diagonal scaling (bhs_csr_reduce_device, bhs_csr_scale_device) on device-resident inputs against
two yardsticks that do not depend on them, in the same process and on the same arrays: a device-to-device copy of X's three
arrays and the entry selection (bhs_csr_select_*) with a rule that keeps every entry; prints one JSON line.

    python tools/reduce_case.py [case ...]      cases: p27_128 uniform tri_rmat20 (default: all three)

tri_rmat20 is the lower triangle of the symmetrised R-MAT 2^20 graph (the mask of the triangle count): its hub columns are
the contended case of axis COLS.  Per case, after 3 warm-ups, medians and minima of REPS (default 12) runs with per-kernel
timers off, device time from the event pair around the whole call: PLUS on every axis, MAX on rows, and the scale with a left
vector, with a right vector, and with both in place.  Achieved bytes per second are over the compulsory bytes -- reductions:
4 B per row of row pointer, 8 B per entry of value, 4 B per entry of column index where the call reads it, 8 B per output;
the scale: 4 B per row, 16 B per entry, 4 B + 8 B of gather per entry with a right vector, 8 B per row with a left one --
and are set beside the copy's rate of the same run."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from benchmark_spgemm_using_csr_amd import _lib, facade, gallery  # noqa: E402
from tools.extract_case import REPS, copy_ms, stat, timed  # noqa: E402
from tools.semiring_case import lower_triangle  # noqa: E402


def make(case):
    if case == "p27_128":
        return gallery.poisson_csr("poisson27pt", 128, 128, 128)
    if case == "uniform":
        return gallery.uniform_csr(1 << 20, 8)
    if case == "tri_rmat20":
        return lower_triangle(*gallery.rmat_csr(scale=20))
    raise ValueError(case)


def run(case, bh, dev):
    rp, col = make(case)
    m = n = len(rp) - 1
    nnz = len(col)
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)   # noqa: E731
    Xp, Xj, Xx = up(rp.astype(np.int32)), up(col.astype(np.int32)), up(gallery.fill_values(nnz))
    rng = np.random.default_rng(1)
    left, right = up(1.0 + rng.random(m)), up(1.0 + rng.random(n))
    Zp = torch.empty(m + 1, dtype=torch.int32, device=dev)
    Zj = torch.empty(nnz, dtype=torch.int32, device=dev)
    Zx = torch.empty(nnz, dtype=torch.float64, device=dev)
    out_v = torch.empty(max(m, n), dtype=torch.float64, device=dev)
    torch.cuda.synchronize()
    assert bh.set_option("kernel_stats", 0) == 0
    lens = np.diff(rp.astype(np.int64))
    out = {"case": case, "m": m, "nnz": nnz, "longest_row": int(lens.max()), "longest_column": int(np.bincount(col, minlength=n).max())}
    cp = copy_ms([(Zp, Xp), (Zj, Xj), (Zx, Xx)])
    copy_bytes = 2 * (4 * (m + 1) + 12 * nnz)
    copy_rate = copy_bytes / (np.median(cp) * 1e6)
    out["device_copy"] = dict(stat(cp), bytes=copy_bytes, achieved_GBps=copy_rate)

    def families(prefix):
        return {s["name"]: {"launches": s["launches"], "ms": round(s["ms"], 4)} for s in bh.kernel_stats()
                if s["name"].startswith(prefix) and s["launches"]}

    A = _lib
    for name, axis, op, cols in (("rows_plus", A.BHS_AXIS_ROWS, A.BHS_RED_PLUS, False), ("rows_max", A.BHS_AXIS_ROWS, A.BHS_RED_MAX, False),
                                 ("cols_plus", A.BHS_AXIS_COLS, A.BHS_RED_PLUS, True), ("all_plus", A.BHS_AXIS_ALL, A.BHS_RED_PLUS, False),
                                 ("diag_plus", A.BHS_AXIS_DIAG, A.BHS_RED_PLUS, True)):
        def red():
            assert bh.csr_reduce_raw_device(m, n, nnz, Xx, Xp, Xj, axis, op, 0, out_v) == 0
        _, d = timed(red, lambda: bh.reduce_ms)
        assert bh.set_option("kernel_stats", 1) == 0
        red()
        fam = families("reduce_")
        assert bh.set_option("kernel_stats", 0) == 0
        n_out = {A.BHS_AXIS_ROWS: m, A.BHS_AXIS_COLS: n, A.BHS_AXIS_ALL: 1, A.BHS_AXIS_DIAG: m}[axis]
        # (the diagonal reads a value only where the column matches: one per row here)
        compulsory = 4 * (m + 1) + (4 * nnz + 8 * m if axis == A.BHS_AXIS_DIAG else 8 * nnz + (4 * nnz if cols else 0)) + 8 * n_out
        med = float(np.median(d))
        out[name] = dict(stat(d), kernels=fam, compulsory_bytes=compulsory, achieved_GBps=compulsory / (med * 1e6),
                         share_of_copy_rate=compulsory / (med * 1e6) / copy_rate)

    work = Xx.clone()
    for name, l, r, dst in (("scale_left", left, None, Zx), ("scale_right", None, right, Zx), ("scale_both_inplace", left, right, work)):
        src = work if dst is work else Xx

        def sc():
            assert bh.csr_scale_raw_device(m, n, nnz, src, Xp, Xj, 1.0, l, r, 0, dst) == 0
        _, d = timed(sc, lambda: bh.scale_ms)
        assert bh.set_option("kernel_stats", 1) == 0
        sc()
        fam = families("scale")
        assert bh.set_option("kernel_stats", 0) == 0
        compulsory = 4 * (m + 1) + 16 * nnz + (12 * nnz if r is not None else 0) + (8 * m if l is not None else 0)
        med = float(np.median(d))
        out[name] = dict(stat(d), kernels=fam, compulsory_bytes=compulsory, achieved_GBps=compulsory / (med * 1e6),
                         share_of_copy_rate=compulsory / (med * 1e6) / copy_rate)

    spec = facade.select_spec(abs_tol=0.5)                          # keeps every entry
    got = {}

    def ssym():
        err, got["nnzZ"] = bh.csr_select_symbolic_device(m, n, nnz, Xx, Xp, Xj, spec, Zp)
        assert err == 0

    def snum():
        assert bh.csr_select_numeric_device(m, n, nnz, Xx, Xp, Xj, spec, Zp, Zj, Zx) == 0
    timed(ssym)
    _, d = timed(snum, lambda: bh.select_ms)
    assert got["nnzZ"] == nnz
    compulsory = 24 * nnz + 8 * (m + 1)
    out["select_keep_all"] = dict(stat(d), compulsory_bytes=compulsory, achieved_GBps=compulsory / (float(np.median(d)) * 1e6))
    return out


if __name__ == "__main__":
    cases = sys.argv[1:] or ["p27_128", "uniform", "tri_rmat20"]
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
    print(json.dumps({"tool": "reduce_case", "reps": REPS, "results": res}))
