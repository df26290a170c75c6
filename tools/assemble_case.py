"""The assembly from triplets (bhs_coo_assemble_device with values and the map; bhs_coo_assemble_values_device) on
device-resident triplets against three yardsticks on the same arrays in the same run: a device copy of the triplets (the
byte floor), bhs_csr_transpose_device of the result (the library's other count / scan / scatter / sort pipeline), and the
torch route callers use today (argsort of the 64-bit key, unique_consecutive, index_add_); prints one JSON line.

    python tools/assemble_case.py [case ...] [f64|f32]     cases: p27_128 q1_1024 uniform rmat one_run (default: all, both types)

p27_128   the triplets of poisson27pt 128^3, shuffled: no duplicates
q1_1024   the 16 contributions an element of a 1024^2 mesh of quadrilaterals, element after element: about 9 runs an entry
uniform   the entries of gallery.uniform_csr (2^20 rows), shuffled
rmat      the R-MAT scale-20 edge draws of gallery.rmat_csr BEFORE np.unique: hubs and duplicates
one_run   2^20 copies of one triplet: the degenerate case -- one raw row for one workgroup's sort, one run for one lane's sum

Per case and type, in one process: after 3 warm-ups, medians and minima of REPS (default 12) runs with per-kernel timers off
-- device time of the full call and of the values-only call, torch events around the others.  One extra full call with
kernel_stats=1 gives the kernel families."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from benchmark_spgemm_using_csr_amd import _lib, assemble, facade, gallery  # noqa: E402

REPS = int(os.environ.get("REPS", "12"))
WARM = 3
CASES = ("p27_128", "q1_1024", "uniform", "rmat", "one_run")


def shuffled(rp, col, seed):
    rows = np.repeat(np.arange(len(rp) - 1, dtype=np.int32), np.diff(np.asarray(rp, np.int64)))
    o = np.random.default_rng(seed).permutation(len(rows))
    return len(rp) - 1, rows[o], np.asarray(col, np.int32)[o]


def make(case):
    """(n, rows, cols): triplets of an n x n matrix"""
    if case == "p27_128":
        return shuffled(*gallery.poisson_csr("poisson27pt", 128, 128, 128), seed=1)
    if case == "uniform":
        return shuffled(*gallery.uniform_csr(), seed=2)
    if case == "q1_1024":
        e = 1024
        x, y = np.meshgrid(np.arange(e), np.arange(e))
        c0 = (y * (e + 1) + x).ravel()
        corners = np.stack((c0, c0 + 1, c0 + e + 1, c0 + e + 2), axis=1)                 # (elements, 4)
        rows = np.repeat(corners, 4, axis=1).ravel()
        cols = np.tile(corners, (1, 4)).ravel()
        return (e + 1) ** 2, rows.astype(np.int32), cols.astype(np.int32)
    if case == "rmat":
        scale, a, b, c = 20, 0.57, 0.19, 0.19                                            # gallery.rmat_csr's draws
        rng = np.random.default_rng(gallery.SEED)
        ne = 2 << scale
        rows, cols = np.zeros(ne, np.int64), np.zeros(ne, np.int64)
        for _ in range(scale):
            u = rng.random(ne)
            rows = (rows << 1) | (u >= a + b)
            cols = (cols << 1) | (((u >= a) & (u < a + b)) | (u >= a + b + c))
        return 1 << scale, rows.astype(np.int32), cols.astype(np.int32)
    if case == "one_run":
        return 16, np.full(1 << 20, 3, np.int32), np.full(1 << 20, 7, np.int32)
    raise ValueError(case)


def stat(xs):
    return {"median_ms": round(float(np.median(xs)), 4), "min_ms": round(float(np.min(xs)), 4)}


def timed(fn, after=None):
    ms = []
    for i in range(WARM + REPS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        if i >= WARM:
            ms.append(after() if after else a.elapsed_time(b))
    return ms


def torch_route(n, rows, cols, vals):
    """what callers do today: (rowPtr, colInd, val) with duplicates added (index_add_: atomics, no fixed order)"""
    key = (rows.to(torch.int64) << 32) | cols.to(torch.int64)
    order = torch.argsort(key)
    uniq, inv = torch.unique_consecutive(key[order], return_inverse=True)
    val = torch.zeros(uniq.numel(), dtype=vals.dtype, device=vals.device).index_add_(0, inv, vals[order])
    rowptr = torch.zeros(n + 1, dtype=torch.int32, device=rows.device)
    rowptr[1:] = torch.cumsum(torch.bincount(uniq >> 32, minlength=n), 0).to(torch.int32)
    return rowptr, (uniq & 0xFFFFFFFF).to(torch.int32), val


def run(case, bh, dtype, dev):
    n, rows, cols = make(case)
    nnz = len(rows)
    vals = np.random.default_rng(5).integers(-4, 5, nnz).astype(dtype)
    d_rows, d_cols, d_vals = (torch.from_numpy(a).to(dev) for a in (rows, cols, vals))
    tdt = d_vals.dtype
    Zp = torch.empty(n + 1, dtype=torch.int32, device=dev)
    Zj, pm = (torch.empty(nnz, dtype=torch.int32, device=dev) for _ in range(2))
    ent = torch.empty(nnz + 1, dtype=torch.int32, device=dev)
    Zx = torch.empty(nnz, dtype=tdt, device=dev)
    copies = [torch.empty_like(t) for t in (d_rows, d_cols, d_vals)]
    assert bh.set_option("kernel_stats", 0) == 0
    out = {"case": case, "type": np.dtype(dtype).name, "n": n, "triplets": nnz}

    def full():
        assert assemble.coo_assemble_raw_device(bh, n, n, nnz, d_rows, d_cols, d_vals, _lib.BHS_COO_SUM, Zp, Zj, Zx, ent, pm) == 0
    full_ms = timed(full, lambda: bh.assemble_ms)
    nz = bh.assemble_nnz
    out["entries"], out["triplets_per_entry"] = nz, round(nnz / max(nz, 1), 3)
    out["longest_raw_row"] = int(np.bincount(rows, minlength=n).max())

    def values():
        assert assemble.coo_values_raw_device(bh, nnz, d_vals, nz, ent, pm, _lib.BHS_COO_SUM, Zx) == 0
    val_ms = timed(values, lambda: bh.assemble_ms)
    want = Zx[:nz].clone()
    full()
    assert torch.equal(want.view(torch.int64 if tdt == torch.float64 else torch.int32),
                       Zx[:nz].view(torch.int64 if tdt == torch.float64 else torch.int32))           # the same bits

    def copy():
        for dst, src in zip(copies, (d_rows, d_cols, d_vals)):
            dst.copy_(src)
    copy_ms = timed(copy)
    Tp = torch.empty(n + 1, dtype=torch.int32, device=dev)
    Tj, tpm = (torch.empty(max(nz, 1), dtype=torch.int32, device=dev) for _ in range(2))
    Tx = torch.empty(max(nz, 1), dtype=tdt, device=dev)

    def transpose():
        assert bh.csr_transpose_raw_device(n, n, nz, Zx, Zp, Zj, Tp, Tj, Tx, tpm) == 0
    tr_ms = timed(transpose, lambda: bh.transpose_ms)
    torch_ms = timed(lambda: torch_route(n, d_rows, d_cols, d_vals))
    tp, tj, tx = torch_route(n, d_rows, d_cols, d_vals)
    assert torch.equal(tp, Zp) and torch.equal(tj, Zj[:nz]) and torch.equal(tx, Zx[:nz])            # (small integers: any order adds exactly)
    assert bh.set_option("kernel_stats", 1) == 0
    full()
    fam = {s["name"]: {"launches": s["launches"], "ms": round(s["ms"], 4), "rows": s["rows"]} for s in bh.kernel_stats()
           if s["name"].startswith("assemble_") and s["launches"]}
    assert bh.set_option("kernel_stats", 0) == 0
    f, v, c, t, p = (float(np.median(x)) for x in (full_ms, val_ms, copy_ms, tr_ms, torch_ms))
    out.update(full=dict(stat(full_ms), kernels=fam), values_only=stat(val_ms), copy_of_triplets=stat(copy_ms),
               transpose_of_result=stat(tr_ms), torch_route=stat(torch_ms),
               full_over_copy=round(f / c, 2), full_over_transpose=round(f / t, 2), full_over_torch=round(f / p, 3),
               values_over_full=round(v / f, 3), values_over_torch=round(v / p, 3))
    return out


if __name__ == "__main__":
    args = sys.argv[1:]
    types = [a for a in args if a in ("f64", "f32")] or ["f64", "f32"]
    cases = [a for a in args if a not in ("f64", "f32")] or list(CASES)
    dev = torch.device("cuda", 0)
    plats = [False] * facade.NUM_PLATFORMS
    plats[facade.BHSPARSE_HIP] = True
    res = []
    for t in types:
        dtype = np.float64 if t == "f64" else np.float32
        bh = facade.bhsparse(value_dtype=dtype)
        assert bh.initPlatform(plats) == 0
        for c in cases:
            res.append(run(c, bh, dtype, dev))
            print(json.dumps(res[-1]), file=sys.stderr, flush=True)
            torch.cuda.empty_cache()
        bh.freePlatform()
    print(json.dumps({"tool": "assemble_case", "reps": REPS, "results": res}))
