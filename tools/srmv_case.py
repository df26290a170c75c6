"""Semiring CSR x dense (bhs_csr_spmv_semiring_device, bhs_csr_spmm_semiring_device) on device-resident inputs against the
plus-times product of the same library (bhs_csr_spmv_device / bhs_csr_spmm_device: code this feature does not touch) in the
same process and on the same arrays; prints one JSON line.

    python tools/srmv_case.py [case ...]      cases: p27_128 uniform tri_rmat20 (default: all three)

Both builds (double, float).  Per case, after 3 warm-ups, medians and minima of REPS (default 12) runs with per-kernel timers
off, device time from the event pair around the whole call (validation, the queue lengths' round trip and the count's
included):
  - the yardstick: y = A x and Y = A X, k = 1, 4, 16 (alpha = 1, beta = 0);
  - MIN_PLUS, OR_AND, PLUS_PAIR and PLUS_TIMES without a mask at k = 1, 4, 16; MIN_PLUS with ACCUM;
  - PLUS_TIMES and MIN_PLUS once more through the C-ABI with a NULL changed_out ("_no_count"): the kernels then skip the
    count of changed elements, so the difference is what the count costs;
  - OR_AND at k = 1 under a complement mask that selects 100 %, 50 %, 10 % and 1 % of the rows, the selected rows random or
    one contiguous block;
  - on uniform and tri_rmat20: one whole BFS (graph.bfs_levels_device) and one whole Bellman-Ford (graph.sssp_device, weights
    1 .. 2) from 1 and from 16 sources: steps, total device time of the calls, wall time of the loop.
"ratio_to_plus_times" sets a median beside the yardstick's of the same k in the same run."""
import ctypes as C
import functools
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from benchmark_spgemm_using_csr_amd import _lib, dense, facade, graph  # noqa: E402
from tools.extract_case import REPS, stat, timed  # noqa: E402
from tools.reduce_case import make  # noqa: E402

KS = (1, 4, 16)
SHARES = (1.0, 0.5, 0.1, 0.01)
CMP, ACC = _lib.BHS_MV_MASK_COMPLEMENT, _lib.BHS_MV_ACCUM
make = functools.lru_cache(maxsize=None)(make)


def run(case, bh, dev, dtype):
    rp, col = make(case)
    m = n = len(rp) - 1
    nnz = len(col)
    V = np.dtype(dtype).itemsize
    tdt = torch.float32 if V == 4 else torch.float64
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)   # noqa: E731
    rng = np.random.default_rng(1)
    Ap, Aj, Ax = up(rp.astype(np.int32)), up(col.astype(np.int32)), up((1.0 + rng.random(nnz)).astype(dtype))
    kmax = max(KS)
    X = up((1.0 + rng.random(n * kmax)).astype(dtype))
    Y = torch.empty(m * kmax, dtype=tdt, device=dev)
    torch.cuda.synchronize()
    assert bh.set_option("kernel_stats", 0) == 0
    lens = np.diff(rp.astype(np.int64))
    out = {"case": case, "value_bytes": V, "m": m, "nnz": nnz, "longest_row": int(lens.max()),
           "rows_beyond_32": int(np.count_nonzero(lens > 32)), "rows_beyond_1024": int(np.count_nonzero(lens > 1024))}
    base = {}

    def measure(name, call, k, extra=None):
        _, d = timed(call, lambda: bh.spmv_ms)
        med = float(np.median(d))
        out[name] = dict(stat(d), **(extra or {}))
        if k in base:
            out[name]["ratio_to_plus_times"] = med / base[k]
        return med

    for k in KS:
        def product(k=k):
            if k == 1:
                assert dense.csr_spmv_raw_device(bh, m, n, nnz, Ax, Ap, Aj, 1.0, X, 0.0, Y) == 0
            else:
                assert dense.csr_spmm_raw_device(bh, m, n, nnz, Ax, Ap, Aj, k, 1.0, X, k, 0.0, Y, k) == 0
        base[k] = measure("yardstick_plus_times_k%d" % k, product, None)

    def semiring(name, k, flags=0, mask=None):
        def call():
            if k == 1:
                assert dense.csr_spmv_semiring_raw_device(bh, name, m, n, nnz, Ax, Ap, Aj, X, flags, mask, Y) == 0
            else:
                assert dense.csr_spmm_semiring_raw_device(bh, name, m, n, nnz, Ax, Ap, Aj, k, X, k, flags, mask, k, Y, k) == 0
        return call

    for name in ("min_plus", "or_and", "plus_pair", "plus_times"):
        for k in KS:
            measure("%s_k%d" % (name, k), semiring(name, k), k, {"changed": None})
            out["%s_k%d" % (name, k)]["changed"] = bh.spmv_changed
    def no_count(name, k):
        code, ms = _lib.SEMIRINGS[name], C.c_double(0)

        def call():
            assert bh._lib.bhs_csr_spmm_semiring_device(bh._h, code, m, n, nnz, Ax.data_ptr(), Ap.data_ptr(), Aj.data_ptr(), k,
                                                        X.data_ptr(), k, 0, None, k, Y.data_ptr(), k, None, C.byref(ms)) == 0
            bh.spmv_ms = ms.value
        return call

    for name in ("plus_times", "min_plus"):
        for k in KS:
            measure("%s_k%d_no_count" % (name, k), no_count(name, k), k)
    for k in KS:
        Y.fill_(float("inf"))
        torch.cuda.synchronize()
        measure("min_plus_accum_k%d" % k, semiring("min_plus", k, ACC), k)
    # OR_AND under the complement of a mask: the rows that are NOT set are selected
    for layout in ("random", "block"):
        for share in SHARES:
            keep = int(round(m * share))
            set_rows = np.ones(m, dtype)
            if layout == "block":
                start = (m - keep) // 2
                set_rows[start:start + keep] = 0
            else:
                set_rows[np.random.default_rng(2).choice(m, keep, replace=False)] = 0
            M = up(set_rows)
            torch.cuda.synchronize()
            measure("or_and_k1_%s_%g" % (layout, share), semiring("or_and", 1, CMP, M), 1, {"rows_selected": keep})
            out["or_and_k1_%s_%g" % (layout, share)]["changed"] = bh.spmv_changed
    # a spot check of what was timed: row 0 and the last row of the k = 16 MIN_PLUS product against numpy
    assert dense.csr_spmm_semiring_raw_device(bh, "min_plus", m, n, nnz, Ax, Ap, Aj, kmax, X, kmax, 0, None, kmax, Y, kmax) == 0
    Yh = Y.view(m, kmax).cpu().numpy()
    Xh, Axh = X.view(n, kmax).cpu().numpy().astype(np.float64), Ax.cpu().numpy().astype(np.float64)
    for i in (0, m - 1):
        if rp[i + 1] > rp[i]:
            ref = (Axh[rp[i]:rp[i + 1], None] + Xh[col[rp[i]:rp[i + 1]]]).min(axis=0)
            assert np.array_equal(Yh[i], ref.astype(dtype)), (case, i)
    # whole traversals (kernel timers stay off)
    if case != "p27_128":
        src16 = [int(s) for s in np.random.default_rng(3).choice(np.flatnonzero(lens > 0), 16, replace=False)]
        for k, sources in ((1, src16[:1]), (16, src16)):
            t0 = time.perf_counter()
            levels, steps, ms = graph._bfs(bh, n, (Ap, Aj, Ax), sources)
            torch.cuda.synchronize()
            out["bfs_k%d" % k] = {"steps": steps, "device_ms": ms, "wall_ms": (time.perf_counter() - t0) * 1e3,
                                  "reached": int((levels != 0).sum())}
            t0 = time.perf_counter()
            try:
                D, sweeps, ms = graph._sssp(bh, n, (Ap, Aj, Ax), sources, 400)
                torch.cuda.synchronize()
                out["sssp_k%d" % k] = {"steps": sweeps, "device_ms": ms, "wall_ms": (time.perf_counter() - t0) * 1e3,
                                       "reached": int(torch.isfinite(D).sum())}
            except facade.BhsparseError:
                out["sssp_k%d" % k] = {"steps": 400, "converged": False}
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
    print(json.dumps({"tool": "srmv_case", "reps": REPS, "device": torch.cuda.get_device_name(0), "source_digest": _lib.source_digest(),
                      "results": res}))
