"""Sparse frontier x CSR (bhs_csr_push_semiring_device) and the frontier traversals (graph.bfs_levels_frontier_device,
graph.sssp_frontier_device) against the pull call and the pull-only traversals of the same library in the same process and
on the same arrays; prints one JSON line.

    python tools/push_case.py [case ...]      cases: roadlike uniform tri_rmat20 (default: all three)

Double build.  Device time from the event pair around the whole call (validation, scans, compaction and the round trip
included), per-kernel timers off except where the kernels' records are wanted.
  (a) the single-call crossover: one OR_AND push call (k = 1, count and list both taken) from a random frontier of 1 vertex,
      0.1 %, 1 %, 10 % and 50 % of the rows, beside the OR_AND pull call of the same frontier under the same complement
      mask.  Two masks: "early" -- only the frontier itself is visited, so the pull call walks every other row --, and
      "late" -- 90 % of the rows are visited.  After 3 warm-ups, medians and minima of REPS (default 12) runs; the push call's
      Y is zeroed between runs (outside the timed span), so every run does the same updates.  "crossover": the largest
      frontier share at which the push call's median is below the pull call's.  The kernels' records of one push call per
      size are listed too.
  (b) whole traversals from 1 and from 16 sources: graph._bfs / graph._sssp (pull only) against graph._bfs_frontier /
      graph._sssp_frontier with the default push_below and with always-push: steps, steps that went by push, total device time
      of the calls, wall time of the loop.  The pull-only loop runs twice: the difference is the run-to-run spread that the
      comparison on the uniform graph is read against.  Results are compared (equal) before anything is reported."""
import functools
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from benchmark_spgemm_using_csr_amd import _lib, dense, facade, gallery, graph  # noqa: E402
from tools.extract_case import REPS, stat, timed  # noqa: E402
from tools.reduce_case import make as make_other  # noqa: E402

SHARES = (0.0, 0.001, 0.01, 0.1, 0.5)                                # 0: a single vertex
CMP = _lib.BHS_MV_MASK_COMPLEMENT
MAX_ROUNDS = 40000


@functools.lru_cache(maxsize=None)
def make(case):
    return gallery.roadlike_csr() if case == "roadlike" else make_other(case)


def run(case, bh, dev, dtype=np.float64):
    rp, col = make(case)
    n = len(rp) - 1
    nnz = len(col)
    tdt = torch.float64
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)   # noqa: E731
    rng = np.random.default_rng(1)
    A = (up(rp.astype(np.int32)), up(col.astype(np.int32)), up((1.0 + rng.random(nnz)).astype(dtype)))
    assert bh.set_option("kernel_stats", 0) == 0
    Tp, Tj, Tx, _ = bh.csr_transpose_device(n, n, A)
    G = (Tp, Tj, Tx)
    lens = np.diff(rp.astype(np.int64))
    out = {"case": case, "n": n, "nnz": nnz, "longest_row": int(lens.max()), "transpose_ms": bh.transpose_ms}

    # ---- (a) one call, push beside pull
    single = {}
    for mask_kind in ("early", "late"):
        for share in SHARES:
            nf = max(1, int(round(n * share)))
            pick = np.sort(np.random.default_rng(2).choice(n, nf, replace=False))
            visited = np.zeros(n, dtype)
            if mask_kind == "late":
                visited[np.random.default_rng(3).choice(n, int(n * 0.9), replace=False)] = 1.0
            visited[pick] = 1.0
            M = up(visited)
            fidx = up(pick.astype(np.int32))
            F = torch.ones(nf, dtype=tdt, device=dev)
            X = torch.zeros(n, dtype=tdt, device=dev)
            X[fidx.long()] = 1.0
            Ypush = torch.zeros(n, dtype=tdt, device=dev)
            Ypull = torch.zeros(n, dtype=tdt, device=dev)
            nxt = torch.empty(n, dtype=torch.int32, device=dev)
            torch.cuda.synchronize()

            def push():
                Ypush.zero_()
                torch.cuda.synchronize()
                assert dense.csr_push_semiring_raw_device(bh, "or_and", n, n, nnz, G[2], G[0], G[1], nf, fidx, 1, F, 1, CMP, M, 1, Ypush, 1,
                                                          nxt) == 0

            def pull():
                assert dense.csr_spmv_semiring_raw_device(bh, "or_and", n, n, nnz, A[2], A[0], A[1], X, CMP, M, Ypull) == 0

            _, d_push = timed(push, lambda: bh.spmv_ms)
            changed_push, listed = bh.spmv_changed, bh.push_next
            _, d_pull = timed(pull, lambda: bh.spmv_ms)
            assert changed_push == bh.spmv_changed == listed and torch.equal(Ypush, Ypull), (case, mask_kind, share)
            assert bh.set_option("kernel_stats", 1) == 0
            push()
            kernels = {s["name"]: round(s["ms"], 5) for s in bh.kernel_stats() if s["launches"] > 0}
            assert bh.set_option("kernel_stats", 0) == 0
            key = "%s_%s" % (mask_kind, "1_vertex" if share == 0 else "%g" % share)
            single[key] = {"frontier": nf, "changed": changed_push, "push": stat(d_push), "pull": stat(d_pull),
                           "push_over_pull": float(np.median(d_push) / np.median(d_pull)), "push_kernels_ms": kernels}
        wins = [s for s in SHARES if single["%s_%s" % (mask_kind, "1_vertex" if s == 0 else "%g" % s)]["push_over_pull"] < 1.0]
        out["crossover_%s" % mask_kind] = max(wins) if wins else None
    out["single_call"] = single

    # ---- (b) whole traversals (kernel timers stay off)
    src16 = [int(s) for s in np.random.default_rng(3).choice(np.flatnonzero(lens > 0), 16, replace=False)]
    trav = {}
    for k, sources in ((1, src16[:1]), (16, src16)):
        def whole(loop):
            t0 = time.perf_counter()
            res = loop()
            torch.cuda.synchronize()
            return res, (time.perf_counter() - t0) * 1e3

        (lv, steps, ms), wall = whole(lambda: graph._bfs(bh, n, A, sources))
        (lv2, steps2, ms2), wall2 = whole(lambda: graph._bfs(bh, n, A, sources))
        rec = {"pull_only": {"steps": steps, "device_ms": ms, "wall_ms": wall}, "pull_only_again": {"device_ms": ms2, "wall_ms": wall2},
               "reached": int((lv != 0).sum())}
        for name, pb in (("frontier_default", None), ("frontier_always_push", float("inf"))):
            (got, fsteps, fms, pushes), fwall = whole(lambda: graph._bfs_frontier(bh, n, A, sources, G, pb))
            assert torch.equal(got, lv), (case, "bfs", name)
            rec[name] = {"steps": fsteps, "push_steps": pushes, "device_ms": fms, "wall_ms": fwall, "pull_only_over_this": ms / fms}
        trav["bfs_k%d" % k] = rec
        try:
            (D, rounds, ms), wall = whole(lambda: graph._sssp(bh, n, A, sources, MAX_ROUNDS))
            (D2, rounds2, ms2), wall2 = whole(lambda: graph._sssp(bh, n, A, sources, MAX_ROUNDS))
        except facade.BhsparseError:
            trav["sssp_k%d" % k] = {"converged": False, "max_rounds": MAX_ROUNDS}
            continue
        rec = {"pull_only": {"steps": rounds, "device_ms": ms, "wall_ms": wall}, "pull_only_again": {"device_ms": ms2, "wall_ms": wall2},
               "reached": int(torch.isfinite(D).sum())}
        for name, pb in (("frontier_default", None), ("frontier_always_push", float("inf"))):
            (got, frounds, fms, pushes), fwall = whole(lambda: graph._sssp_frontier(bh, n, A, sources, G, MAX_ROUNDS, pb))
            assert torch.equal(got, D), (case, "sssp", name)
            rec[name] = {"steps": frounds, "push_steps": pushes, "device_ms": fms, "wall_ms": fwall, "pull_only_over_this": ms / fms}
        trav["sssp_k%d" % k] = rec
    out["traversals"] = trav
    return out


if __name__ == "__main__":
    cases = sys.argv[1:] or ["roadlike", "uniform", "tri_rmat20"]
    dev = torch.device("cuda", 0)
    plats = [False] * facade.NUM_PLATFORMS
    plats[facade.BHSPARSE_HIP] = True
    res = []
    bh = facade.bhsparse(value_dtype=np.float64)
    assert bh.initPlatform(plats) == 0
    for c in cases:
        res.append(run(c, bh, dev))
        print(json.dumps(res[-1]), file=sys.stderr, flush=True)
        torch.cuda.empty_cache()
    bh.freePlatform()
    print(json.dumps({"tool": "push_case", "reps": REPS, "push_below_default": graph.PUSH_BELOW, "device": torch.cuda.get_device_name(0),
                      "source_digest": _lib.source_digest(), "results": res}))
