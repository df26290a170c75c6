"""The k-core decomposition (bhs_csr_kcore_device) case by case: what the call costs per kernel record, beside the connected
components on the same pattern, a torch route on the same device, networkx on the CPU where it finishes, and the k-truss on
top; measured in one process on the same arrays; prints one JSON line per case.

    python tools/kcore_case.py [--no-torch] [--no-nx] [--no-truss] [case ...]
        cases: poisson27pt_128 poisson5pt_1024 uniform20 roadlike rmat20 (default: all five)

Double build.  Per case:
  (a) the pattern: the matrix's own where it is symmetric, pattern U pattern^T through ordering.symmetric_pattern_device
      for the uniform and the R-MAT graph;
  (b) the call: kmax, rounds, device ms of the call from its event pair (every round trip included) after a warm-up, median
      and minimum of REPS runs with the per-launch timers off, and the three kernel records' ms and launches of one further
      run with the timers on;
  (c) bhs_csr_components_device on the same pattern, timed the same way, for scale;
  (d) unless --no-torch: the torch route on the same device -- a round computes the level on the host from the smallest
      present degree, removes everything at or below it and lowers the degrees with one index_add_ over the removed
      vertices' entries --, wall ms of one run after a warm-up of its first 10 rounds, and that it gives the same core
      numbers and rounds; left out where the call took more than TORCH_ABOVE rounds;
  (e) unless --no-nx: networkx's core_number on the CPU where the pattern has at most NX_BELOW entries, wall ms with the
      graph's construction apart, and that it gives the same core numbers;
  (f) unless --no-truss, on the uniform and the R-MAT graph: graph.ktruss_device for k = 3, 4 -- nnz, iterations, wall ms --
      beside ONE masked PLUS_PAIR product on the pattern (device ms)."""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from benchmark_spgemm_using_csr_amd import _lib, facade, gallery, graph, ordering  # noqa: E402

REPS = int(os.environ.get("REPS", "5"))
TORCH_ABOVE = int(os.environ.get("TORCH_ABOVE", "4096"))
NX_BELOW = int(os.environ.get("NX_BELOW", "12000000"))
CASES = ("poisson27pt_128", "poisson5pt_1024", "uniform20", "roadlike", "rmat20")
TRUSS_ON = ("uniform20", "rmat20")


def make(case):
    """(rowPtr, colInd, symmetric already)"""
    if case == "poisson27pt_128":
        return gallery.poisson_csr("poisson27pt", 128, 128, 128) + (True,)
    if case == "poisson5pt_1024":
        return gallery.poisson_csr("poisson5pt", 1024, 1024) + (True,)
    if case == "uniform20":
        return tuple(gallery.uniform_csr(1 << 20, 8)[:2]) + (False,)
    if case == "roadlike":
        return tuple(gallery.roadlike_csr()[:2]) + (True,)
    if case == "rmat20":
        return tuple(gallery.rmat_csr(scale=20)[:2]) + (False,)
    raise SystemExit("unknown case %s" % case)


def stat(xs):
    return {"median": float(np.median(xs)), "min": float(np.min(xs))}


def records(bh):
    return {k["name"]: {"ms": round(k["ms"], 4), "launches": k["launches"]} for k in bh.kernel_stats() if k["launches"] > 0}


def timed_call(bh, call, ms_of):
    """median and minimum of REPS runs behind a warm-up, the per-launch timers off; then the records of one run with them on"""
    ms = []
    assert bh.set_option("kernel_stats", 0) == 0
    for rep in range(REPS + 1):
        assert call() == 0
        if rep >= 1:
            ms.append(ms_of())
    assert bh.set_option("kernel_stats", 1) == 0
    assert call() == 0
    return stat(ms), records(bh)


def torch_route(n, S, max_rounds=None):
    """(core, round, kmax, rounds) by the definition with torch tensor operations: one index_add_ a round"""
    Sp, Sj = S[0].long(), S[1].long()
    lens = Sp[1:] - Sp[:-1]
    rows = torch.repeat_interleave(torch.arange(n, device=Sp.device), lens, output_size=Sj.numel())
    off = rows != Sj
    rows, cols = rows[off], Sj[off]
    deg = torch.bincount(rows, minlength=n)
    present = torch.ones(n, dtype=torch.bool, device=Sp.device)
    core = torch.zeros(n, dtype=torch.int32, device=Sp.device)
    rnd = torch.zeros(n, dtype=torch.int32, device=Sp.device)
    big = torch.iinfo(torch.int64).max
    k, r = 0, 0
    while bool(present.any()) and (max_rounds is None or r < max_rounds):
        r += 1
        k = max(k, int(torch.where(present, deg, big).min()))
        leave = present & (deg <= k)
        core[leave], rnd[leave] = k, r
        present &= ~leave
        gone = leave[rows]                                            # the entries of the vertices that left
        deg.index_add_(0, cols[gone], torch.full((int(gone.sum()),), -1, dtype=deg.dtype, device=deg.device))
    return core, rnd, k, r


def run(case, bh, dev, opts):
    rp, col, symmetric = make(case)
    n = len(rp) - 1
    up = lambda x, dt: torch.from_numpy(np.ascontiguousarray(x, dt)).to(dev)   # noqa: E731
    S = (up(rp, np.int32), up(col, np.int32))
    if not symmetric:
        S = ordering.symmetric_pattern_device(bh, n, S + (torch.ones(len(col), dtype=torch.float64, device=dev),))
    nnz = S[1].numel()
    out = {"case": case, "n": n, "nnz": nnz, "mean_row": nnz / n, "longest_row": int((S[0][1:] - S[0][:-1]).max()),
           "library": os.path.basename(_lib.SO_PATH), "source_digest": _lib.source_digest()}
    core, rnd, root = (torch.empty(n, dtype=torch.int32, device=dev) for _ in range(3))
    torch.cuda.synchronize()
    ms, recs = timed_call(bh, lambda: graph.kcore_raw_device(bh, n, nnz, S[0], S[1], 0, core, rnd), lambda: bh.kcore_ms)
    kmax, rounds = bh.kcore_kmax, bh.kcore_rounds
    out["kcore"] = {"kmax": kmax, "rounds": rounds, "levels": int(torch.unique(core).numel()), "ms": ms, "kernels": recs}
    ms, recs = timed_call(bh, lambda: graph.components_raw_device(bh, n, nnz, S[0], S[1], 0, root, None, None),
                          lambda: bh.components_ms)
    out["components"] = {"ncomp": bh.components_ncomp, "passes": bh.components_passes, "ms": ms}
    if opts["torch"] and rounds <= TORCH_ABOVE:
        torch_route(n, S, 10)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        tcore, trnd, tk, tr = torch_route(n, S)
        torch.cuda.synchronize()
        out["torch"] = {"ms": (time.perf_counter() - t0) * 1e3,
                        "same": bool((tcore == core).all()) and bool((trnd == rnd).all()) and (tk, tr) == (kmax, rounds)}
    elif opts["torch"]:
        out["torch"] = {"skipped": "more than %d rounds" % TORCH_ABOVE}
    if opts["nx"] and nnz <= NX_BELOW:
        import networkx as nx
        Sp, Sj = S[0].cpu().numpy(), S[1].cpu().numpy()
        r = np.repeat(np.arange(n), np.diff(Sp))
        G = nx.Graph()
        G.add_nodes_from(range(n))
        G.add_edges_from(zip(r[r < Sj].tolist(), Sj[r < Sj].tolist()))
        t0 = time.perf_counter()
        cn = nx.core_number(G)
        t1 = time.perf_counter()
        out["networkx"] = {"ms": (t1 - t0) * 1e3, "same": bool(np.array_equal(np.fromiter((cn[v] for v in range(n)), np.int32, n),
                                                                              core.cpu().numpy()))}
    elif opts["nx"]:
        out["networkx"] = {"skipped": "more than %d entries" % NX_BELOW}
    if opts["truss"] and case in TRUSS_ON:
        A = (S[0], S[1], None)
        ones = torch.ones(nnz, dtype=torch.float64, device=dev)
        vals = torch.zeros(nnz, dtype=torch.float64, device=dev)
        assert bh.initData_device(n, n, n, nnz, ones, S[0], S[1], nnz, ones, S[0], S[1]) == 0
        pair = []
        for rep in range(REPS + 1):
            assert bh.spgemm_semiring_masked_device(_lib.BHS_SR_PLUS_PAIR, S[0], S[1], nnz, vals) == 0
            if rep >= 1:
                pair.append(bh.semiring_ms)
        bh.free_mem()
        out["plus_pair_ms"] = stat(pair)
        out["ktruss"] = {}
        for k in (3, 4):
            graph.ktruss_device(bh, n, A, k)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            T, its = graph.ktruss_device(bh, n, A, k)
            torch.cuda.synchronize()
            out["ktruss"][str(k)] = {"nnz": T[1].numel(), "iterations": its, "ms": (time.perf_counter() - t0) * 1e3}
    return out


def main():
    args = sys.argv[1:]
    opts = {"torch": "--no-torch" not in args, "nx": "--no-nx" not in args, "truss": "--no-truss" not in args}
    cases = [a for a in args if not a.startswith("--")] or CASES
    dev = torch.device("cuda", 0)
    with facade._handle(np.float64, 0, None) as bh:
        for case in cases:
            print(json.dumps(run(case, bh, dev, opts)), flush=True)


if __name__ == "__main__":
    main()
