"""The factorised sparse approximate inverse (bhs_csr_fsai_device) and the CG it preconditions (amg.fsai_pcg_device) beside
ILU(0) and the smoothed-aggregation hierarchy, measured in one process on the same device arrays, in double; prints one JSON
line per case.

    python tools/fsai_case.py [case ...]      cases: poisson27pt_128 poisson5pt_1024 aniso_1024 blocks128 (default: all four)

blocks128 is 2048 dense SPD blocks of order 128 with their lower triangles as G -- rows of every length from 1 to 128, so all
three kernel families run -- and measures the setup alone.

Per case, on the patterns tril(A) (the selection's band) and tril(A^2) (a device multiply of A with itself, then the band):
  setup   device ms of bhs_csr_fsai_device (median and minimum of REPS calls after 2, per-kernel timers off) and, from one
          more call with them on, the ms and rows of each family; the transpose that makes G^T; beside them the wall ms of
          amg.ilu0_setup_device in colour order (colouring, permutation, level analysis and factorisation)
  apply   wall ms of amg.fsai_apply_device (two products) beside amg.ilu0_apply_device in natural and in colour order
  solve   iterations and wall ms, setup included, of amg.fsai_pcg_device to 1e-8 from a seeded random right-hand side, beside
          amg.ilu0_pcg_device in colour order and amg.pcg_device on the smoothed-aggregation hierarchy; the true residual
          of each"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from benchmark_spgemm_using_csr_amd import _lib, amg, dense, facade  # noqa: E402
from benchmark_spgemm_using_csr_amd.facade import select_spec  # noqa: E402
from tools.cf_case import REPS, matrix, stat, wall  # noqa: E402

CASES = ("poisson27pt_128", "poisson5pt_1024", "aniso_1024", "blocks128")
MAXITER = 4000


def tril_square_device(bh, n, A):
    """the pattern of tril(A A) on the device"""
    nnz = A[1].numel()
    assert bh.initData_device(n, n, n, nnz, A[2], A[0], A[1], nnz, A[2], A[0], A[1]) == 0 and bh.spgemm() == 0
    C = amg._result_device(bh, n, A[0].device)
    assert bh.free_mem() == 0
    Gp, Gj, _ = bh.csr_select_device(n, n, C, select_spec(band=(None, 0)), values=False)
    return Gp, Gj


def blocks(order, count):
    """`count` dense SPD blocks of this order on the diagonal (a_ij = -1 / (1 + |i - j|), the diagonal their sum + 1), rows
    ascending: (rowPtr, colInd, val) and the pattern of its lower triangle -- rows of 1 .. order entries"""
    k = np.arange(order)
    B = -1.0 / (1.0 + np.abs(k[:, None] - k[None, :]))
    np.fill_diagonal(B, 0.0)
    np.fill_diagonal(B, -B.sum(axis=1) + 1.0)
    n = order * count
    start = np.repeat(np.arange(count) * order, order)
    rp = np.arange(n + 1, dtype=np.int64) * order
    col = (start[:, None] + k[None, :]).ravel()
    val = np.tile(B.ravel(), count)
    lens = np.tile(k + 1, count)
    gp = np.concatenate([[0], np.cumsum(lens)])
    gj = np.concatenate([start[r] + k[:r % order + 1] for r in range(n)])
    return (rp, col, val), (gp, gj)


def fsai_setup(h1, A, Gp, Gj, dev):
    """device ms of bhs_csr_fsai_device on this pattern, in all and by family"""
    n, nnzG = Gp.numel() - 1, int(Gj.numel())
    Gx = torch.empty(nnzG, dtype=torch.float64, device=dev)
    torch.cuda.synchronize()
    call = lambda: amg.fsai_raw_device(h1, n, A[1].numel(), A[0], A[1], A[2], nnzG, Gp, Gj, Gx, 0)   # noqa: E731
    assert h1.set_option("kernel_stats", 0) == 0
    ms = []
    for rep in range(REPS + 2):
        assert call() == 0
        if rep >= 2:
            ms.append(h1.fsai_ms)
    assert h1.set_option("kernel_stats", 1) == 0
    assert call() == 0
    fam = {s["name"]: {"ms": round(s["ms"], 4), "rows": s["rows"]} for s in h1.kernel_stats() if s["launches"] > 0}
    lens = (Gp[1:] - Gp[:-1])
    return {"nnzG": nnzG, "longest_row": int(lens.max()), "setup_ms": stat(ms), "families": fam, "bad_row": h1.fsai_bad_row}


def run(case, h1, h2, dev):
    up = lambda x, dt: torch.from_numpy(np.ascontiguousarray(x, dt)).to(dev)   # noqa: E731
    if case.startswith("blocks"):                                   # the setup alone: every length up to the order
        order = int(case[len("blocks"):])
        (rp, col, val), (gp, gj) = blocks(order, (1 << 18) // order)
        A = (up(rp, np.int32), up(col, np.int32), up(val, np.float64))
        out = {"case": case, "n": len(rp) - 1, "nnz": len(col), "library": os.path.basename(_lib.SO_PATH), "source_digest": _lib.source_digest()}
        out["fsai tril(A)"] = fsai_setup(h1, A, up(gp, np.int32), up(gj, np.int32), dev)
        return out
    rp, col, val = matrix(case)
    n = len(rp) - 1
    A = (up(rp, np.int32), up(col, np.int32), up(val, np.float64))
    b = up(np.random.default_rng(4).standard_normal(n), np.float64)
    out = {"case": case, "n": n, "nnz": len(col), "library": os.path.basename(_lib.SO_PATH), "source_digest": _lib.source_digest()}
    true = lambda x: float(torch.linalg.norm(dense.csr_spmv_device(h1, n, n, A, x, alpha=-1.0, beta=1.0, y=b.clone())) / torch.linalg.norm(b))   # noqa: E731
    patterns = {"tril(A)": h1.csr_select_device(n, n, A, select_spec(band=(None, 0)), values=False)[:2], "tril(A^2)": tril_square_device(h1, n, A)}
    for name, (Gp, Gj) in patterns.items():
        res = fsai_setup(h1, A, Gp, Gj, dev)
        M = amg.fsai_setup_device(h1, A, (Gp, Gj))
        res["transpose_ms"] = h1.transpose_ms
        z = torch.empty_like(b)
        ts = [wall(lambda: amg.fsai_apply_device(h1, M, b, z))[1] for _ in range(REPS + 2)][2:]
        res["apply_wall_ms"] = stat(ts)
        amg.fsai_pcg_device(h1, A, b, 1e-8, 3, (Gp, Gj))
        (x, its, _), t = wall(lambda: amg.fsai_pcg_device(h1, A, b, 1e-8, MAXITER, (Gp, Gj)))
        res["pcg"] = {"iterations": its, "wall_ms": t, "residual": true(x)}
        out["fsai " + name] = res
        del M
        torch.cuda.empty_cache()
    for o in ("natural", "colour"):
        amg.ilu0_setup_device(h1, A, o)
        M, t = wall(lambda: amg.ilu0_setup_device(h1, A, o))
        z = torch.empty_like(b)
        ts = [wall(lambda: amg.ilu0_apply_device(h1, M, b, z))[1] for _ in range(REPS + 2)][2:]
        out["ilu0 " + o] = {"setup_wall_ms": t, "levels": [M["lower"][1], M["upper"][1]], "apply_wall_ms": stat(ts)}
    amg.ilu0_pcg_device(h1, A, b, 1e-8, 3, "colour")
    (x, its, _), t = wall(lambda: amg.ilu0_pcg_device(h1, A, b, 1e-8, MAXITER, "colour"))
    out["ilu0 colour"]["pcg"] = {"iterations": its, "wall_ms": t, "residual": true(x)}

    def amg_pcg():
        levels, _ = amg.sa_setup_device((h1, h2), n, A)
        return amg.pcg_device(h1, levels, b, 1e-8, 200)
    amg_pcg()
    (x, its, _), t = wall(amg_pcg)
    out["amg_pcg"] = {"iterations": its, "wall_ms": t, "residual": true(x)}
    return out


def main():
    cases = sys.argv[1:] or CASES
    dev = torch.device("cuda", 0)
    with facade._handle(np.float64, 0, None) as h1, facade._handle(np.float64, 0, None) as h2:
        for case in cases:
            print(json.dumps(run(case, h1, h2, dev)), flush=True)
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
