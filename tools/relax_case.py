"""What the relaxation and the fused product cost on the GPU (profiles/relax_case.md): a relax call of 1, 2 and 3 steps
beside bhs_csr_spmv_device, one sweep of the Python Jacobi it replaces and one forward Gauss-Seidel sweep, the fused
product beside the product plus two torch reductions, the Lanczos estimate, and -- with --pcg -- PCG to 1e-8 with the
Jacobi, Gauss-Seidel and Chebyshev smoothers on the MIS(2) and the classical hierarchy.  Wall times around synchronous
calls (what a cycle pays), the median of `--reps` after a warm-up; device times where the call reports them.

    python tools/relax_case.py [--case poisson27pt_128] [--dtype f64] [--reps 20] [--pcg]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

CASES = {"poisson27pt_128": ("poisson27pt", 128, 128, 128), "poisson5pt_1024": ("poisson5pt", 1024, 1024, 1),
         "aniso_1024": ("aniso", 1024, 1024, 1), "poisson27pt_32": ("poisson27pt", 32, 32, 32), "poisson5pt_256": ("poisson5pt", 256, 256, 1)}


def matrix(case, tdt, dev):
    """(n, (rowPtr, colInd, val)) on the device: Poisson values, or the 5-point operator with the y-coupling scaled by 1/128"""
    import torch
    from benchmark_spgemm_using_csr_amd import gallery
    name, nx, ny, nz = CASES[case]
    stencil = "poisson5pt" if name == "aniso" else name
    Ap, Aj = gallery.poisson_csr(stencil, nx, ny, nz)
    n = len(Ap) - 1
    r = np.repeat(np.arange(n), np.diff(Ap))
    if name == "aniso":
        eps = 1.0 / 128
        Ax = np.where(r == Aj, 2 + 2 * eps, np.where(np.abs(r - Aj) == 1, -1.0, -eps))
    else:
        Ax = np.where(r == Aj, float(len(gallery.stencil_offsets(name)) - 1), -1.0)
    up = lambda a, t: torch.from_numpy(np.ascontiguousarray(a)).to(dev).to(t)   # noqa: E731
    return n, (up(Ap, torch.int32), up(Aj, torch.int32), up(Ax, tdt))


def median_ms(fn, reps):
    import torch
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", default="poisson27pt_128", choices=sorted(CASES))
    ap.add_argument("--dtype", default="f64", choices=("f64", "f32"))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--pcg", action="store_true")
    args = ap.parse_args()
    import torch
    from benchmark_spgemm_using_csr_amd import _lib, amg, dense
    from benchmark_spgemm_using_csr_amd.facade import _handle
    vdt, tdt = (np.float64, torch.float64) if args.dtype == "f64" else (np.float32, torch.float32)
    dev = torch.device("cuda", 0)
    n, A = matrix(args.case, tdt, dev)
    rec = {"case": args.case, "dtype": args.dtype, "n": n, "nnz": int(A[1].numel())}
    with _handle(vdt, 0, None) as bh, _handle(vdt, 0, None) as h2:
        diag = bh.csr_reduce_device(n, n, A, _lib.BHS_AXIS_DIAG, _lib.BHS_RED_PLUS)
        g = torch.Generator(device="cpu").manual_seed(0)
        b, x, w = (torch.randn(n, generator=g, dtype=torch.float64).to(dev).to(tdt) for _ in range(3))
        y = torch.empty_like(b)
        rec["spmv_ms"] = median_ms(lambda: dense.csr_spmv_raw_device(bh, n, n, A[1].numel(), A[2], A[0], A[1], 1.0, x, 0.0, y), args.reps)
        rec["spmv_device_ms"] = bh.spmv_ms
        carry = torch.zeros_like(x)
        for steps in (1, 2, 3):
            coef = amg.chebyshev_coefficients(0.6, 2.2, steps)
            xs = x.clone()
            for zero in (False, True):
                key = "relax%d%s" % (steps, "_zero" if zero else "")
                rec[key + "_ms"] = median_ms(lambda: amg.relax_raw_device(bh, n, A[1].numel(), A[2], A[0], A[1], diag, steps, coef, b, xs,
                                                                          carry, 1 if zero else 0), args.reps)
                rec[key + "_device_ms"] = bh.relax_ms
        rec["python_jacobi_sweep_ms"] = median_ms(lambda: amg._jacobi(bh, A, diag, b, x, 2.0 / 3.0, 1), args.reps)
        t0 = time.perf_counter()
        S = amg.strength_device(bh, n, A, 0.0)
        coloring = amg.color_device(bh, n, S, 0)
        torch.cuda.synchronize()
        rec["colouring_setup_ms"] = (time.perf_counter() - t0) * 1e3
        rec["ncolors"] = coloring[1]
        xs = x.clone()
        rec["gs_forward_sweep_ms"] = median_ms(lambda: amg.gs_device(bh, A, diag, coloring, b, xs, 1.0, 1, "forward"), args.reps)
        z = torch.empty_like(b)
        dots = np.zeros(2)
        rec["spmv_dots_ms"] = median_ms(lambda: dense.csr_spmv_dots_raw_device(bh, n, n, A[1].numel(), A[2], A[0], A[1], -1.0, x, 1.0, b, z,
                                                                            w, dots), args.reps)
        rec["spmv_dots_device_ms"] = bh.spmv_dots_ms

        def separate():
            r = dense.csr_spmv_device(bh, n, n, A, x, alpha=-1.0, beta=1.0, y=b.clone())
            return float(torch.dot(r, r)), float(torch.dot(w, r))
        rec["spmv_plus_two_torch_dots_ms"] = median_ms(separate, args.reps)
        t0 = time.perf_counter()
        rho = amg.spectral_radius_device(bh, n, A, diag)
        torch.cuda.synchronize()
        rec["lanczos10_ms"] = (time.perf_counter() - t0) * 1e3
        rec["lanczos10_estimate"] = rho
        if args.pcg:
            rec["pcg"] = {}
            for hier, setup in (("mis2", lambda om: amg.sa_setup_device((bh, h2), n, A, omega=om)),
                                ("classical", lambda om: amg.rs_setup_device((bh, h2), n, A))):
                for om in ((2.0 / 3.0, "estimate") if hier == "mis2" else (None,)):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    levels, info = setup(om)
                    torch.cuda.synchronize()
                    setup_ms = (time.perf_counter() - t0) * 1e3
                    for smoother in ("jacobi", "gs", "chebyshev2", "chebyshev3"):
                        torch.cuda.synchronize()
                        t0 = time.perf_counter()
                        if smoother.startswith("chebyshev"):
                            sm = amg.cheby_setup_device(bh, levels, degree=int(smoother[-1]))
                            _, its, res = amg._pcg_chebyshev(bh, levels, b, 1e-8, 200, sm)
                        else:
                            _, its, res = amg.pcg_device(bh, levels, b, 1e-8, 200, smoother)
                        torch.cuda.synchronize()
                        rec["pcg"]["%s omega %s %s" % (hier, om, smoother)] = {
                            "levels": [r["n"] for r in info], "setup_ms": setup_ms, "iterations": its,
                            "solve_ms": (time.perf_counter() - t0) * 1e3, "relative_residual": res[-1] / res[0]}
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
