"""Orderings that make a matrix narrow: reverse Cuthill-McKee on the device (bhs_csr_rcm_device; include/bhsparse_hip.h,
"bandwidth-reducing ordering") and what goes with it -- the symmetric pattern it takes, the bandwidth and the profile it
lowers, the permuted matrix.  Functions of a `facade.bhsparse` handle, as in graph.py and amg.py; amg.ilu0_pcg_rcm_device is
ILU(0)-preconditioned CG in this ordering."""
import ctypes as C

import numpy as np

from . import _lib
from .facade import _alloc, _check, _device_csr, _handle, _host, _ptr

BHS_RCM_PERIPHERAL, BHS_RCM_NO_REVERSE = 1, 2


def rcm_raw_device(bh, n, nnz, dSp, dSj, flags, perm, level, start):
    """bhs_csr_rcm_device on caller-given arrays, the C arguments in order (level and start may be None): the status code,
    BHS_ERR_NOT_READY without a platform; sets bh.rcm_ncomp, bh.rcm_depth, bh.rcm_sweeps (functions of the pattern),
    bh.rcm_passes (a multiple of the batch; depends on timing) and bh.rcm_ms on success only."""
    if bh._h is None:
        return _lib.BHS_ERR_NOT_READY
    ncomp, depth, sweeps, passes, ms = C.c_int(0), C.c_int(0), C.c_int(0), C.c_int(0), C.c_double(0)
    err = bh._lib.bhs_csr_rcm_device(bh._h, int(n), int(nnz), _ptr(dSp), _ptr(dSj), int(flags), _ptr(perm), _ptr(level), _ptr(start),
                                     C.byref(ncomp), C.byref(depth), C.byref(sweeps), C.byref(passes), C.byref(ms))
    if err == _lib.BHS_SUCCESS:
        bh.rcm_ncomp, bh.rcm_depth, bh.rcm_sweeps = int(ncomp.value), int(depth.value), int(sweeps.value)
        bh.rcm_passes, bh.rcm_ms = int(passes.value), float(ms.value)
    return err


def rcm_device(bh, n, S, peripheral=True, reverse=True):
    """The reverse Cuthill-McKee ordering of the n-vertex pattern S = (rowPtr, colInd[, anything]), torch tensors on the
    handle's GPU: rows strictly ascending, structurally symmetric (symmetric_pattern_device makes one of any matrix).
    peripheral: the George-Liu pseudo-peripheral start of every component; reverse=False: the Cuthill-McKee order itself.
    Returns perm, an int32 device tensor: perm[k] is the old index of new row k, what permute_device takes.  bh.rcm_ncomp,
    bh.rcm_depth, bh.rcm_sweeps, bh.rcm_passes and bh.rcm_ms hold the counts and the device time.  Raises BhsparseError on
    failure -- BHS_ERR_INVALID_ARG for a pattern that is not ascending or not symmetric."""
    import torch
    Sp, Sj = S[0], S[1]
    perm = _alloc(n, torch.int32, Sp.device)
    flags = (BHS_RCM_PERIPHERAL if peripheral else 0) | (0 if reverse else BHS_RCM_NO_REVERSE)
    torch.cuda.synchronize()                           # the library works on its own stream (see facade.initData_device)
    _check(rcm_raw_device(bh, n, Sj.numel(), Sp, Sj if Sj.numel() else None, flags, perm, None, None), "bhs_csr_rcm_device")
    return perm[:n]


def symmetric_pattern_device(bh, n, A):
    """pattern(A) U pattern(A^T) of the n x n matrix A = (rowPtr, colInd, val), rows strictly ascending, as (rowPtr, colInd):
    amg.strength_device(bh, n, A, 0.0).  Its rows are checked; where they do not come out strictly ascending the pattern is
    made canonical through assemble.canonical_csr_device."""
    import torch
    from .amg import strength_device
    from .assemble import canonical_csr_device
    Sp, Sj = strength_device(bh, n, A, 0.0)
    if Sj.numel() > 1:
        inner = torch.ones(Sj.numel(), dtype=torch.bool, device=Sj.device)
        inner[Sp[:n][Sp[:n] < Sj.numel()].long()] = False            # a row's first entry has none before it
        if bool((inner[1:] & (Sj[1:] <= Sj[:-1])).any()):
            Sp, Sj, _ = canonical_csr_device(bh, n, n, (Sp, Sj, None))
    return Sp, Sj


def bandwidth_profile_device(n, A, perm=None):
    """(bandwidth, profile) of A(perm, perm) for A = (rowPtr, colInd[, anything]) on the device, perm as rcm_device returns
    it (None: A as it is): the greatest |i - j| over the entries, and the sum over the rows of i - (the first column <= i).
    Torch plumbing, exact in int64."""
    import torch
    Ap, Aj = A[0], A[1]
    if n == 0:
        return 0, 0
    dev = Ap.device
    idx = torch.arange(n, dtype=torch.int64, device=dev)
    new = idx
    if perm is not None:
        new = torch.empty(n, dtype=torch.int64, device=dev)
        new[perm.long()] = idx
    lens = (Ap[1:n + 1] - Ap[:n]).to(torch.int64)
    r = new[torch.repeat_interleave(idx, lens, output_size=Aj.numel())]
    c = new[Aj.long()]
    first = idx.clone().scatter_reduce(0, r, c, "amin", include_self=True)
    band = int((r - c).abs().max()) if Aj.numel() else 0
    return band, int((idx - first).sum())


def permute_device(bh, n, A, perm):
    """A(perm, perm) for the n x n matrix A = (rowPtr, colInd, val), rows ascending (bhsparse.csr_extract_device):
    (rowPtr, colInd, val)."""
    Zp, Zj, Zx, _ = bh.csr_extract_device(n, n, A, rows=perm, cols=perm)
    return Zp, Zj, Zx


def rcm_csr(n, Ap, Aj, Ax, peripheral=True, reverse=True, value_dtype=np.float64, device=0):
    """Convenience: the ordering once on host CSR arrays.  Returns (perm int32[n], (Zp, Zj, Zx) = A(perm, perm), info) with
    info["ncomp"], ["depth"], ["sweeps"], ["passes"], ["ms"], ["kernels"] and ["bandwidth"], ["profile"] as (before, after)."""
    A = _device_csr(Ap, Aj, Ax, value_dtype, device)
    with _handle(value_dtype, device, None) as bh:
        S = symmetric_pattern_device(bh, n, A)
        perm = rcm_device(bh, n, S, peripheral, reverse)
        info = {"ncomp": bh.rcm_ncomp, "depth": bh.rcm_depth, "sweeps": bh.rcm_sweeps, "passes": bh.rcm_passes, "ms": bh.rcm_ms,
                "kernels": bh.kernel_stats()}
        before, after = bandwidth_profile_device(n, A), bandwidth_profile_device(n, A, perm)
        info["bandwidth"], info["profile"] = (before[0], after[0]), (before[1], after[1])
        Z = permute_device(bh, n, A, perm)
        return _host(perm)[0], _host(*Z), info
