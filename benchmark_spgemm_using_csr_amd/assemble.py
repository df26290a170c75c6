"""A CSR matrix from triplets on the device (bhs_coo_assemble_device, bhs_coo_assemble_values_device; include/bhsparse_hip.h,
"assembly"): rows ascending, duplicates combined -- added in a fixed order, or the first or the last kept, or all kept --
and the map (entryPtr, perm) that re-values the same pattern from new values, as finite-element codes do every time step.

Functions of a `facade.bhsparse` handle, as in dense.py and graph.py.  Every output is a function of the input alone: the
same bits from run to run, from handle to handle and, for values both types hold, in both builds.

canonical_csr_device turns any CSR -- rows unsorted, repeats -- into one the strict calls (the add, the C/F splitting, the
interpolation, ILU(0)) accept; symmetric_from_edges_device stores an edge list in both directions."""
import ctypes as C

import numpy as np

from . import _lib
from .facade import BhsparseError, _alloc, _check, _handle, _head, _host, _ptr, _upload  # noqa: F401


def _flags(combine, ignore_negative=False):
    if combine not in _lib.COO_COMBINE:
        raise ValueError("combine: one of %s" % ", ".join(sorted(_lib.COO_COMBINE)))
    return _lib.COO_COMBINE[combine] | (_lib.BHS_COO_IGNORE_NEGATIVE if ignore_negative else 0)


def coo_assemble_raw_device(bh, m, n, nnz_in, d_rows, d_cols, d_vals, flags, d_rowPtrZ, d_colIndZ, d_valZ, d_entryPtr, d_perm):
    """bhs_coo_assemble_device on caller-given arrays, the C arguments in order (d_vals, d_valZ, d_entryPtr and d_perm may be
    None): the status code; sets bh.assemble_nnz, bh.assemble_nkept and bh.assemble_ms on success only."""
    if bh._h is None:
        return _lib.BHS_ERR_NOT_READY
    nnzZ, nkept, ms = C.c_int(0), C.c_int(0), C.c_double(0)
    err = bh._lib.bhs_coo_assemble_device(bh._h, int(m), int(n), int(nnz_in), _ptr(d_rows), _ptr(d_cols), _ptr(d_vals), int(flags),
                                          _ptr(d_rowPtrZ), _ptr(d_colIndZ), _ptr(d_valZ), _ptr(d_entryPtr), _ptr(d_perm),
                                          C.byref(nnzZ), C.byref(nkept), C.byref(ms))
    if err == _lib.BHS_SUCCESS:
        bh.assemble_nnz, bh.assemble_nkept, bh.assemble_ms = int(nnzZ.value), int(nkept.value), float(ms.value)
    return err


def coo_values_raw_device(bh, nnz_in, d_vals, nnzZ, d_entryPtr, d_perm, flags, d_valZ):
    """bhs_coo_assemble_values_device on caller-given arrays, the C arguments in order: the status code; sets bh.assemble_ms
    on success only."""
    if bh._h is None:
        return _lib.BHS_ERR_NOT_READY
    ms = C.c_double(0)
    err = bh._lib.bhs_coo_assemble_values_device(bh._h, int(nnz_in), _ptr(d_vals), int(nnzZ), _ptr(d_entryPtr), _ptr(d_perm),
                                                 int(flags), _ptr(d_valZ), C.byref(ms))
    if err == _lib.BHS_SUCCESS:
        bh.assemble_ms = float(ms.value)
    return err


def coo_assemble_device(bh, m, n, rows, cols, vals=None, combine="sum", ignore_negative=False, want_map=False):
    """Z (m x n) from the triplets (rows, cols, vals): int32 torch tensors of one length on the handle's GPU and values of the
    handle's type, or None for the pattern alone.  combine: "sum" (added in the stable order, in double, one rounding),
    "first", "last" (by input position) or "keep" (every triplet its own entry: sorted, with repeats).  ignore_negative: a
    triplet with a negative row or column is dropped; otherwise it is an error, as an index >= m or >= n always is.
    Returns (rowPtr int32[m + 1], colInd int32[nnzZ], val[nnzZ] or None) -- views of length nnzZ into arrays with room for
    every triplet, nothing is copied to trim them -- and with want_map a fourth element (entryPtr int32[nnzZ + 1], perm
    int32[nkept], number of triplets) for coo_values_device.  bh.assemble_nnz, bh.assemble_nkept and bh.assemble_ms hold the
    counts and the device time.  Raises BhsparseError on failure."""
    import torch
    nnz = rows.numel()
    if cols.numel() != nnz or (vals is not None and vals.numel() != nnz):
        raise ValueError("coo_assemble_device: rows, cols and vals of one length")
    dev = rows.device
    Zp = torch.empty(m + 1, dtype=torch.int32, device=dev)
    Zj = _alloc(nnz, torch.int32, dev)
    Zx = _alloc(nnz, vals.dtype, dev) if vals is not None else None
    ent = _alloc(nnz + 1, torch.int32, dev) if want_map else None
    pm = _alloc(nnz, torch.int32, dev) if want_map else None
    torch.cuda.synchronize()                           # the library works on its own stream (see facade.initData_device)
    some = nnz > 0
    _check(coo_assemble_raw_device(bh, m, n, nnz, rows if some else None, cols if some else None, vals if some else None,
                                   _flags(combine, ignore_negative), Zp, Zj, Zx if some else None, ent, pm),
           "bhs_coo_assemble_device")
    nz = bh.assemble_nnz
    out = (Zp, Zj[:nz], _head(Zx, nz))
    if want_map:
        out += ((ent[:nz + 1], pm[:bh.assemble_nkept], nnz),)
    return out


def coo_values_device(bh, vals, map, combine="sum", out=None):
    """The values of a known pattern from new triplet values: `map` is the fourth element coo_assemble_device returned with
    want_map, vals the values of the same triplets in the same positions.  Returns val[nnzZ] (out, when given); its bits are
    those of a full assembly.  combine: "sum", "first" or "last".  Raises BhsparseError where the map is not one."""
    import torch
    ent, pm, nnz = map
    if vals.numel() != nnz:
        raise ValueError("coo_values_device: %d values for a map of %d triplets" % (vals.numel(), nnz))
    nz = ent.numel() - 1
    if out is None:
        out = _alloc(nz, vals.dtype, vals.device)[:nz]
    torch.cuda.synchronize()
    _check(coo_values_raw_device(bh, nnz, vals if nnz else None, nz, ent, pm if nnz else None, _flags(combine), out),
           "bhs_coo_assemble_values_device")
    return out


def coo_to_csr(m, n, rows, cols, vals, combine="sum", ignore_negative=False, value_dtype=np.float64, device=0):
    """Convenience: coo_assemble_device once on host triplets (vals may be None).  Returns numpy (rowPtr int32[m + 1], colInd
    int32[nnz], val value_dtype[nnz] or None)."""
    r, c = _upload(rows, np.int32, device), _upload(cols, np.int32, device)
    v = None if vals is None else _upload(vals, value_dtype, device)
    with _handle(value_dtype, device, None) as bh:
        Zp, Zj, Zx = coo_assemble_device(bh, m, n, r, c, v, combine, ignore_negative)
        return _host(Zp, Zj) + (None if Zx is None else Zx.cpu().numpy(),)


def canonical_csr_device(bh, m, n, A, combine="sum"):
    """The m x n CSR A = (rowPtr, colInd, val or None) -- torch tensors on the handle's GPU, rows in any order, repeats legal
    -- with its rows strictly ascending and repeats combined ("keep": ascending, repeats kept): (rowPtr, colInd, val or None).
    The triplets' rows come from rowPtr by torch.repeat_interleave; the rest is coo_assemble_device."""
    import torch
    Ap, Aj, Ax = A[0], A[1], A[2] if len(A) > 2 else None
    lens = (Ap[1:m + 1] - Ap[:m]).to(torch.int64)
    rows = torch.repeat_interleave(torch.arange(m, dtype=torch.int32, device=Ap.device), lens, output_size=Aj.numel())
    return coo_assemble_device(bh, m, n, rows, Aj, Ax, combine)


def symmetric_from_edges_device(bh, n, lo, hi, w=None, combine="sum"):
    """The undirected edges (lo[e], hi[e]) of weight w[e] as a symmetric n x n CSR, both directions stored, rows ascending,
    parallel edges combined: (rowPtr, colInd, val or None).  On the edge list of graph.spanning_forest_device it is what
    graph.forest_csr_device builds, through the library."""
    import torch
    rows, cols = torch.cat([lo, hi]).to(torch.int32), torch.cat([hi, lo]).to(torch.int32)
    return coo_assemble_device(bh, n, n, rows, cols, None if w is None else torch.cat([w, w]), combine)
