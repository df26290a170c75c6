"""CSR x dense through a facade handle: y = alpha A x + beta y and Y = alpha A X + beta Y (bhs_csr_spmv_device,
bhs_csr_spmm_device; include/bhsparse_hip.h, "CSR x dense").

Functions of a `facade.bhsparse` handle, not methods of it: the raw calls on caller-given arrays (torch tensors on the
handle's GPU or raw device addresses), the same on torch tensors with the output made here, and conveniences on host CSR
arrays that stage everything on the device for one call.  Every call is a thin one into the C-ABI; a missing library
raises, nothing is computed on the host."""
import numpy as np

from . import _lib
from .facade import BhsparseError, _alloc, _check, _device_csr, _handle, _ptr, _upload  # noqa: F401


def csr_spmv_raw_device(bh, m, n, nnzA, d_valA, d_rowPtrA, d_colIndA, alpha, d_x, beta, d_y):
    """bhs_csr_spmv_device on caller-given arrays (d_valA may be None: every entry counts as 1): the status code; sets
    bh.spmv_ms."""
    if bh._h is None:
        return _lib.BHS_ERR_NOT_READY
    return bh._timed(bh._lib.bhs_csr_spmv_device, "spmv_ms", int(m), int(n), int(nnzA), _ptr(d_valA), _ptr(d_rowPtrA),
                     _ptr(d_colIndA), float(alpha), _ptr(d_x), float(beta), _ptr(d_y))


def csr_spmm_raw_device(bh, m, n, nnzA, d_valA, d_rowPtrA, d_colIndA, k, alpha, d_X, ldX, beta, d_Y, ldY):
    """bhs_csr_spmm_device on caller-given arrays (X: n x k, Y: m x k, row-major with leading dimensions ldX, ldY): the
    status code; sets bh.spmv_ms."""
    if bh._h is None:
        return _lib.BHS_ERR_NOT_READY
    return bh._timed(bh._lib.bhs_csr_spmm_device, "spmv_ms", int(m), int(n), int(nnzA), _ptr(d_valA), _ptr(d_rowPtrA),
                     _ptr(d_colIndA), int(k), float(alpha), _ptr(d_X), int(ldX), float(beta), _ptr(d_Y), int(ldY))


def csr_spmv_device(bh, m, n, A, x, alpha=1.0, beta=0.0, y=None):
    """y = alpha A x + beta y on device arrays: A = (rowPtr, colInd, val or None) and x (n values) torch tensors on the
    handle's GPU; y (m values) is written in place, or made here when None (beta == 0 never reads it).  Returns y; raises
    BhsparseError on failure."""
    import torch
    Ap, Aj, Ax = A
    if y is None:
        y = _alloc(m, x.dtype, x.device)[:m]
    torch.cuda.synchronize()                           # the library works on its own stream (see facade.initData_device)
    _check(csr_spmv_raw_device(bh, m, n, Aj.numel(), Ax, Ap, Aj, alpha, x, beta, y), "bhs_csr_spmv_device")
    return y


def csr_spmm_device(bh, m, n, A, X, alpha=1.0, beta=0.0, Y=None):
    """Y = alpha A X + beta Y on device arrays: A = (rowPtr, colInd, val or None) torch tensors on the handle's GPU, X
    (n x k) and Y (m x k) 2-D torch tensors there whose rows are contiguous -- stride(0) is the leading dimension, so a
    column slice of a wider tensor is passed as it is.  Y is written in place, or made here when None.  Returns Y; raises
    BhsparseError on failure."""
    import torch
    Ap, Aj, Ax = A
    k = X.shape[1] if X.dim() == 2 else 0
    if Y is None and k:
        Y = _alloc(m * k, X.dtype, X.device)[:m * k].view(m, k)
    for name, T, rows in (("X", X, n), ("Y", Y, m)):
        if not k or T.dim() != 2 or tuple(T.shape) != (rows, k) or (k > 1 and T.stride(1) != 1):
            raise ValueError("%s is a row-major %d x k tensor, k >= 1" % (name, rows))
    ld = lambda T: max(int(T.stride(0)), k) if T.shape[0] > 1 else k   # noqa: E731  (one row or none: any ld will do)
    torch.cuda.synchronize()                           # the library works on its own stream (see facade.initData_device)
    _check(csr_spmm_raw_device(bh, m, n, Aj.numel(), Ax, Ap, Aj, k, alpha, X, ld(X), beta, Y, ld(Y)), "bhs_csr_spmm_device")
    return Y


def spmm_csr(m, n, Ap, Aj, Ax, X, alpha=1.0, beta=0.0, Y=None, value_dtype=np.float64, device=0):
    """Convenience: Y = alpha A X + beta Y once on host arrays (A: m x n CSR, rows in any order, duplicates add up, Ax may
    be None: every entry counts as 1; X: n x k, Y: m x k or None), staged as torch tensors on the handle's device.  Returns
    (Y value_dtype[m, k], info) with info["kernels"], info["ms"].  Needs no multiply data."""
    A = _device_csr(Ap, Aj, Ax, value_dtype, device)
    X = np.asarray(X)
    dX = _upload(X.reshape(n, -1), value_dtype, device)
    dY = None if Y is None else _upload(np.asarray(Y).reshape(m, -1), value_dtype, device)
    with _handle(value_dtype, device, None) as bh:
        out = csr_spmm_device(bh, m, n, A, dX, alpha, beta, dY)
        return out.cpu().numpy(), {"kernels": bh.kernel_stats(), "ms": bh.spmv_ms}


def spmv_csr(m, n, Ap, Aj, Ax, x, alpha=1.0, beta=0.0, y=None, value_dtype=np.float64, device=0):
    """Convenience: y = alpha A x + beta y once on host arrays (x: n values, y: m values or None).  Returns
    (y value_dtype[m], info) with info["kernels"], info["ms"]."""
    A = _device_csr(Ap, Aj, Ax, value_dtype, device)
    dx = _upload(x, value_dtype, device)
    dy = None if y is None else _upload(y, value_dtype, device)
    with _handle(value_dtype, device, None) as bh:
        out = csr_spmv_device(bh, m, n, A, dx, alpha, beta, dy)
        return out.cpu().numpy(), {"kernels": bh.kernel_stats(), "ms": bh.spmv_ms}


def residual_csr(m, n, Ap, Aj, Ax, x, b, value_dtype=np.float64, device=0):
    """Convenience: the residual b - A x (alpha = -1, beta = 1 on a copy of b).  Returns (r value_dtype[m], info)."""
    return spmv_csr(m, n, Ap, Aj, Ax, x, alpha=-1.0, beta=1.0, y=b, value_dtype=value_dtype, device=device)
