"""CSR x dense through a facade handle: y = alpha A x + beta y and Y = alpha A X + beta Y (bhs_csr_spmv_device,
bhs_csr_spmm_device; include/bhsparse_hip.h, "CSR x dense"), and the same over a semiring with an output mask and
accumulation, Y<M> (+)= A (+).(x) X (bhs_csr_spmv_semiring_device, bhs_csr_spmm_semiring_device; "semiring CSR x dense"),
and in the push direction from a list of rows (bhs_csr_push_semiring_device; "sparse frontier x CSR").

Functions of a `facade.bhsparse` handle, not methods of it: the raw calls on caller-given arrays (torch tensors on the
handle's GPU or raw device addresses), the same on torch tensors with the output made here, and conveniences on host CSR
arrays that stage everything on the device for one call.  Every call is a thin one into the C-ABI; a missing library
raises, nothing is computed on the host."""
import ctypes as C

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


# ---------------------------------------------------------------- the sampled dense-dense product
def csr_sddmm_raw_device(bh, m, n, nnzM, d_valM, d_rowPtrM, d_colIndM, k, alpha, d_X, ldX, d_Y, ldY, beta, d_valZ, flags):
    """bhs_csr_sddmm_device on caller-given arrays, the C arguments in order (include/bhsparse_hip.h, "sampled dense-dense
    product"; X: m x k, Y: n x k, row-major with leading dimensions ldX, ldY; d_valM may be None without
    BHS_SDDMM_TIMES_M; d_valZ may be d_valM itself): the status code; sets bh.sddmm_ms."""
    if bh._h is None:
        return _lib.BHS_ERR_NOT_READY
    return bh._timed(bh._lib.bhs_csr_sddmm_device, "sddmm_ms", int(m), int(n), int(nnzM), _ptr(d_valM), _ptr(d_rowPtrM),
                     _ptr(d_colIndM), int(k), float(alpha), _ptr(d_X), int(ldX), _ptr(d_Y), int(ldY), float(beta), _ptr(d_valZ),
                     int(flags))


def csr_sddmm_device(bh, m, n, M, X, Y, alpha=1.0, beta=0.0, Z=None, times_m=False):
    """Z(i, j) = alpha (X(i, :) . Y(j, :)) [M(i, j)] + beta Z(i, j) on the entries of M: M = (rowPtr, colInd, val or None)
    torch tensors on the handle's GPU (val is read with times_m only), X (m x k) and Y (n x k) 2-D torch tensors there whose
    rows are contiguous -- stride(0) is the leading dimension; Y may be X itself.  Z (nnz values) is written in place -- it
    may be M's val itself --, or made here when None (beta == 0 never reads it).  Returns Z's values; sets bh.sddmm_ms;
    raises BhsparseError on failure."""
    import torch
    Mp, Mj, Mx = M
    nnz = Mj.numel()
    k = X.shape[1] if X.dim() == 2 else 0
    for name, T, rows in (("X", X, m), ("Y", Y, n)):
        if not k or T.dim() != 2 or tuple(T.shape) != (rows, k) or (k > 1 and T.stride(1) != 1):
            raise ValueError("%s is a row-major %d x k tensor, k >= 1" % (name, rows))
    if times_m and Mx is None:
        raise ValueError("times_m wants M's values")
    if Z is None:
        Z = _alloc(nnz, X.dtype, X.device)[:nnz]
    ld = lambda T: max(int(T.stride(0)), k) if T.shape[0] > 1 else k   # noqa: E731  (one row or none: any ld will do)
    torch.cuda.synchronize()                           # the library works on its own stream (see facade.initData_device)
    _check(csr_sddmm_raw_device(bh, m, n, nnz, Mx if times_m else None, Mp, Mj, k, alpha, X, ld(X), Y, ld(Y), beta, Z,
                                _lib.BHS_SDDMM_TIMES_M if times_m else 0), "bhs_csr_sddmm_device")
    return Z


def sddmm_csr(m, n, Mp, Mj, Mx, X, Y, alpha=1.0, beta=0.0, Z=None, times_m=False, value_dtype=np.float64, device=0):
    """Convenience: the sampled product once on host arrays (M: m x n CSR, rows in any order, duplicates each get their own
    value, Mx may be None without times_m; X: m x k, Y: n x k; Z: nnz values or None), staged as torch tensors on the
    handle's device.  Returns (Z's values value_dtype[nnz], info) with info["kernels"], info["ms"].  Needs no multiply
    data."""
    M = _device_csr(Mp, Mj, Mx, value_dtype, device)
    dX = _upload(np.asarray(X).reshape(m, -1), value_dtype, device)
    dY = _upload(np.asarray(Y).reshape(n, -1), value_dtype, device)
    dZ = None if Z is None else _upload(np.asarray(Z).reshape(-1), value_dtype, device)
    with _handle(value_dtype, device, None) as bh:
        out = csr_sddmm_device(bh, m, n, M, dX, dY, alpha, beta, dZ, times_m)
        return out.cpu().numpy(), {"kernels": bh.kernel_stats(), "ms": bh.sddmm_ms}


# ---------------------------------------------------------------- the product with its reductions
def csr_spmv_dots_raw_device(bh, m, n, nnzA, d_valA, d_rowPtrA, d_colIndA, alpha, d_x, beta, d_y, d_z, d_w, dots):
    """bhs_csr_spmv_dots_device on caller-given arrays, the C arguments in order (include/bhsparse_hip.h, "relaxation and
    fused products"; d_valA, d_y with beta == 0 and d_w may be None; d_z may be d_y itself; dots: a numpy float64 array of
    two on the host, or None): the status code; sets bh.spmv_dots_ms."""
    if bh._h is None:
        return _lib.BHS_ERR_NOT_READY
    out = None if dots is None else dots.ctypes.data_as(C.POINTER(C.c_double))
    return bh._timed(bh._lib.bhs_csr_spmv_dots_device, "spmv_dots_ms", int(m), int(n), int(nnzA), _ptr(d_valA), _ptr(d_rowPtrA),
                     _ptr(d_colIndA), float(alpha), _ptr(d_x), float(beta), _ptr(d_y), _ptr(d_z), _ptr(d_w), out)


def csr_spmv_dots_device(bh, m, n, A, x, alpha=1.0, beta=0.0, y=None, w=None):
    """z = alpha A x + beta y out of place with the reductions of the stored z, in one call: A = (rowPtr, colInd, val or
    None), x (n values), y (m values; None with beta == 0) and w (m values or None; may be x itself when m == n) torch
    tensors on the handle's GPU.  Returns (z, zz, wz): z made here, zz = sum z_i^2 and wz = sum w_i z_i as Python floats
    (wz None without w).  r = b - A x with ||r||^2 is alpha = -1, beta = 1, y = b; q = A p with <p, q> is w = p.  Raises
    BhsparseError on failure."""
    import torch
    Ap, Aj, Ax = A
    z = _alloc(m, x.dtype, x.device)[:m]
    dots = np.zeros(2, np.float64)
    torch.cuda.synchronize()                           # the library works on its own stream (see facade.initData_device)
    _check(csr_spmv_dots_raw_device(bh, m, n, Aj.numel(), Ax, Ap, Aj, alpha, x, beta, y, z, w, dots), "bhs_csr_spmv_dots_device")
    return z, float(dots[0]), (None if w is None else float(dots[1]))


# ---------------------------------------------------------------- over a semiring, with mask and accumulate
def _semiring(semiring):
    """a BHS_SR_* constant from a name of _lib.SEMIRINGS or from the constant itself"""
    return _lib.SEMIRINGS[semiring] if isinstance(semiring, str) else int(semiring)


def semiring_identity(semiring):
    """the (+)-identity of a semiring (include/bhsparse_hip.h, "semiring multiply"): what a row without entries gives"""
    inf = float("inf")
    return (0.0, inf, -inf, -inf, inf, -inf, 0.0, 0.0)[_semiring(semiring)]


def _flags(accumulate, complement):
    return (_lib.BHS_MV_ACCUM if accumulate else 0) | (_lib.BHS_MV_MASK_COMPLEMENT if complement else 0)


def _semiring_call(bh, fn, *args):
    """fn(handle, *args, changed, ms): the status code; sets bh.spmv_ms and bh.spmv_changed on success"""
    changed, ms = C.c_longlong(0), C.c_double(0)
    err = fn(bh._h, *args, C.byref(changed), C.byref(ms))
    if err == _lib.BHS_SUCCESS:
        bh.spmv_ms = float(ms.value)
        bh.spmv_changed = int(changed.value)
    return err


def csr_spmv_semiring_raw_device(bh, semiring, m, n, nnzA, d_valA, d_rowPtrA, d_colIndA, d_x, flags, d_mask, d_y):
    """bhs_csr_spmv_semiring_device on caller-given arrays (d_valA may be None: every entry counts as 1; d_mask may be None:
    everything is selected; flags: BHS_MV_ACCUM | BHS_MV_MASK_COMPLEMENT): the status code; sets bh.spmv_ms and
    bh.spmv_changed."""
    if bh._h is None:
        return _lib.BHS_ERR_NOT_READY
    return _semiring_call(bh, bh._lib.bhs_csr_spmv_semiring_device, _semiring(semiring), int(m), int(n), int(nnzA), _ptr(d_valA),
                          _ptr(d_rowPtrA), _ptr(d_colIndA), _ptr(d_x), int(flags), _ptr(d_mask), _ptr(d_y))


def csr_spmm_semiring_raw_device(bh, semiring, m, n, nnzA, d_valA, d_rowPtrA, d_colIndA, k, d_X, ldX, flags, d_M, ldM, d_Y, ldY):
    """bhs_csr_spmm_semiring_device on caller-given arrays (X: n x k, M and Y: m x k, row-major with leading dimensions ldX,
    ldM, ldY): the status code; sets bh.spmv_ms and bh.spmv_changed."""
    if bh._h is None:
        return _lib.BHS_ERR_NOT_READY
    return _semiring_call(bh, bh._lib.bhs_csr_spmm_semiring_device, _semiring(semiring), int(m), int(n), int(nnzA), _ptr(d_valA),
                          _ptr(d_rowPtrA), _ptr(d_colIndA), int(k), _ptr(d_X), int(ldX), int(flags), _ptr(d_M), int(ldM),
                          _ptr(d_Y), int(ldY))


def csr_spmm_semiring_device(bh, semiring, m, n, A, X, Y=None, mask=None, accumulate=False, complement=False):
    """Y<mask> (+)= A (+).(x) X on device arrays: A = (rowPtr, colInd, val or None) torch tensors on the handle's GPU; X
    (n x k), mask (m x k or None) and Y (m x k) torch tensors there whose rows are contiguous (stride(0) is the leading
    dimension); 1-D tensors are taken as k = 1.  semiring: a name of _lib.SEMIRINGS or a BHS_SR_* constant.  Without
    `accumulate` Y is never read; a Y made here (None) is filled with nothing, so the elements the mask does not select
    hold whatever the allocation held.  Returns (Y, changed) -- Y in the shape of X's kind (1-D for a 1-D X); raises
    BhsparseError on failure."""
    import torch
    Ap, Aj, Ax = A
    flat = X.dim() == 1
    as2d = lambda T: T if T is None or T.dim() != 1 else T.unsqueeze(1)   # noqa: E731
    X2, M2, Y2 = as2d(X), as2d(mask), as2d(Y)
    k = X2.shape[1] if X2.dim() == 2 else 0
    if Y2 is None and k:
        Y2 = _alloc(m * k, X.dtype, X.device)[:m * k].view(m, k)
    for name, T, rows in (("X", X2, n), ("mask", M2, m), ("Y", Y2, m)):
        if name == "mask" and T is None:
            continue
        if not k or T.dim() != 2 or tuple(T.shape) != (rows, k) or (k > 1 and T.stride(1) != 1):
            raise ValueError("%s is a row-major %d x k tensor, k >= 1" % (name, rows))
    ld = lambda T: max(int(T.stride(0)), k) if T.shape[0] > 1 else k   # noqa: E731  (one row or none: any ld will do)
    torch.cuda.synchronize()                           # the library works on its own stream (see facade.initData_device)
    _check(csr_spmm_semiring_raw_device(bh, semiring, m, n, Aj.numel(), Ax, Ap, Aj, k, X2, ld(X2), _flags(accumulate, complement),
                                        M2, ld(M2) if M2 is not None else k, Y2, ld(Y2)), "bhs_csr_spmm_semiring_device")
    out = Y if Y is not None else (Y2[:, 0] if flat else Y2)
    return out, bh.spmv_changed


# ---------------------------------------------------------------- the push direction: a sparse frontier
def csr_push_semiring_raw_device(bh, semiring, m, n, nnzG, d_valG, d_rowPtrG, d_colIndG, nf, d_fidx, k, d_F, ldF, flags, d_M, ldM,
                                 d_Y, ldY, d_next, want_changed=True):
    """bhs_csr_push_semiring_device on caller-given arrays, the C arguments in order (d_valG, d_M and d_next may be None;
    flags: BHS_MV_MASK_COMPLEMENT or 0): the status code; sets bh.spmv_ms, bh.spmv_changed and bh.push_next (the length of
    the list in d_next) on success.  want_changed False passes a NULL changed_out (bh.spmv_changed is then 0)."""
    if bh._h is None:
        return _lib.BHS_ERR_NOT_READY
    changed, count, ms = C.c_longlong(0), C.c_int(0), C.c_double(0)
    err = bh._lib.bhs_csr_push_semiring_device(bh._h, _semiring(semiring), int(m), int(n), int(nnzG), _ptr(d_valG), _ptr(d_rowPtrG),
                                               _ptr(d_colIndG), int(nf), _ptr(d_fidx), int(k), _ptr(d_F), int(ldF), int(flags),
                                               _ptr(d_M), int(ldM), _ptr(d_Y), int(ldY), _ptr(d_next), C.byref(count),
                                               C.byref(changed) if want_changed else None, C.byref(ms))
    if err == _lib.BHS_SUCCESS:
        bh.spmv_ms = float(ms.value)
        bh.spmv_changed = int(changed.value)
        bh.push_next = int(count.value)
    return err


def csr_push_semiring_device(bh, semiring, m, n, G, fidx, F, Y, mask=None, complement=False, want_list=True):
    """Y<mask> (+)= F (+).(x) G(fidx, :) on device arrays, the push direction: G = (rowPtr, colInd, val or None), the m x n
    CSR of OUT-edges (row j lists the vertices j pushes to: the transpose of the pull calls' A) as torch tensors on the
    handle's GPU; fidx an int32 tensor of nf rows of G; F (nf x k), mask (n x k or None) and Y (n x k, updated in place: the
    call always accumulates) tensors there whose rows are contiguous (stride(0) is the leading dimension); 1-D tensors are
    taken as k = 1.  semiring: any but plus_times.  Returns (Y, changed, next_idx): the number of elements of Y that
    changed, and the rows of Y that hold one -- ascending, an int32 view (of the count's length) of a buffer made here; None
    without want_list.  Raises BhsparseError on failure."""
    import torch
    Gp, Gj, Gx = G
    as2d = lambda T: T if T is None or T.dim() != 1 else T.unsqueeze(1)   # noqa: E731
    F2, M2, Y2 = as2d(F), as2d(mask), as2d(Y)
    nf = int(fidx.numel())
    k = Y2.shape[1] if Y2.dim() == 2 else 0
    for name, T, rows in (("F", F2, nf), ("mask", M2, n), ("Y", Y2, n)):
        if name == "mask" and T is None:
            continue
        if not k or T.dim() != 2 or tuple(T.shape) != (rows, k) or (k > 1 and T.stride(1) != 1):
            raise ValueError("%s is a row-major %d x k tensor, k >= 1" % (name, rows))
    if fidx.dtype != torch.int32 or fidx.dim() != 1 or not fidx.is_contiguous():
        raise ValueError("fidx is a contiguous int32 vector")
    ld = lambda T: max(int(T.stride(0)), k) if T.shape[0] > 1 else k   # noqa: E731  (one row or none: any ld will do)
    nxt = torch.empty(max(n, 1), dtype=torch.int32, device=Y.device) if want_list else None
    torch.cuda.synchronize()                           # the library works on its own stream (see facade.initData_device)
    _check(csr_push_semiring_raw_device(bh, semiring, m, n, Gj.numel(), Gx, Gp, Gj, nf, fidx, k, F2, ld(F2),
                                        _flags(False, complement), M2, ld(M2) if M2 is not None else k, Y2, ld(Y2), nxt),
           "bhs_csr_push_semiring_device")
    return Y, bh.spmv_changed, (nxt[:bh.push_next] if want_list else None)


def spmm_semiring_csr(semiring, m, n, Ap, Aj, Ax, X, Y=None, mask=None, accumulate=False, complement=False,
                      value_dtype=np.float64, device=0):
    """Convenience: Y<mask> (+)= A (+).(x) X once on host arrays (A: m x n CSR, Ax may be None; X: n x k or n values; mask
    and Y: m x k or None -- a Y of None starts from the (+)-identity), staged as torch tensors on the handle's device.
    Returns (Y value_dtype[m, k], info) with info["kernels"], info["ms"], info["changed"].  Needs no multiply data."""
    A = _device_csr(Ap, Aj, Ax, value_dtype, device)
    dX = _upload(np.asarray(X).reshape(n, -1), value_dtype, device)
    k = dX.shape[1]
    Y0 = np.full((m, k), semiring_identity(semiring)) if Y is None else np.asarray(Y).reshape(m, k)
    dY = _upload(Y0, value_dtype, device)
    dM = None if mask is None else _upload(np.asarray(mask).reshape(m, k), value_dtype, device)
    with _handle(value_dtype, device, None) as bh:
        out, changed = csr_spmm_semiring_device(bh, semiring, m, n, A, dX, dY, dM, accumulate, complement)
        return out.cpu().numpy(), {"kernels": bh.kernel_stats(), "ms": bh.spmv_ms, "changed": changed}
