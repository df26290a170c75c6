"""Python mirror of the reference's `bhsparse` facade class
(SpGEMM_cuda/bhsparse.h:17-33): same method names, argument order, `int`
return codes (0 == BHSPARSE_SUCCESS, common.h:26) and call sequence

    initPlatform -> initData -> [warmup x3] -> spgemm -> get_nnzC -> get_C
                 -> free_mem -> freePlatform            (main.cu:104-135)

so that the parity tests read like the reference's own driver.  Every method
is a thin call into the C-ABI of libbhsparse_hip.so; arrays are numpy buffers
(host entry, like the reference) or raw device pointers / torch tensors
(`initData_device`, used by the benchmark and the multi-GPU path).
"""
import contextlib
import ctypes as C
import time

import numpy as np

from . import _lib

BHSPARSE_SUCCESS = 0
NUM_PLATFORMS = 9          # common.h:33
BHSPARSE_CUDA = 1          # common.h:36  (accepted as an alias of the HIP backend)
BHSPARSE_OPENCL = 2        # common.h:37  (alias)
BHSPARSE_HIP = 3           # new slot; indices 3..8 are free in the reference


class BhsparseError(RuntimeError):
    def __init__(self, where, code):
        self.code = int(code)
        super().__init__("%s failed: %d (%s)" % (where, code, _lib.strerror(code)))


def _ptr(a):
    if a is None:
        return None
    if isinstance(a, np.ndarray):
        return a.ctypes.data_as(C.c_void_p)
    if isinstance(a, int):
        return C.c_void_p(a)
    if hasattr(a, "data_ptr"):          # torch tensor (device or host)
        return C.c_void_p(a.data_ptr())
    raise TypeError("unsupported buffer type %r" % type(a))


def _sync(*arrays):
    """The library works on its own stream (see initData_device): before it reads torch tensors of the GPU, wait for the
    kernels torch has queued on them.  Host arrays and raw addresses need no wait."""
    if any(hasattr(t, "is_cuda") and t.is_cuda for t in arrays):
        import torch
        torch.cuda.synchronize()


def _alloc(n, dtype, device):
    """Room for n entries as a torch tensor, never a zero-size allocation (its data pointer would be null): the caller
    slices [:n]."""
    import torch
    return torch.empty(max(n, 1), dtype=dtype, device=device)


def _head(a, n):
    return None if a is None else a[:n]


def _check(err, where):
    if err != BHSPARSE_SUCCESS:
        raise BhsparseError(where, err)


class bhsparse(object):
    """index_type = int32, value_type = float64 (common.h:30-31), or float32 with
    `bhsparse(value_dtype=np.float32)` (libbhsparse_hip_f32.so, the reference's float build)."""

    def __init__(self, value_dtype=np.float64):
        self._vdt = np.dtype(value_dtype)
        if self._vdt not in (np.dtype(np.float64), np.dtype(np.float32)):
            raise ValueError("value_type is double or float")
        self._h = None
        self._lib = None
        self._m = 0
        self._rowptrC = None
        self._keep = None
        self.nnzCt = 0
        self.nnzC = 0
        self.stage_ms = [0.0] * 4
        self.time_ms = 0.0
        self.masked_ms = 0.0
        self.add_ms = 0.0
        self.select_ms = 0.0
        self.transpose_ms = 0.0
        self.extract_ms = 0.0
        self.reduce_ms = 0.0
        self.scale_ms = 0.0
        self.spmv_ms = 0.0
        self.spmv_dots_ms = 0.0
        self.relax_ms = 0.0
        self.spmv_changed = 0
        self.push_next = 0
        self.semiring_ms = 0.0
        self.multiply_ms = 0.0
        self.quiet = True

    # -- bhsparse.h:91-125 -------------------------------------------------
    def initPlatform(self, spgemm_platform, device=0):
        plats = list(spgemm_platform)
        if not any(plats[i] for i in (BHSPARSE_CUDA, BHSPARSE_OPENCL, BHSPARSE_HIP) if i < len(plats)):
            return _lib.BHS_ERR_INVALID_ARG
        self._lib = _lib.load(f32=self._vdt == np.dtype(np.float32))   # raises if missing: no fallback
        h = C.c_void_p()
        dev = C.c_int(int(device))
        err = self._lib.bhs_create(C.byref(h), 1, C.byref(dev))
        if err != BHSPARSE_SUCCESS:
            return err
        self._h = h
        # this mirror reports per-kernel times (kernel_stats()): tests and bench.py read them; C callers leave it off
        self._lib.bhs_set_option(self._h, b"kernel_stats", 1)
        if not self.quiet:
            self._lib.bhs_set_verbose(self._h, 1)
        return BHSPARSE_SUCCESS

    # -- bhsparse.h:180-258 ------------------------------------------------
    def initData(self, m, k, n, nnzA, csrValA, csrRowPtrA, csrColIndA,
                 nnzB, csrValB, csrRowPtrB, csrColIndB, csrRowPtrC, use_host_mem=False):
        """Host buffers (numpy), as the reference.  csrRowPtrC: caller-allocated
        int32[m+1], filled by spgemm().  `use_host_mem` mirrors the OpenCL
        variant's trailing flag (SpGEMM_opencl/bhsparse.h:44-47) and is ignored."""
        if self._h is None:
            return _lib.BHS_ERR_NOT_READY
        for a, dt in ((csrValA, self._vdt), (csrRowPtrA, np.int32), (csrColIndA, np.int32),
                      (csrValB, self._vdt), (csrRowPtrB, np.int32), (csrColIndB, np.int32)):
            if not (isinstance(a, np.ndarray) and a.dtype == dt and a.flags.c_contiguous):
                return _lib.BHS_ERR_INVALID_ARG
        if csrRowPtrC is not None and not (isinstance(csrRowPtrC, np.ndarray) and
                                           csrRowPtrC.dtype == np.int32 and csrRowPtrC.size >= m + 1):
            return _lib.BHS_ERR_INVALID_ARG
        self._m = m
        self._rowptrC = csrRowPtrC
        return self._lib.bhs_set_data(self._h, m, k, n, nnzA, _ptr(csrValA), _ptr(csrRowPtrA), _ptr(csrColIndA),
                                      nnzB, _ptr(csrValB), _ptr(csrRowPtrB), _ptr(csrColIndB))

    def initData_device(self, m, k, n, nnzA, d_valA, d_rowPtrA, d_colIndA,
                        nnzB, d_valB, d_rowPtrB, d_colIndB):
        """Device-resident inputs (torch tensors on this handle's GPU, or raw
        device addresses).  Borrowed until free_mem()."""
        if self._h is None:
            return _lib.BHS_ERR_NOT_READY
        self._m = m
        self._rowptrC = None
        self._keep = (d_valA, d_rowPtrA, d_colIndA, d_valB, d_rowPtrB, d_colIndB)
        # The library reads these arrays on ITS stream, starting inside this call (row-length and sortedness
        # scans).  torch tensors may still be being written by kernels queued on torch's stream: wait for them.
        # (Without this a multiply could read half-written row pointers: observed as a memory fault or a hang
        # when freshly generated inputs landed in recycled memory.)
        if any(hasattr(t, "is_cuda") and t.is_cuda for t in self._keep):
            import torch
            torch.cuda.synchronize(self._keep[1].device if hasattr(self._keep[1], "device") else None)
        return self._lib.bhs_set_data_device(self._h, m, k, n, nnzA, _ptr(d_valA), _ptr(d_rowPtrA),
                                             _ptr(d_colIndA), nnzB, _ptr(d_valB), _ptr(d_rowPtrB),
                                             _ptr(d_colIndB))

    # -- bhsparse.h:341-363 ------------------------------------------------
    def warmup(self):
        if self._h is None:
            return _lib.BHS_ERR_NOT_READY
        return self._lib.bhs_warmup(self._h)

    # -- bhsparse.h:260-295 ------------------------------------------------
    def spgemm(self):
        if self._h is None:
            return _lib.BHS_ERR_NOT_READY
        import time
        nnzCt, nnzC = C.c_int64(0), C.c_int(0)
        st = (C.c_double * 4)()
        t0 = time.perf_counter()
        err = self._lib.bhs_spgemm(self._h, _ptr(self._rowptrC), C.byref(nnzCt), C.byref(nnzC), st)
        self.time_ms = (time.perf_counter() - t0) * 1e3
        if err != BHSPARSE_SUCCESS:
            if not self.quiet:
                print("spgemm error = %d" % err)
            return err
        self.nnzCt, self.nnzC, self.stage_ms = int(nnzCt.value), int(nnzC.value), list(st)
        if not self.quiet:
            # bhsparse.h:287-289, tag changed from [ CUDA ] to [ HIP ]
            print("[ HIP ] SpGEMM time: %g ms. Gflops = %g" %
                  (self.time_ms, 2.0 * self.nnzCt / (self.time_ms * 1.0e6)))
        return BHSPARSE_SUCCESS

    # -- extension (not in the reference): the masked multiply C<M> = A·B (bhs_spgemm_masked, include/bhsparse_hip.h)
    def _masked_call(self, fn, semiring, rowPtrM, colIndM, nnzM, valC):
        """One of the four masked entries (host or device arrays, with or without a leading semiring): the status code;
        sets nnzCt and masked_ms / semiring_ms on success."""
        nnzCt, ms = C.c_int64(0), C.c_double(0)
        lead = () if semiring is None else (semiring,)
        err = fn(self._h, *lead, rowPtrM, colIndM, nnzM, valC, C.byref(nnzCt), C.byref(ms))
        if err == BHSPARSE_SUCCESS:
            self.nnzCt = int(nnzCt.value)
            setattr(self, "masked_ms" if semiring is None else "semiring_ms", float(ms.value))
        return err

    def _masked_host(self, semiring, rowPtrM, colIndM, valC):
        where = "bhs_spgemm_masked" if semiring is None else "bhs_spgemm_semiring_masked"
        if self._h is None:
            raise BhsparseError(where, _lib.BHS_ERR_NOT_READY)
        rowPtrM = np.ascontiguousarray(rowPtrM, np.int32)
        colIndM = np.ascontiguousarray(colIndM, np.int32)
        if rowPtrM.size < self._m + 1:
            raise BhsparseError(where, _lib.BHS_ERR_INVALID_ARG)
        nnzM = colIndM.size
        if valC is None:
            valC = np.empty(nnzM, self._vdt)
        elif not (isinstance(valC, np.ndarray) and valC.dtype == self._vdt and valC.size >= nnzM and valC.flags.c_contiguous):
            raise BhsparseError(where, _lib.BHS_ERR_INVALID_ARG)
        fn = self._lib.bhs_spgemm_masked if semiring is None else self._lib.bhs_spgemm_semiring_masked
        _check(self._masked_call(fn, semiring, _ptr(rowPtrM), _ptr(colIndM) if nnzM else None, nnzM,
                                 _ptr(valC) if nnzM else None), where)
        return valC

    def _masked_device(self, semiring, d_rowPtrM, d_colIndM, nnzM, d_valC):
        if self._h is None:
            return _lib.BHS_ERR_NOT_READY
        _sync(d_rowPtrM, d_colIndM, d_valC)
        fn = self._lib.bhs_spgemm_masked_device if semiring is None else self._lib.bhs_spgemm_semiring_masked_device
        return self._masked_call(fn, semiring, _ptr(d_rowPtrM), _ptr(d_colIndM), int(nnzM), _ptr(d_valC))

    def spgemm_masked(self, rowPtrM, colIndM, valC=None):
        """valC[p] = (A·B)(i, colIndM[p]) for every entry p of row i of the pattern M (numpy int32 CSR, m x n, rows strictly
        ascending), 0 where no product lands.  Returns valC (allocated when None).  Raises BhsparseError on failure (an
        invalid M: code BHS_ERR_INVALID_ARG, valC untouched).  Sets nnzCt (products of A·B) and masked_ms (device time)."""
        return self._masked_host(None, rowPtrM, colIndM, valC)

    def spgemm_masked_device(self, d_rowPtrM, d_colIndM, nnzM, d_valC):
        """The same on device arrays (torch tensors on this handle's GPU, or raw device addresses); valC is written in
        place.  Returns the status code (0 on success) and sets nnzCt / masked_ms."""
        return self._masked_device(None, d_rowPtrM, d_colIndM, nnzM, d_valC)

    def _multiply(self, fn, lead, ms1, ms0=None, wall=False):
        """A multiply-then-post-operation entry of the C-ABI, fn(handle, *lead, nnzCt, nnzC, ms[2]): the status code.  On
        success sets nnzCt, nnzC, the attribute `ms1` from ms[1] (device time of the post-operation) and, where named,
        `ms0` from ms[0] (device time of the multiply).  wall: time_ms is taken around the call, as spgemm() does."""
        nnzCt, nnzC = C.c_int64(0), C.c_int(0)
        ms = (C.c_double * 2)()
        t0 = time.perf_counter()
        err = fn(self._h, *lead, C.byref(nnzCt), C.byref(nnzC), ms)
        if wall:
            self.time_ms = (time.perf_counter() - t0) * 1e3
        if err == BHSPARSE_SUCCESS:
            self.nnzCt, self.nnzC = int(nnzCt.value), int(nnzC.value)
            setattr(self, ms1, float(ms[1]))
            if ms0 is not None:
                setattr(self, ms0, float(ms[0]))
        return err

    def _timed(self, fn, ms_attr, *args):
        """A side operation of the C-ABI, fn(handle, *args, ms): the status code; sets `ms_attr` (device time) on success."""
        ms = C.c_double(0)
        err = fn(self._h, *args, C.byref(ms))
        if err == BHSPARSE_SUCCESS:
            setattr(self, ms_attr, float(ms.value))
        return err

    def _counted(self, name, family, count, turns, *args):
        """A graph call of the C-ABI, `name`(handle, *args, count, turns, ms): the status code, BHS_ERR_NOT_READY without
        a platform; sets <family>_ms (device time), <family>_<count> and <family>_<turns> (rounds or passes) on success."""
        if self._h is None:
            return _lib.BHS_ERR_NOT_READY
        n, t, ms = C.c_int(0), C.c_int(0), C.c_double(0)
        err = getattr(self._lib, name)(self._h, *args, C.byref(n), C.byref(t), C.byref(ms))
        if err == BHSPARSE_SUCCESS:
            setattr(self, family + "_ms", float(ms.value))
            setattr(self, family + "_" + count, int(n.value))
            setattr(self, family + "_" + turns, int(t.value))
        return err

    def _symbolic_numeric(self, family, rows, device, vdtype, perm, symbolic, numeric):
        """The two calls of `family` (add, select, extract) on arrays made here: symbolic(Zp) -> (status, nnzZ, ...) fills
        the row pointer of rows + 1 ints, then numeric(nnzZ, Zp, Zj, Zx, pm) -> status fills arrays of nnzZ entries (Zx only
        for a `vdtype`, pm only for `perm`).  Returns (Zp, Zj, Zx, pm) cut to nnzZ entries, followed by whatever else
        symbolic returned; raises BhsparseError naming the call that failed."""
        import torch
        torch.cuda.synchronize()                           # the library works on its own stream (see initData_device)
        Zp = torch.empty(rows + 1, dtype=torch.int32, device=device)
        err, nnzZ, *rest = symbolic(Zp)
        _check(err, family + "_symbolic_device")
        Zj = _alloc(nnzZ, torch.int32, device)
        Zx = None if vdtype is None else _alloc(nnzZ, vdtype, device)
        pm = _alloc(nnzZ, torch.int32, device) if perm else None
        torch.cuda.synchronize()
        _check(numeric(nnzZ, Zp, Zj, Zx, pm), family + "_numeric_device")
        return (Zp, Zj[:nnzZ], _head(Zx, nnzZ), _head(pm, nnzZ)) + tuple(rest)

    # -- extension (not in the reference): C = alpha A·B + beta D and the sparse add (include/bhsparse_hip.h, "sparse add")
    def spgemm_add(self, alpha, beta, rowPtrD, colIndD, valD):
        """C = alpha A·B + beta D on the data of initData; D: host numpy CSR, m x n, rows strictly ascending.  Returns the
        status code like spgemm() (an invalid D: BHS_ERR_INVALID_ARG, the last C untouched); fills the csrRowPtrC given to
        initData and sets nnzCt (products of A·B), nnzC (entries of the sum), time_ms and add_ms (device time of the add).
        get_nnzC / get_C / get_rowptrC / get_C_device then return this C."""
        if self._h is None:
            return _lib.BHS_ERR_NOT_READY
        rowPtrD = np.ascontiguousarray(rowPtrD, np.int32)
        colIndD = np.ascontiguousarray(colIndD, np.int32)
        valD = np.ascontiguousarray(valD, self._vdt)
        if rowPtrD.size < self._m + 1 or valD.size != colIndD.size:
            return _lib.BHS_ERR_INVALID_ARG
        nnzD = colIndD.size
        return self._multiply(self._lib.bhs_spgemm_add, (float(alpha), float(beta), nnzD, _ptr(valD) if nnzD else None,
                                                         _ptr(rowPtrD), _ptr(colIndD) if nnzD else None,
                                                         _ptr(self._rowptrC)), "add_ms", wall=True)

    def spgemm_add_device(self, alpha, beta, nnzD, d_valD, d_rowPtrD, d_colIndD):
        """The same with D on the device (torch tensors on this handle's GPU, or raw device addresses)."""
        if self._h is None:
            return _lib.BHS_ERR_NOT_READY
        _sync(d_valD, d_rowPtrD, d_colIndD)
        return self._multiply(self._lib.bhs_spgemm_add_device, (float(alpha), float(beta), int(nnzD), _ptr(d_valD),
                                                                _ptr(d_rowPtrD), _ptr(d_colIndD), _ptr(self._rowptrC)), "add_ms")

    def csr_add_symbolic_device(self, m, n, nnzX, d_rowPtrX, d_colIndX, nnzY, d_rowPtrY, d_colIndY, d_rowPtrZ):
        """bhs_csr_add_symbolic_device: (status, nnz(Z), y_inside_x); d_rowPtrZ (m+1 ints on the device) is written."""
        nnzZ, inside = C.c_int(0), C.c_int(0)
        err = self._lib.bhs_csr_add_symbolic_device(self._h, int(m), int(n), int(nnzX), _ptr(d_rowPtrX), _ptr(d_colIndX),
                                                    int(nnzY), _ptr(d_rowPtrY), _ptr(d_colIndY), _ptr(d_rowPtrZ),
                                                    C.byref(nnzZ), C.byref(inside))
        return err, int(nnzZ.value), int(inside.value)

    def csr_add_numeric_device(self, m, n, alpha, nnzX, d_valX, d_rowPtrX, d_colIndX, beta, nnzY, d_valY, d_rowPtrY, d_colIndY,
                               d_rowPtrZ, d_colIndZ, d_valZ):
        """bhs_csr_add_numeric_device: the status code; sets add_ms."""
        return self._timed(self._lib.bhs_csr_add_numeric_device, "add_ms", int(m), int(n), float(alpha), int(nnzX),
                           _ptr(d_valX), _ptr(d_rowPtrX), _ptr(d_colIndX), float(beta), int(nnzY), _ptr(d_valY),
                           _ptr(d_rowPtrY), _ptr(d_colIndY), _ptr(d_rowPtrZ), _ptr(d_colIndZ), _ptr(d_valZ))

    def csr_add_device(self, m, n, alpha, X, beta, Y):
        """Z = alpha X + beta Y on device arrays: X, Y = (rowPtr, colInd, val) torch tensors on this handle's GPU.  Returns
        (rowPtrZ, colIndZ, valZ, y_inside_x) as torch tensors; raises BhsparseError on failure."""
        Xp, Xj, Xx = X
        Yp, Yj, Yx = Y
        Zp, Zj, Zx, _, inside = self._symbolic_numeric(
            "bhs_csr_add", m, Xp.device, Xx.dtype, False,
            lambda Zp: self.csr_add_symbolic_device(m, n, Xj.numel(), Xp, Xj, Yj.numel(), Yp, Yj, Zp),
            lambda nnzZ, Zp, Zj, Zx, pm: self.csr_add_numeric_device(m, n, alpha, Xj.numel(), Xx, Xp, Xj, beta, Yj.numel(), Yx,
                                                                     Yp, Yj, Zp, Zj, Zx))
        return Zp, Zj, Zx, inside

    # -- extension (not in the reference): entry selection and the pruned multiply (include/bhsparse_hip.h, "entry selection")
    def spgemm_select(self, spec):
        """C = select(A·B) on the data of initData; spec: a select_spec(...) / _lib.Select.  Returns the status code like
        spgemm(); fills the csrRowPtrC given to initData and sets nnzCt (products of A·B), nnzC (entries after the
        selection), time_ms and select_ms (device time of the selection).  get_nnzC / get_C / get_rowptrC / get_C_device
        then return the selected C."""
        if self._h is None:
            return _lib.BHS_ERR_NOT_READY
        return self._multiply(self._lib.bhs_spgemm_select, (C.byref(spec), _ptr(self._rowptrC)), "select_ms", wall=True)

    def spgemm_select_device(self, spec, d_rowPtrC=None):
        """The same; d_rowPtrC (may be None): m+1 ints on the device that receive the selected C's row pointer."""
        if self._h is None:
            return _lib.BHS_ERR_NOT_READY
        return self._multiply(self._lib.bhs_spgemm_select_device, (C.byref(spec), _ptr(d_rowPtrC)), "select_ms")

    def csr_select_symbolic_device(self, m, n, nnzX, d_valX, d_rowPtrX, d_colIndX, spec, d_rowPtrZ):
        """bhs_csr_select_symbolic_device: (status, nnz(Z)); d_rowPtrZ (m+1 ints on the device) is written."""
        nnzZ = C.c_int(0)
        err = self._lib.bhs_csr_select_symbolic_device(self._h, int(m), int(n), int(nnzX), _ptr(d_valX), _ptr(d_rowPtrX),
                                                       _ptr(d_colIndX), C.byref(spec), _ptr(d_rowPtrZ), C.byref(nnzZ))
        return err, int(nnzZ.value)

    def csr_select_numeric_device(self, m, n, nnzX, d_valX, d_rowPtrX, d_colIndX, spec, d_rowPtrZ, d_colIndZ, d_valZ):
        """bhs_csr_select_numeric_device: the status code; sets select_ms."""
        return self._timed(self._lib.bhs_csr_select_numeric_device, "select_ms", int(m), int(n), int(nnzX), _ptr(d_valX),
                           _ptr(d_rowPtrX), _ptr(d_colIndX), C.byref(spec), _ptr(d_rowPtrZ), _ptr(d_colIndZ), _ptr(d_valZ))

    def csr_select_device(self, m, n, X, spec, values=True):
        """Z = select(X) on device arrays: X = (rowPtr, colInd, val) torch tensors on this handle's GPU (val may be None for
        a rule without value flags).  Returns (rowPtrZ, colIndZ, valZ) as torch tensors (valZ None when values is false or
        X has none); raises BhsparseError on failure."""
        Xp, Xj, Xx = X
        return self._symbolic_numeric(
            "bhs_csr_select", m, Xp.device, Xx.dtype if (values and Xx is not None) else None, False,
            lambda Zp: self.csr_select_symbolic_device(m, n, Xj.numel(), Xx, Xp, Xj, spec, Zp),
            lambda nnzZ, Zp, Zj, Zx, pm: self.csr_select_numeric_device(m, n, Xj.numel(), Xx, Xp, Xj, spec, Zp, Zj, Zx))[:3]

    # -- extension (not in the reference): the stable transpose and its pattern reuse (include/bhsparse_hip.h, "transpose")
    def csr_transpose_raw_device(self, m, n, nnzX, d_valX, d_rowPtrX, d_colIndX, d_rowPtrT, d_colIndT, d_valT, d_perm):
        """bhs_csr_transpose_device: the status code; sets transpose_ms."""
        if self._h is None:
            return _lib.BHS_ERR_NOT_READY
        return self._timed(self._lib.bhs_csr_transpose_device, "transpose_ms", int(m), int(n), int(nnzX), _ptr(d_valX),
                           _ptr(d_rowPtrX), _ptr(d_colIndX), _ptr(d_rowPtrT), _ptr(d_colIndT), _ptr(d_valT), _ptr(d_perm))

    def csr_transpose_device(self, m, n, X, values=True, perm=False):
        """T = X^T on device arrays: X = (rowPtr, colInd, val) torch tensors on this handle's GPU (val may be None: the
        pattern alone).  Returns (rowPtrT, colIndT, valT, perm) as torch tensors (valT None when values is false or X has
        none, perm None unless asked for); raises BhsparseError on failure."""
        import torch
        torch.cuda.synchronize()                           # the library works on its own stream (see initData_device)
        Xp, Xj, Xx = X
        nnz = Xj.numel()
        Tp = torch.empty(n + 1, dtype=torch.int32, device=Xp.device)
        Tj = _alloc(nnz, torch.int32, Xp.device)
        Tx = _alloc(nnz, Xx.dtype, Xp.device) if (values and Xx is not None) else None
        pm = _alloc(nnz, torch.int32, Xp.device) if perm else None
        torch.cuda.synchronize()
        _check(self.csr_transpose_raw_device(m, n, nnz, Xx, Xp, Xj, Tp, Tj, Tx, pm), "bhs_csr_transpose_device")
        return Tp, Tj[:nnz], _head(Tx, nnz), _head(pm, nnz)

    def csr_transpose_values_device(self, d_valX, d_perm, d_valT=None):
        """valT[q] = valX[perm[q]] on torch tensors of this handle's GPU (bhs_csr_transpose_values_device): the values of a
        transpose whose pattern is known.  d_valT (made when None) is returned; sets transpose_ms; raises BhsparseError."""
        import torch
        nnz = d_perm.numel()
        if d_valT is None:
            d_valT = _alloc(nnz, d_valX.dtype, d_valX.device)[:nnz]
        torch.cuda.synchronize()
        ms = C.c_double(0)
        _check(self._lib.bhs_csr_transpose_values_device(self._h, int(nnz), _ptr(d_valX), _ptr(d_perm), _ptr(d_valT),
                                                         C.byref(ms)), "bhs_csr_transpose_values_device")
        self.transpose_ms = float(ms.value)
        return d_valT

    # -- extension (not in the reference): Z = X(rows, cols) (include/bhsparse_hip.h, "extract")
    @staticmethod
    def _index_list(a):
        """An index list for the C-ABI, where NULL means "all": an EMPTY torch tensor (whose data pointer is null) is stood in
        for by a one-element tensor, so that the call sees an empty list."""
        if a is not None and hasattr(a, "numel") and a.numel() == 0:
            return a.new_empty(1)
        return a

    def csr_extract_symbolic_device(self, m, n, nnzX, d_rowPtrX, d_colIndX, mI, d_rows, nJ, d_cols, d_rowPtrZ):
        """bhs_csr_extract_symbolic_device: (status, nnz(Z)); d_rowPtrZ (mI+1 ints on the device) is written."""
        if self._h is None:
            return _lib.BHS_ERR_NOT_READY, 0
        d_rows, d_cols = self._index_list(d_rows), self._index_list(d_cols)
        nnzZ = C.c_int(0)
        err = self._lib.bhs_csr_extract_symbolic_device(self._h, int(m), int(n), int(nnzX), _ptr(d_rowPtrX), _ptr(d_colIndX),
                                                        int(mI), _ptr(d_rows), int(nJ), _ptr(d_cols), _ptr(d_rowPtrZ),
                                                        C.byref(nnzZ))
        return err, int(nnzZ.value)

    def csr_extract_numeric_device(self, m, n, nnzX, d_valX, d_rowPtrX, d_colIndX, mI, d_rows, nJ, d_cols, nnzZ, d_rowPtrZ,
                                   d_colIndZ, d_valZ, d_perm):
        """bhs_csr_extract_numeric_device: the status code; sets extract_ms."""
        if self._h is None:
            return _lib.BHS_ERR_NOT_READY
        d_rows, d_cols = self._index_list(d_rows), self._index_list(d_cols)
        return self._timed(self._lib.bhs_csr_extract_numeric_device, "extract_ms", int(m), int(n), int(nnzX), _ptr(d_valX),
                           _ptr(d_rowPtrX), _ptr(d_colIndX), int(mI), _ptr(d_rows), int(nJ), _ptr(d_cols), int(nnzZ),
                           _ptr(d_rowPtrZ), _ptr(d_colIndZ), _ptr(d_valZ), _ptr(d_perm))

    def csr_extract_raw_device(self, m, n, nnzX, d_valX, d_rowPtrX, d_colIndX, mI, d_rows, nJ, d_cols, d_rowPtrZ, d_colIndZ,
                               d_valZ, d_perm):
        """Both calls on caller-given arrays: (status, nnz(Z)); the numeric call runs only where the symbolic one succeeds."""
        err, nnzZ = self.csr_extract_symbolic_device(m, n, nnzX, d_rowPtrX, d_colIndX, mI, d_rows, nJ, d_cols, d_rowPtrZ)
        if err != BHSPARSE_SUCCESS:
            return err, 0
        err = self.csr_extract_numeric_device(m, n, nnzX, d_valX, d_rowPtrX, d_colIndX, mI, d_rows, nJ, d_cols, nnzZ, d_rowPtrZ,
                                              d_colIndZ, d_valZ, d_perm)
        return err, nnzZ

    def csr_extract_device(self, m, n, X, rows=None, cols=None, values=True, perm=False):
        """Z = X(rows, cols) on device arrays: X = (rowPtr, colInd, val) torch tensors on this handle's GPU (val may be None:
        the pattern alone); rows / cols: int32 torch tensors there, or None for all of them in order.  Returns (rowPtrZ,
        colIndZ, valZ, perm) as torch tensors (valZ None when values is false or X has none, perm None unless asked for);
        raises BhsparseError on failure."""
        Xp, Xj, Xx = X
        nnzX = Xj.numel()
        mI = m if rows is None else rows.numel()
        nJ = n if cols is None else cols.numel()
        return self._symbolic_numeric(
            "bhs_csr_extract", mI, Xp.device, Xx.dtype if (values and Xx is not None) else None, perm,
            lambda Zp: self.csr_extract_symbolic_device(m, n, nnzX, Xp, Xj, mI, rows, nJ, cols, Zp),
            lambda nnzZ, Zp, Zj, Zx, pm: self.csr_extract_numeric_device(m, n, nnzX, Xx, Xp, Xj, mI, rows, nJ, cols, nnzZ, Zp,
                                                                         Zj, Zx, pm))

    # -- extension (not in the reference): reductions and the diagonal scaling (include/bhsparse_hip.h, "reduce / scale")
    def csr_reduce_raw_device(self, m, n, nnzX, d_valX, d_rowPtrX, d_colIndX, axis, op, flags, d_out):
        """bhs_csr_reduce_device on caller-given arrays: the status code; sets reduce_ms."""
        if self._h is None:
            return _lib.BHS_ERR_NOT_READY
        return self._timed(self._lib.bhs_csr_reduce_device, "reduce_ms", int(m), int(n), int(nnzX), _ptr(d_valX),
                           _ptr(d_rowPtrX), _ptr(d_colIndX), int(axis), int(op), int(flags), _ptr(d_out))

    def csr_scale_raw_device(self, m, n, nnzX, d_valX, d_rowPtrX, d_colIndX, alpha, d_left, d_right, flags, d_valZ):
        """bhs_csr_scale_device on caller-given arrays: the status code; sets scale_ms."""
        if self._h is None:
            return _lib.BHS_ERR_NOT_READY
        return self._timed(self._lib.bhs_csr_scale_device, "scale_ms", int(m), int(n), int(nnzX), _ptr(d_valX), _ptr(d_rowPtrX),
                           _ptr(d_colIndX), float(alpha), _ptr(d_left), _ptr(d_right), int(flags), _ptr(d_valZ))

    def csr_reduce_device(self, m, n, X, axis, op, offdiag=False):
        """reduce(X) along `axis` (_lib.BHS_AXIS_*) with `op` (_lib.BHS_RED_*) on device arrays: X = (rowPtr, colInd, val)
        torch tensors on this handle's GPU (val may be None: every entry counts as 1).  Returns a torch tensor of m, n, 1
        or min(m, n) values of this handle's value type; raises BhsparseError on failure."""
        import torch
        torch.cuda.synchronize()                           # the library works on its own stream (see initData_device)
        Xp, Xj, Xx = X
        count = {_lib.BHS_AXIS_ROWS: m, _lib.BHS_AXIS_COLS: n, _lib.BHS_AXIS_ALL: 1, _lib.BHS_AXIS_DIAG: min(m, n)}.get(axis, 1)
        tdt = torch.float32 if self._vdt == np.dtype(np.float32) else torch.float64
        out = _alloc(count, tdt, Xp.device)
        torch.cuda.synchronize()
        _check(self.csr_reduce_raw_device(m, n, Xj.numel(), Xx, Xp, Xj, axis, op, _lib.BHS_RED_OFFDIAG if offdiag else 0, out),
               "bhs_csr_reduce_device")
        return out[:count]

    def csr_scale_device(self, m, n, X, alpha=1.0, left=None, right=None, left_div=False, right_div=False, out=None):
        """valZ of Z = alpha diag(left) X diag(right) on X's pattern: X = (rowPtr, colInd, val) torch tensors on this
        handle's GPU, left / right torch tensors of m / n values there or None; *_div divides by the vector.  out: where
        the values go (X's val itself: in place); a new tensor by default.  Returns it; raises BhsparseError on failure."""
        import torch
        Xp, Xj, Xx = X
        if out is None:
            out = _alloc(Xx.numel(), Xx.dtype, Xx.device)[:Xx.numel()]
        torch.cuda.synchronize()
        flags = (_lib.BHS_SCALE_LEFT_DIV if left_div else 0) | (_lib.BHS_SCALE_RIGHT_DIV if right_div else 0)
        _check(self.csr_scale_raw_device(m, n, Xj.numel(), Xx, Xp, Xj, alpha, left, right, flags, out), "bhs_csr_scale_device")
        return out

    # -- extension (not in the reference): the multiply over a semiring (include/bhsparse_hip.h, "semiring multiply")
    def spgemm_semiring(self, semiring):
        """C = A (+).(x) B on the data of initData; semiring: a _lib.BHS_SR_* constant.  The ordinary multiply, then its C
        re-valued in place.  Returns the status code like spgemm(); fills the csrRowPtrC given to initData and sets nnzCt,
        nnzC, time_ms, multiply_ms (device time of the multiply) and semiring_ms (device time of the re-valuation).
        get_nnzC / get_C / get_rowptrC / get_C_device then return the semiring's values."""
        if self._h is None:
            return _lib.BHS_ERR_NOT_READY
        return self._multiply(self._lib.bhs_spgemm_semiring, (int(semiring), _ptr(self._rowptrC)), "semiring_ms",
                              ms0="multiply_ms", wall=True)

    def spgemm_semiring_masked(self, semiring, rowPtrM, colIndM, valC=None):
        """spgemm_masked over a semiring: valC[p] = the (+)-reduction of A(i,k) (x) B(k, colIndM[p]) for every entry p of row i
        of the pattern M, the (+)-identity where no product lands.  Returns valC (allocated when None); raises BhsparseError
        (an invalid M or an unknown semiring: code BHS_ERR_INVALID_ARG, valC untouched).  Sets nnzCt and semiring_ms."""
        return self._masked_host(int(semiring), rowPtrM, colIndM, valC)

    def spgemm_semiring_masked_device(self, semiring, d_rowPtrM, d_colIndM, nnzM, d_valC):
        """The same on device arrays (torch tensors on this handle's GPU, or raw device addresses); valC is written in
        place.  Returns the status code (0 on success) and sets nnzCt / semiring_ms."""
        return self._masked_device(int(semiring), d_rowPtrM, d_colIndM, nnzM, d_valC)

    def get_nnzC(self):
        if self._h is None:
            return 0
        v = C.c_int(0)
        err = self._lib.bhs_get_nnzC(self._h, C.byref(v))
        return int(v.value) if err == BHSPARSE_SUCCESS else 0

    # -- bhsparse_cuda.h:3006-3020 ------------------------------------------
    def get_C(self, csrColIndC, csrValC):
        if self._h is None:
            return _lib.BHS_ERR_NOT_READY
        nnz = self.get_nnzC()
        for a, dt in ((csrColIndC, np.int32), (csrValC, self._vdt)):
            if nnz and not (isinstance(a, np.ndarray) and a.dtype == dt and a.size >= nnz and
                            a.flags.c_contiguous):
                return _lib.BHS_ERR_INVALID_ARG
        err = self._lib.bhs_get_C(self._h, _ptr(csrColIndC), _ptr(csrValC))
        if err == BHSPARSE_SUCCESS and self._rowptrC is not None:
            err = self._lib.bhs_get_rowptrC(self._h, _ptr(self._rowptrC))   # reference re-copies rowPtrC here
        return err

    # -- the multiply in two halves (include/bhsparse_hip.h): multi-GPU callers place C themselves
    def spgemm_symbolic(self):
        nnzCt, nnzC = C.c_int64(0), C.c_int(0)
        err = self._lib.bhs_spgemm_symbolic(self._h, C.byref(nnzCt), C.byref(nnzC))
        if err == BHSPARSE_SUCCESS:
            self.nnzCt, self.nnzC = int(nnzCt.value), int(nnzC.value)
        return err

    def set_output_device(self, d_colIndC, d_valC, capacity):
        return self._lib.bhs_set_output_device(self._h, _ptr(d_colIndC), _ptr(d_valC), int(capacity))

    def spgemm_numeric(self, row_begin, row_end):
        return self._lib.bhs_spgemm_numeric(self._h, int(row_begin), int(row_end))

    def spgemm_finish(self):
        st = (C.c_double * 4)()
        err = self._lib.bhs_spgemm_finish(self._h, st)
        if err == BHSPARSE_SUCCESS:
            self.stage_ms = list(st)
        return err

    def get_C_device(self):
        """(rowPtrC, colIndC, valC) device addresses of the last result."""
        p = [C.c_void_p(), C.c_void_p(), C.c_void_p()]
        err = self._lib.bhs_get_C_device(self._h, C.byref(p[0]), C.byref(p[1]), C.byref(p[2]))
        if err != BHSPARSE_SUCCESS:
            raise BhsparseError("bhs_get_C_device", err)
        return tuple(int(x.value or 0) for x in p)

    def class_tables_device(self):
        """bhs_get_class_tables_device: (classC, classInfo, classRel) device addresses, slots, rel stride, usable."""
        p = [C.c_void_p(), C.c_void_p(), C.c_void_p()]
        slots, stride, usable = C.c_int(0), C.c_int(0), C.c_int(0)
        err = self._lib.bhs_get_class_tables_device(self._h, C.byref(p[0]), C.byref(p[1]), C.byref(p[2]), C.byref(slots),
                                                    C.byref(stride), C.byref(usable))
        if err != BHSPARSE_SUCCESS:
            raise BhsparseError("bhs_get_class_tables_device", err)
        return tuple(int(x.value or 0) for x in p) + (slots.value, stride.value, bool(usable.value))

    def expand_class_columns_device(self, n, row0, d_classC, d_classInfo, d_classRel, rel_stride, d_rowPtrC, d_colIndC, stream=0):
        """bhs_expand_class_columns_device: colIndC of n rows from their classes (asynchronous on `stream`)."""
        return self._lib.bhs_expand_class_columns_device(C.c_void_p(stream), n, row0, C.c_void_p(d_classC), C.c_void_p(d_classInfo),
                                                         C.c_void_p(d_classRel), rel_stride, C.c_void_p(d_rowPtrC), C.c_void_p(d_colIndC))

    def csr_sort_indices_device(self, n_row, d_rowPtr, d_colInd, d_val):
        """In-place, stable per-row sort by column of a device-resident CSR matrix
        (ref_spgemm::csr_sort_indices, SpGEMM_cuda/ref_spgemm.h:37-62, on the GPU)."""
        if self._h is None:
            return _lib.BHS_ERR_NOT_READY
        _sync(d_rowPtr, d_colInd, d_val)
        return self._lib.bhs_csr_sort_indices_device(self._h, n_row, _ptr(d_rowPtr), _ptr(d_colInd), _ptr(d_val))

    def get_rowptrC(self, out=None):
        out = np.empty(self._m + 1, np.int32) if out is None else out
        err = self._lib.bhs_get_rowptrC(self._h, _ptr(out))
        if err != BHSPARSE_SUCCESS:
            raise BhsparseError("bhs_get_rowptrC", err)
        return out

    def kernel_stats_raw(self, arr):
        """bhs_get_kernel_stats into a caller's (_lib.KernelStat * 64)(): the number of records (decode_kernel_stats reads
        them later -- a timed loop pays one C call per multiply, not a dozen dictionaries)"""
        return self._lib.bhs_get_kernel_stats(self._h, arr, 64)

    @staticmethod
    def decode_kernel_stats(arr, nrec):
        return [{"name": arr[i].name.decode(), "launches": arr[i].launches, "ms": arr[i].ms, "rows": arr[i].rows,
                 "products": arr[i].products, "nnz_out": arr[i].nnz_out, "nnzA_rows": arr[i].nnzA_rows}
                for i in range(min(nrec, 64))]

    def kernel_stats(self):
        arr = (_lib.KernelStat * 64)()
        return self.decode_kernel_stats(arr, self.kernel_stats_raw(arr))

    def set_option(self, key, value):
        return self._lib.bhs_set_option(self._h, key.encode(), int(value))

    def get_info(self, key):
        """bhs_get_info: what the library found out about the bound data set ("b_sorted", "max_row_a", "max_row_b")"""
        v = C.c_int64(0)
        err = self._lib.bhs_get_info(self._h, key.encode(), C.byref(v))
        if err:
            raise BhsparseError("get_info(%s)" % key, err)
        return v.value

    # -- bhsparse.h:151-178 / 127-149 ----------------------------------------
    def free_mem(self):
        if self._h is None:
            return _lib.BHS_ERR_NOT_READY
        self._keep = None
        return self._lib.bhs_free_data(self._h)

    def freePlatform(self):
        if self._h is None:
            return BHSPARSE_SUCCESS
        err = self._lib.bhs_destroy(self._h)
        self._h = None
        return err


@contextlib.contextmanager
def _handle(value_dtype, device, options):
    """A handle on `device` with `options` set, for one `with` block; always destroyed.  free_mem() is left to the block's
    success path (_free)."""
    plats = [False] * NUM_PLATFORMS
    plats[BHSPARSE_HIP] = True
    bh = bhsparse(value_dtype=value_dtype)
    _check(bh.initPlatform(plats, device=device), "initPlatform")
    try:
        for key, val in (options or {}).items():
            _check(bh.set_option(key, val), "set_option(%s)" % key)
        yield bh
    finally:
        bh.freePlatform()


def _bind(bh, m, k, n, Ap, Aj, Ax, Bp, Bj, Bx, Cp):
    """initData on host CSR arrays of any integer / float type (converted here); Cp: int32[m+1] for rowPtrC, or None."""
    Ap, Aj, Ax = np.ascontiguousarray(Ap, np.int32), np.ascontiguousarray(Aj, np.int32), np.ascontiguousarray(Ax, bh._vdt)
    Bp, Bj, Bx = np.ascontiguousarray(Bp, np.int32), np.ascontiguousarray(Bj, np.int32), np.ascontiguousarray(Bx, bh._vdt)
    _check(bh.initData(m, k, n, len(Aj), Ax, Ap, Aj, len(Bj), Bx, Bp, Bj, Cp), "initData")


def _fetch(bh):
    """(rowPtrC, colIndC, valC) of the last result as numpy arrays: the row pointer given to initData, or a new one."""
    nnzC = bh.get_nnzC()
    Cp = bh.get_rowptrC() if bh._rowptrC is None else bh._rowptrC
    Cj = np.empty(nnzC, np.int32)
    Cx = np.empty(nnzC, bh._vdt)
    _check(bh.get_C(Cj, Cx), "get_C")
    return Cp, Cj, Cx


def _free(bh):
    _check(bh.free_mem(), "free_mem")


def _upload(a, dt, device):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dt).copy()).to(torch.device("cuda", device))


def _device_csr(Xp, Xj, Xx, value_dtype, device):
    """(rowPtr, colInd, val) as torch tensors on the device; val stays None."""
    return (_upload(Xp, np.int32, device), _upload(Xj, np.int32, device),
            None if Xx is None else _upload(Xx, value_dtype, device))


def _host(*tensors):
    return tuple(t.cpu().numpy() for t in tensors)


def spgemm_csr(m, k, n, Ap, Aj, Ax, Bp, Bj, Bx, device=0, warmups=0, options=None, value_dtype=np.float64):
    """Convenience: run the reference call sequence once on host CSR arrays and
    return (rowPtrC int32[m+1], colIndC int32[nnzC], valC value_dtype[nnzC], info)."""
    with _handle(value_dtype, device, options) as bh:
        _bind(bh, m, k, n, Ap, Aj, Ax, Bp, Bj, Bx, np.zeros(m + 1, np.int32))
        for _ in range(warmups):
            _check(bh.warmup(), "warmup")
        _check(bh.spgemm(), "spgemm")
        Cp, Cj, Cx = _fetch(bh)
        info = {"nnzCt": bh.nnzCt, "nnzC": len(Cj), "stage_ms": bh.stage_ms, "time_ms": bh.time_ms,
                "kernels": bh.kernel_stats(), "mixed_rows": bh.get_info("mixed_rows"),
                "class_state": bh.get_info("class_state")}
        _free(bh)
    return Cp, Cj, Cx, info


def spgemm_masked_csr(m, k, n, Ap, Aj, Ax, Bp, Bj, Bx, Mp, Mj, options=None, value_dtype=np.float64, device=0):
    """Convenience: the masked multiply once on host CSR arrays.  Returns (valC value_dtype[nnzM], info); the result's
    pattern is the caller's (Mp, Mj)."""
    with _handle(value_dtype, device, options) as bh:
        _bind(bh, m, k, n, Ap, Aj, Ax, Bp, Bj, Bx, None)
        valC = bh.spgemm_masked(Mp, Mj)
        info = {"nnzCt": bh.nnzCt, "ms": bh.masked_ms, "kernels": bh.kernel_stats()}
        _free(bh)
    return valC, info


def spgemm_semiring_csr(m, k, n, Ap, Aj, Ax, Bp, Bj, Bx, semiring, options=None, value_dtype=np.float64, device=0):
    """Convenience: C = A (+).(x) B once on host CSR arrays.  Returns (rowPtrC, colIndC, valC, info)."""
    with _handle(value_dtype, device, options) as bh:
        _bind(bh, m, k, n, Ap, Aj, Ax, Bp, Bj, Bx, np.zeros(m + 1, np.int32))
        _check(bh.spgemm_semiring(semiring), "bhs_spgemm_semiring")
        Cp, Cj, Cx = _fetch(bh)
        info = {"nnzCt": bh.nnzCt, "nnzC": len(Cj), "semiring_ms": bh.semiring_ms, "multiply_ms": bh.multiply_ms,
                "time_ms": bh.time_ms, "kernels": bh.kernel_stats(), "class_state": bh.get_info("class_state")}
        _free(bh)
    return Cp, Cj, Cx, info


def spgemm_semiring_masked_csr(m, k, n, Ap, Aj, Ax, Bp, Bj, Bx, Mp, Mj, semiring, options=None, value_dtype=np.float64,
                               device=0):
    """Convenience: the masked multiply over a semiring once on host CSR arrays.  Returns (valC value_dtype[nnzM], info);
    the result's pattern is the caller's (Mp, Mj)."""
    with _handle(value_dtype, device, options) as bh:
        _bind(bh, m, k, n, Ap, Aj, Ax, Bp, Bj, Bx, None)
        valC = bh.spgemm_semiring_masked(semiring, Mp, Mj)
        info = {"nnzCt": bh.nnzCt, "ms": bh.semiring_ms, "kernels": bh.kernel_stats()}
        _free(bh)
    return valC, info


def select_spec(band=None, drop_diag=False, keep_diag=False, abs_tol=None, rel_tol=None, top_k=None):
    """A bhs_select rule: band = (lo, hi) on col - row (None ends: unbounded), abs_tol / rel_tol / top_k set their flag when
    given."""
    s = _lib.Select()
    s.flags = 0
    s.band_lo, s.band_hi = -2 ** 63, 2 ** 63 - 1
    if band is not None:
        s.flags |= _lib.BHS_SEL_BAND
        s.band_lo = -2 ** 63 if band[0] is None else int(band[0])
        s.band_hi = 2 ** 63 - 1 if band[1] is None else int(band[1])
    if drop_diag:
        s.flags |= _lib.BHS_SEL_DROP_DIAG
    if keep_diag:
        s.flags |= _lib.BHS_SEL_KEEP_DIAG
    if abs_tol is not None:
        s.flags |= _lib.BHS_SEL_ABS
        s.abs_tol = float(abs_tol)
    if rel_tol is not None:
        s.flags |= _lib.BHS_SEL_REL
        s.rel_tol = float(rel_tol)
    if top_k is not None:
        s.flags |= _lib.BHS_SEL_TOPK
        s.top_k = int(top_k)
    return s


def csr_add(m, n, alpha, Xp, Xj, Xx, beta, Yp, Yj, Yx, value_dtype=np.float64, device=0):
    """Convenience: Z = alpha X + beta Y once on host CSR arrays (m x n, rows strictly ascending), staged as torch tensors
    on the handle's device -- the stand-alone add takes device arrays only.  Returns (Zp int32[m+1], Zj int32[nnzZ],
    Zx value_dtype[nnzZ], info) with info["kernels"], info["y_inside_x"], info["ms"].  Needs no multiply data."""
    import torch
    X = _device_csr(Xp, Xj, Xx, value_dtype, device)
    Y = _device_csr(Yp, Yj, Yx, value_dtype, device)
    assert X[2].dtype == (torch.float32 if np.dtype(value_dtype) == np.dtype(np.float32) else torch.float64)
    with _handle(value_dtype, device, None) as bh:
        Zp, Zj, Zx, inside = bh.csr_add_device(m, n, alpha, X, beta, Y)
        info = {"kernels": bh.kernel_stats(), "y_inside_x": inside, "ms": bh.add_ms}
        return _host(Zp, Zj, Zx) + (info,)


def spgemm_add_csr(m, k, n, Ap, Aj, Ax, Bp, Bj, Bx, Dp, Dj, Dx, alpha=1.0, beta=1.0, options=None, value_dtype=np.float64,
                   device=0):
    """Convenience: C = alpha A·B + beta D once on host CSR arrays.  Returns (rowPtrC, colIndC, valC, info)."""
    with _handle(value_dtype, device, options) as bh:
        _bind(bh, m, k, n, Ap, Aj, Ax, Bp, Bj, Bx, np.zeros(m + 1, np.int32))
        _check(bh.spgemm_add(alpha, beta, Dp, Dj, Dx), "bhs_spgemm_add")
        Cp, Cj, Cx = _fetch(bh)
        info = {"nnzCt": bh.nnzCt, "nnzC": len(Cj), "add_ms": bh.add_ms, "time_ms": bh.time_ms, "kernels": bh.kernel_stats(),
                "add_inplace_used": bh.get_info("add_inplace_used"), "class_state": bh.get_info("class_state")}
        _free(bh)
    return Cp, Cj, Cx, info


def csr_select(m, n, Xp, Xj, Xx, spec, value_dtype=np.float64, device=0):
    """Convenience: Z = select(X) once on host CSR arrays (m x n), staged as torch tensors on the handle's device -- the
    stand-alone selection takes device arrays only.  Returns (Zp int32[m+1], Zj int32[nnzZ], Zx value_dtype[nnzZ], info)
    with info["kernels"], info["ms"].  Needs no multiply data."""
    X = _device_csr(Xp, Xj, Xx, value_dtype, device)
    with _handle(value_dtype, device, None) as bh:
        Z = bh.csr_select_device(m, n, X, spec)
        return _host(*Z) + ({"kernels": bh.kernel_stats(), "ms": bh.select_ms},)


def spgemm_select_csr(m, k, n, Ap, Aj, Ax, Bp, Bj, Bx, spec, options=None, value_dtype=np.float64, device=0):
    """Convenience: C = select(A·B) once on host CSR arrays.  Returns (rowPtrC, colIndC, valC, info)."""
    with _handle(value_dtype, device, options) as bh:
        _bind(bh, m, k, n, Ap, Aj, Ax, Bp, Bj, Bx, np.zeros(m + 1, np.int32))
        _check(bh.spgemm_select(spec), "bhs_spgemm_select")
        Cp, Cj, Cx = _fetch(bh)
        info = {"nnzCt": bh.nnzCt, "nnzC": len(Cj), "select_ms": bh.select_ms, "time_ms": bh.time_ms, "kernels": bh.kernel_stats(),
                "select_dropped": bh.get_info("select_dropped"), "class_state": bh.get_info("class_state")}
        _free(bh)
    return Cp, Cj, Cx, info


def csr_transpose(m, n, Xp, Xj, Xx, value_dtype=np.float64, device=0):
    """Convenience: T = X^T once on host CSR arrays (X is m x n; rows in any order, duplicates allowed), staged as torch
    tensors on the handle's device -- the transpose takes device arrays only.  Returns (Tp int32[n+1], Tj int32[nnz],
    Tx value_dtype[nnz], info) with info["kernels"], info["ms"], info["perm"] (int32[nnz]: the position in X of every entry
    of T).  Needs no multiply data."""
    X = _device_csr(Xp, Xj, Xx, value_dtype, device)
    with _handle(value_dtype, device, None) as bh:
        Tp, Tj, Tx, pm = bh.csr_transpose_device(m, n, X, values=True, perm=True)
        info = {"kernels": bh.kernel_stats(), "ms": bh.transpose_ms, "perm": pm.cpu().numpy()}
        return _host(Tp, Tj, Tx) + (info,)


def extract_csr(m, n, Xp, Xj, Xx, rows=None, cols=None, value_dtype=np.float64, device=0):
    """Convenience: Z = X(rows, cols) once on host CSR arrays (X is m x n; rows in any order, duplicates allowed; rows /
    cols: index arrays or None for all in order), staged as torch tensors on the handle's device -- the extraction takes
    device arrays only.  Returns (Zp int32[mI+1], Zj int32[nnzZ], Zx value_dtype[nnzZ], info) with info["kernels"],
    info["ms"], info["reordered_rows"], info["perm"] (int32[nnzZ]: the position in X of every entry of Z).  Needs no
    multiply data."""
    X = _device_csr(Xp, Xj, Xx, value_dtype, device)
    r = None if rows is None else _upload(rows, np.int32, device)
    c = None if cols is None else _upload(cols, np.int32, device)
    with _handle(value_dtype, device, None) as bh:
        Zp, Zj, Zx, pm = bh.csr_extract_device(m, n, X, rows=r, cols=c, values=True, perm=True)
        info = {"kernels": bh.kernel_stats(), "ms": bh.extract_ms, "reordered_rows": bh.get_info("extract_reordered_rows"),
                "perm": pm.cpu().numpy()}
        return _host(Zp, Zj, Zx) + (info,)


def permute_csr(n, Xp, Xj, Xx, p, value_dtype=np.float64, device=0):
    """Convenience: the symmetric reordering X(p, p) of an n x n matrix: extract_csr with rows = cols = p."""
    return extract_csr(n, n, Xp, Xj, Xx, rows=p, cols=p, value_dtype=value_dtype, device=device)


def reduce_csr(m, n, Xp, Xj, Xx, axis, op, offdiag=False, value_dtype=np.float64, device=0):
    """Convenience: reduce(X) once on host CSR arrays (X is m x n; Xx may be None: every entry counts as 1), staged as
    torch tensors on the handle's device.  axis: _lib.BHS_AXIS_*, op: _lib.BHS_RED_*.  Returns (out value_dtype[...],
    info) with info["kernels"], info["ms"].  Needs no multiply data."""
    X = _device_csr(Xp, Xj, Xx, value_dtype, device)
    with _handle(value_dtype, device, None) as bh:
        out = bh.csr_reduce_device(m, n, X, axis, op, offdiag=offdiag)
        return out.cpu().numpy(), {"kernels": bh.kernel_stats(), "ms": bh.reduce_ms}


def diagonal_csr(m, n, Xp, Xj, Xx, value_dtype=np.float64, device=0):
    """Convenience: diag(X), min(m, n) values (duplicate pairs add up, a missing diagonal entry is 0)."""
    return reduce_csr(m, n, Xp, Xj, Xx, _lib.BHS_AXIS_DIAG, _lib.BHS_RED_PLUS, value_dtype=value_dtype, device=device)[0]


def scale_csr(m, n, Xp, Xj, Xx, alpha=1.0, left=None, right=None, left_div=False, right_div=False, value_dtype=np.float64,
              device=0):
    """Convenience: the values of Z = alpha diag(left) X diag(right) once on host CSR arrays (Z has X's pattern).  Returns
    (Zx value_dtype[nnzX], info) with info["kernels"], info["ms"]."""
    X = _device_csr(Xp, Xj, Xx, value_dtype, device)
    l = None if left is None else _upload(left, value_dtype, device)
    r = None if right is None else _upload(right, value_dtype, device)
    with _handle(value_dtype, device, None) as bh:
        Zx = bh.csr_scale_device(m, n, X, alpha, l, r, left_div, right_div)
        return Zx.cpu().numpy(), {"kernels": bh.kernel_stats(), "ms": bh.scale_ms}


def normalize_csr(m, n, Xp, Xj, Xx, axis, norm=1, value_dtype=np.float64, device=0):
    """Convenience: X with every row (axis = _lib.BHS_AXIS_ROWS) or column (BHS_AXIS_COLS) divided by its norm, kept on the
    device between the reduction and the scaling: norm 1 (sum |x|), "inf" (max |x|) or 2 (sqrt of sum x^2).  A zero norm
    divides by 1 (the row or column stays as it is).  Returns (Zx value_dtype[nnzX], norms)."""
    import torch
    if axis not in (_lib.BHS_AXIS_ROWS, _lib.BHS_AXIS_COLS) or norm not in (1, 2, "inf"):
        raise ValueError("axis is BHS_AXIS_ROWS or BHS_AXIS_COLS, norm 1, 2 or \"inf\"")
    X = _device_csr(Xp, Xj, Xx, value_dtype, device)
    op = {1: _lib.BHS_RED_ABS_PLUS, "inf": _lib.BHS_RED_ABS_MAX, 2: _lib.BHS_RED_SQ_PLUS}[norm]
    with _handle(value_dtype, device, None) as bh:
        nrm = bh.csr_reduce_device(m, n, X, axis, op)
        if norm == 2:
            nrm = torch.sqrt(nrm)
        div = torch.where(nrm == 0, torch.ones_like(nrm), nrm)
        rows = axis == _lib.BHS_AXIS_ROWS
        Zx = bh.csr_scale_device(m, n, X, 1.0, div if rows else None, None if rows else div, rows, not rows)
        return _host(Zx, nrm)


def smoothed_prolongator_csr(n, nc, Ap, Aj, Ax, Tp, Tj, Tx, omega, options=None, value_dtype=np.float64, device=0):
    """Convenience: the smoothed prolongator P = T - omega D^-1 A T of an n x n matrix A (D = diag(A)) and an n x nc
    tentative prolongator T (rows strictly ascending) on host CSR arrays, kept on the device between the upload and one
    get_C: diag(A) (bhs_csr_reduce_device), -omega D^-1 A (bhs_csr_scale_device with LEFT_DIV), then the multiply with T
    plus T (bhs_spgemm_add, alpha = beta = 1).  Returns (Pp int32[n+1], Pj, Px, info); info: "nnzCt", "nnzC",
    "reduce_ms", "scale_ms", "add_ms", "kernels"."""
    A = _device_csr(Ap, Aj, Ax, value_dtype, device)
    T = _device_csr(Tp, Tj, Tx, value_dtype, device)
    with _handle(value_dtype, device, options) as bh:
        d = bh.csr_reduce_device(n, n, A, _lib.BHS_AXIS_DIAG, _lib.BHS_RED_PLUS)
        Sx = bh.csr_scale_device(n, n, A, -float(omega), left=d, left_div=True)
        nnzA, nnzT = A[1].numel(), T[1].numel()
        _check(bh.initData_device(n, n, nc, nnzA, Sx, A[0], A[1], nnzT, T[2], T[0], T[1]), "initData_device(-omega D^-1 A, T)")
        _check(bh.spgemm_add_device(1.0, 1.0, nnzT, T[2], T[0], T[1]), "bhs_spgemm_add_device")
        Pp, Pj, Px = _fetch(bh)
        info = {"nnzCt": bh.nnzCt, "nnzC": len(Pj), "reduce_ms": bh.reduce_ms, "scale_ms": bh.scale_ms, "add_ms": bh.add_ms,
                "kernels": bh.kernel_stats()}
        bh.free_mem()
    return Pp, Pj, Px, info


def galerkin_csr(m, nc, Pp, Pj, Px, Ap, Aj, Ax, options=None, value_dtype=np.float64, device=0):
    """Convenience: the Galerkin product C = P^T·(A·P) of an m x m matrix A and an m x nc prolongator P on host CSR
    arrays, kept on the device between the upload and one get_C: P is transposed there, one handle multiplies A·P, a
    second one multiplies P^T with the first one's device-resident result (bhs_get_C_device).  Public calls only.
    Returns (Cp int32[nc+1], Cj, Cx, info); info: "nnzCt_AP", "nnzCt" (products of the two multiplies), "nnzC_AP", "nnzC",
    "transpose_ms", "ap_ms", "ptap_ms" (device times), "class_state_AP", "class_state", "kernels_AP", "kernels"."""
    P = _device_csr(Pp, Pj, Px, value_dtype, device)
    A = _device_csr(Ap, Aj, Ax, value_dtype, device)
    nnzP, nnzA = P[1].numel(), A[1].numel()
    with _handle(value_dtype, device, options) as h1, _handle(value_dtype, device, options) as h2:
        Tp, Tj, Tx, _ = h2.csr_transpose_device(m, nc, P)
        info = {"transpose_ms": h2.transpose_ms}
        _check(h1.initData_device(m, m, nc, nnzA, A[2], A[0], A[1], nnzP, P[2], P[0], P[1]), "initData_device(A, P)")
        _check(h1.spgemm(), "spgemm(A·P)")
        nnzAP = h1.get_nnzC()
        dAPp, dAPj, dAPx = h1.get_C_device()
        info.update({"nnzCt_AP": h1.nnzCt, "nnzC_AP": nnzAP, "ap_ms": float(sum(h1.stage_ms)), "kernels_AP": h1.kernel_stats(),
                     "class_state_AP": h1.get_info("class_state")})
        _check(h2.initData_device(nc, m, nc, nnzP, Tx, Tp, Tj, nnzAP, dAPx, dAPp, dAPj), "initData_device(P^T, A·P)")
        _check(h2.spgemm(), "spgemm(P^T·AP)")
        Cp, Cj, Cx = _fetch(h2)
        info.update({"nnzCt": h2.nnzCt, "nnzC": len(Cj), "ptap_ms": float(sum(h2.stage_ms)), "kernels": h2.kernel_stats(),
                     "class_state": h2.get_info("class_state")})
        h2.free_mem()
        h1.free_mem()
    return Cp, Cj, Cx, info
