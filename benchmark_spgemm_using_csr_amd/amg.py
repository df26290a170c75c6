"""A smoothed-aggregation multigrid setup that never leaves the device: MIS(2) aggregation (bhs_csr_aggregate_device;
include/bhsparse_hip.h, "aggregation") and, built from it and the existing device calls of a `facade.bhsparse` handle, the
strength pattern, the tentative and the smoothed prolongator, the Galerkin product, a V-cycle and a solver.  The cycle's
smoother is weighted Jacobi or multicolour Gauss-Seidel on a device colouring (bhs_csr_color_device, bhs_csr_gs_device;
"colouring and relaxation"); with forward sweeps before and backward sweeps after the coarse correction the cycle is
symmetric and preconditions CG (pcg_device).  A second, value-driven coarsening stands beside MIS(2): heavy-edge matching
(bhs_csr_match_device; "matching"), repeated on the Galerkin-coarsened matrix into pairwise aggregates of up to 2^passes
vertices that follow the strong couplings (pairwise_aggregate_device), and the same hierarchy on them (pa_setup_device):
more levels and a higher operator complexity for fewer iterations (profiles/match_case.md has what that costs in time).
The classical (Ruge-Stueben) half of the family stands beside the aggregations: a C/F splitting of the strength pattern
(bhs_csr_cfsplit_device; "C/F splitting and interpolation": the greedy maximal independent set under the PMIS measure), the
direct interpolation on it as a symbolic / numeric pair (bhs_csr_interp_symbolic_device, bhs_csr_interp_numeric_device) and
the hierarchy of the two (rs_setup_device; profiles/cf_case.md).
A third smoother needs no colouring: sweeps of a polynomial in D^-1 A as one library call (bhs_csr_relax_device;
"relaxation and fused products": relax_device, jacobi_device), Chebyshev coefficients on an interval from a Lanczos estimate
of rho(D^-1 A) (spectral_radius_device, cheby_setup_device), and the cycle and PCG with it (smoother="chebyshev";
profiles/relax_case.md).
Beside it: the level sets of a triangle, the sparse triangular solve and ILU(0) in place (bhs_csr_levels_device, bhs_csr_trsv_device, bhs_csr_ilu0_device; "triangular solve and ILU(0)") and CG
preconditioned with that factorisation in natural or colour order (ilu0_pcg_device).
And a preconditioner without any sequential dependence: the factorised sparse approximate inverse G on tril(A) or a caller's
pattern (bhs_csr_fsai_device; "approximate inverse": fsai_device, fsai_setup_device), applied as two products z = G^T (G r)
(fsai_apply_device), and CG with it (fsai_pcg_device; profiles/fsai_case.md).

Everything is a torch tensor on the handle's GPU: a matrix is (rowPtr int32, colInd int32, val), a pattern the first two.
Functions of handles, not methods.  Every step is a thin call into the C-ABI; a missing library raises, nothing is computed
on the host but the handful of scalars a call returns."""
import ctypes as C
import time

import numpy as np

from . import _lib
from .dense import csr_spmv_device
from .facade import BhsparseError, _alloc, _check, _device_csr, _handle, _host, _ptr, select_spec  # noqa: F401


def _tdt(bh):
    import torch
    return torch.float32 if bh._vdt == np.dtype(np.float32) else torch.float64


# ---------------------------------------------------------------- aggregation
def aggregate_raw_device(bh, n, nnzS, d_rowPtrS, d_colIndS, d_prio, seed, flags, d_agg, d_roots):
    """bhs_csr_aggregate_device on caller-given arrays, the C arguments in order (d_prio and d_roots may be None): the status
    code; sets bh.aggregate_ms, bh.aggregate_nagg and bh.aggregate_rounds on success."""
    return bh._counted("bhs_csr_aggregate_device", "aggregate", "nagg", "rounds", int(n), int(nnzS), _ptr(d_rowPtrS),
                       _ptr(d_colIndS), _ptr(d_prio), int(seed) & 0xFFFFFFFF, int(flags), _ptr(d_agg), _ptr(d_roots))


def aggregate_device(bh, n, S, seed=0, prio=None):
    """MIS(2) aggregates of the n x n pattern S = (rowPtr, colInd[, anything]) of strong connections, torch tensors on the
    handle's GPU; prio: n priorities as an int32 / uint32 tensor's bits, or None for the hash of (vertex, seed).  Returns
    (agg int32[n], nagg, roots int32[nagg]): the aggregate of every vertex and the roots, ascending, agg[roots[a]] == a.
    bh.aggregate_rounds and bh.aggregate_ms hold the rounds and the device time.  Raises BhsparseError on failure."""
    import torch
    Sp, Sj = S[0], S[1]
    agg = _alloc(n, torch.int32, Sp.device)
    roots = _alloc(n, torch.int32, Sp.device)
    torch.cuda.synchronize()                           # the library works on its own stream (see facade.initData_device)
    _check(aggregate_raw_device(bh, n, Sj.numel(), Sp, Sj, prio, seed, 0, agg, roots), "bhs_csr_aggregate_device")
    return agg[:n], bh.aggregate_nagg, roots[:bh.aggregate_nagg]


# ---------------------------------------------------------------- matching and pairwise aggregation
def match_raw_device(bh, n, nnzA, d_rowPtrA, d_colIndA, d_valA, seed, flags, d_mate, d_agg):
    """bhs_csr_match_device on caller-given arrays, the C arguments in order (d_valA and d_agg may be None): the status code;
    sets bh.match_ms, bh.match_npairs and bh.match_rounds on success."""
    return bh._counted("bhs_csr_match_device", "match", "npairs", "rounds", int(n), int(nnzA), _ptr(d_rowPtrA),
                       _ptr(d_colIndA), _ptr(d_valA), int(seed) & 0xFFFFFFFF, int(flags), _ptr(d_mate), _ptr(d_agg))


def match_device(bh, n, A, seed=0):
    """The heavy-edge matching of the n x n matrix A = (rowPtr, colInd, val-or-None), torch tensors on the handle's GPU: the
    greedy matching in descending (|a_ij|, hash, indices) where pattern and weights are symmetric; None for the values:
    every weight 1.  Returns (mate int32[n], agg int32[n], nagg, npairs): mate[i] == i where i is unmatched, agg the pairs
    and singletons numbered by ascending smaller member, nagg = n - npairs.  bh.match_rounds and bh.match_ms hold the rounds
    and the device time.  Raises BhsparseError on failure."""
    import torch
    Ap, Aj = A[0], A[1]
    Ax = A[2] if len(A) > 2 else None
    mate = _alloc(n, torch.int32, Ap.device)
    agg = _alloc(n, torch.int32, Ap.device)
    torch.cuda.synchronize()                           # the library works on its own stream (see facade.initData_device)
    _check(match_raw_device(bh, n, Aj.numel(), Ap, Aj if Aj.numel() else None, Ax if Aj.numel() else None, seed, 0, mate, agg),
           "bhs_csr_match_device")
    return mate[:n], agg[:n], n - bh.match_npairs, bh.match_npairs


def match_csr(n, Ap, Aj, Ax, seed=0, value_dtype=np.float64, device=0):
    """Convenience: match_device once on host CSR arrays (Ax may be None: every weight 1).  Returns numpy (mate int32[n],
    agg int32[n], nagg, npairs)."""
    A = _device_csr(Ap, Aj, Ax, value_dtype, device)
    with _handle(value_dtype, device, None) as bh:
        mate, agg, nagg, npairs = match_device(bh, n, A, seed)
        return _host(mate, agg) + (nagg, npairs)


def pairwise_aggregate_device(handles, n, A, passes=2, seed=0):
    """Pairwise aggregation of the n x n matrix A = (rowPtr, colInd, val): `passes` (1..4) heavy-edge matchings, pass p on the
    current matrix with seed + p; between two passes the matrix is coarsened with the unit tentative prolongator of the
    pass's pairs, T = (0..m, agg_p, ones), through galerkin_device (T^T A T: the sums of A over the pairs), and the
    aggregates are composed, agg = agg_p[agg].  handles: (h1, h2) as galerkin_device takes them.  Stops early where a pass
    matches nothing.  Returns (agg int32[n], nagg, info): aggregates of at most 2^passes vertices, numbered by ascending
    smallest member (a pass numbers its pairs by ascending smaller member, and by induction that is the aggregate of the
    smallest fine vertex); info a list with one entry per pass: n, npairs, rounds and the device ms of match / galerkin."""
    import torch
    if not 1 <= int(passes) <= 4:
        raise ValueError("passes is 1, 2, 3 or 4")
    h1, h2 = handles
    agg, m, info = None, n, []
    for p in range(int(passes)):
        _, agg_p, nagg, npairs = match_device(h1, m, A, seed + p)
        rec = {"n": m, "npairs": npairs, "rounds": h1.match_rounds, "match_ms": h1.match_ms}
        info.append(rec)
        if npairs == 0:
            break
        agg = agg_p if agg is None else agg_p[agg.long()]
        if p + 1 < int(passes):
            T = (torch.arange(m + 1, dtype=torch.int32, device=agg_p.device), agg_p.contiguous(),
                 torch.ones(m, dtype=_tdt(h1), device=agg_p.device))
            A, _ = galerkin_device(h1, h2, m, nagg, A, T)
            rec["galerkin_ms"] = h1.galerkin_ms
        m = nagg
    if agg is None:
        agg = torch.arange(n, dtype=torch.int32, device=A[0].device)
    return agg.to(torch.int32).contiguous(), m, info


# ---------------------------------------------------------------- C/F splitting and direct interpolation
def cfsplit_raw_device(bh, n, nnzS, d_rowPtrS, d_colIndS, d_prio, seed, flags, d_cf, d_cpts):
    """bhs_csr_cfsplit_device on caller-given arrays, the C arguments in order (d_prio and d_cpts may be None): the status code;
    sets bh.cfsplit_ms, bh.cfsplit_nc and bh.cfsplit_rounds on success."""
    return bh._counted("bhs_csr_cfsplit_device", "cfsplit", "nc", "rounds", int(n), int(nnzS), _ptr(d_rowPtrS),
                       _ptr(d_colIndS), _ptr(d_prio), int(seed) & 0xFFFFFFFF, int(flags), _ptr(d_cf), _ptr(d_cpts))


def cfsplit_device(bh, n, S, seed=0, prio=None, degree=True):
    """The C/F splitting of the n x n pattern S = (rowPtr, colInd[, anything]) of strong connections, torch tensors on the
    handle's GPU: the greedy maximal independent set in descending key order.  degree (the default; not with prio): the key's
    priority is the row's length over the hash of (vertex, seed), the PMIS measure; else prio as in aggregate_device.
    Returns (cf int32[n], nc, cpts int32[nc]): the coarse index of every C point, -1 at an F point, and the C points,
    ascending, cf[cpts[c]] == c.  bh.cfsplit_rounds and bh.cfsplit_ms hold the rounds and the device time.  Raises
    BhsparseError on failure."""
    import torch
    Sp, Sj = S[0], S[1]
    cf = _alloc(n, torch.int32, Sp.device)
    cpts = _alloc(n, torch.int32, Sp.device)
    flags = _lib.BHS_CF_DEGREE if degree and prio is None else 0
    torch.cuda.synchronize()                           # the library works on its own stream (see facade.initData_device)
    _check(cfsplit_raw_device(bh, n, Sj.numel(), Sp, Sj if Sj.numel() else None, prio, seed, flags, cf, cpts),
           "bhs_csr_cfsplit_device")
    return cf[:n], bh.cfsplit_nc, cpts[:bh.cfsplit_nc]


def interp_symbolic_raw_device(bh, n, nnzA, d_rowPtrA, d_colIndA, nnzS, d_rowPtrS, d_colIndS, d_cf, nc, d_rowPtrP):
    """bhs_csr_interp_symbolic_device on caller-given arrays, the C arguments in order: the status code; sets
    bh.interp_symbolic_ms and bh.interp_nnzP on success."""
    if bh._h is None:
        return _lib.BHS_ERR_NOT_READY
    nnzP, ms = C.c_longlong(0), C.c_double(0)
    err = bh._lib.bhs_csr_interp_symbolic_device(bh._h, int(n), int(nnzA), _ptr(d_rowPtrA), _ptr(d_colIndA), int(nnzS),
                                                 _ptr(d_rowPtrS), _ptr(d_colIndS), _ptr(d_cf), int(nc), _ptr(d_rowPtrP),
                                                 C.byref(nnzP), C.byref(ms))
    if err == _lib.BHS_SUCCESS:
        bh.interp_symbolic_ms, bh.interp_nnzP = float(ms.value), int(nnzP.value)
    return err


def interp_numeric_raw_device(bh, n, nnzA, d_rowPtrA, d_colIndA, d_valA, nnzS, d_rowPtrS, d_colIndS, d_cf, nc, d_rowPtrP, nnzP,
                              d_colIndP, d_valP, flags=0):
    """bhs_csr_interp_numeric_device on caller-given arrays, the C arguments in order: the status code; sets
    bh.interp_numeric_ms on success."""
    if bh._h is None:
        return _lib.BHS_ERR_NOT_READY
    ms = C.c_double(0)
    err = bh._lib.bhs_csr_interp_numeric_device(bh._h, int(n), int(nnzA), _ptr(d_rowPtrA), _ptr(d_colIndA), _ptr(d_valA),
                                                int(nnzS), _ptr(d_rowPtrS), _ptr(d_colIndS), _ptr(d_cf), int(nc),
                                                _ptr(d_rowPtrP), int(nnzP), _ptr(d_colIndP), _ptr(d_valP), int(flags),
                                                C.byref(ms))
    if err == _lib.BHS_SUCCESS:
        bh.interp_numeric_ms = float(ms.value)
    return err


def _none_if_empty(t):
    return t if t is not None and t.numel() else None


def interp_values_device(bh, n, A, S, cf, nc, rowPtrP):
    """The numeric call alone on a kept pattern: (colIndP, valP) of the direct interpolation for the row pointer an earlier
    interp_direct_device returned on the same patterns and cf -- A's values may have changed.  bh.interp_numeric_ms holds
    the device time.  Raises BhsparseError on failure (a row pointer of another splitting among them)."""
    import torch
    nnzP = int(rowPtrP[n]) if n else 0
    Pj = _alloc(nnzP, torch.int32, A[0].device)
    Px = _alloc(nnzP, _tdt(bh), A[0].device)
    torch.cuda.synchronize()                           # the library works on its own stream (see facade.initData_device)
    _check(interp_numeric_raw_device(bh, n, A[1].numel(), A[0], _none_if_empty(A[1]), _none_if_empty(A[2]), S[1].numel(), S[0],
                                     _none_if_empty(S[1]), cf, nc, rowPtrP, nnzP, Pj, Px), "bhs_csr_interp_numeric_device")
    return Pj[:nnzP], Px[:nnzP]


def interp_direct_device(bh, n, A, S, cf, nc):
    """The direct interpolation P (n x nc) of the n x n matrix A = (rowPtr, colInd, val) on the splitting cf (what
    cfsplit_device returned) and the pattern S = (rowPtr, colInd) of strong connections, rows of both strictly ascending:
    an identity row at a C point, at an F point the weights of include/bhsparse_hip.h ("C/F splitting and interpolation") on
    its strong C neighbours.  Returns (rowPtr, colInd, val); bh.interp_ms is the device time of the symbolic and the numeric
    call.  Raises BhsparseError on failure."""
    import torch
    Pp = _alloc(n + 1, torch.int32, A[0].device)
    torch.cuda.synchronize()                           # the library works on its own stream (see facade.initData_device)
    _check(interp_symbolic_raw_device(bh, n, A[1].numel(), A[0], _none_if_empty(A[1]), S[1].numel(), S[0], _none_if_empty(S[1]),
                                      cf, nc, Pp), "bhs_csr_interp_symbolic_device")
    Pp = Pp[:n + 1]
    Pj, Px = interp_values_device(bh, n, A, S, cf, nc, Pp)
    bh.interp_ms = bh.interp_symbolic_ms + bh.interp_numeric_ms
    return Pp, Pj, Px


# ---------------------------------------------------------------- colouring and relaxation
def color_raw_device(bh, n, nnzS, d_rowPtrS, d_colIndS, d_prio, seed, flags, d_color, d_order, d_colorPtr):
    """bhs_csr_color_device on caller-given arrays, the C arguments in order (d_prio may be None): the status code; sets
    bh.color_ms, bh.color_ncolors and bh.color_rounds on success."""
    return bh._counted("bhs_csr_color_device", "color", "ncolors", "rounds", int(n), int(nnzS), _ptr(d_rowPtrS),
                       _ptr(d_colIndS), _ptr(d_prio), int(seed) & 0xFFFFFFFF, int(flags), _ptr(d_color), _ptr(d_order),
                       _ptr(d_colorPtr))


def color_device(bh, n, S, seed=0, prio=None):
    """The first-fit greedy colouring in descending key order of the n x n pattern S = (rowPtr, colInd[, anything]), torch
    tensors on the handle's GPU; prio as in aggregate_device.  Returns (color int32[n], ncolors, order int32[n],
    colorPtr_host): order holds the vertices by (colour, index), colorPtr_host is a numpy int32 array of ncolors + 1 offsets
    into it, on the host, where bhs_csr_gs_device wants it.  bh.color_rounds and bh.color_ms hold the rounds and the device
    time.  Raises BhsparseError on failure."""
    import torch
    Sp, Sj = S[0], S[1]
    color = _alloc(n, torch.int32, Sp.device)
    order = _alloc(n, torch.int32, Sp.device)
    cptr = _alloc(n + 1, torch.int32, Sp.device)
    torch.cuda.synchronize()                           # the library works on its own stream (see facade.initData_device)
    _check(color_raw_device(bh, n, Sj.numel(), Sp, Sj, prio, seed, 0, color, order, cptr), "bhs_csr_color_device")
    ncolors = bh.color_ncolors
    cptr_host = cptr[:ncolors + 1].cpu().numpy().astype(np.int32) if n else np.zeros(1, np.int32)
    return color[:n], ncolors, order[:n], cptr_host


_GS_DIRECTIONS = {"forward": _lib.BHS_GS_FORWARD, "backward": _lib.BHS_GS_BACKWARD, "symmetric": _lib.BHS_GS_SYMMETRIC}


def gs_raw_device(bh, n, nnzA, d_rowPtrA, d_colIndA, d_valA, d_diag, ncolors, h_colorPtr, d_order, d_color, d_b, d_x, omega,
                  sweeps, flags):
    """bhs_csr_gs_device on caller-given arrays, the C arguments in order (h_colorPtr: a numpy int32 array on the host;
    d_color may be None without BHS_GS_VERIFY): the status code; sets bh.gs_ms on success."""
    if bh._h is None:
        return _lib.BHS_ERR_NOT_READY
    ms = C.c_double(0)
    hptr = None if h_colorPtr is None else np.ascontiguousarray(h_colorPtr, np.int32)
    err = bh._lib.bhs_csr_gs_device(bh._h, int(n), int(nnzA), _ptr(d_rowPtrA), _ptr(d_colIndA), _ptr(d_valA), _ptr(d_diag),
                                    int(ncolors), _ptr(hptr), _ptr(d_order), _ptr(d_color), _ptr(d_b), _ptr(d_x), float(omega),
                                    int(sweeps), int(flags), C.byref(ms))
    if err == _lib.BHS_SUCCESS:
        bh.gs_ms = float(ms.value)
    return err


def gs_device(bh, A, diag, coloring, b, x, omega=1.0, sweeps=1, direction="symmetric", verify=False):
    """`sweeps` multicolour Gauss-Seidel (omega == 1) or SOR sweeps on A x = b, IN PLACE on x: A = (rowPtr, colInd, val),
    diag its diagonal, coloring what color_device returned, all torch tensors on the handle's GPU.  direction: "forward"
    (colours ascending), "backward" or "symmetric" (forward then backward in each sweep); verify: the kernels check the
    colouring against A as they go.  Returns x; bh.gs_ms holds the device time.  Raises BhsparseError on failure."""
    import torch
    color, ncolors, order, cptr = coloring
    flags = _GS_DIRECTIONS[direction] | (_lib.BHS_GS_VERIFY if verify else 0)
    torch.cuda.synchronize()                           # the library works on its own stream (see facade.initData_device)
    _check(gs_raw_device(bh, _rows(A), A[1].numel(), A[0], A[1], A[2], diag, ncolors, cptr, order, color, b, x, omega, sweeps,
                         flags), "bhs_csr_gs_device")
    return x


# ---------------------------------------------------------------- polynomial relaxation
def chebyshev_coefficients(lmin, lmax, steps):
    """bhs_chebyshev_coefficients: the `steps` pairs (a_s, c_s) of the Chebyshev iteration on [lmin, lmax] as a float64
    numpy array of shape (steps, 2), what relax_device takes as coef.  Raises ValueError for anything but
    0 < lmin < lmax, both finite, steps >= 1.  No device work: needs the library, no handle."""
    steps = int(steps)
    out = np.zeros(2 * max(steps, 1), np.float64)
    err = _lib.load().bhs_chebyshev_coefficients(float(lmin), float(lmax), steps, out.ctypes.data_as(C.POINTER(C.c_double)))
    if err != _lib.BHS_SUCCESS:
        raise ValueError("0 < lmin < lmax, both finite, and steps >= 1")
    return out.reshape(steps, 2)


def relax_raw_device(bh, n, nnzA, d_valA, d_rowPtrA, d_colIndA, d_diag, steps, coef, d_b, d_x, d_d, flags):
    """bhs_csr_relax_device on caller-given arrays, the C arguments in order (coef: 2 * steps doubles on the host, anything
    numpy makes a float64 array of, or None; d_valA and d_d may be None): the status code; sets bh.relax_ms."""
    if bh._h is None:
        return _lib.BHS_ERR_NOT_READY
    hcoef = None if coef is None else np.ascontiguousarray(coef, np.float64).reshape(-1)
    cptr = None if hcoef is None else hcoef.ctypes.data_as(C.POINTER(C.c_double))
    return bh._timed(bh._lib.bhs_csr_relax_device, "relax_ms", int(n), int(nnzA), _ptr(d_valA), _ptr(d_rowPtrA), _ptr(d_colIndA),
                     _ptr(d_diag), int(steps), cptr, _ptr(d_b), _ptr(d_x), _ptr(d_d), int(flags))


def relax_device(bh, A, diag, b, x, coef, d=None, zero_guess=False):
    """len(coef) relaxation steps on A x = b, IN PLACE on x (and on d where given): A = (rowPtr, colInd, val), diag the
    divisor of every row, all torch tensors on the handle's GPU; coef the (steps, 2) pairs (a_s, c_s) of
    include/bhsparse_hip.h, "relaxation and fused products" (chebyshev_coefficients; weighted Jacobi is (0, omega)).  d: the
    last step's correction, carried between calls; made here where a step reads it and none is given.  zero_guess: x counts
    as zero and is not read (one product less).  Returns x; bh.relax_ms holds the device time.  Raises BhsparseError on
    failure."""
    import torch
    coef = np.ascontiguousarray(coef, np.float64).reshape(-1, 2)
    if d is None and np.any(coef[:, 0] != 0.0):
        d = torch.zeros_like(x)
    torch.cuda.synchronize()                           # the library works on its own stream (see facade.initData_device)
    _check(relax_raw_device(bh, _rows(A), A[1].numel(), A[2], A[0], _none_if_empty(A[1]), diag, len(coef), coef, b, x, d,
                            _lib.BHS_RELAX_ZERO_GUESS if zero_guess else 0), "bhs_csr_relax_device")
    return x


def jacobi_device(bh, A, diag, b, x, omega, sweeps, zero_guess=False):
    """`sweeps` weighted Jacobi sweeps x <- x + omega D^-1 (b - A x) in one call, IN PLACE on x (relax_device with the
    pairs (0, omega)).  Returns x."""
    return relax_device(bh, A, diag, b, x, [(0.0, float(omega))] * int(sweeps), None, zero_guess)


def _start_vector(n, seed):
    """n values in [-1, 1) from a 64-bit mix of (index, seed) (splitmix64's finaliser): the same on every machine"""
    with np.errstate(over="ignore"):
        z = (np.arange(n, dtype=np.uint64) + np.uint64(1)) * np.uint64(0x9E3779B97F4A7C15) + np.uint64(int(seed) & 0xFFFFFFFF)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z = z ^ (z >> np.uint64(31))
    return (z >> np.uint64(11)).astype(np.float64) * (2.0 ** -52) - 1.0


def spectral_radius_device(bh, n, A, diag=None, steps=10, seed=0):
    """An estimate from below of rho(D^-1 A) for the symmetric n x n matrix A = (rowPtr, colInd, val) with the positive
    diagonal `diag` (taken from A when None): `steps` Lanczos steps on D^-1/2 A D^-1/2 -- formed once with
    csr_scale_device --, every product with its two reductions from csr_spmv_dots_device, from the start vector of
    (index, seed); the largest eigenvalue of the small tridiagonal matrix (numpy.linalg.eigvalsh), a Ritz value and so never
    above the largest eigenvalue.  bh.lanczos_ms holds the device time of the products.  Raises ValueError on a diagonal
    that is not positive."""
    import torch
    from .dense import csr_spmv_dots_device
    if diag is None:
        diag = bh.csr_reduce_device(n, n, A, _lib.BHS_AXIS_DIAG, _lib.BHS_RED_PLUS)
    if n == 0 or not bool((diag > 0).all()):
        raise ValueError("the diagonal must be positive")
    root = torch.sqrt(diag)
    S = (A[0], A[1], bh.csr_scale_device(n, n, A, 1.0, left=root, right=root, left_div=True, right_div=True))
    v = torch.from_numpy(_start_vector(n, seed)).to(device=diag.device, dtype=diag.dtype)
    v = v / torch.linalg.norm(v)
    prev, beta, alphas, betas, ms = None, 0.0, [], [], 0.0
    for _ in range(max(1, min(int(steps), n))):
        z, _, alpha = csr_spmv_dots_device(bh, n, n, S, v, 1.0, -beta, prev, v)      # z = S v - beta v_prev, alpha = <v, z>
        ms += bh.spmv_dots_ms
        alphas.append(alpha)
        z = z - alpha * v
        nrm = float(torch.linalg.norm(z))
        if not nrm > 1e-12 * max(abs(a) for a in alphas):                          # (an invariant subspace: the Ritz values are eigenvalues)
            break
        betas.append(nrm)
        prev, v, beta = v, z / nrm, nrm
    k = len(alphas)
    T = np.diag(alphas) + np.diag(betas[:k - 1], 1) + np.diag(betas[:k - 1], -1)
    bh.lanczos_ms = ms
    return float(np.linalg.eigvalsh(T)[-1])


def cheby_setup_device(bh, levels, degree=2, lanczos_steps=10, upper=1.1, lower_ratio=0.3):
    """What the Chebyshev smoother needs of every level but the last: (diag(A_l), coef) with the `degree` coefficient pairs
    for [lmin, lmax], lmax = upper * spectral_radius_device(A_l, lanczos_steps) and lmin = lower_ratio * lmax (hypre's
    defaults).  A list to pass to vcycle_device as `smoothers`."""
    out = []
    for A, P, _ in levels:
        if P is None:
            continue
        n = _rows(A)
        d = bh.csr_reduce_device(n, n, A, _lib.BHS_AXIS_DIAG, _lib.BHS_RED_PLUS)
        lmax = float(upper) * spectral_radius_device(bh, n, A, d, lanczos_steps)
        out.append((d, chebyshev_coefficients(float(lower_ratio) * lmax, lmax, degree)))
    return out


def _vcycle_chebyshev(bh, levels, b, x, pre, post, smoothers, lvl):
    """The cycle of vcycle_device with the Chebyshev smoother; x None: the guess is zero (BHS_RELAX_ZERO_GUESS)."""
    import torch
    from .dense import csr_spmv_dots_device
    A, P, R = levels[lvl]
    if P is None:
        return vcycle_device(bh, levels, b, x, lvl=lvl)            # (the dense solve: the guess is not looked at)
    n, nc = _rows(A), _rows(R)
    d, coef = smoothers[lvl]
    zero = x is None
    x = torch.empty_like(b) if zero else x.clone()
    carry = torch.empty_like(b)                                    # (step 0 of every call has a == 0: never read before it is written)
    for _ in range(pre):
        relax_device(bh, A, d, b, x, coef, carry, zero)
        zero = False
    if zero:
        x.zero_()
    r, _, _ = csr_spmv_dots_device(bh, n, n, A, x, -1.0, 1.0, b)
    rc = csr_spmv_device(bh, nc, n, R, r)
    xc = _vcycle_chebyshev(bh, levels, rc, None, pre, post, smoothers, lvl + 1)
    x = csr_spmv_device(bh, n, nc, P, xc, alpha=1.0, beta=1.0, y=x)
    for _ in range(post):
        relax_device(bh, A, d, b, x, coef, carry)
    return x


# ---------------------------------------------------------------- the pieces of a level
def strength_device(bh, n, A, theta):
    """The symmetric pattern of strong connections of the n x n matrix A (rows strictly ascending): the selection keeps the
    diagonal and every a_ij unless |a_ij| < theta * max_{k != i} |a_ik| (csr_select_device, rel_tol, keep_diag), its
    transpose (csr_transpose_device) is united with it (csr_add_device).  theta == 0 is pattern(A) U pattern(A^T).
    Returns (rowPtr, colInd); bh.strength_ms is the three calls' device time."""
    import torch
    Zp, Zj, _ = bh.csr_select_device(n, n, A, select_spec(rel_tol=float(theta), keep_diag=True), values=False)
    ms = bh.select_ms
    Tp, Tj, _, _ = bh.csr_transpose_device(n, n, (Zp, Zj, None), values=False)
    ms += bh.transpose_ms
    one = lambda j: torch.ones(max(j.numel(), 1), dtype=_tdt(bh), device=j.device)[:j.numel()]   # noqa: E731
    Sp, Sj, _, _ = bh.csr_add_device(n, n, 1.0, (Zp, Zj, one(Zj)), 1.0, (Tp, Tj, one(Tj)))
    bh.strength_ms = ms + bh.add_ms
    return Sp, Sj


def affinity_strength_device(bh, n, A, theta=0.5, vectors=16, sweeps=8, omega=2.0 / 3.0, seed=0):
    """The symmetric pattern of strong connections of the n x n matrix A (rows strictly ascending, a non-zero diagonal) by
    the affinity of relaxed test vectors (Livne and Brandt's lean AMG; also "algebraic distance"), which a symmetric
    diagonal scaling of A does not defeat as it defeats strength_device's |a_ij| >= theta max: column c of X (n x vectors)
    starts as _start_vector(n, seed + c) and takes `sweeps` weighted Jacobi sweeps on A x = 0, X <- X - omega D^-1 (A X)
    (csr_spmm_device; the diagonal from csr_reduce_device); then, on pattern(A),
        c_ij = (x_i . x_j)^2 / ((x_i . x_i) (x_j . x_j))
    from three sampled products (dense.csr_sddmm_device: g on pattern(A), g^2 by a second call with times_m on g, the
    x_i . x_i on the identity's pattern) and csr_scale_device with both divisions; strength_device's rule on c -- the
    diagonal and every c_ij unless c_ij < theta max_{k != i} c_ik, united with its transpose -- ends it.  Returns
    (rowPtr, colInd), what aggregate_device, cfsplit_device and match_device take; bh.affinity_ms is the calls' device
    time."""
    import torch
    from .dense import csr_sddmm_device, csr_spmm_device
    Ap, Aj, _ = A
    dev, tdt = Ap.device, _tdt(bh)
    X = torch.from_numpy(np.stack([_start_vector(n, seed + c) for c in range(int(vectors))], axis=1))
    X = X.to(device=dev, dtype=tdt).contiguous()
    diag = bh.csr_reduce_device(n, n, A, _lib.BHS_AXIS_DIAG, _lib.BHS_RED_PLUS)
    ms = bh.reduce_ms
    for _ in range(int(sweeps)):
        AX = csr_spmm_device(bh, n, n, A, X)
        ms += bh.spmv_ms
        X = X - float(omega) * (AX / diag[:, None])
    g = csr_sddmm_device(bh, n, n, (Ap, Aj, None), X, X)
    ms += bh.sddmm_ms
    g2 = csr_sddmm_device(bh, n, n, (Ap, Aj, g), X, X, times_m=True)
    ms += bh.sddmm_ms
    eye = (torch.arange(n + 1, dtype=torch.int32, device=dev), torch.arange(n, dtype=torch.int32, device=dev), None)
    dd = csr_sddmm_device(bh, n, n, eye, X, X)
    ms += bh.sddmm_ms
    c = bh.csr_scale_device(n, n, (Ap, Aj, g2), 1.0, left=dd, right=dd, left_div=True, right_div=True)
    ms += bh.scale_ms
    Sp, Sj = strength_device(bh, n, (Ap, Aj, c), theta)
    bh.affinity_ms = ms + bh.strength_ms
    return Sp, Sj


def tentative_device(bh, n, agg, nagg, cand=None):
    """The tentative prolongator T (n x nagg) of the aggregates `agg` and one candidate vector (ones when None):
    T(i, agg[i]) = cand[i] / ||cand over the aggregate||_2.  The column norms come from the stable transpose of T with its
    values (csr_transpose_device), a SQ_PLUS reduction along its rows (csr_reduce_device) and a square root; T's values from
    csr_scale_device with right_div: no scattered sum, so they repeat bit for bit.  Returns ((rowPtr, colInd, val),
    coarse_cand): the norms are the candidate on the coarse level."""
    import torch
    dev = agg.device
    Tp = torch.arange(n + 1, dtype=torch.int32, device=dev)
    Tj = agg.to(torch.int32).contiguous()
    x = torch.ones(n, dtype=_tdt(bh), device=dev) if cand is None else cand.to(_tdt(bh)).contiguous()
    Rp, Rj, Rx, _ = bh.csr_transpose_device(n, nagg, (Tp, Tj, x), values=True)
    nrm = torch.sqrt(bh.csr_reduce_device(nagg, n, (Rp, Rj, Rx), _lib.BHS_AXIS_ROWS, _lib.BHS_RED_SQ_PLUS))
    Tx = bh.csr_scale_device(n, nagg, (Tp, Tj, x), 1.0, right=nrm, right_div=True)
    return (Tp, Tj, Tx), nrm


def _result_device(bh, rows, dev):
    """(rowPtrC, colIndC, valC) of the handle's last multiply as torch tensors of their own: cloned out of bhs_get_C_device
    before the handle is used again"""
    import torch
    nnz = bh.get_nnzC()
    ptrs = bh.get_C_device()
    vstr, tdt = ("<f4", torch.float32) if bh._vdt == np.dtype(np.float32) else ("<f8", torch.float64)

    class _View(object):
        def __init__(self, ptr, count, typestr):
            self.__cuda_array_interface__ = {"shape": (int(count),), "typestr": typestr, "data": (int(ptr), False), "version": 2,
                                             "strides": None}

    def take(ptr, count, typestr, dtype):
        if count == 0 or not ptr:
            return torch.empty(0, dtype=dtype, device=dev)
        return torch.as_tensor(_View(ptr, count, typestr), device=dev).clone()
    out = take(ptrs[0], rows + 1, "<i4", torch.int32), take(ptrs[1], nnz, "<i4", torch.int32), take(ptrs[2], nnz, vstr, tdt)
    torch.cuda.synchronize()
    return out


def smoothed_prolongator_device(bh, n, nc, A, T, omega):
    """P = T - omega D^-1 A T on device tensors, the steps of facade.smoothed_prolongator_csr: diag(A), -omega D^-1 A, the
    multiply with T plus T.  Returns (rowPtr, colInd, val) of its own; bh.prolongator_ms is the device time."""
    d = bh.csr_reduce_device(n, n, A, _lib.BHS_AXIS_DIAG, _lib.BHS_RED_PLUS)
    ms = bh.reduce_ms
    Sx = bh.csr_scale_device(n, n, A, -float(omega), left=d, left_div=True)
    ms += bh.scale_ms
    nnzA, nnzT = A[1].numel(), T[1].numel()
    _check(bh.initData_device(n, n, nc, nnzA, Sx, A[0], A[1], nnzT, T[2], T[0], T[1]), "initData_device(-omega D^-1 A, T)")
    t0 = time.perf_counter()
    _check(bh.spgemm_add_device(1.0, 1.0, nnzT, T[2], T[0], T[1]), "bhs_spgemm_add_device")
    ms += (time.perf_counter() - t0) * 1e3               # (the call is synchronous: the multiply and the add)
    P = _result_device(bh, n, A[0].device)
    _check(bh.free_mem(), "free_mem")
    bh.prolongator_ms = ms
    return P


def galerkin_device(h1, h2, n, nc, A, P):
    """(A_c = P^T (A P), R = P^T) on device tensors, the steps of facade.galerkin_csr: h2 transposes P, h1 multiplies A P, h2
    multiplies P^T with h1's device-resident result.  h1.galerkin_ms is the device time of the three."""
    Rp, Rj, Rx, _ = h2.csr_transpose_device(n, nc, P)
    ms = h2.transpose_ms
    nnzA, nnzP = A[1].numel(), P[1].numel()
    _check(h1.initData_device(n, n, nc, nnzA, A[2], A[0], A[1], nnzP, P[2], P[0], P[1]), "initData_device(A, P)")
    _check(h1.spgemm(), "spgemm(A P)")
    ms += float(sum(h1.stage_ms))
    nnzAP = h1.get_nnzC()
    dAPp, dAPj, dAPx = h1.get_C_device()
    _check(h2.initData_device(nc, n, nc, nnzP, Rx, Rp, Rj, nnzAP, dAPx, dAPp, dAPj), "initData_device(P^T, A P)")
    _check(h2.spgemm(), "spgemm(P^T AP)")
    ms += float(sum(h2.stage_ms))
    Ac = _result_device(h2, nc, A[0].device)
    _check(h2.free_mem(), "free_mem")
    _check(h1.free_mem(), "free_mem")
    h1.galerkin_ms = ms
    return Ac, (Rp, Rj, Rx)


# ---------------------------------------------------------------- the setup
def sa_setup_device(handles, n, A, theta=0.0, omega=2.0 / 3.0, max_levels=10, min_coarse=40, seed=0):
    """The smoothed-aggregation hierarchy of the n x n matrix A = (rowPtr, colInd, val), torch tensors on the GPU, rows
    strictly ascending.  handles: two initialised facade.bhsparse handles (h1, h2) of A's value type, or a callable that
    makes one (called twice; those are destroyed here).  Per level: strength -> aggregate -> tentative -> P = T - omega
    D^-1 A T -> A_c = P^T (A P); coarsening stops at max_levels, at min_coarse rows or fewer, or where nothing is merged.
    omega "estimate" (pa_setup_device the same): 4 / (3 rho) per level, rho from spectral_radius_device on that level's
    matrix; the level's record then holds "omega" and "lanczos_ms".
    Returns (levels, info): levels a list of (A_l, P_l, R_l = P_l^T) with P = R = None on the last; info a list with one
    entry per level: n, nnz and, where the level was coarsened, nagg, rounds and the device ms of strength / aggregate /
    prolongator / galerkin."""
    def coarsen(h1, h2, n, A, lvl):
        S = strength_device(h1, n, A, theta)
        agg, nagg, _ = aggregate_device(h1, n, S, seed)
        return agg, nagg, {"rounds": h1.aggregate_rounds, "strength_ms": h1.strength_ms, "aggregate_ms": h1.aggregate_ms}
    return _setup_levels(handles, n, A, coarsen, omega, max_levels, min_coarse)


def _setup_levels(handles, n, A, coarsen, omega, max_levels, min_coarse, prolong=None, count="nagg"):
    """The level loop of sa_setup_device, pa_setup_device and rs_setup_device: coarsen(h1, h2, n, A, level) -> (agg, nagg,
    what the level's record says of it), then tentative -> smoothed prolongator -> Galerkin product, until max_levels,
    min_coarse rows or fewer, or a level on which nothing is merged.  prolong (None: the tentative and the smoothed
    prolongator): prolong(h1, n, A, agg, nagg) -> (P, what the record says of it) in their place; count: the record's key
    for the coarse size."""
    own = callable(handles)
    h1, h2 = (handles(), handles()) if own else handles
    try:
        levels, info = [], []
        while True:
            rec = {"n": n, "nnz": int(A[1].numel())}
            info.append(rec)
            if len(levels) + 1 >= max_levels or n <= min_coarse:
                break
            agg, nagg, said = coarsen(h1, h2, n, A, len(levels))
            if nagg >= n:
                break
            if prolong is None:
                T, _ = tentative_device(h1, n, agg, nagg)
                timing = {}
                if isinstance(omega, str):                            # "estimate": 4 / (3 rho(D^-1 A_l)) from Lanczos
                    if omega != "estimate":
                        raise ValueError("omega is a number or 'estimate'")
                    level_omega = 4.0 / (3.0 * spectral_radius_device(h1, n, A))
                    timing = {"omega": level_omega, "lanczos_ms": h1.lanczos_ms}
                else:
                    level_omega = omega
                P = smoothed_prolongator_device(h1, n, nagg, A, T, level_omega)
                timing["prolongator_ms"] = h1.prolongator_ms
            else:
                P, timing = prolong(h1, n, A, agg, nagg)
            Ac, R = galerkin_device(h1, h2, n, nagg, A, P)
            rec.update({count: nagg})
            rec.update(said)
            rec.update(timing)
            rec.update({"galerkin_ms": h1.galerkin_ms})
            levels.append((A, P, R))
            A, n = Ac, nagg
        levels.append((A, None, None))
        return levels, info
    finally:
        if own:
            h1.freePlatform()
            h2.freePlatform()


def pa_setup_device(handles, n, A, passes=3, omega=2.0 / 3.0, max_levels=10, min_coarse=40, seed=0):
    """The hierarchy of sa_setup_device with pairwise aggregation in place of strength and MIS(2): per level
    pairwise_aggregate_device(passes) with seed + 8 * level -> tentative -> P = T - omega D^-1 A T -> A_c = P^T (A P).
    handles, the stopping rules and (levels, info) as sa_setup_device; a level's record holds n, nnz and, where it was
    coarsened, nagg, the passes' records ("passes") and the device ms of aggregate (the matchings and the Galerkin products
    between them) / prolongator / galerkin.  vcycle_device, smoother_setup_device, solve_device and pcg_device run on it
    unchanged.  passes defaults to 3: on the MI355X two passes gave fewer iterations but, at a million unknowns, eight or
    nine levels and an operator complexity of 4 to 13, and lost to three passes in setup plus solve time on all three
    matrices measured (profiles/match_case.md)."""
    if not 1 <= int(passes) <= 4:
        raise ValueError("passes is 1, 2, 3 or 4")

    def coarsen(h1, h2, n, A, lvl):
        agg, nagg, said = pairwise_aggregate_device((h1, h2), n, A, passes, seed + 8 * lvl)
        ms = sum(r["match_ms"] + r.get("galerkin_ms", 0.0) for r in said)
        return agg, nagg, {"passes": said, "aggregate_ms": ms}
    return _setup_levels(handles, n, A, coarsen, omega, max_levels, min_coarse)


def rs_setup_device(handles, n, A, theta=0.25, max_levels=10, min_coarse=40, seed=0):
    """The classical (Ruge-Stueben) hierarchy of the n x n matrix A = (rowPtr, colInd, val), rows strictly ascending: per
    level strength_device(theta) -> cfsplit_device (the PMIS measure, seed + 8 * level) -> interp_direct_device ->
    A_c = P^T (A P).  handles, the stopping rules and (levels, info) as sa_setup_device; a level's record holds n, nnz and,
    where it was coarsened, nc, rounds and the device ms of strength / split / interp / galerkin.  P has an identity row at
    every C point and no more entries a row than the strength pattern, so the coarse operators stay sparse where the smoothed
    prolongator's grow.  vcycle_device, smoother_setup_device, solve_device and pcg_device run on it unchanged
    (profiles/cf_case.md has what it costs and where it loses)."""
    kept = {}

    def coarsen(h1, h2, n, A, lvl):
        S = strength_device(h1, n, A, theta)
        cf, nc, _ = cfsplit_device(h1, n, S, seed + 8 * lvl)
        kept["S"] = S
        return cf, nc, {"rounds": h1.cfsplit_rounds, "strength_ms": h1.strength_ms, "split_ms": h1.cfsplit_ms}

    def prolong(h1, n, A, cf, nc):
        P = interp_direct_device(h1, n, A, kept.pop("S"), cf, nc)
        return P, {"interp_ms": h1.interp_ms}
    return _setup_levels(handles, n, A, coarsen, None, max_levels, min_coarse, prolong, "nc")


def _setup_csr(setup, n, Ap, Aj, Ax, value_dtype, device, *args):
    """setup((h1, h2), n, A, *args) -- one of the three hierarchies -- on a host CSR matrix, the levels copied back"""
    A = _device_csr(Ap, Aj, Ax, value_dtype, device)
    with _handle(value_dtype, device, None) as h1, _handle(value_dtype, device, None) as h2:
        levels, info = setup((h1, h2), n, A, *args)
    host = lambda M: None if M is None else _host(*M)   # noqa: E731
    return [(host(a), host(p), host(r)) for a, p, r in levels], info


def rs_setup_csr(n, Ap, Aj, Ax, theta=0.25, max_levels=10, min_coarse=40, seed=0, value_dtype=np.float64, device=0):
    """Convenience: rs_setup_device on a host CSR matrix (rows strictly ascending), built on the device and copied back, as
    sa_setup_csr."""
    return _setup_csr(rs_setup_device, n, Ap, Aj, Ax, value_dtype, device, theta, max_levels, min_coarse, seed)


def pa_setup_csr(n, Ap, Aj, Ax, passes=3, omega=2.0 / 3.0, max_levels=10, min_coarse=40, seed=0, value_dtype=np.float64,
                 device=0):
    """Convenience: pa_setup_device on a host CSR matrix (rows strictly ascending), built on the device and copied back, as
    sa_setup_csr."""
    return _setup_csr(pa_setup_device, n, Ap, Aj, Ax, value_dtype, device, passes, omega, max_levels, min_coarse, seed)


def sa_setup_csr(n, Ap, Aj, Ax, theta=0.0, omega=2.0 / 3.0, max_levels=10, min_coarse=40, seed=0, value_dtype=np.float64,
                 device=0):
    """Convenience: the hierarchy of a host CSR matrix (rows strictly ascending), built on the device and copied back.
    Returns (levels, info): levels a list of (A_l, P_l, R_l) with every matrix a (rowPtr, colInd, val) triple of numpy
    arrays, None for P and R on the last; info as sa_setup_device."""
    return _setup_csr(sa_setup_device, n, Ap, Aj, Ax, value_dtype, device, theta, omega, max_levels, min_coarse, seed)


# ---------------------------------------------------------------- the cycle
def _rows(M):
    return int(M[0].numel()) - 1


def _diagonals(bh, levels):
    """diag(A_l) of every level but the last, kept on the hierarchy's first entry between cycles"""
    return [bh.csr_reduce_device(_rows(A), _rows(A), A, _lib.BHS_AXIS_DIAG, _lib.BHS_RED_PLUS) for A, P, _ in levels if P is not None]


def _jacobi(bh, A, d, b, x, omega_jacobi, sweeps):
    n = _rows(A)
    for _ in range(sweeps):
        r = csr_spmv_device(bh, n, n, A, x, alpha=-1.0, beta=1.0, y=b.clone())      # b - A x
        x = x + omega_jacobi * r / d
    return x


def smoother_setup_device(bh, levels, seed=0):
    """What the Gauss-Seidel smoother needs of every level but the last: (diag(A_l), colouring of pattern(A_l) U
    pattern(A_l^T)) -- the diagonal from csr_reduce_device, the pattern from strength_device(theta = 0), the colouring from
    color_device with the hash of (vertex, seed).  A list to pass to vcycle_device / pcg_device as `smoothers`."""
    out = []
    for A, P, _ in levels:
        if P is None:
            continue
        n = _rows(A)
        d = bh.csr_reduce_device(n, n, A, _lib.BHS_AXIS_DIAG, _lib.BHS_RED_PLUS)
        out.append((d, color_device(bh, n, strength_device(bh, n, A, 0.0), seed)))
    return out


def vcycle_device(bh, levels, b, x, omega_jacobi=2.0 / 3.0, pre=1, post=1, diagonals=None, lvl=0, smoother="jacobi",
                  smoothers=None):
    """One V(pre, post) cycle for A_0 x = b on the hierarchy of sa_setup_device: restriction and prolongation by R_l and P_l
    through csr_spmv_device, the coarsest level by a dense torch.linalg.solve.  smoother "jacobi": weighted Jacobi from
    csr_spmv_device (y = alpha A x + beta y) and the diagonal.  smoother "gs": `pre` forward multicolour Gauss-Seidel
    sweeps before the coarse correction and `post` backward sweeps after it (gs_device; smoothers: what
    smoother_setup_device returned, made here when None) -- a symmetric cycle where pre == post.  smoother "chebyshev":
    `pre` calls of relax_device with the level's Chebyshev coefficients before the coarse correction and `post` after it
    (smoothers: what cheby_setup_device returned, made here when None), the coarse levels from a zero guess that is never
    read, the residual from csr_spmv_dots_device -- a polynomial in D^-1 A on both sides, so symmetric where pre == post,
    with no colouring.  Returns the new x."""
    import torch
    if smoother not in ("jacobi", "gs", "chebyshev"):
        raise ValueError("smoother is 'jacobi', 'gs' or 'chebyshev'")
    if smoother == "chebyshev" and levels[lvl][1] is not None:
        if smoothers is None:
            smoothers = cheby_setup_device(bh, levels)
        return _vcycle_chebyshev(bh, levels, b, x, pre, post, smoothers, lvl)
    A, P, R = levels[lvl]
    n = _rows(A)
    if P is None:
        dense = torch.zeros((n, n), dtype=b.dtype, device=b.device)
        rows = torch.repeat_interleave(torch.arange(n, device=b.device), (A[0][1:] - A[0][:-1]).long())
        dense.index_put_((rows, A[1].long()), A[2], accumulate=True)
        return torch.linalg.solve(dense, b)
    gs = smoother == "gs"
    if gs and smoothers is None:
        smoothers = smoother_setup_device(bh, levels)
    if not gs and diagonals is None:
        diagonals = _diagonals(bh, levels)
    nc = _rows(R)
    if gs:
        d, coloring = smoothers[lvl]
        x = gs_device(bh, A, d, coloring, b, x.clone(), 1.0, pre, "forward")
    else:
        d = diagonals[lvl]
        x = _jacobi(bh, A, d, b, x, omega_jacobi, pre)
    r = csr_spmv_device(bh, n, n, A, x, alpha=-1.0, beta=1.0, y=b.clone())
    rc = csr_spmv_device(bh, nc, n, R, r)
    xc = vcycle_device(bh, levels, rc, torch.zeros_like(rc), omega_jacobi, pre, post, diagonals, lvl + 1, smoother, smoothers)
    x = csr_spmv_device(bh, n, nc, P, xc, alpha=1.0, beta=1.0, y=x.clone())
    if gs:
        return gs_device(bh, A, d, coloring, b, x, 1.0, post, "backward")
    return _jacobi(bh, A, d, b, x, omega_jacobi, post)


def solve_device(bh, levels, b, tol=1e-8, maxiter=100):
    """V(1,1) cycles from x = 0 until ||b - A x|| <= tol ||b|| or maxiter cycles.  Returns (x, cycles, residual norms)."""
    import torch
    A = levels[0][0]
    n = _rows(A)
    diagonals = _diagonals(bh, levels)
    x = torch.zeros_like(b)
    res = [float(torch.linalg.norm(b))]
    cycles = 0
    while res[-1] > tol * res[0] and cycles < maxiter:
        x = vcycle_device(bh, levels, b, x, diagonals=diagonals)
        r = csr_spmv_device(bh, n, n, A, x, alpha=-1.0, beta=1.0, y=b.clone())
        res.append(float(torch.linalg.norm(r)))
        cycles += 1
    return x, cycles, res


def pcg_device(bh, levels, b, tol=1e-8, maxiter=100, smoother="gs"):
    """Conjugate gradients for A_0 x = b from x = 0, preconditioned with one V(1,1) cycle from zero (smoother "gs": forward
    before and backward after, a symmetric operator; "jacobi" is symmetric too), until ||r|| <= tol ||b|| or maxiter
    iterations.  The products with A_0 are csr_spmv_device, the dot products and updates torch's.  Returns (x, iterations,
    residual norms): the norms of the recurrence's residual, the first ||b||.  smoother "chebyshev": the cycle of
    vcycle_device(smoother="chebyshev") on cheby_setup_device's defaults, from a zero guess that is never read, and
    q = A p with <p, q> from one csr_spmv_dots_device call."""
    import torch
    A = levels[0][0]
    n = _rows(A)
    if smoother == "chebyshev":
        return _pcg_chebyshev(bh, levels, b, tol, maxiter)
    smoothers = smoother_setup_device(bh, levels) if smoother == "gs" else None
    diagonals = _diagonals(bh, levels) if smoother == "jacobi" else None
    x = torch.zeros_like(b)
    r = b.clone()
    res = [float(torch.linalg.norm(r))]
    p, rz, its = None, 0.0, 0
    while res[-1] > tol * res[0] and its < maxiter:
        z = vcycle_device(bh, levels, r, torch.zeros_like(r), diagonals=diagonals, smoother=smoother, smoothers=smoothers)
        rz_new = float(torch.dot(r, z))
        p = z if p is None else z + (rz_new / rz) * p
        rz = rz_new
        q = csr_spmv_device(bh, n, n, A, p)
        alpha = rz / float(torch.dot(p, q))
        x = x + alpha * p
        r = r - alpha * q
        res.append(float(torch.linalg.norm(r)))
        its += 1
    return x, its, res


def _pcg_chebyshev(bh, levels, b, tol, maxiter, smoothers=None):
    """pcg_device's iteration with the Chebyshev cycle and the fused product"""
    import torch
    from .dense import csr_spmv_dots_device
    A = levels[0][0]
    n = _rows(A)
    if smoothers is None:
        smoothers = cheby_setup_device(bh, levels)
    x = torch.zeros_like(b)
    r = b.clone()
    res = [float(torch.linalg.norm(r))]
    p, rz, its = None, 0.0, 0
    while res[-1] > tol * res[0] and its < maxiter:
        z = _vcycle_chebyshev(bh, levels, r, None, 1, 1, smoothers, 0)
        rz_new = float(torch.dot(r, z))
        p = z if p is None else z + (rz_new / rz) * p
        rz = rz_new
        q, _, pq = csr_spmv_dots_device(bh, n, n, A, p, w=p)
        alpha = rz / pq
        x = x + alpha * p
        r = r - alpha * q
        res.append(float(torch.linalg.norm(r)))
        its += 1
    return x, its, res


# ---------------------------------------------------------------- triangular solve and ILU(0)
def levels_raw_device(bh, n, nnzA, d_rowPtrA, d_colIndA, flags, d_level, d_order, d_levelPtr):
    """bhs_csr_levels_device on caller-given arrays, the C arguments in order: the status code; sets bh.levels_ms,
    bh.levels_nlevels and bh.levels_passes (the passes depend on timing) on success."""
    return bh._counted("bhs_csr_levels_device", "levels", "nlevels", "passes", int(n), int(nnzA), _ptr(d_rowPtrA),
                       _ptr(d_colIndA), int(flags), _ptr(d_level), _ptr(d_order), _ptr(d_levelPtr))


def levels_device(bh, n, A, upper=False):
    """The level sets of the lower (j < i) or upper (j > i) triangle of the n x n pattern A = (rowPtr, colInd[, anything]),
    torch tensors on the handle's GPU: level(i) = 0 for a row without a counted entry, else 1 + the greatest level among
    them.  Returns (level int32[n], nlevels, order int32[n], levelPtr_host): order holds the rows by (level, index),
    levelPtr_host is a numpy int32 array of nlevels + 1 offsets into it, on the host, where bhs_csr_trsv_device and
    bhs_csr_ilu0_device want it.  bh.levels_ms holds the device time.  Raises BhsparseError on failure."""
    import torch
    Ap, Aj = A[0], A[1]
    level = _alloc(n, torch.int32, Ap.device)
    order = _alloc(n, torch.int32, Ap.device)
    lptr = _alloc(n + 1, torch.int32, Ap.device)
    torch.cuda.synchronize()                           # the library works on its own stream (see facade.initData_device)
    _check(levels_raw_device(bh, n, Aj.numel(), Ap, Aj, _lib.BHS_TRI_UPPER if upper else _lib.BHS_TRI_LOWER, level, order, lptr),
           "bhs_csr_levels_device")
    nlevels = bh.levels_nlevels
    lptr_host = lptr[:nlevels + 1].cpu().numpy().astype(np.int32) if n else np.zeros(1, np.int32)
    return level[:n], nlevels, order[:n], lptr_host


def trsv_raw_device(bh, n, nnzA, d_rowPtrA, d_colIndA, d_valA, nlevels, h_levelPtr, d_order, alpha, d_b, d_x, flags):
    """bhs_csr_trsv_device on caller-given arrays, the C arguments in order (h_levelPtr: a numpy int32 array on the host): the
    status code; sets bh.trsv_ms on success."""
    if bh._h is None:
        return _lib.BHS_ERR_NOT_READY
    ms = C.c_double(0)
    hptr = None if h_levelPtr is None else np.ascontiguousarray(h_levelPtr, np.int32)
    err = bh._lib.bhs_csr_trsv_device(bh._h, int(n), int(nnzA), _ptr(d_rowPtrA), _ptr(d_colIndA), _ptr(d_valA), int(nlevels),
                                      _ptr(hptr), _ptr(d_order), float(alpha), _ptr(d_b), _ptr(d_x), int(flags), C.byref(ms))
    if err == _lib.BHS_SUCCESS:
        bh.trsv_ms = float(ms.value)
    return err


def trsv_device(bh, A, levels, b, x, alpha=1.0, upper=False, unit_diag=False):
    """Solves T x = alpha b for T the lower or the upper triangle of A = (rowPtr, colInd, val) with its diagonal, read in
    place; levels: what levels_device returned for that triangle; b and x torch tensors on the handle's GPU, x may be b
    itself.  unit_diag: the diagonal is taken as 1 and diagonal entries are ignored.  Returns x; bh.trsv_ms holds the device
    time.  Raises BhsparseError on failure."""
    import torch
    _, nlevels, order, lptr = levels
    flags = (_lib.BHS_TRI_UPPER if upper else _lib.BHS_TRI_LOWER) | (_lib.BHS_TRI_UNIT_DIAG if unit_diag else 0)
    torch.cuda.synchronize()                           # the library works on its own stream (see facade.initData_device)
    _check(trsv_raw_device(bh, _rows(A), A[1].numel(), A[0], A[1], A[2], nlevels, lptr, order, alpha, b, x, flags),
           "bhs_csr_trsv_device")
    return x


def ilu0_raw_device(bh, n, nnzA, d_rowPtrA, d_colIndA, d_valA, nlevels, h_levelPtr, d_order, flags):
    """bhs_csr_ilu0_device on caller-given arrays, the C arguments in order (h_levelPtr: a numpy int32 array on the host): the
    status code; sets bh.ilu0_ms and bh.ilu0_pivot (the smallest row with a zero or non-finite pivot, or -1) on success."""
    if bh._h is None:
        return _lib.BHS_ERR_NOT_READY
    pivot, ms = C.c_int(-1), C.c_double(0)
    hptr = None if h_levelPtr is None else np.ascontiguousarray(h_levelPtr, np.int32)
    err = bh._lib.bhs_csr_ilu0_device(bh._h, int(n), int(nnzA), _ptr(d_rowPtrA), _ptr(d_colIndA), _ptr(d_valA), int(nlevels),
                                      _ptr(hptr), _ptr(d_order), int(flags), C.byref(pivot), C.byref(ms))
    if err == _lib.BHS_SUCCESS:
        bh.ilu0_ms, bh.ilu0_pivot = float(ms.value), int(pivot.value)
    return err


def ilu0_device(bh, A, levels):
    """A = L U on A's own pattern, IN PLACE on the values of A = (rowPtr, colInd, val) (rows strictly ascending, a diagonal
    entry in every row); levels: what levels_device returned for the lower triangle.  Afterwards the entries with j < i
    hold L (unit diagonal, not stored), those with j >= i hold U.  Returns A; bh.ilu0_pivot is the smallest row whose pivot
    is 0 or not finite, or -1; bh.ilu0_ms the device time.  Raises BhsparseError on failure."""
    import torch
    _, nlevels, order, lptr = levels
    torch.cuda.synchronize()                           # the library works on its own stream (see facade.initData_device)
    _check(ilu0_raw_device(bh, _rows(A), A[1].numel(), A[0], A[1], A[2], nlevels, lptr, order, 0), "bhs_csr_ilu0_device")
    return A


def _permuted_device(bh, n, A, perm):
    """A(perm, perm), rows ascending (csr_extract_device)"""
    Zp, Zj, Zx, _ = bh.csr_extract_device(n, n, A, rows=perm, cols=perm)
    return Zp, Zj, Zx


def ilu0_setup_device(bh, A, ordering="natural", seed=0):
    """The ILU(0) preconditioner of A = (rowPtr, colInd, val), rows strictly ascending.  ordering "natural": A as it is.
    "colour": A permuted by (colour, index) of the colouring of pattern(A) U pattern(A^T) (strength_device(theta = 0),
    color_device with the hash of (vertex, seed), csr_extract_device), whose triangles have as many levels as there are
    colours.  Both triangles are analysed (levels_device), the values copied and factorised (ilu0_device).  Returns what
    ilu0_apply_device needs: a dict with "LU" (rowPtr, colInd, val), "lower" and "upper" (the levels), "perm" (the
    permutation as an int64 tensor, None for "natural"), "ncolors" and "pivot"."""
    if ordering not in ("natural", "colour"):
        raise ValueError("ordering is 'natural' or 'colour'")
    n = _rows(A)
    perm, ncolors = None, 0
    if ordering == "colour":
        _, ncolors, order, _ = color_device(bh, n, strength_device(bh, n, A, 0.0), seed)
        A = _permuted_device(bh, n, A, order)
        perm = order.long()
    LU = (A[0], A[1], A[2].clone())
    lower = levels_device(bh, n, LU)
    upper = levels_device(bh, n, LU, upper=True)
    ilu0_device(bh, LU, lower)
    return {"LU": LU, "lower": lower, "upper": upper, "perm": perm, "ncolors": ncolors, "pivot": getattr(bh, "ilu0_pivot", -1)}


def ilu0_setup_permuted_device(bh, A, perm):
    """The ILU(0) preconditioner of A(perm, perm) for A = (rowPtr, colInd, val), rows strictly ascending, and a caller's
    permutation (an int32 device tensor: perm[k] is the old index of new row k -- ordering.rcm_device's, for one).  The
    same dict that ilu0_setup_device returns, so ilu0_apply_device serves unchanged; "ncolors" is 0."""
    n = _rows(A)
    A = _permuted_device(bh, n, A, perm)
    LU = (A[0], A[1], A[2].clone())
    lower = levels_device(bh, n, LU)
    upper = levels_device(bh, n, LU, upper=True)
    ilu0_device(bh, LU, lower)
    return {"LU": LU, "lower": lower, "upper": upper, "perm": perm.long(), "ncolors": 0, "pivot": getattr(bh, "ilu0_pivot", -1)}


def ilu0_apply_device(bh, M, r, z):
    """z = (L U)^-1 r for M of ilu0_setup_device: r permuted where M has a permutation, the unit lower solve, the upper solve
    in place, the result scattered back into z.  Returns z."""
    perm = M["perm"]
    y = r.clone() if perm is None else r[perm]
    trsv_device(bh, M["LU"], M["lower"], y, y, unit_diag=True)
    trsv_device(bh, M["LU"], M["upper"], y, y, upper=True)
    if perm is None:
        z.copy_(y)
    else:
        z[perm] = y
    return z


def _pcg_with(bh, A, b, tol, maxiter, apply):
    """Conjugate gradients for A x = b from x = 0 with z = apply(r, z) as the preconditioner, until ||r|| <= tol ||b|| or
    maxiter iterations: the loop ilu0_pcg_device and fsai_pcg_device share.  The products with A are csr_spmv_device, the
    dot products and updates torch's.  Returns (x, iterations, residual norms)."""
    import torch
    n = _rows(A)
    x = torch.zeros_like(b)
    r = b.clone()
    res = [float(torch.linalg.norm(r))]
    p, rz, its = None, 0.0, 0
    while res[-1] > tol * res[0] and its < maxiter:
        z = apply(r, torch.empty_like(r))
        rz_new = float(torch.dot(r, z))
        p = z if p is None else z + (rz_new / rz) * p
        rz = rz_new
        q = csr_spmv_device(bh, n, n, A, p)
        alpha = rz / float(torch.dot(p, q))
        x = x + alpha * p
        r = r - alpha * q
        res.append(float(torch.linalg.norm(r)))
        its += 1
    return x, its, res


def ilu0_pcg_device(bh, A, b, tol=1e-8, maxiter=100, ordering="colour"):
    """Conjugate gradients for A x = b from x = 0, preconditioned with ILU(0) of A in the given ordering
    (ilu0_setup_device, ilu0_apply_device), until ||r|| <= tol ||b|| or maxiter iterations.  The products with A are
    csr_spmv_device, the dot products and updates torch's.  Returns (x, iterations, residual norms) as pcg_device does."""
    M = ilu0_setup_device(bh, A, ordering)
    return _pcg_with(bh, A, b, tol, maxiter, lambda r, z: ilu0_apply_device(bh, M, r, z))


def ilu0_pcg_rcm_device(bh, A, b, tol=1e-8, maxiter=100):
    """ilu0_pcg_device with ILU(0) of A in reverse Cuthill-McKee order: ordering.rcm_device (pseudo-peripheral starts) on
    ordering.symmetric_pattern_device(A), ilu0_setup_permuted_device.  Returns (x, iterations, residual norms)."""
    from .ordering import rcm_device, symmetric_pattern_device
    n = _rows(A)
    M = ilu0_setup_permuted_device(bh, A, rcm_device(bh, n, symmetric_pattern_device(bh, n, A)))
    return _pcg_with(bh, A, b, tol, maxiter, lambda r, z: ilu0_apply_device(bh, M, r, z))


# ---------------------------------------------------------------- approximate inverse
def fsai_raw_device(bh, n, nnzA, d_rowPtrA, d_colIndA, d_valA, nnzG, d_rowPtrG, d_colIndG, d_valG, flags):
    """bhs_csr_fsai_device on caller-given arrays, the C arguments in order (include/bhsparse_hip.h, "approximate inverse"):
    the status code; sets bh.fsai_ms and bh.fsai_bad_row (the smallest row with a pivot that is not positive and finite, or
    -1) on success."""
    if bh._h is None:
        return _lib.BHS_ERR_NOT_READY
    bad, ms = C.c_int(-1), C.c_double(0)
    err = bh._lib.bhs_csr_fsai_device(bh._h, int(n), int(nnzA), _ptr(d_rowPtrA), _ptr(d_colIndA), _ptr(d_valA), int(nnzG),
                                      _ptr(d_rowPtrG), _ptr(d_colIndG), _ptr(d_valG), int(flags), C.byref(bad), C.byref(ms))
    if err == _lib.BHS_SUCCESS:
        bh.fsai_ms, bh.fsai_bad_row = float(ms.value), int(bad.value)
    return err


def fsai_device(bh, A, pattern=None):
    """The factorised sparse approximate inverse of the SPD matrix A = (rowPtr, colInd, val), rows strictly ascending: the
    lower-triangular G with G A G^T ~ I on `pattern` = (rowPtr, colInd) -- rows strictly ascending, each ending in its
    diagonal, at most BHS_FSAI_MAX_ROW entries --, by default the pattern of tril(A) (csr_select_device with the band
    col - row <= 0, no values).  Returns (rowPtrG, colIndG, valG); bh.fsai_bad_row is the smallest row with a bad pivot or
    -1, bh.fsai_ms the device time.  Raises BhsparseError on failure."""
    import torch
    n = _rows(A)
    if pattern is None:
        Gp, Gj, _ = bh.csr_select_device(n, n, A, select_spec(band=(None, 0)), values=False)
    else:
        Gp, Gj = pattern[0], pattern[1]
    nnzG = Gj.numel()
    Gx = _alloc(nnzG, A[2].dtype, A[0].device)
    torch.cuda.synchronize()                           # the library works on its own stream (see facade.initData_device)
    _check(fsai_raw_device(bh, n, A[1].numel(), A[0], A[1], A[2], nnzG, Gp, Gj, Gx, 0), "bhs_csr_fsai_device")
    return Gp, Gj, Gx[:nnzG]


def fsai_setup_device(bh, A, pattern=None):
    """The FSAI preconditioner of A (fsai_device) with its transpose (csr_transpose_device).  Returns what fsai_apply_device
    needs: a dict with "G" and "Gt" (rowPtr, colInd, val) and "bad_row"."""
    n = _rows(A)
    G = fsai_device(bh, A, pattern)
    bad_row = bh.fsai_bad_row
    Tp, Tj, Tx, _ = bh.csr_transpose_device(n, n, G)
    return {"G": G, "Gt": (Tp, Tj, Tx), "bad_row": bad_row}


def fsai_apply_device(bh, M, r, z):
    """z = G^T (G r) for M of fsai_setup_device: two products (csr_spmv_device), nothing sequential.  Returns z."""
    n = r.numel()
    y = csr_spmv_device(bh, n, n, M["G"], r)
    return csr_spmv_device(bh, n, n, M["Gt"], y, y=z)


def fsai_pcg_device(bh, A, b, tol=1e-8, maxiter=100, pattern=None):
    """Conjugate gradients for A x = b from x = 0, preconditioned with the factorised sparse approximate inverse of A on
    `pattern` (fsai_setup_device, fsai_apply_device; None: tril(A)), until ||r|| <= tol ||b|| or maxiter iterations.
    Returns (x, iterations, residual norms) as ilu0_pcg_device does."""
    M = fsai_setup_device(bh, A, pattern)
    return _pcg_with(bh, A, b, tol, maxiter, lambda r, z: fsai_apply_device(bh, M, r, z))
