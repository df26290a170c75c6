"""Graph traversals on top of semiring CSR x dense (dense.csr_spmm_semiring_device; include/bhsparse_hip.h, "semiring CSR x
dense"): breadth-first levels and single-source shortest paths, from k sources at once, with every array on the device --
a step is one call of the library, and what ends the loop is the call's count of changed elements, not a copy of the result.

Functions of a `facade.bhsparse` handle, as in dense.py.  The direction: row i pulls from its columns, so an entry A(i, j)
is an edge j -> i (of weight A(i, j)).  A symmetric matrix is an undirected graph; for a matrix of out-edge lists --
A(i, j) an edge i -> j -- transpose first (facade.csr_transpose, bhsparse.csr_transpose_device)."""
import numpy as np

from . import _lib
from .dense import csr_spmm_semiring_device
from .facade import BhsparseError, _device_csr, _handle


def _sources(sources, n):
    s = np.atleast_1d(np.asarray(sources, np.int64))
    if s.ndim != 1 or len(s) < 1:
        raise ValueError("sources: one vertex or a list of them")
    if s.min() < 0 or s.max() >= n:
        raise ValueError("sources: vertices of a graph of %d vertices" % n)
    return s


def _value_type(bh, A):
    import torch
    if A[2] is not None:
        return A[2].dtype
    return torch.float32 if bh._vdt == np.dtype(np.float32) else torch.float64


def bfs_levels_device(bh, n, A, sources):
    """Breadth-first levels of the n-vertex graph A = (rowPtr, colInd, val or None) (torch tensors on the handle's GPU; an
    entry A(i, j) is an edge j -> i; every entry is an edge unless its value is zero) from each of the k `sources`: an
    n x k tensor of the value type, 0 for a vertex that is not reached, depth + 1 otherwise (1 for the source itself).
    Each step is one OR_AND call under the complement of the levels -- visited vertices are skipped, rows all of whose k
    elements are visited are not walked -- into a fresh frontier; `changed` is the size of the new frontier and ends the
    loop at 0; the level update is a torch elementwise op.  At most n steps."""
    return _bfs(bh, n, A, sources)[0]


def _bfs(bh, n, A, sources):
    """(levels, steps, total device ms of the steps)"""
    import torch
    src = _sources(sources, n)
    k = len(src)
    Ap = A[0]
    dt = _value_type(bh, A)
    levels = torch.zeros((n, k), dtype=dt, device=Ap.device)
    cols = torch.arange(k, device=Ap.device)
    rows = torch.as_tensor(src, device=Ap.device)
    levels[rows, cols] = 1.0
    frontier = (levels != 0).to(dt)
    steps, ms = 0, 0.0
    for depth in range(1, n + 1):
        nxt = torch.zeros_like(frontier)                            # (elements the mask does not select are not written)
        nxt, changed = csr_spmm_semiring_device(bh, "or_and", n, n, A, frontier, nxt, mask=levels, accumulate=False,
                                                complement=True)
        steps, ms = steps + 1, ms + bh.spmv_ms
        if changed == 0:
            break
        levels += nxt * float(depth + 1)
        frontier = nxt
    return levels, steps, ms


def sssp_device(bh, n, A, sources, max_sweeps=None):
    """Shortest distances in the n-vertex graph A = (rowPtr, colInd, val) (an entry A(i, j) is an edge j -> i of that
    weight; val None: every edge weighs 1) from each of the k `sources`: an n x k tensor, +Inf for a vertex that is not
    reached.  Bellman-Ford in Jacobi form: D' = copy(D), one MIN_PLUS call with accumulation into D' (which reads D alone),
    swap; it stops when a sweep changes nothing.  Raises BhsparseError when a sweep still changes something after
    max_sweeps (default n, at least 1) of them: with n sweeps that is a cycle of negative weight.  ValueError for a source
    that is no vertex."""
    return _sssp(bh, n, A, sources, max_sweeps)[0]


def _sssp(bh, n, A, sources, max_sweeps):
    """(distances, sweeps, total device ms of the sweeps)"""
    import torch
    src = _sources(sources, n)
    k = len(src)
    Ap = A[0]
    dt = _value_type(bh, A)
    D = torch.full((n, k), float("inf"), dtype=dt, device=Ap.device)
    D[torch.as_tensor(src, device=Ap.device), torch.arange(k, device=Ap.device)] = 0.0
    limit = n if max_sweeps is None else int(max_sweeps)
    if limit < 1:
        raise ValueError("max_sweeps: at least one sweep")
    sweeps, ms = 0, 0.0
    for _ in range(limit):
        D2 = D.clone()
        D2, changed = csr_spmm_semiring_device(bh, "min_plus", n, n, A, D, D2, accumulate=True)
        sweeps, ms = sweeps + 1, ms + bh.spmv_ms
        D = D2
        if changed == 0:
            return D, sweeps, ms
    why = "a cycle of negative weight" if sweeps >= n else "max_sweeps is below the number of vertices: no verdict on a negative cycle"
    raise BhsparseError("sssp_device: still changing after %d sweeps (%s)" % (sweeps, why), _lib.BHS_ERR_INVALID_ARG)


def bfs_levels_csr(n, Ap, Aj, Ax, sources, value_dtype=np.float64, device=0):
    """Convenience: bfs_levels_device once on host CSR arrays.  Returns (levels value_dtype[n, k], info) with
    info["kernels"] (of the last step), info["steps"], info["ms"] (total device time of the steps)."""
    A = _device_csr(Ap, Aj, Ax, value_dtype, device)
    with _handle(value_dtype, device, None) as bh:
        out, steps, ms = _bfs(bh, n, A, sources)
        return out.cpu().numpy(), {"kernels": bh.kernel_stats(), "steps": steps, "ms": ms}


def sssp_csr(n, Ap, Aj, Ax, sources, max_sweeps=None, value_dtype=np.float64, device=0):
    """Convenience: sssp_device once on host CSR arrays.  Returns (distances value_dtype[n, k], info) with info["kernels"]
    (of the last sweep), info["steps"], info["ms"]."""
    A = _device_csr(Ap, Aj, Ax, value_dtype, device)
    with _handle(value_dtype, device, None) as bh:
        out, steps, ms = _sssp(bh, n, A, sources, max_sweeps)
        return out.cpu().numpy(), {"kernels": bh.kernel_stats(), "steps": steps, "ms": ms}

