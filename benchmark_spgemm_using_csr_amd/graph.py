"""Graph traversals on top of semiring CSR x dense (dense.csr_spmm_semiring_device; include/bhsparse_hip.h, "semiring CSR x
dense"): breadth-first levels and single-source shortest paths, from k sources at once, with every array on the device --
a step is one call of the library, and what ends the loop is the call's count of changed elements, not a copy of the result.

Functions of a `facade.bhsparse` handle, as in dense.py.  The direction: row i pulls from its columns, so an entry A(i, j)
is an edge j -> i (of weight A(i, j)).  A symmetric matrix is an undirected graph; for a matrix of out-edge lists --
A(i, j) an edge i -> j -- transpose first (facade.csr_transpose, bhsparse.csr_transpose_device).

The *_frontier_* functions give the same results and choose a direction per step: a step whose frontier is small goes by
push (dense.csr_push_semiring_device; "sparse frontier x CSR"), which reads the out-edges of the frontier's vertices and
nothing else, a step whose frontier is large by the pull call above.  On a graph of high diameter -- a road network, a mesh,
a banded matrix -- that is the difference between touching every edge once and touching every edge once per level.

components_* answer which vertices belong together, for all components at once and whatever the direction of the entries
(bhs_csr_components_device; "connected components"): the passes grow like the logarithm of the diameter, not like the
diameter.

scc_* answer the question about the DIRECTION of the entries: the strongly connected components (bhs_csr_scc_device;
"strongly connected components"), by trimming and forward-backward rounds; condensation_device is the DAG of the SCCs,
largest_scc_csr the submatrix of the largest one.

kcore_* give the core number of every vertex of an undirected graph and the round of the synchronous peeling in which it
leaves (bhs_csr_kcore_device; "k-core decomposition"): the degeneracy, a degeneracy ordering, the k-core as a submatrix;
ktruss_device is the k-truss on top of the masked PLUS_PAIR product and the entry selection.

sssp_delta_* are the shortest paths in ONE device-resident call (bhs_csr_sssp_device; "shortest paths"): delta-stepping on a
queue over the OUT-EDGE matrix -- G(i, j) an edge i -> j, the push call's orientation, no transpose and no dense frontier --
with distances that are the same bits as sssp_device's and, optionally, parents: path_from_parents walks them back to a
source, bfs_levels_queue_device is the unit-weight case.

betweenness_* say which vertices the shortest paths run through (bhs_csr_betweenness_device; "betweenness centrality"):
Brandes' algorithm a source after the other over the out-edges and the in-edges, every sum with one writer and a fixed
order, so that the doubles are a function of the input; betweenness_sample_csr estimates it from k pivots, and
closeness_device reads the classic and the harmonic closeness off the levels of single-source calls.

spanning_forest_* give the minimum or maximum spanning forest of the weighted graph (bhs_csr_spanning_forest_device;
"spanning forest"), unique for any input, in at most log2 n Boruvka rounds; single_linkage_device cuts its heaviest edges
and calls the components on the rest."""
import ctypes as C

import numpy as np

from . import _lib
from .dense import csr_push_semiring_device, csr_spmm_semiring_device
from .facade import BhsparseError, _alloc, _check, _device_csr, _handle, _host, _ptr, extract_csr


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


# ---------------------------------------------------------------- a direction per step
# The frontier size at which one OR_AND push call stops being cheaper than the pull call under the matching complement
# mask, as n / frontier vertices (tools/push_case.py, profiles/push_case.md).
PUSH_BELOW = 10


def _by_push(nf, n, push_below):
    """does a frontier of nf vertices go by push: at most n / push_below of them (0: never, inf: always)"""
    return push_below > 0 and (push_below == float("inf") or nf * push_below <= n)


def _out_edges(bh, n, A, At):
    """the out-edge CSR: given, or A's transpose by the handle (once)"""
    if At is not None:
        return At
    Tp, Tj, Tx, _ = bh.csr_transpose_device(n, n, A, values=A[2] is not None)
    return Tp, Tj, Tx


def _rows_with(T):
    """the rows of the n x k tensor T that hold a non-zero (a True), ascending: int32"""
    import torch
    return torch.nonzero(T.any(dim=1)).flatten().to(torch.int32)


def bfs_levels_frontier_device(bh, n, A, sources, At=None, push_below=None):
    """bfs_levels_device with a direction per level: the same n x k tensor of levels (A(i, j) is an edge j -> i; At =
    (rowPtr, colInd, val or None) is the CSR of out-edges, A's transpose, computed once with the handle's transpose when
    None; for a symmetric A pass At=A).  A level whose frontier has at most n / push_below vertices goes by push
    (push_below None: PUSH_BELOW, the measured crossover; 0: never push; inf: always), the others by the pull call of
    bfs_levels_device.  A push level is one library call and no pass over all n vertices: the call returns the rows it
    changed, and the levels and the next frontier's values are read and written at those rows only."""
    return _bfs_frontier(bh, n, A, sources, At, push_below)[0]


def _bfs_frontier(bh, n, A, sources, At=None, push_below=None):
    """(levels, steps, total device ms of the steps, steps that went by push)"""
    import torch
    push_below = PUSH_BELOW if push_below is None else push_below
    src = _sources(sources, n)
    k = len(src)
    dev = A[0].device
    dt = _value_type(bh, A)
    levels = torch.zeros((n, k), dtype=dt, device=dev)
    levels[torch.as_tensor(src, device=dev), torch.arange(k, device=dev)] = 1.0
    # the frontier: a list of vertices, ascending, with their nf x k rows of 0 / 1 -- or, idx None, the dense n x k tensor
    idx = torch.as_tensor(np.unique(src), device=dev).to(torch.int32)
    F = levels.index_select(0, idx.to(torch.int64))
    G = None
    reach = None                                                        # push levels' Y: all zero between the levels
    steps, ms, pushes = 0, 0.0, 0
    for depth in range(1, n + 1):
        if idx is not None and _by_push(idx.numel(), n, push_below):
            if G is None:
                G = _out_edges(bh, n, A, At)
            if reach is None:
                reach = torch.zeros((n, k), dtype=dt, device=dev)
            _, changed, nxt = csr_push_semiring_device(bh, "or_and", n, n, G, idx, F, reach, mask=levels, complement=True)
            steps, ms, pushes = steps + 1, ms + bh.spmv_ms, pushes + 1
            if changed == 0:
                break
            at = nxt.to(torch.int64)
            F = reach.index_select(0, at)
            levels.index_add_(0, at, F * float(depth + 1))              # (the mask let through unvisited elements only: 0 + level)
            reach.index_fill_(0, at, 0.0)
            idx = nxt
        else:
            frontier = F if idx is None else torch.zeros((n, k), dtype=dt, device=dev).index_copy_(0, idx.to(torch.int64), F)
            nxt = torch.zeros_like(frontier)
            nxt, changed = csr_spmm_semiring_device(bh, "or_and", n, n, A, frontier, nxt, mask=levels, accumulate=False,
                                                    complement=True)
            steps, ms = steps + 1, ms + bh.spmv_ms
            if changed == 0:
                break
            levels += nxt * float(depth + 1)
            idx, F = None, nxt                                          # a dense frontier ...
            if _by_push((changed + k - 1) // k, n, push_below):         # ... unless it may be small enough: then its list
                rows = _rows_with(nxt)
                if _by_push(rows.numel(), n, push_below):
                    idx, F = rows, nxt.index_select(0, rows.to(torch.int64))
    return levels, steps, ms, pushes


def sssp_frontier_device(bh, n, A, sources, At=None, max_rounds=None, push_below=None):
    """sssp_device with a direction per round: the same n x k tensor of distances (At, push_below: as
    bfs_levels_frontier_device).  Round-synchronous Bellman-Ford on a frontier: the vertices whose distance changed in the
    last round -- the sources at first -- relax their out-edges.  A push round gathers F, a snapshot of D at the frontier,
    and one MIN_PLUS push call takes the minima into D in place and returns the rows it changed: the next frontier.  A pull
    round is sssp_device's Jacobi sweep, and its frontier the rows the sweep changed.

    The distances equal sssp_device's bit for bit.  Floating add is monotone (a <= b gives a + w <= b + w after rounding)
    and min is exact, so a vertex's distance only ever takes values that are the left-to-right sum of the weights along
    some path from the source, and relaxing an edge from a vertex whose distance has not changed since it last relaxed
    changes nothing.  Both loops therefore stop at the same point: the least fixed point of D = min(D, D (min.+) A), the
    minimum over the paths of their left-to-right sums -- whatever the order of the relaxations, and with the frontier's
    rounds even after the same number of steps as the sweeps.

    Raises BhsparseError when a round still changes something after max_rounds (default n, at least 1) of them: with n
    rounds that is a cycle of negative weight.  ValueError for a source that is no vertex."""
    return _sssp_frontier(bh, n, A, sources, At, max_rounds, push_below)[0]


def _sssp_frontier(bh, n, A, sources, At=None, max_rounds=None, push_below=None):
    """(distances, rounds, total device ms of the rounds, rounds that went by push)"""
    import torch
    push_below = PUSH_BELOW if push_below is None else push_below
    src = _sources(sources, n)
    k = len(src)
    dev = A[0].device
    dt = _value_type(bh, A)
    D = torch.full((n, k), float("inf"), dtype=dt, device=dev)
    D[torch.as_tensor(src, device=dev), torch.arange(k, device=dev)] = 0.0
    limit = n if max_rounds is None else int(max_rounds)
    if limit < 1:
        raise ValueError("max_rounds: at least one round")
    idx = torch.as_tensor(np.unique(src), device=dev).to(torch.int32)   # None: everything relaxes (a pull round)
    G = None
    rounds, ms, pushes = 0, 0.0, 0
    for _ in range(limit):
        if idx is not None and _by_push(idx.numel(), n, push_below):
            if G is None:
                G = _out_edges(bh, n, A, At)
            F = D.index_select(0, idx.to(torch.int64))                  # the snapshot: a round reads last round's distances
            _, changed, idx = csr_push_semiring_device(bh, "min_plus", n, n, G, idx, F, D)
            rounds, ms, pushes = rounds + 1, ms + bh.spmv_ms, pushes + 1
        else:
            D2 = D.clone()
            D2, changed = csr_spmm_semiring_device(bh, "min_plus", n, n, A, D, D2, accumulate=True)
            rounds, ms = rounds + 1, ms + bh.spmv_ms
            idx = _rows_with(D2 != D) if changed and _by_push((changed + k - 1) // k, n, push_below) else None
            D = D2
        if changed == 0:
            return D, rounds, ms, pushes
    why = "a cycle of negative weight" if rounds >= n else "max_rounds is below the number of vertices: no verdict on a negative cycle"
    raise BhsparseError("sssp_frontier_device: still changing after %d rounds (%s)" % (rounds, why), _lib.BHS_ERR_INVALID_ARG)


# ---------------------------------------------------------------- connected components
def components_raw_device(bh, n, nnz, dAp, dAj, flags, root, comp, size):
    """bhs_csr_components_device on caller-given arrays, the C arguments in order (comp and size may be None): the status
    code; sets bh.components_ncomp, bh.components_passes (the passes depend on timing) and bh.components_ms on success
    only."""
    return bh._counted("bhs_csr_components_device", "components", "ncomp", "passes", int(n), int(nnz), _ptr(dAp), _ptr(dAj),
                       int(flags), _ptr(root), _ptr(comp), _ptr(size))


def components_device(bh, n, A):
    """The connected components of the n-vertex pattern A = (rowPtr, colInd[, anything]), torch tensors on the handle's GPU:
    i and j are joined where A stores (i, j) or (j, i), so A need not be symmetric; values are not taken.  Returns (root
    int32[n], comp int32[n], sizes int32[ncomp]) as device tensors: the smallest vertex of i's component, the component's
    number by ascending root, and the components' sizes.  bh.components_ncomp, bh.components_passes and bh.components_ms
    hold the count, the passes and the device time.  Raises BhsparseError on failure."""
    import torch
    Ap, Aj = A[0], A[1]
    root, comp, size = (_alloc(n, torch.int32, Ap.device) for _ in range(3))
    torch.cuda.synchronize()                           # the library works on its own stream (see facade.initData_device)
    _check(components_raw_device(bh, n, Aj.numel(), Ap, Aj if Aj.numel() else None, 0, root, comp, size),
           "bhs_csr_components_device")
    return root[:n], comp[:n], size[:bh.components_ncomp]


def component_lists_device(bh, n, comp, ncomp):
    """The vertices by (component, index) from components_device's comp: (order int32[n], compPtr int32[ncomp + 1]) as device
    tensors, component c is order[compPtr[c] : compPtr[c + 1]].  The handle's stable transpose of the n x ncomp membership
    pattern (rowPtr = 0 .. n, colInd = comp, no values): T's columns are the order, T's row pointer the offsets."""
    import torch
    rowptr = torch.arange(n + 1, dtype=torch.int32, device=comp.device)
    Tp, Tj, _, _ = bh.csr_transpose_device(n, ncomp, (rowptr, comp, None), values=False)
    return Tj, Tp


def components_csr(n, Ap, Aj, device=0):
    """Convenience: components_device once on host CSR arrays.  Returns numpy (root int32[n], comp int32[n], sizes
    int32[ncomp])."""
    A = _device_csr(Ap, Aj, None, np.float64, device)
    with _handle(np.float64, device, None) as bh:
        return _host(*components_device(bh, n, A))


def largest_component_csr(n, Ap, Aj, Ax, value_dtype=np.float64, device=0):
    """Convenience: the largest connected component of the n x n matrix (Ap, Aj, Ax) on host CSR arrays -- of the greatest
    size, ties to the smaller root.  Returns (vertices int32[size] ascending, (Zp, Zj, Zx)): Z = A(vertices, vertices)
    through facade.extract_csr."""
    _, comp, sizes = components_csr(n, Ap, Aj, device=device)
    return _largest_csr(n, Ap, Aj, Ax, comp, sizes, value_dtype, device)


def _largest_csr(n, Ap, Aj, Ax, comp, sizes, value_dtype, device):
    """(vertices, (Zp, Zj, Zx)) of the component of greatest size, numbered as comp and sizes have them"""
    if n == 0:
        return np.zeros(0, np.int32), (np.zeros(1, np.int32), np.zeros(0, np.int32), np.zeros(0, value_dtype))
    c = int(np.argmax(sizes))                                         # (the first of equal sizes: components are numbered by ascending root)
    vertices = np.flatnonzero(comp == c).astype(np.int32)
    Zp, Zj, Zx, _ = extract_csr(n, n, Ap, Aj, Ax, rows=vertices, cols=vertices, value_dtype=value_dtype, device=device)
    return vertices, (Zp, Zj, Zx)


# ---------------------------------------------------------------- strongly connected components
def scc_raw_device(bh, n, nnz, dAp, dAj, flags, root, comp, size):
    """bhs_csr_scc_device on caller-given arrays, the C arguments in order (comp and size may be None): the status code,
    BHS_ERR_NOT_READY without a platform; sets bh.scc_nscc, bh.scc_rounds (a function of the pattern), bh.scc_passes (the
    passes depend on timing) and bh.scc_ms on success only."""
    if bh._h is None:
        return _lib.BHS_ERR_NOT_READY
    nscc, rounds, passes, ms = C.c_int(0), C.c_int(0), C.c_int(0), C.c_double(0)
    err = bh._lib.bhs_csr_scc_device(bh._h, int(n), int(nnz), _ptr(dAp), _ptr(dAj), int(flags), _ptr(root), _ptr(comp), _ptr(size),
                                     C.byref(nscc), C.byref(rounds), C.byref(passes), C.byref(ms))
    if err == _lib.BHS_SUCCESS:
        bh.scc_nscc, bh.scc_rounds, bh.scc_passes, bh.scc_ms = int(nscc.value), int(rounds.value), int(passes.value), float(ms.value)
    return err


def scc_device(bh, n, A):
    """The strongly connected components of the n-vertex pattern A = (rowPtr, colInd[, anything]), torch tensors on the
    handle's GPU: an entry (i, j) is a directed edge (which way it points does not matter: a graph and its reverse have the
    same SCCs); values are not taken.  Returns (root int32[n], comp int32[n], sizes int32[nscc]) as device tensors: the
    smallest vertex of i's SCC, the SCC's number by ascending root, and the SCCs' sizes.  bh.scc_nscc, bh.scc_rounds,
    bh.scc_passes and bh.scc_ms hold the count, the rounds, the passes and the device time.  Raises BhsparseError on failure."""
    import torch
    Ap, Aj = A[0], A[1]
    root, comp, size = (_alloc(n, torch.int32, Ap.device) for _ in range(3))
    torch.cuda.synchronize()                           # the library works on its own stream (see facade.initData_device)
    _check(scc_raw_device(bh, n, Aj.numel(), Ap, Aj if Aj.numel() else None, 0, root, comp, size), "bhs_csr_scc_device")
    return root[:n], comp[:n], size[:bh.scc_nscc]


def scc_csr(n, Ap, Aj, device=0):
    """Convenience: scc_device once on host CSR arrays.  Returns numpy (root int32[n], comp int32[n], sizes int32[nscc])."""
    A = _device_csr(Ap, Aj, None, np.float64, device)
    with _handle(np.float64, device, None) as bh:
        return _host(*scc_device(bh, n, A))


def condensation_device(bh, n, A, comp, nscc):
    """The condensation of the n-vertex pattern A = (rowPtr, colInd[, anything]) under scc_device's comp: the DAG of the
    SCCs as a device CSR (rowPtr int32[nscc + 1], colInd, val) of nscc x nscc.  Its triplets are (comp[i], comp[j]) over the
    entries (i, j) whose ends have different numbers, assembled by assemble.coo_assemble_device with "sum" on values of 1
    in the handle's type: a value counts the entries of A between two SCCs.  The vertex lists of the SCCs are
    component_lists_device(bh, n, comp, nscc)."""
    import torch
    from .assemble import coo_assemble_device
    Ap, Aj = A[0], A[1]
    lens = (Ap[1:n + 1] - Ap[:n]).to(torch.int64)
    rows = torch.repeat_interleave(torch.arange(n, dtype=torch.int64, device=Ap.device), lens, output_size=Aj.numel())
    ci, cj = comp[rows], comp[Aj.to(torch.int64)]
    keep = ci != cj
    ci, cj = ci[keep].contiguous(), cj[keep].contiguous()
    vals = torch.ones(ci.numel(), dtype=torch.float32 if bh._vdt == np.dtype(np.float32) else torch.float64, device=Ap.device)
    return coo_assemble_device(bh, nscc, nscc, ci, cj, vals, "sum")


def largest_scc_csr(n, Ap, Aj, Ax, value_dtype=np.float64, device=0):
    """Convenience: the largest strongly connected component of the n x n matrix (Ap, Aj, Ax) on host CSR arrays -- of the
    greatest size, ties to the smaller root.  Returns (vertices int32[size] ascending, (Zp, Zj, Zx)): Z = A(vertices,
    vertices) through facade.extract_csr."""
    _, comp, sizes = scc_csr(n, Ap, Aj, device=device)
    return _largest_csr(n, Ap, Aj, Ax, comp, sizes, value_dtype, device)


# ---------------------------------------------------------------- shortest paths in one call
def sssp_delta_raw_device(bh, n, nnz, dGp, dGj, dGx, nsrc, dsources, delta, flags, dist, parent):
    """bhs_csr_sssp_device on caller-given arrays, the C arguments in order (dGx and parent may be None): the status code,
    BHS_ERR_NOT_READY without a platform; sets bh.sssp_reached, bh.sssp_passes (functions of the input and delta) and
    bh.sssp_ms on success only.  bh.get_info("sssp_buckets"), ("sssp_loose") and ("sssp_work_passes") read the rest."""
    return bh._counted("bhs_csr_sssp_device", "sssp", "reached", "passes", int(n), int(nnz), _ptr(dGp), _ptr(dGj), _ptr(dGx),
                       int(nsrc), _ptr(dsources), C.c_double(float(delta)), int(flags), _ptr(dist), _ptr(parent))


def sssp_delta_device(bh, n, G, sources, delta=None, parents=False):
    """Shortest paths of the n-vertex graph G = (rowPtr, colInd, val or None) -- torch tensors on the handle's GPU, G(i, j) an
    edge i -> j of weight val, not negative (1 without val) -- from the nearest of `sources`, in one call of the library.
    Returns (dist[, parent], reached, passes): dist of the value type, +Inf where not reached; parent int32 (-1 a source or
    not reached, -2 reached only over edges that gain nothing; every other parent has a strictly smaller distance);
    reached the vertices with a finite distance; passes the passes launched.  delta is the bucket width and changes the
    work, never the result; None: +Inf, one bucket -- the rule profiles/sssp_case.md's table gives (its "inf" rows: a pass
    costs four launches whatever it holds, and on every measured input the fewest passes won by up to 50 ms or lost by less
    than 1 ms; narrower buckets are for weights spread over many decades on a graph too large for the re-relaxations,
    which that table does not hold).  bh.sssp_ms holds the device time.  Raises BhsparseError on failure -- BHS_ERR_INVALID_ARG for a negative or NaN weight; ValueError for a
    source that is no vertex."""
    import torch
    Gp, Gj, Gx = G
    src = torch.as_tensor(_sources(sources, n).astype(np.int32), device=Gp.device)
    if delta is None:
        delta = float("inf")
    dist = _alloc(n, _value_type(bh, G), Gp.device)
    parent = _alloc(n, torch.int32, Gp.device) if parents else None
    torch.cuda.synchronize()                           # the library works on its own stream (see facade.initData_device)
    _check(sssp_delta_raw_device(bh, n, Gj.numel(), Gp, Gj if Gj.numel() else None, Gx if Gj.numel() else None, src.numel(), src,
                                 delta, 0, dist, parent), "bhs_csr_sssp_device")
    out = (dist[:n], parent[:n]) if parents else (dist[:n],)
    return out + (bh.sssp_reached, bh.sssp_passes)


def sssp_delta_csr(n, Gp, Gj, Gx, sources, delta=None, parents=False, value_dtype=np.float64, device=0):
    """Convenience: sssp_delta_device once on host CSR arrays (out-edges).  Returns (dist[, parent], info), the arrays as
    numpy, with info["reached"], info["passes"], info["buckets"], info["loose"], info["ms"], info["kernels"]."""
    G = _device_csr(Gp, Gj, Gx, value_dtype, device)
    with _handle(value_dtype, device, None) as bh:
        *arrays, reached, passes = sssp_delta_device(bh, n, G, sources, delta, parents)
        info = {"reached": reached, "passes": passes, "buckets": bh.get_info("sssp_buckets"), "loose": bh.get_info("sssp_loose"),
                "ms": bh.sssp_ms, "kernels": bh.kernel_stats()}
        return _host(*arrays) + (info,)


def path_from_parents(parent, target):
    """The vertices from a source to `target` along sssp_delta_*'s parents (a host array): [source, ..., target]; every step
    goes to a strictly smaller distance, so the walk ends.  A target with parent -1 gives [target]: a source, or a vertex that
    is not reached -- its distance tells which.  Raises ValueError where the walk meets a vertex without a parent edge (-2)."""
    parent = np.asarray(parent)
    out = [int(target)]
    for _ in range(len(parent)):
        p = int(parent[out[-1]])
        if p == -1:
            return out[::-1]
        if p < 0 or p >= len(parent):
            raise ValueError("path_from_parents: vertex %d is reached over edges that gain nothing only (parent %d)" % (out[-1], p))
        out.append(p)
    raise ValueError("path_from_parents: the parents do not lead to a source")


def bfs_levels_queue_device(bh, n, G, sources):
    """Breadth-first levels by the queue: sssp_delta_device on the pattern of G = (rowPtr, colInd[, anything]) with unit
    weights and delta = 1, so that a pass is a level.  int32[n]: depth + 1, 0 where not reached (bfs_levels_device's
    numbering, for out-edges)."""
    import torch
    dist, _, _ = sssp_delta_device(bh, n, (G[0], G[1], None), sources, delta=1.0)
    return torch.where(torch.isinf(dist), torch.zeros_like(dist), dist + 1.0).to(torch.int32)


# ---------------------------------------------------------------- betweenness centrality
def betweenness_raw_device(bh, n, nnzG, dGp, dGj, nnzT, dTp, dTj, nsrc, dsources, flags, bc, level, sigma):
    """bhs_csr_betweenness_device on caller-given arrays, the C arguments in order (level and sigma may be None): the status
    code, BHS_ERR_NOT_READY without a platform; sets bh.bc_reached, bh.bc_passes (functions of the input) and bh.bc_ms on
    success only.  bh.get_info("bc_levels"), ("bc_overflow") and ("bc_work_passes") read the rest."""
    return bh._counted("bhs_csr_betweenness_device", "bc", "reached", "passes", int(n), int(nnzG), _ptr(dGp), _ptr(dGj), int(nnzT),
                       _ptr(dTp), _ptr(dTj), int(nsrc), _ptr(dsources), int(flags), _ptr(bc), _ptr(level), _ptr(sigma))


def betweenness_device(bh, n, G, sources=None, Gt=None, accumulate=None, last=False):
    """The betweenness of the n-vertex graph G = (rowPtr, colInd[, anything]) -- torch tensors on the handle's GPU, G(i, j) an
    edge i -> j; values are not taken -- summed over `sources` in list order (None: all vertices, the exact centrality), in
    one call of the library.  Gt holds the in-edges: None computes the transpose once with bh.csr_transpose_device; Gt = G
    says the graph is undirected (every edge stored both ways).  accumulate: a float64 tensor of n sums that is added to in
    place and returned, so that chained calls give the bits of one call; None: a new one, from zero.
    Returns (bc[, level, sigma], reached, passes): bc float64, UNSCALED -- every ordered pair (s, t) counts, so an
    undirected graph's values are twice networkx's; with last=True level (int32, -1 where not reached) and sigma (float64
    path counts) of the last source; reached summed over the sources; passes the forward passes launched.  bh.bc_ms holds the
    device time; profiles/bc_case.md says what it costs and where it loses.  Raises BhsparseError on failure; ValueError for
    a source that is no vertex."""
    import torch
    Gp, Gj = G[0], G[1]
    dev = Gp.device
    src = np.arange(n, dtype=np.int32) if sources is None else _sources(sources, n).astype(np.int32)
    src = torch.as_tensor(src, device=dev)
    if Gt is None:
        Tp, Tj, _, _ = bh.csr_transpose_device(n, n, (Gp, Gj, None), values=False)
    else:
        Tp, Tj = Gt[0], Gt[1]
    if accumulate is not None and (accumulate.dtype != torch.float64 or accumulate.numel() < n or not accumulate.is_contiguous()):
        raise ValueError("accumulate: a contiguous float64 tensor of n sums")
    bc = _alloc(n, torch.float64, dev) if accumulate is None else accumulate
    level = _alloc(n, torch.int32, dev) if last else None
    sigma = _alloc(n, torch.float64, dev) if last else None
    torch.cuda.synchronize()                           # the library works on its own stream (see facade.initData_device)
    _check(betweenness_raw_device(bh, n, Gj.numel(), Gp, Gj if Gj.numel() else None, Tj.numel(), Tp, Tj if Tj.numel() else None,
                                  src.numel(), src if n else None, 0 if accumulate is None else _lib.BHS_BC_ACCUMULATE,
                                  bc if n else None, level, sigma), "bhs_csr_betweenness_device")
    out = (bc[:n], level[:n], sigma[:n]) if last else (bc[:n],)
    return out + (bh.bc_reached, bh.bc_passes)


def _bc_scaled(bc, n, directed, normalized, factor=1.0):
    """networkx's conventions: an undirected graph's pairs count once, normalised by the (n - 1)(n - 2) ordered pairs"""
    if normalized:
        return bc * (factor / ((n - 1) * (n - 2))) if n > 2 else bc * 0.0
    return bc * (factor if directed else 0.5 * factor)


def _betweenness_raw_csr(n, Gp, Gj, sources, directed, device):
    """(raw, info): the UNSCALED sums of betweenness_device on host CSR arrays -- every ordered pair counts -- and the counts"""
    G = _device_csr(Gp, Gj, None, np.float64, device)
    with _handle(np.float64, device, None) as bh:
        bc, reached, passes = betweenness_device(bh, n, G, sources, None if directed else G)
        info = {"reached": reached, "passes": passes, "levels": bh.get_info("bc_levels"), "overflow": bh.get_info("bc_overflow"),
                "ms": bh.bc_ms, "kernels": bh.kernel_stats()}
        return _host(bc)[0], info


def betweenness_csr(n, Gp, Gj, sources=None, directed=True, normalized=False, device=0):
    """Convenience: betweenness_device once on host CSR arrays (out-edges; an undirected graph stores every edge both ways and
    says directed=False, which halves).  Returns (bc float64[n], info) with networkx's betweenness_centrality conventions --
    betweenness_centrality_subset's where sources is a list -- and info["reached"], info["passes"], info["levels"],
    info["overflow"], info["ms"], info["kernels"]."""
    raw, info = _betweenness_raw_csr(n, Gp, Gj, sources, directed, device)
    return _bc_scaled(raw, n, directed, normalized), info


def betweenness_sample_csr(n, Gp, Gj, k, seed=0, directed=True, normalized=False, device=0):
    """The Brandes-Pich estimate: the dependencies of k pivots drawn without replacement by numpy's default_rng(seed), scaled
    by n / k and then as betweenness_csr scales -- the raw sums are scaled ONCE, so with k = n the estimate is
    betweenness_csr's value up to the order of the sources and the rounding of n / k = 1.  Returns (bc, info) as betweenness_csr
    does, with info["pivots"]."""
    if not 1 <= k <= n:
        raise ValueError("k: between 1 and n pivots")
    pivots = np.sort(np.random.default_rng(seed).choice(n, int(k), replace=False))
    raw, info = _betweenness_raw_csr(n, Gp, Gj, pivots, directed, device)
    info["pivots"] = pivots
    return _bc_scaled(raw, n, directed, normalized, n / float(k)), info


def closeness_device(bh, n, G, sources):
    """The closeness of every vertex of `sources` over the out-edges of G, from the levels of single-source calls (the call's
    d_level; its sums are not used).  Returns (classic, harmonic), float64 numpy arrays in the order of the sources: classic
    is Wasserman and Faust's (r - 1) / (n - 1) * (r - 1) / sum of the distances to the r - 1 vertices reached, 0 where none
    is; harmonic the sum of 1 / distance over them, added level by level in ascending order.  Every call still pulls the
    path counts and runs the backward sweep, which closeness does not need: where the levels alone are wanted,
    bfs_levels_queue_device gives them at 0.75 to 0.9 of the cost (profiles/bc_case.md, "BFS calls")."""
    import torch
    src = _sources(sources, n)
    Gt = (G[0], G[1])                                  # the path counts are not read: any in-edges do
    bc = torch.zeros(max(n, 1), dtype=torch.float64, device=G[0].device)
    classic, harmonic = np.zeros(len(src)), np.zeros(len(src))
    for k, s in enumerate(src):
        _, level, _, reached, _ = betweenness_device(bh, n, G, [int(s)], Gt, bc, last=True)
        per = torch.bincount(level[level > 0].to(torch.int64)).cpu().numpy()       # vertices at every distance
        total = sum(int(d) * int(c) for d, c in enumerate(per))
        if total:
            classic[k] = (reached - 1) / (n - 1) * (reached - 1) / total
            for d in range(1, len(per)):
                harmonic[k] += per[d] / d
    return classic, harmonic


# ---------------------------------------------------------------- k-core and k-truss
def kcore_raw_device(bh, n, nnz, dAp, dAj, flags, core, round):
    """bhs_csr_kcore_device on caller-given arrays, the C arguments in order (round may be None): the status code,
    BHS_ERR_NOT_READY without a platform; sets bh.kcore_kmax, bh.kcore_rounds (functions of the pattern) and bh.kcore_ms on
    success only."""
    return bh._counted("bhs_csr_kcore_device", "kcore", "kmax", "rounds", int(n), int(nnz), _ptr(dAp), _ptr(dAj), int(flags),
                       _ptr(core), _ptr(round))


def kcore_device(bh, n, A):
    """The k-core decomposition of the n-vertex pattern A = (rowPtr, colInd[, anything]), torch tensors on the handle's GPU:
    rows strictly ascending, structurally symmetric (ordering.symmetric_pattern_device and assemble.canonical_csr_device make
    one of any matrix); the diagonal is ignored, values are not taken.  Returns (core int32[n], round int32[n], kmax,
    rounds): every vertex's core number, the round of the synchronous peeling in which it leaves (from 1), the degeneracy and
    the number of rounds.  bh.kcore_ms holds the device time.  Raises BhsparseError on failure -- BHS_ERR_INVALID_ARG for a
    pattern that is not ascending or not symmetric."""
    import torch
    Ap, Aj = A[0], A[1]
    core, rnd = (_alloc(n, torch.int32, Ap.device) for _ in range(2))
    torch.cuda.synchronize()                           # the library works on its own stream (see facade.initData_device)
    _check(kcore_raw_device(bh, n, Aj.numel(), Ap, Aj if Aj.numel() else None, 0, core, rnd), "bhs_csr_kcore_device")
    return core[:n], rnd[:n], bh.kcore_kmax, bh.kcore_rounds


def kcore_csr(n, Ap, Aj, device=0):
    """Convenience: kcore_device once on host CSR arrays.  Returns (core int32[n], round int32[n], kmax, rounds), the arrays
    as numpy."""
    A = _device_csr(Ap, Aj, None, np.float64, device)
    with _handle(np.float64, device, None) as bh:
        core, rnd, kmax, rounds = kcore_device(bh, n, A)
        return _host(core, rnd) + (kmax, rounds)


def degeneracy_order_device(round):
    """The vertices by (round, index) from kcore_device's round, through torch's stable sort: int32[n] on the device.  Every
    vertex has at most core[v] <= kmax neighbours behind it in this order: those of its own round and of later ones were
    present when it left with a degree of at most its core number."""
    import torch
    return torch.sort(round, stable=True)[1].to(torch.int32)


def kcore_subgraph_device(bh, n, A, core, k):
    """The k-core of A = (rowPtr, colInd, val or None) from kcore_device's core: (V int32 ascending, (Zp, Zj, Zx)) with
    V = {v: core[v] >= k} and Z = A(V, V) through the handle's extraction (Zx None where A has no values).  Off the diagonal
    every row of Z has at least k entries."""
    import torch
    V = torch.nonzero(core >= k).flatten().to(torch.int32)
    if V.numel() == 0:
        Ax = A[2] if len(A) > 2 else None
        return V, (torch.zeros(1, dtype=torch.int32, device=core.device), torch.zeros(0, dtype=torch.int32, device=core.device),
                   None if Ax is None else Ax[:0])
    Zp, Zj, Zx, _ = bh.csr_extract_device(n, n, (A[0], A[1], A[2] if len(A) > 2 else None), rows=V, cols=V)
    return V, (Zp, Zj, Zx)


def ktruss_device(bh, n, A, k):
    """The k-truss of the n-vertex pattern A = (rowPtr, colInd[, anything]) (rows strictly ascending, structurally
    symmetric; the diagonal is dropped first): the maximal subgraph T in which every edge lies in at least k - 2 triangles
    of T.  Returns ((rowPtr, colInd, support), iterations): T as a symmetric device CSR whose values, in the handle's type,
    are the supports -- the triangles of T an edge lies in.  An iteration is one masked PLUS_PAIR product T.T on T's own
    pattern (bhsparse.spgemm_semiring_masked_device: the common neighbours of an edge's ends) and one entry selection that
    keeps support > k - 2.5 (bhsparse.csr_select_device; supports are exact small integers); it is repeated until nnz stops
    falling, so the last product's values are the supports inside T.  k <= 2 keeps every edge: one product."""
    import torch
    dt = torch.float32 if bh._vdt == np.dtype(np.float32) else torch.float64
    off = _lib.Select(flags=_lib.BHS_SEL_DROP_DIAG)
    Tp, Tj, _ = bh.csr_select_device(n, n, (A[0], A[1], None), off, values=False)
    keep = _lib.Select(flags=_lib.BHS_SEL_DROP_DIAG | _lib.BHS_SEL_ABS, abs_tol=float(k) - 2.5) if k > 2 else None
    iterations = 0
    while True:
        nnz = Tj.numel()
        if nnz == 0:
            return (Tp, Tj, torch.zeros(0, dtype=dt, device=Tp.device)), iterations
        ones = torch.ones(nnz, dtype=dt, device=Tp.device)
        support = torch.zeros(nnz, dtype=dt, device=Tp.device)
        _check(bh.initData_device(n, n, n, nnz, ones, Tp, Tj, nnz, ones, Tp, Tj), "initData_device")
        try:
            _check(bh.spgemm_semiring_masked_device(_lib.BHS_SR_PLUS_PAIR, Tp, Tj, nnz, support), "bhs_spgemm_semiring_masked_device")
        finally:
            bh.free_mem()
        iterations += 1
        if keep is None:
            return (Tp, Tj, support), iterations
        Zp, Zj, _ = bh.csr_select_device(n, n, (Tp, Tj, support), keep, values=False)
        if Zj.numel() == nnz:
            return (Tp, Tj, support), iterations
        Tp, Tj = Zp, Zj


def ktruss_csr(n, Ap, Aj, k, value_dtype=np.float64, device=0):
    """Convenience: ktruss_device once on host CSR arrays.  Returns ((Tp, Tj, support) as numpy, iterations)."""
    A = _device_csr(Ap, Aj, None, value_dtype, device)
    with _handle(value_dtype, device, None) as bh:
        T, iterations = ktruss_device(bh, n, A, k)
        return _host(*T), iterations


# ---------------------------------------------------------------- spanning forest
def spanning_forest_raw_device(bh, n, nnzA, d_rowPtrA, d_colIndA, d_valA, flags, d_label, d_edgeLo, d_edgeHi, d_edgeVal):
    """bhs_csr_spanning_forest_device on caller-given arrays, the C arguments in order (d_valA and d_edgeVal may be None): the
    status code; sets bh.forest_nedges, bh.forest_rounds and bh.forest_ms on success only."""
    return bh._counted("bhs_csr_spanning_forest_device", "forest", "nedges", "rounds", int(n), int(nnzA), _ptr(d_rowPtrA),
                       _ptr(d_colIndA), _ptr(d_valA), int(flags), _ptr(d_label), _ptr(d_edgeLo), _ptr(d_edgeHi), _ptr(d_edgeVal))


def spanning_forest_device(bh, n, A, maximum=False, absolute=False):
    """The minimum spanning forest of the n-vertex graph A = (rowPtr, colInd, val or None), torch tensors on the handle's GPU
    (include/bhsparse_hip.h, "spanning forest"): every entry (i, j), j != i, whose weight is not NaN is an undirected edge,
    from whichever end and however often it is stored; val None: every weight 1.  maximum: the maximum forest; absolute: the
    weights are |a_ij|.  Returns (lo int32[m], hi int32[m], w[m], label int32[n]) as device tensors: the forest's edges
    sorted by (lo, hi), lo < hi, with the weights as compared, and the root of every vertex's tree.  bh.forest_nedges,
    bh.forest_rounds and bh.forest_ms hold m, the rounds and the device time.  Raises BhsparseError on failure."""
    import torch
    Ap, Aj, Ax = A[0], A[1], A[2] if len(A) > 2 else None
    dt = _value_type(bh, (Ap, Aj, Ax))
    label, lo, hi = (_alloc(n, torch.int32, Ap.device) for _ in range(3))
    w = _alloc(n, dt, Ap.device)
    flags = (_lib.BHS_FOREST_MAXIMUM if maximum else 0) | (_lib.BHS_FOREST_ABS if absolute else 0)
    torch.cuda.synchronize()                           # the library works on its own stream (see facade.initData_device)
    _check(spanning_forest_raw_device(bh, n, Aj.numel(), Ap, Aj if Aj.numel() else None, Ax if Aj.numel() else None, flags,
                                      label, lo, hi, w), "bhs_csr_spanning_forest_device")
    m = bh.forest_nedges
    order = torch.argsort((lo[:m].to(torch.int64) << 32) | hi[:m].to(torch.int64))
    return lo[:m][order], hi[:m][order], w[:m][order], label[:n]


def forest_csr_device(n, lo, hi, w):
    """The edge list (lo, hi, w) of spanning_forest_device as a symmetric n x n CSR (rowPtr int32[n + 1], colInd int32[2 m],
    val[2 m]), both directions stored, rows ascending: torch plumbing only."""
    import torch
    rows = torch.cat([lo, hi]).to(torch.int64)
    cols = torch.cat([hi, lo]).to(torch.int64)
    order = torch.argsort((rows << 32) | cols)
    rowptr = torch.zeros(n + 1, dtype=torch.int32, device=lo.device)
    if rows.numel():
        rowptr[1:] = torch.cumsum(torch.bincount(rows, minlength=n), 0).to(torch.int32)
    return rowptr, cols[order].to(torch.int32), torch.cat([w, w])[order]


def _weight_order(w):
    """int64 whose signed order is the order of the weights as numbers, -0 below +0 (the library's key)"""
    import torch
    b = w.to(torch.float64).view(torch.int64)
    return torch.where(b < 0, b ^ 0x7fffffffffffffff, b)


def single_linkage_device(bh, n, A, nclusters):
    """Single-linkage clustering of the n-vertex graph A = (rowPtr, colInd, val or None) into nclusters clusters: the minimum
    spanning forest, without its heaviest edges -- by the forest's own key order (weight, lo, hi) -- until nclusters trees
    remain, then components_device on what is left.  Returns comp int32[n], the clusters numbered by ascending smallest
    vertex.  ValueError where nclusters is below the number of components of A or above n."""
    import torch
    lo, hi, w, _ = spanning_forest_device(bh, n, A)
    m = lo.numel()
    if nclusters < n - m or nclusters > n:
        raise ValueError("single_linkage_device: %d clusters of a graph with %d vertices and %d components" % (nclusters, n, n - m))
    keep = torch.sort(_weight_order(w), stable=True)[1][:n - nclusters]   # (the edges came sorted by (lo, hi): ties keep that order)
    rest = forest_csr_device(n, lo[keep], hi[keep], w[keep])
    return components_device(bh, n, rest)[1]


def spanning_forest_csr(n, Ap, Aj, Ax, maximum=False, absolute=False, value_dtype=np.float64, device=0):
    """Convenience: spanning_forest_device once on host CSR arrays.  Returns numpy (lo int32[m], hi int32[m], w
    value_dtype[m], label int32[n])."""
    A = _device_csr(Ap, Aj, Ax, value_dtype, device)
    with _handle(value_dtype, device, None) as bh:
        return _host(*spanning_forest_device(bh, n, A, maximum, absolute))


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



def bfs_levels_frontier_csr(n, Ap, Aj, Ax, sources, push_below=None, value_dtype=np.float64, device=0):
    """Convenience: bfs_levels_frontier_device once on host CSR arrays (the out-edges by the handle's transpose).  Returns
    (levels value_dtype[n, k], info) with info["kernels"] (of the last step), info["steps"], info["push_steps"], info["ms"]."""
    A = _device_csr(Ap, Aj, Ax, value_dtype, device)
    with _handle(value_dtype, device, None) as bh:
        out, steps, ms, pushes = _bfs_frontier(bh, n, A, sources, None, push_below)
        return out.cpu().numpy(), {"kernels": bh.kernel_stats(), "steps": steps, "push_steps": pushes, "ms": ms}


def sssp_frontier_csr(n, Ap, Aj, Ax, sources, max_rounds=None, push_below=None, value_dtype=np.float64, device=0):
    """Convenience: sssp_frontier_device once on host CSR arrays.  Returns (distances value_dtype[n, k], info) with
    info["kernels"] (of the last round), info["steps"], info["push_steps"], info["ms"]."""
    A = _device_csr(Ap, Aj, Ax, value_dtype, device)
    with _handle(value_dtype, device, None) as bh:
        out, steps, ms, pushes = _sssp_frontier(bh, n, A, sources, None, max_rounds, push_below)
        return out.cpu().numpy(), {"kernels": bh.kernel_stats(), "steps": steps, "push_steps": pushes, "ms": ms}
