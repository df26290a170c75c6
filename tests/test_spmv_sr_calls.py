"""CPU call-trace test of the semiring calls of benchmark_spgemm_using_csr_amd/dense.py and of graph.py's conveniences
against the fake library of tests/test_facade_calls.py: which C function each call makes, where each torch.cuda.synchronize
falls, every argument in order (pointers as the address of the array that was passed, None = NULL), what is returned or
raised, and that spmv_ms and spmv_changed -- and nothing else -- are set from the call's last two outputs.  No GPU, no real
library call."""
import ctypes as C

import numpy as np
import pytest
import torch

from test_facade_calls import ATTRS, FAIL, FakeLib, H, NR, O, OD, P, RS, Dev, _handle, _match_events, tf, ti

from benchmark_spgemm_using_csr_amd import _lib, dense, facade, graph

SV, SM = "bhs_csr_spmv_semiring_device", "bhs_csr_spmm_semiring_device"
OLL = O(C.c_longlong)
ACC, CMP = _lib.BHS_MV_ACCUM, _lib.BHS_MV_MASK_COMPLEMENT
MIN_PLUS, OR_AND = _lib.BHS_SR_MIN_PLUS, _lib.BHS_SR_OR_AND


@pytest.fixture
def fake(monkeypatch):
    lib = FakeLib()
    lib.outs[SV] = {12: 7, 13: 1.25}
    lib.outs[SM] = {16: 9, 17: 2.5}
    monkeypatch.setattr(facade._lib, "load", lambda f32=False: lib)
    monkeypatch.setattr(torch.cuda, "synchronize", lambda *a, **k: lib.events.append("sync"))
    return lib


def handle(lib, init=True):
    bh = _handle(lib, init)
    bh.spmv_ms, bh.spmv_changed = "before", "before"
    return bh


def untouched(bh, spmv_ms="before", spmv_changed="before"):
    assert bh.spmv_ms == spmv_ms and type(bh.spmv_ms) is type(spmv_ms)
    assert bh.spmv_changed == spmv_changed and type(bh.spmv_changed) is type(spmv_changed)
    for i, a in enumerate(ATTRS):
        assert getattr(bh, a) == "before %d" % i, a


m, n = 4, 6
Ap, Aj, Ax = ti(5), ti(9), tf(9)


def test_raw_calls(fake):
    bh = handle(fake)
    x, y, mask = tf(n), tf(m), tf(m)
    assert dense.csr_spmv_semiring_raw_device(bh, "min_plus", m, n, 9, Ax, Ap, Aj, x, ACC, mask, y) == 0
    _match_events(fake.events, [(SV, [H, MIN_PLUS, m, n, 9, P(Ax), P(Ap), P(Aj), P(x), ACC, P(mask), P(y), OLL, OD])], None)
    untouched(bh, 1.25, 7)
    del fake.events[:]
    # the semiring by constant; NULL for absent values and an absent mask, raw addresses and tensors of the GPU alike; no
    # synchronisation of their own
    assert dense.csr_spmm_semiring_raw_device(bh, OR_AND, m, n, 9, None, Dev(0x100), 0x200, 3, Dev(0x300), 5, CMP, 0x500, 4,
                                              0x400, 6) == 0
    _match_events(fake.events, [(SM, [H, OR_AND, m, n, 9, None, P(0x100), P(0x200), 3, P(0x300), 5, CMP, P(0x500), 4, P(0x400), 6,
                                      OLL, OD])], None)
    untouched(bh, 2.5, 9)
    del fake.events[:]
    assert dense.csr_spmm_semiring_raw_device(bh, "plus_pair", m, n, 9, None, Ap, Aj, 1, None, 1, 0, None, 1, tf(m), 1) == 0
    assert fake.events[0][1][1] == _lib.BHS_SR_PLUS_PAIR and fake.events[0][1][9] is None and fake.events[0][1][12] is None
    with pytest.raises(KeyError):
        dense.csr_spmv_semiring_raw_device(bh, "plus_minus", m, n, 9, Ax, Ap, Aj, x, 0, None, y)


@pytest.mark.parametrize("fn", (SV, SM))
def test_failing_status(fake, fn):
    fake.status[fn] = FAIL
    bh = handle(fake)
    x, y, X, Y = tf(n), tf(m), tf(n * 2).view(n, 2), tf(m * 2).view(m, 2)
    if fn == SV:
        assert dense.csr_spmv_semiring_raw_device(bh, 1, m, n, 9, Ax, Ap, Aj, x, 0, None, y) == FAIL
    else:
        assert dense.csr_spmm_semiring_raw_device(bh, 1, m, n, 9, Ax, Ap, Aj, 2, X, 2, 0, None, 2, Y, 2) == FAIL
        with pytest.raises(facade.BhsparseError) as ei:
            dense.csr_spmm_semiring_device(bh, "min_plus", m, n, (Ap, Aj, Ax), X)
        assert ei.value.code == FAIL and str(ei.value).startswith(fn + " failed: %d" % FAIL)
    untouched(bh)                                                    # (the fake writes its outputs all the same)


def test_before_initPlatform(fake):
    bh = handle(fake, init=False)
    assert dense.csr_spmv_semiring_raw_device(bh, 1, m, n, 9, Ax, Ap, Aj, tf(n), 0, None, tf(m)) == NR
    assert dense.csr_spmm_semiring_raw_device(bh, 1, m, n, 9, Ax, Ap, Aj, 1, tf(n), 1, 0, None, 1, tf(m), 1) == NR
    with pytest.raises(facade.BhsparseError) as ei:
        dense.csr_spmm_semiring_device(bh, "or_and", m, n, (Ap, Aj, Ax), tf(n))
    assert ei.value.code == NR
    # the traversals answer the same way: their first step raises, nothing reaches a library
    for call in (lambda: graph.bfs_levels_device(bh, m, (ti(m + 1), ti(3), tf(3)), [0]),
                 lambda: graph.sssp_device(bh, m, (ti(m + 1), ti(3), None), 0, 5)):
        with pytest.raises(facade.BhsparseError) as ei:
            call()
        assert ei.value.code == NR
    assert [e for e in fake.events if e != "sync"] == []
    untouched(bh)
    assert bh._h is None and bh._lib is None


def test_traversals_check_their_arguments(fake):
    bh = handle(fake)
    A = (ti(4), ti(3), tf(3))
    for sources in ([], [3], [-1], [[0, 1]]):
        with pytest.raises(ValueError):
            graph.bfs_levels_device(bh, 3, A, sources)
        with pytest.raises(ValueError):
            graph.sssp_device(bh, 3, A, sources)
    with pytest.raises(ValueError):
        graph.bfs_levels_device(bh, 0, (ti(1), ti(0), tf(0)), [0])   # no vertex to start from
    with pytest.raises(ValueError):
        graph.sssp_device(bh, 3, A, 0, max_sweeps=0)
    assert [e for e in fake.events if e != "sync"] == []
    # what a sweep limit below n says when it runs out: no verdict on a negative cycle
    fake.outs[SM] = {16: 1, 17: 2.5}
    with pytest.raises(facade.BhsparseError) as ei:
        graph.sssp_device(bh, 3, A, 0, max_sweeps=2)
    assert "after 2 sweeps" in str(ei.value) and "no verdict" in str(ei.value)
    with pytest.raises(facade.BhsparseError) as ei:
        graph.sssp_device(bh, 3, A, 0)
    assert "after 3 sweeps" in str(ei.value) and "a cycle of negative weight" in str(ei.value)


def test_tensor_calls(fake):
    bh = handle(fake)
    x = tf(n)
    # a 1-D tensor is k = 1 of the matrix call; the output is made here, before the synchronisation
    y, changed = dense.csr_spmm_semiring_device(bh, "min_plus", m, n, (Ap, Aj, Ax), x)
    assert isinstance(y, torch.Tensor) and y.shape == (m,) and y.dtype == torch.float64 and changed == 9 and type(changed) is int
    _match_events(fake.events, ["sync", (SM, [H, MIN_PLUS, m, n, 9, P(Ax), P(Ap), P(Aj), 1, P(x), 1, 0, None, 1, RS(), 1, OLL, OD])], y)
    assert bh.spmv_ms == 2.5 and bh.spmv_changed == 9
    del fake.events[:]
    y0, mask = tf(m), tf(m)
    out, _ = dense.csr_spmm_semiring_device(bh, OR_AND, m, n, (Ap, Aj, None), x, y0, mask, accumulate=True, complement=True)
    assert out is y0
    _match_events(fake.events, ["sync", (SM, [H, OR_AND, m, n, 9, None, P(Ap), P(Aj), 1, P(x), 1, ACC | CMP, P(mask), 1, P(y0), 1,
                                              OLL, OD])], None)
    del fake.events[:]
    # the leading dimensions are the row strides: three columns of wider arrays, the output made here contiguous
    wide, wideM = tf(n * 5, torch.float32).view(n, 5), tf(m * 4, torch.float32).view(m, 4)
    X, M = wide[:, 1:4], wideM[:, :3]
    Y, _ = dense.csr_spmm_semiring_device(bh, "max_min", m, n, (Ap, Aj, Ax), X, mask=M)
    assert Y.shape == (m, 3) and Y.dtype == torch.float32 and Y.is_contiguous()
    _match_events(fake.events, ["sync", (SM, [H, _lib.BHS_SR_MAX_MIN, m, n, 9, P(Ax), P(Ap), P(Aj), 3, P(X), 5, 0, P(M), 4, RS(), 3,
                                              OLL, OD])], Y)
    del fake.events[:]
    # what is no row-major n x k / m x k tensor never reaches the library
    for X, Y, M in ((tf(n * 3).view(3, n).t(), None, None), (tf(n * 3).view(n, 3), tf(m * 2).view(m, 2), None),
                    (tf(n * 3).view(n, 3), None, tf(m * 2).view(m, 2)), (tf((n + 1) * 3).view(n + 1, 3), None, None),
                    (tf(n * 3).view(n, 3), None, tf(m))):
        with pytest.raises(ValueError):
            dense.csr_spmm_semiring_device(bh, 1, m, n, (Ap, Aj, Ax), X, Y, M)
    assert [e for e in fake.events if e != "sync"] == []


def stage_on_the_host(monkeypatch):
    up = lambda a, dt, device: torch.from_numpy(np.ascontiguousarray(a, dt).copy())   # noqa: E731
    csr = lambda p, j, x, dt, device: (up(p, np.int32, 0), up(j, np.int32, 0), None if x is None else up(x, dt, 0))   # noqa: E731
    for mod in (dense, graph):
        monkeypatch.setattr(mod, "_device_csr", csr)
    monkeypatch.setattr(dense, "_upload", up)


def test_conveniences_stage_through_the_handle(fake, monkeypatch):
    stage_on_the_host(monkeypatch)
    hAp, hAj, hAx = np.arange(5), np.arange(9) % n, np.arange(9.0)
    Y, info = dense.spmm_semiring_csr("min_plus", m, n, hAp, hAj, hAx, np.ones((n, 3)), value_dtype=np.float32)
    assert Y.dtype == np.float32 and Y.shape == (m, 3) and np.all(Y == np.inf)      # (the fake computes nothing: the identity comes back)
    assert info["ms"] == 2.5 and info["changed"] == 9 and [s["name"] for s in info["kernels"]] == ["k_a", "k_b"]
    names = [e[0] for e in fake.events if e != "sync"]
    assert names == ["bhs_create", "bhs_set_option", SM, "bhs_get_kernel_stats", "bhs_destroy"]
    call = [e for e in fake.events if e != "sync" and e[0] == SM][0][1]
    assert call[1] == MIN_PLUS and call[8] == 3 and call[11] == 0 and call[12] is None
    del fake.events[:]
    Y, info = dense.spmm_semiring_csr(OR_AND, m, n, hAp, hAj, None, np.ones(n), np.zeros(m), np.ones(m), True, True)
    call = [e for e in fake.events if e != "sync" and e[0] == SM][0][1]
    assert call[5] is None and call[8] == 1 and call[11] == ACC | CMP and call[12] is not None and Y.shape == (m, 1)


def test_traversals_are_loops_of_semiring_calls(fake, monkeypatch):
    """bfs_levels_csr / sssp_csr: one OR_AND call under the complement of the levels per step, one accumulating MIN_PLUS
    call per sweep; the fake's count of changed elements drives the loops"""
    stage_on_the_host(monkeypatch)
    nv = 5
    hAp, hAj, hAx = np.arange(nv + 1), (np.arange(nv) + 1) % nv, np.ones(nv)
    fake.outs[SM] = {16: 0, 17: 2.5}                                 # nothing changes: the first step is the last
    levels, info = graph.bfs_levels_csr(nv, hAp, hAj, hAx, [0, 3])
    assert levels.shape == (nv, 2) and levels[0, 0] == 1 and levels[3, 1] == 1 and levels.sum() == 2
    assert info["steps"] == 1 and info["ms"] == 2.5 and [s["name"] for s in info["kernels"]] == ["k_a", "k_b"]
    calls = [e[1] for e in fake.events if e != "sync" and e[0] == SM]
    assert len(calls) == 1 and calls[0][1] == OR_AND and calls[0][8] == 2 and calls[0][11] == CMP and calls[0][12] is not None
    assert calls[0][12] != calls[0][9] and calls[0][14] not in (calls[0][9], calls[0][12])     # levels, frontier, next: three arrays
    del fake.events[:]
    dist, info = graph.sssp_csr(nv, hAp, hAj, hAx, 2)
    assert dist.shape == (nv, 1) and dist[2, 0] == 0 and np.isinf(np.delete(dist[:, 0], 2)).all() and info["steps"] == 1
    calls = [e[1] for e in fake.events if e != "sync" and e[0] == SM]
    assert len(calls) == 1 and calls[0][1] == MIN_PLUS and calls[0][11] == ACC and calls[0][12] is None
    assert calls[0][9] != calls[0][14]                               # Jacobi: the sweep reads D and writes its copy
    del fake.events[:]
    fake.outs[SM] = {16: 1, 17: 2.5}                                 # something always changes
    with pytest.raises(facade.BhsparseError):
        graph.sssp_csr(nv, hAp, hAj, hAx, 2)
    assert len([e for e in fake.events if e != "sync" and e[0] == SM]) == nv
    del fake.events[:]
    levels, info = graph.bfs_levels_csr(nv, hAp, hAj, hAx, 0)
    assert info["steps"] == nv and info["ms"] == 2.5 * nv            # at most n steps
    assert _lib.BHS_ERR_NOT_READY == NR
