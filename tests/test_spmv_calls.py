"""CPU call-trace test of benchmark_spgemm_using_csr_amd/dense.py against the fake library of tests/test_facade_calls.py: which
C function each call makes, where each torch.cuda.synchronize falls, every argument in order (pointers as the address of the
array that was passed, None = NULL), what is returned or raised, and that spmv_ms -- and nothing else -- is set from the
call's last output.  No GPU, no real library call."""
import numpy as np
import pytest
import torch

from test_facade_calls import ATTRS, FAIL, FakeLib, H, NR, OD, P, RS, Dev, _handle, _match_events, tf, ti

from benchmark_spgemm_using_csr_amd import _lib, dense, facade

MV, MM = "bhs_csr_spmv_device", "bhs_csr_spmm_device"


@pytest.fixture
def fake(monkeypatch):
    lib = FakeLib()
    lib.outs[MV] = {11: 1.25}
    lib.outs[MM] = {14: 2.5}
    monkeypatch.setattr(facade._lib, "load", lambda f32=False: lib)
    monkeypatch.setattr(torch.cuda, "synchronize", lambda *a, **k: lib.events.append("sync"))
    return lib


def handle(lib, init=True):
    bh = _handle(lib, init)
    bh.spmv_ms = "before"
    return bh


def untouched(bh, spmv_ms="before"):
    assert bh.spmv_ms == spmv_ms and type(bh.spmv_ms) is type(spmv_ms)
    for i, a in enumerate(ATTRS):
        assert getattr(bh, a) == "before %d" % i, a


m, n = 4, 6
Ap, Aj, Ax = ti(5), ti(9), tf(9)


def test_raw_calls(fake):
    bh = handle(fake)
    x, y = tf(n), tf(m)
    assert dense.csr_spmv_raw_device(bh, m, n, 9, Ax, Ap, Aj, 2, x, 3, y) == 0
    _match_events(fake.events, [(MV, [H, m, n, 9, P(Ax), P(Ap), P(Aj), 2.0, P(x), 3.0, P(y), OD])], None)
    untouched(bh, 1.25)
    del fake.events[:]
    # NULL for absent values, raw addresses and tensors of the GPU alike; no synchronisation of their own
    assert dense.csr_spmm_raw_device(bh, m, n, 9, None, Dev(0x100), 0x200, 3, 1.5, Dev(0x300), 5, 0, 0x400, 4) == 0
    _match_events(fake.events, [(MM, [H, m, n, 9, None, P(0x100), P(0x200), 3, 1.5, P(0x300), 5, 0.0, P(0x400), 4, OD])], None)
    untouched(bh, 2.5)


@pytest.mark.parametrize("fn", (MV, MM))
def test_failing_status(fake, fn):
    fake.status[fn] = FAIL
    bh = handle(fake)
    x, y, X, Y = tf(n), tf(m), tf(n * 2).view(n, 2), tf(m * 2).view(m, 2)
    if fn == MV:
        assert dense.csr_spmv_raw_device(bh, m, n, 9, Ax, Ap, Aj, 1, x, 0, y) == FAIL
        with pytest.raises(facade.BhsparseError) as ei:
            dense.csr_spmv_device(bh, m, n, (Ap, Aj, Ax), x)
    else:
        assert dense.csr_spmm_raw_device(bh, m, n, 9, Ax, Ap, Aj, 2, 1, X, 2, 0, Y, 2) == FAIL
        with pytest.raises(facade.BhsparseError) as ei:
            dense.csr_spmm_device(bh, m, n, (Ap, Aj, Ax), X)
    assert ei.value.code == FAIL and str(ei.value).startswith(fn + " failed: %d" % FAIL)
    assert [e[0] for e in fake.events if e != "sync"] == [fn, fn]
    untouched(bh)                                                    # (the fake writes its outputs all the same)


def test_before_initPlatform(fake):
    bh = handle(fake, init=False)
    assert dense.csr_spmv_raw_device(bh, m, n, 9, Ax, Ap, Aj, 1, tf(n), 0, tf(m)) == NR
    assert dense.csr_spmm_raw_device(bh, m, n, 9, Ax, Ap, Aj, 1, 1, tf(n), 1, 0, tf(m), 1) == NR
    for call in (lambda: dense.csr_spmv_device(bh, m, n, (Ap, Aj, Ax), tf(n)),
                 lambda: dense.csr_spmm_device(bh, m, n, (Ap, Aj, Ax), tf(n * 2).view(n, 2))):
        with pytest.raises(facade.BhsparseError) as ei:
            call()
        assert ei.value.code == NR
    assert [e for e in fake.events if e != "sync"] == []
    untouched(bh)
    assert bh._h is None and bh._lib is None


def test_tensor_calls(fake):
    bh = handle(fake)
    x = tf(n)
    # the output is made here: before the synchronisation, the library's call after it
    y = dense.csr_spmv_device(bh, m, n, (Ap, Aj, Ax), x)
    assert isinstance(y, torch.Tensor) and y.shape == (m,) and y.dtype == torch.float64
    _match_events(fake.events, ["sync", (MV, [H, m, n, 9, P(Ax), P(Ap), P(Aj), 1.0, P(x), 0.0, RS(), OD])], y)
    assert bh.spmv_ms == 1.25
    del fake.events[:]
    y0 = tf(m)
    assert dense.csr_spmv_device(bh, m, n, (Ap, Aj, None), x, -1, 1, y0) is y0
    _match_events(fake.events, ["sync", (MV, [H, m, n, 9, None, P(Ap), P(Aj), -1.0, P(x), 1.0, P(y0), OD])], None)
    del fake.events[:]
    # the leading dimension is the row stride: three columns of a five-column array, the output contiguous
    wide = tf(n * 5, torch.float32).view(n, 5)
    X = wide[:, 1:4]
    Y = dense.csr_spmm_device(bh, m, n, (Ap, Aj, Ax), X, 2)
    assert Y.shape == (m, 3) and Y.dtype == torch.float32 and Y.is_contiguous()
    _match_events(fake.events, ["sync", (MM, [H, m, n, 9, P(Ax), P(Ap), P(Aj), 3, 2.0, P(X), 5, 0.0, RS(), 3, OD])], Y)
    assert bh.spmv_ms == 2.5
    del fake.events[:]
    Yw = tf(m * 4).view(m, 4)
    Yv = Yw[:, :3]
    assert dense.csr_spmm_device(bh, m, n, (Ap, Aj, Ax), tf(n * 3).view(n, 3), 1, -1, Yv) is Yv
    assert fake.events[1][1][10] == 3 and fake.events[1][1][13] == 4 and fake.events[1][1][12] == ("p", Yw.data_ptr())
    del fake.events[:]
    # what is no row-major n x k / m x k tensor never reaches the library
    for X, Y in ((tf(n * 3).view(3, n).t(), None), (tf(n * 3).view(n, 3), tf(m * 2).view(m, 2)), (tf(n), None),
                 (tf((n + 1) * 3).view(n + 1, 3), None)):
        with pytest.raises(ValueError):
            dense.csr_spmm_device(bh, m, n, (Ap, Aj, Ax), X, 1, 0, Y)
    assert [e for e in fake.events if e != "sync"] == []


def test_conveniences_stage_through_the_handle(fake, monkeypatch):
    """spmv_csr / spmm_csr / residual_csr: a handle of their own, the arrays uploaded in the value type, one call, the kernel
    records and the time in info, the handle destroyed"""
    monkeypatch.setattr(dense, "_upload", lambda a, dt, device: torch.from_numpy(np.ascontiguousarray(a, dt).copy()))
    monkeypatch.setattr(dense, "_device_csr", lambda p, j, x, dt, device: (
        torch.from_numpy(np.ascontiguousarray(p, np.int32)), torch.from_numpy(np.ascontiguousarray(j, np.int32)),
        None if x is None else torch.from_numpy(np.ascontiguousarray(x, dt))))
    hAp, hAj, hAx = np.arange(5), np.arange(9) % n, np.arange(9.0)
    y, info = dense.spmv_csr(m, n, hAp, hAj, hAx, np.arange(n), value_dtype=np.float32)
    assert y.dtype == np.float32 and y.shape == (m,) and info["ms"] == 1.25 and [s["name"] for s in info["kernels"]] == ["k_a", "k_b"]
    names = [e[0] for e in fake.events if e != "sync"]
    assert names == ["bhs_create", "bhs_set_option", MV, "bhs_get_kernel_stats", "bhs_destroy"]
    del fake.events[:]
    b = np.arange(m) + 1.0
    r, info = dense.residual_csr(m, n, hAp, hAj, hAx, np.arange(n), b)
    call = [e for e in fake.events if e != "sync" and e[0] == MV][0][1]
    assert call[7] == -1.0 and call[9] == 1.0 and r.dtype == np.float64
    assert np.array_equal(r, b) and r is not b                       # (the fake computes nothing: the copy of b comes back)
    del fake.events[:]
    Y, info = dense.spmm_csr(m, n, hAp, hAj, None, np.ones((n, 3)), 2.0)
    call = [e for e in fake.events if e != "sync" and e[0] == MM][0][1]
    assert call[4] is None and call[7] == 3 and call[8] == 2.0 and call[10] == 3 and call[11] == 0.0 and call[13] == 3
    assert Y.shape == (m, 3) and info["ms"] == 2.5
    assert _lib.BHS_ERR_NOT_READY == NR
