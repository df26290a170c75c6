"""CPU call-trace test of the Python facade: every public method of `bhsparse` against a fake library that records each C
call, fills the outputs with scripted values and returns a scripted status.  The expected calls are written out by hand from
include/bhsparse_hip.h: which function, where each torch.cuda.synchronize falls, every argument in order (pointers as the
address of the array that was passed, None = NULL), what is returned or raised, and which attributes are set from which
output.  No GPU, no real library call."""
import ctypes as C

import numpy as np
import pytest
import torch

from benchmark_spgemm_using_csr_amd import _lib, facade

HANDLE = 0xABC0
NR, IA = _lib.BHS_ERR_NOT_READY, _lib.BHS_ERR_INVALID_ARG
FAIL = _lib.BHS_ERR_LAUNCH
ST4 = [0.5, 1.5, 3.5, 4.5]
KS = [dict(name="k_a", launches=3, ms=0.5, rows=10, products=20, nnz_out=30, nnzA_rows=40),
      dict(name="k_b", launches=4, ms=0.75, rows=11, products=21, nnz_out=31, nnzA_rows=41)]
# argument index -> value the fake writes there (counted from include/bhsparse_hip.h)
OUTS = {
    "bhs_create": {0: HANDLE},
    "bhs_spgemm": {2: 7001, 3: 501, 4: ST4},
    "bhs_spgemm_symbolic": {1: 7001, 2: 501},
    "bhs_spgemm_finish": {1: ST4},
    "bhs_get_nnzC": {1: 41},
    "bhs_get_C_device": {1: 0x1000, 2: 0x2000, 3: 0x3000},
    "bhs_get_info": {2: 99},
    "bhs_get_class_tables_device": {1: 0x4000, 2: 0x5000, 3: 0x6000, 4: 12, 5: 34, 6: 1},
    "bhs_spgemm_masked": {5: 7001, 6: 1.25},
    "bhs_spgemm_masked_device": {5: 7001, 6: 1.25},
    "bhs_spgemm_semiring_masked": {6: 7001, 7: 1.25},
    "bhs_spgemm_semiring_masked_device": {6: 7001, 7: 1.25},
    "bhs_csr_add_symbolic_device": {10: 37, 11: 1},
    "bhs_csr_add_numeric_device": {16: 1.25},
    "bhs_spgemm_add": {8: 7001, 9: 501, 10: [1.25, 2.5]},
    "bhs_spgemm_add_device": {8: 7001, 9: 501, 10: [1.25, 2.5]},
    "bhs_csr_select_symbolic_device": {9: 37},
    "bhs_csr_select_numeric_device": {11: 1.25},
    "bhs_spgemm_select": {3: 7001, 4: 501, 5: [1.25, 2.5]},
    "bhs_spgemm_select_device": {3: 7001, 4: 501, 5: [1.25, 2.5]},
    "bhs_spgemm_semiring": {3: 7001, 4: 501, 5: [1.25, 2.5]},
    "bhs_csr_transpose_device": {11: 1.25},
    "bhs_csr_transpose_values_device": {5: 1.25},
    "bhs_csr_extract_symbolic_device": {11: 37},
    "bhs_csr_extract_numeric_device": {16: 1.25},
    "bhs_csr_reduce_device": {11: 1.25},
    "bhs_csr_scale_device": {12: 1.25},
}
ATTRS = ("nnzCt", "nnzC", "stage_ms", "time_ms", "multiply_ms", "masked_ms", "add_ms", "select_ms", "transpose_ms",
         "extract_ms", "reduce_ms", "scale_ms", "semiring_ms")


def _norm(a):
    """What the fake records of one argument: plain values as they are, pointers as ("p", address) or None for NULL,
    byref(x) as ("ref", x), a ctypes array as ("arr", array)."""
    if isinstance(a, C.c_void_p):
        return ("p", a.value) if a.value else None
    if type(a).__name__ == "CArgObject":
        return ("ref", a._obj)
    if isinstance(a, C.Array):
        return ("arr", a)
    assert a is None or type(a) in (int, float, bytes), a
    return a


class FakeLib(object):
    def __init__(self):
        self.events, self.status, self.outs = [], {}, {k: dict(v) for k, v in OUTS.items()}
        for name in _lib.SYMBOLS:
            setattr(self, name, self._make(name))

    def _make(self, name):
        def call(*args):
            if name == "bhs_strerror":
                return b"scripted"
            if name == "bhs_version":
                return b"fake"
            self.events.append((name, [_norm(a) for a in args]))
            for i, v in self.outs.get(name, {}).items():
                if isinstance(args[i], C.Array):
                    args[i][:] = v
                else:
                    args[i]._obj.value = v
            if name == "bhs_get_kernel_stats":
                for i, rec in enumerate(KS):
                    for k, v in rec.items():
                        setattr(args[1][i], k, v.encode() if k == "name" else v)
                return self.status.get(name, len(KS))
            return self.status.get(name, 0)
        return call


class Dev(object):
    """stands for a tensor on the GPU: the facade synchronises before the library reads one"""
    is_cuda, device = True, "cuda:0"

    def __init__(self, addr):
        self._addr = addr

    def data_ptr(self):
        return self._addr


def _addr(x):
    if isinstance(x, np.ndarray):
        return x.ctypes.data
    if isinstance(x, torch.Tensor):      # an empty slice keeps its allocation
        return x.untyped_storage().data_ptr() + x.storage_offset() * x.element_size()
    return x if isinstance(x, int) else x.data_ptr()


class P(object):
    """a pointer to this array (or this raw address)"""
    def __init__(self, x):
        self.x = x

    def ok(self, got, ret):
        return got == ("p", _addr(self.x))


class RS(object):
    """a pointer to what the method returned (item i of the returned tuple)"""
    def __init__(self, i=None):
        self.i = i

    def ok(self, got, ret):
        if ret is None:                  # the method raised: all that is known is that something was allocated
            return NonNull().ok(got, ret)
        x = ret if self.i is None else ret[self.i]
        return x is not None and got == ("p", _addr(x))


class RV(RS):
    """a pointer to the returned tensor as it is returned: sliced before the call, so NULL when it has no entries"""
    def ok(self, got, ret):
        if ret is None:
            return True
        return got == (("p", ret.data_ptr()) if ret.data_ptr() else None)


class O(object):
    """byref of a fresh output of this ctype"""
    def __init__(self, ctype):
        self.t = ctype

    def ok(self, got, ret):
        return isinstance(got, tuple) and got[0] == "ref" and type(got[1]) is self.t


class A(O):
    """a fresh double[n] output"""
    def ok(self, got, ret):
        return isinstance(got, tuple) and got[0] == "arr" and got[1]._type_ is C.c_double and len(got[1]) == self.t


class IS(O):
    """byref of (or the ctypes array that is) this very object"""
    def ok(self, got, ret):
        return isinstance(got, tuple) and got[0] in ("ref", "arr") and got[1] is self.t


class IN(object):
    """byref of an input of this ctype and value"""
    def __init__(self, ctype, v):
        self.t, self.v = ctype, v

    def ok(self, got, ret):
        return isinstance(got, tuple) and got[0] == "ref" and type(got[1]) is self.t and got[1].value == self.v


class NonNull(object):
    def ok(self, got, ret):
        return isinstance(got, tuple) and got[0] == "p" and got[1]


class KSArr(object):
    def ok(self, got, ret):
        return isinstance(got, tuple) and got[0] == "arr" and got[1]._type_ is _lib.KernelStat and len(got[1]) == 64


O64, OI, OD, OV = O(C.c_int64), O(C.c_int), O(C.c_double), O(C.c_void_p)
H = P(HANDLE)
WALL = object()          # time_ms: taken with perf_counter around the call, on success and on failure


def _match_events(got, want, ret):
    assert [e if e == "sync" else e[0] for e in got] == [e if e == "sync" else e[0] for e in want]
    for g, w in zip(got, want):
        if w == "sync":
            continue
        assert len(g[1]) == len(w[1]), (g[0], len(g[1]), len(w[1]))
        for i, (ga, wa) in enumerate(zip(g[1], w[1])):
            if hasattr(wa, "ok"):
                assert wa.ok(ga, ret), "%s argument %d: %r" % (g[0], i, ga)
            else:
                assert type(ga) is type(wa) and ga == wa, "%s argument %d: %r, expected %r" % (g[0], i, ga, wa)


def i32(n):
    return np.arange(n, dtype=np.int32)


def f64(n):
    return np.arange(n, dtype=np.float64)


def ti(n):
    return torch.arange(n, dtype=torch.int32)


def tf(n, dt=torch.float64):
    return torch.arange(n, dtype=dt)


def t_numel(n, dtype):
    """a torch tensor of n entries of this dtype; 0 entries: an empty slice of a 1-element allocation"""
    def check(x):
        return (isinstance(x, torch.Tensor) and x.numel() == n and x.dtype == dtype and
                x.untyped_storage().nbytes() == max(n, 1) * x.element_size())
    return check


def _check_ret(ret, want):
    if isinstance(want, tuple):
        assert isinstance(ret, tuple) and len(ret) == len(want), ret
        for r, w in zip(ret, want):
            _check_ret(r, w)
    elif callable(want):
        assert want(ret), ret
    elif want is None:
        assert ret is None
    else:
        assert type(ret) is type(want) and ret == want, (ret, want)


class Raises(object):
    def __init__(self, code, where):
        self.code, self.where = code, where


class Case(object):
    """One call of one method.  events: the calls it makes ("sync" or (C function, arguments)); ret: what it returns, or a
    Raises; attrs: what it sets; fails: {C function made to fail: what the method then returns (or a Raises)} -- the events
    then end with that call and no attribute but time_ms (where WALL) changes; uninit: the same call before initPlatform
    (a value, a Raises, or an exception type), which reaches no C function; outs: other scripted outputs; after: a further
    check of the object."""
    def __init__(self, name, method, args, events, ret=0, attrs=None, fails=None, uninit=None, kwargs=None, outs=None,
                 setup=None, after=None):
        self.__dict__.update(name=name, method=method, args=args, events=events, ret=ret, attrs=attrs or {},
                             fails=fails or {}, uninit=uninit, kwargs=kwargs or {}, outs=outs or {}, setup=setup,
                             after=after)


def _cases():
    c = []
    Cp = i32(5)
    Ax, Ap, Aj, Bx, Bp, Bj = f64(7), i32(5), i32(7), f64(8), i32(6), i32(8)
    add = c.append

    # ---- data, warmup, the multiply ----
    add(Case("initData", "initData", (4, 5, 6, 7, Ax, Ap, Aj, 8, Bx, Bp, Bj, Cp),
             [("bhs_set_data", [H, 4, 5, 6, 7, P(Ax), P(Ap), P(Aj), 8, P(Bx), P(Bp), P(Bj)])],
             fails={"bhs_set_data": FAIL}, uninit=NR, setup=lambda bh: setattr(bh, "_m", 0),
             after=lambda bh: bh._m == 4 and bh._rowptrC is Cp))
    add(Case("initData_wrong_dtype", "initData", (4, 5, 6, 7, Ax.astype(np.float32), Ap, Aj, 8, Bx, Bp, Bj, Cp), [], ret=IA))
    add(Case("initData_short_rowptrC", "initData", (4, 5, 6, 7, Ax, Ap, Aj, 8, Bx, Bp, Bj, i32(4)), [], ret=IA))
    dev = (Ax, Ap, Aj, Bx, Bp, Bj)
    add(Case("initData_device_host_arrays", "initData_device", (4, 5, 6, 7, Ax, Ap, Aj, 8, Bx, Bp, Bj),
             [("bhs_set_data_device", [H, 4, 5, 6, 7, P(Ax), P(Ap), P(Aj), 8, P(Bx), P(Bp), P(Bj)])],
             fails={"bhs_set_data_device": FAIL}, uninit=NR,
             after=lambda bh: bh._m == 4 and bh._rowptrC is None and all(a is b for a, b in zip(bh._keep, dev))))
    d = [Dev(0x100 * (i + 1)) for i in range(6)]
    add(Case("initData_device_gpu_arrays", "initData_device", (4, 5, 6, 7, d[0], d[1], d[2], 8, d[3], d[4], d[5]),
             ["sync", ("bhs_set_data_device", [H, 4, 5, 6, 7, P(0x100), P(0x200), P(0x300), 8, P(0x400), P(0x500), P(0x600)])]))
    add(Case("warmup", "warmup", (), [("bhs_warmup", [H])], fails={"bhs_warmup": FAIL}, uninit=NR))
    add(Case("spgemm", "spgemm", (), [("bhs_spgemm", [H, P(Cp), O64, OI, A(4)])],
             attrs={"nnzCt": 7001, "nnzC": 501, "stage_ms": ST4, "time_ms": WALL}, fails={"bhs_spgemm": FAIL}, uninit=NR,
             setup=lambda bh: setattr(bh, "_rowptrC", Cp)))
    add(Case("spgemm_no_rowptrC", "spgemm", (), [("bhs_spgemm", [H, None, O64, OI, A(4)])],
             attrs={"nnzCt": 7001, "nnzC": 501, "stage_ms": ST4, "time_ms": WALL},
             setup=lambda bh: setattr(bh, "_rowptrC", None)))

    # ---- masked and semiring-masked multiply ----
    for meth, fn, lead, attr in (("spgemm_masked", "bhs_spgemm_masked", (), "masked_ms"),
                                 ("spgemm_semiring_masked", "bhs_spgemm_semiring_masked", (3,), "semiring_ms")):
        Mp, Mj, vC = i32(5), i32(3), f64(3)
        nd = lambda x: isinstance(x, np.ndarray) and x.dtype == np.float64 and x.size == 3   # noqa: E731
        add(Case(meth, meth, lead + (Mp, Mj), [(fn, [H] + list(lead) + [P(Mp), P(Mj), 3, RS(), O64, OD])], ret=nd,
                 attrs={"nnzCt": 7001, attr: 1.25}, fails={fn: Raises(FAIL, fn)}, uninit=Raises(NR, fn)))
        add(Case(meth + "_valC", meth, lead + (Mp, Mj, vC), [(fn, [H] + list(lead) + [P(Mp), P(Mj), 3, P(vC), O64, OD])],
                 ret=lambda x, vC=vC: x is vC, attrs={"nnzCt": 7001, attr: 1.25}))
        add(Case(meth + "_empty", meth, lead + (Mp, i32(0)), [(fn, [H] + list(lead) + [P(Mp), None, 0, None, O64, OD])],
                 ret=lambda x: isinstance(x, np.ndarray) and x.dtype == np.float64 and x.size == 0,
                 attrs={"nnzCt": 7001, attr: 1.25}))
        add(Case(meth + "_short_rowPtrM", meth, lead + (i32(4), Mj), [], ret=Raises(IA, fn)))
        add(Case(meth + "_bad_valC", meth, lead + (Mp, Mj, np.zeros(3, np.float32)), [], ret=Raises(IA, fn)))
        add(Case(meth + "_small_valC", meth, lead + (Mp, Mj, f64(2)), [], ret=Raises(IA, fn)))
        fn, meth = fn + "_device", meth + "_device"
        add(Case(meth, meth, lead + (Mp, Mj, 3, vC), [(fn, [H] + list(lead) + [P(Mp), P(Mj), 3, P(vC), O64, OD])],
                 attrs={"nnzCt": 7001, attr: 1.25}, fails={fn: FAIL}, uninit=NR))
        add(Case(meth + "_gpu_arrays", meth, lead + (Dev(0x100), 0x200, 3, 0x300),
                 ["sync", (fn, [H] + list(lead) + [P(0x100), P(0x200), 3, P(0x300), O64, OD])],
                 attrs={"nnzCt": 7001, attr: 1.25}))

    # ---- multiply, then add / select / semiring ----
    Dp, Dj, Dx = i32(5), i32(3), f64(3)
    mul = {"nnzCt": 7001, "nnzC": 501}
    rp = lambda bh: setattr(bh, "_rowptrC", Cp)      # noqa: E731
    add(Case("spgemm_add", "spgemm_add", (2, 3, Dp, Dj, Dx),
             [("bhs_spgemm_add", [H, 2.0, 3.0, 3, P(Dx), P(Dp), P(Dj), P(Cp), O64, OI, A(2)])],
             attrs=dict(mul, add_ms=2.5, time_ms=WALL), fails={"bhs_spgemm_add": FAIL}, uninit=NR, setup=rp))
    add(Case("spgemm_add_empty_D", "spgemm_add", (2, 3, Dp, i32(0), f64(0)),
             [("bhs_spgemm_add", [H, 2.0, 3.0, 0, None, P(Dp), None, P(Cp), O64, OI, A(2)])],
             attrs=dict(mul, add_ms=2.5, time_ms=WALL), setup=rp))
    add(Case("spgemm_add_short_rowPtrD", "spgemm_add", (2, 3, i32(4), Dj, Dx), [], ret=IA))
    add(Case("spgemm_add_val_col_mismatch", "spgemm_add", (2, 3, Dp, Dj, f64(2)), [], ret=IA))
    add(Case("spgemm_add_device", "spgemm_add_device", (2, 3, 3, Dx, Dp, Dj),
             [("bhs_spgemm_add_device", [H, 2.0, 3.0, 3, P(Dx), P(Dp), P(Dj), P(Cp), O64, OI, A(2)])],
             attrs=dict(mul, add_ms=2.5), fails={"bhs_spgemm_add_device": FAIL}, uninit=NR, setup=rp))
    add(Case("spgemm_add_device_gpu_arrays", "spgemm_add_device", (2, 3, 3, 0x100, 0x200, Dev(0x300)),
             ["sync", ("bhs_spgemm_add_device", [H, 2.0, 3.0, 3, P(0x100), P(0x200), P(0x300), None, O64, OI, A(2)])],
             attrs=dict(mul, add_ms=2.5), setup=lambda bh: setattr(bh, "_rowptrC", None)))
    spec = _lib.Select()
    add(Case("spgemm_select", "spgemm_select", (spec,), [("bhs_spgemm_select", [H, IS(spec), P(Cp), O64, OI, A(2)])],
             attrs=dict(mul, select_ms=2.5, time_ms=WALL), fails={"bhs_spgemm_select": FAIL}, uninit=NR, setup=rp))
    add(Case("spgemm_select_device", "spgemm_select_device", (spec,),
             [("bhs_spgemm_select_device", [H, IS(spec), None, O64, OI, A(2)])],
             attrs=dict(mul, select_ms=2.5), fails={"bhs_spgemm_select_device": FAIL}, uninit=NR, setup=rp))
    add(Case("spgemm_select_device_rowptr", "spgemm_select_device", (spec, Dev(0x700)),
             [("bhs_spgemm_select_device", [H, IS(spec), P(0x700), O64, OI, A(2)])], attrs=dict(mul, select_ms=2.5)))
    add(Case("spgemm_semiring", "spgemm_semiring", (5,), [("bhs_spgemm_semiring", [H, 5, P(Cp), O64, OI, A(2)])],
             attrs=dict(mul, semiring_ms=2.5, multiply_ms=1.25, time_ms=WALL), fails={"bhs_spgemm_semiring": FAIL},
             uninit=NR, setup=rp))

    # ---- the stand-alone add ----
    m, n = 4, 6
    Xp, Xj, Xx = ti(5), ti(9), tf(9)
    Yp, Yj, Yx = ti(5), ti(7), tf(7)
    Zp, Zj, Zx, pm = ti(5), ti(37), tf(37), ti(37)
    X, Y = (Xp, Xj, Xx), (Yp, Yj, Yx)
    sym, num = "bhs_csr_add_symbolic_device", "bhs_csr_add_numeric_device"
    add(Case("csr_add_symbolic_device", "csr_add_symbolic_device", (m, n, 9, Xp, Xj, 7, Yp, Yj, Zp),
             [(sym, [H, m, n, 9, P(Xp), P(Xj), 7, P(Yp), P(Yj), P(Zp), OI, OI])], ret=(0, 37, 1),
             fails={sym: (FAIL, 37, 1)}, uninit=AttributeError))
    add(Case("csr_add_numeric_device", "csr_add_numeric_device", (m, n, 2, 9, Xx, Xp, Xj, 3, 7, Yx, Yp, Yj, Zp, Zj, Zx),
             [(num, [H, m, n, 2.0, 9, P(Xx), P(Xp), P(Xj), 3.0, 7, P(Yx), P(Yp), P(Yj), P(Zp), P(Zj), P(Zx), OD])],
             attrs={"add_ms": 1.25}, fails={num: FAIL}, uninit=AttributeError))
    for nz in (37, 0):
        add(Case("csr_add_device_nnzZ_%d" % nz, "csr_add_device", (m, n, 2, X, 3, Y),
                 ["sync", (sym, [H, m, n, 9, P(Xp), P(Xj), 7, P(Yp), P(Yj), RS(0), OI, OI]),
                  "sync", (num, [H, m, n, 2.0, 9, P(Xx), P(Xp), P(Xj), 3.0, 7, P(Yx), P(Yp), P(Yj), RS(0), RS(1), RS(2), OD])],
                 ret=(t_numel(m + 1, torch.int32), t_numel(nz, torch.int32), t_numel(nz, torch.float64), 1),
                 attrs={"add_ms": 1.25}, fails={sym: Raises(FAIL, sym), num: Raises(FAIL, num)}, uninit=AttributeError,
                 outs={sym: {10: nz, 11: 1}}))

    # ---- the stand-alone selection ----
    sym, num = "bhs_csr_select_symbolic_device", "bhs_csr_select_numeric_device"
    add(Case("csr_select_symbolic_device", "csr_select_symbolic_device", (m, n, 9, Xx, Xp, Xj, spec, Zp),
             [(sym, [H, m, n, 9, P(Xx), P(Xp), P(Xj), IS(spec), P(Zp), OI])], ret=(0, 37), fails={sym: (FAIL, 37)},
             uninit=AttributeError))
    add(Case("csr_select_numeric_device", "csr_select_numeric_device", (m, n, 9, Xx, Xp, Xj, spec, Zp, Zj, Zx),
             [(num, [H, m, n, 9, P(Xx), P(Xp), P(Xj), IS(spec), P(Zp), P(Zj), P(Zx), OD])], attrs={"select_ms": 1.25},
             fails={num: FAIL}, uninit=AttributeError))
    X32 = (Xp, Xj, tf(9, torch.float32))
    for nm, Xs, kw, nz, vdt in (("", X, {}, 37, torch.float64), ("_f32", X32, {}, 37, torch.float32), ("_nnzZ_0", X, {}, 0, torch.float64),
                                ("_no_values", X, {"values": False}, 37, None), ("_pattern", (Xp, Xj, None), {}, 37, None)):
        add(Case("csr_select_device" + nm, "csr_select_device", (m, n, Xs, spec),
                 ["sync", (sym, [H, m, n, 9, Xs[2] if Xs[2] is None else P(Xs[2]), P(Xp), P(Xj), IS(spec), RS(0), OI]),
                  "sync", (num, [H, m, n, 9, Xs[2] if Xs[2] is None else P(Xs[2]), P(Xp), P(Xj), IS(spec), RS(0), RS(1),
                                 RS(2) if vdt else None, OD])],
                 ret=(t_numel(m + 1, torch.int32), t_numel(nz, torch.int32), t_numel(nz, vdt) if vdt else None), kwargs=kw,
                 attrs={"select_ms": 1.25}, fails={sym: Raises(FAIL, sym), num: Raises(FAIL, num)}, uninit=AttributeError,
                 outs={sym: {9: nz}}))

    # ---- transpose ----
    Tp = ti(n + 1)
    tr = "bhs_csr_transpose_device"
    add(Case("csr_transpose_raw_device", "csr_transpose_raw_device", (m, n, 9, Xx, Xp, Xj, Tp, Zj, Zx, pm),
             [(tr, [H, m, n, 9, P(Xx), P(Xp), P(Xj), P(Tp), P(Zj), P(Zx), P(pm), OD])], attrs={"transpose_ms": 1.25},
             fails={tr: FAIL}, uninit=NR))
    add(Case("csr_transpose_raw_device_pattern", "csr_transpose_raw_device", (m, n, 9, None, Xp, Xj, Tp, Zj, None, None),
             [(tr, [H, m, n, 9, None, P(Xp), P(Xj), P(Tp), P(Zj), None, None, OD])], attrs={"transpose_ms": 1.25}))
    for nm, Xs, kw, vals, perm in (("", X, {}, True, False), ("_perm", X, {"perm": True}, True, True),
                                   ("_no_values", X, {"values": False}, False, False),
                                   ("_pattern", (Xp, Xj, None), {"perm": True}, False, True)):
        add(Case("csr_transpose_device" + nm, "csr_transpose_device", (m, n, Xs),
                 ["sync", "sync", (tr, [H, m, n, 9, Xs[2] if Xs[2] is None else P(Xs[2]), P(Xp), P(Xj), RS(0), RS(1),
                                        RS(2) if vals else None, RS(3) if perm else None, OD])],
                 ret=(t_numel(n + 1, torch.int32), t_numel(9, torch.int32), t_numel(9, torch.float64) if vals else None,
                      t_numel(9, torch.int32) if perm else None), kwargs=kw, attrs={"transpose_ms": 1.25},
                 fails={tr: Raises(FAIL, tr)}, uninit=Raises(NR, tr)))
    E = (ti(5) * 0, ti(0), tf(0))
    add(Case("csr_transpose_device_empty", "csr_transpose_device", (m, n, E),
             ["sync", "sync", (tr, [H, m, n, 0, None, P(E[0]), None, RS(0), RS(1), RS(2), RS(3), OD])],
             ret=(t_numel(n + 1, torch.int32), t_numel(0, torch.int32), t_numel(0, torch.float64), t_numel(0, torch.int32)),
             kwargs={"perm": True}, attrs={"transpose_ms": 1.25}))
    tv = "bhs_csr_transpose_values_device"
    pm9 = ti(9)
    add(Case("csr_transpose_values_device", "csr_transpose_values_device", (Xx, pm9),
             ["sync", (tv, [H, 9, P(Xx), P(pm9), RV(), OD])], ret=t_numel(9, torch.float64), attrs={"transpose_ms": 1.25},
             fails={tv: Raises(FAIL, tv)}, uninit=AttributeError))
    vT = tf(9)
    add(Case("csr_transpose_values_device_out", "csr_transpose_values_device", (Xx, pm9, vT),
             ["sync", (tv, [H, 9, P(Xx), P(pm9), P(vT), OD])], ret=lambda x: x is vT, attrs={"transpose_ms": 1.25}))
    add(Case("csr_transpose_values_device_empty", "csr_transpose_values_device", (tf(0), ti(0)),
             ["sync", (tv, [H, 0, None, None, RV(), OD])], ret=t_numel(0, torch.float64), attrs={"transpose_ms": 1.25}))

    # ---- extract ----
    sym, num = "bhs_csr_extract_symbolic_device", "bhs_csr_extract_numeric_device"
    rows, cols = ti(3), ti(2)
    Zp4 = ti(4)
    add(Case("csr_extract_symbolic_device", "csr_extract_symbolic_device", (m, n, 9, Xp, Xj, 3, rows, 2, cols, Zp4),
             [(sym, [H, m, n, 9, P(Xp), P(Xj), 3, P(rows), 2, P(cols), P(Zp4), OI])], ret=(0, 37), fails={sym: (FAIL, 37)},
             uninit=(NR, 0)))
    add(Case("csr_extract_symbolic_device_all_and_empty", "csr_extract_symbolic_device", (m, n, 9, Xp, Xj, m, None, 0, ti(0), Zp),
             [(sym, [H, m, n, 9, P(Xp), P(Xj), m, None, 0, NonNull(), P(Zp), OI])], ret=(0, 37)))
    add(Case("csr_extract_numeric_device", "csr_extract_numeric_device",
             (m, n, 9, Xx, Xp, Xj, 3, rows, 2, cols, 37, Zp4, Zj, Zx, pm),
             [(num, [H, m, n, 9, P(Xx), P(Xp), P(Xj), 3, P(rows), 2, P(cols), 37, P(Zp4), P(Zj), P(Zx), P(pm), OD])],
             attrs={"extract_ms": 1.25}, fails={num: FAIL}, uninit=NR))
    add(Case("csr_extract_numeric_device_empty_and_all", "csr_extract_numeric_device",
             (m, n, 9, None, Xp, Xj, 0, ti(0), n, None, 37, Zp4, Zj, None, None),
             [(num, [H, m, n, 9, None, P(Xp), P(Xj), 0, NonNull(), n, None, 37, P(Zp4), P(Zj), None, None, OD])],
             attrs={"extract_ms": 1.25}))
    add(Case("csr_extract_raw_device", "csr_extract_raw_device", (m, n, 9, Xx, Xp, Xj, 3, rows, 2, cols, Zp4, Zj, Zx, pm),
             [(sym, [H, m, n, 9, P(Xp), P(Xj), 3, P(rows), 2, P(cols), P(Zp4), OI]),
              (num, [H, m, n, 9, P(Xx), P(Xp), P(Xj), 3, P(rows), 2, P(cols), 37, P(Zp4), P(Zj), P(Zx), P(pm), OD])],
             ret=(0, 37), attrs={"extract_ms": 1.25}, fails={sym: (FAIL, 0), num: (FAIL, 37)}, uninit=(NR, 0)))
    e0 = ti(0)
    for nm, Xs, kw, nz, vals, perm, mI, r, nJ, cc in (
            ("", X, {"rows": rows, "cols": cols}, 37, True, False, 3, P(rows), 2, P(cols)),
            ("_all", X, {"perm": True}, 37, True, True, m, None, n, None),
            ("_nnzZ_0", X, {"rows": rows, "perm": True}, 0, True, True, 3, P(rows), n, None),
            ("_empty_lists", X, {"rows": e0, "cols": e0}, 0, True, False, 0, NonNull(), 0, NonNull()),
            ("_no_values", X, {"cols": cols, "values": False}, 37, False, False, m, None, 2, P(cols)),
            ("_pattern", (Xp, Xj, None), {"rows": rows}, 37, False, False, 3, P(rows), n, None)):
        vx = Xs[2] if Xs[2] is None else P(Xs[2])
        add(Case("csr_extract_device" + nm, "csr_extract_device", (m, n, Xs),
                 ["sync", (sym, [H, m, n, 9, P(Xp), P(Xj), mI, r, nJ, cc, RS(0), OI]),
                  "sync", (num, [H, m, n, 9, vx, P(Xp), P(Xj), mI, r, nJ, cc, nz, RS(0), RS(1), RS(2) if vals else None,
                                 RS(3) if perm else None, OD])],
                 ret=(t_numel(mI + 1, torch.int32), t_numel(nz, torch.int32), t_numel(nz, torch.float64) if vals else None,
                      t_numel(nz, torch.int32) if perm else None), kwargs=kw, attrs={"extract_ms": 1.25},
                 fails={sym: Raises(FAIL, sym), num: Raises(FAIL, num)}, uninit=Raises(NR, sym), outs={sym: {11: nz}}))

    # ---- reduce / scale ----
    rd, sc = "bhs_csr_reduce_device", "bhs_csr_scale_device"
    out, left, right = tf(4), tf(m), tf(n)
    add(Case("csr_reduce_raw_device", "csr_reduce_raw_device", (m, n, 9, Xx, Xp, Xj, 1, 4, 1, out),
             [(rd, [H, m, n, 9, P(Xx), P(Xp), P(Xj), 1, 4, 1, P(out), OD])], attrs={"reduce_ms": 1.25}, fails={rd: FAIL},
             uninit=NR))
    add(Case("csr_scale_raw_device", "csr_scale_raw_device", (m, n, 9, Xx, Xp, Xj, 2, left, right, 3, Zx),
             [(sc, [H, m, n, 9, P(Xx), P(Xp), P(Xj), 2.0, P(left), P(right), 3, P(Zx), OD])], attrs={"scale_ms": 1.25},
             fails={sc: FAIL}, uninit=NR))
    for axis, count in ((_lib.BHS_AXIS_ROWS, m), (_lib.BHS_AXIS_COLS, n), (_lib.BHS_AXIS_ALL, 1), (_lib.BHS_AXIS_DIAG, m)):
        add(Case("csr_reduce_device_axis_%d" % axis, "csr_reduce_device", (m, n, X, axis, _lib.BHS_RED_ABS_MAX),
                 ["sync", "sync", (rd, [H, m, n, 9, P(Xx), P(Xp), P(Xj), axis, _lib.BHS_RED_ABS_MAX, 0, RS(), OD])],
                 ret=t_numel(count, torch.float64), attrs={"reduce_ms": 1.25}, fails={rd: Raises(FAIL, rd)},
                 uninit=Raises(NR, rd)))
    add(Case("csr_reduce_device_offdiag_pattern_no_rows", "csr_reduce_device", (0, n, (Xp, Xj, None), 0, 6),
             ["sync", "sync", (rd, [H, 0, n, 9, None, P(Xp), P(Xj), 0, 6, _lib.BHS_RED_OFFDIAG, RS(), OD])],
             ret=t_numel(0, torch.float64), kwargs={"offdiag": True}, attrs={"reduce_ms": 1.25}))
    add(Case("csr_scale_device", "csr_scale_device", (m, n, X),
             ["sync", (sc, [H, m, n, 9, P(Xx), P(Xp), P(Xj), 1.0, None, None, 0, RV(), OD])], ret=t_numel(9, torch.float64),
             attrs={"scale_ms": 1.25}, fails={sc: Raises(FAIL, sc)}, uninit=Raises(NR, sc)))
    add(Case("csr_scale_device_in_place", "csr_scale_device", (m, n, X, 2.5, left, right, True, True, Xx),
             ["sync", (sc, [H, m, n, 9, P(Xx), P(Xp), P(Xj), 2.5, P(left), P(right), 3, P(Xx), OD])],
             ret=lambda x: x is Xx, attrs={"scale_ms": 1.25}))
    add(Case("csr_scale_device_right_div_f32", "csr_scale_device", (m, n, X32),
             ["sync", (sc, [H, m, n, 9, P(X32[2]), P(Xp), P(Xj), 1.0, None, P(right), 2, RV(), OD])],
             ret=t_numel(9, torch.float32), kwargs={"right": right, "right_div": True}, attrs={"scale_ms": 1.25}))
    add(Case("csr_scale_device_empty", "csr_scale_device", (m, n, E),
             ["sync", (sc, [H, m, n, 0, None, P(E[0]), None, 1.0, None, None, 0, RV(), OD])], ret=t_numel(0, torch.float64),
             attrs={"scale_ms": 1.25}))

    # ---- results ----
    Cj, Cx = i32(41), f64(41)
    add(Case("get_nnzC", "get_nnzC", (), [("bhs_get_nnzC", [H, OI])], ret=41, fails={"bhs_get_nnzC": 0}, uninit=0))
    add(Case("get_C", "get_C", (Cj, Cx), [("bhs_get_nnzC", [H, OI]), ("bhs_get_C", [H, P(Cj), P(Cx)]),
                                          ("bhs_get_rowptrC", [H, P(Cp)])],
             fails={"bhs_get_C": FAIL, "bhs_get_rowptrC": FAIL}, uninit=NR, setup=rp))
    add(Case("get_C_no_rowptrC", "get_C", (Cj, Cx), [("bhs_get_nnzC", [H, OI]), ("bhs_get_C", [H, P(Cj), P(Cx)])],
             setup=lambda bh: setattr(bh, "_rowptrC", None)))
    add(Case("get_C_small", "get_C", (i32(40), Cx), [("bhs_get_nnzC", [H, OI])], ret=IA))
    add(Case("get_C_wrong_dtype", "get_C", (Cj, Cx.astype(np.float32)), [("bhs_get_nnzC", [H, OI])], ret=IA))
    add(Case("get_C_nothing", "get_C", (None, None), [("bhs_get_nnzC", [H, OI]), ("bhs_get_C", [H, None, None])],
             outs={"bhs_get_nnzC": {1: 0}}, setup=lambda bh: setattr(bh, "_rowptrC", None)))
    add(Case("spgemm_symbolic", "spgemm_symbolic", (), [("bhs_spgemm_symbolic", [H, O64, OI])], attrs=mul,
             fails={"bhs_spgemm_symbolic": FAIL}, uninit=AttributeError))
    add(Case("set_output_device", "set_output_device", (Dev(0x100), 0x200, 55),
             [("bhs_set_output_device", [H, P(0x100), P(0x200), 55])], fails={"bhs_set_output_device": FAIL},
             uninit=AttributeError))
    add(Case("spgemm_numeric", "spgemm_numeric", (3, 9), [("bhs_spgemm_numeric", [H, 3, 9])],
             fails={"bhs_spgemm_numeric": FAIL}, uninit=AttributeError))
    add(Case("spgemm_finish", "spgemm_finish", (), [("bhs_spgemm_finish", [H, A(4)])], attrs={"stage_ms": ST4},
             fails={"bhs_spgemm_finish": FAIL}, uninit=AttributeError))
    add(Case("get_C_device", "get_C_device", (), [("bhs_get_C_device", [H, OV, OV, OV])], ret=(0x1000, 0x2000, 0x3000),
             fails={"bhs_get_C_device": Raises(FAIL, "bhs_get_C_device")}, uninit=AttributeError))
    add(Case("get_C_device_null", "get_C_device", (), [("bhs_get_C_device", [H, OV, OV, OV])], ret=(0x1000, 0, 0),
             outs={"bhs_get_C_device": {1: 0x1000}}))
    ct = "bhs_get_class_tables_device"
    add(Case("class_tables_device", "class_tables_device", (), [(ct, [H, OV, OV, OV, OI, OI, OI])],
             ret=(0x4000, 0x5000, 0x6000, 12, 34, True), fails={ct: Raises(FAIL, ct)}, uninit=AttributeError))
    ex = "bhs_expand_class_columns_device"
    add(Case("expand_class_columns_device", "expand_class_columns_device", (8, 16, 0x100, 0x200, 0x300, 24, 0x400, 0x500),
             [(ex, [None, 8, 16, P(0x100), P(0x200), P(0x300), 24, P(0x400), P(0x500)])], fails={ex: FAIL},
             uninit=AttributeError))
    add(Case("expand_class_columns_device_stream", "expand_class_columns_device",
             (8, 16, 0x100, 0x200, 0x300, 24, 0x400, 0x500, 0x77),
             [(ex, [P(0x77), 8, 16, P(0x100), P(0x200), P(0x300), 24, P(0x400), P(0x500)])]))
    so = "bhs_csr_sort_indices_device"
    add(Case("csr_sort_indices_device", "csr_sort_indices_device", (4, Xp, Xj, Xx), [(so, [H, 4, P(Xp), P(Xj), P(Xx)])],
             fails={so: FAIL}, uninit=NR))
    add(Case("csr_sort_indices_device_gpu_arrays", "csr_sort_indices_device", (4, 0x100, Dev(0x200), 0x300),
             ["sync", (so, [H, 4, P(0x100), P(0x200), P(0x300)])]))
    gr = "bhs_get_rowptrC"
    add(Case("get_rowptrC", "get_rowptrC", (), [(gr, [H, RS()])],
             ret=lambda x: isinstance(x, np.ndarray) and x.dtype == np.int32 and x.size == 5, fails={gr: Raises(FAIL, gr)},
             uninit=AttributeError, setup=lambda bh: setattr(bh, "_m", 4)))
    add(Case("get_rowptrC_out", "get_rowptrC", (Cp,), [(gr, [H, P(Cp)])], ret=lambda x: x is Cp))

    # ---- measurement, options ----
    arr = (_lib.KernelStat * 64)()
    gk = "bhs_get_kernel_stats"
    add(Case("kernel_stats_raw", "kernel_stats_raw", (arr,), [(gk, [H, IS(arr), 64])], ret=2, fails={gk: FAIL},
             uninit=AttributeError))
    add(Case("kernel_stats", "kernel_stats", (), [(gk, [H, KSArr(), 64])], ret=lambda x: x == KS, fails={gk: []},
             uninit=AttributeError))
    add(Case("set_option", "set_option", ("force_path", 2), [("bhs_set_option", [H, b"force_path", 2])],
             fails={"bhs_set_option": FAIL}, uninit=AttributeError))
    add(Case("set_option_bool", "set_option", ("no_pack32", True), [("bhs_set_option", [H, b"no_pack32", 1])]))
    add(Case("get_info", "get_info", ("max_row_a",), [("bhs_get_info", [H, b"max_row_a", O64])], ret=99,
             fails={"bhs_get_info": Raises(FAIL, "get_info(max_row_a)")}, uninit=AttributeError))
    add(Case("free_mem", "free_mem", (), [("bhs_free_data", [H])], fails={"bhs_free_data": FAIL}, uninit=NR,
             setup=lambda bh: setattr(bh, "_keep", (1, 2)), after=lambda bh: bh._keep is None))
    add(Case("freePlatform", "freePlatform", (), [("bhs_destroy", [H])], fails={"bhs_destroy": FAIL}, uninit=0,
             after=lambda bh: bh._h is None))
    return c


CASES = {c.name: c for c in _cases()}


@pytest.fixture
def fake(monkeypatch):
    lib = FakeLib()
    monkeypatch.setattr(facade._lib, "load", lambda f32=False: lib)
    monkeypatch.setattr(torch.cuda, "synchronize", lambda *a, **k: lib.events.append("sync"))
    return lib


def _handle(lib, init=True):
    bh = facade.bhsparse()
    if init:
        plats = [False] * facade.NUM_PLATFORMS
        plats[facade.BHSPARSE_HIP] = True
        assert bh.initPlatform(plats) == 0
        del lib.events[:]
    bh._m = 4
    for i, a in enumerate(ATTRS):
        setattr(bh, a, "before %d" % i)
    return bh


def _run(lib, case, want, init=True):
    """Call the method; returns (what it returned, the object).  want: a value, a Raises or an exception type."""
    bh = _handle(lib, init)
    if case.setup:
        case.setup(bh)
    meth = getattr(bh, case.method)
    if isinstance(want, Raises):
        with pytest.raises(facade.BhsparseError) as ei:
            meth(*case.args, **case.kwargs)
        assert ei.value.code == want.code and str(ei.value).startswith(want.where + " failed: %d" % want.code), ei.value
        return None, bh
    if isinstance(want, type):
        with pytest.raises(want):
            meth(*case.args, **case.kwargs)
        return None, bh
    ret = meth(*case.args, **case.kwargs)
    _check_ret(ret, want)
    return ret, bh


def _check_attrs(bh, attrs, wall):
    for i, a in enumerate(ATTRS):
        got = getattr(bh, a)
        if a == "time_ms" and wall:
            assert type(got) is float and got >= 0.0
        elif a in attrs:
            assert type(got) is type(attrs[a]) and got == attrs[a], (a, got)
        else:
            assert got == "before %d" % i, (a, got)


@pytest.mark.parametrize("name", sorted(CASES))
def test_call(fake, name):
    case = CASES[name]
    fake.outs.update({k: dict(v) for k, v in case.outs.items()})
    ret, bh = _run(fake, case, case.ret)
    _match_events(fake.events, case.events, ret)
    _check_attrs(bh, case.attrs if not isinstance(case.ret, Raises) else {}, case.attrs.get("time_ms") is WALL)
    if case.after:
        assert case.after(bh)


@pytest.mark.parametrize("name,fn", sorted((c.name, fn) for c in CASES.values() for fn in c.fails))
def test_failing_status(fake, name, fn):
    """The C function `fn` fails (its outputs are written all the same): the events end with that call, the method returns
    or raises what the case says, and no attribute changes (time_ms excepted where wall time is taken)."""
    case = CASES[name]
    fake.outs.update({k: dict(v) for k, v in case.outs.items()})
    fake.status[fn] = FAIL
    ret, bh = _run(fake, case, case.fails[fn])
    last = [i for i, e in enumerate(case.events) if e != "sync" and e[0] == fn][0]
    _match_events(fake.events, case.events[:last + 1], None)
    _check_attrs(bh, {}, case.attrs.get("time_ms") is WALL)
    if case.method == "freePlatform":
        assert bh._h is None


@pytest.mark.parametrize("name", sorted(c.name for c in CASES.values() if c.uninit is not None))
def test_before_initPlatform(fake, name):
    case = CASES[name]
    ret, bh = _run(fake, case, case.uninit, init=False)
    assert [e for e in fake.events if e != "sync"] == []
    _check_attrs(bh, {}, False)
    assert bh._h is None and bh._lib is None


def test_every_public_method_has_a_case():
    public = sorted(k for k, v in vars(facade.bhsparse).items() if not k.startswith("_"))
    covered = set(c.method for c in CASES.values()) | {"initPlatform", "decode_kernel_stats"}
    assert [k for k in public if k not in covered] == []
    stateless = {"initPlatform", "decode_kernel_stats"}
    assert [k for k in public if k not in stateless and not any(c.method == k and c.uninit is not None
                                                                for c in CASES.values())] == []


def test_initPlatform(fake):
    plats = [False] * facade.NUM_PLATFORMS
    bh = facade.bhsparse()
    assert bh.initPlatform(plats) == IA and fake.events == [] and bh._h is None and bh._lib is None
    plats[facade.BHSPARSE_CUDA] = True            # an alias of the HIP backend
    assert bh.initPlatform(plats, device=3) == 0
    _match_events(fake.events, [("bhs_create", [OV, 1, IN(C.c_int, 3)]), ("bhs_set_option", [H, b"kernel_stats", 1])], None)
    assert bh._lib is fake and bh._h.value == HANDLE
    del fake.events[:]
    bh = facade.bhsparse()
    bh.quiet = False
    assert bh.initPlatform(plats) == 0
    _match_events(fake.events, [("bhs_create", [OV, 1, IN(C.c_int, 0)]), ("bhs_set_option", [H, b"kernel_stats", 1]),
                                ("bhs_set_verbose", [H, 1])], None)
    del fake.events[:]
    fake.status["bhs_create"] = FAIL
    bh = facade.bhsparse()
    assert bh.initPlatform(plats) == FAIL and bh._h is None
    assert [e[0] for e in fake.events] == ["bhs_create"]


def test_float_handle_loads_the_float_library(monkeypatch):
    asked = []
    lib = FakeLib()
    monkeypatch.setattr(facade._lib, "load", lambda f32=False: asked.append(f32) or lib)
    monkeypatch.setattr(torch.cuda, "synchronize", lambda *a, **k: None)
    plats = [False] * facade.NUM_PLATFORMS
    plats[facade.BHSPARSE_HIP] = True
    for dt, f32 in ((np.float64, False), (np.float32, True)):
        bh = facade.bhsparse(value_dtype=dt)
        assert bh.initPlatform(plats) == 0 and asked[-1] == f32
    Mp, Mj = i32(5), i32(3)
    bh._m = 4
    assert bh.spgemm_masked(Mp, Mj).dtype == np.float32
    X = (ti(5), ti(9), tf(9, torch.float32))
    assert bh.csr_reduce_device(4, 6, X, _lib.BHS_AXIS_ROWS, _lib.BHS_RED_PLUS).dtype == torch.float32
    with pytest.raises(ValueError):
        facade.bhsparse(value_dtype=np.int32)


def test_decode_kernel_stats():
    arr = (_lib.KernelStat * 64)()
    for i, rec in enumerate(KS):
        for k, v in rec.items():
            setattr(arr[i], k, v.encode() if k == "name" else v)
    assert facade.bhsparse.decode_kernel_stats(arr, 2) == KS
    assert facade.bhsparse.decode_kernel_stats(arr, 1) == KS[:1]
    assert facade.bhsparse.decode_kernel_stats(arr, 0) == []
    for i in range(64):
        arr[i].name = b"k"
    assert len(facade.bhsparse.decode_kernel_stats(arr, 100)) == 64
