"""One long-lived handle across multiply -> relax -> dots -> colouring -> relax -> multiply: every result is a fresh
handle's, and C, the options and "class_state" survive the new calls."""
import numpy as np
import pytest
import torch

from conftest import load_golden
from test_spmv_gpu import bits, new_handle, up

from benchmark_spgemm_using_csr_amd import amg, dense

pytestmark = pytest.mark.gpu

KEYS = ("class_state", "mixed_rows", "spec_launches", "spec_refuted", "b_sorted", "max_row_a", "max_row_b")


@pytest.mark.parametrize("dtype", (np.float64, np.float32), ids=("f64", "f32"))
def test_one_handle_across_the_calls(dtype):
    g = load_golden("p9_12.npz")
    m, kk, n = int(g["m"]), int(g["k"]), int(g["n"])
    assert m == kk == n
    rng = np.random.default_rng(15)
    Ap, Aj = (np.ascontiguousarray(g[key], np.int32) for key in ("Ap", "Aj"))
    Ax = np.ascontiguousarray(rng.integers(1, 5, len(Aj)), dtype)
    A = (up(Ap, np.int32), up(Aj, np.int32), up(Ax, dtype))
    diag = up(np.full(m, 8.0), dtype)
    b, x0, w = (up(rng.standard_normal(m), dtype) for _ in range(3))
    coef = amg.chebyshev_coefficients(0.3, 1.1, 3)

    def multiply(bh):
        Cp = np.zeros(m + 1, np.int32)
        assert bh.initData(m, kk, n, len(Aj), Ax, Ap, Aj, len(Aj), Ax, Ap, Aj, Cp) == 0
        assert bh.spgemm() == 0 and bh.spgemm() == 0
        nnzC = bh.get_nnzC()
        Cj, Cx = np.empty(nnzC, np.int32), np.empty(nnzC, dtype)
        assert bh.get_C(Cj, Cx) == 0
        return Cp, Cj, Cx

    def relax(bh, zero):
        x, d = x0.clone(), torch.zeros_like(x0)
        amg.relax_device(bh, A, diag, b, x, coef, d, zero_guess=zero)
        return x.cpu().numpy(), d.cpu().numpy()

    def dots(bh):
        z, zz, wz = dense.csr_spmv_dots_device(bh, m, n, A, x0, -1.0, 1.0, b, w)
        return z.cpu().numpy(), np.array([zz, wz])

    def colour(bh):
        color, ncolors, order, ptr = amg.color_device(bh, m, (A[0], A[1]), 0)
        return color.cpu().numpy(), np.array([ncolors]), order.cpu().numpy(), ptr

    fresh = {}
    for key, fn in (("multiply", multiply), ("relax", lambda h: relax(h, False)), ("dots", dots), ("colour", colour),
                    ("relax zero", lambda h: relax(h, True))):
        h = new_handle(dtype, {"class_path": 2})
        try:
            fresh[key] = fn(h)
        finally:
            h.freePlatform()

    def same(got, want, what):
        for a, c in zip(got, want):
            assert a.dtype == c.dtype and np.array_equal(bits(a) if a.dtype.kind == "f" else a, bits(c) if c.dtype.kind == "f" else c), what

    bh = new_handle(dtype, {"class_path": 2})
    try:
        C = multiply(bh)
        same(C, fresh["multiply"], "multiply")
        before = {key: bh.get_info(key) for key in KEYS}
        ptrs, nnzC = bh.get_C_device(), bh.get_nnzC()

        def unchanged(what):
            assert {key: bh.get_info(key) for key in KEYS} == before, what
            assert bh.get_C_device() == ptrs and bh.get_nnzC() == nnzC, what
            Cj, Cx = np.empty(nnzC, np.int32), np.empty(nnzC, dtype)
            assert bh.get_C(Cj, Cx) == 0 and np.array_equal(Cj, C[1]) and np.array_equal(bits(Cx), bits(C[2])), what
        same(relax(bh, False), fresh["relax"], "relax")
        unchanged("after relax")
        same(dots(bh), fresh["dots"], "dots")
        unchanged("after dots")
        same(colour(bh), fresh["colour"], "colour")
        same(relax(bh, True), fresh["relax zero"], "relax zero")
        unchanged("after the second relax")
        assert bh.spgemm() == 0
        Cj, Cx = np.empty(nnzC, np.int32), np.empty(nnzC, dtype)
        assert bh.get_nnzC() == nnzC and bh.get_C(Cj, Cx) == 0
        assert np.array_equal(Cj, C[1]) and np.array_equal(bits(Cx), bits(C[2]))
        bh.free_mem()
    finally:
        bh.freePlatform()
