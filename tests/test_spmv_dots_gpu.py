"""bhs_csr_spmv_dots_device on the GPU, both builds: z has the bits of bhs_csr_spmv_device on the same arguments, the two
reductions are those of the stored z -- exact on small integers, within the bound of tests/valuecheck.py for ANY order of
K = m + 1 operations (a product and m additions) on real values --, repeat bit for bit, and are never written by a
refused call.  Reference: tests/relaxref.py (dots) and tests/spmvref.py."""
import numpy as np
import pytest
import torch

import relaxref as rr
import spmvref as sr
from helpers import wide_values
from test_spmv_gpu import MATRICES, PAD, SENTINEL, Dev, bits, int_dense, new_handle, same_numbers, tdt, up
from valuecheck import check_values

from benchmark_spgemm_using_csr_amd import _lib, dense
from benchmark_spgemm_using_csr_amd.facade import bhsparse

pytestmark = pytest.mark.gpu

DTYPES = (np.float64, np.float32)
INV = _lib.BHS_ERR_INVALID_ARG
UNTOUCHED = -123.25


@pytest.fixture(scope="module", params=DTYPES, ids=("f64", "f32"))
def hd(request):
    bh = new_handle(request.param)
    yield bh, request.param
    bh.freePlatform()


def call(bh, D, x, alpha=1.0, beta=0.0, y=None, w=None, in_place=False, w_is_x=False, want=0):
    """(z, dots) of the fused call and z of bhs_csr_spmv_device on the same arguments (numpy); dots prefilled"""
    m, n, t = D.m, D.n, tdt(D.dtype)
    dx = up(np.concatenate([x, [0]]), D.dtype)
    dy = None if y is None else up(np.concatenate([y, [0]]), D.dtype)
    dw = dx if w_is_x else (None if w is None else up(np.concatenate([w, [0]]), D.dtype))
    zbuf = torch.full((m + PAD,), SENTINEL, dtype=t).cuda()
    if in_place:
        zbuf[:m] = dy[:m]
    else:
        zbuf[:m] = float("nan")
    plain = torch.full((m + PAD,), SENTINEL, dtype=t).cuda()
    plain[:m] = dy[:m] if (y is not None and beta != 0.0) else float("nan")
    dots = np.full(2, UNTOUCHED)
    torch.cuda.synchronize()
    err = dense.csr_spmv_dots_raw_device(bh, m, n, D.nnz, D.d[2], D.d[0], D.d[1], alpha, dx, beta, zbuf if in_place else dy, zbuf, dw, dots)
    assert err == want, (err, want)
    assert bool((zbuf[m:] == SENTINEL).all()), "written past the end of z"
    if want:
        assert dots[0] == UNTOUCHED and dots[1] == UNTOUCHED, "dots written by a refused call"
        return None, dots, None
    fam = {s["name"] for s in bh.kernel_stats() if s["launches"] > 0}
    assert {"spmv_short", "dots_part", "dots_finish"} <= fam and bh.spmv_dots_ms >= 0.0
    assert dense.csr_spmv_raw_device(bh, m, n, D.nnz, D.d[2], D.d[0], D.d[1], alpha, dx, beta, plain) == 0
    if w is None and not w_is_x:
        assert dots[1] == UNTOUCHED, "dots[1] written without w"
    return zbuf[:m].cpu().numpy(), dots, plain[:m].cpu().numpy()


def check_dots(z, w, dots, exact, what):
    zz, wz, Szz, Swz = rr.dots(z, w)
    K = np.array([len(z) + 1])
    for got, ref, S in ((dots[0], zz, Szz),) + (((dots[1], wz, Swz),) if w is not None else ()):
        if exact:
            assert got == ref, (what, got, ref)
        else:
            check_values(np.array([ref]), np.array([S]), K, np.array([got]), "f64", what)


def test_ladder_z_has_the_product_bits_and_exact_dots(hd):
    bh, dtype = hd
    m, n, A = MATRICES["ladder 33..1025"]()
    D = Dev(m, n, A, dtype)
    x, y, w = int_dense(n, 1, 1)[:, 0], int_dense(m, 1, 2)[:, 0], int_dense(m, 1, 3)[:, 0]
    for alpha, beta, yy, in_place in ((1.0, 0.0, None, False), (-2.0, 1.0, y, False), (-1.0, 1.0, y, True), (1.0, 0.0, y, False)):
        z, dots, plain = call(bh, D, x, alpha, beta, yy, w, in_place)
        assert np.array_equal(bits(z), bits(plain)), (alpha, beta, in_place)
        same_numbers(z, sr.spmv(m, n, D.Ap, D.Aj, D.Ax, x, alpha, beta, yy, dtype)[0], (alpha, beta))
        check_dots(z, w, dots, True, (alpha, beta, in_place))
    z, dots, _ = call(bh, D, x, 1.0, 0.0, None, None)                # no w: dots[1] stays as it was
    check_dots(z, None, dots, True, "no w")


@pytest.mark.parametrize("m", (0, 1, 255, 256, 257, 6007))
def test_sizes_and_w_is_x(hd, m):
    bh, dtype = hd
    rng = np.random.default_rng(40 + m)
    lens = rng.integers(0, min(9, m + 1), m)
    if m >= 6007:
        lens[rng.choice(m, 3, replace=False)] = (33, 1025, 5000)
    from test_spmv_gpu import rows_matrix
    _, _, A = rows_matrix(lens, m, 50 + m)
    D = Dev(m, m, A, dtype)
    x, y = int_dense(m, 1, 4)[:, 0], int_dense(m, 1, 5)[:, 0]
    z, dots, plain = call(bh, D, x, 2.0, -1.0, y, None, w_is_x=True)
    assert np.array_equal(bits(z), bits(plain))
    check_dots(z, np.ascontiguousarray(x, dtype), dots, True, ("w is x", m))
    # real values: within the bound of any order
    r_ = lambda v: np.ascontiguousarray(v, dtype).astype(np.float64)   # noqa: E731
    D = Dev(m, m, (A[0], A[1], r_(wide_values(len(A[1]), rng))), dtype)
    x, y, w = r_(wide_values(m, rng)), r_(wide_values(m, rng)), r_(wide_values(m, rng))
    z, dots, plain = call(bh, D, x, -0.75, 1.5, y, w)
    assert np.array_equal(bits(z), bits(plain))
    check_dots(z, w, dots, False, ("real", m))
    again = call(bh, D, x, -0.75, 1.5, y, w)
    other = new_handle(dtype)
    try:
        fresh = call(other, D, x, -0.75, 1.5, y, w)
    finally:
        other.freePlatform()
    for z2, dots2, _ in (again, fresh):
        assert np.array_equal(bits(z), bits(z2)) and np.array_equal(bits(dots), bits(dots2)), m


def test_nan_and_infinities_propagate(hd):
    bh, dtype = hd
    m, n, A = MATRICES["rectangular"]()
    D = Dev(m, n, A, dtype)
    x, w = int_dense(n, 1, 6)[:, 0], np.ones(m)
    for special, where in ((np.nan, "x"), (np.inf, "x"), (np.nan, "w"), (-np.inf, "w")):
        xs, ws = x.copy(), w.copy()
        (xs if where == "x" else ws)[7] = special
        z, dots, plain = call(bh, D, xs, 1.0, 0.0, None, ws)
        assert np.array_equal(bits(z), bits(plain))
        zz, wz, _, _ = rr.dots(z, ws)
        for got, ref in ((dots[0], zz), (dots[1], wz)):
            assert (np.isnan(got) and np.isnan(ref)) or got == ref, (special, where, got, ref)
    assert np.isnan(dots[1]) or np.isinf(dots[1])


def test_refusals_never_write_dots(hd):
    bh, dtype = hd
    m, n, A = MATRICES["ladder 33..1025"]()
    Ap, Aj, Ax = A
    x, y, w = int_dense(n, 1, 7)[:, 0], int_dense(m, 1, 8)[:, 0], int_dense(m, 1, 9)[:, 0]
    bad = Aj.copy()
    bad[Ap[int(np.flatnonzero(np.diff(Ap) == 5000)[0])] + 100] = n
    p0 = Ap.copy(); p0[0] = 1
    for p, j in ((Ap, bad), (p0, Aj)):
        call(bh, Dev(m, n, (p, j, Ax), dtype), x, -1.0, 1.0, y, w, want=INV)
    D = Dev(m, n, A, dtype)
    t = tdt(dtype)
    dx, dy, dw = up(x, dtype), up(y, dtype), up(w, dtype)
    z = torch.full((m + PAD,), SENTINEL, dtype=t).cuda()
    dots = np.full(2, UNTOUCHED)
    torch.cuda.synchronize()

    def go(m=m, n=n, nnz=D.nnz, Ax=D.d[2], Ap=D.d[0], Aj=D.d[1], x=dx, beta=1.0, y=dy, z=z, w=dw, dots=dots):
        return dense.csr_spmv_dots_raw_device(bh, m, n, nnz, Ax, Ap, Aj, 1.0, x, beta, y, z, w, dots)
    codes = (go(m=-1), go(n=-1), go(nnz=-1), go(Ap=None), go(Aj=None), go(x=None), go(z=None), go(y=None), go(dots=None),
             go(z=dx), go(z=D.d[2]), go(z=dw), go(z=dy[1:]), go(y=z[1:]))
    assert all(c == INV for c in codes), codes
    assert dots[0] == UNTOUCHED and dots[1] == UNTOUCHED and bool((z == SENTINEL).all())
    assert go(beta=0.0, y=None) == 0 and dots[0] != UNTOUCHED         # a NULL y is legal where beta == 0
    assert dense.csr_spmv_dots_raw_device(bhsparse(dtype), 0, 0, 0, None, None, None, 1.0, None, 0.0, None, None, None, dots) == _lib.BHS_ERR_NOT_READY


@pytest.mark.parametrize("dtype", DTYPES)
def test_tensor_call(dtype):
    m, n, A = MATRICES["rectangular"]()
    D = Dev(m, n, A, dtype)
    x, b, w = int_dense(n, 1, 10)[:, 0], int_dense(m, 1, 11)[:, 0], int_dense(m, 1, 12)[:, 0]
    bh = new_handle(dtype)
    try:
        db = up(b, dtype)
        r, rr_, wr = dense.csr_spmv_dots_device(bh, m, n, D.d, up(x, dtype), -1.0, 1.0, db, up(w, dtype))
        want = sr.spmv(m, n, D.Ap, D.Aj, D.Ax, x, -1.0, 1.0, b, dtype)[0]
        same_numbers(r.cpu().numpy(), want, "residual")
        assert r.data_ptr() != db.data_ptr() and np.array_equal(db.cpu().numpy(), b.astype(dtype))   # out of place
        assert rr_ == float((want.astype(np.float64) ** 2).sum()) and wr == float((w * want.astype(np.float64)).sum())
        assert dense.csr_spmv_dots_device(bh, m, n, D.d, up(x, dtype))[2] is None
    finally:
        bh.freePlatform()
