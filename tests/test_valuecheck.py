"""CPU tests of the error-bound check (tests/valuecheck.py) and the real-value generators (helpers.real_values): a
result summed in any order in double passes, one whose products or sums were formed in float does not."""
import numpy as np
import pytest

from helpers import VALUE_KINDS, random_csr, real_values
from valuecheck import check_bounded, on_pattern, references


def _products(m, n, A, B):
    """Every product of A·B as (row * n + column, A value, B value)."""
    Ap, Aj, Ax = (np.asarray(x) for x in A)
    Bp, Bj, Bx = (np.asarray(x) for x in B)
    Ap, Bp = Ap.astype(np.int64), Bp.astype(np.int64)
    rows = np.repeat(np.arange(m), np.diff(Ap))
    lens = np.diff(Bp)[Aj]
    e = np.repeat(np.arange(len(Aj)), lens)
    first = np.cumsum(lens) - lens
    b = np.repeat(Bp[:-1][Aj], lens) + (np.arange(int(lens.sum())) - np.repeat(first, lens))
    return rows[e] * n + Bj[b], Ax[e], Bx[b]


def numpy_multiply(oracle, m, k, n, A, B, rng, prod=np.float64, acc=np.float64, out=np.float64):
    """C = A·B on the oracle's pattern, every product formed in `prod`, added one at a time in `acc` in a random
    order, the sums rounded to `out`: a stand-in for a kernel with atomics."""
    Cp, Cj, _ = oracle.spgemm(m, k, n, *A, *B)
    key, a, b = _products(m, n, A, B)
    ckey = np.repeat(np.arange(m, dtype=np.int64), np.diff(Cp)) * n + Cj
    pos = np.searchsorted(ckey, key)
    p = (a.astype(prod) * b.astype(prod)).astype(acc)
    o = rng.permutation(len(p))
    Cx = np.zeros(len(Cj), acc)
    np.add.at(Cx, pos[o], p[o])
    return Cp.astype(np.int32), Cj, Cx.astype(out)


def _case(kind, seed, f32=False):
    rng = np.random.default_rng(seed)
    m, k, n = 300, 250, 280
    A = random_csr(m, k, 0.06, rng, empty_rows=(0, 7))
    B = random_csr(k, n, 0.06, rng, empty_rows=(3,))
    k2, A, B = real_values(kind, k, A, B, rng, f32=f32)
    return m, k2, n, A, B, rng


def _f32(X):
    return (X[0], X[1], np.asarray(X[2], np.float32).astype(np.float64))


@pytest.mark.parametrize("kind", VALUE_KINDS)
def test_generators(kind, oracle):
    m, k, n, A, B, rng = _case(kind, 1)
    assert k == (500 if kind == "cancel" else 250)
    for X in (A, B):
        e = np.frexp(np.abs(X[2]))[1] - 1
        assert e.min() >= -20 and e.max() <= 20 and np.all(X[2] != 0)
    ref, S, K = references(oracle, m, k, n, A, B, "f64")
    assert K.max() >= 4
    rel = np.abs(ref[2]) / S
    if kind == "cancel":
        assert np.mean(rel < 2.0 ** -29) > 0.9          # C' = -2^-30 A (B o r): most entries far below their S
        assert K.min() >= 2 and np.all(K % 2 == 0)
    else:
        assert np.mean(rel > 2.0 ** -10) > 0.9


@pytest.mark.parametrize("kind", VALUE_KINDS)
def test_double_in_any_order_passes(kind, oracle):
    m, k, n, A, B, rng = _case(kind, 2)
    ref = oracle.spgemm(m, k, n, *A, *B)
    worst = 0.0
    for _ in range(3):
        got = numpy_multiply(oracle, m, k, n, A, B, rng)
        worst = max(worst, check_bounded(oracle, m, k, n, A, B, got, "f64"))
    print("%s: shuffled double sums, worst err/bound %.3g" % (kind, worst))
    assert worst > 0.0 or kind == "wide"                  # (the cancelling sums do round differently in another order)
    assert check_bounded(oracle, m, k, n, A, B, (ref[0].astype(np.int32), ref[1], ref[2]), "f64") == 0.0


@pytest.mark.parametrize("kind", VALUE_KINDS)
@pytest.mark.parametrize("where", ["products", "sums"])
def test_float_arithmetic_fails_the_double_bound(kind, where, oracle):
    m, k, n, A, B, rng = _case(kind, 3)
    got = numpy_multiply(oracle, m, k, n, A, B, rng, **({"prod": np.float32} if where == "products" else {"acc": np.float32}))
    with pytest.raises(AssertionError, match="over the bound"):
        check_bounded(oracle, m, k, n, A, B, got, "f64")


@pytest.mark.parametrize("kind", VALUE_KINDS)
def test_float_build_bounds(kind, oracle):
    """Float inputs: double products and sums rounded once meet f32_once; float products added in float meet only
    f32_atomic, and on cancelling sums they miss f32_once."""
    m, k, n, A, B, rng = _case(kind, 4, f32=True)
    A32, B32 = _f32(A), _f32(B)
    once = numpy_multiply(oracle, m, k, n, A32, B32, rng, out=np.float32)
    assert check_bounded(oracle, m, k, n, A, B, once, "f32_once") <= 1.0
    atomic = numpy_multiply(oracle, m, k, n, A32, B32, rng, prod=np.float32, acc=np.float32)
    assert check_bounded(oracle, m, k, n, A, B, atomic, "f32_atomic") <= 1.0
    if kind == "cancel":
        with pytest.raises(AssertionError, match="over the bound"):
            check_bounded(oracle, m, k, n, A, B, atomic, "f32_once")
    # a double-build result passes the float bounds of the same inputs only once they are rounded to float
    with pytest.raises(AssertionError, match="over the bound"):
        check_bounded(oracle, m, k, n, A, B, numpy_multiply(oracle, m, k, n, A, B, rng), "f32_once")


def test_nan_where_the_reference_is_finite_fails(oracle):
    m, k, n, A, B, rng = _case("wide", 5)
    Cp, Cj, Cx = numpy_multiply(oracle, m, k, n, A, B, rng)
    for bad in (np.nan, np.inf, -np.inf):
        x = Cx.copy()
        x[len(x) // 2] = bad
        with pytest.raises(AssertionError, match="differ in being"):
            check_bounded(oracle, m, k, n, A, B, (Cp, Cj, x), "f64")
    with pytest.raises(AssertionError, match="colIndC"):
        check_bounded(oracle, m, k, n, A, B, (Cp, Cj[::-1].copy(), Cx), "f64")


def test_non_finite_inputs_match_by_class(oracle):
    """NaN, +-Inf and explicit zeros in the inputs (0 x Inf = NaN): a reordered double result has the oracle's classes
    and passes; a NaN turned into an Inf does not."""
    m, k, n, A, B, rng = _case("wide", 6)
    Ax, Bx = A[2].copy(), B[2].copy()
    Ax[rng.integers(0, len(Ax), 3)] = np.nan
    Ax[rng.integers(0, len(Ax), 3)] = 0.0
    Bx[rng.integers(0, len(Bx), 4)] = np.inf
    Bx[rng.integers(0, len(Bx), 4)] = -np.inf
    Bx[rng.integers(0, len(Bx), 3)] = 0.0
    A, B = (A[0], A[1], Ax), (B[0], B[1], Bx)
    got = numpy_multiply(oracle, m, k, n, A, B, rng)
    ref = oracle.spgemm(m, k, n, *A, *B)[2]
    assert np.isnan(ref).sum() > 0 and np.isinf(ref).sum() > 0 and np.isfinite(ref).sum() > 0
    check_bounded(oracle, m, k, n, A, B, got, "f64")
    x = got[2].copy()
    x[np.flatnonzero(np.isnan(ref))[0]] = np.inf
    with pytest.raises(AssertionError, match="differ in being"):
        check_bounded(oracle, m, k, n, A, B, (got[0], got[1], x), "f64")


def test_masked_values_on_a_pattern(oracle):
    """With a mask, the entries of M that no product lands on must read exactly 0, and a NaN there fails."""
    m, k, n, A, B, rng = _case("wide", 7)
    Cp, Cj, Cx = numpy_multiply(oracle, m, k, n, A, B, rng)
    Mp = np.zeros(m + 1, np.int32)
    rows = [np.union1d(Cj[Cp[i]:Cp[i + 1]][::2], [i % n]).astype(np.int32) for i in range(m)]
    Mp[1:] = np.cumsum([len(r) for r in rows])
    Mj = np.concatenate(rows)
    val = on_pattern((Cp, Cj, Cx), n, Mp, Mj)
    assert check_bounded(oracle, m, k, n, A, B, val, "f64", mask=(Mp, Mj)) <= 1.0
    off = np.flatnonzero(on_pattern((Cp, Cj, np.ones(len(Cx))), n, Mp, Mj) == 0)
    assert len(off)
    v2 = val.copy(); v2[off[0]] = 1e-300
    with pytest.raises(AssertionError, match="over the bound"):
        check_bounded(oracle, m, k, n, A, B, v2, "f64", mask=(Mp, Mj))
    v2[off[0]] = np.nan
    with pytest.raises(AssertionError, match="differ in being"):
        check_bounded(oracle, m, k, n, A, B, v2, "f64", mask=(Mp, Mj))
