"""Values of a multiply against an a-priori error bound (test infrastructure).

Three products of the double-precision oracle bound the error of ANY summation order of an entry's K products,
FMA and atomics included (Higham, "Accuracy and Stability of Numerical Algorithms", 2nd ed., §3.1):

    ref = A·B,   S = |A|·|B|,   K = ones(A)·ones(B)        gamma_u(K) = K·u / (1 - K·u)

    mode "f64"        products and sums in double:  |got - ref| <= 2·gamma_{2^-53}(K)·S  (both sides carry gamma·S)
    mode "f32_once"   float inputs, products and sums in double, one rounding to float per entry:
                      |got - ref| <= 2^-24·|ref| + 2.1·gamma_{2^-53}(K)·S
    mode "f32_atomic" float inputs, products rounded to float and added with float atomics (§7's exceptions):
                      |got - ref| <= gamma_{2^-24}(K+1)·S + gamma_{2^-53}(K)·S

A kernel that forms its products or sums in float misses the f64 bound by about 10^8.  The inputs must keep every
product and partial sum far from underflow and overflow (helpers.real_values: exponents within +-20), so no absolute
term is needed.  Non-finite entries must match in class -- NaN, +Inf, -Inf in the same places: the class of an IEEE sum
does not depend on the order of its additions as long as no finite partial sum overflows.
"""
import numpy as np

MODES = ("f64", "f32_once", "f32_atomic")


def gamma(K, u):
    Ku = K * u
    return Ku / (1.0 - Ku)


def bound(mode, ref, S, K):
    K = K.astype(np.float64)
    if mode == "f64":
        return 2.0 * gamma(K, 2.0 ** -53) * S
    if mode == "f32_once":
        return 2.0 ** -24 * np.abs(ref) + 2.1 * gamma(K, 2.0 ** -53) * S
    if mode == "f32_atomic":
        return gamma(K + 1.0, 2.0 ** -24) * S + gamma(K, 2.0 ** -53) * S
    raise ValueError(mode)


def on_pattern(C, n, Mp, Mj):
    """The values of the CSR matrix C = (Cp, Cj, Cx) at the entries of the pattern (Mp, Mj), 0 where C has none."""
    Cp, Cj, Cx = C
    m = len(Mp) - 1
    ckey = np.repeat(np.arange(m, dtype=np.int64), np.diff(np.asarray(Cp, np.int64))) * n + np.asarray(Cj, np.int64)
    mkey = np.repeat(np.arange(m, dtype=np.int64), np.diff(np.asarray(Mp, np.int64))) * n + np.asarray(Mj, np.int64)
    out = np.zeros(len(mkey), np.float64)
    if len(ckey) and len(mkey):
        pos = np.minimum(np.searchsorted(ckey, mkey), len(ckey) - 1)
        hit = ckey[pos] == mkey
        out[hit] = np.asarray(Cx, np.float64)[pos[hit]]
    return out


def references(oracle, m, k, n, A, B, mode):
    """(ref, S, K) as CSR triples of the oracle; for the float build the inputs are rounded to float first."""
    assert mode in MODES, mode
    Ap, Aj, Ax = A
    Bp, Bj, Bx = B
    Ax, Bx = np.asarray(Ax, np.float64), np.asarray(Bx, np.float64)
    if mode != "f64":
        Ax, Bx = Ax.astype(np.float32).astype(np.float64), Bx.astype(np.float32).astype(np.float64)
    ref = oracle.spgemm(m, k, n, Ap, Aj, Ax, Bp, Bj, Bx)
    S = oracle.spgemm(m, k, n, Ap, Aj, np.abs(Ax), Bp, Bj, np.abs(Bx))[2]
    K = oracle.spgemm(m, k, n, Ap, Aj, np.ones_like(Ax), Bp, Bj, np.ones_like(Bx))[2]
    return ref, S, K


def _classes(x):
    return np.isnan(x), x == np.inf, x == -np.inf


def check_values(ref, S, K, got, mode, what=""):
    """got, ref, S, K: values of the same entries.  Asserts the class and bound conditions; returns the worst err/bound
    over the finite entries (0.0 when every finite entry is exact)."""
    got = np.asarray(got, np.float64)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    for name, r, g in zip(("NaN", "+Inf", "-Inf"), _classes(ref), _classes(got)):
        wrong = np.flatnonzero(r != g)
        assert len(wrong) == 0, "%s%s: %d entries differ in being %s (first at %d: got %r, ref %r)" % (
            what, mode, len(wrong), name, wrong[0], got[wrong[0]], ref[wrong[0]])
    fin = np.isfinite(ref)
    r, g = ref[fin], got[fin]
    b = bound(mode, r, S[fin], K[fin])
    err = np.abs(g - r)
    if not len(err):
        return 0.0
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(err == 0.0, 0.0, err / b)
    worst = int(np.argmax(ratio))
    assert ratio[worst] <= 1.0, "%s%s: %d entries over the bound; worst err/bound %.3g at entry %d (got %r, ref %r, S %r, K %d)" % (
        what, mode, int(np.count_nonzero(ratio > 1.0)), ratio[worst], int(np.flatnonzero(fin)[worst]), g[worst], r[worst],
        S[fin][worst], int(K[fin][worst]))
    return float(ratio[worst])


def check_bounded(oracle, m, k, n, A, B, got, mode, mask=None, what=""):
    """got = (Cp, Cj, Cx) of a multiply of A (m x k) and B (k x n): rowPtr and colInd bit-exact, values within the bound
    of `mode`.  With mask = (Mp, Mj), got is the masked multiply's valC on M's pattern instead.  Returns the worst
    err/bound."""
    ref, S, K = references(oracle, m, k, n, A, B, mode)
    if mask is not None:
        Mp, Mj = mask
        pat = lambda x: on_pattern((ref[0], ref[1], x), n, Mp, Mj)       # noqa: E731
        return check_values(pat(ref[2]), pat(S), pat(K), got, mode, what)
    Cp, Cj, Cx = got
    assert np.array_equal(np.asarray(Cp, np.int64), ref[0]), (what, "rowPtrC differs")
    assert np.array_equal(np.asarray(Cj, np.int32), ref[1]), (what, "colIndC differs")
    return check_values(ref[2], S, K, Cx, mode, what)
