"""The semiring multiply's rule (include/bhsparse_hip.h, "semiring multiply") restated in numpy, bit for bit:

  1. expand every product (i, k, j) of A(i,k) and B(k,j);
  2. form the product (x) in float64;
  3. encode order-preserving unsigned keys with integer operations (sign bit flipped for non-negative values, every bit
     for negative ones: -0 below +0; a NaN product takes the extreme key that wins the reduction);
  4. group by (row, column);
  5. reduce, decode and round once to the value type.

It is the reference of tests/test_semiring_gpu.py (the oracle only knows plus-times) and is itself pinned against a dense
triple loop in tests/test_semiring_abi.py."""
import numpy as np

from benchmark_spgemm_using_csr_amd import _lib

SEMIRINGS = dict(_lib.SEMIRINGS)
NEW = [k for k in SEMIRINGS if k != "plus_times"]                   # the semirings that run the new kernels
SIGN = np.uint64(1 << 63)
ALL1 = np.uint64(0xFFFFFFFFFFFFFFFF)


def identity(name):
    return {"plus_times": 0.0, "min_plus": np.inf, "max_plus": -np.inf, "max_times": -np.inf, "min_max": np.inf,
            "max_min": -np.inf, "or_and": 0.0, "plus_pair": 0.0}[name]


def encode(v):
    """float64 -> uint64 keys whose unsigned order is the values' order, -0 below +0 (NaNs: callers replace them)"""
    b = np.ascontiguousarray(v, np.float64).view(np.uint64)
    return np.where((b >> np.uint64(63)) != 0, ~b, b | SIGN)


def decode(k):
    k = np.ascontiguousarray(k, np.uint64)
    return np.where((k >> np.uint64(63)) != 0, k & ~SIGN, ~k).astype(np.uint64).view(np.float64)


def expand(m, A, B):
    """Every product: (row, column, a, b), in the order of A's entries and, within one, of the B row's entries."""
    Ap, Aj, Ax = (np.asarray(A[0], np.int64), np.asarray(A[1], np.int64), np.asarray(A[2], np.float64))
    Bp, Bj, Bx = (np.asarray(B[0], np.int64), np.asarray(B[1], np.int64), np.asarray(B[2], np.float64))
    arow = np.repeat(np.arange(m, dtype=np.int64), np.diff(Ap))
    lens = Bp[Aj + 1] - Bp[Aj]
    total = int(lens.sum())
    src = np.repeat(np.arange(len(Aj), dtype=np.int64), lens)      # the A entry of every product
    start = np.cumsum(lens) - lens
    pos = np.arange(total, dtype=np.int64) - np.repeat(start, lens) + np.repeat(Bp[Aj], lens)
    return arow[src], Bj[pos], Ax[src], Bx[pos]


def ordered(a, b, take_max):
    """max / min of two float64 arrays in the keys' order (-0 below +0); NaN where an operand is NaN"""
    ka, kb = encode(a), encode(b)
    k = np.maximum(ka, kb) if take_max else np.minimum(ka, kb)
    return np.where(np.isnan(a) | np.isnan(b), np.nan, decode(k))


def pattern(m, n, A, B):
    """The structural pattern of A·B as CSR (rows strictly ascending)."""
    r, c, _, _ = expand(m, A, B)
    key = np.unique(r * n + c)
    Cp = np.zeros(m + 1, np.int64)
    np.cumsum(np.bincount(key // n, minlength=m), out=Cp[1:])
    return Cp.astype(np.int32), (key % n).astype(np.int32)


def semiring_masked(name, m, n, A, B, Mp, Mj, dtype=np.float64):
    """C<M> = A (+).(x) B on M's pattern, as `dtype`.  A and B hold the values the library sees (for the float build:
    already rounded to float32)."""
    r, c, a, b = expand(m, A, B)
    key = r * n + c
    mrow = np.repeat(np.arange(m, dtype=np.int64), np.diff(np.asarray(Mp, np.int64)))
    mkey = mrow * n + np.asarray(Mj, np.int64)
    out = np.full(len(mkey), identity(name), np.float64)
    if len(key) == 0 or len(mkey) == 0:
        return out.astype(dtype)
    is_max = name.startswith("max")
    with np.errstate(all="ignore"):
        if name in ("min_plus", "max_plus"):
            p = a + b
        elif name in ("max_times", "plus_times"):
            p = a * b
        elif name == "min_max":
            p = ordered(a, b, True)
        elif name == "max_min":
            p = ordered(a, b, False)
        elif name == "or_and":
            p = ((a != 0) & (b != 0)).astype(np.float64)
        else:
            p = np.ones(len(a))
    order = np.argsort(key, kind="stable")
    skey = key[order]
    first = np.flatnonzero(np.concatenate([[True], skey[1:] != skey[:-1]]))
    ukey = skey[first]
    if name in ("plus_times", "plus_pair"):
        with np.errstate(all="ignore"):
            red = np.add.reduceat(p[order], first)
    elif name == "or_and":
        red = np.maximum.reduceat(p[order], first)
    else:
        k = np.where(np.isnan(p), ALL1 if is_max else np.uint64(0), encode(p))[order]
        red = decode((np.maximum if is_max else np.minimum).reduceat(k, first))
    loc = np.minimum(np.searchsorted(ukey, mkey), len(ukey) - 1)
    hit = ukey[loc] == mkey
    out[hit] = red[loc[hit]]
    with np.errstate(all="ignore"):
        return out.astype(dtype)                                    # the one rounding


def same_bits(got, want):
    """Bit for bit, NaNs compared as NaNs (which NaN is not specified)."""
    got, want = np.asarray(got), np.asarray(want)
    if got.dtype != want.dtype or got.shape != want.shape:
        return False
    gn, wn = np.isnan(got), np.isnan(want)
    if not np.array_equal(gn, wn):
        return False
    u = np.uint64 if got.dtype == np.float64 else np.uint32
    return np.array_equal(np.ascontiguousarray(got[~gn]).view(u), np.ascontiguousarray(want[~wn]).view(u))


def edge_values(rng, count, plus_safe=False, integers=False):
    """Reals of both signs with edge cases sprinkled in: explicit zeros of both signs and infinities (plus_safe: +Inf only,
    so that a + b is never Inf - Inf)."""
    v = rng.integers(-6, 7, count).astype(np.float64) if integers else rng.standard_normal(count) * 4.0
    u = rng.random(count)
    v[u < 0.05] = 0.0
    v[(u >= 0.05) & (u < 0.10)] = -0.0
    v[(u >= 0.10) & (u < 0.13)] = np.inf
    if not plus_safe:
        v[(u >= 0.13) & (u < 0.16)] = -np.inf
    return v
