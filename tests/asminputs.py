"""The inputs of tests/test_assemble_gpu.py (test infrastructure), made once per session (scantiles' cache) and shared by both
builds; tests/test_assemble_shapes.py asserts on the CPU that they have the roles claimed for them.

bins()         one matrix whose raw rows hold 0, 1, 32, 33, 1024, 1025, 4096 and 4100 triplets -- both sides of every limit of
               the library's three sort shapes and of the keys a workgroup holds in LDS -- with empty rows first, last and in
               between, a row that is one single run, and m no multiple of 64.  In the sorted row every row that has room
               carries a run of two at its start, at its end, across places 15 | 16 (a 16-lane boundary) and 63 | 64 (a wave
               boundary); the last column of the 1024-row is the first of the 1025-row.  Returned in generation order
               (sorted by row and column), with a shuffle and the reverse beside it.
tiles(step)    the triplets whose bitmap words ceil(nkept / 64) and whose rows m both take scantiles.COUNTS[step].
Values are integers in [-4, 4]; no run is longer than 5000, so every sum is exact in float."""
import numpy as np

import scantiles as st

BIN_LENS = (0, 1, 0, 32, 33, 1024, 1025, 0, 4096, 4100, 40, 0, 0)      # row 10: one single run
SINGLE_RUN_ROW = 10
TOUCHING = (5, 6)                                                    # the last column of the first is the first of the second
BIN_N = 12000
PAIR_AT = (0, 15, 63)                                                # and at L - 2
SHORT, WAVE, LDS_KEYS = 32, 1024, 4096                               # kTrShortL, kTrWaveL, kTrLdsMax
N_TILE_COLS = 200


def pair_places(L):
    """where in a sorted row of L triplets a run of two begins"""
    return sorted(p for p in set(PAIR_AT) | {L - 2} if 0 <= p and p + 1 < L)


def _row_columns(L, rng, lo, hi, pin):
    """L sorted columns in [lo, hi) with runs of two at pair_places(L); pin: "max" the greatest is hi - 1, "min" the
    smallest is lo"""
    want, counts, pos = set(pair_places(L)), [], 0
    while pos < L:
        c = 2 if pos in want else 1
        counts.append(c)
        pos += c
    assert pos == L
    d = np.sort(rng.choice(np.arange(lo, hi), len(counts), replace=False))
    if pin == "max":
        d[-1] = hi - 1
    if pin == "min":
        d[0] = lo
    return np.repeat(d, counts)


def bins():
    def make():
        rng = np.random.default_rng(4242)
        rows, cols = [], []
        for i, L in enumerate(BIN_LENS):
            if i == SINGLE_RUN_ROW:
                c = np.full(L, 7)
            elif i == TOUCHING[0]:
                c = _row_columns(L, rng, 0, BIN_N // 2 + 1, "max")
            elif i == TOUCHING[1]:
                c = _row_columns(L, rng, BIN_N // 2, BIN_N, "min")
            else:
                c = _row_columns(L, rng, 0, BIN_N, None)
            rows.append(np.full(L, i))
            cols.append(c)
        rows, cols = np.concatenate(rows).astype(np.int32), np.concatenate(cols).astype(np.int32)
        vals = rng.integers(-4, 5, len(rows)).astype(np.float64)
        return len(BIN_LENS), BIN_N, rows, cols, vals, rng.permutation(len(rows))
    return st.cached("asm bins", make)


def orders(count, shuffle):
    return {"shuffled": shuffle, "sorted": np.arange(count), "reversed": np.arange(count)[::-1].copy()}


def tile_sizes(step):
    """(m, nkept): both scanned counts take COUNTS[step] -- m rows, ceil(nkept / 64) bitmap words"""
    T = st.COUNTS[step]
    return T, 64 * T - (3 if T and T != st.SCAN_TILE else 0)


def tiles(step):
    def make():
        m, nnz = tile_sizes(step)
        rng = np.random.default_rng(900 + step)
        rows = np.minimum(m * rng.random(nnz) ** 2, max(m - 1, 0)).astype(np.int32)   # (skewed: short rows beside wave rows)
        cols = rng.integers(0, N_TILE_COLS, nnz).astype(np.int32)
        return m, N_TILE_COLS, rows, cols, rng.integers(-4, 5, nnz).astype(np.float64)
    return st.cached(("asm tiles", step), make)


def csr_triplets(Ap, Aj, Ax, seed):
    """the entries of a CSR matrix as shuffled triplets"""
    rows = np.repeat(np.arange(len(Ap) - 1), np.diff(np.asarray(Ap, np.int64))).astype(np.int32)
    o = np.random.default_rng(seed).permutation(len(rows))
    return rows[o], np.asarray(Aj, np.int32)[o], np.asarray(Ax)[o]
