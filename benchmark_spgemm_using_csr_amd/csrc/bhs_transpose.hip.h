// bhs_transpose.hip.h -- the stable transpose of a CSR matrix (bhs_csr_transpose_device, bhs_csr_transpose_values_device; the
// contract is worded in include/bhsparse_hip.h, "transpose").  T = X^T: row j of T holds the entries of X with column j in
// the order of their position in X's arrays.  Values are moved, never computed on; no atomic touches an output array and
// the result does not depend on scheduling: atomics hand out places in a scratch array of keys, and every T row's keys are
// put in order before anything caller-owned is written from them.
//
//   k_tr_count     one pass over X, 16 lanes per row, 256 rows per workgroup: validity (rowPtr monotone and within [0, nnz],
//                  columns in [0, n); rows need not be ascending) and the histogram of the columns into n counters.  The
//                  workgroup takes the smallest and largest column of its rows; a window of up to kTrWin columns (stencils,
//                  bands, meshes: 256 consecutive rows touch a few hundred columns) is counted in LDS and flushed with one
//                  global atomic per touched column, anything wider with one global atomic per entry.  The window goes to
//                  a scratch word pair per workgroup: k_tr_scatter does not look for it again.
//   k_tr_bin       the T rows' bins by length, from the counts (queues as the selection's)
//   k_tr_scatter   the same mapping and window.  Inside the window the workgroup counts again in LDS, reserves per touched
//                  column a range of that T row with ONE returning global atomic and hands out the places of the range from
//                  LDS; outside it takes one returning global atomic per entry.  What is written is the 64-bit key
//                  (row << 32) | position in X.  Rows of X lie one behind the other, so the key is monotone in the position
//                  alone: ascending keys are the stable order, and the row index -- T's column -- comes with it.
//   k_tr_fill_*    a T row's keys in ascending order, then colIndT = key >> 32, perm = (int)key, valT = valX[perm]:
//                    short  rows of up to 32 entries, 16 lanes per row: an entry's place is the number of keys below its own
//                    wave   rows of up to 1024 entries, a wave per row: wave_bitonic_sort in registers
//                    long   a workgroup per row, the flip network of k_sort_rows_block; keys in LDS up to 4096 entries, in
//                           place in the scratch array beyond
//                  a wave / long row whose keys arrived in order is written straight through.
//   k_tr_values    valT[q] = valX[perm[q]], 16 bytes a lane where valT is aligned; a perm entry outside [0, nnz) raises the
//                  error word and is not followed.
#pragma once
#include "bhs_kernels.hip.h"
#include "bhs_wave.hip.h"
#include "bhs_row_wave.hip.h"

namespace bhs {

enum { kTrShort = 0, kTrWave = 1, kTrLong = 2, kTrBins = 3 };
constexpr int kTrShortL = 32;         // short bin: two keys a lane of a 16-lane group
constexpr int kTrWaveL = 1024;        // wave bin: 16 keys a lane
constexpr int kTrLdsMax = 4096;       // long bin: keys of a row in LDS up to here
constexpr int kTrG = 16;              // lanes per row of k_tr_count / k_tr_scatter
constexpr int kTrRows = 256;          // rows per workgroup of them
constexpr int kTrWin = 8192;          // columns of the LDS window (32 KB: four workgroups a CU)

// counters of the transpose (ints of its own workspace block): T rows per bin, error flag, the scan's ticket / longest row /
// total / histogram words
enum { TR_COUNT = 0, TR_ERR = 4, TR_TICKET = 6, TR_MAXCNT = 7, TR_SCANTOTAL = 8 /* i64 */, TR_SCANBINS = 12 /* kMaxBins */,
       TR_INTS = 32 };

typedef unsigned long long tr_u64;

// Thread t of the workgroup loads row rowBase + t: where it starts, how long it is (0 for a row with bad bounds: nothing of
// such a row is read).  Returns whether the row's bounds are bad.
__device__ __forceinline__ bool tr_load_rows(int m, int nnzX, const int* __restrict__ Xp, int rowBase, int* sX0, int* sLen)
{
    const int tid = threadIdx.x, row = rowBase + tid;
    int x0 = 0, len = 0;
    bool bad = false;
    if (row < m) {
        const int a = Xp[row], b = Xp[row + 1];
        if (a < 0 || b < a || b > nnzX) bad = true;
        else { x0 = a; len = b - a; }
    }
    sX0[tid] = x0;
    sLen[tid] = len;
    return bad;
}

__global__ __launch_bounds__(256) void k_tr_count(int m, int n, int nnzX, const int* __restrict__ Xp, const int* __restrict__ Xj,
                                                  int* __restrict__ cnt, int* __restrict__ ctl, int2* __restrict__ win)
{
    __shared__ int sTab[kTrWin];
    __shared__ int sX0[kTrRows], sLen[kTrRows];
    __shared__ int sMin, sMax;
    const int tid = threadIdx.x, lane = tid & 63, sl = tid & (kTrG - 1), grp = tid / kTrG;
    const int rowBase = blockIdx.x * kTrRows;
    bool bad = blockIdx.x == 0 && tid == 0 && (Xp[0] != 0 || Xp[m] != nnzX);
    bad |= tr_load_rows(m, nnzX, Xp, rowBase, sX0, sLen);
    if (tid == 0) { sMin = 0x7fffffff; sMax = -1; }
    __syncthreads();
    int mn = 0x7fffffff, mx = -1;
    for (int it = 0; it < kTrRows / (256 / kTrG); ++it) {
        const int slot = it * (256 / kTrG) + grp;
        const int x0 = sX0[slot], x1 = x0 + sLen[slot];
        for (int q = x0 + sl; q < x1; q += kTrG) {
            const int c = Xj[q];
            if (c < 0 || c >= n) bad = true;
            else { mn = min(mn, c); mx = max(mx, c); }
        }
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) { mn = min(mn, __shfl_xor(mn, o)); mx = max(mx, __shfl_xor(mx, o)); }
    if (lane == 0 && mx >= 0) { atomicMin(&sMin, mn); atomicMax(&sMax, mx); }
    if (__ballot(bad) != 0ull && lane == 0) atomicOr(ctl + TR_ERR, 1);
    __syncthreads();
    const int lo = sMin, hi = sMax;
    if (tid == 0) win[blockIdx.x] = make_int2(lo, hi);
    if (hi < 0) return;                                           // (no entry with a legal column)
    const bool inLds = hi - lo < kTrWin;
    if (inLds) {
        for (int i = tid; i <= hi - lo; i += 256) sTab[i] = 0;
        __syncthreads();
    }
    for (int it = 0; it < kTrRows / (256 / kTrG); ++it) {
        const int slot = it * (256 / kTrG) + grp;
        const int x0 = sX0[slot], x1 = x0 + sLen[slot];
        for (int q = x0 + sl; q < x1; q += kTrG) {
            const int c = Xj[q];
            if (c < lo || c > hi) continue;                       // (an illegal column: counted nowhere)
            if (inLds) atomicAdd(&sTab[c - lo], 1);
            else atomicAdd(&cnt[c], 1);
        }
    }
    if (inLds) {
        __syncthreads();
        for (int i = tid; i <= hi - lo; i += 256) {
            const int v = sTab[i];
            if (v) atomicAdd(&cnt[lo + i], v);
        }
    }
}

// The T rows' bins from their lengths; rows appended to per-bin queues with one atomic per workgroup and bin (see add_enqueue).
__global__ __launch_bounds__(256) void k_tr_bin(int n, const int* __restrict__ cnt, int* __restrict__ ctl, int* __restrict__ queue)
{
    __shared__ int sCnt[kTrBins], sBase[kTrBins];
    const int tid = threadIdx.x;
    if (tid < kTrBins) sCnt[tid] = 0;
    __syncthreads();
    const int row = blockIdx.x * 256 + tid;
    const int L = row < n ? cnt[row] : 0;
    const int bin = L <= 0 ? -1 : L <= kTrShortL ? kTrShort : L <= kTrWaveL ? kTrWave : kTrLong;
    int rank = 0;
    if (bin >= 0) rank = atomicAdd(&sCnt[bin], 1);
    __syncthreads();
    if (tid < kTrBins && sCnt[tid]) sBase[tid] = atomicAdd(ctl + TR_COUNT + tid, sCnt[tid]);
    __syncthreads();
    if (bin >= 0) queue[(size_t)bin * n + sBase[bin] + rank] = row;
}

// cur: a copy of rowPtrT, the next free place of every T row.  X has passed k_tr_count; the guards that remain keep a write
// inside the arrays whatever the input.
__global__ __launch_bounds__(256) void k_tr_scatter(int m, int nnzX, const int* __restrict__ Xp, const int* __restrict__ Xj,
                                                    int* __restrict__ cur, const int2* __restrict__ win, tr_u64* __restrict__ keys)
{
    __shared__ int sTab[kTrWin];
    __shared__ int sX0[kTrRows], sLen[kTrRows];
    const int tid = threadIdx.x, sl = tid & (kTrG - 1), grp = tid / kTrG;
    const int rowBase = blockIdx.x * kTrRows;
    (void)tr_load_rows(m, nnzX, Xp, rowBase, sX0, sLen);
    const int2 w = win[blockIdx.x];
    const int lo = w.x, hi = w.y;
    __syncthreads();
    if (hi < 0) return;
    const bool inLds = hi - lo < kTrWin;
    if (inLds) {
        for (int i = tid; i <= hi - lo; i += 256) sTab[i] = 0;
        __syncthreads();
        for (int it = 0; it < kTrRows / (256 / kTrG); ++it) {
            const int slot = it * (256 / kTrG) + grp;
            const int x0 = sX0[slot], x1 = x0 + sLen[slot];
            for (int q = x0 + sl; q < x1; q += kTrG) {
                const int c = Xj[q];
                if (c >= lo && c <= hi) atomicAdd(&sTab[c - lo], 1);
            }
        }
        __syncthreads();
        for (int i = tid; i <= hi - lo; i += 256) {               // the workgroup's range of every T row it touches
            const int v = sTab[i];
            if (v) sTab[i] = atomicAdd(&cur[lo + i], v);
        }
        __syncthreads();
    }
    for (int it = 0; it < kTrRows / (256 / kTrG); ++it) {
        const int slot = it * (256 / kTrG) + grp;
        const int x0 = sX0[slot], x1 = x0 + sLen[slot];
        for (int q = x0 + sl; q < x1; q += kTrG) {
            const int c = Xj[q];
            if (c < lo || c > hi) continue;
            const int at = inLds ? atomicAdd(&sTab[c - lo], 1) : atomicAdd(&cur[c], 1);
            if ((unsigned)at < (unsigned)nnzX) keys[at] = ((tr_u64)(unsigned)(rowBase + slot) << 32) | (unsigned)q;
        }
    }
}

// entry `at` of T from its key
__device__ __forceinline__ void tr_emit(int at, tr_u64 key, int nnzX, const value_t* __restrict__ Xx, int* __restrict__ Tj,
                                        value_t* __restrict__ Tx, int* __restrict__ perm)
{
    const unsigned pos = (unsigned)key;
    if (pos >= (unsigned)nnzX) return;                            // (never a key k_tr_scatter wrote)
    Tj[at] = (int)(key >> 32);
    if (perm) perm[at] = (int)pos;
    if (Tx) Tx[at] = Xx[pos];
}

__global__ __launch_bounds__(256) void k_tr_fill_short(int nq, const int* __restrict__ queue, int nnzX, const int* __restrict__ Tp,
                                                       const tr_u64* __restrict__ keys, const value_t* __restrict__ Xx,
                                                       int* __restrict__ Tj, value_t* __restrict__ Tx, int* __restrict__ perm)
{
    const int tid = threadIdx.x, g = tid / 16, lane = tid & 15;
    const int qi = blockIdx.x * 16 + g;
    int t0 = 0, len = 0;
    if (qi < nq) {
        const int row = queue[qi];
        t0 = Tp[row];
        len = Tp[row + 1] - t0;
        if (len > kTrShortL) len = 0;                             // (the binning keeps such rows out)
    }
    // positions in X are distinct: an entry's place in its row is the number of positions below its own
    tr_u64 key[2] = {~0ull, ~0ull};
#pragma unroll
    for (int e = 0; e < 2; ++e)
        if (e * 16 + lane < len) key[e] = keys[t0 + e * 16 + lane];
    const unsigned p0 = (unsigned)key[0], p1 = (unsigned)key[1];
    int r0 = 0, r1 = 0;
    for (int j = 0; j < 16; ++j) {
        const unsigned a = (unsigned)__shfl((int)p0, j, 16), b = (unsigned)__shfl((int)p1, j, 16);
        r0 += (a < p0 ? 1 : 0) + (b < p0 ? 1 : 0);
        r1 += (a < p1 ? 1 : 0) + (b < p1 ? 1 : 0);
    }
    if (lane < len) tr_emit(t0 + r0, key[0], nnzX, Xx, Tj, Tx, perm);
    if (16 + lane < len) tr_emit(t0 + r1, key[1], nnzX, Xx, Tj, Tx, perm);
}

template <int E>
__device__ __forceinline__ void tr_sort_row_wave(int t0, int len, int lane, int nnzX, const tr_u64* __restrict__ keys,
                                                 const value_t* __restrict__ Xx, int* __restrict__ Tj, value_t* __restrict__ Tx,
                                                 int* __restrict__ perm)
{
    tr_u64 x[E];
#pragma unroll
    for (int e = 0; e < E; ++e) {
        const int i = lane * E + e;
        x[e] = i < len ? keys[t0 + i] : ~0ull;
    }
    wave_bitonic_sort<tr_u64, E>(x, lane);
#pragma unroll
    for (int e = 0; e < E; ++e) {
        const int i = lane * E + e;
        if (i < len) tr_emit(t0 + i, x[e], nnzX, Xx, Tj, Tx, perm);
    }
}

__global__ __launch_bounds__(256) void k_tr_fill_wave(int nq, const int* __restrict__ queue, int nnzX, const int* __restrict__ Tp,
                                                      const tr_u64* __restrict__ keys, const value_t* __restrict__ Xx,
                                                      int* __restrict__ Tj, value_t* __restrict__ Tx, int* __restrict__ perm)
{
    const int lane = threadIdx.x & 63;
    const int qi = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (qi >= nq) return;                                         // (wave-uniform)
    const int row = queue[qi];
    const int t0 = Tp[row], len = Tp[row + 1] - t0;
    bool bad = false;
    for (int i = lane; i + 1 < len; i += 64) bad |= keys[t0 + i] > keys[t0 + i + 1];
    if (!__any(bad)) {                                            // arrived in order: straight through
        for (int i = lane; i < len; i += 64) tr_emit(t0 + i, keys[t0 + i], nnzX, Xx, Tj, Tx, perm);
    }
    else if (len <= 64) tr_sort_row_wave<1>(t0, len, lane, nnzX, keys, Xx, Tj, Tx, perm);
    else if (len <= 128) tr_sort_row_wave<2>(t0, len, lane, nnzX, keys, Xx, Tj, Tx, perm);
    else if (len <= 256) tr_sort_row_wave<4>(t0, len, lane, nnzX, keys, Xx, Tj, Tx, perm);
    else if (len <= 512) tr_sort_row_wave<8>(t0, len, lane, nnzX, keys, Xx, Tj, Tx, perm);
    else if (len <= kTrWaveL) tr_sort_row_wave<16>(t0, len, lane, nnzX, keys, Xx, Tj, Tx, perm);
}

// keys is written: a row beyond kTrLdsMax entries is ordered in place there
__global__ __launch_bounds__(256) void k_tr_fill_long(int nq, const int* __restrict__ queue, int nnzX, const int* __restrict__ Tp,
                                                      tr_u64* keys, const value_t* __restrict__ Xx, int* __restrict__ Tj,
                                                      value_t* __restrict__ Tx, int* __restrict__ perm)
{
    __shared__ tr_u64 ldsK[kTrLdsMax];
    const int tid = threadIdx.x;
    for (int qi = blockIdx.x; qi < nq; qi += gridDim.x) {
        const int row = queue[qi];
        const int t0 = Tp[row], len = Tp[row + 1] - t0;
        tr_u64* g = keys + t0;
        bool bad = false;
        for (int i = tid; i + 1 < len; i += 256) bad |= g[i] > g[i + 1];
        tr_u64* buf = g;
        if (__syncthreads_or(bad ? 1 : 0)) {
            if (len <= kTrLdsMax) {
                buf = ldsK;
                for (int i = tid; i < len; i += 256) buf[i] = g[i];
            }
            __syncthreads();
            int P = 1;
            while (P < len) P <<= 1;
            auto cmpx = [&](int a, int b) {
                const tr_u64 x = buf[a], y = buf[b];
                if (x > y) { buf[a] = y; buf[b] = x; }
            };
            for (int k = 2; k <= P; k <<= 1) {
                const int hk = k >> 1;
                for (int i = tid; i < (P >> 1); i += 256) {       // flip: o-th element of a block with its mirror image
                    const int blk = i / hk, o = i - blk * hk;
                    const int a = blk * k + o, b = blk * k + k - 1 - o;
                    if (b < len) cmpx(a, b);
                }
                __syncthreads();
                for (int j = k >> 2; j > 0; j >>= 1) {
                    for (int i = tid; i < (P >> 1); i += 256) {
                        const int a = (i / j) * 2 * j + (i % j), b = a + j;
                        if (b < len) cmpx(a, b);
                    }
                    __syncthreads();
                }
            }
        }
        for (int i = tid; i < len; i += 256) tr_emit(t0 + i, buf[i], nnzX, Xx, Tj, Tx, perm);
        __syncthreads();                                          // (ldsK is the next row's)
    }
}

// ---- the values alone ----
constexpr int kTrVec = 16 / (int)sizeof(value_t);
struct alignas(16) tr_vec { value_t v[kTrVec]; };

__global__ __launch_bounds__(256) void k_tr_values(int nnzX, const value_t* __restrict__ Xx, const int* __restrict__ perm,
                                                   value_t* __restrict__ Tx, int vec, int* __restrict__ ctl)
{
    bool bad = false;
    const long long stride = (long long)gridDim.x * 256;
    const int nv = vec ? nnzX / kTrVec : 0;                       // 16-byte pieces (Tx is aligned), then the rest one by one
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < nv; i += stride) {
        tr_vec o;
#pragma unroll
        for (int e = 0; e < kTrVec; ++e) {
            const int p = perm[i * kTrVec + e];
            const bool ok = (unsigned)p < (unsigned)nnzX;
            bad |= !ok;
            o.v[e] = ok ? Xx[p] : (value_t)0;
        }
        *reinterpret_cast<tr_vec*>(Tx + i * kTrVec) = o;
    }
    for (long long q = (long long)nv * kTrVec + (long long)blockIdx.x * 256 + threadIdx.x; q < nnzX; q += stride) {
        const int p = perm[q];
        const bool ok = (unsigned)p < (unsigned)nnzX;
        bad |= !ok;
        if (ok) Tx[q] = Xx[p];
    }
    if (__ballot(bad) != 0ull && (threadIdx.x & 63) == 0) atomicOr(ctl + TR_ERR, 1);
}

}  // namespace bhs
