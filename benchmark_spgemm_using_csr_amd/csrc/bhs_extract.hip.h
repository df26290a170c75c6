// bhs_extract.hip.h -- submatrix extraction and permutation of a CSR matrix, Z = X(rows, cols)
// (bhs_csr_extract_{symbolic,numeric}_device; the contract is worded in include/bhsparse_hip.h, "extract").
// Row i of Z holds the entries of X's row rows[i] whose column is named by cols, relabelled to their place in cols, in
// ascending order of that place; ties (duplicate pairs of X) keep the order of their position in X.  Values are moved,
// never computed on; no atomic touches an output array and the result does not depend on scheduling: a row's survivors
// are compacted stably (ballot + popcount, a scan for the long rows) and put in order by the key (place << 32 | position
// in X) only where the compacted sequence does not already ascend.
//
//   k_ex_map          rowPtrX monotone and within [0, nnz] over all of X, rows in [0, m), cols in [0, n); the inverse map
//                     inv[cols[j]] = j (cleared to -1 before) with one atomicCAS per entry of cols: the loser of a CAS is a
//                     repeated column.
//   k_ex_count        16 lanes per Z row, 256 Z rows per workgroup: the X row's bounds and columns (only rows that `rows`
//                     names are read), the survivors of every row of up to kExWaveL entries, the row's bin by the length
//                     of the X row, nnz(Z).  With a row pointer of Z (the numeric call) every count is compared with it.
//   k_ex_count_long   the rows k_ex_count queued as long, a workgroup per row
//   k_ex_fill_short   X rows of up to 32 entries, 16 lanes per row, both entries of a lane in registers: a survivor's place
//                     is the number of survivors whose key is below its own (shuffles within the group)
//   k_ex_fill_wave    up to 1024 entries, a wave per row: keys compacted into the wave's 8 KB of LDS, neighbour compare,
//                     wave_bitonic_sort in registers where the row does not ascend
//   k_ex_fill_long    a workgroup per row: keys compacted by chunks of 256 into LDS (up to kExLdsMax survivors) or into a
//                     scratch array beyond, the flip network of k_tr_fill_long where the row does not ascend
#pragma once
#include "bhs_kernels.hip.h"
#include "bhs_wave.hip.h"
#include "bhs_row_wave.hip.h"
#include "bhs_add.hip.h"

namespace bhs {

enum { kExShort = 0, kExWave = 1, kExLong = 2, kExBins = 3 };
constexpr int kExShortL = 32;         // short bin: two entries a lane of a 16-lane group
constexpr int kExWaveL = 1024;        // wave bin: the row's keys fit a wave's LDS slice (8 KB)
constexpr int kExLdsMax = 4096;       // long bin: keys of a Z row in LDS up to here
constexpr int kExG = 16;              // lanes per row of k_ex_count
constexpr int kExRows = 256;          // rows per workgroup of it

// counters of the extraction (ints of its own workspace block): Z rows per bin, error flag, the scan's ticket / longest row /
// total / histogram words, nnz(Z); then the rows put in order, spread over kExReordSlots counters a cache line apart (a
// workgroup adds to the one of its number: with every row reordered one counter would take half a million atomics in a row)
constexpr int kExReordSlots = 64, kExReordStride = 32;
enum { EX_COUNT = 0, EX_ERR = 4, EX_TICKET = 6, EX_MAXCNT = 7, EX_TOTAL = 8 /* u64 */, EX_SCANTOTAL = 10 /* i64 */,
       EX_SCANBINS = 12 /* kMaxBins */, EX_HEAD = 32 /* what the host reads after the count pass */, EX_REORD = 32,
       EX_INTS = 32 + kExReordSlots * kExReordStride };

__device__ __forceinline__ void ex_add_reordered(int* __restrict__ ctl, int rows)
{
    atomicAdd(ctl + EX_REORD + (int)(blockIdx.x % kExReordSlots) * kExReordStride, rows);
}

typedef unsigned long long ex_u64;

__global__ __launch_bounds__(256) void k_ex_map(int m, int n, int nnzX, const int* __restrict__ Xp, int mI, const int* __restrict__ rows,
                                                int nJ, const int* __restrict__ cols, int* __restrict__ inv, int* __restrict__ ctl)
{
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    bool bad = t == 0 && (Xp[0] != 0 || Xp[m] != nnzX);
    if (t < m) {
        const int a = Xp[t], b = Xp[t + 1];
        if (a < 0 || b < a || b > nnzX) bad = true;
    }
    if (rows && t < mI && (unsigned)rows[t] >= (unsigned)m) bad = true;
    if (cols && t < nJ) {
        const int c = cols[t];
        if ((unsigned)c >= (unsigned)n) bad = true;
        else if (atomicCAS(&inv[c], -1, (int)t) != -1) bad = true;   // (a repeated column)
    }
    if (__ballot(bad) != 0ull && (threadIdx.x & 63) == 0) atomicOr(ctl + EX_ERR, 1);
}

// Row zi of Z: where its row of X starts and how long it is (0 for a row index out of range or a row with bad bounds:
// nothing of such a row is read).  Returns whether it is bad.
__device__ __forceinline__ bool ex_row(int m, int nnzX, const int* __restrict__ Xp, const int* __restrict__ rows, int zi, int& x0,
                                       int& len)
{
    x0 = 0;
    len = 0;
    const int r = rows ? rows[zi] : zi;
    if ((unsigned)r >= (unsigned)m) return true;
    const int a = Xp[r], b = Xp[r + 1];
    if (a < 0 || b < a || b > nnzX) return true;
    x0 = a;
    len = b - a;
    return false;
}

// the place in cols of column c (-1: not named, or not a column of X); without a map every column keeps its number
__device__ __forceinline__ int ex_place(int c, int n, const int* __restrict__ inv)
{
    if ((unsigned)c >= (unsigned)n) return -1;
    return inv ? inv[c] : c;
}

// Thread t of the workgroup owns Z row rowBase + t whose X row has L entries: the row joins its bin's queue (see add_enqueue).
__device__ __forceinline__ void ex_enqueue(int mI, int zi, int L, int* sCnt, int* sBase, int* __restrict__ ctl, int* __restrict__ queue)
{
    const int tid = threadIdx.x;
    const int bin = (zi >= mI || L <= 0) ? -1 : L <= kExShortL ? kExShort : L <= kExWaveL ? kExWave : kExLong;
    int rank = 0;
    if (bin >= 0) rank = atomicAdd(&sCnt[bin], 1);
    __syncthreads();
    if (tid < kExBins && sCnt[tid]) sBase[tid] = atomicAdd(ctl + EX_COUNT + tid, sCnt[tid]);
    __syncthreads();
    if (bin >= 0) queue[(size_t)bin * mI + sBase[bin] + rank] = zi;
}

// does row zi of a given row pointer of Z hold c entries
__device__ __forceinline__ bool ex_zp_bad(const int* __restrict__ Zp, int zi, int c)
{
    if (!Zp) return false;
    const int z0 = Zp[zi];
    return z0 < 0 || Zp[zi + 1] - z0 != c;
}

__global__ __launch_bounds__(256) void k_ex_count(int m, int n, int nnzX, const int* __restrict__ Xp, const int* __restrict__ Xj,
                                                  int mI, const int* __restrict__ rows, const int* __restrict__ inv,
                                                  const int* __restrict__ Zp, int nnzZ, int* __restrict__ cnt, int* __restrict__ ctl,
                                                  int* __restrict__ queue)
{
    __shared__ int sRowCnt[kExRows], sRowLen[kExRows];
    __shared__ int sCnt[kExBins], sBase[kExBins];
    __shared__ unsigned long long sTot;
    const int tid = threadIdx.x, lane = tid & 63, sl = tid & (kExG - 1);
    if (tid < kExBins) sCnt[tid] = 0;
    if (tid == 0) sTot = 0;
    const int rowBase = blockIdx.x * kExRows;
    bool bad = blockIdx.x == 0 && tid == 0 && (Xp[0] != 0 || Xp[m] != nnzX || (Zp && (Zp[0] != 0 || Zp[mI] != nnzZ)));
    for (int it = 0; it < kExRows / (256 / kExG); ++it) {
        const int slot = it * (256 / kExG) + tid / kExG;
        const int zi = rowBase + slot;
        int c = 0, x0 = 0, len = 0;
        if (zi < mI) {
            if (ex_row(m, nnzX, Xp, rows, zi, x0, len)) bad = true;
            else if (len <= kExWaveL) {
                for (int q = x0 + sl; q < x0 + len; q += kExG) {
                    const int col = Xj[q];
                    if ((unsigned)col >= (unsigned)n) bad = true;
                    else c += (inv ? inv[col] >= 0 : true) ? 1 : 0;
                }
            }                                                     // (else k_ex_count_long counts and checks the row)
        }
#pragma unroll
        for (int o = kExG / 2; o >= 1; o >>= 1) c += __shfl_xor(c, o);
        if (sl == 0) { sRowCnt[slot] = c; sRowLen[slot] = len; }
    }
    __syncthreads();
    const int zi = rowBase + tid;
    const int c = sRowCnt[tid];
    if (zi < mI && sRowLen[tid] <= kExWaveL) {
        cnt[zi] = c;
        if (ex_zp_bad(Zp, zi, c)) bad = true;
    }
    if (__ballot(bad) != 0ull && lane == 0) atomicOr(ctl + EX_ERR, 1);
    long long t64 = c;                                            // (nnz(Z) may pass 2^31 with repeated rows: the host decides)
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) t64 += __shfl_xor(t64, o);
    if (lane == 0 && t64) atomicAdd(&sTot, (unsigned long long)t64);
    ex_enqueue(mI, zi, sRowLen[tid], sCnt, sBase, ctl, queue);
    if (tid == 0 && sTot) atomicAdd((unsigned long long*)(ctl + EX_TOTAL), sTot);
}

// The long rows of k_ex_count's queue, a workgroup per row; the number of rows is read from the device (the host has not
// seen it yet): the workgroups stride over the queue.
__global__ __launch_bounds__(256) void k_ex_count_long(int m, int n, int nnzX, const int* __restrict__ Xp, const int* __restrict__ Xj,
                                                       int mI, const int* __restrict__ rows, const int* __restrict__ inv,
                                                       const int* __restrict__ Zp, int* __restrict__ cnt, int* __restrict__ ctl,
                                                       const int* __restrict__ queue)
{
    __shared__ int sW[4];
    const int tid = threadIdx.x;
    const int nq = ctl[EX_COUNT + kExLong];
    for (int qi = blockIdx.x; qi < nq; qi += gridDim.x) {
        const int zi = queue[(size_t)kExLong * mI + qi];
        int x0, len;
        (void)ex_row(m, nnzX, Xp, rows, zi, x0, len);             // (bounds checked by k_ex_count)
        int c = 0;
        bool bad = false;
        for (int q = x0 + tid; q < x0 + len; q += 256) {
            const int col = Xj[q];
            if ((unsigned)col >= (unsigned)n) bad = true;
            else c += (inv ? inv[col] >= 0 : true) ? 1 : 0;
        }
        int tot;
        (void)add_scan_flags<256>(c, tid, sW, tot);
        if (tid == 0) {
            cnt[zi] = tot;
            if (tot) atomicAdd((unsigned long long*)(ctl + EX_TOTAL), (unsigned long long)tot);
            if (ex_zp_bad(Zp, zi, tot)) bad = true;
        }
        if (__ballot(bad) != 0ull && (tid & 63) == 0) atomicOr(ctl + EX_ERR, 1);
    }
}

// entry `at` of Z from its key
__device__ __forceinline__ void ex_emit(int at, ex_u64 key, int nnzX, int nnzZ, const value_t* __restrict__ Xx, int* __restrict__ Zj,
                                        value_t* __restrict__ Zx, int* __restrict__ perm)
{
    const unsigned pos = (unsigned)key;
    if (pos >= (unsigned)nnzX || (unsigned)at >= (unsigned)nnzZ) return;   // (never a key of this row; never a place of Z)
    Zj[at] = (int)(key >> 32);
    if (perm) perm[at] = (int)pos;
    if (Zx) Zx[at] = Xx[pos];
}

__device__ __forceinline__ ex_u64 ex_key(int place, int q) { return ((ex_u64)(unsigned)place << 32) | (unsigned)q; }

__global__ __launch_bounds__(256) void k_ex_fill_short(int nq, const int* __restrict__ queue, int m, int n, int nnzX,
                                                       const int* __restrict__ Xp, const int* __restrict__ Xj,
                                                       const value_t* __restrict__ Xx, const int* __restrict__ rows,
                                                       const int* __restrict__ inv, int nnzZ, const int* __restrict__ Zp,
                                                       int* __restrict__ Zj, value_t* __restrict__ Zx, int* __restrict__ perm,
                                                       int* __restrict__ ctl)
{
    const int tid = threadIdx.x, g = tid / 16, lane = tid & 15;
    const int qi = blockIdx.x * 16 + g;
    int x0 = 0, len = 0, z0 = 0, zlen = 0;
    if (qi < nq) {
        const int zi = queue[qi];
        if (!ex_row(m, nnzX, Xp, rows, zi, x0, len)) {
            z0 = Zp[zi];
            zlen = Zp[zi + 1] - z0;
        }
        if (len > kExShortL) len = 0;                             // (the binning keeps such rows out)
    }
    int j0 = -1, j1 = -1;
    if (lane < len) j0 = ex_place(Xj[x0 + lane], n, inv);
    if (16 + lane < len) j1 = ex_place(Xj[x0 + 16 + lane], n, inv);
    // where the stable compaction puts the survivors ...
    int tot0, tot1;
    const int c0 = add_scan_flags<16>(j0 >= 0 ? 1 : 0, tid, nullptr, tot0);
    const int c1 = tot0 + add_scan_flags<16>(j1 >= 0 ? 1 : 0, tid, nullptr, tot1);
    // ... and where their order does: the number of survivors with a smaller place, or the same place earlier in the row
    int r0 = 0, r1 = 0;
    for (int k = 0; k < 16; ++k) {
        const int a = __shfl(j0, k, 16), b = __shfl(j1, k, 16);
        r0 += (a >= 0 && (a < j0 || (a == j0 && k < lane))) ? 1 : 0;
        r0 += (b >= 0 && b < j0) ? 1 : 0;
        r1 += (a >= 0 && a <= j1) ? 1 : 0;
        r1 += (b >= 0 && (b < j1 || (b == j1 && k < lane))) ? 1 : 0;
    }
    const bool ok = tot0 + tot1 == zlen;                          // (else the row is not what rowPtrZ says: nothing of it is written)
    if (ok && j0 >= 0) ex_emit(z0 + r0, ex_key(j0, x0 + lane), nnzX, nnzZ, Xx, Zj, Zx, perm);
    if (ok && j1 >= 0) ex_emit(z0 + r1, ex_key(j1, x0 + 16 + lane), nnzX, nnzZ, Xx, Zj, Zx, perm);
    const bool moved = (j0 >= 0 && r0 != c0) || (j1 >= 0 && r1 != c1);
    const unsigned movedGrp = (unsigned)(__ballot(moved) >> ((tid & 63) & ~15)) & 0xffffu;
    const bool mine = qi < nq && lane == 0;
    if (__ballot(mine && !ok) != 0ull && (tid & 63) == 0) atomicOr(ctl + EX_ERR, 1);
    const int reordered = __popcll(__ballot(mine && ok && movedGrp != 0u));
    if (reordered && (tid & 63) == 0) ex_add_reordered(ctl, reordered);
}

template <int E>
__device__ __forceinline__ void ex_sort_row_wave(const ex_u64* key, int z0, int zlen, int lane, int nnzX, int nnzZ,
                                                 const value_t* __restrict__ Xx, int* __restrict__ Zj, value_t* __restrict__ Zx,
                                                 int* __restrict__ perm)
{
    ex_u64 x[E];
#pragma unroll
    for (int e = 0; e < E; ++e) {
        const int i = lane * E + e;
        x[e] = i < zlen ? key[i] : ~0ull;
    }
    wave_bitonic_sort<ex_u64, E>(x, lane);
#pragma unroll
    for (int e = 0; e < E; ++e) {
        const int i = lane * E + e;
        if (i < zlen) ex_emit(z0 + i, x[e], nnzX, nnzZ, Xx, Zj, Zx, perm);
    }
}

__global__ __launch_bounds__(256) void k_ex_fill_wave(int nq, const int* __restrict__ queue, int m, int n, int nnzX,
                                                      const int* __restrict__ Xp, const int* __restrict__ Xj,
                                                      const value_t* __restrict__ Xx, const int* __restrict__ rows,
                                                      const int* __restrict__ inv, int nnzZ, const int* __restrict__ Zp,
                                                      int* __restrict__ Zj, value_t* __restrict__ Zx, int* __restrict__ perm,
                                                      int* __restrict__ ctl)
{
    __shared__ ex_u64 sKey[4][kExWaveL];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int qi = blockIdx.x * 4 + w;
    if (qi >= nq) return;                                         // (wave-uniform, as everything below)
    const int zi = queue[qi];
    int x0, len;
    if (ex_row(m, nnzX, Xp, rows, zi, x0, len) || len > kExWaveL) {
        if (lane == 0) atomicOr(ctl + EX_ERR, 1);
        return;
    }
    const int z0 = Zp[zi], zlen = Zp[zi + 1] - z0;
    ex_u64* key = sKey[w];
    int out = 0;
    for (int t0 = 0; t0 < len; t0 += 64) {
        const int i = t0 + lane;
        const int j = i < len ? ex_place(Xj[x0 + i], n, inv) : -1;
        const unsigned long long bl = __ballot(j >= 0);
        const int at = out + __popcll(bl & ((1ull << lane) - 1ull));
        if (j >= 0) key[at] = ex_key(j, x0 + i);                  // (at < len <= kExWaveL)
        out += __popcll(bl);
    }
    if (out != zlen) {                                            // the row is not what rowPtrZ says: nothing of it is written
        if (lane == 0) atomicOr(ctl + EX_ERR, 1);
        return;
    }
    wave_sync();
    bool dis = false;
    for (int i = lane; i + 1 < zlen; i += 64) dis |= key[i] > key[i + 1];
    if (!__any(dis)) {                                            // already ascending: straight through
        for (int i = lane; i < zlen; i += 64) ex_emit(z0 + i, key[i], nnzX, nnzZ, Xx, Zj, Zx, perm);
        return;
    }
    if (lane == 0) ex_add_reordered(ctl, 1);
    if (zlen <= 64) ex_sort_row_wave<1>(key, z0, zlen, lane, nnzX, nnzZ, Xx, Zj, Zx, perm);
    else if (zlen <= 128) ex_sort_row_wave<2>(key, z0, zlen, lane, nnzX, nnzZ, Xx, Zj, Zx, perm);
    else if (zlen <= 256) ex_sort_row_wave<4>(key, z0, zlen, lane, nnzX, nnzZ, Xx, Zj, Zx, perm);
    else if (zlen <= 512) ex_sort_row_wave<8>(key, z0, zlen, lane, nnzX, nnzZ, Xx, Zj, Zx, perm);
    else ex_sort_row_wave<16>(key, z0, zlen, lane, nnzX, nnzZ, Xx, Zj, Zx, perm);
}

// len keys of buf (LDS or global) in ascending order, by the whole workgroup: the flip network of k_tr_fill_long
__device__ __forceinline__ void ex_block_sort(ex_u64* buf, int len, int tid)
{
    int P = 1;
    while (P < len) P <<= 1;
    auto cmpx = [&](int a, int b) {
        const ex_u64 x = buf[a], y = buf[b];
        if (x > y) { buf[a] = y; buf[b] = x; }
    };
    for (int k = 2; k <= P; k <<= 1) {
        const int hk = k >> 1;
        for (int i = tid; i < (P >> 1); i += 256) {               // flip: o-th element of a block with its mirror image
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

// keys: scratch of nnzZ words; a row of more than kExLdsMax survivors is compacted and ordered in its own slice of it
__global__ __launch_bounds__(256) void k_ex_fill_long(int nq, const int* __restrict__ queue, int m, int n, int nnzX,
                                                      const int* __restrict__ Xp, const int* __restrict__ Xj,
                                                      const value_t* __restrict__ Xx, const int* __restrict__ rows,
                                                      const int* __restrict__ inv, int nnzZ, const int* __restrict__ Zp, ex_u64* keys,
                                                      int* __restrict__ Zj, value_t* __restrict__ Zx, int* __restrict__ perm,
                                                      int* __restrict__ ctl)
{
    __shared__ ex_u64 ldsK[kExLdsMax];
    __shared__ int sW[4];
    const int tid = threadIdx.x;
    for (int qi = blockIdx.x; qi < nq; qi += gridDim.x) {         // (everything below is workgroup-uniform)
        const int zi = queue[qi];
        int x0, len;
        bool bad = ex_row(m, nnzX, Xp, rows, zi, x0, len);
        const int z0 = Zp[zi], zlen = Zp[zi + 1] - z0;
        if (z0 < 0 || zlen < 0 || (long long)z0 + zlen > nnzZ) bad = true;
        if (bad) {
            if (tid == 0) atomicOr(ctl + EX_ERR, 1);
            continue;
        }
        ex_u64* buf = zlen <= kExLdsMax ? ldsK : keys + z0;
        int out = 0;
        for (int t0 = 0; t0 < len; t0 += 256) {
            const int i = t0 + tid;
            const int j = i < len ? ex_place(Xj[x0 + i], n, inv) : -1;
            int tot;
            const int at = out + add_scan_flags<256>(j >= 0 ? 1 : 0, tid, sW, tot);
            if (j >= 0 && at < zlen) buf[at] = ex_key(j, x0 + i);
            out += tot;
        }
        __syncthreads();
        if (out != zlen) {                                        // the row is not what rowPtrZ says: nothing of it is written
            if (tid == 0) atomicOr(ctl + EX_ERR, 1);
            continue;
        }
        bool dis = false;
        for (int i = tid; i + 1 < zlen; i += 256) dis |= buf[i] > buf[i + 1];
        if (__syncthreads_or(dis ? 1 : 0)) {
            if (tid == 0) ex_add_reordered(ctl, 1);
            ex_block_sort(buf, zlen, tid);
        }
        for (int i = tid; i < zlen; i += 256) ex_emit(z0 + i, buf[i], nnzX, nnzZ, Xx, Zj, Zx, perm);
        __syncthreads();                                          // (ldsK is the next row's)
    }
}

}  // namespace bhs
