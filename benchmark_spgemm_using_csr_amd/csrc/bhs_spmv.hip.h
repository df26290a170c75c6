// bhs_spmv.hip.h -- CSR x dense: y = alpha A x + beta y and Y = alpha A X + beta Y for k columns
// (bhs_csr_spmv_device, bhs_csr_spmm_device; the contract is worded in include/bhsparse_hip.h, "CSR x dense").
//
// Rows are binned by length exactly as the reductions bin them (bhs_reduce.hip.h: its constants, its control words, its
// row-pointer check and its queues are used as they are):
//
//   k_mv_short   all rows in order, 256 rows a workgroup: the row pointer's validation (every row), the rows of up to 32
//                entries on the spot, the longer ones queued for
//   k_mv_wave    up to 1024 entries, a wave per row, and
//   k_mv_long    a workgroup per row.
//
// Every kernel is a template of the column tile T (1, 2, 4, .. 64): the lanes that work on a row lie along T columns of X
// first -- lane l of them holds column c0 + l % T and entry slot l / T --, so one entry's gather is ONE contiguous read
// of T values of X's row, and the entry itself (column, value) is one address for the T lanes that share a slot.  T = 1 is
// the vector product: 16 lanes a short row, each entry its own gather.  k beyond the widest tile loops over tiles of 64;
// a k that is no tile multiple masks the tail (those lanes read nothing and store nothing).
//
// Arithmetic: products double(a) * double(x) summed in double from +0 -- a lane adds its slot's entries in row order, the
// slots of a column meet in a DPP / permlane butterfly (both partners of a step compute the same bits), the four waves of
// k_mv_long in LDS in wave order -- then t = alpha * s, t += beta * double(y_old) only where beta != 0, one rounding.  The
// order is a function of the row's length and T alone: no atomics on an output, two calls give the same bits.
//
// Validation precedes every dependent read: a row whose bounds the row pointer's check refuses is not read at all, a column
// outside [0, n) is never an index into X; both raise ctl[RD_ERR].  Stores go to (r, c) with r < m and c < k only.
#pragma once
#include "bhs_reduce.hip.h"

namespace bhs {

struct MvDims {
    int m, n, nnzA, k;
    long long ldX, ldY;
    double alpha, beta;
};

// lanes that share a short row: a DPP row of 16, or the tile where it is wider
template <int T> constexpr int mv_group() { return T > kRdG ? T : kRdG; }

// the sum over the W / T entry slots of every column of the tile, W = 16, 32 or 64 lanes a row (all lanes active); every
// lane of a column ends with the same bits
template <int T, int W>
__device__ __forceinline__ double mv_lanes(double s, int lane)
{
    rd_u64 v = rd_bits(s);
    if constexpr (T <= 1 && W > 1) v = rd_comb<kRdSum>(v, lane_xor64<1>(v, lane));
    if constexpr (T <= 2 && W > 2) v = rd_comb<kRdSum>(v, lane_xor64<2>(v, lane));
    if constexpr (T <= 4 && W > 4) v = rd_comb<kRdSum>(v, lane_xor64<4>(v, lane));
    if constexpr (T <= 8 && W > 8) v = rd_comb<kRdSum>(v, lane_xor64<8>(v, lane));
    if constexpr (T <= 16 && W > 16) v = rd_comb<kRdSum>(v, lane_xor64<16>(v, lane));
    if constexpr (T <= 32 && W > 32) v = rd_comb<kRdSum>(v, lane_xor64<32>(v, lane));
    return rd_real(v);
}

// entries a + slot, a + slot + step, .. of a row of len entries against column `col` (below k) of X, added in that order.
// B entries at a time: their columns first, then their values and gathers together -- one dependent round of loads per
// batch instead of one per entry (a lane of a 16-column tile walks a whole short row by itself).  B = 4; 2 where a lane
// never has more than two entries (the short rows of the vector product).
template <int B>
__device__ __forceinline__ double mv_row(const MvDims& d, const int* __restrict__ Aj, const value_t* __restrict__ Ax,
                                         const value_t* __restrict__ X, int a, int len, int slot, int step, int col, bool& bad)
{
    double s = 0.0;
    for (int i0 = slot; i0 < len; i0 += step * B) {
        int c[B];
        bool ok[B];
#pragma unroll
        for (int u = 0; u < B; ++u) {
            ok[u] = i0 < len - u * step;
            c[u] = ok[u] ? Aj[a + i0 + u * step] : 0;
            if ((unsigned)c[u] >= (unsigned)d.n) { bad |= ok[u]; ok[u] = false; }   // (never an index)
        }
        double av[B], xv[B];
#pragma unroll
        for (int u = 0; u < B; ++u) {
            av[u] = (ok[u] && Ax) ? (double)Ax[a + i0 + u * step] : 1.0;
            xv[u] = ok[u] ? (double)X[(long long)c[u] * d.ldX + col] : 0.0;
        }
#pragma unroll
        for (int u = 0; u < B; ++u)
            if (ok[u]) s += av[u] * xv[u];
    }
    return s;
}

// Y(r, col) from the row's sum: r < m, col < k
__device__ __forceinline__ void mv_store(const MvDims& d, value_t* __restrict__ Y, int r, int col, double s)
{
    value_t* p = Y + (long long)r * d.ldY + col;
    double t = d.alpha * s;
    if (d.beta != 0.0) t = t + d.beta * (double)*p;                   // (beta == 0 never reads y)
    *p = (value_t)t;
}

template <int T>
__global__ __launch_bounds__(256) void k_mv_short(MvDims d, const int* __restrict__ Ap, const int* __restrict__ Aj,
                                                  const value_t* __restrict__ Ax, const value_t* __restrict__ X,
                                                  value_t* __restrict__ Y, int* __restrict__ ctl, int* __restrict__ queue)
{
    constexpr int GS = mv_group<T>();                             // lanes a row
    constexpr int RPI = 256 / GS;                                 // rows an iteration
    __shared__ int sLen[kRdRows];
    __shared__ int sCnt[2], sBase[2];
    const int tid = threadIdx.x, lane = tid & 63, sl = tid & (GS - 1);
    const int col = sl % T, slot = sl / T;
    if (tid < 2) sCnt[tid] = 0;
    sLen[tid] = 0;
    __syncthreads();
    const int rowBase = blockIdx.x * kRdRows;
    bool bad = blockIdx.x == 0 && tid == 0 && (Ap[0] != 0 || Ap[d.m] != d.nnzA);
    for (int it = 0; it < kRdRows / RPI; ++it) {
        if (rowBase + it * RPI >= d.m) break;                     // (workgroup-uniform)
        const int rslot = it * RPI + tid / GS;
        const int r = rowBase + rslot;
        int a = 0, len = -1;                                      // -1: no row here, or bounds that are refused
        if (r < d.m) {
            a = Ap[r];
            const int b = Ap[r + 1];
            if (rd_bounds_bad(a, b, d.nnzA)) bad = true;
            else len = b - a;
        }
        const bool here = len >= 0 && len <= kRdShortL;
        for (int c0 = 0; c0 < d.k; c0 += T) {
            const bool mine = here && c0 + col < d.k;
            double s = 0.0;
            if (mine) s = mv_row<(T == 1 ? 2 : 4)>(d, Aj, Ax, X, a, len, slot, GS / T, c0 + col, bad);
            s = mv_lanes<T, GS>(s, lane);
            if (mine && slot == 0) mv_store(d, Y, r, c0 + col, s);
        }
        if (sl == 0 && len > 0) sLen[rslot] = len;
    }
    __syncthreads();
    rd_flag(bad, ctl);
    rd_enqueue(d.m, rowBase + tid, sLen[tid], sCnt, sBase, ctl, queue);
}

template <int T>
__global__ __launch_bounds__(256) void k_mv_wave(int nq, const int* __restrict__ queue, MvDims d, const int* __restrict__ Ap,
                                                 const int* __restrict__ Aj, const value_t* __restrict__ Ax,
                                                 const value_t* __restrict__ X, value_t* __restrict__ Y, int* __restrict__ ctl)
{
    const int lane = threadIdx.x & 63, col = lane % T, slot = lane / T;
    const int qi = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (qi >= nq) return;                                         // (wave-uniform, as everything below)
    const int r = queue[qi];
    if ((unsigned)r >= (unsigned)d.m) return;
    const int a = Ap[r], b = Ap[r + 1];
    if (rd_bounds_bad(a, b, d.nnzA)) return;                      // (k_mv_short queues no such row)
    bool bad = false;
    for (int c0 = 0; c0 < d.k; c0 += T) {
        const bool mine = c0 + col < d.k;
        double s = 0.0;
        if (mine) s = mv_row<4>(d, Aj, Ax, X, a, b - a, slot, 64 / T, c0 + col, bad);
        s = mv_lanes<T, 64>(s, lane);
        if (mine && slot == 0) mv_store(d, Y, r, c0 + col, s);
    }
    rd_flag(bad, ctl);
}

template <int T>
__global__ __launch_bounds__(256) void k_mv_long(int nq, const int* __restrict__ queue, MvDims d, const int* __restrict__ Ap,
                                                 const int* __restrict__ Aj, const value_t* __restrict__ Ax,
                                                 const value_t* __restrict__ X, value_t* __restrict__ Y, int* __restrict__ ctl)
{
    __shared__ double sW[4][T];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int col = lane % T, slot = wave * (64 / T) + lane / T;
    bool bad = false;
    for (int qi = blockIdx.x; qi < nq; qi += gridDim.x) {         // (everything below is workgroup-uniform)
        const int r = queue[qi];
        if ((unsigned)r >= (unsigned)d.m) continue;
        const int a = Ap[r], b = Ap[r + 1];
        if (rd_bounds_bad(a, b, d.nnzA)) continue;
        for (int c0 = 0; c0 < d.k; c0 += T) {
            const bool mine = c0 + col < d.k;
            double s = 0.0;
            if (mine) s = mv_row<4>(d, Aj, Ax, X, a, b - a, slot, 256 / T, c0 + col, bad);
            s = mv_lanes<T, 64>(s, lane);
            if (lane < T) sW[wave][lane] = s;
            __syncthreads();
            if (tid < T && mine) mv_store(d, Y, r, c0 + col, ((sW[0][tid] + sW[1][tid]) + sW[2][tid]) + sW[3][tid]);
            __syncthreads();                                      // (sW is the next tile's)
        }
    }
    rd_flag(bad, ctl);
}

}  // namespace bhs
