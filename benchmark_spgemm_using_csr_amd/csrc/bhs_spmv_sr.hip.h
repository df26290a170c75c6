// bhs_spmv_sr.hip.h -- semiring CSR x dense with an output mask and accumulation: Y<M> (+)= A (+).(x) X for k columns
// (bhs_csr_spmv_semiring_device, bhs_csr_spmm_semiring_device; the contract is worded in include/bhsparse_hip.h,
// "semiring CSR x dense").
//
// The kernels have the shape of bhs_spmv.hip.h's -- its bins, its queues, its column tiles T (lane l of a row's lanes holds
// column c0 + l % T and entry slot l / T), its batched loads -- and use its and bhs_reduce.hip.h's pieces as they are:
//
//   k_smv_short  all rows in order, 256 rows a workgroup: the row pointer's validation (every row, selected or not), the
//                rows of up to 32 entries on the spot, the longer ones THAT HOLD A SELECTED ELEMENT queued for
//   k_smv_wave   up to 1024 entries, a wave per row, and
//   k_smv_long   a workgroup per row; its four waves meet in LDS in wave order.
//
// What combines two accumulators is the template parameter KIND of bhs_reduce.hip.h (kRdSum; kRdMin / kRdMax on its
// order-preserving keys, which bring the NaN rule and -0 below +0 with them; or is max over {0, 1}); the product is a
// wave-uniform switch at run time (SmvDims::mult), and so are the mask, its complement and the accumulation.
//
// An element decides whether it is selected BEFORE anything of its row is loaded for it: lanes whose element the mask does
// not select load no column, no value and no X, and store nothing; a row none of whose k elements is selected is not walked
// at all.  Stores go to selected (r < m, c < k) only, M is read at (r < m, c < k) only.  Validation precedes every dependent
// read as in bhs_spmv.hip.h: a refused row pointer is never an address, a refused column never an index into X.
//
// The count of changed elements is summed per lane, then per wave (butterfly), then in one LDS word per workgroup, and
// added once per workgroup, where it is not zero, to the 64-bit control word SMV_CHANGED: integer adds, the same total
// from run to run.  A caller that passes no changed_out does not pay for it (kSmvCount).  No atomic touches Y, no loop
// waits for another workgroup, every loop is bounded by a row's length or k.
#pragma once
#include "bhs_spmv.hip.h"

namespace bhs {

enum { kSmvTimes = 0, kSmvPlus = 1, kSmvMax = 2, kSmvMin = 3, kSmvAnd = 4, kSmvPair = 5 };   // the product (x)
enum { kSmvAccum = 1, kSmvComplement = 2 };                                               // BHS_MV_*
constexpr int kSmvCount = 4;          // beside them in SmvDims::flags, set by the host: the caller wants the count
// control words: the reductions' four, then the 64-bit count of changed elements (8-byte aligned)
enum { SMV_CHANGED = RD_INTS, SMV_INTS = RD_INTS + 2 };

struct SmvDims {
    int m, n, nnzA, k;
    long long ldX, ldM, ldY;
    int mult, flags;
    rd_u64 id;                        // the (+)-identity as an accumulator: bits of +0, or a key
};

template <int KIND>
__device__ __forceinline__ rd_u64 smv_acc(double x)
{
    if constexpr (KIND == kRdSum) return rd_bits(x);
    else return rd_key(x, KIND == kRdMax);
}

// a (x) b as an accumulator; a NaN product takes the key that wins
template <int KIND>
__device__ __forceinline__ rd_u64 smv_prod(int mult, double a, double x)
{
    if constexpr (KIND == kRdSum) {
        return rd_bits(mult == kSmvPair ? 1.0 : a * x);
    } else {
        constexpr bool forMax = KIND == kRdMax;
        if (mult == kSmvMax || mult == kSmvMin) {                   // max(a, b) / min(a, b) in the keys' order
            if (a != a || x != x) return forMax ? ~0ull : 0ull;
            const rd_u64 ka = rd_key(a, forMax), kx = rd_key(x, forMax);
            return ((mult == kSmvMax) == (ka < kx)) ? kx : ka;
        }
        const double p = mult == kSmvTimes ? a * x : mult == kSmvPlus ? a + x : ((a != 0.0 && x != 0.0) ? 1.0 : 0.0);
        return rd_key(p, forMax);
    }
}

// is element (r, col) selected: r < m, col < k
__device__ __forceinline__ bool smv_selected(const SmvDims& d, const value_t* __restrict__ M, int r, int col)
{
    if (!M) return true;
    const value_t v = M[(long long)r * d.ldM + col];
    return (v != (value_t)0) != ((d.flags & kSmvComplement) != 0);   // (NaN != 0: set)
}

// mv_lanes over KIND: the W / T entry slots of every column of the tile (all lanes active)
template <int KIND, int T, int W>
__device__ __forceinline__ rd_u64 smv_lanes(rd_u64 v, int lane)
{
    if constexpr (T <= 1 && W > 1) v = rd_comb<KIND>(v, lane_xor64<1>(v, lane));
    if constexpr (T <= 2 && W > 2) v = rd_comb<KIND>(v, lane_xor64<2>(v, lane));
    if constexpr (T <= 4 && W > 4) v = rd_comb<KIND>(v, lane_xor64<4>(v, lane));
    if constexpr (T <= 8 && W > 8) v = rd_comb<KIND>(v, lane_xor64<8>(v, lane));
    if constexpr (T <= 16 && W > 16) v = rd_comb<KIND>(v, lane_xor64<16>(v, lane));
    if constexpr (T <= 32 && W > 32) v = rd_comb<KIND>(v, lane_xor64<32>(v, lane));
    return v;
}

// mv_row over the semiring: entries a + slot, a + slot + step, .. of a row of len entries against column `col` (below k,
// selected) of X, combined in that order from the identity; B entries' loads in flight.  PLUS_PAIR reads the columns
// (they are validated) and neither the values nor X.
template <int KIND, int B>
__device__ __forceinline__ rd_u64 smv_row(const SmvDims& d, const int* __restrict__ Aj, const value_t* __restrict__ Ax,
                                         const value_t* __restrict__ X, int a, int len, int slot, int step, int col, bool& bad)
{
    rd_u64 s = d.id;
    const bool vals = d.mult != kSmvPair;
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
            av[u] = (ok[u] && vals && Ax) ? (double)Ax[a + i0 + u * step] : 1.0;
            xv[u] = (ok[u] && vals) ? (double)X[(long long)c[u] * d.ldX + col] : 1.0;
        }
#pragma unroll
        for (int u = 0; u < B; ++u)
            if (ok[u]) s = rd_comb<KIND>(s, smv_prod<KIND>(d.mult, av[u], xv[u]));
    }
    return s;
}

// Y(r, col) from the row's accumulator: r < m, col < k, selected.  1 where the stored value differs, as a number, from
// what it was accumulated into (y_old, or the identity without ACCUM, which never reads y).
template <int KIND>
__device__ __forceinline__ int smv_store(const SmvDims& d, value_t* __restrict__ Y, int r, int col, rd_u64 s)
{
    value_t* p = Y + (long long)r * d.ldY + col;
    value_t was;
    if (d.flags & kSmvAccum) {
        was = *p;
        double y = (double)was;
        if (d.mult == kSmvAnd) y = y != 0.0 ? 1.0 : 0.0;
        s = rd_comb<KIND>(smv_acc<KIND>(y), s);
    } else {
        was = rd_round<KIND>(d.id);
    }
    const value_t now = rd_round<KIND>(s);
    *p = now;
    return (now == was || (now != now && was != was)) ? 0 : 1;
}

// the workgroup's count to the control word: sChg is zero and a barrier lies between that and here; every thread of the
// workgroup comes here
__device__ __forceinline__ void smv_count(rd_u64 v, rd_u64* sChg, int* __restrict__ ctl)
{
    const int lane = threadIdx.x & 63;
    v += lane_xor64<1>(v, lane);
    v += lane_xor64<2>(v, lane);
    v += lane_xor64<4>(v, lane);
    v += lane_xor64<8>(v, lane);
    v += lane_xor64<16>(v, lane);
    v += lane_xor64<32>(v, lane);
    if (lane == 0 && v) (void)atomicAdd(sChg, v);
    __syncthreads();
    if (threadIdx.x == 0 && *sChg) (void)atomicAdd((rd_u64*)(ctl + SMV_CHANGED), *sChg);
}

template <int KIND, int T>
__global__ __launch_bounds__(256) void k_smv_short(SmvDims d, const int* __restrict__ Ap, const int* __restrict__ Aj,
                                                   const value_t* __restrict__ Ax, const value_t* __restrict__ X,
                                                   const value_t* __restrict__ M, value_t* __restrict__ Y,
                                                   int* __restrict__ ctl, int* __restrict__ queue)
{
    constexpr int GS = mv_group<T>();                             // lanes a row
    constexpr int RPI = 256 / GS;                                 // rows an iteration
    __shared__ int sLen[kRdRows];
    __shared__ int sCnt[2], sBase[2];
    __shared__ rd_u64 sChg;
    const int tid = threadIdx.x, lane = tid & 63, sl = tid & (GS - 1);
    const int col = sl % T, slot = sl / T;
    if (tid < 2) sCnt[tid] = 0;
    if (tid == 0) sChg = 0;
    sLen[tid] = 0;
    __syncthreads();
    const int rowBase = blockIdx.x * kRdRows;
    bool bad = blockIdx.x == 0 && tid == 0 && (Ap[0] != 0 || Ap[d.m] != d.nnzA);
    rd_u64 nchg = 0;
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
        bool any = false;
        for (int c0 = 0; c0 < d.k; c0 += T) {
            const bool sel = len >= 0 && c0 + col < d.k && smv_selected(d, M, r, c0 + col);
            any |= sel;
            const bool mine = here && sel;
            rd_u64 s = d.id;
            if (mine) s = smv_row<KIND, (T == 1 ? 2 : 4)>(d, Aj, Ax, X, a, len, slot, GS / T, c0 + col, bad);
            s = smv_lanes<KIND, T, GS>(s, lane);
            if (mine && slot == 0) nchg += smv_store<KIND>(d, Y, r, c0 + col, s);
        }
        // a longer row is queued only where one of its k elements is selected
        const rd_u64 anyGroup = (__ballot(any) >> (lane & ~(GS - 1))) & (GS == 64 ? ~0ull : ((1ull << (GS & 63)) - 1));
        if (sl == 0 && len > 0 && anyGroup) sLen[rslot] = len;
    }
    __syncthreads();
    rd_flag(bad, ctl);
    rd_enqueue(d.m, rowBase + tid, sLen[tid], sCnt, sBase, ctl, queue);
    if (d.flags & kSmvCount) smv_count(nchg, &sChg, ctl);             // (uniform: a kernel argument)
}

template <int KIND, int T>
__global__ __launch_bounds__(256) void k_smv_wave(int nq, const int* __restrict__ queue, SmvDims d, const int* __restrict__ Ap,
                                                  const int* __restrict__ Aj, const value_t* __restrict__ Ax,
                                                  const value_t* __restrict__ X, const value_t* __restrict__ M,
                                                  value_t* __restrict__ Y, int* __restrict__ ctl)
{
    __shared__ rd_u64 sChg;
    const int lane = threadIdx.x & 63, col = lane % T, slot = lane / T;
    if (threadIdx.x == 0) sChg = 0;
    __syncthreads();
    const int qi = blockIdx.x * 4 + (threadIdx.x >> 6);
    int r = -1, a = 0, len = -1;                                  // (wave-uniform, as everything below)
    if (qi < nq) r = queue[qi];
    if ((unsigned)r < (unsigned)d.m) {
        a = Ap[r];
        const int b = Ap[r + 1];
        if (!rd_bounds_bad(a, b, d.nnzA)) len = b - a;            // (k_smv_short queues no other row)
    }
    bool bad = false;
    rd_u64 nchg = 0;
    if (len >= 0) {
        for (int c0 = 0; c0 < d.k; c0 += T) {
            const bool mine = c0 + col < d.k && smv_selected(d, M, r, c0 + col);
            rd_u64 s = d.id;
            if (mine) s = smv_row<KIND, 4>(d, Aj, Ax, X, a, len, slot, 64 / T, c0 + col, bad);
            s = smv_lanes<KIND, T, 64>(s, lane);
            if (mine && slot == 0) nchg += smv_store<KIND>(d, Y, r, c0 + col, s);
        }
    }
    rd_flag(bad, ctl);
    if (d.flags & kSmvCount) smv_count(nchg, &sChg, ctl);             // (uniform: a kernel argument)
}

template <int KIND, int T>
__global__ __launch_bounds__(256) void k_smv_long(int nq, const int* __restrict__ queue, SmvDims d, const int* __restrict__ Ap,
                                                  const int* __restrict__ Aj, const value_t* __restrict__ Ax,
                                                  const value_t* __restrict__ X, const value_t* __restrict__ M,
                                                  value_t* __restrict__ Y, int* __restrict__ ctl)
{
    __shared__ rd_u64 sW[4][T];
    __shared__ rd_u64 sChg;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int col = lane % T, slot = wave * (64 / T) + lane / T;
    if (tid == 0) sChg = 0;
    __syncthreads();
    bool bad = false;
    rd_u64 nchg = 0;
    for (int qi = blockIdx.x; qi < nq; qi += gridDim.x) {         // (everything below is workgroup-uniform)
        const int r = queue[qi];
        if ((unsigned)r >= (unsigned)d.m) continue;
        const int a = Ap[r], b = Ap[r + 1];
        if (rd_bounds_bad(a, b, d.nnzA)) continue;
        for (int c0 = 0; c0 < d.k; c0 += T) {
            const bool mine = c0 + col < d.k && smv_selected(d, M, r, c0 + col);
            rd_u64 s = d.id;
            if (mine) s = smv_row<KIND, 4>(d, Aj, Ax, X, a, b - a, slot, 256 / T, c0 + col, bad);
            s = smv_lanes<KIND, T, 64>(s, lane);
            if (lane < T) sW[wave][lane] = s;
            __syncthreads();
            if (tid < T && mine)
                nchg += smv_store<KIND>(d, Y, r, c0 + col,
                                       rd_comb<KIND>(rd_comb<KIND>(rd_comb<KIND>(sW[0][tid], sW[1][tid]), sW[2][tid]), sW[3][tid]));
            __syncthreads();                                      // (sW is the next tile's)
        }
    }
    rd_flag(bad, ctl);
    if (d.flags & kSmvCount) smv_count(nchg, &sChg, ctl);             // (uniform: a kernel argument)
}

}  // namespace bhs
