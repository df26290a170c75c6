// bhs_semiring.hip.h -- the masked multiply over a semiring, C<M> = A (+).(x) B (bhs_spgemm_semiring*, include/bhsparse_hip.h,
// "semiring multiply"): the kernels of bhs_masked.hip.h with the product (x) and the reduction (+) made template parameters.
// The walk over the products, the lookup-only table over the mask row, the bins, their limits and the launch shapes are
// those of the masked multiply; k_masked_scan, mask_find and mask_sub are used as they are.  What differs is the accumulator:
//
//   min / max   an ORDER-PRESERVING UNSIGNED KEY of the value (the selection kernels' idea, bhs_select.hip.h): the sign bit
//               flipped for non-negative values, every bit for negative ones, so that the keys' unsigned order is the
//               values' order with -0 below +0; a NaN product takes the extreme key that wins the reduction (0 for min,
//               all ones for max -- both decode to a NaN).  Reduced with the native unsigned atomicMin / atomicMax: 64-bit
//               in LDS and in valC of the double build, 32-bit (the key of the product rounded to float: rounding is
//               monotone) in valC of the float build.  No float-atomic semantics, and no dependence on the operands' order:
//               the result is the same bits from run to run.
//   or          the accumulator word is 0 or 1; a product that is 1 stores a 1 (every writer writes the same word)
//   pair        the accumulator word counts: integer 1s added; neither valA nor valB is loaded
//
// An accumulator is 8 bytes in LDS, as k_masked_lds's double: the footprint and the occupancy are its.  In the long and the
// hub bin the row of valC itself holds ENCODED accumulators ("cells": an unsigned word of bhs_value_t's size) while products
// arrive: a pass writes the encoded identity first, a pass decodes in place last -- phases of one workgroup in k_sr_long,
// k_sr_init and k_sr_decode around k_sr_hub.  valC is only ever touched as cells there, and every store is a vector store
// from plain C++.
//
//   k_sr_lds<S, G>   rows whose mask fits an LDS table (short bin: 16 lanes per row; wave bins: tables of 256 and 2048)
//   k_sr_long<S>     mask rows beyond the tables: 256 lanes per row, global atomics on the cells of the row
//   k_sr_hub<S>      rows with hub-sized product counts: parts across workgroups, LDS partials where the mask row fits
#pragma once
#include "bhs_masked.hip.h"

namespace bhs {

typedef unsigned long long sr_u64;
typedef std::conditional<sizeof(value_t) == 8, unsigned long long, unsigned int>::type cell_t;   // an accumulator in valC

__device__ __forceinline__ sr_u64 sr_key64(double v)
{
    const sr_u64 b = (sr_u64)__double_as_longlong(v);
    return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
__device__ __forceinline__ double sr_val64(sr_u64 k)
{
    return __longlong_as_double((long long)((k >> 63) ? (k & 0x7fffffffffffffffull) : ~k));
}
__device__ __forceinline__ unsigned sr_key32(float v)
{
    const unsigned b = __float_as_uint(v);
    return (b >> 31) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float sr_val32(unsigned k) { return __uint_as_float((k >> 31) ? (k & 0x7fffffffu) : ~k); }

// the bits of a value as a cell, and back
__device__ __forceinline__ cell_t sr_bits(value_t v)
{
    if constexpr (sizeof(value_t) == 8) return (cell_t)__double_as_longlong((double)v);
    else return (cell_t)__float_as_uint((float)v);
}

// max / min of two values in the order of the keys (-0 below +0); a NaN operand gives NaN
__device__ __forceinline__ double sr_order(double a, double b, bool takeMax)
{
    if (a != a || b != b) return __longlong_as_double(0x7ff8000000000000ll);
    const bool aAbove = sr_key64(a) >= sr_key64(b);
    return (aAbove == takeMax) ? a : b;
}

enum { kSrAdd = 0, kSrMul = 1, kSrMax = 2, kSrMin = 3 };

// ---- the semirings: what a product is (a 64-bit contribution), how it meets an accumulator in LDS (8 bytes) and a cell of
// valC, and what an accumulator reads as at the end ----
template <bool MAX, int MUL>
struct SrMinMax {
    static constexpr bool kValues = true;
    static __device__ __forceinline__ sr_u64 win() { return MAX ? ~0ull : 0ull; }
    static __device__ __forceinline__ sr_u64 ident() { return MAX ? 0x000fffffffffffffull /* -Inf */ : 0xfff0000000000000ull /* +Inf */; }
    static __device__ __forceinline__ sr_u64 prod(acc_t a, acc_t b)
    {
        acc_t v;
        if constexpr (MUL == kSrAdd) v = a + b;
        else if constexpr (MUL == kSrMul) v = a * b;
        else v = sr_order(a, b, MUL == kSrMax);
        return v != v ? win() : sr_key64(v);
    }
    static __device__ __forceinline__ void lds(sr_u64* p, sr_u64 k)
    {
        if constexpr (MAX) atomicMax(p, k); else atomicMin(p, k);
    }
    static __device__ __forceinline__ value_t out(sr_u64 k) { return (value_t)sr_val64(k); }
    static __device__ __forceinline__ cell_t cell(sr_u64 k)
    {
        if constexpr (sizeof(value_t) == 8) return (cell_t)k;
        else {
            const float f = (float)sr_val64(k);
            return (cell_t)(f != f ? (MAX ? ~0u : 0u) : sr_key32(f));
        }
    }
    static __device__ __forceinline__ void glob(cell_t* p, cell_t c)
    {
        if constexpr (MAX) atomicMax(p, c); else atomicMin(p, c);
    }
    static __device__ __forceinline__ cell_t cellOut(cell_t c)      // the bits of the entry's value
    {
        if constexpr (sizeof(value_t) == 8) return (cell_t)__double_as_longlong(sr_val64((sr_u64)c));
        else return (cell_t)__float_as_uint(sr_val32((unsigned)c));
    }
};

struct SrOrAnd {
    static constexpr bool kValues = true;
    static __device__ __forceinline__ sr_u64 ident() { return 0; }
    static __device__ __forceinline__ sr_u64 prod(acc_t a, acc_t b) { return (a != 0 && b != 0) ? 1 : 0; }   // (NaN != 0)
    // lds / glob are PLAIN stores that race with other waves' (glob in the hub bin: other workgroups') stores to the same word:
    // harmless, every writer stores the same 1.  What orders them against the identity stores before and the decode after is
    // not here: the __syncthreads of k_sr_lds / k_sr_hub, the __threadfence + __syncthreads pairs of k_sr_long (whose decode
    // reads with an agent-scope load) and the kernel boundaries of k_sr_init / k_sr_hub / k_sr_decode.  Keep those.
    static __device__ __forceinline__ void lds(sr_u64* p, sr_u64 k) { if (k) *p = 1; }
    static __device__ __forceinline__ value_t out(sr_u64 k) { return (value_t)(k ? 1 : 0); }
    static __device__ __forceinline__ cell_t cell(sr_u64 k) { return (cell_t)k; }
    static __device__ __forceinline__ void glob(cell_t* p, cell_t c) { if (c) *p = 1; }
    static __device__ __forceinline__ cell_t cellOut(cell_t c) { return sr_bits((value_t)(c ? 1 : 0)); }
};

struct SrPlusPair {
    static constexpr bool kValues = false;                           // the walk loads neither valA nor valB
    static __device__ __forceinline__ sr_u64 ident() { return 0; }
    static __device__ __forceinline__ sr_u64 prod(acc_t, acc_t) { return 1; }
    static __device__ __forceinline__ void lds(sr_u64* p, sr_u64 k) { atomicAdd(p, k); }
    static __device__ __forceinline__ value_t out(sr_u64 k) { return (value_t)k; }
    static __device__ __forceinline__ cell_t cell(sr_u64 k) { return (cell_t)k; }
    static __device__ __forceinline__ void glob(cell_t* p, cell_t c) { atomicAdd(p, c); }
    static __device__ __forceinline__ cell_t cellOut(cell_t c) { return sr_bits((value_t)c); }
};

typedef SrMinMax<false, kSrAdd> SrMinPlus;
typedef SrMinMax<true, kSrAdd> SrMaxPlus;
typedef SrMinMax<true, kSrMul> SrMaxTimes;
typedef SrMinMax<false, kSrMax> SrMinMaxS;
typedef SrMinMax<true, kSrMin> SrMaxMin;

// mask_walk with the semiring's product: add(c, contribution)
template <int G, typename S, typename F>
__device__ __forceinline__ void sr_walk(int lane, int a0, int a1, int sub, int sj, int ss, const int* __restrict__ Aj,
                                        const value_t* __restrict__ Ax, const int* __restrict__ Bp,
                                        const int* __restrict__ Bj, const value_t* __restrict__ Bx, int cmin, int cmax,
                                        bool bSorted, F&& add)
{
    const int groups = G / sub, gi = lane / sub, off = lane & (sub - 1);
    for (int a = a0 + gi; a < a1; a += groups) {
        const int kk = Aj[a];
        acc_t av = 0;
        if constexpr (S::kValues) av = (acc_t)Ax[a];
        int b0 = Bp[kk], b1 = Bp[kk + 1];
        if (ss > 1) {
            const long long len = b1 - b0;
            const int s0 = b0 + (int)(len * sj / ss), s1 = b0 + (int)(len * (sj + 1) / ss);
            b0 = s0;
            b1 = s1;
        }
        if (b1 <= b0) continue;
        if (bSorted && (Bj[b0] > cmax || Bj[b1 - 1] < cmin)) continue;   // the whole (slice of the) B row misses the mask row
        for (int b = b0 + off; b < b1; b += sub) {
            const int c = Bj[b];
            if (c < cmin || c > cmax) continue;
            acc_t bv = 0;
            if constexpr (S::kValues) bv = (acc_t)Bx[b];
            add(c, S::prod(av, bv));
        }
    }
}

// ---- rows whose mask row fits an LDS table of CAP entries: G lanes per row, BLOCK / G rows per workgroup ----
template <typename S, int G, int CAP, int BLOCK>
__global__ __launch_bounds__(BLOCK) void k_sr_lds(int nq, const int2* __restrict__ queue, const int* __restrict__ Mp,
                                                  const int* __restrict__ Mj, const int* __restrict__ Ap,
                                                  const int* __restrict__ Aj, const value_t* __restrict__ Ax,
                                                  const int* __restrict__ Bp, const int* __restrict__ Bj,
                                                  const value_t* __restrict__ Bx, int bSorted, value_t* __restrict__ valC)
{
    constexpr int RPB = BLOCK / G;
    __shared__ int sCol[RPB][CAP];
    __shared__ sr_u64 sAcc[RPB][CAP];
    const int g = threadIdx.x / G, lane = threadIdx.x % G;
    const int qi = blockIdx.x * RPB + g;
    int row = 0, r0 = 0, LM = 0, P = 0;
    if (qi < nq) {
        const int2 q = queue[qi];
        row = q.x;
        P = q.y;
        r0 = Mp[row];
        LM = min(Mp[row + 1] - r0, CAP);                    // (the binning keeps LM <= CAP: the min only guards LDS)
    }
    int* sc = sCol[g];
    sr_u64* sa = sAcc[g];
    for (int t = lane; t < LM; t += G) { sc[t] = Mj[r0 + t]; sa[t] = S::ident(); }
    __syncthreads();
    if (LM > 0) {
        const int a0 = Ap[row], a1 = Ap[row + 1];
        const int cmin = sc[0], cmax = sc[LM - 1];
        sr_walk<G, S>(lane, a0, a1, mask_sub(P, a1 - a0, G), 0, 1, Aj, Ax, Bp, Bj, Bx, cmin, cmax, bSorted != 0,
                      [&](int c, sr_u64 k) {
                          const int idx = mask_find(sc, LM, c);
                          if (idx >= 0) S::lds(&sa[idx], k);
                      });
    }
    __syncthreads();
    for (int t = lane; t < LM; t += G) valC[r0 + t] = S::out(sa[t]);
}

// ---- mask rows beyond the LDS tables: 256 lanes per row, lookups in HBM / L2.  Three phases of one workgroup on the cells
// of its row: the encoded identity, the products (atomics at the L2), the decode in place.  The decode reads the cells with
// loads that bypass this CU's L1, behind a fence that waits for the workgroup's own atomics. ----
template <typename S>
__global__ __launch_bounds__(256) void k_sr_long(int nq, const int2* __restrict__ queue, const int* __restrict__ Mp,
                                                 const int* __restrict__ Mj, const int* __restrict__ Ap,
                                                 const int* __restrict__ Aj, const value_t* __restrict__ Ax,
                                                 const int* __restrict__ Bp, const int* __restrict__ Bj,
                                                 const value_t* __restrict__ Bx, int bSorted, cell_t* valC)
{
    const int2 q = queue[blockIdx.x];
    const int row = q.x, r0 = Mp[row], LM = Mp[row + 1] - r0;
    cell_t* out = valC + r0;
    const cell_t id = S::cell(S::ident());
    for (int t = threadIdx.x; t < LM; t += 256) out[t] = id;
    __threadfence();                                     // (the identity is in the L2 before any wave's product arrives there:
    __syncthreads();                                     //  the reductions below, SrOrAnd's plain stores too, rely on this pair)
    const int* mc = Mj + r0;
    const int a0 = Ap[row], a1 = Ap[row + 1];
    if (LM > 0)
        sr_walk<256, S>(threadIdx.x, a0, a1, mask_sub(q.y, a1 - a0, 256), 0, 1, Aj, Ax, Bp, Bj, Bx, mc[0], mc[LM - 1], bSorted != 0,
                        [&](int c, sr_u64 k) {
                            const int idx = mask_find(mc, LM, c);
                            if (idx >= 0) S::glob(&out[idx], S::cell(k));
                        });
    __threadfence();
    __syncthreads();
    for (int t = threadIdx.x; t < LM; t += 256) {
        const cell_t c = __hip_atomic_load(&out[t], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        out[t] = S::cellOut(c);
    }
}

// ---- hub rows: the identity pass, gridDim.x parts per row, the decode pass ----
template <typename S>
__global__ __launch_bounds__(256) void k_sr_init(int nq, const int2* __restrict__ queue, const int* __restrict__ Mp,
                                                 cell_t* __restrict__ valC)
{
    const cell_t id = S::cell(S::ident());
    for (int y = blockIdx.x; y < nq; y += gridDim.x) {
        const int row = queue[y].x, r0 = Mp[row], LM = Mp[row + 1] - r0;
        for (int t = threadIdx.x; t < LM; t += 256) valC[r0 + t] = id;
    }
}

template <typename S>
__global__ __launch_bounds__(256) void k_sr_decode(int nq, const int2* __restrict__ queue, const int* __restrict__ Mp,
                                                   cell_t* __restrict__ valC)
{
    for (int y = blockIdx.x; y < nq; y += gridDim.x) {
        const int row = queue[y].x, r0 = Mp[row], LM = Mp[row + 1] - r0;
        for (int t = threadIdx.x; t < LM; t += 256) valC[r0 + t] = S::cellOut(valC[r0 + t]);
    }
}

template <typename S>
__global__ __launch_bounds__(256) void k_sr_hub(int nq, const int2* __restrict__ queue, const int* __restrict__ Mp,
                                                const int* __restrict__ Mj, const int* __restrict__ Ap,
                                                const int* __restrict__ Aj, const value_t* __restrict__ Ax,
                                                const int* __restrict__ Bp, const int* __restrict__ Bj,
                                                const value_t* __restrict__ Bx, int bSorted, int ldsCap, cell_t* valC)
{
    __shared__ int sCol[kMaskHubLds];
    __shared__ sr_u64 sAcc[kMaskHubLds];
    const int X = gridDim.x, x = blockIdx.x;
    for (int y = blockIdx.y; y < nq; y += gridDim.y) {
        const int2 q = queue[y];
        const int row = q.x, r0 = Mp[row], LM = Mp[row + 1] - r0;
        const int a0 = Ap[row], nA = Ap[row + 1] - a0;
        // this part's share: whole A entries where the row has at least X of them, else a slice of one entry's B row
        int ea, eb, sj = 0, ss = 1;
        if (nA >= X) {
            ea = a0 + (int)((long long)nA * x / X);
            eb = a0 + (int)((long long)nA * (x + 1) / X);
        } else {
            ss = X / max(nA, 1);
            const int e = x / ss;
            sj = x % ss;
            ea = a0 + e;
            eb = e < nA ? ea + 1 : ea;
        }
        const bool lds = LM <= ldsCap && LM <= kMaskHubLds;   // (block-uniform; the second test only guards LDS)
        if (lds)
            for (int t = threadIdx.x; t < LM; t += 256) { sCol[t] = Mj[r0 + t]; sAcc[t] = S::ident(); }
        __syncthreads();
        const int* mc = lds ? (const int*)sCol : Mj + r0;
        const long long perEntry = (long long)q.y / max(nA, 1) / ss;
        const int sub = mask_sub(perEntry, 1, 256);
        if (eb > ea && LM > 0)
            sr_walk<256, S>(threadIdx.x, ea, eb, sub, sj, ss, Aj, Ax, Bp, Bj, Bx, Mj[r0], Mj[r0 + LM - 1], bSorted != 0,
                            [&](int c, sr_u64 k) {
                                const int idx = mask_find(mc, LM, c);
                                if (idx < 0) return;
                                if (lds) S::lds(&sAcc[idx], k);
                                else S::glob(&valC[r0 + idx], S::cell(k));
                            });
        __syncthreads();
        if (lds)
            for (int t = threadIdx.x; t < LM; t += 256)
                if (sAcc[t] != S::ident()) S::glob(&valC[r0 + t], S::cell(sAcc[t]));
        __syncthreads();                                 // (the next row reuses the LDS)
    }
}

}  // namespace bhs
