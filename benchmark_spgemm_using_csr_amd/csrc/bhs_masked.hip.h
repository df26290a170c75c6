// bhs_masked.hip.h -- the masked multiply C<M> = A·B (bhs_spgemm_masked[_device], include/bhsparse_hip.h): for every entry
// (i, j) of a caller-given CSR pattern M, valC = sum over k of A(i,k) B(k,j); products outside M are dropped, the result is
// written on M's pattern.  No symbolic stage, no scan, no sort, no column indices written: the accumulator of a row is a
// LOOKUP-ONLY table -- the mask row's sorted columns -- where the general pipeline's kernels insert into a hash table.
//
//   k_masked_scan     one pass over M and rowPtrA: validity of M (rowPtrM monotone and within [0, nnzM], columns in
//                     [0, n), rows strictly ascending), the mask row length LM and the product count P of every row, the
//                     row's bin, the product total; rows appended to per-bin queues with one atomic per workgroup and bin
//   k_masked_lds<G>   rows whose mask fits an LDS table: G lanes per row (16: four rows per wave, the short bin; 64: a wave
//                     per row), the mask row's columns and an fp64 accumulator per entry in LDS, ds_add_f64 per product,
//                     the row stored as LM coalesced values
//   k_masked_long     mask rows beyond the LDS tables: 256 lanes per row, binary search over the sorted row in HBM / L2,
//                     global atomics into the row of valC, which the kernel zeroes first
//   k_masked_hub      rows with hub-sized P: the row's products cut into parts across workgroups (by A entries, or by
//                     slices of B rows where the A row is shorter than the parts), each part accumulating in LDS where
//                     the mask row fits and adding its sums to the row of valC (zeroed by k_masked_zero) atomically
//
// Cheap rejections: a product column outside [first, last] column of the mask row is not looked up; with ascending rows
// of B (bhs_get_info "b_sorted") a whole B row whose [first, last] misses that interval is not read.
#pragma once
#include "bhs_kernels.hip.h"

namespace bhs {

enum { kMaskShort = 0, kMaskWaveS = 1, kMaskWaveL = 2, kMaskLong = 3, kMaskHub = 4, kMaskBins = 5 };
constexpr int kMaskScanG = 16;        // lanes per row of k_masked_scan
constexpr int kMaskShortLM = 32;      // short bin: mask rows of <= 32 entries ...
constexpr int kMaskShortP = 256;      // ... and <= 256 products, 16 lanes per row
constexpr int kMaskWaveTab = 256;      // LDS table of the small wave bin (entries of the mask row)
constexpr int kMaskHubLds = 2048;     // k_masked_hub keeps the mask row in LDS up to this length

// counters of the masked multiply (ints of its own workspace block): bin counts, error flag, product total, largest hub
// row, products per bin
enum { MS_COUNT = 0, MS_ERR = 8, MS_TOTAL = 10 /* u64 */, MS_HUBMAX = 12 /* u64 */, MS_SUMS = 16 /* kMaskBins u64: products per bin */,
       MS_INTS = 32 };

struct MaskSpec {
    int shortLM, shortP;   // short bin limits
    int waveS, waveL;      // LDS table sizes of the two wave bins (0: bin unused); mask rows beyond waveL are long rows
    long long hubMin;      // rows with at least this many products go to the hub bin (0: never)
};

// lower bound of c in cols[0, len) -- the index of c, or -1 when the sorted list does not hold it
template <typename P>
__device__ __forceinline__ int mask_find(P cols, int len, int c)
{
    int lo = 0, hi = len;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (cols[mid] < c) lo = mid + 1; else hi = mid;
    }
    return (lo < len && cols[lo] == c) ? lo : -1;
}

// The products of A row entries [a0, a1), each with the slice [sj/ss, (sj+1)/ss) of its B row,
// walked by G lanes: sub-groups of `sub` lanes (a power of two: about the average B row length) take one entry each and
// stride its B row, so that rows of short B rows keep every lane busy and long B rows are read coalesced.
template <int G, typename F>
__device__ __forceinline__ void mask_walk(int lane, int a0, int a1, int sub, int sj, int ss, const int* __restrict__ Aj,
                                          const value_t* __restrict__ Ax, const int* __restrict__ Bp,
                                          const int* __restrict__ Bj, const value_t* __restrict__ Bx, int cmin, int cmax,
                                          bool bSorted, F&& add)
{
    const int groups = G / sub, gi = lane / sub, off = lane & (sub - 1);
    for (int a = a0 + gi; a < a1; a += groups) {
        const int kk = Aj[a];
        const acc_t av = (acc_t)Ax[a];
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
            add(c, av * (acc_t)Bx[b]);
        }
    }
}

__device__ __forceinline__ int mask_sub(long long P, int nA, int G)
{
    const long long avg = nA > 0 ? (P + nA - 1) / nA : 1;
    int sub = 1;
    while (sub < G && sub < avg) sub <<= 1;
    return sub;
}

// ---- validation and binning: kMaskScanG lanes per row of M, kMaskScanRows rows per workgroup.  A row is appended to its
// bin's queue as (row, products); rows with an empty mask row write nothing and go nowhere.  The workgroup gathers its
// rows' bins in LDS and takes its places in each queue (and adds its product sums) with one global atomic per bin: one
// per wave measured 12.6 ms on poisson27pt 128^3 -- half a million atomics on the same few words, serialised in L2.
// ctl[MS_ERR] != 0: M is invalid (the host then launches nothing that writes valC). ----
constexpr int kMaskScanRows = 256;
__global__ __launch_bounds__(256) void k_masked_scan(int m, int n, int nnzM, const int* __restrict__ Mp,
                                                     const int* __restrict__ Mj, const int* __restrict__ Ap,
                                                     const int* __restrict__ Aj, const int* __restrict__ Bp, MaskSpec spec,
                                                     int* __restrict__ ctl, int2* __restrict__ queue)
{
    __shared__ int sBin[kMaskScanRows];
    __shared__ long long sP[kMaskScanRows];
    __shared__ int sCnt[kMaskBins], sBase[kMaskBins];
    __shared__ unsigned long long sSum[kMaskBins + 1];
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int sl = tid & (kMaskScanG - 1);
    if (tid < kMaskBins) sCnt[tid] = 0;
    if (tid <= kMaskBins) sSum[tid] = 0;
    const int rowBase = blockIdx.x * kMaskScanRows;
    bool bad = false;
    if (blockIdx.x == 0 && tid == 0 && (Mp[0] != 0 || Mp[m] != nnzM)) bad = true;
    for (int it = 0; it < kMaskScanRows / (256 / kMaskScanG); ++it) {
        const int slot = it * (256 / kMaskScanG) + tid / kMaskScanG;
        const int row = rowBase + slot;
        int LM = 0;
        long long P = 0;
        if (row < m) {
            const int r0 = Mp[row], r1 = Mp[row + 1];
            if (r0 < 0 || r1 < r0 || r1 > nnzM) {
                bad = true;                                   // (nothing of the row is read: its bounds may point anywhere)
            } else {
                LM = r1 - r0;
                for (int q = r0 + sl; q < r1; q += kMaskScanG) {
                    const int c = Mj[q];
                    if (c < 0 || c >= n || (q + 1 < r1 && Mj[q + 1] <= c)) bad = true;
                }
                const int a0 = Ap[row], a1 = Ap[row + 1];
                for (int a = a0 + sl; a < a1; a += kMaskScanG) {
                    const int kk = Aj[a];
                    P += Bp[kk + 1] - Bp[kk];
                }
            }
        }
#pragma unroll
        for (int o = kMaskScanG / 2; o >= 1; o >>= 1) P += __shfl_xor(P, o);
        if (sl == 0) {
            int bin = -1;                                     // (-1: nothing to do)
            if (LM > 0) {
                if (spec.hubMin > 0 && P >= spec.hubMin) bin = kMaskHub;
                else if (LM > spec.waveL) bin = kMaskLong;
                else if (LM <= spec.shortLM && P <= spec.shortP) bin = kMaskShort;
                else if (LM <= spec.waveS) bin = kMaskWaveS;
                else bin = kMaskWaveL;
                if (bin == kMaskHub) atomicMax((unsigned long long*)(ctl + MS_HUBMAX), (unsigned long long)P);
            }
            sBin[slot] = bin;
            sP[slot] = P;
        }
    }
    if (__ballot(bad) != 0ull && lane == 0) atomicOr(ctl + MS_ERR, 1);
    __syncthreads();
    // thread t now owns row rowBase + t
    const int bin = sBin[tid];
    const long long P = sP[tid];
    int rank = 0;
    if (bin >= 0) {
        rank = atomicAdd(&sCnt[bin], 1);
        atomicAdd(&sSum[bin], (unsigned long long)P);
    }
    long long t = P;
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) t += __shfl_xor(t, o);
    if (lane == 0 && t) atomicAdd(&sSum[kMaskBins], (unsigned long long)t);
    __syncthreads();
    if (tid < kMaskBins && sCnt[tid]) {
        sBase[tid] = atomicAdd(ctl + MS_COUNT + tid, sCnt[tid]);
        if (sSum[tid]) atomicAdd((unsigned long long*)(ctl + MS_SUMS) + tid, sSum[tid]);
    }
    if (tid == kMaskBins && sSum[kMaskBins]) atomicAdd((unsigned long long*)(ctl + MS_TOTAL), sSum[kMaskBins]);
    __syncthreads();
    if (bin >= 0)
        queue[(size_t)bin * m + sBase[bin] + rank] = make_int2(rowBase + tid, (int)(P < 0x7fffffff ? P : 0x7fffffff));
}

// ---- rows whose mask row fits an LDS table of CAP entries: G lanes per row, BLOCK / G rows per workgroup ----
template <int G, int CAP, int BLOCK>
__global__ __launch_bounds__(BLOCK) void k_masked_lds(int nq, const int2* __restrict__ queue, const int* __restrict__ Mp,
                                                      const int* __restrict__ Mj, const int* __restrict__ Ap,
                                                      const int* __restrict__ Aj, const value_t* __restrict__ Ax,
                                                      const int* __restrict__ Bp, const int* __restrict__ Bj,
                                                      const value_t* __restrict__ Bx, int bSorted, value_t* __restrict__ valC)
{
    constexpr int RPB = BLOCK / G;
    __shared__ int sCol[RPB][CAP];
    __shared__ acc_t sAcc[RPB][CAP];
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
    acc_t* sa = sAcc[g];
    for (int t = lane; t < LM; t += G) { sc[t] = Mj[r0 + t]; sa[t] = 0; }
    __syncthreads();
    if (LM > 0) {
        const int a0 = Ap[row], a1 = Ap[row + 1];
        const int cmin = sc[0], cmax = sc[LM - 1];
        mask_walk<G>(lane, a0, a1, mask_sub(P, a1 - a0, G), 0, 1, Aj, Ax, Bp, Bj, Bx, cmin, cmax, bSorted != 0,
                     [&](int c, acc_t v) {
                         const int idx = mask_find(sc, LM, c);
                         if (idx >= 0) unsafeAtomicAdd(&sa[idx], v);
                     });
    }
    __syncthreads();
    for (int t = lane; t < LM; t += G) valC[r0 + t] = (value_t)sa[t];
}

// ---- mask rows beyond the LDS tables: 256 lanes per row, lookups in HBM / L2, global atomics into the zeroed row ----
__global__ __launch_bounds__(256) void k_masked_long(int nq, const int2* __restrict__ queue, const int* __restrict__ Mp,
                                                     const int* __restrict__ Mj, const int* __restrict__ Ap,
                                                     const int* __restrict__ Aj, const value_t* __restrict__ Ax,
                                                     const int* __restrict__ Bp, const int* __restrict__ Bj,
                                                     const value_t* __restrict__ Bx, int bSorted, value_t* __restrict__ valC)
{
    const int2 q = queue[blockIdx.x];
    const int row = q.x, r0 = Mp[row], LM = Mp[row + 1] - r0;
    value_t* out = valC + r0;
    for (int t = threadIdx.x; t < LM; t += 256) out[t] = (value_t)0;
    __threadfence();
    __syncthreads();
    const int* mc = Mj + r0;
    const int a0 = Ap[row], a1 = Ap[row + 1];
    mask_walk<256>(threadIdx.x, a0, a1, mask_sub(q.y, a1 - a0, 256), 0, 1, Aj, Ax, Bp, Bj, Bx, mc[0], mc[LM - 1], bSorted != 0,
                   [&](int c, acc_t v) {
                       const int idx = mask_find(mc, LM, c);
                       if (idx >= 0) unsafeAtomicAdd(&out[idx], (value_t)v);
                   });
}

// ---- hub rows: the zeroing pass, then gridDim.x parts per row ----
__global__ __launch_bounds__(256) void k_masked_zero(int nq, const int2* __restrict__ queue, const int* __restrict__ Mp,
                                                     value_t* __restrict__ valC)
{
    for (int y = blockIdx.x; y < nq; y += gridDim.x) {
        const int row = queue[y].x, r0 = Mp[row], LM = Mp[row + 1] - r0;
        for (int t = threadIdx.x; t < LM; t += 256) valC[r0 + t] = (value_t)0;
    }
}

__global__ __launch_bounds__(256) void k_masked_hub(int nq, const int2* __restrict__ queue, const int* __restrict__ Mp,
                                                    const int* __restrict__ Mj, const int* __restrict__ Ap,
                                                    const int* __restrict__ Aj, const value_t* __restrict__ Ax,
                                                    const int* __restrict__ Bp, const int* __restrict__ Bj,
                                                    const value_t* __restrict__ Bx, int bSorted, int ldsCap,
                                                    value_t* __restrict__ valC)
{
    __shared__ int sCol[kMaskHubLds];
    __shared__ acc_t sAcc[kMaskHubLds];
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
        const bool lds = LM <= ldsCap;                   // (block-uniform)
        if (lds)
            for (int t = threadIdx.x; t < LM; t += 256) { sCol[t] = Mj[r0 + t]; sAcc[t] = 0; }
        __syncthreads();
        const int* mc = lds ? (const int*)sCol : Mj + r0;
        const long long perEntry = (long long)q.y / max(nA, 1) / ss;
        const int sub = mask_sub(perEntry, 1, 256);
        if (eb > ea)
            mask_walk<256>(threadIdx.x, ea, eb, sub, sj, ss, Aj, Ax, Bp, Bj, Bx, Mj[r0], Mj[r0 + LM - 1], bSorted != 0,
                           [&](int c, acc_t v) {
                               const int idx = mask_find(mc, LM, c);
                               if (idx < 0) return;
                               if (lds) unsafeAtomicAdd(&sAcc[idx], v);
                               else unsafeAtomicAdd(&valC[r0 + idx], (value_t)v);
                           });
        __syncthreads();
        if (lds)
            for (int t = threadIdx.x; t < LM; t += 256)
                if (sAcc[t] != (acc_t)0) unsafeAtomicAdd(&valC[r0 + t], (value_t)sAcc[t]);
        __syncthreads();                                 // (the next row reuses the LDS)
    }
}

}  // namespace bhs
