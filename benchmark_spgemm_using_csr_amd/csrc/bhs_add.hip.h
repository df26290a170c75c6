// bhs_add.hip.h -- the sparse add Z = alpha X + beta Y on CSR with the union of the patterns (bhs_csr_add_*_device,
// bhs_spgemm_add[_device], include/bhsparse_hip.h).  X and Y are m x n with strictly ascending rows; so is Z.  The pattern
// never depends on values: an entry of both reads alpha x + beta y even where that is 0.
//
//   k_add_check       validity of one CSR matrix (bhs_spgemm_add: D, before the multiply is started)
//   k_add_count       one pass over X and Y: validity of both (rowPtr monotone and within [0, nnz], columns in [0, n), rows
//                     strictly ascending), |row(X) u row(Y)| of every row (every entry of Y looked up in its row of X), the
//                     row's bin by len(X) + len(Y), whether any entry of Y is outside X, nnz(Z); optionally where in X every
//                     entry of Y was found (the in-place path adds there without a second search).  Rows appended to
//                     per-bin queues with one atomic per workgroup and bin.  The counts go through k_scan_onepass.
//   k_add_bin         the bins alone, from the three row pointers (bhs_csr_add_numeric_device: no column is read)
//   k_add_fill<G>     G lanes per row: 16 (short bin, four rows per wave), 64 (a wave per row) or 256 (a workgroup per row,
//                     the row cut into chunks of kAddChunk merged entries by merge-path partition).  The two rows' chunks
//                     are staged in LDS; an entry's slot in Z is its merge rank minus the matches before it:
//                         x_i -> i + |{y < x_i}| - |{matched x before i}|      y_j (unmatched) -> j + |{x < y_j}| - |{matched y before j}|
//                     -- a binary search in the other row's chunk and a scan of the match flags over the lanes.  The lane of
//                     x owns a matched slot and fetches y; a matched y writes nothing: no atomics, nothing depends on
//                     scheduling.
//   k_add_inplace     Y inside X, alpha == 1: X's values at the places k_add_count found, += beta y (nothing else is touched)
//   k_add_inplace_rows  Y inside X, any alpha: one streaming pass over X, x = alpha x + beta y where Y has the column
// Arithmetic in double, one rounding to value_t per entry.
#pragma once
#include "bhs_kernels.hip.h"
#include "bhs_wave.hip.h"

namespace bhs {

enum { kAddShort = 0, kAddWave = 1, kAddLong = 2, kAddBins = 3 };
constexpr int kAddShortL = 32;        // short bin: len(X) + len(Y) <= 32, 16 lanes per row
constexpr int kAddWaveL = 1024;       // wave bin: both rows fit a wave's LDS slice
constexpr int kAddChunk = 2048;       // long rows: merged entries per chunk of the workgroup's walk
constexpr int kAddCountG = 16;        // lanes per row of k_add_count / k_add_check
constexpr int kAddCountRows = 256;    // rows per workgroup of them

// counters of the sparse add (ints of its own workspace block): rows per bin, error flag, "an entry of Y is outside X",
// the scan's ticket / longest row / total / histogram words, nnz(Z)
enum { AD_COUNT = 0, AD_ERR = 4, AD_OUTSIDE = 5, AD_TICKET = 6, AD_MAXCNT = 7, AD_TOTAL = 8 /* u64 */, AD_SCANTOTAL = 10 /* i64 */,
       AD_SCANBINS = 12 /* kMaxBins */, AD_INTS = 32 };

// number of entries of the ascending list cols[0, len) that are < c
template <typename P>
__device__ __forceinline__ int add_lower_bound(P cols, int len, int c)
{
    int lo = 0, hi = len;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (cols[mid] < c) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// true when row [r0, r1) of (J, nnz, n) breaks the contract; nothing of a row with bad bounds is read
__device__ __forceinline__ bool add_row_bad(const int* __restrict__ J, int r0, int r1, int nnz, int n, int sl)
{
    if (r0 < 0 || r1 < r0 || r1 > nnz) return true;
    bool bad = false;
    for (int q = r0 + sl; q < r1; q += kAddCountG) {
        const int c = J[q];
        if (c < 0 || c >= n || (q + 1 < r1 && J[q + 1] <= c)) bad = true;
    }
    return bad;
}

__global__ __launch_bounds__(256) void k_add_check(int m, int n, int nnz, const int* __restrict__ P, const int* __restrict__ J,
                                                   int* __restrict__ ctl)
{
    const int tid = threadIdx.x, sl = tid & (kAddCountG - 1);
    bool bad = blockIdx.x == 0 && tid == 0 && (P[0] != 0 || P[m] != nnz);
    const int row = blockIdx.x * (256 / kAddCountG) + tid / kAddCountG;
    if (row < m) bad = add_row_bad(J, P[row], P[row + 1], nnz, n, sl) || bad;
    if (__ballot(bad) != 0ull && (tid & 63) == 0) atomicOr(ctl + AD_ERR, 1);
}

// Thread t of the workgroup owns row rowBase + t with L = len(X) + len(Y) entries to merge: the row joins its bin's queue.
// One global atomic per workgroup and bin (see k_masked_scan).  Ends with the workgroup in step.
__device__ __forceinline__ void add_enqueue(int m, int row, int L, int* sCnt, int* sBase, int* __restrict__ ctl,
                                            int* __restrict__ queue)
{
    const int tid = threadIdx.x;
    const int bin = (row >= m || L <= 0) ? -1 : L <= kAddShortL ? kAddShort : L <= kAddWaveL ? kAddWave : kAddLong;
    int rank = 0;
    if (bin >= 0) rank = atomicAdd(&sCnt[bin], 1);
    __syncthreads();
    if (tid < kAddBins && sCnt[tid]) sBase[tid] = atomicAdd(ctl + AD_COUNT + tid, sCnt[tid]);
    __syncthreads();
    if (bin >= 0) queue[(size_t)bin * m + sBase[bin] + rank] = row;
}

__global__ __launch_bounds__(256) void k_add_count(int m, int n, int nnzX, const int* __restrict__ Xp, const int* __restrict__ Xj,
                                                   int nnzY, const int* __restrict__ Yp, const int* __restrict__ Yj,
                                                   int* __restrict__ cnt, int* __restrict__ ypos, int* __restrict__ ctl,
                                                   int* __restrict__ queue)
{
    __shared__ int sRowCnt[kAddCountRows], sRowLen[kAddCountRows];
    __shared__ int sCnt[kAddBins], sBase[kAddBins];
    __shared__ unsigned long long sTot;
    const int tid = threadIdx.x, lane = tid & 63, sl = tid & (kAddCountG - 1);
    if (tid < kAddBins) sCnt[tid] = 0;
    if (tid == 0) sTot = 0;
    const int rowBase = blockIdx.x * kAddCountRows;
    bool bad = blockIdx.x == 0 && tid == 0 && (Xp[0] != 0 || Xp[m] != nnzX || Yp[0] != 0 || Yp[m] != nnzY);
    bool outside = false;
    for (int it = 0; it < kAddCountRows / (256 / kAddCountG); ++it) {
        const int slot = it * (256 / kAddCountG) + tid / kAddCountG;
        const int row = rowBase + slot;
        int a = 0, b = 0, matches = 0;
        if (row < m) {
            const int x0 = Xp[row], x1 = Xp[row + 1], y0 = Yp[row], y1 = Yp[row + 1];
            const bool badX = add_row_bad(Xj, x0, x1, nnzX, n, sl), badY = add_row_bad(Yj, y0, y1, nnzY, n, sl);
            const bool boundsOk = !(x0 < 0 || x1 < x0 || x1 > nnzX || y0 < 0 || y1 < y0 || y1 > nnzY);
            if (badX || badY) bad = true;
            if (boundsOk) {                                   // (an unsorted row is still searched within its bounds: the call fails anyway)
                a = x1 - x0;
                b = y1 - y0;
                for (int q = y0 + sl; q < y1; q += kAddCountG) {
                    const int c = Yj[q];
                    const int lb = add_lower_bound(Xj + x0, a, c);
                    const bool hit = lb < a && Xj[x0 + lb] == c;
                    matches += hit ? 1 : 0;
                    if (!hit) outside = true;
                    if (ypos) ypos[q] = hit ? x0 + lb : -1;
                }
            }
        }
#pragma unroll
        for (int o = kAddCountG / 2; o >= 1; o >>= 1) matches += __shfl_xor(matches, o);
        if (sl == 0) { sRowCnt[slot] = a + b - matches; sRowLen[slot] = a + b; }
    }
    if (__ballot(bad) != 0ull && lane == 0) atomicOr(ctl + AD_ERR, 1);
    if (__ballot(outside) != 0ull && lane == 0) atomicOr(ctl + AD_OUTSIDE, 1);
    __syncthreads();
    const int row = rowBase + tid;
    const int c = sRowCnt[tid];
    if (row < m) cnt[row] = c;
    long long t64 = c;                                        // (nnz(Z) may pass 2^31: summed in 64 bits, the host decides)
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) t64 += __shfl_xor(t64, o);
    if (lane == 0 && t64) atomicAdd(&sTot, (unsigned long long)t64);
    add_enqueue(m, row, sRowLen[tid], sCnt, sBase, ctl, queue);
    if (tid == 0 && sTot) atomicAdd((unsigned long long*)(ctl + AD_TOTAL), sTot);
}

// bhs_csr_add_numeric_device: the bins from the row pointers; AD_ERR when they cannot belong together (a rowPtr that is
// not monotone within its nnz, a row of Z shorter than the longer of its two rows or longer than both together)
__global__ __launch_bounds__(256) void k_add_bin(int m, int nnzX, const int* __restrict__ Xp, int nnzY, const int* __restrict__ Yp,
                                                 const int* __restrict__ Zp, int* __restrict__ ctl, int* __restrict__ queue)
{
    __shared__ int sCnt[kAddBins], sBase[kAddBins];
    const int tid = threadIdx.x;
    if (tid < kAddBins) sCnt[tid] = 0;
    __syncthreads();
    const int row = blockIdx.x * 256 + tid;
    bool bad = blockIdx.x == 0 && tid == 0 && (Xp[0] != 0 || Xp[m] != nnzX || Yp[0] != 0 || Yp[m] != nnzY || Zp[0] != 0);
    int L = 0;
    if (row < m) {
        const int x0 = Xp[row], x1 = Xp[row + 1], y0 = Yp[row], y1 = Yp[row + 1], z = Zp[row + 1] - Zp[row];
        if (x0 < 0 || x1 < x0 || x1 > nnzX || y0 < 0 || y1 < y0 || y1 > nnzY) bad = true;
        else {
            L = (x1 - x0) + (y1 - y0);
            if (Zp[row] < 0 || z < max(x1 - x0, y1 - y0) || z > L) bad = true;
        }
    }
    if (__ballot(bad) != 0ull && (tid & 63) == 0) atomicOr(ctl + AD_ERR, 1);
    add_enqueue(m, row, bad ? 0 : L, sCnt, sBase, ctl, queue);
}

// exclusive prefix of `flag` over the G lanes of a group, in lane order; total: the group's sum.  G = 64 / 256: every lane of
// the wave / workgroup takes part (DPP scan; the workgroup form goes through sW and two barriers).
template <int G>
__device__ __forceinline__ int add_scan_flags(int flag, int tid, int* sW, int& total)
{
    if constexpr (G == 16) {
        const unsigned long long bl = __ballot(flag != 0);
        const unsigned mine = (unsigned)(bl >> ((tid & 63) & ~15)) & 0xffffu;
        total = __popc(mine);
        return __popc(mine & ((1u << (tid & 15)) - 1u));
    } else {
        const int incl = wave_incl_scan_dpp(flag);
        const int wtot = __builtin_amdgcn_readlane(incl, 63);
        if constexpr (G == 64) {
            total = wtot;
            return incl - flag;
        } else {
            const int w = tid >> 6;
            if ((tid & 63) == 0) sW[w] = wtot;
            __syncthreads();
            int before = 0;
            total = 0;
#pragma unroll
            for (int q = 0; q < G / 64; ++q) { before += q < w ? sW[q] : 0; total += sW[q]; }
            __syncthreads();
            return before + incl - flag;
        }
    }
}

// ---- the fill pass: G lanes per row, BLOCK / G rows per workgroup, chunks of at most CAP (+ 1) merged entries in LDS.
// G < BLOCK: the binning keeps len(X) + len(Y) <= CAP, one chunk.  G == BLOCK: the row is cut at every CAP-th place of the
// merge (x before an equal y; a pair is never cut apart: the chunk then takes the y as its CAP + 1st entry). ----
template <int G, int CAP, int BLOCK>
__global__ __launch_bounds__(BLOCK) void k_add_fill(int nq, const int* __restrict__ queue, double alpha, const int* __restrict__ Xp,
                                                    const int* __restrict__ Xj, const value_t* __restrict__ Xx, double beta,
                                                    const int* __restrict__ Yp, const int* __restrict__ Yj,
                                                    const value_t* __restrict__ Yx, const int* __restrict__ Zp,
                                                    int* __restrict__ Zj, value_t* __restrict__ Zx)
{
    constexpr int RPB = BLOCK / G;
    __shared__ int sCol[RPB][CAP + 1];
    __shared__ int sW[BLOCK / 64];
    const int tid = threadIdx.x, g = tid / G, lane = tid % G;
    const int qi = blockIdx.x * RPB + g;
    int x0 = 0, a = 0, y0 = 0, b = 0, out = 0, zEnd = 0;
    if (qi < nq) {
        const int row = queue[qi];
        x0 = Xp[row];
        a = Xp[row + 1] - x0;
        y0 = Yp[row];
        b = Yp[row + 1] - y0;
        out = Zp[row];
        zEnd = Zp[row + 1];
    }
    if (G < BLOCK && a + b > CAP) a = b = 0;                  // (the binning keeps such rows out: this only guards the LDS)
    int* sx = sCol[g];
    int i0 = 0, j0 = 0;
    do {
        int ax = a - i0, by = b - j0;
        if (G == BLOCK && ax + by > CAP) {
            // merge path: how many of the next CAP merged entries are X's
            int lo = max(0, CAP - by), hi = min(ax, CAP);
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if (Xj[x0 + i0 + mid] <= Yj[y0 + j0 + CAP - mid - 1]) lo = mid + 1; else hi = mid;
            }
            int jy = CAP - lo;
            if (lo > 0 && jy < by && Xj[x0 + i0 + lo - 1] == Yj[y0 + j0 + jy]) ++jy;
            ax = lo;
            by = jy;
        }
        int* sy = sx + ax;
        for (int t = lane; t < ax; t += G) sx[t] = Xj[x0 + i0 + t];
        for (int t = lane; t < by; t += G) sy[t] = Yj[y0 + j0 + t];
        __syncthreads();
        int matched = 0;
        for (int t0 = 0; t0 < ax; t0 += G) {                  // X's entries: all of them are entries of Z
            const int i = t0 + lane;
            int c = 0, lb = 0, hit = 0;
            if (i < ax) {
                c = sx[i];
                lb = add_lower_bound(sy, by, c);
                hit = (lb < by && sy[lb] == c) ? 1 : 0;
            }
            int tot;
            const int before = add_scan_flags<G>(hit, tid, sW, tot);
            if (i < ax) {
                const int pos = out + i + lb - (matched + before);
                const double x = (double)Xx[x0 + i0 + i];
                const double v = hit ? alpha * x + beta * (double)Yx[y0 + j0 + lb] : alpha * x;
                if (pos < zEnd) { Zj[pos] = c; Zx[pos] = (value_t)v; }
            }
            matched += tot;
        }
        int matchedY = 0;
        for (int t0 = 0; t0 < by; t0 += G) {                  // Y's entries: those outside X
            const int j = t0 + lane;
            int c = 0, lb = 0, hit = 0;
            if (j < by) {
                c = sy[j];
                lb = add_lower_bound(sx, ax, c);
                hit = (lb < ax && sx[lb] == c) ? 1 : 0;
            }
            int tot;
            const int before = add_scan_flags<G>(hit, tid, sW, tot);
            if (j < by && !hit) {
                const int pos = out + j + lb - (matchedY + before);
                if (pos < zEnd) { Zj[pos] = c; Zx[pos] = (value_t)(beta * (double)Yx[y0 + j0 + j]); }
            }
            matchedY += tot;
        }
        out += ax + by - matched;
        i0 += ax;
        j0 += by;
        if (G == BLOCK) __syncthreads();                      // (the next chunk reuses the LDS)
    } while (G == BLOCK && (i0 < a || j0 < b));
}

// ---- in place, alpha == 1: only the entries Y names ----
__global__ __launch_bounds__(256) void k_add_inplace(int nnzY, double beta, const value_t* __restrict__ Yx,
                                                     const int* __restrict__ ypos, value_t* __restrict__ Xx)
{
    const long long stride = (long long)gridDim.x * 256;
    for (long long q = (long long)blockIdx.x * 256 + threadIdx.x; q < nnzY; q += stride) {
        const int p = ypos[q];
        if (p >= 0) Xx[p] = (value_t)((double)Xx[p] + beta * (double)Yx[q]);
    }
}

// ---- in place, any alpha: G lanes per row of X, every entry scaled, beta y added where Y's row has the column ----
template <int G>
__global__ __launch_bounds__(256) void k_add_inplace_rows(int m, double alpha, const int* __restrict__ Xp, const int* __restrict__ Xj,
                                                          value_t* __restrict__ Xx, double beta, const int* __restrict__ Yp,
                                                          const int* __restrict__ Yj, const value_t* __restrict__ Yx)
{
    const int lane = threadIdx.x % G;
    const long long groups = (long long)gridDim.x * (256 / G);
    for (long long row = (long long)blockIdx.x * (256 / G) + threadIdx.x / G; row < m; row += groups) {
        const int x0 = Xp[row], x1 = Xp[row + 1], y0 = Yp[row], b = Yp[row + 1] - y0;
        for (int q = x0 + lane; q < x1; q += G) {
            const int c = Xj[q];
            const double x = (double)Xx[q];
            const int lb = b > 0 ? add_lower_bound(Yj + y0, b, c) : 0;
            const bool hit = lb < b && Yj[y0 + lb] == c;
            Xx[q] = (value_t)(hit ? alpha * x + beta * (double)Yx[y0 + lb] : alpha * x);
        }
    }
}

}  // namespace bhs
