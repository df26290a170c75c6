// bhs_select.hip.h -- the selection of entries of a CSR matrix by position, magnitude and rank within the row
// (bhs_csr_select_*_device, bhs_spgemm_select[_device]; the rule is worded in include/bhsparse_hip.h, "entry selection").
// A stable compaction: the survivors keep their order and their bits.  Nothing is computed on values but comparisons and
// the one double product rel_tol * rowmax; no atomics on values, nothing depends on scheduling.
//
//   k_sel_count       one pass over X: validity (rowPtr monotone and within [0, nnz], columns in [0, n); rows need not be
//                     ascending), the survivors of every row of up to kSelWaveL entries, the row's bin by its length,
//                     nnz(Z).  16 lanes per row, rows appended to per-bin queues with one atomic per workgroup and bin.
//                     The count needs no cut: with TOPK it is min(candidates, top_k) (+ the diagonals KEEP_DIAG lets by).
//   k_sel_count_long  the rows k_sel_count queued as long, a workgroup per row (a hub row streams at the device's rate, not
//                     at that of 16 lanes)
//   k_sel_bin         the bins alone, from the two row pointers (bhs_csr_select_numeric_device: nothing of X is read twice)
//   k_sel_fill<G, TOPK>  G lanes per row: 16 (short bin, rows of up to 32 entries, four rows per wave, both entries of a lane
//                     in registers), 64 (a wave per row) or 256 (a workgroup per row, any length).  The rule is evaluated
//                     again; a survivor's slot is its exclusive rank among the survivors (ballot + popcount, the DPP scan,
//                     the DPP scan + wave totals in LDS).  A row whose survivors are not what rowPtrZ says raises SL_ERR and
//                     never writes outside its own slice of Z.
//                     TOPK = false: streaming; one extra pass over the row where REL needs its maximum.
//                     TOPK = true: a row with more candidates than top_k needs its cut -- the rank key of the top_k-th
//                     largest candidate and how many entries of exactly that key to admit from the front of the row.
//                       G = 16   no cut: every entry counts the entries that beat it (shuffles within the group)
//                       G = 64   keys staged in LDS (8 KB a wave, one wave per workgroup), most-significant-digit radix
//                                select: 8-bit digit, 256-bin LDS histogram, scan of the histogram, descent into one bin;
//                                stops as soon as the bin holds one key
//                       G = 256  the same select, the row's values read again from HBM / L2 for every digit
// The rank key of an entry is the bit pattern of fabs((double)v) read as an unsigned 64-bit integer (NaN above Inf).
#pragma once
#include "bhs_kernels.hip.h"
#include "bhs_wave.hip.h"
#include "bhs_add.hip.h"

namespace bhs {

enum { kSelShort = 0, kSelWave = 1, kSelLong = 2, kSelBins = 3 };
constexpr int kSelShortL = 32;        // short bin: two entries a lane of a 16-lane group
constexpr int kSelWaveL = 1024;       // wave bin: the row's keys fit a wave's LDS slice (8 KB)
constexpr int kSelCountG = 16;        // lanes per row of k_sel_count
constexpr int kSelCountRows = 256;    // rows per workgroup of it

// flags of the rule (BHS_SEL_* of include/bhsparse_hip.h)
enum { SEL_BAND = 1, SEL_DROP_DIAG = 2, SEL_KEEP_DIAG = 4, SEL_ABS = 8, SEL_REL = 16, SEL_TOPK = 32, SEL_VALUE = 8 | 16 | 32 };

struct SelSpec {
    unsigned flags;
    int topK;
    long long lo, hi;
    double absTol, relTol;
};

// counters of the selection (ints of its own workspace block): rows per bin, error flag, the scan's ticket / longest row /
// total / histogram words, nnz(Z)
enum { SL_COUNT = 0, SL_ERR = 4, SL_TICKET = 6, SL_MAXCNT = 7, SL_TOTAL = 8 /* u64 */, SL_SCANTOTAL = 10 /* i64 */,
       SL_SCANBINS = 12 /* kMaxBins */, SL_INTS = 32 };

typedef unsigned long long sel_u64;

__device__ __forceinline__ sel_u64 sel_key(const value_t* __restrict__ Xx, int q)
{
    return Xx ? (sel_u64)__double_as_longlong(fabs((double)Xx[q])) : 0ull;
}

// the word of lane j of the caller's 16-lane group
__device__ __forceinline__ sel_u64 sel_shfl16(sel_u64 v, int j)
{
    const unsigned lo = (unsigned)__shfl((int)(unsigned)v, j, 16), hi = (unsigned)__shfl((int)(unsigned)(v >> 32), j, 16);
    return ((sel_u64)hi << 32) | lo;
}

// stage 1
__device__ __forceinline__ bool sel_pos(const SelSpec& s, int row, int col)
{
    if (s.flags & SEL_BAND) {
        const long long d = (long long)col - (long long)row;
        if (d < s.lo || d > s.hi) return false;
    }
    return !((s.flags & SEL_DROP_DIAG) && col == row);
}

// does the entry enter the row maximum (it passed stage 1 and is not a diagonal KEEP_DIAG sets apart)
__device__ __forceinline__ bool sel_in_max(const SelSpec& s, int row, int col)
{
    return sel_pos(s, row, col) && !((s.flags & SEL_KEEP_DIAG) && col == row);
}

// stages 1-3 of one entry: 0 dropped; ~0 kept whatever follows (the diagonal under KEEP_DIAG); else key + 1, a candidate of
// stage 4 (a key has its sign bit clear: key + 1 is neither 0 nor ~0)
constexpr sel_u64 kSelKeep = ~0ull;
__device__ __forceinline__ sel_u64 sel_eval(const SelSpec& s, int row, int col, sel_u64 key, double thr)
{
    if (!sel_pos(s, row, col)) return 0ull;
    if ((s.flags & SEL_KEEP_DIAG) && col == row) return kSelKeep;
    const double mag = __longlong_as_double((long long)key);
    if ((s.flags & SEL_ABS) && mag <= s.absTol) return 0ull;      // (written so that NaN is kept)
    if ((s.flags & SEL_REL) && mag < thr) return 0ull;
    return key + 1ull;
}

__device__ __forceinline__ double sel_threshold(const SelSpec& s, sel_u64 maxKey)
{
    return s.relTol * __longlong_as_double((long long)maxKey);
}

// survivors of a row with c1 unconditional entries and c2 candidates
__device__ __forceinline__ int sel_row_count(const SelSpec& s, int c1, int c2)
{
    return c1 + ((s.flags & SEL_TOPK) ? min(c2, s.topK) : c2);
}

// Thread t of the workgroup owns row rowBase + t of L entries: the row joins its bin's queue (see add_enqueue).
__device__ __forceinline__ void sel_enqueue(int m, int row, int L, int* sCnt, int* sBase, int* __restrict__ ctl,
                                            int* __restrict__ queue)
{
    const int tid = threadIdx.x;
    const int bin = (row >= m || L <= 0) ? -1 : L <= kSelShortL ? kSelShort : L <= kSelWaveL ? kSelWave : kSelLong;
    int rank = 0;
    if (bin >= 0) rank = atomicAdd(&sCnt[bin], 1);
    __syncthreads();
    if (tid < kSelBins && sCnt[tid]) sBase[tid] = atomicAdd(ctl + SL_COUNT + tid, sCnt[tid]);
    __syncthreads();
    if (bin >= 0) queue[(size_t)bin * m + sBase[bin] + rank] = row;
}

__global__ __launch_bounds__(256) void k_sel_count(int m, int n, int nnzX, const int* __restrict__ Xp, const int* __restrict__ Xj,
                                                   const value_t* __restrict__ Xx, SelSpec spec, int* __restrict__ cnt,
                                                   int* __restrict__ ctl, int* __restrict__ queue)
{
    __shared__ int sRowCnt[kSelCountRows], sRowLen[kSelCountRows];
    __shared__ int sCnt[kSelBins], sBase[kSelBins];
    __shared__ unsigned long long sTot;
    const int tid = threadIdx.x, lane = tid & 63, sl = tid & (kSelCountG - 1);
    if (tid < kSelBins) sCnt[tid] = 0;
    if (tid == 0) sTot = 0;
    const int rowBase = blockIdx.x * kSelCountRows;
    bool bad = blockIdx.x == 0 && tid == 0 && (Xp[0] != 0 || Xp[m] != nnzX);
    for (int it = 0; it < kSelCountRows / (256 / kSelCountG); ++it) {
        const int slot = it * (256 / kSelCountG) + tid / kSelCountG;
        const int row = rowBase + slot;
        int c1 = 0, c2 = 0, len = 0;
        if (row < m) {
            const int x0 = Xp[row], x1 = Xp[row + 1];
            if (x0 < 0 || x1 < x0 || x1 > nnzX) bad = true;       // (nothing of a row with bad bounds is read)
            else if (x1 - x0 <= kSelWaveL) {
                len = x1 - x0;
                sel_u64 mx = 0;
                if (spec.flags & SEL_REL) {
                    for (int q = x0 + sl; q < x1; q += kSelCountG)
                        if (sel_in_max(spec, row, Xj[q])) mx = max(mx, sel_key(Xx, q));
#pragma unroll
                    for (int o = kSelCountG / 2; o >= 1; o >>= 1) mx = max(mx, (sel_u64)__shfl_xor((long long)mx, o));
                }
                const double thr = sel_threshold(spec, mx);
                for (int q = x0 + sl; q < x1; q += kSelCountG) {
                    const int c = Xj[q];
                    if (c < 0 || c >= n) bad = true;
                    const sel_u64 w = sel_eval(spec, row, c, (spec.flags & SEL_VALUE) ? sel_key(Xx, q) : 0ull, thr);
                    c1 += w == kSelKeep ? 1 : 0;
                    c2 += (w != 0ull && w != kSelKeep) ? 1 : 0;
                }
            } else len = x1 - x0;                                 // (k_sel_count_long counts and checks the row)
        }
#pragma unroll
        for (int o = kSelCountG / 2; o >= 1; o >>= 1) { c1 += __shfl_xor(c1, o); c2 += __shfl_xor(c2, o); }
        if (sl == 0) { sRowCnt[slot] = sel_row_count(spec, c1, c2); sRowLen[slot] = len; }
    }
    if (__ballot(bad) != 0ull && lane == 0) atomicOr(ctl + SL_ERR, 1);
    __syncthreads();
    const int row = rowBase + tid;
    const int c = sRowCnt[tid];
    if (row < m && sRowLen[tid] <= kSelWaveL) cnt[row] = c;
    long long t64 = c;
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) t64 += __shfl_xor(t64, o);
    if (lane == 0 && t64) atomicAdd(&sTot, (unsigned long long)t64);
    sel_enqueue(m, row, sRowLen[tid], sCnt, sBase, ctl, queue);
    if (tid == 0 && sTot) atomicAdd((unsigned long long*)(ctl + SL_TOTAL), sTot);
}

// maximum / sum over the workgroup's 256 threads, result in every thread (two barriers)
__device__ __forceinline__ sel_u64 sel_wg_max(sel_u64 v, int tid, sel_u64* sRed)
{
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v = max(v, (sel_u64)__shfl_xor((long long)v, o));
    if ((tid & 63) == 0) sRed[tid >> 6] = v;
    __syncthreads();
    v = max(max(sRed[0], sRed[1]), max(sRed[2], sRed[3]));
    __syncthreads();
    return v;
}

// The long rows of k_sel_count's queue, a workgroup per row; the number of rows is read from the device (the host has not
// seen it yet): the workgroups stride over the queue.
__global__ __launch_bounds__(256) void k_sel_count_long(int m, int n, const int* __restrict__ Xp, const int* __restrict__ Xj,
                                                        const value_t* __restrict__ Xx, SelSpec spec, int* __restrict__ cnt,
                                                        int* __restrict__ ctl, const int* __restrict__ queue)
{
    __shared__ sel_u64 sRed[4];
    __shared__ int sW[4];
    const int tid = threadIdx.x;
    const int nq = ctl[SL_COUNT + kSelLong];
    for (int qi = blockIdx.x; qi < nq; qi += gridDim.x) {
        const int row = queue[(size_t)kSelLong * m + qi];
        const int x0 = Xp[row], x1 = Xp[row + 1];                 // (bounds checked by k_sel_count)
        sel_u64 mx = 0;
        if (spec.flags & SEL_REL) {
            for (int q = x0 + tid; q < x1; q += 256)
                if (sel_in_max(spec, row, Xj[q])) mx = max(mx, sel_key(Xx, q));
            mx = sel_wg_max(mx, tid, sRed);
        }
        const double thr = sel_threshold(spec, mx);
        int c1 = 0, c2 = 0;
        bool bad = false;
        for (int q = x0 + tid; q < x1; q += 256) {
            const int c = Xj[q];
            if (c < 0 || c >= n) bad = true;
            const sel_u64 w = sel_eval(spec, row, c, (spec.flags & SEL_VALUE) ? sel_key(Xx, q) : 0ull, thr);
            c1 += w == kSelKeep ? 1 : 0;
            c2 += (w != 0ull && w != kSelKeep) ? 1 : 0;
        }
        int t1, t2;
        (void)add_scan_flags<256>(c1, tid, sW, t1);
        (void)add_scan_flags<256>(c2, tid, sW, t2);
        if (__ballot(bad) != 0ull && (tid & 63) == 0) atomicOr(ctl + SL_ERR, 1);
        if (tid == 0) {
            const int c = sel_row_count(spec, t1, t2);
            cnt[row] = c;
            if (c) atomicAdd((unsigned long long*)(ctl + SL_TOTAL), (unsigned long long)c);
        }
    }
}

// bhs_csr_select_numeric_device: the bins from the row pointers; SL_ERR when they cannot belong together (a rowPtr that is
// not monotone within its nnz, a row of Z longer than its row of X)
__global__ __launch_bounds__(256) void k_sel_bin(int m, int nnzX, const int* __restrict__ Xp, const int* __restrict__ Zp,
                                                 int* __restrict__ ctl, int* __restrict__ queue)
{
    __shared__ int sCnt[kSelBins], sBase[kSelBins];
    const int tid = threadIdx.x;
    if (tid < kSelBins) sCnt[tid] = 0;
    __syncthreads();
    const int row = blockIdx.x * 256 + tid;
    bool bad = blockIdx.x == 0 && tid == 0 && (Xp[0] != 0 || Xp[m] != nnzX || Zp[0] != 0);
    int L = 0;
    if (row < m) {
        const int x0 = Xp[row], x1 = Xp[row + 1], z0 = Zp[row], z = Zp[row + 1] - z0;
        if (x0 < 0 || x1 < x0 || x1 > nnzX || z0 < 0 || z < 0 || z > x1 - x0) bad = true;
        else L = x1 - x0;
    }
    if (__ballot(bad) != 0ull && (tid & 63) == 0) atomicOr(ctl + SL_ERR, 1);
    sel_enqueue(m, row, bad ? 0 : L, sCnt, sBase, ctl, queue);
}

// The cut of a row with more than k >= 1 candidates: T = the k-th largest of w(0 .. len), quota = how many entries equal to T
// are among the k largest.  Most-significant-digit radix select; G = 64 (a wave that is the whole workgroup) or 256: every
// thread of the workgroup takes part.  hist: 256 ints, sBc: 4 ints, sT: one word.
template <int G, typename F>
__device__ __forceinline__ void sel_radix_cut(int len, int k, F w_at, int* hist, int* sW, int* sBc, sel_u64* sT, sel_u64& T,
                                              int& quota)
{
    constexpr int BPL = 256 / G;                                  // bins a thread owns
    const int tid = threadIdx.x;
    sel_u64 prefix = 0, mask = 0;
    int rem = k;
    for (int shift = 56; shift >= 0; shift -= 8) {
#pragma unroll
        for (int b = 0; b < BPL; ++b) hist[tid * BPL + b] = 0;
        __syncthreads();
        for (int i = tid; i < len; i += G) {
            const sel_u64 w = w_at(i);
            if ((w & mask) == prefix) atomicAdd(&hist[(int)(w >> shift) & 255], 1);
        }
        __syncthreads();
        int hb[BPL], s = 0;
#pragma unroll
        for (int b = 0; b < BPL; ++b) { hb[b] = hist[tid * BPL + b]; s += hb[b]; }
        int tot;
        const int excl = add_scan_flags<G>(s, tid, sW, tot);
        int greater = tot - excl - s;                             // keys in the bins above this thread's
#pragma unroll
        for (int b = BPL - 1; b >= 0; --b) {
            if (greater < rem && rem <= greater + hb[b]) { sBc[0] = tid * BPL + b; sBc[1] = rem - greater; sBc[2] = hb[b]; }
            greater += hb[b];
        }
        __syncthreads();
        const int d = sBc[0], inBin = sBc[2];
        rem = sBc[1];
        prefix |= (sel_u64)d << shift;
        mask |= 255ull << shift;
        if (inBin == 1 && shift > 0) {                            // resolved: the one key of the bin is the cut
            for (int i = tid; i < len; i += G) {
                const sel_u64 w = w_at(i);
                if ((w & mask) == prefix) *sT = w;
            }
            __syncthreads();
            prefix = *sT;
            break;
        }
    }
    __syncthreads();                                              // (sBc / sT may be written again by the next row)
    T = prefix;
    quota = rem;
}

// ---- the fill pass ----
template <int G, bool TOPK, int BLOCK>
__global__ __launch_bounds__(BLOCK) void k_sel_fill(int nq, const int* __restrict__ queue, SelSpec spec, const int* __restrict__ Xp,
                                                    const int* __restrict__ Xj, const value_t* __restrict__ Xx,
                                                    const int* __restrict__ Zp, int* __restrict__ Zj, value_t* __restrict__ Zx,
                                                    int* __restrict__ ctl)
{
    constexpr int RPB = BLOCK / G;
    static_assert(G == 16 || RPB == 1 || !TOPK, "the radix select's barriers want one row per workgroup");
    __shared__ int sW[4], sBc[4];
    __shared__ sel_u64 sRed[4], sT;
    __shared__ int sHist[(TOPK && G >= 64) ? 256 : 1];
    __shared__ sel_u64 sKey[(TOPK && G == 64) ? kSelWaveL : 1];
    const int tid = threadIdx.x, g = tid / G, lane = tid % G;
    const int qi = blockIdx.x * RPB + g;
    int row = 0, x0 = 0, len = 0, out = 0, zEnd = 0;
    if (qi < nq) {
        row = queue[qi];
        x0 = Xp[row];
        len = Xp[row + 1] - x0;
        out = Zp[row];
        zEnd = Zp[row + 1];
    }
    const bool useVal = (spec.flags & SEL_VALUE) != 0;
    (void)sW; (void)sBc; (void)sRed; (void)sT; (void)sHist; (void)sKey;

    if constexpr (G == 16) {
        // both entries of the lane in registers; every group of the wave runs the same two steps
        if (len > kSelShortL) len = 0;                            // (the binning keeps such rows out)
        int col[2] = {0, 0};
        sel_u64 key[2] = {0, 0}, w[2] = {0, 0};
        sel_u64 mx = 0;
#pragma unroll
        for (int e = 0; e < 2; ++e) {
            const int i = e * 16 + lane;
            if (i < len) {
                col[e] = Xj[x0 + i];
                key[e] = useVal ? sel_key(Xx, x0 + i) : 0ull;
                if (sel_in_max(spec, row, col[e])) mx = max(mx, key[e]);
            }
        }
#pragma unroll
        for (int o = 8; o >= 1; o >>= 1) mx = max(mx, (sel_u64)__shfl_xor((long long)mx, o));
        const double thr = sel_threshold(spec, mx);
#pragma unroll
        for (int e = 0; e < 2; ++e)
            if (e * 16 + lane < len) w[e] = sel_eval(spec, row, col[e], key[e], thr);
        bool keep[2] = {w[0] != 0ull, w[1] != 0ull};
        if constexpr (TOPK) {
            // a candidate survives when fewer than top_k candidates beat it: a larger key, or the same key earlier in the row
            const sel_u64 c0 = w[0] == kSelKeep ? 0ull : w[0], c1 = w[1] == kSelKeep ? 0ull : w[1];
            int beat0 = 0, beat1 = 0;
            for (int j = 0; j < 16; ++j) {
                const sel_u64 a = sel_shfl16(c0, j), b = sel_shfl16(c1, j);
                beat0 += (a > c0 || (a == c0 && j < lane)) ? 1 : 0;
                beat0 += b > c0 ? 1 : 0;
                beat1 += (a >= c1) ? 1 : 0;
                beat1 += (b > c1 || (b == c1 && j < lane)) ? 1 : 0;
            }
            if (c0 != 0ull) keep[0] = beat0 < spec.topK;
            if (c1 != 0ull) keep[1] = beat1 < spec.topK;
        }
#pragma unroll
        for (int e = 0; e < 2; ++e) {
            int tot;
            const int before = add_scan_flags<16>(keep[e] ? 1 : 0, tid, nullptr, tot);
            if (keep[e]) {
                const int pos = out + before;
                if (pos < zEnd) {
                    Zj[pos] = col[e];
                    if (Zx) Zx[pos] = Xx[x0 + e * 16 + lane];
                }
            }
            out += tot;
        }
        if (qi < nq && lane == 0 && out != zEnd) atomicOr(ctl + SL_ERR, 1);
    } else {
        // G = 64: wave-uniform; G = 256: workgroup-uniform (one row per workgroup wherever a barrier is met)
        sel_u64 mx = 0;
        if (spec.flags & SEL_REL) {
            for (int i = lane; i < len; i += G)
                if (sel_in_max(spec, row, Xj[x0 + i])) mx = max(mx, sel_key(Xx, x0 + i));
            if constexpr (G == 64) {
#pragma unroll
                for (int o = 32; o >= 1; o >>= 1) mx = max(mx, (sel_u64)__shfl_xor((long long)mx, o));
            } else mx = sel_wg_max(mx, tid, sRed);
        }
        const double thr = sel_threshold(spec, mx);
        auto w_mem = [&](int i) -> sel_u64 {
            return sel_eval(spec, row, Xj[x0 + i], useVal ? sel_key(Xx, x0 + i) : 0ull, thr);
        };
        sel_u64 T = 0;                                            // a candidate w survives when w > T, or w == T within the quota
        int quota = 0;
        if constexpr (TOPK) {
            if (G == 64 && len > kSelWaveL) len = 0;              // (the binning keeps such rows out: this only guards the LDS)
            int c2 = 0;
            for (int i = lane; i < len; i += G) {
                sel_u64 w = w_mem(i);
                if (w == kSelKeep) w = 0ull;                      // (the select sees candidates only)
                if constexpr (G == 64) sKey[i] = w;
                c2 += w != 0ull ? 1 : 0;
            }
            int tot;
            (void)add_scan_flags<G>(c2, tid, sW, tot);
            if (spec.topK == 0) T = kSelKeep;                     // no candidate survives
            else if (tot > spec.topK) {
                if constexpr (G == 64) {
                    __syncthreads();
                    sel_radix_cut<G>(len, spec.topK, [&](int i) -> sel_u64 { return sKey[i]; }, sHist, sW, sBc, &sT, T, quota);
                } else {
                    sel_radix_cut<G>(len, spec.topK, [&](int i) -> sel_u64 { const sel_u64 w = w_mem(i); return w == kSelKeep ? 0ull : w; },
                                     sHist, sW, sBc, &sT, T, quota);
                }
            }
        }
        int ties = 0;                                             // entries equal to the cut met so far
        for (int t0 = 0; t0 < len; t0 += G) {
            const int i = t0 + lane;
            int c = 0;
            sel_u64 w = 0;
            if (i < len) {
                c = Xj[x0 + i];
                w = w_mem(i);
            }
            bool keep = w != 0ull;
            if constexpr (TOPK) {
                const int tie = (w == T && w != kSelKeep) ? 1 : 0;
                int tieTot;
                const int tieBefore = add_scan_flags<G>(tie, tid, sW, tieTot);
                if (w != 0ull && w != kSelKeep) keep = w > T || (tie && ties + tieBefore < quota);
                ties += tieTot;
            }
            int tot;
            const int before = add_scan_flags<G>(keep ? 1 : 0, tid, sW, tot);
            if (keep) {
                const int pos = out + before;
                if (pos < zEnd) {
                    Zj[pos] = c;
                    if (Zx) Zx[pos] = Xx[x0 + i];
                }
            }
            out += tot;
        }
        if (qi < nq && lane == 0 && out != zEnd) atomicOr(ctl + SL_ERR, 1);
    }
}

}  // namespace bhs
