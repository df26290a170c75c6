// bhs_reduce.hip.h -- reductions of a CSR matrix to a vector or a scalar, and the diagonal scaling Z = alpha Dl X Dr
// (bhs_csr_reduce_device, bhs_csr_scale_device; the contract is worded in include/bhsparse_hip.h, "reduce / scale").
//
// Every entry is converted to double and reduced in double.  An accumulator is one 64-bit word whatever the operator: the
// bits of the running double for the sums, an order-preserving integer key of the double for min and max (rd_key: unsigned
// order of the keys == numeric order of the values with -0 below +0; a NaN gets the key that wins, so it comes out).  That
// makes min, max and count bit-for-bit functions of the input on every path, atomics included (integer min / max, adds of
// 1.0), and leaves the order of the additions as the only freedom of the sums.  It is fixed -- a function of the input and
// this file -- everywhere except on axis COLS, whose sums meet in memory through atomics.
//
// No kernel writes the caller's d_out: all of them reduce into 64-bit words of scratch and raise ctl[RD_ERR] for what the
// validation refuses; k_red_finish looks at that word, and only where it is clear rounds once and stores.
//
//   k_red_short   all rows in order, 16 lanes a row, 256 rows a workgroup: the row pointer's validation (every row), the
//                 rows of up to 32 entries reduced on the spot (two entries a lane, DPP butterfly within the 16 lanes),
//                 the longer ones queued for
//   k_red_wave    up to 1024 entries, a wave per row, and
//   k_red_long    a workgroup per row.  Axis ROWS and DIAG (the entries with col == row of the rows below min(m, n)).
//   k_red_rowlen  COUNT on ROWS: the row pointer alone
//   k_red_cols    axis COLS, 2048 consecutive entries a workgroup: what falls into the window of 2048 columns from the
//                 workgroup's lowest column meets in LDS first and goes to memory once per column and workgroup, as
//                 contiguous runs; the rest goes to memory entry by entry
//   k_red_all     axis ALL: a contiguous piece of the values per workgroup, one partial each; the number of workgroups
//                 depends on the number of entries alone
//   k_red_finish  the error word, the partials of k_red_all in a fixed order, the rounding, the store
//   k_sc_check    the scale: the row pointer's validation, BEFORE the kernels that write (they leave at once where it failed)
//   k_sc_flat     no left vector: entry by entry, no row needed
//   k_sc_short / k_sc_wave / k_sc_long   with a left vector: by rows, binned as above
#pragma once
#include "bhs_kernels.hip.h"
#include "bhs_wave.hip.h"

namespace bhs {

typedef unsigned long long rd_u64;

enum { kRdSum = 0, kRdMin = 1, kRdMax = 2 };                 // what combines two accumulators
enum { kRdOpPlus = 0, kRdOpMin = 1, kRdOpMax = 2, kRdOpAbsPlus = 3, kRdOpAbsMax = 4, kRdOpSqPlus = 5, kRdOpCount = 6 };   // BHS_RED_*
enum { kRdAll = 0, kRdOffdiag = 1, kRdDiag = 2 };            // which entries of a row count
constexpr int kRdShortL = 32;         // short bin: two entries a lane of a 16-lane group
constexpr int kRdWaveL = 1024;        // wave bin
constexpr int kRdG = 16;              // lanes per row of the short kernels
constexpr int kRdRows = 256;          // rows per workgroup of them
constexpr int kRdColE = 8;            // k_red_cols: entries a thread
constexpr int kRdColW = 2048;         // ... columns of its LDS window (16 KB)
constexpr int kRdAllPer = 256 * 16;   // k_red_all: entries a workgroup at least
constexpr int kRdAllMax = 2048;       // ... workgroups at most
constexpr int kScFlatE = 4;           // k_sc_flat: entries a thread

// counters (ints of the workspace block): rows queued for the wave and the long kernel, the error flag
enum { RD_CNT_WAVE = 0, RD_CNT_LONG = 1, RD_ERR = 2, RD_INTS = 4 };

__host__ __device__ __forceinline__ rd_u64 rd_bits(double x)
{
    rd_u64 b;
    __builtin_memcpy(&b, &x, 8);
    return b;
}

__host__ __device__ __forceinline__ double rd_real(rd_u64 b)
{
    double x;
    __builtin_memcpy(&x, &b, 8);
    return x;
}

// the key of x: unsigned order of keys == order of the values as numbers, -0 below +0; a NaN gets the largest key under
// max and the smallest under min (both decode to a NaN)
__host__ __device__ __forceinline__ rd_u64 rd_key(double x, bool forMax)
{
    if (x != x) return forMax ? ~0ull : 0ull;
    const rd_u64 b = rd_bits(x);
    return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}

__host__ __device__ __forceinline__ double rd_unkey(rd_u64 k)
{
    return rd_real((k >> 63) ? (k & 0x7fffffffffffffffull) : ~k);
}

// the accumulator of a row, column or diagonal without an entry
__host__ __device__ __forceinline__ rd_u64 rd_identity(int kind, int op)
{
    if (kind == kRdSum) return 0ull;                              // +0
    if (kind == kRdMin) return rd_key(__builtin_inf(), false);
    return op == kRdOpAbsMax ? rd_key(0.0, true) : rd_key(-__builtin_inf(), true);
}

template <int KIND>
__device__ __forceinline__ rd_u64 rd_term(int op, double x)
{
    if constexpr (KIND == kRdSum) return rd_bits(op == kRdOpAbsPlus ? fabs(x) : op == kRdOpSqPlus ? x * x : x);
    else if constexpr (KIND == kRdMin) return rd_key(x, false);
    else return rd_key(op == kRdOpAbsMax ? fabs(x) : x, true);
}

template <int KIND>
__device__ __forceinline__ rd_u64 rd_comb(rd_u64 a, rd_u64 b)
{
    if constexpr (KIND == kRdSum) return rd_bits(rd_real(a) + rd_real(b));
    else if constexpr (KIND == kRdMin) return a < b ? a : b;
    else return a < b ? b : a;
}

template <int KIND>
__device__ __forceinline__ void rd_atomic(rd_u64* p, rd_u64 v)
{
    if constexpr (KIND == kRdSum) (void)atomicAdd((double*)p, rd_real(v));
    else if constexpr (KIND == kRdMin) (void)atomicMin(p, v);
    else (void)atomicMax(p, v);
}

template <int KIND>
__device__ __forceinline__ value_t rd_round(rd_u64 v)
{
    if constexpr (KIND == kRdSum) return (value_t)rd_real(v);
    else return (value_t)rd_unkey(v);
}

// butterfly over W = 16 (a DPP row) or 64 lanes, all of them active: every lane ends with the same word (an IEEE add is
// commutative, so both partners of a step compute the same bits)
template <int KIND, int W>
__device__ __forceinline__ rd_u64 rd_lanes(rd_u64 v, int lane)
{
    v = rd_comb<KIND>(v, lane_xor64<1>(v, lane));
    v = rd_comb<KIND>(v, lane_xor64<2>(v, lane));
    v = rd_comb<KIND>(v, lane_xor64<4>(v, lane));
    v = rd_comb<KIND>(v, lane_xor64<8>(v, lane));
    if constexpr (W == 64) {
        v = rd_comb<KIND>(v, lane_xor64<16>(v, lane));
        v = rd_comb<KIND>(v, lane_xor64<32>(v, lane));
    }
    return v;
}

// the four waves' words in a fixed order; the result in thread 0
template <int KIND>
__device__ __forceinline__ rd_u64 rd_block(rd_u64 v, int tid, rd_u64* sW)
{
    v = rd_lanes<KIND, 64>(v, tid & 63);
    if ((tid & 63) == 0) sW[tid >> 6] = v;
    __syncthreads();
    if (tid == 0) v = rd_comb<KIND>(rd_comb<KIND>(rd_comb<KIND>(sW[0], sW[1]), sW[2]), sW[3]);
    return v;
}

// are a row's bounds what a row pointer may hold
__device__ __forceinline__ bool rd_bounds_bad(int a, int b, int nnzX) { return a < 0 || b < a || b > nnzX; }

// the whole row pointer, once: thread `gid` of `total`
__device__ __forceinline__ bool rd_rowptr_bad(int m, int nnzX, const int* __restrict__ Xp, long long gid, long long total)
{
    bool bad = gid == 0 && (Xp[0] != 0 || Xp[m] != nnzX);
    for (long long t = gid; t < m; t += total) bad |= rd_bounds_bad(Xp[t], Xp[t + 1], nnzX);
    return bad;
}

__device__ __forceinline__ void rd_flag(bool bad, int* __restrict__ ctl)
{
    if (__ballot(bad) != 0ull && (threadIdx.x & 63) == 0) atomicOr(ctl + RD_ERR, 1);
}

// what entry q of row r gives (the identity where the filter drops it, or its column is no column: that is flagged)
template <int KIND>
__device__ __forceinline__ rd_u64 rd_entry(int q, int r, int n, const int* __restrict__ Xj, const value_t* __restrict__ Xx, int op,
                                           int filt, rd_u64 id, bool& bad)
{
    if (filt != kRdAll) {
        const int c = Xj[q];
        if ((unsigned)c >= (unsigned)n) { bad = true; return id; }
        if ((c == r) != (filt == kRdDiag)) return id;
    }
    return rd_term<KIND>(op, Xx ? (double)Xx[q] : 1.0);
}

// Thread t of the workgroup owns row rowBase + t of L entries (0: nothing to queue): rows beyond the short bin join the wave
// or the long queue (m ints each)
__device__ __forceinline__ void rd_enqueue(int m, int r, int L, int* sCnt, int* sBase, int* __restrict__ ctl, int* __restrict__ queue)
{
    const int tid = threadIdx.x;
    const int bin = (r >= m || L <= kRdShortL) ? -1 : L <= kRdWaveL ? RD_CNT_WAVE : RD_CNT_LONG;
    int rank = 0;
    if (bin >= 0) rank = atomicAdd(&sCnt[bin], 1);
    __syncthreads();
    if (tid < 2 && sCnt[tid]) sBase[tid] = atomicAdd(ctl + tid, sCnt[tid]);
    __syncthreads();
    if (bin >= 0) queue[(size_t)bin * m + sBase[bin] + rank] = r;
}

// nRead: the rows whose entries count (m, or min(m, n) for the diagonal); the row pointer is checked in all m rows
template <int KIND>
__global__ __launch_bounds__(256) void k_red_short(int m, int n, int nnzX, const int* __restrict__ Xp, const int* __restrict__ Xj,
                                                   const value_t* __restrict__ Xx, int op, int filt, int nRead, rd_u64 id,
                                                   rd_u64* __restrict__ acc, int* __restrict__ ctl, int* __restrict__ queue)
{
    __shared__ int sLen[kRdRows];
    __shared__ int sCnt[2], sBase[2];
    const int tid = threadIdx.x, lane = tid & 63, sl = tid & (kRdG - 1);
    if (tid < 2) sCnt[tid] = 0;
    const int rowBase = blockIdx.x * kRdRows;
    bool bad = blockIdx.x == 0 && tid == 0 && (Xp[0] != 0 || Xp[m] != nnzX);
    for (int it = 0; it < kRdRows / (256 / kRdG); ++it) {
        const int slot = it * (256 / kRdG) + tid / kRdG;
        const int r = rowBase + slot;
        rd_u64 v = id;
        int len = 0;
        if (r < m) {
            const int a = Xp[r], b = Xp[r + 1];
            if (rd_bounds_bad(a, b, nnzX)) bad = true;
            else if (r < nRead) {
                len = b - a;
                if (len <= kRdShortL)
                    for (int i = sl; i < len; i += kRdG) v = rd_comb<KIND>(v, rd_entry<KIND>(a + i, r, n, Xj, Xx, op, filt, id, bad));
            }
        }
        v = rd_lanes<KIND, kRdG>(v, lane);
        if (sl == 0) {
            sLen[slot] = len;
            if (r < nRead && len <= kRdShortL) acc[r] = v;
        }
    }
    __syncthreads();
    rd_flag(bad, ctl);
    rd_enqueue(m, rowBase + tid, sLen[tid], sCnt, sBase, ctl, queue);
}

template <int KIND>
__global__ __launch_bounds__(256) void k_red_wave(int nq, const int* __restrict__ queue, int m, int n, int nnzX,
                                                  const int* __restrict__ Xp, const int* __restrict__ Xj,
                                                  const value_t* __restrict__ Xx, int op, int filt, rd_u64 id,
                                                  rd_u64* __restrict__ acc, int* __restrict__ ctl)
{
    const int lane = threadIdx.x & 63;
    const int qi = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (qi >= nq) return;                                         // (wave-uniform, as everything below)
    const int r = queue[qi];
    if ((unsigned)r >= (unsigned)m) return;
    const int a = Xp[r], b = Xp[r + 1];
    if (rd_bounds_bad(a, b, nnzX)) return;                        // (k_red_short queues no such row)
    const int len = b - a;
    bool bad = false;
    rd_u64 v = id;
    for (int i = lane; i < len; i += 64) v = rd_comb<KIND>(v, rd_entry<KIND>(a + i, r, n, Xj, Xx, op, filt, id, bad));
    v = rd_lanes<KIND, 64>(v, lane);
    rd_flag(bad, ctl);
    if (lane == 0) acc[r] = v;
}

template <int KIND>
__global__ __launch_bounds__(256) void k_red_long(int nq, const int* __restrict__ queue, int m, int n, int nnzX,
                                                  const int* __restrict__ Xp, const int* __restrict__ Xj,
                                                  const value_t* __restrict__ Xx, int op, int filt, rd_u64 id,
                                                  rd_u64* __restrict__ acc, int* __restrict__ ctl)
{
    __shared__ rd_u64 sW[4];
    const int tid = threadIdx.x;
    for (int qi = blockIdx.x; qi < nq; qi += gridDim.x) {         // (everything below is workgroup-uniform)
        const int r = queue[qi];
        if ((unsigned)r >= (unsigned)m) continue;
        const int a = Xp[r], b = Xp[r + 1];
        if (rd_bounds_bad(a, b, nnzX)) continue;
        const int len = b - a;
        bool bad = false;
        rd_u64 v = id;
        for (int i = tid; i < len; i += 256) v = rd_comb<KIND>(v, rd_entry<KIND>(a + i, r, n, Xj, Xx, op, filt, id, bad));
        v = rd_block<KIND>(v, tid, sW);
        rd_flag(bad, ctl);
        if (tid == 0) acc[r] = v;
        __syncthreads();                                          // (sW is the next row's)
    }
}

// COUNT on ROWS without a filter: the row pointer is all that is read
__global__ __launch_bounds__(256) void k_red_rowlen(int m, int nnzX, const int* __restrict__ Xp, rd_u64* __restrict__ acc,
                                                    int* __restrict__ ctl)
{
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    bool bad = t == 0 && (Xp[0] != 0 || Xp[m] != nnzX);
    if (t < m) {
        const int a = Xp[t], b = Xp[t + 1];
        if (rd_bounds_bad(a, b, nnzX)) bad = true;
        else acc[t] = rd_bits((double)(b - a));
    }
    rd_flag(bad, ctl);
}

__global__ __launch_bounds__(256) void k_red_fill(long long count, rd_u64 id, rd_u64* __restrict__ acc)
{
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t < count) acc[t] = id;
}

// the row of entry q among the rows lo .. hi: the last one that starts at or before q (any row pointer ends the search
// inside [lo, hi])
__device__ __forceinline__ int rd_row_of(const int* __restrict__ Xp, int lo, int hi, long long q)
{
    while (lo < hi) {
        const int mid = lo + (hi - lo + 1) / 2;
        if (Xp[mid] <= q) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

// acc: n words holding the identity.  filt: kRdAll or kRdOffdiag (the row of an entry is then searched in the row pointer
// between the rows of the workgroup's first and last entry).
template <int KIND>
__global__ __launch_bounds__(256) void k_red_cols(int m, int n, int nnzX, const int* __restrict__ Xp, const int* __restrict__ Xj,
                                                  const value_t* __restrict__ Xx, int op, int filt, rd_u64 id,
                                                  rd_u64* __restrict__ acc, int* __restrict__ ctl)
{
    __shared__ rd_u64 sWin[kRdColW];
    __shared__ int sMin[4], sRow[2];
    const int tid = threadIdx.x, lane = tid & 63;
    bool bad = rd_rowptr_bad(m, nnzX, Xp, (long long)blockIdx.x * 256 + tid, (long long)gridDim.x * 256);
    const long long base = (long long)blockIdx.x * (256 * kRdColE);
    int c[kRdColE];
    int cmin = 0x7fffffff;
#pragma unroll
    for (int k = 0; k < kRdColE; ++k) {
        const long long q = base + k * 256 + tid;
        c[k] = -1;
        if (q < nnzX) {
            const int cc = Xj[q];
            if ((unsigned)cc >= (unsigned)n) bad = true;
            else { c[k] = cc; cmin = min(cmin, cc); }
        }
    }
    if (filt == kRdOffdiag && m > 0) {
        if (tid < 2) sRow[tid] = rd_row_of(Xp, 0, m - 1, tid == 0 ? base : min(base + 256 * kRdColE, (long long)nnzX) - 1);
        __syncthreads();
        const int lo = min(sRow[0], sRow[1]), hi = max(sRow[0], sRow[1]);
#pragma unroll
        for (int k = 0; k < kRdColE; ++k)
            if (c[k] >= 0 && rd_row_of(Xp, lo, hi, base + k * 256 + tid) == c[k]) c[k] = -1;
    }
    // the window: from the workgroup's lowest column
    unsigned um = (unsigned)cmin;
    um = min(um, lane_xor<1>(um, lane));
    um = min(um, lane_xor<2>(um, lane));
    um = min(um, lane_xor<4>(um, lane));
    um = min(um, lane_xor<8>(um, lane));
    um = min(um, lane_xor<16>(um, lane));
    um = min(um, lane_xor<32>(um, lane));
    if (lane == 0) sMin[tid >> 6] = (int)um;
    for (int s = tid; s < kRdColW; s += 256) sWin[s] = id;
    __syncthreads();
    const int c0 = min(min(sMin[0], sMin[1]), min(sMin[2], sMin[3]));
#pragma unroll
    for (int k = 0; k < kRdColE; ++k) {
        if (c[k] < 0) continue;
        const rd_u64 t = rd_term<KIND>(op, Xx ? (double)Xx[base + k * 256 + tid] : 1.0);
        const unsigned off = (unsigned)(c[k] - c0);
        if (off < (unsigned)kRdColW) rd_atomic<KIND>(&sWin[off], t);
        else rd_atomic<KIND>(&acc[c[k]], t);
    }
    __syncthreads();
    for (int s = tid; s < kRdColW; s += 256) {
        const rd_u64 v = sWin[s];
        if (v != id && (long long)c0 + s < n) rd_atomic<KIND>(&acc[c0 + s], v);   // (a sum of +0 adds nothing)
    }
    rd_flag(bad, ctl);
}

// One partial a workgroup over `count` items: the values of X through the operator (Xp: the row pointer to validate), or
// RAW accumulators (the rows' results of an off-diagonal total).  gridDim.x is a function of count alone.
template <int KIND, bool RAW>
__global__ __launch_bounds__(256) void k_red_all(int m, int nnzX, const int* __restrict__ Xp, const value_t* __restrict__ Xx,
                                                 const rd_u64* __restrict__ raw, long long count, int op, rd_u64 id,
                                                 rd_u64* __restrict__ part, int* __restrict__ ctl)
{
    __shared__ rd_u64 sW[4];
    const int tid = threadIdx.x;
    if constexpr (!RAW) rd_flag(rd_rowptr_bad(m, nnzX, Xp, (long long)blockIdx.x * 256 + tid, (long long)gridDim.x * 256), ctl);
    long long per = (count + gridDim.x - 1) / gridDim.x;
    per = (per + 1023) / 1024 * 1024;
    const long long begin = (long long)blockIdx.x * per, end = min(count, begin + per);
    auto item = [&](long long i) -> rd_u64 {
        if constexpr (RAW) return raw[i];
        else return rd_term<KIND>(op, Xx ? (double)Xx[i] : 1.0);
    };
    rd_u64 v0 = id, v1 = id, v2 = id, v3 = id;                    // four chains a thread: loads in flight, the order still fixed
    long long i = begin + tid;
    for (; i + 768 < end; i += 1024) {
        v0 = rd_comb<KIND>(v0, item(i));
        v1 = rd_comb<KIND>(v1, item(i + 256));
        v2 = rd_comb<KIND>(v2, item(i + 512));
        v3 = rd_comb<KIND>(v3, item(i + 768));
    }
    for (; i < end; i += 256) v0 = rd_comb<KIND>(v0, item(i));
    rd_u64 v = rd_comb<KIND>(rd_comb<KIND>(v0, v1), rd_comb<KIND>(v2, v3));
    v = rd_block<KIND>(v, tid, sW);
    if (tid == 0) part[blockIdx.x] = v;
}

// nPart > 0: out[0] from the nPart partials of k_red_all (workgroup 0 alone); else out[i] from acc[i], i < nOut.  Nothing
// where the validation failed.
template <int KIND>
__global__ __launch_bounds__(256) void k_red_finish(int nOut, const rd_u64* __restrict__ acc, int nPart, rd_u64 id,
                                                    value_t* __restrict__ out, const int* __restrict__ ctl)
{
    __shared__ rd_u64 sW[4];
    if (ctl[RD_ERR]) return;
    const int tid = threadIdx.x;
    if (nPart > 0) {
        if (blockIdx.x) return;
        rd_u64 v = id;
        for (int i = tid; i < nPart; i += 256) v = rd_comb<KIND>(v, acc[i]);
        v = rd_block<KIND>(v, tid, sW);
        if (tid == 0) out[0] = rd_round<KIND>(v);
        return;
    }
    const long long t = (long long)blockIdx.x * 256 + tid;
    if (t < nOut) out[t] = rd_round<KIND>(acc[t]);
}

// ---------------------------------------------------------------- the scale
struct ScArgs {
    int m, n, nnzX;
    const int* Xp; const int* Xj;
    const value_t* Xx;                // (may be Zx: no __restrict__ on the two)
    const value_t* left; const value_t* right;
    double alpha;
    int leftDiv, rightDiv;
    value_t* Zx;
};

__global__ __launch_bounds__(256) void k_sc_check(int m, int nnzX, const int* __restrict__ Xp, int* __restrict__ ctl)
{
    rd_flag(rd_rowptr_bad(m, nnzX, Xp, (long long)blockIdx.x * 256 + threadIdx.x, (long long)gridDim.x * 256), ctl);
}

// entry q (below nnzX) whose left factor has been applied to the rule: t = double(x) (*|/) l (*|/) r * alpha, one rounding
__device__ __forceinline__ void sc_entry(const ScArgs& s, long long q, bool hasLeft, double l, bool& bad)
{
    double t = (double)s.Xx[q];
    if (hasLeft) t = s.leftDiv ? t / l : t * l;
    if (s.right) {
        const int c = s.Xj[q];
        if ((unsigned)c >= (unsigned)s.n) { bad = true; return; }  // (never an index; the entry stays as it is)
        const double r = (double)s.right[c];
        t = s.rightDiv ? t / r : t * r;
    }
    t = t * s.alpha;
    s.Zx[q] = (value_t)t;
}

__global__ __launch_bounds__(256) void k_sc_flat(ScArgs s, int* __restrict__ ctl)
{
    if (ctl[RD_ERR]) return;                                      // (k_sc_check refused the row pointer)
    const long long base = (long long)blockIdx.x * (256 * kScFlatE) + threadIdx.x;
    bool bad = false;
#pragma unroll
    for (int k = 0; k < kScFlatE; ++k) {
        const long long q = base + k * 256;
        if (q < s.nnzX) sc_entry(s, q, false, 0.0, bad);
    }
    rd_flag(bad, ctl);
}

__global__ __launch_bounds__(256) void k_sc_short(ScArgs s, int* __restrict__ ctl, int* __restrict__ queue)
{
    __shared__ int sLen[kRdRows];
    __shared__ int sCnt[2], sBase[2], sErr;
    const int tid = threadIdx.x, sl = tid & (kRdG - 1);
    if (tid == 0) sErr = ctl[RD_ERR];                             // (one read a workgroup: another one may raise the word for a bad column meanwhile)
    if (tid < 2) sCnt[tid] = 0;
    __syncthreads();
    if (sErr) return;                                             // (k_sc_check refused the row pointer)
    const int rowBase = blockIdx.x * kRdRows;
    bool bad = false;
    for (int it = 0; it < kRdRows / (256 / kRdG); ++it) {
        const int slot = it * (256 / kRdG) + tid / kRdG;
        const int r = rowBase + slot;
        int len = 0;
        if (r < s.m) {
            const int a = s.Xp[r];
            len = s.Xp[r + 1] - a;                                // (a valid row pointer: k_sc_check)
            if (len > 0 && len <= kRdShortL) {
                const double l = (double)s.left[r];
                for (int i = sl; i < len; i += kRdG) sc_entry(s, a + i, true, l, bad);
            }
        }
        if (sl == 0) sLen[slot] = len;
    }
    __syncthreads();
    rd_flag(bad, ctl);
    rd_enqueue(s.m, rowBase + tid, sLen[tid], sCnt, sBase, ctl, queue);
}

__global__ __launch_bounds__(256) void k_sc_wave(int nq, const int* __restrict__ queue, ScArgs s, int* __restrict__ ctl)
{
    const int lane = threadIdx.x & 63;
    const int qi = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (qi >= nq) return;
    const int r = queue[qi];
    if ((unsigned)r >= (unsigned)s.m) return;
    const int a = s.Xp[r], len = s.Xp[r + 1] - a;
    const double l = (double)s.left[r];
    bool bad = false;
    for (int i = lane; i < len; i += 64) sc_entry(s, a + i, true, l, bad);
    rd_flag(bad, ctl);
}

__global__ __launch_bounds__(256) void k_sc_long(int nq, const int* __restrict__ queue, ScArgs s, int* __restrict__ ctl)
{
    const int tid = threadIdx.x;
    bool bad = false;
    for (int qi = blockIdx.x; qi < nq; qi += gridDim.x) {
        const int r = queue[qi];
        if ((unsigned)r >= (unsigned)s.m) continue;
        const int a = s.Xp[r], len = s.Xp[r + 1] - a;
        const double l = (double)s.left[r];
        for (int i = tid; i < len; i += 256) sc_entry(s, a + i, true, l, bad);
    }
    rd_flag(bad, ctl);
}

}  // namespace bhs
