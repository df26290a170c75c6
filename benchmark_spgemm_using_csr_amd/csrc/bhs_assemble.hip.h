// bhs_assemble.hip.h -- a CSR matrix from triplets (bhs_coo_assemble_device, bhs_coo_assemble_values_device; the contract is
// worded in include/bhsparse_hip.h, "assembly").  Z's entry q is a run of equal (row, column) in the stable order of the kept
// triplets -- sorted by (row, column, position) -- and its value the run's first, last or sequentially added values.  No atomic
// touches an output array and the result does not depend on scheduling: atomics hand out places in a scratch array of keys,
// every raw row's keys are put in order there, and everything caller-owned is written by index from scanned counts.
//
//   k_as_count     a lane a triplet: validity (an index >= m or >= n, or a negative one without BHS_COO_IGNORE_NEGATIVE,
//                  raises the error word), the number of dropped triplets, the histogram of the kept ones' rows into m
//                  counters -- one atomic a wave where its kept triplets share a row, one a triplet otherwise (as_take).
//   k_tr_bin       the transpose's: the raw rows' bins by length.  The library's one-pass scan makes rawPtr of the counts.
//   k_as_scatter   the same mapping; places from cursors (a copy of rawPtr).  A place is compared with its row's range BEFORE
//                  the store: outside it the error word is raised and nothing is stored (the caller may have changed the
//                  triplets since k_as_count).  What is stored: the key (column << 32) | position, and the row beside it.
//   k_as_sort_*    a raw row's keys ascending, in place -- the transpose's three shapes: up to 32 keys by rank over 16 lanes,
//                  up to 1024 with wave_bitonic_sort, beyond by a workgroup's flip network (as_flip_sort), in LDS up to 4096
//                  keys and in the scratch array itself past that.  Keys are distinct (the positions are), so any correct
//                  sort gives the same array.  A row whose keys arrived in order is left alone.
//   k_as_flag      flat over the sorted array: element i heads a run where its row or its column differs from element i - 1's
//                  (BHS_COO_KEEP: everywhere); a wave per 64 elements writes a bitmap word and its popcount, the one-pass
//                  scan numbers the heads as the components number their roots.
//   k_as_emit      perm[i], and from the heads entryPtr[q] and colIndZ[q]; k_as_rowptr: rowPtrZ[r] = the heads below rawPtr[r].
//   k_as_values    a lane an entry walks its run in order, in double, and rounds once.  The values call launches it on the
//                  caller's map after k_as_check_map has read all of it: a refusal writes nothing.
//
// Nothing spins, nothing waits for another workgroup; every lane of a wave reaches every ballot and shuffle.  Every index
// that addresses memory is validated in the same kernel ahead of the access or comes from scanned counts of validated data,
// and is compared with its array's size all the same.
#pragma once
#include "bhs_transpose.hip.h"

namespace bhs {

enum { kAsSum = 0, kAsFirst = 1, kAsLast = 2, kAsKeep = 3, kAsMode = 3, kAsIgnoreNeg = 4 };   // BHS_COO_*

// control words: the raw rows per bin and the error word where the transpose keeps its own (k_tr_bin is launched on this
// block), then the words of two scans -- the raw rows', the bitmap words' -- and the dropped triplets
enum { AS_COUNT = TR_COUNT, AS_ERR = TR_ERR, AS_TICKET_A = 8, AS_MAXCNT_A = 9, AS_TOTAL_A = 10 /* i64 */,
       AS_BINS_A = 12 /* kMaxBins */, AS_TICKET_B = 28, AS_MAXCNT_B = 29, AS_TOTAL_B = 30 /* i64 */, AS_BINS_B = 32 /* kMaxBins */,
       AS_DROPPED = 48 /* kAsDropSlots: the triplets dropped for a negative index, a workgroup adds to slot blockIdx % 16 */,
       AS_INTS = 64 };
constexpr int kAsDropSlots = 16;
static_assert(AS_COUNT + kTrBins <= AS_ERR && AS_BINS_A + kMaxBins <= AS_TICKET_B && AS_BINS_B + kMaxBins <= AS_DROPPED &&
              AS_DROPPED + kAsDropSlots <= AS_INTS, "control block");
enum { kAsBadArg = 1, kAsBroken = 2 };                                // bits of the error word: the caller's input; a place or index of our own

__device__ __forceinline__ void as_flag(bool bad, int bit, int* __restrict__ ctl)
{
    if (__ballot(bad) != 0ull && (threadIdx.x & 63) == 0) (void)atomicOr(ctl + AS_ERR, bit);
}

// is triplet (r, c) kept; *bad where it is an error
__device__ __forceinline__ bool as_kept(int r, int c, int m, int n, int flags, bool* bad)
{
    if (r >= m || c >= n) { *bad = true; return false; }              // (with or without the flag)
    if (r < 0 || c < 0) { *bad = (flags & kAsIgnoreNeg) == 0; return false; }
    return true;
}

// cur[r] += 1 for every lane with keep, r validated: the value before.  Where the kept lanes of the wave share one row -- the
// input came sorted, or is one long run -- the first of them adds their number once.  Every lane of the wave calls this.
__device__ __forceinline__ int as_take(bool keep, int r, int lane, int* __restrict__ cur)
{
    const tr_u64 act = __ballot(keep);
    if (act == 0ull) return 0;                                        // (wave-uniform)
    const int first = __ffsll((long long)act) - 1;
    const int r0 = __shfl(r, first);
    const bool uni = __ballot(keep && r != r0) == 0ull;
    int at = 0;
    if (uni) {
        int base = 0;
        if (lane == first) base = atomicAdd(&cur[r0], __popcll(act));
        base = __shfl(base, first);
        at = base + __popcll(act & ((1ull << lane) - 1ull));
    } else if (keep) {
        at = atomicAdd(&cur[r], 1);
    }
    return at;
}

__global__ __launch_bounds__(256) void k_as_count(int m, int n, int nnzIn, const int* __restrict__ rows, const int* __restrict__ cols,
                                                  int flags, int* __restrict__ cnt, int* __restrict__ ctl)
{
    __shared__ int sDrop;
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    const int lane = threadIdx.x & 63;
    if (threadIdx.x == 0) sDrop = 0;
    __syncthreads();
    bool bad = false, keep = false;
    int r = 0;
    if (e < nnzIn) {
        r = rows[e];
        keep = as_kept(r, cols[e], m, n, flags, &bad);
    }
    (void)as_take(keep, r, lane, cnt);
    // the kept triplets are all but the dropped ones: nothing is added where nothing is dropped -- one word for every wave
    // of 56 M triplets took 10 of the call's 16 ms
    const tr_u64 drop = __ballot(e < nnzIn && !keep && !bad);
    if (lane == 0 && drop) (void)atomicAdd(&sDrop, __popcll(drop));
    as_flag(bad, kAsBadArg, ctl);
    __syncthreads();
    if (threadIdx.x == 0 && sDrop) (void)atomicAdd(ctl + AS_DROPPED + (blockIdx.x & (kAsDropSlots - 1)), sDrop);
}

// rawPtr: the scanned counts; cur: a copy of it, the next free place of every raw row
__global__ __launch_bounds__(256) void k_as_scatter(int m, int n, int nnzIn, const int* __restrict__ rows, const int* __restrict__ cols,
                                                    int flags, const int* __restrict__ rawPtr, int* __restrict__ cur,
                                                    tr_u64* __restrict__ keys, int* __restrict__ rowOf, int* __restrict__ ctl)
{
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    const int lane = threadIdx.x & 63;
    bool bad = false, keep = false, broken = false;
    int r = 0, c = 0;
    if (e < nnzIn) {
        r = rows[e];
        c = cols[e];
        keep = as_kept(r, c, m, n, flags, &bad);
    }
    const int at = as_take(keep, r, lane, cur);
    if (keep) {
        const int beg = rawPtr[r], end = rawPtr[r + 1];               // (0 <= r < m)
        if (at < beg || at >= end || (unsigned)at >= (unsigned)nnzIn) broken = true;   // (the triplets are not those that were counted)
        else {
            keys[at] = ((tr_u64)(unsigned)c << 32) | (tr_u64)(unsigned)e;
            rowOf[at] = r;
        }
    }
    as_flag(broken, kAsBroken, ctl);
}

// raw row `row` of the queue: where its keys start and how many there are (0 for anything the scan cannot have made)
__device__ __forceinline__ void as_row_range(const int* __restrict__ rawPtr, int row, int nkept, int* t0, int* len)
{
    const int a = rawPtr[row], b = rawPtr[row + 1];
    const bool ok = a >= 0 && b >= a && b <= nkept;
    *t0 = ok ? a : 0;
    *len = ok ? b - a : 0;
}

__global__ __launch_bounds__(256) void k_as_sort_short(int nq, const int* __restrict__ queue, const int* __restrict__ rawPtr, int nkept,
                                                       tr_u64* keys)
{
    const int tid = threadIdx.x, g = tid / 16, lane = tid & 15;
    const long long qi = (long long)blockIdx.x * 16 + g;
    int t0 = 0, len = 0;
    if (qi < nq) {
        as_row_range(rawPtr, queue[qi], nkept, &t0, &len);
        if (len > kTrShortL) len = 0;                                 // (the binning keeps such rows out)
    }
    // keys are distinct: a key's place in its row is the number of keys below it (the padding is below none)
    tr_u64 key[2] = {~0ull, ~0ull};
#pragma unroll
    for (int e = 0; e < 2; ++e)
        if (e * 16 + lane < len) key[e] = keys[(size_t)t0 + e * 16 + lane];
    int r0 = 0, r1 = 0;
    for (int j = 0; j < 16; ++j) {
        const tr_u64 a = __shfl(key[0], j, 16), b = __shfl(key[1], j, 16);
        r0 += (a < key[0] ? 1 : 0) + (b < key[0] ? 1 : 0);
        r1 += (a < key[1] ? 1 : 0) + (b < key[1] ? 1 : 0);
    }
    if (lane < len && r0 < len) keys[(size_t)t0 + r0] = key[0];
    if (16 + lane < len && r1 < len) keys[(size_t)t0 + r1] = key[1];
}

template <int E>
__device__ __forceinline__ void as_sort_row_wave(tr_u64* g, int len, int lane)
{
    tr_u64 x[E];
#pragma unroll
    for (int e = 0; e < E; ++e) {
        const int i = lane * E + e;
        x[e] = i < len ? g[i] : ~0ull;
    }
    wave_bitonic_sort<tr_u64, E>(x, lane);
#pragma unroll
    for (int e = 0; e < E; ++e) {
        const int i = lane * E + e;
        if (i < len) g[i] = x[e];
    }
}

__global__ __launch_bounds__(256) void k_as_sort_wave(int nq, const int* __restrict__ queue, const int* __restrict__ rawPtr, int nkept,
                                                      tr_u64* keys)
{
    const int lane = threadIdx.x & 63;
    const long long qi = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (qi >= nq) return;                                             // (wave-uniform)
    int t0, len;
    as_row_range(rawPtr, queue[qi], nkept, &t0, &len);
    tr_u64* g = keys + t0;
    bool bad = false;
    for (int i = lane; i + 1 < len; i += 64) bad |= g[i] > g[i + 1];
    if (!__any(bad)) return;                                          // arrived in order (wave-uniform)
    if (len <= 64) as_sort_row_wave<1>(g, len, lane);
    else if (len <= 128) as_sort_row_wave<2>(g, len, lane);
    else if (len <= 256) as_sort_row_wave<4>(g, len, lane);
    else if (len <= 512) as_sort_row_wave<8>(g, len, lane);
    else if (len <= kTrWaveL) as_sort_row_wave<16>(g, len, lane);
}

// buf[0 .. len) ascending by a workgroup of 256: the flip network of k_tr_fill_long (a flip of every block of k with its mirror
// image, then half-cleaners), on LDS or on global memory -- every step ends at a barrier
__device__ __forceinline__ void as_flip_sort(tr_u64* buf, int len, int tid)
{
    int P = 1;
    while (P < len) P <<= 1;
    auto cmpx = [&](int a, int b) {
        const tr_u64 x = buf[a], y = buf[b];
        if (x > y) { buf[a] = y; buf[b] = x; }
    };
    for (int k = 2; k <= P; k <<= 1) {
        const int hk = k >> 1;
        for (int i = tid; i < (P >> 1); i += 256) {
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

// a workgroup a raw row, the rows of the queue in turn
__global__ __launch_bounds__(256) void k_as_sort_long(int nq, const int* __restrict__ queue, const int* __restrict__ rawPtr, int nkept,
                                                      tr_u64* keys)
{
    __shared__ tr_u64 ldsK[kTrLdsMax];
    const int tid = threadIdx.x;
    for (int qi = blockIdx.x; qi < nq; qi += gridDim.x) {             // (uniform in the workgroup)
        int t0, len;
        as_row_range(rawPtr, queue[qi], nkept, &t0, &len);
        tr_u64* g = keys + t0;
        bool bad = false;
        for (int i = tid; i + 1 < len; i += 256) bad |= g[i] > g[i + 1];
        if (__syncthreads_or(bad ? 1 : 0)) {
            if (len <= kTrLdsMax) {
                for (int i = tid; i < len; i += 256) ldsK[i] = g[i];
                __syncthreads();
                as_flip_sort(ldsK, len, tid);
                for (int i = tid; i < len; i += 256) g[i] = ldsK[i];
            } else {
                as_flip_sort(g, len, tid);
            }
        }
        __syncthreads();                                              // (ldsK is the next row's)
    }
}

// map[w] = the heads among elements 64 w .. 64 w + 63 as bits, cnt[w] their number (a wave per word)
__global__ __launch_bounds__(256) void k_as_flag(int nkept, const tr_u64* __restrict__ keys, const int* __restrict__ rowOf, int keepAll,
                                                 tr_u64* __restrict__ map, int* __restrict__ cnt)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    bool head = false;
    if (i < nkept)
        head = keepAll || i == 0 || rowOf[i] != rowOf[i - 1] || (unsigned)(keys[i] >> 32) != (unsigned)(keys[i - 1] >> 32);
    const tr_u64 bits = __ballot(head);
    if ((threadIdx.x & 63) == 0 && (i >> 6) < (((long long)nkept + 63) >> 6)) {
        map[i >> 6] = bits;
        cnt[i >> 6] = __popcll(bits);
    }
}

// element i of the sorted array belongs to entry q = (the heads at or below i) - 1: perm[i]; from a head entryPtr[q] and
// colIndZ[q]; from the last element entryPtr[nnzZ] = nkept.  off: the scanned counts of k_as_flag.
__global__ __launch_bounds__(256) void k_as_emit(int nkept, const tr_u64* __restrict__ keys, const tr_u64* __restrict__ map,
                                                 const int* __restrict__ off, int* __restrict__ Zj, int* __restrict__ entryPtr,
                                                 int* __restrict__ perm, int* __restrict__ ctl)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= nkept) return;                                           // (no cross-lane step below)
    const tr_u64 w = map[i >> 6];
    const int b = (int)(i & 63);
    const int q = off[i >> 6] + __popcll(w & ((2ull << b) - 1ull)) - 1;
    if ((unsigned)q >= (unsigned)nkept) { (void)atomicOr(ctl + AS_ERR, kAsBroken); return; }   // (never: i = 0 is a head, heads <= nkept)
    const tr_u64 key = keys[i];
    if (perm) perm[i] = (int)(unsigned)key;
    if ((w >> b) & 1ull) {
        Zj[q] = (int)(key >> 32);
        if (entryPtr) entryPtr[q] = (int)i;
    }
    if (i == (long long)nkept - 1 && entryPtr) entryPtr[q + 1] = nkept;
}

// rowPtrZ[r] = the heads below rawPtr[r], r = 0 .. m
__global__ __launch_bounds__(256) void k_as_rowptr(int m, int nkept, const int* __restrict__ rawPtr, const tr_u64* __restrict__ map,
                                                   const int* __restrict__ off, int* __restrict__ Zp, int* __restrict__ ctl)
{
    const long long r = (long long)blockIdx.x * 256 + threadIdx.x;
    if (r > m) return;
    const int p = rawPtr[r];
    if (p < 0 || p > nkept) { (void)atomicOr(ctl + AS_ERR, kAsBroken); return; }
    const int nWords = (int)(((long long)nkept + 63) >> 6), w = p >> 6;
    Zp[r] = w >= nWords ? off[nWords] : off[w] + __popcll(map[w] & ((1ull << (p & 63)) - 1ull));
}

// The caller's map, all of it, ahead of k_as_values: entryPtr[0] = 0, entryPtr ascending (equal neighbours: an empty run),
// entryPtr[nnzZ] <= nnzIn, perm[k] in [0, nnzIn) for k < entryPtr[nnzZ].  Lane k looks at entryPtr[k] and perm[k].
__global__ __launch_bounds__(256) void k_as_check_map(int nnzZ, int nnzIn, const int* __restrict__ entryPtr, const int* __restrict__ perm,
                                                      int* __restrict__ ctl)
{
    const long long k = (long long)blockIdx.x * 256 + threadIdx.x;
    bool bad = false;
    if (k == 0 && entryPtr[0] != 0) bad = true;
    if (k < nnzZ && entryPtr[k] > entryPtr[k + 1]) bad = true;
    const int nk = entryPtr[nnzZ];
    if (nk < 0 || nk > nnzIn) bad = true;                             // (perm is then not read)
    else if (k < nk && (unsigned)perm[k] >= (unsigned)nnzIn) bad = true;
    as_flag(bad, kAsBadArg, ctl);
}

// valZ[q] from the run perm[entryPtr[q] .. entryPtr[q + 1]): the first, the last, or s = double(first), s += double(next) in
// order, one rounding.  The positions come from `keys` (the full call: their low halves) or from `perm`.  total (the full
// call): the scan's count of entries, read here.  limit: what entryPtr may reach.  Every index is compared before it is
// followed; a bad one raises `bit`, and the entry is not written.
__global__ __launch_bounds__(256) void k_as_values(int nnzZ, const long long* __restrict__ total, int limit, int nnzIn,
                                                   const int* __restrict__ entryPtr, const int* __restrict__ perm,
                                                   const tr_u64* __restrict__ keys, const value_t* __restrict__ valIn, int mode,
                                                   int bit, value_t* __restrict__ valZ, int* __restrict__ ctl)
{
    const long long q = (long long)blockIdx.x * 256 + threadIdx.x;
    long long nz = nnzZ;
    if (total) nz = min(nz, *total);
    bool bad = false;
    if (q < nz) {
        const int a = entryPtr[q], b = entryPtr[q + 1];
        auto pos = [&](int k) -> unsigned { return keys ? (unsigned)keys[k] : (unsigned)perm[k]; };
        if (a < 0 || b < a || b > limit) bad = true;
        else if (a == b) valZ[q] = (value_t)0;                        // (an empty run: only a caller's map has one)
        else if (mode != kAsSum) {
            const unsigned e = pos(mode == kAsFirst ? a : b - 1);
            if (e >= (unsigned)nnzIn) bad = true;
            else valZ[q] = valIn[e];
        } else {
            double s = 0.0;
            for (int k = a; k < b && !bad; k += 8) {                  // eight loads in flight, added in order
                double v[8];
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    v[j] = 0.0;
                    if (k + j < b) {
                        const unsigned e = pos(k + j);
                        if (e >= (unsigned)nnzIn) bad = true;
                        else v[j] = (double)valIn[e];
                    }
                }
#pragma unroll
                for (int j = 0; j < 8; ++j)
                    if (k + j < b) s = (k + j == a) ? v[j] : s + v[j];
            }
            if (!bad) valZ[q] = (value_t)s;
        }
    }
    as_flag(bad, bit, ctl);
}

}  // namespace bhs
