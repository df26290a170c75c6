// bhs_push_sr.hip.h -- sparse frontier x CSR over a semiring, in the push direction: for every listed row j of G, every
// entry (j, v) of it and every column c, Y(v, c) (+)= g (x) F(p, c) (bhs_csr_push_semiring_device; the contract is worded in
// include/bhsparse_hip.h, "sparse frontier x CSR").
//
// Work follows edges, not rows.  A frontier holds vertices of one out-edge next to hubs of 10^5, so nothing here gives a
// frontier vertex to a lane, a wave or a workgroup:
//
//   k_push_degrees   a thread per list position: fidx[p] is checked BEFORE it indexes the row pointer, the row's two bounds
//                    before anything is derived from them; deg[p] = the row's length, 0 for a position that is refused.
//                    The library's one-pass scan turns deg into offsets off[0 .. nf] (host: side_scan).
//   k_push_edges     the frontier's E = off[nf] entries cut into runs of consecutive ones, a run a wave, runs dealt round
//                    robin over the grid's waves.  A run is kPuRun (entry x column) pairs: kPuRun / T entries, T the power
//                    of two that holds k (64 at most; the kernel loops over wider k) -- four steps of a wave whatever k
//                    is, so a hub of 10^5 entries is 400 runs at k = 1 and 6250 at k = 16.  A wave finds the list positions
//                    of its run's first and last entry by a binary search in off (uniform), a lane the position of its own
//                    entry by one between the two.  Lane l holds column c0 + l % T and entry slot l / T of the run, so the
//                    T lanes of an entry touch T consecutive elements of F, M and Y.
//   k_push_count     a thread per 64 rows of Y: the number of bits in the row map's word, scanned like the degrees, for
//   k_push_compact   the same thread to write its word's rows at its offset: ascending, each once, the same from run to run.
//
// The update of an element is a compare-and-swap loop on its bits (pu_update): the element is read first, combined on the
// order-preserving keys of bhs_reduce.hip.h (which bring the NaN rule and -0 below +0 with them), rounded, and swapped in
// only where the rounded value has other bits than what is there -- most pushes improve nothing and write nothing.  A swap
// fails only because another lane's swap on the same element succeeded, and the loop takes that lane's value as its next
// `old`: every retry is somebody's progress, no loop waits for another workgroup.  min, max and or give the same bits in any
// order; every PLUS_PAIR product is 1, so the order of its adds cannot matter either.  The hardware's floating min / max
// atomics are not used: their NaN and zero ordering is not the contract's.
//
// A swap that changes the element AS A NUMBER test-and-sets the element's bit in a workspace bitmap and the row's bit in the
// row map; the lane that turned the element's bit on counts it.  All seven (+) move an element one way only, so an element
// differs from its value on entry exactly where one such swap happened: the count is exact and the same from run to run,
// and so is the row map.  Counts are summed per lane, wave, workgroup and added once per workgroup (smv_count).
//
// Every column is checked before it indexes M or Y; M is read before Y and an element it does not select is neither read
// nor written.  Rows of G that are not listed are not read at all.
#pragma once
#include "bhs_spmv_sr.hip.h"

namespace bhs {

constexpr int kPuRun = 256;           // (entry x column) pairs of a wave's run: 256 / T entries
constexpr int kPuRowMap = 8;          // beside kSmvCount in PuDims::flags: the row map is wanted
// control words: the reductions' four (RD_ERR), the 64-bit count of changed elements where smv_count adds it, then the words
// of the two scans (degrees -> offsets, row-map words -> places in d_next)
enum { PU_CHANGED = SMV_CHANGED, PU_TICKET_A = 8, PU_MAXCNT_A = 9, PU_TOTAL_A = 10 /* i64 */, PU_BINS_A = 12 /* kMaxBins */,
       PU_TICKET_B = 28, PU_MAXCNT_B = 29, PU_TOTAL_B = 30 /* i64 */, PU_BINS_B = 32 /* kMaxBins */, PU_INTS = 48 };
static_assert(PU_CHANGED == 4 && PU_BINS_A + kMaxBins <= PU_TICKET_B && PU_BINS_B + kMaxBins <= PU_INTS, "control block");

struct PuDims {
    int m, n, nnzG, nf, k;
    long long ldF, ldM, ldY;
    int mult, flags;                  // kSmv*; kSmvComplement | kSmvCount | kPuRowMap
    int tile;                         // T: a power of two, min(k, 64) <= T <= 64
};

// the bits of a value_t as the integer the swap works on
#ifdef BHS_VALUE_FLOAT
typedef unsigned int pu_bits_t;
#else
typedef unsigned long long pu_bits_t;
#endif
static_assert(sizeof(pu_bits_t) == sizeof(value_t), "the swap is as wide as a value");

__device__ __forceinline__ pu_bits_t pu_to_bits(value_t v)
{
    pu_bits_t b;
    __builtin_memcpy(&b, &v, sizeof(b));
    return b;
}

__device__ __forceinline__ value_t pu_to_value(pu_bits_t b)
{
    value_t v;
    __builtin_memcpy(&v, &b, sizeof(v));
    return v;
}

// Y(v, c) (+)= prod: 1 where this lane's swap changed the element as a number (several lanes can see that for one
// element: the bitmaps tell them apart), else 0.  prod: an accumulator of KIND (smv_prod).
template <int KIND>
__device__ __forceinline__ int pu_update(const PuDims& d, value_t* p, rd_u64 prod)
{
    pu_bits_t* pb = (pu_bits_t*)p;
    pu_bits_t old = *pb;
    int changed = 0;
    for (;;) {
        const value_t was = pu_to_value(old);
        double y = (double)was;
        if (d.mult == kSmvAnd) y = y != 0.0 ? 1.0 : 0.0;
        const value_t now = rd_round<KIND>(rd_comb<KIND>(smv_acc<KIND>(y), prod));
        const pu_bits_t nb = pu_to_bits(now);
        if (nb == old || (now != now && was != was)) break;         // nothing to improve (a NaN stays the NaN it is)
        const pu_bits_t seen = atomicCAS(pb, old, nb);
        if (seen == old) {
            changed = now == was ? 0 : 1;                           // (-0 to +0: other bits, the same number)
            break;
        }
        old = seen;                                                  // another lane's update went in: combine with that
    }
    return changed;
}

// the last position of off[lo .. hi] that starts at or before entry e (off[lo] <= e: the answer is in [lo, hi])
__device__ __forceinline__ int pu_position(const int* __restrict__ off, int lo, int hi, int e)
{
    while (lo < hi) {
        const int mid = lo + (hi - lo + 1) / 2;
        if (off[mid] <= e) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

__global__ __launch_bounds__(256) void k_push_degrees(PuDims d, const int* __restrict__ fidx, const int* __restrict__ Gp,
                                                      int* __restrict__ deg, int* __restrict__ ctl)
{
    const long long p = (long long)blockIdx.x * 256 + threadIdx.x;
    bool bad = false;
    if (p < d.nf) {
        int len = 0;
        const int j = fidx[p];
        if ((unsigned)j >= (unsigned)d.m) bad = true;               // (never an index)
        else {
            const int a = Gp[j], b = Gp[j + 1];
            if (rd_bounds_bad(a, b, d.nnzG)) bad = true;
            else len = b - a;
        }
        deg[p] = len;
    }
    rd_flag(bad, ctl);
}

// off: nf + 1 offsets (the scanned degrees); bits: the changed elements' bitmap (a bit per element of the n x k block, 32
// a word), rows: the row map (a bit per row of Y, 64 a word); either is touched only where d.flags asks for it
template <int KIND>
__global__ __launch_bounds__(256) void k_push_edges(PuDims d, const int* __restrict__ fidx, const int* __restrict__ off,
                                                    const int* __restrict__ Gp, const int* __restrict__ Gj,
                                                    const value_t* __restrict__ Gx, const value_t* __restrict__ F,
                                                    const value_t* __restrict__ M, value_t* Y, unsigned* __restrict__ bits,
                                                    rd_u64* __restrict__ rows, int* __restrict__ ctl)
{
    __shared__ rd_u64 sChg;
    const int lane = threadIdx.x & 63;
    const int T = d.tile, col = lane & (T - 1), slot = lane / T, step = 64 / T;
    if (threadIdx.x == 0) sChg = 0;
    __syncthreads();
    const long long total = *(const long long*)(ctl + PU_TOTAL_A);
    bool bad = total > 0x7fffffffLL;                                 // (the offsets are ints: refused, nothing is pushed)
    const int E = bad ? 0 : (int)total;
    const bool vals = d.mult != kSmvPair;
    rd_u64 nchg = 0;
    const long long nWaves = (long long)gridDim.x * 4;
    const int perRun = kPuRun / T;
    for (long long run = (long long)blockIdx.x * 4 + (threadIdx.x >> 6); run * perRun < E; run += nWaves) {   // (wave-uniform)
        const int e0 = (int)(run * perRun), e1 = min(E, e0 + perRun);
        const int pLo = pu_position(off, 0, d.nf - 1, e0), pHi = pu_position(off, pLo, d.nf - 1, e1 - 1);
        for (int e = e0 + slot; e < e1; e += step) {
            const int p = pu_position(off, pLo, pHi, e);
            const int j = fidx[p];                                   // (k_push_degrees: a row of G, its bounds in order)
            const int q = Gp[j] + (e - off[p]);
            const int v = Gj[q];
            if ((unsigned)v >= (unsigned)d.n) { bad = true; continue; }   // (never an index)
            const double g = (vals && Gx) ? (double)Gx[q] : 1.0;
            for (int c = col; c < d.k; c += T) {
                if (M) {
                    const value_t mv = M[(long long)v * d.ldM + c];
                    if ((mv != (value_t)0) == ((d.flags & kSmvComplement) != 0)) continue;   // not selected (NaN != 0: set)
                }
                const double f = vals ? (double)F[(long long)p * d.ldF + c] : 1.0;
                if (!pu_update<KIND>(d, Y + (long long)v * d.ldY + c, smv_prod<KIND>(d.mult, g, f))) continue;
                if (d.flags & kSmvCount) {
                    const unsigned long long at = (unsigned long long)v * (unsigned)d.k + (unsigned)c;
                    const unsigned bit = 1u << (at & 31);
                    if (!(atomicOr(bits + (at >> 5), bit) & bit)) ++nchg;
                }
                if (d.flags & kPuRowMap) (void)atomicOr(rows + (v >> 6), 1ull << (v & 63));
            }
        }
    }
    rd_flag(bad, ctl);
    if (d.flags & kSmvCount) smv_count(nchg, &sChg, ctl);             // (uniform: a kernel argument)
}

// cnt[w] = rows of word w of the row map (nWords of them)
__global__ __launch_bounds__(256) void k_push_count(int nWords, const rd_u64* __restrict__ rows, int* __restrict__ cnt)
{
    const long long w = (long long)blockIdx.x * 256 + threadIdx.x;
    if (w < nWords) cnt[w] = __popcll(rows[w]);
}

// next[at[w] ..] = the rows of word w, ascending (at: the scanned counts; no bit at or beyond row n is ever set)
__global__ __launch_bounds__(256) void k_push_compact(int nWords, const rd_u64* __restrict__ rows, const int* __restrict__ at,
                                                      int* __restrict__ next)
{
    const long long w = (long long)blockIdx.x * 256 + threadIdx.x;
    if (w >= nWords) return;
    rd_u64 b = rows[w];
    int o = at[w];
    while (b) {
        next[o++] = (int)(w * 64) + (__ffsll((long long)b) - 1);
        b &= b - 1;
    }
}

}  // namespace bhs
