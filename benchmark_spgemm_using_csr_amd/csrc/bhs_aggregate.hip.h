// bhs_aggregate.hip.h -- MIS(2) aggregation of the vertices of an n x n pattern S of strong connections
// (bhs_csr_aggregate_device; the contract is worded in include/bhsparse_hip.h, "aggregation").  Values are never taken:
// the same code, and the same result bit for bit, in the double and the float library.
//
// One 64-bit word a vertex: state << 62 | key, key = prio31 << 31 | index (distinct, so every tie is broken by index);
// state 1 undecided, 2 in (a root), 0 out.  The roots are the greedy distance-2 independent set in descending key order,
// found in synchronous rounds of two gathers, a kernel each:
//
//   k_agg_init     a thread per vertex: its key (the caller's priority or the hash), its word as undecided, its row's two
//                  bounds checked.
//   k_agg_near     t1[i] = the greatest word over i and N(i).
//   k_agg_decide   for an undecided i: t2 = the greatest t1 over i and N(i), the greatest word within two steps.  t2 is i's
//                  own word: i is in.  t2's state is in: a root lies within two steps, i is out.  Else i stays.  A decided
//                  row reads nothing of its row.  The vertices that stay are counted lane -> wave -> workgroup -> one add
//                  (smv_count) for the host, which reads the count once a round and ends the loop; no kernel spins or
//                  waits for another workgroup.  The grid is bounded and a workgroup walks several blocks of rows, so the
//                  adds to the one count word are a few thousand a launch: with a workgroup per 256 / L rows they were
//                  131 k on poisson27pt 128^3 and the kernel took three times the first gather's time.
//   k_agg_count    a wave per 64 vertices: the roots among them as a bitmap word and its count; the library's one-pass
//                  scan over the counts gives every word its first number (host: side_scan), as k_push_count does.
//   k_agg_number   a thread per word: its roots numbered ascending; agg1[root] = its number, d_roots[number] = root.
//   k_agg_join<1>  pass 1, every other vertex: the root of greatest key in N(i) gives agg1[i], -1 without one.
//   k_agg_join<2>  pass 2: agg[i] = agg1[i] where pass 1 or the numbering placed i, else agg1 of the placed member of N(i)
//                  of greatest key.  Pass 2 reads agg1 and writes agg, never the array it reads: no result depends on timing.
//
// The three gathers (near, decide, join) spread a row over L = 1, 4, 16 or 64 lanes, chosen on the host from the pattern's
// mean row length; a row longer than L loops and the L lanes' maxima meet in a DPP reduction of the two 32-bit halves
// (lane_xor64), which every lane of the wave reaches: no thread returns early, a row beyond n or one that has nothing to
// do has an empty range.  Results are written by the one lane that owns the row -- no atomics on results, no LDS beyond the
// count's one word, no scratch.
//
// Validation on the device, ahead of each dependent read: a row's bounds are checked wherever they are read and a row that
// fails is taken as empty; a column is checked before it indexes anything and skipped where it fails; either raises
// ctl[RD_ERR], which the host reads with the first round's count.
#pragma once
#include "bhs_spmv_sr.hip.h"

namespace bhs {

// control words: the reductions' four (RD_ERR), the 64-bit count of undecided vertices where smv_count adds it, the scan's
enum { AG_UNDEC = SMV_CHANGED, AG_TICKET = 8, AG_MAXCNT = 9, AG_TOTAL = 10 /* i64 */, AG_BINS = 12 /* kMaxBins */, AG_INTS = 28 };
static_assert(AG_UNDEC == 4 && AG_BINS + kMaxBins <= AG_INTS, "control block");

constexpr rd_u64 kAgKeyMask = (1ull << 62) - 1ull;
constexpr rd_u64 kAgUndecided = 1ull << 62, kAgIn = 2ull << 62;
constexpr rd_u64 kAgValid = 1ull << 63;       // a candidate of the join passes: kAgValid | key (0: none)

struct AgDims {
    int n, nnzS;
    unsigned seed;
    int hasPrio;
};

__device__ __forceinline__ unsigned ag_hash(unsigned i, unsigned seed)
{
    unsigned h = (i ^ seed) + 0x9e3779b9u;
    h ^= h >> 16; h *= 0x85ebca6bu;
    h ^= h >> 13; h *= 0xc2b2ae35u;
    h ^= h >> 16;
    return h;
}

// the maximum of v over the L lanes that share a row (L consecutive lanes, L a power of two); every lane of the wave comes here
template <int L>
__device__ __forceinline__ rd_u64 ag_lanes_max(rd_u64 v, int lane)
{
    if constexpr (L > 1) v = max(v, lane_xor64<1>(v, lane));
    if constexpr (L > 2) v = max(v, lane_xor64<2>(v, lane));
    if constexpr (L > 4) v = max(v, lane_xor64<4>(v, lane));
    if constexpr (L > 8) v = max(v, lane_xor64<8>(v, lane));
    if constexpr (L > 16) v = max(v, lane_xor64<16>(v, lane));
    if constexpr (L > 32) v = max(v, lane_xor64<32>(v, lane));
    return v;
}

// the row of this thread's group of L lanes (n and beyond: no row), and its checked range [a, b) -- empty where the row
// pointer is refused (bad is raised) or there is no row
template <int L>
__device__ __forceinline__ long long ag_row(const AgDims& d, const int* __restrict__ Sp, long long block, int& a, int& b, bool& bad)
{
    const long long i = block * (256 / L) + threadIdx.x / L;
    a = b = 0;
    if (i < d.n) {
        const int lo = Sp[i], hi = Sp[i + 1];
        if (rd_bounds_bad(lo, hi, d.nnzS)) bad = true;
        else { a = lo; b = hi; }
    }
    return i;
}

__global__ __launch_bounds__(256) void k_agg_init(AgDims d, const int* __restrict__ Sp, const unsigned* __restrict__ prio,
                                                  rd_u64* __restrict__ w, int* __restrict__ ctl)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    bool bad = false;
    if (i < d.n) {
        const unsigned p = d.hasPrio ? prio[i] : ag_hash((unsigned)i, d.seed);
        w[i] = kAgUndecided | ((rd_u64)(p >> 1) << 31) | (rd_u64)i;
        bad = rd_bounds_bad(Sp[i], Sp[i + 1], d.nnzS);
    }
    rd_flag(bad, ctl);
}

template <int L>
__global__ __launch_bounds__(256) void k_agg_near(AgDims d, const int* __restrict__ Sp, const int* __restrict__ Sj,
                                                  const rd_u64* __restrict__ w, rd_u64* __restrict__ t1, int* __restrict__ ctl)
{
    const int lane = threadIdx.x & 63, sub = threadIdx.x & (L - 1);
    bool bad = false;
    int a, b;
    const long long i = ag_row<L>(d, Sp, blockIdx.x, a, b, bad);
    rd_u64 v = 0;
    for (int q = a + sub; q < b; q += L) {
        const int j = Sj[q];
        if ((unsigned)j >= (unsigned)d.n) { bad = true; continue; }   // (never an index)
        v = max(v, w[j]);
    }
    v = ag_lanes_max<L>(v, lane);
    if (i < d.n && sub == 0) t1[i] = max(v, w[i]);
    rd_flag(bad, ctl);
}

template <int L>
__global__ __launch_bounds__(256) void k_agg_decide(AgDims d, const int* __restrict__ Sp, const int* __restrict__ Sj,
                                                    const rd_u64* __restrict__ t1, rd_u64* __restrict__ w, int* __restrict__ ctl)
{
    __shared__ rd_u64 sLeft;
    const int lane = threadIdx.x & 63, sub = threadIdx.x & (L - 1);
    if (threadIdx.x == 0) sLeft = 0;
    __syncthreads();
    bool bad = false;
    rd_u64 left = 0;
    const long long nBlocks = ((long long)d.n + 256 / L - 1) / (256 / L);
    for (long long block = blockIdx.x; block < nBlocks; block += gridDim.x) {   // (uniform in the workgroup: every lane reaches the reduction)
        int a, b;
        const long long i = ag_row<L>(d, Sp, block, a, b, bad);
        const rd_u64 mine = i < d.n ? w[i] : 0;
        const bool open = (mine >> 62) == 1;
        if (!open) a = b = 0;                                        // decided: nothing of the row is read
        rd_u64 v = 0;
        for (int q = a + sub; q < b; q += L) {
            const int j = Sj[q];
            if ((unsigned)j >= (unsigned)d.n) { bad = true; continue; }   // (never an index)
            v = max(v, t1[j]);
        }
        v = ag_lanes_max<L>(v, lane);
        if (open && sub == 0) {
            v = max(v, t1[i]);
            if (v == mine) w[i] = kAgIn | (mine & kAgKeyMask);
            else if ((v >> 62) == 2) w[i] = mine & kAgKeyMask;
            else ++left;
        }
    }
    rd_flag(bad, ctl);
    smv_count(left, &sLeft, ctl);
}

// map[g] = the roots among vertices 64 g .. 64 g + 63 as bits, cnt[g] their number (a wave per word)
__global__ __launch_bounds__(256) void k_agg_count(int n, const rd_u64* __restrict__ w, rd_u64* __restrict__ map,
                                                   int* __restrict__ cnt)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    const bool root = i < n && (w[i] >> 62) == 2;
    const rd_u64 bits = __ballot(root);
    if ((threadIdx.x & 63) == 0 && (i >> 6) < (((long long)n + 63) >> 6)) {
        map[i >> 6] = bits;
        cnt[i >> 6] = __popcll(bits);
    }
}

// the roots of word g numbered from at[g] on, ascending: agg1[root] = number, roots[number] = root (roots may be null)
__global__ __launch_bounds__(256) void k_agg_number(int nWords, const rd_u64* __restrict__ map, const int* __restrict__ at,
                                                    int* __restrict__ agg1, int* __restrict__ roots)
{
    const long long g = (long long)blockIdx.x * 256 + threadIdx.x;
    if (g >= nWords) return;
    rd_u64 bits = map[g];
    int o = at[g];
    while (bits) {
        const int v = (int)(g * 64) + (__ffsll((long long)bits) - 1);
        agg1[v] = o;
        if (roots) roots[o] = v;
        ++o;
        bits &= bits - 1;
    }
}

// PASS 1: from = agg1 (read at roots only, which this kernel does not write), to = agg1 (written at the others).
// PASS 2: from = agg1 (read only), to = the caller's agg.
template <int L, int PASS>
__global__ __launch_bounds__(256) void k_agg_join(AgDims d, const int* __restrict__ Sp, const int* __restrict__ Sj,
                                                  const rd_u64* __restrict__ w, const int* from, int* to, int* __restrict__ ctl)
{
    const int lane = threadIdx.x & 63, sub = threadIdx.x & (L - 1);
    bool bad = false;
    int a, b;
    const long long i = ag_row<L>(d, Sp, blockIdx.x, a, b, bad);
    bool placed = false;
    if (i < d.n) placed = PASS == 1 ? (w[i] >> 62) == 2 : from[i] >= 0;
    if (placed) a = b = 0;
    rd_u64 v = 0;
    for (int q = a + sub; q < b; q += L) {
        const int j = Sj[q];
        if ((unsigned)j >= (unsigned)d.n) { bad = true; continue; }   // (never an index)
        const rd_u64 wj = w[j];
        const bool cand = PASS == 1 ? (wj >> 62) == 2 : from[j] >= 0;
        if (cand) v = max(v, kAgValid | (wj & kAgKeyMask));
    }
    v = ag_lanes_max<L>(v, lane);
    if (i < d.n && sub == 0) {
        if (PASS == 1) {
            if (!placed) to[i] = v ? from[(int)(v & 0x7fffffffull)] : -1;
        } else {
            to[i] = placed ? from[i] : v ? from[(int)(v & 0x7fffffffull)] : 0;   // (a vertex always has a placed neighbour: see the header)
        }
    }
    rd_flag(bad, ctl);
}

}  // namespace bhs
