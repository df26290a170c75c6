// bhs_color.hip.h -- greedy colouring of the vertices of an n x n pattern S (bhs_csr_color_device; the contract is worded in
// include/bhsparse_hip.h, "colouring and relaxation").  Values are never taken: the same code, and the same result bit for
// bit, in the double and the float library.
//
// The key of a vertex is the aggregation's, prio31 << 31 | index (bhs_aggregate.hip.h), made where it is needed from the
// caller's priority or the hash: nothing is kept per vertex but its colour, -1 while it has none.  The colouring is the
// first-fit greedy one in descending key order, found in synchronous rounds of one kernel:
//
//   k_col_round    an uncoloured i whose key exceeds that of every uncoloured off-diagonal neighbour takes the smallest
//                  colour no neighbour holds; every other vertex keeps what it has.  A round reads one colour array and
//                  writes the other, never the one it reads.  The free colour comes from a 64-bit mask of the neighbours'
//                  colours inside a window of 64 colours, OR-reduced over the row's L lanes (lane_xor64); a row whose
//                  window is full walks its row again with the next window, and the wave goes round until none of its
//                  rows has to -- a row of degree g at most g / 64 + 1 times.  The vertices left uncoloured are counted as
//                  k_agg_decide counts (smv_count), the colours in use go to one word by a maximum a workgroup; the host
//                  reads both once a round.  No kernel spins or waits for another workgroup.
//   k_col_count    a wave per 64 vertices: how many of them hold each colour, to cnt[colour * words + word] -- colour-major,
//                  so that the library's one-pass scan (host: side_scan) over the table gives every (colour, word) its
//                  place in the order and every colour its first place.
//   k_col_number   the same wave: a vertex goes to the place of its (colour, word) plus the vertices of its colour below it
//                  in the wave.  The first ncolors + 1 threads copy the colours' first places to colorPtr.
//
// Both find the lanes of a wave that share a colour by going through the colours present, a ballot each (co_same): no
// histogram in LDS, no atomics on results.  Results are written by the one lane that owns the vertex.
//
// Validation as in the aggregation, ahead of each dependent read: a row's bounds wherever they are read (a row that fails is
// taken as empty), a column before it indexes anything (skipped where it fails); either raises ctl[RD_ERR].
#pragma once
#include "bhs_aggregate.hip.h"

namespace bhs {

// control words: the aggregation's (the error word, the count of uncoloured vertices, the scan's), then the colours in use
enum { CO_NCOL = AG_INTS, CO_INTS = AG_INTS + 4 };

__device__ __forceinline__ rd_u64 co_key(const AgDims& d, const unsigned* __restrict__ prio, int i)
{
    const unsigned p = d.hasPrio ? prio[i] : ag_hash((unsigned)i, d.seed);
    return ((rd_u64)(p >> 1) << 31) | (rd_u64)i;
}

// the OR of v over the L lanes that share a row; every lane of the wave comes here
template <int L>
__device__ __forceinline__ rd_u64 co_lanes_or(rd_u64 v, int lane)
{
    if constexpr (L > 1) v |= lane_xor64<1>(v, lane);
    if constexpr (L > 2) v |= lane_xor64<2>(v, lane);
    if constexpr (L > 4) v |= lane_xor64<4>(v, lane);
    if constexpr (L > 8) v |= lane_xor64<8>(v, lane);
    if constexpr (L > 16) v |= lane_xor64<16>(v, lane);
    if constexpr (L > 32) v |= lane_xor64<32>(v, lane);
    return v;
}

template <int L>
__device__ __forceinline__ unsigned co_lanes_or32(unsigned v, int lane)
{
    if constexpr (L > 1) v |= lane_xor<1>(v, lane);
    if constexpr (L > 2) v |= lane_xor<2>(v, lane);
    if constexpr (L > 4) v |= lane_xor<4>(v, lane);
    if constexpr (L > 8) v |= lane_xor<8>(v, lane);
    if constexpr (L > 16) v |= lane_xor<16>(v, lane);
    if constexpr (L > 32) v |= lane_xor<32>(v, lane);
    return v;
}

template <int L>
__global__ __launch_bounds__(256) void k_col_round(AgDims d, const int* __restrict__ Sp, const int* __restrict__ Sj,
                                                   const unsigned* __restrict__ prio, const int* __restrict__ cin,
                                                   int* __restrict__ cout, int* __restrict__ ctl)
{
    __shared__ rd_u64 sLeft;
    __shared__ int sCols;
    const int lane = threadIdx.x & 63, sub = threadIdx.x & (L - 1);
    if (threadIdx.x == 0) { sLeft = 0; sCols = 0; }
    __syncthreads();
    bool bad = false;
    rd_u64 left = 0;
    unsigned cols = 0;                                                // the colours in use as far as this lane's rows show
    const long long nBlocks = ((long long)d.n + 256 / L - 1) / (256 / L);
    for (long long block = blockIdx.x; block < nBlocks; block += gridDim.x) {   // (uniform in the workgroup)
        int a, b;
        const long long i = ag_row<L>(d, Sp, block, a, b, bad);
        int got = i < d.n ? cin[i] : 0;
        const bool open = i < d.n && got < 0;
        const rd_u64 mine = open ? co_key(d, prio, (int)i) : 0;
        bool walk = open;                                             // (the same in the L lanes of a row)
        int base = 0;
        do {                                                          // a window of 64 colours a turn
            rd_u64 mask = 0;
            unsigned blocked = 0;
            if (walk)
                for (int q = a + sub; q < b; q += L) {
                    const int j = Sj[q];
                    if ((unsigned)j >= (unsigned)d.n) { bad = true; continue; }   // (never an index)
                    if (j == i) continue;
                    const int cj = cin[j];
                    if (cj < 0) { if (co_key(d, prio, j) > mine) blocked = 1; }
                    else if ((unsigned)(cj - base) < 64u) mask |= 1ull << (cj - base);
                }
            mask = co_lanes_or<L>(mask, lane);
            blocked = co_lanes_or32<L>(blocked, lane);
            if (walk) {
                if (blocked) walk = false;                            // an uncoloured neighbour of greater key: not this round
                else if (~mask) { got = base + __ffsll((long long)~mask) - 1; walk = false; }
                else base += 64;
            }
        } while (__ballot(walk) != 0ull);
        if (i < d.n && sub == 0) {
            cout[i] = got;
            if (got < 0) ++left;
            else cols = max(cols, (unsigned)got + 1u);
        }
    }
    cols = max(cols, lane_xor<1>(cols, lane));
    cols = max(cols, lane_xor<2>(cols, lane));
    cols = max(cols, lane_xor<4>(cols, lane));
    cols = max(cols, lane_xor<8>(cols, lane));
    cols = max(cols, lane_xor<16>(cols, lane));
    cols = max(cols, lane_xor<32>(cols, lane));
    if (lane == 0 && cols) (void)atomicMax(&sCols, (int)cols);
    rd_flag(bad, ctl);
    smv_count(left, &sLeft, ctl);                                     // (a barrier inside: sCols is complete behind it)
    if (threadIdx.x == 0 && sCols) (void)atomicMax(ctl + CO_NCOL, sCols);
}

// the lanes of the wave whose vertex holds this lane's colour (0 for a lane without a vertex); every lane comes here
__device__ __forceinline__ rd_u64 co_same(int c, bool has)
{
    rd_u64 rest = __ballot(has), mine = 0;
    while (rest) {                                                    // (uniform in the wave: a turn per colour present)
        const int leader = __ffsll((long long)rest) - 1;
        const int lc = __shfl(c, leader);
        const rd_u64 m = __ballot(has && c == lc);
        if (has && c == lc) mine = m;
        rest &= ~m;
    }
    return mine;
}

// cnt[c * nWords + g] = the vertices of colour c among 64 g .. 64 g + 63 (the table is zero beforehand)
__global__ __launch_bounds__(256) void k_col_count(int n, int nWords, int ncolors, const int* __restrict__ color,
                                                   int* __restrict__ cnt, int* __restrict__ ctl)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    const int lane = threadIdx.x & 63;
    bool has = i < n, bad = false;
    const int c = has ? color[i] : 0;
    if (has && (unsigned)c >= (unsigned)ncolors) { bad = true; has = false; }   // (never an index)
    const rd_u64 m = co_same(c, has);
    if (has && lane == __ffsll((long long)m) - 1) cnt[(long long)c * nWords + (i >> 6)] = __popcll(m);
    rd_flag(bad, ctl);
}

// order[at[c * nWords + g] + the vertices of colour c below i in its wave] = i; colorPtr[c] = at[c * nWords], c <= ncolors
__global__ __launch_bounds__(256) void k_col_number(int n, int nWords, int ncolors, const int* __restrict__ color,
                                                    const int* __restrict__ at, int* __restrict__ order,
                                                    int* __restrict__ colorPtr, int* __restrict__ ctl)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    const int lane = threadIdx.x & 63;
    bool has = i < n, bad = false;
    const int c = has ? color[i] : 0;
    if (has && (unsigned)c >= (unsigned)ncolors) { bad = true; has = false; }   // (never an index)
    const rd_u64 m = co_same(c, has);
    if (has) {
        const int o = at[(long long)c * nWords + (i >> 6)] + __popcll(m & ((1ull << lane) - 1ull));
        if ((unsigned)o < (unsigned)n) order[o] = (int)i;
        else bad = true;
    }
    if (i <= ncolors) colorPtr[i] = at[i * nWords];
    rd_flag(bad, ctl);
}

}  // namespace bhs
