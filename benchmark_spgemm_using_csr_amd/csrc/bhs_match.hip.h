// bhs_match.hip.h -- heavy-edge matching of the vertices of an n x n matrix A: every vertex is paired with the neighbour it is
// most strongly coupled to, greedily in descending edge key (bhs_csr_match_device; the contract is worded in
// include/bhsparse_hip.h, "matching").
//
// An entry (i, j) of row i is an edge seen from i where j != i, w = |a_ij| > 0 and w is not NaN (+Inf is a weight, an explicit
// zero is no connection, without values every weight is 1; of a repeated (i, j) the greatest weight counts, because a maximum
// is taken; rows need not be sorted).  The key of an edge is the tuple (w, h(lo, hi), lo, hi), compared lexicographically,
// lo = min(i, j), hi = max(i, j), h(lo, hi) = mix(mix(lo ^ seed) ^ hi) with the aggregation's finaliser (ag_hash).  w is
// compared in the library's value type: the bit pattern of a non-negative IEEE number read as an unsigned integer preserves
// order.  SEEN FROM ONE VERTEX i the pairs (lo, hi) of two of its edges compare as their other endpoints do -- both beyond i:
// lo is i for both; both below i: hi is i for both; one on each side: the one below has the smaller lo -- so "the greater
// other endpoint wins" and a vertex needs only TWO WORDS a candidate: the weight's bits and h << 32 | j (mt_key).  The hash
// stands in front of the indices because with index tie-breaks alone a path of equal weights is matched from one end, one
// pair a round.
//
// mate[] holds -1 undecided, i itself finally unmatched, j matched with j.  A round is synchronous over mate[]:
//
//   k_mt_init      a thread per vertex: mate[i] = -1, its row's two bounds checked.
//   k_mt_propose   reads mate, writes cand: for an undecided i, cand[i] = the undecided neighbour of greatest key over i's
//                  edges, -1 without one.  A row over L = 1, 4, 16 or 64 lanes (ag_lanes), the L lanes' candidates meet in a
//                  DPP reduction of the two words (mt_lanes_max), which every lane of the wave reaches.  The lanes of a decided
//                  vertex skip its row.  mate[j] is read only after j passed the range check.
//   k_mt_accept    reads cand, reads and writes the vertex's OWN word of mate alone: an undecided i with cand[i] == -1 becomes
//                  i -- final, because eligibility only shrinks; one with c = cand[i] and cand[c] == i becomes c (c was
//                  undecided when the round began, so cand[c] is this round's).  No launch both reads and writes words that
//                  another vertex's lanes touch: nothing depends on timing.  The pairs a round made and the vertices it left
//                  undecided go to the host in one 64-bit word, pairs in the low half: lane -> wave -> workgroup -> one add
//                  (smv_count); the grid is bounded and a workgroup walks several blocks of vertices.
//   k_mt_finish    after a round that matched nothing although vertices were left (possible only where pattern or weights
//                  are not symmetric): mate[i] = i for them.
//   k_mt_flag      a wave per 64 vertices: the leaders (mate[i] >= i, the smaller end of a pair or a single vertex) among them
//                  as a bitmap word and its count; the library's one-pass scan gives every word its first number (host:
//                  side_scan), as the components number their roots.
//   k_mt_number    agg[i] = the rank of min(i, mate[i]) among the leaders: pairs and singletons by ascending leader.
//
// Where pattern and weights are symmetric the edge of greatest key among the undecided is proposed from both ends, so every
// round makes a pair while an edge is left, and an edge is taken exactly when no edge of greater key at either end is: the
// greedy matching in descending key order, unique and maximal.  For any other input the rounds still give a matching
// (mate[mate[i]] == i: both ends write in the same launch, from the same cand) that is a function of the input.
//
// Nothing spins, nothing waits for another workgroup; no atomics on results, no LDS beyond the count's one word.  Validation
// on the device, ahead of each dependent read: a row's bounds wherever they are read (a row that fails is taken as empty), a
// column before it indexes anything (skipped where it fails); either raises ctl[RD_ERR], which the host reads with the first
// round's count -- in the first round every vertex is undecided, so every row is read.
#pragma once
#include "bhs_components.hip.h"

namespace bhs {

// control words: the aggregation's (the error word, the round's 64-bit count where smv_count adds it, the scan's)
enum { MT_INTS = AG_INTS };

// what a vertex keeps of a candidate: the weight's bits (0: none -- a weight is greater than zero) and h << 32 | j
struct MtKey {
    rd_u64 w, k;
};

__device__ __forceinline__ bool mt_less(const MtKey& a, const MtKey& b) { return a.w < b.w || (a.w == b.w && a.k < b.k); }

// h(lo, hi) << 32 | j for the edge {i, j} seen from i
__device__ __forceinline__ rd_u64 mt_key(unsigned i, unsigned j, unsigned seed)
{
    const unsigned lo = min(i, j), hi = max(i, j);
    return ((rd_u64)ag_hash(ag_hash(lo, seed) ^ hi, 0u) << 32) | (rd_u64)j;
}

// the bits of |v| where that is a weight, else 0 (zero, minus zero, NaN)
__device__ __forceinline__ rd_u64 mt_weight(value_t v)
{
    if (v != v) return 0;
#ifdef BHS_VALUE_FLOAT
    return (rd_u64)__float_as_uint(fabsf(v));
#else
    return (rd_u64)__double_as_longlong(fabs(v));
#endif
}

template <int S>
__device__ __forceinline__ MtKey mt_meet(MtKey v, int lane)
{
    MtKey o;
    o.w = lane_xor64<S>(v.w, lane);
    o.k = lane_xor64<S>(v.k, lane);
    return mt_less(v, o) ? o : v;
}

// the greatest candidate of the L lanes that share a row; every lane of the wave comes here
template <int L>
__device__ __forceinline__ MtKey mt_lanes_max(MtKey v, int lane)
{
    if constexpr (L > 1) v = mt_meet<1>(v, lane);
    if constexpr (L > 2) v = mt_meet<2>(v, lane);
    if constexpr (L > 4) v = mt_meet<4>(v, lane);
    if constexpr (L > 8) v = mt_meet<8>(v, lane);
    if constexpr (L > 16) v = mt_meet<16>(v, lane);
    if constexpr (L > 32) v = mt_meet<32>(v, lane);
    return v;
}

__global__ __launch_bounds__(256) void k_mt_init(AgDims d, const int* __restrict__ Ap, int* __restrict__ mate, int* __restrict__ ctl)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    bool bad = false;
    if (i < d.n) {
        mate[i] = -1;
        bad = rd_bounds_bad(Ap[i], Ap[i + 1], d.nnzS);
    }
    rd_flag(bad, ctl);
}

// (d.hasPrio: are there values)
template <int L>
__global__ __launch_bounds__(256) void k_mt_propose(AgDims d, const int* __restrict__ Ap, const int* __restrict__ Aj,
                                                    const value_t* __restrict__ Ax, const int* __restrict__ mate,
                                                    int* __restrict__ cand, int* __restrict__ ctl)
{
    const int lane = threadIdx.x & 63, sub = threadIdx.x & (L - 1);
    bool bad = false;
    int a, b;
    const long long i = ag_row<L>(d, Ap, blockIdx.x, a, b, bad);
    const bool open = i < d.n && mate[i] < 0;
    if (!open) a = b = 0;                                            // decided: nothing of the row is read
    MtKey v = {0, 0};
    for (int q = a + sub; q < b; q += L) {
        const int j = Aj[q];
        if ((unsigned)j >= (unsigned)d.n) { bad = true; continue; }   // (never an index)
        if (j == i) continue;
        MtKey e;
        e.w = d.hasPrio ? mt_weight(Ax[q]) : 1ull;
        if (e.w == 0 || mate[j] >= 0) continue;
        e.k = mt_key((unsigned)i, (unsigned)j, d.seed);
        if (mt_less(v, e)) v = e;
    }
    v = mt_lanes_max<L>(v, lane);
    if (open && sub == 0) cand[i] = v.w ? (int)(v.k & 0xffffffffull) : -1;
    rd_flag(bad, ctl);
}

__global__ __launch_bounds__(256) void k_mt_accept(int n, const int* __restrict__ cand, int* __restrict__ mate, int* __restrict__ ctl)
{
    __shared__ rd_u64 sCount;
    if (threadIdx.x == 0) sCount = 0;
    __syncthreads();
    rd_u64 count = 0;                                                // pairs (counted at their smaller end) | undecided left << 32
    const long long nBlocks = ((long long)n + 255) / 256;
    for (long long block = blockIdx.x; block < nBlocks; block += gridDim.x) {   // (uniform in the workgroup: every lane reaches the reduction)
        const long long i = block * 256 + threadIdx.x;
        if (i < n && mate[i] < 0) {
            const int c = cand[i];                                   // (-1, or an index that passed the range check)
            if (c < 0) mate[i] = (int)i;
            else if (cand[c] == (int)i) {
                mate[i] = c;
                if (i < c) count += 1ull;
            } else count += 1ull << 32;
        }
    }
    smv_count(count, &sCount, ctl);
}

__global__ __launch_bounds__(256) void k_mt_finish(int n, int* __restrict__ mate)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i < n && mate[i] < 0) mate[i] = (int)i;
}

// map[g] = the leaders among vertices 64 g .. 64 g + 63 as bits, cnt[g] their number (a wave per word)
__global__ __launch_bounds__(256) void k_mt_flag(int n, const int* __restrict__ mate, rd_u64* __restrict__ map, int* __restrict__ cnt)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    const rd_u64 bits = __ballot(i < n && mate[i] >= (int)i);
    if ((threadIdx.x & 63) == 0 && (i >> 6) < (((long long)n + 63) >> 6)) {
        map[i >> 6] = bits;
        cnt[i >> 6] = __popcll(bits);
    }
}

// agg[i] = at[word of the leader] + the leaders below it in its word, the leader min(i, mate[i])
__global__ __launch_bounds__(256) void k_mt_number(int n, const int* __restrict__ mate, const rd_u64* __restrict__ map,
                                                   const int* __restrict__ at, int* __restrict__ agg, int* __restrict__ ctl)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    bool bad = false;
    if (i < n) {
        const int r = min((int)i, mate[i]);
        if ((unsigned)r >= (unsigned)n) bad = true;                  // (never an index; the mates were this call's own)
        else {
            const int c = at[r >> 6] + __popcll(map[r >> 6] & ((1ull << (r & 63)) - 1ull));
            if ((unsigned)c >= (unsigned)n) bad = true;
            else agg[i] = c;
        }
    }
    rd_flag(bad, ctl);
}

}  // namespace bhs
