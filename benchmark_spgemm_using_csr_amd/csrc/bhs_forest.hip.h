// bhs_forest.hip.h -- the minimum (or maximum) spanning forest of the multigraph that an n x n matrix A stores, by synchronous
// Boruvka rounds (bhs_csr_spanning_forest_device; the contract is worded in include/bhsparse_hip.h, "spanning forest").
//
// An entry (i, j) with j != i whose weight w is not NaN is the undirected edge {i, j}; w is a_ij, |a_ij| under BHS_FOREST_ABS,
// 1 without values.  Its key is the tuple (k(w), lo, hi), lo = min(i, j), hi = max(i, j), k the reductions' order-preserving
// key of w widened to double (rd_key: -0 below +0), in TWO 64-bit words: k(w) and lo << 32 | hi.  Under BHS_FOREST_MAXIMUM
// both words are complemented, which reverses the whole order; ~0 in either word is no key of any edge and stands for "none".
// The order is strict over distinct tuples, so the forest that Kruskal's algorithm builds in ascending key order is unique,
// and every tree's lightest crossing edge belongs to it: the rounds below build exactly that forest.
//
// label[i] is the root of i's tree (label[label[i]] == label[i]); it changes in k_sf_relabel alone.  A round:
//
//   k_sf_clear      bestW[c] = bestE[c] = ~0.
//   k_sf_weight<L>  reads label, lowers bestW: every entry that crosses two trees lowers the weight word of both trees.  A row
//                   over L = 1, 4, 16 or 64 lanes (ag_lanes); the row's own side is reduced across its lanes first
//                   (sf_lanes_min), the far side is lowered entry by entry.
//   k_sf_edge<L>    reads label and bestW, lowers bestE: the crossing entries whose weight word equals their tree's lower the
//                   tree's edge word, both sides as above.  After it (bestW[c], bestE[c]) is the least key over the entries
//                   that cross c's boundary, from whichever end and however often they are stored.
//   k_sf_hook       a root c with a pick reads the root d of the pick's far endpoint; where d picked the same tuple (a mutual
//                   pair) the smaller of c and d stays a root; every other c writes parent[c] = d and its pick to SLOT c
//                   (lo, hi, the weight from rd_unkey).  A root hooks once in the whole call, so a slot is written once.  With
//                   a strict order the hook graph has no cycle but the mutual pairs.  The trees hooked go to the host in
//                   one word (smv_count).
//   k_sf_jump       parent[c] = parent[parent[c]] over the round's roots, in place: whatever the races, a launch at least
//                   doubles the distance every pointer covers, so ceil(log2 R) launches reach the fixed point from R roots.
//   k_sf_relabel    label[i] = parent[label[i]], the vertex's own word; where parent[parent[l]] != parent[l] it raises the
//                   control word SF_BROKEN (the host: BHS_ERR_INTERNAL).
//
// Every launch either reads an array or writes the caller's own word of it, or lowers a word by a 64-bit unsigned atomicMin,
// whose result no order can change: everything is a function of the input.  An atomic is issued only where the word as read
// past the L1 (sf_load, as cc_load) is greater than what it would store; a stale read costs an unneeded atomic, never a
// result.  After the rounds:
//
//   k_sf_flag       a wave per 64 vertices: the written slots (slotLo >= 0) among them as a bitmap word and its count; the
//                   library's one-pass scan over the counts gives every word its first place (host: side_scan).
//   k_sf_write      the written slots in ascending slot order to the caller's edge list.
//
// Nothing spins, nothing waits for another workgroup, no floating atomics.  Validation as in the components, ahead of each
// dependent read: a row's bounds wherever they are read (a row that fails is taken as empty), a column before it indexes
// anything (skipped where it fails); either raises ctl[RD_ERR].  The indices that the hook takes out of an edge word went
// through that check; they are checked again before they index (SF_BROKEN), as are the places of the write-out.
#pragma once
#include "bhs_components.hip.h"

namespace bhs {

// control words: the aggregation's (the error word, the 64-bit count of trees hooked where smv_count adds it, the scan's);
// word 0, which the reductions use for a queue, is this family's "the call's own arrays are inconsistent"
enum { SF_BROKEN = RD_CNT_WAVE, SF_INTS = AG_INTS };
enum { kSfMaximum = 1, kSfAbs = 2 };                                  // BHS_FOREST_*
constexpr rd_u64 kSfNone = ~0ull;

__device__ __forceinline__ rd_u64 sf_load(const rd_u64* p)
{
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// *p = min(*p, v), where the word as read is greater
__device__ __forceinline__ void sf_lower(rd_u64* p, rd_u64 v)
{
    if (sf_load(p) > v) (void)atomicMin(p, v);
}

// raises SF_BROKEN: a plain store of the one value the word ever takes after its clearing; every lane of the wave comes here
__device__ __forceinline__ void sf_flag(bool broken, int* __restrict__ ctl)
{
    if (__ballot(broken) != 0ull && (threadIdx.x & 63) == 0) ctl[SF_BROKEN] = 1;
}

// the minimum of v over the L lanes that share a row; every lane of the wave comes here
template <int L>
__device__ __forceinline__ rd_u64 sf_lanes_min(rd_u64 v, int lane)
{
    if constexpr (L > 1) v = min(v, lane_xor64<1>(v, lane));
    if constexpr (L > 2) v = min(v, lane_xor64<2>(v, lane));
    if constexpr (L > 4) v = min(v, lane_xor64<4>(v, lane));
    if constexpr (L > 8) v = min(v, lane_xor64<8>(v, lane));
    if constexpr (L > 16) v = min(v, lane_xor64<16>(v, lane));
    if constexpr (L > 32) v = min(v, lane_xor64<32>(v, lane));
    return v;
}

// the weight word of entry q (kSfNone: a NaN, no edge); d.hasPrio: are there values, d.seed: the flags
__device__ __forceinline__ rd_u64 sf_weight(const AgDims& d, const value_t* __restrict__ Ax, int q)
{
    double w = 1.0;
    if (d.hasPrio) {
        w = (double)Ax[q];                                            // (exact: both libraries compare alike)
        if (w != w) return kSfNone;
        if (d.seed & kSfAbs) w = fabs(w);
    }
    const rd_u64 k = rd_key(w, false);
    return (d.seed & kSfMaximum) ? ~k : k;
}

__device__ __forceinline__ rd_u64 sf_pair(const AgDims& d, long long i, int j)
{
    const rd_u64 lo = (rd_u64)min((long long)j, i), hi = (rd_u64)max((long long)j, i);
    const rd_u64 e = lo << 32 | hi;
    return (d.seed & kSfMaximum) ? ~e : e;
}

__global__ __launch_bounds__(256) void k_sf_init(AgDims d, const int* __restrict__ Ap, int* __restrict__ label,
                                                 int* __restrict__ parent, int* __restrict__ slotLo, int* __restrict__ ctl)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    bool bad = false;
    if (i < d.n) {
        label[i] = (int)i;
        parent[i] = (int)i;
        slotLo[i] = -1;
        bad = rd_bounds_bad(Ap[i], Ap[i + 1], d.nnzS);
    }
    rd_flag(bad, ctl);
}

__global__ __launch_bounds__(256) void k_sf_clear(int n, rd_u64* __restrict__ bestW, rd_u64* __restrict__ bestE)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i < n) {
        bestW[i] = kSfNone;
        bestE[i] = kSfNone;
    }
}

template <int L>
__global__ __launch_bounds__(256) void k_sf_weight(AgDims d, const int* __restrict__ Ap, const int* __restrict__ Aj,
                                                   const value_t* __restrict__ Ax, const int* __restrict__ label, rd_u64* bestW,
                                                   int* __restrict__ ctl)
{
    const int lane = threadIdx.x & 63, sub = threadIdx.x & (L - 1);
    bool bad = false;
    const long long nBlocks = ((long long)d.n + 256 / L - 1) / (256 / L);
    for (long long t = blockIdx.x; t < nBlocks; t += gridDim.x) {     // (uniform in the workgroup)
        int a, b;
        const long long i = ag_row<L>(d, Ap, t, a, b, bad);
        const int li = i < d.n ? label[i] : 0;
        rd_u64 m = kSfNone;
        for (int q = a + sub; q < b; q += L) {
            const int j = Aj[q];
            if ((unsigned)j >= (unsigned)d.n) { bad = true; continue; }   // (never an index)
            if (j == i) continue;
            const int lj = label[j];
            if (lj == li) continue;
            const rd_u64 k = sf_weight(d, Ax, q);
            if (k == kSfNone) continue;
            m = min(m, k);
            sf_lower(bestW + lj, k);                                  // (a label is a vertex: lj < n)
        }
        m = sf_lanes_min<L>(m, lane);
        if (i < d.n && sub == 0 && m != kSfNone) sf_lower(bestW + li, m);
    }
    rd_flag(bad, ctl);
}

// (the columns and the row bounds were flagged by k_sf_weight: here they are skipped alone)
template <int L>
__global__ __launch_bounds__(256) void k_sf_edge(AgDims d, const int* __restrict__ Ap, const int* __restrict__ Aj,
                                                 const value_t* __restrict__ Ax, const int* __restrict__ label,
                                                 const rd_u64* __restrict__ bestW, rd_u64* bestE)
{
    const int lane = threadIdx.x & 63, sub = threadIdx.x & (L - 1);
    bool bad = false;
    const long long nBlocks = ((long long)d.n + 256 / L - 1) / (256 / L);
    for (long long t = blockIdx.x; t < nBlocks; t += gridDim.x) {     // (uniform in the workgroup)
        int a, b;
        const long long i = ag_row<L>(d, Ap, t, a, b, bad);
        const int li = i < d.n ? label[i] : 0;
        const rd_u64 mine = i < d.n ? bestW[li] : kSfNone;
        rd_u64 m = kSfNone;
        if (mine == kSfNone) a = b = 0;                               // a tree without a crossing entry: nothing of the row is read
        for (int q = a + sub; q < b; q += L) {
            const int j = Aj[q];
            if ((unsigned)j >= (unsigned)d.n || j == i) continue;     // (never an index)
            const int lj = label[j];
            if (lj == li) continue;
            const rd_u64 k = sf_weight(d, Ax, q);
            if (k == kSfNone) continue;
            const bool here = k == mine, there = k == bestW[lj];
            if (!here && !there) continue;
            const rd_u64 e = sf_pair(d, i, j);
            if (here) m = min(m, e);
            if (there) sf_lower(bestE + lj, e);
        }
        m = sf_lanes_min<L>(m, lane);
        if (i < d.n && sub == 0 && m != kSfNone) sf_lower(bestE + li, m);
    }
}

__global__ __launch_bounds__(256) void k_sf_hook(AgDims d, const int* __restrict__ label, const rd_u64* __restrict__ bestW,
                                                 const rd_u64* __restrict__ bestE, int* __restrict__ parent,
                                                 int* __restrict__ slotLo, int* __restrict__ slotHi, value_t* __restrict__ slotVal,
                                                 int* __restrict__ ctl)
{
    __shared__ rd_u64 sCount;
    if (threadIdx.x == 0) sCount = 0;
    __syncthreads();
    rd_u64 count = 0;                                                 // the trees this round hooked
    bool broken = false;
    const long long nBlocks = ((long long)d.n + 255) / 256;
    for (long long block = blockIdx.x; block < nBlocks; block += gridDim.x) {   // (uniform in the workgroup: every lane reaches the reduction)
        const long long c = block * 256 + threadIdx.x;
        if (c >= d.n || label[c] != (int)c) continue;
        const rd_u64 kw = bestW[c], ke = bestE[c];
        if (kw == kSfNone) continue;                                  // no entry leaves the tree
        const rd_u64 e = (d.seed & kSfMaximum) ? ~ke : ke;
        const unsigned lo = (unsigned)(e >> 32), hi = (unsigned)(e & 0xffffffffull);
        if (ke == kSfNone || lo >= hi || hi >= (unsigned)d.n) { broken = true; continue; }   // (never an index)
        const int llo = label[lo], lhi = label[hi];
        if ((llo == (int)c) == (lhi == (int)c)) { broken = true; continue; }   // (one end inside, one outside)
        const int far = llo == (int)c ? lhi : llo;
        if ((unsigned)far >= (unsigned)d.n) { broken = true; continue; }
        if (bestW[far] == kw && bestE[far] == ke && c < far) continue;   // a mutual pair: the smaller stays a root
        parent[c] = far;
        slotLo[c] = (int)lo;
        slotHi[c] = (int)hi;
        slotVal[c] = (value_t)rd_unkey((d.seed & kSfMaximum) ? ~kw : kw);
        count += 1ull;
    }
    sf_flag(broken, ctl);
    smv_count(count, &sCount, ctl);
}

// over the round's roots (label has not moved yet); the words are read past the L1: what another workgroup wrote in this
// launch may be seen, which only shortens the way
__global__ __launch_bounds__(256) void k_sf_jump(int n, const int* __restrict__ label, int* parent)
{
    const long long c = (long long)blockIdx.x * 256 + threadIdx.x;
    if (c >= n || label[c] != (int)c) return;
    const int p = cc_load(parent + c);
    if ((unsigned)p >= (unsigned)n || p == (int)c) return;            // (never an index)
    const int g = cc_load(parent + p);
    if (g != p && (unsigned)g < (unsigned)n) parent[c] = g;
}

__global__ __launch_bounds__(256) void k_sf_relabel(int n, const int* __restrict__ parent, int* __restrict__ label,
                                                    int* __restrict__ ctl)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    bool broken = false;
    if (i < n) {
        const int l = label[i];
        if ((unsigned)l >= (unsigned)n) broken = true;                // (never an index)
        else {
            const int p = parent[l];
            if ((unsigned)p >= (unsigned)n || parent[p] != p) broken = true;
            else if (p != l) label[i] = p;
        }
    }
    sf_flag(broken, ctl);
}

// map[g] = the written slots among 64 g .. 64 g + 63 as bits, cnt[g] their number (a wave per word)
__global__ __launch_bounds__(256) void k_sf_flag(int n, const int* __restrict__ slotLo, rd_u64* __restrict__ map, int* __restrict__ cnt)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    const rd_u64 bits = __ballot(i < n && slotLo[i] >= 0);
    if ((threadIdx.x & 63) == 0 && (i >> 6) < (((long long)n + 63) >> 6)) {
        map[i >> 6] = bits;
        cnt[i >> 6] = __popcll(bits);
    }
}

// slot c to place at[word of c] + the written slots below c in its word (edgeVal may be null)
__global__ __launch_bounds__(256) void k_sf_write(int n, const int* __restrict__ slotLo, const int* __restrict__ slotHi,
                                                  const value_t* __restrict__ slotVal, const rd_u64* __restrict__ map,
                                                  const int* __restrict__ at, int* __restrict__ edgeLo, int* __restrict__ edgeHi,
                                                  value_t* __restrict__ edgeVal, int* __restrict__ ctl)
{
    const long long c = (long long)blockIdx.x * 256 + threadIdx.x;
    bool broken = false;
    if (c < n && slotLo[c] >= 0) {
        const int at0 = at[c >> 6] + __popcll(map[c >> 6] & ((1ull << (c & 63)) - 1ull));
        if ((unsigned)at0 >= (unsigned)n) broken = true;              // (never an index; the places were this call's own)
        else {
            edgeLo[at0] = slotLo[c];
            edgeHi[at0] = slotHi[c];
            if (edgeVal) edgeVal[at0] = slotVal[c];
        }
    }
    sf_flag(broken, ctl);
}

}  // namespace bhs
