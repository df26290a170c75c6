// bhs_rcm.hip.h -- the reverse Cuthill-McKee ordering of an n x n pattern S with ascending rows and a symmetric structure
// (bhs_csr_rcm_device; the contract is worded in include/bhsparse_hip.h, "bandwidth-reducing ordering").  Values are never
// taken: the same code, and the same result bit for bit, in the double and the float library.
//
// deg(i) counts the entries of row i off the diagonal; key(i) = deg(i) << 32 | i.  The textbook queue is restated level by
// level, so that everything is a function of the pattern:
//
//   k_rcm_check<L>    degrees and the four refusals: the row pointer (ag_row; rowPtr[n] against nnzS), a column outside
//                     [0, n), a row that does not ascend strictly, an entry (i, j) without (j, i) -- a binary search in row j,
//                     whose bounds are checked first.  Each raises ctl[RD_ERR]; the host reads it before anything else runs.
//   (components)      bhs_components.hip.h's kernels, unchanged: root[i], comp[i].
//   k_rcm_start       slot[root[i]] = min key, a 64-bit atomic minimum issued only where the value read is greater.
//   k_rcm_seed        per root: the start is the slot's vertex, no eccentricity yet, not done.
//   k_rcm_init        level[i] = 0 at its component's start, -1 elsewhere.
//   k_rcm_level<L>    one pull pass: a row with level -1 and a neighbour on level cur takes cur + 1 and is counted
//                     (smv_count).  A pass stores cur + 1 alone, so a racing read sees -1 or cur + 1, never cur: plain stores,
//                     unique levels.
//   k_rcm_far_max     eslot[root[i]] = max level, a 64-bit atomic maximum (issued only where the value read is smaller).
//   k_rcm_far_min     xslot[root[i]] = min key among the vertices on that level.
//   k_rcm_decide      per root: the depth (a maximum a wave, then one atomic), and under BHS_RCM_PERIPHERAL the George-Liu
//                     step: after sweep 0 the start moves to x; later a component whose eccentricity did not grow is done and
//                     keeps its start, any other takes the new one and moves to x.  The components that moved are counted.
//   k_rcm_roots       level 0 of the numbering: pos[start] = comp[start], forest[comp] = start, d_start[comp] = start.
//   k_rcm_parent<L>   over the slice of level l (the vertices by (level, index)): parent = the least pos among the neighbours
//                     on level l - 1; one atomicAdd into the parent's child count (indexed by its place in its level).
//   k_rcm_place<L>    the same slice: the rank among the siblings by walking the PARENT's row and counting the entries on
//                     level l with the same parent and a smaller key; pos = levelPtr[l] + offset(parent) + rank, the offsets
//                     being the library's one-pass scan of the child counts (host: side_scan); forest[pos] = v.  The walk costs
//                     deg(parent) a child: quadratic in a hub's degree (profiles/rcm_case.md).
//                     It also hands down the places its component holds in the level (RcmSeg) and from them loc, the
//                     vertex's place among its component's vertices in forest order.
//   k_rcm_perm        the forest order stably regrouped by component: k = compPtr[comp[v]] + loc[v], compPtr being the
//                     library's scan of the components' sizes; perm[k] or perm[n - 1 - k] = v.
//
// Every grid is capped and every kernel walks its blocks in a loop.  Nothing spins, nothing waits for another workgroup; every
// lane of a wave reaches the reductions.  Validation as in the components, ahead of each dependent read: a row's bounds
// wherever they are read, a column before it indexes anything, and every index the call made itself before it is one.
#pragma once
#include "bhs_components.hip.h"

namespace bhs {

// control words: the components'; behind them the greatest number of levels of a component.  The components that moved
// are counted where the passes count (AG_UNDEC).
enum { RCM_DEPTH = CC_INTS, RCM_INTS = CC_INTS + 4 };

constexpr int kRcmPeripheral = 1, kRcmNoReverse = 2;                  // BHS_RCM_PERIPHERAL, BHS_RCM_NO_REVERSE

// a level's slice of the order by (level, index), and the one before it
struct RcmLevel {
    int l, lo, cnt, prevLo, prevCnt;
};

// Per vertex, for the regrouping: the places [first, end) its component holds in its level -- the components of a level are
// contiguous and ascend, since a level is ordered by the parents' places -- and loc, its place among its component's
// vertices in forest order: the component's vertices on the levels before, plus its place in the segment.
struct RcmSeg {
    int* first; int* end; int* loc;
};

__device__ __forceinline__ rd_u64 rcm_key(const int* __restrict__ deg, int i)
{
    return ((rd_u64)(unsigned)deg[i] << 32) | (rd_u64)(unsigned)i;
}

__device__ __forceinline__ rd_u64 rcm_load64(const rd_u64* p)
{
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// the sum of v over the L lanes that share a row; every lane of the wave comes here
template <int L>
__device__ __forceinline__ unsigned rcm_lanes_sum(unsigned v, int lane)
{
    if constexpr (L > 1) v += lane_xor<1>(v, lane);
    if constexpr (L > 2) v += lane_xor<2>(v, lane);
    if constexpr (L > 4) v += lane_xor<4>(v, lane);
    if constexpr (L > 8) v += lane_xor<8>(v, lane);
    if constexpr (L > 16) v += lane_xor<16>(v, lane);
    if constexpr (L > 32) v += lane_xor<32>(v, lane);
    return v;
}

// the vertex of this thread's group of L lanes in a level's slice (-1: none), and its checked range [a, b)
template <int L>
__device__ __forceinline__ int rcm_item(const AgDims& d, const RcmLevel& lv, const int* __restrict__ Sp, const int* __restrict__ byLevel,
                                        long long block, int& a, int& b, bool& bad)
{
    const long long t = block * (256 / L) + threadIdx.x / L;
    a = b = 0;
    if (t >= lv.cnt) return -1;
    const int v = byLevel[lv.lo + t];
    if ((unsigned)v >= (unsigned)d.n) { bad = true; return -1; }      // (never an index)
    const int lo = Sp[v], hi = Sp[v + 1];
    if (rd_bounds_bad(lo, hi, d.nnzS)) bad = true;
    else { a = lo; b = hi; }
    return v;
}

template <int L>
__global__ __launch_bounds__(256) void k_rcm_check(AgDims d, const int* __restrict__ Sp, const int* __restrict__ Sj, int* __restrict__ deg,
                                                   int* __restrict__ ctl)
{
    const int lane = threadIdx.x & 63, sub = threadIdx.x & (L - 1);
    bool bad = blockIdx.x == 0 && threadIdx.x == 0 && Sp[d.n] != d.nnzS;
    const long long nBlocks = ((long long)d.n + 256 / L - 1) / (256 / L);
    for (long long t = blockIdx.x; t < nBlocks; t += gridDim.x) {     // (uniform in the workgroup)
        int a, b;
        const long long i = ag_row<L>(d, Sp, t, a, b, bad);
        unsigned cnt = 0;
        for (int q = a + sub; q < b; q += L) {
            const int j = Sj[q];
            if ((unsigned)j >= (unsigned)d.n) { bad = true; continue; }   // (never an index)
            if (q > a && Sj[q - 1] >= j) bad = true;                  // strictly ascending
            if (j == i) continue;
            ++cnt;
            const int lo0 = Sp[j], hi0 = Sp[j + 1];
            if (rd_bounds_bad(lo0, hi0, d.nnzS)) { bad = true; continue; }
            int lo = lo0, hi = hi0;                                   // the first entry of row j that is not below i
            for (int s = 0; s < 32; ++s) {
                if (lo >= hi) break;
                const int mid = lo + (hi - lo) / 2;
                if (Sj[mid] < (int)i) lo = mid + 1;
                else hi = mid;
            }
            if (lo >= hi0 || Sj[lo] != (int)i) bad = true;            // (i, j) without (j, i)
        }
        cnt = rcm_lanes_sum<L>(cnt, lane);
        if (i < d.n && sub == 0) deg[i] = (int)cnt;
    }
    rd_flag(bad, ctl);
}

__global__ __launch_bounds__(256) void k_rcm_start(int n, const int* __restrict__ root, const int* __restrict__ deg, rd_u64* slot,
                                                   int* __restrict__ ctl)
{
    bool bad = false;
    const long long nBlocks = ((long long)n + 255) / 256;
    for (long long t = blockIdx.x; t < nBlocks; t += gridDim.x) {
        const long long i = t * 256 + threadIdx.x;
        if (i < n) {
            const int r = root[i];
            if ((unsigned)r >= (unsigned)n) { bad = true; continue; }    // (never an index; the roots were this call's own)
            const rd_u64 k = rcm_key(deg, (int)i);
            if (rcm_load64(slot + r) > k) (void)atomicMin(slot + r, k);
        }
    }
    rd_flag(bad, ctl);
}

__global__ __launch_bounds__(256) void k_rcm_seed(int n, const int* __restrict__ root, const rd_u64* __restrict__ slot,
                                                  int* __restrict__ start, int* __restrict__ ecc, int* __restrict__ done)
{
    const long long nBlocks = ((long long)n + 255) / 256;
    for (long long t = blockIdx.x; t < nBlocks; t += gridDim.x) {
        const long long i = t * 256 + threadIdx.x;
        if (i < n && root[i] == (int)i) {
            start[i] = (int)(slot[i] & 0xffffffffull);
            ecc[i] = -1;
            done[i] = 0;
        }
    }
}

__global__ __launch_bounds__(256) void k_rcm_init(int n, const int* __restrict__ root, const int* __restrict__ start, int* __restrict__ level,
                                                  int* __restrict__ ctl)
{
    bool bad = false;
    const long long nBlocks = ((long long)n + 255) / 256;
    for (long long t = blockIdx.x; t < nBlocks; t += gridDim.x) {
        const long long i = t * 256 + threadIdx.x;
        if (i < n) {
            const int r = root[i];
            if ((unsigned)r >= (unsigned)n) { bad = true; continue; }    // (never an index)
            level[i] = start[r] == (int)i ? 0 : -1;
        }
    }
    rd_flag(bad, ctl);
}

template <int L>
__global__ __launch_bounds__(256) void k_rcm_level(AgDims d, const int* __restrict__ Sp, const int* __restrict__ Sj, int* level, int cur,
                                                   int* __restrict__ ctl)
{
    __shared__ rd_u64 sChg;
    const int lane = threadIdx.x & 63, sub = threadIdx.x & (L - 1);
    if (threadIdx.x == 0) sChg = 0;
    __syncthreads();
    bool bad = false;
    rd_u64 chg = 0;
    const long long nBlocks = ((long long)d.n + 256 / L - 1) / (256 / L);
    for (long long t = blockIdx.x; t < nBlocks; t += gridDim.x) {     // (uniform in the workgroup)
        int a, b;
        const long long i = ag_row<L>(d, Sp, t, a, b, bad);
        const bool open = i < d.n && cc_load(level + i) == -1;        // (written by this row's owner alone)
        if (!open) a = b = 0;                                         // visited: nothing of the row is read
        unsigned none = 1;
        for (int q = a + sub; q < b; q += L) {
            const int j = Sj[q];
            if ((unsigned)j >= (unsigned)d.n) { bad = true; continue; }   // (never an index)
            if (j != i && cc_load(level + j) == cur) { none = 0; break; }
        }
        none = ts_lanes_min<L>(none, lane);
        if (open && sub == 0 && !none) {
            level[i] = cur + 1;
            ++chg;
        }
    }
    rd_flag(bad, ctl);
    smv_count(chg, &sChg, ctl);
}

__global__ __launch_bounds__(256) void k_rcm_far_max(int n, const int* __restrict__ root, const int* __restrict__ level, rd_u64* eslot,
                                                     int* __restrict__ ctl)
{
    bool bad = false;
    const long long nBlocks = ((long long)n + 255) / 256;
    for (long long t = blockIdx.x; t < nBlocks; t += gridDim.x) {
        const long long i = t * 256 + threadIdx.x;
        if (i < n) {
            const int r = root[i], l = level[i];
            if ((unsigned)r >= (unsigned)n || l < 0) { bad = true; continue; }   // (a vertex the sweep did not reach: not symmetric)
            if (rcm_load64(eslot + r) < (rd_u64)l) (void)atomicMax(eslot + r, (rd_u64)l);
        }
    }
    rd_flag(bad, ctl);
}

__global__ __launch_bounds__(256) void k_rcm_far_min(int n, const int* __restrict__ root, const int* __restrict__ level,
                                                     const int* __restrict__ deg, const rd_u64* __restrict__ eslot, rd_u64* xslot,
                                                     int* __restrict__ ctl)
{
    bool bad = false;
    const long long nBlocks = ((long long)n + 255) / 256;
    for (long long t = blockIdx.x; t < nBlocks; t += gridDim.x) {
        const long long i = t * 256 + threadIdx.x;
        if (i < n) {
            const int r = root[i];
            if ((unsigned)r >= (unsigned)n) { bad = true; continue; }    // (never an index)
            if ((rd_u64)(long long)level[i] != eslot[r]) continue;
            const rd_u64 k = rcm_key(deg, (int)i);
            if (rcm_load64(xslot + r) > k) (void)atomicMin(xslot + r, k);
        }
    }
    rd_flag(bad, ctl);
}

__global__ __launch_bounds__(256) void k_rcm_decide(int n, const int* __restrict__ root, const rd_u64* __restrict__ eslot,
                                                    const rd_u64* __restrict__ xslot, int* __restrict__ start, int* __restrict__ ecc,
                                                    int* __restrict__ done, int sweep, int peripheral, int* __restrict__ ctl)
{
    __shared__ rd_u64 sMoved;
    const int lane = threadIdx.x & 63;
    if (threadIdx.x == 0) sMoved = 0;
    __syncthreads();
    bool bad = false;
    rd_u64 moved = 0;
    unsigned depth = 0;
    const long long nBlocks = ((long long)n + 255) / 256;
    for (long long t = blockIdx.x; t < nBlocks; t += gridDim.x) {     // (uniform in the workgroup)
        const long long i = t * 256 + threadIdx.x;
        if (i < n && root[i] == (int)i) {
            const rd_u64 e = eslot[i], x = xslot[i] & 0xffffffffull;
            if (e >= (rd_u64)n || x >= (rd_u64)n) { bad = true; continue; }   // (the component holds its root: both were set)
            depth = max(depth, (unsigned)e + 1u);
            if (!peripheral) continue;
            if (sweep == 0 || (!done[i] && (int)e > ecc[i])) {
                ecc[i] = (int)e;
                start[i] = (int)x;
                ++moved;
            } else {
                done[i] = 1;
            }
        }
    }
    depth = max(depth, lane_xor<1>(depth, lane));
    depth = max(depth, lane_xor<2>(depth, lane));
    depth = max(depth, lane_xor<4>(depth, lane));
    depth = max(depth, lane_xor<8>(depth, lane));
    depth = max(depth, lane_xor<16>(depth, lane));
    depth = max(depth, lane_xor<32>(depth, lane));
    if (lane == 0 && depth) (void)atomicMax(ctl + RCM_DEPTH, (int)depth);
    rd_flag(bad, ctl);
    smv_count(moved, &sMoved, ctl);
}

__global__ __launch_bounds__(256) void k_rcm_roots(int n, int ncomp, const int* __restrict__ byLevel, const int* __restrict__ comp,
                                                   int* __restrict__ pos, int* __restrict__ forest, RcmSeg seg,
                                                   int* __restrict__ startOut, int* __restrict__ ctl)
{
    bool bad = false;
    const long long nBlocks = ((long long)ncomp + 255) / 256;
    for (long long t = blockIdx.x; t < nBlocks; t += gridDim.x) {
        const long long k = t * 256 + threadIdx.x;
        if (k < ncomp) {
            const int v = byLevel[k];
            if ((unsigned)v >= (unsigned)n) { bad = true; continue; }    // (never an index)
            const int c = comp[v];
            if ((unsigned)c >= (unsigned)ncomp) { bad = true; continue; }
            pos[v] = c;
            forest[c] = v;
            seg.first[v] = c;
            seg.end[v] = c + 1;
            seg.loc[v] = 0;
            if (startOut) startOut[c] = v;
        }
    }
    rd_flag(bad, ctl);
}

template <int L>
__global__ __launch_bounds__(256) void k_rcm_parent(AgDims d, RcmLevel lv, const int* __restrict__ Sp, const int* __restrict__ Sj,
                                                    const int* __restrict__ byLevel, const int* __restrict__ level,
                                                    const int* __restrict__ pos, int* __restrict__ parent, int* __restrict__ kids,
                                                    int* __restrict__ ctl)
{
    const int lane = threadIdx.x & 63, sub = threadIdx.x & (L - 1);
    bool bad = false;
    const long long nBlocks = ((long long)lv.cnt + 256 / L - 1) / (256 / L);
    for (long long t = blockIdx.x; t < nBlocks; t += gridDim.x) {     // (uniform in the workgroup)
        int a, b;
        const int v = rcm_item<L>(d, lv, Sp, byLevel, t, a, b, bad);
        unsigned m = 0xffffffffu;
        for (int q = a + sub; q < b; q += L) {
            const int j = Sj[q];
            if ((unsigned)j >= (unsigned)d.n) { bad = true; continue; }   // (never an index)
            if (level[j] == lv.l - 1) m = min(m, (unsigned)pos[j]);
        }
        m = ts_lanes_min<L>(m, lane);
        if (v >= 0 && sub == 0) {
            if (m - (unsigned)lv.prevLo >= (unsigned)lv.prevCnt) { bad = true; continue; }   // (a place in the level before)
            parent[v] = (int)m;
            (void)atomicAdd(kids + (m - (unsigned)lv.prevLo), 1);
        }
    }
    rd_flag(bad, ctl);
}

template <int L>
__global__ __launch_bounds__(256) void k_rcm_place(AgDims d, RcmLevel lv, const int* __restrict__ Sp, const int* __restrict__ Sj,
                                                   const int* __restrict__ byLevel, const int* __restrict__ level,
                                                   const int* __restrict__ deg, const int* __restrict__ parent,
                                                   const int* __restrict__ off, int* __restrict__ pos, int* forest, RcmSeg seg,
                                                   int* __restrict__ ctl)
{
    const int lane = threadIdx.x & 63, sub = threadIdx.x & (L - 1);
    bool bad = false;
    const long long nBlocks = ((long long)lv.cnt + 256 / L - 1) / (256 / L);
    for (long long t = blockIdx.x; t < nBlocks; t += gridDim.x) {     // (uniform in the workgroup)
        int a, b;
        const int v = rcm_item<L>(d, lv, Sp, byLevel, t, a, b, bad);
        a = b = 0;                                                    // (the row walked is the parent's)
        int pp = -1, p = -1;
        if (v >= 0) {
            pp = parent[v];
            if ((unsigned)(pp - lv.prevLo) >= (unsigned)lv.prevCnt) { bad = true; pp = -1; }   // (never an index)
            else {
                p = forest[pp];                                       // (placed by the launches of the level before)
                if ((unsigned)p >= (unsigned)d.n) { bad = true; p = pp = -1; }
                else {
                    const int lo = Sp[p], hi = Sp[p + 1];
                    if (rd_bounds_bad(lo, hi, d.nnzS)) bad = true;
                    else { a = lo; b = hi; }
                }
            }
        }
        const rd_u64 kv = v >= 0 ? rcm_key(deg, v) : 0;
        unsigned rank = 0;
        for (int q = a + sub; q < b; q += L) {
            const int u = Sj[q];
            if ((unsigned)u >= (unsigned)d.n) { bad = true; continue; }   // (never an index)
            if (u != p && level[u] == lv.l && parent[u] == pp && rcm_key(deg, u) < kv) ++rank;
        }
        rank = rcm_lanes_sum<L>(rank, lane);
        if (pp >= 0 && sub == 0) {
            const int k = off[pp - lv.prevLo] + (int)rank;
            // the component's segment of the level before, [fp, ep) from prevLo: its children are this level's [off[fp], off[ep])
            const int fp = seg.first[p] - lv.prevLo, ep = seg.end[p] - lv.prevLo;
            if (fp < 0 || fp > pp - lv.prevLo || ep <= pp - lv.prevLo || ep > lv.prevCnt) { bad = true; continue; }   // (never an index)
            const int f = off[fp], e = off[ep];
            if (f < 0 || k < f || k >= e || e > lv.cnt) { bad = true; continue; }   // (a place in this level)
            pos[v] = lv.lo + k;
            forest[lv.lo + k] = v;
            seg.first[v] = lv.lo + f;
            seg.end[v] = lv.lo + e;
            seg.loc[v] = seg.loc[p] - (pp - lv.prevLo - fp) + (ep - fp) + (k - f);
        }
    }
    rd_flag(bad, ctl);
}

__global__ __launch_bounds__(256) void k_rcm_perm(int n, int ncomp, const int* __restrict__ comp, const int* __restrict__ compPtr,
                                                  const int* __restrict__ loc, int reverse, int* __restrict__ perm, int* __restrict__ ctl)
{
    bool bad = false;
    const long long nBlocks = ((long long)n + 255) / 256;
    for (long long t = blockIdx.x; t < nBlocks; t += gridDim.x) {
        const long long v = t * 256 + threadIdx.x;
        if (v < n) {
            const int c = comp[v];
            if ((unsigned)c >= (unsigned)ncomp) { bad = true; continue; }    // (never an index)
            const long long k = (long long)compPtr[c] + loc[v];
            if (k < compPtr[c] || k >= compPtr[c + 1] || k >= n) { bad = true; continue; }   // (a place of its component)
            perm[reverse ? n - 1 - k : k] = (int)v;
        }
    }
    rd_flag(bad, ctl);
}

}  // namespace bhs
