// bhs_sssp.hip.h -- shortest paths from a set of sources over the out-edges of an n x n matrix G with weights that are not
// negative, by delta-stepping on a queue (bhs_csr_sssp_device; the contract is worded in include/bhsparse_hip.h, "shortest
// paths").  d[v] is the least fixed point of d[s] = 0, d[v] = min over the edges (u, v) of fl(d[u] + w): ONE rounding to the
// value type an edge.  Floating add is monotone (a <= b gives fl(a + w) <= fl(b + w)) and min is exact, so that fixed point
// does not depend on the order of the relaxations: the same bits for every bucket width, and a textbook Dijkstra's.
//
// Distances are kept as the unsigned integer words of the value type's width (ss_word): values that are not negative order as
// their words do, +Inf's word is the start value and an integer atomicMin is the relaxation.  done[v] is the distance at which
// v last relaxed its out-edges, +Inf at first; v is PENDING while dist[v] < done[v].  A pass's vertices are a slice of at most
// n ints with, beside every vertex, the distance it had when the pass before ended (sval): a pass relaxes from these
// snapshots alone, so which words it lowers, to what, and which vertices it appends are functions of the input -- the passes
// are SYNCHRONOUS, and their number is an output.  The order INSIDE a slice DEPENDS ON TIMING and is none.
//
// A pass is four launches with no host decision between them:
//
//   k_sssp_relax<L>   over the slice, L lanes a vertex, a row beyond 32 entries a lane by a whole wave: for a slice vertex v
//                     with dv (its snapshot) below done[v], done[v] = dv, and for every out-edge (v, u, w) nd = fl(dv + w);
//                     where nd is below dist[u] as read (a filter only), old = atomicMin(dist + u, nd).  The thread with
//                     nd < old and nd below the bucket's bound claims u by atomicExch(stamp + u, tag) != tag, the tag being
//                     the pass's, and appends it to the other slice at a place an atomicAdd hands out: at most one append a
//                     vertex a pass, so a slice never exceeds n.  A vertex lowered to the bound or beyond is not appended: it
//                     is pending, and the gather finds it.  u is appended exactly where the pass lowers it and leaves it
//                     below the bound: the thread that stores the word's last value sees both.
//   k_sssp_min        where the relax appended something: the appended vertices' snapshots, read when no word moves any
//                     more.  Where it appended nothing: the smallest dist among the pending vertices, an atomicMin a
//                     workgroup on a control word.
//   k_sssp_gather     where the relax appended nothing and a vertex is pending: bound = (floor(min / delta) + 1) delta in
//                     double, and every pending vertex with dist below the bound or EQUAL to the minimum is appended with its
//                     snapshot -- the minimum's holder is taken whatever the rounding of the bound, and empty buckets cost
//                     nothing.
//   k_sssp_advance    ONE thread: the slices swap, the bound is stored, the bucket is counted where the gather ran, the pass
//                     is counted, and the next slice's length goes where the host's loop reads its count.  A pass that leaves
//                     no slice has left nothing pending: it raises SSSP_DONE, and every later launch leaves at once.
//
// Before the passes k_sssp_check refuses what the contract refuses and sets the workspace, and k_sssp_seed puts the sources in
// slice 0.  Behind them k_sssp_parents<L> takes, per vertex v, the least u with an edge (u, v), fl(d[u] + w) == d[v] and
// d[u] < d[v] by an integer atomicMin on a workspace word, k_sssp_roots marks the sources, and k_sssp_finish -- the only code
// that writes an output, with plain stores -- copies and counts.
//
// Every grid is capped and every kernel walks its blocks in a loop; nothing spins, nothing waits for another workgroup, every
// loop is bounded.  Whatever is read from device memory and then used as an index is checked first and raises ctl[RD_ERR]
// instead: a slice's length, a slice entry, a row's bounds (rd_bounds_bad), a column, a source, a place handed out.  Once the
// word is up -- by the check's refusal, before any output is written -- every later launch leaves at once.  The atomics are
// integer atomics on the workspace alone.
#pragma once
#include "bhs_kcore.hip.h"

namespace bhs {

#ifdef BHS_VALUE_FLOAT
typedef unsigned int ss_word;
#else
typedef unsigned long long ss_word;
#endif
static_assert(sizeof(ss_word) == sizeof(value_t), "a distance is one atomic word");

// control words: bhs_aggregate.hip.h's; behind them the smallest pending distance (64 bits: the word, widened), the bucket's
// bound (a double), the slice in use, its length, the vertices the relax and the gather appended, the passes that had a
// slice, the buckets that were not empty, the call's end, and the finish's two counts.  The next slice's length is counted
// where the passes count (AG_UNDEC, 64 bits).
enum { SSSP_MIN = AG_INTS, SSSP_BOUND = AG_INTS + 2, SSSP_CUR = AG_INTS + 4, SSSP_LEN, SSSP_APPEND, SSSP_GATHERED, SSSP_PASS,
       SSSP_BUCKETS, SSSP_DONE, SSSP_REACHED, SSSP_LOOSE, SSSP_INTS = AG_INTS + 14 };
static_assert(SSSP_MIN % 2 == 0 && SSSP_BOUND % 2 == 0, "64-bit control words");

constexpr rd_u64 kSsNone = ~0ull;                                     // no pending vertex seen yet
constexpr int kSsNoParent = 0x7fffffff;                               // no tight edge seen yet
constexpr int kSsLong = kCoreLong;                                    // a row of more entries a lane goes to a whole wave

struct SsDims {
    int n, nnzG, hasVal, nsrc;
    double delta;
};

// the slices and the snapshots beside them: slice c is q[c], sv[c]
struct SsSlices {
    int* q[2];
    ss_word* sv[2];
};

__device__ __forceinline__ ss_word ss_bits(value_t x)
{
    ss_word b;
    __builtin_memcpy(&b, &x, sizeof(b));
    return b;
}

__device__ __forceinline__ value_t ss_value(ss_word b)
{
    value_t x;
    __builtin_memcpy(&x, &b, sizeof(x));
    return x;
}

__device__ __forceinline__ ss_word ss_inf() { return ss_bits((value_t)__builtin_inf()); }

__device__ __forceinline__ ss_word ss_load(const ss_word* p)
{
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// an entry's weight: 1 without values, -0 as 0
__device__ __forceinline__ value_t ss_weight(const SsDims& d, const value_t* __restrict__ Gx, int q)
{
    return d.hasVal ? Gx[q] + (value_t)0 : (value_t)1;
}

// the bound of the bucket that holds m: in double, in both libraries
__device__ __forceinline__ double ss_bound(double m, double delta)
{
#pragma clang fp contract(off)
    return (floor(m / delta) + 1.0) * delta;
}

// does this launch run: one read of the words a workgroup, so that all its threads agree.  jump: only where the relax
// appended nothing
__device__ __forceinline__ bool sssp_go(const int* ctl, bool jump, int* sGo)
{
    if (threadIdx.x == 0) *sGo = ctl[RD_ERR] == 0 && ctl[SSSP_DONE] == 0 && (!jump || ctl[SSSP_APPEND] == 0);
    __syncthreads();
    return *sGo != 0;
}

// The check and the workspace's start: the row pointer (its ends, every row's bounds), every source, and -- entry by entry,
// whatever row it lies in, so that a hub row costs what its entries cost -- every column and every weight: NaN or negative is
// refused, -0 is not; dist = done = +Inf, no stamp, no parent.
__global__ __launch_bounds__(256) void k_sssp_check(SsDims d, const int* __restrict__ Gp, const int* __restrict__ Gj,
                                                    const value_t* __restrict__ Gx, const int* __restrict__ src, ss_word* __restrict__ dist,
                                                    ss_word* __restrict__ done, unsigned* __restrict__ stamp, int* __restrict__ par,
                                                    int* __restrict__ ctl)
{
    bool bad = blockIdx.x == 0 && threadIdx.x == 0 && (Gp[0] != 0 || Gp[d.n] != d.nnzG);
    const ss_word inf = ss_inf();
    const long long total = (long long)gridDim.x * 256, gid = (long long)blockIdx.x * 256 + threadIdx.x;
    for (long long i = gid; i < d.n; i += total) {
        if (rd_bounds_bad(Gp[i], Gp[i + 1], d.nnzG)) bad = true;
        dist[i] = inf;
        done[i] = inf;
        stamp[i] = 0u;
        if (par) par[i] = kSsNoParent;
    }
    for (long long q = gid; q < d.nnzG; q += total) {                 // (the arrays hold nnzG entries)
        if ((unsigned)Gj[q] >= (unsigned)d.n) bad = true;
        if (d.hasVal) {
            const value_t w = Gx[q];
            if (w != w || w < (value_t)0) bad = true;                 // (-0 < 0 is false)
        }
    }
    for (long long s = gid; s < d.nsrc; s += total)
        if ((unsigned)src[s] >= (unsigned)d.n) bad = true;
    rd_flag(bad, ctl);
}

// the sources into slice 0 at distance 0, a repeated one once; the first bucket is [0, delta)
__global__ __launch_bounds__(256) void k_sssp_seed(SsDims d, const int* __restrict__ src, ss_word* __restrict__ dist, unsigned* stamp,
                                                   SsSlices sl, int* ctl)
{
    __shared__ int sGo;
    if (!sssp_go(ctl, false, &sGo)) return;
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        *(double*)(ctl + SSSP_BOUND) = ss_bound(0.0, d.delta);
        *(rd_u64*)(ctl + SSSP_MIN) = kSsNone;
        ctl[SSSP_BUCKETS] = 1;
    }
    bool bad = false;
    const long long total = (long long)gridDim.x * 256;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < d.nsrc; i += total) {
        const int s = src[i];
        if ((unsigned)s >= (unsigned)d.n) { bad = true; continue; }   // (never an index)
        if (atomicExch(stamp + s, 1u) == 1u) continue;
        const int at = atomicAdd(ctl + SSSP_LEN, 1);
        if ((unsigned)at >= (unsigned)d.n) { bad = true; continue; }  // (inside the slice)
        dist[s] = ss_bits((value_t)0);
        sl.q[0][at] = s;
        sl.sv[0][at] = ss_bits((value_t)0);
    }
    if (__ballot(bad) != 0ull && (threadIdx.x & 63) == 0) atomicOr(ctl + RD_ERR, 1);
}

// one out-edge (v, u, w) of a slice vertex at distance dv
__device__ __forceinline__ void ss_edge(const SsDims& d, value_t dv, int u, value_t w, double bound, unsigned tag, ss_word* dist,
                                        unsigned* stamp, int* next, int* ctl, bool& bad)
{
#pragma clang fp contract(off)
    if ((unsigned)u >= (unsigned)d.n) { bad = true; return; }         // (never an index)
    const value_t nd = dv + w;                                        // ONE rounding
    const ss_word nb = ss_bits(nd);
    if (!(nb < ss_load(dist + u))) return;                            // (a filter: +Inf lowers nothing)
    const ss_word old = atomicMin(dist + u, nb);
    if (!(nb < old) || !((double)nd < bound)) return;
    if (atomicExch(stamp + u, tag) == tag) return;                    // (appended in this pass already)
    const int at = atomicAdd(ctl + SSSP_APPEND, 1);
    if ((unsigned)at >= (unsigned)d.n) { bad = true; return; }        // (inside the slice)
    next[at] = u;
}

template <int L>
__global__ __launch_bounds__(256) void k_sssp_relax(SsDims d, const int* __restrict__ Gp, const int* __restrict__ Gj,
                                                    const value_t* __restrict__ Gx, ss_word* dist, ss_word* done, unsigned* stamp,
                                                    SsSlices sl, int* ctl)
{
    __shared__ int sGo, sCount, sLong[256 / L];
    __shared__ ss_word sLongD[256 / L];
    if (!sssp_go(ctl, false, &sGo)) return;                           // (uniform in the workgroup)
    const int sub = threadIdx.x & (L - 1);
    const int cur = ctl[SSSP_CUR] & 1, len = ctl[SSSP_LEN];
    const unsigned tag = (unsigned)ctl[SSSP_PASS] + 2u;               // (1: the seeds')
    const double bound = *(const double*)(ctl + SSSP_BOUND);
    const int* slice = sl.q[cur];
    const ss_word* sval = sl.sv[cur];
    int* next = sl.q[cur ^ 1];
    bool bad = len < 0 || len > d.n;
    const long long cnt = bad ? 0 : len;
    const long long nBlocks = (cnt + 256 / L - 1) / (256 / L);
    for (long long t = blockIdx.x; t < nBlocks; t += gridDim.x) {     // (uniform in the workgroup: every thread meets the barriers)
        if (threadIdx.x == 0) sCount = 0;
        __syncthreads();
        const long long it = t * (256 / L) + threadIdx.x / L;
        int a = 0, b = 0;
        value_t dv = (value_t)0;
        if (it < cnt) {
            const int v = slice[it];
            if ((unsigned)v >= (unsigned)d.n) bad = true;             // (never an index)
            else {
                const ss_word dvb = sval[it];
                if (dvb < done[v]) {                                  // (the L lanes read before lane 0 stores: one wave)
                    const int lo = Gp[v], hi = Gp[v + 1];
                    if (rd_bounds_bad(lo, hi, d.nnzG)) bad = true;
                    else {
                        if (sub == 0) done[v] = dvb;
                        if (hi - lo > kSsLong * L) {
                            if (sub == 0) {
                                const int at = atomicAdd(&sCount, 1); // (at most 256 / L vertices a turn)
                                sLong[at] = v;
                                sLongD[at] = dvb;
                            }
                        } else { a = lo; b = hi; dv = ss_value(dvb); }
                    }
                }
            }
        }
        for (int q = a + sub; q < b; q += L) ss_edge(d, dv, Gj[q], ss_weight(d, Gx, q), bound, tag, dist, stamp, next, ctl, bad);
        __syncthreads();
        const int nLong = sCount;
        for (int s = threadIdx.x >> 6; s < nLong; s += 4) {           // (a wave a listed row)
            const int w = sLong[s];                                   // (its row's bounds were checked where it was listed)
            const value_t dw = ss_value(sLongD[s]);
            const int lo = Gp[w], hi = Gp[w + 1];
            for (int q = lo + (int)(threadIdx.x & 63); q < hi; q += 64)
                ss_edge(d, dw, Gj[q], ss_weight(d, Gx, q), bound, tag, dist, stamp, next, ctl, bad);
        }
        __syncthreads();                                              // (the list is read before the next turn clears it)
    }
    rd_flag(bad, ctl);
}

__global__ __launch_bounds__(256) void k_sssp_min(SsDims d, const ss_word* __restrict__ dist, const ss_word* __restrict__ done, SsSlices sl,
                                                  int* ctl)
{
    __shared__ int sGo;
    __shared__ rd_u64 sMin;
    if (threadIdx.x == 0) sMin = kSsNone;
    if (!sssp_go(ctl, false, &sGo)) return;                           // (a barrier inside: sMin is set behind it)
    const int app = ctl[SSSP_APPEND];
    if (app != 0) {                                                   // the appended vertices' snapshots: no word moves now
        const int cur = ctl[SSSP_CUR] & 1;
        const int* next = sl.q[cur ^ 1];
        ss_word* nval = sl.sv[cur ^ 1];
        bool bad = app < 0 || app > d.n;
        const long long cnt = bad ? 0 : app;
        const long long nBlocks = (cnt + 255) / 256;
        for (long long t = blockIdx.x; t < nBlocks; t += gridDim.x) {
            const long long i = t * 256 + threadIdx.x;
            if (i < cnt) {
                const int u = next[i];
                if ((unsigned)u >= (unsigned)d.n) bad = true;         // (never an index)
                else nval[i] = dist[u];
            }
        }
        rd_flag(bad, ctl);
        return;
    }
    rd_u64 m = kSsNone;
    const long long nBlocks = ((long long)d.n + 255) / 256;
    for (long long t = blockIdx.x; t < nBlocks; t += gridDim.x) {
        const long long i = t * 256 + threadIdx.x;
        if (i < d.n) {
            const ss_word di = dist[i];
            if (di < done[i]) m = min(m, (rd_u64)di);
        }
    }
    if (m != kSsNone) (void)atomicMin(&sMin, m);
    __syncthreads();
    if (threadIdx.x == 0 && sMin != kSsNone) (void)atomicMin((rd_u64*)(ctl + SSSP_MIN), sMin);
}

__global__ __launch_bounds__(256) void k_sssp_gather(SsDims d, const ss_word* __restrict__ dist, const ss_word* __restrict__ done,
                                                     SsSlices sl, int* ctl)
{
    __shared__ int sGo;
    if (!sssp_go(ctl, true, &sGo)) return;
    const rd_u64 m = *(const rd_u64*)(ctl + SSSP_MIN);
    if (m == kSsNone) return;                                         // nothing is pending (uniform: no launch writes the word now)
    const int lane = threadIdx.x & 63;
    const int cur = ctl[SSSP_CUR] & 1;
    int* next = sl.q[cur ^ 1];
    ss_word* nval = sl.sv[cur ^ 1];
    const double bound = ss_bound((double)ss_value((ss_word)m), d.delta);
    bool bad = false;
    const long long nBlocks = ((long long)d.n + 255) / 256;
    for (long long t = blockIdx.x; t < nBlocks; t += gridDim.x) {     // (uniform in the workgroup: every lane votes)
        const long long i = t * 256 + threadIdx.x;
        bool take = false;
        ss_word di = 0;
        if (i < d.n) {
            di = dist[i];
            take = di < done[i] && ((double)ss_value(di) < bound || (rd_u64)di == m);
        }
        const unsigned long long votes = __ballot(take);
        if (votes == 0ull) continue;                                  // (uniform in the wave)
        const int first = __ffsll((long long)votes) - 1;
        int off = 0;
        if (lane == first) off = atomicAdd(ctl + SSSP_GATHERED, __popcll(votes));   // one add a wave
        off = __shfl(off, first);
        if (take) {
            const long long at = (long long)off + __popcll(votes & ((1ull << lane) - 1ull));
            if (off < 0 || at >= d.n) { bad = true; continue; }       // (inside the slice)
            next[at] = (int)i;
            nval[at] = di;
        }
    }
    rd_flag(bad, ctl);
}

__global__ __launch_bounds__(64) void k_sssp_advance(SsDims d, int* ctl)
{
    if (blockIdx.x != 0 || threadIdx.x != 0 || ctl[RD_ERR] || ctl[SSSP_DONE]) return;
    const int app = ctl[SSSP_APPEND], g = ctl[SSSP_GATHERED];
    if (app < 0 || app > d.n || g < 0 || g > d.n || (app != 0 && g != 0)) { atomicOr(ctl + RD_ERR, 1); return; }
    int next = app;
    if (app == 0 && g > 0) {                                          // the jump ran: the bucket that holds the minimum
        const rd_u64 m = *(const rd_u64*)(ctl + SSSP_MIN);
        if (m == kSsNone) { atomicOr(ctl + RD_ERR, 1); return; }
        *(double*)(ctl + SSSP_BOUND) = ss_bound((double)ss_value((ss_word)m), d.delta);
        ctl[SSSP_BUCKETS] += 1;
        next = g;
    }
    ctl[SSSP_CUR] = (ctl[SSSP_CUR] & 1) ^ 1;
    ctl[SSSP_LEN] = next;
    ctl[SSSP_APPEND] = 0;
    ctl[SSSP_GATHERED] = 0;
    *(rd_u64*)(ctl + SSSP_MIN) = kSsNone;
    ctl[SSSP_PASS] += 1;
    if (next == 0) ctl[SSSP_DONE] = 1;                                // no slice: nothing was pending either
    *(long long*)(ctl + AG_UNDEC) = next;
}

// one edge (u, v, w) behind the fixed point: u is v's parent where the edge is tight and u strictly closer, the least such u
__device__ __forceinline__ void ss_tight(const SsDims& d, int u, ss_word du, int v, value_t w, const ss_word* __restrict__ dist, int* par,
                                         bool& bad)
{
#pragma clang fp contract(off)
    if ((unsigned)v >= (unsigned)d.n) { bad = true; return; }         // (never an index)
    const ss_word to = dist[v];
    const value_t nd = ss_value(du) + w;
    if (ss_bits(nd) == to && du < to && par[v] > u) (void)atomicMin(par + v, u);
}

// the fixed point stands: par[v] = the least u with an edge (u, v), fl(d[u] + w) == d[v] and d[u] < d[v]; the rows as the
// relax walks them, a row beyond kSsLong entries a lane by a whole wave
template <int L>
__global__ __launch_bounds__(256) void k_sssp_parents(SsDims d, const int* __restrict__ Gp, const int* __restrict__ Gj,
                                                      const value_t* __restrict__ Gx, const ss_word* __restrict__ dist, int* par,
                                                      int* __restrict__ ctl)
{
    __shared__ int sCount, sLong[256 / L];
    if (ctl[RD_ERR]) return;                                          // (uniform: no launch writes the word now)
    const int sub = threadIdx.x & (L - 1);
    bool bad = false;
    AgDims ad;
    ad.n = d.n; ad.nnzS = d.nnzG; ad.seed = 0; ad.hasPrio = 0;
    const ss_word inf = ss_inf();
    const long long nBlocks = ((long long)d.n + 256 / L - 1) / (256 / L);
    for (long long t = blockIdx.x; t < nBlocks; t += gridDim.x) {     // (uniform in the workgroup: every thread meets the barriers)
        if (threadIdx.x == 0) sCount = 0;
        __syncthreads();
        int a, b;
        const long long i = ag_row<L>(ad, Gp, t, a, b, bad);
        ss_word du = inf;
        if (i < d.n) du = dist[i];
        if (du == inf) a = b = 0;                                     // not reached: no edge of it is tight
        else if (b - a > kSsLong * L) {
            if (sub == 0) sLong[atomicAdd(&sCount, 1)] = (int)i;      // (at most 256 / L rows a turn)
            a = b = 0;
        }
        for (int q = a + sub; q < b; q += L) ss_tight(d, (int)i, du, Gj[q], ss_weight(d, Gx, q), dist, par, bad);
        __syncthreads();
        const int nLong = sCount;
        for (int s = threadIdx.x >> 6; s < nLong; s += 4) {           // (a wave a listed row)
            const int u = sLong[s];                                   // (its row's bounds were checked where it was listed)
            const ss_word dw = dist[u];
            const int lo = Gp[u], hi = Gp[u + 1];
            for (int q = lo + (int)(threadIdx.x & 63); q < hi; q += 64) ss_tight(d, u, dw, Gj[q], ss_weight(d, Gx, q), dist, par, bad);
        }
        __syncthreads();                                              // (the list is read before the next turn clears it)
    }
    rd_flag(bad, ctl);
}

// a source has no parent
__global__ __launch_bounds__(256) void k_sssp_roots(SsDims d, const int* __restrict__ src, int* __restrict__ par, int* __restrict__ ctl)
{
    if (ctl[RD_ERR]) return;
    const long long total = (long long)gridDim.x * 256;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < d.nsrc; i += total) {
        const int s = src[i];
        if ((unsigned)s < (unsigned)d.n) par[s] = -1;                 // (the check accepted it)
    }
}

// the only writer of the outputs: the distances, the parents (-1 a source or not reached, -2 reached over no tight edge from
// a smaller distance), and the two counts
__global__ __launch_bounds__(256) void k_sssp_finish(SsDims d, const ss_word* __restrict__ dist, const int* __restrict__ par,
                                                     value_t* __restrict__ outDist, int* __restrict__ outPar, int* ctl)
{
    if (ctl[RD_ERR]) return;
    const ss_word inf = ss_inf();
    int reached = 0, loose = 0;
    const long long nBlocks = ((long long)d.n + 255) / 256;
    for (long long t = blockIdx.x; t < nBlocks; t += gridDim.x) {     // (uniform in the workgroup: every lane votes)
        const long long i = t * 256 + threadIdx.x;
        bool r = false, l = false;
        if (i < d.n) {
            const ss_word di = dist[i];
            outDist[i] = ss_value(di);
            r = di != inf;
            if (outPar) {
                const int p = par[i];
                l = r && p == kSsNoParent;
                outPar[i] = !r ? -1 : l ? -2 : p;
            }
        }
        reached += __popcll(__ballot(r));
        loose += __popcll(__ballot(l));
    }
    if ((threadIdx.x & 63) == 0) {
        if (reached) atomicAdd(ctl + SSSP_REACHED, reached);
        if (loose) atomicAdd(ctl + SSSP_LOOSE, loose);
    }
}

}  // namespace bhs
