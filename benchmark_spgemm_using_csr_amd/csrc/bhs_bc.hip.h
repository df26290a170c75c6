// bhs_bc.hip.h -- betweenness centrality by Brandes' algorithm, a source after the other, over the out-edges G of an n-vertex
// graph and its in-edges T (bhs_csr_betweenness_device; the contract is worded in include/bhsparse_hip.h, "betweenness
// centrality").  Values are never taken and every number is a double: the same code, and the same result bit for bit, in the
// double and the float library.
//
// Per source every reached vertex enters ONE queue of n ints exactly once; level l is the slice [levelPtr[l], levelPtr[l + 1])
// of it.  The order INSIDE a slice DEPENDS ON TIMING and is no output; which vertices a slice holds does not.  sigma and delta
// have ONE writer a word -- the group of lanes that owns the vertex -- and a fixed summation order (bc_fold), so they are
// functions of the input however the queue is ordered.
//
//   k_bc_check        refuses what the contract refuses: both row pointers, every column of both matrices entry by entry,
//                     every source.
//   k_bc_seed         level = -1, sigma = delta = 0 everywhere but level[s] = 0, sigma[s] = 1; the source is slice 0; on the
//                     call's first source without BHS_BC_ACCUMULATE d_bc = 0.
//   k_bc_expand<L>    over slice l, L lanes a vertex, a row of G beyond 32 entries a lane by a whole wave: the thread whose
//                     atomicCAS turns level[v] from -1 into l + 1 appends v behind the queue's filled part, at a place an
//                     atomicAdd on a control word hands out.
//   k_bc_count<L>     over the appended range, L lanes a vertex, rows of T: sigma[v] = the sum of sigma[u] over the entries u
//                     with level[u] == l.  No atomic but the flag of a sigma that is not finite.
//   k_bc_advance      ONE thread: levelPtr[l + 2], the appended range becomes the next slice and its length goes where the
//                     host's loop reads its count; a pass that appended nothing ends the source: the deepest level, the
//                     reached vertices and the overflow are counted, and every later pass leaves at once.
//   k_bc_back<L>      for l = deepest - 1 down to 1, a launch each with no host decision between them, over slice l, rows of G:
//                     delta[u] = sigma[u] * the sum of (1 + delta[v]) / sigma[v] over the entries v with level[v] == l + 1, and
//                     bc[u] = bc[u] + delta[u], plain stores by u's own group.
//   k_bc_finish       behind the last source: level and sigma to the caller where asked for.
//
// Every grid is capped and every kernel walks its blocks in a loop; nothing spins, nothing waits for another workgroup, every
// loop is bounded.  Whatever is read from device memory and then used as an index is checked first and raises ctl[RD_ERR]
// instead: a slice's bounds, a queue entry, a row's bounds (rd_bounds_bad), a column, a source, a place handed out.  Once the
// word is up -- by the check's refusal, before any output is written -- every later launch leaves at once.  The atomics are
// integer atomics on the workspace alone; no output is written by an atomic.
#pragma once
#include "bhs_sssp.hip.h"

namespace bhs {

// control words: bhs_aggregate.hip.h's; behind them the slice [head, tail), the place the expand appends at, the slice's
// level, the source's end and its deepest level, the flag of a sigma that is not finite, the call's end, and four 64-bit
// counts over the sources: the reached vertices, the levels, the sources that overflowed, the passes that had a slice.  The
// next slice's length is counted where the passes count (AG_UNDEC, 64 bits).
enum { BC_HEAD = AG_INTS, BC_TAIL, BC_APPEND, BC_LEVEL, BC_DONE, BC_DEEPEST, BC_INF, BC_FINISHED, BC_REACHED = AG_INTS + 8,
       BC_LEVELS = AG_INTS + 10, BC_OVERFLOW = AG_INTS + 12, BC_WORK = AG_INTS + 14, BC_INTS = AG_INTS + 16 };
static_assert(BC_REACHED % 2 == 0, "64-bit control words");

constexpr int kBcLong = kCoreLong;                                    // a row of more entries a lane goes to a whole wave
constexpr rd_u64 kBcNaN = 0x7ff8000000000000ull;                      // the one NaN the call stores

struct BcDims {
    int n, nnzG, nnzT, nsrc;
};

// the workspace: level, queue, levelPtr (n + 2) as ints, sigma and delta as doubles
struct BcWork {
    int* level; int* queue; int* levelPtr;
    double* sigma; double* delta;
};

// every NaN as kBcNaN: the word does not depend on what the hardware gives an invalid operation
__device__ __forceinline__ double bc_canon(double x)
{
    if (x != x) __builtin_memcpy(&x, &kBcNaN, sizeof(x));
    return x;
}

// the lane sums of W lanes combined by the xor butterfly: every lane of the group ends with the same word
template <int W>
__device__ __forceinline__ double bc_fold(double t)
{
#pragma clang fp contract(off)
#pragma unroll
    for (int off = W / 2; off >= 1; off >>= 1) t = t + __shfl_xor(t, off);
    return t;
}

// does this launch run: one read of the words a workgroup, so that all its threads agree
__device__ __forceinline__ bool bc_go(const int* ctl, int* sGo)
{
    if (threadIdx.x == 0) *sGo = ctl[RD_ERR] == 0 && ctl[BC_DONE] == 0;
    __syncthreads();
    return *sGo != 0;
}

// The check: both row pointers (their ends, every row's bounds), every source, and -- entry by entry, whatever row it lies
// in, so that a hub row costs what its entries cost -- every column of both matrices.
__global__ __launch_bounds__(256) void k_bc_check(BcDims d, const int* __restrict__ Gp, const int* __restrict__ Gj,
                                                  const int* __restrict__ Tp, const int* __restrict__ Tj, const int* __restrict__ src,
                                                  int* __restrict__ ctl)
{
    bool bad = blockIdx.x == 0 && threadIdx.x == 0 && (Gp[0] != 0 || Gp[d.n] != d.nnzG || Tp[0] != 0 || Tp[d.n] != d.nnzT);
    const long long total = (long long)gridDim.x * 256, gid = (long long)blockIdx.x * 256 + threadIdx.x;
    for (long long i = gid; i < d.n; i += total)
        if (rd_bounds_bad(Gp[i], Gp[i + 1], d.nnzG) || rd_bounds_bad(Tp[i], Tp[i + 1], d.nnzT)) bad = true;
    for (long long q = gid; q < d.nnzG; q += total)                   // (the arrays hold nnzG and nnzT entries)
        if ((unsigned)Gj[q] >= (unsigned)d.n) bad = true;
    for (long long q = gid; q < d.nnzT; q += total)
        if ((unsigned)Tj[q] >= (unsigned)d.n) bad = true;
    for (long long s = gid; s < d.nsrc; s += total)
        if ((unsigned)src[s] >= (unsigned)d.n) bad = true;
    rd_flag(bad, ctl);
}

// source number si starts: the workspace, slice 0, and d_bc where this is the call's first source and it is not added to
__global__ __launch_bounds__(256) void k_bc_seed(BcDims d, const int* __restrict__ src, int si, int zero, BcWork w, double* __restrict__ bc,
                                                 int* ctl)
{
    if (ctl[RD_ERR]) return;                                          // (uniform: this launch raises the word only for a source the check accepted)
    const int s = src[si];
    if ((unsigned)s >= (unsigned)d.n) {                               // (never an index)
        if (blockIdx.x == 0 && threadIdx.x == 0) atomicOr(ctl + RD_ERR, 1);
        return;
    }
    const long long total = (long long)gridDim.x * 256;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < d.n; i += total) {
        w.level[i] = i == s ? 0 : -1;
        w.sigma[i] = i == s ? 1.0 : 0.0;
        w.delta[i] = 0.0;
        if (zero) bc[i] = 0.0;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        w.queue[0] = s;
        w.levelPtr[0] = 0;
        w.levelPtr[1] = 1;
        ctl[BC_HEAD] = 0;
        ctl[BC_TAIL] = 1;
        ctl[BC_APPEND] = 1;
        ctl[BC_LEVEL] = 0;
        ctl[BC_DEEPEST] = 0;
        ctl[BC_INF] = 0;
        ctl[BC_DONE] = 0;
    }
}

// one out-edge (u, v) of a slice vertex: the thread that turns level[v] from -1 into next appends v
__device__ __forceinline__ void bc_claim(const BcDims& d, int v, int next, int tail, const BcWork& w, int* ctl, bool& bad)
{
    if ((unsigned)v >= (unsigned)d.n) { bad = true; return; }         // (never an index)
    if (__hip_atomic_load(w.level + v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != -1) return;   // (a filter)
    if (atomicCAS(w.level + v, -1, next) != -1) return;
    const int at = atomicAdd(ctl + BC_APPEND, 1);                     // v is reached: this thread alone saw it turn
    if (at < tail || at >= d.n) { bad = true; return; }               // (behind the slice, inside the queue)
    w.queue[at] = v;
}

template <int L>
__global__ __launch_bounds__(256) void k_bc_expand(BcDims d, const int* __restrict__ Gp, const int* __restrict__ Gj, BcWork w, int* ctl)
{
    __shared__ int sGo, sCount, sLong[256 / L];
    if (!bc_go(ctl, &sGo)) return;                                    // (uniform in the workgroup)
    const int sub = threadIdx.x & (L - 1);
    const int head = ctl[BC_HEAD], tail = ctl[BC_TAIL], lev = ctl[BC_LEVEL];
    bool bad = head < 0 || tail < head || tail > d.n || lev < 0 || lev >= d.n;
    const long long cnt = bad ? 0 : (long long)tail - head;
    const long long nBlocks = (cnt + 256 / L - 1) / (256 / L);
    for (long long t = blockIdx.x; t < nBlocks; t += gridDim.x) {     // (uniform in the workgroup: every thread meets the barriers)
        if (threadIdx.x == 0) sCount = 0;
        __syncthreads();
        const long long it = t * (256 / L) + threadIdx.x / L;
        int a = 0, b = 0;
        if (it < cnt) {
            const int u = w.queue[head + it];
            if ((unsigned)u >= (unsigned)d.n) bad = true;             // (never an index)
            else {
                const int lo = Gp[u], hi = Gp[u + 1];
                if (rd_bounds_bad(lo, hi, d.nnzG)) bad = true;
                else if (hi - lo > kBcLong * L) {
                    if (sub == 0) sLong[atomicAdd(&sCount, 1)] = u;   // (at most 256 / L vertices a turn)
                } else { a = lo; b = hi; }
            }
        }
        for (int q = a + sub; q < b; q += L) bc_claim(d, Gj[q], lev + 1, tail, w, ctl, bad);
        __syncthreads();
        const int nLong = sCount;
        for (int s = threadIdx.x >> 6; s < nLong; s += 4) {           // (a wave a listed row)
            const int u = sLong[s];                                   // (its row's bounds were checked where it was listed)
            const int lo = Gp[u], hi = Gp[u + 1];
            for (int q = lo + (int)(threadIdx.x & 63); q < hi; q += 64) bc_claim(d, Gj[q], lev + 1, tail, w, ctl, bad);
        }
        __syncthreads();                                              // (the list is read before the next turn clears it)
    }
    rd_flag(bad, ctl);
}

// what entry q of a row gives its lane's sum.  BACK: (1 + delta[v]) / sigma[v] where level[v] == want, a true division;
// else sigma[u] where level[u] == want; nothing otherwise
template <bool BACK>
__device__ __forceinline__ double bc_term(const BcDims& d, int c, int want, const BcWork& w, double t, bool& bad)
{
#pragma clang fp contract(off)
    if ((unsigned)c >= (unsigned)d.n) { bad = true; return t; }       // (never an index)
    if (w.level[c] != want) return t;
    if constexpr (BACK) {
        const double one = 1.0 + w.delta[c];
        return t + one / w.sigma[c];
    } else
        return t + w.sigma[c];
}

// The sums of a slice [from, from + cnt) of the queue over the rows of X = (Xp, Xj), by the contract's rule: L lanes a row,
// lane p mod L takes entry p, ascending, from +0; a row of more than kBcLong * L entries takes a wave, lane p mod 64; the lane
// sums fold by the xor butterfly.  store(vertex, sum) runs on ONE lane a vertex.
template <int L, bool BACK, typename F>
__device__ __forceinline__ void bc_rows(const BcDims& d, const int* __restrict__ Xp, const int* __restrict__ Xj, int nnzX, int from,
                                        long long cnt, int want, const BcWork& w, int* sCount, int* sLong, bool& bad, F&& store)
{
    const int sub = threadIdx.x & (L - 1);
    const long long nBlocks = (cnt + 256 / L - 1) / (256 / L);
    for (long long t = blockIdx.x; t < nBlocks; t += gridDim.x) {     // (uniform in the workgroup: every thread meets the barriers)
        if (threadIdx.x == 0) *sCount = 0;
        __syncthreads();
        const long long it = t * (256 / L) + threadIdx.x / L;
        int x = -1, a = 0, b = 0;
        if (it < cnt) {
            const int v = w.queue[from + it];
            if ((unsigned)v >= (unsigned)d.n) bad = true;             // (never an index)
            else {
                const int lo = Xp[v], hi = Xp[v + 1];
                if (rd_bounds_bad(lo, hi, nnzX)) bad = true;
                else if (hi - lo > kBcLong * L) {
                    if (sub == 0) sLong[atomicAdd(sCount, 1)] = v;    // (at most 256 / L vertices a turn)
                } else { x = v; a = lo; b = hi; }
            }
        }
        double acc = 0.0;
        for (int q = a + sub; q < b; q += L) acc = bc_term<BACK>(d, Xj[q], want, w, acc, bad);
        acc = bc_fold<L>(acc);                                        // (every lane of the wave is here)
        if (x >= 0 && sub == 0) store(x, acc);
        __syncthreads();
        const int nLong = *sCount;
        for (int s = threadIdx.x >> 6; s < nLong; s += 4) {           // (a wave a listed row)
            const int v = sLong[s];                                   // (its row's bounds were checked where it was listed)
            const int lo = Xp[v], hi = Xp[v + 1];
            double sum = 0.0;
            for (int q = lo + (int)(threadIdx.x & 63); q < hi; q += 64) sum = bc_term<BACK>(d, Xj[q], want, w, sum, bad);
            sum = bc_fold<64>(sum);
            if ((threadIdx.x & 63) == 0) store(v, sum);
        }
        __syncthreads();                                              // (the list is read before the next turn clears it)
    }
}

// the path counts of the vertices the expand appended: pulled over the rows of T, one writer a word
template <int L>
__global__ __launch_bounds__(256) void k_bc_count(BcDims d, const int* __restrict__ Tp, const int* __restrict__ Tj, BcWork w, int* ctl)
{
    __shared__ int sGo, sCount, sLong[256 / L];
    if (!bc_go(ctl, &sGo)) return;                                    // (uniform in the workgroup)
    const int tail = ctl[BC_TAIL], app = ctl[BC_APPEND], lev = ctl[BC_LEVEL];
    bool bad = tail < 0 || app < tail || app > d.n || lev < 0 || lev >= d.n;
    bool inf = false;
    bc_rows<L, false>(d, Tp, Tj, d.nnzT, tail, bad ? 0 : (long long)app - tail, lev, w, &sCount, sLong, bad, [&](int v, double s) {
        w.sigma[v] = s;
        if (!(s - s == 0.0)) inf = true;                              // +Inf (a sum of words that are not negative is never NaN)
    });
    if (__ballot(inf) != 0ull && (threadIdx.x & 63) == 0) atomicOr(ctl + BC_INF, 1);
    rd_flag(bad, ctl);
}

__global__ __launch_bounds__(64) void k_bc_advance(BcDims d, BcWork w, int* ctl)
{
    if (blockIdx.x != 0 || threadIdx.x != 0 || ctl[RD_ERR] || ctl[BC_DONE]) return;
    const int tail = ctl[BC_TAIL], app = ctl[BC_APPEND], lev = ctl[BC_LEVEL];
    if (tail < 1 || app < tail || app > d.n || lev < 0 || lev >= d.n) { atomicOr(ctl + RD_ERR, 1); return; }
    *(long long*)(ctl + BC_WORK) += 1;
    if (app > tail) {                                                 // level lev + 1 is [tail, app)
        w.levelPtr[lev + 2] = app;
        ctl[BC_HEAD] = tail;
        ctl[BC_TAIL] = app;
        ctl[BC_LEVEL] = lev + 1;
    } else {                                                          // nothing new: lev is the deepest level
        ctl[BC_DONE] = 1;
        ctl[BC_DEEPEST] = lev;
        *(long long*)(ctl + BC_REACHED) += tail;
        *(long long*)(ctl + BC_LEVELS) += (long long)lev + 1;
        if (ctl[BC_INF]) *(long long*)(ctl + BC_OVERFLOW) += 1;
    }
    *(long long*)(ctl + AG_UNDEC) = (long long)app - tail;
}

// level lev's dependencies, and what they add to d_bc: 0 < lev < the deepest level, so the source is not among them
template <int L>
__global__ __launch_bounds__(256) void k_bc_back(BcDims d, const int* __restrict__ Gp, const int* __restrict__ Gj, int lev, BcWork w,
                                                 double* __restrict__ bc, int* ctl)
{
    __shared__ int sCount, sLong[256 / L];
    if (ctl[RD_ERR]) return;                                          // (uniform: the word is raised behind the walk only)
    bool bad = lev < 1 || lev >= d.n;
    int head = 0, tail = 0;
    if (!bad) {
        head = w.levelPtr[lev];
        tail = w.levelPtr[lev + 1];
        bad = head < 1 || tail < head || tail > d.n;
    }
    bc_rows<L, true>(d, Gp, Gj, d.nnzG, head, bad ? 0 : (long long)tail - head, lev + 1, w, &sCount, sLong, bad, [&](int u, double s) {
#pragma clang fp contract(off)
        const double dl = bc_canon(w.sigma[u] * s);
        w.delta[u] = dl;
        const double sum = bc[u] + dl;
        bc[u] = bc_canon(sum);
    });
    rd_flag(bad, ctl);
}

// behind the last source: its levels and path counts to the caller where asked for, with plain stores
__global__ __launch_bounds__(256) void k_bc_finish(BcDims d, BcWork w, int* __restrict__ outLevel, double* __restrict__ outSigma, int* ctl)
{
    if (ctl[RD_ERR] || ctl[BC_DONE] != 1) return;
    const long long total = (long long)gridDim.x * 256;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < d.n; i += total) {
        if (outLevel) outLevel[i] = w.level[i];
        if (outSigma) outSigma[i] = w.sigma[i];
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) ctl[BC_FINISHED] = 1;
}

}  // namespace bhs
