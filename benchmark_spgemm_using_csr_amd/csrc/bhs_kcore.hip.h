// bhs_kcore.hip.h -- the k-core decomposition of an n x n pattern S with ascending rows and a symmetric structure by a
// work-efficient frontier peel (bhs_csr_kcore_device; the contract is worded in include/bhsparse_hip.h, "k-core
// decomposition").  Values are never taken: the same code, and the same result bit for bit, in the double and the float library.
//
// deg[v] starts as the entries of row v off the diagonal (k_rcm_check, unchanged, which also refuses what the contract
// refuses).  Every vertex enters ONE queue of n ints exactly once; a round's vertices are a slice [head, tail) of it.  The
// order INSIDE a slice DEPENDS ON TIMING and is no output; which vertices a slice holds does not.  A vertex is PRESENT while
// deg[v] > k: it leaves with deg[v] <= k, and a degree only ever falls (never below 0: an entry is walked once).
//
// A pass is four launches with no host decision between them:
//
//   k_core_peel<L>    over the slice, L lanes a vertex, a row beyond 32 entries a lane by a whole wave: for a frontier
//                     vertex v and every neighbour u != v, old = atomicSub(deg + u, 1), unconditionally.  The ONE thread
//                     that sees old == k + 1 appends u behind the queue's filled part (an atomicAdd on a control word
//                     hands out the place) and stores core[u] = k and round[u] = r + 1: the only writer these words ever
//                     have, with plain stores.  A present vertex has deg > k when the pass starts and each decrement
//                     returns a value of its own, so it crosses k + 1 exactly once if it ends at or below k -- however
//                     many neighbours it loses -- and never otherwise; a vertex that has left is at or below k already
//                     and only sinks.
//   k_core_min        where the peel appended nothing and vertices remain (else every workgroup leaves at once): the
//                     smallest degree among the present vertices, an integer atomicMin a workgroup on a control word.
//   k_core_gather     under the same condition: every present vertex of that degree is appended and stamped with it -- the
//                     level jump, so empty levels cost nothing.  The call's first frontier comes from this pair (k = -1).
//   k_core_advance    ONE thread: the appended range becomes the next slice, k takes the jump's level, the round counts on
//                     where the slice is not empty, and the vertices still present go where the host's loop reads its count.
//                     No other workgroup runs beside it, and no kernel reads a control word that its own launch writes
//                     except the places handed out by atomicAdd and the error word.
//
// Every grid is capped and every kernel walks its blocks in a loop; nothing spins, nothing waits for another workgroup, every
// loop is bounded.  Whatever is read from device memory and then used as an index is checked first and raises ctl[RD_ERR]
// instead: the slice's bounds, a queue entry, a row's bounds (rd_bounds_bad), a column, a place handed out.  Once the word is
// up -- by the check's refusal, before any output is written -- every later launch leaves at once.  The atomics are integer
// atomics on the workspace alone; no output is written by an atomic.
#pragma once
#include "bhs_rcm.hip.h"

namespace bhs {

// control words: bhs_aggregate.hip.h's; behind them the level k, the slice [head, tail), the place the peel appends at, the
// vertices the gather appended, the smallest present degree, and the slice's round.  The vertices still present are counted
// where the passes count (AG_UNDEC, 64 bits).
enum { CORE_K = AG_INTS, CORE_HEAD, CORE_TAIL, CORE_APPEND, CORE_GATHERED, CORE_MIN, CORE_ROUND, CORE_INTS = AG_INTS + 8 };

constexpr int kCoreNone = 0x7fffffff;                                 // no present vertex seen yet

// does this launch run: one read of the words a workgroup, so that all its threads agree
__device__ __forceinline__ bool core_go(const int* ctl, int n, bool jump, int* sGo)
{
    if (threadIdx.x == 0) {
        const int app = ctl[CORE_APPEND];
        *sGo = ctl[RD_ERR] == 0 && (!jump || (app == ctl[CORE_TAIL] && app < n));
    }
    __syncthreads();
    return *sGo != 0;
}

// the call's start: no level yet, so every vertex is present; the first pass's peel finds an empty slice
__global__ __launch_bounds__(64) void k_core_begin(int* ctl)
{
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        ctl[CORE_K] = -1;
        ctl[CORE_MIN] = kCoreNone;
    }
}

// one entry (v, u) of a frontier vertex v: u's degree drops, and the one thread that sees it cross k + 1 appends and stamps u
__device__ __forceinline__ void core_drop(const AgDims& d, int v, int u, int k, int r, int tail, int* deg, int* queue,
                                          int* __restrict__ core, int* __restrict__ round, int* ctl, bool& bad)
{
    if ((unsigned)u >= (unsigned)d.n) { bad = true; return; }         // (never an index)
    if (u == v) return;
    const int old = atomicSub(deg + u, 1);
    if (old != k + 1) return;
    const int at = atomicAdd(ctl + CORE_APPEND, 1);                   // u leaves: this thread alone saw it cross
    if (at < tail || at >= d.n) { bad = true; return; }               // (behind the slice, inside the queue)
    queue[at] = u;
    core[u] = k;
    if (round) round[u] = r;
}

// A row of more than kCoreLong entries a lane is not walked by its L lanes: its vertex goes to a list in LDS, and behind a
// barrier the workgroup's four waves take the listed rows in turn, a wave a row, 64 entries a step.
constexpr int kCoreLong = 32;

template <int L>
__global__ __launch_bounds__(256) void k_core_peel(AgDims d, const int* __restrict__ Sp, const int* __restrict__ Sj, int* deg, int* queue,
                                                   int* __restrict__ core, int* __restrict__ round, int* ctl)
{
    __shared__ int sGo, sCount, sLong[256 / L];
    if (!core_go(ctl, d.n, false, &sGo)) return;                      // (uniform in the workgroup)
    const int sub = threadIdx.x & (L - 1);
    const int head = ctl[CORE_HEAD], tail = ctl[CORE_TAIL], k = ctl[CORE_K], r = ctl[CORE_ROUND] + 1;
    bool bad = head < 0 || tail < head || tail > d.n;
    const long long cnt = bad ? 0 : (long long)tail - head;
    const long long nBlocks = (cnt + 256 / L - 1) / (256 / L);
    for (long long t = blockIdx.x; t < nBlocks; t += gridDim.x) {     // (uniform in the workgroup: every thread meets the barriers)
        if (threadIdx.x == 0) sCount = 0;
        __syncthreads();
        const long long it = t * (256 / L) + threadIdx.x / L;
        int v = -1, a = 0, b = 0;
        if (it < cnt) {
            v = queue[head + it];
            if ((unsigned)v >= (unsigned)d.n) bad = true;             // (never an index)
            else {
                const int lo = Sp[v], hi = Sp[v + 1];
                if (rd_bounds_bad(lo, hi, d.nnzS)) bad = true;
                else if (hi - lo > kCoreLong * L) {
                    if (sub == 0) sLong[atomicAdd(&sCount, 1)] = v;   // (at most 256 / L vertices a turn)
                } else { a = lo; b = hi; }
            }
        }
        for (int q = a + sub; q < b; q += L) core_drop(d, v, Sj[q], k, r, tail, deg, queue, core, round, ctl, bad);
        __syncthreads();
        const int nLong = sCount;
        for (int s = threadIdx.x >> 6; s < nLong; s += 4) {           // (a wave a listed row)
            const int w = sLong[s];                                   // (its row's bounds were checked where it was listed)
            const int lo = Sp[w], hi = Sp[w + 1];
            for (int q = lo + (int)(threadIdx.x & 63); q < hi; q += 64) core_drop(d, w, Sj[q], k, r, tail, deg, queue, core, round, ctl, bad);
        }
        __syncthreads();                                              // (the list is read before the next turn clears it)
    }
    rd_flag(bad, ctl);
}

__global__ __launch_bounds__(256) void k_core_min(int n, const int* __restrict__ deg, int* ctl)
{
    __shared__ int sGo, sMin;
    if (threadIdx.x == 0) sMin = kCoreNone;
    if (!core_go(ctl, n, true, &sGo)) return;                         // (a barrier inside: sMin is set behind it)
    const int k = ctl[CORE_K];
    int m = kCoreNone;
    const long long nBlocks = ((long long)n + 255) / 256;
    for (long long t = blockIdx.x; t < nBlocks; t += gridDim.x) {
        const long long i = t * 256 + threadIdx.x;
        if (i < n) {
            const int dg = deg[i];
            if (dg > k) m = min(m, dg);
        }
    }
    if (m != kCoreNone) (void)atomicMin(&sMin, m);
    __syncthreads();
    if (threadIdx.x == 0 && sMin != kCoreNone) (void)atomicMin(ctl + CORE_MIN, sMin);
}

__global__ __launch_bounds__(256) void k_core_gather(int n, const int* __restrict__ deg, int* queue, int* __restrict__ core,
                                                     int* __restrict__ round, int* ctl)
{
    __shared__ int sGo;
    if (!core_go(ctl, n, true, &sGo)) return;
    const int lane = threadIdx.x & 63;
    const int k = ctl[CORE_K], kn = ctl[CORE_MIN], base = ctl[CORE_APPEND], r = ctl[CORE_ROUND] + 1;
    bool bad = kn <= k || kn == kCoreNone || base < 0;                // (vertices remain: one of them has the least degree)
    const long long nBlocks = bad ? 0 : ((long long)n + 255) / 256;
    for (long long t = blockIdx.x; t < nBlocks; t += gridDim.x) {     // (uniform in the workgroup: every lane votes)
        const long long i = t * 256 + threadIdx.x;
        bool take = false;
        if (i < n) {
            const int dg = deg[i];
            take = dg > k && dg <= kn;
        }
        const unsigned long long votes = __ballot(take);
        if (votes == 0ull) continue;                                  // (uniform in the wave)
        const int first = __ffsll((long long)votes) - 1;
        int off = 0;
        if (lane == first) off = atomicAdd(ctl + CORE_GATHERED, __popcll(votes));   // one add a wave
        off = __shfl(off, first);
        if (take) {
            const long long at = (long long)base + off + __popcll(votes & ((1ull << lane) - 1ull));
            if (off < 0 || at >= n) { bad = true; continue; }         // (inside the queue)
            queue[at] = (int)i;
            core[i] = kn;
            if (round) round[i] = r;
        }
    }
    rd_flag(bad, ctl);
}

__global__ __launch_bounds__(64) void k_core_advance(int n, int* ctl)
{
    if (blockIdx.x != 0 || threadIdx.x != 0 || ctl[RD_ERR]) return;
    const int tail = ctl[CORE_TAIL], app = ctl[CORE_APPEND];
    int next = app;
    if (app == tail && app < n) {                                     // the jump ran
        const int g = ctl[CORE_GATHERED];
        if (g < 1 || g > n - app) { atomicOr(ctl + RD_ERR, 1); return; }
        ctl[CORE_K] = ctl[CORE_MIN];
        next = app + g;
    }
    if (next < tail || next > n) { atomicOr(ctl + RD_ERR, 1); return; }
    ctl[CORE_HEAD] = tail;
    ctl[CORE_TAIL] = next;
    ctl[CORE_APPEND] = next;
    ctl[CORE_GATHERED] = 0;
    ctl[CORE_MIN] = kCoreNone;
    if (next > tail) ctl[CORE_ROUND] += 1;
    *(long long*)(ctl + AG_UNDEC) = (long long)n - next;              // the vertices still present
}

}  // namespace bhs
