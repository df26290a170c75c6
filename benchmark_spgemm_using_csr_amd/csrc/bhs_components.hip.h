// bhs_components.hip.h -- the connected components of an n x n pattern S, weakly: i and j are joined where S stores (i, j) or
// (j, i) (bhs_csr_components_device; the contract is worded in include/bhsparse_hip.h, "connected components").  Values are
// never taken: the same code, and the same result bit for bit, in the double and the float library.
//
// One int a vertex, its parent, in the caller's d_root itself.  Three invariants hold at every instant:
//   (I1) parent[v] <= v;  (I2) parent[v] lies in v's component;  (I3) a word only ever falls.
// I3 is why every write after k_cc_init is an atomicMin, the shortcut included: a plain store of parent[parent[i]] could
// raise a word that another lane lowered in between.  The value the atomic returns tells whether the word fell.
//
//   k_cc_init      parent[i] = i.
//   k_cc_pass<L>   one pass, in place, a row over L = 1, 4, 16 or 64 lanes.  A lane carries a running minimum m that starts
//                  at parent[i]; for each of its entries j != i it reads parent[j] and lowers parent[j] to m where it is
//                  greater, else takes it as m -- so after the row both ends of every entry are at most
//                  min(parent[i], parent[j]) as they were read.  The L minima meet (ts_lanes_min); the owner lowers
//                  parent[i] to the row's minimum, HOOKS the grandparent -- with old = parent[i] as the row found it, the word
//                  of parent[old] is lowered to the minimum too, which moves a whole tree under a smaller root in one step
//                  -- and JUMPS twice: parent[i] is lowered to parent[parent[i]].  An atomic is issued only where the value read is greater than what it would store:
//                  near convergence a pass issues almost none.  The words a pass lowered are counted as k_lev_pass counts
//                  (smv_count) and the vertices with parent[i] == i go to one word by an add a workgroup; the host reads
//                  both once a batch of passes.  A pass that lowered nothing wrote nothing, so it read one stable array: a
//                  fixed point of "both ends of every entry are equal", constant on components, and by I1 and I2 at the
//                  component's smallest vertex that constant is the smallest vertex -- however the reads of a pass race
//                  with other lanes' writes.  Parents are read past the L1 (agent-scope relaxed loads): a pass sees what
//                  other workgroups lowered during it, which saves passes, never correctness.
//   k_cc_flag      a wave per 64 vertices: the roots (parent[i] == i) among them as a bitmap word and its count; the
//                  library's one-pass scan over the counts gives every word its first number (host: side_scan), as the
//                  aggregation numbers its roots.
//   k_cc_clear     size[c] = 0 for c < ncomp, the scan's total read on the device.
//   k_cc_number    comp[i] = the rank of root[i] among the roots; the vertices of a wave that share a component (co_same) add
//                  their number to size[comp] once.  Integer sums do not depend on order.
//
// Nothing spins, nothing waits for another workgroup; every lane of a wave reaches the reductions.  Validation as in the
// colouring, ahead of each dependent read: a row's bounds wherever they are read (a row that fails is taken as empty), a
// column before it indexes anything (skipped where it fails); either raises ctl[RD_ERR].
#pragma once
#include "bhs_trsv.hip.h"

namespace bhs {

// control words: the aggregation's (the error word, the count of words a pass lowered, the scan's); the roots a pass saw
// sit in the unused half behind the count, so that one 16-byte fill clears both
enum { CC_ROOTS = AG_UNDEC + 2, CC_INTS = AG_INTS };
static_assert(CC_ROOTS + 1 < AG_TICKET, "control block");

// The two choices of the pass, decided by measurement (profiles/components_case.md; -DBHS_CC_HOOK_GRAND=0 and
// -DBHS_CC_JUMPS=1 build the variants that were measured against): hooking lowers the word of i's GRANDPARENT, not of its
// old parent, and parent[i] is jumped TWICE a pass.
#ifndef BHS_CC_HOOK_GRAND
#define BHS_CC_HOOK_GRAND 1
#endif
#ifndef BHS_CC_JUMPS
#define BHS_CC_JUMPS 2
#endif
constexpr bool kCcHookGrand = BHS_CC_HOOK_GRAND != 0;
constexpr int kCcJumps = BHS_CC_JUMPS;

__device__ __forceinline__ int cc_load(const int* p)
{
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// *p = min(*p, v): did the word fall
__device__ __forceinline__ rd_u64 cc_lower(int* p, int v)
{
    return atomicMin(p, v) > v ? 1ull : 0ull;
}

__global__ __launch_bounds__(256) void k_cc_init(int n, int* __restrict__ parent)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i < n) parent[i] = (int)i;
}

template <int L>
__global__ __launch_bounds__(256) void k_cc_pass(AgDims d, const int* __restrict__ Sp, const int* __restrict__ Sj, int* parent,
                                                 int* __restrict__ ctl)
{
    __shared__ rd_u64 sChg;
    __shared__ int sRoots;
    const int lane = threadIdx.x & 63, sub = threadIdx.x & (L - 1);
    if (threadIdx.x == 0) { sChg = 0; sRoots = 0; }
    __syncthreads();
    bool bad = false;
    rd_u64 chg = 0;
    unsigned roots = 0;                                               // the vertices with parent[i] == i among this lane's rows
    const long long nBlocks = ((long long)d.n + 256 / L - 1) / (256 / L);
    for (long long t = blockIdx.x; t < nBlocks; t += gridDim.x) {     // (uniform in the workgroup)
        int a, b;
        const long long i = ag_row<L>(d, Sp, t, a, b, bad);
        const int old = i < d.n ? cc_load(parent + i) : 0x7fffffff;
        int m = old;
        for (int q = a + sub; q < b; q += L) {
            const int j = Sj[q];
            if ((unsigned)j >= (unsigned)d.n) { bad = true; continue; }   // (never an index)
            if (j == i) continue;
            const int pj = cc_load(parent + j);
            if (pj > m) chg += cc_lower(parent + j, m);               // (m < pj <= j: I1 holds)
            else m = pj;
        }
        m = (int)ts_lanes_min<L>((unsigned)m, lane);
        if (i < d.n && sub == 0) {
            if (m < old) {
                chg += cc_lower(parent + i, m);
                if constexpr (kCcHookGrand) {                         // hooking: the tree above i goes under m
                    const int top = cc_load(parent + old);            // (old <= i < n)
                    if (m < top) chg += cc_lower(parent + top, m);    // (m < top: I1 holds)
                } else {
                    if (old != i) chg += cc_lower(parent + old, m);
                }
            }
            int p = m;
            for (int s = 0; s < kCcJumps; ++s) {                      // pointer jumping
                const int g = cc_load(parent + p);                    // (p <= i < n)
                if (g >= p) break;
                chg += cc_lower(parent + i, g);
                p = g;
            }
            if (p == i) ++roots;
        }
    }
    roots += lane_xor<1>(roots, lane);
    roots += lane_xor<2>(roots, lane);
    roots += lane_xor<4>(roots, lane);
    roots += lane_xor<8>(roots, lane);
    roots += lane_xor<16>(roots, lane);
    roots += lane_xor<32>(roots, lane);
    if (lane == 0 && roots) (void)atomicAdd(&sRoots, (int)roots);
    rd_flag(bad, ctl);
    smv_count(chg, &sChg, ctl);                                       // (a barrier inside: sRoots is complete behind it)
    if (threadIdx.x == 0 && sRoots) (void)atomicAdd(ctl + CC_ROOTS, sRoots);
}

// map[g] = the roots among vertices 64 g .. 64 g + 63 as bits, cnt[g] their number (a wave per word)
__global__ __launch_bounds__(256) void k_cc_flag(int n, const int* __restrict__ root, rd_u64* __restrict__ map, int* __restrict__ cnt)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    const rd_u64 bits = __ballot(i < n && root[i] == (int)i);
    if ((threadIdx.x & 63) == 0 && (i >> 6) < (((long long)n + 63) >> 6)) {
        map[i >> 6] = bits;
        cnt[i >> 6] = __popcll(bits);
    }
}

// size[c] = 0 for c < ncomp: the scan's total, read here (never beyond n)
__global__ __launch_bounds__(256) void k_cc_clear(int n, const int* __restrict__ ctl, int* __restrict__ size)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    const long long ncomp = *(const long long*)(ctl + AG_TOTAL);
    if (i < n && i < ncomp) size[i] = 0;
}

// comp[i] = at[word of root[i]] + the roots below root[i] in its word; size[comp[i]] += 1, once for the vertices of a wave
// that share a component (size may be null)
__global__ __launch_bounds__(256) void k_cc_number(int n, const int* __restrict__ root, const rd_u64* __restrict__ map,
                                                   const int* __restrict__ at, int* __restrict__ comp, int* __restrict__ size,
                                                   int* __restrict__ ctl)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    const int lane = threadIdx.x & 63;
    bool has = i < n, bad = false;
    int c = 0;
    if (has) {
        const int r = root[i];
        if ((unsigned)r >= (unsigned)n) { bad = true; has = false; }  // (never an index; the roots were this call's own)
        else {
            c = at[r >> 6] + __popcll(map[r >> 6] & ((1ull << (r & 63)) - 1ull));
            if ((unsigned)c >= (unsigned)n) { bad = true; has = false; }
            else comp[i] = c;
        }
    }
    if (size) {                                                       // (uniform: every lane reaches the ballots)
        const rd_u64 m = co_same(c, has);
        if (has && lane == __ffsll((long long)m) - 1) (void)atomicAdd(size + c, __popcll(m));
    }
    rd_flag(bad, ctl);
}

}  // namespace bhs
