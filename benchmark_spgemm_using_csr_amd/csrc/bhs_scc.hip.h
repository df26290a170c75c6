// bhs_scc.hip.h -- the strongly connected components of an n x n pattern S: i and j belong together where a directed path
// leads from i to j and one from j to i (bhs_csr_scc_device; the contract is worded in include/bhsparse_hip.h, "strongly
// connected components").  Values are never taken: the same code, and the same result bit for bit, in the double and the
// float library.  An entry (i, j), j != i, is an edge between i and j; the components of a graph and of its reverse are the
// same, so the kernels read it as i -> j and need no transpose.
//
// Per vertex: part[v], the colour class the previous round left v in, -1 once v is decided (all 0 at the start); lab[v], in
// the caller's d_root itself, final where v is decided; a stamp word and a reach flag.  An edge i -> j is VALID where j != i,
// both ends are live and part[i] == part[j].  A round:
//
//   trim       a live vertex without a valid out-edge or without a valid in-edge is a component by itself.  A pass is two
//              launches: k_scc_mark<L> stores the pass's stamp to stamp[j] over the valid edges -- plain stores of one value,
//              nothing cleared, no atomic -- and reads a liveness that no lane changes meanwhile; k_scc_trim<L> looks for a
//              valid out-edge in the row and for the stamp, and kills in place: part[v] = -1, root[v] = v.  Liveness only
//              falls, so a vertex killed on a racing read would have been killed a pass later: the fixed point is unique.
//              A pass counts its kills, and the vertices it left live in a word of its own.
//   forward    k_scc_start sets lab[v] = v on the live vertices.  k_scc_forward<L>, in place over the live rows: lab[j] is
//              lowered to lab[i] over the valid edges, by an atomic minimum issued only where the value read is greater; after
//              the start no other write touches lab (a word only ever falls).  The shortcut lab[i] <- lab[lab[i]] is taken
//              kSccJumps times a row: lab[i] = u says that u reaches i inside the class, and lab[u] reaches u.  A pass that
//              lowered nothing read one stable array: lab[v] is the smallest live vertex of v's class that reaches v.
//   backward   k_scc_seed: reach[v] = (lab[v] == v).  k_scc_backward<L>, a pull over the rows: a live i that is not yet
//              reached becomes reached where some edge i -> j has lab[j] == lab[i] and j reached (equal labels are of one
//              class, and a decided vertex carries the index of a decided one, never a live label).  Flags only rise.
//   decide     k_scc_decide: a reached v is final with root[v] = lab[v] -- every member reaches the root and the root every
//              member, and no smaller vertex reaches it --, every other live v goes to part[v] = lab[v]; the vertices left
//              are counted.
//
// The loads that race with other workgroups' writes go past the L1 (cc_load).  The components a kernel decides are added to
// ctl[SCC_COUNT], a word no loop clears.  Nothing spins, nothing waits for another workgroup; every lane of a wave reaches
// the reductions.  Validation as in the components, ahead of each dependent read: a row's bounds wherever they are read (a
// row that fails is taken as empty), a column before it indexes anything (skipped where it fails); either raises ctl[RD_ERR].
// The numbering is the components' (k_cc_flag, k_cc_clear, k_cc_number).
#pragma once
#include "bhs_components.hip.h"

namespace bhs {

// control words: the components'; the vertices a trim pass left live where the components count their roots, and behind it
// the components decided so far, which the pass loop does not clear (it clears three words from AG_UNDEC on)
enum { SCC_LIVE = CC_ROOTS, SCC_COUNT = CC_ROOTS + 1, SCC_INTS = CC_INTS };
static_assert(SCC_COUNT < AG_TICKET, "control block");

// The shortcuts of a forward row, decided by measurement (profiles/scc_case.md; -DBHS_SCC_JUMPS=0 and =2 build the variants
// that were measured against).
#ifndef BHS_SCC_JUMPS
#define BHS_SCC_JUMPS 1
#endif
constexpr int kSccJumps = BHS_SCC_JUMPS;

__device__ __forceinline__ void scc_store(int* p, int v)
{
    __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// the sum of v over the wave; every lane comes here
__device__ __forceinline__ unsigned scc_wave_sum(unsigned v, int lane)
{
    v += lane_xor<1>(v, lane);
    v += lane_xor<2>(v, lane);
    v += lane_xor<4>(v, lane);
    v += lane_xor<8>(v, lane);
    v += lane_xor<16>(v, lane);
    v += lane_xor<32>(v, lane);
    return v;
}

template <int L>
__global__ __launch_bounds__(256) void k_scc_mark(AgDims d, const int* __restrict__ Sp, const int* __restrict__ Sj,
                                                  const int* __restrict__ part, int* __restrict__ stamp, int s, int* __restrict__ ctl)
{
    const int sub = threadIdx.x & (L - 1);
    bool bad = false;
    const long long nBlocks = ((long long)d.n + 256 / L - 1) / (256 / L);
    for (long long t = blockIdx.x; t < nBlocks; t += gridDim.x) {
        int a, b;
        const long long i = ag_row<L>(d, Sp, t, a, b, bad);
        const int pi = i < d.n ? part[i] : -1;
        if (pi < 0) a = b = 0;                                        // decided: nothing of the row is read
        for (int q = a + sub; q < b; q += L) {
            const int j = Sj[q];
            if ((unsigned)j >= (unsigned)d.n) { bad = true; continue; }   // (never an index)
            if (j != i && part[j] == pi) stamp[j] = s;
        }
    }
    rd_flag(bad, ctl);
}

template <int L>
__global__ __launch_bounds__(256) void k_scc_trim(AgDims d, const int* __restrict__ Sp, const int* __restrict__ Sj, int* part,
                                                  const int* __restrict__ stamp, int* __restrict__ root, int s, int* __restrict__ ctl)
{
    __shared__ rd_u64 sChg;
    __shared__ int sLive;
    const int lane = threadIdx.x & 63, sub = threadIdx.x & (L - 1);
    if (threadIdx.x == 0) { sChg = 0; sLive = 0; }
    __syncthreads();
    bool bad = false;
    rd_u64 killed = 0;
    unsigned live = 0;
    const long long nBlocks = ((long long)d.n + 256 / L - 1) / (256 / L);
    for (long long t = blockIdx.x; t < nBlocks; t += gridDim.x) {     // (uniform in the workgroup)
        int a, b;
        const long long i = ag_row<L>(d, Sp, t, a, b, bad);
        const int pi = i < d.n ? cc_load(part + i) : -1;
        if (pi < 0) a = b = 0;
        unsigned none = 1;                                            // no valid out-edge seen
        for (int q = a + sub; q < b; q += L) {
            const int j = Sj[q];
            if ((unsigned)j >= (unsigned)d.n) { bad = true; continue; }   // (never an index)
            if (j != i && cc_load(part + j) == pi) { none = 0; break; }
        }
        none = ts_lanes_min<L>(none, lane);
        if (pi >= 0 && sub == 0) {
            if (none || stamp[i] != s) {
                scc_store(part + i, -1);
                root[i] = (int)i;
                ++killed;
            } else {
                ++live;
            }
        }
    }
    live = scc_wave_sum(live, lane);
    if (lane == 0 && live) (void)atomicAdd(&sLive, (int)live);
    rd_flag(bad, ctl);
    smv_count(killed, &sChg, ctl);                                    // (a barrier inside: sLive is complete behind it)
    if (threadIdx.x == 0) {
        if (sLive) (void)atomicAdd(ctl + SCC_LIVE, sLive);
        if (sChg) (void)atomicAdd(ctl + SCC_COUNT, (int)sChg);
    }
}

__global__ __launch_bounds__(256) void k_scc_start(int n, const int* __restrict__ part, int* __restrict__ lab)
{
    const long long nBlocks = ((long long)n + 255) / 256;
    for (long long t = blockIdx.x; t < nBlocks; t += gridDim.x) {
        const long long i = t * 256 + threadIdx.x;
        if (i < n && part[i] >= 0) lab[i] = (int)i;
    }
}

template <int L>
__global__ __launch_bounds__(256) void k_scc_forward(AgDims d, const int* __restrict__ Sp, const int* __restrict__ Sj,
                                                     const int* __restrict__ part, int* lab, int* __restrict__ ctl)
{
    __shared__ rd_u64 sChg;
    const int sub = threadIdx.x & (L - 1);
    if (threadIdx.x == 0) sChg = 0;
    __syncthreads();
    bool bad = false;
    rd_u64 chg = 0;
    const long long nBlocks = ((long long)d.n + 256 / L - 1) / (256 / L);
    for (long long t = blockIdx.x; t < nBlocks; t += gridDim.x) {     // (uniform in the workgroup)
        int a, b;
        const long long i = ag_row<L>(d, Sp, t, a, b, bad);
        const int pi = i < d.n ? part[i] : -1;
        if (pi < 0) a = b = 0;
        int m = pi >= 0 ? cc_load(lab + i) : 0;
        if (pi >= 0 && sub == 0) {
            for (int k = 0; k < kSccJumps; ++k) {                     // the shortcut: what reaches lab[i] reaches i
                if ((unsigned)m >= (unsigned)d.n) { bad = true; break; }   // (never an index; the labels are this call's own)
                const int g = cc_load(lab + m);
                if (g >= m) break;
                chg += cc_lower(lab + i, g);
                m = g;
            }
        }
        for (int q = a + sub; q < b; q += L) {
            const int j = Sj[q];
            if ((unsigned)j >= (unsigned)d.n) { bad = true; continue; }   // (never an index)
            if (j == i || part[j] != pi) continue;
            if (cc_load(lab + j) > m) chg += cc_lower(lab + j, m);
        }
    }
    rd_flag(bad, ctl);
    smv_count(chg, &sChg, ctl);
}

__global__ __launch_bounds__(256) void k_scc_seed(int n, const int* __restrict__ part, const int* __restrict__ lab, int* __restrict__ reach)
{
    const long long nBlocks = ((long long)n + 255) / 256;
    for (long long t = blockIdx.x; t < nBlocks; t += gridDim.x) {
        const long long i = t * 256 + threadIdx.x;
        if (i < n) reach[i] = part[i] >= 0 && lab[i] == (int)i ? 1 : 0;
    }
}

template <int L>
__global__ __launch_bounds__(256) void k_scc_backward(AgDims d, const int* __restrict__ Sp, const int* __restrict__ Sj,
                                                      const int* __restrict__ part, const int* __restrict__ lab, int* reach,
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
        const bool open = i < d.n && part[i] >= 0 && cc_load(reach + i) == 0;
        if (!open) a = b = 0;
        const int li = open ? lab[i] : 0;
        unsigned none = 1;
        for (int q = a + sub; q < b; q += L) {
            const int j = Sj[q];
            if ((unsigned)j >= (unsigned)d.n) { bad = true; continue; }   // (never an index)
            if (j != i && lab[j] == li && cc_load(reach + j) != 0) { none = 0; break; }
        }
        none = ts_lanes_min<L>(none, lane);
        if (open && sub == 0 && !none) {
            scc_store(reach + i, 1);
            ++chg;
        }
    }
    rd_flag(bad, ctl);
    smv_count(chg, &sChg, ctl);
}

__global__ __launch_bounds__(256) void k_scc_decide(int n, int* __restrict__ part, const int* __restrict__ lab, const int* __restrict__ reach,
                                                    int* __restrict__ ctl)
{
    __shared__ rd_u64 sLeft;
    __shared__ int sDone;
    const int lane = threadIdx.x & 63;
    if (threadIdx.x == 0) { sLeft = 0; sDone = 0; }
    __syncthreads();
    rd_u64 left = 0;
    unsigned done = 0;                                                // the roots among the decided: one a component
    const long long nBlocks = ((long long)n + 255) / 256;
    for (long long t = blockIdx.x; t < nBlocks; t += gridDim.x) {     // (uniform in the workgroup)
        const long long i = t * 256 + threadIdx.x;
        if (i < n && part[i] >= 0) {
            const int l = lab[i];
            if (reach[i]) {
                part[i] = -1;
                if (l == (int)i) ++done;
            } else {
                part[i] = l;
                ++left;
            }
        }
    }
    done = scc_wave_sum(done, lane);
    if (lane == 0 && done) (void)atomicAdd(&sDone, (int)done);
    smv_count(left, &sLeft, ctl);                                     // (a barrier inside: sDone is complete behind it)
    if (threadIdx.x == 0 && sDone) (void)atomicAdd(ctl + SCC_COUNT, sDone);
}

}  // namespace bhs
