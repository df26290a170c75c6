// bhs_cfsplit.hip.h -- C/F splitting of the vertices of an n x n pattern S of strong connections: the coarse points of a
// classical (Ruge-Stueben) multigrid setup (bhs_csr_cfsplit_device; the contract is worded in include/bhsparse_hip.h,
// "C/F splitting and interpolation").  Values are never taken: the same code, and the same result bit for bit, in the double
// and the float library.
//
// One 64-bit word a vertex, the aggregation's (bhs_aggregate.hip.h): state << 62 | key, key = prio31 << 31 | index; state 1
// undecided, 2 in (a C point), 0 out (an F point).  The C points are the greedy distance-ONE independent set in descending
// key order -- PMIS where the priority carries the row's length (BHS_CF_DEGREE) --, found in synchronous rounds of one gather:
//
//   k_cf_init     a thread per vertex: its key (the caller's priority, the hash, or the row length over the hash), its word
//                 as undecided, its row's two bounds checked.
//   k_cf_round    for an undecided i: m = the greatest word over i and N(i).  m's state is in: a C point is a neighbour, i is
//                 out.  m is i's own word: i is in.  Else i stays.  A decided vertex copies its word and reads nothing of its
//                 row.  A round reads one array of words and writes the other, never the one it reads.  The vertices that stay
//                 are counted as k_agg_decide counts them (smv_count: one add a workgroup, the grid bounded, a workgroup
//                 walks several blocks of rows); the host reads the count once a round.  No kernel spins or waits for another
//                 workgroup.
//   k_agg_count   (the aggregation's) a wave per 64 vertices: the C points among them as a bitmap word and its count; the
//                 library's one-pass scan over the counts gives every word its first number (host: side_scan).
//   k_cf_number   a thread per vertex: a C point's number is its word's first number plus the C points below it in the word,
//                 cf[i] = number and cpts[number] = i; an F point gets cf[i] = -1.  Every element of cf is written once, by
//                 the thread that owns it: no atomics on results.
//
// The gather spreads a row over L = 1, 4, 16 or 64 lanes (host: ag_lanes) exactly as the aggregation's do (ag_row,
// ag_lanes_max); validation likewise, ahead of each dependent read: a row's bounds wherever they are read (a row that fails
// is taken as empty), a column before it indexes anything (skipped where it fails); either raises ctl[RD_ERR].
#pragma once
#include "bhs_aggregate.hip.h"

namespace bhs {

__global__ __launch_bounds__(256) void k_cf_init(AgDims d, int degree, const int* __restrict__ Sp, const unsigned* __restrict__ prio,
                                                 rd_u64* __restrict__ w, int* __restrict__ ctl)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    bool bad = false;
    if (i < d.n) {
        const int lo = Sp[i], hi = Sp[i + 1];
        bad = rd_bounds_bad(lo, hi, d.nnzS);
        unsigned p31;
        if (degree) {
            const unsigned len = bad ? 0u : (unsigned)(hi - lo);
            p31 = (min(len, 1023u) << 21) | (ag_hash((unsigned)i, d.seed) >> 11);
        } else {
            p31 = (d.hasPrio ? prio[i] : ag_hash((unsigned)i, d.seed)) >> 1;
        }
        w[i] = kAgUndecided | ((rd_u64)p31 << 31) | (rd_u64)i;
    }
    rd_flag(bad, ctl);
}

template <int L>
__global__ __launch_bounds__(256) void k_cf_round(AgDims d, const int* __restrict__ Sp, const int* __restrict__ Sj,
                                                  const rd_u64* __restrict__ win, rd_u64* __restrict__ wout, int* __restrict__ ctl)
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
        const rd_u64 mine = i < d.n ? win[i] : 0;
        const bool open = (mine >> 62) == 1;
        if (!open) a = b = 0;                                        // decided: nothing of the row is read
        rd_u64 v = 0;
        for (int q = a + sub; q < b; q += L) {
            const int j = Sj[q];
            if ((unsigned)j >= (unsigned)d.n) { bad = true; continue; }   // (never an index)
            v = max(v, win[j]);
        }
        v = ag_lanes_max<L>(v, lane);
        if (i < d.n && sub == 0) {
            rd_u64 out = mine;
            if (open) {
                v = max(v, mine);
                if ((v >> 62) == 2) out = mine & kAgKeyMask;
                else if (v == mine) out = kAgIn | (mine & kAgKeyMask);
                else ++left;
            }
            wout[i] = out;
        }
    }
    rd_flag(bad, ctl);
    smv_count(left, &sLeft, ctl);
}

// cf[i] = at[i / 64] + the C points of its bitmap word below i, cpts[that] = i (cpts may be null); -1 for an F point
__global__ __launch_bounds__(256) void k_cf_number(int n, const rd_u64* __restrict__ map, const int* __restrict__ at,
                                                   int* __restrict__ cf, int* __restrict__ cpts, int* __restrict__ ctl)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    bool bad = false;
    if (i < n) {
        const rd_u64 bits = map[i >> 6];
        const int bit = (int)(i & 63);
        int c = -1;
        if ((bits >> bit) & 1ull) {
            c = at[i >> 6] + __popcll(bits & ((1ull << bit) - 1ull));
            if ((unsigned)c >= (unsigned)n) { bad = true; c = -1; }  // (never an index)
            else if (cpts) cpts[c] = (int)i;
        }
        cf[i] = c;
    }
    rd_flag(bad, ctl);
}

}  // namespace bhs
