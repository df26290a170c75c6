// bhs_trsv.hip.h -- the level sets of a triangle of an n x n pattern and the sparse triangular solve on them, the triangle
// read in place (bhs_csr_levels_device, bhs_csr_trsv_device; the contract is worded in include/bhsparse_hip.h, "triangular
// solve and ILU(0)").
//
//   k_lev_pass<L>   one pass of the monotone relaxation level[i] = max(level[i], 1 + max level[j]) over the counted entries
//                   of row i (j < i for LOWER, j > i for UPPER; the diagonal and the other triangle are not counted), in
//                   place: levels start at 0, only rise and never pass the true level, so the fixed point is the definition
//                   however the reads of a pass race with its writes -- `level` is a plain pointer.  A bounded grid walks the
//                   blocks of rows ascending for LOWER and descending for UPPER, so that one pass carries a level across many
//                   rows.  The rows a pass raised are counted as k_col_round counts (smv_count), the levels in use go to
//                   one word by a maximum a workgroup; the host reads both once a batch of passes.  Values are never taken:
//                   the same code and the same result in the double and the float library.
//   k_trsv_level<L> the rows order[lo .. lo + cnt) of ONE level, a launch: s = the sum over the triangle's off-diagonal
//                   entries of double(a_ij) * double(x_j), every lane summing its entries q = a + sub, a + sub + L, ... in
//                   double from +0 and the L sums meeting in gs_lanes_sum -- the Gauss-Seidel sweep's order.  The diagonal
//                   is the row's first entry with j == i, its place the minimum over the row's lanes.
//                   t = (alpha * b_i - s) / a_ii, without the division for a unit diagonal; one rounding to the value type.
//                   The rows of a level read only x of earlier levels: the kernel boundary is the only synchronisation.
//                   b and x are plain pointers: they may be the same array.
//
// Every lane of a wave reaches the reductions: a place beyond the rows, or a row that is refused, has an empty range.
// Results are written by the lane that owns the row.  Validation ahead of each dependent read: an entry of order before it
// is a row, the row's bounds before its entries, a column before it indexes anything; each raises ctl[RD_ERR].
#pragma once
#include "bhs_color.hip.h"
#include "bhs_gs.hip.h"

namespace bhs {

// control words: the colouring's (the error word, the count of rows a pass raised, the scan's, the levels in use at
// CO_NCOL), then the factorisation's smallest bad pivot row
enum { TS_PIVOT = CO_INTS, TS_INTS = CO_INTS + 4 };

template <int L>
__device__ __forceinline__ unsigned ts_lanes_max(unsigned v, int lane)
{
    if constexpr (L > 1) v = max(v, lane_xor<1>(v, lane));
    if constexpr (L > 2) v = max(v, lane_xor<2>(v, lane));
    if constexpr (L > 4) v = max(v, lane_xor<4>(v, lane));
    if constexpr (L > 8) v = max(v, lane_xor<8>(v, lane));
    if constexpr (L > 16) v = max(v, lane_xor<16>(v, lane));
    if constexpr (L > 32) v = max(v, lane_xor<32>(v, lane));
    return v;
}

template <int L>
__device__ __forceinline__ unsigned ts_lanes_min(unsigned v, int lane)
{
    if constexpr (L > 1) v = min(v, lane_xor<1>(v, lane));
    if constexpr (L > 2) v = min(v, lane_xor<2>(v, lane));
    if constexpr (L > 4) v = min(v, lane_xor<4>(v, lane));
    if constexpr (L > 8) v = min(v, lane_xor<8>(v, lane));
    if constexpr (L > 16) v = min(v, lane_xor<16>(v, lane));
    if constexpr (L > 32) v = min(v, lane_xor<32>(v, lane));
    return v;
}

template <int L>
__global__ __launch_bounds__(256) void k_lev_pass(AgDims d, int upper, const int* __restrict__ Ap, const int* __restrict__ Aj,
                                                  int* level, int* __restrict__ ctl)
{
    __shared__ rd_u64 sChg;
    __shared__ int sTop;
    const int lane = threadIdx.x & 63, sub = threadIdx.x & (L - 1);
    if (threadIdx.x == 0) { sChg = 0; sTop = 0; }
    __syncthreads();
    bool bad = false;
    rd_u64 chg = 0;
    unsigned top = 0;                                                 // the levels in use as far as this lane's rows show
    const long long nBlocks = ((long long)d.n + 256 / L - 1) / (256 / L);
    for (long long t = blockIdx.x; t < nBlocks; t += gridDim.x) {     // (uniform in the workgroup)
        int a, b;
        const long long i = ag_row<L>(d, Ap, upper ? nBlocks - 1 - t : t, a, b, bad);
        unsigned m = 0;
        for (int q = a + sub; q < b; q += L) {
            const int j = Aj[q];
            if ((unsigned)j >= (unsigned)d.n) { bad = true; continue; }   // (never an index)
            if (upper ? j > i : j < i) m = max(m, (unsigned)level[j] + 1u);
        }
        m = ts_lanes_max<L>(m, lane);
        if (i < d.n && sub == 0) {
            const unsigned was = (unsigned)level[i];
            if (m > was) { level[i] = (int)m; ++chg; }
            top = max(top, max(m, was) + 1u);
        }
    }
    top = ts_lanes_max<64>(top, lane);
    if (lane == 0 && top) (void)atomicMax(&sTop, (int)top);
    rd_flag(bad, ctl);
    smv_count(chg, &sChg, ctl);                                       // (a barrier inside: sTop is complete behind it)
    if (threadIdx.x == 0 && sTop) (void)atomicMax(ctl + CO_NCOL, sTop);
}

struct TsDims {
    int n, nnzA;
    int lo, cnt;            // the level's rows: order[lo .. lo + cnt)
    int upper, unit;
    double alpha;
};

// the k-th row of the level for this thread's group of L lanes: -1 where there is none or it is refused, [a, e) its range
__device__ __forceinline__ int ts_listed(int n, int nnzA, int lo, int cnt, long long k, const int* __restrict__ Ap,
                                         const int* __restrict__ order, int& a, int& e, bool& bad)
{
    a = e = 0;
    if (k >= cnt) return -1;
    const int r = order[lo + k];
    if ((unsigned)r >= (unsigned)n) { bad = true; return -1; }        // (never an index)
    const int p = Ap[r], q = Ap[r + 1];
    if (rd_bounds_bad(p, q, nnzA)) { bad = true; return -1; }
    a = p; e = q;
    return r;
}

// one row of a level: the k-th of order[lo .. lo + cnt), for this thread's group of L lanes (every lane of the wave comes here)
template <int L>
__device__ __forceinline__ void ts_row(const TsDims& d, int lo, int cnt, long long k, const int* __restrict__ Ap,
                                       const int* __restrict__ Aj, const value_t* __restrict__ Ax, const int* __restrict__ order,
                                       const value_t* b, value_t* x, bool& bad)
{
    const int lane = threadIdx.x & 63, sub = threadIdx.x & (L - 1);
    int a, e;
    const int i = ts_listed(d.n, d.nnzA, lo, cnt, k, Ap, order, a, e, bad);
    double s = 0.0;
    unsigned dq = 0xFFFFFFFFu;                                        // the place of the row's first diagonal entry
    for (int q = a + sub; q < e; q += L) {
        const int j = Aj[q];
        if ((unsigned)j >= (unsigned)d.n) { bad = true; continue; }   // (never an index)
        if (j == i) { dq = min(dq, (unsigned)q); continue; }
        if (d.upper ? j > i : j < i) s += (double)Ax[q] * (double)x[j];
    }
    s = gs_lanes_sum<L>(s, lane);
    if (!d.unit) dq = ts_lanes_min<L>(dq, lane);
    if (i >= 0 && sub == 0) {
        const double t = d.alpha * (double)b[i] - s;
        if (d.unit) x[i] = (value_t)t;
        else if (dq == 0xFFFFFFFFu) bad = true;                       // a listed row without a diagonal entry
        else x[i] = (value_t)(t / (double)Ax[dq]);
    }
}

template <int L>
__global__ __launch_bounds__(256) void k_trsv_level(TsDims d, const int* __restrict__ Ap, const int* __restrict__ Aj,
                                                    const value_t* __restrict__ Ax, const int* __restrict__ order,
                                                    const value_t* b, value_t* x, int* __restrict__ ctl)
{
    bool bad = false;
    ts_row<L>(d, d.lo, d.cnt, (long long)blockIdx.x * (256 / L) + threadIdx.x / L, Ap, Aj, Ax, order, b, x, bad);
    rd_flag(bad, ctl);
}

}  // namespace bhs
